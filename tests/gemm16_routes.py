"""The 16-bit GEMM router's table without a GPU (shared by test_gemm16_route_table_cpu.py and golden/gen_gemm16_routes.py).

build() compiles ptdeco_amd/csrc/gemm_bf16.hip HOST-ONLY with tests/gemm16_route_probe/shim.h force-included (every
launch becomes a call of a recorder) and links it with the driver and no HIP library; table() runs that program once per
switch setting and names each launched kernel by the demangled symbol of its handle, which is the exact template
instance however the source spells the launch."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptdeco_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "gemm16_route_probe")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm16_routes.txt")

# the route switches at their non-default settings; each runs in a process of its own (some are read once per process)
SWITCHES = ("PTD_GEMM_8PH=0", "PTD_GEMM_8PH=1", "PTD_GEMM_8PH_PERSIST=0", "PTD_GEMM_6PH=0", "PTD_GEMM_NO_GLDS=1")


def hipcc():
    return shutil.which(os.environ.get("HIPCC", "hipcc"))


def tools_missing():
    """-> what build() / table() need and this machine lacks (the test skips on it), or None."""
    return next((t for t, path in (("hipcc", hipcc()), ("nm", _nm())) if path is None), None)


def _run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300, **kw)


def _llvm_bin():
    return _run([hipcc(), "--version"]).stdout.split("InstalledDir:", 1)[1].split()[0]


def _nm():
    return shutil.which("nm")


def build(workdir, source="gemm_bf16.hip", driver="driver.cpp", name="gemm16_route_probe"):
    """-> path of the probe program, built under workdir (str or Path): `source` of ptdeco_amd/csrc compiled host-only
    behind the shim, linked with `driver` of the probe directory."""
    workdir = str(workdir)
    cc = hipcc()
    host = [cc, "--cuda-host-only", "-O1", "-std=c++17", "-include", os.path.join(PROBE, "shim.h"), "-c"]
    gemm_o = os.path.join(workdir, os.path.splitext(source)[0] + ".o")
    driver_o = os.path.join(workdir, os.path.splitext(driver)[0] + ".o")
    _run(host + [os.path.join(CSRC, source), "-o", gemm_o])
    _run(host + [os.path.join(PROBE, driver), "-o", driver_o])
    # the device image the host object expects to find linked in: a zeroed array under the name it asks for
    undefined = _run([_nm(), "-u", gemm_o]).stdout
    fatbin = re.search(r"\b(__hip_fatbin_\w*)", undefined).group(1)
    fatbin_c = os.path.join(workdir, "fatbin.c")
    with open(fatbin_c, "w") as f:
        f.write(f"const char {fatbin}[4096] __attribute__((aligned(4096))) = {{0}};\n")
    exe = os.path.join(workdir, name)
    _run([os.path.join(_llvm_bin(), "clang++"), "-no-pie", "-o", exe, gemm_o, driver_o, "-x", "c", fatbin_c])
    return exe


def _instances(exe):
    """handle address -> 'gemm_bf16_nt_glds_kernel<Bf16, 1, 4, 1>' (the handles are local read-only symbols)."""
    names = {}
    for line in _run([_nm(), "-C", exe]).stdout.splitlines():
        m = re.match(r"^([0-9a-f]+) [rRdD] (?:void )?(.*_kernel.*)$", line)
        if m and "__device_stub__" not in m.group(2):
            name = m.group(2).replace("ptd::(anonymous namespace)::", "")
            depth, end = 0, len(name)          # cut the parameter list: the last top-level '('
            for i, ch in enumerate(name):
                depth += ch == "<"
                depth -= ch == ">"
                if ch == "(" and depth == 0:
                    end = i
                    break
            names[int(m.group(1), 16)] = name[:end].replace(", ", ",")
    return names


def _rows(exe, names, setting=None, args=(), stdin=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PTD_GEMM_")}
    if setting:
        key, value = setting.split("=")
        env[key] = value
    out = _run([exe, *args], env=env, input=stdin).stdout
    return [re.sub(r"@(0x[0-9a-f]+)", lambda m: names[int(m.group(1), 16)], line) for line in out.splitlines()]


def table(exe):
    """The whole table as text: every case at the default switches, then per switch setting the named cases it changes."""
    names = _instances(exe)
    lines = ["# default"] + _rows(exe, names)
    named = _rows(exe, names, args=("named",))
    for setting in SWITCHES:
        lines.append("# " + setting)
        changed = [row for row, base in zip(_rows(exe, names, setting, ("named",)), named) if row != base]
        lines.extend(changed)
    return "\n".join(lines) + "\n"
