#!/usr/bin/env python3
"""Is the bf16 device code unchanged?  Compiles the 16-bit kernel sources of a base revision and of the working tree
to gfx950 assembly and compares every bf16 function instruction for instruction.

    python tools/bf16_isa_diff.py [--base REV] [--src gemm_bf16.hip reduce.hip eigh_factored.hip]

The kernels of gemm_bf16.hip gained an element-type template parameter (Bf16 | F16); functions are matched by
demangled name with the `Bf16` argument dropped.  Labels, comments and directives are stripped; branch targets are
compared by block number, symbol operands by name.  Functions of the working tree that instantiate F16 (or take
_Float16) are new and only counted.  Exit status 0 = every base function is present and identical.
"""

from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_asm(tree: str, src: str, out: str) -> str:
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(tree, "ptdeco_amd", "csrc", src)], check=True, capture_output=True)
    with open(out) as f:
        return f.read()


def functions(text: str) -> dict[str, list[str]]:
    funcs, name, body = {}, None, []
    for line in text.split("\n"):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            funcs[name] = body
            name = None
            continue
        s = line.split(";", 1)[0].strip()
        if not s or s.startswith(".") or re.match(r"^[\w.$]+:$", s):
            continue
        s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
        body.append(s)
    return funcs


def demangle(names: list[str]) -> dict[str, str]:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def normalise(funcs: dict[str, list[str]]) -> dict[str, list[str]]:
    dem = demangle(list(funcs))
    sym = {m: re.sub(r"ptd::\(anonymous namespace\)::Bf16, ", "", d) for m, d in dem.items()}
    out = {}
    for m, body in funcs.items():
        # symbol operands (kernels calling helpers, relocations) by their normalised names
        out[sym[m]] = [re.sub(r"_Z\w+", lambda t: sym.get(t.group(0), t.group(0)), s) for s in body]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD", help="git revision of the reference code (default HEAD)")
    ap.add_argument("--src", nargs="+", default=["gemm_bf16.hip", "reduce.hip", "eigh_factored.hip"])
    args = ap.parse_args()
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        arch = subprocess.run(["git", "-C", ROOT, "archive", args.base, "ptdeco_amd/csrc", "include"], check=True,
                              capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base], input=arch, check=True)
        for src in args.src:
            old = normalise(functions(device_asm(base, src, os.path.join(tmp, "old.s"))))
            new = normalise(functions(device_asm(ROOT, src, os.path.join(tmp, "new.s"))))
            missing = [n for n in old if n not in new]
            differ = [n for n in old if n in new and old[n] != new[n]]
            added = [n for n in new if n not in old]
            n_instr = sum(len(b) for b in old.values())
            print(f"{src}: {len(old)} base functions ({n_instr} instructions): {len(old) - len(missing) - len(differ)} "
                  f"identical, {len(differ)} differ, {len(missing)} missing; {len(added)} new "
                  f"({sum('F16' in n or '_Float16' in n for n in added)} f16 instantiations)")
            for n in missing:
                print("  missing:", n)
            for n in differ:
                a, b = old[n], new[n]
                i = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
                print(f"  differs: {n}\n    first at instruction {i}: {a[i] if i < len(a) else '<end>'!r} vs "
                      f"{b[i] if i < len(b) else '<end>'!r}")
            ok = ok and not missing and not differ
    print("bf16 device code unchanged" if ok else "bf16 device code CHANGED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
