#!/usr/bin/env python3
"""Rewrite tests/golden/gemm_f64_routes.txt: the f64 GEMM router's table (tests/gemm_f64_routes.py), recorded from the
sources in this tree.  Needs hipcc, no GPU.  The file is the recorded behaviour a change of gemm_f64.hip's host code is
compared against: regenerate it only for a change that is MEANT to move a call to another kernel, instance or grid (or
for new cases in tests/gemm_f64_cases.py), and review the diff line by line.

    python tests/golden/gen_gemm_f64_routes.py
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gemm_f64_routes  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        text = gemm_f64_routes.table(gemm_f64_routes.build(tmp))
    with open(gemm_f64_routes.GOLDEN, "w") as f:
        f.write(text)
    print(f"{gemm_f64_routes.GOLDEN}: {text.count(chr(10))} lines, {len(text)} bytes")
