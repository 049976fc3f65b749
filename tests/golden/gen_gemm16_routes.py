#!/usr/bin/env python3
"""Rewrite tests/golden/gemm16_routes.txt: the 16-bit GEMM router's table (tests/gemm16_routes.py), recorded from the
sources in this tree.  Needs hipcc, no GPU.  The file is the recorded behaviour a change of the router is compared
against: regenerate it only for a change that is MEANT to alter a route, and review the diff line by line.

    python tests/golden/gen_gemm16_routes.py
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gemm16_routes  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        text = gemm16_routes.table(gemm16_routes.build(tmp))
    with open(gemm16_routes.GOLDEN, "w") as f:
        f.write(text)
    print(f"{gemm16_routes.GOLDEN}: {text.count(chr(10))} lines, {len(text)} bytes")
