#!/usr/bin/env python3
"""Builds tools/runs_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the host table of
tests/test_runs_host.py through it: the bedGraph line formatter of the per-base arrays' writer (scs_runs.h: runs_line with its
counting sink and its capped buffer) as a stand-alone CPU program, every line compared with printf's, every output in a heap block of
exactly its size.  No GPU.

    python tools/runs_host_check.py [--cxx g++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    import test_runs_host as t
    rows = t.host_check_rows()
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "runs_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "runs_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
