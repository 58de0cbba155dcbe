#!/usr/bin/env python3
"""Builds tools/lift_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the grid and the case table
of tests/test_lift_host.py through it: the host code of the lift table (scs_lift.h: lift_read, the file's parser and writer) as a
stand-alone CPU program, every report compared with the restatement's (POS, CIGAR, the table), every array in a heap block of
exactly its size.  No GPU.

    python tools/lift_host_check.py [--cxx g++]
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
    import test_lift_host as t
    rows = t.host_check_rows()
    with tempfile.TemporaryDirectory() as td:
        for name, lines, line in [("valid", t.VALID, 0)] + t.BROKEN:
            p = os.path.join(td, name + ".lift")
            open(p, "w").write("".join(ln + "\n" for ln in lines))
            rows.append("file %s %d" % (p, line))
        exe = os.path.join(td, "lift_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "lift_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
