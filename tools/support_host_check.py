#!/usr/bin/env python3
"""Builds tools/support_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the grid of
tests/test_support_host.py through it: the host code of the site support (scs_support.h) as a stand-alone CPU program, every
report compared with the restatement's (POS, CIGAR, SEQ), every array in a heap block of exactly its size.  No GPU.

    python tools/support_host_check.py [--cxx g++]
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
    import test_support_host as t
    rows = []
    for name, n, events, reverse, pos0, fq, positions in t.grid():
        pos, cigar, seq = t.sam_fields(pos0, n, events, reverse, fq)
        want = t.restatement(pos, cigar, seq, positions)
        f = [n, pos0, int(reverse), t.REC_LEN, fq, len(events)] + [v for e in events for v in e] + [len(positions)] + positions + [len(want)] + [v for w in want for v in w]
        rows.append("case " + " ".join(str(v) for v in f))
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "support_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "support_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
