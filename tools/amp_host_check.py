#!/usr/bin/env python3
"""Builds tools/amp_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the case table of
tests/test_amplicons_host.py through it: the host code of the amplicon table (scs_amp.h) as a stand-alone CPU program, every line
compared with the restatement's (tests/amp_cases.py), every genome window in a heap block of exactly its size.  No GPU.

    python tools/amp_host_check.py [--cxx g++]
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
    import test_amplicons_host as t
    from amp_cases import amplicon_line
    rows = ["genome " + t.GENOME]

    def case(frag, semi, full, rec, gs, gl, rc, want=None):
        e1, e2 = [(p << 3) | b for p, b in semi[2]], [(p << 3) | b for p, b in full[2]]
        f = [frag[0], frag[1], frag[2], semi[0], semi[1], len(e1)] + e1 + [full[0], full[1], len(e2)] + e2 + [gs, gl, t.REC_OFF[rec], t.REC_LENS[rec], t.NAMES[rec], 123456, 6, 4321, rc]
        rows.append("case " + " ".join(str(v) for v in f))
        if want is not None:
            rows.append(want.rstrip("\n"))

    for name, rec, frag, semi, full in t.CASES:
        want = amplicon_line(t.G, frag, semi, full, t.REC_OFF[rec], t.NAMES[rec], 123456, 6, 4321)
        case(frag, semi, full, rec, 0, len(t.GENOME), 0, want)
        lo = t.REC_OFF[rec] + int(want.split("\t")[1])
        case(frag, semi, full, rec, lo, full[1], 0, want)          # the window that just covers the amplicon
        case(frag, semi, full, rec, lo + 1, full[1] - 1, 1)        # one base short at the left, at the right: refused, nothing read
        case(frag, semi, full, rec, lo, full[1] - 1, 1)
    case((1100, 600, -1), (250, 400, []), (30, 300, []), 1, 0, len(t.GENOME), 1)
    case((1100, 600, -1), (50, 400, []), (101, 300, []), 1, 0, len(t.GENOME), 1)
    case((2500, 600, -1), (50, 400, []), (30, 300, []), 1, 0, len(t.GENOME), 1)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "amp_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "amp_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
