#!/usr/bin/env python3
"""Builds tools/site_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the case table of
tests/test_artefacts_host.py through it: the host code of the artefact table (scs_site.h) as a stand-alone CPU program, every body
compared with the restatement's (tests/site_cases.py) at min_reads 0, 1 and 1000, every array in a heap block of exactly its size.
No GPU.

    python tools/site_host_check.py [--cxx g++]
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
    import test_artefacts_host as t
    from site_cases import probe_inputs, sites_from_table
    rows = ["genome " + t.GENOME, "records %d " % len(t.NAMES) + " ".join("%s %d" % nl for nl in zip(t.NAMES, t.REC_LENS))]

    def case(starts, lens, reads, edits, min_reads, rc, want=""):
        f = [min_reads, rc, len(starts)] + [v for amp in zip(starts, lens, reads) for v in amp] + [len(edits)] + [v for e in edits for v in e] + [want.count("\n")]
        rows.append("case " + " ".join(str(v) for v in f))
        if want:
            rows.append(want.rstrip("\n"))

    for name in sorted(t.CASES):
        for min_reads in (0, 1, 1000):
            want, _ = sites_from_table(t.CASES[name], t.NAMES, t.REC_LENS, t.G, min_reads)
            case(*probe_inputs(t.CASES[name], t.NAMES, t.REC_LENS), min_reads, 0, want)
    case([40], [30], [1], [(0, 45, 1)], 0, 1)                  # an amplicon over its record's end; beyond the genome; an edit outside
    case([190], [20], [1], [], 0, 1)                           # its amplicon; of no amplicon; a base that is no code: refused, nothing read
    case([5], [35], [3], [(0, 40, 1)], 0, 1)
    case([5], [35], [3], [(1, 17, 1)], 0, 1)
    case([5], [35], [3], [(0, 17, 4)], 0, 1)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "site_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "site_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
