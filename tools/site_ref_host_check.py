#!/usr/bin/env python3
"""Builds tools/site_ref_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the case table of
tests/test_artefacts_ref_host.py through it: the host code of the artefact table on the original reference (scs_site_ref.h) as a
stand-alone CPU program, every body and both unlifted totals compared with the restatement's (tests/site_ref_cases.py) at min_reads
0, 1 and 1000 and at every slab size of the test, every array in a heap block of exactly its size; then the test's broken inputs,
each refused.  No GPU, nothing preloaded, no Python in the sanitized process.

    python tools/site_ref_host_check.py [--cxx g++]
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
    import numpy as np
    import test_artefacts_ref_host as t
    rows = []

    def case(w, starts, lens, reads, edits, min_reads, slab, rc, lift_err=0, want="", unl=(0, 0), hap_lens=None, ref_lens=None, seg=None):
        hap_lens, ref_lens = hap_lens or w.hap_lens, ref_lens or w.ref_lens
        seg = seg if seg is not None else np.stack([getattr(w.segs, k) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")], axis=1)
        f = [min_reads, slab or (1 << 28), rc, lift_err, unl[0], unl[1], w.genome, len(hap_lens)] + list(hap_lens) + [len(ref_lens)] + [v for nl in zip(w.ref_names, ref_lens) for v in nl]
        f += [len(seg)] + [int(v) for s in seg for v in s] + [len(starts)] + [v for amp in zip(starts, lens, reads) for v in amp] + [len(edits)] + [v for e in edits for v in e] + [want.count("\n")]
        rows.append("case " + " ".join(str(v) for v in f))
        if want:
            rows.append(want.rstrip("\n"))

    for name in sorted(t.CASES):
        w, amps = t.CASES[name]
        for min_reads in (0, 1, 1000):
            want, _, unl, _ = w.want(amps, min_reads)
            for slab in t.SLABS:
                case(w, *w.inputs(amps), min_reads, slab, 0, 0, want, unl)
    # the broken inputs of test_inputs_that_do_not_fit_are_refused, made the same way: refused (SCS_EINVAL = 1), nothing read outside
    w = t.MIX
    starts, lens, reads, edits = w.inputs([(0, 60, 170, 2, [(70, 1)])])
    base = np.stack([getattr(w.segs, k) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")], axis=1)
    case(w, [150], [60], reads, [], 0, 0, 1)
    case(w, [int(w.hap_off[-1]) - 5], [20], reads, [], 0, 0, 1)
    case(w, starts, lens, reads, [(0, 170, 1)], 0, 0, 1)
    case(w, starts, lens, reads, [(1, 70, 1)], 0, 0, 1)
    case(w, starts, lens, reads, [(0, 70, 4)], 0, 0, 1)
    case(w, starts, lens, reads, [(0, 70, 1), (0, 70, 2)], 0, 0, 1)
    case(w, starts, lens, reads, edits, 0, 0, 1, hap_lens=w.hap_lens[:-1] + [w.hap_lens[-1] - 1])
    s = base.copy(); s[2][0] += 1; s[2][1] -= 1
    case(w, starts, lens, reads, edits, 0, 0, 1, 2, seg=s)
    case(w, starts, lens, reads, edits, 0, 0, 1, 2, seg=base[:2])
    s = base.copy(); s[3][2] += 1
    case(w, starts, lens, reads, edits, 0, 0, 1, 3, seg=s)
    s = base.copy(); s[2][3] = 2
    case(w, starts, lens, reads, edits, 0, 0, 1, 3, seg=s)
    s = base.copy(); s[3][1] += 5
    case(w, [150], [40], reads, [], 0, 0, 1, 2, seg=s)
    case(w, starts, lens, reads, edits, 0, 0, 1, ref_lens=[w.ref_lens[0], 1 << 58])
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "site_ref_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "site_ref_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
