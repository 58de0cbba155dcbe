#!/usr/bin/env python3
"""Builds tools/support_ref_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and replays the case table of
tests/test_support_ref_host.py through it: the host code of the site support table on the original reference (scs_support_ref.h) as
a stand-alone CPU program -- every layout and list of positions at every fill chunk of the test, the staged positions, their
reference positions and the gathered counters compared with the restatement's (tests/support_ref_cases.py), every array in a heap
block of exactly its size; then broken tables, each refused with its reason.  No GPU, nothing preloaded, no Python in the
sanitized process.

    python tools/support_ref_host_check.py [--cxx g++]
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
    import test_support_ref_host as t
    from support_ref_cases import restate
    rows = []

    def case(w, xs, chunk, rc=0, why=0, seg=None, counts=True, seed=3):
        seg = seg if seg is not None else np.stack([getattr(w.segs, k) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")], axis=1)
        n = int(sum(w.hap_lens))
        f = [chunk, rc, why, len(w.hap_lens)] + list(w.hap_lens) + [len(w.ref_lens)] + list(w.ref_lens) + [len(seg)] + [int(v) for s in seg for v in s] + [len(xs)] + [int(v) for v in xs]
        g = np.random.default_rng(seed).integers(0, 50, (n, 6)) if counts else None
        f += [1 if counts else 0] + ([] if g is None else g.reshape(-1).tolist())
        if rc == 0:
            pos, px, sums = restate(n, w.segs, w.ref_lens, xs, g)
            f += [len(pos)] + [int(v) for pv in zip(pos, px) for v in pv] + ([] if sums is None else sums.reshape(-1).tolist())
        else:
            f += [0]
        rows.append("case " + " ".join(str(v) for v in f))

    for name in sorted(t.LAYOUTS):
        w = t.LAYOUTS[name]
        for xs in t.x_lists(w).values():
            for chunk in [0] + t.CHUNKS:
                case(w, xs, chunk)
            case(w, xs, 0, counts=False)
    rng = np.random.default_rng(23)
    for trial in range(6):
        w = t.random_world(rng, trial)
        for k in (1, 40, int(sum(w.ref_lens))):
            xs = np.sort(rng.choice(int(sum(w.ref_lens)), k, replace=False))
            for chunk in (0, 1, 3):
                case(w, xs, chunk, seed=trial)
    # broken tables, made as test_broken_tables_are_refused_with_their_reason makes them: refused (SCS_EINVAL = 1), nothing read outside
    w, xs = t.MIX, [10, 150, 250]
    base = np.stack([getattr(w.segs, k) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")], axis=1)
    s = base.copy(); s[3][2] += 1
    case(w, xs, 0, 1, 3, seg=s)
    s = base.copy(); s[2][3] = 2
    case(w, xs, 0, 1, 3, seg=s)
    case(w, xs, 0, 1, 2, seg=np.concatenate([base[:1], base[2:3], base[1:2], base[3:]]))
    s = base.copy(); s[2][0] += 1; s[2][1] -= 1
    case(w, xs, 0, 1, 2, seg=s)
    s = base.copy(); s[1][1] = 0
    case(w, xs, 0, 1, 2, seg=s)
    s = base.copy(); s[3][1] += 5
    case(w, xs, 0, 1, 2, seg=s)
    case(w, [150, 10], 0, 1, 4)
    case(w, [10, 10], 0, 1, 4)
    case(w, [10, 300], 0, 1, 4)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "support_ref_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "support_ref_host_check.cpp"), "-o", exe])
        r = subprocess.run([exe], input="\n".join(rows) + "\n", text=True)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
