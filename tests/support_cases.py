"""The site support's reference restatement on the SAM side, shared by tests/test_gpu_support.py and tests/test_gpu_support_ref.py:
a pileup of a truth SAM at given coordinates in plain numpy."""
import numpy as np

from gpu_readers import CIG, _sam

CLS = {"A": 0, "C": 1, "G": 2, "T": 3}


def pileup_from_sam(path, rec, pos):
    """The contract from the SAM alone: (counts [positions, 6], positions' index per site, figures) at the distinct coordinates of
    the sites (rec, pos).  POS, CIGAR and SEQ; inserted bases are skipped, D gives class 5."""
    hdr, recs = _sam(path)
    sq = [(h.split("\t")[1][3:], int(h.split("\t")[2][3:])) for h in hdr if h.startswith("@SQ")]
    off = np.concatenate([[0], np.cumsum([ln for _, ln in sq])]).astype(np.int64)
    first = {name: off[i] for i, (name, _) in enumerate(sq)}
    x = off[rec.astype(np.int64)] + pos.astype(np.int64)
    assert (np.diff(x) >= 0).all()
    P, site_pos = np.unique(x, return_inverse=True)
    cnt = np.zeros((len(P), 6), np.int64)
    fig = dict(records=len(recs), reverse=0, ins_left=0, contributions=0)
    for r in recs:
        g, qi, seq, rev, ins, hit_after_ins = first[r[2]] + int(r[3]) - 1, 0, r[9], int(r[1]) & 16, False, False
        for n, k in CIG.findall(r[5]):
            n = int(n)
            if k == "I":
                qi += n; ins = True
                continue
            lo, hi = np.searchsorted(P, [g, g + n])
            for j in range(lo, hi):
                cnt[j, 5 if k == "D" else CLS.get(seq[qi + P[j] - g], 4)] += 1
                fig["contributions"] += 1
                fig["reverse"] += 1 if rev else 0
                hit_after_ins |= ins
            g += n
            if k == "M":
                qi += n
        fig["ins_left"] += 1 if hit_after_ins else 0
    return cnt, site_pos, fig
