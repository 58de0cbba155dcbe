"""The restatement of the site support table on the original reference (scs_set_site_support_ref), shared by
tests/test_support_ref_host.py, tests/test_gpu_support_ref.py and tools/support_ref_host_check.py.

Plain numpy and PER BASE: X(g) for every staged index from the segment table (-1 in inserted sequence), the staged positions are
the indices whose X is listed, the reference counters are np.add.at of per-index counters onto X(g).  Nothing here is shared with
the library: no segments as intervals, no ranges, no bisection, no scan, no output slots."""
import numpy as np

from site_ref_cases import ref_index

INFO3 = ['##INFO=<ID=DP,Number=1,Type=Integer,Description="reads of the job with a base aligned at the site">',
         '##INFO=<ID=AD,Number=2,Type=Integer,Description="reads that show the reference base, reads that show the alternate base">',
         '##INFO=<ID=DL,Number=1,Type=Integer,Description="reads whose alignment deletes the site">']


def staged_positions(n, segs, ref_lens, site_x):
    """(X(g) per staged index, the staged positions: every g whose X(g) is one of site_x, ascending)"""
    X, _ = ref_index(n, segs, ref_lens)
    return X, np.nonzero(np.isin(X, np.asarray(site_x, np.int64)))[0]


def restate(n, segs, ref_lens, site_x, g_counts=None):
    """(staged positions, for each the index of its X in the sorted distinct site_x, [len(x), 6] sums of g_counts or None)"""
    xs = np.unique(np.asarray(site_x, np.int64))
    X, pos = staged_positions(n, segs, ref_lens, xs)
    pos_x = np.searchsorted(xs, X[pos])
    sums = None
    if g_counts is not None:
        by_x = np.zeros((int(np.sum(np.asarray(ref_lens, np.int64))), 6), np.int64)
        R = X >= 0
        np.add.at(by_x, X[R], np.asarray(g_counts, np.int64)[R])
        sums = by_x[xs]
    return pos, pos_x, sums


def strip_support(text):
    """A site support file's text without its three ##INFO lines and without ';DP=..;AD=..;DL=..' at the end of every line"""
    out = []
    for ln in text.split("\n"):
        if ln in INFO3:
            continue
        if ln and not ln.startswith("#"):
            head, sep, _ = ln.rpartition(";DP=")
            assert sep, ln
            ln = head
        out.append(ln)
    return "\n".join(out)


def fields(line):
    """(DP, (AD_ref, AD_alt), DL) of one line of the table"""
    kv = dict(f.split("=") for f in line.rstrip("\n").split("\t")[7].split(";"))
    r, a = kv["AD"].split(",")
    return int(kv["DP"]), (int(r), int(a)), int(kv["DL"])
