"""The coverage profile (scs_set_coverage) restated in plain numpy, shared by tests/test_coverage_host.py and
tests/test_gpu_coverage.py: what one read marks, by way of POS and CIGAR; per-base depth, histogram and sums from a difference
array or from a SAM; the summary (mean, breadths, Gini) from per-base depths; the file.  Not collected."""
import re

import numpy as np

CIG = re.compile(r"(\d+)([MID])")
BREADTHS = (1, 5, 10, 20)


# ---- one read

def window_bases(n, events):
    """Profile::predict's output: per read base its window index, or -1 for an inserted base (after the n + delta < 50 rollback)."""
    if n + sum(-l if d else l for _, d, l in events) < 50:
        events = []
    ev = {p: (d, l) for p, d, l in events}
    out, j = [], 0
    while j < n:
        if j in ev and ev[j][0]:
            j += ev[j][1]
            continue
        out.append(j)
        if j in ev:
            out += [-1] * ev[j][1]
        j += 1
    return out


def pos_cigar(pos0, n, events, reverse):
    """(POS - 1, CIGAR) of the read, genome-forward, as the truth SAM states them: deletions before the first and after the last
    aligned base are dropped, an insertion at either end stays."""
    coords = [None if x < 0 else (pos0 - x if reverse else pos0 + x) for x in window_bases(n, events)]
    if reverse:
        coords = coords[::-1]
    ops, prev = [], None
    for c in coords:
        if c is None:
            k, l = "I", 1
        else:
            if prev is not None and c > prev + 1:
                ops.append(["D", c - prev - 1])
            k, l, prev = "M", 1, c
        if ops and ops[-1][0] == k:
            ops[-1][1] += l
        else:
            ops.append([k, l])
    return min(c for c in coords if c is not None), "".join("%d%s" % (l, k) for k, l in ops)


def intervals(pos, cigar):
    """The contract, from POS and CIGAR alone: the maximal runs [start, end) of genome bases an M operation aligns; only a D ends a run."""
    cov, g = set(), pos
    for l, k in CIG.findall(cigar):
        l = int(l)
        if k == "M":
            cov.update(range(g, g + l))
        if k != "I":
            g += l
    xs = sorted(cov)
    out = []
    for x in xs:
        if out and out[-1][1] == x:
            out[-1][1] = x + 1
        else:
            out.append([x, x + 1])
    return [tuple(iv) for iv in out]


def m_length(cigar):
    return sum(int(l) for l, k in CIG.findall(cigar) if k == "M")


# ---- the tables from per-base depths

def tables(depth, codes, rec_lens, D):
    """hist[records][D + 1], n_bases, sum, sum_n per record from per-base depths (any integer array), codes (4 = N) and the records' lengths."""
    depth, codes = np.asarray(depth, np.int64), np.asarray(codes)
    off = np.concatenate([[0], np.cumsum(np.asarray(rec_lens, np.int64))])
    nr = len(rec_lens)
    hist, n_n, s, s_n = np.zeros((nr, D + 1), np.uint64), np.zeros(nr, np.uint64), np.zeros(nr, np.uint64), np.zeros(nr, np.uint64)
    for r in range(nr):
        d, c = depth[off[r]:off[r + 1]], codes[off[r]:off[r + 1]]
        acgt = c < 4
        hist[r] = np.bincount(np.minimum(d[acgt], D), minlength=D + 1)
        n_n[r], s[r], s_n[r] = int((~acgt).sum()), int(d[acgt].sum()), int(d[~acgt].sum())
    return dict(hist=hist, n_bases=n_n, sum=s, sum_n=s_n)


def with_genome_row(t):
    return {k: np.concatenate([v, v.sum(axis=0, keepdims=True)]).astype(np.uint64) for k, v in t.items()}


def stats_from_depths(depth, D):
    """The documented summary of non-N per-base depths with buckets 0 .. D: mean; breadth at t = the fraction at depth >= min(t, D)
    (a threshold above D can only count the top bucket); Gini of the Lorenz curve with every base of depth >= D taken at the mean
    depth of those bases -- the Gini of the depths themselves when none reaches D.  No bases, or all depths 0: gini 0."""
    d = np.asarray(depth, np.int64)
    n = d.size
    if n == 0:
        return dict(mean=0.0, breadth=(0.0,) * 4, gini=0.0)
    total = int(d.sum())
    breadth = tuple(float((d >= min(t, D)).sum()) / n for t in BREADTHS)
    if total == 0:
        return dict(mean=0.0, breadth=breadth, gini=0.0)
    # the Lorenz curve over the distinct values: at most D + 1 terms, the masses integers (the top bucket's: the exact sum of its depths)
    k = np.minimum(d, D)
    cnt = np.bincount(k, minlength=D + 1).astype(np.float64)
    mass = np.bincount(k, weights=d.astype(np.float64), minlength=D + 1)
    S = np.cumsum(mass)
    acc = float((cnt * (S - mass + S)).sum())
    return dict(mean=total / n, breadth=breadth, gini=1.0 - acc / (float(n) * float(total)))


def gini_pairwise(x):
    """sum |x_i - x_j| / (2 n^2 mean): the definition, for small arrays."""
    x = np.asarray(x, np.float64)
    return float(np.abs(x[:, None] - x[None, :]).sum()) / (2.0 * x.size * x.size * x.mean())


# ---- from a difference array (the end-of-job kernels)

def finish_reference(diff, codes, rec_lens, D):
    depth = np.cumsum(np.asarray(diff, np.int64))
    assert depth[-1] == 0 and (depth >= 0).all()
    t = tables(depth[:-1], codes, rec_lens, D)
    t["depth"] = depth[:-1].astype(np.uint32)
    return t


# ---- from a truth SAM

def depth_from_sam(hdr, recs):
    """({record: int64 per-base depth}, [(name, length)] in @SQ order, sum of the M lengths, records with I or D) from @SQ, POS and CIGAR."""
    sq = [(h.split("\t")[1][3:], int(h.split("\t")[2][3:])) for h in hdr if h.startswith("@SQ")]
    diff = {name: np.zeros(ln + 1, np.int64) for name, ln in sq}
    m_sum = indel = 0
    for r in recs:
        g, d = int(r[3]) - 1, diff[r[2]]
        indel += ("I" in r[5]) or ("D" in r[5])
        for l, k in CIG.findall(r[5]):
            l = int(l)
            if k == "M":
                d[g] += 1; d[g + l] -= 1; m_sum += l
            if k != "I":
                g += l
    return {name: np.cumsum(d)[:-1] for name, d in diff.items()}, sq, m_sum, indel


# ---- the file

def parse_file(path):
    """(max_depth, {record: summary row as floats}, [(record, depth, count, size, fraction)]) of scs_write_coverage's text."""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("#coverage\tmax_depth=") and ">=" in lines[0]
    D = int(lines[0].split("\t")[1].split("=")[1])
    assert lines[1] == "#summary\trecord\tbases\tn_bases\taligned\tmean\tbreadth1\tbreadth5\tbreadth10\tbreadth20\tgini"
    summ, i = [], 2
    while lines[i].startswith("#s\t"):
        f = lines[i].split("\t")
        summ.append((f[1], [int(v) for v in f[2:5]] + [float(v) for v in f[5:]]))
        i += 1
    assert lines[i] == "#record\tdepth\tcount\tsize\tfraction"
    rows = [(f[0], int(f[1]), int(f[2]), int(f[3]), float(f[4])) for f in (ln.split("\t") for ln in lines[i + 1:-1])]
    return D, summ, rows


def render(names, t, D):
    """What the file must hold, from the downloaded arrays (records + 1 rows, the genome's last): the summary rows and the histogram rows."""
    summ, rows = [], []
    for r, name in enumerate(list(names) + ["genome"]):
        h = t["hist"][r].astype(np.int64)
        size = int(h.sum())
        # the summary from the histogram alone: the top bucket's bases at their mean depth (the documented rule)
        s = stats_from_hist(h, int(t["sum"][r]), D)
        summ.append((name, [size + int(t["n_bases"][r]), int(t["n_bases"][r]), int(t["sum"][r]) + int(t["sum_n"][r]), s["mean"]] + list(s["breadth"]) + [s["gini"]]))
        rows += [(name, k, int(h[k]), size, int(h[k]) / size) for k in range(D + 1) if h[k]]
    return summ, rows


def stats_from_hist(h, total, D):
    h = np.asarray(h, np.int64)
    n = int(h.sum())
    if n == 0:
        return dict(mean=0.0, breadth=(0.0,) * 4, gini=0.0)
    breadth = tuple(float(h[min(t, D):].sum()) / n for t in BREADTHS)
    if total == 0:
        return dict(mean=0.0, breadth=breadth, gini=0.0)
    mass = (np.arange(D + 1) * h).astype(np.float64)
    mass[D] = total - float(mass[:D].sum())
    S = np.cumsum(mass)
    acc = float((h * (S - mass + S)).sum())
    return dict(mean=total / n, breadth=breadth, gini=1.0 - acc / (float(n) * float(total)))


# ---- the case table of the end-of-job kernels (scs_coverage_finish_probe).  spec: size (a name below), fam (the difference family),
# recs (one | mixed), codes (acgt | all_n | blocks), lds (buckets of the LDS histogram; -1: the product's)

def finish_name(spec):
    return "%s-%s-%s-%s-lds%d" % (spec["size"], spec["fam"], spec["recs"], spec["codes"], spec["lds"])


def finish_case(spec, T, C):
    """(diff int32[G + 1], codes uint8[G], rec_lens, max_depth) of a case, from the tile T and the offset scan's chunk C."""
    G = {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "1000003": 1000003,
         "T(C-1)": T * (C - 1), "TC": T * C, "TC+1": T * C + 1}[spec["size"]]
    rng = np.random.default_rng(abs(hash_name(finish_name(spec))) % (1 << 32))
    D = 65535 if spec["fam"] == "pile" and spec["recs"] == "one" else 50
    # records: one, or lengths 1, 2, 37, T - 1, T, T + 1 repeated (several records in one tile, records over several tiles)
    if spec["recs"] == "one":
        lens = [G]
    else:
        lens, left, k = [], G, 0
        cyc = [1, 2, 37, T - 1, T, T + 1]
        while left:
            lens.append(min(cyc[k % 6], left)); left -= lens[-1]; k += 1
    off = np.concatenate([[0], np.cumsum(lens)])
    # codes: no N, all N, or N blocks over tile borders and record borders (and the first bases)
    codes = rng.integers(0, 4, G).astype(np.uint8)
    if spec["codes"] == "all_n":
        codes[:] = 4
    elif spec["codes"] == "blocks":
        codes[:min(G, 2)] = 4
        for b in list(range(T, G, T)) + [int(x) for x in off[1:-1][::max(1, len(off) // 400)]]:
            codes[max(0, b - 3):min(G, b + 5)] = 4
    d = np.zeros(G + 1, np.int64)

    def reads(n, max_len=150):
        st = rng.integers(0, G, n)
        en = np.minimum(st + rng.integers(1, max_len + 1, n), G)
        np.add.at(d, st, 1); np.add.at(d, en, -1)
    fam = spec["fam"]
    if fam == "ones":
        d[0] += 1; d[G] -= 1
    elif fam == "reads":
        reads(max(1, G * 3 // 100))
    elif fam == "tile_edges":                               # intervals that end, and begin, exactly on tile borders; one that ends on G
        for b in range(T, G + 1, T):
            l = int(rng.integers(1, 200))
            d[max(0, b - l)] += 1; d[b] -= 1
            if b < G:
                d[b] += 1; d[min(G, b + l)] -= 1
        d[max(0, G - 7)] += 1; d[G] -= 1
    elif fam == "pile":                                     # 70 000 on one base: the top bucket, and past any LDS table
        p = G // 2
        d[p] += 70000; d[p + 1] -= 70000
        reads(max(1, G // 100))
    elif fam == "around_d":                                 # depth D - 1, D, D + 1 on neighbouring bases
        if G >= 3:
            p = min(max(G // 3, 0), G - 3)
            d[p] += D - 1; d[p + 1] += 1; d[p + 2] += 1; d[p + 3] -= D + 1
        else:
            d[0] += D; d[1] -= D
        reads(max(1, G // 200))
    else:
        assert fam == "zeros", fam
    return d.astype(np.int32), codes, lens, D


def hash_name(name):
    h = 0
    for ch in name.encode():
        h = (h * 131 + ch) % 1000000007
    return h


def finish_seen(want, codes, lens, D, T):
    """What a case reaches, for the tests to assert that the table puts its cases where it says."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G = int(off[-1])
    borders = off[1:-1]
    tb = np.arange(T, G, T)
    n4 = np.asarray(codes) == 4
    return dict(records_in_one_tile=int(np.bincount(off[:-1] // T).max()), tiles_of_one_record=int(-(-max(lens) // T)),
                n_over_tile_border=bool(len(tb) and (n4[tb - 1] & n4[tb]).any()), n_over_record_border=bool(len(borders) and (n4[borders - 1] & n4[borders]).any()),
                distinct_depths=int(len(np.unique(want["depth"]))), max_depth_seen=int(want["depth"].max()), top_bucket=int(want["hist"][:, D].sum()), D=int(D))
