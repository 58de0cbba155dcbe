"""The GC-bias table of the per-base depth (scs_gc_bias, scs_write_gc_bias) restated in plain numpy, the case
table of its kernel (scs_gc_bias_probe), what a case reaches, and the file's reader and rendering.  Shared by
tests/test_gcbias_host.py (no GPU) and tests/test_gpu_gcbias.py; imports from no test module.

The rule: every window of W neighbouring bases inside one record, sliding by one base.  A window with an N (code >= 4) counts in
n_windows only; every other one adds 1 to windows[b] and the sum of its W depths to depth_sum[b], b = 100 * gc // W, gc its bases of
code 1 or 2 (C, G: scs_common.h's is_gc)."""
import numpy as np

BINS = 101
MAX_WINDOW = 1024


def windows_of(depth, codes, rec_lens, W):
    """Per record with at least W bases: (record, global index of its first window, depth sums uint64, G/C counts, N counts) of its
    windows in order -- numpy.cumsum per record and differences at distance W."""
    depth, codes, off = np.asarray(depth), np.asarray(codes), 0
    for r, L in enumerate(int(x) for x in rec_lens):
        if L >= W:
            d, c = depth[off:off + L].astype(np.uint64), codes[off:off + L]
            pd = np.concatenate([np.zeros(1, np.uint64), np.cumsum(d, dtype=np.uint64)])
            pg = np.concatenate([[0], np.cumsum((c == 1) | (c == 2))]).astype(np.int64)
            pn = np.concatenate([[0], np.cumsum(c >= 4)]).astype(np.int64)
            yield r, off, pd[W:] - pd[:-W], pg[W:] - pg[:-W], pn[W:] - pn[:-W]
        off += L


def reference(depth, codes, rec_lens, W):
    """dict(windows=uint64[records][101], depth_sum=uint64[records][101], n_windows=uint64[records]): exact integers throughout
    (numpy.add.at on uint64, no float weights)."""
    assert 1 <= W <= MAX_WINDOW
    nr = len(rec_lens)
    out = dict(windows=np.zeros((nr, BINS), np.uint64), depth_sum=np.zeros((nr, BINS), np.uint64), n_windows=np.zeros(nr, np.uint64))
    for r, _, ds, gc, nn in windows_of(depth, codes, rec_lens, W):
        ok = nn == 0
        b = 100 * gc[ok] // W
        out["n_windows"][r] = int((~ok).sum())
        out["windows"][r] = np.bincount(b, minlength=BINS).astype(np.uint64)
        np.add.at(out["depth_sum"][r], b, ds[ok])
    return out


def with_genome_row(t):
    """One more row, the sum of the records' rows (what scs_gc_bias returns)."""
    return {k: np.concatenate([v, v.sum(axis=0, keepdims=True, dtype=np.uint64)]) for k, v in t.items()}


def brute_force(depth, codes, rec_lens, W):
    """The rule as a loop over windows, in Python integers."""
    nr, off = len(rec_lens), 0
    win, dsum, nwin = [[0] * BINS for _ in range(nr)], [[0] * BINS for _ in range(nr)], [0] * nr
    for r, L in enumerate(rec_lens):
        for p in range(off, off + L - W + 1):
            c = [int(x) for x in codes[p:p + W]]
            if any(x >= 4 for x in c):
                nwin[r] += 1
            else:
                b = 100 * sum(x in (1, 2) for x in c) // W
                win[r][b] += 1; dsum[r][b] += sum(int(x) for x in depth[p:p + W])
        off += L
    return dict(windows=win, depth_sum=dsum, n_windows=nwin)


def same(got, want):
    """The three tables equal, bit for bit; else what differs."""
    bad = []
    for k in ("windows", "depth_sum", "n_windows"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != np.uint64 or g.shape != w.shape or not (g == w.astype(np.uint64)).all():
            bad.append(k)
    return bad


# ---- derived values and the file

def derived(windows, depth_sum, W):
    """(mean_depth[101], row_mean, normalized[101]) of one row as the contract states them, from Python's integer quotients."""
    n, s = [int(x) for x in windows], [int(x) for x in depth_sum]
    row_mean = sum(s) / (W * sum(n)) if sum(n) else 0.0
    mean = [s[b] / (n[b] * W) if n[b] else 0.0 for b in range(BINS)]
    return mean, row_mean, [m / row_mean if row_mean > 0 else 0.0 for m in mean]


def render(names, t, W, model):
    """The file's text from a table with the genome's row last; model: the profile's 101 gc_means as floats, or None."""
    names = list(names) + ["genome"]
    rows = [derived(t["windows"][r], t["depth_sum"][r], W) for r in range(len(names))]
    out = ["#gc_bias\twindow=%d\tstep=1\texcluded=windows_with_N\tbin=100*gc/window" % W, "#summary\trecord\twindows\tn_windows\tmean_depth"]
    out += ["#s\t%s\t%d\t%d\t%.6f" % (nm, int(t["windows"][r].sum()), int(t["n_windows"][r]), rows[r][1]) for r, nm in enumerate(names)]
    out.append("#record\tgc\twindows\tdepth_sum\tmean_depth\tnormalized\tmodel")
    for r, nm in enumerate(names):
        out += ["%s\t%d\t%d\t%d\t%.6f\t%.6f\t%s" % (nm, b, int(t["windows"][r][b]), int(t["depth_sum"][r][b]), rows[r][0][b], rows[r][2][b], "%.6g" % model[b] if model is not None else ".")
                for b in range(BINS) if int(t["windows"][r][b])]
    return "\n".join(out) + "\n"


def profile_gc_means(path):
    """gc_means[0 .. 100] of a .profile text: the [Log Ratio Mean Value] section's gc<TAB>mean lines."""
    lines = open(path).read().split("\n")
    at = lines.index("[Log Ratio Mean Value]")
    m = [None] * BINS
    for ln in lines[at + 1:at + 1 + BINS]:
        k, v = ln.split("\t")
        m[int(k)] = float(v)
    assert None not in m
    return m


def codes_of(seq):
    """base codes of an upper-case sequence of bytes: ACGT = 0 .. 3, anything else 4"""
    lut = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    return lut[np.frombuffer(seq, np.uint8)]


# ---- the case table of the kernel (scs_gc_bias_probe).  spec: size (a name below), W, lay (one | mix | halo), codes, depth (family names),
# lds (-1: the product's choice; 0: no LDS table)

SIZES = ["1", "2", "63", "64", "65", "99", "100", "101", "T-1", "T", "T+1", "T+W-2", "T+W-1", "T+W", "2T+1"]
WINDOWS = [1, 2, 7, 63, 64, 65, 100, 1000, 1024]
LAYOUTS = ["one", "mix", "halo"]
CODES = ["acgt", "gc", "at", "ramp", "all_n", "n_blocks", "n_last"]
DEPTHS = ["zeros", "ones", "reads", "pile", "huge"]
LDS = [-1, 0]
BIG = ["1000003", "4Tx1024+1"]


def name_of(spec):
    return "%s-w%d-%s-%s-%s-lds%d" % (spec["size"], spec["W"], spec["lay"], spec["codes"], spec["depth"], spec["lds"])


def size_of(spec, T):
    W = spec["W"]
    return {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "99": 99, "100": 100, "101": 101, "T-1": T - 1, "T": T, "T+1": T + 1, "T+W-2": max(1, T + W - 2),
            "T+W-1": T + W - 1, "T+W": T + W, "2T+1": 2 * T + 1, "1000003": 1000003, "4Tx1024+1": 4 * T * 1024 + 1}[spec["size"]]


def table_cases():
    """Every (size, W) pair once per lds with the layouts and families rotating under them (steps of 2, 7 and 5 are coprime, so every
    family meets every other and each lds); named cases for what the rotation could miss; the two large ones."""
    out, i = [], 0
    for lds in LDS:
        for size in SIZES:
            for W in WINDOWS:
                out.append(dict(size=size, W=W, lay=LAYOUTS[i % 2], codes=CODES[i % 7], depth=DEPTHS[i % 5], lds=lds)); i += 1
        i += 3
        out += [dict(size="2T+1", W=100, lay="mix", codes="ramp", depth="reads", lds=lds), dict(size="2T+1", W=7, lay="mix", codes="n_blocks", depth="pile", lds=lds),
                dict(size="T+W", W=1024, lay="one", codes="acgt", depth="huge", lds=lds), dict(size="2T+1", W=1000, lay="mix", codes="n_last", depth="huge", lds=lds),
                dict(size="2T+1", W=100, lay="halo", codes="acgt", depth="reads", lds=lds), dict(size="2T+1", W=1024, lay="halo", codes="n_blocks", depth="ones", lds=lds),
                dict(size="2T+1", W=65, lay="mix", codes="gc", depth="reads", lds=lds), dict(size="2T+1", W=64, lay="one", codes="n_blocks", depth="reads", lds=lds)]
    out += [dict(size="1000003", W=100, lay="one", codes="ramp", depth="reads", lds=-1), dict(size="1000003", W=100, lay="mix", codes="ramp", depth="reads", lds=0),
            dict(size="4Tx1024+1", W=1024, lay="one", codes="acgt", depth="reads", lds=-1)]
    seen, uniq = set(), []
    for s in out:
        if name_of(s) not in seen:
            seen.add(name_of(s)); uniq.append(s)
    return uniq


def hash_name(name):
    h = 0
    for ch in name.encode():
        h = (h * 131 + ch) % 1000000007
    return h


def layout_of(lay, G, W, T):
    """one record; records of 1, 2, 37, W - 1, W, W + 1, T - 1, T, T + 1 repeated until G bases are placed; or two records with
    their border one base behind the first tile border: inside the halo of the first tile's windows"""
    if lay == "one" or (lay == "halo" and G <= T + 1):
        return [G]
    if lay == "halo":
        return [T + 1, G - T - 1]
    assert lay == "mix", lay
    cyc = [x for x in (1, 2, 37, W - 1, W, W + 1, T - 1, T, T + 1) if x > 0]
    lens, left, k = [], G, 0
    while left:
        lens.append(min(cyc[k % len(cyc)], left)); left -= lens[-1]; k += 1
    return lens


def case(spec, T):
    """(depth uint32[G], codes uint8[G], rec_lens, W, lds) of a case, seeded by its name."""
    W, G = spec["W"], size_of(spec, T)
    rng = np.random.default_rng(hash_name(name_of(dict(spec, lds=0))))     # (both lds choices of a case see the same arrays)
    lens = layout_of(spec["lay"], G, W, T)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fam = spec["codes"]
    codes = rng.integers(0, 4, G).astype(np.uint8)
    if fam == "gc":
        codes = rng.integers(1, 3, G).astype(np.uint8)
    elif fam == "at":
        codes = (3 * rng.integers(0, 2, G)).astype(np.uint8)
    elif fam == "ramp":                                     # blocks of 2 W bases; in block k every W neighbours hold k * W // 100 of G or C: at W = 100 bin k
        i = np.arange(G, dtype=np.int64)
        k = (i // (2 * W)) % BINS
        is_gc = (i % W) < (k * W + 99) // 100
        codes = np.where(is_gc, 1 + (i & 1), 3 * ((i >> 1) & 1)).astype(np.uint8)
    elif fam == "all_n":
        codes[:] = 4
    elif fam == "n_blocks":                                 # N over every odd tile border and over some record borders, on the first bases,
        codes[:min(G, 2)] = 4                               # and from every even tile border on: an N only in the halo of the windows before it
        for b in list(range(T, G, 2 * T)) + [int(x) for x in off[1:-1][::max(1, len(off) // 400)]]:
            codes[max(0, b - 3):min(G, b + 5)] = 4
        for b in range(2 * T, G, 2 * T):
            codes[b:min(G, b + 5)] = 4
    elif fam == "n_last":                                   # a single N at every fourth tile's last base (the first tile's too)
        codes[T - 1::4 * T] = 4
    else:
        assert fam == "acgt", fam
    d = np.zeros(G + 1, np.int64)

    def reads(n, max_len=150):
        st = rng.integers(0, G, n)
        en = np.minimum(st + rng.integers(1, max_len + 1, n), G)
        np.add.at(d, st, 1); np.add.at(d, en, -1)
    fam = spec["depth"]
    if fam == "ones":
        d[0] += 1; d[G] -= 1
    elif fam == "reads":
        reads(max(1, G * 3 // 100))
    elif fam == "pile":                                     # 70 000 on a few bases
        p = G // 2
        d[p] += 70000; d[min(G, p + 3)] -= 70000
        reads(max(1, G // 100))
    elif fam == "huge":                                     # a stretch near 2^31 - 1: a window of three bases or more passes 2^32
        p, q = G // 3, min(G, G // 3 + 3000)
        d[p] += 2 ** 31 - 1 - 200; d[max(q, p + 1)] -= 2 ** 31 - 1 - 200
        reads(max(1, G // 100))
    else:
        assert fam == "zeros", fam
    depth = np.cumsum(d)[:G]
    assert depth.min() >= 0 and depth.max() < 2 ** 32
    return depth.astype(np.uint32), codes, lens, W, spec["lds"]


def seen(depth, codes, lens, W, T):
    """What a case reaches, from the restatement alone, for the host test to assert that the table puts its cases where it says."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G, borders, n4 = int(off[-1]), off[1:-1], np.asarray(codes) >= 4
    pn = np.concatenate([[0], np.cumsum(n4)]).astype(np.int64)
    tb = np.arange(T, G, T)
    s = dict(crosses_tile=False, n_only_in_halo=False, max_sum=0, bins=set(), windows=0, n_windows=0)
    for r, o, ds, gc, nn in windows_of(depth, codes, lens, W):
        p = o + np.arange(len(ds), dtype=np.int64)
        tile_end = (p // T + 1) * T
        s["crosses_tile"] |= bool((p + W > tile_end).any())
        s["n_only_in_halo"] |= bool(((nn > 0) & (pn[np.minimum(p + W, tile_end)] - pn[p] == 0)).any())
        s["max_sum"] = max(s["max_sum"], int(ds.max()))
        s["bins"] |= set((100 * gc[nn == 0] // W).tolist())
        s["windows"] += int((nn == 0).sum()); s["n_windows"] += int((nn > 0).sum())
    lens = [int(x) for x in lens]
    s.update(ends_on_record_end=any(L >= W for L in lens), shorter=any(0 < L < W for L in lens), exact=W in lens, plus1=W + 1 in lens,
             border_in_tile=bool((borders % T != 0).any()), border_in_halo=bool(((borders > T) & (borders % T > 0) & (borders % T < W - 1)).any()),
             n_over_tile_border=bool(len(tb) and (n4[tb - 1] & n4[tb]).any()), n_over_record_border=bool(len(borders) and (n4[borders - 1] & n4[borders]).any()),
             tiles=-(-G // T))
    return s
