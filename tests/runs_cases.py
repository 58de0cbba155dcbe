"""Plain-numpy restatement of the bedGraph writer (scs_write_coverage_bedgraph, scs_write_coverage_ref_bedgraph,
scs_write_copy_number_ref) and the case table of its kernels' probe (scs_runs_probe).  Nothing here is shared
with the library.  Not collected."""
import numpy as np

FULL, LOW = 0xFFFFFFFF, 0xFFFF
LONG_NAME = "chrLong_" + "x" * 192                          # 200 bytes

# ---- the restatement


def runs(values, mask, rec_lens):
    """(global start, global end, record, masked value) of every maximal run of equal masked value inside a record, in order, as
    numpy arrays: a run starts at a record's first base and wherever the masked value differs from its left neighbour's."""
    v = np.asarray(values).astype(np.uint64) & np.uint64(mask)
    lens = np.asarray(rec_lens, np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    assert roff[-1] == v.size
    start = np.zeros(v.size, bool)
    start[1:] = v[1:] != v[:-1]
    start[roff[:-1][lens > 0]] = True
    st = np.flatnonzero(start)
    en = np.r_[st[1:], v.size]
    rec = np.searchsorted(roff, st, side="right") - 1
    return st, en, rec, v[st], roff


def lines_of(values, mask, rec_lens, names):
    """The lines as a list of bytes, and each line's global start."""
    st, en, rec, val, roff = runs(values, mask, rec_lens)
    nm = [n if isinstance(n, bytes) else n.encode() for n in names]
    out = [b"%s\t%d\t%d\t%d\n" % (nm[r], s - roff[r], e - roff[r], x) for s, e, r, x in zip(st.tolist(), en.tolist(), rec.tolist(), val.tolist())]
    return out, st


def bedgraph_text(values, mask, rec_lens, names):
    return b"".join(lines_of(values, mask, rec_lens, names)[0])


def tile_bytes(values, mask, rec_lens, names, T):
    """Bytes of text per tile of T entries: a line belongs to the tile its run starts in."""
    lines, st = lines_of(values, mask, rec_lens, names)
    nt = (len(np.asarray(values)) + T - 1) // T
    return np.bincount(st // T, weights=[len(ln) for ln in lines], minlength=nt).astype(np.int64)


def plan_slabs(tb, cap):
    """The slabs [(first tile, end tile, bytes)] a cap cuts the tiles into: a slab takes tiles while their text fits.  None: a tile's
    text alone exceeds the cap."""
    out, t0, cur = [], 0, 0
    for t, b in enumerate(int(x) for x in tb):
        if b > cap:
            return None
        if cur + b > cap:
            out.append((t0, t, cur)); t0, cur = t, 0
        cur += b
    if len(tb) > t0:
        out.append((t0, len(tb), cur))
    return out


def per_base_loop(values, mask, rec_lens, names):
    """The same text from a per-base Python loop (small arrays only)."""
    out, i = [], 0
    for r, n in enumerate(rec_lens):
        s = 0
        for k in range(n):
            last = k + 1 == n or (int(values[i + k + 1]) & mask) != (int(values[i + k]) & mask)
            if last:
                out.append("%s\t%d\t%d\t%d\n" % (names[r], s, k + 1, int(values[i + k]) & mask)); s = k + 1
        i += n
    return "".join(out).encode()


def parse(text):
    """[(name, per-base int64 array)] in order of appearance from bedGraph text; asserts the format's invariants: four columns, the
    lines of a record tile it from 0 without gaps, neighbouring lines of a record differ in value, a record appears once."""
    if isinstance(text, bytes):
        text = text.decode()
    assert text == "" or text.endswith("\n")
    cols = text.split("\n")[:-1]
    f = [ln.split("\t") for ln in cols]
    assert all(len(x) == 4 for x in f)
    names = np.array([x[0] for x in f], dtype=object)
    st, en, val = (np.array([int(x[k]) for x in f], np.int64) for k in (1, 2, 3))
    assert (en > st).all()
    first = np.r_[True, names[1:] != names[:-1]] if len(f) else np.zeros(0, bool)
    assert (st[first] == 0).all() and (st[~first] == en[:-1][~first[1:]]).all() and (val[1:][~first[1:]] != val[:-1][~first[1:]]).all()
    out, at = [], np.flatnonzero(first).tolist() + [len(f)]
    for a, b in zip(at[:-1], at[1:]):
        out.append((names[a], np.repeat(val[a:b], en[a:b] - st[a:b])))
    assert len({n for n, _ in out}) == len(out)
    return out


def weighted_length(text):
    """sum over the lines of (end - start) * value"""
    return sum(int(v.sum()) for _, v in parse(text))


# ---- the case table of scs_runs_probe: sizes x value families x record layouts
SIZES = ("1", "2", "T-1", "T", "T+1", "2T+1", "4T+3")
FAMILIES = ("equal", "alt", "tile_edge", "geom", "digits", "upper")
LAYOUTS = ("one", "ones", "mid", "edge", "many", "long")


def size_of(name, T):
    return {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "4T+3": 4 * T + 3}[name]


def _geom(rng, n, mean, draw):
    v = np.zeros(n, np.uint32); i = 0
    while i < n:
        k = int(rng.geometric(1.0 / mean)); v[i:i + k] = draw(); i += k
    return v


def values_of(fam, n, T, seed):
    """(values uint32[n], mask)"""
    rng = np.random.default_rng(seed)
    if fam == "equal":
        return np.full(n, 7, np.uint32), FULL
    if fam == "alt":
        return (np.arange(n) & 1).astype(np.uint32), FULL
    if fam == "tile_edge":                                  # a change exactly at a tile's last entry and at the next tile's first
        v = np.full(n, 5, np.uint32); v[T - 1:] = 6; v[T:] = 7; v[2 * T - 1:] = 8; v[2 * T:] = 9
        return v, FULL
    if fam == "geom":
        return _geom(rng, n, 40, lambda: rng.integers(0, 60)), FULL
    if fam == "digits":                                     # 1 .. 10 digits, 4294967295 among them
        edges = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, 4294967295]
        return _geom(rng, n, 2, lambda: edges[rng.integers(len(edges))]), FULL
    assert fam == "upper"                                   # under 0xFFFF: words that differ only in the upper half are one run
    low = _geom(rng, n, 30, lambda: rng.integers(0, 5))
    return (low | (rng.integers(0, 1 << 16, n).astype(np.uint32) << 16)).astype(np.uint32), LOW


def layout_of(lay, n, T):
    """(rec_lens, names)"""
    if lay == "ones":
        lens = [1] * n
    elif lay == "mid" and n >= 2:
        lens = [n // 2, n - n // 2] if n < T else [T // 2 + 3, n - T // 2 - 3]
    elif lay == "edge" and n > T:                           # a border at a tile edge: equal values on both sides must still be cut
        lens = [T, n - T]
    elif lay == "many" and n > 900:                         # 300 records, 299 of them inside the first tile
        lens = [1] * 100 + [3] * 100 + [5] * 99 + [n - 895]
    else:
        lens = [n]
    names = ["r%d" % i for i in range(len(lens))]
    if lay == "long":
        names[0] = LONG_NAME
    return lens, names


def table_cases():
    """Every size under every family with the layouts rotating, and the sizes T + 1 and 4T + 3 under all of them."""
    out, k = [], 0
    for s in SIZES:
        for f in FAMILIES:
            lays = LAYOUTS if s in ("T+1", "4T+3") else (LAYOUTS[k % len(LAYOUTS)],)
            k += 1
            out += [dict(size=s, fam=f, lay=lay) for lay in lays]
    return out


def name_of(spec):
    return "%s-%s-%s" % (spec["size"], spec["fam"], spec["lay"])


def case(spec, T):
    """(values, mask, rec_lens, names)"""
    n = size_of(spec["size"], T)
    v, mask = values_of(spec["fam"], n, T, sum(map(ord, name_of(spec))))
    lens, names = layout_of(spec["lay"], n, T)
    return v, mask, lens, names


def slab_case(T):
    """Six tiles: one run over tiles 0 .. 2 and five entries of tile 3 (tiles 1 and 2 hold no run start), then every base a new
    run, tile 3 with the longest values.  (values, mask, rec_lens, names)"""
    n = 6 * T
    v = (np.arange(n) & 1).astype(np.uint32) + 1
    v[3 * T:4 * T] += 1000000                                # (tile 3's text is the largest: a cap of that size cuts in front of it)
    v[:3 * T + 5] = 0
    return v, FULL, [n], ["chr1"]
