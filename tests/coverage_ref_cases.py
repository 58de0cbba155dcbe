"""The coverage profile on the reference (scs_set_coverage_ref) restated in plain numpy, shared by tests/test_coverage_ref_host.py
and tests/test_gpu_coverage_ref.py: every staged base's reference index through the segment arrays, the reference depths and
copies by np.add.at, the classes and tables, the file; and the case table of the kernels' probe
(scs_coverage_ref_finish_probe).  Nothing here is shared with the library.  Not collected."""
import numpy as np

CN = 16                                                     # depth by copy number 0 .. CN, the last one copies >= CN
LDS = 4096                                                  # the largest LDS histogram of the count kernel
LAYOUTS = ["identity", "two_haps", "tandem3x8", "tandem_tile_x3", "back_jump", "ins_first", "ins_mid", "ins_last", "ins_record", "cn0_tile", "cn0_record",
           "borders", "one_base_segs", "second_ref_record"]
SIZES = ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "2T+1"]
NS = ["none", "all", "blocks", "mixed"]
FAMILIES = ["zeros", "ones", "small", "pile", "eight_copies"]


# ---- the restatement

def lift_index(seg, ref_lens):
    """Per staged base its global reference index (the reference records concatenated), -1 under an I segment.  seg: (hap_off,
    len, ref_pos, ref_rec, kind) arrays of segments that tile the staged genome."""
    hap_off, ln, ref_pos, ref_rec, kind = (np.asarray(v, np.int64) for v in seg)
    assert hap_off[0] == 0 and (hap_off[1:] == hap_off[:-1] + ln[:-1]).all() and (ln > 0).all()
    roff = np.concatenate([[0], np.cumsum(np.asarray(ref_lens, np.int64))])
    si = np.repeat(np.arange(len(ln)), ln)
    within = np.arange(int(ln.sum())) - hap_off[si]
    return np.where(kind[si] == 0, roff[ref_rec[si]] + ref_pos[si] + within, -1)


def lift_arrays(depth, codes, seg, ref_lens):
    """(ref_depth, copies, n_copies as int64 per reference base, unlifted) by np.add.at through the segment arrays."""
    depth, codes = np.asarray(depth, np.int64), np.asarray(codes)
    idx = lift_index(seg, ref_lens)
    assert idx.size == depth.size == codes.size
    R, at = int(np.sum(np.asarray(ref_lens, np.int64))), idx >= 0
    ref_depth, copies, n_copies = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    np.add.at(ref_depth, idx[at], depth[at])
    np.add.at(copies, idx[at], 1)
    np.add.at(n_copies, idx[at], (codes[at] >= 4).astype(np.int64))
    return ref_depth, copies, n_copies, int(depth[~at].sum())


def tables(ref_depth, copies, n_copies, ref_lens, D):
    """The tables per reference record: N = copies > 0 and every copy N (in no bucket); absent = copies 0 (in bucket 0); a base with
    mixed copies counts as sequence."""
    off = np.concatenate([[0], np.cumsum(np.asarray(ref_lens, np.int64))])
    nf = len(ref_lens)
    t = dict(hist=np.zeros((nf, D + 1), np.uint64), n_bases=np.zeros(nf, np.uint64), absent=np.zeros(nf, np.uint64), sum=np.zeros(nf, np.uint64), sum_n=np.zeros(nf, np.uint64),
             cn_bases=np.zeros((nf, CN + 1), np.uint64), cn_sum=np.zeros((nf, CN + 1), np.uint64))
    for r in range(nf):
        d, c, n = (v[off[r]:off[r + 1]] for v in (ref_depth, copies, n_copies))
        is_n = (c > 0) & (n == c)
        cnt = ~is_n
        t["hist"][r] = np.bincount(np.minimum(d[cnt], D), minlength=D + 1)
        t["n_bases"][r], t["absent"][r], t["sum"][r], t["sum_n"][r] = int(is_n.sum()), int((c == 0).sum()), int(d[cnt].sum()), int(d[is_n].sum())
        cn = np.minimum(c[cnt], CN)
        t["cn_bases"][r] = np.bincount(cn, minlength=CN + 1)
        s = np.zeros(CN + 1, np.int64)
        np.add.at(s, cn, d[cnt])
        t["cn_sum"][r] = s
    return t


def with_genome_row(t):
    return {k: np.concatenate([v, v.sum(axis=0, keepdims=True)]).astype(np.uint64) for k, v in t.items()}


def reference(depth, codes, seg, ref_lens, D):
    """Everything the probe returns, from the restatement."""
    ref_depth, copies, n_copies, unlifted = lift_arrays(depth, codes, seg, ref_lens)
    t = tables(ref_depth, copies, n_copies, ref_lens, D)
    t.update(ref_depth=ref_depth.astype(np.uint32), packed=(copies | (n_copies << 16)).astype(np.uint32), unlifted=unlifted)
    return t


def bin_sums(per_base, ref_lens, w):
    """The per-base array summed over the reference records' bins of w bases (scs_set_depth_ref's layout, without the pseudo-bin)."""
    off = np.concatenate([[0], np.cumsum(np.asarray(ref_lens, np.int64))])
    return np.concatenate([np.add.reduceat(per_base[off[r]:off[r + 1]], np.arange(0, off[r + 1] - off[r], w)) for r in range(len(ref_lens))]).astype(np.uint64)


# ---- the file

def parse_file(path):
    """dict(D=, summary=[(record, [bases, n_bases, absent, aligned] + six floats)], cn=[(record, copies, bases, aligned, mean)],
    unlifted=(aligned bases, inserted bases), rows=[(record, depth, count, size, fraction)]) of scs_write_coverage_ref's text."""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("#coverage\tmax_depth=") and ">=" in lines[0]
    out = dict(D=int(lines[0].split("\t")[1].split("=")[1]), summary=[], cn=[])
    assert lines[1] == "#summary\trecord\tbases\tn_bases\tabsent\taligned\tmean\tbreadth1\tbreadth5\tbreadth10\tbreadth20\tgini"
    i = 2
    while lines[i].startswith("#s\t"):
        f = lines[i].split("\t")
        out["summary"].append((f[1], [int(v) for v in f[2:6]] + [float(v) for v in f[6:]]))
        i += 1
    assert lines[i] == "#cn\trecord\tcopies\tbases\taligned\tmean"
    i += 1
    while lines[i].startswith("#c\t"):
        f = lines[i].split("\t")
        out["cn"].append((f[1], int(f[2]), int(f[3]), int(f[4]), float(f[5])))
        i += 1
    f = lines[i].split("\t")
    assert f[0] == "#unlifted" and len(f) == 3 and lines[i + 1] == "#record\tdepth\tcount\tsize\tfraction"
    out["unlifted"] = (int(f[1]), int(f[2]))
    out["rows"] = [(g[0], int(g[1]), int(g[2]), int(g[3]), float(g[4])) for g in (ln.split("\t") for ln in lines[i + 2:-1])]
    return out


def render_counts(names, t):
    """The integer columns the file must hold, from downloaded tables (reference records + 1 rows, the genome's last)."""
    summ, cn, rows = [], [], []
    for r, name in enumerate(list(names) + ["genome"]):
        h = t["hist"][r].astype(np.int64)
        size = int(h.sum())
        summ.append((name, [size + int(t["n_bases"][r]), int(t["n_bases"][r]), int(t["absent"][r]), int(t["sum"][r]) + int(t["sum_n"][r])]))
        cn += [(name, c, int(t["cn_bases"][r][c]), int(t["cn_sum"][r][c])) for c in range(CN + 1) if t["cn_bases"][r][c]]
        rows += [(name, k, int(h[k]), size) for k in range(len(h)) if h[k]]
    return summ, cn, rows


# ---- the case table of scs_coverage_ref_finish_probe.  spec: layout, size (the reference length by name: 1 .. 2T + 1), n (the N
# layout), fam (the staged depths), lds (buckets of the LDS histogram; -1: the product's)

def name_of(spec):
    return "%s-%s-%s-%s-lds%d" % (spec["layout"], spec["size"], spec["n"], spec["fam"], spec["lds"])


def _hash(name):
    h = 0
    for ch in name.encode():
        h = (h * 131 + ch) % 1000000007
    return h


def layout(kind, S, T):
    """(seg arrays, hap_lens, ref_lens) of a layout over a reference stretch of S bases (T: the tile).  R pieces are (ref_rec,
    ref_pos, len), I pieces (None, 0, len); `recs` lists the pieces of every staged record."""
    I = lambda n: (None, 0, n)
    h = S // 2
    if kind == "identity":
        ref, recs = [S], [[(0, 0, S)]]
    elif kind == "two_haps":                               # every reference base is added from two distant workgroups
        ref, recs = [S], [[(0, 0, S)], [(0, 0, S)]]
    elif kind in ("tandem3x8", "tandem_tile_x3"):          # a unit of 3 bases x 8 (collisions inside one wave), of T + 1 bases x 3 (across tiles)
        u, k = (min(3, S), 8) if kind == "tandem3x8" else (min(T + 1, S), 3)
        a = (S - u) // 2
        ref, recs = [S], [[(0, 0, a)] + [(0, a, u)] * k + [(0, a + u, S - a - u)]]
    elif kind == "back_jump":                              # the second half first
        ref, recs = [S], [[(0, h, S - h), (0, 0, h)]]
    elif kind == "ins_first":
        ref, recs = [S], [[I(5), (0, 0, S)]]
    elif kind == "ins_mid":
        ref, recs = [S], [[(0, 0, h), I(T + 1 if S > 64 else 5), (0, h, S - h)]]
    elif kind == "ins_last":
        ref, recs = [S], [[(0, 0, S), I(5)]]
    elif kind == "ins_record":                             # a whole staged record of inserted sequence
        ref, recs = [S], [[(0, 0, S)], [I(min(S, 70))], [(0, 0, S)]]
    elif kind == "cn0_tile":                               # the reference tile [T, 2 T) is lifted to by nothing
        ref, recs = [2 * T + S], [[(0, 0, T), (0, 2 * T, S)]]
    elif kind == "cn0_record":                             # ... and so is the whole second reference record of three
        ref, recs = [S, S, 7], [[(0, 0, S), (2, 0, 7)]]
    elif kind == "borders":                                # segment borders at T - 1, T, T + 1 on the staged and on the reference side
        ref, recs = [T + 1 + S], [[(0, 0, T - 1), (0, T, 1), (0, T - 1, 1), (0, T + 1, S)]]
    elif kind == "one_base_segs":                          # S segments of one base, each a backwards jump
        ref, recs = [S], [[(0, S - 1 - i, 1) for i in range(S)]]
    else:
        assert kind == "second_ref_record", kind           # a second reference record that starts inside a tile
        ref, recs = [37, S], [[(0, 0, 37), (1, 0, S)], [(1, 0, S)]]
    cols, hap_lens, at = [], [], 0
    for rec in recs:
        n0 = at
        for rr, rp, ln in rec:
            if ln:
                cols.append((at, ln, rp, rr if rr is not None else 0, 0 if rr is not None else 1))
                at += ln
        hap_lens.append(at - n0)
    seg = tuple(np.array([c[k] for c in cols], np.int64) for k in range(5))
    return seg, hap_lens, ref


def case(spec, T):
    """(depth uint32[G], codes uint8[G], seg, hap_lens, ref_lens, max_depth) of a case."""
    S = {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[spec["size"]]
    seg, hap_lens, ref_lens = layout(spec["layout"], S, T)
    G = int(sum(hap_lens))
    rng = np.random.default_rng(_hash(name_of(spec)) % (1 << 32))
    codes = rng.integers(0, 4, G).astype(np.uint8)
    if spec["n"] == "all":
        codes[:] = 4
    elif spec["n"] == "blocks":
        codes[:min(G, 2)] = 4
        for b in list(range(T, G, T)) + [int(x) for x in seg[0][1:][::max(1, len(seg[0]) // 50)]]:
            codes[max(0, b - 3):min(G, b + 5)] = 4
    elif spec["n"] == "mixed":                              # N in the first staged half only: in one of two copies where a base has two
        codes[:G // 2] = 4
    else:
        assert spec["n"] == "none", spec["n"]
    fam, D = spec["fam"], 50
    if fam == "zeros":
        depth = np.zeros(G, np.int64)
    elif fam == "ones":
        depth = np.ones(G, np.int64)
    elif fam == "small":                                   # mostly zeros, as a low-coverage job leaves them
        depth = rng.integers(0, 6, G) * (rng.random(G) < 0.4)
    elif fam == "pile":                                    # above D and above the LDS table; and between the two
        D = 5000
        depth = rng.integers(0, 4, G)
        depth[G // 2] = 70000
        depth[G // 3] = 4500
    else:
        assert fam == "eight_copies", fam                  # eight copies cross D together, each stays below it
        depth = np.full(G, D // 8 + 1, np.int64)
    return depth.astype(np.uint32), codes, seg, hap_lens, ref_lens, D


def table_cases(lds):
    """The probe's cases at one LDS size: every layout at every size, the N layouts and depth families rotating so that every pair
    of them meets several layouts; and four layouts at T + 1 under every pair."""
    out, k = [], 0
    for layout_name in LAYOUTS:
        for size in SIZES:
            out.append(dict(layout=layout_name, size=size, n=NS[k % 4], fam=FAMILIES[(k // 4) % 5], lds=lds))
            k += 1
    for layout_name in ("two_haps", "tandem3x8", "ins_mid", "second_ref_record"):
        for n in NS:
            for fam in FAMILIES:
                spec = dict(layout=layout_name, size="T+1", n=n, fam=fam, lds=lds)
                if spec not in out:
                    out.append(spec)
    return out


def seen(spec, T):
    """What a case reaches, for the tests to assert that the table puts its cases where it says."""
    depth, codes, seg, hap_lens, ref_lens, D = case(spec, T)
    want = reference(depth, codes, seg, ref_lens, D)
    copies, n_copies = (want["packed"] & 0xFFFF).astype(np.int64), (want["packed"] >> 16).astype(np.int64)
    idx = lift_index(seg, ref_lens)
    hap_off, ln, ref_pos, ref_rec, kind = seg
    roff = np.concatenate([[0], np.cumsum(ref_lens)])
    R = int(roff[-1])
    # two staged bases of one aligned block of 64 that lift to one reference base: they collide inside one wave's atomic instruction
    wave = idx[:len(idx) // 64 * 64].reshape(-1, 64)
    collide = any(len(np.unique(w[w >= 0])) < (w >= 0).sum() for w in wave) if len(wave) else False
    absent = copies == 0
    tiles_absent = [bool(absent[t0:t0 + T].all()) for t0 in range(0, R - T + 1, T)]
    r_ends = (roff[ref_rec] + ref_pos + ln)[kind == 0]
    r_starts = (roff[ref_rec] + ref_pos)[kind == 0]
    staged_deep = np.zeros(R, np.int64)
    np.maximum.at(staged_deep, idx[idx >= 0], depth.astype(np.int64)[idx >= 0])
    return dict(max_copies=int(copies.max()), collide_in_wave=bool(collide), absent=int(absent.sum()), absent_tile=any(tiles_absent),
                absent_record=any(bool(absent[roff[r]:roff[r + 1]].all()) and roff[r + 1] > roff[r] for r in range(len(ref_lens))),
                mixed_n=int(((n_copies > 0) & (n_copies < copies)).sum()), all_n=int(((copies > 0) & (n_copies == copies)).sum()),
                back=int(((kind[1:] == 0) & (kind[:-1] == 0) & (ref_pos[1:] < ref_pos[:-1] + ln[:-1]) & (ref_rec[1:] == ref_rec[:-1])).sum()),
                inserted=int(ln[kind == 1].sum()), unlifted=int(want["unlifted"]), first_is_i=bool(kind[0] == 1), last_is_i=bool(kind[-1] == 1),
                i_record=any(any((hap_off[i] == sum(hap_lens[:r]) and ln[i] == hap_lens[r] and kind[i] == 1) for i in range(len(ln))) for r in range(len(hap_lens))),
                staged_borders=sorted(set(int(x) for x in hap_off[1:]) & {T - 1, T, T + 1}), ref_borders=sorted((set(int(x) for x in r_ends) | set(int(x) for x in r_starts)) & {T - 1, T, T + 1}),
                ref_record_starts_inside_tile=any(int(x) % T for x in roff[1:-1]), one_base_segs=int((ln == 1).sum()), staged_tiles=-(-len(idx) // T), ref_tiles=-(-R // T),
                max_depth_seen=int(want["ref_depth"].max()) if R else 0, top_bucket=int(want["hist"][:, D].sum()), D=D,
                sum_crosses_d=int(((want["ref_depth"] >= D) & (staged_deep < D) & (staged_deep > 0)).sum()), n_segs=len(ln), far_adders=bool(len(hap_lens) > 1 and copies.max() >= 2))
