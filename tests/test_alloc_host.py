"""CPU-only checks around the read allocation's kernels: the host plan (alloc_plan_build through scs_alloc_plan_probe) against brute
force written from the rule, the oracle's fixed-shape sums against exact references with bounds derived from their shapes, and the
proof that the case table of tests/alloc_cases.py reaches the branches it names -- so that tests/test_gpu_alloc.py compares the
kernels with the oracle where they can go wrong."""
import math

import numpy as np
import pytest

import alloc_cases as ac

import scssim_amd

CHUNK = ac.CHUNK
U = 2.0 ** -53


def gamma(k):
    """(1 + 2^-53)^k - 1, the relative error k roundings can add up to"""
    return math.expm1(k * math.log1p(U))


# ---------------------------------------------------------------- the plan against brute force
def _random_table(rng):
    """a counts table of 1..8 shards: cells empty, tiny, around a chunk, or a few chunks long, some of them whole chunks"""
    R = int(rng.integers(1, 9))
    kind = rng.integers(0, 6, (R, ac.SLOTS))
    c = np.zeros((R, ac.SLOTS), np.uint64)
    c[kind == 1] = rng.integers(1, 8, (R, ac.SLOTS))[kind == 1]
    c[kind == 2] = rng.integers(900, 1101, (R, ac.SLOTS))[kind == 2]
    c[kind == 3] = rng.integers(1, 6000, (R, ac.SLOTS))[kind == 3]
    c[kind == 4] = CHUNK * rng.integers(1, 4, (R, ac.SLOTS))[kind == 4]
    if rng.random() < 0.2:
        c[int(rng.integers(0, R))] = 0                                  # a shard with no amplicon
    if rng.random() < 0.2:
        c[:, int(rng.integers(0, ac.SLOTS)):] = 0                        # a short job
    return c


def _check_plans(counts, what):
    """the plans of all ranks of one table against the rule: the whole list takes the shards' segments slot by slot, shard by shard;
    a chunk of 1000 list entries that is wholly one shard's is read in place, every other chunk a shard has entries in is a boundary row"""
    R = counts.shape[0]
    total = int(counts.sum())
    nch = (total + CHUNK - 1) // CHUNK
    owner, local = np.zeros(total, np.int64), np.zeros(total, np.int64)
    segs, loff, at = [], [0] * R, 0                                      # brute force: every entry's shard and local index
    for slot in range(ac.SLOTS):
        for r in range(R):
            n = int(counts[r, slot])
            if n:
                owner[at:at + n], local[at:at + n] = r, np.arange(loff[r], loff[r] + n)
                segs.append((at, loff[r], n, r, slot))
            loff[r] += n
            at += n
    chunk_of = np.arange(total) // CHUNK
    chunk_len = np.bincount(chunk_of, minlength=nch)
    owners_of_chunk = np.zeros(nch, np.int64)                            # how many ranks own each chunk, and which
    owner_rank = np.full(nch, -1, np.int64)
    for me in range(R):
        p = scssim_amd.alloc_plan_probe(counts, me)
        assert (p["total"], p["nch"], p["ac"]) == (total, nch, int(counts[me].sum())), (what, me)
        assert p["scratch"] == nch // CHUNK * 3 + 4096
        # gseg: every non-empty segment in list order, tiling [0, total)
        g = p["gsegs"].astype(np.int64)
        assert [tuple(x) for x in g.tolist()] == segs, (what, me, "gseg")
        assert (len(g) == 0 and total == 0) or (g[0, 0] == 0 and (g[1:, 0] == g[:-1, 0] + g[:-1, 2]).all() and g[-1, 0] + g[-1, 2] == total)
        # my_seg: the rank's segment of every slot; order enumerates the list
        m = p["my_seg"].astype(np.int64)
        lo = 0
        for slot in range(ac.SLOTS):
            n = int(counts[me, slot])
            assert m[slot, 2] == n and m[slot, 1] == lo and m[slot, 3] == slot * R + me, (what, me, slot)
            assert m[slot, 0] == int(counts[:, :slot].sum()) + int(counts[:me, slot].sum()), (what, me, slot)
            lo += n
        # the work chunks
        mine = owner == me
        own_in_chunk = np.bincount(chunk_of[mine], minlength=nch) if total else np.zeros(0, np.int64)
        covered = np.zeros(total, np.int64)
        rng_, interior = p["ranges"].astype(np.int64), []
        assert len(rng_) == 0 or rng_[0, 0] == 0
        for k in range(len(rng_)):
            q0, c0, local0 = rng_[k]
            q1 = rng_[k + 1, 0] if k + 1 < len(rng_) else p["n_interior"]
            assert q1 > q0, (what, me, "an empty range")
            for q in range(q0, q1):
                c = c0 + (q - q0)
                a, b = c * CHUNK, min(total, (c + 1) * CHUNK)
                assert mine[a:b].all(), (what, me, "interior chunk %d holds another shard's amplicon" % c)
                assert (local[a:b] == local0 + (q - q0) * CHUNK + np.arange(b - a)).all(), (what, me, "local0 of chunk %d" % c)
                covered[a:b] += 1
                interior.append(c)
        b_ = p["bchunks"].astype(np.int64)
        for c, n, own in b_.tolist():
            a, b = c * CHUNK, min(total, (c + 1) * CHUNK)
            assert n == b - a and own == int(owner[a] == me), (what, me, "boundary chunk %d" % c)
            covered[a:b] += 1
        assert (covered[mine] == 1).all(), (what, me, "an own amplicon in no work chunk, or in two")
        # a chunk is interior exactly when it is wholly this shard's, a boundary row when it is partly; nothing else is worked on
        assert sorted(interior) == np.flatnonzero((own_in_chunk == chunk_len) & (chunk_len > 0)).tolist(), (what, me, "interior set")
        assert sorted(b_[:, 0].tolist()) == np.flatnonzero((own_in_chunk > 0) & (own_in_chunk < chunk_len)).tolist(), (what, me, "boundary set")
        assert p["n_interior"] + p["n_boundary"] == int((own_in_chunk > 0).sum()), (what, me)
        # every maximal run of own entries in the whole list has at most two boundary chunks
        if mine.any():
            edge = np.diff(np.concatenate([[0], mine.astype(np.int8), [0]]))
            for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
                touched = set(range(a // CHUNK, (b - 1) // CHUNK + 1)) & set(b_[:, 0].tolist())
                assert len(touched) <= 2, (what, me, "run [%d, %d) has boundary chunks %s" % (a, b, sorted(touched)))
        for c in interior:
            owners_of_chunk[c] += 1; owner_rank[c] = me
        for c, n, own in b_.tolist():
            if own:
                owners_of_chunk[c] += 1; owner_rank[c] = me
    assert (owners_of_chunk == 1).all(), (what, "a chunk with %s owners" % owners_of_chunk[owners_of_chunk != 1][:3])
    assert total == 0 or (owner_rank == owner[np.arange(nch) * CHUNK]).all(), (what, "the owner holds the chunk's first amplicon")


@pytest.mark.parametrize("name", list(ac.LAYOUTS))
def test_plan_of_every_layout_against_brute_force(name):
    _check_plans(ac.layout_counts(name), name)


def test_plan_of_random_tables_against_brute_force():
    rng = np.random.default_rng(2718)
    for i in range(300):
        _check_plans(_random_table(rng), "random table %d" % i)
    one = np.zeros((1, ac.SLOTS), np.uint64)
    _check_plans(one, "an empty job")
    one[0, 7] = 1
    _check_plans(one, "one amplicon")


# ---------------------------------------------------------------- the oracle's sums against exact references
def _levels(n):
    k = 0
    while True:
        n, k = (n + CHUNK - 1) // CHUNK, k + 1
        if n <= 1:
            return k


def _scan_path(n):
    """additions between an input and an output of scan_all: 6 of the row's Hillis-Steele scan, at most 15 of the carry from row to
    row and the one that adds the carry; with more than one group, the scan over the groups' last entries and the fix-up's one"""
    ng = (n + CHUNK - 1) // CHUNK
    return 22 if ng <= 1 else 22 + _scan_path(ng) + 1


@pytest.mark.parametrize("n", ac.SUM_SIZES)
def test_oracle_tree_sum_is_the_exact_sum_within_its_shape(n, oracle_lib):
    """scso_tree_sum against math.fsum.  A value passes through at most 16 additions of its lane's accumulator and 6 of the butterfly
    per level, over ceil(log_1000 n) levels: k additions of relative error 2^-53 each are off by at most ((1 + 2^-53)^k - 1) sum|v|
    (the exact sum's own rounding is one more)."""
    k = 22 * _levels(n) + 1
    assert _levels(n) == (1 if n <= 1000 else 2 if n <= 1000000 else 3)
    for fam in ac.SUM_FAMILIES:
        v = ac.sum_values(fam, n)
        got, want = ac.oracle_tree_sum(oracle_lib, v), math.fsum(v.tolist())
        bound = gamma(k) * math.fsum(np.abs(v).tolist())
        print("%s %d: off by %.3g, bound %.3g" % (fam, n, abs(got - want), bound))
        assert abs(got - want) <= bound, (fam, n, got, want, bound)


@pytest.mark.parametrize("n", ac.SUM_SIZES)
def test_oracle_scan_all_is_the_exact_scan_within_its_shape(n, oracle_lib):
    """scso_scan_all against numpy.cumsum in longdouble, taken inside groups of 1000 and over the groups' sums (at most 2200
    longdouble additions on the way to any entry: the reference's own error).  Entry i of the scan is off by at most
    ((1 + 2^-53)^path - 1) sum(|v[..i]|), path = the additions of _scan_path."""
    path = _scan_path(n)
    assert path == (22 if n <= 1000 else 45 if n <= 1000000 else 68)
    ref_err = 2200 * float(np.finfo(np.longdouble).eps) / 2
    for fam in ac.SUM_FAMILIES:
        v = ac.sum_values(fam, n)
        got = ac.oracle_scan_all(oracle_lib, v)
        pad = np.zeros((n + CHUNK - 1) // CHUNK * CHUNK, np.longdouble)
        pad[:n] = v
        rows = np.cumsum(pad.reshape(-1, CHUNK), axis=1, dtype=np.longdouble)
        before = np.concatenate([[np.longdouble(0)], np.cumsum(rows[:-1, -1], dtype=np.longdouble)])
        want = (rows + before[:, None]).reshape(-1)[:n]
        bound = (gamma(path) + ref_err) * want.astype(np.float64) * (1 + 2 * U)
        off = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        worst = int(np.argmax(off - bound))
        print("%s %d: worst entry %d off by %.3g, bound %.3g" % (fam, n, worst, off[worst], bound[worst]))
        assert (off <= bound).all(), (fam, n, worst, got[worst], want[worst], bound[worst])
        assert got[0] == v[0]


# ---------------------------------------------------------------- the table reaches what it names
@pytest.fixture(scope="module")
def diags(oracle_lib):
    """(ac, family, reads) -> (the read numbers BEFORE the parity fix, the oracle's diag): the SE run of every one-shard case; a PE case
    has the same weights, floors, quotas and draws, and only the parity fix behind them"""
    out = {}
    for n in ac.ONE_SIZES:
        for fam, reads, paired in ac.one_cases(n):
            if not paired:
                out[n, fam, reads] = ac.oracle_allocate(oracle_lib, ac.weights(fam, n), reads, 0)
    return out


def test_every_case_is_inside_the_contract_and_under_the_leftover_cap(diags, oracle_lib):
    """weights finite, not negative, summing to at least 1e-3; 0 <= leftover < nch + 1024 (the threads k_alloc_top_draws launches) on
    the oracle's diag for every one-shard case -- SE and PE share it -- and every layout run"""
    worst = 0
    for (n, fam, reads), (rn, d) in diags.items():
        w = ac.weights(fam, n)
        nch = (n + CHUNK - 1) // CHUNK
        assert np.isfinite(w).all() and (w >= 0).all() and w.sum() >= 1e-3 and d["total"] >= 1e-3, (n, fam)
        assert 0 <= d["leftover"] < nch + 1024, (n, fam, reads, d["leftover"])
        assert d["residual"] == reads - int((w / (2.2204e-16 + d["total"]) * reads).astype(np.uint64).sum()) and int(d["quota"].sum()) + d["leftover"] == d["residual"]
        assert int(rn.astype(np.uint64).sum()) == reads
        worst = max(worst, d["leftover"])
    for name in ac.LAYOUTS:
        for fam, reads, paired in ac.layout_runs(name):
            w = ac.layout_weights(name, fam)
            _, d = ac.oracle_allocate(oracle_lib, w, reads, paired)
            assert np.isfinite(w).all() and (w >= 0).all() and w.sum() >= 1e-3
            assert 0 <= d["leftover"] < (w.size + CHUNK - 1) // CHUNK + 1024, (name, fam, reads, d["leftover"])
    print("largest leftover: %d" % worst)
    assert {f for (_, f, _) in diags} == set(ac.ONE_FAMILIES) and {n for (n, _, _) in diags} == set(ac.ONE_SIZES)


def test_the_table_reaches_the_sampling_branches_it_names(diags):
    big = [(k, d) for k, (_, d) in diags.items() if k[0] >= 1000001]
    assert any(d["leftover"] > 0 for _, d in big), "no case with top draws over 1001 chunks or more (the two-level scan under first_le)"
    assert len(big) >= 6 and all(len(d["quota"]) >= 1001 for _, d in big)
    quotas = [d["quota"] for _, d in diags.values()]
    assert any((q > 1024).any() for q in quotas), "no chunk quota above 1024: the draw loop never makes a second trip"
    assert any((q % 4 != 0).any() for q in quotas), "no chunk quota that is not a multiple of 4"
    assert any((q > 100000).any() for q in quotas), "no chunk quota above 100 000"
    assert any((q[:1] == 0).all() and q.sum() > 0 for (n, f, _), (_, d) in diags.items() for q in [d["quota"]] if f == "zerochunk0"), "no chunk without a quota beside chunks with one"
    # a chunk of a single entry that draws (its quota may come from the leftover's draws): the entry ends above its floor
    def last_floor(n, fam, reads, d):
        return int(ac.weights(fam, n)[-1] / (2.2204e-16 + d["total"]) * reads)
    assert any(n % CHUNK == 1 and rn[-1] > last_floor(n, fam, reads, d) for (n, fam, reads), (rn, d) in diags.items()), "no chunk of one entry that draws"
    assert any(n > CHUNK and n % CHUNK == 1 for (n, _, _) in diags), "no last chunk of one entry behind full ones"
    assert {1, 63, 64, 65} <= {n for (n, _, _) in diags} and {999, 1000, 1001} <= {n for (n, _, _) in diags}
    # ties in a chunk's CDF: equal weights, and zero entries (a CDF step of zero width must never be drawn)
    for (n, fam, reads), (rn, _) in diags.items():
        if fam == "halfzero" and n > 1:
            assert not rn[1::2].any(), (n, reads, "a zero weight got a read")
        if fam == "zerochunk0":
            assert not rn[:CHUNK].any(), (n, reads, "a zero weight got a read")


def test_pe_cases_have_odd_read_numbers_on_both_sides_of_the_parity_scans_tile(diags):
    """the parity scan works in tiles of 4096 entries: before the fix, odd read numbers (the ones it changes, alternately + 1 and - 1)
    lie below and above entry 4096, so the count carried from tile to tile matters"""
    for n in (8191, 8192, 64000, 1000001):
        both = [k for k, (rn, _) in diags.items() if k[0] == n and (rn[:4096] & 1).any() and (rn[4097:] & 1).any()]
        assert len(both) >= 4, (n, both)
    for n in (4095, 4096, 4097):
        assert any((rn & 1).sum() >= 100 for k, (rn, _) in diags.items() if k[0] == n)


def test_the_layouts_reach_the_plan_branches_they_name():
    plans = {name: [scssim_amd.alloc_plan_probe(ac.layout_counts(name), r) for r in range(ac.LAYOUTS[name][0])] for name in ac.LAYOUTS}

    def rows(name):
        """per boundary chunk of every rank: (rank, the gsegs that touch it as rows of go, lo, n, owner, slot)"""
        for r, p in enumerate(plans[name]):
            g = p["gsegs"].astype(np.int64)
            for c, n, _ in p["bchunks"].astype(np.int64).tolist():
                yield r, c, g[(g[:, 0] < c * CHUNK + n) & (g[:, 0] + g[:, 2] > c * CHUNK)]

    def foreign_tail(name, lo, hi):
        """a boundary row reads a foreign segment of lo <= n < hi entries at j >= 1000 (the `last 1000` half of k_alloc_bpack)"""
        return any(sg[3] != r and lo <= sg[2] < hi and min(sg[0] + sg[2], (c + 1) * CHUNK) - 1 - sg[0] >= CHUNK for r, c, t in rows(name) for sg in t.tolist())

    assert any(len(t) >= 3 and len(set(t[:, 3].tolist())) >= 3 for _, _, t in rows("straddle")), "straddle: no boundary chunk with segments of three shards"
    assert foreign_tail("straddle", 1001, 2000) and foreign_tail("straddle", 2001, 1 << 32)
    r, c, t = next(rows("crumbs"))
    assert plans["crumbs"][0]["nch"] == 1 and len(t) == 120 and all(p["n_boundary"] == 1 and p["n_interior"] == 0 for p in plans["crumbs"])
    assert all(p["n_boundary"] == 0 and p["n_ranges"] >= 2 for p in plans["aligned"])
    assert plans["empty_rank"][1]["ac"] == 0 and plans["empty_rank"][1]["n_interior"] + plans["empty_rank"][1]["n_boundary"] == 0
    m = plans["merge"][0]                                                # four segments, one run [1150, 3894): chunk 2 in place, chunks 1 and 3 as rows
    assert m["ranges"].tolist() == [[0, 2, 700 + 850]] and sorted(m["bchunks"][:, 0].tolist()) == [0, 1, 3] and m["n_interior"] == 1
    t = plans["tail_in_place"][1]                                        # the last range ends with the job's partial chunk
    assert t["total"] % CHUNK == 345 and t["n_boundary"] == 0 and t["ranges"][-1].tolist() == [2, 6, 2000] and t["n_interior"] == 5
    for p in plans["tail_boundary"]:
        assert p["total"] == 4377 and [4, 377] in p["bchunks"][:, :2].tolist()
    assert sum(p["n_boundary"] for p in plans["random4"]) >= 100 and sum(p["n_interior"] for p in plans["random4"]) >= 100
