"""The case table of the read allocation's kernels (scs_k_allocate.hip) and of its host plan (scs_alloc_plan.h), shared by
tests/test_alloc_host.py (which proves on the CPU that the table reaches the branches named here) and tests/test_gpu_alloc.py /
tests/alloc_gpu_worker.py (which run every case on the GPU and compare it with the oracle's rule).

THE CONTRACT on the weights: finite, not negative, and summing to at least 1e-3 over the whole job.  All-zero or denormal-scale
totals are out of contract: the library cannot produce them (a GC weight is a length over frag_size^2 times a factor around 1), and
there the leftover after the per-chunk quotas is no longer below the chunk count, which is what k_alloc_top_draws' nch + 1024 threads
rely on.  Every case here is inside the contract, and test_alloc_host.py checks 0 <= leftover < nch + 1024 on the oracle's own
numbers for every one of them, so that no case leaves it silently.

Sums and scans (SUM_SIZES x SUM_FAMILIES): what each size reaches in launch_tree_sum / k_tree1000 and scan_all_dev / k_scan1000 /
k_scan_fix
  1                   the memcpy of launch_tree_sum; one row of one entry
  2                   the smallest k_tree1000 launch
  63, 64, 65          a row of the scan short by one, full, and one entry into the second row (the carry)
  127, 128            two rows, the second short by one / full
  999, 1000, 1001     one group short by one, full, and a second group of one entry (k_scan_fix, one level above)
  1999, 2000, 2001    the same one group later (pre[0] and pre[1])
  64 000              64 groups: the level above is one row of the scan
  999 999 .. 1 000 001  1000 groups, full and short, and group 1001: a THIRD level of both the tree and the scan
  1 001 001           1002 groups whose level above has a second group of two
  families: uniform, logu (12 decades), equal, spike (one entry 10^12 times the rest), zerorun (zeros over one whole group of 1000;
  below 1001 entries over the middle half)

One shard (ONE_SIZES x families x reads x SE/PE): ac = 1 (a chunk of one entry), 63/64/65, 999/1000/1001 (a last chunk of one
entry), 1999/2000/2001, 4095/4096/4097 and 8191/8192 (ac + 1 on both sides of the parity scan's tiles of 4096), 64 000 and 1 000 001
(1001 chunks: the two-level scan_all_dev and launch_tree_sum inside the allocation).  Families: uniform (rand + 1e-3), logu
(10^U(-12, 0)), equal (ties in every CDF), dominant (1e-6 rand, one entry 1.0 in the middle: quotas above 1024 and, at 1 000 001,
above 100 000 on one chunk), halfzero (every second entry 0), zerochunk0 (the first 1000 entries 0: a chunk with tp = 0 and no quota;
only for ac > 1000).  reads: 1, 7, ac / 3 + 1, 3 ac + 5, 50 ac; at ac = 1 000 001 the two middle ones over three families.

Shard layouts (LAYOUTS): lists of (slot, rank, count) in the whole job's list order; what each reaches is said at its definition."""
import functools

import numpy as np

SEED = 20240611                                    # the allocation's Philox seed in every case
CHUNK = 1000
SLOTS = 40

# ---------------------------------------------------------------- sums and scans
SUM_SIZES = (1, 2, 63, 64, 65, 127, 128, 999, 1000, 1001, 1999, 2000, 2001, 64000, 999999, 1000000, 1000001, 1001001)
SUM_FAMILIES = ("uniform", "logu", "equal", "spike", "zerorun")


@functools.lru_cache(maxsize=8)
def sum_values(family, n):
    rng = np.random.default_rng([11, SUM_FAMILIES.index(family), n])
    if family == "uniform":
        return rng.random(n)
    if family == "logu":
        return 10.0 ** rng.uniform(-12.0, 0.0, n)
    if family == "equal":
        return np.full(n, 0.1)
    v = rng.random(n) + 1e-3
    if family == "spike":
        v[n // 2] *= 1e12
        return v
    assert family == "zerorun"
    if n > CHUNK:
        g = ((n + CHUNK - 1) // CHUNK) // 2
        v[g * CHUNK:(g + 1) * CHUNK] = 0.0
    else:
        v[n // 4:max(n // 4, 3 * n // 4)] = 0.0
    return v


# ---------------------------------------------------------------- the whole allocation, one shard
ONE_SIZES = (1, 2, 63, 64, 65, 999, 1000, 1001, 1999, 2000, 2001, 4095, 4096, 4097, 8191, 8192, 64000, 1000001)
ONE_FAMILIES = ("uniform", "logu", "equal", "dominant", "halfzero", "zerochunk0")
BIG = 1000001
BIG_FAMILIES = ("uniform", "dominant", "zerochunk0")


@functools.lru_cache(maxsize=8)
def weights(family, ac, seed=0):
    """the family's vector of ac weights: the first of its seeded draws that is inside the contract (only logu at one or two amplicons
    ever needs a second one)"""
    for attempt in range(64):
        w = _draw(family, ac, np.random.default_rng([23, ONE_FAMILIES.index(family), ac, seed, attempt]))
        if w.sum() >= 1e-3:
            return w
    raise AssertionError("no draw of %s at %d inside the contract" % (family, ac))


def _draw(family, ac, rng):
    if family == "uniform":
        return rng.random(ac) + 1e-3
    if family == "logu":
        return 10.0 ** rng.uniform(-12.0, 0.0, ac)
    if family == "equal":
        return np.full(ac, 0.37)
    if family == "dominant":
        w = 1e-6 * rng.random(ac)
        w[ac // 2] = 1.0
        return w
    w = rng.random(ac) + 1e-3
    if family == "halfzero":
        w[(1 if ac > 1 else 2)::2] = 0.0                                 # (a single amplicon keeps its weight: the contract)
        return w
    assert family == "zerochunk0" and ac > CHUNK
    w[:CHUNK] = 0.0
    return w


def reads_of(ac):
    return (ac // 3 + 1, 3 * ac + 5) if ac == BIG else (1, 7, ac // 3 + 1, 3 * ac + 5, 50 * ac)


def one_cases(ac):
    """(family, reads, paired) of every one-shard case of `ac` amplicons"""
    fams = BIG_FAMILIES if ac == BIG else [f for f in ONE_FAMILIES if f != "zerochunk0" or ac > CHUNK]
    return [(f, r, p) for f in fams for r in reads_of(ac) for p in (0, 1)]


def one_key(ac, family, reads, paired):
    return "%d.%s.%d.%s" % (ac, family, reads, "PE" if paired else "SE")


# ---------------------------------------------------------------- shard layouts
def _random4():
    rng = np.random.default_rng(404)
    out = []
    for slot in range(SLOTS):
        for rank in range(4):
            n = int(np.exp(rng.uniform(0.0, np.log(30000.0))))
            if rng.random() >= 0.3:
                out.append((slot, rank, max(1, n)))
    return out


def _crumbs():
    rng = np.random.default_rng(120)
    return [(slot, rank, int(rng.integers(1, 8))) for slot in range(SLOTS) for rank in range(3)]


# name -> (shards, [(slot, rank, count) in list order: slot ascending, rank ascending inside a slot])
LAYOUTS = {
    # every segment a multiple of 1000: no boundary row at all, three ranges per rank
    "aligned": (2, [(0, 0, 2000), (0, 1, 1000), (1, 0, 3000), (2, 1, 2000), (3, 0, 1000), (3, 1, 4000)]),
    # all 120 cells hold 1..7 amplicons: ONE chunk of the job, shared by three shards, 120 segments in it
    "crumbs": (3, _crumbs()),
    # chunk 1 = [1000, 2000) holds the tail of rank 0's 1500 (read by the others' rows at j >= 1000 of a segment between 1000 and 2000),
    # rank 1's 300, rank 2's 1 and rank 0's 199; chunk 4 holds the tail of rank 1's 2500 (j >= 2000 of a segment above 2000) in rank 2's
    # row; chunk 8 the tail of rank 2's 2600 in rank 0's row; a last chunk of 501 shared by ranks 0 and 1
    "straddle": (3, [(0, 0, 1500), (0, 1, 300), (0, 2, 1), (1, 0, 199), (1, 1, 2500), (1, 2, 999), (2, 0, 1), (2, 2, 2600), (3, 0, 1400), (3, 1, 1)]),
    # rank 1 holds no amplicon
    "empty_rank": (3, [(0, 0, 1200), (0, 2, 700), (1, 0, 50), (1, 2, 2300), (2, 0, 1000), (5, 2, 333)]),
    # rank 1 is empty in slots 1..3 (and rank 0's slot 4 follows at once): rank 0's four segments there are contiguous in the whole
    # list, one run [1150, 3894) that is not chunk-aligned -- one interior chunk between two boundary chunks
    "merge": (2, [(0, 0, 700), (0, 1, 450), (1, 0, 600), (2, 0, 900), (3, 0, 1234), (4, 0, 10), (4, 1, 1500)]),
    # 8345 amplicons, the last segment longer than a chunk: the partial last chunk (345) is interior to rank 1 and read in place
    "tail_in_place": (2, [(0, 0, 1000), (0, 1, 2000), (1, 0, 3000), (1, 1, 2345)]),
    # 4377 amplicons: the partial last chunk [4000, 4377) holds rank 1's tail, rank 0's 100 and rank 1's 77
    "tail_boundary": (2, [(0, 0, 2500), (0, 1, 1700), (1, 0, 100), (1, 1, 77)]),
    # seeded: counts log-uniform in 1..30 000 over the 160 cells, 30 % of them empty
    "random4": (4, _random4()),
}
LAYOUT_FAMILIES = ("uniform", "dominant")
# which collectives each layout runs under on the GPU
LAYOUT_HOOKS = {"aligned": ("host",), "crumbs": ("device",), "straddle": ("host", "device"), "empty_rank": ("host",), "merge": ("device",),
                "tail_in_place": ("host",), "tail_boundary": ("device",), "random4": ("host", "device")}


def layout_counts(name):
    """the table [R][40] the shards all-reduce"""
    R, segs = LAYOUTS[name]
    c = np.zeros((R, SLOTS), np.uint64)
    for slot, rank, n in segs:
        assert 0 <= slot < SLOTS and 0 <= rank < R and n > 0 and c[rank, slot] == 0
        c[rank, slot] = n
    assert segs == sorted(segs, key=lambda s: (s[0], s[1])), "a layout is stated in list order"
    return c


def layout_total(name):
    return sum(n for _, _, n in LAYOUTS[name][1])


def layout_runs(name):
    """(family, reads, paired) of the layout's four runs"""
    t = layout_total(name)
    return [(f, r, p) for f in LAYOUT_FAMILIES for r, p in ((3 * t + 5, 1), (t // 3 + 1, 0))]


def layout_weights(name, family):
    """the whole job's weights in list order"""
    return weights(family, layout_total(name), seed=1 + list(LAYOUTS).index(name))


def layout_slices(name):
    """per rank: the (start, stop) pieces of the whole-job list that are the rank's local list, in local (= list) order"""
    R, segs = LAYOUTS[name]
    out, at = [[] for _ in range(R)], 0
    for _, rank, n in segs:
        out[rank].append((at, at + n))
        at += n
    return out


def local_weights(name, family, rank):
    w = layout_weights(name, family)
    pieces = [w[a:b] for a, b in layout_slices(name)[rank]]
    return np.concatenate(pieces) if pieces else np.zeros(0)


def layout_key(name, hooks, family, reads, paired, rank):
    return "%s.%s.%s.%d.%s.r%d" % (name, hooks, family, reads, "PE" if paired else "SE", rank)


# ---------------------------------------------------------------- the oracle's rule (oracle/scs_oracle.cpp: tree_sum, scan_all, allocate_reads)
def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def oracle_tree_sum(lib, v):
    import ctypes as C
    v, out = _f64(v), C.c_double()
    lib.scso_tree_sum.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_double)]
    assert lib.scso_tree_sum(v.ctypes.data, v.size, C.byref(out)) == 0
    return out.value


def oracle_scan_all(lib, v):
    import ctypes as C
    v = _f64(v)
    out = np.empty(v.size, np.float64)
    lib.scso_scan_all.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    assert lib.scso_scan_all(v.ctypes.data, v.size, out.ctypes.data) == 0
    return out


def oracle_allocate(lib, w, reads, paired, threads=8):
    """(read numbers, diag): diag = dict(total, residual, leftover, quota[nch]) of scso_allocate_reads' diag_out"""
    import ctypes as C
    w = _f64(w)
    nch = (w.size + CHUNK - 1) // CHUNK
    rn, diag = np.empty(w.size, np.uint32), np.zeros(4 + nch, np.uint64)
    lib.scso_allocate_reads.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.scso_last_error.restype = C.c_char_p
    rc = lib.scso_allocate_reads(w.ctypes.data, w.size, int(reads), int(paired), SEED, threads, rn.ctypes.data, diag.ctypes.data)
    assert rc == 0, lib.scso_last_error()
    assert int(diag[3]) == nch
    return rn, dict(total=float(diag[:1].view(np.float64)[0]), residual=int(diag[1]), leftover=int(np.int64(diag[2])), quota=diag[4:].astype(np.int64))


def pair_offsets(rn, paired):
    """pair_off[n + 1]: the exclusive cumulative sum of rn (SE) or of ceil(rn / 2) (PE: rn / 2 after the parity fix), mod 2^32"""
    per = (rn.astype(np.uint64) + 1) // 2 if paired else rn.astype(np.uint64)
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint64).astype(np.uint32)
