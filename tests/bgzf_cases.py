"""The inputs the BGZF kernels are checked on, shared by the CPU test (tests/test_host_logic.py: every case reaches the branch
it names, under the host emulation) and the GPU test (tests/test_gpu_bgzf.py: the device's bytes against zlib and against the
emulation).  Every case comes from a fixed-seed numpy generator; `reach` names the branch of scs_bgzf.hip it is there for.

kinds of a block: "deflated" (one dynamic-Huffman block), "stored_incompressible" (cbytes >= n + 5), "stored_cap" (the deflate
data would exceed BGZF_LDS_OUT).  `kinds`: what every block of the case must be (a list: block by block); None: not pinned.

At the end: the sizes and inputs of the scan test (the scan makes the BGZF block offsets), shared by its child process and its checks."""
import functools

import numpy as np

BGZF_IN = 64512            # scs_bgzf.h
BGZF_LDS_OUT = 40960
CAP_WINDOW = 64            # the lds_cap cases lie within this many bytes of BGZF_LDS_OUT

SMALL_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 251, 252, 253)


def fastq_text(nbytes, seed):
    """FASTQ-like text: 8-digit names, 150 bases (A/C/G/T with a few N), 150 qualities with a triangular distribution."""
    rng = np.random.default_rng(seed)
    L, reclen = 150, 14 + 150 + 3 + 150 + 1
    nrec = nbytes // reclen + 1
    rec = np.empty((nrec, reclen), np.uint8)
    ids = 10000000 + np.arange(nrec, dtype=np.int64) * 7
    rec[:, 0] = ord("@")
    for d in range(8):
        rec[:, 1 + d] = 48 + (ids // 10 ** (7 - d)) % 10
    rec[:, 9:14] = np.frombuffer(b"#1/1\n", np.uint8)
    rec[:, 14:14 + L] = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=(nrec, L), p=[.3, .2, .2, .29, .01])]
    rec[:, 14 + L:17 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 17 + L:17 + 2 * L] = 33 + rng.choice(41, size=(nrec, L), p=np.arange(1, 42) / 861.0)
    rec[:, -1] = 10
    return rec.tobytes()[:nbytes]


def _uniform(nbytes, nsym, seed, first=32):
    return np.random.default_rng(seed).integers(first, first + nsym, nbytes, dtype=np.uint8).tobytes()


def _counts(counts, first, seed=None):
    """bytes(first + i) * counts[i], in symbol order, or shuffled when a seed is given"""
    a = np.repeat(np.arange(first, first + len(counts), dtype=np.uint8), counts)
    if seed is not None:
        np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def _fibonacci():
    # 1, 2, 3, 5, 8, ...: with the end-of-block symbol's 1 the only ties are at the bottom, so every merge hangs the next leaf
    # beside everything merged so far and the tree is as deep as the alphabet (20).  The host test's 1, 1, 2, 3, ... ties all the
    # way up, the two-queue merge takes the leaf first, and its tree is 12 deep: it never reached the repair.
    fib = [1, 2]
    while sum(fib) + fib[-1] + fib[-2] <= BGZF_IN:
        fib.append(fib[-1] + fib[-2])
    return _counts(fib, 65)


def skewed_counts(nsym):
    """every count one more than the sum of the two before it (1, 2, 4, 7, 12, 20, 33, ...): trees deeper than 17"""
    cnt = [1, 2]
    while len(cnt) < nsym:
        cnt.append(cnt[-1] + cnt[-2] + 1)
    return cnt


def _all_256_skewed():
    cnt = np.maximum(1, np.floor(6000 * 0.9 ** np.arange(256))).astype(np.int64)     # geometric, every value at least once
    assert cnt.sum() <= BGZF_IN
    return _counts(cnt, 0, seed=21)


def _ties_with_eob():
    # 200 literals once each -- the end-of-block symbol (256) has count 1 too and must rank behind all of them --, ten more with
    # 50 each (ties among themselves)
    return _counts([1] * 200 + [50] * 10, 0, seed=22)


def cap_mix(k64, seed):
    """one block: k64 bytes uniform over 64 symbols, the rest uniform over 32 of them, shuffled (about 5.08 bits per byte)"""
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.integers(32, 96, k64, dtype=np.uint8), rng.integers(32, 64, BGZF_IN - k64, dtype=np.uint8)])
    rng.shuffle(a)
    return a.tobytes()


# found by search_cap_mix() below (the CPU test checks that they still lie where they are meant to)
CAP_SEED = 5
CAP_K64 = {"lds_cap_below": 994, "lds_cap_exact": 995, "lds_cap_above": 998}     # deflate data of 40959, 40960 and 40961 bytes


def search_cap_mix(seed=CAP_SEED):
    """The search that found CAP_K64: k64 by bisection on the emulation's block size, then a walk over its neighbourhood."""
    import scssim_amd
    size = lambda k: len(scssim_amd.bgzf_probe(cap_mix(k, seed), 1 << 30)) - 26
    lo, hi = 0, BGZF_IN
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if size(mid) <= BGZF_LDS_OUT:
            lo = mid
        else:
            hi = mid
    found = {}                                                          # per case: the first k whose size is nearest to the cap
    for k in range(max(0, lo - 100), min(BGZF_IN, lo + 100)):
        s = size(k)
        name = "lds_cap_exact" if s == BGZF_LDS_OUT else "lds_cap_below" if s < BGZF_LDS_OUT else "lds_cap_above"
        if abs(s - BGZF_LDS_OUT) < CAP_WINDOW and (name not in found or abs(s - BGZF_LDS_OUT) < abs(found[name][1] - BGZF_LDS_OUT)):
            found[name] = (k, s)
    return found


MIXED_KINDS = ["deflated", "stored_incompressible", "stored_cap"] * 4 + ["deflated"]


def _mixed():
    parts = []
    for i, kind in enumerate(MIXED_KINDS):
        if kind == "deflated":
            parts.append(fastq_text(BGZF_IN, 300 + i))
        elif kind == "stored_incompressible":
            parts.append(_uniform(BGZF_IN, 256, 300 + i, first=0))
        else:
            parts.append(_uniform(BGZF_IN, 45, 300 + i))                 # log2(45) = 5.49 bits per byte: 44 KB of deflate data
    return b"".join(parts)


_FQ = functools.lru_cache(None)(lambda: fastq_text(BGZF_IN + 1, 1))

# name -> (builder, kinds, reach); "deep": an unrestricted Huffman tree over block 0's histogram is deeper than 15
CASES = {"empty": (lambda: b"", [], "nbytes == 0: nothing is launched")}
for _n in SMALL_LENGTHS:
    CASES["len_%d" % _n] = (lambda n=_n: _FQ()[:n], None, "n < 16 (no uint4 histogram loop), n % 4 != 0 (byte-wise CRC), n < CHUNK (255 empty chunks)")
CASES.update({
    "one_symbol": (lambda: b"N" * 70000, ["deflated"] * 2, "m == 2: one literal and the end-of-block symbol; two blocks, the second short"),
    "two_symbols_equal": (lambda: b"AB" * 1000, ["deflated"], "equal frequencies: ties broken by symbol"),
    "all_256_flat": (lambda: _counts([252] * 256, 0, seed=20), ["stored_incompressible"], "stored by cbytes >= n + 5; all 256 literals used"),
    "all_256_skewed": (_all_256_skewed, ["deflated"], "all 256 literals used and deflated: every literal has a code"),
    "ties_with_eob": (_ties_with_eob, ["deflated"], "device rank order against the host's stable_sort: 200 literals tie with the end-of-block symbol's count 1"),
    "fibonacci": (_fibonacci, ["deflated"], "deep: the 15-bit repair of huff_lengths"),
})
for _n in range(17, 24):
    if sum(skewed_counts(_n)) <= 64000:                                   # (as in test_bgzf_arithmetic_inflates_with_zlib: one block)
        CASES["skewed_%d" % _n] = (lambda n=_n: _counts(skewed_counts(n), 97), ["deflated"], "deep: the 15-bit repair of huff_lengths, internal nodes below the limit")
CASES.update({
    "random": (lambda: _uniform(150000, 256, 23, first=0), ["stored_incompressible"] * 3, "stored, several blocks, the last one partial"),
    "exact_block": (lambda: _FQ()[:BGZF_IN], ["deflated"], "block boundary: exactly one block"),
    "block_plus_1": (lambda: _FQ()[:BGZF_IN + 1], ["deflated", None], "block boundary: a second block of one byte"),
    "block_minus_1": (lambda: _FQ()[:BGZF_IN - 1], ["deflated"], "block boundary: one byte short, n % 4 == 3"),
    "lds_cap_below": (lambda: cap_mix(CAP_K64["lds_cap_below"], CAP_SEED), ["deflated"], "LDS cap: deflate data at most BGZF_LDS_OUT, by less than 64 bytes"),
    "lds_cap_exact": (lambda: cap_mix(CAP_K64["lds_cap_exact"], CAP_SEED), ["deflated"], "LDS cap: deflate data of exactly BGZF_LDS_OUT bytes"),
    "lds_cap_above": (lambda: cap_mix(CAP_K64["lds_cap_above"], CAP_SEED), ["stored_cap"], "LDS cap: deflate data over BGZF_LDS_OUT, by less than 64 bytes"),
    "mixed": (_mixed, MIXED_KINDS, "deflated, stored-incompressible and stored-LDS-cap blocks adjacent in one output, all four values of dst & 3"),
    "big_text": (lambda: fastq_text(20200000, 24), ["deflated"] * 314, "many blocks (314): offsets far into the scan, one workgroup per block"),
})
DEEP = ["fibonacci"] + [k for k in CASES if k.startswith("skewed_")]
ZBASES = {name: ((0,) if name == "big_text" else (0, 1, 2, 3)) for name in CASES}


@functools.lru_cache(None)
def data(name):
    return CASES[name][0]()


def cut(d):
    """the input's cut into blocks: the ISIZE list"""
    return [min(BGZF_IN, len(d) - o) for o in range(0, len(d), BGZF_IN)]


def block_kinds(d):
    """Every block's kind under the host emulation: byte 18 says stored (0x01) or dynamic Huffman (low bits 0b101); a stored block
    that deflates once the LDS cap is lifted was stored for the cap, one that stays stored is incompressible."""
    import scssim_amd
    kinds = []
    blocks = scssim_amd.bgzf_blocks(scssim_amd.bgzf_probe(d))
    for i, (b, _) in enumerate(blocks):
        if b[18] == 0x01:
            free = scssim_amd.bgzf_probe(d[i * BGZF_IN:(i + 1) * BGZF_IN], 1 << 30)
            kinds.append("stored_incompressible" if free[18] == 0x01 else "stored_cap")
        else:
            assert b[18] & 7 == 0b101, "block %d: neither stored nor dynamic Huffman" % i
            kinds.append("deflated")
    return kinds


def huffman_depth(hist):
    """depth of an unrestricted Huffman tree over the non-zero counts"""
    import heapq
    h = [(int(c), 0) for c in hist if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def block_hist(block):
    """a block's literal counts + the end-of-block symbol's 1"""
    return list(np.bincount(np.frombuffer(block, np.uint8), minlength=256)) + [1]


# ---- the small scan (k_scan_small, scs_k_misc.hip)
SCAN_SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 262143, 262144, 262145, 1000003)
SMALL_SCAN_MAX = 262144                                                   # the last size of the one-workgroup path


def scan_partner(n):
    """the size of the first array when n is scanned as the second of a pair: another size of the list, 7 places on"""
    return SCAN_SIZES[(SCAN_SIZES.index(n) + 7) % len(SCAN_SIZES)]


def scan_input(n, kind, salt=0):
    """kind "small": values below 2^12 (below 2^16, and no sum of up to 1000003 of them wraps); "full": the whole uint32 range"""
    rng = np.random.default_rng([n, int(kind == "full"), salt])
    return rng.integers(0, 1 << 12 if kind == "small" else 1 << 32, n, dtype=np.uint64).astype(np.uint32)
