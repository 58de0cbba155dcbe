"""The jobs the attach kernels are checked on (tests/test_gpu_attach.py): genomes from fixed-seed numpy generators, the oracle's
dump read into arrays, and the arithmetic that says -- from that dump alone -- which branch of k_attach / k_attach_dense a job
reaches.  The primer budget of a template is Poisson with mean 65536 * primers * gamma * len / mean_len: 6.5 at the defaults,
65 and 131 in the high-budget cases here, below 1 in the sparse one (the fragments take their share of the pool).

k_attach_dense numbers a pass's primers through (item = slot_off[t] + i); wave w takes the templates whose first item lies in
[56 w, 56 w + 56) and works through their items 64 lanes at a time, every template of a chunk on a bitmap row of its own.  So
  a budget above 56 / 112 / 168      spans at least two / three / four chunks,
  fewer free positions than budget   (free = len - amp_min - 26 places a primer can take) makes the > 50 tries abort certain;
                                     free < 56 < budget: certain while chunks of the template are still to come (the carry),
  more templates in a window of 56 items than a chunk has bitmap rows (1024 / 33 = 31): the chunk ends early, and the next one
                                     starts with a new template on row 0, which must have been cleared.
k_attach<true, 64> walks a fragment's budget 64 primers at a time: a semi amplicon whose uid carries a primer index >= 64 was
made in a second round."""
import numpy as np

AMP_MIN, AMP_MAX = 1000, 2000          # Config.cpp:35-48 (not options of the command line)
DENSE_STRIDE, WAVE = 56, 64            # scs_k_amplify.hip: ATTACH_DENSE_STRIDE, lanes of a chunk
ROW_WORDS = (AMP_MAX - AMP_MIN) // 32 + 2
MAX_ROWS = 1024 // ROW_WORDS           # bitmap rows of a chunk: 31
MODEL, SEED, COVERAGE = "Illumina_HiSeq2500", 3, "0.5"

# genome writer, haplotype length, genome seed, -p, -r
CASES = {
    "high_budget":     dict(genome="random", n=20000, gseed=101, primers=100000, gamma=1e-8),
    "three_chunks":    dict(genome="random", n=10000, gseed=102, primers=200000, gamma=1e-8),
    "dry_high_budget": dict(genome="at_runs", n=20000, gseed=103, primers=100000, gamma=1e-8),
    "sparse":          dict(genome="random", n=600000, gseed=104, primers=1000, gamma=1e-8),
    "row_overflow":    dict(genome="random", n=4000000, gseed=105, primers=2500, gamma=1e-8),
}


def _write_diploid(path, seq, name=b"5"):
    n = len(seq)
    assert n % 100 == 0
    body = np.concatenate([seq.reshape(-1, 100), np.full((n // 100, 1), 10, np.uint8)], axis=1).tobytes()
    with open(path, "wb") as f:
        for hap in (1, 2):
            f.write(b">%s_%d_%d\n" % (name, hap, n))
            f.write(body)
    return path


def write_random_genome(path, n, seed):
    """Two haplotype records of n i.i.d. ACGT bases, 100-column lines."""
    rng = np.random.default_rng(seed)
    return _write_diploid(path, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def write_at_runs_genome(path, n, seed):
    """Alternating runs of A and of T, 8 to 40 bases each: a few hundred primer types carry every attachment."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(8, 41, size=n // 8 + 1)
    base = np.where(np.arange(len(runs)) % 2 == 0, ord("A"), ord("T")).astype(np.uint8)
    return _write_diploid(path, np.repeat(base, runs)[:n].copy())


def write_genome(case, path):
    c = CASES[case]
    return (write_random_genome if c["genome"] == "random" else write_at_runs_genome)(path, c["n"], c["gseed"])


def oracle_args(case):
    c = CASES[case]
    return ["-c", COVERAGE, "-p", str(c["primers"]), "-r", repr(c["gamma"])]


AMP_COLUMNS = ("parent", "spos", "len", "gc", "primers", "uid")


def load_amps(path):
    """A semis / fulls table of the oracle's dump (index, parent, spos, len, gc, primers, uid, pos:alt[,pos:alt...]) as arrays:
    the six columns, the error count and the first four errors (pos << 3 | alt, 0 beyond the count) per amplicon."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    n = len(lines)
    if n == 0:
        out = {k: np.zeros(0, np.uint64) for k in AMP_COLUMNS}
        out["nerr"] = np.zeros(0, np.uint32); out["errs"] = np.zeros((0, 4), np.uint32)
        return out
    heads, tails = [], []
    for l in lines:
        k = l.rfind("\t")
        heads.append(l[:k]); tails.append(l[k + 1:])
    cols = np.array("\t".join(heads).split("\t"), dtype=np.uint64).reshape(n, 7)
    assert np.array_equal(cols[:, 0], np.arange(n, dtype=np.uint64)), path
    out = {k: cols[:, 1 + j].copy() for j, k in enumerate(AMP_COLUMNS)}
    nerr = np.fromiter((t.count(":") for t in tails), np.int64, n)
    errs = np.zeros((n, 4), np.uint32)
    if nerr.sum():
        flat = np.array(",".join(t for t in tails if t).replace(":", ",").split(","), dtype=np.uint32).reshape(-1, 2)
        packed = flat[:, 0] << 3 | flat[:, 1]
        off = np.cumsum(nerr) - nerr
        for k in range(4):
            rows = np.nonzero(nerr > k)[0]
            errs[rows, k] = packed[off[rows] + k]
    out["nerr"] = nerr.astype(np.uint32); out["errs"] = errs
    return out


def load_primer_stock(path, stock):
    """primers.tsv (type, attachments, stock left; the types that were used) -> the 65536 stocks, and the table."""
    prim = np.loadtxt(path, dtype=np.int64, ndmin=2).reshape(-1, 3)
    want = np.full(65536, stock, np.int64)
    want[prim[:, 0]] = prim[:, 2]
    return want, prim


def load_read_numbers(path, n_fulls):
    rn = np.zeros(n_fulls, np.uint32)
    t = np.loadtxt(path, dtype=np.int64, ndmin=2).reshape(-1, 2)
    rn[t[:, 0]] = t[:, 1]
    return rn


def budget_counts(semis):
    """Of the last cycle's budgets: how many lie above 56 / 112 / 168, how many cannot be placed (budget > free positions), and how
    many of those are certain aborts with carry (free < 56 < budget: abandoned among the first 56 primers, further chunks follow)."""
    b = semis["primers"].astype(np.int64)
    free = semis["len"].astype(np.int64) - AMP_MIN - 26
    return dict(semis=int(b.size), mean_budget=float(b.mean()) if b.size else 0.0, max_budget=int(b.max()) if b.size else 0,
                above_56=int((b > 56).sum()), above_112=int((b > 112).sum()), above_168=int((b > 168).sum()),
                unplaceable=int((b > free).sum()), certain_aborts_with_carry=int(((b > 56) & (free < 56)).sum()))


def fragment_second_rounds(semis):
    """(fragment, pass) pairs that attached a primer of index >= 64 -- semi uid = fragment << 23 | pass << 20 | primer index --: their
    budget was above 64 and k_attach<true, 64> went into a second round for them.  Returns their number and the largest index."""
    idx = semis["uid"] & np.uint64(0xFFFFF)
    late = idx >= 64
    return int(np.unique(semis["uid"][late] >> np.uint64(20)).size), int(idx.max()) if idx.size else 0


def dry_types(prim, stock):
    """Primer types that end at 0, exactly: attachments + left == stock for every type."""
    assert (prim[:, 1] + prim[:, 2] == stock).all(), "attachments + left != stock"
    return int((prim[:, 2] == 0).sum()), int(prim.shape[0])


def densest_window(semis):
    """The most templates whose first primer item lies in one window [56 w, 56 w + 56) of the last cycle's items in list order
    (what one wave of k_attach_dense takes): more than MAX_ROWS of them do not fit a chunk's bitmap rows."""
    b = semis["primers"].astype(np.int64)
    first = (np.cumsum(b) - b)[b > 0]
    if first.size == 0:
        return 0
    return int(np.bincount(first // DENSE_STRIDE).max())


def row_split_restarts(semis):
    """k_attach_dense's chunking of the last cycle's items, wave by wave: how many chunks end early because their templates need
    more than MAX_ROWS bitmap rows -- each is followed by a chunk of the same wave whose first template is a new one (not the
    continuation of a cut one) and has to find row 0 empty."""
    b = semis["primers"].astype(np.int64)
    first = (np.cumsum(b) - b)[b > 0]
    if first.size == 0:
        return 0
    total, wave, restarts = int(b.sum()), first // DENSE_STRIDE, 0
    for w in np.unique(wave):
        mine = np.nonzero(wave == w)[0]
        item0 = int(first[mine[0]])
        end = int(first[mine[-1] + 1]) if mine[-1] + 1 < first.size else total
        while item0 < end:
            lanes = min(WAVE, end - item0)
            inside = first[np.searchsorted(first, item0, side="right"):np.searchsorted(first, item0 + lanes, side="left")]
            if 1 + inside.size > MAX_ROWS:                       # lane 0 heads a row of its own; the chunk ends before the first head without a row
                lanes = int(inside[MAX_ROWS - 1]) - item0
                restarts += 1
            item0 += lanes
    return restarts


def preconditions(case, semis, prim):
    """What the dump says about the branches the case is there for: (counts, list of unmet conditions)."""
    c = budget_counts(semis)
    c["fragment_second_rounds"], c["max_fragment_primer"] = fragment_second_rounds(semis)
    c["dry_types"], c["types_used"] = dry_types(prim, CASES[case]["primers"])
    c["densest_window"] = densest_window(semis)
    c["row_split_restarts"] = row_split_restarts(semis)
    need = {"high_budget": dict(above_56=1000, certain_aborts_with_carry=20, fragment_second_rounds=1),
            "three_chunks": dict(above_112=1000, above_168=100, certain_aborts_with_carry=100),
            "dry_high_budget": dict(dry_types=1, certain_aborts_with_carry=20),
            "sparse": dict(densest_window=MAX_ROWS + 1), "row_overflow": dict(row_split_restarts=300)}[case]
    unmet = ["%s = %d, needs >= %d" % (k, c[k], v) for k, v in need.items() if c[k] < v]
    return c, unmet
