"""The artefact table's reference restatement, shared by tests/test_artefacts_host.py and tests/test_gpu_artefacts.py.

Plain numpy over a parsed amplicon table (amp_cases.parse_table): the edits grouped by (record, coordinate, alternate base), and
TA / TR counted by brute-force containment of the coordinate in every amplicon's interval.  Nothing here is shared with the
library: no sort keys, no bisection, no prefix sums."""
import numpy as np

LETTERS = "ACGTN"
INFO = ['##INFO=<ID=NA,Number=1,Type=Integer,Description="full amplicons that carry the alternate base">',
        '##INFO=<ID=TA,Number=1,Type=Integer,Description="full amplicons that cover the site">',
        '##INFO=<ID=NR,Number=1,Type=Integer,Description="reads allotted to the NA amplicons">',
        '##INFO=<ID=TR,Number=1,Type=Integer,Description="reads allotted to the TA amplicons">']
KEYS = ("rec", "pos", "ref", "alt", "na", "ta", "nr", "tr")


def header(names, rec_lens):
    return "".join(ln + "\n" for ln in ["##fileformat=VCFv4.2", "##source=scssim"] + ["##contig=<ID=%s,length=%d>" % (n, l) for n, l in zip(names, rec_lens)]
                   + INFO + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"])


def sites_from_table(tab, names, rec_lens, G, min_reads=0, brute=True):
    """(body text, dict of arrays) of the artefact table of a parsed amplicon table.  G: the genome's codes 0..4, records concatenated.
    brute: TA / TR by testing every amplicon of the record against the coordinate.  A table with a million sites (ber = 0.01) takes
    brute=False: every amplicon adds one (and its reads) to each base of its interval in a per-base array, which the sites then
    read; tests/test_artefacts_host.py holds the two equal on the whole g1 table."""
    rec_of = {n: i for i, n in enumerate(names)}
    rec_off = np.concatenate([[0], np.cumsum(rec_lens)]).astype(np.int64)
    a_rec = np.array([rec_of[t[0]] for t in tab], np.int64)
    a_start, a_end, a_reads = (np.array([t[k] for t in tab], np.int64) for k in (1, 2, 5))
    carried = {}
    for t in tab:
        for pos, ref, alt in t[7]:
            assert LETTERS[G[rec_off[rec_of[t[0]]] + pos]] == ref and t[1] <= pos < t[2]
            c = carried.setdefault((rec_of[t[0]], pos, LETTERS.index(alt)), [0, 0])
            c[0] += 1
            c[1] += t[5]
    by_rec = {r: np.nonzero(a_rec == r)[0] for r in range(len(names))}
    if not brute:
        cov_a, cov_r = np.zeros(int(rec_off[-1]) + 1, np.int64), np.zeros(int(rec_off[-1]) + 1, np.int64)
        for lo, hi, rd in zip(rec_off[a_rec] + a_start, rec_off[a_rec] + a_end, a_reads):
            cov_a[lo:hi] += 1
            cov_r[lo:hi] += rd
    lines, arr = [], {k: [] for k in KEYS}
    for (r, pos, alt) in sorted(carried):
        na, nr = carried[(r, pos, alt)]
        if nr < min_reads:
            continue
        ref = int(G[rec_off[r] + pos])
        if brute:
            idx = by_rec[r]
            cover = idx[(a_start[idx] <= pos) & (pos < a_end[idx])]
            ta, tr = len(cover), int(a_reads[cover].sum())
        else:
            ta, tr = int(cov_a[rec_off[r] + pos]), int(cov_r[rec_off[r] + pos])
        lines.append("%s\t%d\t.\t%s\t%s\t.\t.\tNA=%d;TA=%d;NR=%d;TR=%d\n" % (names[r], pos + 1, LETTERS[ref], LETTERS[alt], na, ta, nr, tr))
        for k, v in zip(KEYS, (r, pos, ref, alt, na, ta, nr, tr)):
            arr[k].append(v)
    return "".join(lines), {k: np.array(v, np.int64) for k, v in arr.items()}


def figures(arr):
    """(sites, sum of NA, sites with NA >= 2, largest NA, coordinates with two or more alternate bases, sites with NR = 0)"""
    coord = arr["rec"] * (1 << 40) + arr["pos"]
    _, per_coord = np.unique(coord, return_counts=True)
    return (len(arr["na"]), int(arr["na"].sum()), int((arr["na"] >= 2).sum()), int(arr["na"].max()), int((per_coord >= 2).sum()), int((arr["nr"] == 0).sum()))


def most_alts_at_a_coordinate(arr):
    _, per_coord = np.unique(arr["rec"] * (1 << 40) + arr["pos"], return_counts=True)
    return int(per_coord.max()) if len(per_coord) else 0


def probe_inputs(tab, names, rec_lens):
    """The amplicon intervals and edit entries scs_artefact_probe takes, from a parsed amplicon table."""
    rec_of = {n: i for i, n in enumerate(names)}
    rec_off = np.concatenate([[0], np.cumsum(rec_lens)]).astype(np.int64)
    starts = [int(rec_off[rec_of[t[0]]]) + t[1] for t in tab]
    lens = [t[2] - t[1] for t in tab]
    reads = [t[5] for t in tab]
    edits = [(i, int(rec_off[rec_of[t[0]]]) + pos, LETTERS.index(alt)) for i, t in enumerate(tab) for pos, _, alt in t[7]]
    return starts, lens, reads, edits


def fasta(path):
    """(first word of every header, record lengths, the bases' codes 0..4 concatenated) of a FASTA file; the callers hold the names
    equal to scs_fasta_probe's."""
    from amp_cases import codes
    names, seqs = [], []
    for ln in open(path).read().split("\n"):
        if ln.startswith(">"):
            names.append(ln[1:].split()[0])
            seqs.append([])
        elif ln:
            seqs[-1].append(ln)
    seqs = ["".join(s) for s in seqs]
    return names, [len(s) for s in seqs], codes("".join(seqs))
