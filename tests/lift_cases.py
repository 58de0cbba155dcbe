"""The lift table's restatements and the dense layout, shared by tests/test_lift_host.py and the GPU tests of everything that goes
through the table (test_gpu_lift.py, test_gpu_truth_ref.py, test_gpu_artefacts_ref.py, test_gpu_support_ref.py).  Plain numpy,
base by base; nothing here is shared with the library."""
import numpy as np

from gpu_readers import CIG, _sam


def ref_layout(ref_lens, w):
    """(bin_off, n_bins) of the reference records' bins."""
    off = np.concatenate([[0], np.cumsum([-(-int(ln) // w) for ln in ref_lens])]).astype(np.int64)
    return off, int(off[-1])


def copies_from_table(t, ref_lens, w):
    """copies[b] of the contract in numpy, base by base: n_bins + 1 entries, the last one the inserted bases."""
    off, nb = ref_layout(ref_lens, w)
    r = np.asarray(t.kind) == 0
    ln, rp, rr = np.asarray(t.len, np.int64)[r], np.asarray(t.ref_pos, np.int64)[r], np.asarray(t.ref_rec, np.int64)[r]
    within = np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln)
    copies = np.bincount(np.repeat(off[rr], ln) + (np.repeat(rp, ln) + within) // w, minlength=nb + 1).astype(np.uint64)
    assert copies[nb] == 0
    copies[nb] = np.asarray(t.len, np.uint64)[~r].sum()
    return copies


def lift_from_sam(path, seg, w):
    """The contract from the SAM's @SQ lines, POS and CIGAR through the segment table, base by base in numpy: (reads, bases) of
    n_bins + 1 entries, the record count, the sum of the M lengths, and what the reads of the job reach (the dense case's conditions)."""
    hdr, recs = _sam(path)
    sq = [(h.split("\t")[1][3:], int(h.split("\t")[2][3:])) for h in hdr if h.startswith("@SQ")]
    start = dict(zip([n for n, _ in sq], np.concatenate([[0], np.cumsum([ln for _, ln in sq])])[:-1]))
    off, nb = ref_layout(seg.ref_lens, w)
    m_start, m_len, m_read, has_d = [], [], [], np.zeros(len(recs), bool)
    for i, r in enumerate(recs):
        g = int(start[r[2]]) + int(r[3]) - 1
        for n, k in CIG.findall(r[5]):
            n = int(n)
            if k == "M":
                m_start.append(g); m_len.append(n); m_read.append(i)
            if k == "D":
                has_d[i] = True
            if k != "I":
                g += n
    m_start, m_len, m_read = np.array(m_start, np.int64), np.array(m_len, np.int64), np.array(m_read, np.int64)
    x = np.repeat(m_start, m_len) + np.arange(m_len.sum()) - np.repeat(np.cumsum(m_len) - m_len, m_len)   # every M-aligned base, read by read, ascending
    rid = np.repeat(m_read, m_len)
    si = np.searchsorted(seg.hap_off, x, side="right") - 1
    lifted = seg.kind[si] == 0
    r = seg.ref_pos[si] + x - seg.hap_off[si]
    b = np.where(lifted, off[seg.ref_rec[si]] + r // w, nb)
    bases = np.bincount(b, minlength=nb + 1).astype(np.uint64)
    idx = np.nonzero(lifted)[0]
    u, first = np.unique(rid[idx], return_index=True)
    reads = np.bincount(b[idx[first]], minlength=nb + 1).astype(np.uint64)
    reads[nb] += len(recs) - len(u)
    # what the reads reach
    touched = np.bincount(np.unique(rid * len(seg) + si) // len(seg), minlength=len(recs))    # segments a read's M runs touch
    _, first_base = np.unique(rid, return_index=True)
    same = (rid[1:] == rid[:-1]) & (x[1:] == x[:-1] + 1) & (si[1:] != si[:-1]) & lifted[1:] & lifted[:-1]
    back = same & (seg.ref_rec[si[1:]] == seg.ref_rec[si[:-1]]) & (r[1:] < r[:-1])
    reach = dict(cross=int((touched >= 2).sum()), cross2=int((touched >= 3).sum()), wholly_inserted=len(recs) - len(u),
                 starts_inserted=int((~lifted[first_base] & np.isin(np.arange(len(recs)), u)).sum()), back=len(np.unique(rid[1:][back])),
                 deletion_and_boundary=int((has_d & (touched >= 2)).sum()), n=len(recs))
    return reads, bases, len(recs), int(m_len.sum()), reach


# ---- the dense case
DENSE_INS, DENSE_STEP = 130, 170                           # bases of every insertion; reference bases from one insertion to the next (a deletion 40 behind each)
DENSE_COV = 14.0                                           # of the 60 kb REFERENCE, as genreads counts it (14x and not 3x: only two junctions jump backwards, and some reads of the job must cross one)


def write_dense_inputs(d, seed=5):
    """A 60 kb one-record reference and a variation file: every 170 bases an insertion of 130 bases and, 40 bases on, a deletion
    of 5 .. 40 bases; CN 4, CN 1 and CN 0 stretches of 4, 2 and 5 kb.  (The insertions are 130 bases and not 400: with reads of 75
    bases, boundaries must lie closer than two read lengths on average for most reads to cross one; 130 still holds a read of 125.)"""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 60000)]
    ref, var = str(d / "dense_ref.fa"), str(d / "dense_vars.txt")
    with open(ref, "wb") as f:
        f.write(b">1\n")
        f.write(np.concatenate([seq.reshape(-1, 60), np.full((1000, 1), 10, np.uint8)], axis=1).tobytes())
    lines, dels = ["# dense test variations"], [5, 12, 19, 26, 33, 40]
    for k, p in enumerate(range(300, 59500, DENSE_STEP)):
        lines.append("i\tchr1\t%d\t%s\thomo" % (p, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, DENSE_INS)]).decode()))
        lines.append("d\tchr1\t%d\t%d\thomo" % (p + 40, dels[k % len(dels)]))
    lines += ["c\tchr1\t10001\t14000\t4\t2", "c\tchr1\t25001\t27000\t1\t1", "c\tchr1\t40001\t45000\t0\t0"]
    open(var, "w").write("\n".join(lines) + "\n")
    return ref, var


DENSE_LONG_INS = 2500                                      # one insertion that holds whole amplicons (they are 1 to 2 kb; the layout's own insertions are 130 bases)


def write_dense_het_inputs(d):
    """write_dense_inputs' reference, and a copy of its variation file with a het substitution every 50 bases (REF as the
    reference has it, ALT the next base), one het insertion of 2500 bases and a stretch of 600 bases at CN 4 (two copies in tandem on
    either haplotype)."""
    ref, var = write_dense_inputs(d)
    seq = "".join(open(ref).read().split("\n")[1:])
    nxt = dict(A="C", C="G", G="T", T="A")
    lines = open(var).read().rstrip("\n").split("\n")
    lines += ["s\tchr1\t%d\t%s\t%s\thet" % (p, seq[p - 1], nxt[seq[p - 1]]) for p in range(325, 59500, 50)]
    rng = np.random.default_rng(3)
    lines.append("i\tchr1\t31000\t%s\thet" % bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, DENSE_LONG_INS)]).decode())
    lines.append("c\tchr1\t52001\t52600\t4\t2")             # a tandem unit shorter than an amplicon: two pieces of one amplicon overlap on the reference
    var2 = str(d / "dense_het_vars.txt")
    open(var2, "w").write("\n".join(lines) + "\n")
    return ref, var2


def expected_reach(t, L, n_reads):
    """What reads of L bases whose starts are uniform over the staged records reach in this layout (the builder's check on the CPU):
    expected reads per condition.  Amplicons of 1 - 2 kb are many boundaries long, so their ends change little."""
    kind, hap_off, ln = np.asarray(t.kind), np.asarray(t.hap_off, np.int64), np.asarray(t.len, np.int64)
    total = int(np.asarray(t.hap_lens).sum())
    x = np.arange(total - L)
    s0, s1 = np.searchsorted(hap_off, x, side="right") - 1, np.searchsorted(hap_off, x + L - 1, side="right") - 1
    rec_end = np.cumsum(np.asarray(t.hap_lens, np.int64))
    ok = np.searchsorted(rec_end, x, side="right") == np.searchsorted(rec_end, x + L - 1, side="right")   # inside one record
    rp = np.asarray(t.ref_pos, np.int64)
    jump_back = np.zeros(len(t), bool)
    jump_back[1:] = (kind[1:] == 0) & (kind[:-1] == 0) & (rp[1:] < rp[:-1] + ln[:-1])
    cum_back = np.concatenate([[0], np.cumsum(jump_back)])
    f = lambda m: float((m & ok).sum()) / ok.sum() * n_reads
    return dict(cross=f(s1 > s0), cross2=f(s1 > s0 + 1), wholly_inserted=f((s1 == s0) & (kind[s0] == 1)), starts_inserted=f((s1 > s0) & (kind[s0] == 1)),
                back=f(cum_back[s1 + 1] - cum_back[s0 + 1] > 0))
