"""The reference restatement of the artefact table on the original reference (scs_write_artefacts_ref / scs_artefact_ref_sites),
shared by tests/test_artefacts_ref_host.py, tests/test_gpu_artefacts_ref.py and tools/site_ref_host_check.py.

Plain numpy, PER BASE and not per interval: the coverage of every staged index by amplicons and by reads (difference arrays and a
cumsum), scattered onto the reference index X(g) of every R-segment base with np.add.at; the entries grouped with np.unique over
(X, REF, ALT).  Nothing here is shared with the library: no pieces, no segment cursor, no sort keys, no bisection, no slabs."""
import numpy as np

LETTERS = "ACGTN"
NOTE = ("the base of the haplotype the amplicon copied (the template the polymerase misread); it differs from the reference FASTA where a "
        "substitution was planted")
INFO = ['##INFO=<ID=NA,Number=1,Type=Integer,Description="edit entries (full amplicon, haplotype position) that carry the alternate base and lift to the site">',
        '##INFO=<ID=TA,Number=1,Type=Integer,Description="pieces of full amplicons, of any haplotype and copy, that cover the site">',
        '##INFO=<ID=NR,Number=1,Type=Integer,Description="reads allotted to the amplicons of the NA entries">',
        '##INFO=<ID=TR,Number=1,Type=Integer,Description="reads allotted to the amplicons of the TA pieces">']
KEYS = ("ref_rec", "pos", "ref", "alt", "na", "ta", "nr", "tr")


class Segs:
    """A lift table as five integer arrays (scssim_amd.LiftTable's names)."""
    def __init__(self, rows):
        """rows: (hap_off, len, ref_pos, ref_rec, kind) per segment"""
        a = np.array(rows, np.int64).reshape(-1, 5)
        self.hap_off, self.len, self.ref_pos, self.ref_rec, self.kind = (np.ascontiguousarray(a[:, k]) for k in range(5))


def header(ref_names, ref_lens, unlifted):
    return "".join(ln + "\n" for ln in ["##fileformat=VCFv4.2", "##source=scssim", "##scssim_coordinates=reference", "##scssim_REF=<%s>" % NOTE,
                                        "##scssim_unlifted=<entries=%d,reads=%d>" % tuple(unlifted)]
                   + ["##contig=<ID=%s,length=%d>" % (n, l) for n, l in zip(ref_names, ref_lens)] + INFO + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"])


def ref_index(n, segs, ref_lens):
    """X(g) for every staged index g (-1: inserted sequence, or covered by no segment)"""
    ref_off = np.concatenate([[0], np.cumsum(np.asarray(ref_lens, np.int64))]).astype(np.int64)
    X = np.full(n, -1, np.int64)
    for h, l, rp, rr, k in zip(*(np.asarray(getattr(segs, f), np.int64) for f in ("hap_off", "len", "ref_pos", "ref_rec", "kind"))):
        if k == 0:
            X[h:h + l] = ref_off[rr] + rp + np.arange(l)
    return X, ref_off


def restate(starts, lens, reads, ed_g, ed_alt, ed_n, ed_reads, G, segs, ref_lens, ref_names, min_reads=0):
    """(body text, dict of arrays, (unlifted entries, unlifted reads), dict(ta=, tr= per reference index)).
    starts / lens / reads: the full amplicons (global staged start, length, read number).  Entry group i: ed_n[i] entries at staged
    index ed_g[i] with alternate base ed_alt[i], whose amplicons were allotted ed_reads[i] reads together (one entry each: ed_n = 1,
    ed_reads = its amplicon's reads).  G: the staged bases' codes 0..4, records concatenated."""
    G = np.asarray(G, np.int64)
    n = len(G)
    starts, lens, reads = (np.asarray(v, np.int64).reshape(-1) for v in (starts, lens, reads))
    ed_g, ed_alt, ed_n, ed_reads = (np.asarray(v, np.int64).reshape(-1) for v in (ed_g, ed_alt, ed_n, ed_reads))
    da, dr = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.add.at(da, starts, 1)
    np.add.at(da, starts + lens, -1)
    np.add.at(dr, starts, reads)
    np.add.at(dr, starts + lens, -reads)
    cov_a, cov_r = np.cumsum(da)[:n], np.cumsum(dr)[:n]
    X, ref_off = ref_index(n, segs, ref_lens)
    R = X >= 0
    ta, tr = np.zeros(int(ref_off[-1]), np.int64), np.zeros(int(ref_off[-1]), np.int64)
    np.add.at(ta, X[R], cov_a[R])
    np.add.at(tr, X[R], cov_r[R])
    xe = X[ed_g] if len(ed_g) else np.zeros(0, np.int64)
    lifted = xe >= 0
    unlifted = (int(ed_n[~lifted].sum()), int(ed_reads[~lifted].sum()))
    key = (xe[lifted] * 5 + G[ed_g[lifted]]) * 4 + ed_alt[lifted]
    uk, inv = np.unique(key, return_inverse=True)
    na, nr = np.zeros(len(uk), np.int64), np.zeros(len(uk), np.int64)
    np.add.at(na, inv, ed_n[lifted])
    np.add.at(nr, inv, ed_reads[lifted])
    x, ref, alt = uk // 20, (uk // 4) % 5, uk % 4
    rec = np.searchsorted(ref_off, x, side="right") - 1
    keep = nr >= min_reads
    arr = dict(ref_rec=rec[keep], pos=(x - ref_off[rec])[keep], ref=ref[keep], alt=alt[keep], na=na[keep], ta=ta[x][keep], nr=nr[keep], tr=tr[x][keep])
    lines = ["%s\t%d\t.\t%s\t%s\t.\t.\tNA=%d;TA=%d;NR=%d;TR=%d\n" % (ref_names[r], p + 1, LETTERS[f], LETTERS[a], v, w, y, z)
             for r, p, f, a, v, w, y, z in zip(*(arr[k].tolist() for k in KEYS))]
    return "".join(lines), arr, unlifted, dict(ta=ta, tr=tr, X=X)


def restate_entries(starts, lens, reads, edits, G, segs, ref_lens, ref_names, min_reads=0):
    """restate over edit entries (amplicon, global staged index, alternate base) -- scs_artefact_ref_probe's inputs."""
    e = np.array(edits, np.int64).reshape(-1, 3)
    return restate(starts, lens, reads, e[:, 1], e[:, 2], np.ones(len(e), np.int64), np.asarray(reads, np.int64).reshape(-1)[e[:, 0]] if len(e) else np.zeros(0, np.int64),
                   G, segs, ref_lens, ref_names, min_reads)


def conservation(arr, unlifted, extra, starts, lens, n_entries, entry_reads):
    """The three laws as literal assertions: every entry is in a line or unlifted, so are its reads, and the pieces' bases are the
    amplicon bases that lie in R segments."""
    assert int(arr["na"].sum()) + unlifted[0] == n_entries
    assert int(arr["nr"].sum()) + unlifted[1] == entry_reads
    X = extra["X"]
    in_r = np.concatenate([[0], np.cumsum(X >= 0)])
    starts, lens = np.asarray(starts, np.int64).reshape(-1), np.asarray(lens, np.int64).reshape(-1)
    assert int(extra["ta"].sum()) == int((in_r[starts + lens] - in_r[starts]).sum())


def pieces_of(start, length, segs, ref_lens):
    """The reference intervals [X0, X1) of one amplicon, one per R segment it touches, in staged order (the test's own statement of
    a piece, for the figures the GPU tests assert about their jobs)."""
    ref_off = np.concatenate([[0], np.cumsum(np.asarray(ref_lens, np.int64))]).astype(np.int64)
    h, l = np.asarray(segs.hap_off, np.int64), np.asarray(segs.len, np.int64)
    out = []
    for i in range(int(np.searchsorted(h, start, side="right")) - 1, len(h)):
        if h[i] >= start + length:
            break
        if int(segs.kind[i]) == 0:
            g0, g1 = max(start, int(h[i])), min(start + length, int(h[i] + l[i]))
            x0 = int(ref_off[int(segs.ref_rec[i])]) + int(segs.ref_pos[i]) + g0 - int(h[i])
            out.append((x0, x0 + g1 - g0))
    return out
