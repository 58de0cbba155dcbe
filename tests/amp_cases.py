"""The amplicon table's reference restatement and case table, shared by tests/test_amplicons_host.py and tests/test_gpu_amplicons.py.

amplicon_line() builds a full amplicon's sequence the way oracle/scs_oracle.cpp does -- the fragment's template strand
(split_to_frags), semi_sequence, full_sequence -- and carries the genome index of every base through the same slices and
reversals.  Strand, interval and edits are then read off the sequence and its indices; no view arithmetic is restated here."""
import numpy as np

COMP = np.array([3, 2, 1, 0, 4], np.uint8)
LETTERS = "ACGTN"
HEADER = "#record\tstart\tend\tamplicon\tstrand\treads\tsemi\tedits\n"


def codes(seq):
    """ASCII bases -> codes 0..3, 4 for anything else."""
    lut = np.full(256, 4, np.uint8)
    for k, ch in enumerate("ACGT"):
        lut[ord(ch)] = lut[ord(ch.lower())] = k
    return lut[np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)]


def frag_template(G, goff, flen, strand):
    """(T, genome index of every base of T): T[i] = comp(g[len - 1 - i]) for strand +1, g[i] for -1 (split_to_frags)."""
    idx = np.arange(goff, goff + flen, dtype=np.int64)
    g = G[idx]
    return (COMP[g[::-1]], idx[::-1]) if strand == 1 else (g.copy(), idx)


def full_sequence(T, Ti, semi, full):
    """U and its genome indices: tmp = T[s : s + l] with the semi's substitutions, S = tmp reversed (semi_sequence);
    U[t] = comp(S[s2 + t]) with the full's substitutions (full_sequence)."""
    s, l, e1 = semi
    s2, l2, e2 = full
    if s + l > len(T) or s2 + l2 > l or l2 == 0:
        raise ValueError("the lineage does not fit")
    tmp, tmpi = T[s:s + l].copy(), Ti[s:s + l]
    for pos, alt in e1:
        tmp[pos] = alt
    S, Si = tmp[::-1], tmpi[::-1]
    U, Ui = COMP[S[s2:s2 + l2]], Si[s2:s2 + l2]
    for pos, alt in e2:
        U[pos] = alt
    return U, Ui


def amplicon_entry(G, frag, semi, full, rec_off, T=None):
    """(start, length, strand '+'/'-', [(record coordinate, ref code, alt code), ...]) of the full amplicon, genome-forward."""
    if T is None:
        T = frag_template(G, *frag)
    U, Ui = full_sequence(T[0], T[1], semi, full)
    fwd = len(Ui) < 2 or Ui[1] > Ui[0]
    if not fwd:                                            # the reverse complement of the genome: read it genome-forward
        U, Ui = COMP[U[::-1]], Ui[::-1]
    assert (np.diff(Ui) == 1).all()
    ref = G[Ui]
    at = np.nonzero(U != ref)[0]
    return int(Ui[0] - rec_off), len(U), "+" if fwd else "-", [(int(Ui[k] - rec_off), int(ref[k]), int(U[k])) for k in at]


def format_line(name, start, length, index, strand, reads, semi_index, edits):
    ed = ",".join("%d:%s>%s" % (x, LETTERS[r], LETTERS[a]) for x, r, a in edits) or "."
    return "%s\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (name, start, start + length, index, strand, reads, semi_index, ed)


def amplicon_line(G, frag, semi, full, rec_off, name, index, reads, semi_index, T=None):
    start, length, strand, edits = amplicon_entry(G, frag, semi, full, rec_off, T)
    return format_line(name, start, length, index, strand, reads, semi_index, edits)


# ---- the oracle's tables (--dump PREFIX) -> the whole table
def _errs(field):
    return [tuple(int(v) for v in e.split(":")) for e in field.split(",")] if field else []


def load_amps(path):
    out = []
    for ln in open(path).read().split("\n"):
        if ln:
            f = ln.split("\t")
            out.append((int(f[1]), int(f[2]), int(f[3]), _errs(f[7] if len(f) > 7 else "")))   # parent, spos, len, errors
    return out


def table_from_oracle(prefix, names, rec_lens, G):
    """Every line of the table, and the arrays of scs_amplicon_places, rebuilt from PREFIX.frags.tsv / .semis.tsv / .fulls.tsv /
    .readnum.tsv.  Returns (text, dict of arrays, most errors of a full, most errors of a semi that has a full)."""
    rec_off = np.concatenate([[0], np.cumsum(rec_lens)]).astype(np.int64)
    frags = [tuple(int(v) for v in ln.split("\t")) for ln in open(prefix + ".frags.tsv").read().split("\n") if ln]   # i, rec, start (1-based), len, strand
    semis, fulls = load_amps(prefix + ".semis.tsv"), load_amps(prefix + ".fulls.tsv")
    reads = np.zeros(len(fulls), np.int64)
    for ln in open(prefix + ".readnum.tsv").read().split("\n"):
        if ln:
            i, n = ln.split("\t")
            reads[int(i)] = int(n)
    tmpl = {}
    lines, arr = [HEADER], dict(rec=[], start=[], len=[], strand=[], n_edits=[])
    most_full = most_semi = 0
    for i, (sm, s2, l2, e2) in enumerate(fulls):
        f, s, l, e1 = semis[sm]
        _, rec, fstart, flen, fstrand = frags[f]
        goff = int(rec_off[rec]) + fstart - 1
        if f not in tmpl:
            tmpl[f] = frag_template(G, goff, flen, fstrand)
        start, length, strand, edits = amplicon_entry(G, (goff, flen, fstrand), (s, l, e1), (s2, l2, e2), int(rec_off[rec]), tmpl[f])
        assert 0 <= start and start + length <= rec_lens[rec]
        lines.append(format_line(names[rec], start, length, i, strand, int(reads[i]), sm, edits))
        for k, v in zip(("rec", "start", "len", "strand", "n_edits"), (rec, start, length, 1 if strand == "+" else -1, len(edits))):
            arr[k].append(v)
        most_full, most_semi = max(most_full, len(e2)), max(most_semi, len(e1))
    return "".join(lines), {k: np.array(v, np.int64) for k, v in arr.items()}, most_full, most_semi


def parse_table(text):
    """[(record, start, end, amplicon, strand, reads, semi, [(pos, ref, alt), ...]), ...] of a table's text."""
    lines = text.split("\n")
    assert lines[0] + "\n" == HEADER and lines[-1] == ""
    out = []
    for ln in lines[1:-1]:
        f = ln.split("\t")
        ed = [] if f[7] == "." else [(int(e.split(":")[0]), e.split(":")[1][0], e.split(":")[1][2]) for e in f[7].split(",")]
        out.append((f[0], int(f[1]), int(f[2]), int(f[3]), f[4], int(f[5]), int(f[6]), ed))
    return out
