"""The truth SAM on the original reference restated base by base, for tests/test_truth_ref_host.py and
tests/test_gpu_truth_ref.py: a haplotype alignment (global staged index of POS, CIGAR) is expanded to columns, every haplotype
position is looked up in the segment table with numpy.searchsorted, and blocks, primary block, clips and mate fields are derived
from the column list, which is then run-length encoded.  Nothing here walks segments with a cursor, as the library does."""
import re

import numpy as np

CIG = re.compile(r"(\d+)([MIDS])")


class Table:
    """A lift table for the restatement: the five arrays as int64, the reference records' names and lengths, the staged records'."""

    def __init__(self, hap_off, length, ref_pos, ref_rec, kind, ref_names, ref_lens, hap_names, hap_lens):
        self.hap_off, self.len, self.ref_pos, self.ref_rec, self.kind = (np.asarray(x, np.int64) for x in (hap_off, length, ref_pos, ref_rec, kind))
        self.ref_names, self.ref_lens = list(ref_names), [int(x) for x in ref_lens]
        self.hap_names, self.hap_lens = list(hap_names), [int(x) for x in hap_lens]
        self.hap_start = dict(zip(self.hap_names, np.concatenate([[0], np.cumsum(self.hap_lens)])[:-1].tolist()))

    def __len__(self):
        return len(self.hap_off)


def lift_columns(t, glo, cigar):
    """The lifted columns of a haplotype alignment that starts at global staged index glo: a list of (kind, read index or None,
    reference record, reference coordinate, block) in walk order, kind 'M' / 'I' / 'D'; then the number of blocks.  Raises
    ValueError(3) when a segment it touches lifts outside its reference record."""
    kinds, gs, qs, g, q = [], [], [], glo, 0
    for n, k in CIG.findall(cigar):
        n = int(n)
        for _ in range(n):
            kinds.append(k); gs.append(-1 if k == "I" else g); qs.append(None if k == "D" else q)
            g += k != "I"; q += k != "D"
    si = np.searchsorted(t.hap_off, np.array(gs, np.int64), side="right") - 1
    cols, prev, block = [], None, -1
    for k, g, q, s in zip(kinds, gs, qs, si.tolist()):
        if k == "I":
            cols.append(("I", q, None, None, None))
            continue
        if t.kind[s] == 1:
            if k == "M":
                cols.append(("I", q, None, None, None))
            continue
        rec, r = int(t.ref_rec[s]), int(t.ref_pos[s] + g - t.hap_off[s])
        if rec >= len(t.ref_lens) or t.ref_pos[s] + t.len[s] > t.ref_lens[rec]:
            raise ValueError(3)
        if prev is None:
            block = 0
        elif s != prev:
            p_rec, p_end = int(t.ref_rec[prev]), int(t.ref_pos[prev] + t.len[prev])
            if p_rec == rec and int(t.ref_pos[s]) >= p_end:
                cols += [("D", None, rec, x, block) for x in range(p_end, int(t.ref_pos[s]))]
            else:
                block += 1
        prev = s
        cols.append((k, q, rec, r, block))
    return cols, block + 1


def lift_alignment(t, glo, cigar):
    """dict(mapped, rec, pos, end, cigar, blocks) of the alignment's primary block (pos 0-based, end exclusive)."""
    cols, blocks = lift_columns(t, glo, cigar)
    qlen = sum(int(n) for n, k in CIG.findall(cigar) if k != "D")
    m_of = [sum(1 for c in cols if c[0] == "M" and c[4] == b) for b in range(blocks)]
    if not blocks or max(m_of) == 0:
        return dict(mapped=False, rec=None, pos=None, end=None, cigar="*", blocks=0)
    best = m_of.index(max(m_of))                                                         # (the first of equals)
    idx = [i for i, c in enumerate(cols) if c[0] == "M" and c[4] == best]
    first, last = idx[0], idx[-1]
    q0, q1 = cols[first][1], cols[last][1] + 1
    ops = [["S", q0]] if q0 else []
    for c in cols[first:last + 1]:
        if ops and ops[-1][0] == c[0]:
            ops[-1][1] += 1
        else:
            ops.append([c[0], 1])
    if qlen > q1:
        ops.append(["S", qlen - q1])
    return dict(mapped=True, rec=cols[first][2], pos=cols[first][3], end=cols[last][3] + 1, cigar="".join("%d%s" % (n, k) for k, n in ops), blocks=blocks)


def lifted(t, r):
    return lift_alignment(t, t.hap_start[r[2]] + int(r[3]) - 1, r[5])


def lift_line(t, rec, mate, a=None, m=None):
    """The reference SAM line of a haplotype SAM record (its tab-separated fields, NM / MD or none behind QUAL) and its mate's
    (None: single end).  a, m: their lifted alignments where the caller has them already."""
    a, flag = a or lifted(t, rec), int(rec[1])
    m = (m or lifted(t, mate)) if mate is not None else None
    read2 = bool(flag & 0x80)
    out_flag = flag & 0x10
    if m is not None:
        same = a["mapped"] and m["mapped"] and a["rec"] == m["rec"]
        out_flag |= 0x1 | (flag & 0xE0) | (0 if m["mapped"] else 0x8) | (0x2 if same else 0)
    if not a["mapped"]:
        out_flag |= 0x4
    own = a if a["mapped"] else m if m is not None and m["mapped"] else None
    rname, pos = (t.ref_names[own["rec"]], own["pos"] + 1) if own else ("*", 0)
    rnext, pnext, tlen = "*", 0, 0
    if m is not None and own:
        theirs = m if m["mapped"] else a
        rnext, pnext = "=" if theirs["rec"] == own["rec"] else t.ref_names[theirs["rec"]], theirs["pos"] + 1
        if same:
            span = max(a["end"], m["end"]) - min(a["pos"], m["pos"])
            tlen = span if a["pos"] < m["pos"] or (a["pos"] == m["pos"] and not read2) else -span
    f = [rec[0], str(out_flag), rname, str(pos), "255" if a["mapped"] else "0", a["cigar"], rnext, str(pnext), str(tlen), rec[9], rec[10],
         "YH:Z:" + rec[2], "YP:i:" + rec[3], "YB:i:%d" % a["blocks"]]
    return "\t".join(f) + "\n"


def lift_sam_records(t, recs, paired):
    """Every record of a haplotype SAM (its field lists, FASTQ order: read 1 then its read 2) as reference SAM lines."""
    al = [lifted(t, r) for r in recs]
    return [lift_line(t, r, recs[i ^ 1] if paired else None, al[i], al[i ^ 1] if paired else None) for i, r in enumerate(recs)]


def table_from_lift_file(path):
    """The table of a ##scssim-lift v1 file (global haplotype offsets, as the library numbers them)."""
    ref, hap, rows = [], [], []
    for ln in open(path).read().split("\n")[1:-1]:
        f = ln.split("\t")
        if f[0] in ("#ref", "#hap"):
            (ref if f[0] == "#ref" else hap).append((f[1], int(f[2])))
        else:
            rows.append(f)
    start = dict(zip([n for n, _ in hap], np.concatenate([[0], np.cumsum([l for _, l in hap])])[:-1].tolist()))
    ridx = {n: i for i, (n, _) in enumerate(ref)}
    return Table([start[f[0]] + int(f[1]) for f in rows], [int(f[2]) - int(f[1]) for f in rows], [int(f[4]) for f in rows], [ridx[f[3]] for f in rows],
                 [f[6] == "I" for f in rows], [n for n, _ in ref], [l for _, l in ref], [n for n, _ in hap], [l for _, l in hap])


def column_check(t, hap_recs, ref_recs, lift_positions):
    """The independent check of every record of a reference SAM against the haplotype SAM of the same job: every M column of the
    lifted CIGAR, walked from POS, holds a read base whose haplotype position (the haplotype SAM's own POS and CIGAR) lifts -- one
    lift_positions(record indices, record coordinates) call for all of them -- to kind R and exactly that reference record and
    coordinate; M + I + S is the SEQ length; no record starts or ends with D; the unmapped records are exactly the reads with no M
    base in an R segment.  Returns (records, M columns checked, unmapped records)."""
    assert len(hap_recs) == len(ref_recs)
    hidx, ridx = {n: i for i, n in enumerate(t.hap_names)}, {n: i for i, n in enumerate(t.ref_names)}
    h_rec, h_pos, h_read, h_q = [], [], [], []                                         # every M base of every haplotype record
    for i, h in enumerate(hap_recs):
        g, q = int(h[3]) - 1, 0
        for n, k in CIG.findall(h[5]):
            n = int(n)
            if k == "M":
                h_pos.append(np.arange(g, g + n)); h_q.append(np.arange(q, q + n)); h_read.append(np.full(n, i)); h_rec.append(np.full(n, hidx[h[2]]))
            g += n if k != "I" else 0; q += n if k != "D" else 0
    h_rec, h_pos, h_read, h_q = (np.concatenate(x).astype(np.int64) for x in (h_rec, h_pos, h_read, h_q))
    l_rec, l_pos, l_kind = (np.asarray(x).astype(np.int64) for x in lift_positions(h_rec, h_pos))
    has_r = np.bincount(h_read[l_kind == 0], minlength=len(hap_recs)) > 0
    first = np.concatenate([[0], np.cumsum(np.bincount(h_read, minlength=len(hap_recs)))])   # read i's M bases: [first[i], first[i + 1]), ascending read index
    n_cols = n_unmapped = 0
    for i, (h, r) in enumerate(zip(hap_recs, ref_recs)):
        assert r[0] == h[0] and r[9] == h[9] and r[10] == h[10] and int(r[1]) & 0x10 == int(h[1]) & 0x10, (i, r)
        if int(r[1]) & 0x4:
            assert not has_r[i] and r[5] == "*" and r[4] == "0", (i, r)
            n_unmapped += 1
            continue
        assert has_r[i], (i, r)
        ops = [(int(n), k) for n, k in CIG.findall(r[5])]
        assert "".join("%d%s" % o for o in ops) == r[5] and sum(n for n, k in ops if k in "MIS") == len(r[9]), (i, r)
        core = [o for o in ops if o[1] != "S"]
        assert core[0][1] != "D" and core[-1][1] != "D" and all(k != "S" for _, k in ops[1:-1]), (i, r)
        qs, xs, q, x = [], [], 0, int(r[3]) - 1
        for n, k in ops:
            if k == "M":
                qs.append(np.arange(q, q + n)); xs.append(np.arange(x, x + n))
            q += n if k != "D" else 0; x += n if k in "MD" else 0
        qs, xs = np.concatenate(qs), np.concatenate(xs)
        mine = slice(first[i], first[i + 1])
        at = np.searchsorted(h_q[mine], qs)                                             # the read base's place among the haplotype record's M bases
        assert (at < first[i + 1] - first[i]).all() and (h_q[mine][at] == qs).all(), (i, r)   # every lifted M base is an M base of the haplotype record
        assert (l_kind[mine][at] == 0).all() and (l_rec[mine][at] == ridx[r[2]]).all() and (l_pos[mine][at] == xs).all(), (i, r)
        n_cols += len(qs)
    return len(ref_recs), n_cols, n_unmapped
