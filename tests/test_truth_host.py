"""Host-side tests of the truth SAM (scs_set_truth_sam): the record formatter the truth kernels run, through its host probe, against
a short restatement of the semantics in Python; the CLI's --truth option and its refusals.  No GPU needed."""
import os
import random
import subprocess

import pytest

from conftest import ROOT

import scssim_amd

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def read_bases(n, events):
    """Profile::predict's output positions: window index, or -1 for an inserted base (after the n + delta < 50 rollback)."""
    if n + sum(-l if d else l for _, d, l in events) < 50:
        events = []
    ev = {p: (d, l) for p, d, l in events}
    out, j = [], 0
    while j < n:
        if j in ev and ev[j][0]:
            j += ev[j][1]
            continue
        out.append(j)
        if j in ev:
            out += [-1] * ev[j][1]
        j += 1
    return out


def placement(pos0, n, events, reverse):
    """Genome-forward list of the read's bases: genome coordinate, or None for an inserted base."""
    w = read_bases(n, events)
    coords = [None if x < 0 else (pos0 - x if reverse else pos0 + x) for x in w]
    return coords[::-1] if reverse else coords


def restate(seq, qual, genome, gstart, pos0, n, events, reverse, rname, amp, cnt, paired=False, is_read2=False, mate=None):
    coords = placement(pos0, n, events, reverse)
    assert len(coords) == len(seq)
    fseq, fqual = (revcomp(seq), qual[::-1]) if reverse else (seq, qual)
    ops, prev, nm, md, run = [], None, 0, "", 0

    def op(k, l):
        if ops and ops[-1][0] == k:
            ops[-1][1] += l
        else:
            ops.append([k, l])
    for i, c in enumerate(coords):
        if c is None:
            op("I", 1)
            nm += 1
            continue
        if prev is not None and c > prev + 1:
            op("D", c - prev - 1)
            nm += c - prev - 1
            md += "%d^%s" % (run, genome[prev + 1 - gstart:c - gstart])
            run = 0
        op("M", 1)
        g = genome[c - gstart]
        if fseq[i] == g:
            run += 1
        else:
            md += "%d%s" % (run, g)
            run, nm = 0, nm + 1
        prev = c
    md += "%d" % run
    lo, hi = min(c for c in coords if c is not None), max(c for c in coords if c is not None)
    cigar = "".join("%d%s" % (l, k) for k, l in ops)
    if paired:
        mc = [c for c in placement(mate[0], n, mate[2], mate[1]) if c is not None]
        mlo, mhi = min(mc), max(mc)
        t = max(hi, mhi) - min(lo, mlo) + 1
        flag = 0x3 | (0x80 if is_read2 else 0x40) | (0x10 if reverse else 0) | (0x20 if mate[1] else 0)
        tlen = t if (lo < mlo or (lo == mlo and not is_read2)) else -t
        mates = "=\t%d\t%d" % (mlo + 1, tlen)
    else:
        flag, mates = (0x10 if reverse else 0), "*\t0\t0"
    return "%d#%d\t%d\t%s\t%d\t255\t%s\t%s\t%s\t%s\tNM:i:%d\tMD:Z:%s\n" % (amp, cnt, flag, rname, lo + 1, cigar, mates, fseq, fqual, nm, md)


def make_read(rng, genome, gstart, pos0, n, events, reverse, subs=(), n_at=()):
    """The FASTQ bases a read with these events would carry: the genome under it, random inserted bases, substitutions at the
    given read positions, N at others; qualities are arbitrary."""
    coords = placement(pos0, n, events, reverse)
    f = [rng.choice("ACGT") if c is None else genome[c - gstart] for c in coords]
    for i in subs:
        f[i] = {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[f[i]]
    for i in n_at:
        f[i] = "N"
    fs = "".join(f)
    seq = revcomp(fs) if reverse else fs
    qual = "".join(chr(33 + rng.randrange(42)) for _ in seq)
    return seq, qual


CASES = [
    # name, n, events, reverse, extra (subs, n in read, n in genome)
    ("no_events", 150, [], False, {}),
    ("leading_deletion", 150, [(0, 1, 3)], False, {}),
    ("deletion_clipped_at_window_end", 150, [(40, 0, 1), (147, 1, 3)], False, {}),
    ("insertion_after_last_base", 150, [(149, 0, 2)], False, {}),
    ("insertion_then_deletion", 150, [(10, 0, 2), (11, 1, 3)], False, {"subs": (30, 31, 90)}),
    ("reverse_strand", 150, [(5, 0, 1), (60, 1, 2)], True, {"subs": (0, 77)}),
    ("reverse_leading_trailing", 150, [(0, 1, 2), (149, 0, 3)], True, {}),
    ("n_in_genome_and_read", 150, [(20, 1, 1)], False, {"n_at": (5, 6), "g_n": (150, 151, 152)}),
    ("rollback_51", 51, [(10, 1, 2)], False, {}),
    ("many_events", 150, [(3, 0, 1), (4, 1, 2), (9, 1, 1), (10, 1, 1), (100, 0, 4), (120, 1, 5)], False, {"subs": (2, 50)}),
]


@pytest.mark.parametrize("name,n,events,reverse,extra", CASES, ids=[c[0] for c in CASES])
def test_single_end_record_matches_the_semantics(name, n, events, reverse, extra):
    rng = random.Random(sum(map(ord, name)))
    gstart, glen = 1000, 400
    genome = [rng.choice("ACGT") for _ in range(glen)]
    for i in extra.get("g_n", ()):
        genome[i] = "N"
    genome = "".join(genome)
    pos0 = gstart + (300 if reverse else 100)
    seq, qual = make_read(rng, genome, gstart, pos0, n, events, reverse, extra.get("subs", ()), extra.get("n_at", ()))
    got = scssim_amd.truth_record_probe(seq, qual, genome, pos0, n, events, reverse=reverse, genome_start=gstart, rname="chr7_1_5000", amp=17, cnt=3)
    want = restate(seq, qual, genome, gstart, pos0, n, events, reverse, "chr7_1_5000", 17, 3)
    assert got == want
    f = got.rstrip("\n").split("\t")
    if name == "leading_deletion":
        assert f[3] == str(pos0 + 3 + 1) and f[5] == "147M"
    if name == "deletion_clipped_at_window_end":
        assert f[5] == "41M1I106M" and "D" not in f[5]
    if name == "insertion_after_last_base":
        assert f[5] == "150M2I"
    if name == "insertion_then_deletion":
        assert f[5] == "11M2I3D136M"
    if name == "reverse_leading_trailing":
        assert f[1] == "16" and f[5] == "3I148M"
    if name == "rollback_51":
        assert f[5] == "51M" and f[-2] == "NM:i:0"
    if name == "n_in_genome_and_read":
        assert "N" in f[9] and f[-2] != "NM:i:0"


def test_pairs_read2_reversed_cigar_nine_digit_pos_negative_tlen():
    rng = random.Random(5)
    gstart, glen = 123456000, 2000
    genome = "".join(rng.choice("ACGTN" if i % 97 == 0 else "ACGT") for i in range(glen))
    n = 150
    # forward amplicon: read 1 forward at 123456700, read 2 = revcomp of the far end (window base 0 = its rightmost base)
    e1, e2 = [(7, 1, 2)], [(3, 0, 2), (30, 1, 4), (100, 0, 1)]
    p1, p2 = 123456700, 123456700 + 310
    s1, q1 = make_read(rng, genome, gstart, p1, n, e1, False, (12,))
    s2, q2 = make_read(rng, genome, gstart, p2, n, e2, True, (0, 140))
    r1 = scssim_amd.truth_record_probe(s1, q1, genome, p1, n, e1, False, gstart, "9_2_200000000", 123456, 7, True, False, (p2, True, e2))
    r2 = scssim_amd.truth_record_probe(s2, q2, genome, p2, n, e2, True, gstart, "9_2_200000000", 123456, 7, True, True, (p1, False, e1))
    assert r1 == restate(s1, q1, genome, gstart, p1, n, e1, False, "9_2_200000000", 123456, 7, True, False, (p2, True, e2))
    assert r2 == restate(s2, q2, genome, gstart, p2, n, e2, True, "9_2_200000000", 123456, 7, True, True, (p1, False, e1))
    f1, f2 = r1.split("\t"), r2.split("\t")
    assert f1[1] == "99" and f2[1] == "147"
    assert len(f1[3]) == 9 and int(f1[8]) > 0 and int(f2[8]) == -int(f1[8])
    assert f2[5] == "49M1I67M4D26M2I4M"                      # read 2's events (4M2I26M4D67M1I49M in read order), genome-forward
    assert f1[7] == f2[3] and f2[7] == f1[3]


def test_probe_refuses_what_is_not_an_alignment():
    g = "ACGT" * 100
    with pytest.raises(scssim_amd.ScsError):                 # SEQ shorter than the events make the read
        scssim_amd.truth_record_probe("A" * 149, "I" * 149, g, 10, 150, [])
    with pytest.raises(scssim_amd.ScsError):                 # events out of order
        scssim_amd.truth_record_probe("A" * 150, "I" * 150, g, 10, 150, [(20, 1, 1), (10, 0, 1)])


def test_cli_lists_truth():
    r = subprocess.run([CLI, "genreads", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--truth" in r.stderr


@pytest.mark.parametrize("extra,msg", [(["--writers", "4"], "--writers 1"), (["--gpus", "2"], "--gpus 1")])
def test_cli_refuses_truth_with_parts_or_shards(extra, msg, tmp_path):
    # the inputs do not exist: a run that got as far as opening the GPU or a file would say something else
    r = subprocess.run([CLI, "genreads", "-i", str(tmp_path / "none.fa"), "-m", str(tmp_path / "none.profile"), "-o", str(tmp_path / "o"),
                        "--truth", str(tmp_path / "t.sam")] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert r.stderr.strip().splitlines() == [r.stderr.strip().splitlines()[0]] and msg in r.stderr and "--truth" in r.stderr
    assert not os.path.exists(tmp_path / "t.sam")
