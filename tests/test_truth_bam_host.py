"""Host-side tests of the truth BAM (scs_set_truth_bam): the BAM record formatter the truth kernels run, through its host probe,
against the truth SAM's probe of the same read column for column (tests/test_truth_host.py pins that one to the semantics), the
fields BAM adds (block_size, l_read_name, bin, the packed SEQ, Phred bytes, the NM tag's type), the probe's refusals, and the
CLI's --truth-bam option.  No GPU needed."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT

import scssim_amd
from bam_cases import parse_record, reg2bin

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def placement(pos0, n, events, reverse):
    """Genome-forward list of the read's bases: genome coordinate, or None for an inserted base (Profile::predict's output
    positions after the n + delta < 50 rollback)."""
    if n + sum(-l if d else l for _, d, l in events) < 50:
        events = []
    ev = {p: (d, l) for p, d, l in events}
    w, j = [], 0
    while j < n:
        if j in ev and ev[j][0]:
            j += ev[j][1]
            continue
        w.append(j)
        if j in ev:
            w += [-1] * ev[j][1]
        j += 1
    coords = [None if x < 0 else (pos0 - x if reverse else pos0 + x) for x in w]
    return coords[::-1] if reverse else coords


def make_read(rng, genome, gstart, pos0, n, events, reverse, subs=(), n_at=(), qual=None):
    """The FASTQ bases a read with these events would carry: the genome under it, random inserted bases, substitutions and N at
    the given read positions."""
    f = [rng.choice("ACGT") if c is None else genome[c - gstart] for c in placement(pos0, n, events, reverse)]
    for i in subs:
        f[i] = {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[f[i]]
    for i in n_at:
        f[i] = "N"
    fs = "".join(f)
    seq = revcomp(fs) if reverse else fs
    return seq, qual if qual is not None else "".join(chr(33 + rng.randrange(42)) for _ in seq)


# the single-end grid of tests/test_truth_host.py: name, n, events, reverse, extra (subs, N in the read, N in the genome)
CASES = [
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


def both(seq, qual, genome, pos0, n, events, **kw):
    """The SAM probe's columns and the BAM probe's record, decoded, of one read."""
    sam = scssim_amd.truth_record_probe(seq, qual, genome, pos0, n, events, **kw)
    raw = scssim_amd.truth_bam_record_probe(seq, qual, genome, pos0, n, events, **kw)
    rec, end = parse_record(raw, 0, [kw.get("rname", "chr")])
    assert end == len(raw)
    assert sam.endswith("\n")
    return sam[:-1].split("\t"), rec, raw


def direct_checks(cols, rec, raw, paired):
    assert rec["block_size"] == len(raw) - 4
    assert rec["l_read_name"] == len(cols[0]) + 1
    assert rec["refID"] == 0 and rec["mapq"] == 255 and rec["pos"] == int(cols[3]) - 1
    assert rec["bin"] == reg2bin(rec["pos"], rec["pos"] + rec["span"])
    assert rec["n_cigar_op"] == sum(c in "MID" for c in cols[5])
    assert (rec["next_refID"], rec["next_pos"]) == ((0, int(cols[7]) - 1) if paired else (-1, -1))
    assert [(t, ty) for t, ty, _ in rec["tags"]] == [("NM", "i"), ("MD", "Z")]
    if rec["l_seq"] & 1:
        assert rec["seq_bytes"][-1] & 15 == 0


@pytest.mark.parametrize("name,n,events,reverse,extra", CASES, ids=[c[0] for c in CASES])
def test_single_end_record_equals_the_sam_line(name, n, events, reverse, extra):
    rng = random.Random(sum(map(ord, name)))
    gstart, glen = 1000, 400
    genome = [rng.choice("ACGT") for _ in range(glen)]
    for i in extra.get("g_n", ()):
        genome[i] = "N"
    genome = "".join(genome)
    pos0 = gstart + (300 if reverse else 100)
    seq, qual = make_read(rng, genome, gstart, pos0, n, events, reverse, extra.get("subs", ()), extra.get("n_at", ()))
    cols, rec, raw = both(seq, qual, genome, pos0, n, events, reverse=reverse, genome_start=gstart, rname="chr7_1_5000", amp=17, cnt=3)
    assert rec["cols"] == cols
    direct_checks(cols, rec, raw, False)
    if name == "insertion_after_last_base":
        assert rec["n_cigar_op"] == 2 and cols[5] == "150M2I"
    if name == "rollback_51":
        assert rec["l_seq"] == 51 and rec["seq_bytes"][-1] & 15 == 0 and len(rec["seq_bytes"]) == 26
    if name == "n_in_genome_and_read":
        assert rec["seq_bytes"][2] & 15 == 15 and rec["seq_bytes"][3] >> 4 == 15      # N at read bases 5 and 6


def test_pair_read2_reversed_cigar_nine_digit_pos_negative_tlen():
    rng = random.Random(5)
    gstart, glen = 123456000, 2000
    genome = "".join(rng.choice("ACGTN" if i % 97 == 0 else "ACGT") for i in range(glen))
    n = 150
    e1, e2 = [(7, 1, 2)], [(3, 0, 2), (30, 1, 4), (100, 0, 1)]
    p1, p2 = 123456700, 123456700 + 310
    s1, q1 = make_read(rng, genome, gstart, p1, n, e1, False, (12,))
    s2, q2 = make_read(rng, genome, gstart, p2, n, e2, True, (0, 140))
    kw = dict(genome_start=gstart, rname="9_2_200000000", amp=123456, cnt=7, paired=True)
    c1, r1, raw1 = both(s1, q1, genome, p1, n, e1, reverse=False, is_read2=False, mate=(p2, True, e2), **kw)
    c2, r2, raw2 = both(s2, q2, genome, p2, n, e2, reverse=True, is_read2=True, mate=(p1, False, e1), **kw)
    assert r1["cols"] == c1 and r2["cols"] == c2
    direct_checks(c1, r1, raw1, True)
    direct_checks(c2, r2, raw2, True)
    assert c2[5] == "49M1I67M4D26M2I4M" and r2["n_cigar_op"] == 7
    assert len(c1[3]) == 9 and r1["tlen"] > 0 and r2["tlen"] == -r1["tlen"]
    assert (r1["flag"], r2["flag"]) == (99, 147)
    assert r1["next_pos"] == r2["pos"] and r2["next_pos"] == r1["pos"]


@pytest.mark.parametrize("pos0,reverse,level", [(16384 - 70, False, 17), (3 * 16384 + 80, True, 17), (131072 - 100, False, 20), (9 * 131072 + 20, True, 20)],
                         ids=["16k_forward", "16k_reverse", "128k_forward", "128k_reverse"])
def test_bin_of_a_read_across_a_bin_boundary(pos0, reverse, level):
    """A read across a 16 Kb boundary lies in a 128 Kb bin (585 ...), one across a 128 Kb boundary in a 1 Mb bin (73 ...)."""
    rng = random.Random(pos0)
    gstart = pos0 - 400
    genome = "".join(rng.choice("ACGT") for _ in range(800))
    events = [(30, 1, 2), (90, 0, 1)]
    seq, qual = make_read(rng, genome, gstart, pos0, 150, events, reverse)
    cols, rec, raw = both(seq, qual, genome, pos0, 150, events, reverse=reverse, genome_start=gstart)
    assert rec["cols"] == cols
    beg, end = rec["pos"], rec["pos"] + rec["span"]
    small = 14 if level == 17 else 17
    assert beg >> small != (end - 1) >> small and beg >> level == (end - 1) >> level
    first = {17: 585, 20: 73}[level]
    assert rec["bin"] == reg2bin(beg, end) == first + (beg >> level)


def test_qualities_are_phred_bytes_reversed_with_the_read():
    rng = random.Random(9)
    genome = "".join(rng.choice("ACGT") for _ in range(400))
    qual = "!~" + "".join(chr(33 + i % 94) for i in range(149))
    for reverse in (False, True):
        pos0 = 300 if reverse else 100
        seq, _ = make_read(rng, genome, 0, pos0, 151, [], reverse)
        cols, rec, raw = both(seq, qual, genome, pos0, 151, [], reverse=reverse)
        assert rec["cols"] == cols
        want = bytes(ord(c) - 33 for c in qual)
        assert rec["raw_qual"] == (want[::-1] if reverse else want)
        assert (rec["raw_qual"][-1], rec["raw_qual"][-2]) == (0, 93) if reverse else (rec["raw_qual"][0], rec["raw_qual"][1]) == (0, 93)
        assert rec["l_seq"] == 151 and rec["seq_bytes"][-1] & 15 == 0       # odd length: the last nibble is padding
        packed = (revcomp(seq) if reverse else seq)
        assert [b >> 4 for b in rec["seq_bytes"]] == [{"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}[c] for c in packed[0::2]]
        nm = struct.unpack_from("<i", raw, raw.index(b"NMi") + 3)[0]
        assert raw[raw.index(b"NMi") + 7:raw.index(b"NMi") + 10] == b"MDZ" and "NM:i:%d" % nm == cols[11]


def _raw_probe(fn, seq, qual, genome, pos0, n, events, out, cap):
    L = scssim_amd.load_library()
    f = getattr(L, fn)
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int,
                  C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int64, C.c_uint64,
                  C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    ev = (C.c_int32 * max(1, 3 * len(events)))(*[int(v) for e in events for v in e])
    size = C.c_size_t(0)
    rc = f(0, 0, 0, 1, b"chr", n, pos0, 0, ev, len(events), 0, 0, None, 0, seq.encode(), qual.encode(), len(seq), genome.encode(), 0, len(genome), out, cap, C.byref(size))
    return rc, size.value


def test_probe_refuses_what_the_sam_probe_refuses():
    g = "ACGT" * 100
    bad = [("A" * 149, 10, 150, []),                              # SEQ shorter than the events make the read
           ("A" * 150, 10, 150, [(20, 1, 1), (10, 0, 1)]),        # events out of order
           ("A" * 150, 300, 150, []),                             # the read runs off the genome given
           ("A" * 150, 10, 150, [(20, 1, 0)])]                    # an event of no length
    for seq, pos0, n, events in bad:
        codes = [_raw_probe(fn, seq, "I" * len(seq), g, pos0, n, events, None, 0)[0] for fn in ("scs_truth_record_probe", "scs_truth_bam_record_probe")]
        assert codes == [scssim_amd.SCS_EINVAL] * 2, (seq[:4], pos0, events, codes)
        with pytest.raises(scssim_amd.ScsError):
            scssim_amd.truth_bam_record_probe(seq, "I" * len(seq), g, pos0, n, events)
    # the size query, a short cap, an exact cap
    seq, qual = g[10:160], "I" * 150
    rc, size = _raw_probe("scs_truth_bam_record_probe", seq, qual, g, 10, 150, [], None, 0)
    assert rc == 0 and size == 36 + 4 + 4 + 75 + 150 + 7 + 3 + 4          # head, "0#1\0", 150M, SEQ, QUAL, NM, MD:Z:150\0
    buf = C.create_string_buffer(size)
    rc, need = _raw_probe("scs_truth_bam_record_probe", seq, qual, g, 10, 150, [], buf, size - 1)
    assert rc == scssim_amd.SCS_EOVERFLOW and need == size
    rc, got = _raw_probe("scs_truth_bam_record_probe", seq, qual, g, 10, 150, [], buf, size)
    assert rc == 0 and got == size and buf.raw == scssim_amd.truth_bam_record_probe(seq, qual, g, 10, 150)
    assert _raw_probe("scs_truth_record_probe", seq, qual, g, 10, 150, [], buf, 5)[0] == scssim_amd.SCS_EOVERFLOW


def test_cli_lists_truth_bam():
    r = subprocess.run([CLI, "genreads", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--truth-bam <string>" in r.stderr and "--truth <string>" in r.stderr


@pytest.mark.parametrize("extra,msg", [(["--truth", "t.sam"], "--truth and --truth-bam"), (["--writers", "3"], "--writers 1"), (["--gpus", "2"], "--gpus 1")],
                         ids=["with_truth", "writers_3", "gpus_2"])
def test_cli_refuses_truth_bam_with_sam_parts_or_shards(extra, msg, tmp_path):
    # the inputs do not exist: a run that got as far as opening the GPU or a file would say something else
    if extra[0] == "--truth":
        extra = ["--truth", str(tmp_path / "t.sam")]
    r = subprocess.run([CLI, "genreads", "-i", str(tmp_path / "none.fa"), "-m", str(tmp_path / "none.profile"), "-o", str(tmp_path / "o"),
                        "--truth-bam", str(tmp_path / "t.bam")] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert len(r.stderr.strip().splitlines()) == 1 and msg in r.stderr and "--truth-bam" in r.stderr
    assert not os.path.exists(tmp_path / "t.bam") and not os.path.exists(tmp_path / "t.sam")
