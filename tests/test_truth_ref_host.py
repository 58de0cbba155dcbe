"""Host tests of the truth SAM on the original reference (scs_set_truth_ref_sam, `scssim genreads --lift --truth-ref`; DESIGN.md
section 17).  No GPU.  The formatter the kernels run (scs_truth_ref.h, through scs_truth_ref_record_probe) against a restatement
written a different way (tests/truth_ref_cases.py: base by base, numpy.searchsorted per haplotype position, blocks and clips from
the column list), over the event lists of tests/test_depth_host.py, both strands, SE and both mates of PE, one-segment and mixed
layouts; the worked examples of the contract as literal strings; the exported symbols; the CLI's refusals; the stand-alone
sanitizer program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_depth_host import EVENTS, pos_cigar, window_bases
from truth_ref_cases import Table, lift_line

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
COMP = str.maketrans("ACGT", "TGCA")
ALL_EVENTS = EVENTS + [("plain_100", 100, [])]


def table(segs, hap_lens, ref_lens, hap_names=None, ref_names=("chrA", "chrB")):
    """segs: (kind 'R' / 'I', bases, reference record, reference start) in haplotype order."""
    off = np.concatenate([[0], np.cumsum([s[1] for s in segs])])[:-1]
    assert sum(s[1] for s in segs) == sum(hap_lens)
    return Table(off, [s[1] for s in segs], [s[3] for s in segs], [s[2] for s in segs], [0 if s[0] == "R" else 1 for s in segs],
                 ref_names[:len(ref_lens)], ref_lens, hap_names or ["h%d" % (i + 1) for i in range(len(hap_lens))], hap_lens)


# name -> (table, read starts (global index of the leftmost window base), pairs of starts for PE)
LAYOUTS = {
    "one_segment": (table([("R", 5000, 0, 0)], [5000], [5000]), [0, 1234, 4850], [(100, 400), (700, 700)]),
    # the worked example: R[100, 200) at 0, I of 8 at 100, R[210, ...) at 108
    "worked_r_i_r": (table([("R", 100, 0, 100), ("I", 8, 0, 200), ("R", 2000, 0, 210)], [2108], [3000]), [50, 0, 8, 95, 100, 104, 108], [(50, 300), (100, 20)]),
    # insertions under the first and the last base, a read wholly in an insertion (mapped and unmapped mate), a deletion that
    # swallows the whole I segment (starts 340 with the event list deletion_over_a_boundary: window bases 60 .. 89)
    "mixed": (table([("R", 400, 0, 1000), ("I", 30, 0, 1400), ("R", 1000, 0, 1425), ("I", 200, 0, 2425), ("R", 575, 0, 2425)], [2205], [3000]),
              [300, 400, 415, 270, 340, 335, 330, 1440, 1400, 1300, 1560, 1629], [(1440, 600), (600, 1440), (1440, 1450), (300, 1300), (1300, 270)]),
    # tandem copies (a backwards jump): 60/40, 40/60, 50/50 with 100 bases; 90/60, 60/90, 75/75 with 150; a deletion across the cut (930)
    "tandem": (table([("R", 1000, 0, 1000), ("R", 1000, 0, 1000), ("R", 1000, 0, 1000), ("R", 500, 0, 2000)], [3500], [2500]),
               [940, 960, 950, 910, 925, 930, 1850, 2900], [(940, 1960), (960, 200), (950, 950)]),
    # three blocks: 40 / 60 / 50 bases of a read at 460
    "three_blocks": (table([("R", 500, 0, 500), ("R", 60, 0, 940), ("R", 1060, 0, 940)], [1620], [2000]), [460, 440, 495, 380], [(460, 700), (100, 460)]),
    # a collinear junction with a gap (a planted deletion of 40 bases): a sequencing deletion across it gives one merged D (930)
    "collinear_gap": (table([("R", 1000, 0, 0), ("R", 1960, 0, 1040)], [2960], [3000]), [930, 900, 999, 1000, 850], [(930, 1100), (1100, 900)]),
    # a junction into another reference record: RNEXT by name, TLEN 0
    "other_record": (table([("R", 1000, 0, 0), ("R", 1000, 1, 100)], [2000], [1000, 1100]), [900, 960, 925, 100, 1200], [(100, 1200), (1200, 100), (900, 960), (960, 1500)]),
    # two staged records: POS and YH / YP are the second record's own
    "two_records": (table([("R", 3000, 0, 0), ("R", 1000, 0, 0), ("I", 50, 0, 1000), ("R", 1950, 0, 1050)], [3000, 3000], [3000]), [3000, 3900, 3920, 3990, 5850, 100], [(3900, 4200), (100, 500)]),
}


def hap_record(t, start, n, events, reverse, flag, rng):
    """The haplotype SAM record of a read whose window covers [start, start + n), restated by tests/test_depth_host.py: its
    fields (as _sam splits them), and the probe's arguments for it."""
    pos0 = start + n - 1 if reverse else start
    lo, cigar = pos_cigar(pos0, n, events, reverse)
    qlen = len(window_bases(n, events))
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, qlen)); qual = "".join(chr(35 + i) for i in rng.integers(0, 40, qlen))
    ends = np.cumsum(t.hap_lens); r = int(np.searchsorted(ends, lo, side="right"))
    fields = ["7#3", str(flag | (0x10 if reverse else 0)), t.hap_names[r], str(lo - (ends[r] - t.hap_lens[r]) + 1), "255", cigar, "*", "0", "0",
              seq.translate(COMP)[::-1] if reverse else seq, qual[::-1] if reverse else qual]
    return fields, dict(seq=seq, qual=qual, pos0=pos0, n=n, events=events, reverse=reverse)


def probe(t, a, mate=None, is_read2=False):
    return scssim_amd.truth_ref_record_probe(t, t.hap_lens, t.ref_lens, t.ref_names, a["seq"], a["qual"], a["pos0"], a["n"], a["events"], a["reverse"], hap_names=t.hap_names,
                                             amp=7, cnt=3, paired=mate is not None, is_read2=is_read2,
                                             mate=(mate["pos0"], mate["reverse"], mate["events"]) if mate is not None else None)


def grid_cases(layout):
    """(read, mate or None, is_read2, the restatement's line) over the event lists, both strands, SE and both mates of PE (read 1
    forward / read 2 reverse and the other way round, the mate with the next event list of its window length)."""
    t, starts, pairs = LAYOUTS[layout]
    rng = np.random.default_rng(len(layout))
    total, ends = sum(t.hap_lens), np.cumsum(t.hap_lens)
    for name, n, events in ALL_EVENTS:
        same_n = [e for e in ALL_EVENTS if e[1] == n]                                  # (a pair shares its window length)
        events2 = same_n[(same_n.index((name, n, events)) + 1) % len(same_n)][2]
        for reverse in (False, True):
            for s in starts:
                if s + n > total or np.searchsorted(ends, s, side="right") != np.searchsorted(ends, s + n - 1, side="right"):
                    continue
                rec, a = hap_record(t, s, n, events, reverse, 0, rng)
                yield a, None, False, lift_line(t, rec, None)
            for s1, s2 in pairs:
                if max(s1, s2) + n > total:
                    continue
                r1, a1 = hap_record(t, s1, n, events, reverse, 0x43 | (0 if reverse else 0x20), rng)
                r2, a2 = hap_record(t, s2, n, events2, not reverse, 0x83 | (0x20 if reverse else 0), rng)
                yield a1, a2, False, lift_line(t, r1, r2)
                yield a2, a1, True, lift_line(t, r2, r1)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_probe_equals_the_restatement(layout):
    """1: every line of the grid byte for byte."""
    n_lines = 0
    for a, mate, is_read2, want in grid_cases(layout):
        assert probe(LAYOUTS[layout][0], a, mate, is_read2) == want, (layout, a, mate, is_read2)
        n_lines += 1
    assert n_lines > 60


def host_check_rows():
    """The grid as the input lines of tools/truth_ref_host_check.cpp."""
    rows = []
    ev = lambda a: "%d %s" % (len(a["events"]), " ".join("%d %d %d" % e for e in a["events"]))
    for k, layout in enumerate(LAYOUTS):
        t = LAYOUTS[layout][0]
        rows.append("table %d %d %d %d %s %s %s %s %s" % (k, len(t), len(t.hap_lens), len(t.ref_lens),
                    " ".join("%d %d %d %d %d" % x for x in zip(t.hap_off, t.len, t.ref_pos, t.ref_rec, t.kind)),
                    " ".join(map(str, t.hap_lens)), " ".join(map(str, t.ref_lens)), " ".join(t.ref_names), " ".join(t.hap_names)))
        for a, mate, is_read2, want in grid_cases(layout):
            m = mate or dict(pos0=0, reverse=False, events=[])
            rows.append("read %d %d %d %d %d %d %s %d %d %s %s %s %s" % (k, mate is not None, is_read2, a["n"], a["pos0"], a["reverse"], ev(a), m["pos0"], m["reverse"], ev(m),
                        a["seq"], a["qual"], want.rstrip("\n").replace("\t", "|")))
    return rows


def _line(t, start, n=100, events=(), reverse=False):
    rec, a = hap_record(t, start, n, list(events), reverse, 0, np.random.default_rng(1))
    got = probe(t, a)
    assert got == lift_line(t, rec, None)
    f = got.rstrip("\n").split("\t")
    return int(f[3]), f[5], f[13], f


def test_worked_examples_and_named_cases():
    """The contract's worked examples and the named cases of the grid, as literal values (they anchor the restatement too)."""
    t = LAYOUTS["worked_r_i_r"][0]
    assert _line(t, 50)[:3] == (151, "50M8I10D42M", "YB:i:1")
    t = LAYOUTS["tandem"][0]
    assert _line(t, 940)[:3] == (1941, "60M40S", "YB:i:2")
    assert _line(t, 960)[:3] == (1001, "40S60M", "YB:i:2")
    assert _line(t, 950)[:3] == (1951, "50M50S", "YB:i:2")                              # a tie: the first block
    assert _line(t, 2900, 150)[:3] == (1901, "150M", "YB:i:1")                          # copy 3 runs on into what follows the unit: collinear, no gap
    # a sequencing deletion across a cut: the D at the block's edge is dropped (window bases 60 .. 89 of a read at 930 = 990 .. 1019)
    assert _line(t, 930, 150, [(60, 1, 30)])[:3] == (1931, "60M60S", "YB:i:2")
    assert _line(LAYOUTS["three_blocks"][0], 460, 150)[:3] == (941, "40S60M50S", "YB:i:3")
    # ... across a collinear junction: one merged D (10 bases of the first segment, the gap of 40, 20 of the second)
    assert _line(LAYOUTS["collinear_gap"][0], 930, 150, [(60, 1, 30)])[:3] == (931, "60M70D60M", "YB:i:1")
    t = LAYOUTS["mixed"][0]
    assert _line(t, 340, 150, [(60, 1, 30)])[:3] == (1341, "60M25D60M", "YB:i:1")     # the deletion swallows the whole I segment: only the gap is left
    assert _line(t, 400, 150)[:3] == (1426, "30S120M", "YB:i:1")                        # an insertion under the first base
    assert _line(t, 270, 150)[:3] == (1271, "130M20S", "YB:i:1")                        # ... and under the last one
    pos, cigar, yb, f = _line(t, 1440, 150)                                             # wholly in an insertion
    assert (f[1], f[2], pos, f[4], cigar, f[6], f[7], f[8], yb) == ("4", "*", 0, "0", "*", "*", "0", "0", "YB:i:0")
    assert _line(LAYOUTS["one_segment"][0], 100, 150, [(149, 0, 3)])[1] == "150M3S"     # a sequencing insertion at the read's end
    assert _line(LAYOUTS["one_segment"][0], 100, 150, [(149, 0, 3)], True)[1] == "3S150M"
    pos, cigar, yb, f = _line(LAYOUTS["two_records"][0], 3920, 150)
    assert (f[2], pos, cigar, f[11], f[12]) == ("chrA", 921, "80M50I50D20M", "YH:Z:h2", "YP:i:921")


def test_mate_fields():
    rng = np.random.default_rng(2)
    t = LAYOUTS["mixed"][0]
    r1, a1 = hap_record(t, 1440, 150, [], False, 0x63, rng); r2, a2 = hap_record(t, 600, 150, [], True, 0x93, rng)
    f1, f2 = probe(t, a1, a2, False).split("\t"), probe(t, a2, a1, True).split("\t")
    assert f1[1:9] == [str(0x1 | 0x4 | 0x20 | 0x40), "chrA", "1596", "0", "*", "=", "1596", "0"]       # unmapped: at its mate's place
    assert f2[1:9] == [str(0x1 | 0x8 | 0x10 | 0x80), "chrA", "1596", "255", "150M", "=", "1596", "0"]  # PNEXT: its own POS
    r2, a2 = hap_record(t, 1450, 150, [], True, 0x93, rng)
    f1 = probe(t, a1, a2, False).split("\t")
    assert f1[1:9] == [str(0x1 | 0x4 | 0x8 | 0x20 | 0x40), "*", "0", "0", "*", "*", "0", "0"]
    t = LAYOUTS["other_record"][0]
    r1, a1 = hap_record(t, 100, 150, [], False, 0x63, rng); r2, a2 = hap_record(t, 1200, 150, [], True, 0x93, rng)
    f1, f2 = probe(t, a1, a2, False).split("\t"), probe(t, a2, a1, True).split("\t")
    assert f1[1:9] == [str(0x1 | 0x20 | 0x40), "chrA", "101", "255", "150M", "chrB", "301", "0"]
    assert f2[1:9] == [str(0x1 | 0x10 | 0x80), "chrB", "301", "255", "150M", "chrA", "101", "0"]
    t = LAYOUTS["one_segment"][0]
    r1, a1 = hap_record(t, 700, 150, [], False, 0x63, rng); r2, a2 = hap_record(t, 700, 150, [], True, 0x93, rng)
    assert probe(t, a1, a2, False).split("\t")[8] == "150" and probe(t, a2, a1, True).split("\t")[8] == "-150"   # a tie: + on read 1
    r2, a2 = hap_record(t, 900, 150, [], True, 0x93, rng)
    f1, f2 = probe(t, a1, a2, False).split("\t"), probe(t, a2, a1, True).split("\t")
    assert (f1[1], f1[6:9]) == (str(0x63), ["=", "901", "350"]) and (f2[1], f2[6:9]) == (str(0x93), ["=", "701", "-350"])


def test_a_table_that_lifts_outside_the_reference_is_refused():
    t = table([("R", 1000, 0, 0), ("R", 1000, 0, 1500)], [2000], [2000])
    rng = np.random.default_rng(3)
    rec, a = hap_record(t, 100, 150, [], False, 0, rng)
    assert probe(t, a) == lift_line(t, rec, None)                                       # the first segment alone is fine
    for s in (900, 1200):
        rec, a = hap_record(t, s, 150, [], False, 0, rng)
        with pytest.raises(ValueError, match="3"):
            lift_line(t, rec, None)
        with pytest.raises(ScsError) as e:
            probe(t, a)
        assert e.value.code == SCS_EINVAL and e.value.lift_err == 3
    # a mate that cannot be lifted fails the read's line too; a read outside its record: 1
    r1, a1 = hap_record(t, 100, 150, [], False, 0x63, rng); r2, a2 = hap_record(t, 1200, 150, [], True, 0x93, rng)
    with pytest.raises(ScsError) as e:
        probe(t, a1, a2, False)
    assert e.value.lift_err == 3
    a = dict(a1, pos0=1950)
    with pytest.raises(ScsError) as e:
        probe(t, a)
    assert e.value.code == SCS_EINVAL and e.value.lift_err == 1


@pytest.mark.parametrize("lib", ["libscssim_hip.so", "libscssim_hip_seams.so"])
def test_both_libraries_export_the_new_symbols(lib):
    L = ctypes.CDLL(os.path.join(ROOT, "scssim_amd", lib))
    for sym in ("scs_set_truth_ref_sam", "scs_truth_ref_record_probe"):
        assert getattr(L, sym) is not None


@pytest.mark.parametrize("args,words", [
    (["--truth-ref", "x.sam"], ["--truth-ref", "--lift"]),
    (["--lift", "x.lift", "--truth-ref", "x.sam", "--truth", "y.sam"], ["--truth-ref", "--truth", "one truth output"]),
    (["--lift", "x.lift", "--truth-ref", "x.sam", "--truth-bam", "y.bam"], ["--truth-ref", "--truth-bam", "one truth output"]),
    (["--lift", "x.lift", "--truth-ref", "x.sam", "--gpus", "2"], ["--truth-ref", "--gpus 1"]),
    (["--lift", "x.lift", "--truth-ref", "x.sam", "--writers", "2"], ["--truth-ref", "--writers 1"]),
])
def test_cli_refusals(args, words, tmp_path):
    """Refused before any GPU work (none is here), with the reference's exit status 1; nothing is written."""
    r = subprocess.run([CLI, "genreads", "-i", "none.fa", "-m", "none.profile", "-o", str(tmp_path / "o")] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and all(w in r.stderr for w in words), r.stderr
    assert os.listdir(str(tmp_path)) == []
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--truth-ref <string>" in h.stdout + h.stderr


def test_stand_alone_sanitizer_check():
    """tools/truth_ref_host_check.py: the grid above through scs_truth_ref.h as a stand-alone CPU program under AddressSanitizer and
    UndefinedBehaviorSanitizer; its lines equal the probe's."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "truth_ref_host_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
