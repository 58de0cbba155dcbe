"""Host-side tests of the amplicon table (scs_amplicon_places / scs_write_amplicons): one amplicon's line through the functions the
kernels run (scs_amp.h, by way of scs_amplicon_line_probe) against the restatement of tests/amp_cases.py, which builds the
sequences as oracle/scs_oracle.cpp does; the exported symbols; the CLI's refusals.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SEAMS_LIB
from amp_cases import COMP, amplicon_line, codes, frag_template, full_sequence

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")

# three records: 1000, 2000 and 100200 bases; an N block in the second; the genome index of each record's first base
REC_LENS = [1000, 2000, 100200]
REC_OFF = [0, 1000, 3000]
NAMES = ["20_1_1000", "20_2_2000", "21_1_100200"]


def _genome():
    rng = np.random.default_rng(5)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, sum(REC_LENS))].copy()
    g[1000 + 700:1000 + 760] = ord("N")
    return g.tobytes().decode()


GENOME = _genome()
G = codes(GENOME)


def other(c, k=1):
    return int((c + k) % 4)


def semi_err_at(semi, full, t):
    """the semi's error position whose base lands on the full's base t (t = l - 1 - s2 - pos)"""
    return semi[1] - 1 - full[0] - t


def unpatched(frag, semi, full):
    return full_sequence(*frag_template(G, *frag), (semi[0], semi[1], []), (full[0], full[1], []))[0]


def _cases():
    """name, record, fragment (offset inside the record, length, strand), semi (spos, len), full (spos, len), and a function that
    gives the two error lists from the unpatched sequence U."""
    out = []

    def add(name, rec, frag, semi, full, errs=lambda U, semi, full: ([], [])):
        fr = (REC_OFF[rec] + frag[0], frag[1], frag[2])
        e1, e2 = errs(unpatched(fr, semi, full), semi, full)
        out.append((name, rec, fr, (semi[0], semi[1], e1), (full[0], full[1], e2)))

    for strand in (1, -1):
        sg = "plus" if strand == 1 else "minus"
        add("no_errors_" + sg, 0, (100, 600, strand), (50, 400), (30, 300))
        add("one_full_error_" + sg, 0, (100, 600, strand), (50, 400), (30, 300), lambda U, s, f: ([], [(17, other(U[17]))]))
        add("four_inline_" + sg, 0, (100, 600, strand), (50, 400), (30, 300),
            lambda U, s, f: ([(semi_err_at(s, f, t), int(COMP[other(U[t])])) for t in (5, 90, 91, 250)], [(t, other(U[t], 2)) for t in (8, 100, 200, 299)]))
        add("overflow_5_" + sg, 1, (200, 900, strand), (100, 700), (50, 600),
            lambda U, s, f: ([(semi_err_at(s, f, t), int(COMP[other(U[t])])) for t in (0, 10, 20, 30, 599)], [(t, other(U[t], 3)) for t in (1, 11, 21, 31, 598)]))
        add("overflow_40_" + sg, 2, (50000, 3000, strand), (400, 2000), (100, 1800),
            lambda U, s, f: ([(semi_err_at(s, f, t), int(COMP[other(U[t])])) for t in range(3, 1800, 45)], [(t, other(U[t], 2)) for t in range(7, 1800, 45)]))
        # a semi error just outside and just inside each end of the full's window: t = -1, 0, len - 1, len
        add("semi_error_at_the_window_ends_" + sg, 1, (100, 800, strand), (60, 500), (40, 300),
            lambda U, s, f: ([(semi_err_at(s, f, t), 2) for t in (-1, 300)] + [(semi_err_at(s, f, t), int(COMP[other(U[t])])) for t in (0, 299)], []))
        add("semi_and_full_error_on_one_base_" + sg, 0, (100, 600, strand), (50, 400), (30, 300),
            lambda U, s, f: ([(semi_err_at(s, f, 77), int(COMP[other(U[77])]))], [(77, other(U[77], 2))]))
        add("full_error_restores_the_genome_" + sg, 0, (100, 600, strand), (50, 400), (30, 300),
            lambda U, s, f: ([(semi_err_at(s, f, 77), int(COMP[other(U[77])])), (semi_err_at(s, f, 120), int(COMP[other(U[120])]))], [(77, int(U[77]))]))
        add("error_on_an_N_" + sg, 1, (400, 900, strand), (100, 700), (50, 600),
            lambda U, s, f: ([(semi_err_at(s, f, int(np.nonzero(U == 4)[0][3])), 1)], [(int(np.nonzero(U == 4)[0][20]), 2), (int(np.nonzero(U == 4)[0][-1]), 0)]))
    # (an error on an amplicon's own base 0 is the semi's: the packed entry of position 0, base A is the empty slot, and the
    # amplification draws no error on the first 8 bases of a new amplicon)
    # the record's first and last base: strand +1 gives a '+' amplicon at frag + flen - s - l + s2, strand -1 a '-' one at frag + s + l - s2 - l2
    add("starts_at_record_coordinate_0_plus", 1, (0, 500, 1), (100, 400), (0, 300), lambda U, s, f: ([(semi_err_at(s, f, 0), int(COMP[other(U[0])]))], []))
    add("starts_at_record_coordinate_0_minus", 1, (0, 500, -1), (0, 400), (100, 300), lambda U, s, f: ([], [(299, other(U[299]))]))
    add("ends_on_the_last_base_plus", 1, (1500, 500, 1), (0, 400), (100, 300), lambda U, s, f: ([], [(299, other(U[299]))]))
    add("ends_on_the_last_base_minus", 1, (1500, 500, -1), (100, 400), (0, 300), lambda U, s, f: ([(semi_err_at(s, f, 0), int(COMP[other(U[0])]))], []))
    add("last_record_ends_on_the_genome_end_minus", 2, (100200 - 700, 700, -1), (200, 500), (0, 400), lambda U, s, f: ([(semi_err_at(s, f, 0), int(COMP[other(U[0])]))], []))
    # digits: an amplicon [9, 309) with edits at 9 and 10; one over 99999 -> 100000
    add("digits_9_to_10", 0, (9, 500, 1), (200, 300), (0, 300), lambda U, s, f: ([(semi_err_at(s, f, 0), int(COMP[other(U[0])]))], [(1, other(U[1]))]))
    add("digits_99999_to_100000", 2, (99990, 200, -1), (0, 150), (50, 100),
        lambda U, s, f: ([(semi_err_at(s, f, 99 - 9), int(COMP[other(U[99 - 9])]))], [(99 - 10, other(U[99 - 10]))]))
    return out


CASES = _cases()


def probe(case, **kw):
    name, rec, frag, semi, full = case
    a = dict(genome=GENOME, genome_start=0, rec_off=REC_OFF[rec], rec_len=REC_LENS[rec], rec_name=NAMES[rec], index=123456, reads=6, semi_index=4321)
    a.update(kw)
    return scssim_amd.amplicon_line_probe(frag, semi, full, **a)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_line_equals_the_restatement(case):
    name, rec, frag, semi, full = case
    want = amplicon_line(G, frag, semi, full, REC_OFF[rec], NAMES[rec], 123456, 6, 4321)
    assert probe(case) == want
    f = want.rstrip("\n").split("\t")
    assert f[4] == ("+" if frag[2] == 1 else "-") and int(f[2]) - int(f[1]) == full[1]
    # a window of the genome that just covers the amplicon gives the same line
    lo = REC_OFF[rec] + int(f[1])
    assert probe(case, genome=GENOME[lo:lo + full[1]], genome_start=lo) == want


def test_the_case_table_reaches_what_it_names():
    lines = {c[0]: probe(c).rstrip("\n").split("\t") for c in CASES}
    edits = {k: ([] if v[7] == "." else v[7].split(",")) for k, v in lines.items()}
    for sg in ("plus", "minus"):
        assert edits["no_errors_" + sg] == [] and len(edits["one_full_error_" + sg]) == 1
        assert len(edits["four_inline_" + sg]) == 8 and len(edits["overflow_5_" + sg]) == 10 and len(edits["overflow_40_" + sg]) == 80
        assert len(edits["semi_error_at_the_window_ends_" + sg]) == 2              # the two inside; the two outside are not the amplicon's
        assert len(edits["semi_and_full_error_on_one_base_" + sg]) == 1
        assert len(edits["full_error_restores_the_genome_" + sg]) == 1             # only the second semi error is left
        assert [e.split(":")[1][0] for e in edits["error_on_an_N_" + sg]] == ["N", "N", "N"]
        for k in ("four_inline_", "overflow_40_"):
            pos = [int(e.split(":")[0]) for e in edits[k + sg]]
            assert pos == sorted(set(pos))
    assert lines["starts_at_record_coordinate_0_plus"][1] == lines["starts_at_record_coordinate_0_minus"][1] == "0"
    assert edits["starts_at_record_coordinate_0_plus"][0].startswith("0:") and edits["starts_at_record_coordinate_0_minus"][0].startswith("0:")
    assert lines["ends_on_the_last_base_plus"][2] == lines["ends_on_the_last_base_minus"][2] == "2000"
    assert edits["ends_on_the_last_base_plus"][0].startswith("1999:") and edits["ends_on_the_last_base_minus"][0].startswith("1999:")
    assert lines["last_record_ends_on_the_genome_end_minus"][2] == "100200"
    assert lines["digits_9_to_10"][1] == "9" and [e.split(":")[0] for e in edits["digits_9_to_10"]] == ["9", "10"]
    assert [e.split(":")[0] for e in edits["digits_99999_to_100000"]] == ["99999", "100000"]
    assert int(lines["digits_99999_to_100000"][1]) < 99999 < 100000 < int(lines["digits_99999_to_100000"][2])


@pytest.mark.parametrize("what", ["semi_beyond_the_fragment", "full_beyond_the_semi", "fragment_over_the_record_end", "genome_does_not_cover", "error_beyond_the_amplicon"])
def test_a_lineage_that_does_not_fit_is_refused(what):
    frag, semi, full, kw = (REC_OFF[1] + 100, 600, -1), (50, 400, []), (30, 300, []), {}
    if what == "semi_beyond_the_fragment":
        semi = (250, 400, [])
    elif what == "full_beyond_the_semi":
        full = (101, 300, [])
    elif what == "fragment_over_the_record_end":
        frag = (REC_OFF[1] + 1500, 600, -1)
    elif what == "genome_does_not_cover":
        kw = dict(genome=GENOME[1000:1400], genome_start=1000)
    else:
        full = (30, 300, [(300, 1)])
    with pytest.raises(ScsError) as e:
        probe((what, 1, frag, semi, full), **kw)
    assert e.value.code == SCS_EINVAL


def test_both_libraries_export_the_amplicon_abi():
    want = {"scs_amplicon_places", "scs_write_amplicons", "scs_amplicon_line_probe", "scs_amplicon_kernel_time"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    assert len(scssim_amd.GenReads.KERNELS) == 8            # the table's kernels have no slot of scs_kernel_time


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--amplicons with --gpus 2, and --amplicons without a file name, end the CLI with a message before it touches a device (this
    machine may have none) or an input file (these do not exist)."""
    r = _cli(["--amplicons", "/nonexistent/a.tsv", "--gpus", "2"])
    assert r.returncode != 0 and "--amplicons needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--amplicons"])
    assert r.returncode != 0 and "amplicons" in r.stderr and "requires an argument" in r.stderr, r.stderr
    r = _cli(["--amplicons", ""])
    assert r.returncode != 0 and "--amplicons needs the name of the file" in r.stderr, r.stderr
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--amplicons <string>" in h.stdout + h.stderr
