"""Host-side tests of the coverage profile (scs_set_coverage): the function the per-batch kernel runs on one placed read, through
its host probe, against the intervals that POS and CIGAR give (tests/coverage_cases.py); the summary function of the file against
numpy on per-base arrays; the CLI's options and their refusals; the ABI surface.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEAMS_LIB

import coverage_cases as cc
import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
REC_LEN = 100000

EVENTS = [
    # name, n, events (window position, deletion?, length)
    ("no_events", 150, []),
    ("insertion_at_0", 150, [(0, 0, 2)]),
    ("insertion_at_n_minus_1", 150, [(149, 0, 3)]),
    ("leading_deletion", 150, [(0, 1, 4)]),
    ("trailing_deletion", 150, [(146, 1, 4)]),
    ("deletion_of_30", 150, [(60, 1, 30)]),
    ("two_deletions_insertion_between", 150, [(20, 1, 5), (70, 0, 4), (110, 1, 12)]),
    ("rollback_51", 51, [(10, 1, 2)]),
]


def starts(n, reverse):
    """pos0 of a window whose leftmost base is the record's first, whose rightmost is its last, and one in the middle."""
    return [l + n - 1 if reverse else l for l in (0, REC_LEN - n, 41234)]


@pytest.mark.parametrize("name,n,events", EVENTS, ids=[e[0] for e in EVENTS])
def test_read_marks_the_runs_of_pos_and_cigar(name, n, events):
    """cov_read (what k_cov_mark runs per read) marks the maximal runs of M-aligned genome bases: their lengths add up to the
    CIGAR's M lengths, an insertion does not split a run, a deletion does; both strands; at the record's two ends and inside."""
    for reverse in (False, True):
        for pos0 in starts(n, reverse):
            pos, cigar = cc.pos_cigar(pos0, n, events, reverse)
            want = cc.intervals(pos, cigar)
            got = scssim_amd.coverage_read_probe(pos0, n, events, reverse, rec_len=REC_LEN)
            assert got == want, (name, reverse, pos0, cigar)
            assert sum(e - s for s, e in got) == cc.m_length(cigar)
            assert len(got) == 1 + sum(1 for l, k in cc.CIG.findall(cigar) if k == "D")
            assert got[0][0] == pos and 0 <= got[0][0] and got[-1][1] <= REC_LEN
    if name == "no_events":
        assert scssim_amd.coverage_read_probe(REC_LEN - 150, 150, [], False, rec_len=REC_LEN) == [(REC_LEN - 150, REC_LEN)]   # the genome's last base: entry G
    if name in ("insertion_at_0", "insertion_at_n_minus_1"):
        assert "I" in cc.pos_cigar(5000, n, events, False)[1] and len(scssim_amd.coverage_read_probe(5000, n, events, False, rec_len=REC_LEN)) == 1
    if name == "two_deletions_insertion_between":
        assert cc.pos_cigar(1000, n, events, False)[1] == "20M5D46M4I39M12D28M"
        assert scssim_amd.coverage_read_probe(1000, n, events, False, rec_len=REC_LEN) == [(1000, 1020), (1025, 1110), (1122, 1150)]
    if name == "rollback_51":
        assert cc.pos_cigar(0, n, events, False)[1] == "51M" and scssim_amd.coverage_read_probe(0, n, events, False, rec_len=REC_LEN) == [(0, 51)]
    if name == "leading_deletion":
        assert scssim_amd.coverage_read_probe(1000, n, events, False, rec_len=REC_LEN) == [(1004, 1150)]
        assert scssim_amd.coverage_read_probe(1149, n, events, True, rec_len=REC_LEN) == [(1000, 1146)]


def test_reads_outside_the_record_and_bad_event_lists_are_refused():
    for pos0, rev in ((REC_LEN - 149, False), (148, True), (-1, False)):
        with pytest.raises(ScsError) as e:
            scssim_amd.coverage_read_probe(pos0, 150, [], rev, rec_len=REC_LEN)
        assert e.value.code == SCS_EINVAL
    for events in ([(10, 0, 1), (5, 1, 2)], [(148, 1, 5)], [(3, 0, 0)], [(i * 4, 0, 1) for i in range(33)]):   # out of order, past the window, empty, 33 events
        with pytest.raises(ScsError) as e:
            scssim_amd.coverage_read_probe(5000, 150, events, False, rec_len=REC_LEN)
        assert e.value.code == SCS_EINVAL


def _arrays():
    rng = np.random.default_rng(5)
    heavy = np.minimum((rng.pareto(1.2, 20000) * 8).astype(np.int64), 60000)
    one = np.zeros(5000, np.int64); one[1234] = 777
    return dict(all_zero=np.zeros(3000, np.int64), constant=np.full(3000, 17, np.int64), one_deep=one,
                poisson=rng.poisson(30.0, 20000).astype(np.int64), heavy_tail=heavy)


ARRAYS = _arrays()
# both sides sum at most D + 1 float64 terms of the same integers: (D + 1) 2^-52 relative to quantities of at most 1 (fractions, 1 - gini), rounded up
TOL = 1e-10


@pytest.mark.parametrize("which", sorted(ARRAYS))
@pytest.mark.parametrize("side", ["above", "below"])
def test_summary_against_numpy_on_per_base_arrays(which, side):
    """cov_stats (what scs_write_coverage runs) from a histogram row and its exact sum against numpy on the per-base depths: with
    max_depth above the maximum (exact: the Gini is that of the depths) and below it (the top bucket at its mean depth)."""
    d = ARRAYS[which]
    mx = int(d.max())
    D = mx + 3 if side == "above" else max(1, mx // 2)
    hist = np.bincount(np.minimum(d, D), minlength=D + 1)
    got = scssim_amd.coverage_stats_probe(hist, int(d.sum()))
    want = cc.stats_from_depths(d, D)
    assert got["mean"] == pytest.approx(want["mean"], rel=TOL, abs=TOL)
    assert got["breadth"] == pytest.approx(want["breadth"], rel=TOL, abs=TOL)
    assert got["gini"] == pytest.approx(want["gini"], rel=TOL, abs=TOL)
    if which in ("all_zero", "constant"):
        assert got["gini"] == pytest.approx(0.0, abs=TOL)
    if which == "all_zero":
        assert got["mean"] == 0.0 and got["breadth"] == (0.0, 0.0, 0.0, 0.0)
    if which == "one_deep":
        assert got["gini"] == pytest.approx(1.0 - 1.0 / d.size, abs=TOL) and got["breadth"][0] == pytest.approx(1.0 / d.size)
    if side == "above" and d.sum():
        sub = d[:1500]                                      # the definition, where n^2 terms are affordable
        h2 = np.bincount(sub, minlength=D + 1)
        if sub.sum():
            assert scssim_amd.coverage_stats_probe(h2, int(sub.sum()))["gini"] == pytest.approx(cc.gini_pairwise(sub), abs=1e-9)
    if side == "below" and which in ("poisson", "heavy_tail"):
        exact = cc.stats_from_depths(d, mx + 1)["gini"]
        assert got["gini"] < exact                          # a lower bound once bases reach max_depth


def test_summary_of_a_row_without_bases_is_all_zero():
    got = scssim_amd.coverage_stats_probe(np.zeros(11, np.uint64), 0)
    assert got == dict(mean=0.0, breadth=(0.0, 0.0, 0.0, 0.0), gini=0.0)


def test_breadth_thresholds_above_max_depth_count_the_top_bucket():
    d = np.array([0, 0, 1, 2, 3, 9, 30], np.int64)
    got = scssim_amd.coverage_stats_probe(np.bincount(np.minimum(d, 3), minlength=4), int(d.sum()))
    assert got["breadth"] == pytest.approx((5 / 7, 3 / 7, 3 / 7, 3 / 7))


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--coverage-max without --coverage-profile, values outside 1 .. 65535 and --coverage-profile with --gpus 2 end the CLI with
    their own message before it touches a device (this machine has none) or an input file (these do not exist).  -c / --coverage
    stays the sequencing coverage."""
    r = _cli(["--coverage-max", "500"])
    assert r.returncode != 0 and "--coverage-max needs --coverage-profile" in r.stderr, r.stderr
    for v in ("0", "65536", "-3", "x"):
        r = _cli(["--coverage-profile", "/nonexistent/c.txt", "--coverage-max", v])
        assert r.returncode != 0 and "--coverage-max should be an integer in 1~65535" in r.stderr, (v, r.stderr)
    r = _cli(["--coverage-profile", "/nonexistent/c.txt", "--gpus", "2"])
    assert r.returncode != 0 and "--coverage-profile needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--coverage", "0"])
    assert r.returncode != 0 and "sequencing coverage not properly specified" in r.stderr, r.stderr
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--coverage-profile <string>" in h.stdout + h.stderr and "--coverage-max <int>" in h.stdout + h.stderr and "-c, --coverage <float>" in h.stdout + h.stderr


def test_both_libraries_export_the_coverage_abi_and_the_product_reads_no_seam():
    want = {"scs_set_coverage", "scs_coverage_shape", "scs_download_coverage", "scs_coverage_range", "scs_write_coverage", "scs_coverage_kernel_time",
            "scs_coverage_read_probe", "scs_coverage_stats_probe", "scs_coverage_finish_probe", "scs_coverage_tile"}
    product = os.path.join(ROOT, "scssim_amd", "libscssim_hip.so")
    for lib in (product, SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    # SCS_TEST_COV_LDS set in the environment: the product library answers "unset", the seams build hands the value through
    code = "import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.scs_test_seam.restype = ctypes.c_char_p; L.scs_test_seam.argtypes = [ctypes.c_char_p]; print((L.scs_test_seam(b'SCS_TEST_COV_LDS') or b'<unset>').decode())"
    seen = [subprocess.run([sys.executable, "-c", code, lib], env=dict(os.environ, SCS_TEST_COV_LDS="4"), capture_output=True, text=True).stdout.strip() for lib in (product, SEAMS_LIB)]
    assert seen == ["<unset>", "4"]
    assert "SCS_TEST_COV_LDS" in open(os.path.join(ROOT, "scssim_amd", "csrc", "scs_seams.h")).read()
    assert "k_depth" in scssim_amd.GenReads.KERNELS and len(scssim_amd.GenReads.KERNELS) == 8     # scs_kernel_time's table is not extended


def test_tile_query():
    tile, chunk = scssim_amd.coverage_tile()
    assert tile > 0 and chunk > 0 and tile % 4 == 0
