"""Host-side tests of the coverage profile on the reference (scs_set_coverage_ref): the ABI surface, the CLI's option and its
refusals, the restatement's own invariants (tests/coverage_ref_cases.py) on the dense layout, and the kernels' case table reaching
the branches it names.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT, SEAMS_LIB

import coverage_ref_cases as rc
import scssim_amd
from lift_cases import write_dense_inputs

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
T = 4096                                                    # COV_TILE (test_the_tile_is_the_one_the_cases_assume)


def test_both_libraries_export_the_abi_and_the_product_reads_no_seam():
    want = {"scs_set_coverage_ref", "scs_coverage_ref_shape", "scs_download_coverage_ref", "scs_coverage_ref_range", "scs_write_coverage_ref", "scs_coverage_ref_kernel_time",
            "scs_coverage_ref_finish_probe"}
    product = os.path.join(ROOT, "scssim_amd", "libscssim_hip.so")
    for lib in (product, SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    code = "import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.scs_test_seam.restype = ctypes.c_char_p; L.scs_test_seam.argtypes = [ctypes.c_char_p]; print((L.scs_test_seam(b'SCS_TEST_COV_LDS') or b'<unset>').decode())"
    seen = [subprocess.run([sys.executable, "-c", code, lib], env=dict(os.environ, SCS_TEST_COV_LDS="4"), capture_output=True, text=True).stdout.strip() for lib in (product, SEAMS_LIB)]
    assert seen == ["<unset>", "4"]
    assert "k_cov_ref_hist" in open(os.path.join(ROOT, "scssim_amd", "csrc", "scs_seams.h")).read()
    for m in ("set_coverage_ref", "coverage_ref_shape", "download_coverage_ref", "coverage_ref_range", "write_coverage_ref", "coverage_ref_kernel_time"):
        assert callable(getattr(scssim_amd.GenReads, m)), m
    assert callable(scssim_amd.coverage_ref_finish_probe)
    assert len(scssim_amd.GenReads.KERNELS) == 8            # scs_kernel_time's table is not extended


def test_the_tile_is_the_one_the_cases_assume():
    assert scssim_amd.coverage_tile()[0] == T


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--coverage-profile-ref without --lift, with --gpus 2, and --coverage-max alone end the CLI with their own message before it
    touches a device or an input file (these do not exist); --coverage-max serves either profile."""
    r = _cli(["--coverage-profile-ref", "/nonexistent/c.txt"])
    assert r.returncode != 0 and "--coverage-profile-ref needs --lift" in r.stderr, r.stderr
    r = _cli(["--coverage-profile-ref", "/nonexistent/c.txt", "--lift", "/nonexistent/x.lift", "--gpus", "2"])
    assert r.returncode != 0 and "--coverage-profile-ref needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--coverage-max", "500"])
    assert r.returncode != 0 and "--coverage-max needs --coverage-profile or --coverage-profile-ref" in r.stderr, r.stderr
    r = _cli(["--coverage-profile-ref", "/nonexistent/c.txt", "--lift", "/nonexistent/x.lift", "--coverage-max", "65536"])
    assert r.returncode != 0 and "--coverage-max should be an integer in 1~65535" in r.stderr, r.stderr
    r = _cli(["--coverage-profile-ref", "/nonexistent/c.txt", "--lift", "/nonexistent/x.lift", "--coverage-max", "500"])
    assert "--coverage-max needs" not in r.stderr and "--coverage-profile-ref needs" not in r.stderr      # (it fails later, on the missing input)
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--coverage-profile-ref <string>" in h.stdout + h.stderr
    assert "--coverage-profile-ref" in open(os.path.join(ROOT, "scssim_amd", "csrc", "scssim_main.cpp")).read().split("\n")[4]   # the header comment's list


def test_restatement_on_the_dense_layout(tmp_path):
    """The dense layout of lift_cases.write_dense_inputs through scs_lift_plan_probe: sum copies + inserted = staged bases; the CN-0
    stretch 40001 .. 45000 is absent and nothing else is; the CN-4 stretch 10001 .. 14000 has 4 copies per haplotype copy (2 on
    either haplotype) wherever no planted deletion took a base; a depth of ones lifts to the copies."""
    ref, var = write_dense_inputs(tmp_path)
    t, _ = scssim_amd.lift_plan_probe(ref, None, var)
    seg = tuple(np.asarray(getattr(t, k), np.int64) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind"))
    ref_lens, G = np.asarray(t.ref_lens, np.int64), int(np.asarray(t.hap_lens).sum())
    codes = np.zeros(G, np.uint8)
    ref_depth, copies, n_copies, unlifted = rc.lift_arrays(np.ones(G, np.int64), codes, seg, ref_lens)
    inserted = int(seg[1][seg[4] == 1].sum())
    assert int(copies.sum()) + inserted == G and unlifted == inserted > 0 and (ref_depth == copies).all() and not n_copies.any()
    assert (copies[40000:45000] == 0).all() and (copies[45000:45100] == 2).sum() > 50 and (copies[39900:40000] == 2).sum() > 50   # (planted deletions take some)
    cn4 = copies[10000:14000]
    assert set(np.unique(cn4)) <= {0, 4} and (cn4 == 4).sum() > 3000                        # (planted deletions are homozygous: 0 copies, never 1 .. 3)
    assert set(np.unique(copies[25000:27000])) <= {0, 1} and (copies[25000:27000] == 1).sum() > 1500
    outside = np.r_[copies[:10000], copies[14000:25000], copies[27000:40000], copies[45000:]]
    assert set(np.unique(outside)) <= {0, 2}
    tb = rc.tables(ref_depth, copies, n_copies, ref_lens, 3)
    assert int(tb["absent"][0]) == int((copies == 0).sum()) == int(tb["cn_bases"][0][0]) >= 5000 and int(tb["hist"][0][0]) == int(tb["absent"][0])
    assert int(tb["sum"][0]) + unlifted == G and int(tb["cn_sum"][0][4]) == 4 * int(tb["cn_bases"][0][4])
    # N in one haplotype only is sequence; N in both is N
    codes[:G // 2] = 4
    _, c2, n2, _ = rc.lift_arrays(np.ones(G, np.int64), codes, seg, ref_lens)
    assert ((n2 > 0) & (n2 < c2)).sum() > 40000 and int(rc.tables(ref_depth, c2, n2, ref_lens, 3)["n_bases"][0]) == int(((c2 > 0) & (n2 == c2)).sum())


def _seen(layout, size, n, fam):
    return rc.seen(dict(layout=layout, size=size, n=n, fam=fam, lds=-1), T)


def test_the_case_table_reaches_the_branches_it_names():
    cases = rc.table_cases(-1)
    names = [rc.name_of(s) for s in cases]
    assert len(set(names)) == len(names) and {s["layout"] for s in cases} == set(rc.LAYOUTS) and {s["size"] for s in cases} == set(rc.SIZES)
    assert {(s["n"], s["fam"]) for s in cases} == {(n, f) for n in rc.NS for f in rc.FAMILIES}
    for lay in rc.LAYOUTS:                                  # every layout at every size, and under several N layouts and families
        mine = [s for s in cases if s["layout"] == lay]
        assert {s["size"] for s in mine} == set(rc.SIZES) and len({s["n"] for s in mine}) >= 3 and len({s["fam"] for s in mine}) >= 2, lay
    s = _seen("two_haps", "T+1", "mixed", "ones")
    assert s["far_adders"] and s["max_copies"] == 2 and s["mixed_n"] == T + 1 and s["all_n"] == 0 and s["staged_tiles"] == 3
    s = _seen("two_haps", "T+1", "all", "ones")
    assert s["all_n"] == T + 1 and s["mixed_n"] == 0
    s = _seen("tandem3x8", "65", "none", "eight_copies")
    assert s["max_copies"] == 8 and s["collide_in_wave"] and s["back"] == 7 and s["sum_crosses_d"] == 3 and s["top_bucket"] == 3
    s = _seen("tandem_tile_x3", "2T+1", "none", "small")
    assert s["max_copies"] == 3 and s["back"] == 2 and s["staged_tiles"] >= 4 and not s["collide_in_wave"]
    assert _seen("back_jump", "T", "none", "ones")["back"] == 1
    s = _seen("ins_first", "64", "none", "ones")
    assert s["first_is_i"] and s["unlifted"] == s["inserted"] == 5
    s = _seen("ins_mid", "T+1", "none", "ones")
    assert not s["first_is_i"] and not s["last_is_i"] and s["unlifted"] == s["inserted"] == T + 1
    assert _seen("ins_last", "T", "none", "ones")["last_is_i"]
    assert _seen("ins_record", "T-1", "none", "ones")["i_record"]
    s = _seen("cn0_tile", "65", "none", "ones")
    assert s["absent_tile"] and s["absent"] == T and s["ref_tiles"] == 3
    s = _seen("cn0_record", "T+1", "none", "ones")
    assert s["absent_record"] and s["absent"] == T + 1
    s = _seen("borders", "T", "none", "small")
    assert s["staged_borders"] == [T - 1, T, T + 1] and s["ref_borders"] == [T - 1, T, T + 1]
    s = _seen("one_base_segs", "2T+1", "none", "ones")
    assert s["one_base_segs"] == s["n_segs"] == 2 * T + 1 and s["back"] == 2 * T
    assert _seen("second_ref_record", "T+1", "blocks", "small")["ref_record_starts_inside_tile"]
    s = _seen("identity", "2T+1", "none", "pile")
    assert s["max_depth_seen"] == 70000 > s["D"] > rc.LDS and s["top_bucket"] == 1
    d = rc.case(dict(layout="identity", size="2T+1", n="none", fam="pile", lds=-1), T)[0]
    assert ((d > rc.LDS) & (d < 5000)).sum() == 1           # between the LDS table and D: a bucket that exists only in memory
    assert rc.case(dict(layout="identity", size="T", n="none", fam="small", lds=-1), T)[0].tolist().count(0) > T // 2
