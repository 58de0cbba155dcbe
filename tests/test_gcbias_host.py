"""Host-side tests of the GC-bias table of the per-base depth (scs_gc_bias, scs_write_gc_bias / scssim genreads --gc-bias,
--gc-window): the restatement (tests/gcbias_cases.py) against a loop over windows, what the kernel's case
table reaches, the CLI's options and refusals, the ABI surface.  No GPU needed."""
import os
import re
import subprocess

import numpy as np

from conftest import ROOT, SEAMS_LIB

import gcbias_cases as gc
import scssim_amd

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
CSRC = os.path.join(ROOT, "scssim_amd", "csrc")
T = 4096                                                    # COV_TILE (tests/test_coverage_ref_host.py holds it to the library's)


def _define(name):
    """the value of a #define of scs_gcbias.h: the restatement's constants are held to the library's"""
    m = re.search(r"#define %s (\d+)u" % name, open(os.path.join(CSRC, "scs_gcbias.h")).read())
    return int(m.group(1))


def test_restatement_against_a_loop_over_windows():
    """reference (cumsum per record, differences at distance W, bincount and add.at on uint64) is the loop's table on arrays of up to
    a few hundred bases: every code and depth family, both layouts, windows below, at and above the record lengths -- under a tile
    of 50, so that the families' tile borders fall inside the small arrays."""
    assert (gc.BINS, gc.MAX_WINDOW) == (_define("GCB_BINS"), _define("GCB_MAX_WINDOW"))
    hd = open(os.path.join(CSRC, "scs_gcbias.h")).read()
    assert "return 100u * (gc < window ? gc : window) / window;" in hd      # the bin the restatement restates: 100 * gc // W
    n = 0
    for size in ("1", "2", "63", "65", "100", "101", "T+W-1", "2T+1"):
        for k, W in enumerate((1, 2, 7, 64, 100)):
            for j, codes in enumerate(gc.CODES):
                spec = dict(size=size, W=W, lay=gc.LAYOUTS[(k + j) % 2], codes=codes, depth=gc.DEPTHS[(k + j + n) % 5], lds=-1)
                depth, cd, lens, W, _ = gc.case(spec, 50)
                assert len(depth) == len(cd) == sum(lens) <= 300
                got, want = gc.reference(depth, cd, lens, W), gc.brute_force(depth, cd, lens, W)
                assert not gc.same(got, {k_: np.array(v, dtype=object) for k_, v in want.items()}), gc.name_of(spec)
                n += 1
    assert n == 8 * 5 * 7
    # by hand: two records, a window never crosses the border; an N counts its windows out; bins by integer division
    t = gc.reference([1, 2, 3, 4, 5, 6], [1, 0, 2, 4, 2, 2], [3, 3], 2)       # CA, AG | NG, GG
    assert t["windows"][0].nonzero()[0].tolist() == [50] and int(t["windows"][0][50]) == 2 and int(t["depth_sum"][0][50]) == 3 + 5
    assert int(t["n_windows"][1]) == 1 and int(t["windows"][1][100]) == 1 and int(t["depth_sum"][1][100]) == 11 and int(t["n_windows"][0]) == 0
    t = gc.with_genome_row(gc.reference([2 ** 32 - 1] * 4, [1, 2, 1, 2], [4], 3))
    assert t["depth_sum"].dtype == np.uint64 and int(t["depth_sum"][1][100]) == 2 * 3 * (2 ** 32 - 1) and t["windows"].shape == (2, 101)
    mean, row_mean, norm = gc.derived(t["windows"][0], t["depth_sum"][0], 3)
    assert mean[100] == row_mean == float(2 ** 32 - 1) and norm[100] == 1.0 and norm[0] == 0.0


def test_the_case_table_holds_what_it_names():
    """Every (size, W) pair under each lds, every family under each lds; and over the listed cases at least one of each: a window over
    a tile border, one that ends on its record's end, records shorter than, of and one above W, a record border inside a tile and one
    inside a halo, an N only in a window's halo part, N runs over a tile border and over a record border, every bin at W = 100, empty
    bins at W = 7, a window sum above 2^32.  Conditions on the inputs, from the restatement alone."""
    cases = gc.table_cases()
    names = [gc.name_of(s) for s in cases]
    assert len(set(names)) == len(names) and 250 < len(cases) < 400
    assert max(gc.WINDOWS) == _define("GCB_MAX_WINDOW") and min(gc.WINDOWS) == 1          # the table reaches both ends of the library's range
    for lds in gc.LDS:
        mine = [s for s in cases if s["lds"] == lds]
        assert {(s["size"], s["W"]) for s in mine} >= {(a, b) for a in gc.SIZES for b in gc.WINDOWS}
        assert {s["codes"] for s in mine} == set(gc.CODES) and {s["depth"] for s in mine} == set(gc.DEPTHS) and {s["lay"] for s in mine} == set(gc.LAYOUTS)
    assert [gc.size_of(dict(size=s, W=100), T) for s in gc.SIZES] == [1, 2, 63, 64, 65, 99, 100, 101, T - 1, T, T + 1, T + 98, T + 99, T + 100, 2 * T + 1]
    assert {s["size"] for s in cases} == set(gc.SIZES) | set(gc.BIG) and gc.size_of(dict(size="4Tx1024+1", W=1), T) == 4 * T * 1024 + 1
    flags = ("crosses_tile", "ends_on_record_end", "shorter", "exact", "plus1", "border_in_tile", "border_in_halo", "n_only_in_halo", "n_over_tile_border", "n_over_record_border")
    hit = {f: 0 for f in flags}
    bins100, bins7, max_sum, most_tiles = set(), set(), 0, 0
    for s in cases:
        if s["size"] == "4Tx1024+1":                        # (its size is asserted above; the others reach everything named here)
            continue
        depth, cd, lens, W, _ = gc.case(s, T)
        assert len(depth) == len(cd) == sum(lens) == gc.size_of(s, T) and depth.dtype == np.uint32
        r = gc.seen(depth, cd, lens, W, T)
        for f in flags:
            hit[f] += bool(r[f])
        max_sum, most_tiles = max(max_sum, r["max_sum"]), max(most_tiles, r["tiles"])
        if W == 100:
            bins100 |= r["bins"]
        if W == 7:
            bins7 |= r["bins"]
    assert all(hit[f] >= 2 for f in flags), hit
    assert bins100 == set(range(101)) and bins7 == {100 * g // 7 for g in range(8)} and len(bins7) == 8
    assert max_sum > 2 ** 32 and most_tiles == -(-1000003 // T)
    # the families are what they say
    d, cd, lens, W, _ = gc.case(dict(size="2T+1", W=1000, lay="mix", codes="n_last", depth="huge", lds=0), T)
    assert np.flatnonzero(cd >= 4).tolist() == [T - 1] and int(d.max()) > 2 ** 31 - 1000 and lens == [1, 2, 37, 999, 1000, 1001, T - 1, 2 * T + 1 - 3040 - (T - 1)]
    d, cd, lens, W, _ = gc.case(dict(size="T+1", W=1, lay="mix", codes="all_n", depth="ones", lds=0), T)
    assert (cd == 4).all() and (d == 1).all() and lens[:3] == [1, 2, 37] and 0 not in lens
    r = gc.reference(d, cd, lens, 1)
    assert int(r["windows"].sum()) == 0 and r["n_windows"].astype(np.int64).tolist() == lens


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work_and_the_help_names_the_options():
    """--gc-window without --gc-bias, windows of 0 and 1025, --gpus 2 and an empty file name end the CLI with their own message
    before it touches a device or an input file (these do not exist); --coverage-max serves the new option."""
    r = _cli(["--gc-window", "50"])
    assert r.returncode != 0 and "--gc-window needs --gc-bias" in r.stderr, r.stderr
    for w in ("0", "1025", "x"):
        r = _cli(["--gc-bias", "/nonexistent/x.gc", "--gc-window", w])
        assert r.returncode != 0 and "--gc-window should be an integer in 1~1024" in r.stderr, r.stderr
    r = _cli(["--gc-bias", "/nonexistent/x.gc", "--gpus", "2"])
    assert r.returncode != 0 and "--gc-bias needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--gc-bias", ""])
    assert r.returncode != 0 and "--gc-bias needs the name of the file" in r.stderr, r.stderr
    for w in ("1", "1024"):
        r = _cli(["--gc-bias", "/nonexistent/x.gc", "--gc-window", w, "--coverage-max", "500"])
        assert r.returncode != 0 and "--gc-window" not in r.stderr and "--coverage-max needs" not in r.stderr and "needs --gpus" not in r.stderr   # (it fails later, on the missing input)
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    for opt in ("--gc-bias <string>", "--gc-window <int>"):
        assert opt in h.stdout + h.stderr, opt
    head = open(os.path.join(CSRC, "scssim_main.cpp")).read().split("\n")[4]                                                     # the header comment's list
    assert "--gc-bias," in head and "--gc-window" in head


def test_both_libraries_export_the_abi_and_the_new_sources_read_no_environment():
    want = {"scs_gc_bias", "scs_write_gc_bias", "scs_gc_bias_kernel_time", "scs_gc_bias_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    for src in ("scs_gcbias.cpp", "scs_gcbias.h", "scs_k_gcbias.hip"):
        text = open(os.path.join(CSRC, src)).read()
        assert "getenv" not in text and "seam_env" not in text, src
    hdr = open(os.path.join(ROOT, "include", "scssim_hip.h")).read()
    for sym in want:
        assert "int         %s(" % sym in hdr, sym
    for m in ("gc_bias", "write_gc_bias", "gc_bias_kernel_time"):
        assert callable(getattr(scssim_amd.GenReads, m)), m
    assert callable(scssim_amd.gc_bias_probe)
    assert len(scssim_amd.GenReads.KERNELS) == 8            # scs_kernel_time's table is not extended


def test_render_and_profile_reader(models):
    """The file's rendering over a small table: header, one #s line per record and the genome, rows only for bins with windows, the
    genome's rows last, model as %.6g of the profile's gc_means or `.`."""
    m = gc.profile_gc_means(models["Illumina_HiSeq2500"])
    assert len(m) == 101 and all(isinstance(x, float) for x in m) and len(set(m)) > 10
    t = gc.with_genome_row(gc.reference([1, 2, 3, 4, 5, 6], [1, 0, 2, 4, 2, 2], [3, 3], 2))
    text = gc.render(["a", "b"], t, 2, m).split("\n")
    assert text[0] == "#gc_bias\twindow=2\tstep=1\texcluded=windows_with_N\tbin=100*gc/window" and text[-1] == ""
    assert text[2:5] == ["#s\ta\t2\t0\t2.000000", "#s\tb\t1\t1\t5.500000", "#s\tgenome\t3\t1\t%.6f" % (19 / 6)]
    assert text[6:] == ["a\t50\t2\t8\t2.000000\t1.000000\t%.6g" % m[50], "b\t100\t1\t11\t5.500000\t1.000000\t%.6g" % m[100],
                        "genome\t50\t2\t8\t2.000000\t%.6f\t%.6g" % (2.0 / (19 / 6), m[50]), "genome\t100\t1\t11\t5.500000\t%.6f\t%.6g" % (5.5 / (19 / 6), m[100]), ""]
    assert gc.render(["a", "b"], t, 2, None).split("\n")[6].endswith("\t.")
    # the rendering's fixed lines are the writer's own (scs_gcbias.cpp), so neither can change alone
    src = open(os.path.join(CSRC, "scs_gcbias.cpp")).read()
    for ln in (text[1], text[5], text[0].replace("window=2", "window=%u")):
        assert '"' + ln.replace("\t", "\\t") + '\\n"' in src, ln
