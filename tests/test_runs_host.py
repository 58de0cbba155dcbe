"""Host-side tests of the bedGraph writer of the per-base arrays (scs_write_coverage_bedgraph, scs_write_coverage_ref_bedgraph,
scs_write_copy_number_ref): the restatement (tests/runs_cases.py) against a per-base loop, the one line
formatter of kernels and probe (scs_runs_line_probe) at every digit-count edge, the CLI's options and refusals, the ABI surface,
and the formatter as a stand-alone program under the sanitizers.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEAMS_LIB

import runs_cases as rc
import scssim_amd
from scssim_amd import SCS_EOVERFLOW

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
T = 4096                                                    # COV_TILE (tests/test_coverage_ref_host.py holds it to the library's)


def _edges(top):
    """0, 9, 10, 99, 100, ... 10^k - 1, 10^k up to `top`, and `top`"""
    out, p = [0], 10
    while p <= top:
        out += [p - 1, p]; p *= 10
    return out + [p - 1 if p - 1 <= top else top, top]


VALUES = sorted(set(_edges(2 ** 32 - 1)))
POSITIONS = sorted(set(_edges(10 ** 19) + [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 63, 2 ** 64 - 1]))


def host_rows():
    """(name, start, end, value) of the host table: every digit-count edge of each number against two others, an empty name and
    one of 200 bytes."""
    rows = [("chr1", p, p + 1 if p < 2 ** 64 - 1 else p, 7) for p in POSITIONS]
    rows += [("chr1", 0, p, 4294967295) for p in POSITIONS]
    rows += [("chrX_alt", 5, 2 ** 33, v) for v in VALUES]
    rows += [("", 0, 1, 0), ("", 2 ** 40, 2 ** 40 + 1, 4294967295), (rc.LONG_NAME, 0, 10, 3), (rc.LONG_NAME, 2 ** 64 - 2, 2 ** 64 - 1, 4294967295)]
    return rows


def host_check_rows():
    """The host table as the lines tools/runs_host_check.cpp reads (@: the empty name)."""
    return ["%s %d %d %d" % (n or "@", s, e, v) for n, s, e, v in host_rows()]


def test_restatement_against_a_per_base_loop():
    """bedgraph_text (numpy.flatnonzero over the differences and the record starts) is the per-base loop's text on small arrays of
    every family under several record layouts, both masks; parse() expands it back to the masked values."""
    rng = np.random.default_rng(5)
    n_checked = 0
    for fam in rc.FAMILIES:
        for n in (1, 2, 3, 17, 64, 301):
            v, mask = rc.values_of(fam, n, 8, 3 * n)        # (a tile of 8: tile_edge's changes fall inside the small arrays)
            for lens in ([n], [1] * n, [n // 2, n - n // 2] if n > 1 else [n], rng.multinomial(n, [0.25] * 4).tolist()):
                lens = [x for x in lens if x] if lens != [n] else lens
                names = ["rec%d" % i for i in range(len(lens))]
                text = rc.bedgraph_text(v, mask, lens, names)
                assert text == rc.per_base_loop(v, mask, lens, names), (fam, n, lens)
                back = rc.parse(text)
                assert [nm for nm, _ in back] == names and (np.concatenate([a for _, a in back]) == (v.astype(np.int64) & mask)).all()
                n_checked += 1
    assert n_checked > 100
    # equal values on both sides of a record border are two runs; under 0xFFFF the upper half neither cuts nor prints
    assert rc.bedgraph_text([4, 4, 4, 4], rc.FULL, [2, 2], ["a", "b"]) == b"a\t0\t2\t4\nb\t0\t2\t4\n"
    assert rc.bedgraph_text([0x10002, 0x20002, 0x30003], rc.LOW, [3], ["a"]) == b"a\t0\t2\t2\na\t2\t3\t3\n"
    assert rc.bedgraph_text([0, 0, 5], rc.FULL, [3], ["a"]) == b"a\t0\t2\t0\na\t2\t3\t5\n"    # runs of 0 are written
    tb = rc.tile_bytes(np.r_[np.zeros(20, np.uint32), 1], rc.FULL, [21], ["c"], 8)
    assert tb.tolist() == [len(b"c\t0\t20\t0\n"), 0, len(b"c\t20\t21\t1\n")]              # a line belongs to the tile its run starts in
    assert rc.plan_slabs([5, 0, 0, 7, 7], 7) == [(0, 3, 5), (3, 4, 7), (4, 5, 7)] and rc.plan_slabs([5, 8], 7) is None


def test_line_probe_at_every_digit_count_edge():
    """scs_runs_line_probe, the SCS_HD formatter the sizing and emit kernels run, against "%s\\t%d\\t%d\\t%d\\n" with start, end and
    value at 0, 9, 10, ..., 10^k - 1, 10^k, 2^32 - 1 for the value and positions beyond 2^32 up to 2^64 - 1; an empty name and one
    of 200 bytes."""
    rows = host_rows()
    assert len(rows) > 100 and len(rc.LONG_NAME) == 200 and {len(str(v)) for v in VALUES} == set(range(1, 11)) and {len(str(p)) for p in POSITIONS} == set(range(1, 21))
    for name, s, e, v in rows:
        assert scssim_amd.runs_line_probe(name, s, e, v) == ("%s\t%d\t%d\t%d\n" % (name, s, e, v)).encode(), (name, s, e, v)


def test_line_probe_with_a_cap_one_byte_short():
    for name, s, e, v in [("chr1", 0, 1, 0), (rc.LONG_NAME, 2 ** 40, 2 ** 41, 4294967295), ("", 9, 10, 9)]:
        want = ("%s\t%d\t%d\t%d\n" % (name, s, e, v)).encode()
        assert scssim_amd.runs_line_probe(name, s, e, v, cap=len(want)) == want
        with pytest.raises(scssim_amd.ScsError) as ei:
            scssim_amd.runs_line_probe(name, s, e, v, cap=len(want) - 1)
        assert ei.value.code == SCS_EOVERFLOW and ei.value.needed == len(want)
    with pytest.raises(scssim_amd.ScsError) as ei:
        scssim_amd.runs_line_probe("chr1", 0, 1, 0, cap=0)
    assert ei.value.code == SCS_EOVERFLOW and ei.value.needed == len(b"chr1\t0\t1\t0\n")


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work_and_the_help_names_the_options():
    """The -ref options without --lift, any of the three with --gpus 2 and an empty name end the CLI with their own message before it
    touches a device or an input file (these do not exist); --coverage-max alone is refused as before, and serves the new options."""
    for opt in ("--coverage-bedgraph-ref", "--copy-number-ref"):
        r = _cli([opt, "/nonexistent/x.bg"])
        assert r.returncode != 0 and opt + " needs --lift" in r.stderr, r.stderr
    for opt in ("--coverage-bedgraph", "--coverage-bedgraph-ref", "--copy-number-ref"):
        r = _cli([opt, "/nonexistent/x.bg", "--lift", "/nonexistent/x.lift", "--gpus", "2"])
        assert r.returncode != 0 and opt + " needs --gpus 1" in r.stderr, r.stderr
        r = _cli([opt, ""])
        assert r.returncode != 0 and opt + " needs the name of the file" in r.stderr, r.stderr
        r = _cli([opt, "/nonexistent/x.bg.gz", "--lift", "/nonexistent/x.lift", "--coverage-max", "500"])
        assert "--coverage-max needs" not in r.stderr and " needs --lift" not in r.stderr and "needs --gpus" not in r.stderr      # (it fails later, on the missing input)
        r = _cli([opt, "/nonexistent/x.bg", "--lift", "/nonexistent/x.lift", "--coverage-max", "65536"])
        assert r.returncode != 0 and "--coverage-max should be an integer in 1~65535" in r.stderr, r.stderr
    r = _cli(["--coverage-max", "500"])
    assert r.returncode != 0 and "--coverage-max needs --coverage-profile or --coverage-profile-ref" in r.stderr, r.stderr
    r = _cli(["--coverage-profile-ref", "/nonexistent/c.txt"])
    assert r.returncode != 0 and "--coverage-profile-ref needs --lift" in r.stderr, r.stderr
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    for opt in ("--coverage-bedgraph <string>", "--coverage-bedgraph-ref <string>", "--copy-number-ref <string>"):
        assert opt in h.stdout + h.stderr, opt
    head = open(os.path.join(ROOT, "scssim_amd", "csrc", "scssim_main.cpp")).read().split("\n")[4]                                # the header comment's list
    assert "--coverage-bedgraph," in head and "--coverage-bedgraph-ref" in head and "--copy-number-ref" in head


def test_both_libraries_export_the_abi_and_the_product_reads_no_seam():
    want = {"scs_write_coverage_bedgraph", "scs_write_coverage_ref_bedgraph", "scs_write_copy_number_ref", "scs_coverage_bedgraph_kernel_time", "scs_runs_probe", "scs_runs_line_probe"}
    product = os.path.join(ROOT, "scssim_amd", "libscssim_hip.so")
    for lib in (product, SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    code = "import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.scs_test_seam.restype = ctypes.c_char_p; L.scs_test_seam.argtypes = [ctypes.c_char_p]; print((L.scs_test_seam(b'SCS_TEST_RUNS_TEXT_CAP') or b'<unset>').decode())"
    seen = [subprocess.run([sys.executable, "-c", code, lib], env=dict(os.environ, SCS_TEST_RUNS_TEXT_CAP="4096"), capture_output=True, text=True).stdout.strip() for lib in (product, SEAMS_LIB)]
    assert seen == ["<unset>", "4096"]
    assert "SCS_TEST_RUNS_TEXT_CAP" in open(os.path.join(ROOT, "scssim_amd", "csrc", "scs_seams.h")).read()
    assert "getenv" not in open(os.path.join(ROOT, "scssim_amd", "csrc", "scs_runs.cpp")).read()
    for m in ("write_coverage_bedgraph", "write_coverage_ref_bedgraph", "write_copy_number_ref", "coverage_bedgraph_kernel_time"):
        assert callable(getattr(scssim_amd.GenReads, m)), m
    assert callable(scssim_amd.runs_probe) and callable(scssim_amd.runs_line_probe)
    assert len(scssim_amd.GenReads.KERNELS) == 8            # scs_kernel_time's table is not extended


def test_the_case_table_holds_what_it_names():
    """Every size under every family, every layout; the families reach what they name at the sizes that can."""
    cases = rc.table_cases()
    names = [rc.name_of(s) for s in cases]
    assert len(set(names)) == len(names) and {s["size"] for s in cases} == set(rc.SIZES) and {s["lay"] for s in cases} == set(rc.LAYOUTS)
    assert {(s["size"], s["fam"]) for s in cases} == {(a, b) for a in rc.SIZES for b in rc.FAMILIES}
    assert [rc.size_of(s, T) for s in rc.SIZES] == [1, 2, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3]
    st = rc.runs(*rc.case(dict(size="4T+3", fam="equal", lay="one"), T)[:3])[0]
    assert st.tolist() == [0]                               # one run over every tile
    assert len(rc.runs(*rc.case(dict(size="4T+3", fam="alt", lay="one"), T)[:3])[0]) == 4 * T + 3
    st = rc.runs(*rc.case(dict(size="2T+1", fam="tile_edge", lay="one"), T)[:3])[0]
    assert st.tolist() == [0, T - 1, T, 2 * T - 1, 2 * T]
    v, mask, lens, names_ = rc.case(dict(size="4T+3", fam="equal", lay="edge"), T)
    assert lens == [T, 3 * T + 3] and rc.runs(v, mask, lens)[0].tolist() == [0, T]                 # equal values, a border at a tile edge: cut
    v, mask, lens, names_ = rc.case(dict(size="4T+3", fam="upper", lay="one"), T)
    assert mask == rc.LOW and len(rc.runs(v, rc.FULL, lens)[0]) > 10 * len(rc.runs(v, mask, lens)[0]) > 100
    v, mask, lens, names_ = rc.case(dict(size="T+1", fam="digits", lay="one"), T)
    assert {len(str(int(x))) for x in v} == set(range(1, 11)) and 4294967295 in v
    lens, names_ = rc.layout_of("many", T + 1, T)
    assert len(lens) == 300 and sum(lens[:299]) < T and sum(lens) == T + 1
    assert rc.layout_of("ones", T + 1, T)[0] == [1] * (T + 1) and rc.layout_of("long", 5, T)[1] == [rc.LONG_NAME]
    lens, _ = rc.layout_of("mid", 2 * T + 1, T)
    assert 0 < lens[0] < T and sum(lens) == 2 * T + 1
    # the slab case: tiles 1 and 2 hold no run start, the first run spans three tiles and ends inside the fourth
    v, mask, lens, names_ = rc.slab_case(T)
    tb = rc.tile_bytes(v, mask, lens, names_, T)
    assert tb[1] == tb[2] == 0 and tb[0] == len(b"chr1\t0\t%d\t0\n" % (3 * T + 5)) and (tb[3:] > 10 * T).all()
    assert int(tb.max()) == int(tb[3]) and rc.plan_slabs(tb, int(tb[0])) is None and rc.plan_slabs(tb, int(tb.max()) - 1) is None
    assert [s[:2] for s in rc.plan_slabs(tb, int(tb.max()))] == [(0, 3), (3, 4), (4, 5), (5, 6)]                       # a cut right behind a tile with no run start, inside the run over three tiles


def test_sanitizer_build_of_the_formatter():
    """tools/runs_host_check.py: scs_runs.h (runs_line, the counting sink, the capped buffer) as a stand-alone CPU program under
    AddressSanitizer and UndefinedBehaviorSanitizer over the host table, every output in a heap block of exactly its size."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "runs_host_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) lines, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == len(host_rows()), r.stdout[-500:]
