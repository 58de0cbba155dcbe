"""Host-side tests of the site support table on the original reference (scs_set_site_support_ref): the expansion
of the listed reference positions to staged positions and the gather of the staged counters, through the functions the kernels run
(scs_support_ref.h, by way of scs_support_ref_probe), against the per-base numpy restatement of tests/support_ref_cases.py on the
hand-made lift tables of tests/test_artefacts_ref_host.py; fill chunks; broken tables; the header's bytes; the line suffix; the
exported symbols; the CLI's refusals.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SEAMS_LIB
from site_ref_cases import Segs, header
from support_ref_cases import INFO3, fields, restate, strip_support
from test_artefacts_ref_host import HETDEL, MIX, ONE, TANDEM, TWO, World

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
CHUNKS = [1, 2, 3, 257]

# a het substitution does not break a segment: TWO is that layout.  CN 4 of reference [40, 100) on both haplotypes: eight staged
# indices under every X in it
CN4 = World([200], [[("R", 0, 0, 100), ("R", 0, 40, 100), ("R", 0, 40, 100), ("R", 0, 40, 100), ("R", 0, 100, 200)]] * 2)
LAYOUTS = {"one_segment": ONE, "two_haplotypes_het_substitution": TWO, "two_tandem_copies": TANDEM, "het_deletion": HETDEL,
           "insertion_cn0_and_two_reference_records": MIX, "cn4_on_two_haplotypes": CN4}


def ref_off(w):
    return np.concatenate([[0], np.cumsum(w.ref_lens)]).astype(np.int64)


def x_lists(w):
    """The listed positions the issue names, per layout: the first and last base of every R segment; just outside either end; bases
    in no segment; every base of one segment; all of them together; none; one"""
    off, total = ref_off(w), int(sum(w.ref_lens))
    s = w.segs
    R = [i for i in range(len(s.kind)) if s.kind[i] == 0]
    x0 = [int(off[s.ref_rec[i]] + s.ref_pos[i]) for i in R]
    x1 = [a + int(s.len[i]) for a, i in zip(x0, R)]
    covered = np.zeros(total, bool)
    for a, b in zip(x0, x1):
        covered[a:b] = True
    out = {"first_and_last_base": sorted(set(x0) | {b - 1 for b in x1}),
           "just_outside_either_end": sorted({a - 1 for a in x0 if a > 0} | {b for b in x1 if b < total}),
           "in_no_segment": np.nonzero(~covered)[0].tolist(),
           "every_base_of_a_segment": list(range(x0[min(1, len(R) - 1)], x1[min(1, len(R) - 1)])),
           "empty": [], "one": [x0[-1]]}
    out["all"] = sorted(set(sum((list(v) for v in out.values()), [])))
    return out


def check(w, xs, chunks=CHUNKS, seed=3):
    n = int(sum(w.hap_lens))
    g = np.random.default_rng(seed).integers(0, 50, (n, 6)).astype(np.uint32)
    want_pos, want_px, want_sum = restate(n, w.segs, w.ref_lens, xs, g)
    for chunk in [0] + list(chunks):
        pos, px, sums = scssim_amd.support_ref_probe(w.segs, w.hap_lens, w.ref_lens, xs, chunk=chunk, g_counts=g)
        assert np.array_equal(pos, want_pos) and np.array_equal(px, want_px), chunk
        assert np.array_equal(sums, want_sum), chunk
        assert (np.diff(pos.astype(np.int64)) > 0).all()
    pos, px, sums = scssim_amd.support_ref_probe(w.segs, w.hap_lens, w.ref_lens, xs)
    assert sums is None and np.array_equal(pos, want_pos)
    return want_pos, want_px, want_sum


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_expansion_and_gather_equal_the_restatement_at_every_chunk(layout):
    w = LAYOUTS[layout]
    for name, xs in x_lists(w).items():
        pos, px, sums = check(w, xs)
        if name in ("empty", "in_no_segment"):
            assert len(pos) == 0, (layout, name)


def test_the_layouts_reach_what_they_name():
    def n_under(w, x):
        return len(restate(int(sum(w.hap_lens)), w.segs, w.ref_lens, [x])[0])
    assert n_under(ONE, 0) == 1 and n_under(ONE, 199) == 1
    assert n_under(TWO, 100) == 2                               # the het substitution: both haplotypes, one segment each
    assert [n_under(TANDEM, x) for x in (39, 40, 99, 100)] == [2, 3, 3, 2]
    assert [n_under(HETDEL, x) for x in (99, 100, 120, 139, 140)] == [2, 1, 1, 1, 2]   # the gap: one staged index, not two
    pos, _, _ = restate(int(sum(HETDEL.hap_lens)), HETDEL.segs, HETDEL.ref_lens, [120])
    assert pos.tolist() == [int(HETDEL.hap_off[1]) + 120]
    assert [n_under(MIX, x) for x in (119, 120, 139, 140)] == [2, 0, 0, 2]             # CN 0
    assert n_under(MIX, 200) == 2 and n_under(MIX, 200 + 50) == 2                      # the second reference record
    assert [n_under(CN4, x) for x in (39, 40, 99, 100)] == [2, 8, 8, 2]
    # the insertion: no staged index of [80, 90) of record 0 is ever listed
    X_all = list(range(300))
    pos, _, _ = restate(int(sum(MIX.hap_lens)), MIX.segs, MIX.ref_lens, X_all)
    assert not set(range(80, 90)) & set(pos.tolist()) and len(pos) == int((np.asarray(MIX.segs.len)[np.asarray(MIX.segs.kind) == 0]).sum())
    # a launch border inside a segment's range: the second copy of TANDEM holds 60 listed positions at chunk 1, 2, 3 and 257
    assert len(x_lists(TANDEM)["every_base_of_a_segment"]) == 60


def random_world(rng, trial):
    """The random tables of tests/test_artefacts_ref_host.py::test_random_haplotypes_amplicons_and_slabs: copies that jump backwards,
    insertions, deletions, two reference records (the same procedure; the amplicons there are not needed here)"""
    ref_lens = [int(rng.integers(300, 600)), int(rng.integers(100, 300))]
    haps = []
    for rr in (0, 0, 1, 1):
        h, total = [], 0
        while total < 500:
            if rng.random() < 0.25 and h and h[-1][0] == "R":
                h.append(("I", int(rng.integers(1, 30))))
            else:
                a = int(rng.integers(0, ref_lens[rr] - 1))
                b = int(rng.integers(a + 1, min(ref_lens[rr], a + 120) + 1))
                if h and h[-1][0] == "R" and h[-1][3] == a:
                    continue                                    # (would be one segment)
                h.append(("R", rr, a, b))
            total += h[-1][1] if h[-1][0] == "I" else h[-1][3] - h[-1][2]
        if h[0][0] == "I":
            h = h[1:]
        haps.append(h)
    return World(ref_lens, haps, seed=trial)


def test_random_tables_of_backward_jumping_copies_and_insertions():
    rng = np.random.default_rng(23)
    for trial in range(6):
        w = random_world(rng, trial)
        total = int(sum(w.ref_lens))
        for k in (1, 40, total):
            xs = np.sort(rng.choice(total, k, replace=False))
            pos, px, sums = check(w, xs, seed=trial)
        assert np.bincount(px).max() >= 3 and (np.asarray(w.segs.kind) == 1).any()   # a position under three or more copies; an insertion


@pytest.mark.parametrize("what,why", [("segment_past_its_reference_record", 3), ("segment_of_an_unknown_reference_record", 3), ("segments_out_of_order", 2), ("a_gap_between_segments", 2),
                                      ("segment_of_no_bases", 2), ("segment_past_its_staged_record", 2), ("positions_out_of_order", 4), ("position_twice", 4),
                                      ("position_outside_the_reference", 4)])
def test_broken_tables_are_refused_with_their_reason(what, why):
    w, xs = MIX, [10, 150, 250]
    seg = [np.array(getattr(w.segs, k)) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")]
    if what == "segment_past_its_reference_record":             # [140, 200) of the reference moved to [141, 201)
        seg[2][3] += 1
    elif what == "segment_of_an_unknown_reference_record":
        seg[3][2] = 2
    elif what == "segments_out_of_order":
        seg = [np.concatenate([s[:1], s[2:3], s[1:2], s[3:]]) for s in seg]
    elif what == "a_gap_between_segments":
        seg[0][2] += 1
        seg[1][2] -= 1
    elif what == "segment_of_no_bases":
        seg[1][1] = 0
    elif what == "segment_past_its_staged_record":              # the last segment of record 0 runs into record 1
        seg[1][3] += 5
    elif what == "positions_out_of_order":
        xs = [150, 10]
    elif what == "position_twice":
        xs = [10, 10]
    else:
        xs = [10, 300]
    with pytest.raises(ScsError) as e:
        scssim_amd.support_ref_probe(Segs(np.stack(seg, axis=1)), w.hap_lens, w.ref_lens, xs)
    assert e.value.code == SCS_EINVAL and e.value.why == why
    assert {2: "does not follow the last", 3: "past its reference record", 4: "out of order or outside the reference"}[why] in str(e.value)


def test_a_counter_past_2_32_minus_1_is_refused_never_wrapped():
    n = int(sum(TWO.hap_lens))
    g = np.zeros((n, 6), np.uint32)
    g[50, 2], g[250, 2] = 0xFFFFFFFF, 1                        # the two haplotypes' counters of X = 50
    with pytest.raises(ScsError) as e:
        scssim_amd.support_ref_probe(TWO.segs, TWO.hap_lens, TWO.ref_lens, [50], g_counts=g)
    assert e.value.why == 6
    g[250, 2] = 0
    assert scssim_amd.support_ref_probe(TWO.segs, TWO.hap_lens, TWO.ref_lens, [50], g_counts=g)[2][0, 2] == 0xFFFFFFFF


def test_header_bytes_and_the_stripped_text():
    base = header(MIX.ref_names, MIX.ref_lens, (3, 12))
    got = scssim_amd.support_ref_header_probe(MIX.ref_names, MIX.ref_lens, (3, 12))
    lines = base.split("\n")
    at = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    assert got == "\n".join(lines[:at] + INFO3 + lines[at:])     # the three lines behind the four, in front of #CHROM
    assert "##scssim_unlifted=<entries=3,reads=12>\n" in got and got.count("##INFO=") == 7
    # a line with its counters, stripped, is the artefact table's line (the formatter the emit kernel runs)
    cnt = np.array([7, 0, 3, 11, 2, 5], np.uint32)
    body = plain = ""
    for ref, alt in ((0, 3), (4, 1), (2, 2)):
        with_c = scssim_amd.site_support_line_probe("chr2", 49, ref, alt, 2, 9, 13, 40, cnt)
        without = scssim_amd.site_support_line_probe("chr2", 49, ref, alt, 2, 9, 13, 40)
        assert with_c.endswith(";DP=23;AD=%d,%d;DL=5\n" % (cnt[ref], cnt[alt])) and strip_support(with_c) == without
        dp, ad, dl = fields(with_c)
        assert ad[0] + ad[1] <= dp or ref == alt
        body += with_c
        plain += without
    assert strip_support(got + body) == base + plain


def test_both_libraries_export_the_abi():
    want = {"scs_set_site_support_ref", "scs_site_support_ref", "scs_write_site_support_ref", "scs_site_support_ref_kernel_time", "scs_site_support_ref_step_time",
            "scs_support_ref_probe", "scs_support_ref_header_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    assert len(scssim_amd.GenReads.KERNELS) == 8                # the new kernels have no slot of scs_kernel_time
    for m in ("set_site_support_ref", "site_support_ref", "write_site_support_ref", "site_support_ref_kernel_time"):
        assert callable(getattr(scssim_amd.GenReads, m))
    assert callable(scssim_amd.support_ref_probe)


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    r = _cli(["--support-ref", "/nonexistent/s.vcf"])
    assert r.returncode == 1 and "--support-ref needs --lift" in r.stderr, r.stderr
    r = _cli(["--support-ref", "/nonexistent/s.vcf", "--lift", "/nonexistent/a.lift", "--support", "/nonexistent/t.vcf"])
    assert r.returncode == 1 and "--support-ref can not be combined with --support" in r.stderr, r.stderr
    r = _cli(["--support-ref", "/nonexistent/s.vcf", "--lift", "/nonexistent/a.lift", "--gpus", "2"])
    assert r.returncode == 1 and "--support-ref needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--support-ref", ""])
    assert r.returncode == 1 and "--support-ref needs the name of the file" in r.stderr, r.stderr
    r = _cli(["--support-min-reads", "1"])
    assert r.returncode == 1 and "--support-min-reads needs --support (the file the site support table goes to)" in r.stderr, r.stderr
    r = _cli(["--support-ref", "/nonexistent/s.vcf", "--support-min-reads", "1"])
    assert r.returncode == 1 and "--support-ref needs --lift" in r.stderr, r.stderr     # (the min-reads option is accepted with this table alone)
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--support-ref <string>" in h.stdout + h.stderr
