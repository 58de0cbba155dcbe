"""GPU tests of the coverage profile on the reference (scs_set_coverage_ref / scssim genreads --lift --coverage-profile-ref; DESIGN.md
section 21): the kernels alone over given staged depths, codes and segment tables against numpy's np.add.at
(scs_coverage_ref_finish_probe, tests/coverage_ref_cases.py); whole jobs against the truth SAM of the same yield call lifted in
numpy through the downloaded table, against the staged profile lifted the same way and against the depth track by reference bin;
invariance over sinks, batches, LDS sizes and the two switches; the file and the CLI's two-step flow; refusals and ownership.
Each job runs in a child process under its own time limit.  Run with `-m gpu`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child, sv_ref  # noqa: F401 (a fixture)
from gpu_readers import CLI, SV, Segs, _exact_profile, _fasta, _sam, make_genome
from lift_cases import DENSE_COV, copies_from_table, expected_reach, lift_from_sam, ref_layout, write_dense_inputs

import coverage_cases as cc
import coverage_ref_cases as rc
import scssim_amd

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- 1: the kernels alone
# The child builds every case from the case table (plain numpy, seeded), runs the probe and compares there: only verdicts travel.
_PROBE = r'''
import numpy as np
import coverage_ref_cases as rc
import scssim_amd
from gpu_child import emit, job_args
a = job_args()
g = scssim_amd.GenReads()
T, _ = scssim_amd.coverage_tile()
res = {}
for spec in rc.table_cases(a["lds"]):
    depth, codes, seg, hap_lens, ref_lens, D = rc.case(spec, T)
    want = rc.reference(depth, codes, seg, ref_lens, D)
    got = scssim_amd.coverage_ref_finish_probe(g, depth, codes, seg, hap_lens, ref_lens, D, spec["lds"])
    bad = [k for k in ("ref_depth", "packed", "hist", "n_bases", "absent", "sum", "sum_n", "cn_bases", "cn_sum") if got[k].shape != want[k].shape or not (got[k] == want[k]).all()]
    if got["unlifted"] != want["unlifted"]:
        bad.append("unlifted")
    if int(got["sum"].sum()) + int(got["sum_n"].sum()) + got["unlifted"] != int(depth.astype(np.int64).sum()):
        bad.append("identity")
    res[rc.name_of(spec)] = "ok" if not bad else "differs: " + ",".join(bad)
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
emit(res)
'''


@pytest.mark.parametrize("lds", [-1, 0, 4], ids=["lds_default", "lds_0", "lds_4"])
def test_kernels_alone_against_numpy(lds):
    """Reference lengths 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 T + 1 x fourteen segment layouts (identity, two haplotypes, tandem units
    of 3 x 8 and (T + 1) x 3, a backwards jump, I segments first / in the middle / last / as a whole staged record, CN 0 over a whole
    reference tile and a whole reference record, borders at T - 1, T, T + 1 on both sides, one-base segments, a second reference record
    inside a tile) under rotating N layouts and depth families, and four layouts under all of them: reference depths, packed copies,
    every table and `unlifted` are numpy's, exactly.  tests/test_coverage_ref_host.py proves what the cases reach."""
    res = run_child(_PROBE, dict(lds=lds), timeout=300)
    names = [rc.name_of(s) for s in rc.table_cases(lds)]
    bad = {k: v for k, v in res.items() if v != "ok"}
    assert not bad and set(names) == set(res) and len(names) > 150, (dict(list(bad.items())[:10]), len(bad))


_BAD = r'''
import numpy as np
import coverage_ref_cases as rc
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EOVERFLOW
from gpu_child import fails, job_args
g = scssim_amd.GenReads()
T, _ = scssim_amd.coverage_tile()
u64 = lambda *v: np.array(v, np.int64)
G = T + 10
depth, codes = np.ones(G, np.uint32), np.zeros(G, np.uint8)
for lds in (-1, 0):
    # the second segment lifts 1 base past the end of its reference record; one that names a reference record that does not exist
    seg = (u64(0, T), u64(T, 10), u64(0, T - 9), u64(0, 0), u64(0, 0))
    fails(lambda: scssim_amd.coverage_ref_finish_probe(g, depth, codes, seg, [G], [T], 50, lds), SCS_EOVERFLOW, "lifts outside its reference record")
    seg = (u64(0, T), u64(T, 10), u64(0, 0), u64(0, 1), u64(0, 0))
    fails(lambda: scssim_amd.coverage_ref_finish_probe(g, depth, codes, seg, [G], [T], 50, lds), SCS_EOVERFLOW, "lifts outside its reference record")
    # and the ctx is as good as new
    spec = dict(layout="tandem3x8", size="T+1", n="mixed", fam="small", lds=lds)
    d, cd, sg, hl, rl, D = rc.case(spec, T)
    want, got = rc.reference(d, cd, sg, rl, D), scssim_amd.coverage_ref_finish_probe(g, d, cd, sg, hl, rl, D, lds)
    assert all((got[k] == want[k]).all() for k in ("ref_depth", "packed", "hist", "absent", "cn_bases", "cn_sum")) and got["unlifted"] == want["unlifted"]
# segments that do not tile the staged records never reach a kernel
fails(lambda: scssim_amd.coverage_ref_finish_probe(g, depth, codes, (u64(0, T), u64(T, 9), u64(0, 0), u64(0, 0), u64(0, 0)), [G], [T], 50), SCS_EINVAL, "tile")
# 65536 staged bases on one reference base: the packed word's 16 bits would wrap -- refused, never silent
n = 65536
seg = (np.arange(n, dtype=np.int64), np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64))
fails(lambda: scssim_amd.coverage_ref_finish_probe(g, np.zeros(n, np.uint32), np.zeros(n, np.uint8), seg, [n], [1], 50), SCS_EOVERFLOW, "65535")
got = scssim_amd.coverage_ref_finish_probe(g, np.ones(n - 1, np.uint32), np.zeros(n - 1, np.uint8), tuple(v[:n - 1] for v in seg), [n - 1], [1], 50)
assert got["packed"].tolist() == [65535] and got["ref_depth"].tolist() == [65535] and got["cn_bases"][0][16] == 1 and got["cn_sum"][0][16] == 65535
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_a_segment_past_its_reference_record_gives_the_lift_error_and_leaves_the_ctx_usable():
    """A table whose segment ends one base past its reference record, and one that names a record the reference does not have: the
    lift flag's error from kernels that add nothing for such a segment, and the same ctx then runs a good case right.  A table
    that would put 65536 copies on one base is refused before any kernel; 65535 fit."""
    run_child(_BAD, {}, timeout=300, ok=True)


# ---------------------------------------------------------------- 2 - 5: jobs
# one ctx, one genome by simuvars (or a FASTA and its lift file), one amplified job, then a yield per leg:
# {name, dr (max_depth on the reference; 0: off), d (staged max_depth; 0: off), wr (reference bins; 0: off), sink, sam, lds, write, staged_refused}
_CHILD = r'''
import ctypes
import numpy as np
from scssim_amd import SCS_EINVAL
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a, segs=True)
t = g.lift_segments()
res = {}
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    g.set_seed(a["seed"])
    g.set_coverage(leg.get("d", 0)); g.set_coverage_ref(leg.get("dr", 0)); g.set_depth_ref(leg.get("wr", 0))
    g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
    with leg_env({"SCS_TEST_COV_LDS": str(leg["lds"])} if "lds" in leg else {}):
        yield_leg(g, pre, leg)
    res[leg["name"]] = dict(reads_written=g.stats()["reads_written"], mark=g.coverage_kernel_time(0), finish=g.coverage_kernel_time(1), copies=g.coverage_ref_kernel_time(0),
                            ref_finish=g.coverage_ref_kernel_time(1), k_reads=g.kernel_times()["k_reads"])
    arrays = {}
    if leg.get("dr"):
        tb = g.download_coverage_ref()
        nf, D = g.coverage_ref_shape()
        per = [g.coverage_ref_range(r, 0, int(t.ref_lens[r])) for r in range(nf)]
        assert all(d.dtype == np.uint32 and c.dtype == np.uint32 for d, c in per)
        arrays.update(ref_depth=np.concatenate([d for d, _ in per]), copies=np.concatenate([c for _, c in per]), unlifted=np.uint64(tb.pop("unlifted")), **tb)
        if leg.get("write"):
            g.write_coverage_ref(pre + ".cov")
    if leg.get("d"):
        arrays["staged"] = np.concatenate([g.coverage_range(r, 0, n) for r, n in enumerate(a["hap_lens"])])
        arrays["staged_sum"] = g.coverage()["sum"]
    if leg.get("wr"):
        arrays["bin_reads"], arrays["bin_bases"], arrays["bin_copies"], arrays["bin_off"] = g.depth_ref()
    if leg.get("staged_refused"):                            # only the reference switch is on: what scs_set_coverage exposes stays refused
        g._L.scs_download_coverage.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_uint64]
        assert g._L.scs_download_coverage(g._ctx, None, None, None, None, 1 << 20) == SCS_EINVAL
        g._L.scs_coverage_range.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        assert g._L.scs_coverage_range(g._ctx, 0, 0, 0, None) == SCS_EINVAL
        res[leg["name"]]["staged_refused"] = True
    np.savez(pre + "_cov.npz", **arrays)
emit(res)
'''

TABLES = ("hist", "n_bases", "absent", "sum", "sum_n", "cn_bases", "cn_sum")


def _run(tmp_path, legs, hap_lens, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"], a["hap_lens"] = legs, [int(v) for v in hap_lens]
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def _arrays(out, name):
    z = np.load(out + "_" + name + "_cov.npz")
    return {k: z[k] for k in z.files}


def _seg(s):
    return (s.hap_off, s.len, s.ref_pos, s.ref_rec, s.kind)


def check_against_sam(out, res, name, staged_fa, D, w=0):
    """Every array of the leg against the truth SAM of the same yield call: the per-base depth rebuilt from @SQ, POS and CIGAR
    (coverage_cases.depth_from_sam), carried through the downloaded segment table by np.add.at.  Returns (arrays, segments, what the
    reads reach)."""
    got, seg = _arrays(out, name), Segs(out)
    hdr, recs = _sam(out + "_" + name + ".sam")
    per, sq, m_sum, _ = cc.depth_from_sam(hdr, recs)
    seqs = _fasta(staged_fa)
    assert [n for n, _ in sq] == list(seqs) and [ln for _, ln in sq] == [len(v) for v in seqs.values()]
    staged = np.concatenate([per[n] for n, _ in sq])
    codes = np.concatenate([np.where(np.frombuffer(seqs[n], np.uint8) == ord("N"), 4, 0) for n, _ in sq]).astype(np.uint8)
    assert len(recs) == res[name]["reads_written"] > 500
    want_depth, copies, n_copies, unlifted = rc.lift_arrays(staged, codes, _seg(seg), seg.ref_lens)
    assert got["ref_depth"].dtype == np.uint32 and got["ref_depth"].shape == want_depth.shape and len(np.unique(want_depth)) >= 3
    assert (got["ref_depth"] == want_depth).all(), np.nonzero(got["ref_depth"] != want_depth)[0][:10]
    assert (got["copies"] == copies).all(), np.nonzero(got["copies"] != copies)[0][:10]
    want = rc.with_genome_row(rc.tables(want_depth, copies, n_copies, seg.ref_lens, D))
    for k in TABLES:
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape and (got[k] == want[k]).all(), k
    assert int(got["unlifted"]) == unlifted
    assert int(got["sum"][-1]) + int(got["sum_n"][-1]) + unlifted == m_sum == int(staged.sum())           # the sum identity
    assert (got["cn_bases"][:, 0] == got["absent"]).all() and (got["hist"].sum(axis=1) + got["n_bases"] == np.r_[seg.ref_lens, seg.ref_lens.sum()]).all()
    if "staged" in got:                                     # the staged profile of the same call, lifted the same way
        assert (got["staged"] == staged).all()
        assert (rc.lift_arrays(got["staged"], codes, _seg(seg), seg.ref_lens)[0] == got["ref_depth"]).all()
    assert res[name]["ref_finish"]["launches"] == 1 and res[name]["ref_finish"]["units"] == staged.size and res[name]["finish"]["launches"] == 1
    assert res[name]["mark"]["launches"] == res[name]["k_reads"]["launches"] >= 1                          # one marking pass per batch whichever switches are on
    reach = lift_from_sam(out + "_" + name + ".sam", seg, w or 1000)[4]
    if w:                                                   # the depth track by reference bin is the bin sums of the per-base arrays
        nb = ref_layout(seg.ref_lens, w)[1]
        assert (got["bin_bases"][:nb] == rc.bin_sums(got["ref_depth"].astype(np.int64), seg.ref_lens, w)).all() and int(got["bin_bases"][nb]) == unlifted
        assert (got["bin_copies"][:nb] == rc.bin_sums(got["copies"].astype(np.int64), seg.ref_lens, w)).all() and (got["bin_copies"] == copies_from_table(seg, seg.ref_lens, w)).all()
    return got, seg, reach


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    ref, var = write_dense_inputs(d)
    table, _ = scssim_amd.lift_plan_probe(ref, None, var)
    return dict(ref=ref, var=var, table=table, dir=d)


def test_dense_layout(dense, models, tmp_path):
    """2: the dense layout of test_gpu_lift.py (boundaries closer than a read is long, CN 4 / 1 / 0), PE HiSeq2500 under the exact-
    placement model with indel rates 0.004 at 14x, truth SAM, both profiles and the depth track at bins of 37 in one yield call.
    The geometry is checked on the CPU first; what the reads of the job reached is asserted from the SAM."""
    t, L = dense["table"], 125
    n_reads = DENSE_COV * float(np.asarray(t.ref_lens).sum()) / L
    exp = expected_reach(t, L, n_reads)
    assert exp["cross"] > 0.55 * n_reads and min(exp["wholly_inserted"], exp["back"]) >= 8, exp                # safe before relying on it
    prof = _exact_profile(models["Illumina_HiSeq2500"], str(tmp_path / "x.profile"), 0.004, 0.004)
    fa = str(tmp_path / "staged.fa")
    out, res = _run(tmp_path, [dict(name="a", d=1000, dr=1000, wr=37, sam=True)], t.hap_lens, prof=prof, ref=dense["ref"], vars=dense["var"], out_fasta=fa, cov=DENSE_COV, layout="PE", seed=19, ber=0.0)
    got, seg, reach = check_against_sam(out, res, "a", fa, 1000, w=37)
    assert reach["back"] >= 1 and reach["wholly_inserted"] >= 1 and int(got["unlifted"]) > 0, reach           # reads over a backwards junction; reads wholly in inserted sequence
    assert int(got["copies"].max()) >= 4 and int(got["absent"][-1]) >= 5000 and (got["copies"][40000:45000] == 0).all() and (got["ref_depth"][40000:45000] == 0).all()
    cn = got["cn_sum"][-1].astype(np.float64) / np.maximum(got["cn_bases"][-1], 1)
    assert got["cn_bases"][-1][[1, 2, 4]].min() > 1000 and cn[0] == 0.0 and cn[[1, 2, 4]].min() > 0.0          # depth as a function of copy number: every class is there
    assert res["a"]["copies"]["launches"] == 1 and res["a"]["copies"]["units"] == int(np.asarray(t.hap_lens).sum())


def test_golden_simuvars_genome(sv_ref, models, tmp_path):
    """2: the golden simuvars genome (1.5 Mb staged, CN 0 .. 8, three reference records), PE HiSeq2500 at 2x."""
    host, _ = scssim_amd.lift_plan_probe(sv_ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"))
    fa = str(tmp_path / "staged.fa")
    out, res = _run(tmp_path, [dict(name="a", d=50, dr=50, wr=37, sam=True)], host.hap_lens, prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"),
                    vars=os.path.join(SV, "vars.txt"), out_fasta=fa, cov=2.0, layout="PE", seed=41)
    got, seg, _ = check_against_sam(out, res, "a", fa, 50, w=37)
    assert got["hist"].shape == (4, 51) and int(got["copies"].max()) >= 8 and int(got["absent"][-1]) > 0 and (got["ref_depth"][149999:160000] == 0).all()


def test_plain_two_haplotype_genome(models, tmp_path):
    """2: simuvars without variant files: one R segment per haplotype, so the reference depth is the sum of the two haplotypes'
    staged depths, every base has two copies, nothing is absent and nothing unlifted."""
    ref = make_genome(str(tmp_path / "ref.fa"), "60000,40500", 17, ref=True)
    out, res = _run(tmp_path, [dict(name="both", d=1000, dr=1000)], [60000, 60000, 40500, 40500], prof=models["Illumina_HiSeq2500"], ref=ref, cov=3.0, layout="PE", seed=3)
    z, seg = _arrays(out, "both"), Segs(out)
    assert len(seg) == 4 and seg.ref_lens.tolist() == [60000, 40500]
    s = z["staged"].astype(np.int64)
    want = np.concatenate([s[0:60000] + s[60000:120000], s[120000:160500] + s[160500:201000]])
    assert (z["ref_depth"] == want).all() and want.sum() > 100000 and (z["copies"] == 2).all()
    assert int(z["unlifted"]) == 0 and not z["absent"].any() and (z["cn_bases"][:, 2] == [60000, 40500, 100500]).all() and int(z["cn_sum"][-1][2]) == int(want.sum())
    assert int(z["sum"][-1]) + int(z["sum_n"][-1]) == int(s.sum())


INV = dict(cov=24.0, layout="PE", seed=23)                 # the dense genome at 24x of its 60 kb reference: 5760 pairs -- two batches of 4096 at SCS_TEST_BATCH_SHIFT=12


@pytest.fixture(scope="module")
def invariance(dense, models, tmp_path_factory):
    """One PE job through every sink on one ctx of the seams build in two batches: computed once, shared, never changed."""
    d = tmp_path_factory.mktemp("inv")
    legs = [dict(name="cb", dr=1000, sam=True, staged_refused=True), dict(name="off", sink="files"), dict(name="on", dr=1000, sink="files"),
            dict(name="parts", dr=1000, sink="files", writers=3, generations=2), dict(name="bgzf", dr=1000, sink="files", bgzf=True),
            dict(name="null", dr=1000, sink="null"), dict(name="dev", dr=1000, sink="device"), dict(name="again", dr=1000),
            dict(name="lds0", dr=1000, sink="null", lds=0), dict(name="lds4", dr=1000, sink="null", lds=4),
            dict(name="both", d=7, dr=1000, sink="null"), dict(name="d3", dr=3, sink="null"), dict(name="staged_only", d=7, sink="null")]
    fa = str(d / "staged.fa")
    out, res = _run(d, legs, dense["table"].hap_lens, env=seams_env(SCS_TEST_BATCH_SHIFT="12"), prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], out_fasta=fa, **INV)
    return out, res, fa


def test_invariance_over_sinks_batches_and_lds_sizes_on_one_ctx(invariance):
    """3: a callback (checked against its SAM), files, 3 writers x 2 generations, BGZF, a NULL sink, the text left in device memory, a
    second yield after set_seed (the arrays were zeroed), no LDS histogram and one of 4 buckets: the same arrays every time, from
    two batches; the copies are made once on this ctx; the FASTQ files with the profile on are the files with it off."""
    out, res, fa = invariance
    ref, _, _ = check_against_sam(out, res, "cb", fa, 1000)
    assert res["cb"]["mark"]["launches"] == res["cb"]["k_reads"]["launches"] == 2 and res["cb"]["copies"]["launches"] == 1 and res["cb"]["staged_refused"]
    for name in ("on", "parts", "bgzf", "null", "dev", "again", "lds0", "lds4", "both"):
        got = _arrays(out, name)
        for k in TABLES + ("ref_depth", "copies", "unlifted"):
            assert (got[k] == ref[k]).all(), (name, k)
        assert res[name]["mark"]["launches"] == 2 and res[name]["finish"]["launches"] == 1 and res[name]["ref_finish"]["launches"] == 1
        assert res[name]["copies"]["launches"] == (1 if name == "on" else 0)                  # made again after the switch was off; else the layout stands
    for k in ("mark", "finish", "copies", "ref_finish"):
        assert res["off"][k]["launches"] == 0 and res["off"][k]["units"] == 0, k              # off: no code of it runs
    assert res["staged_only"]["ref_finish"]["launches"] == 0 and res["staged_only"]["mark"]["launches"] == 2
    for m in ("_1.fq", "_2.fq"):
        want = open(out + "_off" + m, "rb").read()
        assert len(want) > 100000 and open(out + "_on" + m, "rb").read() == want == open(out + "_cb" + m, "rb").read()


def test_the_two_switches_and_max_depth_3_against_1000(invariance):
    """3: both switches with different max_depth: one array, the staged tables at their own max_depth (7), the reference's unchanged;
    with max_depth 3 on the reference the buckets below 3 are those of 1000 and the top bucket is the tail's sum."""
    out, res, _ = invariance
    ref, both, d3, st = _arrays(out, "cb"), _arrays(out, "both"), _arrays(out, "d3"), _arrays(out, "staged_only")
    assert both["staged_sum"].shape == st["staged_sum"].shape and (both["staged_sum"] == st["staged_sum"]).all() and (both["staged"] == st["staged"]).all()
    assert int(both["staged"].astype(np.int64).sum()) == int(ref["sum"][-1]) + int(ref["sum_n"][-1]) + int(ref["unlifted"])
    assert d3["hist"].shape == (ref["hist"].shape[0], 4) and (d3["hist"][:, :3] == ref["hist"][:, :3]).all()
    assert (d3["hist"][:, 3] == ref["hist"][:, 3:].sum(axis=1)).all() and int(d3["hist"][-1, 3]) > 0
    for k in ("ref_depth", "copies", "n_bases", "absent", "sum", "sum_n", "cn_bases", "cn_sum", "unlifted"):
        assert (d3[k] == ref[k]).all(), k
    assert res["d3"]["copies"]["launches"] == 1                                               # another max_depth released the arrays: the copies are made again


def test_file_and_the_cli_two_step_flow(sv_ref, models, tmp_path):
    """4: write_coverage_ref's file parsed back against the downloaded tables; `scssim simuvars --lift`, then `scssim genreads --lift
    --coverage-profile-ref --coverage-max 50` writes the same file for the same seed, byte for byte."""
    prof, snp, var = models["Illumina_HiSeq2500"], os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt")
    host, _ = scssim_amd.lift_plan_probe(sv_ref, snp, var)
    out, res = _run(tmp_path, [dict(name="api", dr=50, sink="null", write=True)], host.hap_lens, prof=prof, ref=sv_ref, snp=snp, vars=var, cov=2.0, layout="PE", seed=77)
    t, f = _arrays(out, "api"), rc.parse_file(out + "_api.cov")
    names = list(host.ref_names)
    summ, cn, rows = rc.render_counts(names, t)
    assert f["D"] == 50 and [(n, v[:4]) for n, v in f["summary"]] == summ and [c[:4] for c in f["cn"]] == cn and [r[:4] for r in f["rows"]] == rows
    for (_, v), r in zip(f["summary"], range(len(names) + 1)):
        s = cc.stats_from_hist(t["hist"][r], int(t["sum"][r]), 50)
        assert v[4:] == pytest.approx([s["mean"]] + list(s["breadth"]) + [s["gini"]], rel=1e-9, abs=1e-12)   # (the file prints ten significant digits)
    assert [c[4] for c in f["cn"]] == pytest.approx([c[3] / c[2] for c in cn], rel=1e-9) and [r[4] for r in f["rows"]] == pytest.approx([r[2] / r[3] for r in rows], rel=1e-9)
    assert f["unlifted"] == (int(t["unlifted"]), int(np.asarray(host.len)[np.asarray(host.kind) == 1].sum())) and f["unlifted"][1] > 0
    simu, lift, pre = str(tmp_path / "simu.fa"), str(tmp_path / "simu.lift"), str(tmp_path / "cli")
    r = subprocess.run([CLI, "simuvars", "-r", sv_ref, "-s", snp, "-v", var, "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([CLI, "genreads", "-i", simu, "-m", prof, "-c", "2", "-o", pre, "--seed", "77", "--lift", lift, "--coverage-profile-ref", pre + ".cov", "--coverage-max", "50"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(pre + ".cov").read() == open(out + "_api.cov").read()


_OWN = r'''
import ctypes
import numpy as np
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_coverage_ref(1000)
fails(s.yield_reads, SCS_EINVAL, "scs_set_coverage_ref", "sharded")
s.set_coverage_ref(0)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")       # the refusal is gone: what is missing now is the job itself
fails(lambda: s.set_coverage_ref(65536), SCS_EINVAL, "65535")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_coverage_ref(1000)
fails(g.coverage_ref_shape, SCS_EINVAL, "lift table")
fails(lambda: g.yield_reads(collect=False), SCS_EINVAL, "scs_set_coverage_ref", "scs_load_lift", "scs_simuvars")   # a staged genome without a table
g.set_coverage_ref(0)
g.yield_reads(collect=False)
# a genome with its table
g.simuvars(a["ref"], None, None)
g.run(collect=False)
before = scssim_amd.live_resources()
fails(g.coverage_ref_shape, SCS_EINVAL, "off")
g.set_coverage_ref(1000)
assert g.coverage_ref_shape() == (3, 1000)
fails(g.download_coverage_ref, SCS_EINVAL, "scs_download_coverage_ref")     # before any yield
fails(lambda: g.coverage_ref_range(0, 0, 10), SCS_EINVAL, "scs_coverage_ref_range")
fails(lambda: g.write_coverage_ref(a["out"] + ".cov"), SCS_EINVAL, "scs_write_coverage_ref")
g.set_seed(5); g.yield_reads(collect=False)
t = g.download_coverage_ref()
assert g.coverage_ref_kernel_time(0)["launches"] == 1 and g.coverage_ref_kernel_time(1)["launches"] == 1 and scssim_amd.live_resources()[0] > before[0]
d, cp = g.coverage_ref_range(0, 0, 400000)
assert (cp == 2).all() and int(d.sum()) == int(t["sum"][0]) + int(t["sum_n"][0]) > 0 and t["unlifted"] == 0
d2, cp2 = g.coverage_ref_range(0, 100, 350)
assert (d2 == d[100:350]).all() and (cp2 == 2).all() and g.coverage_ref_range(2, 60000, 60000)[0].size == 0
fails(lambda: g.coverage_ref_range(0, 0, 400001), SCS_EINVAL, "not inside")
fails(lambda: g.coverage_ref_range(0, 11, 10), SCS_EINVAL, "not inside")
fails(lambda: g.coverage_ref_range(3, 0, 1), SCS_EINVAL, "not inside")
buf = (ctypes.c_uint64 * 4)()
g._L.scs_download_coverage_ref.argtypes = [ctypes.c_void_p] * 8 + [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64]
assert g._L.scs_download_coverage_ref(g._ctx, None, buf, None, None, None, None, None, None, 3) == SCS_EOVERFLOW
assert g._L.scs_download_coverage_ref(g._ctx, None, None, None, buf, None, None, None, None, 4) == 0 and list(buf) == t["sum"].tolist()
g._L.scs_coverage_ref_range.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
assert g._L.scs_coverage_ref_range(g._ctx, 0, 0, 10, None, None) == 0                     # either output may be NULL
# off: nothing of it is left, the staged array it brought included; on again: the copies are made again
g.set_coverage_ref(0)
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())
g.set_seed(5); g.yield_reads(collect=False)
assert g.coverage_ref_kernel_time(1)["launches"] == 0 and g.coverage_kernel_time(0)["launches"] == 0
fails(g.download_coverage_ref, SCS_EINVAL, "off")
g.set_coverage_ref(1000)
g.set_seed(5); g.yield_reads(collect=False)
assert g.coverage_ref_kernel_time(0)["launches"] == 1 and all((g.download_coverage_ref()[k] == t[k]).all() for k in ("hist", "sum", "cn_sum"))
# another table for the same genome: the copies are made again, from it
g.write_lift(a["out"] + ".lift")
lines = open(a["out"] + ".lift").read().split("\n")
head, body = [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if ln and not ln.startswith("#")]
f = body[0].split("\t")                                       # the first staged record: its second half becomes inserted sequence
half = int(f[2]) // 2
body[0:1] = ["\t".join([f[0], "0", str(half), f[3], "0", str(half), "R"]), "\t".join([f[0], str(half), f[2], f[3], str(half), str(half), "I"])]
open(a["out"] + "_2.lift", "w").write("\n".join(head + body) + "\n")
g.load_lift(a["out"] + "_2.lift")
fails(g.download_coverage_ref, SCS_EINVAL, "scs_download_coverage_ref")     # another table: the last call's arrays are not its
g.set_seed(5); g.yield_reads(collect=False)
assert g.coverage_ref_kernel_time(0)["launches"] == 1
t2 = g.download_coverage_ref()
d, cp = g.coverage_ref_range(0, 0, 400000)
assert (cp[:half] == 2).all() and (cp[half:] == 1).all() and t2["unlifted"] > 0 and int(t2["cn_bases"][0][1]) == 400000 - half
assert int(t2["sum"][-1]) + int(t2["sum_n"][-1]) + t2["unlifted"] == int(t["sum"][-1]) + int(t["sum_n"][-1])
g.set_seed(5); g.yield_reads(collect=False)
assert g.coverage_ref_kernel_time(0)["launches"] == 0 and g.coverage_ref_kernel_time(1)["launches"] == 1     # the layout stands
# staging another genome drops the table and clears `valid`
g.load_genome(a["fa"])
fails(g.download_coverage_ref, SCS_EINVAL)
g.simuvars(a["ref"], None, None); g.set_coverage_ref(9)
g.run(collect=False)                                          # destroyed right after a yield
assert g.download_coverage_ref()["hist"].shape == (4, 10) and g.coverage_ref_kernel_time(0)["launches"] == 1
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(sv_ref, models, golden_inputs, tmp_path):
    """5: a sharded ctx and a genome without a table are refused at the yield call by name; no download, range or file before a
    yield, none into too few rows, no range outside a reference record; load_lift of another table invalidates the arrays and has the
    copies remade from it; the live resources read the same before the feature goes on and after it goes off; restaging clears
    `valid`; nothing is left once the contexts are destroyed right after a yield."""
    own = dict(prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], ref=sv_ref, out=str(tmp_path / "own"))
    run_child(_OWN, own, timeout=300, ok=True)


# the four states of the two switches, walked along a closed path that takes each of the twelve transitions between them once
_MATRIX = r'''
import numpy as np
import scssim_amd
from scssim_amd import SCS_EINVAL
from gpu_child import fails, job_args
a = job_args()
g = scssim_amd.GenReads(profile=a["prof"], coverage=2.0, seed=5)
g.simuvars(a["ref"], a["snp"], a["vars"])
g.run(collect=False)
never_on = scssim_amd.live_resources()                        # before the feature was ever switched on
WALK = [(0, 0), (1, 0), (0, 0), (0, 1), (0, 0), (1, 1), (1, 0), (0, 1), (1, 0), (1, 1), (0, 1), (1, 1), (0, 0)]
assert len(set(zip(WALK, WALK[1:]))) == 12 and all(p != q for p, q in zip(WALK, WALK[1:]))
same = lambda x, y: all((np.asarray(x[k]) == np.asarray(y[k])).all() for k in x)
first, now, drift = {}, (0, 0), []
for state in WALK:
    had_ref, came_from = now[1], now
    if state[0] != now[0]: g.set_coverage(50 if state[0] else 0)
    if state[1] != now[1]: g.set_coverage_ref(1000 if state[1] else 0)
    now = state
    staged, ref = state
    g.set_seed(5); g.yield_reads(collect=False)
    seen = {}
    if staged:
        g.gc_bias(100); g.write_coverage_bedgraph(a["out"] + ".bg")
        seen["cov"] = g.coverage(); seen["range"] = dict(d=g.coverage_range(0, 1000, 1250))
        assert seen["cov"]["hist"].shape == (g.coverage_shape()[0] + 1, 51)
    else:
        fails(g.coverage_shape, SCS_EINVAL, "off"); fails(g.coverage, SCS_EINVAL, "off")
        fails(lambda: g.coverage_range(0, 1000, 1250), SCS_EINVAL, "scs_coverage_range")
        if ref: g.write_coverage_ref_bedgraph(a["out"] + "_ref.bg")
    if ref:
        seen["ref"] = g.download_coverage_ref(); d, cp = g.coverage_ref_range(0, 1000, 1250); seen["ref_range"] = dict(d=d, cp=cp)
        assert seen["ref"]["hist"].shape == (4, 1001)
    else:
        fails(g.coverage_ref_shape, SCS_EINVAL, "off"); fails(g.download_coverage_ref, SCS_EINVAL, "off")
        fails(lambda: g.coverage_ref_range(0, 1000, 1250), SCS_EINVAL, "scs_coverage_ref_range")
    live = scssim_amd.live_resources()
    launches = [g.coverage_kernel_time(0)["launches"], g.coverage_kernel_time(1)["launches"], g.coverage_ref_kernel_time(0)["launches"], g.coverage_ref_kernel_time(1)["launches"]]
    print(state, "live", live, "launches", launches, flush=True)
    # the staged array's two passes run for either switch; the copies are made once per layout, which a change of the reference switch forgets
    assert (launches[0] > 0 and launches[1] == 1) if staged or ref else launches[:2] == [0, 0], (state, launches)
    assert launches[2:] == ([1 if not had_ref else 0, 1] if ref else [0, 0]), (state, had_ref, launches)
    if state == (0, 0): assert live == never_on, (never_on, live)
    if state not in first: first[state] = (live, seen)
    else:
        if live != first[state][0]: drift.append((came_from, state, first[state][0], live))   # (asserted behind the walk, so that the walk's other checks run)
        assert all(same(seen[k], first[state][1][k]) for k in seen) and seen.keys() == first[state][1].keys(), state
assert len(first) == 4
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
assert not drift, drift
print("ok")
'''


def test_the_switch_matrix(sv_ref, models, tmp_path):
    """6: one ctx on the golden simuvars genome walks the four states of (scs_set_coverage 50, scs_set_coverage_ref 1000) along a
    closed path that takes each of the twelve transitions once, a yield in every state (gc_bias and a bedGraph where the staged
    switch is on, the reference bedGraph where only the other one is).  In every state the live resources, the tables of the
    switches that are on and one 250-base window equal those of the state's first visit; off/off holds what the ctx held before the
    feature was ever on; an off switch's accessors are refused and its timers read no launch; the copies kernel runs exactly when the
    reference switch has just come on; nothing is left after close()."""
    run_child(_MATRIX, dict(prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), out=str(tmp_path / "mx")), timeout=300, ok=True)
