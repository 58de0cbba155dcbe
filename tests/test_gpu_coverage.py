"""GPU tests of the coverage profile (scs_set_coverage / scssim genreads --coverage-profile): the end-of-job kernels alone over
given difference arrays against numpy.cumsum / bincount (scs_coverage_finish_probe: tile and chunk edges, record and N layouts, the
LDS histogram's sizes, inconsistent arrays); whole jobs against the truth SAM of the same yield call, base for base; invariance
over sinks, batches and table sizes on one ctx; the file and the CLI; the refusals and the ownership of the buffers.  Each job runs
in a child process under its own time limit.  Run with `-m gpu`."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child
from gpu_readers import CLI, _exact_profile, _fasta, _sam, make_genome

import coverage_cases as cc
import scssim_amd

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- 1: the end-of-job kernels alone
# The child builds every case of its list from the case table (coverage_cases.finish_case: plain numpy, seeded), runs the probe and
# compares with numpy there -- the arrays are up to 4 M entries, so only verdicts travel back: {case: "ok" | what differs}.
_FINISH = r'''
import numpy as np
import coverage_cases as cc
import scssim_amd
from gpu_child import emit, job_args
a = job_args()
g = scssim_amd.GenReads()
T, C = scssim_amd.coverage_tile()
res = {}
for spec in a["cases"]:
    name = cc.finish_name(spec)
    diff, codes, lens, D = cc.finish_case(spec, T, C)
    want = cc.finish_reference(diff, codes, lens, D)
    got = scssim_amd.coverage_finish_probe(g, diff, codes, lens, D, spec["lds"])
    bad = [k for k in ("depth", "hist", "n_bases", "sum", "sum_n") if got[k].shape != want[k].shape or not (got[k] == want[k]).all()]
    res[name] = "ok" if not bad else "differs: " + ",".join(bad) + " first depth " + str(np.nonzero(got["depth"] != want["depth"])[0][:5].tolist())
    if spec.get("seen") is not None:
        res[name + "/seen"] = cc.finish_seen(want, codes, lens, D, T)
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
emit(res)
'''

SMALL = ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "2T+1"]
LARGE = ["1000003", "T(C-1)", "TC", "TC+1"]
FAMILIES = ["zeros", "ones", "reads", "tile_edges", "pile", "around_d"]


def _finish(cases, timeout=300):
    res = run_child(_FINISH, dict(cases=cases), timeout=timeout)
    names = [cc.finish_name(s) for s in cases]
    assert len(set(names)) == len(names)
    bad = {k: v for k, v in res.items() if not k.endswith("/seen") and v != "ok"}
    assert not bad and set(names) <= set(res), (bad, sorted(set(names) - set(res)))
    return res


@pytest.mark.parametrize("lds", [-1, 0, 4], ids=["lds_default", "lds_0", "lds_4"])
def test_finish_kernels_small_sizes(lds):
    """G = 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 T + 1 x six difference families x {one record, records of 1, 2, 37, T - 1, T, T + 1
    repeated} x {no N, all N, N blocks over tile and record borders}: depth, histogram and the three sums are numpy's, bit for bit."""
    cases = [dict(size=s, fam=f, recs=r, codes=c, lds=lds) for s in SMALL for f in FAMILIES for r in ("one", "mixed") for c in ("acgt", "all_n", "blocks")]
    _finish(cases)


@pytest.mark.parametrize("size", LARGE)
def test_finish_kernels_large_sizes(size):
    """1 000 003 entries and the edges of the tile-offset scan's chunk, T (C - 1), T C, T C + 1: several families, record layouts and
    LDS sizes; the case table proves what it reaches (a tile with several records, a record over several tiles, N over both borders,
    depths in the top bucket and past the LDS table)."""
    cases = [dict(size=size, fam="reads", recs="mixed", codes="blocks", lds=-1, seen=1), dict(size=size, fam="tile_edges", recs="one", codes="blocks", lds=4),
             dict(size=size, fam="pile", recs="one", codes="acgt", lds=-1, seen=1), dict(size=size, fam="around_d", recs="mixed", codes="acgt", lds=0),
             dict(size=size, fam="ones", recs="mixed", codes="all_n", lds=4), dict(size=size, fam="zeros", recs="one", codes="acgt", lds=-1)]
    res = _finish(cases)
    seen = res[cc.finish_name(cases[0]) + "/seen"]
    assert seen["records_in_one_tile"] > 1 and seen["tiles_of_one_record"] > 1 and seen["n_over_tile_border"] and seen["n_over_record_border"] and seen["distinct_depths"] >= 3
    pile = res[cc.finish_name(cases[2]) + "/seen"]
    assert pile["max_depth_seen"] >= 70000 and pile["top_bucket"] >= 1 and pile["D"] == 65535


_BAD = r'''
import numpy as np
import coverage_cases as cc
import scssim_amd
from scssim_amd import SCS_EOVERFLOW
from gpu_child import fails, job_args
g = scssim_amd.GenReads()
T, C = scssim_amd.coverage_tile()
G = 2 * T + 1
codes, lens = np.zeros(G, np.uint8), [G]
for lds in (-1, 0, 4):
    d = np.zeros(G + 1, np.int32); d[0] = -1; d[5] = 1                 # a negative running depth
    fails(lambda: scssim_amd.coverage_finish_probe(g, d, codes, lens, 50, lds), SCS_EOVERFLOW, "coverage profile")
    d = np.zeros(G + 1, np.int32); d[0] = 1                            # never closed: not 0 behind the last base
    fails(lambda: scssim_amd.coverage_finish_probe(g, d, codes, lens, 50, lds), SCS_EOVERFLOW, "coverage profile")
    d = np.zeros(G + 1, np.int32); d[T] = -2000000000; d[T + 1] = 2000000000   # far outside any table: buckets are indexed by the clamped depth only
    fails(lambda: scssim_amd.coverage_finish_probe(g, d, codes, lens, 50, lds), SCS_EOVERFLOW, "coverage profile")
    spec = dict(size="2T+1", fam="reads", recs="mixed", codes="blocks", lds=lds)   # and the ctx is as good as new
    diff, cd, ln, D = cc.finish_case(spec, T, C)
    want, got = cc.finish_reference(diff, cd, ln, D), scssim_amd.coverage_finish_probe(g, diff, cd, ln, D, lds)
    assert all((got[k] == want[k]).all() for k in want)
g.close()
print("ok")
'''


def test_inconsistent_differences_give_the_flags_error_and_leave_the_ctx_usable():
    """-1 at 0 and +1 at 5; +1 at 0 never closed; +-2e9 in the middle: SCS_EOVERFLOW naming the coverage profile from kernels that
    index nothing by an unclamped depth, and the same ctx then runs a good case right."""
    run_child(_BAD, {}, timeout=300, ok=True)


# ---------------------------------------------------------------- 2 - 5: jobs
# one ctx, one amplified job, then a yield per leg: {name, d (max_depth; 0: off), w (depth track's bins; 0: off), sink, sam, lds, ...}
_CHILD = r'''
import numpy as np
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a)
res = {}
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    g.set_seed(a["seed"])
    g.set_coverage(leg.get("d", 0)); g.set_depth(leg.get("w", 0))
    g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
    with leg_env({"SCS_TEST_COV_LDS": str(leg["lds"])} if "lds" in leg else {}):
        yield_leg(g, pre, leg)
    res[leg["name"]] = dict(reads_written=g.stats()["reads_written"], mark=g.coverage_kernel_time(0), finish=g.coverage_kernel_time(1), k_reads=g.kernel_times()["k_reads"])
    if leg.get("d"):
        t = g.coverage()
        nr, D = g.coverage_shape()
        per = np.concatenate([g.coverage_range(r, 0, a["lens"][r]) for r in range(nr)])
        assert per.dtype == np.uint32
        np.savez(pre + "_cov.npz", depth=per, **t)
        if leg.get("w"):
            r, b, off = g.depth()
            np.savez(pre + "_depth.npz", bases=b, off=off)
        if leg.get("write"):
            g.write_coverage(pre + ".cov")
emit(res)
'''


def _run(tmp_path, legs, fa, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"], a["fa"], a["lens"] = legs, fa, [len(v) for v in _fasta(fa).values()]
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def _arrays(out, name):
    z = np.load(out + "_" + name + "_cov.npz")
    assert z["depth"].dtype == np.uint32 and all(z[k].dtype == np.uint64 for k in ("hist", "n_bases", "sum", "sum_n"))
    return {k: z[k] for k in ("depth", "hist", "n_bases", "sum", "sum_n")}


def check_against_sam(out, res, name, fa, D, w=0):
    """Every array of the leg against the per-base depth rebuilt from the SAM's @SQ, POS and CIGAR.  Returns (arrays, SAM records, records with I or D)."""
    got = _arrays(out, name)
    hdr, recs = _sam(out + "_" + name + ".sam")
    per, sq, m_sum, indel = cc.depth_from_sam(hdr, recs)
    seqs = _fasta(fa)
    assert [n for n, _ in sq] == list(seqs) and [ln for _, ln in sq] == [len(v) for v in seqs.values()]
    depth = np.concatenate([per[n] for n, _ in sq])
    codes = np.concatenate([np.where(np.frombuffer(seqs[n], np.uint8) == ord("N"), 4, 0) for n, _ in sq]).astype(np.uint8)
    assert len(recs) == res[name]["reads_written"] > 500 and len(np.unique(depth)) >= 3       # (the comparison is not vacuous)
    assert got["depth"].shape == depth.shape and (got["depth"] == depth).all(), np.nonzero(got["depth"] != depth)[0][:10]
    want = cc.with_genome_row(cc.tables(depth, codes, [ln for _, ln in sq], D))
    for k in ("hist", "n_bases", "sum", "sum_n"):
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), k
    assert int(got["sum"][-1]) + int(got["sum_n"][-1]) == m_sum == int(depth.sum())
    assert res[name]["mark"]["launches"] >= 1 and res[name]["mark"]["units"] > 0 and res[name]["finish"]["launches"] == 1 and res[name]["finish"]["units"] == depth.size
    if w:
        z = np.load(out + "_" + name + "_depth.npz")
        roff = np.concatenate([[0], np.cumsum([ln for _, ln in sq])])
        bins = np.concatenate([np.add.reduceat(depth[roff[r]:roff[r + 1]], np.arange(0, roff[r + 1] - roff[r], w)) for r in range(len(sq))])
        assert (z["bases"] == bins.astype(np.uint64)).all()
    return got, len(recs), indel


@pytest.mark.parametrize("case,model,layout,cov,isize", [
    ("g1_hiseq2500_pe", "Illumina_HiSeq2500", "PE", 3.0, 260),
    ("g3_hiseq2000_se", "Illumina_HiSeq2000", "SE", 2.0, 260),
    ("g2_xten_pe_nblock", "Illumina_HiSeqXTen", "PE", 3.0, 300)])
def test_arrays_equal_the_truth_sam_of_the_same_job(case, model, layout, cov, isize, models, golden_inputs, tmp_path):
    """2: truth SAM, coverage and the depth track at bins of 37 on in one yield call: the whole per-base array of every record, the
    histogram and the three sums per record and the genome row are what POS and CIGAR give; the bin sums of the array are the depth
    track's `bases`.  g2: several records and an N block."""
    fa = golden_inputs[case]
    out, res = _run(tmp_path, [dict(name="a", d=1000, w=37, sam=True)], fa, prof=models[model], cov=cov, layout=layout, seed=41, isize=isize)
    got, _, _ = check_against_sam(out, res, "a", fa, 1000, w=37)
    if case == "g2_xten_pe_nblock":
        assert got["hist"].shape[0] > 2 and int(got["n_bases"][-1]) > 0 and (got["n_bases"][:-1] > 0).all()


@pytest.mark.parametrize("variant", ["plain", "replay"])
def test_frequent_indels(variant, models, tmp_path):
    """2: the two-record genome 60000,40000 under the exact-placement profile at indel rates 0.01: more than half the reads carry I
    or D.  replay: every read with events has them drawn again (SCS_EV_REPLAY), the other branch of read_place."""
    fa = make_genome(str(tmp_path / "g.fa"), "60000,40000", 17)
    prof = _exact_profile(models["Illumina_HiSeq2500"], str(tmp_path / "x.profile"), 0.01, 0.01)
    env = seams_env(SCS_EV_REPLAY="1") if variant == "replay" else None
    out, res = _run(tmp_path, [dict(name="a", d=1000, w=37, sam=True)], fa, env=env, prof=prof, cov=4.0, layout="PE", seed=7, ber=0.0)
    _, n, indel = check_against_sam(out, res, "a", fa, 1000, w=37)
    assert indel > 0.5 * n


INV = dict(cov=12.0, layout="PE", seed=23)                 # g1 at 12x: 5760 pairs -- two batches of 4096 at SCS_TEST_BATCH_SHIFT=12


@pytest.fixture(scope="module")
def invariance(models, golden_inputs, tmp_path_factory):
    """The one PE job of check 3 through every sink, on one ctx of the seams build in two batches: computed once, shared, never changed."""
    d = tmp_path_factory.mktemp("inv")
    legs = [dict(name="cb", d=1000, sam=True), dict(name="off", d=0, sink="files"), dict(name="on", d=1000, sink="files"),
            dict(name="parts", d=1000, sink="files", writers=3, generations=2), dict(name="bgzf", d=1000, sink="files", bgzf=True),
            dict(name="null", d=1000, sink="null"), dict(name="dev", d=1000, sink="device"), dict(name="again", d=1000),
            dict(name="lds0", d=1000, sink="null", lds=0), dict(name="lds4", d=1000, sink="null", lds=4), dict(name="d3", d=3, sink="null")]
    fa = golden_inputs["g1_hiseq2500_pe"]
    out, res = _run(d, legs, fa, env=seams_env(SCS_TEST_BATCH_SHIFT="12"), prof=models["Illumina_HiSeq2500"], **INV)
    return out, res, fa


def test_invariance_over_sinks_and_table_sizes_on_one_ctx(invariance):
    """3: a callback (checked against its SAM), files, 3 writers x 2 generations, BGZF, a NULL sink, the text left in device memory, a
    second yield after set_seed (the array was zeroed), no LDS histogram and one of 4 buckets: the same arrays every time, from two
    batches; the FASTQ files with coverage on are the files with coverage off."""
    out, res, fa = invariance
    ref, _, _ = check_against_sam(out, res, "cb", fa, 1000)
    assert res["cb"]["mark"]["launches"] == res["cb"]["k_reads"]["launches"] == 2
    for name in ("on", "parts", "bgzf", "null", "dev", "again", "lds0", "lds4"):
        got = _arrays(out, name)
        for k in ref:
            assert (got[k] == ref[k]).all(), (name, k)
        assert res[name]["mark"]["launches"] == 2 and res[name]["finish"]["launches"] == 1
    assert res["off"]["mark"]["launches"] == 0 and res["off"]["finish"]["launches"] == 0 and res["off"]["mark"]["units"] == 0
    for m in ("_1.fq", "_2.fq"):
        want = open(out + "_off" + m, "rb").read()
        assert len(want) > 100000 and open(out + "_on" + m, "rb").read() == want == open(out + "_cb" + m, "rb").read()
        k = 0 if m == "_1.fq" else 1
        assert b"".join(open(p, "rb").read() for p in scssim_amd.part_paths(out + "_parts", 6)[k]) == want
        assert gzip.open(out + "_bgzf" + m + ".gz", "rb").read() == want


def test_max_depth_3_against_1000(invariance):
    """3: with max_depth 3 the buckets below 3 are those of max_depth 1000, the top bucket is the tail's sum; depths and sums do not change."""
    out, res, _ = invariance
    ref, d3 = _arrays(out, "cb"), _arrays(out, "d3")
    assert d3["hist"].shape == (ref["hist"].shape[0], 4) and (d3["hist"][:, :3] == ref["hist"][:, :3]).all()
    assert (d3["hist"][:, 3] == ref["hist"][:, 3:].sum(axis=1)).all() and int(d3["hist"][-1, 3]) > 0
    for k in ("depth", "n_bases", "sum", "sum_n"):
        assert (d3[k] == ref[k]).all(), k


def _check_file(path, names, t, D):
    gotD, summ, rows = cc.parse_file(path)
    want_summ, want_rows = cc.render(names, t, D)
    assert gotD == D and [s[0] for s in summ] == [s[0] for s in want_summ] == list(names) + ["genome"]
    for (_, g), (_, w) in zip(summ, want_summ):
        assert g[:3] == w[:3] and g[3:] == pytest.approx(w[3:], rel=1e-9, abs=1e-12)     # (the file prints ten significant digits)
    assert [r[:4] for r in rows] == [r[:4] for r in want_rows]
    assert [r[4] for r in rows] == pytest.approx([r[4] for r in want_rows], rel=1e-9)
    return summ


def test_coverage_file_and_cli(models, golden_inputs, tmp_path):
    """4: write_coverage's file is the rendering of the downloaded arrays (floats numerically): summary lines per record and for the
    genome, then genomecov's five columns for the buckets with bases; `scssim genreads --coverage-profile f --coverage-max 50 --writers 2`
    writes the same file for the same seed."""
    fa, prof = golden_inputs["g2_xten_pe_nblock"], models["Illumina_HiSeqXTen"]
    out, res = _run(tmp_path, [dict(name="api", d=50, sink="null", write=True)], fa, prof=prof, cov=3.0, layout="PE", seed=77)
    names, _, _ = scssim_amd.fasta_probe(fa)
    t = _arrays(out, "api")
    summ = _check_file(out + "_api.cov", names, t, 50)
    assert all(0.0 < s[1][8] < 1.0 and s[1][3] > 0 and s[1][1] > 0 for s in summ)          # gini, mean, N bases of every row
    pre = str(tmp_path / "cli")
    r = subprocess.run([CLI, "genreads", "-i", fa, "-m", prof, "-c", "3", "-o", pre, "--seed", "77", "--coverage-profile", pre + ".cov", "--coverage-max", "50", "--writers", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(pre + ".cov").read() == open(out + "_api.cov").read()
    assert os.path.exists(pre + ".p00_1.fq") and os.path.exists(pre + ".p01_2.fq")


def test_a_record_of_n_alone_has_a_summary_of_zeros(models, tmp_path):
    """4: records of 60000, 40000 and 20000 bases whose first 20000 are N: the third is N alone -- no bucket, no division fault, a
    summary of zeros; its N bases and whatever aligned to them are in n_bases and sum_n."""
    fa = make_genome(str(tmp_path / "g.fa"), "60000,40000,20000", 5, n_block=20000)
    out, res = _run(tmp_path, [dict(name="a", d=100, sink="null", write=True)], fa, prof=models["Illumina_HiSeq2500"], cov=3.0, layout="PE", seed=3)
    names, _, _ = scssim_amd.fasta_probe(fa)
    t = _arrays(out, "a")
    summ = dict(_check_file(out + "_a.cov", names, t, 100))
    for r in (4, 5):                                        # the two haplotypes of the third chromosome
        assert int(t["hist"][r].sum()) == 0 and int(t["n_bases"][r]) == 20000 and int(t["sum"][r]) == 0
        assert summ[names[r]][:2] == [20000, 20000] and summ[names[r]][3:] == [0.0] * 6
    assert int(t["hist"][-1].sum()) == 2 * (40000 + 20000) and res["a"]["reads_written"] > 500


_OWN = r'''
import ctypes
import numpy as np
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_coverage(1000)
fails(s.coverage_shape, SCS_EINVAL, "no genome")
fails(s.yield_reads, SCS_EINVAL, "scs_set_coverage")
s.set_coverage(0)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")       # the refusal is gone: what is missing now is the job itself
fails(lambda: s.set_coverage(65536), SCS_EINVAL, "65535")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
fails(g.coverage_shape, SCS_EINVAL, "off")
g.set_coverage(1000)
nr, D = g.coverage_shape()
assert D == 1000 and nr == len(a["lens"])
fails(g.coverage, SCS_EINVAL, "scs_download_coverage")      # before any yield
fails(lambda: g.coverage_range(0, 0, 10), SCS_EINVAL, "scs_coverage_range")
fails(lambda: g.write_coverage(a["out"] + ".cov"), SCS_EINVAL, "scs_write_coverage")
g.run(collect=False)
t = g.coverage()
assert g.coverage_kernel_time(0)["launches"] >= 1 and g.coverage_kernel_time(1)["launches"] == 1
L0 = a["lens"][0]
whole = g.coverage_range(0, 0, L0)
assert int(whole.sum()) == int(t["sum"][0]) + int(t["sum_n"][0]) > 0
assert (g.coverage_range(0, 100, 350) == whole[100:350]).all() and g.coverage_range(0, L0, L0).size == 0 and (g.coverage_range(nr - 1, a["lens"][-1] - 1, a["lens"][-1]) >= 0).all()
fails(lambda: g.coverage_range(0, 0, L0 + 1), SCS_EINVAL, "not inside")
fails(lambda: g.coverage_range(0, 11, 10), SCS_EINVAL, "not inside")
fails(lambda: g.coverage_range(nr, 0, 1), SCS_EINVAL, "not inside")
buf = (ctypes.c_uint64 * (nr + 1))()
g._L.scs_download_coverage.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_uint64]
assert g._L.scs_download_coverage(g._ctx, None, buf, None, None, nr) == SCS_EOVERFLOW
assert g._L.scs_download_coverage(g._ctx, None, None, buf, None, nr + 1) == 0 and list(buf) == t["sum"].tolist()
g.set_coverage(7)                                             # another max_depth between two yields
fails(g.coverage, SCS_EINVAL, "scs_download_coverage")
g.set_seed(5); g.yield_reads(collect=False)
t7 = g.coverage()
assert t7["hist"].shape == (nr + 1, 8) and (t7["sum"] == t["sum"]).all() and (t7["hist"][:, :7] == t["hist"][:, :7]).all() and (t7["hist"][:, 7] == t["hist"][:, 7:].sum(axis=1)).all()
assert (g.coverage_range(0, 0, L0) == whole).all()
g.set_coverage(0)
g.set_seed(5); g.yield_reads(collect=False)
assert g.coverage_kernel_time(0)["launches"] == 0 and g.coverage_kernel_time(1)["launches"] == 0
fails(g.coverage, SCS_EINVAL, "off")
fails(lambda: g.coverage_range(0, 0, 10), SCS_EINVAL, "scs_coverage_range")
g.set_coverage(1000)
g.set_seed(5); g.yield_reads(collect=False)                   # destroyed right after a yield
assert scssim_amd.live_resources()[0] > 0
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(models, golden_inputs, tmp_path):
    """5: a sharded ctx is refused at the yield call by name and is rid of the refusal after set_coverage(0); no download, range or file
    before a yield, none into too few rows, no range outside a record; another max_depth between yields works and releases the old
    arrays; off again: the yield runs and the download is refused; nothing is left once the contexts are destroyed right after a yield."""
    fa = golden_inputs["g1_hiseq2500_pe"]
    run_child(_OWN, dict(prof=models["Illumina_HiSeq2500"], fa=fa, lens=[len(v) for v in _fasta(fa).values()], out=str(tmp_path / "own")), timeout=300, ok=True)
