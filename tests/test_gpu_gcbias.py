"""GPU tests of the GC-bias table of the per-base depth (scs_gc_bias, scs_write_gc_bias / scssim genreads --gc-bias, --gc-window;
DESIGN.md section 23): the kernel alone over given arrays against the numpy restatement, bit for bit (scs_gc_bias_probe,
tests/gcbias_cases.py); whole jobs against the restatement run over the arrays read back base by base and the FASTA's codes; the
identities at a window of one base; invariance over sinks and batch cuts; the file and the CLI; refusals and ownership.  Each job
runs in a child process under its own time limit.  Run with `-m gpu`."""
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child
from gpu_readers import CLI, _fasta, make_genome

import gcbias_cases as gc
import scssim_amd

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- 1: the kernel alone
# The child builds every case from the case table (plain numpy, seeded), runs the probe and compares there: only verdicts travel.
_PROBE = r'''
import gcbias_cases as gc
import scssim_amd
from gpu_child import emit, job_args
big = job_args()["big"]
g = scssim_amd.GenReads()
T, _ = scssim_amd.coverage_tile()
res = {}
for spec in gc.table_cases():
    if (spec["size"] in gc.BIG) != big:
        continue
    depth, codes, lens, W, lds = gc.case(spec, T)
    bad = gc.same(scssim_amd.gc_bias_probe(g, depth, codes, lens, W, lds), gc.reference(depth, codes, lens, W))
    res[gc.name_of(spec)] = "ok" if not bad else "differs: " + ", ".join(bad)
t = g.gc_bias_kernel_time()
assert t["launches"] == 1 and t["units"] == len(depth) and t["ms"] > 0, t
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
emit(res)
'''


def _verdicts(big):
    res = run_child(_PROBE, dict(big=big), timeout=300)
    names = [gc.name_of(s) for s in gc.table_cases() if (s["size"] in gc.BIG) == big]
    bad = {k: v for k, v in res.items() if v != "ok"}
    assert not bad and set(names) == set(res), (dict(list(bad.items())[:10]), len(bad))
    return names


def test_kernel_alone_against_numpy():
    """Sizes 1 .. 2T + 1 (T - 1, T, T + 1, T + W - 2, T + W - 1, T + W among them) x windows 1, 2, 7, 63, 64, 65, 100, 1000, 1024,
    every pair with and without the LDS table; under them rotate one record / records of 1, 2, 37, W - 1, W, W + 1, T - 1, T, T + 1 /
    a border inside a halo, seven code families (random, all G/C, all A/T, a GC ramp, all N, N blocks over tile and record borders, a
    single N at a tile's last base) and five depth families (zeros, ones, read-like, a pile of 70 000, a stretch near 2^31 whose
    window sums pass 2^32): windows, depth_sum and n_windows are the restatement's, bit for bit.  tests/test_gcbias_host.py proves
    what the cases reach."""
    assert len(_verdicts(False)) > 250


def test_many_workgroups_flush_into_one_row():
    """1 000 003 bases (245 tiles; the GC ramp at a window of 100: every bin) as one record and as many, with and without the LDS
    table, and 4 T x 1024 + 1 bases at a window of 1024: 4097 workgroups add to one row."""
    assert len(_verdicts(True)) == 3


# ---------------------------------------------------------------- 2: whole jobs
_JOB = r'''
import numpy as np
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a)
pre = a["out"]
g.set_seed(a["seed"]); g.set_coverage(a["d"])
yield_leg(g, pre, dict(sink="null"))


def arrays():
    t = g.coverage()
    return dict(t, depth=np.concatenate([g.coverage_range(r, 0, n) for r, n in enumerate(a["lens"])]))


before = arrays()
res, keep = dict(time={}), dict(before)
for W in a["windows"]:
    t = g.gc_bias(W)
    res["time"][str(W)] = g.gc_bias_kernel_time()
    for k in ("windows", "depth_sum", "n_windows"):
        keep["w%d_%s" % (W, k)] = t[k]
    assert t["mean_depth"].shape == t["normalized"].shape == t["windows"].shape and t["row_mean"].shape == t["n_windows"].shape
between = arrays()                                         # a download between two table calls
t = g.gc_bias(a["windows"][0])                             # ... and the first window again, behind the others
res["again"] = all((t[k] == keep["w%d_%s" % (a["windows"][0], k)]).all() for k in ("windows", "depth_sum", "n_windows"))
g.write_gc_bias(pre + ".gc", a["file_window"])
g.write_gc_bias(pre + "_default.gc")
after = arrays()
res["untouched"] = all((before[k] == between[k]).all() and (before[k] == after[k]).all() for k in before)
res["reads_written"] = g.stats()["reads_written"]
np.savez(pre + "_arrays.npz", **keep)
g.close()
emit(res)
'''

JOBS = {"g1": ("g1_hiseq2500_pe", "Illumina_HiSeq2500", 12.0, 23), "g2": ("g2_xten_pe_nblock", "Illumina_HiSeqXTen", 3.0, 77), "nblock": (None, "Illumina_HiSeq2500", 3.0, 3)}
WINDOWS = [1, 100, 1000]


@pytest.fixture(scope="module")
def jobs(models, golden_inputs, tmp_path_factory):
    """The golden genomes g1 and g2 (several records, an N block) and a generated genome whose third chromosome is N alone: one yield
    call each with coverage on, the table at windows of 1, 100 and 1000, the file.  Computed once per genome, shared, never changed."""
    made = {}

    def job(name):
        if name not in made:
            d = tmp_path_factory.mktemp(name)
            case, model, cov, seed = JOBS[name]
            fa = golden_inputs[case] if case else make_genome(str(d / "g.fa"), "60000,40000,20000", 5, n_block=20000)
            seqs = _fasta(fa)
            a = dict(out=str(d / "job"), fa=fa, prof=models[model], cov=cov, seed=seed, layout="PE", d=50, windows=WINDOWS, file_window=100, lens=[len(v) for v in seqs.values()])
            res = run_child(_JOB, a, timeout=300)
            z = np.load(a["out"] + "_arrays.npz")
            made[name] = (a, res, {k: z[k] for k in z.files}, seqs)
        return made[name]
    return job


@pytest.mark.parametrize("name", sorted(JOBS))
def test_table_of_a_whole_job(name, jobs):
    """gc_bias(W), W = 1, 100, 1000, is the restatement run over coverage_range of every whole record and the codes of the FASTA, with
    the genome's row the sum of the records'; a second call with the first window behind the others returns the first's table, and
    scs_download_coverage and scs_coverage_range answer the same before, between and after."""
    a, res, arr, seqs = jobs(name)
    codes = np.concatenate([gc.codes_of(v) for v in seqs.values()])
    assert arr["depth"].dtype == np.uint32 and arr["depth"].shape == codes.shape and res["reads_written"] > 500 and len(np.unique(arr["depth"])) >= 3
    for W in WINDOWS:
        want = gc.with_genome_row(gc.reference(arr["depth"], codes, a["lens"], W))
        got = {k: arr["w%d_%s" % (W, k)] for k in want}
        assert not gc.same(got, want), W
        assert int(got["windows"][-1].sum()) + int(got["n_windows"][-1]) == sum(max(0, n - W + 1) for n in a["lens"]) > 0
        assert res["time"][str(W)]["launches"] == 1 and res["time"][str(W)]["units"] == codes.size and res["time"][str(W)]["ms"] > 0
    assert res["again"] and res["untouched"]
    if name != "g1":
        assert int(arr["w100_n_windows"][-1]) > 0 and len(a["lens"]) > 2


@pytest.mark.parametrize("name", sorted(JOBS))
def test_a_window_of_one_base_is_the_coverage_profile(name, jobs):
    """At W = 1 a window is a base: per record and for the genome windows[0] + windows[100] are the histogram's bases, depth_sum[0] +
    depth_sum[100] is scs_download_coverage's sum, n_windows its n_bases, and no other bin holds anything."""
    _, _, arr, _ = jobs(name)
    w, s = arr["w1_windows"].astype(np.int64), arr["w1_depth_sum"].astype(np.int64)
    assert (w[:, 0] + w[:, 100] == arr["hist"].astype(np.int64).sum(axis=1)).all() and (w[:, 1:100] == 0).all()
    assert (s[:, 0] + s[:, 100] == arr["sum"].astype(np.int64)).all() and (arr["w1_n_windows"] == arr["n_bases"]).all() and int(s.sum()) > 100000


def test_the_file_is_the_rendering_of_the_table(jobs):
    """write_gc_bias's bytes are the restatement's rendering of gc_bias's table: the integer columns, the three double columns as
    "%.6f" of the integer quotients, model as "%.6g" of the profile's gc_means read from the .profile text, the genome's rows last;
    the default window is 100.  g2: several records, windows with N."""
    a, _, arr, seqs = jobs("g2")
    t = {k: arr["w100_" + k] for k in ("windows", "depth_sum", "n_windows")}
    want = gc.render(list(seqs), t, 100, gc.profile_gc_means(a["prof"]))
    got = open(a["out"] + ".gc").read()
    assert got == want == open(a["out"] + "_default.gc").read()
    rows = [ln.split("\t") for ln in got.split("\n")[:-1] if not ln.startswith("#")]
    order = list(dict.fromkeys(r[0] for r in rows))        # (first appearances; a record without a counted window has no row)
    assert len(rows) > 3 * len(seqs) and order[-1] == "genome" and order[:-1] == [n for n in seqs if n in order] and len(order) > 2
    assert any(float(r[5]) > 0 for r in rows) and all(r[6] != "." for r in rows)


def test_the_cli_writes_the_librarys_file(jobs, tmp_path):
    """`scssim genreads --gc-bias f --gc-window 1000` and, without --gc-window, the default of 100 write write_gc_bias's bytes for the
    same seed; the option switches the per-base array on by itself."""
    a, _, arr, seqs = jobs("g1")
    case, model, cov, seed = JOBS["g1"]
    for extra, W in ((["--gc-window", "1000"], 1000), ([], 100)):
        pre = str(tmp_path / ("cli%d" % W))
        r = subprocess.run([CLI, "genreads", "-i", a["fa"], "-m", a["prof"], "-c", "%g" % cov, "-o", pre, "--seed", str(seed), "--gc-bias", pre + ".gc"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        t = {k: arr["w%d_%s" % (W, k)] for k in ("windows", "depth_sum", "n_windows")}
        assert open(pre + ".gc").read() == gc.render(list(seqs), t, W, gc.profile_gc_means(a["prof"]))
    assert open(pre + ".gc").read() == open(a["out"] + ".gc").read()


# ---------------------------------------------------------------- 3: invariance over sinks and batch cuts
_SINKS = r'''
import numpy as np
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a)
g.set_coverage(1000)
res, first = {}, None
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    g.set_seed(a["seed"])
    yield_leg(g, pre, leg)
    t = g.gc_bias(100)
    if first is None:
        first = t
        np.savez(a["out"] + "_table.npz", **{k: t[k] for k in ("windows", "depth_sum", "n_windows")})
    res[leg["name"]] = all((t[k] == first[k]).all() for k in t)
res["batches"] = g.kernel_times()["k_reads"]["launches"]
emit(res)
'''


def test_the_same_table_from_every_sink_and_batch_cut(jobs, tmp_path):
    """A callback, a NULL sink, files and the text left in device memory, in two batches (SCS_TEST_BATCH_SHIFT=12) on the seams
    build with max_depth 1000: the table of the shared job, which ran on the product library with max_depth 50 in one batch."""
    a, _, arr, _ = jobs("g1")
    legs = [dict(name="cb"), dict(name="null", sink="null"), dict(name="files", sink="files"), dict(name="dev", sink="device")]
    res = run_child(_SINKS, dict(out=str(tmp_path / "s"), legs=legs, fa=a["fa"], prof=a["prof"], cov=a["cov"], layout="PE", seed=a["seed"]),
                    env=seams_env(SCS_TEST_BATCH_SHIFT="12"), timeout=300)
    assert all(res[leg["name"]] for leg in legs) and res["batches"] == 2
    z = np.load(str(tmp_path / "s") + "_table.npz")
    for k in ("windows", "depth_sum", "n_windows"):
        assert (z[k] == arr["w100_" + k]).all(), k


# ---------------------------------------------------------------- 4: refusals and ownership
_OWN = r'''
import os
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
p = a["out"] + ".gc"
NOT_YET = "no yield call with the coverage profile on (scs_set_coverage) has finished"
fails(lambda: g.gc_bias(100), SCS_EINVAL, "scs_set_coverage")                                  # coverage off
fails(lambda: g.write_gc_bias(p), SCS_EINVAL, "scs_write_gc_bias", NOT_YET)
g.set_coverage(1000)
fails(lambda: g.gc_bias(100), SCS_EINVAL, "scs_gc_bias", NOT_YET)                              # before any yield
fails(lambda: g.write_gc_bias(p), SCS_EINVAL, "scs_write_gc_bias", NOT_YET)
g.set_coverage(0)
g.yield_reads(collect=False)
before = scssim_amd.live_resources()                         # (what a yield keeps is there)
g.set_coverage(1000)
fails(lambda: g.gc_bias(100), SCS_EINVAL, "scs_gc_bias", NOT_YET)                              # the yield ran with it off
assert not os.path.exists(p)
g.set_seed(5); g.yield_reads(collect=False)
with_array = scssim_amd.live_resources()
nr, _ = g.coverage_shape()
first = g.gc_bias(100)
assert first["windows"].shape == (nr + 1, 101) and int(first["windows"][-1].sum()) > 1000
assert g.gc_bias_kernel_time()["launches"] == 1 and scssim_amd.live_resources()[0] > with_array[0]   # the table's buffer is the ctx's
# windows outside 1 .. 1024, too few rows, bad paths: refused, and the ctx stays usable
for w in (0, 1025):
    fails(lambda: g.gc_bias(w), SCS_EINVAL, "scs_gc_bias", "window of %d bases" % w)
    fails(lambda: g.write_gc_bias(p, w), SCS_EINVAL, "scs_write_gc_bias", "window of %d bases" % w)
fails(lambda: g.gc_bias(100, cap_rows=nr), SCS_EOVERFLOW, "scs_gc_bias", "%d rows" % (nr + 1), "room for %d" % nr)
fails(lambda: g.write_gc_bias(a["out"] + "_missing/x.gc"), SCS_EIO, "scs_write_gc_bias", "can not open")
fails(lambda: g.write_gc_bias(""), SCS_EINVAL, "no path")
assert not os.path.exists(p)
again = g.gc_bias(100)
assert all((again[k] == first[k]).all() for k in first)
g.write_gc_bias(p)
assert open(p).read().startswith("#gc_bias\twindow=100\t")
# after scs_set_coverage(ctx, 0): refused, and nothing of the feature is left
g.set_coverage(0)
fails(lambda: g.gc_bias(100), SCS_EINVAL, "scs_set_coverage")
fails(lambda: g.write_gc_bias(p + ".2"), SCS_EINVAL, "scs_write_gc_bias", NOT_YET)
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())
assert g.gc_bias_kernel_time()["launches"] == 0 and not os.path.exists(p + ".2")
# another genome staged: the table's buffer goes with the rows it was sized for
g.set_coverage(7); g.set_seed(5); g.yield_reads(collect=False)
g.gc_bias(1024)
held = scssim_amd.live_resources()[0]
g.load_genome(a["fa"])
assert scssim_amd.live_resources()[0] < held
fails(lambda: g.gc_bias(100), SCS_EINVAL, "scs_gc_bias", NOT_YET)
# destroyed directly behind a call
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_seed(5); g.yield_reads(collect=False)
last = g.gc_bias(100)
assert int(last["windows"][-1].sum()) == int(first["windows"][-1].sum()) and (last["n_windows"] == first["n_windows"]).all()   # (the windows are the genome's, whatever the reads)
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(models, golden_inputs, tmp_path):
    """A call with coverage off, before any yield, after a yield that ran with it off and after scs_set_coverage(ctx, 0) is SCS_EINVAL
    naming scs_set_coverage; windows of 0 and 1025 are SCS_EINVAL, cap_rows one short SCS_EOVERFLOW, a path in a missing directory
    SCS_EIO, and the same table follows on the same ctx.  The table's buffer is the ctx's: it goes when coverage goes off (the live
    resources read as before the feature) and when another genome is staged, and `delete ctx` directly behind a call leaves nothing."""
    own = dict(prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], out=str(tmp_path / "own"))
    run_child(_OWN, own, timeout=300, ok=True)
