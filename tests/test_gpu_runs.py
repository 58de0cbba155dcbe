"""GPU tests of the bedGraph writer of the per-base arrays (scs_write_coverage_bedgraph, scs_write_coverage_ref_bedgraph,
scs_write_copy_number_ref / scssim genreads --coverage-bedgraph, --coverage-bedgraph-ref, --copy-number-ref):
the kernels and the slab loop alone over given arrays against the numpy restatement, byte for byte (scs_runs_probe,
tests/runs_cases.py); slab cuts and BGZF; whole jobs against the arrays read back base by base; invariance over sinks, caps and
repeated writes; the CLI; refusals and ownership.  Each job runs in a child process under its own time limit.  Run with `-m gpu`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child, sv_ref  # noqa: F401 (a fixture)
from gpu_readers import CLI, SV, Segs, _fasta, _inflate

import runs_cases as rc
import scssim_amd

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- 1: the kernels and the slab loop alone
# The child builds every case from the case table (plain numpy, seeded), runs the probe and compares there: only verdicts travel.
_PROBE = r'''
import runs_cases as rc
import scssim_amd
from gpu_child import emit
g = scssim_amd.GenReads()
T, _ = scssim_amd.coverage_tile()
res = {}
for spec in rc.table_cases():
    v, mask, lens, names = rc.case(spec, T)
    want = rc.bedgraph_text(v, mask, lens, names)
    got = scssim_amd.runs_probe(g, v, mask, lens, names)
    bad = []
    if got["data"] != want:
        bad.append("bytes (%d, wanted %d)" % (len(got["data"]), len(want)))
    if got["lines"] != want.count(b"\n"):
        bad.append("lines %d" % got["lines"])
    if got["slabs"] != 1:
        bad.append("slabs %d" % got["slabs"])
    res[rc.name_of(spec)] = "ok" if not bad else "differs: " + ", ".join(bad)
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
emit(res)
'''


def test_kernels_alone_against_numpy():
    """Lengths 1, 2, T - 1, T, T + 1, 2T + 1, 4T + 3 x six value families (one run over every tile; every base a new run; a change
    exactly at a tile's last and first entry; geometric runs; values of 1 .. 10 digits with 4294967295; under 0xFFFF words that differ
    only in the upper half) with the record layouts rotating (one record; records of length 1; a border in mid-tile; a border at a
    tile edge; 300 records, 299 of them in one tile; a name of 200 bytes), T + 1 and 4T + 3 under all of them: the bytes, the line count
    and one slab are the restatement's.  tests/test_runs_host.py proves what the cases reach."""
    res = run_child(_PROBE, {}, timeout=300)
    names = [rc.name_of(s) for s in rc.table_cases()]
    bad = {k: v for k, v in res.items() if v != "ok"}
    assert not bad and set(names) == set(res) and len(names) > 100, (dict(list(bad.items())[:10]), len(bad))


_SLABS = r'''
import zlib
import numpy as np
import runs_cases as rc
import scssim_amd
from scssim_amd import SCS_EINVAL
from gpu_child import fails
from gpu_readers import EOF_BLOCK
g = scssim_amd.GenReads()
T, _ = scssim_amd.coverage_tile()


def blocks(z):
    """the inflated size of every BGZF member but the end-of-file block, and the inflated text"""
    assert z.endswith(EOF_BLOCK)
    sizes, text, at = [], b"", 0
    while at < len(z) - len(EOF_BLOCK):
        assert z[at:at + 4] == b"\x1f\x8b\x08\x04" and z[at + 12:at + 14] == b"BC"
        size = int.from_bytes(z[at + 16:at + 18], "little") + 1
        part = zlib.decompress(z[at + 18:at + size - 8], -15)
        assert zlib.crc32(part) == int.from_bytes(z[at + size - 8:at + size - 4], "little") and len(part) == int.from_bytes(z[at + size - 4:at + size], "little")
        sizes.append(len(part)); text += part; at += size
    assert at == len(z) - len(EOF_BLOCK)
    return sizes, text


def check(v, mask, lens, names, caps):
    want, tb = rc.bedgraph_text(v, mask, lens, names), rc.tile_bytes(v, mask, lens, names, T)
    assert int(tb.sum()) == len(want)
    seen = set()
    for cap in caps(tb):
        plan = rc.plan_slabs(tb, cap or 128 << 20)         # (0: the product's default, 128 MB)
        got =scssim_amd.runs_probe(g, v, mask, lens, names, text_cap=cap)
        assert got["data"] == want and got["lines"] == want.count(b"\n") and got["slabs"] == len(plan), (cap, got["slabs"], plan)
        z = scssim_amd.runs_probe(g, v, mask, lens, names, text_cap=cap, bgzf=True)
        sizes, text = blocks(z["data"])
        assert text == want and z["slabs"] == len(plan) and z["lines"] == got["lines"]
        ends = set(np.cumsum(sizes).tolist())
        assert all(sum(s[2] for s in plan[:k]) in ends for k in range(1, len(plan) + 1)), cap     # every slab starts on a block border
        seen.add(tuple(s[:2] for s in plan))
    return seen


# one run over tiles 0 .. 2 and into tile 3, tiles 1 and 2 without a run start, tile 3 the largest
v, mask, lens, names = rc.slab_case(T)
seen = check(v, mask, lens, names, lambda tb: [int(tb.max()), int(tb[3] + tb[4]), int(tb.sum()) - 1, int(tb.sum()), 0])
assert ((0, 3), (3, 4), (4, 5), (5, 6)) in seen        # cap = the largest tile's text: a cut right behind a tile with no run start, inside the run over three tiles
assert ((0, 6),) in seen and len(seen) >= 4
# every base a new run: with cap = the largest tile's text a cut falls after every tile
v, mask, lens, names = rc.case(dict(size="4T+3", fam="alt", lay="one"), T)
seen = check(v, mask, lens, names, lambda tb: [int(tb.max())])
assert seen == {((0, 1), (1, 2), (2, 3), (3, 4), (4, 5))}
# a cap below one tile's text: refused with the bytes, and the next call on the same ctx is right
tb = rc.tile_bytes(v, mask, lens, names, T)
fails(lambda: scssim_amd.runs_probe(g, v, mask, lens, names, text_cap=int(tb.max()) - 1), SCS_EINVAL, "scs_runs_probe", "text cap", str(int(tb.max())))
fails(lambda: scssim_amd.runs_probe(g, v, mask, lens, names, text_cap=1, bgzf=True), SCS_EINVAL, "text cap")
assert scssim_amd.runs_probe(g, v, mask, lens, names, text_cap=int(tb.max()))["data"] == rc.bedgraph_text(v, mask, lens, names)
# lengths that do not add up, and nothing at all
fails(lambda: scssim_amd.runs_probe(g, v, mask, [len(v) - 1], ["a"]), SCS_EINVAL, "add up")
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_slab_cuts_and_bgzf():
    """text_cap chosen from the restatement's per-tile bytes: a cut right behind a tile with no run start and inside a run that spans
    three tiles, a cut after every tile (cap = the largest tile's text), one slab, the product's default: the same bytes, the
    restatement's slab count; as BGZF every leg inflates to the plain bytes, block by block with CRC and size, and every slab
    starts on a block border.  A cap below one tile's text is SCS_EINVAL stating the bytes and the ctx stays usable."""
    run_child(_SLABS, {}, timeout=300, ok=True)


# ---------------------------------------------------------------- 2: whole jobs
# one ctx, one genome, one yield call; then every file, and the arrays read back base by base
_JOB = r'''
import numpy as np
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a, segs="ref" in a)
pre = a["out"]
g.set_seed(a["seed"]); g.set_coverage(a["d"])
if "ref" in a:
    g.set_coverage_ref(a["d"])
yield_leg(g, pre, dict(sink="null"))
res, arrays = {}, {}
res["staged"] = g.write_coverage_bedgraph(pre + ".bg"); res["staged_time"] = g.coverage_bedgraph_kernel_time()
arrays["staged"] = np.concatenate([g.coverage_range(r, 0, n) for r, n in enumerate(a["lens"])])
t = g.coverage()
arrays["sum"], arrays["sum_n"] = t["sum"], t["sum_n"]
if "ref" in a:
    res["ref"] = g.write_coverage_ref_bedgraph(pre + "_ref.bg"); res["ref_time"] = g.coverage_bedgraph_kernel_time()
    res["cn"] = g.write_copy_number_ref(pre + "_cn.bg")
    seg = g.lift_segments()
    per = [g.coverage_ref_range(r, 0, int(seg.ref_lens[r])) for r in range(len(seg.ref_lens))]
    arrays["ref_depth"], arrays["copies"] = np.concatenate([d for d, _ in per]), np.concatenate([c for _, c in per])
    tr = g.download_coverage_ref()
    arrays["ref_sum"], arrays["ref_sum_n"] = tr["sum"], tr["sum_n"]
# again, compressed, and under a small cap (the seams build reads it at every write call): the same bytes
res["again"] = g.write_coverage_bedgraph(pre + "_again.bg")
res["gz"] = g.write_coverage_bedgraph(pre + ".bg.gz")
with leg_env({"SCS_TEST_RUNS_TEXT_CAP": str(a["cap"])}):
    res["small"] = g.write_coverage_bedgraph(pre + "_small.bg"); res["small_time"] = g.coverage_bedgraph_kernel_time()
    res["small_gz"] = g.write_coverage_bedgraph(pre + "_small.bg.gz")
    if "ref" in a:
        g.write_coverage_ref_bedgraph(pre + "_ref_small.bg.gz"); g.write_copy_number_ref(pre + "_cn_small.bg.gz")
assert (np.concatenate([g.coverage_range(r, 0, n) for r, n in enumerate(a["lens"])]) == arrays["staged"]).all()   # the writes left the array untouched
np.savez(pre + "_arrays.npz", **arrays)
emit(res)
'''


def _job(d, models, seed, fa=None, **a):
    a.update(out=str(d / "job"), prof=models["Illumina_HiSeq2500"], seed=seed, d=50, layout="PE")
    if fa:
        a["fa"] = fa
        seqs = _fasta(fa)
    res = run_child(_JOB, dict(a, lens=a.get("lens") or [len(v) for v in seqs.values()]), env=seams_env(), timeout=300)
    z = np.load(a["out"] + "_arrays.npz")
    return a["out"], res, {k: z[k] for k in z.files}


def _check_file(path, names, lens, want, info):
    """The file parsed and expanded: the records in order, every base the array's; the line and byte counts the call reported."""
    text = open(path, "rb").read()
    back = rc.parse(text)
    assert [n for n, _ in back] == list(names) and [len(v) for _, v in back] == [int(x) for x in lens]
    got = np.concatenate([v for _, v in back])
    assert got.shape == want.shape and (got == want.astype(np.int64)).all(), np.nonzero(got != want)[0][:10]
    assert info["lines"] == text.count(b"\n") > len(names) and info["text_bytes"] == len(text)
    return text


@pytest.fixture(scope="module")
def g1_job(models, golden_inputs, tmp_path_factory):
    """The g1 golden genome at 12x, one yield call, every staged file: computed once, shared, never changed."""
    return _job(tmp_path_factory.mktemp("g1"), models, 23, fa=golden_inputs["g1_hiseq2500_pe"], cov=12.0, cap=1 << 17) + (golden_inputs["g1_hiseq2500_pe"],)


def test_staged_file_of_a_whole_job(g1_job):
    """The g1 genome: the bedGraph parsed and expanded is coverage_range of every staged record, base by base; the lines tile the
    records and neighbouring values differ (parse asserts it); the value-weighted length of the lines is the profile's sum + sum_n."""
    out, res, arr, fa = g1_job
    seqs = _fasta(fa)
    text = _check_file(out + ".bg", list(seqs), [len(v) for v in seqs.values()], arr["staged"], res["staged"])
    assert rc.weighted_length(text) == int(arr["sum"][-1]) + int(arr["sum_n"][-1]) == int(arr["staged"].astype(np.int64).sum()) > 100000
    assert res["staged_time"]["units"] == arr["staged"].size and res["staged_time"]["launches"] == 2 and res["staged_time"]["ms"] > 0   # the plan passes, one slab


def test_second_write_gz_and_small_caps_give_the_same_bytes(g1_job):
    """A second write after the same yield, the .gz inflated, and both again with SCS_TEST_RUNS_TEXT_CAP small enough for several
    slabs (one event pair for the plan passes and one per slab): the same bytes, the same counts."""
    out, res, _, _ = g1_job
    want = open(out + ".bg", "rb").read()
    assert open(out + "_again.bg", "rb").read() == want == open(out + "_small.bg", "rb").read()
    assert _inflate(open(out + ".bg.gz", "rb").read()) == want == _inflate(open(out + "_small.bg.gz", "rb").read())
    assert res["again"] == res["staged"] == res["gz"] == res["small"] == res["small_gz"]
    assert res["small_time"]["launches"] >= 4 and res["small_time"]["launches"] == 1 + len(rc.plan_slabs(_tile_bytes_of(want), 1 << 17))


def _tile_bytes_of(text, T=4096):
    """bytes of text per tile from the file of ONE staged genome whose records are concatenated in file order"""
    f = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
    lens, off, at = {}, {}, 0
    for x in f:
        lens[x[0]] = int(x[2])
    for n in lens:                                         # (dicts keep the order of appearance)
        off[n] = at; at += lens[n]
    st = np.array([off[x[0]] + int(x[1]) for x in f], np.int64)
    return np.bincount(st // T, weights=[len(b"\t".join(x)) + 1 for x in f], minlength=(at + T - 1) // T).astype(np.int64)


@pytest.fixture(scope="module")
def sv_job(sv_ref, models, tmp_path_factory):
    """The golden simuvars genome through its lift table at 2x, one yield call, all three files."""
    d = tmp_path_factory.mktemp("sv")
    snp, var = os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt")
    host, _ = scssim_amd.lift_plan_probe(sv_ref, snp, var)
    return _job(d, models, 77, ref=sv_ref, snp=snp, vars=var, out_fasta=str(d / "staged.fa"), cov=2.0, cap=1 << 17, lens=[int(x) for x in host.hap_lens]) + (host, d)


def test_all_three_files_of_the_simuvars_genome(sv_job):
    """The golden simuvars genome (1.5 Mb staged, CN 0 .. 8, three reference records): the staged file against coverage_range, the
    reference depth and the copy-number files against coverage_ref_range (depth and copies) of every reference record; the
    value-weighted lengths are the profiles' sum + sum_n, the copy-number file's the lift table's R-segment bases; CN 0 is a run of 0."""
    out, res, arr, host, d = sv_job
    seqs = _fasta(str(d / "staged.fa"))
    assert [len(v) for v in seqs.values()] == [int(x) for x in host.hap_lens]
    text = _check_file(out + ".bg", list(seqs), host.hap_lens, arr["staged"], res["staged"])
    assert rc.weighted_length(text) == int(arr["sum"][-1]) + int(arr["sum_n"][-1])
    seg = Segs(out)
    assert len(host.ref_names) == 3 == len(seg.ref_lens)
    text = _check_file(out + "_ref.bg", host.ref_names, seg.ref_lens, arr["ref_depth"], res["ref"])
    assert rc.weighted_length(text) == int(arr["ref_sum"][-1]) + int(arr["ref_sum_n"][-1]) > 100000
    text = _check_file(out + "_cn.bg", host.ref_names, seg.ref_lens, arr["copies"], res["cn"])
    assert rc.weighted_length(text) == int(seg.len[seg.kind == 0].sum()) and int(arr["copies"].max()) >= 8 and (arr["copies"] == 0).any()
    assert res["cn"]["lines"] < 1000 < res["ref"]["lines"]                                    # maximal segments, not bases
    assert res["ref_time"]["units"] == arr["ref_depth"].size
    for k in ("_ref", "_cn"):                                                                # compressed, in several slabs: the same bytes
        assert _inflate(open(out + k + "_small.bg.gz", "rb").read()) == open(out + k + ".bg", "rb").read()


def test_the_cli_writes_the_librarys_files(sv_job, sv_ref, models, tmp_path):
    """`scssim simuvars --lift`, then `scssim genreads --lift` with all three options (and no --coverage-max: 1000, which no value
    depends on) writes the library's three files for the same seed, byte for byte; a .gz name is BGZF."""
    out = sv_job[0]
    snp, var = os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt")
    simu, lift, pre = str(tmp_path / "simu.fa"), str(tmp_path / "simu.lift"), str(tmp_path / "cli")
    r = subprocess.run([CLI, "simuvars", "-r", sv_ref, "-s", snp, "-v", var, "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([CLI, "genreads", "-i", simu, "-m", models["Illumina_HiSeq2500"], "-c", "2", "-o", pre, "--seed", "77", "--lift", lift,
                        "--coverage-bedgraph", pre + ".bg", "--coverage-bedgraph-ref", pre + "_ref.bg.gz", "--copy-number-ref", pre + "_cn.bg"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(pre + ".bg", "rb").read() == open(out + ".bg", "rb").read() and open(pre + "_cn.bg", "rb").read() == open(out + "_cn.bg", "rb").read()
    assert _inflate(open(pre + "_ref.bg.gz", "rb").read()) == open(out + "_ref.bg", "rb").read()


# ---------------------------------------------------------------- 3: invariance over sinks
_SINKS = r'''
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a)
g.set_coverage(1000)
res = {}
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    g.set_seed(a["seed"])
    yield_leg(g, pre, leg)
    res[leg["name"]] = g.write_coverage_bedgraph(pre + ".bg")
emit(res)
'''


def test_the_same_bytes_from_every_sink(g1_job, models, tmp_path):
    """A callback, a NULL sink and the text left in device memory, in two batches (SCS_TEST_BATCH_SHIFT=12) and slabs of 128 KB: the
    file of the shared job, which ran with max_depth 50 in one batch and one slab -- values are never clamped by max_depth."""
    out, _, _, fa = g1_job
    legs = [dict(name="cb"), dict(name="null", sink="null"), dict(name="dev", sink="device")]
    res = run_child(_SINKS, dict(out=str(tmp_path / "s"), legs=legs, fa=fa, prof=models["Illumina_HiSeq2500"], cov=12.0, layout="PE", seed=23),
                    env=seams_env(SCS_TEST_BATCH_SHIFT="12", SCS_TEST_RUNS_TEXT_CAP=str(1 << 17)), timeout=300)
    want = open(out + ".bg", "rb").read()
    for leg in legs:
        assert open(str(tmp_path / "s") + "_" + leg["name"] + ".bg", "rb").read() == want, leg["name"]
        assert res[leg["name"]]["lines"] == want.count(b"\n")


# ---------------------------------------------------------------- 4: refusals and ownership
_OWN = r'''
import os
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO
from gpu_child import fails, job_args
a = job_args()
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
p = a["out"] + ".bg"
g.set_coverage(1000)
fails(lambda: g.write_coverage_bedgraph(p), SCS_EINVAL, "scs_write_coverage_bedgraph", "no yield call with the coverage profile on (scs_set_coverage) has finished")   # before any yield
g.set_coverage(0)
g.yield_reads(collect=False)
before = scssim_amd.live_resources()                         # (what a yield keeps is there)
g.set_coverage(1000)
fails(lambda: g.write_coverage_bedgraph(p), SCS_EINVAL, "scs_write_coverage_bedgraph", "no yield call with the coverage profile on")   # the yield ran with it off
assert not os.path.exists(p)
g.set_seed(5); g.yield_reads(collect=False)
first = g.write_coverage_bedgraph(p)
want = open(p, "rb").read()
assert first["lines"] == want.count(b"\n") > 10 and first["text_bytes"] == len(want)
assert g.coverage_bedgraph_kernel_time()["launches"] == 2 and scssim_amd.live_resources()[0] > before[0]
# the -ref writes without a lift table (and without scs_set_coverage_ref)
fails(lambda: g.write_coverage_ref_bedgraph(p + ".ref"), SCS_EINVAL, "scs_write_coverage_ref_bedgraph", "scs_set_coverage_ref")
fails(lambda: g.write_copy_number_ref(p + ".cn"), SCS_EINVAL, "scs_write_copy_number_ref", "scs_set_coverage_ref")
assert not os.path.exists(p + ".ref") and not os.path.exists(p + ".cn")
# a path in a missing directory: SCS_EIO, and a good write on the same ctx
fails(lambda: g.write_coverage_bedgraph(a["out"] + "_missing/x.bg"), SCS_EIO, "scs_write_coverage_bedgraph", "can not open")
fails(lambda: g.write_coverage_bedgraph(a["out"] + "_missing/x.bg.gz"), SCS_EIO, "can not open")
fails(lambda: g.write_coverage_bedgraph(""), SCS_EINVAL, "no path")
assert g.write_coverage_bedgraph(p + ".2") == first and open(p + ".2", "rb").read() == want
# after scs_set_coverage(ctx, 0): refused, and nothing of the feature is left
g.set_coverage(0)
fails(lambda: g.write_coverage_bedgraph(p + ".3"), SCS_EINVAL, "scs_write_coverage_bedgraph")
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())
assert g.coverage_bedgraph_kernel_time()["launches"] == 0
# the reference switch without a lift table: the yield call is refused, so no write can follow
g.set_coverage_ref(1000)
fails(lambda: g.write_copy_number_ref(p + ".cn"), SCS_EINVAL, "scs_write_copy_number_ref")
g.set_coverage_ref(0)
# destroyed directly behind a write
g.set_coverage(7); g.set_seed(5); g.yield_reads(collect=False)
assert g.write_coverage_bedgraph(p + ".gz")["lines"] == first["lines"]
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(models, golden_inputs, tmp_path):
    """A write before any yield and after scs_set_coverage(ctx, 0) is SCS_EINVAL in scs_write_coverage's words; the -ref writes
    without a lift table are SCS_EINVAL and leave no file; a path in a missing directory is SCS_EIO and a good write on the same ctx
    follows with the same bytes; the live resources read the same before the feature goes on and after it goes off, and zero after
    `delete ctx` directly behind a write."""
    own = dict(prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], out=str(tmp_path / "own"))
    run_child(_OWN, own, timeout=300, ok=True)
