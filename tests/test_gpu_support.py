"""GPU tests of the site support (scs_set_site_support / scssim genreads --support): the six counters per artefact position equal
a pileup of the truth SAM of the same yield call, made in numpy (tests/support_cases.py); they do not depend on the sink, its writers, batch cuts, the
LDS table's size, the slabs of the site table or whether the text leaves the GPU; nothing else moves; the file, the CLI, the
refusals and the ownership of the buffers.  Each job runs in a child process under its own time limit; the checks run here.
Run with `-m gpu`."""
import gzip
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child
from gpu_readers import CLI, EOF_BLOCK, _exact_profile, _sam
from support_cases import pileup_from_sam

import scssim_amd

pytestmark = pytest.mark.gpu

KEYS = ("rec", "pos", "ref", "alt", "na", "ta", "nr", "tr")
SUFFIX_HEADER = [b'##INFO=<ID=DP,Number=1,Type=Integer,', b'##INFO=<ID=AD,Number=2,Type=Integer,', b'##INFO=<ID=DL,Number=1,Type=Integer,']

# one ctx, one allocated job, then a yield per leg: {name, sup (min_reads; absent: off), w (depth bin width, 0: off), sam, sink
# (callback / null / files / device), writers, generations, bgzf, env (seams set for the leg), write (the files of the table)}
_CHILD = r'''
import numpy as np
import scssim_amd
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a)
res = {}
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    with leg_env(leg.get("env", {})):
        g.set_seed(a["seed"])
        on = "sup" in leg
        g.set_site_support(on, leg.get("sup", 0))
        g.set_depth(leg.get("w", 0))
        g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
        yield_leg(g, pre, leg)
        r = dict(reads_written=g.stats()["reads_written"], k_support=g.site_support_kernel_time(), k_reads=g.kernel_times()["k_reads"])
        if leg.get("w"):
            dr, db, off = g.depth()
            np.savez(pre + "_depth.npz", reads=dr, bases=db, off=off)
        if on:
            np.savez(pre + "_support.npz", **g.site_support())
            np.savez(pre + "_sites.npz", **g.artefact_sites(leg["sup"]))
            if leg.get("write"):
                r["plain"] = g.write_site_support(pre + ".vcf")
                r["bgzf"] = g.write_site_support(pre + ".vcf.gz", bgzf=True)
                r["art"] = g.write_artefacts(pre + "_art.vcf", min_reads=leg["sup"])
            g.set_site_support(False)
    res[leg["name"]] = r
g.close()
res["live_end"] = scssim_amd.live_resources()
emit(res)
'''


def _run(tmp_path, legs, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"] = legs
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def check_against_sam(out, name):
    """All six counters at every position equal the SAM's pileup, and the site arrays are scs_artefact_sites' own."""
    z, s = np.load(out + "_" + name + "_support.npz"), np.load(out + "_" + name + "_sites.npz")
    for k in KEYS:
        assert z[k].dtype == s[k].dtype and len(z[k]) == len(s[k]) and (z[k] == s[k]).all(), (name, k)
    assert z["counts"].dtype == np.uint32 and z["counts"].shape == (len(z["na"]), 6)
    want, site_pos, fig = pileup_from_sam(out + "_" + name + ".sam", z["rec"], z["pos"])
    got = z["counts"].astype(np.int64)
    bad = np.nonzero((got != want[site_pos]).any(axis=1))[0]
    assert len(bad) == 0, (name, len(bad), bad[:5], got[bad[:5]], want[site_pos][bad[:5]])
    sites = np.arange(len(site_pos))
    ad_alt = want[site_pos, z["alt"].astype(np.int64)]
    fig.update(sites=len(site_pos), positions=len(want), observed=int((ad_alt > 0).sum()), deleted=int((want[:, 5] > 0).sum()), other=int(want[:, 4].sum()))
    dp = want[site_pos, :5].sum(axis=1)
    assert (want[site_pos, np.minimum(z["ref"], 4).astype(np.int64)] + ad_alt <= dp).all() and len(sites) == fig["sites"]
    print(name, fig)
    return z, want, site_pos, fig


JOBS = {"g1": ("g1_hiseq2500_pe", "Illumina_HiSeq2500", "PE", 3.0, 260, {}),
        "g3": ("g3_hiseq2000_se", "Illumina_HiSeq2000", "SE", 2.0, 260, {}),
        "g2": ("g2_xten_pe_nblock", "Illumina_HiSeqXTen", "PE", 3.0, 300, {}),
        "dense": ("g1_hiseq2500_pe", "Illumina_HiSeq2500", "PE", 1.0, 260, dict(ber=0.01, seed=9))}
G1 = dict(cov=3.0, layout="PE", seed=41)                    # the job of the invariance, file and CLI checks: 1200 pairs, five workgroups


@pytest.fixture(scope="module")
def g1_reference(models, golden_inputs, tmp_path_factory):
    """g1 (PE, 3x, seed 41) on the seams build, one ctx: support at min_reads 0 and 1 beside the truth SAM and the depth track, the same
    yield without support, every sink, the site table in slabs of 1000, the table's files.  Made once, shared, never changed."""
    d = tmp_path_factory.mktemp("g1")
    legs = [dict(name="off", w=100, sam=True), dict(name="m0", sup=0, w=100, sam=True, write=True), dict(name="m1", sup=1, sam=True, write=True),
            dict(name="null", sup=0, sink="null"), dict(name="files", sup=0, sink="files"), dict(name="parts", sup=0, sink="files", writers=3, generations=2),
            dict(name="bgzf", sup=0, sink="files", bgzf=True), dict(name="dev", sup=0, sink="device"),
            dict(name="slab", sup=0, sink="null", env=dict(SCS_TEST_SITE_SLAB="1000")),
            dict(name="lds16", sup=0, sink="null", write=True, env=dict(SCS_TEST_SITE_LDS="16")),
            dict(name="none", sup=4000000000, sink="null", write=True)]
    return _run(d, legs, env=seams_env(), prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], **G1)


def test_g1_counters_equal_the_truth_sam_of_the_same_yield(g1_reference):
    """1: g1 PE 3x, truth SAM and support on together, at min_reads 0 and 1.  Measured on the SAM side (the restatement, not the code
    under test): min_reads 0 -- 22834 sites at 22098 positions, 2880 reads, 36187 contributions, 18112 of them from
    reverse-strand reads, 262 sites with AD_alt > 0 (floor: 50); min_reads 1 -- 1171 sites, 224 of them with AD_alt > 0."""
    out, res = g1_reference
    z, want, site_pos, fig = check_against_sam(out, "m0")
    assert fig["sites"] == 22834 and fig["records"] == res["m0"]["reads_written"] > 2000
    assert fig["observed"] >= 50 and fig["reverse"] >= 1                      # floors: the test cannot pass on zeros
    assert res["m0"]["k_support"]["launches"] >= 1 and res["m0"]["k_support"]["units"] >= fig["records"] // 2
    z1, _, _, fig1 = check_against_sam(out, "m1")
    assert fig1["sites"] == 1171 and (z1["nr"] >= 1).all()
    assert res["off"]["k_support"]["launches"] == 0


@pytest.mark.parametrize("job", ["g3", "g2", "dense"])
def test_counters_equal_the_truth_sam_of_the_same_yield(job, models, golden_inputs, tmp_path):
    """1: g3 SE 2x; g2 PE 3x (several records, an N block, record edges); g1 at ber = 0.01 (dense: three alternate bases at a coordinate)."""
    case, model, layout, cov, isize, extra = JOBS[job]
    a = dict(prof=models[model], fa=golden_inputs[case], cov=cov, layout=layout, seed=41, isize=isize)
    a.update(extra)
    out, res = _run(tmp_path, [dict(name="s", sup=0, sam=True)], **a)
    z, want, site_pos, fig = check_against_sam(out, "s")
    assert fig["records"] == res["s"]["reads_written"] > 500 and fig["contributions"] > 1000 and fig["observed"] >= 1
    if job == "g2":
        assert len(set(z["rec"].tolist())) > 1
    if job == "dense":
        x = z["rec"].astype(np.int64) * (1 << 40) + z["pos"].astype(np.int64)
        assert np.unique(x, return_counts=True)[1].max() == 3 and fig["sites"] > 200000


def test_frequent_indels(models, golden_inputs, tmp_path):
    """1: g1 with the exact-placement model of test_gpu_truth.py at indel rates at which most reads carry events: deleted positions
    (class 5) and reads with an insertion left of a counted position.  Measured on the SAM side: 507 positions with class 5 > 0,
    1959 reads with an insertion left of a counted position, 219 sites with AD_alt > 0."""
    prof = _exact_profile(models["Illumina_HiSeq2500"], str(tmp_path / "x.profile"), 0.01, 0.01)
    out, res = _run(tmp_path, [dict(name="s", sup=0, sam=True)], prof=prof, fa=golden_inputs["g1_hiseq2500_pe"], **G1)
    z, want, site_pos, fig = check_against_sam(out, "s")
    assert fig["deleted"] >= 1 and fig["ins_left"] >= 1 and fig["reverse"] >= 1
    _, recs = _sam(out + "_s.sam")
    assert sum(1 for r in recs if "I" in r[5] or "D" in r[5]) > 0.5 * len(recs)


def _counts(out, name):
    return np.load(out + "_" + name + "_support.npz")["counts"]


def test_invariance_over_sinks_and_slabs(g1_reference):
    """2: a callback, a NULL sink, files, 3 writers x 2 generations, BGZF files, the text left in device memory, and the site table made
    in slabs of 1000 (sites on both sides of slab borders): the same counters every time -- each a yield after scs_set_seed on the
    same ctx, so every one of them is the counters of its call, not a sum."""
    out, res = g1_reference
    want = _counts(out, "m0")
    assert want.sum() > 10000
    for name in ("null", "files", "parts", "bgzf", "dev", "slab", "lds16"):
        assert (_counts(out, name) == want).all(), name
        assert res[name]["k_support"]["launches"] >= 1, name
    x = np.load(out + "_slab_support.npz")["pos"].astype(np.int64)
    assert ((x % 1000) == 999).any() and ((x % 1000) == 0).any()


@pytest.mark.parametrize("knob,value", [("SCS_TEST_BATCH_SHIFT", "7"), ("SCS_TEST_SUPPORT_SLOTS", "4"), ("SCS_TEST_SUPPORT_SLOTS", "0"), ("SCS_TEST_SUPPORT_SLOTS", "1024")])
def test_invariance_over_batch_cuts_and_table_sizes(knob, value, g1_reference, models, golden_inputs, tmp_path):
    """2: batches of 128 pairs (ten of them), an LDS table of 4 slots (most adds overflow into direct ones), none at all, and the
    default's 1024 slots by name: the counters of the reference."""
    ref_out, _ = g1_reference
    out, res = _run(tmp_path, [dict(name="v", sup=0, sink="null")], env=seams_env(**{knob: value}), prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], **G1)
    assert (_counts(out, "v") == _counts(ref_out, "m0")).all()
    if knob == "SCS_TEST_BATCH_SHIFT":
        assert res["v"]["k_support"]["launches"] == res["v"]["k_reads"]["launches"] >= 8                 # one event pair per batch


def test_nothing_else_moves(g1_reference):
    """3: FASTQ, truth SAM and depth arrays of the same ctx are byte-equal with the feature on and off."""
    out, _ = g1_reference
    for f in ("_1.fq", "_2.fq", ".sam"):
        want = open(out + "_off" + f, "rb").read()
        assert len(want) > 100000 and open(out + "_m0" + f, "rb").read() == want, f
    a, b = np.load(out + "_off_depth.npz"), np.load(out + "_m0_depth.npz")
    assert (a["reads"] == b["reads"]).all() and (a["bases"] == b["bases"]).all() and a["reads"].sum() > 2000


def _strip(text):
    """The site support file without its three header lines and without every line's ;DP=..;AD=..;DL=.. ; and those fields."""
    lines, fields = [], []
    for ln in text.split(b"\n")[:-1]:
        if any(ln.startswith(h) for h in SUFFIX_HEADER):
            continue
        if not ln.startswith(b"#"):
            ln, _, tail = ln.partition(b";DP=")
            dp, ad, dl = tail.split(b";")
            assert ad.startswith(b"AD=") and dl.startswith(b"DL=")
            fields.append((int(dp), int(ad[3:].split(b",")[0]), int(ad[3:].split(b",")[1]), int(dl[3:])))
        lines.append(ln)
    return b"".join(ln + b"\n" for ln in lines), np.array(fields, np.int64).reshape(-1, 4)


@pytest.mark.parametrize("name", ["m0", "m1", "lds16"])
def test_file(name, g1_reference):
    """4: the plain file stripped of the suffix and the three header lines is scs_write_artefacts' file at the same min_reads, byte for
    byte; its DP / AD / DL are the arrays'; the BGZF file inflates to the plain one and ends with the end-of-file block.  lds16: an
    LDS window of 16 bytes (every line straddles windows) writes the same file."""
    out, res = g1_reference
    text = open(out + "_" + name + ".vcf", "rb").read()
    assert sum(text.count(h) for h in SUFFIX_HEADER) == 3 and text.index(SUFFIX_HEADER[0]) > text.index(b"##INFO=<ID=TR,")
    body, f = _strip(text)
    assert body == open(out + "_" + name + "_art.vcf", "rb").read()
    z = np.load(out + "_" + name + "_support.npz")
    c, n = z["counts"].astype(np.int64), len(z["na"])
    assert len(f) == n == res[name]["plain"]["sites"] > 1000 and res[name]["plain"]["bytes"] == len(text)
    idx = np.arange(n)
    assert (f[:, 0] == c[:, :5].sum(axis=1)).all() and (f[:, 1] == c[idx, np.minimum(z["ref"], 4).astype(np.int64)]).all() and (f[:, 2] == c[idx, z["alt"].astype(np.int64)]).all() and (f[:, 3] == c[:, 5]).all()
    zb = open(out + "_" + name + ".vcf.gz", "rb").read()
    assert gzip.decompress(zb) == text and zb[-28:] == EOF_BLOCK and res[name]["bgzf"] == dict(sites=n, bytes=len(zb)) and len(scssim_amd.bgzf_blocks(zb)) >= 3
    if name == "lds16":
        assert text == open(out + "_m0.vcf", "rb").read()


def test_a_job_with_no_site_writes_the_header_only(g1_reference):
    out, res = g1_reference
    text = open(out + "_none.vcf", "rb").read()
    assert res["none"]["plain"] == dict(sites=0, bytes=len(text)) and text.endswith(b"\tINFO\n") and all(ln.startswith(b"#") for ln in text.split(b"\n")[:-1])
    assert _strip(text)[0] == open(out + "_none_art.vcf", "rb").read() and sum(text.count(h) for h in SUFFIX_HEADER) == 3
    zb = open(out + "_none.vcf.gz", "rb").read()
    assert gzip.decompress(zb) == text and zb[-28:] == EOF_BLOCK
    assert len(np.load(out + "_none_support.npz")["na"]) == 0


def test_cli_writes_the_bytes_of_the_api(g1_reference, models, golden_inputs, tmp_path):
    """4: `--support x.vcf.gz --support-min-reads 1` and `--support x.vcf` beside --depth and two writers."""
    out, _ = g1_reference
    base = [CLI, "genreads", "-i", golden_inputs["g1_hiseq2500_pe"], "-m", models["Illumina_HiSeq2500"], "-c", "3", "--seed", "41"]
    r = subprocess.run(base + ["-o", str(tmp_path / "a"), "--support", str(tmp_path / "a.vcf.gz"), "--support-min-reads", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["-o", str(tmp_path / "b"), "--support", str(tmp_path / "b.vcf"), "--writers", "2", "--depth", str(tmp_path / "b.tsv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    za = open(str(tmp_path / "a.vcf.gz"), "rb").read()
    assert gzip.decompress(za) == open(out + "_m1.vcf", "rb").read() and za[-28:] == EOF_BLOCK
    assert open(str(tmp_path / "b.vcf"), "rb").read() == open(out + "_m0.vcf", "rb").read()
    assert open(str(tmp_path / "a_1.fq"), "rb").read() == open(out + "_off_1.fq", "rb").read()


_OWN = r'''
import ctypes, os
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
out = a["out"]
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_site_support(True)
fails(s.yield_reads, SCS_EINVAL, "scs_set_site_support")
s.set_site_support(False)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")       # the refusal is gone: what is missing now is the job itself
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
for seed in (5, 6):                                         # the yields' own buffers exist before the census is taken
    g.set_seed(seed); g.yield_reads(collect=False)
g.set_seed(5)
before = scssim_amd.live_resources()
fails(g.site_support, SCS_EINVAL, "scs_set_site_support")   # off
g.set_site_support(True, 0)
fails(g.site_support, SCS_EINVAL, "no yield call")          # before any yield
fails(lambda: g.write_site_support(out + "_early.vcf"), SCS_EINVAL, "no yield call")
g.yield_reads(collect=False)
first = g.site_support()
assert first["counts"].sum() > 1000 and g.site_support_kernel_time()["launches"] >= 1
n = ctypes.c_uint64()
fn = g._L.scs_site_support
fn.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 9 + [ctypes.c_uint64, ctypes.c_void_p]
assert fn(g._ctx, *([None] * 9), 0, ctypes.byref(n)) == SCS_EOVERFLOW and n.value == len(first["na"]) > 10000      # cap = 0 returns the count
g._L.scs_write_site_support.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
assert g._L.scs_write_site_support(g._ctx, (out + "_flag.vcf").encode(), 2, None, None) == SCS_EINVAL and b"unknown flag" in g._L.scs_last_error(g._ctx)
fails(lambda: g.write_site_support(out + "_no_such_dir/a.vcf"), SCS_EIO, "can not open")
fails(lambda: g.write_site_support(out + "_no_such_dir/a.vcf.gz", bgzf=True), SCS_EIO, "can not open")
r = g.write_site_support(out + ".vcf")                      # the ctx stays usable
assert r["sites"] == n.value
g.set_seed(6); g.yield_reads(collect=False)
second = g.site_support()
g.set_seed(5); g.yield_reads(collect=False)
third = g.site_support()
assert (third["counts"] == first["counts"]).all() and (second["counts"] != first["counts"]).any()       # the counters of the new call, not the sum of both
assert abs(int(second["counts"].sum()) - int(first["counts"].sum())) < 0.2 * first["counts"].sum()
g.set_site_support(False)
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())
g.set_seed(5); g.yield_reads(collect=False)
assert g.site_support_kernel_time()["launches"] == 0
fails(g.site_support, SCS_EINVAL, "scs_set_site_support")
assert not os.path.exists(out + "_early.vcf") and not os.path.exists(out + "_flag.vcf")
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(g1_reference, models, golden_inputs, tmp_path):
    """5: a sharded ctx is refused at the yield call by the setter's name and is rid of the refusal once the feature is off; no
    read-out or file before a yield; cap = 0 returns the count; an unknown flag bit; an unwritable path is SCS_EIO and the ctx goes
    on; a second yield after scs_set_seed holds its own counters; scs_live_resources is back after set_site_support(0), and zero
    once the contexts are gone."""
    run_child(_OWN, dict(out=str(tmp_path / "own"), prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"]), timeout=300, ok=True)
    _, res = g1_reference
    assert res["live_end"] == [0, 0, 0, 0]


# the four per-batch side outputs of one ctx: leg "all" has them on together, then each alone after set_seed
_SIDE = r'''
import numpy as np
import scssim_amd
from gpu_child import emit, job_args
a = job_args()
out = a["out"]
g = scssim_amd.GenReads(profile=a["prof"], coverage=3.0, layout="PE", seed=41)
g.simuvars(a["fa"])                                          # no variant files: the identity lift table
g.create_frags(); g.amplify(); g.allocate_reads(0)
res = {}
for name in ("all", "sam", "depth", "depth_ref", "support"):
    on = lambda k: name in ("all", k)
    g.set_seed(41)
    g.set_truth_sam(out + "_" + name + ".sam" if on("sam") else None)
    g.set_depth(100 if on("depth") else 0); g.set_depth_ref(100 if on("depth_ref") else 0); g.set_site_support(on("support"), 0)
    f1, f2 = g.yield_reads()
    open(out + "_" + name + "_1.fq", "wb").write(f1); open(out + "_" + name + "_2.fq", "wb").write(f2)
    z = {}
    if on("depth"):
        z["hreads"], z["hbases"], _ = g.depth()
    if on("depth_ref"):
        z["reads"], z["bases"], z["copies"], _ = g.depth_ref()
    if on("support"):
        z["counts"] = g.site_support()["counts"]
    np.savez(out + "_" + name + ".npz", **z)
    res[name] = dict(reads_written=g.stats()["reads_written"], batches=g.kernel_times()["k_reads"]["launches"], k_depth=g.kernel_times()["k_depth"]["launches"],
                     k_truth=g.kernel_times()["k_truth"]["launches"], k_depth_lift=g.depth_ref_kernel_time()["launches"], k_support=g.site_support_kernel_time()["launches"])
g.close()
res["live_end"] = scssim_amd.live_resources()
emit(res)
'''


def test_all_side_outputs_in_one_yield_equal_each_alone(models, golden_inputs, tmp_path):
    """The truth SAM, both depth tracks and the site support share the code that hands a batch to their kernels: g1 as the reference
    of an identity lift table, batches of 256 pairs (many batches, both buffer sets), one yield with all four on and, after set_seed,
    one with each alone.  The SAM's bytes, both haplotype depth arrays, the three reference arrays and the support counters of
    the combined call equal the single calls'; the FASTQ text is the same five times; nothing is left after close()."""
    out = str(tmp_path / "side")
    res = run_child(_SIDE, dict(out=out, prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"]), env=seams_env(SCS_TEST_BATCH_SHIFT="8"), timeout=300)
    print(res)
    every, singles = np.load(out + "_all.npz"), {"depth": ("hreads", "hbases"), "depth_ref": ("reads", "bases", "copies"), "support": ("counts",)}
    n = res["all"]["batches"]
    assert n >= 4 and res["all"]["reads_written"] > 1000                       # at least two batches through each buffer set
    assert [res["all"][k] for k in ("k_depth", "k_depth_lift", "k_support")] == [n, n, n] and res["all"]["k_truth"] >= n   # one event pair per batch and kernel
    for name, k in (("sam", "k_truth"), ("depth", "k_depth"), ("depth_ref", "k_depth_lift"), ("support", "k_support")):
        assert [res[name][j] > 0 for j in ("k_truth", "k_depth", "k_depth_lift", "k_support")] == [j == k for j in ("k_truth", "k_depth", "k_depth_lift", "k_support")], name
        assert res[name]["reads_written"] == res["all"]["reads_written"] and res[name]["batches"] == n
    for name, keys in singles.items():
        one = np.load(out + "_" + name + ".npz")
        assert sorted(one.files) == sorted(keys)
        for k in keys:
            assert every[k].shape == one[k].shape and (every[k] == one[k]).all() and every[k].sum() > 1000, (name, k)
    sam = open(out + "_all.sam", "rb").read()
    assert len(sam) > 100000 and open(out + "_sam.sam", "rb").read() == sam
    for f in ("_1.fq", "_2.fq"):
        want = open(out + "_all" + f, "rb").read()
        assert len(want) > 100000
        for name in ("sam",) + tuple(singles):
            assert open(out + "_" + name + f, "rb").read() == want, (name, f)
    assert res["live_end"] == [0, 0, 0, 0]
