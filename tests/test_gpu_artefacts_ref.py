"""GPU tests of the artefact table on the original reference (scs_write_artefacts_ref / scs_artefact_ref_sites / `scssim genreads
--lift --artefacts-ref`).  The reference side of every check is the per-base restatement of
tests/site_ref_cases.py over what the SAME ctx reports: amplicon_places(), download_read_numbers(), artefact_sites(0), the staged
bases and lift_segments().  The golden simuvars genome; the dense layout of tests/lift_cases.py with het substitutions and a raised
error rate, held to what it must reach; a plain genome; slab, chunk and LDS edges, BGZF and a second call; nothing else moves; the
two-step CLI flow; refusals and ownership.  Each job runs in a child process under its own time limit; the checks run here.
Run with `-m gpu`."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child, sv_ref  # noqa: F401 (a fixture)
from gpu_readers import CLI, SV, Segs, _inflate, _same, make_genome
from lift_cases import write_dense_het_inputs
from site_ref_cases import KEYS, conservation, header, pieces_of, restate

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one genome (built by simuvars, or a FASTA and its lift file), one allocated job: the table as VCF (min_reads 0 and 1, BGZF,
# a second call) and as arrays, what the restatement reads from the same ctx, then the plain file again under each variant's seams
# (read at every call by the seams build).  moves: the haplotype table, a yield with site support and its table, before and after.
_CHILD = r'''
import numpy as np
import scssim_amd
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a, lift_file=True, segs=True)
out = a["out"]
res = {}
import time
t0 = time.time(); res["times"] = []
def lap(what):
    global t0
    res["times"].append((what, round(time.time() - t0, 2))); t0 = time.time()
lap("stage + amplify + allocate")
def moves(tag):
    res["hap_" + tag] = g.write_artefacts(out + "_hap_" + tag + ".vcf")
    np.savez(out + "_hapsites_" + tag + ".npz", **g.artefact_sites())
    g.set_site_support(True, 0); g.set_seed(a["seed"])
    yield_leg(g, out + "_" + tag, {})
    g.write_site_support(out + "_sup_" + tag + ".vcf")
    g.set_site_support(False)
if a.get("moves"):
    moves("before"); lap("moves")
live0 = scssim_amd.live_resources()
res["plain"] = g.write_artefacts_ref(out + ".vcf"); res["kt"] = g.artefact_ref_kernel_time()
res["live0"], res["live1"] = live0, scssim_amd.live_resources()
res["min1"] = g.write_artefacts_ref(out + "_m1.vcf", min_reads=1)
res["bgzf"] = g.write_artefacts_ref(out + ".vcf.gz", bgzf=True)
res["none"] = g.write_artefacts_ref(out + "_none.vcf", min_reads=4000000000)
res["none_bgzf"] = g.write_artefacts_ref(out + "_none.vcf.gz", bgzf=True, min_reads=4000000000)
res["again"] = g.write_artefacts_ref(out + "_again.vcf")
res["kt_before_arrays"] = g.artefact_ref_kernel_time()         # (of a call that wrote every site)
for m in (0, 1):
    s = g.artefact_ref_sites(m)
    res["unlifted%d" % m] = s.pop("unlifted")
    np.savez(out + "_sites%d.npz" % m, **s)
res["kt_after_arrays"] = g.artefact_ref_kernel_time()
res["live2"] = scssim_amd.live_resources()
lap("the table in every form")
if a.get("moves"):
    moves("after"); lap("moves")
np.savez(out + "_places.npz", **g.amplicon_places())
np.savez(out + "_hap.npz", **g.artefact_sites(0))
np.save(out + "_rn.npy", g.download_read_numbers())
np.save(out + "_codes.npy", g.download_genome()["codes"])
for v in a.get("variants", []):
    with leg_env(v["env"]):
        res[v["name"]] = g.write_artefacts_ref(out + "_" + v["name"] + ".vcf")
        if v.get("bgzf"):
            g.write_artefacts_ref(out + "_" + v["name"] + ".vcf.gz", bgzf=True)
    lap(v["name"])
emit(res)
'''


def _run(out, env=None, timeout=300, **a):
    a["out"] = str(out)
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


class Inputs:
    """What the restatement takes, read back from the job's own ctx."""
    def __init__(self, out):
        pl, hs = np.load(out + "_places.npz"), np.load(out + "_hap.npz")
        self.table = scssim_amd.lift_file_probe(out + ".lift")
        self.seg = Segs(out)
        self.hap_off = np.concatenate([[0], np.cumsum(np.asarray(self.table.hap_lens, np.int64))])
        self.starts, self.lens, self.reads = self.hap_off[pl["rec"].astype(np.int64)] + pl["start"].astype(np.int64), pl["len"].astype(np.int64), np.load(out + "_rn.npy").astype(np.int64)
        self.G = np.load(out + "_codes.npy")
        self.hap = {k: hs[k].astype(np.int64) for k in hs.files}
        self.ed_g = self.hap_off[self.hap["rec"]] + self.hap["pos"]
        assert len(self.G) == self.hap_off[-1] and (self.G[self.ed_g] == self.hap["ref"]).all() and int(pl["n_edits"].sum()) == int(self.hap["na"].sum())
        self.ref_lens, self.ref_names = [int(v) for v in self.table.ref_lens], list(self.table.ref_names)
        assert self.seg.ref_lens.tolist() == self.ref_lens

    def restate(self, min_reads=0):
        return restate(self.starts, self.lens, self.reads, self.ed_g, self.hap["alt"], self.hap["na"], self.hap["nr"], self.G, self.seg, self.ref_lens, self.ref_names, min_reads)


def check_job(out, res, what):
    """The file (plain, min_reads 1, BGZF, a second call, no site at all) and the arrays of a job equal the restatement of its own
    ctx's tables byte for byte; the conservation laws hold.  Returns (inputs, restated arrays, unlifted, per-base extras)."""
    inp = Inputs(out)
    want, arr, unl, extra = inp.restate()
    hd = header(inp.ref_names, inp.ref_lens, unl)
    _same(open(out + ".vcf").read(), hd + want, what + " min_reads 0")
    assert res["plain"] == dict(sites=len(arr["na"]), bytes=len(hd + want), unlifted_entries=unl[0], unlifted_reads=unl[1]) and len(arr["na"]) > 100
    assert [ln for ln in hd.split("\n") if ln.startswith("##contig")] == ["##contig=<ID=%s,length=%d>" % nl for nl in zip(inp.ref_names, inp.ref_lens)]
    want1, arr1, unl1, _ = inp.restate(1)
    assert unl1 == unl and want1 == "".join(ln + "\n" for ln in want.split("\n")[:-1] if ";NR=0;" not in ln) and 0 < len(arr1["na"]) < len(arr["na"])
    _same(open(out + "_m1.vcf").read(), hd + want1, what + " min_reads 1")
    assert res["min1"]["sites"] == len(arr1["na"])
    assert open(out + "_again.vcf").read() == hd + want and res["again"] == res["plain"]
    assert _inflate(open(out + ".vcf.gz", "rb").read()).decode() == hd + want and gzip.open(out + ".vcf.gz").read().decode() == hd + want
    assert res["bgzf"]["sites"] == res["plain"]["sites"] and res["bgzf"]["bytes"] == os.path.getsize(out + ".vcf.gz")
    assert open(out + "_none.vcf").read() == hd and res["none"]["sites"] == 0 and _inflate(open(out + "_none.vcf.gz", "rb").read()).decode() == hd
    for m, ref in ((0, arr), (1, arr1)):
        z = np.load(out + "_sites%d.npz" % m)
        assert z["ref_rec"].dtype == np.uint32 and z["pos"].dtype == np.uint64 and z["ref"].dtype == np.uint8 and z["nr"].dtype == np.uint64
        for k in KEYS:
            assert len(z[k]) == len(ref[k]) and (z[k].astype(np.int64) == ref[k]).all(), (m, k)
        assert tuple(res["unlifted%d" % m]) == unl
    assert (arr["na"] >= 1).all() and (arr["na"] <= arr["ta"]).all() and (arr["nr"] <= arr["tr"]).all()
    conservation(arr, unl, extra, inp.starts, inp.lens, int(inp.hap["na"].sum()), int(inp.hap["nr"].sum()))
    # ownership: the call's buffers, streams and events are gone when it returns; only the timed call moves the timer
    assert res["live0"] == res["live1"] == res["live2"]
    assert res["kt"]["launches"] >= 2 and res["kt"]["units"] == len(arr["na"]) and res["kt"]["ms"] > 0
    assert res["kt_before_arrays"]["units"] == len(arr["na"]) > 0 and res["kt_after_arrays"] == res["kt_before_arrays"]   # the array calls neither reset nor move the timer
    return inp, arr, unl, extra


def test_golden_simuvars_genome(sv_ref, models, tmp_path):
    """1: the golden simuvars genome (1.5 Mb staged, CN 0 .. 8, het insertions / deletions / substitutions, three reference records),
    PE HiSeq2500 at 2x, the default error rate: file and arrays equal the restatement at min_reads 0 and 1; the contig lines are the
    table's reference records; the conservation laws; nothing lifts into the CN-0 stretch."""
    out, res = _run(tmp_path / "job", prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, layout="PE", seed=41)
    inp, arr, unl, extra = check_job(out, res, "golden")
    assert inp.ref_lens == [400000, 150000, 60000] and len(inp.seg) == 92
    assert (extra["ta"][149999:160000] == 0).all() and not ((arr["ref_rec"] == 0) & (arr["pos"] >= 149999) & (arr["pos"] < 160000)).any()   # c chr20 150000 160000 0 0
    assert len(np.unique(arr["ref_rec"])) == 3 and extra["ta"].max() > 2 * np.median(extra["ta"][extra["ta"] > 0])


# ---- 2: the dense case
DENSE_BER, DENSE_COV, DENSE_SEED = 0.01, 6.0, 19
DENSE_VARIANTS = [dict(name="slab3", env=dict(SCS_TEST_SITE_SLAB="20000")),                       # 3 slabs
                  dict(name="slab1200", env=dict(SCS_TEST_SITE_SLAB="50")),                       # 1200 slabs: more than the counting pass sums in LDS; a copy junction jumps 80 slabs back
                  dict(name="chunk257", env=dict(SCS_TEST_AMP_CHUNK="257")), dict(name="lds16", env=dict(SCS_TEST_SITE_LDS="16")),
                  dict(name="all", env=dict(SCS_TEST_SITE_SLAB="977", SCS_TEST_AMP_CHUNK="4099", SCS_TEST_SITE_LDS="16", SCS_TEST_SITE_PIECE="65521"), bgzf=True)]


@pytest.fixture(scope="module")
def dense_job(models, tmp_path_factory):
    """The dense layout with het substitutions at ber = 0.01 on the seams build: the table in every form, again under the seams, and
    the haplotype table, the reads and the support table before and after.  Made once, shared, never changed."""
    d = tmp_path_factory.mktemp("dense_ref")
    ref, var = write_dense_het_inputs(d)
    return _run(d / "job", env=seams_env(), prof=models["Illumina_HiSeq2500"], ref=ref, vars=var, cov=DENSE_COV, layout="PE", seed=DENSE_SEED, ber=DENSE_BER,
                variants=DENSE_VARIANTS, moves=True) + (ref, var)


def test_dense_layout_reaches_what_it_must(dense_job):
    """2: about 2000 segments in 60 kb of reference: an amplicon of 1 to 2 kb is cut into many pieces.  What the job reaches is
    computed from the restatement's inputs and asserted before the comparison is relied on."""
    out, res, _, _ = dense_job
    print("times", res["times"])
    inp, arr, unl, extra = check_job(out, res, "dense")
    seg = inp.seg
    assert len(seg) > 1500
    pcs = [pieces_of(int(s), int(l), seg, inp.ref_lens) for s, l in zip(inp.starts, inp.lens)]
    n_pieces = np.array([len(p) for p in pcs])
    overlap = sum(1 for p in pcs if any(a[0] < b[1] and b[0] < a[1] for i, a in enumerate(p) for b in p[i + 1:]))
    X = extra["X"]
    xe = X[inp.ed_g]
    lifted = xe >= 0
    key = (xe[lifted] * 5 + inp.hap["ref"][lifted]) * 4 + inp.hap["alt"][lifted]
    _, merged = np.unique(key, return_counts=True)                                           # haplotype lines (distinct staged indices) per reference site
    hap_ta_max = np.zeros(int(key.max()) + 1, np.int64)
    np.maximum.at(hap_ta_max, key, inp.hap["ta"][lifted])
    site_key = ((np.concatenate([[0], np.cumsum(inp.ref_lens)])[arr["ref_rec"]] + arr["pos"]) * 5 + arr["ref"]) * 4 + arr["alt"]
    _, alts = np.unique(site_key // 4, return_counts=True)                                   # lines per (X, REF)
    _, refs_per_pos = np.unique(np.unique(site_key // 4) // 5, return_counts=True)           # distinct REF per X
    reach = dict(amplicons=len(pcs), pieces3=int((n_pieces >= 3).sum()), overlap=overlap, merged=int((merged >= 2).sum()), ta_above_every_haplotype_line=int((arr["ta"] > hap_ta_max[site_key]).sum()),
                 two_ref_at_a_pos=int((refs_per_pos >= 2).sum()), three_alt=int((alts >= 3).sum()), unlifted_entries=unl[0], wholly_inserted=int((n_pieces == 0).sum()))
    print("reach", reach)
    assert min(reach.values()) >= 1, reach
    assert reach["pieces3"] > reach["amplicons"] // 2, reach                                   # most amplicons are cut into three pieces or more


def test_invariance_over_slabs_chunks_lds_and_bgzf(dense_job):
    """4: 1, 3 and 1200 slabs (the last: more than the counting pass sums in LDS, and an amplicon over a copy junction has pieces
    80 slabs apart), chunks of 257 amplicons, LDS windows of 16 bytes, pieces of 65521 bytes, BGZF: the bytes of the default call."""
    out, res, _, _ = dense_job
    inp = Inputs(out)
    want = open(out + ".vcf").read()
    assert (sum(inp.ref_lens) + 19999) // 20000 == 3 and (sum(inp.ref_lens) + 49) // 50 == 1200
    far = 0                                                                                   # amplicons with two pieces in slabs of 50 that are not neighbours
    for s, l in zip(inp.starts.tolist(), inp.lens.tolist()):
        p = pieces_of(s, l, inp.seg, inp.ref_lens)
        far += any(abs(b[0] // 50 - (a[1] - 1) // 50) >= 2 for a, b in zip(p, p[1:]))
    assert far >= 1
    for v in DENSE_VARIANTS:
        assert open(out + "_" + v["name"] + ".vcf").read() == want and res[v["name"]] == res["plain"], v["name"]
        if v.get("bgzf"):
            assert _inflate(open(out + "_" + v["name"] + ".vcf.gz", "rb").read()).decode() == want


def test_nothing_else_moves(dense_job):
    """5: the haplotype table (file and arrays), the FASTQ of the following yield and the support table of the same ctx are the same
    bytes before and after the calls of this table."""
    out, res, _, _ = dense_job
    for f in ("_hap_%s.vcf", "_%s_1.fq", "_%s_2.fq", "_sup_%s.vcf"):
        a, b = open(out + f % "before", "rb").read(), open(out + f % "after", "rb").read()
        assert a == b and len(a) > 10000, f
    a, b = np.load(out + "_hapsites_before.npz"), np.load(out + "_hapsites_after.npz")
    assert all(a[k].tobytes() == b[k].tobytes() for k in a.files) and res["hap_before"] == res["hap_after"]


def test_two_step_flow_through_the_cli(dense_job, models, tmp_path):
    """5: `scssim simuvars --lift`, then `scssim genreads --lift --artefacts-ref`, plain and .gz, with --artefacts-min-reads: the
    in-process files of a job of the same seed over the loaded FASTA and table."""
    _, _, ref, var = dense_job
    prof, simu, lift = models["Illumina_HiSeq2500"], str(tmp_path / "simu.fa"), str(tmp_path / "simu.lift")
    r = subprocess.run([CLI, "simuvars", "-r", ref, "-v", var, "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, res = _run(tmp_path / "api", prof=prof, fasta=simu, lift=lift, cov=2.0, layout="PE", seed=77)
    for name, extra, want in (("cli.vcf", [], out + ".vcf"), ("cli.vcf.gz", [], out + ".vcf"), ("cli_m1.vcf", ["--artefacts-min-reads", "1"], out + "_m1.vcf")):
        pre = str(tmp_path / name)
        r = subprocess.run([CLI, "genreads", "-i", simu, "-m", prof, "-c", "2", "-o", pre, "--seed", "77", "--lift", lift, "--artefacts-ref", pre] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = open(pre, "rb").read()
        assert (_inflate(got) if name.endswith(".gz") else got) == open(want, "rb").read() and len(got) > 1000, name


def test_plain_genome(models, tmp_path):
    """3: no variant files, two identical haplotypes: every line's NA / NR is the sum of the haplotype table's lines at that
    coordinate, TA / TR the sum of the two haplotypes' coverage; nothing is unlifted."""
    ref = make_genome(str(tmp_path / "ref.fa"), "60000,40500", 17, ref=True)
    out, res = _run(tmp_path / "job", prof=models["Illumina_HiSeq2500"], ref=ref, cov=3.0, layout="PE", seed=3)
    inp, arr, unl, extra = check_job(out, res, "plain")
    assert unl == (0, 0) and len(inp.seg) == 4 and inp.ref_lens == [60000, 40500]
    z = np.load(out + "_sites0.npz")
    ref_off = np.array([0, 60000])
    n = len(inp.G)
    cov_a, cov_r = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    for lo, hi, rd in zip(inp.starts, inp.starts + inp.lens, inp.reads):
        cov_a[lo:hi] += 1
        cov_r[lo:hi] += rd
    hap = {}
    for rec, pos, alt, na, nr in zip(*(inp.hap[k].tolist() for k in ("rec", "pos", "alt", "na", "nr"))):
        h = hap.setdefault((rec // 2, pos, alt), [0, 0])
        h[0] += na
        h[1] += nr
    assert len(hap) == len(z["na"]) > 100
    for rr, pos, alt, na, ta, nr, tr in zip(*(z[k].tolist() for k in ("ref_rec", "pos", "alt", "na", "ta", "nr", "tr"))):
        g0, g1 = int(inp.hap_off[2 * rr]) + pos, int(inp.hap_off[2 * rr + 1]) + pos
        assert [na, nr] == hap[(rr, pos, alt)] and ta == cov_a[g0] + cov_a[g1] and tr == cov_r[g0] + cov_r[g1]


_OWN = r'''
import ctypes
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO
from gpu_child import fails, job_args
a = job_args()
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
fails(lambda: s.write_artefacts_ref(a["tmp"] + "/s.vcf"), SCS_EINVAL, "scs_write_artefacts_ref", "sharded")
fails(s.artefact_ref_sites, SCS_EINVAL, "scs_artefact_ref_sites", "sharded")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
live = scssim_amd.live_resources()
fails(lambda: g.write_artefacts_ref(a["tmp"] + "/a.vcf"), SCS_EINVAL, "no lift table", "scs_simuvars", "scs_load_lift")
fails(g.artefact_ref_sites, SCS_EINVAL, "no lift table")
assert scssim_amd.live_resources() == live
g.simuvars(a["ref"], None, None)                              # a genome with its table, nothing allocated yet
fails(lambda: g.write_artefacts_ref(a["tmp"] + "/a.vcf"), SCS_EINVAL, "scs_allocate_reads")
fails(g.artefact_ref_sites, SCS_EINVAL, "scs_allocate_reads")
g.create_frags(); g.amplify(); g.allocate_reads(0)
live = scssim_amd.live_resources()
fails(lambda: g.write_artefacts_ref(a["tmp"] + "/no/such/dir/a.vcf"), SCS_EIO, "scs_write_artefacts_ref", "can not open")
fails(lambda: g.write_artefacts_ref(""), SCS_EINVAL, "no path")
assert scssim_amd.live_resources() == live                   # a failed call leaves nothing
r = g.write_artefacts_ref(a["tmp"] + "/a.vcf")
assert r["sites"] > 0 and scssim_amd.live_resources() == live
assert g._L.scs_write_artefacts_ref(g._ctx, (a["tmp"] + "/b.vcf").encode(), 2, 0, None, None, None) == SCS_EINVAL      # an unknown flag
assert g._L.scs_write_artefacts_ref(g._ctx, (a["tmp"] + "/b.vcf").encode(), 0, 0, None, None, None) == 0              # every output pointer may be NULL
assert open(a["tmp"] + "/b.vcf").read() == open(a["tmp"] + "/a.vcf").read()
n = ctypes.c_uint64()
g._L.scs_artefact_ref_sites.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
assert g._L.scs_artefact_ref_sites(g._ctx, 0, *([None] * 8), 0, ctypes.byref(n), None) == scssim_amd.SCS_EOVERFLOW and n.value == r["sites"]
assert scssim_amd.live_resources() == live
g.yield_reads(collect=False)                                 # the ctx stays usable
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(sv_ref, models, golden_inputs, tmp_path):
    """6: a sharded ctx, a genome without a lift table, a call before allocate_reads and an unwritable path are refused by code and
    words; the live resources read the same around good and failed calls, and zero after scs_destroy."""
    run_child(_OWN, dict(prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], ref=sv_ref, tmp=str(tmp_path)), timeout=300, ok=True)
