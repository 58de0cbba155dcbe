"""GPU tests of the lift table and the depth track by reference bin (scs_simuvars / scs_load_lift / scs_set_depth_ref, `scssim
simuvars --lift`, `scssim genreads --lift --depth-ref`): the per-bin counters equal what the truth SAM of the
same yield call gives, read by read, through the downloaded segment table; the copies equal the host value; a dense layout where
most reads cross segment boundaries; a plain genome against the haplotype depth track; nothing else moves; the counters do not
depend on sinks, batch cuts or the LDS table's size; positions lifted on the device; the two-step flow through the CLI; refusals
and ownership.  Each job runs in a child process under its own time limit; the checks run here.  Run with `-m gpu`."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child, sv_ref  # noqa: F401 (a fixture)
from gpu_readers import CLI, SV, Segs, _exact_profile, make_genome
from lift_cases import DENSE_COV, copies_from_table, expected_reach, lift_from_sam, ref_layout, write_dense_inputs

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one genome (built by simuvars, or a FASTA and its lift file), one amplified job, then a yield per leg:
# {name, wr (reference bins; 0: off), w (haplotype bins; 0: off), sink (callback / null / files / device), sam, writers, ...}
_CHILD = r'''
import numpy as np
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a, lift_file="ref" in a, segs=True)
res = {}
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    g.set_seed(a["seed"])
    g.set_depth(leg.get("w", 0)); g.set_depth_ref(leg.get("wr", 0))
    g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
    yield_leg(g, pre, leg)
    res[leg["name"]] = dict(reads_written=g.stats()["reads_written"], k_depth_lift=g.depth_ref_kernel_time(), k_reads=g.kernel_times()["k_reads"], k_depth=g.kernel_times()["k_depth"])
    arrays = {}
    if leg.get("wr"):
        arrays["reads"], arrays["bases"], arrays["copies"], arrays["off"] = g.depth_ref()
        if leg.get("write"):
            g.write_depth_ref(pre + ".tsv")
    if leg.get("w"):
        arrays["hreads"], arrays["hbases"], arrays["hoff"] = g.depth()
    np.savez(pre + "_depth.npz", **arrays)
emit(res)
'''


def _run(tmp_path, legs, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"] = legs
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def _arrays(out, name):
    return np.load(out + "_" + name + "_depth.npz")


def check_against_sam(out, res, name, w, seg):
    z = _arrays(out, name)
    reads, bases, copies = z["reads"], z["bases"], z["copies"]
    off, nb = ref_layout(seg.ref_lens, w)
    assert reads.dtype == bases.dtype == copies.dtype == np.uint64 and len(reads) == len(bases) == len(copies) == nb + 1 and (z["off"] == off.astype(np.uint64)).all()
    want_reads, want_bases, n_recs, m_sum, reach = lift_from_sam(out + "_" + name + ".sam", seg, w)
    assert n_recs == res[name]["reads_written"] > 500 and int(reads.sum()) == n_recs and int(bases.sum()) == m_sum
    assert (reads == want_reads).all(), np.nonzero(reads != want_reads)[0][:10]
    assert (bases == want_bases).all(), np.nonzero(bases != want_bases)[0][:10]
    assert (copies == copies_from_table(seg, seg.ref_lens, w)).all()
    assert res[name]["k_depth_lift"]["launches"] >= 1 and res[name]["k_depth_lift"]["units"] > 0
    return reads, bases, reach


def test_counters_equal_the_truth_sam_through_the_table(sv_ref, models, tmp_path):
    """1: the golden simuvars genome (1.5 Mb staged, CN 0 .. 8, three reference records), PE HiSeq2500 at 2x, bins of 1000 and 37:
    reads, bases and the pseudo-bin rebuilt from the SAM's POS and CIGAR through the downloaded table, bin for bin; copies = the
    host value; the device copy of the table = the host probe's."""
    legs = [dict(name="w%d" % w, wr=w, sam=True) for w in (1000, 37)]
    out, res = _run(tmp_path, legs, prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, layout="PE", seed=41)
    seg = Segs(out)
    host, _ = scssim_amd.lift_plan_probe(sv_ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"))
    assert all((getattr(seg, k) == np.asarray(getattr(host, k), np.int64)).all() for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")) and len(seg) == len(host)
    assert open(out + ".lift").read() == open(_write_host_lift(sv_ref, tmp_path)).read()
    for w in (1000, 37):
        reads, bases, reach = check_against_sam(out, res, "w%d" % w, w, seg)
        off, nb = ref_layout(seg.ref_lens, w)
        cn0 = np.arange(-(-149999 // w), 160000 // w)
        assert (reads[cn0] == 0).all() and (bases[cn0] == 0).all() and reads[:nb].sum() > 0   # no read lifts into the CN-0 stretch


def _write_host_lift(ref, tmp_path):
    p = str(tmp_path / "host.lift")
    scssim_amd.lift_plan_probe(ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"), p)
    return p


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    ref, var = write_dense_inputs(d)
    table, _ = scssim_amd.lift_plan_probe(ref, None, var)
    return dict(ref=ref, var=var, table=table, dir=d)


@pytest.mark.parametrize("model,layout,L", [("Illumina_HiSeq2000", "SE", 75), ("Illumina_HiSeq2500", "PE", 125)])
def test_dense_layout(model, layout, L, dense, models, tmp_path):
    """2: boundaries closer than a read is long: insertions, deletions, CN 4 / 1 / 0 in 60 kb, sequenced at 14x with frequent
    sequencing indels (the exact-placement model of test_gpu_truth.py).  The builder's geometry is checked on the CPU first; what
    the reads of the job really reached is computed from the SAM and asserted, so that the test cannot pass beside the branches."""
    t = dense["table"]
    n_reads = DENSE_COV * float(np.asarray(t.ref_lens).sum()) / L                               # genreads takes the coverage of the reference length the record names state
    exp = expected_reach(t, L, n_reads)
    assert exp["cross"] > 0.55 * n_reads and min(exp["cross2"], exp["wholly_inserted"], exp["starts_inserted"], exp["back"]) >= 8, exp   # safe before relying on it
    prof = _exact_profile(models[model], str(tmp_path / "x.profile"), 0.004, 0.004)
    out, res = _run(tmp_path, [dict(name="w%d" % w, wr=w, sam=True) for w in (1000, 37)], prof=prof, ref=dense["ref"], vars=dense["var"], cov=DENSE_COV, layout=layout, seed=19, ber=0.0)
    seg = Segs(out)
    assert len(seg) == len(t) > 600
    for w in (1000, 37):
        reads, bases, reach = check_against_sam(out, res, "w%d" % w, w, seg)
    assert reach["cross"] > 0.5 * reach["n"], reach                                          # most reads cross a segment boundary
    assert reach["cross2"] >= 1 and reach["starts_inserted"] >= 1 and reach["wholly_inserted"] >= 1 and reach["back"] >= 1 and reach["deletion_and_boundary"] >= 1, reach
    nb = ref_layout(seg.ref_lens, 37)[1]
    assert reads[nb] == reach["wholly_inserted"] and (reads[-(-40000 // 37):45000 // 37] == 0).all()


def test_plain_genome_agrees_with_the_haplotype_track(models, tmp_path):
    """3: simuvars without variant files: one R segment per haplotype, so the reference track is the sum of the two haplotypes'
    tracks of k_depth in the same call, nothing is unlifted and every reference base has two copies."""
    ref = make_genome(str(tmp_path / "ref.fa"), "60000,40500", 17, ref=True)
    out, res = _run(tmp_path, [dict(name="both", w=1000, wr=1000)], prof=models["Illumina_HiSeq2500"], ref=ref, cov=3.0, layout="PE", seed=3)
    z, seg = _arrays(out, "both"), Segs(out)
    assert len(seg) == 4 and seg.ref_lens.tolist() == [60000, 40500] and z["hoff"].tolist() == [0, 60, 120, 161, 202] and z["off"].tolist() == [0, 60, 101]
    for name in ("reads", "bases"):
        h = z["h" + name]
        want = np.concatenate([h[0:60] + h[60:120], h[120:161] + h[161:202], [0]])
        assert (z[name] == want).all() and z[name].sum() > 500
    width = np.concatenate([np.full(60, 1000), np.full(40, 1000), [500]])
    assert (z["copies"][:101] == 2 * width).all() and z["copies"][101] == 0
    assert int(z["reads"].sum()) == res["both"]["reads_written"]


INV = dict(cov=24.0, layout="PE", seed=23)                 # the dense genome at 24x of its 60 kb reference: 5760 pairs -- 23 workgroups, two batches of 4096 at SCS_TEST_BATCH_SHIFT=12


@pytest.fixture(scope="module")
def invariance_reference(dense, models, tmp_path_factory):
    """The one PE job of checks 4 and 5 with every sink the default build offers, on one ctx: computed once, shared, never changed."""
    d = tmp_path_factory.mktemp("inv")
    legs = [dict(name="cb", wr=100, sam=True), dict(name="off", w=100, sink="files"), dict(name="on", w=100, wr=100, sink="files"),
            dict(name="parts", wr=100, sink="files", writers=3, generations=2), dict(name="bgzf", wr=100, sink="files", bgzf=True),
            dict(name="null", wr=100, sink="null"), dict(name="dev", wr=100, sink="device"), dict(name="again", wr=100)]
    out, res = _run(d, legs, prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], **INV)
    return out, res


def test_nothing_else_moves_and_sinks_do_not_matter(invariance_reference):
    """4, 5: the FASTQ files and the haplotype depth arrays with the reference track on are those with it off; a callback (checked
    against its SAM), files, 3 writers x 2 generations, BGZF, a NULL sink, the text left in device memory and a second callback
    yield after set_seed give the same counters."""
    out, res = invariance_reference
    reads, bases, _ = check_against_sam(out, res, "cb", 100, Segs(out))
    assert res["cb"]["reads_written"] > 2 * 4096                                              # more than 4096 pairs: two batches at SCS_TEST_BATCH_SHIFT=12
    for name in ("on", "parts", "bgzf", "null", "dev", "again"):
        z = _arrays(out, name)
        assert (z["reads"] == reads).all() and (z["bases"] == bases).all() and (z["copies"] == _arrays(out, "cb")["copies"]).all(), name
        assert res[name]["k_depth_lift"]["launches"] == res[name]["k_reads"]["launches"] >= 1      # one event pair per batch
    assert res["off"]["k_depth_lift"]["launches"] == 0 and res["off"]["k_depth_lift"]["units"] == 0
    off, on = _arrays(out, "off"), _arrays(out, "on")
    for k in ("hreads", "hbases", "hoff"):
        assert off[k].tobytes() == on[k].tobytes() and off[k].sum() > 0
    for m in ("_1.fq", "_2.fq"):
        want = open(out + "_off" + m, "rb").read()
        assert len(want) > 100000 and open(out + "_on" + m, "rb").read() == want == open(out + "_cb" + m, "rb").read()
        k = 0 if m == "_1.fq" else 1
        assert b"".join(open(p, "rb").read() for p in scssim_amd.part_paths(out + "_parts", 6)[k]) == want
        assert gzip.open(out + "_bgzf" + m + ".gz", "rb").read() == want


@pytest.mark.parametrize("knob,value", [("SCS_TEST_BATCH_SHIFT", "12"), ("SCS_TEST_BATCH_SHIFT", "8"), ("SCS_TEST_LIFT_SLOTS", "0"), ("SCS_TEST_LIFT_SLOTS", "4")])
def test_invariance_over_batch_cuts_and_table_sizes(knob, value, invariance_reference, dense, models, tmp_path):
    """5: batches of 4096 pairs and of 256 (a workgroup each), no LDS table at all (every add goes to memory) and a table of 4 slots
    (most adds overflow into direct ones): the arrays of the default build."""
    ref_out, _ = invariance_reference
    want = _arrays(ref_out, "cb")
    out, res = _run(tmp_path, [dict(name="v", wr=100)], env=seams_env(**{knob: value}), prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], **INV)
    z = _arrays(out, "v")
    assert (z["reads"] == want["reads"]).all() and (z["bases"] == want["bases"]).all() and (z["copies"] == want["copies"]).all()
    if knob == "SCS_TEST_BATCH_SHIFT":
        assert res["v"]["k_depth_lift"]["launches"] == res["v"]["k_reads"]["launches"] >= (res["v"]["reads_written"] // 2) >> int(value) >= 1


_POS = r'''
import numpy as np
import scssim_amd
from scssim_amd import SCS_EINVAL
from gpu_child import fails, job_args
a = job_args()
g = scssim_amd.GenReads(seed=5)
g.simuvars(a["ref"], a["snp"], a["vars"])
t = g.lift_segments()
n, nr = g.lift_info()
assert n == len(t) == 92 and nr == 3 and t.ref_lens.tolist() == [400000, 150000, 60000]
hap_lens = np.array(a["hap_lens"], np.int64)
off = np.concatenate([[0], np.cumsum(hap_lens)])
rng = np.random.default_rng(1)
x = np.concatenate([rng.integers(0, off[-1], 100000), t.hap_off.astype(np.int64), (t.hap_off + t.len - 1).astype(np.int64)])
rec = np.searchsorted(off, x, side="right") - 1
rr, rp, k = g.lift_positions(rec, x - off[rec])
si = np.searchsorted(t.hap_off.astype(np.int64), x, side="right") - 1
assert (k == t.kind[si]).all() and (rr == t.ref_rec[si]).all() and (k == 1).sum() > 10
want = np.where(t.kind[si] == 0, t.ref_pos[si].astype(np.int64) + x - t.hap_off[si].astype(np.int64), t.ref_pos[si].astype(np.int64))
assert (rp.astype(np.int64) == want).all()
for bad_rec, bad_pos in ((0, hap_lens[0]), (5, hap_lens[5]), (6, 0)):
    fails(lambda: g.lift_positions([0, bad_rec], [5, bad_pos]), SCS_EINVAL, "outside")      # a position past its record
assert g.lift_positions([], [])[0].size == 0
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_lift_positions(sv_ref, tmp_path):
    """6: 10^5 random staged positions and every segment's first and last base through k_lift_points against numpy.searchsorted on
    the downloaded table; a position past its record is refused."""
    host, _ = scssim_amd.lift_plan_probe(sv_ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"))
    run_child(_POS, dict(ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), hap_lens=host.hap_lens.tolist()), timeout=300, ok=True)


def test_two_step_flow_through_the_cli(sv_ref, models, golden_inputs, tmp_path):
    """7: `scssim simuvars --lift`, then `scssim genreads -i simu.fa --lift --depth-ref`: the depth file is the in-process route's for
    the same seed, byte for byte; the lift file is the host probe's and loads to the table simuvars kept; a lift file of another
    genome is refused with the record named."""
    prof, simu, lift, pre = models["Illumina_HiSeq2500"], str(tmp_path / "simu.fa"), str(tmp_path / "simu.lift"), str(tmp_path / "cli")
    r = subprocess.run([CLI, "simuvars", "-r", sv_ref, "-s", os.path.join(SV, "snp.txt"), "-v", os.path.join(SV, "vars.txt"), "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(simu, "rb").read() == gzip.open(os.path.join(SV, "expected_full.fa.gz")).read()   # the FASTA stays the reference binary's
    assert open(lift).read() == open(_write_host_lift(sv_ref, tmp_path)).read()
    r = subprocess.run([CLI, "genreads", "-i", simu, "-m", prof, "-c", "2", "-o", pre, "--seed", "77", "--lift", lift, "--depth-ref", pre + ".tsv", "--depth-bin", "1000"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, res = _run(tmp_path, [dict(name="api", wr=1000, sink="null", write=True)], prof=prof, ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, layout="PE", seed=77)
    text = open(pre + ".tsv").read()
    assert text == open(out + "_api.tsv").read()
    lines = text.split("\n")
    z = _arrays(out, "api")
    assert lines[0] == "#record\tstart\tend\treads\tbases\tcopies" and lines[1].split("\t")[:3] == ["20", "0", "1000"] and lines[-1] == "" and len(lines) == 1 + 610 + 1 + 1
    assert lines[-2] == "#unlifted\t%d\t%d\t%d" % (z["reads"][-1], z["bases"][-1], z["copies"][-1])
    assert [int(ln.split("\t")[3]) for ln in lines[1:-2]] == z["reads"][:-1].tolist() and [int(ln.split("\t")[5]) for ln in lines[1:-2]] == z["copies"][:-1].tolist()
    # the loaded table is the kept one
    out2, _ = _run(tmp_path, [], out=str(tmp_path / "loaded"), prof=prof, fasta=simu, lift=lift, cov=2.0, layout="PE", seed=77)
    a, b = Segs(out), Segs(out2)
    assert all((getattr(a, k) == getattr(b, k)).all() for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind", "ref_lens")) and len(a) == len(b) == 92
    # another genome
    r = subprocess.run([CLI, "genreads", "-i", golden_inputs["g1_hiseq2500_pe"], "-m", prof, "-o", pre + "_x", "--lift", lift, "--depth-ref", pre + "_x.tsv"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "belongs to another genome" in r.stderr and "20_1_400000" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(pre + "_x.tsv") and not os.path.exists(pre + "_x_1.fq")


_OWN = r'''
import ctypes
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_depth_ref(1000)
fails(s.yield_reads, SCS_EINVAL, "scs_set_depth_ref", "sharded")
s.set_depth_ref(0)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")       # the refusal is gone: what is missing now is the job itself
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
fails(g.lift_info, SCS_EINVAL, "scs_simuvars", "scs_load_lift")
fails(lambda: g.write_lift(a["tmp"] + "/none.lift"), SCS_EINVAL, "no lift table")
fails(lambda: g.load_lift(a["tmp"] + "/missing.lift"), SCS_EIO, "can not open")
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_depth_ref(1000)
fails(lambda: g.yield_reads(collect=False), SCS_EINVAL, "scs_load_lift", "scs_simuvars")   # a staged genome without a table
g.set_depth_ref(0)
g.yield_reads(collect=False)
# a genome with its table
g.simuvars(a["ref"], None, None)
live = scssim_amd.live_resources()
fails(g.depth_ref_bins, SCS_EINVAL, "off")
g.set_depth_ref(1)
n, w = g.depth_ref_bins()
assert (n, w) == (610000, 1)
g.set_depth_ref(1000)
fails(g.depth_ref, SCS_EINVAL, "scs_download_depth_ref")     # before any yield
g.run(collect=False)
r, b, c, off = g.depth_ref()
assert int(r.sum()) == g.stats()["reads_written"] > 0 and len(r) == 611 and r[610] == 0 and int(c.sum()) == 2 * 610000
assert g.depth_ref_kernel_time()["launches"] >= 1
buf = (ctypes.c_uint64 * 611)()
g._L.scs_download_depth_ref.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
assert g._L.scs_download_depth_ref(g._ctx, buf, None, None, 610) == SCS_EOVERFLOW
assert g._L.scs_download_depth_ref(g._ctx, None, buf, None, 611) == 0 and list(buf) == b.tolist()
g.set_depth_ref(0)
g.set_seed(5); g.yield_reads(collect=False)
assert g.depth_ref_kernel_time()["launches"] == 0
fails(g.depth_ref, SCS_EINVAL, "off")
# staging another genome drops the table
g.load_genome(a["fa"])
fails(g.lift_info, SCS_EINVAL, "no lift table")
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
# more than 2^27 bins: refused by the layout before any GPU work, with the smallest admissible width
h = scssim_amd.GenReads(profile=a["prof"], seed=5)
h.load_genome(a["fa"]); h.load_lift(a["big"])
h.set_depth_ref(1)
fails(h.depth_ref_bins, SCS_EINVAL, "2^27", "smallest bin width it admits is 8")
h.create_frags(); h.amplify(); h.allocate_reads(0)
fails(lambda: h.yield_reads(collect=False), SCS_EINVAL, "2^27", "smallest bin width it admits is 8")
h.set_depth_ref(8)
assert h.depth_ref_bins() == (1 << 27, 8)
h.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''

_OWN_LIVE = r'''
import scssim_amd
from gpu_child import job_args
a = job_args()
g = scssim_amd.GenReads(profile=a["prof"], coverage=2.0, seed=5)
g.simuvars(a["ref"], None, None)
g.run(collect=False)
before = scssim_amd.live_resources()
g.set_depth_ref(1000); g.set_seed(5); g.yield_reads(collect=False)
during = scssim_amd.live_resources()
g.set_depth_ref(0)
after = scssim_amd.live_resources()
assert during[0] > before[0] and after == before, (before, during, after)
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0)
print("ok")
'''


def test_refusals_and_ownership(sv_ref, models, golden_inputs, tmp_path):
    """8: a sharded ctx and a genome without a table are refused at the yield call by name; no download before a yield, none into too
    small a buffer; more than 2^27 bins name the smallest admissible width; staging a new genome drops the table; the live resources
    read the same before the feature goes on and after it goes off, and zero after scs_destroy."""
    fa = golden_inputs["g1_hiseq2500_pe"]
    names, _, _ = scssim_amd.fasta_probe(fa)
    scssim_amd.fasta_write_index(fa)
    lens = [int(ln.split("\t")[1]) for ln in open(fa + ".fai").read().split("\n") if ln]
    big = str(tmp_path / "big.lift")                       # the staged records as copies of a reference record of 2^30 bases
    with open(big, "w") as f:
        f.write("##scssim-lift v1\n#ref\tbig\t%d\n" % (1 << 30) + "".join("#hap\t%s\t%d\n" % (n, ln) for n, ln in zip(names, lens)))
        f.write("".join("%s\t0\t%d\tbig\t%d\t%d\tR\n" % (n, ln, (1 << 30) - ln, 1 << 30) for n, ln in zip(names, lens)))
    own = dict(prof=models["Illumina_HiSeq2500"], fa=fa, ref=sv_ref, tmp=str(tmp_path), big=big)
    run_child(_OWN, own, timeout=300, ok=True)
    run_child(_OWN_LIVE, own, timeout=300, ok=True)
