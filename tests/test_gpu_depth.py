"""GPU tests of the depth track (scs_set_depth / scssim genreads --depth): the per-bin counters equal what the truth SAM of the same
job gives, read by read; they do not depend on batch cuts, the sink, its writers, the LDS table's size or whether the text leaves
the GPU; the FASTQ does not change; the file, the CLI, the refusals and the ownership of the buffers.  Each job runs in a child
process under its own time limit; the checks run here.  Run with `-m gpu`."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child
from gpu_readers import CIG, CLI, _exact_profile, _sam, make_genome

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one amplified job, then a yield per leg: {name, w (0: depth off), sink (callback / null / files / device), sam, writers, ...}
_CHILD = r'''
import numpy as np
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a)
res = {}
for leg in a["legs"]:
    pre = a["out"] + "_" + leg["name"]
    g.set_seed(a["seed"])
    g.set_depth(leg.get("w", 0))
    g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
    yield_leg(g, pre, leg)
    res[leg["name"]] = dict(reads_written=g.stats()["reads_written"], k_depth=g.kernel_times()["k_depth"], k_reads=g.kernel_times()["k_reads"])
    if leg.get("w"):
        r, b, off = g.depth()
        np.savez(pre + "_depth.npz", reads=r, bases=b, off=off)
        if leg.get("write"):
            g.write_depth(pre + ".tsv")
emit(res)
'''


def _run(tmp_path, legs, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"] = legs
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def _arrays(out, name):
    z = np.load(out + "_" + name + "_depth.npz")
    assert z["reads"].dtype == np.uint64 and z["bases"].dtype == np.uint64
    return z["reads"], z["bases"], z["off"]


def depth_from_sam(path, w):
    """(reads, bases, bin_off, records, sum of the M lengths) from the SAM's @SQ lines, POS and CIGAR, in numpy."""
    hdr, recs = _sam(path)
    sq = [(h.split("\t")[1][3:], int(h.split("\t")[2][3:])) for h in hdr if h.startswith("@SQ")]
    off = np.concatenate([[0], np.cumsum([-(-ln // w) for _, ln in sq])]).astype(np.int64)
    first = {name: off[i] for i, (name, _) in enumerate(sq)}
    pos = np.array([int(r[3]) - 1 for r in recs], np.int64)
    b0 = np.array([first[r[2]] for r in recs], np.int64)
    reads = np.bincount(b0 + pos // w, minlength=off[-1]).astype(np.uint64)
    m_start, m_len, m_b0 = [], [], []
    for i, r in enumerate(recs):
        g = pos[i]
        for n, k in CIG.findall(r[5]):
            n = int(n)
            if k == "M":
                m_start.append(g); m_len.append(n); m_b0.append(b0[i])
            if k != "I":
                g += n
    m_start, m_len, m_b0 = np.array(m_start, np.int64), np.array(m_len, np.int64), np.array(m_b0, np.int64)
    within = np.arange(m_len.sum()) - np.repeat(np.cumsum(m_len) - m_len, m_len)          # 0 .. len - 1 inside every M run
    bases = np.bincount(np.repeat(m_b0, m_len) + (np.repeat(m_start, m_len) + within) // w, minlength=off[-1]).astype(np.uint64)
    return reads, bases, off.astype(np.uint64), len(recs), int(m_len.sum())


def check_against_sam(out, res, name, w):
    reads, bases, off = _arrays(out, name)
    want_reads, want_bases, want_off, n_recs, m_sum = depth_from_sam(out + "_" + name + ".sam", w)
    assert (off == want_off).all() and len(reads) == len(bases) == int(off[-1])
    assert n_recs == res[name]["reads_written"] > 500 and int(reads.sum()) == n_recs and int(bases.sum()) == m_sum
    assert (reads == want_reads).all(), np.nonzero(reads != want_reads)[0][:10]
    assert (bases == want_bases).all(), np.nonzero(bases != want_bases)[0][:10]
    return reads, bases


@pytest.mark.parametrize("case,model,layout,cov,isize,widths", [
    ("g1_hiseq2500_pe", "Illumina_HiSeq2500", "PE", 3.0, 260, (1000, 37)),
    ("g3_hiseq2000_se", "Illumina_HiSeq2000", "SE", 2.0, 260, (1000, 37)),
    ("g2_xten_pe_nblock", "Illumina_HiSeqXTen", "PE", 3.0, 300, (500,))])
def test_counters_equal_the_truth_sam_of_the_same_job(case, model, layout, cov, isize, widths, models, golden_inputs, tmp_path):
    """1: truth SAM and depth on in the same yield call; both arrays rebuilt from the SAM's POS and CIGAR are equal to the GPU's, bin
    for bin.  g2: several records and an N block -- the records' edges and their bin offsets."""
    legs = [dict(name="w%d" % w, w=w, sam=True) for w in widths]
    out, res = _run(tmp_path, legs, prof=models[model], fa=golden_inputs[case], cov=cov, layout=layout, seed=41, isize=isize)
    for w in widths:
        reads, _ = check_against_sam(out, res, "w%d" % w, w)
        assert res["w%d" % w]["k_depth"]["launches"] >= 1 and res["w%d" % w]["k_depth"]["units"] > 0
    if case == "g2_xten_pe_nblock":
        _, _, off = _arrays(out, "w500")
        assert len(off) > 2                                 # more than one record


@pytest.mark.parametrize("variant", ["plain", "replay"])
def test_frequent_indels(variant, models, tmp_path):
    """2: the exact-placement model of test_gpu_truth.py with indel rates at which most reads carry events, at bins of 1 and 64
    bases against the SAM.  replay: every read with events has them drawn again (SCS_EV_REPLAY), the other branch of read_place."""
    fa = make_genome(str(tmp_path / "g.fa"), "60000,40000", 17)
    prof = _exact_profile(models["Illumina_HiSeq2500"], str(tmp_path / "x.profile"), 0.01, 0.01)
    env = seams_env(SCS_EV_REPLAY="1") if variant == "replay" else None
    widths = (1, 64) if variant == "plain" else (64,)
    out, res = _run(tmp_path, [dict(name="w%d" % w, w=w, sam=True) for w in widths], env=env, prof=prof, fa=fa, cov=4.0, layout="PE", seed=7, ber=0.0)
    for w in widths:
        check_against_sam(out, res, "w%d" % w, w)
    _, recs = _sam(out + "_w64.sam")
    assert sum(1 for r in recs if "I" in r[5] or "D" in r[5]) > 0.5 * len(recs)


INV = dict(cov=12.0, layout="PE", seed=23)                 # g1 at 12x: 5760 pairs -- 23 workgroups, two batches of 4096


@pytest.fixture(scope="module")
def invariance_reference(models, golden_inputs, tmp_path_factory):
    """The one PE job of check 3 with every sink the default build offers, on one ctx: computed once, shared, never changed."""
    d = tmp_path_factory.mktemp("inv")
    legs = [dict(name="cb", w=100, sam=True), dict(name="off", w=0, sink="files"), dict(name="on", w=100, sink="files"),
            dict(name="parts", w=100, sink="files", writers=3, generations=2), dict(name="bgzf", w=100, sink="files", bgzf=True),
            dict(name="null", w=100, sink="null"), dict(name="dev", w=100, sink="device"), dict(name="again", w=100)]
    out, res = _run(d, legs, prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], **INV)
    return out, res


def test_invariance_over_sinks_on_one_ctx(invariance_reference):
    """3: default batches through a callback (checked against its SAM), files, 3 writers x 2 generations, BGZF, a NULL sink, the text
    left in device memory, and a second callback yield after set_seed (the counters were zeroed): the same arrays every time; the
    FASTQ files with depth on are the files with depth off."""
    out, res = invariance_reference
    reads, bases = check_against_sam(out, res, "cb", 100)
    for name in ("on", "parts", "bgzf", "null", "dev", "again"):
        r, b, _ = _arrays(out, name)
        assert (r == reads).all() and (b == bases).all(), name
        assert res[name]["k_depth"]["launches"] >= 1
    assert res["off"]["k_depth"]["launches"] == 0 and res["off"]["k_depth"]["units"] == 0
    for m in ("_1.fq", "_2.fq"):
        want = open(out + "_off" + m, "rb").read()
        assert len(want) > 100000 and open(out + "_on" + m, "rb").read() == want == open(out + "_cb" + m, "rb").read()
        k = 0 if m == "_1.fq" else 1
        assert b"".join(open(p, "rb").read() for p in scssim_amd.part_paths(out + "_parts", 6)[k]) == want
        assert gzip.open(out + "_bgzf" + m + ".gz", "rb").read() == want


@pytest.mark.parametrize("knob,value", [("SCS_TEST_BATCH_SHIFT", "12"), ("SCS_TEST_BATCH_SHIFT", "8"), ("SCS_TEST_DEPTH_SLOTS", "0"), ("SCS_TEST_DEPTH_SLOTS", "4")])
def test_invariance_over_batch_cuts_and_table_sizes(knob, value, invariance_reference, models, golden_inputs, tmp_path):
    """3: batches of 4096 pairs (two) and of 256 (a workgroup each), no LDS table at all (every add goes to memory) and a table of
    4 slots (most adds overflow into direct ones): the arrays of the default build."""
    ref_out, _ = invariance_reference
    reads, bases, _ = _arrays(ref_out, "cb")
    out, res = _run(tmp_path, [dict(name="v", w=100)], env=seams_env(**{knob: value}), prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], **INV)
    r, b, _ = _arrays(out, "v")
    assert (r == reads).all() and (b == bases).all()
    if knob == "SCS_TEST_BATCH_SHIFT":
        assert res["v"]["k_depth"]["launches"] == res["v"]["k_reads"]["launches"] >= (res["v"]["reads_written"] // 2) >> int(value) >= 1   # one event pair per batch


def _parse_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "#record\tstart\tend\treads\tbases" and lines[-1] == ""
    return [ln.split("\t") for ln in lines[1:-1]]


def test_depth_file_and_cli(models, golden_inputs, tmp_path):
    """4: write_depth's file parses back to the arrays, the names of scs_fasta_probe and BED coordinates with the short last bin of
    every record (bins of 1100 bases: no record of g2 is a multiple); `scssim genreads --depth f --depth-bin 500 --writers 2` writes the same file for the same seed."""
    fa, prof = golden_inputs["g2_xten_pe_nblock"], models["Illumina_HiSeqXTen"]
    legs = [dict(name="api", w=500, sink="null", write=True), dict(name="short", w=1100, sink="null", write=True)]   # 1100 divides no record: short last bins
    out, res = _run(tmp_path, legs, prof=prof, fa=fa, cov=3.0, layout="PE", seed=77)
    names, _, _ = scssim_amd.fasta_probe(fa)
    lens = [int(ln.split("\t")[1]) for ln in open(fa + ".fai").read().split("\n") if ln]
    for name, w in (("api", 500), ("short", 1100)):
        reads, bases, off = _arrays(out, name)
        rows = _parse_tsv(out + "_" + name + ".tsv")
        assert len(rows) == len(reads) == int(off[-1])
        assert [int(r[3]) for r in rows] == reads.tolist() and [int(r[4]) for r in rows] == bases.tolist()
        want = [(n, s, min(s + w, ln)) for n, ln in zip(names, lens) for s in range(0, ln, w)]
        assert [(r[0], int(r[1]), int(r[2])) for r in rows] == want
        assert int(reads.sum()) == res[name]["reads_written"] > 500
    assert sum(1 for _, s, e in want if e - s < 1100) == len(names) > 1     # every record ends in a short bin at 1100
    pre = str(tmp_path / "cli")
    r = subprocess.run([CLI, "genreads", "-i", fa, "-m", prof, "-c", "3", "-o", pre, "--seed", "77", "--depth", pre + ".tsv", "--depth-bin", "500", "--writers", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(pre + ".tsv").read() == open(out + "_api.tsv").read()
    assert os.path.exists(pre + ".p00_1.fq") and os.path.exists(pre + ".p01_2.fq")
    for extra, msg in ((["--depth", pre + "_x.tsv", "--gpus", "2"], "--depth needs --gpus 1"), (["--depth-bin", "500"], "--depth-bin needs --depth")):
        r = subprocess.run([CLI, "genreads", "-i", fa, "-m", prof, "-o", pre + "_x"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, r.stderr[-1000:]
        assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("cli_x")]


_OWN = r'''
import ctypes
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_depth(1000)
fails(s.depth_bins, SCS_EINVAL, "no genome")
fails(s.yield_reads, SCS_EINVAL, "scs_set_depth")
s.set_depth(0)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")       # the refusal is gone: what is missing now is the job itself
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
fails(g.depth_bins, SCS_EINVAL, "off")
g.set_depth(1000)
n, w = g.depth_bins()
assert w == 1000 and n > 10
fails(g.depth, SCS_EINVAL, "scs_download_depth")            # before any yield
g.run(collect=False)
r, b, off = g.depth()
assert int(r.sum()) == g.stats()["reads_written"] > 0 and len(r) == n
assert g.kernel_times()["k_depth"]["launches"] >= 1
buf = (ctypes.c_uint64 * n)()
g._L.scs_download_depth.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
assert g._L.scs_download_depth(g._ctx, buf, None, n - 1) == SCS_EOVERFLOW
assert g._L.scs_download_depth(g._ctx, None, buf, n) == 0 and list(buf) == b.tolist()
g.set_depth(0)
g.set_seed(5); g.yield_reads(collect=False)
assert g.kernel_times()["k_depth"]["launches"] == 0
fails(g.depth, SCS_EINVAL, "off")
live = scssim_amd.live_resources()
assert live[0] > 0
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(models, golden_inputs, tmp_path):
    """5: a sharded ctx is refused at the yield call by name and is rid of the refusal after set_depth(0); no download before a yield,
    none into too small a buffer; the timer counts launches only with depth on; nothing is left once the contexts are destroyed."""
    run_child(_OWN, dict(prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"]), timeout=300, ok=True)
