"""GPU tests of the truth BAM (scs_set_truth_bam / scssim genreads --truth-bam).  The reference of every comparison is the
project's own truth SAM of the same job (tests/test_gpu_truth.py pins that one to the genome and the lineage): a child process
runs the job twice on one ctx with the same seed, once with set_truth_sam and once with set_truth_bam, and the checks here decode
the BAM with tests/bam_cases.py and compare it with the SAM record for record, column for column.  Run with `-m gpu`."""
import os

import pytest

from conftest import seams_env
from bam_cases import read_bam, reg2bin
from gpu_child import run_child
from gpu_readers import CUT_JOB, CUT_LDS, _exact_profile, cut_job_inputs, make_genome, pair_floor

import scssim_amd

pytestmark = pytest.mark.gpu

_CHILD = r'''
import scssim_amd
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a)
out = a["out"]
res = {}
for kind in ("sam", "bam"):
    g.set_truth_sam(out + ".sam" if kind == "sam" else None)
    g.set_truth_bam(out + ".bam" if kind == "bam" else None)
    yield_leg(g, out + "_" + kind, dict(sink=a["sink"], bgzf=True))
    res[kind] = dict(truth_bytes=g.truth_bytes(), pairs=g.stats()["pairs_written"], k_truth=g.kernel_times()["k_truth"])
g.close()
res["live"] = list(scssim_amd.live_resources())
emit(res)
'''


def _run(tmp_path, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def check_bam_equals_sam(bam_path, sam_path, paired, truth_bytes=None):
    """The decoded BAM against the SAM: header text, reference table, every record's 13 columns in order; the fields BAM adds
    (bin, l_read_name, block_size, next_refID) against their definitions.  read_bam asserts the BGZF framing.  Returns the records."""
    bam = read_bam(bam_path)
    lines = open(sam_path).read().split("\n")[:-1]
    hdr = [ln for ln in lines if ln.startswith("@")]
    sam = [ln.split("\t") for ln in lines[len(hdr):]]
    assert bam["text"] == "".join(h + "\n" for h in hdr)
    assert ["@SQ\tSN:%s\tLN:%d" % r for r in bam["refs"]] == hdr[1:-1]
    recs = bam["records"]
    assert len(recs) == len(sam)
    names = {r[0]: i for i, r in enumerate(bam["refs"])}
    for i, (b, s) in enumerate(zip(recs, sam)):
        assert b["cols"] == s, (i, b["cols"], s)
        assert b["refID"] == names[s[2]] and b["block_size"] == b["length"] - 4 and b["l_read_name"] == len(s[0]) + 1 and b["mapq"] == 255
        assert b["bin"] == reg2bin(b["pos"], b["pos"] + b["span"])
        assert (b["next_refID"], b["next_pos"]) == ((b["refID"], int(s[7]) - 1) if paired else (-1, -1))
        assert [(t, ty) for t, ty, _ in b["tags"]] == [("NM", "i"), ("MD", "Z")]
    if truth_bytes is not None:
        assert truth_bytes == bam["size"] == os.path.getsize(bam_path)
    return bam


def _same_fastq(out, sink, paired=True):
    for m in (("_1", "_2") if paired else ("_1",)):
        ext = ".fq.gz" if sink == "files" else ".fq"
        a, b = open(out + "_sam" + m + ext, "rb").read(), open(out + "_bam" + m + ext, "rb").read()
        assert a == b and len(a) > 0


def _check_job(out, res, paired, sink="callback", min_records=1000):
    bam = check_bam_equals_sam(out + ".bam", out + ".sam", paired, res["bam"]["truth_bytes"])
    _same_fastq(out, sink, paired)
    assert res["sam"]["truth_bytes"] == os.path.getsize(out + ".sam")
    assert len(bam["records"]) == res["bam"]["pairs"] * (2 if paired else 1) >= min_records
    return bam


@pytest.mark.parametrize("case,model,layout,cov", [("g1_hiseq2500_pe", "Illumina_HiSeq2500", "PE", 3.0), ("g3_hiseq2000_se", "Illumina_HiSeq2000", "SE", 2.0)])
def test_golden_bam_equals_sam(case, model, layout, cov, models, golden_inputs, tmp_path):
    """1 + 6: the golden PE and SE inputs through the callback sink; after the ctx is destroyed nothing is left alive."""
    out, res = _run(tmp_path, prof=models[model], fa=golden_inputs[case], cov=cov, layout=layout, seed=41, sink="callback")
    bam = _check_job(out, res, layout == "PE")
    if layout == "SE":
        assert all(r["next_refID"] == -1 and r["next_pos"] == -1 and r["tlen"] == 0 for r in bam["records"])
    assert res["live"] == [0, 0, 0, 0]


def _genome(tmp_path, lengths, seed, n_block=None):
    return make_genome(str(tmp_path / "g.fa"), lengths, seed, n_block)


@pytest.mark.parametrize("variant", ["plain", "replay", "cut_runs"])
def test_frequent_indels(variant, models, tmp_path):
    """2: insertion and deletion rates of 0.01: multi-op CIGARs, reversed for half the reads.  replay: the events come from the
    replay path of truth_load (SCS_EV_REPLAY).  cut_runs: the emit pass fills 4 KB of LDS at a time (SCS_TEST_TRUTH_LDS), so every
    workgroup copies its pairs out in about ten runs instead of one."""
    fa = _genome(tmp_path, "200000,150000", 17)
    prof = _exact_profile(models["Illumina_HiSeq2500"], str(tmp_path / "x.profile"), 0.01, 0.01)
    env = {"plain": None, "replay": seams_env(SCS_EV_REPLAY="1"), "cut_runs": seams_env(SCS_TEST_TRUTH_LDS="4096")}[variant]
    out, res = _run(tmp_path, env=env, prof=prof, fa=fa, cov=4.0, layout="PE", seed=7, sink="callback", ber=0.0)
    bam = _check_job(out, res, True)
    multi = sum(r["n_cigar_op"] > 1 for r in bam["records"])
    assert multi > 0.2 * len(bam["records"]), (multi, len(bam["records"]))


@pytest.mark.parametrize("sink", ["files", "callback"])
def test_many_small_batches_and_an_n_block(sink, models, tmp_path):
    """3: batches of 1024 pairs (about nine BGZF blocks each): records straddle blocks and batches.  files: BGZF FASTQ, the BAM
    blocks' total rides the FASTQ blocks' event and the batch ships one iteration late; callback: plain FASTQ, its own event."""
    fa = _genome(tmp_path, "700000,500000", 31, n_block=20000)
    out, res = _run(tmp_path, env=seams_env(SCS_TEST_BATCH_SHIFT="10"), prof=models["Illumina_HiSeqXTen"], fa=fa, cov=1.0, layout="PE", seed=8, sink=sink)
    bam = _check_job(out, res, True, sink)
    assert res["bam"]["k_truth"]["launches"] > 2          # two event pairs per batch: more than one batch
    assert bam["members"] > res["bam"]["k_truth"]["launches"] // 2 + 2


def test_a_batch_smaller_than_one_block(models, tmp_path):
    """4: batches of 64 pairs, about 37 KB of records: one BGZF block per batch, and the last batch's short tail."""
    fa = _genome(tmp_path, "700000,500000", 31, n_block=20000)
    out, res = _run(tmp_path, env=seams_env(SCS_TEST_BATCH_SHIFT="6"), prof=models["Illumina_HiSeqXTen"], fa=fa, cov=0.02, layout="PE", seed=8, sink="callback")
    bam = _check_job(out, res, True, min_records=100)
    batches = res["bam"]["k_truth"]["launches"] // 2
    assert batches > 1 and bam["members"] == 1 + batches + 1     # header, one block per batch, end of file


# the job with the truth BAM or the truth SAM on the reference set: the yield must fail with SCS_EOVERFLOW and name the truth output
_REFUSED = r'''
import scssim_amd
from scssim_amd import ScsError, SCS_EOVERFLOW
from gpu_child import emit, job_args, open_job
a = job_args()
out = a["out"]
g = open_job(a, segs=a["kind"] == "ref", allocate=False)
if a["kind"] == "bam":
    g.set_truth_bam(out + ".bam")
else:
    g.set_truth_ref_sam(out + ".sam")
g.create_frags(); g.amplify(); g.allocate_reads(0)
res = dict(reads_requested=g.stats()["reads_requested"])
try:
    g.yield_reads(); raise SystemExit("a pair larger than the emit pass' LDS: no error")
except ScsError as e:
    res["code"], res["message"], res["overflow"] = e.code, str(e), SCS_EOVERFLOW
g.close()
res["live"] = list(scssim_amd.live_resources())
emit(res)
'''


@pytest.mark.parametrize("kind", ["bam", "ref"])
def test_a_pair_larger_than_the_lds_is_refused(kind, models, tmp_path):
    """The emit passes of the truth BAM and of the truth SAM on the reference refuse a pair that alone outgrows their LDS: with
    SCS_TEST_TRUTH_LDS=256 the yield fails with SCS_EOVERFLOW, the message names the truth output, and the ctx closes with nothing
    left alive.  bam: the 280-pair job of test_gpu_truth.py::test_sam_under_a_cut_lds.  ref: the variant-free simuvars genome of
    test_gpu_truth_ref.py::test_plain_genome (100.5 kb reference) at 0.7x, 281 pairs.  256 is below any pair (pair_floor, on the
    CPU, asserted here): the smallest pair of BAM records is 264 bytes, of records on the reference 324."""
    if kind == "bam":
        fa, prof = cut_job_inputs(tmp_path, models)
        a = dict(CUT_JOB, kind=kind, fa=fa, prof=prof)
    else:
        ref = make_genome(str(tmp_path / "ref.fa"), "60000,40500", 17, ref=True)
        prof = _exact_profile(models["Illumina_HiSeq2500"], str(tmp_path / "x.profile"), 0.01, 0.01)
        a = dict(CUT_JOB, kind=kind, ref=ref, prof=prof, cov=0.7)
    a["out"] = str(tmp_path / "job")
    res = run_child(_REFUSED, a, env=seams_env(SCS_TEST_TRUTH_LDS=str(CUT_LDS)), timeout=300)
    print(res)
    assert 200 <= res["reads_requested"] // 2 <= 400
    assert res["code"] == res["overflow"] and "truth SAM / BAM" in res["message"], res
    assert res["live"] == [0, 0, 0, 0]
    if kind == "bam":
        floor = pair_floor(scssim_amd.truth_bam_record_probe, "20_1_200000", genome="A" * 60)
    else:
        import numpy as np
        from types import SimpleNamespace
        t = np.load(a["out"] + "_segs.npz")
        hap_lens = [60000, 60000, 40500, 40500]
        assert t["len"].tolist() == hap_lens and t["ref_lens"].tolist() == [60000, 40500]      # one R segment per staged record
        floor = pair_floor(scssim_amd.truth_ref_record_probe, "20_1_60000", table=SimpleNamespace(**{k: t[k] for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")}), hap_lens=hap_lens, ref_lens=t["ref_lens"], ref_names=["chr20", "chr21"])
    print("smallest pair: %d bytes" % floor)
    assert floor > CUT_LDS


_ERR = r'''
import scssim_amd
from scssim_amd import SCS_EINVAL
from gpu_child import device_buffers, fails, job_args
a = job_args()
out = a["out"]
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_truth_bam(out + "_s.bam")
fails(s.yield_reads, SCS_EINVAL, "sharded", "BAM")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_truth_sam(out + ".sam")
fails(lambda: g.set_truth_bam(out + ".bam"), SCS_EINVAL, "scs_set_truth_sam", "scs_set_truth_bam")       # BAM over SAM
g.set_truth_bam(None)                                    # clears only its own: the SAM stays on
f1, f2 = g.yield_reads()
open(out + "_sam_1.fq", "wb").write(f1); open(out + "_sam_2.fq", "wb").write(f2)
g.set_truth_sam(None)
g.set_truth_bam(out + ".bam")
fails(lambda: g.set_truth_sam(out + "_2.sam"), SCS_EINVAL, "scs_set_truth_sam", "scs_set_truth_bam")     # SAM over BAM
g.set_truth_sam(None)                                    # ... and the BAM stays on
fails(lambda: g.yield_reads_files(out + "_w", 3), SCS_EINVAL, "writers", "BAM")
with device_buffers(1 << 24) as (d1, d2):
    fails(lambda: g.yield_reads_device(d1, 1 << 24, d2, 1 << 24), SCS_EINVAL, "scs_yield_reads_device", "BAM")
f1, f2 = g.yield_reads()
open(out + "_bam_1.fq", "wb").write(f1); open(out + "_bam_2.fq", "wb").write(f2)
print("ok", g.truth_bytes())
'''


def test_refusals_leave_the_ctx_usable(models, golden_inputs, tmp_path):
    """5: a sharded ctx, writers = 3 and scs_yield_reads_device with the BAM set fail with SCS_EINVAL and say BAM; one truth output
    per ctx, either way round; the same ctx then writes a BAM that equals its SAM."""
    out = str(tmp_path / "e")
    so = run_child(_ERR, dict(prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], out=out), timeout=300, ok=True)
    assert not os.path.exists(out + "_w_1.fq") and not os.path.exists(out + "_2.sam") and not os.path.exists(out + "_s.bam")
    check_bam_equals_sam(out + ".bam", out + ".sam", True, int(so.split()[-1]))
    _same_fastq(out, "callback")

