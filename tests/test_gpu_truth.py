"""GPU tests of the truth SAM (scs_set_truth_sam / scssim genreads --truth): the FASTQ does not change, the SAM is complete and
well-formed, and every read lies where its lineage says, base for base.  Each job runs in a child process under its own time
limit; the checks run here.  Run with `-m gpu`."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seams_env
from gpu_child import run_child
from gpu_readers import CIG, CUT_JOB, CUT_LDS, _exact_profile, _fasta, _fastq, _oracle, _sam, cut_job_inputs, make_genome, pair_floor

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one amplified job: (lineage) the tables a read's place is checked against, (plain) a yield without the SAM, then the yield with it
_CHILD = r'''
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a)
out = a["out"]
if a.get("lineage"):
    import numpy as np
    f = g.download_frags(); s = g.download_amplicons(0); u = g.download_amplicons(1)
    np.savez(out + "_lineage.npz", fgoff=f["goff"], flen=f["len"], fstrand=f["strand"], spar=s["parent"], sspos=s["spos"], slen=s["len"],
             upar=u["parent"], uspos=u["spos"], ulen=u["len"])
if a.get("plain"):
    yield_leg(g, out + "_plain", {})
g.set_truth_sam(out + ".sam")
yield_leg(g, out, a)
emit(dict(truth_bytes=g.truth_bytes(), pairs=g.stats()["pairs_written"], k_truth=g.kernel_times()["k_truth"]))
'''


def _run(tmp_path, env=None, timeout=900, **a):
    a.setdefault("out", str(tmp_path / "job"))
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _ops(c):
    return [(int(n), k) for n, k in CIG.findall(c)]


def _md_nm(seq, gen, pos0, ops):
    """MD and NM of a genome-forward read against its record (pos0: 0-based)."""
    md, run, nm, g, q = "", 0, 0, pos0, 0
    for n, k in ops:
        if k == "I":
            q += n; nm += n
        elif k == "D":
            md += "%d^%s" % (run, gen[g:g + n].decode()); run = 0; g += n; nm += n
        else:
            for _ in range(n):
                if seq[q] == gen[g]:
                    run += 1
                else:
                    md += "%d%s" % (run, chr(gen[g])); run = 0; nm += 1
                q += 1; g += 1
    return md + "%d" % run, nm


def check_sam(sam, fq_files, fasta, paired, isize=None, exact=False, lineage=None, min_records=1000):
    """Checks 2 (and 4 / 3 when asked): header, one record per FASTQ record in order, SEQ / QUAL, CIGAR, mate fields, NM / MD
    against the FASTA.  exact: SEQ equals the genome under the CIGAR (no substitution anywhere).  Returns the records."""
    hdr, recs = _sam(sam)
    gen = _fasta(fasta)
    assert hdr[0] == "@HD\tVN:1.6\tSO:unsorted" and hdr[-1].startswith("@PG\tID:scssim")
    assert hdr[1:-1] == ["@SQ\tSN:%s\tLN:%d" % (k, len(v)) for k, v in gen.items()]
    fqs = [_fastq(f) for f in fq_files]
    fq = [r for pair in zip(*fqs) for r in pair] if paired else fqs[0]
    assert len(recs) == len(fq) > min_records
    rec_off, o = {}, 0
    for k, v in gen.items():
        rec_off[k] = o; o += len(v)
    f = np.array([int(r[1]) for r in recs])
    rev = (f & 0x10) != 0
    pos = np.array([int(r[3]) for r in recs])
    simple = np.array([r[5] == "%dM" % len(r[9]) for r in recs])
    for i, (r, (name, s, q)) in enumerate(zip(recs, fq)):
        assert r[0] == (name[:-2] if paired else name), (i, r[0], name)
        seq = s.encode().translate(COMP)[::-1].decode() if rev[i] else s
        assert r[9] == seq and r[10] == (q[::-1] if rev[i] else q)
        assert r[4] == "255"
    if paired:
        assert (f[0::2] & 0xC3 == 0x43).all() and (f[1::2] & 0xC3 == 0x83).all()
        assert (rev[0::2] != rev[1::2]).all()
        assert (((f[0::2] & 0x20) != 0) == rev[1::2]).all() and (((f[1::2] & 0x20) != 0) == rev[0::2]).all()
        assert all(a[6] == "=" and b[6] == "=" and int(a[7]) == int(b[3]) and int(b[7]) == int(a[3]) and int(a[8]) == -int(b[8]) != 0
                   and a[2] == b[2] for a, b in zip(recs[0::2], recs[1::2]))
        if isize:
            t = np.array([abs(int(a[8])) for a in recs[0::2]], float)
            assert abs(t.mean() - isize) < 5 * t.std() / math.sqrt(len(t)) + 3, (t.mean(), isize)
    else:
        assert (f & ~0x10 == 0).all() and all(r[6] == "*" and r[7] == "0" and r[8] == "0" for r in recs)
    # spans; NM / MD: vectorised for the single-M reads, one by one for the rest
    span = np.zeros(len(recs), np.int64)
    n_indel = 0
    for i in np.nonzero(~simple)[0]:
        r = recs[i]; ops = _ops(r[5])
        assert sum(n for n, k in ops if k != "D") == len(r[9]) and ops[0][1] != "D" and ops[-1][1] != "D"
        span[i] = sum(n for n, k in ops if k != "I")
        g = gen[r[2]]
        md, nm = _md_nm(r[9].encode(), g, pos[i] - 1, ops)
        assert r[11] == "NM:i:%d" % nm and r[12] == "MD:Z:" + md, (i, r)
        indel = sum(n for n, k in ops if k != "M")
        n_indel += 1
        if exact:
            assert nm == indel and not re.search(r"[ACGTN]", re.sub(r"\^[ACGTN]+", "", md)), r
    rname = np.array([r[2] for r in recs]); rlen = np.array([len(r[9]) for r in recs])
    for name, L in sorted(set(zip(rname[simple], rlen[simple]))):   # (a read with only leading / trailing deletions is one shorter M)
        idx = np.nonzero(simple & (rname == name) & (rlen == L))[0]
        g = np.frombuffer(gen[name], np.uint8)
        seqs = np.frombuffer("".join(recs[i][9] for i in idx).encode(), np.uint8).reshape(len(idx), L)
        win = g[(pos[idx] - 1)[:, None] + np.arange(L)[None, :]]
        mism = seqs != win
        nms = np.array([int(recs[i][11][5:]) for i in idx])
        assert (mism.sum(1) == nms).all()
        if exact:
            assert not mism.any()
        span[idx] = L
        for i in idx[mism.any(1)]:                        # the MD strings of the reads with substitutions
            assert recs[i][12] == "MD:Z:" + _md_nm(recs[i][9].encode(), gen[name], pos[i] - 1, [(L, "M")])[0]
        assert all(recs[i][12] == "MD:Z:%d" % L for i in idx[~mism.any(1)])
    if lineage is not None:
        check_lineage(recs, pos, span, rev, rec_off, lineage, paired)
    return recs, simple, n_indel


def check_lineage(recs, pos, span, rev, rec_off, lz, paired):
    """Check 4: every read inside its full amplicon's genome interval, on the strand the chain fragment -> semi -> full gives
    (index maps of scs_kernels_common.h: frag_view, semi_tmpl_view, shift_view), rebuilt here from the downloaded tables."""
    z = np.load(lz)
    f = z["spar"][z["upar"]]
    st = z["fstrand"][f].astype(np.int64); goff = z["fgoff"][f].astype(np.int64); flen = z["flen"][f].astype(np.int64)
    base = np.where(st > 0, goff + flen - 1, goff); d = np.where(st > 0, -1, 1)
    s, l = z["sspos"][z["upar"]].astype(np.int64), z["slen"][z["upar"]].astype(np.int64)
    base = base + d * (s + l - 1); d = -d                    # the semi's template strand
    base = base + d * z["uspos"].astype(np.int64)            # the full amplicon
    end = base + d * (z["ulen"].astype(np.int64) - 1)
    lo, hi = np.minimum(base, end), np.maximum(base, end)
    amp = np.array([int(r[0].split("#")[0]) for r in recs])
    start = np.array([rec_off[r[2]] for r in recs]) + pos - 1
    assert (start >= lo[amp]).all() and (start + span - 1 <= hi[amp]).all()
    fwd_amp = d[amp] > 0
    if paired:
        assert (rev[0::2] == ~fwd_amp[0::2]).all() and (rev[1::2] == fwd_amp[1::2]).all()
    else:
        assert (rev == ~fwd_amp).all()


@pytest.mark.parametrize("case,model,layout,cov", [("g1_hiseq2500_pe", "Illumina_HiSeq2500", "PE", 3.0), ("g3_hiseq2000_se", "Illumina_HiSeq2000", "SE", 2.0)])
def test_fastq_unchanged_and_sam_complete(case, model, layout, cov, oracle_bin, models, golden_inputs, tmp_path):
    """1 + 2 + 4: with truth on the FASTQ is byte-identical to truth off and to the oracle; the SAM has a record per FASTQ record,
    well-formed, its NM / MD right, every read inside its amplicon on the strand the lineage gives."""
    fa = golden_inputs[case]
    out, so = _run(tmp_path, prof=models[model], fa=fa, cov=cov, layout=layout, seed=41, sink="callback", plain=True, lineage=True)
    orc = str(tmp_path / "orc")
    _oracle(oracle_bin, fa, models[model], orc, ["-c", "%g" % cov, "-l", layout], 41)
    paired = layout == "PE"
    mates = ("_1", "_2") if paired else ("_1",)
    for k, m in enumerate(mates):
        want = open(orc + (m + ".fq" if paired else ".fq"), "rb").read()
        assert open(out + m + ".fq", "rb").read() == want == open(out + "_plain" + m + ".fq", "rb").read()
    check_sam(out + ".sam", [out + m + ".fq" for m in mates], fa, paired, isize=260 if paired else None, lineage=out + "_lineage.npz")
    assert so["truth_bytes"] == os.path.getsize(out + ".sam")


@pytest.mark.parametrize("variant", ["plain", "replay", "rollback51"])
def test_exact_placement(variant, models, tmp_path):
    """3: an N-free genome, no amplification errors, substitution rows that always call the window's base and frequent indels:
    every read is the genome under its CIGAR (inserted bases aside) and NM is its indel bases.  An off-by-one anywhere shows as
    ~75 % mismatches.  replay: every read with events takes the replay path (SCS_EV_REPLAY).  rollback51: 51-base reads with
    many deletions, so that n + delta < 50 rolls reads back to no events at all."""
    fa = make_genome(str(tmp_path / "g.fa"), "400000,300000", 17)
    src = models["Illumina_HiSeq2500"]
    if variant == "rollback51":
        src51 = str(tmp_path / "m51.profile")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), "--read-length", "51", src, src51])
        prof = _exact_profile(src51, str(tmp_path / "x.profile"), 0.002, 0.03)
    else:
        prof = _exact_profile(src, str(tmp_path / "x.profile"), 0.01, 0.01)
    env = seams_env(SCS_EV_REPLAY="1") if variant == "replay" else None
    out, _ = _run(tmp_path, env=env, prof=prof, fa=fa, cov=6.0, layout="PE", seed=7, sink="callback", ber=0.0)
    recs, simple, n_indel = check_sam(out + ".sam", [out + "_1.fq", out + "_2.fq"], fa, True, exact=True)
    assert n_indel > 0.2 * len(recs) if variant != "rollback51" else n_indel > 0.05 * len(recs)
    if variant == "rollback51":
        # reads rolled back to no events: 51M reads beyond the event-free ones (per-base event probability from the model)
        p = scssim_amd.Profile(prof)
        q = p.t_indel / 2.0 ** 32
        n51 = int(simple.sum())
        free = len(recs) * (1 - q) ** 51
        rolled = n51 - free
        assert rolled > 6 * math.sqrt(free) + 50, (n51, free)


@pytest.mark.parametrize("sink", ["files", "callback"])
def test_many_batches_and_ns(sink, models, tmp_path):
    """5: the 12 Mb two-record genome with an N block, many small batches; the file sink with BGZF FASTQ and a callback sink."""
    fa = make_genome(str(tmp_path / "simu.fa"), "7000000,5000000", 31, n_block=20000)
    out, _ = _run(tmp_path, env=seams_env(SCS_TEST_BATCH_SHIFT="12"), prof=models["Illumina_HiSeqXTen"], fa=fa, cov=1.0, layout="PE", seed=8,
                  sink=sink, bgzf=True, lineage=True)
    fqs = [out + m + (".fq.gz" if sink == "files" else ".fq") for m in ("_1", "_2")]
    check_sam(out + ".sam", fqs, fa, True, isize=260, lineage=out + "_lineage.npz")


# ---- the emit pass under a cut LDS (SCS_TEST_TRUTH_LDS): the job, its inputs and pair_floor are in tests/gpu_readers.py

@pytest.fixture(scope="module")
def cut_reference(models, tmp_path_factory):
    """The job with the emit pass as shipped: its SAM checked against the genome, its FASTQ against a yield without the SAM."""
    d = tmp_path_factory.mktemp("cut")
    fa, prof = cut_job_inputs(d, models)
    out, so = _run(d, prof=prof, fa=fa, plain=True, **CUT_JOB)
    pairs = so["pairs"]
    print("pairs: %d" % pairs)
    assert 200 <= pairs <= 400
    for m in ("_1.fq", "_2.fq"):
        assert open(out + m, "rb").read() == open(out + "_plain" + m, "rb").read()
    recs, _, n_indel = check_sam(out + ".sam", [out + "_1.fq", out + "_2.fq"], fa, True, exact=True, min_records=2 * 200 - 1)
    assert len(recs) == 2 * pairs and n_indel > 0.2 * len(recs)
    return dict(fa=fa, prof=prof, sam=open(out + ".sam", "rb").read(), fq=[open(out + m, "rb").read() for m in ("_1.fq", "_2.fq")], names=[r[2] for r in recs])


@pytest.mark.parametrize("knobs", [dict(SCS_TEST_TRUTH_LDS="4096"), dict(SCS_TEST_TRUTH_LDS="1024"), dict(SCS_TEST_TRUTH_LDS=str(CUT_LDS)),
                                   dict(SCS_TEST_TRUTH_LDS="24576", SCS_TEST_BATCH_SHIFT="5"), dict(SCS_TEST_BATCH_SHIFT="5")],
                         ids=["lds4096", "lds1024", "lds256", "lds24576_batch32", "batch32"])
def test_sam_under_a_cut_lds(knobs, cut_reference, tmp_path):
    """The truth SAM does not depend on the LDS its emit pass may fill, nor on how the job is cut into batches: the file and the
    FASTQ are the plain run's, byte for byte (cut_reference checks that one against the genome with check_sam(exact=True)).
    k_truth_emit builds a workgroup's run (64 pairs of this job, about 40 KB) in LDS in one turn, or, where the run outgrows the
    LDS, has every lane write its pair straight to memory; it refuses no pair.  lds4096, lds1024, lds256: every run outgrows the
    LDS, every pair takes the direct write -- 256 is below any single pair: pair_floor gives 306 bytes for this job (asserted
    here).  batch32: batches of 32 pairs, fewer lanes with a pair than the wave has, a short last batch, all in LDS.
    lds24576_batch32: the 32-pair runs (about 20 KB) fit, so both paths meet in one file only where a batch's run is longer; the
    bytes are the same either way."""
    assert pair_floor(scssim_amd.truth_record_probe, min(cut_reference["names"], key=len), genome="A" * 60) > CUT_LDS
    out, _ = _run(tmp_path, env=seams_env(**knobs), prof=cut_reference["prof"], fa=cut_reference["fa"], **CUT_JOB)
    assert open(out + ".sam", "rb").read() == cut_reference["sam"]
    assert [open(out + m, "rb").read() for m in ("_1.fq", "_2.fq")] == cut_reference["fq"]


_ERR = r'''
import scssim_amd
from scssim_amd import SCS_EINVAL
from gpu_child import device_buffers, fails, job_args
a = job_args()
out = a["out"]
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_truth_sam(out + "_s.sam")
fails(s.yield_reads, SCS_EINVAL, "sharded")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_truth_sam(out + ".sam")
fails(lambda: g.yield_reads_files(out + "_w", 3), SCS_EINVAL, "writers")
with device_buffers(1 << 24) as (d1, d2):
    fails(lambda: g.yield_reads_device(d1, 1 << 24, d2, 1 << 24), SCS_EINVAL, "scs_yield_reads_device")
f1, f2 = g.yield_reads()
open(out + "_1.fq", "wb").write(f1); open(out + "_2.fq", "wb").write(f2)
print("ok")
'''


def test_refusals_leave_the_ctx_usable(models, golden_inputs, tmp_path):
    """6: a sharded ctx, writers = 3 and scs_yield_reads_device with truth set fail with SCS_EINVAL; the ctx then still writes
    reads and their SAM."""
    out = str(tmp_path / "e")
    fa = golden_inputs["g1_hiseq2500_pe"]
    run_child(_ERR, dict(prof=models["Illumina_HiSeq2500"], fa=fa, out=out), timeout=600, ok=True)
    assert not os.path.exists(out + "_w_1.fq") and not os.path.exists(out + "_w.p00_1.fq")
    check_sam(out + ".sam", [out + "_1.fq", out + "_2.fq"], fa, True)
