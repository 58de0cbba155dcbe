"""GPU tests of the truth SAM (scs_set_truth_sam / scssim genreads --truth): the FASTQ does not change, the SAM is complete and
well-formed, and every read lies where its lineage says, base for base.  Each job runs in a child process under its own time
limit; the checks run here.  Run with `-m gpu`."""
import gzip
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seams_env

import scssim_amd

pytestmark = pytest.mark.gpu

_CHILD = r'''
import json, os, sys, ctypes
sys.path.insert(0, %(root)r)
import scssim_amd
a = json.loads(%(args)r)
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=a["cov"], layout=a["layout"], seed=a["seed"], isize=a.get("isize", 260), ber=a.get("ber", 3.4e-4))
out = a["out"]
g.create_frags(); g.amplify(); g.allocate_reads(0)
if a.get("lineage"):
    import numpy as np
    f = g.download_frags(); s = g.download_amplicons(0); u = g.download_amplicons(1)
    np.savez(out + "_lineage.npz", fgoff=f["goff"], flen=f["len"], fstrand=f["strand"], spar=s["parent"], sspos=s["spos"], slen=s["len"],
             upar=u["parent"], uspos=u["spos"], ulen=u["len"])
if a.get("plain"):
    f1, f2 = g.yield_reads()
    open(out + "_plain_1.fq", "wb").write(f1); open(out + "_plain_2.fq", "wb").write(f2)
g.set_truth_sam(out + ".sam")
if a["sink"] == "files":
    g.yield_reads_files(out, 1, bgzf=a.get("bgzf", False))
else:
    f1, f2 = g.yield_reads()
    open(out + "_1.fq", "wb").write(f1); open(out + "_2.fq", "wb").write(f2)
print("truth_bytes", g.truth_bytes(), "pairs", g.stats()["pairs_written"], json.dumps(g.kernel_times()["k_truth"]))
'''


def _run(tmp_path, env=None, timeout=900, **a):
    a.setdefault("out", str(tmp_path / "job"))
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, args=json.dumps(a))], env=env or dict(os.environ),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return a["out"], r.stdout


def _fastq(path):
    op = gzip.open if path.endswith(".gz") else open
    lines = op(path, "rb").read().split(b"\n")
    return [(lines[i][1:].decode(), lines[i + 1].decode(), lines[i + 3].decode()) for i in range(0, len(lines) - 1, 4)]


def _fasta(path):
    recs, name, parts = {}, None, []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            if name is not None:
                recs[name] = b"".join(parts).upper()
            name, parts = ln[1:].split()[0].decode(), []
        else:
            parts.append(ln.strip())
    recs[name] = b"".join(parts).upper()
    return {k: re.sub(rb"[^ACGT]", b"N", v) for k, v in recs.items()}


def _sam(path):
    hdr, recs = [], []
    for ln in open(path).read().split("\n")[:-1]:
        (hdr if ln.startswith("@") else recs).append(ln if ln.startswith("@") else ln.split("\t"))
    return hdr, recs


CIG = re.compile(r"(\d+)([MID])")
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


def _oracle(oracle_bin, fa, prof, prefix, args, seed):
    subprocess.check_call([oracle_bin, "genreads", "-i", fa, "-m", prof, "-o", prefix, "--rng", "counter", "--seed", str(seed), "-t", "16", "-q"] + args)


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
    assert int(so.split()[1]) == os.path.getsize(out + ".sam")


def _exact_profile(src, dst, ins, dele):
    """Substitution rows with all their mass on the row's own base (kmer XYZ -> Z), and the given indel rates."""
    lines = open(src).read().split("\n")
    out, i, L = [], 0, None
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("readLength:"):
            L = int(ln.split(":")[1])
        if ln in ("[Insert Rate]", "[Deletion Rate]"):
            out += [ln, "%g" % (ins if ln == "[Insert Rate]" else dele)]
            i += 2
            continue
        m = re.match(r"kmer: ([ACGTNX]{3})$", ln)
        if m:
            b = m.group(1)[2]
            out.append(ln)
            row = "\t".join("1" if c == b else "0" for c in "ACGT")
            for r in lines[i + 1:i + 1 + 2 * L]:
                out.append(row if b in "ACGT" else r)
            i += 1 + 2 * L
            continue
        out.append(ln)
        i += 1
    open(dst, "w").write("\n".join(out))
    return dst


@pytest.mark.parametrize("variant", ["plain", "replay", "rollback51"])
def test_exact_placement(variant, models, tmp_path):
    """3: an N-free genome, no amplification errors, substitution rows that always call the window's base and frequent indels:
    every read is the genome under its CIGAR (inserted bases aside) and NM is its indel bases.  An off-by-one anywhere shows as
    ~75 % mismatches.  replay: every read with events takes the replay path (SCS_EV_REPLAY).  rollback51: 51-base reads with
    many deletions, so that n + delta < 50 rolls reads back to no events at all."""
    fa = str(tmp_path / "g.fa")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", "400000,300000", "--seed", "17", "--simu-out", fa])
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
    fa = str(tmp_path / "simu.fa")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", "7000000,5000000", "--seed", "31", "--n-block", "20000", "--simu-out", fa])
    out, _ = _run(tmp_path, env=seams_env(SCS_TEST_BATCH_SHIFT="12"), prof=models["Illumina_HiSeqXTen"], fa=fa, cov=1.0, layout="PE", seed=8,
                  sink=sink, bgzf=True, lineage=True)
    fqs = [out + m + (".fq.gz" if sink == "files" else ".fq") for m in ("_1", "_2")]
    check_sam(out + ".sam", fqs, fa, True, isize=260, lineage=out + "_lineage.npz")


# ---- the emit pass under a cut LDS (SCS_TEST_TRUTH_LDS).  The job: test_gpu_truth_bam.py::test_frequent_indels' genome and
# profile (insertion and deletion rates 0.01, no substitution anywhere), PE, at a coverage of 0.2: 350 kb / (2 x 125) x 0.2 = 280 pairs
CUT_JOB = dict(cov=0.2, layout="PE", seed=7, sink="callback", ber=0.0)
CUT_LDS = 256                                             # bytes: below any pair of the job (pair_floor)


def cut_job_inputs(d, models):
    fa = str(d / "g.fa")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", "200000,150000", "--seed", "17", "--simu-out", fa])
    return fa, _exact_profile(models["Illumina_HiSeq2500"], str(d / "x.profile"), 0.01, 0.01)


def pair_floor(probe, rname, **kw):
    """Bytes of the smallest pair of records a job can hold, on the CPU, through the formatter the kernels run (`probe`: one of the
    record probes of scssim_amd).  The shortest read the profile admits has n + delta = 50 bases (fewer: the events are rolled
    back); its smallest record has every field at its narrowest: amplicon 0, count 1, a one-digit POS and PNEXT, FLAG 99, TLEN 50,
    the 75 deleted bases at the window's end (dropped from the CIGAR: "50M"), no mismatch.  A pair is two records, read 2's FLAG
    (147) a digit wider."""
    ev = [(50, 1, 75)]
    rec = probe(seq="A" * 50, qual="I" * 50, pos0=0, n=125, events=ev, reverse=False, rname=rname, amp=0, cnt=1, paired=True, is_read2=False, mate=(49, True, ev), **kw)
    return 2 * len(rec)


@pytest.fixture(scope="module")
def cut_reference(models, tmp_path_factory):
    """The job with the emit pass as shipped: its SAM checked against the genome, its FASTQ against a yield without the SAM."""
    d = tmp_path_factory.mktemp("cut")
    fa, prof = cut_job_inputs(d, models)
    out, so = _run(d, prof=prof, fa=fa, plain=True, **CUT_JOB)
    pairs = int(so.split()[3])
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
import sys, ctypes
sys.path.insert(0, %(root)r)
import scssim_amd
from scssim_amd import ScsError, SCS_EINVAL
kw = dict(profile=%(prof)r, input_fasta=%(fa)r, coverage=2.0, seed=5)
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=kw["profile"], seed=5)
s.set_truth_sam(%(out)r + "_s.sam")
try:
    s.yield_reads(); raise SystemExit("sharded: no error")
except ScsError as e:
    assert e.code == SCS_EINVAL and "sharded" in str(e), e
g = scssim_amd.GenReads(**kw)
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_truth_sam(%(out)r + ".sam")
try:
    g.yield_reads_files(%(out)r + "_w", 3); raise SystemExit("writers: no error")
except ScsError as e:
    assert e.code == SCS_EINVAL and "writers" in str(e), e
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
d1, d2 = ctypes.c_void_p(), ctypes.c_void_p()
assert hip.hipMalloc(ctypes.byref(d1), 1 << 24) == 0 and hip.hipMalloc(ctypes.byref(d2), 1 << 24) == 0
try:
    g.yield_reads_device(d1, 1 << 24, d2, 1 << 24); raise SystemExit("device: no error")
except ScsError as e:
    assert e.code == SCS_EINVAL and "scs_yield_reads_device" in str(e), e
f1, f2 = g.yield_reads()
open(%(out)r + "_1.fq", "wb").write(f1); open(%(out)r + "_2.fq", "wb").write(f2)
print("ok")
'''


def test_refusals_leave_the_ctx_usable(models, golden_inputs, tmp_path):
    """6: a sharded ctx, writers = 3 and scs_yield_reads_device with truth set fail with SCS_EINVAL; the ctx then still writes
    reads and their SAM."""
    out = str(tmp_path / "e")
    fa = golden_inputs["g1_hiseq2500_pe"]
    r = subprocess.run([sys.executable, "-c", _ERR % dict(root=ROOT, prof=models["Illumina_HiSeq2500"], fa=fa, out=out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert not os.path.exists(out + "_w_1.fq") and not os.path.exists(out + "_w.p00_1.fq")
    check_sam(out + ".sam", [out + "_1.fq", out + "_2.fq"], fa, True)
