"""GPU tests of the truth SAM on the original reference (scs_set_truth_ref_sam, `scssim genreads --lift --truth-ref`; DESIGN.md
section 17).  Each job runs twice on one ctx with the same seed -- haplotype SAM, then reference SAM: every record of the second
equals the restatement's lift (tests/truth_ref_cases.py) of the first through the downloaded table, byte for byte; an independent
column check of every record through scs_lift_positions; the dense layout, where cuts, gaps and insertions meet; a plain genome;
the file does not depend on sinks, batch cuts or the emit pass' LDS run, and the FASTQ does not know of it; the two-step flow
through the CLI; refusals and ownership.  Each job runs in a child process under its own time limit.  Run with `-m gpu`."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child, sv_ref  # noqa: F401 (a fixture)
from gpu_readers import CIG, CLI, SV, Segs, _exact_profile, _sam, make_genome
from lift_cases import DENSE_COV, expected_reach, lift_from_sam, write_dense_inputs
from truth_ref_cases import lift_sam_records, table_from_lift_file

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one genome built by simuvars, one amplified job, then a yield per leg with the same seed:
# {name, truth ("sam" / "ref" / none), sink (callback / null / files), bgzf, wr (depth by reference bin), support}; then the column check
_CHILD = r'''
import scssim_amd
from gpu_child import emit, job_args, open_job, yield_leg
a = job_args()
g = open_job(a, lift_file=True, segs=True)
out = a["out"]
res = {}
for leg in a["legs"]:
    pre = out + "_" + leg["name"]
    g.set_seed(a["seed"])
    g.set_depth_ref(leg.get("wr", 0)); g.set_site_support(bool(leg.get("support")), 0)
    g.set_truth_sam(None); g.set_truth_ref_sam(None)
    if leg.get("truth") == "sam":
        g.set_truth_sam(pre + ".sam")
    if leg.get("truth") == "ref":
        g.set_truth_ref_sam(pre + ".sam")
    yield_leg(g, pre, leg)
    res[leg["name"]] = dict(reads_written=g.stats()["reads_written"], truth_bytes=g.truth_bytes(), k_truth=g.kernel_times()["k_truth"], k_reads=g.kernel_times()["k_reads"])
if a.get("column_check"):
    from truth_ref_cases import column_check, table_from_lift_file
    from gpu_readers import _sam
    hap, ref = a["column_check"]
    res["columns"] = column_check(table_from_lift_file(out + ".lift"), _sam(out + "_" + hap + ".sam")[1], _sam(out + "_" + ref + ".sam")[1], g.lift_positions)
g.close()
res["live_end"] = scssim_amd.live_resources()
emit(res)
'''


def _run(tmp_path, legs, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"] = legs
    res = run_child(_CHILD, a, env=env, timeout=timeout)
    assert res["live_end"] == [0, 0, 0, 0]
    return a["out"], res


PAIR = [dict(name="hap", truth="sam"), dict(name="ref", truth="ref")]


def check_lifted(out, res, paired, hap="hap", ref="ref"):
    """Checks 1 and 2: the header, every record against the restatement's lift of the haplotype SAM's record, the record count, the
    bytes the ctx reports, the column check the child ran on every record.  Returns the reference SAM's records."""
    t = table_from_lift_file(out + ".lift")
    seg = Segs(out)
    assert all((getattr(seg, k) == getattr(t, k)).all() for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")) and seg.ref_lens.tolist() == t.ref_lens   # the downloaded table
    hdr, hap_recs = _sam(out + "_" + hap + ".sam")
    text = open(out + "_" + ref + ".sam").read()
    lines = text.split("\n")[:-1]
    n_hdr = len(t.ref_names) + 2
    assert lines[:n_hdr] == ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % x for x in zip(t.ref_names, t.ref_lens)] + ["@PG\tID:scssim\tPN:scssim"]
    want = lift_sam_records(t, hap_recs, paired)
    got = [ln + "\n" for ln in lines[n_hdr:]]
    assert len(got) == len(want) == res[ref]["reads_written"] == res[hap]["reads_written"] > 500
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, (len(bad), got[bad[0]], want[bad[0]])
    assert res[ref]["truth_bytes"] == len(text.encode()) and res[ref]["k_truth"]["launches"] == 2 * res[ref]["k_reads"]["launches"] >= 2 and res[ref]["k_truth"]["units"] > 0
    n, n_cols, n_unmapped = res["columns"]
    recs = [ln.split("\t") for ln in lines[n_hdr:]]
    assert n == len(got) and n_cols > 50 * (n - n_unmapped) and n_unmapped == sum(1 for r in recs if int(r[1]) & 4)
    for m in ("_1.fq", "_2.fq"):
        assert open(out + "_" + hap + m, "rb").read() == open(out + "_" + ref + m, "rb").read()
    return recs


def test_golden_simuvars_genome(sv_ref, models, tmp_path):
    """1, 2: the golden simuvars genome (1.5 Mb staged, CN 0 .. 8, three reference records), PE HiSeq2500 at 2x, seed 41."""
    out, res = _run(tmp_path, PAIR, prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, layout="PE", seed=41,
                    column_check=["hap", "ref"])
    recs = check_lifted(out, res, True)
    assert any(int(r[13][5:]) >= 2 for r in recs) and any("D" in r[5] for r in recs)    # a copy junction and a planted deletion are crossed
    # a planted insertion, spanned: more I bases than the haplotype record has (this model's sequencing insertions reach 29 bases,
    # the planted ones 8: by length alone the two cannot be told apart here)
    i_sum = lambda c: sum(int(n) for n, k in re.findall(r"(\d+)([MIDS])", c) if k == "I")
    n_planted = sum(1 for h, r in zip(_sam(out + "_hap.sam")[1], recs) if i_sum(r[5]) > i_sum(h[5]))
    print("records that show a planted insertion as I: %d" % n_planted)
    assert n_planted >= 1


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    ref, var = write_dense_inputs(d)
    table, _ = scssim_amd.lift_plan_probe(ref, None, var)
    return dict(ref=ref, var=var, table=table, dir=d)


@pytest.mark.parametrize("model,layout,L", [("Illumina_HiSeq2000", "SE", 75), ("Illumina_HiSeq2500", "PE", 125)])
def test_dense_layout(model, layout, L, dense, models, tmp_path):
    """3: the jobs of test_gpu_lift.py::test_dense_layout (60 kb, 2031 segments, frequent sequencing indels, 14x, seed 19): the
    geometry is checked on the CPU first, what the reads reached is asserted from the haplotype SAM, and the reference SAM must show
    every branch it can reach -- two blocks, both clips, a collinear gap, an unmapped read -- before checks 1 and 2 run."""
    t = dense["table"]
    n_reads = DENSE_COV * float(np.asarray(t.ref_lens).sum()) / L
    exp = expected_reach(t, L, n_reads)
    assert exp["cross"] > 0.55 * n_reads and min(exp["cross2"], exp["wholly_inserted"], exp["starts_inserted"], exp["back"]) >= 8, exp
    prof = _exact_profile(models[model], str(tmp_path / "x.profile"), 0.004, 0.004)
    out, res = _run(tmp_path, PAIR, prof=prof, ref=dense["ref"], vars=dense["var"], cov=DENSE_COV, layout=layout, seed=19, ber=0.0, column_check=["hap", "ref"])
    seg = Segs(out)
    assert len(seg) == len(t) == 2031
    reach = lift_from_sam(out + "_hap.sam", seg, 37)[4]
    assert reach["cross"] > 0.5 * reach["n"], reach
    assert reach["cross2"] >= 1 and reach["starts_inserted"] >= 1 and reach["wholly_inserted"] >= 1 and reach["back"] >= 1 and reach["deletion_and_boundary"] >= 1, reach
    recs = [ln.split("\t") for ln in open(out + "_ref.sam").read().split("\n")[:-1] if not ln.startswith("@")]
    ops = [[(int(n), k) for n, k in re.findall(r"(\d+)([MIDS])", r[5])] for r in recs]
    seq_ins = max(int(n) for r in _sam(out + "_hap.sam")[1] for n, k in CIG.findall(r[5]) if k == "I")
    r_seg = seg.kind == 0                                                                    # a collinear gap: from the end of an R segment to the start of one
    ends, starts = set((seg.ref_pos + seg.len)[r_seg].tolist()), set(seg.ref_pos[r_seg].tolist())

    def has_gap_d(r, o):
        x = int(r[3]) - 1
        for n, k in o:
            if k == "D" and x in ends and x + n in starts:
                return True
            x += n if k in "MD" else 0
        return False
    assert any(int(r[13][5:]) >= 2 for r in recs)
    assert any(o and o[0][1] == "S" for o in ops) and any(o and o[-1][1] == "S" for o in ops)
    # An I made of a planted insertion needs an M base on both sides of the whole I segment.  This layout cannot show one: its
    # insertions are 130 bases and a read's window is 75 or 125 haplotype bases, so what a read holds of one is clipped.  That branch
    # is asserted where reads span planted insertions: test_golden_simuvars_genome (insertions of 4 .. 8 bases).
    assert int(seg.len[seg.kind == 1].min()) == 130 > L and max(n for o in ops for n, k in o if k == "I") <= seq_ins < 130
    assert any(has_gap_d(r, o) for r, o in zip(recs, ops))
    assert sum(1 for r in recs if int(r[1]) & 4) == reach["wholly_inserted"] >= 1
    check_lifted(out, res, layout == "PE")


def test_plain_genome(models, tmp_path):
    """4: simuvars without variants, one R segment per staged record: every record is the haplotype SAM's line with RNAME mapped to
    the reference's name, NM / MD replaced by YH / YP / YB:i:1 and an I at either end turned into S."""
    ref = make_genome(str(tmp_path / "ref.fa"), "60000,40500", 17, ref=True)
    out, res = _run(tmp_path, PAIR, prof=models["Illumina_HiSeq2500"], ref=ref, cov=3.0, layout="PE", seed=3)
    t = table_from_lift_file(out + ".lift")
    assert len(t) == 4 and t.ref_lens == [60000, 40500]
    to_ref = {h: t.ref_names[i // 2] for i, h in enumerate(t.hap_names)}
    hap = _sam(out + "_hap.sam")[1]
    got = [ln for ln in open(out + "_ref.sam").read().split("\n")[:-1] if not ln.startswith("@")]
    assert len(got) == len(hap) == res["ref"]["reads_written"] > 500
    n_clipped = 0
    for h, ln in zip(hap, got):
        ops = [[int(n), k] for n, k in CIG.findall(h[5])]
        for end in (0, -1):
            if ops[end][1] == "I":
                ops[end][1] = "S"; n_clipped += 1
        want = h[:2] + [to_ref[h[2]], h[3], h[4], "".join("%d%s" % (n, k) for n, k in ops)] + h[6:11] + ["YH:Z:" + h[2], "YP:i:" + h[3], "YB:i:1"]
        assert ln == "\t".join(want), (ln, want)
    assert n_clipped >= 1


INV = dict(cov=24.0, layout="PE", seed=23)                 # the dense genome at 24x of its 60 kb reference: 5760 pairs -- two batches of 4096 at SCS_TEST_BATCH_SHIFT=12


@pytest.fixture(scope="module")
def invariance_reference(dense, models, tmp_path_factory):
    """The one PE job of check 5 on one ctx, every sink: computed once, shared, never changed."""
    d = tmp_path_factory.mktemp("inv")
    legs = [dict(name="off"), dict(name="hap", truth="sam"), dict(name="ref", truth="ref"), dict(name="null", truth="ref", sink="null"), dict(name="files", truth="ref", sink="files"),
            dict(name="bgzf", truth="ref", sink="files", bgzf=True), dict(name="beside", truth="ref", wr=100, support=True)]
    return _run(d, legs, prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], column_check=["hap", "ref"], **INV)


def test_sinks_do_not_matter_and_the_fastq_does_not_move(invariance_reference):
    """5: callback, NULL and file sinks, BGZF FASTQ, beside the depth by reference bin and the site support: one file; the FASTQ
    with the output on is the FASTQ with it off."""
    out, res = invariance_reference
    check_lifted(out, res, True)
    want = open(out + "_ref.sam", "rb").read()
    assert res["ref"]["reads_written"] > 2 * 4096
    for name in ("null", "files", "bgzf", "beside"):
        assert open(out + "_" + name + ".sam", "rb").read() == want, name
        assert res[name]["truth_bytes"] == len(want)
    assert res["off"]["truth_bytes"] == 0 and res["off"]["k_truth"]["launches"] == 0
    for m in ("_1.fq", "_2.fq"):
        off = open(out + "_off" + m, "rb").read()
        assert len(off) > 100000 and open(out + "_ref" + m, "rb").read() == off == open(out + "_files" + m, "rb").read() == open(out + "_beside" + m, "rb").read()
        assert gzip.open(out + "_bgzf" + m + ".gz", "rb").read() == off


@pytest.mark.parametrize("knob,value", [("SCS_TEST_BATCH_SHIFT", "12"), ("SCS_TEST_BATCH_SHIFT", "8"), ("SCS_TEST_TRUTH_LDS", "4096")])
def test_invariance_over_batch_cuts_and_the_lds_run(knob, value, invariance_reference, dense, models, tmp_path):
    """5: batches of 4096 pairs and of 256, and an emit pass whose LDS run holds 4096 bytes (about five pairs a turn): the file of
    the default build."""
    ref_out, _ = invariance_reference
    out, res = _run(tmp_path, [dict(name="v", truth="ref", sink="null")], env=seams_env(**{knob: value}), prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], **INV)
    assert open(out + "_v.sam", "rb").read() == open(ref_out + "_ref.sam", "rb").read()
    if knob == "SCS_TEST_BATCH_SHIFT":
        assert res["v"]["k_truth"]["launches"] == 2 * res["v"]["k_reads"]["launches"] >= 2 * ((res["v"]["reads_written"] // 2) >> int(value)) >= 2


def test_two_step_flow_through_the_cli(sv_ref, models, tmp_path):
    """6: `scssim simuvars --lift`, then `scssim genreads --lift --truth-ref`: the file is the in-process route's, byte for byte."""
    prof, simu, lift, pre = models["Illumina_HiSeq2500"], str(tmp_path / "simu.fa"), str(tmp_path / "simu.lift"), str(tmp_path / "cli")
    r = subprocess.run([CLI, "simuvars", "-r", sv_ref, "-s", os.path.join(SV, "snp.txt"), "-v", os.path.join(SV, "vars.txt"), "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([CLI, "genreads", "-i", simu, "-m", prof, "-c", "1", "-o", pre, "--seed", "77", "--lift", lift, "--truth-ref", pre + ".ref.sam"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, res = _run(tmp_path, [dict(name="api", truth="ref")], prof=prof, ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=1.0, layout="PE", seed=77)
    text = open(pre + ".ref.sam", "rb").read()
    assert text == open(out + "_api.sam", "rb").read() and text.count(b"\n") == res["api"]["reads_written"] + 5 > 500
    for m in ("_1.fq", "_2.fq"):
        assert open(pre + m, "rb").read() == open(out + "_api" + m, "rb").read()


_OWN = r'''
import os
import scssim_amd
from scssim_amd import SCS_EINVAL
from gpu_child import device_buffers, fails, job_args
a = job_args()
out = a["out"]
kw = dict(profile=a["prof"], coverage=2.0, seed=5)
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, **kw)
s.set_truth_ref_sam(out + "_s.sam")
fails(s.yield_reads, SCS_EINVAL, "sharded", "scs_set_truth_ref_sam")
# a genome without a lift table
g = scssim_amd.GenReads(**kw)
g.load_genome(a["fa"])
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_truth_ref_sam(out + "_nolift.sam")
fails(g.yield_reads, SCS_EINVAL, "scs_set_truth_ref_sam", "scs_load_lift", "scs_simuvars")
g.set_truth_ref_sam(None)
# a genome with its table
g.simuvars(a["ref"], None, None)
g.create_frags(); g.amplify(); g.allocate_reads(0)
for seed in (5, 6):                                         # the yields' own buffers exist before the census is taken
    g.set_seed(seed); g.yield_reads()
g.set_seed(5)
before = scssim_amd.live_resources()
g.set_truth_sam(out + "_h.sam")
fails(lambda: g.set_truth_ref_sam(out + "_r.sam"), SCS_EINVAL, "scs_set_truth_sam", "scs_set_truth_ref_sam")
g.set_truth_ref_sam(None)                                   # clears only its own: the SAM stays on
fails(lambda: g.set_truth_bam(out + "_b.bam"), SCS_EINVAL, "scs_set_truth_sam", "scs_set_truth_bam")
g.set_truth_sam(None)
g.set_truth_bam(out + "_b.bam")
fails(lambda: g.set_truth_ref_sam(out + "_r.sam"), SCS_EINVAL, "scs_set_truth_bam", "scs_set_truth_ref_sam")
g.set_truth_bam(None)
g.set_truth_ref_sam(out + "_r.sam")
fails(lambda: g.set_truth_sam(out + "_h.sam"), SCS_EINVAL, "scs_set_truth_ref_sam", "scs_set_truth_sam")
fails(lambda: g.set_truth_bam(out + "_b.bam"), SCS_EINVAL, "scs_set_truth_ref_sam", "scs_set_truth_bam")
g.set_truth_sam(None); g.set_truth_bam(None)                # ... and the reference SAM stays on
fails(lambda: g.yield_reads_files(out + "_w", 3), SCS_EINVAL, "writers", "scs_set_truth_ref_sam")
with device_buffers(1 << 24) as (d1, d2):
    fails(lambda: g.yield_reads_device(d1, 1 << 24, d2, 1 << 24), SCS_EINVAL, "scs_yield_reads_device", "scs_set_truth_ref_sam")
g.yield_reads()
during = scssim_amd.live_resources()
n = g.truth_bytes()
assert n == len(open(out + "_r.sam", "rb").read()) > 100000 and g.kernel_times()["k_truth"]["launches"] >= 2
g.set_truth_ref_sam(None)
after = scssim_amd.live_resources()
assert during[0] > before[0] and after == before, (before, during, after)
g.set_seed(5); g.yield_reads()
assert g.kernel_times()["k_truth"]["launches"] == 0
assert not any(os.path.exists(out + x) for x in ("_s.sam", "_nolift.sam", "_h.sam", "_b.bam", "_w_1.fq"))
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(models, golden_inputs, tmp_path):
    """7: a sharded ctx, a ctx without a lift table, writers = 3 and scs_yield_reads_device fail the yield call with SCS_EINVAL by the
    setter's name; one truth output per ctx, every way round, NULL clearing only its own; scs_live_resources is back after the
    output is switched off, and zero once the contexts are gone."""
    ref = make_genome(str(tmp_path / "ref.fa"), "60000,40500", 17, ref=True)
    run_child(_OWN, dict(out=str(tmp_path / "own"), prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], ref=ref), timeout=300, ok=True)
