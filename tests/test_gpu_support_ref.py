"""GPU tests of the site support table on the original reference (scs_set_site_support_ref / `scssim genreads --lift --support-ref`;
DESIGN.md section 19).  The sites are scs_artefact_ref_sites' own; the six counters of every reference position equal the truth SAM
of the same yield call piled up (pileup_from_sam of tests/support_cases.py) at the staged positions the per-base restatement of
tests/support_ref_cases.py names, summed by X(g).  The golden simuvars genome; the dense het layout of tests/lift_cases.py,
held to what it must reach; invariance over fill chunks, slabs, LDS table sizes, batch cuts, sinks and a second call; a plain
genome against --support of the two haplotypes; the file, the CLI, nothing else moving; refusals and ownership.  Each job runs in
a child process under its own time limit; the checks run here.  Run with `-m gpu`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from gpu_child import run_child, sv_ref  # noqa: F401 (a fixture)
from gpu_readers import CLI, SV, Segs, _inflate, make_genome
from lift_cases import write_dense_het_inputs
from site_ref_cases import header
from support_cases import pileup_from_sam
from support_ref_cases import INFO3, fields, restate, strip_support

import scssim_amd

pytestmark = pytest.mark.gpu

KEYS = ("ref_rec", "pos", "ref", "alt", "na", "ta", "nr", "tr")

# one ctx, one genome (built by simuvars, or a FASTA and its lift file), one allocated job, then a yield per leg: {name, ref
# (min_reads of the table on the reference; absent: off), sup (the same of the staged table), w / wr (bin width of the depth track
# and of the one by reference bin), sam, sink (callback / null / files / device), writers, generations, bgzf, env (seams set for the
# leg), write (the table's files and the artefact table's of the same min_reads), art (min_reads of an artefact table on the
# reference written with the feature off)}
_CHILD = r'''
import numpy as np
import scssim_amd
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a, lift_file=True, segs=True)
out = a["out"]
np.savez(out + "_hap.npz", **g.artefact_sites(0))
res = {}
for leg in a["legs"]:
    pre = out + "_" + leg["name"]
    with leg_env(leg.get("env", {})):
        g.set_seed(a["seed"])
        g.set_site_support(False); g.set_site_support_ref(False)
        if "ref" in leg:
            g.set_site_support_ref(True, leg["ref"])
        if "sup" in leg:
            g.set_site_support(True, leg["sup"])
        g.set_depth(leg.get("w", 0)); g.set_depth_ref(leg.get("wr", 0))
        g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
        yield_leg(g, pre, leg)
        r = dict(reads_written=g.stats()["reads_written"], k_support=g.site_support_kernel_time(), k_reads=g.kernel_times()["k_reads"])
        if leg.get("w"):
            dr, db, off = g.depth()
            np.savez(pre + "_depth.npz", reads=dr, bases=db)
        if leg.get("wr"):
            dr, db, dc, off = g.depth_ref()
            np.savez(pre + "_depth_ref.npz", reads=dr, bases=db, copies=dc)
        if "sup" in leg:
            np.savez(pre + "_hsupport.npz", **g.site_support())
            g.write_site_support(pre + "_hsup.vcf")
        if "ref" in leg:
            r["k_support_ref"], r["k_open"], r["k_gather"] = g.site_support_ref_kernel_time(), g.site_support_ref_kernel_time(0), g.site_support_ref_kernel_time(1)
            s = g.site_support_ref(); r["unlifted"] = s.pop("unlifted")
            np.savez(pre + "_support.npz", **s)
            s = g.artefact_ref_sites(leg["ref"]); r["art_unlifted"] = s.pop("unlifted")
            np.savez(pre + "_sites.npz", **s)
            if leg.get("write"):
                r["plain"] = g.write_site_support_ref(pre + ".vcf")
                r["bgzf"] = g.write_site_support_ref(pre + ".vcf.gz", bgzf=True)
                r["art"] = g.write_artefacts_ref(pre + "_art.vcf", min_reads=leg["ref"])
        if "art" in leg:
            r["art"] = g.write_artefacts_ref(pre + "_art.vcf", min_reads=leg["art"])
    res[leg["name"]] = r
g.set_site_support(False); g.set_site_support_ref(False); g.set_depth(0); g.set_depth_ref(0); g.set_truth_sam(None)
g.close()
res["live_closed"] = scssim_amd.live_resources()
emit(res)
'''


def _run(out, legs, env=None, timeout=300, **a):
    a["out"], a["legs"] = str(out), legs
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


class Job:
    """The tables of a job's own ctx the restatement takes: the lift table's segments, the staged and the reference records."""
    def __init__(self, out):
        self.seg = Segs(out)
        table = scssim_amd.lift_file_probe(out + ".lift")
        self.ref_names, self.ref_lens, self.hap_lens = list(table.ref_names), [int(v) for v in table.ref_lens], [int(v) for v in table.hap_lens]
        assert self.seg.ref_lens.tolist() == self.ref_lens
        self.ref_off = np.concatenate([[0], np.cumsum(self.ref_lens)]).astype(np.int64)
        self.hap_off = np.concatenate([[0], np.cumsum(self.hap_lens)]).astype(np.int64)
        self.n = int(self.hap_off[-1])


def check_against_sam(out, name, job):
    """The site arrays are scs_artefact_ref_sites' own; all six counters of every site equal the truth SAM piled up at the
    restatement's staged positions and summed by X(g).  Returns (arrays, X per site, staged positions, index of each one's X among
    the distinct X, SAM counters per staged position, figures)."""
    z, s = np.load(out + "_" + name + "_support.npz"), np.load(out + "_" + name + "_sites.npz")
    for k in KEYS:
        assert z[k].dtype == s[k].dtype and len(z[k]) == len(s[k]) and (z[k] == s[k]).all(), (name, k)
    assert z["counts"].dtype == np.uint32 and z["counts"].shape == (len(z["na"]), 6)
    x = job.ref_off[z["ref_rec"].astype(np.int64)] + z["pos"].astype(np.int64)
    assert (np.diff(x) >= 0).all()
    xs, site_x = np.unique(x, return_inverse=True)
    pos, pos_x, _ = restate(job.n, job.seg, job.ref_lens, xs)
    rec = np.searchsorted(job.hap_off, pos, side="right") - 1
    cnt, sp, fig = pileup_from_sam(out + "_" + name + ".sam", rec, pos - job.hap_off[rec])
    assert len(cnt) == len(pos) and (sp == np.arange(len(pos))).all()          # the staged positions are distinct
    by_x = np.zeros((len(xs), 6), np.int64)
    np.add.at(by_x, pos_x, cnt)
    got, want = z["counts"].astype(np.int64), by_x[site_x]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (name, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    dp = want[:, :5].sum(axis=1)
    assert (want[np.arange(len(x)), np.minimum(z["ref"], 4).astype(np.int64)] * (z["ref"] != z["alt"]) + want[np.arange(len(x)), z["alt"].astype(np.int64)] <= dp).all()
    fig.update(sites=len(x), positions=len(xs), staged=len(pos))
    return z, x, pos, pos_x, cnt, fig


def test_golden_simuvars_genome(sv_ref, models, tmp_path):
    """1: the job of test_gpu_artefacts_ref.py::test_golden_simuvars_genome (PE HiSeq2500 at 2x, seed 41) with --truth in the same
    yield call, at min_reads 0 and 1: the site arrays are artefact_ref_sites(m)'s, the counters the SAM's; nothing in the CN-0
    stretch."""
    legs = [dict(name="m0", ref=0, sam=True), dict(name="m1", ref=1, sam=True)]
    out, res = _run(tmp_path / "job", legs, prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, seed=41)
    job = Job(out)
    assert job.ref_lens == [400000, 150000, 60000] and len(job.seg) == 92
    for name in ("m0", "m1"):
        z, x, pos, pos_x, cnt, fig = check_against_sam(out, name, job)
        print(name, fig, res[name]["k_open"], res[name]["k_gather"], res[name]["k_support_ref"])
        assert fig["records"] == res[name]["reads_written"] > 2000 and fig["contributions"] > 1000 and fig["sites"] > 100
        assert tuple(res[name]["unlifted"]) == tuple(res[name]["art_unlifted"])
        assert not ((z["ref_rec"] == 0) & (z["pos"] >= 149999) & (z["pos"] < 160000)).any()      # c chr20 150000 160000 0 0
        assert res[name]["k_support_ref"] == res[name]["k_support"] and res[name]["k_support"]["launches"] >= 1
        assert res[name]["k_open"]["units"] == res[name]["k_gather"]["units"] == fig["staged"] and res[name]["k_gather"]["launches"] == 1
        copies = np.bincount(pos_x, minlength=fig["positions"])
        assert copies.min() >= 1 and copies.max() > 2                                          # CN up to 8 on this genome
    assert (np.load(out + "_m1_support.npz")["nr"] >= 1).all()


# ---- 2, 3: the dense het layout
DENSE = dict(cov=6.0, seed=19, ber=0.01)
DENSE_LEGS = [dict(name="base", ref=0, sam=True, write=True),
              dict(name="chunk1", ref=0, sink="null", write=True, env=dict(SCS_TEST_SUPPORT_REF_CHUNK="1")),
              dict(name="chunk257", ref=0, sink="null", write=True, env=dict(SCS_TEST_SUPPORT_REF_CHUNK="257")),
              dict(name="slab50", ref=0, sink="null", write=True, env=dict(SCS_TEST_SITE_SLAB="50")),
              dict(name="slab20000", ref=0, sink="null", write=True, env=dict(SCS_TEST_SITE_SLAB="20000")),
              dict(name="dev", ref=0, sink="device", write=True),
              dict(name="parts", ref=0, sink="files", writers=3, generations=2, write=True),
              dict(name="bgzf", ref=0, sink="files", bgzf=True, write=True),
              dict(name="again", ref=0, sink="null", write=True)]


@pytest.fixture(scope="module")
def dense_inputs(tmp_path_factory):
    return write_dense_het_inputs(tmp_path_factory.mktemp("dense_sup_ref_in"))


@pytest.fixture(scope="module")
def dense_job(models, dense_inputs, tmp_path_factory):
    """write_dense_het_inputs at ber 0.01, coverage 6, seed 19 on the seams build, one ctx: the table beside the truth SAM, then the
    same yield again under each seam and sink.  Made once, shared, never changed."""
    ref, var = dense_inputs
    return _run(tmp_path_factory.mktemp("dense_sup_ref") / "job", DENSE_LEGS, env=seams_env(), prof=models["Illumina_HiSeq2500"], ref=ref, vars=var, **DENSE)


def test_dense_layout_reaches_what_it_must(dense_job):
    """2: what the job reaches is computed from the restatement and the SAM, printed and asserted, each at least once, before the
    comparison is relied on."""
    out, res = dense_job
    job = Job(out)
    z, x, pos, pos_x, cnt, fig = check_against_sam(out, "base", job)
    n_x = fig["positions"]
    copies = np.bincount(pos_x, minlength=n_x)
    # the haplotype of every staged index: even staged records are haplotype 1, odd ones haplotype 2
    hap = (np.searchsorted(job.hap_off, pos, side="right") - 1) % 2
    on_hap = np.zeros((n_x, 2), np.int64)
    np.add.at(on_hap, (pos_x, hap), 1)
    xs, site_x = np.unique(x, return_inverse=True)
    _, refs_per_pos = np.unique(np.unique(site_x.astype(np.int64) * 5 + z["ref"].astype(np.int64)) // 5, return_counts=True)   # distinct REF per X
    # staged positions whose own g carries no artefact: no site of the haplotype table (artefact_sites(0) of the same ctx) lies there
    hs = np.load(out + "_hap.npz")
    with_artefact = np.isin(pos, job.hap_off[hs["rec"].astype(np.int64)] + hs["pos"].astype(np.int64))
    spare = ~with_artefact & (cnt.sum(axis=1) > 0)
    c = z["counts"].astype(np.int64)
    reach = dict(sites=fig["sites"], positions=n_x, staged=fig["staged"], two_staged=int((copies == 2).sum()), four_or_more=int((copies >= 4).sum()),
                 one_staged_other_haplotype_lacks_it=int(((copies == 1) & (on_hap.min(axis=1) == 0)).sum()), two_ref=int((refs_per_pos >= 2).sum()),
                 ad_alt=int((c[np.arange(len(x)), z["alt"].astype(np.int64)] > 0).sum()), dl=int((c[:, 5] > 0).sum()), reverse=fig["reverse"], ins_left=fig["ins_left"],
                 staged_without_an_artefact_that_received_reads=int(spare.sum()))
    print("reach", reach, "times", res["base"]["k_open"], res["base"]["k_gather"], res["base"]["k_support"])
    assert min(reach.values()) >= 1, reach
    assert fig["records"] == res["base"]["reads_written"]


def test_invariance_on_the_dense_job(dense_job):
    """3: fill launches of 1 and 257 slots, site slabs of 50 and 20000 reference indices, the text left on the device, files with
    three writers, BGZF files, a second yield call: the counters, the site arrays and the file of the first call, byte for byte."""
    out, res = dense_job
    want, text = np.load(out + "_base_support.npz"), open(out + "_base.vcf", "rb").read()
    assert want["counts"].sum() > 10000 and len(text) > 100000
    for leg in DENSE_LEGS[1:]:
        got = np.load(out + "_" + leg["name"] + "_support.npz")
        assert all(got[k].tobytes() == want[k].tobytes() for k in want.files), leg["name"]
        assert open(out + "_" + leg["name"] + ".vcf", "rb").read() == text, leg["name"]
        assert _inflate(open(out + "_" + leg["name"] + ".vcf.gz", "rb").read()) == text, leg["name"]
        assert res[leg["name"]]["k_support"]["launches"] >= 1 and res[leg["name"]]["k_gather"]["launches"] == 1
    assert res["chunk1"]["k_open"]["units"] == res["base"]["k_open"]["units"] > 257


@pytest.mark.parametrize("knob,value", [("SCS_TEST_SUPPORT_SLOTS", "0"), ("SCS_TEST_SUPPORT_SLOTS", "4"), ("SCS_TEST_SUPPORT_SLOTS", "1024"), ("SCS_TEST_BATCH_SHIFT", "7")])
def test_invariance_over_table_sizes_and_batch_cuts(knob, value, dense_job, dense_inputs, models, tmp_path):
    """3: no LDS table, one of 4 slots, the default's 1024 by name, and batches of 128 pairs (both are read once per process: a job
    of its own each): the counters and the file of the dense job."""
    ref_out, _ = dense_job
    ref, var = dense_inputs
    out, res = _run(tmp_path / "job", [dict(name="v", ref=0, sink="null", write=True)], env=seams_env(**{knob: value}), prof=models["Illumina_HiSeq2500"], ref=ref, vars=var, **DENSE)
    assert np.load(out + "_v_support.npz")["counts"].tobytes() == np.load(ref_out + "_base_support.npz")["counts"].tobytes()
    assert open(out + "_v.vcf", "rb").read() == open(ref_out + "_base.vcf", "rb").read()
    if knob == "SCS_TEST_BATCH_SHIFT":
        assert res["v"]["k_support"]["launches"] == res["v"]["k_reads"]["launches"] >= 8


# ---- 4, 5: a plain genome
PLAIN = dict(cov=3.0, seed=3)
PLAIN_LEGS = [dict(name="before", sup=0, w=100, wr=100, art=0), dict(name="m0", ref=0, w=100, wr=100, sam=True, write=True), dict(name="m1", ref=1, sink="null", write=True),
              dict(name="none", ref=4000000000, sink="null", write=True), dict(name="off", w=100, wr=100, art=0), dict(name="after", sup=0, w=100, wr=100, art=0)]


@pytest.fixture(scope="module")
def plain_job(models, tmp_path_factory):
    """Two reference records, no variant files (one segment per staged record, two haplotypes): `scssim simuvars --lift`, then one
    ctx over the FASTA and the table it wrote: --support before, the table on the reference at min_reads 0, 1 and 4000000000,
    everything off, --support after; both depth tracks beside them."""
    d = tmp_path_factory.mktemp("plain_sup_ref")
    ref, simu, lift = str(d / "ref.fa"), str(d / "simu.fa"), str(d / "simu.lift")
    make_genome(ref, "60000,40500", 17, ref=True)
    r = subprocess.run([CLI, "simuvars", "-r", ref, "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return _run(d / "job", PLAIN_LEGS, prof=models["Illumina_HiSeq2500"], fasta=simu, lift=lift, **PLAIN) + (simu, lift)


def test_plain_genome_equals_the_two_haplotypes_of_the_staged_table(plain_job):
    """4: the counters of a reference position are the sum of --support's counters of the two haplotypes at that coordinate, from a
    separate yield of the same seed.  The issue asks for that equality at every coordinate; as written it cannot be met from the
    --support table, which lists a haplotype's coordinate only where an artefact lies on that haplotype and so has no counters for
    the other haplotype at most positions.  Where it lists both (2167 positions of this job), the sum is asserted; where it lists
    one (20 461), the reference counters are at least that haplotype's (the other's are not negative) -- a weaker bound on purpose,
    not an oversight.  The full equality at every position is held by the truth SAM of the same call (check_against_sam), which
    covers both haplotypes whether or not an artefact lies on them."""
    out, res = plain_job[:2]
    job = Job(out)
    assert len(job.seg) == 4 and job.ref_lens == [60000, 40500] and tuple(res["m0"]["unlifted"]) == (0, 0)
    z, x, pos, pos_x, cnt, fig = check_against_sam(out, "m0", job)
    assert (np.bincount(pos_x) == 2).all()
    h = np.load(out + "_before_hsupport.npz")
    hx = job.ref_off[h["rec"].astype(np.int64) // 2] + h["pos"].astype(np.int64)              # staged records 2 r and 2 r + 1 are reference record r
    by = {}
    for xx, rec, c in zip(hx.tolist(), h["rec"].tolist(), h["counts"].astype(np.int64)):
        by.setdefault(xx, {})[rec % 2] = c
    both = one = 0
    for xx, c in zip(x.tolist(), z["counts"].astype(np.int64)):
        haps = by[xx]
        if len(haps) == 2:
            assert (c == haps[0] + haps[1]).all(), xx
            both += 1
        else:
            assert (c >= next(iter(haps.values()))).all(), xx
            one += 1
    print("positions listed on both haplotypes", both, "on one", one, fig)
    assert both >= 1 and one >= 1 and set(by) == set(x.tolist())


def test_file_and_header_only(plain_job):
    """5: the file at min_reads 0 and 1, plain and BGZF (inflated member by member): stripped of the three lines and the suffix it is
    write_artefacts_ref's file of the same ctx and min_reads; its DP / AD / DL are the arrays'.  A job with no site writes the
    header only."""
    out, res = plain_job[:2]
    job = Job(out)
    for name in ("m0", "m1"):
        text, art = open(out + "_" + name + ".vcf").read(), open(out + "_" + name + "_art.vcf").read()
        assert strip_support(text) == art and text.startswith(header(job.ref_names, job.ref_lens, res[name]["unlifted"]).split("##INFO")[0])
        lines = text.split("\n")
        at = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
        assert lines[at - 3:at] == INFO3 and lines[at - 4].startswith("##INFO=<ID=TR,")
        z = np.load(out + "_" + name + "_support.npz")
        c, n = z["counts"].astype(np.int64), len(z["na"])
        f = [fields(ln) for ln in lines[at + 1:-1]]
        assert len(f) == n == res[name]["plain"]["sites"] > 100 and res[name]["plain"]["bytes"] == len(text)
        idx = np.arange(n)
        assert [v[0] for v in f] == c[:, :5].sum(axis=1).tolist() and [v[2] for v in f] == c[:, 5].tolist()
        assert [v[1] for v in f] == list(zip(c[idx, np.minimum(z["ref"], 4).astype(np.int64)].tolist(), c[idx, z["alt"].astype(np.int64)].tolist()))
        zb = open(out + "_" + name + ".vcf.gz", "rb").read()
        assert _inflate(zb).decode() == text and res[name]["bgzf"] == dict(sites=n, bytes=len(zb))
    assert res["m1"]["plain"]["sites"] < res["m0"]["plain"]["sites"]
    text = open(out + "_none.vcf").read()
    assert res["none"]["plain"] == dict(sites=0, bytes=len(text)) and text == scssim_amd.support_ref_header_probe(job.ref_names, job.ref_lens, res["none"]["unlifted"])
    assert strip_support(text) == open(out + "_none_art.vcf").read() and _inflate(open(out + "_none.vcf.gz", "rb").read()).decode() == text


def test_cli_writes_the_bytes_of_the_api(plain_job, models, tmp_path):
    """5: `scssim genreads --lift --support-ref`, plain, and .gz with --support-min-reads 1."""
    out, res, simu, lift = plain_job
    base = [CLI, "genreads", "-i", simu, "-m", models["Illumina_HiSeq2500"], "-c", "3", "--seed", "3", "--lift", lift]
    for name, extra, want in (("a.vcf", [], "m0"), ("b.vcf.gz", ["--support-min-reads", "1"], "m1")):
        r = subprocess.run(base + ["-o", str(tmp_path / name), "--support-ref", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = open(str(tmp_path / name), "rb").read()
        assert (_inflate(got) if name.endswith(".gz") else got) == open(out + "_" + want + ".vcf", "rb").read() and len(got) > 1000, name
    assert open(str(tmp_path / "a.vcf_1.fq"), "rb").read() == open(out + "_off_1.fq", "rb").read()


def test_nothing_else_moves(plain_job):
    """5: the FASTQ and both depth tracks of the same ctx are the same bytes with the feature on (m0), off, and in the --support
    yields before and after it; the --support table is the same file before and after; the --artefacts-ref file written before the
    feature was ever on, with it off and after it is the one written while it is on."""
    out, res = plain_job[:2]
    for f in ("_1.fq", "_2.fq"):
        want = open(out + "_off" + f, "rb").read()
        assert len(want) > 100000 and all(open(out + "_" + n + f, "rb").read() == want for n in ("before", "m0", "after")), f
    for f in ("_depth.npz", "_depth_ref.npz"):
        a = np.load(out + "_off" + f)
        for n in ("before", "m0", "after"):
            b = np.load(out + "_" + n + f)
            assert all(a[k].tobytes() == b[k].tobytes() for k in a.files) and a["reads"].sum() > 1000, (f, n)
    a, b = open(out + "_before_hsup.vcf", "rb").read(), open(out + "_after_hsup.vcf", "rb").read()
    assert a == b and len(a) > 10000
    a, b = np.load(out + "_before_hsupport.npz"), np.load(out + "_after_hsupport.npz")
    assert all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    want = open(out + "_m0_art.vcf", "rb").read()
    assert len(want) > 10000 and b"##scssim_unlifted=<entries=0,reads=0>\n" in want
    for n in ("before", "off", "after"):
        assert open(out + "_" + n + "_art.vcf", "rb").read() == want and res[n]["art"] == res["m0"]["art"], n
    assert res["off"]["k_support"]["launches"] == 0
    assert res["live_closed"] == [0, 0, 0, 0]


_OWN = r'''
import ctypes, os
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
out = a["out"]
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
s.set_site_support_ref(True)
fails(s.yield_reads, SCS_EINVAL, "scs_set_site_support_ref", "sharded")
s.set_site_support_ref(False)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")      # the refusal is gone: what is missing now is the job itself
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=2.0, seed=5)
g.create_frags(); g.amplify(); g.allocate_reads(0)
census = scssim_amd.live_resources()
g.set_site_support_ref(True)
fails(lambda: g.yield_reads(collect=False), SCS_EINVAL, "scs_set_site_support_ref", "no lift table", "scs_load_lift")
assert scssim_amd.live_resources() == census                # a refused yield call leaves nothing
g.set_site_support_ref(False)
assert scssim_amd.live_resources() == census
g.simuvars(a["ref"], None, None)
g.create_frags(); g.amplify(); g.allocate_reads(0)
for seed in (5, 6):                                         # the yields' own buffers exist before the census is taken
    g.set_seed(seed); g.yield_reads(collect=False)
g.set_seed(5)
before = scssim_amd.live_resources()
fails(g.site_support_ref, SCS_EINVAL, "scs_set_site_support_ref")       # off
g.set_site_support(True, 0)
fails(lambda: g.set_site_support_ref(True, 0), SCS_EINVAL, "scs_set_site_support_ref", "scs_set_site_support(ctx, 0, 0)")
g.set_site_support_ref(False)                               # switching the other table off does not touch this one
g.yield_reads(collect=False)
assert g.site_support()["counts"].sum() > 1000
g.set_site_support(False)
g.set_site_support_ref(True, 0)
fails(lambda: g.set_site_support(True, 0), SCS_EINVAL, "scs_set_site_support", "scs_set_site_support_ref(ctx, 0, 0)")
fails(g.site_support_ref, SCS_EINVAL, "no yield call")      # before any yield
fails(lambda: g.write_site_support_ref(out + "_early.vcf"), SCS_EINVAL, "no yield call")
fails(g.site_support, SCS_EINVAL, "scs_set_site_support")   # the staged table's read-out: its own table is not on
g.set_seed(5); g.yield_reads(collect=False)
first = g.site_support_ref()
kt, ko, kg = g.site_support_ref_kernel_time(), g.site_support_ref_kernel_time(0), g.site_support_ref_kernel_time(1)
assert first["counts"].sum() > 1000 and kt == g.site_support_kernel_time() and kt["launches"] >= 1
# the timer's units are the PLANNED pairs of the batches (as scs_site_support_kernel_time's: equal above); pairs_written leaves out
# the holes (pairs whose insert size found no place), so it may lie below them and never above; k_reads' units are the same pairs
assert kt["units"] == g.kernel_times()["k_reads"]["units"] >= g.stats()["pairs_written"] > 0 and ko["units"] == kg["units"] > 0 and kg["launches"] == 1     # pairs; staged positions
n = ctypes.c_uint64()
fn = g._L.scs_site_support_ref
fn.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 9 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
assert fn(g._ctx, *([None] * 9), 0, ctypes.byref(n), None) == SCS_EOVERFLOW and n.value == len(first["na"]) > 1000      # cap = 0 returns the count
g._L.scs_write_site_support_ref.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
assert g._L.scs_write_site_support_ref(g._ctx, (out + "_flag.vcf").encode(), 2, None, None) == SCS_EINVAL and b"unknown flag" in g._L.scs_last_error(g._ctx)
fails(lambda: g.write_site_support_ref(out + "_no_such_dir/a.vcf"), SCS_EIO, "can not open")
assert g.write_site_support_ref(out + ".vcf")["sites"] == n.value       # the ctx stays usable
g.set_seed(6); g.yield_reads(collect=False)
second = g.site_support_ref()
g.set_seed(5); g.yield_reads(collect=False)
third = g.site_support_ref()
assert (third["counts"] == first["counts"]).all() and (second["counts"] != first["counts"]).any()       # the counters of the new call, not the sum of both
g.set_site_support_ref(False)
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())
fails(lambda: g.write_site_support_ref(out + "_off.vcf"), SCS_EINVAL, "scs_set_site_support_ref")
g.set_seed(5); g.yield_reads(collect=False)
assert g.site_support_ref_kernel_time()["launches"] == 0 and g.site_support_ref_kernel_time(1)["launches"] == 0
assert not os.path.exists(out + "_early.vcf") and not os.path.exists(out + "_flag.vcf") and not os.path.exists(out + "_off.vcf")
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_refusals_and_ownership(sv_ref, models, golden_inputs, tmp_path):
    """6: a sharded ctx and a ctx without a lift table are refused at the yield call by the setter's name; either setter refuses
    while the other table is on, naming both; no read-out or file before a yield; cap = 0 returns the count; an unknown flag bit;
    an unwritable path is SCS_EIO and the ctx goes on; a second yield holds its own counters; the timer's units are pairs;
    scs_live_resources is back after scs_set_site_support_ref(ctx, 0, ..) and zero once the contexts are gone."""
    run_child(_OWN, dict(out=str(tmp_path / "own"), prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], ref=sv_ref), timeout=300, ok=True)
