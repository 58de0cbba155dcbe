"""GPU tests of the artefact table (scs_write_artefacts / scs_artefact_sites / scssim genreads --artefacts): the file and the
arrays equal what the restatement of tests/site_cases.py makes of the amplicon table rebuilt from the oracle's dump, byte for
byte; the same ctx's scs_amplicon_places agree; dense edits (ber = 0.01); slab, chunk and LDS edges; BGZF; the CLI; the refusals
and the ownership of the buffers.  Each job runs in a child process under its own time limit; the checks run here.
Run with `-m gpu`."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import seams_env
from amp_cases import parse_table, table_from_oracle
from gpu_child import run_child
from gpu_readers import CLI, EOF_BLOCK, _oracle, _same, make_genome
from site_cases import KEYS, fasta, figures, header, most_alts_at_a_coordinate, sites_from_table

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one allocated job: the table as VCF (min_reads 0 and 1, BGZF) and as arrays, the amplicon places (and table) of the same ctx.
# variants: [{name, env, bgzf}]: the plain file again under these seams (read at every call by the seams build)
_CHILD = r'''
import numpy as np
import scssim_amd
from gpu_child import emit, job_args, leg_env, open_job
a = job_args()
g = open_job(a)
out = a["out"]
live0 = scssim_amd.live_resources()
res = dict(plain=g.write_artefacts(out + ".vcf"), kt=g.artefact_kernel_time(), live0=live0, live1=scssim_amd.live_resources())
res["min1"] = g.write_artefacts(out + "_m1.vcf", min_reads=1)
res["bgzf"] = g.write_artefacts(out + ".vcf.gz", bgzf=True)
res["none"] = g.write_artefacts(out + "_none.vcf", min_reads=4000000000)
res["none_bgzf"] = g.write_artefacts(out + "_none.vcf.gz", bgzf=True, min_reads=4000000000)
np.savez(out + "_sites.npz", **g.artefact_sites()); np.savez(out + "_sites1.npz", **g.artefact_sites(1))
res["kt_after_arrays"] = g.artefact_kernel_time()
res["live2"] = scssim_amd.live_resources()
np.savez(out + "_places.npz", **g.amplicon_places())
if a.get("table"):
    g.write_amplicons(out + ".tsv")
for v in a.get("variants", []):
    with leg_env(v["env"]):
        res[v["name"]] = g.write_artefacts(out + "_" + v["name"] + ".vcf")
        if v.get("bgzf"):
            g.write_artefacts(out + "_" + v["name"] + ".vcf.gz", bgzf=True)
emit(res)
'''


def _run(out, env=None, timeout=300, **a):
    a["out"] = str(out)
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


JOBS = {"g1_hiseq2500_pe": ("Illumina_HiSeq2500", "PE", 3.0, 41), "g3_hiseq2000_se": ("Illumina_HiSeq2000", "SE", 2.0, 23), "g2_xten_pe_nblock": ("Illumina_HiSeqXTen", "PE", 2.0, 41)}
# the oracle's own figures, counted on the CPU: sites, edit entries, sites with NA >= 2, largest NA, coordinates with two or more
# alternate bases, sites with NR = 0; and the lines left at min_reads = 1
FIGURES = {"g1_hiseq2500_pe": ((22834, 42024, 2429, 44, 728, 21663), 1171), "g2_xten_pe_nblock": ((24677, 45877, 2578, 36, 981, 24034), 643),
           "g3_hiseq2000_se": ((19890, 36824, 2124, 45, 777, 18204), 1686)}
G1_VARIANTS = [dict(name="slab1000", env=dict(SCS_TEST_SITE_SLAB="1000")), dict(name="slab4096", env=dict(SCS_TEST_SITE_SLAB="4096")),
               dict(name="slab200", env=dict(SCS_TEST_SITE_SLAB="200")),                       # 1200 slabs: more than the counting pass sums in LDS
               dict(name="chunk257", env=dict(SCS_TEST_AMP_CHUNK="257")), dict(name="lds16", env=dict(SCS_TEST_SITE_LDS="16")),
               dict(name="piece4099", env=dict(SCS_TEST_SITE_PIECE="4099"), bgzf=True),             # the slab's bytes cross to the host in 285 pieces
               dict(name="all", env=dict(SCS_TEST_SITE_SLAB="1000", SCS_TEST_AMP_CHUNK="257", SCS_TEST_SITE_LDS="16", SCS_TEST_SITE_PIECE="1000"), bgzf=True)]


def _job(case, models, golden_inputs, out, **kw):
    model, layout, cov, seed = JOBS[case]
    return _run(out, prof=models[model], fa=golden_inputs[case], cov=cov, layout=layout, seed=seed, **kw)


@pytest.fixture(scope="module")
def g1_job(models, golden_inputs, tmp_path_factory):
    """g1 (PE, 3x, seed 41) on the seams build: the table in every form, and again under the seams.  Made once, shared, never changed."""
    return _job("g1_hiseq2500_pe", models, golden_inputs, tmp_path_factory.mktemp("g1") / "job", env=seams_env(), variants=G1_VARIANTS)


@pytest.fixture(scope="module")
def g2_job(models, golden_inputs, tmp_path_factory):
    return _job("g2_xten_pe_nblock", models, golden_inputs, tmp_path_factory.mktemp("g2") / "job", env=seams_env(),
                variants=[dict(name="slab1000", env=dict(SCS_TEST_SITE_SLAB="1000"))])


def _reference(case, oracle_bin, models, golden_inputs, tmp_path):
    model, layout, cov, seed = JOBS[case]
    fa, orc = golden_inputs[case], str(tmp_path / "orc")
    _oracle(oracle_bin, fa, models[model], orc, ["-c", "%g" % cov, "-l", layout, "--dump", orc], seed)
    names, lens, G = fasta(fa)
    assert names == scssim_amd.fasta_probe(fa)[0]
    text, _, _, _ = table_from_oracle(orc, names, lens, G)
    return names, lens, G, parse_table(text)


@pytest.mark.parametrize("case", list(JOBS))
def test_file_and_arrays_equal_the_restatement_of_the_oracles_tables(case, g1_job, g2_job, oracle_bin, models, golden_inputs, tmp_path):
    """1: the oracle in counter mode dumps its fragments, amplicons and read numbers; the restatement groups the rebuilt table's edits
    by site; the GPU's file and arrays equal it byte for byte, at min_reads 0 and 1.  The reference itself is held to the oracle's
    figures counted on the CPU, so that no run passes on an empty or trivial table."""
    out, res = g1_job if case == "g1_hiseq2500_pe" else g2_job if case == "g2_xten_pe_nblock" else _job(case, models, golden_inputs, tmp_path / "job")
    names, lens, G, tab = _reference(case, oracle_bin, models, golden_inputs, tmp_path)
    want, arr = sites_from_table(tab, names, lens, G)
    assert figures(arr) == FIGURES[case][0]
    hd = header(names, lens)
    _same(open(out + ".vcf").read(), hd + want, "min_reads 0")
    assert res["plain"] == dict(sites=len(arr["na"]), bytes=len(hd + want)) and os.path.getsize(out + ".vcf") == len(hd + want)
    want1, arr1 = sites_from_table(tab, names, lens, G, 1)
    assert want1.count("\n") == FIGURES[case][1] and want1 == "".join(ln + "\n" for ln in want.split("\n")[:-1] if ";NR=0;" not in ln)
    _same(open(out + "_m1.vcf").read(), hd + want1, "min_reads 1")
    assert res["min1"] == dict(sites=FIGURES[case][1], bytes=len(hd + want1))
    for f, ref in (("_sites.npz", arr), ("_sites1.npz", arr1)):
        z = np.load(out + f)
        assert z["rec"].dtype == np.uint32 and z["pos"].dtype == np.uint64 and z["ref"].dtype == np.uint8 and z["nr"].dtype == np.uint64
        for k in KEYS:
            assert len(z[k]) == len(ref[k]) and (z[k].astype(np.int64) == ref[k]).all(), (f, k)
    assert (arr["na"] >= 1).all() and (arr["na"] <= arr["ta"]).all() and (arr["nr"] <= arr["tr"]).all()
    # a job's table without a site: the header, and in BGZF the end-of-file block
    assert open(out + "_none.vcf").read() == hd and res["none"] == dict(sites=0, bytes=len(hd))
    zn = open(out + "_none.vcf.gz", "rb").read()
    assert gzip.decompress(zn).decode() == hd and zn[-28:] == EOF_BLOCK and res["none_bgzf"] == dict(sites=0, bytes=len(zn))
    kt = res["kt"]
    assert kt["launches"] >= 3 and kt["units"] == len(arr["na"]) and kt["ms"] > 0 and res["kt_after_arrays"]["units"] == 0   # (the last write call found no site; scs_artefact_sites is not timed)
    assert res["live1"] == res["live0"] == res["live2"], (res["live0"], res["live1"], res["live2"])


def test_sites_agree_with_the_amplicon_places_of_the_same_ctx(g1_job):
    """2: the sum of NA is the sum of n_edits, and TA of every site is a searchsorted count over the places' starts and ends."""
    out, _ = g1_job
    z, p = np.load(out + "_sites.npz"), np.load(out + "_places.npz")
    rec_off = np.array([0, 120000], np.int64)
    assert int(z["na"].sum()) == int(p["n_edits"].sum()) > 10000
    lo = rec_off[p["rec"].astype(np.int64)] + p["start"].astype(np.int64)
    starts, ends = np.sort(lo), np.sort(lo + p["len"].astype(np.int64))
    x = rec_off[z["rec"].astype(np.int64)] + z["pos"].astype(np.int64)
    ta = np.searchsorted(starts, x, "right") - np.searchsorted(ends, x, "right")
    assert (ta == z["ta"].astype(np.int64)).all() and ta.min() >= 1 and ta.max() > 100


def test_dense_edits_ber_001(models, golden_inputs, tmp_path):
    """3: amplification errors at 0.01 per base (g1, 1x, seed 9; the oracle cannot run it): the reference is the restatement over the
    amplicon table the same ctx wrote, which tests/test_gpu_amplicons.py pins to the truth SAM.  Many alleles per coordinate."""
    fa = golden_inputs["g1_hiseq2500_pe"]
    out, res = _run(tmp_path / "job", prof=models["Illumina_HiSeq2500"], fa=fa, cov=1.0, layout="PE", seed=9, ber=0.01, table=True)
    names, lens, G = fasta(fa)
    tab = parse_table(open(out + ".tsv").read())
    want, arr = sites_from_table(tab, names, lens, G, brute=False)
    print("ber 0.01: sites %d, entries %d, largest NA %d, most alternate bases at a coordinate %d" % (len(arr["na"]), arr["na"].sum(), arr["na"].max(), most_alts_at_a_coordinate(arr)))
    assert most_alts_at_a_coordinate(arr) == 3 and len(arr["na"]) > 200000
    hd = header(names, lens)
    _same(open(out + ".vcf").read(), hd + want, "ber 0.01")
    want1 = "".join(ln + "\n" for ln in want.split("\n")[:-1] if ";NR=0;" not in ln)        # (the g1 test holds this equal to the restatement at min_reads 1)
    assert 0 < want1.count("\n") < want.count("\n")
    _same(open(out + "_m1.vcf").read(), hd + want1, "ber 0.01, min_reads 1")
    z = np.load(out + "_sites.npz")
    for k in KEYS:
        assert len(z[k]) == len(arr[k]) and (z[k].astype(np.int64) == arr[k]).all(), k
    assert gzip.decompress(open(out + ".vcf.gz", "rb").read()).decode() == hd + want


def test_slab_chunk_and_lds_edges(g1_job, g2_job):
    """4: slabs of 1000 (no power of two: every amplicon straddles a border, sites lie on both sides of one), of 4096 and of 200 (more
    slabs than the counting pass holds in LDS), amplicon chunks of 257, an LDS run of 16 bytes (every line straddles runs), pieces of 4099 bytes on the way to the file, and all
    of them together with BGZF write the default's bytes.  g2: slabs inside the N blocks, where no amplicon lies."""
    out, res = g1_job
    want = open(out + ".vcf", "rb").read()
    assert want.count(b"\n") > 20000
    for v in G1_VARIANTS:
        assert open(out + "_" + v["name"] + ".vcf", "rb").read() == want, v["name"]
        assert res[v["name"]] == res["plain"]
        if v.get("bgzf"):
            assert gzip.open(out + "_" + v["name"] + ".vcf.gz", "rb").read() == want, v["name"]
    z, p = np.load(out + "_sites.npz"), np.load(out + "_places.npz")
    lo = np.array([0, 120000], np.int64)[p["rec"].astype(np.int64)] + p["start"].astype(np.int64)
    assert (lo // 1000 != (lo + p["len"].astype(np.int64) - 1) // 1000).mean() > 0.5           # most amplicons straddle a border of the slabs of 1000
    x = np.array([0, 120000], np.int64)[z["rec"].astype(np.int64)] + z["pos"].astype(np.int64)
    assert len(set((x // 1000).tolist())) > 200 and ((x % 1000) == 999).any() and ((x % 1000) == 0).any()
    out2, res2 = g2_job
    assert open(out2 + "_slab1000.vcf", "rb").read() == open(out2 + ".vcf", "rb").read() and res2["slab1000"] == res2["plain"]
    p2 = np.load(out2 + "_places.npz")
    lo2 = np.array([0, 70000, 140000, 190000], np.int64)[p2["rec"].astype(np.int64)] + p2["start"].astype(np.int64)
    assert not ((lo2 >= 1000) & (lo2 < 2000)).any() and not ((lo2 >= 71000) & (lo2 < 72000)).any() and lo2.min() >= 3000


def test_bgzf(g1_job):
    """5: every BGZF block inflates (zlib, raw deflate) to its part of the plain file; the end-of-file block is last; *bytes is the size."""
    out, res = g1_job
    z = open(out + ".vcf.gz", "rb").read()
    want = open(out + ".vcf", "rb").read()
    blocks = scssim_amd.bgzf_blocks(z)
    text, at = b"", 0
    for blk, n in blocks:
        part = zlib.decompressobj(-15).decompress(blk[18:-8])
        assert len(part) == n and zlib.crc32(part) == int.from_bytes(blk[-8:-4], "little")
        text += part
        at += len(blk)
    assert at == len(z) and text == want and gzip.decompress(z) == want
    assert z[-28:] == EOF_BLOCK and blocks[-1][1] == 0 and len(blocks) >= 3
    assert res["bgzf"] == dict(sites=res["plain"]["sites"], bytes=len(z)) and len(z) < len(want)        # (repetitive text: no block is stored)


def test_cli(models, tmp_path):
    """6: `--artefacts x.vcf.gz --artefacts-min-reads 1` beside `--amplicons`: the table of the Python binding on the same job; neither
    option changes the FASTQ files."""
    fa = make_genome(str(tmp_path / "g.fa"), "14000,11000", 3)
    base = [CLI, "genreads", "-i", fa, "-m", models["Illumina_HiSeq2500"], "-c", "2", "--seed", "5"]
    for name, extra in (("off", []), ("gz", ["--artefacts", str(tmp_path / "a.vcf.gz"), "--artefacts-min-reads", "1", "--amplicons", str(tmp_path / "a.tsv")]),
                        ("vcf", ["--artefacts", str(tmp_path / "a.vcf")])):
        r = subprocess.run(base + ["-o", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    out, res = _run(tmp_path / "py", prof=models["Illumina_HiSeq2500"], fa=fa, cov=2.0, layout="PE", seed=5, table=True)
    assert gzip.open(str(tmp_path / "a.vcf.gz"), "rb").read() == open(out + "_m1.vcf", "rb").read() and 0 < res["min1"]["sites"] < res["plain"]["sites"]
    assert open(str(tmp_path / "a.vcf.gz"), "rb").read()[-28:] == EOF_BLOCK
    assert open(str(tmp_path / "a.vcf"), "rb").read() == open(out + ".vcf", "rb").read() and open(str(tmp_path / "a.tsv"), "rb").read() == open(out + ".tsv", "rb").read()
    for m in ("_1.fq", "_2.fq"):
        want = open(str(tmp_path / "off") + m, "rb").read()
        assert len(want) > 10000 and open(str(tmp_path / "gz") + m, "rb").read() == want == open(str(tmp_path / "vcf") + m, "rb").read()


_OWN = r'''
import ctypes, os
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
out = a["out"]
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
fails(lambda: s.write_artefacts(out + "_s.vcf"), SCS_EINVAL, "sharded")
fails(s.artefact_sites, SCS_EINVAL, "sharded")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=3.0, seed=41)
fails(lambda: g.write_artefacts(out + "_early.vcf"), SCS_EINVAL, "scs_allocate_reads")
fails(g.artefact_sites, SCS_EINVAL, "scs_allocate_reads")
g.create_frags(); g.amplify()
fails(lambda: g.write_artefacts(out + "_early.vcf"), SCS_EINVAL, "scs_allocate_reads")
g.allocate_reads(0)
before = scssim_amd.live_resources()
g._L.scs_write_artefacts.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
assert g._L.scs_write_artefacts(g._ctx, (out + "_flag.vcf").encode(), 2, 0, None, None) == SCS_EINVAL and b"unknown flag" in g._L.scs_last_error(g._ctx)
fails(lambda: g.write_artefacts(out + "_no_such_dir/a.vcf"), SCS_EIO, "can not open")
fails(lambda: g.write_artefacts(out + "_no_such_dir/a.vcf.gz", bgzf=True), SCS_EIO, "can not open")
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())       # after failed calls
n = ctypes.c_uint64()
g._L.scs_artefact_sites.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 8 + [ctypes.c_uint64, ctypes.c_void_p]
assert g._L.scs_artefact_sites(g._ctx, 0, *([None] * 8), 0, ctypes.byref(n)) == SCS_EOVERFLOW and n.value > 20000
total = n.value
na = (ctypes.c_uint32 * total)()
assert g._L.scs_artefact_sites(g._ctx, 0, None, None, None, None, na, None, None, None, total - 1, ctypes.byref(n)) == SCS_EOVERFLOW and n.value == total
assert g._L.scs_artefact_sites(g._ctx, 0, None, None, None, None, na, None, None, None, total, ctypes.byref(n)) == 0 and n.value == total and min(na) >= 1
assert g._L.scs_write_artefacts(g._ctx, (out + "_null.vcf").encode(), 0, 0, None, None) == 0             # *sites and *bytes may be NULL
r = g.write_artefacts(out + ".vcf")
assert r["sites"] == total
assert scssim_amd.live_resources() == before, (before, scssim_amd.live_resources())       # after calls: every buffer, stream and event of a call is gone
f1, f2 = g.yield_reads()
open(out + "_1.fq", "wb").write(f1); open(out + "_2.fq", "wb").write(f2)
assert not os.path.exists(out + "_early.vcf") and not os.path.exists(out + "_s.vcf") and not os.path.exists(out + "_flag.vcf")
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok", r["bytes"])
'''


def test_refusals_and_ownership(g1_job, oracle_bin, models, golden_inputs, tmp_path):
    """7: SCS_EINVAL before scs_allocate_reads (by name), for a sharded ctx and for an unknown flag; SCS_EIO for a path that cannot be
    opened, after which the ctx writes the table of the job that never failed and yields the oracle's FASTQ; SCS_EOVERFLOW for too
    small a cap, with the count; scs_live_resources unchanged after a call and after a failed call, zero once the contexts are gone."""
    out = str(tmp_path / "own")
    run_child(_OWN, dict(out=out, prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"]), timeout=300, ok=True)
    ref, _ = g1_job
    assert open(out + ".vcf", "rb").read() == open(ref + ".vcf", "rb").read() == open(out + "_null.vcf", "rb").read()
    orc = str(tmp_path / "orc")
    _oracle(oracle_bin, golden_inputs["g1_hiseq2500_pe"], models["Illumina_HiSeq2500"], orc, ["-c", "3", "-l", "PE"], 41)
    for m in ("_1.fq", "_2.fq"):
        assert open(out + m, "rb").read() == open(orc + m, "rb").read()
