"""GPU tests of the amplicon table (scs_amplicon_places / scs_write_amplicons / scssim genreads --amplicons): the file and the
arrays equal what the restatement of tests/amp_cases.py rebuilds from the oracle's tables, byte for byte; every read of the truth
SAM of the same job lies inside the amplicon its name states, on its strand, and carries the amplicon's edits; chunk and LDS
edges; BGZF; the CLI; the refusals and the ownership of the buffers.  Each job runs in a child process under its own time limit;
the checks run here.  Run with `-m gpu`."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import seams_env
from amp_cases import codes, parse_table, table_from_oracle
from gpu_child import run_child
from gpu_readers import CIG, CLI, EOF_BLOCK, _oracle, _sam, _same, make_genome

import scssim_amd

pytestmark = pytest.mark.gpu

# one ctx, one allocated job: the table as text (plain, BGZF) and as arrays, then (sam) a yield with the truth SAM on.
# variants: [{name, env}]: the plain file again under these seams (read at every call by the seams build)
_CHILD = r'''
import numpy as np
from gpu_child import emit, job_args, leg_env, open_job, yield_leg
a = job_args()
g = open_job(a)
out = a["out"]
res = dict(plain=g.write_amplicons(out + ".tsv"), kt=g.amplicon_kernel_time(), bgzf=g.write_amplicons(out + ".tsv.gz", bgzf=True), fulls=g.stats()["full_amplicons"])
np.savez(out + "_places.npz", **g.amplicon_places())
for v in a.get("variants", []):
    with leg_env(v["env"]):
        res[v["name"]] = g.write_amplicons(out + "_" + v["name"] + ".tsv")
        if v.get("bgzf"):
            g.write_amplicons(out + "_" + v["name"] + ".tsv.gz", bgzf=True)
if a.get("sam"):
    g.set_truth_sam(out + ".sam")
    yield_leg(g, out, {})
    res["reads_written"] = g.stats()["reads_written"]
emit(res)
'''


def _run(out, env=None, timeout=300, **a):
    a["out"] = str(out)
    return a["out"], run_child(_CHILD, a, env=env, timeout=timeout)


def _genome(fa):
    names, _, _ = scssim_amd.fasta_probe(fa)
    lens = [int(ln.split("\t")[1]) for ln in open(fa + ".fai").read().split("\n") if ln]
    seq = "".join(ln for ln in open(fa).read().split("\n") if not ln.startswith(">"))
    return names, lens, codes(seq)


JOBS = {"g1_hiseq2500_pe": ("Illumina_HiSeq2500", "PE", 3.0, 41), "g3_hiseq2000_se": ("Illumina_HiSeq2000", "SE", 2.0, 23), "g2_xten_pe_nblock": ("Illumina_HiSeqXTen", "PE", 2.0, 41)}


@pytest.fixture(scope="module")
def g1_job(models, golden_inputs, tmp_path_factory):
    """g1 (PE, 3x, seed 41): the table in every form and the truth SAM of the same job.  Made once, shared, never changed."""
    model, layout, cov, seed = JOBS["g1_hiseq2500_pe"]
    return _run(tmp_path_factory.mktemp("g1") / "job", prof=models[model], fa=golden_inputs["g1_hiseq2500_pe"], cov=cov, layout=layout, seed=seed, sam=True)


@pytest.mark.parametrize("case", list(JOBS))
def test_file_and_arrays_equal_the_oracles_tables(case, g1_job, oracle_bin, models, golden_inputs, tmp_path):
    """1: the oracle in counter mode dumps its fragments, amplicons (full error lists) and read numbers; every line rebuilt from
    them equals the GPU's file byte for byte, the arrays of scs_amplicon_places equal theirs.  g1 and g2 at seed 41 hold full
    amplicons with five own errors and semi amplicons with five (checked on the CPU: 3 and 2 of 51228 in g1): both overflow pools."""
    model, layout, cov, seed = JOBS[case]
    fa = golden_inputs[case]
    out, res = g1_job if case == "g1_hiseq2500_pe" else _run(tmp_path / "job", prof=models[model], fa=fa, cov=cov, layout=layout, seed=seed)
    orc = str(tmp_path / "orc")
    _oracle(oracle_bin, fa, models[model], orc, ["-c", "%g" % cov, "-l", layout, "--dump", orc], seed)
    names, lens, G = _genome(fa)
    want, arr, most_full, most_semi = table_from_oracle(orc, names, lens, G)
    got = open(out + ".tsv").read()
    _same(got, want, case)
    assert res["plain"] == len(want) == os.path.getsize(out + ".tsv") and res["fulls"] == len(arr["rec"]) > 30000
    z = np.load(out + "_places.npz")
    assert z["rec"].dtype == np.uint32 and z["start"].dtype == np.uint64 and z["strand"].dtype == np.int8
    for k in ("rec", "start", "len", "strand", "n_edits"):
        assert (z[k].astype(np.int64) == arr[k]).all(), k
    assert set(np.unique(z["strand"])) == {-1, 1} and (arr["n_edits"] > 0).mean() > 0.3
    assert res["kt"]["launches"] >= 2 and res["kt"]["units"] == res["fulls"] and res["kt"]["ms"] > 0
    if case != "g3_hiseq2000_se":
        assert most_full > 4 and most_semi > 4              # lists of the overflow pools take part
    if case == "g2_xten_pe_nblock":
        assert len(set(z["rec"].tolist())) == 4 and (G == 4).sum() > 1000   # every record, behind its N block (no primer attaches on one: the host cases hold the errors on an N)
    if case == "g1_hiseq2500_pe":                           # (what test 6 compares its yield with)
        assert open(out + "_1.fq", "rb").read() == open(orc + "_1.fq", "rb").read() and open(out + "_2.fq", "rb").read() == open(orc + "_2.fq", "rb").read()


def check_against_sam(out, paired):
    """Every SAM record inside the amplicon its QNAME states, read 1 on its strand; the share of (read, covered edit) pairs in
    which the read shows the edit's base, over the reads whose CIGAR is one M run.  Returns (records, one-M reads, pairs, share)."""
    tab = parse_table(open(out + ".tsv").read())
    _, recs = _sam(out + ".sam")
    one_m = pairs = hit = 0
    for r in recs:
        rec, start, end, _, strand, reads, _, edits = tab[int(r[0].split("#")[0])]
        flag, pos, ops = int(r[1]), int(r[3]) - 1, CIG.findall(r[5])
        span = sum(int(n) for n, k in ops if k != "I")
        assert r[2] == rec and start <= pos and pos + span <= end and reads > 0, r[:6]
        if not paired or flag & 0x40:
            assert ("-" if flag & 0x10 else "+") == strand, r[:6]
        elif paired:
            assert ("+" if flag & 0x10 else "-") == strand, r[:6]
        if len(ops) == 1 and ops[0][1] == "M":
            one_m += 1
            for x, _, alt in edits:
                if pos <= x < pos + span:
                    pairs += 1
                    hit += r[9][x - pos] == alt
    return len(recs), one_m, pairs, hit / max(1, pairs)


def test_truth_sam_of_the_same_job_g1(g1_job):
    """2: g1.  A wrong mapping leaves the share near the model's substitution rate; a right one at one minus that rate: floor 0.9.
    (The restatement alone, on the oracle's FASTQ and tables of this job: share 1.0 over its covered edits.)"""
    out, res = g1_job
    n, one_m, pairs, share = check_against_sam(out, True)
    print("g1: records %d, one-M reads %d, (read, covered edit) pairs %d, share %.4f" % (n, one_m, pairs, share))
    assert n == res["reads_written"] > 2000 and one_m >= 0.8 * n
    assert pairs > 100 and share >= 0.9


def test_truth_sam_of_the_same_job_ber_001(models, golden_inputs, tmp_path):
    """2: amplification errors at 0.01 per base (the oracle cannot run it): most amplicons carry more than ten edits, every list goes
    through an overflow pool, and every read covers some."""
    out, res = _run(tmp_path / "job", prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"], cov=1.0, layout="PE", seed=9, ber=0.01, sam=True)
    n, one_m, pairs, share = check_against_sam(out, True)
    print("ber 0.01: records %d, one-M reads %d, (read, covered edit) pairs %d, share %.4f" % (n, one_m, pairs, share))
    tab = parse_table(open(out + ".tsv").read())
    assert np.mean([len(t[7]) for t in tab]) > 10 and max(len(t[7]) for t in tab) > 16      # (a list holds 16 errors at the most: more than 16 edits are the semi's and the full's together)
    for t in tab[::97]:
        assert [e[0] for e in t[7]] == sorted(set(e[0] for e in t[7])) and all(t[1] <= e[0] < t[2] and e[1] != e[2] for e in t[7])
    assert n == res["reads_written"] > 500 and one_m >= 0.8 * n
    assert pairs > one_m and share >= 0.9                 # (a read of 125 bases covers 2 to 3 of the about 20 edits per 1000 bases)


def test_chunk_and_lds_edges(models, tmp_path):
    """3: chunks of 257 amplicons (a workgroup and one lane), of 1, and larger than the job; an LDS run of 64 bytes, shorter than
    most lines and never a whole number of them: every setting writes the default's file, plain and (257, the LDS run) BGZF."""
    fa = make_genome(str(tmp_path / "g.fa"), "14000,11000", 3)
    variants = [dict(name="c257", env=dict(SCS_TEST_AMP_CHUNK="257"), bgzf=True), dict(name="c1", env=dict(SCS_TEST_AMP_CHUNK="1")),
                dict(name="cbig", env=dict(SCS_TEST_AMP_CHUNK="100000000")), dict(name="lds64", env=dict(SCS_TEST_AMP_LDS="64"), bgzf=True),
                dict(name="c257lds48", env=dict(SCS_TEST_AMP_CHUNK="257", SCS_TEST_AMP_LDS="48"))]
    out, res = _run(tmp_path / "job", env=seams_env(), prof=models["Illumina_HiSeq2500"], fa=fa, cov=2.0, layout="PE", seed=5, variants=variants)
    want = open(out + ".tsv", "rb").read()
    assert 1000 < res["fulls"] < 100000 and want.count(b"\n") == res["fulls"] + 1 and res["fulls"] % 257 != 0
    assert max(len(ln) for ln in want.split(b"\n")) > 64    # a line alone outgrows the small LDS run
    for v in variants:
        assert open(out + "_" + v["name"] + ".tsv", "rb").read() == want, v["name"]
        assert res[v["name"]] == len(want)
        if v.get("bgzf"):
            assert gzip.open(out + "_" + v["name"] + ".tsv.gz", "rb").read() == want, v["name"]


def test_bgzf(g1_job):
    """4: the BGZF file inflates to the plain file's bytes, block by block; its last 28 bytes are the end-of-file block; *bytes is its size."""
    out, res = g1_job
    z = open(out + ".tsv.gz", "rb").read()
    want = open(out + ".tsv", "rb").read()
    assert gzip.decompress(z) == want
    assert z[-28:] == EOF_BLOCK and res["bgzf"] == len(z) < len(want) // 2
    blocks = scssim_amd.bgzf_blocks(z)
    assert len(blocks) >= 3 and sum(n for _, n in blocks) == len(want) and blocks[-1][1] == 0


def test_cli(models, tmp_path):
    """5: `--amplicons out.tsv` and `--amplicons out.tsv.gz` beside a normal job write the same table; the job's FASTQ is the FASTQ
    of a run without the option."""
    fa = make_genome(str(tmp_path / "g.fa"), "14000,11000", 3)
    base = [CLI, "genreads", "-i", fa, "-m", models["Illumina_HiSeq2500"], "-c", "2", "--seed", "5"]
    for name, extra in (("off", []), ("tsv", ["--amplicons", str(tmp_path / "a.tsv")]), ("gz", ["--amplicons", str(tmp_path / "a.tsv.gz")])):
        r = subprocess.run(base + ["-o", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    table = open(str(tmp_path / "a.tsv"), "rb").read()
    assert len(parse_table(table.decode())) > 1000 and gzip.open(str(tmp_path / "a.tsv.gz"), "rb").read() == table
    assert open(str(tmp_path / "a.tsv.gz"), "rb").read()[-28:] == EOF_BLOCK
    for m in ("_1.fq", "_2.fq"):
        want = open(str(tmp_path / "off") + m, "rb").read()
        assert len(want) > 10000 and open(str(tmp_path / "tsv") + m, "rb").read() == want == open(str(tmp_path / "gz") + m, "rb").read()
    # the Python binding on the same job and seed: the same table
    out, _ = _run(tmp_path / "py", prof=models["Illumina_HiSeq2500"], fa=fa, cov=2.0, layout="PE", seed=5)
    assert open(out + ".tsv", "rb").read() == table


_OWN = r'''
import ctypes, os
import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
from gpu_child import fails, job_args
a = job_args()
out = a["out"]
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=a["prof"], seed=5)
fails(lambda: s.write_amplicons(out + "_s.tsv"), SCS_EINVAL, "sharded")
fails(s.amplicon_places, SCS_EINVAL, "sharded")
g = scssim_amd.GenReads(profile=a["prof"], input_fasta=a["fa"], coverage=3.0, seed=41)
fails(lambda: g.write_amplicons(out + "_early.tsv"), SCS_EINVAL, "scs_allocate_reads")
fails(g.amplicon_places, SCS_EINVAL, "scs_allocate_reads")
g.create_frags(); g.amplify()
fails(lambda: g.write_amplicons(out + "_early.tsv"), SCS_EINVAL, "scs_allocate_reads")
g.allocate_reads(0)
before = scssim_amd.live_resources()
fails(lambda: g.write_amplicons(out + "_no_such_dir/a.tsv"), SCS_EIO, "can not open")
fails(lambda: g.write_amplicons(out + "_no_such_dir/a.tsv.gz", bgzf=True), SCS_EIO, "can not open")
n = g.stats()["full_amplicons"]
buf = (ctypes.c_uint32 * n)()
g._L.scs_amplicon_places.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_uint64]
assert g._L.scs_amplicon_places(g._ctx, buf, None, None, None, None, n - 1) == SCS_EOVERFLOW
assert g._L.scs_amplicon_places(g._ctx, None, None, buf, None, None, n) == 0 and 64 <= min(buf) and max(buf) <= 2000
size = g.write_amplicons(out + ".tsv")
assert g.write_amplicons(out + ".tsv.gz", bgzf=True) > 28
after = scssim_amd.live_resources()
assert after == before, (before, after)                    # the calls' buffers, streams, events and pinned blocks are gone: they were the calls' own
f1, f2 = g.yield_reads()
open(out + "_1.fq", "wb").write(f1); open(out + "_2.fq", "wb").write(f2)
assert not os.path.exists(out + "_early.tsv") and not os.path.exists(out + "_s.tsv")
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok", size)
'''


def test_refusals_and_ownership(g1_job, models, golden_inputs, tmp_path):
    """6: SCS_EINVAL before scs_allocate_reads (by name) and for a sharded ctx; SCS_EIO for a path that cannot be opened, after which
    the ctx writes the same table and yields the same FASTQ as the job that never failed (g1_job: equal to the oracle's in test
    1); SCS_EOVERFLOW for too small a cap; the call's buffers are gone when it returns, everything once the contexts are destroyed."""
    out = str(tmp_path / "own")
    run_child(_OWN, dict(out=out, prof=models["Illumina_HiSeq2500"], fa=golden_inputs["g1_hiseq2500_pe"]), timeout=300, ok=True)
    ref, _ = g1_job
    assert open(out + ".tsv", "rb").read() == open(ref + ".tsv", "rb").read()
    for m in ("_1.fq", "_2.fq"):
        assert open(out + m, "rb").read() == open(ref + m, "rb").read()
