"""CPU-only checks of the product's host logic and of the C-ABI surface (no compute calls without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SEAMS_CLI, SEAMS_LIB
import bgzf_cases

import scssim_amd

ZF = 2.2204e-16


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "scssim_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(scs_[a-z_0-9]+)\s*\(", hdr)) - {"scs_sink_fn"}
    assert len(names) >= 20 and "scs_live_resources" in names
    lib = scssim_amd.load_library()
    for n in sorted(names):
        assert hasattr(lib, n), "libscssim_hip.so does not export %s" % n


def test_host_probes_hold_no_device_resource(golden_inputs):
    """The census of the library's owning handles (scs_live_resources) in a fresh process that has only used host probes: nothing
    was allocated, so all four counters -- device bytes, streams, events, pinned bytes -- are zero."""
    import subprocess
    import sys
    code = """
import sys
sys.path.insert(0, %r)
import scssim_amd
assert scssim_amd.live_resources() == (0, 0, 0, 0)
assert len(scssim_amd.bgzf_probe(b"ACGT" * 5000)) > 0
names, total, _ = scssim_amd.fasta_probe(%r)
assert names and total > 0
assert scssim_amd.truth_record_probe("ACGTACGT", "IIIIIIII", "ACGTACGT", 0, 8).endswith("\\n")
print(scssim_amd.live_resources())
""" % (ROOT, golden_inputs["g1_hiseq2500_pe"])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "(0, 0, 0, 0)"


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(scssim_amd.ScsError) as e:
        scssim_amd.GenReads()
    assert "no HIP device" in str(e.value)


def _r(x):
    return ZF + (1 - ZF) * (x.astype(np.float64) / 4294967296.0)


@pytest.mark.parametrize("model", ["Illumina_HiSeq2500", "Illumina_HiSeqXTen", "Illumina_HiSeq2000", "Illumina_GenomeAnalyzerIIx"])
def test_thresholds_equal_the_reference_double_comparison(model, models, oracle_lib):
    """`x < T[k]` must equal the reference's `r(x) <= cdf[k]` (MyDefine.cpp:274-282) for the oracle's
    independently built CDF tables: checked at both sides of every threshold and at random draws."""
    P = scssim_amd.Profile(models[model], paired=True, isize=260)
    oracle_lib.scso_profile_load.restype = ctypes.c_void_p
    oracle_lib.scso_profile_load.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    oracle_lib.scso_profile_table.restype = ctypes.c_size_t
    oracle_lib.scso_profile_table.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.POINTER(ctypes.c_double))]
    h = oracle_lib.scso_profile_load(models[model].encode(), 1, 260)
    assert h
    rng = np.random.default_rng(5)
    for name, which in (("subs1", 0), ("subs2", 1), ("qual", 2), ("ins", 3), ("del", 4), ("isize", 5)):
        thr, cdf = P.table(name)
        p = ctypes.POINTER(ctypes.c_double)()
        n = oracle_lib.scso_profile_table(h, which, ctypes.byref(p))
        ocdf = np.ctypeslib.as_array(p, (n,)).copy()
        assert n == thr.size, name
        assert np.array_equal(ocdf, cdf), "%s: product CDF differs from the oracle's" % name
        t = thr.astype(np.uint64)
        below = np.where(t > 0, t - 1, 0)                  # largest x that must satisfy (when T > 0)
        ok_below = (_r(below) <= ocdf) | (t == 0)
        assert ok_below.all(), name
        at = np.minimum(t, 0xFFFFFFFF)                     # first x that must fail (unless clamped)
        fails = ~(_r(at) <= ocdf)
        clamped = t == 0xFFFFFFFF
        assert (fails | clamped).all(), name
        x = rng.integers(0, 1 << 32, size=thr.size, dtype=np.uint64)
        x = np.minimum(x, 0xFFFFFFFE)
        assert np.array_equal(x < t, _r(x) <= ocdf), name
    oracle_lib.scso_profile_free.argtypes = [ctypes.c_void_p]
    oracle_lib.scso_profile_free(h)
    assert P.read_length in (74, 75, 125, 151) and P.bins == P.read_length
    # rate thresholds: p <= insertRate / p < delRate/(1-insertRate) with p = x/2^32
    ti, td = P.t_insert, P.t_delete
    assert ((ti - 1) / 4294967296.0 <= P.insert_rate) and not (ti / 4294967296.0 <= P.insert_rate)
    c = P.del_rate / (1 - P.insert_rate)
    assert ((td - 1) / 4294967296.0 < c) and not (td / 4294967296.0 < c)


def test_profile_errors_are_reported(tmp_path):
    bad = tmp_path / "bad.profile"
    bad.write_text("bases: ACGT\nreadLength: 10\nbinCount: 10\nkmer: 3\n[Insert Rate]\n0.1\n")
    with pytest.raises(scssim_amd.ScsError) as e:
        scssim_amd.Profile(str(bad))
    assert "corrupted model file" in str(e.value)
    with pytest.raises(scssim_amd.ScsError):
        scssim_amd.Profile(str(tmp_path / "missing.profile"))


def test_philox_known_answers(oracle_lib):
    """Random123 known-answer vectors for Philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        c = (ctypes.c_uint32 * 4)(*ctr)
        k = (ctypes.c_uint32 * 2)(*key)
        o = (ctypes.c_uint32 * 4)()
        oracle_lib.scso_philox4x32_10(c, k, o)
        assert tuple(o) == want


def test_det_log_is_accurate(oracle_lib):
    import math
    oracle_lib.scso_det_log.restype = ctypes.c_double
    oracle_lib.scso_det_log.argtypes = [ctypes.c_double]
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.random(2000), 10 ** rng.uniform(-300, 300, 2000), [1.0, 2.0, 0.5, 1e-310]])
    for x in xs:
        got, want = oracle_lib.scso_det_log(float(x)), math.log(float(x))
        assert abs(got - want) <= 4.5e-16 * max(1.0, abs(want)), x


def _fnv(seq):
    h = 1469598103934665603
    for b in seq.upper().encode():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_det_exp_is_accurate(oracle_lib):
    oracle_lib.scso_det_exp.restype = ctypes.c_double
    oracle_lib.scso_det_exp.argtypes = [ctypes.c_double]
    rng = np.random.default_rng(5)
    x = -np.concatenate([rng.random(5000) * 256, rng.random(2000) * 10, [0.0, 256.0]])
    got = np.array([oracle_lib.scso_det_exp(float(v)) for v in x])
    assert np.max(np.abs(got - np.exp(x)) / np.exp(x)) < 4e-16
    assert oracle_lib.scso_det_exp(-300.0) == 0.0 and oracle_lib.scso_det_exp(0.0) == 1.0


def test_fasta_staging_edge_cases(tmp_path):
    """mmap/memchr FASTA staging (lib/fastahack/Fasta.cpp:45-215 semantics): names lose a chr/chrom prefix and anything
    after the first blank; CRLF, comments, blank lines, lower case, a missing final newline and empty records are handled."""
    cases = {
        "plain": (">chr20_1_12\nACGTAC\nGTACGT\n>chr20_2_12 extra words\nacgtnn\nNNACGT\n", ["20_1_12", "20_2_12"], "ACGTACGTACGT" + "ACGTNNNNACGT"),
        "crlf_nonl": (">chrom7_1_8\r\nACGT\r\nTTGA\r\n>x\r\nAC", ["7_1_8", "x"], "ACGTTTGA" + "AC"),
        "comments": (";file comment\n>a b\n;in-record comment\nAAAA\n\nCCCC\n>empty\n>b\nG\n", ["a", "empty", "b"], "AAAACCCC" + "" + "G"),
    }
    for name, (text, want_names, want_seq) in cases.items():
        p = tmp_path / (name + ".fa")
        p.write_bytes(text.encode())
        names, tot, h = scssim_amd.fasta_probe(str(p))
        assert names == want_names, name
        assert tot == len(want_seq) and h == _fnv(want_seq), name
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"ACGT\n>late\nAC\n")
    with pytest.raises(scssim_amd.ScsError):
        scssim_amd.fasta_probe(str(bad))
    with pytest.raises(scssim_amd.ScsError):
        scssim_amd.fasta_probe(str(tmp_path / "missing.fa"))


@pytest.mark.parametrize("model", ["Illumina_HiSeqXTen", "Illumina_HiSeq2500", "Illumina_GenomeAnalyzerIIx"])
def test_alias_quality_rows_hit_every_symbol_with_the_reference_count(model, models):
    """[REMAP] quality symbols are drawn by the alias method.  Of the 2^32 possible draws, the reference's comparison
    (first k with r(x) <= cdf[k], else the last symbol; MyDefine.cpp:274-282) sends w_k = T[k] - T[k-1] to symbol k; the alias
    row (K columns of 2^32 / K draws: the lowest t_j of a column to its own symbol, the rest to its alias) must send EXACTLY
    as many -- for every row of every shipped model."""
    P = scssim_amd.Profile(models[model])
    thr, _ = P.table("qual")
    al, _ = P.table("qual_alias")
    K = P.qual_k
    assert K == (16 if model == "Illumina_HiSeqXTen" else 64)
    abits = {16: 4, 64: 6, 128: 7}[K]
    C = (1 << 32) >> abits
    rows = thr.reshape(-1, 94).astype(np.int64)
    al = al.reshape(rows.shape[0], K + K // 4)
    assert rows.shape[0] == 16 * P.bins
    # the reference's counts: thresholds are clamped at 2^32 - 1, and whatever the comparison leaves falls to the last symbol
    cnt = np.maximum.accumulate(rows, axis=1)
    cnt[:, 93] = 1 << 32
    want = np.diff(np.concatenate([np.zeros((rows.shape[0], 1), np.int64), cnt], axis=1), axis=1)
    top = rows == 0xFFFFFFFF                                          # a clamped threshold stands for 2^32 - 1 or 2^32: one draw of slack
    ent = al[:, :K].astype(np.int64)
    t, alias = ent >> abits, ent & (K - 1)
    syms = np.ascontiguousarray(al[:, K:]).view(np.uint8).reshape(rows.shape[0], K).astype(np.int64)
    own_mass = np.where((t == 0) & (alias == np.arange(K)[None, :]), C, t)     # "always my own symbol" is stored as threshold 0 + self alias
    got = np.zeros_like(want)
    r = np.repeat(np.arange(rows.shape[0]), K)
    np.add.at(got, (r, syms.ravel()), own_mass.ravel())
    np.add.at(got, (r, np.take_along_axis(syms, alias, axis=1).ravel()), (C - own_mass).ravel())
    assert (got.sum(axis=1) == 1 << 32).all()
    diff = np.abs(got - want)
    assert diff.max() <= 1 and (diff[~(top | np.roll(top, 1, axis=1))] == 0).all()
    # the one-draw indel test: x < t_insert -> insertion, else x < t_indel -> deletion, deletion threshold rescaled
    assert P.t_indel == P.t_insert + (((1 << 32) - P.t_insert) * P.t_delete >> 32)


@pytest.mark.parametrize("case", ["g1_hiseq2500_pe", "g2_xten_pe_nblock", "g3_hiseq2000_se", "g4_gaiix_pe_lowprimers"])
def test_fasta_index_matches_the_reference(case, golden_inputs, tmp_path):
    """Loading a genome leaves <fasta>.fai beside it when there is none, like the reference (fastahack).  Golden = the index
    the compiled reference wrote for the same file (tests/golden/<case>.simu.fa.fai)."""
    import shutil
    fa = tmp_path / "simu.fa"
    shutil.copyfile(golden_inputs[case], fa)
    scssim_amd.fasta_write_index(str(fa))
    want = open(os.path.join(ROOT, "tests", "golden", case + ".simu.fa.fai")).read()
    assert open(str(fa) + ".fai").read() == want
    # an existing index is left alone
    open(str(fa) + ".fai", "w").write("kept\n")
    scssim_amd.fasta_write_index(str(fa))
    assert open(str(fa) + ".fai").read() == "kept\n"


def test_shard_merge_copies_byte_ranges_in_list_order(tmp_path):
    """scs_merge_fastq_shards (host only): the whole job's file = the shards' list segments slot by slot, shard by shard.
    Three shards with ragged / empty segments; PE and SE; shards removed unless asked to keep them."""
    import random
    import scssim_amd
    rnd = random.Random(4)
    for paired in (True, False):
        pre = str(tmp_path / ("m_pe" if paired else "m_se"))
        world, nslot = 3, 40
        seg = [[[bytes(rnd.getrandbits(8) for _ in range(rnd.choice([0, 0, 1, 17, 4096, 70000]))) for _ in range(nslot)] for _ in range(world)] for _ in range(2)]
        for r in range(world):
            off = [[0], [0]]
            for k in range(2 if paired else 1):
                name = pre + ".r%d%s" % (r, ("_1.fq", "_2.fq")[k] if paired else ".fq")
                with open(name, "wb") as f:
                    for sl in range(nslot):
                        f.write(seg[k][r][sl]); off[k].append(off[k][-1] + len(seg[k][r][sl]))
            if not paired:
                off[1] = [0] * (nslot + 1)
            with open(pre + ".r%d.idx" % r, "w") as f:
                f.write("# index\n")
                for i in range(nslot + 1):
                    f.write("%d\t%d\t%d\n" % (i, off[0][i], off[1][i]))
        scssim_amd.merge_fastq_shards(pre, world, paired=paired, keep_shards=not paired)
        for k in range(2 if paired else 1):
            want = b"".join(seg[k][r][sl] for sl in range(nslot) for r in range(world))
            assert open(pre + (("_1.fq", "_2.fq")[k] if paired else ".fq"), "rb").read() == want
        assert os.path.exists(pre + ".r0.idx") == (not paired)
    with pytest.raises(scssim_amd.ScsError):
        scssim_amd.merge_fastq_shards(str(tmp_path / "absent"), 2)


def test_cli_sharded_job_fails_fast_when_its_ranks_cannot_start(golden_inputs, models, tmp_path):
    """`scssim genreads --gpus 3` forks its ranks before the first HIP call.  Here (no GPU) every rank fails in scs_create; with a
    failure injected into rank 2 it dies before that.  Either way rank 0 must come back with a non-zero status at once -- not sit
    in waitpid or in a collective -- and leave no rank behind (the fork / watch / reap path; the GPU suite runs it to the end)."""
    import signal
    import subprocess
    import time
    exe = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
    for extra, env in (([], {}), (["--host-collectives", "--one-device"], {"SCS_TEST_FAIL_AT": "start", "SCS_TEST_FAIL_RANK": "2"})):
        t0 = time.time()
        p = subprocess.Popen([SEAMS_CLI if env else exe, "genreads", "-i", golden_inputs["g1_hiseq2500_pe"], "-m", models["Illumina_HiSeq2500"], "-o", str(tmp_path / "o"), "--gpus", "3", "--seed", "1"] + extra,
                             env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            _, err = p.communicate(timeout=120)
        finally:
            try:
                os.killpg(p.pid, signal.SIGKILL)                      # whatever the job left behind
            except ProcessLookupError:
                pass
        if p.returncode == 0:
            pytest.skip("a GPU is present: the job ran")
        assert time.time() - t0 < 60 and p.returncode in (1, 2, 3), err
        assert "no HIP device" in err or "failed" in err


def test_bench_starts_its_own_ranks_and_relays_their_failure(tmp_path):
    """`python bench.py --gpus 2` with no launcher on the command line: the parent (which never touches a GPU) starts the two ranks as
    children and returns non-zero when they die -- here, on the GPU-less build box, both do at once; no JSON line, no usage line."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_parity.py::test_bench_two_rank_control_flow runs the real thing")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--genome-mb", "4"],
                       env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")] and "launch with" not in r.stderr
    assert "local_rank: 1" in r.stderr or "rank      : 1" in r.stderr or "exitcode" in r.stderr      # torch.distributed.run's report of the dead ranks
    # a rank count that disagrees with the launcher's is refused by every rank
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3"], env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_bench_dump_sample_is_the_records_of_the_text_whatever_its_parts(tmp_path):
    """bench.py --dump-outputs samples a mate's FASTQ text at seeded byte offsets: the records it returns are the ones holding those
    bytes, parsed right (qualities that contain '@' and '+', reads of 50 .. L + 64 bases), and the same when the text is one file or
    part files cut anywhere between records (empty parts, a one-record part)."""
    import bench
    rng = np.random.default_rng(5)
    L = 150
    recs = []
    for i in range(3000):
        m = int(rng.integers(50, L + 65))
        recs.append((1000000000 + 3 * i, int(rng.integers(1, 9)), bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, m)]),
                     bytes(rng.integers(33, 127, m).astype(np.uint8))))
    raw = [b"@%d#%d/1\n%s\n+\n%s\n" % r for r in recs]
    starts = np.cumsum([0] + [len(r) for r in raw])

    def parts(name, cuts):
        bounds = [0] + cuts + [len(raw)]
        paths = [str(tmp_path / ("%s.p%02d" % (name, k))) for k in range(len(bounds) - 1)]
        for p, lo, hi in zip(paths, bounds, bounds[1:]):
            open(p, "wb").write(b"".join(raw[lo:hi]))
        return paths
    one = bench.sample_fastq(parts("one", []), 2048, L, np.random.default_rng(1))
    cut = bench.sample_fastq(parts("cut", [0, 1, 700, 701, 701, 2999, 3000]), 2048, L, np.random.default_rng(1))
    assert all(np.array_equal(one[k], cut[k]) for k in one)
    offs = np.sort(np.random.default_rng(1).integers(0, int(starts[-1]), 2048))
    for k, r in enumerate(np.searchsorted(starts, offs, side="right") - 1):
        amp, att, seq, qual = recs[r]
        m = len(seq)
        assert (one["amplicon"][k], one["attempt"][k], one["length"][k]) == (amp, att, m)
        assert np.array_equal(one["bases"][k, :m], ["ACGTN".index(c) for c in seq.decode()])
        assert np.array_equal(one["quals"][k, :m], np.frombuffer(qual, np.uint8) - 33.0)
        assert (one["bases"][k, m:] == -1).all() and (one["quals"][k, m:] == -1).all()


def test_bgzf_arithmetic_inflates_with_zlib():
    """The BGZF kernels' arithmetic run on the CPU (scs_bgzf_probe: the same functions "thread" by "thread" -- Huffman lengths with
    the 15-bit limit, the run-length coded header under a fixed code-length code, 256 chunks packed at prefix-sum bit offsets, 256
    chunk CRCs combined by carry-less multiplication) against zlib: every block is a well-framed BGZF block that inflates to its
    63 KB of the input with the right CRC, for FASTQ-like text, one symbol, random bytes, tiny inputs, Fibonacci frequencies
    (code lengths beyond 15 without the limit) and the stored fallback."""
    import gzip
    import zlib
    import scssim_amd
    rng = np.random.default_rng(1)
    recs = []
    for i in range(450):
        recs.append("@%d#1/1\n%s\n+\n%s\n" % (90000 + i, "".join(rng.choice(list("ACGTN"), 150, p=[.3, .2, .2, .29, .01])),
                                             "".join(chr(33 + int(x)) for x in rng.choice(41, 150, p=np.arange(1, 42) / 861.0))))
    fq = "".join(recs).encode()
    fib = [1, 1]
    while sum(fib) < 60000:
        fib.append(fib[-1] + fib[-2])
    cases = {"fastq": fq, "tiny": b"A", "two": b"AB", "one_symbol": b"N" * 70000, "random": np.random.default_rng(2).integers(0, 256, 150000, dtype=np.uint8).tobytes(), "empty": b"",
             "exact_block": fq[:64512], "block_plus_1": fq[:64513], "fibonacci": b"".join(bytes([65 + i]) * f for i, f in enumerate(fib))}
    # trees deeper than 17: every count one more than the sum of all but the latest before it (1, 2, 4, 7, 12, 20, 33, ...).  The
    # 15-bit repair must count the internal nodes below the limit too (zlib's gen_bitlen), or the code is oversubscribed
    for nsym in range(17, 24):
        cnt = [1, 2]
        while len(cnt) < nsym:
            cnt.append(cnt[-1] + cnt[-2] + 1)
        if sum(cnt) <= 64000:
            cases["skewed_%d" % nsym] = b"".join(bytes([97 + i]) * f for i, f in enumerate(cnt))
    assert sum(1 for k in cases if k.startswith("skewed")) >= 4
    for name, data in cases.items():
        for cap in (0, 64):                                         # 64: every block takes the stored path
            z = scssim_amd.bgzf_probe(data, cap)
            blocks = scssim_amd.bgzf_blocks(z)
            assert len(blocks) == (len(data) + 64511) // 64512, name
            assert b"".join(zlib.decompress(b, 31) for b, _ in blocks) == data, (name, cap)      # wbits 31: gzip framing, CRC-32 and ISIZE checked
            assert [i for _, i in blocks] == [min(64512, len(data) - o) for o in range(0, len(data), 64512)]
            if data:
                assert gzip.decompress(z) == data
    assert len(scssim_amd.bgzf_probe(fq)) < 0.6 * len(fq)             # 2 bits per base + the qualities' entropy (5 bits here)


@pytest.mark.parametrize("name", list(bgzf_cases.CASES))
def test_bgzf_cases_reach_the_branches_they_name(name):
    """The shared BGZF case table (tests/bgzf_cases.py; the GPU test runs the device over it) under the host emulation: every
    case reaches the branch it is there for -- per block stored (byte 18 = 0x01) or dynamic Huffman (low bits 0b101), and of the
    stored ones which reason (incompressible, or over the LDS cap: it deflates once the cap is lifted); the repair cases have an
    unrestricted Huffman tree deeper than 15 over block 0's histogram (end-of-block count included); the LDS-cap cases lie within
    64 bytes of BGZF_LDS_OUT on their side; `mixed` has all three kinds of block and all four residues of the block offsets mod 4
    -- and passes the zlib checks of test_bgzf_arithmetic_inflates_with_zlib.  A case that a later change of scs_bgzf.h moves off
    its branch fails here."""
    import gzip
    import zlib
    bc = bgzf_cases
    data, (_, want, reach) = bc.data(name), bc.CASES[name]
    z = scssim_amd.bgzf_probe(data)
    blocks = scssim_amd.bgzf_blocks(z)
    assert len(blocks) == (len(data) + bc.BGZF_IN - 1) // bc.BGZF_IN
    assert b"".join(zlib.decompress(b, 31) for b, _ in blocks) == data
    assert [i for _, i in blocks] == bc.cut(data)
    if data:
        assert gzip.decompress(z) == data
    kinds = bc.block_kinds(data)
    if want is not None:
        assert len(kinds) == len(want) and all(w is None or w == k for w, k in zip(want, kinds)), (reach, kinds[:16])
    if name in bc.DEEP:
        assert len(blocks) == 1 and bc.huffman_depth(bc.block_hist(data)) > 15, reach
    cb = len(blocks[0][0]) - 26 if blocks else 0                      # the first block's deflate data
    if name == "lds_cap_below":
        assert bc.BGZF_LDS_OUT - bc.CAP_WINDOW < cb < bc.BGZF_LDS_OUT and len(data) == bc.BGZF_IN, cb
    if name == "lds_cap_exact":
        assert cb == bc.BGZF_LDS_OUT and len(data) == bc.BGZF_IN, cb
    if name == "lds_cap_above":
        free = len(scssim_amd.bgzf_probe(data, 1 << 30)) - 26           # what it would deflate to without the cap
        assert bc.BGZF_LDS_OUT < free < bc.BGZF_LDS_OUT + bc.CAP_WINDOW and len(data) == bc.BGZF_IN, free
    if name == "mixed":
        offs = np.cumsum([0] + [len(b) for b, _ in blocks])[:-1]
        assert len(blocks) >= 12 and set(kinds) == {"deflated", "stored_incompressible", "stored_cap"} and set(int(o) % 4 for o in offs) == {0, 1, 2, 3}
        assert all(len(data[i * bc.BGZF_IN:(i + 1) * bc.BGZF_IN]) == bc.BGZF_IN for i in range(len(blocks)))
    if name.startswith("len_"):
        assert len(data) == int(name[4:]) < 256
    if name == "one_symbol":
        assert len(set(data)) == 1 and len(blocks) == 2
    if name.startswith("all_256"):
        assert len(set(data)) == 256
    if name == "all_256_flat":
        assert len(set(np.bincount(np.frombuffer(data, np.uint8)))) == 1 and len(data) == bc.BGZF_IN
    if name == "two_symbols_equal":
        assert sorted(np.bincount(np.frombuffer(data, np.uint8))[[65, 66]]) == [len(data) // 2] * 2
    if name == "ties_with_eob":
        assert int((np.bincount(np.frombuffer(data, np.uint8)) == 1).sum()) >= 100
    if name == "big_text":
        assert len(blocks) > 300


def test_part_files_are_one_logical_file_for_both_merges(tmp_path):
    """A sink with K writers leaves K part files per mate (<base>.p00_1.fq ...) + <base>.parts; their concatenation is the
    single file.  Host only: scs_merge_fastq_parts rebuilds the reference's two files from them, and scs_merge_fastq_shards
    reads a shard that was written in parts (segments straddling part boundaries, empty parts) like a plain one."""
    import random
    import scssim_amd
    rnd = random.Random(11)
    blob = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    # (1) parts -> the two files
    for paired in (True, False):
        pre = str(tmp_path / ("p_pe" if paired else "p_se"))
        K = 5
        data = [[blob(rnd.choice([0, 1, 33, 5000, 70001])) for _ in range(K)] for _ in range(2 if paired else 1)]
        paths = scssim_amd.part_paths(pre, K, paired)
        for m, files in enumerate(paths):
            for k, f in enumerate(files):
                open(f, "wb").write(data[m][k])
        with open(pre + ".parts", "w") as f:
            f.write("# parts\n")
            for k in range(K):
                f.write("%d\t%d\t%d\n" % (k, len(data[0][k]), len(data[1][k]) if paired else 0))
        scssim_amd.merge_fastq_parts(pre, paired=paired, keep_parts=not paired)
        for m, files in enumerate(scssim_amd.part_paths(pre, 1, paired)):
            assert open(files[0], "rb").read() == b"".join(data[m])
        assert os.path.exists(paths[0][0]) == (not paired) and os.path.exists(pre + ".parts") == (not paired)
    # (2) shards written in parts
    pre = str(tmp_path / "sp"); world, nslot = 2, 40
    seg = [[[blob(rnd.choice([0, 3, 900, 40000])) for _ in range(nslot)] for _ in range(world)] for _ in range(2)]
    for r in range(world):
        K = 3 + r
        off = [[0], [0]]
        for m in range(2):
            whole = b"".join(seg[m][r])
            for sl in range(nslot):
                off[m].append(off[m][-1] + len(seg[m][r][sl]))
            cuts = sorted(rnd.randrange(0, len(whole) + 1) for _ in range(K - 1))
            cuts = [0] + cuts + [len(whole)]
            if r == 1:
                cuts[1] = 0                                           # an empty first part
            for k, f in enumerate(scssim_amd.part_paths(pre + ".r%d" % r, K, True)[m]):
                open(f, "wb").write(whole[cuts[k]:cuts[k + 1]])
            off[m].append(cuts)
        with open(pre + ".r%d.parts" % r, "w") as f:
            for k in range(K):
                f.write("%d\t%d\t%d\n" % (k, off[0][-1][k + 1] - off[0][-1][k], off[1][-1][k + 1] - off[1][-1][k]))
        with open(pre + ".r%d.idx" % r, "w") as f:
            for i in range(nslot + 1):
                f.write("%d\t%d\t%d\n" % (i, off[0][i], off[1][i]))
    scssim_amd.merge_fastq_shards(pre, world, paired=True)
    for m, suffix in enumerate(("_1.fq", "_2.fq")):
        assert open(pre + suffix, "rb").read() == b"".join(seg[m][r][sl] for sl in range(nslot) for r in range(world))
    assert not os.path.exists(pre + ".r0.p00_1.fq") and not os.path.exists(pre + ".r1.parts")
    # a part whose size disagrees with the index is refused, not copied
    pre = str(tmp_path / "bad")
    for f in scssim_amd.part_paths(pre, 2, False)[0]:
        open(f, "wb").write(b"xx")
    open(pre + ".parts", "w").write("0\t2\t0\n1\t3\t0\n")
    with pytest.raises(scssim_amd.ScsError):
        scssim_amd.merge_fastq_parts(pre, paired=False)


def test_two_word_stream_step_is_sound():
    """[REMAP] stream B of a read advances one xoshiro128 step per output position and takes TWO words from it: the xoshiro128++
    output (scrambler on state words s0, s3) for the substitution draw and the same scrambler on the other two words (s1, s2)
    for the quality draw (scs_common.h Xoshiro::next2, mirrored in the oracle).  A numpy restatement over 4096 independent
    streams x 512 steps: both words uniform (chi-square over their top byte), uncorrelated with each other within a step and
    across consecutive steps, and the first word is bit for bit the published generator's output."""
    rng = np.random.default_rng(5)
    s = [rng.integers(1, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32) for _ in range(4)]

    def rotl(x, k):
        return ((x << np.uint32(k)) | (x >> np.uint32(32 - k))).astype(np.uint32)

    def reference_next(st):                                # xoshiro128++ 1.0 (Blackman & Vigna), one stream, python ints
        s0, s1, s2, s3 = st
        m = 0xFFFFFFFF
        r = ((((s0 + s3) & m) << 7 | ((s0 + s3) & m) >> 25) + s0) & m
        t = (s1 << 9) & m
        s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t; s3 = ((s3 << 11) | (s3 >> 21)) & m
        return r, [s0, s1, s2, s3]

    ref_state = [int(w[0]) for w in s]
    A, Bw = [], []
    for step in range(512):
        a = (rotl(s[0] + s[3], 7) + s[0]).astype(np.uint32)
        b = (rotl(s[1] + s[2], 7) + s[1]).astype(np.uint32)
        t = (s[1] << np.uint32(9)).astype(np.uint32)
        s[2] = s[2] ^ s[0]; s[3] = s[3] ^ s[1]; s[1] = s[1] ^ s[2]; s[0] = s[0] ^ s[3]
        s[2] = s[2] ^ t; s[3] = rotl(s[3], 11)
        A.append(a); Bw.append(b)
        if step < 64:
            r, ref_state = reference_next(ref_state)
            assert int(a[0]) == r
    A = np.array(A, dtype=np.float64) / 2.0 ** 32
    Bn = np.array(Bw, dtype=np.float64) / 2.0 ** 32
    n = A.size
    for x in (A, Bn):
        assert abs(x.mean() - 0.5) < 4 * np.sqrt(1.0 / 12 / n)
        counts = np.bincount((x.ravel() * 256).astype(np.int64), minlength=256)
        chi2 = ((counts - n / 256.0) ** 2 / (n / 256.0)).sum()
        assert chi2 < 255 + 5 * np.sqrt(2 * 255), chi2
    def corr(x, y):
        return float(np.corrcoef(x.ravel(), y.ravel())[0, 1])
    lim = 5.0 / np.sqrt(n)
    assert abs(corr(A, Bn)) < lim
    assert abs(corr(Bn[:-1], A[1:])) < lim and abs(corr(A[:-1], Bn[1:])) < lim and abs(corr(Bn[:-1], Bn[1:])) < lim


def test_the_product_library_reads_no_test_seam():
    """The knobs the tests turn (scssim_amd/csrc/scs_seams.h) exist in libscssim_hip_seams.so only: with every one of them set in the
    environment the product library still answers "unset" -- its seam_env is a function that returns NULL, no getenv behind it --
    while the seams build hands the values through.  Both builds export the same C ABI."""
    import subprocess
    import sys
    knobs = re.findall(r"SCS_[A-Z0-9_]+", open(os.path.join(ROOT, "scssim_amd", "csrc", "scs_seams.h")).read().split("#pragma once")[0])
    knobs = sorted(set(k for k in knobs if k not in ("SCS_HD",)))
    assert "SCS_TEST_BATCH_SHIFT" in knobs and "SCS_TEST_QK" in knobs and len(knobs) >= 12
    code = """
import ctypes, sys
L = ctypes.CDLL(sys.argv[1]); L.scs_test_seam.restype = ctypes.c_char_p; L.scs_test_seam.argtypes = [ctypes.c_char_p]
print(",".join("%s=%s" % (k, (L.scs_test_seam(k.encode()) or b"<unset>").decode()) for k in sys.argv[2:]))
"""
    env = dict(os.environ, **{k: "7" for k in knobs})
    out = {}
    for name, lib in (("product", scssim_amd.lib_path() if not os.environ.get("SCSSIM_HIP_LIB") else os.path.join(ROOT, "scssim_amd", "libscssim_hip.so")), ("seams", SEAMS_LIB)):
        r = subprocess.run([sys.executable, "-c", code, lib] + knobs, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = dict(kv.split("=") for kv in r.stdout.strip().split(","))
    assert all(v == "<unset>" for v in out["product"].values()), out["product"]
    assert all(v == "7" for v in out["seams"].values()), out["seams"]
    nm = lambda lib: set(l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout.splitlines() if " T " in l and "scs_" in l)
    assert nm(SEAMS_LIB) == nm(os.path.join(ROOT, "scssim_amd", "libscssim_hip.so")) and "scs_test_seam" in nm(SEAMS_LIB)
    # and no getenv of a seam is left in the library's sources outside scs_seams_on.cpp
    for fn in os.listdir(os.path.join(ROOT, "scssim_amd", "csrc")):
        if fn.endswith((".cpp", ".hip", ".h")) and fn != "scs_seams_on.cpp":
            src = open(os.path.join(ROOT, "scssim_amd", "csrc", fn)).read()
            assert not re.search(r'(?<![_a-z])getenv\("SCS_(TEST|READS|ERRS|ATTACH|VMM|NO_VMM|HOST_FASTA|STAGE|EV_)', src), fn


def test_gz_input_is_inflated_beside_itself_whatever_its_name(golden_inputs, tmp_path):
    """Genome::loadRefSeq inflates "<name>.gz" with `gzip -cd <name>.gz > <name>` through system() (lib/genome/Genome.cpp:183-187).
    Same behaviour here, with the path as ONE shell word: a directory with a blank and a quote in its name works (and runs nothing)."""
    import gzip
    import shutil
    d = tmp_path / "my dir; it's $(touch pwned)"
    d.mkdir()
    plain = str(d / "simu.fa")
    shutil.copy(golden_inputs["g2_xten_pe_nblock"], plain)
    want = scssim_amd.fasta_probe(plain)
    os.remove(plain); os.remove(plain + ".fai") if os.path.exists(plain + ".fai") else None
    with open(golden_inputs["g2_xten_pe_nblock"], "rb") as f, gzip.open(plain + ".gz", "wb") as g:
        g.write(f.read())
    got = scssim_amd.fasta_probe(plain + ".gz")
    assert got == want and os.path.exists(plain), "the plain file is left beside the .gz, as the reference leaves it"
    assert not os.path.exists("pwned") and not (tmp_path / "pwned").exists()
    with pytest.raises(Exception):
        scssim_amd.fasta_probe(str(d / "absent.fa.gz"))


# (writers, regions) of a sink: regions a multiple of writers, and one pair where it is not
_PLAN_SINKS = [(w, r) for r in (1, 3, 4, 12, 24) for w in (1, 3, 4, 12) if r % w == 0] + [(4, 6)]


@pytest.mark.parametrize("writers,regions", _PLAN_SINKS)
def test_batch_plan_order(writers, regions):
    """The order a yield makes its batches in (plan_batches through scs_batch_plan_probe): a permutation; region r owns the contiguous
    batches [nbatch r / regions, nbatch (r + 1) / regions) and gets them in ascending order; a generation (`writers` regions) is over
    before the next begins; within one, every round visits the regions that still have batches, in ascending order."""
    shift, per = 6, 64
    for nbatch_want in sorted({0, 1, regions - 1, regions, 10 * regions + 3}):
        for pairs in sorted({max(0, per * nbatch_want - 5), 1 if nbatch_want == 1 else per * nbatch_want}):
            batch, order, region_of = scssim_amd.batch_plan_probe(pairs, 150, True, writers, regions, shift)
            nbatch = len(order)
            assert batch == min(max(pairs, 1), per) and nbatch == (pairs + batch - 1) // batch == len(region_of)
            assert sorted(order) == list(range(nbatch))
            own = {r: [b for b, q in zip(order, region_of) if q == r] for r in range(regions)}
            assert set(region_of) <= set(range(regions))
            for r in range(regions):                                  # (an empty region: nothing)
                assert own[r] == list(range(nbatch * r // regions, nbatch * (r + 1) // regions)), (pairs, r)
            gens = [q // writers for q in region_of]
            assert gens == sorted(gens)
            for g in range((regions + writers - 1) // writers):
                seq = [q for q in region_of if q // writers == g]
                left = {r: len(own[r]) for r in range(g * writers, min(regions, (g + 1) * writers))}
                while seq:
                    live = [r for r in sorted(left) if left[r]]
                    assert live and seq[:len(live)] == live, (pairs, g)
                    seq = seq[len(live):]
                    for r in live:
                        left[r] -= 1
                assert not any(left.values())


def test_batch_plan_sizes():
    """Pairs per batch, worked out by hand from the rules: 2^23 with the text staying in HBM; 2^19 towards a sink with at most 4 writers;
    else 2^18 doubled while two batches fit a part file (2 batch <= P / (2 regions)) up to 2^21, then halved down to 2^18 while
    (writers + 2) slots of batch (4 L + 64) bytes exceed 24 GiB; a batch shift overrides all of it; never more than the pairs there are."""
    size = lambda *a: scssim_amd.batch_plan_probe(*a)[0]
    assert size(10 ** 9, 150, False, 1, 1, 0) == 1 << 23
    assert size(10 ** 9, 150, True, 3, 3, 0) == 1 << 19
    assert size(8 * 10 ** 8, 150, True, 12, 12, 0) == 1 << 21     # 8e8 / 24 = 33.3 M >= 2^22; 14 x 2^21 x 664 B = 19.5 GB
    assert size(4 * 10 ** 9, 150, True, 64, 64, 0) == 1 << 19     # 66 x 2^21 x 664 B = 91.9 GB, x 2^20 = 46 GB, x 2^19 = 23 GB < 24 GiB
    assert size(5 * 10 ** 6, 150, True, 12, 12, 0) == 1 << 18     # 5e6 / 24 = 208 k < 2^19: the floor
    for sink in (False, True):
        batch, order, region_of = scssim_amd.batch_plan_probe(1000, 150, sink, 1, 1, 6)
        assert batch == 64 and order == list(range(16)) and region_of == [0] * 16
        assert 1000 - (len(order) - 1) * batch == 40                  # what is left for the last batch, from the probe's batch and nbatch
    assert scssim_amd.batch_plan_probe(0, 150, False)[1:] == ([], []) and scssim_amd.batch_plan_probe(1, 150, True, 4, 4)[0] == 1


def test_output_file_sanitizer_tool_builds_and_passes(tmp_path):
    """tools/outfile_host_check.py: the output file of the truth SAM / BAM and of the tables (scs_outfile.h) as a stand-alone CPU
    program under AddressSanitizer and UndefinedBehaviorSanitizer -- header, buffers and end-of-file block, plain and BGZF, read back
    and inflated; the error texts.  Skips only where the host compiler has no sanitizer runtimes."""
    import subprocess
    import sys
    probe = tmp_path / "p.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "p")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "p")]).returncode != 0:
        pytest.skip("the host compiler lacks the AddressSanitizer / UndefinedBehaviorSanitizer runtimes: " + r.stderr[-300:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "outfile_host_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 wrong" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
