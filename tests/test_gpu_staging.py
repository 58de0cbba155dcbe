"""The staging kernels (scs_k_staging.hip) on their own: what the chunked FASTA parser (k_fa_kind / k_fa_keep / k_fa_scatter /
k_fa_close), the slice gather of a sharded ctx (k_fa_gather_regular) and the genome index (k_encode_bases, k_genome_bits, the two
prefix scans, k_genome_pair, the two-bit copy, k_frag_has_n) leave on the device, copied back by scs_download_genome and compared
with the reference parser and the numpy references of tests/fasta_cases.py.  SCS_TEST_FASTA_CHUNK puts the chunk borders of the
parser and the pieces of the gather where the case table needs them.  Every comparison is exact; no job needs a profile.  One child
process per group of tests (tests/staging_gpu_worker.py) does the GPU work under a time limit of its own; every check runs here."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fasta_cases as fc
from conftest import ROOT, seams_env

import scssim_amd

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "staging_gpu_worker.py")


def _run(mode, tmp_path_factory, env, timeout, *args):
    out = str(tmp_path_factory.mktemp("staging_" + mode))
    t0 = time.time()
    r = subprocess.run([sys.executable, WORKER, mode, out] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print("%s (%.1f s)" % (r.stdout.strip().splitlines()[-1], time.time() - t0))
    return np.load(os.path.join(out, mode + ".npz")), json.load(open(os.path.join(out, mode + ".json")))


@pytest.fixture(scope="module")
def parser_run(tmp_path_factory):
    return _run("parser", tmp_path_factory, seams_env(), 600)


@pytest.fixture(scope="module")
def index_run(tmp_path_factory):
    return _run("index", tmp_path_factory, dict(os.environ), 300)


@pytest.fixture(scope="module")
def hasn_run(tmp_path_factory):
    return _run("hasn", tmp_path_factory, dict(os.environ), 300)


@pytest.fixture(scope="module")
def slice_run(tmp_path_factory):
    """(line ends, piece size) -> that worker's output, run once"""
    cache = {}

    def get(eol, chunk):
        if (eol, chunk) not in cache:
            cache[eol, chunk] = _run("slice", tmp_path_factory, seams_env(), 300, eol, str(chunk))
        return cache[eol, chunk]
    return get


@pytest.fixture(scope="module")
def slice_extra_run(tmp_path_factory):
    return _run("slice_extra", tmp_path_factory, seams_env(), 300)


@pytest.fixture(scope="module")
def cap_run(tmp_path_factory):
    return _run("cap", tmp_path_factory, seams_env(), 300)


def _same_codes(got, want, what):
    assert got.dtype == np.uint8 and len(got) == len(want), "%s: %d bases, the reference has %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d codes differ, the first at %d (got %d, expected %d)" % (what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])


def _check_parsed(res, meta, key, want, what):
    m = meta[key]
    assert "error" not in m, "%s: refused: %s" % (what, m.get("error"))
    assert m["names"] == want.names and res[key + ".rec_lens"].tolist() == want.lens, (what, m["names"], res[key + ".rec_lens"].tolist())
    assert m["records"] == len(want.names) and m["genome_bases"] == m["staged_bases"] == want.total and m["slice_base"] == 0 and m["slice_len"] == want.total, (what, m)
    _same_codes(res[key + ".codes"], want.codes, what)


# ---------------------------------------------------------------- a. the parser over the table
@pytest.mark.parametrize("chunk", fc.CHUNKS)
@pytest.mark.parametrize("name", [n for n in fc.CASES if n not in fc.CR_CASES])
def test_device_parser_gives_the_reference_records_at_every_chunk_size(name, chunk, parser_run, tmp_path):
    """load_genome of every case of the table under every chunk size (unset: one chunk): records, lengths and base codes are the
    reference parser's, and the .fai left beside the file (fasta_write_fai) is byte for byte the one the host's load_fasta writes
    for the same file, which tests/test_fasta_host.py pins to the reference.  The refused case is refused by name at every size."""
    res, meta = parser_run
    key = "%s.%s" % (name, chunk)
    if name in fc.REFUSED:
        assert meta[key].get("code") == scssim_amd.SCS_EIO and fc.REFUSED[name] in meta[key]["error"], meta[key]
        return
    _check_parsed(res, meta, key, fc.parsed(name), key)
    p = tmp_path / "host.fa"
    p.write_bytes(fc.data(name))
    scssim_amd.fasta_write_index(str(p))
    host = open(str(p) + ".fai", "rb").read()
    assert meta[key]["fai"].encode("latin-1") == host == fc.fai(fc.data(name))


@pytest.mark.parametrize("chunk", fc.RAGGED_CHUNKS)
def test_device_parser_on_the_ragged_100k_file_in_several_chunks(chunk, parser_run):
    """the file of test_fasta_parsed_on_the_device_handles_ragged_text (one chunk there) in chunks of 4096 and of 65536 bytes"""
    res, meta = parser_run
    want = fc.Parsed(fc.ragged_100k())
    assert want.names == ["3_1_30011", "3_2_40000", "4_1_25000", "4_2_9"] and want.total == 95011 and len(fc.ragged_100k()) > chunk
    _check_parsed(res, meta, "ragged_100k.%s" % chunk, want, "ragged_100k at %d" % chunk)
    assert meta["ragged_100k.%s" % chunk]["fai"].encode("latin-1") == fc.fai(fc.ragged_100k())


# ---------------------------------------------------------------- b. the '\r' rule
@pytest.mark.parametrize("chunk", fc.CHUNKS)
@pytest.mark.parametrize("name", fc.CR_CASES)
def test_a_carriage_return_is_a_line_end_only_in_front_of_a_newline_or_the_end_of_the_file(name, chunk, parser_run):
    """AC\\rGT\\n, ACGT\\r\\r\\n and a final ACGT\\r: the device parser keeps every '\\r' but the one in front of a '\\n' or of the end
    of the file, as the host parser and the oracle do -- at every chunk size, the ones that cut between '\\r' and '\\n', behind a
    '\\r' in the middle of a line and in front of the file's last byte among them (tests/test_fasta_host.py checks that they do)."""
    res, meta = parser_run
    want = fc.parsed(name)
    assert 13 in want.seq or name == "cr_at_file_end"
    _check_parsed(res, meta, "%s.%s" % (name, chunk), want, "%s at chunk %s" % (name, chunk))
    assert meta["%s.%s" % (name, chunk)]["fai"].encode("latin-1") == fc.fai(fc.data(name))


# ---------------------------------------------------------------- c. the index
@pytest.mark.parametrize("total", fc.INDEX_TOTALS)
def test_genome_index_equals_numpy(total, index_run):
    """upload_genome of `total` bases -- as one record and as three whose borders are no multiples of 16; N at 0, over 60..70, at 63
    alone, at 64 alone, over the last base; both cases and bytes that are no base -- then everything index_genome made: the codes
    (k_encode_bases' aligned and unaligned paths), gc_bits / n_bits (packbits, little bit order) with word nwords zero, both prefix
    arrays (the exclusive cumulative popcount, nwords + 1 entries), gc_pair (the two interleaved), g2 (two bits per base, a code 4 as
    0).  The ctx is the same for all lengths, longest first: a shorter genome's tail and sentinel words lie where a longer one wrote."""
    res, meta = index_run
    for variant in fc.INDEX_VARIANTS:
        codes = fc.codes_of(fc.index_genome(total, variant))
        for layout, lens in (("one", [total]), ("three", fc.split_three(total))):
            key = "%d.%s.%s" % (total, variant, layout)
            assert res[key + ".rec_lens"].tolist() == lens and meta[key]["slice_len"] == total and meta[key]["slice_base"] == 0, key
            fc.check_index({k: res[key + "." + k] for k in ("codes",) + fc.INDEX_KEYS}, codes, key)


def test_download_genome_is_refused_before_a_genome_is_staged(index_run):
    _, meta = index_run
    assert meta["before_staging"]["code"] == scssim_amd.SCS_EINVAL and "no genome" in meta["before_staging"]["error"]


# ---------------------------------------------------------------- d. has_n
def test_fragments_know_whether_they_hold_an_n(hasn_run):
    """has_n of every fragment of create_frags (k_frag_has_n: two bit_rank reads of n_bits / n_pref) == any(codes[goff : goff + len] > 3)."""
    res, meta = hasn_run
    assert meta["before_frags"]["code"] == scssim_amd.SCS_EINVAL
    recs = fc.hasn_genome()
    codes = fc.codes_of(b"".join(s for _, s in recs))
    _same_codes(res["hasn.codes"], codes, "hasn genome")
    goff, ln, has_n = res["frags.goff"].astype(np.int64), res["frags.len"].astype(np.int64), res["hasn.has_n"]
    assert len(goff) == len(has_n) > 0
    want = np.array([(codes[a:a + n] > 3).any() for a, n in zip(goff, ln)], np.uint8)
    print("fragments: %d, with an N %d, without %d, ending on a multiple of 64: %d, ending on the last base: %d"
          % (len(goff), int(want.sum()), int((want == 0).sum()), int(((goff + ln) % 64 == 0).sum()), int((goff + ln == len(codes)).sum())))
    # the floors: without them the comparison below could pass on fragments that never reach the tail word or the sentinel
    assert want.sum() >= 2 and (want == 0).sum() >= 2
    assert ((goff + ln) % 64 == 0).sum() >= 1, "no fragment ends on a multiple of 64 (bit_rank reads the next word's entry with no bits below)"
    assert (goff + ln == len(codes)).sum() >= 1, "no fragment ends on the genome's last base"
    assert has_n.tolist() == want.tolist()


# ---------------------------------------------------------------- e. the slice path in one process
def _slice_ranks(res, meta, prefix, n, reference):
    """every rank of an n-shard job staged its own stretch: codes and index equal the reference's slice; the slices cover the genome"""
    covered = np.zeros(len(reference.codes), bool)
    for r in range(n):
        key = "%s.%d.%d" % (prefix, n, r)
        m = meta[key]
        assert "error" not in m, (key, m)
        assert m["names"] == reference.names and res[key + ".rec_lens"].tolist() == reference.lens, key
        base, ln = m["slice_base"], m["slice_len"]
        assert m["genome_bases"] == reference.total and m["staged_bases"] == ln and 0 < ln < reference.total, (key, m)
        fc.check_index({k: res[key + "." + k] for k in ("codes",) + fc.INDEX_KEYS}, reference.codes[base:base + ln], key)
        covered[base:base + ln] = True
    assert covered.all(), "%s, %d shards: bases %s... are in no rank's slice" % (prefix, n, np.flatnonzero(~covered)[:3])


@pytest.mark.parametrize("n", fc.SLICE_SHARDS)
@pytest.mark.parametrize("chunk", fc.SLICE_CHUNKS)
@pytest.mark.parametrize("eol", ["lf", "crlf"])
def test_every_rank_stages_its_own_slice_of_an_indexed_fasta(eol, chunk, n, slice_run):
    """ctxs with shard_count = n and no collectives on three records of 70-column lines (LF; CRLF without a final newline): pieces of
    150 bytes (two lines do not fit: one base per piece), of 256 (one line per piece, every later piece starts inside a line) and
    of 1000.  Each rank's codes and index arrays are the reference's over [slice_base, slice_base + slice_len), each stages less than
    the genome, together they cover it.  The index beside the file is the host writer's and equals the one stated from the records."""
    res, meta = slice_run(eol, chunk)
    recs = fc.slice_records()
    text = fc.fasta_text(recs, 70, b"\n" if eol == "lf" else b"\r\n", eol == "lf")
    assert meta["fai"] == fc.fai_regular(recs, 70, b"\n" if eol == "lf" else b"\r\n") == fc.fai(text).decode()
    per = chunk // (71 if eol == "lf" else 72) * 70                                  # bases whose lines fit a piece; up to two lines of them: one base per piece
    assert (per <= 140) == (chunk == 150)
    _slice_ranks(res, meta, "slice", n, fc.Parsed(text))


def test_a_line_longer_than_the_piece_buffer_is_gathered_base_by_base(slice_extra_run):
    """records on one line each, the first of 5000 bases, under pieces of 256 bytes: not one line fits, every piece is one base"""
    res, meta = slice_extra_run
    _slice_ranks(res, meta, "long", 2, fc.Parsed(fc.fasta_text(fc.long_line_records(), 5000)))


FALLBACKS = {"no_fai": "no index beside the file", "stale_fai": "an index older than the file",
             "widths_cancel_out": "lines of 71, 69, 70, 70 bases under an index that states 70 / 71: a line end among the gathered bases (*ragged), the ctx's records put back",
             "empty_record": "an empty record in the middle, named by the index: its offset is the next header's"}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_slice_path_falls_back_to_the_parser_and_slices_the_next_file_again(name, slice_extra_run):
    """Each way the slice path gives up ends with the whole genome staged by the parser: all bases resident and equal to the reference,
    the right names and lengths.  A regular indexed file loaded on the same ctx afterwards is staged as a slice again."""
    res, meta = slice_extra_run
    recs = fc.slice_records()
    with_empty = recs[:1] + [("empty_1_0", b"")] + recs[1:]
    want = fc.Parsed(fc.fasta_text(with_empty if name == "empty_record" else recs))
    regular = fc.Parsed(fc.fasta_text(recs))
    for n, r in ((2, 0), (2, 1), (3, 1)):
        key = "fall.%s.%d.%d" % (name, n, r)
        m = meta[key]
        assert "error" not in m, (key, m)
        assert m["names"] == want.names and res[key + ".rec_lens"].tolist() == want.lens, (key, m["names"])
        assert m["staged_bases"] == m["genome_bases"] == m["slice_len"] == want.total and m["slice_base"] == 0, (key, m)
        fc.check_index({k: res[key + "." + k] for k in ("codes",) + fc.INDEX_KEYS}, want.codes, key)
        if name == "no_fai":
            assert m["fai"] == fc.fai_regular(recs)
        m = meta[key + ".then_regular"]
        assert "error" not in m and m["names"] == regular.names and 0 < m["staged_bases"] == m["slice_len"] < m["genome_bases"] == regular.total, (key, m)
        fc.check_index({k: res[key + ".then_regular." + k] for k in ("codes",) + fc.INDEX_KEYS}, regular.codes[m["slice_base"]:m["slice_base"] + m["slice_len"]], key + " then regular")


def test_an_empty_last_record_is_within_what_the_index_describes(slice_extra_run):
    """an empty record at the end of the file lies where the index says (its offset is the file's size): the ranks still stage slices"""
    res, meta = slice_extra_run
    recs = fc.slice_records() + [("empty_1_0", b"")]
    want = fc.Parsed(fc.fasta_text(recs))
    assert want.lens[-1] == 0
    for n, r in ((2, 0), (2, 1), (3, 1)):
        key = "fall.empty_last_record.%d.%d" % (n, r)
        m = meta[key]
        assert "error" not in m and m["names"] == want.names and res[key + ".rec_lens"].tolist() == want.lens, (key, m)
        assert 0 < m["staged_bases"] == m["slice_len"] < m["genome_bases"] == want.total, (key, m)
        fc.check_index({k: res[key + "." + k] for k in ("codes",) + fc.INDEX_KEYS}, want.codes[m["slice_base"]:m["slice_base"] + m["slice_len"]], key)


# ---------------------------------------------------------------- f. the header list's cap
def test_more_headers_than_the_list_holds_are_refused_and_the_ctx_stays_usable(cap_run):
    """2^20 + 1 headers in 3 MB: SCS_EOVERFLOW "more than 2^20 FASTA records" (k_fa_scatter counts on and writes no entry past the
    list); the next load_genome on the same ctx stages its file."""
    res, meta = cap_run
    assert meta["many"].get("code") == scssim_amd.SCS_EOVERFLOW and "more than 2^20 FASTA records" in meta["many"]["error"], meta["many"]
    _check_parsed(res, meta, "then_lf", fc.parsed("lf"), "lf behind the refused file")
