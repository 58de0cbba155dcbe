"""The host FASTA parser and its index writer over the case table of tests/fasta_cases.py, against the table's reference parser; and
the table itself: every case is as small as it says, and the table puts a chunk border of every kind where the GPU tests
(tests/test_gpu_staging.py) need one.  No GPU."""
import numpy as np
import pytest

import fasta_cases as fc

import scssim_amd


def _write(tmp_path, name):
    p = tmp_path / (name + ".fa")
    p.write_bytes(fc.data(name))
    return str(p)


def test_cases_are_small_and_say_what_they_are_for():
    for name, (_, why) in fc.CASES.items():
        assert why and len(fc.data(name)) <= fc.SIZE_CAP.get(name, 2048), name
    assert set(fc.CR_CASES) <= set(fc.CASES) and set(fc.REFUSED) <= set(fc.CASES)
    every = set().union(*[set(fc.data(n)) for n in ("all_bytes",)])
    assert every == set(range(1, 256))
    assert b"AC\rGT\n" in fc.data("cr_inside_line") and b"ACGT\r\r\n" in fc.data("cr_twice_at_line_end") and fc.data("cr_at_file_end").endswith(b"ACGT\r")


def test_reference_parser_on_cases_worked_by_hand():
    p = fc.Parsed(b";c\n\r\n>chr2_1_9 words\r\nAC\rGT\r\n;x\nacgN\n>chrom3\n>e")
    assert p.names == ["2_1_9", "3", "e"] and p.lens == [9, 0, 0] and p.seq == b"AC\rGTacgN"
    assert p.codes.tolist() == [0, 1, 4, 2, 3, 0, 1, 2, 4]
    assert fc.Parsed(b">a\nACGT\r").seq == b"ACGT" and fc.Parsed(b">a\nACGT\r\r\n").seq == b"ACGT\r" and fc.Parsed(b">a\nAC\rGT\n").lens == [5]
    assert fc.fnv1a_upper(b"") == 1469598103934665603 and fc.fnv1a_upper(b"a") == fc.fnv1a_upper(b"A") == 0x44BD6AD473CD62A6
    with pytest.raises(fc.Refused):
        fc.parse(b"\n;c\nA\n>late\n")
    assert fc.fai(b">chr1 d\r\n;c\r\nACGT\r\nAC\r\n>e\n>f\n\nAC") == b"chr1\t6\t13\t4\t6\n" b"e\t0\t26\t0\t0\n" b"f\t2\t29\t0\t1\n"


@pytest.mark.parametrize("name", [n for n in fc.CASES if n not in fc.REFUSED])
def test_host_parser_gives_the_reference_records(name, tmp_path):
    """scs_fasta_probe (load_fasta, "the host parser's view") over the whole table: names, total and checksum are the reference's"""
    want = fc.parsed(name)
    names, total, checksum = scssim_amd.fasta_probe(_write(tmp_path, name))
    assert names == want.names and total == want.total
    assert checksum == want.checksum


@pytest.mark.parametrize("name", [n for n in fc.CASES if n not in fc.REFUSED])
def test_host_index_is_the_one_the_reference_states(name, tmp_path):
    """fasta_write_index leaves the .fai the table's reference states from the file's bytes: first word of the name, length, offset of
    the first line behind the header and any comment lines, that line's bases and bytes"""
    path = _write(tmp_path, name)
    scssim_amd.fasta_write_index(path)
    assert open(path + ".fai", "rb").read() == fc.fai(fc.data(name))


@pytest.mark.parametrize("name", sorted(fc.REFUSED))
def test_refused_cases_are_refused_by_name(name, tmp_path):
    with pytest.raises(fc.Refused):
        fc.parse(fc.data(name))
    path = _write(tmp_path, name)
    for call in (scssim_amd.fasta_probe, scssim_amd.fasta_write_index):
        with pytest.raises(scssim_amd.ScsError) as e:
            call(path)
        assert e.value.code == scssim_amd.SCS_EIO and fc.REFUSED[name] in str(e.value)


def test_table_puts_every_kind_of_border_at_chunk_1_and_at_a_chunk_of_several_bytes():
    """Every kind of chunk border the device parser's carried state has to survive is in the table: at one byte per chunk, and -- so that
    the chunk in front of the border holds a line start or a look-ahead of its own -- at some size of 2, 3, 5, 7."""
    one = fc.kinds_reached(1)
    assert all(one[k] for k in fc.BORDER_KINDS), {k: v for k, v in one.items() if not v}
    small = {c: fc.kinds_reached(c) for c in fc.SMALL_CHUNKS}
    for k in fc.BORDER_KINDS:
        assert any(small[c][k] for c in fc.SMALL_CHUNKS), k
    # the '\r' cases: a chunk of several bytes ends between the second '\r' of ACGT\r\r\n and its '\n', one right behind the '\r' of AC\rGT
    assert any(fc.kinds_reached(c, ("cr_twice_at_line_end",))["between_cr_and_lf"] for c in fc.SMALL_CHUNKS)
    d = fc.data("cr_inside_line")
    assert any((d.index(b"\r") + 1) % c == 0 for c in fc.SMALL_CHUNKS)
    d = fc.data("cr_at_file_end")
    assert any((len(d) - 1) % c == 0 for c in fc.CHUNKS if c), "no chunk size puts the final '\\r' into a chunk of its own"


def test_the_chunk_seam_the_gpu_tests_turn_is_the_one_staging_reads():
    """tests/staging_gpu_worker.py sets SCS_TEST_FASTA_CHUNK; a knob of another name would leave every file in one chunk and the
    table's borders untested without a test failing.  The name is listed in scs_seams.h and read, through seam_env, by the one function
    that sizes the parser's chunks and the slice path's pieces."""
    import os
    import re
    from conftest import ROOT
    csrc = os.path.join(ROOT, "scssim_amd", "csrc")
    worker = open(os.path.join(ROOT, "tests", "staging_gpu_worker.py")).read()
    knobs = set(re.findall(r'"(SCS_TEST_[A-Z_]+)"', worker))
    assert knobs == {"SCS_TEST_FASTA_CHUNK"}
    assert "SCS_TEST_FASTA_CHUNK" in open(os.path.join(csrc, "scs_seams.h")).read().split("#pragma once")[0]
    stage = open(os.path.join(csrc, "scs_stage.cpp")).read()
    assert len(re.findall(r'seam_env\("SCS_TEST_FASTA_CHUNK"\)', stage)) == 1
    assert len(re.findall(r"const size_t CH = fasta_chunk_bytes\(\);", stage)) == 2 and "64u << 20; const" not in stage


def test_index_references_on_words_worked_by_hand():
    codes = np.array([1, 2, 4, 0, 3] + [0] * 59 + [2], np.uint8)                       # 65 bases: G/C at 0, 1 and 64, an N at 2
    r = fc.index_reference(codes)
    assert r["gc_bits"].tolist() == [3, 1, 0] and r["n_bits"].tolist() == [4, 0, 0]
    assert r["gc_pref"].tolist() == [0, 2, 3] and r["n_pref"].tolist() == [0, 1, 1]
    assert r["gc_pair"].tolist() == [[3, 0], [1, 2], [0, 3]]
    assert r["g2"].tolist() == [1 | 2 << 2 | 0 << 4 | 0 << 6 | 3 << 8, 0, 0, 0, 2, 0, 0, 0]
    for total in fc.INDEX_TOTALS:
        lens = fc.split_three(total)
        assert sum(lens) == total and all(n > 0 for n in lens) and (len(lens) == 1 or (lens[0] % 16 and (lens[0] + lens[1]) % 16))
        for v in fc.INDEX_VARIANTS:
            g = fc.index_genome(total, v)
            assert len(g) == total and fc.codes_of(g)[-1] == 4 and fc.codes_of(g)[0] == 4
    g = fc.codes_of(fc.index_genome(129, "n_63_alone"))
    assert g[63] == 4 and (g[58:63] < 4).all() and (g[64:70] < 4).all()
    g = fc.codes_of(fc.index_genome(129, "n_64_alone"))
    assert g[64] == 4 and (g[58:64] < 4).all() and (g[65:70] < 4).all()
    assert (fc.codes_of(fc.index_genome(129, "n_60_to_70"))[60:70] == 4).all()
