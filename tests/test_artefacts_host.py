"""Host-side tests of the artefact table (scs_write_artefacts / scs_artefact_sites): the table's body through the functions the
kernels run (scs_site.h, by way of scs_artefact_probe) against the numpy restatement of tests/site_cases.py, on hand-made amplicon
tables and on the whole g1 table rebuilt from the oracle's dump; the header's bytes; the exported symbols; the CLI's refusals.
No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SEAMS_LIB
from amp_cases import parse_table, table_from_oracle
from site_cases import LETTERS, fasta, figures, header, probe_inputs, sites_from_table

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")

# three records of 60, 90 and 50 bases; an N block in the second
NAMES = ["20_1_60", "20_2_90", "21_1_50"]
REC_LENS = [60, 90, 50]


def _genome():
    rng = np.random.default_rng(7)
    g = rng.integers(0, 4, sum(REC_LENS)).astype(np.uint8)
    g[60 + 40:60 + 50] = 4
    return g


G = _genome()
GENOME = "".join(LETTERS[c] for c in G)
REC_OFF = [0, 60, 150]


def amp(rec, start, end, reads, *edits):
    """a row of a parsed amplicon table; edits = (record coordinate, k): the alternate base is the genome's base + k (an N: base k - 1)"""
    ed = []
    for pos, k in edits:
        ref = int(G[REC_OFF[rec] + pos])
        ed.append((pos, LETTERS[ref], LETTERS[(ref + k) % 4 if ref < 4 else k - 1]))
    return (NAMES[rec], start, end, 0, "+", reads, 0, ed)


CASES = {
    "one_amplicon_one_edit": [amp(0, 5, 40, 3, (17, 1))],
    "two_amplicons_same_edit": [amp(0, 5, 40, 3, (17, 1)), amp(0, 10, 50, 4, (17, 1)), amp(0, 0, 17, 9)],
    "two_alternate_bases_at_one_coordinate": [amp(0, 5, 40, 3, (17, 1)), amp(0, 10, 50, 4, (17, 2)), amp(0, 12, 30, 1, (17, 2)), amp(0, 16, 18, 2, (17, 3))],
    "edits_on_the_first_and_last_base_of_an_amplicon": [amp(1, 10, 30, 2, (10, 1), (29, 1)), amp(1, 0, 10, 5), amp(1, 30, 60, 7), amp(1, 29, 31, 11), amp(1, 9, 11, 13)],
    "edit_on_a_genome_N": [amp(1, 35, 70, 2, (42, 1), (49, 4)), amp(1, 20, 45, 3, (42, 2))],
    "coordinate_0_and_the_last_base_of_a_record": [amp(0, 0, 20, 1, (0, 1)), amp(0, 40, 60, 2, (59, 2)), amp(2, 30, 50, 3, (49, 3)), amp(2, 0, 9, 4, (0, 2))],
    "first_base_of_the_second_record": [amp(0, 30, 60, 6, (59, 1)), amp(1, 0, 25, 2, (0, 1)), amp(1, 0, 9, 5)],
    "reads_of_zero_everywhere": [amp(0, 5, 40, 0, (17, 1), (18, 2)), amp(0, 10, 50, 0, (17, 1))],
    "no_edit_at_all": [amp(0, 5, 40, 3), amp(1, 10, 50, 4)],
    "no_amplicon": [],
}
CASES["all_of_them_together"] = [t for k in sorted(CASES) for t in CASES[k]]


def probe(tab, **kw):
    return scssim_amd.artefact_probe(*probe_inputs(tab, NAMES, REC_LENS), REC_LENS, NAMES, GENOME, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("min_reads", [0, 1, 1000])
def test_body_equals_the_restatement(case, min_reads):
    """min_reads 0 and 1, and one above every NR (an empty body)."""
    want, arr = sites_from_table(CASES[case], NAMES, REC_LENS, G, min_reads)
    assert probe(CASES[case], min_reads=min_reads) == want
    if min_reads == 1000:
        assert want == ""


def test_the_case_table_reaches_what_it_names():
    def rows(case, **kw):
        return [ln.split("\t") for ln in probe(CASES[case], **kw).split("\n")[:-1]]
    assert rows("one_amplicon_one_edit") == [[NAMES[0], "18", ".", LETTERS[G[17]], LETTERS[(G[17] + 1) % 4], ".", ".", "NA=1;TA=1;NR=3;TR=3"]]
    assert [r[7] for r in rows("two_amplicons_same_edit")] == ["NA=2;TA=2;NR=7;TR=7"]          # [0, 17) ends on 17: it does not cover it
    two = rows("two_alternate_bases_at_one_coordinate")
    b = int(G[17])
    assert [r[1] for r in two] == ["18"] * 3 and {r[4]: r[7] for r in two} == {LETTERS[(b + 1) % 4]: "NA=1;TA=4;NR=3;TR=10", LETTERS[(b + 2) % 4]: "NA=2;TA=4;NR=5;TR=10", LETTERS[(b + 3) % 4]: "NA=1;TA=4;NR=2;TR=10"}
    assert [LETTERS.index(r[4]) for r in two] == sorted(LETTERS.index(r[4]) for r in two)
    ends = rows("edits_on_the_first_and_last_base_of_an_amplicon")
    assert [(r[1], r[7]) for r in ends] == [("11", "NA=1;TA=2;NR=2;TR=15"), ("30", "NA=1;TA=2;NR=2;TR=13")]   # start and end - 1; [0, 10) and [30, 60) cover neither
    n = rows("edit_on_a_genome_N")
    assert [r[3] for r in n] == ["N", "N", "N"] and [(r[1], r[4]) for r in n] == [("43", "A"), ("43", "C"), ("50", "T")]
    c = rows("coordinate_0_and_the_last_base_of_a_record")
    assert [(r[0], r[1]) for r in c] == [(NAMES[0], "1"), (NAMES[0], "60"), (NAMES[2], "1"), (NAMES[2], "50")]
    f = rows("first_base_of_the_second_record")
    assert [(r[0], r[1], r[7]) for r in f] == [(NAMES[0], "60", "NA=1;TA=1;NR=6;TR=6"), (NAMES[1], "1", "NA=1;TA=2;NR=2;TR=7")]
    assert [r[7] for r in rows("reads_of_zero_everywhere")] == ["NA=2;TA=2;NR=0;TR=0", "NA=1;TA=2;NR=0;TR=0"]
    assert rows("reads_of_zero_everywhere", min_reads=1) == [] and rows("no_edit_at_all") == [] and rows("no_amplicon") == []
    assert len(rows("all_of_them_together", min_reads=1)) < len(rows("all_of_them_together"))


def test_header_bytes():
    want = ("##fileformat=VCFv4.2\n##source=scssim\n##contig=<ID=20_1_60,length=60>\n##contig=<ID=20_2_90,length=90>\n##contig=<ID=21_1_50,length=50>\n"
            '##INFO=<ID=NA,Number=1,Type=Integer,Description="full amplicons that carry the alternate base">\n'
            '##INFO=<ID=TA,Number=1,Type=Integer,Description="full amplicons that cover the site">\n'
            '##INFO=<ID=NR,Number=1,Type=Integer,Description="reads allotted to the NA amplicons">\n'
            '##INFO=<ID=TR,Number=1,Type=Integer,Description="reads allotted to the TA amplicons">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    assert header(NAMES, REC_LENS) == want
    assert probe([], header=True) == want
    body = probe(CASES["one_amplicon_one_edit"])
    assert probe(CASES["one_amplicon_one_edit"], header=True) == want + body and body


@pytest.mark.parametrize("what", ["amplicon_over_the_record_end", "amplicon_beyond_the_genome", "edit_outside_its_amplicon", "edit_of_no_amplicon", "alternate_base_4", "records_do_not_add_up"])
def test_inputs_that_do_not_fit_are_refused(what):
    starts, lens, reads, edits = probe_inputs(CASES["one_amplicon_one_edit"], NAMES, REC_LENS)
    rec_lens = REC_LENS
    if what == "amplicon_over_the_record_end":
        starts, lens = [40], [30]
        edits = [(0, 45, 1)]
    elif what == "amplicon_beyond_the_genome":
        starts, lens = [190], [20]
        edits = []
    elif what == "edit_outside_its_amplicon":
        edits = [(0, 40, 1)]
    elif what == "edit_of_no_amplicon":
        edits = [(1, 17, 1)]
    elif what == "alternate_base_4":
        edits = [(0, 17, 4)]
    else:
        rec_lens = [60, 90, 49]
    with pytest.raises(ScsError) as e:
        scssim_amd.artefact_probe(starts, lens, reads, edits, rec_lens, NAMES, GENOME)
    assert e.value.code == SCS_EINVAL


def test_whole_g1_table_from_the_oracles_dump(oracle_bin, models, golden_inputs, tmp_path):
    """The table of g1 (PE, 3x, seed 41) rebuilt from the oracle's dump: the probe's body equals the restatement's at min_reads 0
    and 1, and the restatement's figures are the ones the GPU test asserts about its reference."""
    fa, orc = golden_inputs["g1_hiseq2500_pe"], str(tmp_path / "orc")
    subprocess.check_call([oracle_bin, "genreads", "-i", fa, "-m", models["Illumina_HiSeq2500"], "-o", orc, "--rng", "counter", "--seed", "41", "-t", "16", "-q",
                           "-c", "3", "-l", "PE", "--dump", orc])
    names, lens, Gc = fasta(fa)
    assert names == scssim_amd.fasta_probe(fa)[0]
    text, _, _, _ = table_from_oracle(orc, names, lens, Gc)
    tab = parse_table(text)
    want, arr = sites_from_table(tab, names, lens, Gc)
    assert figures(arr) == (22834, 42024, 2429, 44, 728, 21663)
    assert sites_from_table(tab, names, lens, Gc, brute=False)[0] == want              # the restatement's two ways of counting the cover
    inputs = probe_inputs(tab, names, lens)
    genome = "".join(LETTERS[c] for c in Gc)
    assert scssim_amd.artefact_probe(*inputs, lens, names, genome) == want
    want1, arr1 = sites_from_table(tab, names, lens, Gc, 1)
    assert want1.count("\n") == 1171 and want1 == "".join(ln + "\n" for ln in want.split("\n")[:-1] if ";NR=0;" not in ln)
    assert scssim_amd.artefact_probe(*inputs, lens, names, genome, min_reads=1) == want1


def test_both_libraries_export_the_artefact_abi():
    want = {"scs_write_artefacts", "scs_artefact_sites", "scs_artefact_kernel_time", "scs_artefact_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    assert len(scssim_amd.GenReads.KERNELS) == 8            # the table's kernels have no slot of scs_kernel_time
    for m in ("write_artefacts", "artefact_sites", "artefact_kernel_time"):
        assert callable(getattr(scssim_amd.GenReads, m))


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--artefacts with --gpus 2 or without a file name, and --artefacts-min-reads without --artefacts, end the CLI with a message
    before it touches a device (this machine may have none) or an input file (these do not exist)."""
    r = _cli(["--artefacts", "/nonexistent/a.vcf", "--gpus", "2"])
    assert r.returncode != 0 and "--artefacts needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--artefacts"])
    assert r.returncode != 0 and "artefacts" in r.stderr and "requires an argument" in r.stderr, r.stderr
    r = _cli(["--artefacts", ""])
    assert r.returncode != 0 and "--artefacts needs the name of the file" in r.stderr, r.stderr
    r = _cli(["--artefacts-min-reads", "1"])
    assert r.returncode != 0 and "--artefacts-min-reads needs --artefacts" in r.stderr, r.stderr
    r = _cli(["--artefacts", "/nonexistent/a.vcf", "--artefacts-min-reads", "-3"])
    assert r.returncode != 0 and "--artefacts-min-reads should be" in r.stderr, r.stderr
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--artefacts <string>" in h.stdout + h.stderr and "--artefacts-min-reads <int>" in h.stdout + h.stderr
