"""Host-side tests of the artefact table on the original reference (scs_write_artefacts_ref / scs_artefact_ref_sites): the table's
body through the functions the kernels run (scs_site_ref.h, by way of scs_artefact_ref_probe) against the per-base numpy restatement
of tests/site_ref_cases.py, byte for byte, on hand-made haplotypes, amplicons and lift tables; slab borders; the conservation laws;
broken inputs; the header's bytes; the exported symbols; the CLI's refusals.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SEAMS_LIB
from site_ref_cases import LETTERS, NOTE, Segs, conservation, header, pieces_of, restate_entries

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")


class World:
    """Reference records and the haplotype records staged from them.  haps: per staged record a list of ("R", ref_rec, ref_start,
    ref_end) / ("I", length) stretches; subst: (staged record, record coordinate) whose base is replaced (a planted substitution:
    it does not break a segment)."""
    def __init__(self, ref_lens, haps, subst=(), seed=5):
        rng = np.random.default_rng(seed)
        self.ref_lens, self.ref_names = list(ref_lens), ["chr%d" % (i + 1) for i in range(len(ref_lens))]
        ref = [rng.integers(0, 4, l).astype(np.uint8) for l in ref_lens]
        rows, seqs, self.hap_lens, at = [], [], [], 0
        for h in haps:
            rec0, anchor = at, 0
            for p in h:
                if p[0] == "R":
                    rows.append((at, p[3] - p[2], p[2], p[1], 0))
                    seqs.append(ref[p[1]][p[2]:p[3]])
                    at += p[3] - p[2]
                    anchor = p[3]
                else:
                    rows.append((at, p[1], anchor, h[0][1] if h[0][0] == "R" else 0, 1))
                    seqs.append(rng.integers(0, 4, p[1]).astype(np.uint8))
                    at += p[1]
            self.hap_lens.append(at - rec0)
        self.G = np.concatenate(seqs)
        self.hap_off = np.concatenate([[0], np.cumsum(self.hap_lens)]).astype(np.int64)
        for r, pos in subst:
            self.G[self.hap_off[r] + pos] = (self.G[self.hap_off[r] + pos] + 2) % 4
        self.segs = Segs(rows)
        self.genome = "".join(LETTERS[c] for c in self.G)

    def inputs(self, amps):
        """amps: (staged record, start, end, reads, [(record coordinate, k), ...]); the alternate base is the staged base + k"""
        starts = [int(self.hap_off[a[0]]) + a[1] for a in amps]
        lens = [a[2] - a[1] for a in amps]
        reads = [a[3] for a in amps]
        edits = [(i, int(self.hap_off[a[0]]) + pos, int(self.G[self.hap_off[a[0]] + pos] + k) % 4) for i, a in enumerate(amps) for pos, k in a[4]]
        return starts, lens, reads, edits

    def probe(self, amps, **kw):
        return scssim_amd.artefact_ref_probe(*self.inputs(amps), self.hap_lens, self.genome, self.segs, self.ref_lens, self.ref_names, **kw)

    def want(self, amps, min_reads=0):
        return restate_entries(*self.inputs(amps), self.G, self.segs, self.ref_lens, self.ref_names, min_reads)


ONE = World([200], [[("R", 0, 0, 200)]])
TWO = World([200], [[("R", 0, 0, 200)], [("R", 0, 0, 200)]], subst=[(1, 100)])
TANDEM = World([200], [[("R", 0, 0, 100), ("R", 0, 40, 100), ("R", 0, 100, 200)], [("R", 0, 0, 200)]])
# record 0 deletes [100, 140) of the reference, record 1 keeps it: a het deletion
HETDEL = World([200], [[("R", 0, 0, 100), ("R", 0, 140, 200)], [("R", 0, 0, 200)]])
# record 0: an insertion of 10 behind reference base 80 and a deletion of [120, 140); record 1: the same deletion (CN 0 there);
# records 2 and 3: the second reference record, plain and with an insertion of 7 behind base 50
MIX = World([200, 100], [[("R", 0, 0, 80), ("I", 10), ("R", 0, 80, 120), ("R", 0, 140, 200)], [("R", 0, 0, 120), ("R", 0, 140, 200)],
                         [("R", 1, 0, 100)], [("R", 1, 0, 50), ("I", 7), ("R", 1, 50, 100)]])

CASES = {
    "one_segment": (ONE, [(0, 5, 40, 3, [(17, 1)]), (0, 10, 50, 4, [(17, 1)]), (0, 0, 17, 9, []), (0, 16, 18, 2, [(17, 3)]), (0, 150, 200, 1, [(199, 2)])]),
    "two_haplotypes_artefact_on_one": (TWO, [(0, 20, 90, 3, [(50, 1)]), (1, 30, 80, 5, []), (1, 0, 51, 7, [])]),
    "same_artefact_on_both_haplotypes": (TWO, [(0, 20, 90, 3, [(50, 1)]), (1, 30, 80, 5, [(50, 1)]), (1, 0, 50, 7, [])]),
    "het_substitution_artefact_on_each_allele": (TWO, [(0, 60, 140, 3, [(100, 1)]), (1, 70, 130, 5, [(100, 1)]), (1, 100, 101, 2, [(100, 3)])]),
    "tandem_copies_amplicon_spans_the_junction": (TANDEM, [(0, 50, 150, 4, [(60, 1), (110, 1), (120, 2)]), (1, 30, 100, 6, [(70, 2)]), (0, 95, 105, 1, [])]),
    "deletion_inside_an_amplicon": (MIX, [(1, 100, 150, 3, [(119, 1), (120, 1)]), (0, 100, 170, 2, [(125, 1)])]),
    # record 0's amplicon [60, 130) is reference [60, 100) and [140, 170): it spans the deletion and must not cover the gap, where
    # record 1 has an artefact at 120 under its amplicons [80, 160) and [110, 125) ([121, 180) starts behind it)
    "het_deletion_site_in_the_gap": (HETDEL, [(0, 60, 130, 5, [(90, 1), (100, 1)]), (1, 80, 160, 3, [(120, 1)]), (1, 110, 125, 4, []), (1, 121, 180, 6, [])]),
    "insertion_under_middle_first_and_last_base": (MIX, [(0, 60, 120, 2, [(70, 1), (85, 1), (95, 1)]), (0, 80, 110, 3, [(80, 1), (90, 2)]), (0, 50, 90, 4, [(89, 3), (79, 1)])]),
    "amplicon_wholly_in_an_insertion": (MIX, [(0, 82, 88, 5, [(82, 1), (87, 2)]), (0, 70, 100, 1, []), (3, 50, 57, 2, [(53, 1)])]),
    "edit_on_the_first_and_last_base_of_a_segment": (MIX, [(0, 60, 170, 2, [(79, 1), (90, 1), (129, 1), (130, 1)]), (1, 0, 180, 3, [(0, 1), (119, 2), (120, 2), (179, 3)])]),
    "cn0_stretch": (MIX, [(0, 90, 160, 2, [(129, 1)]), (1, 90, 150, 3, [(119, 1), (120, 1)])]),
    "two_reference_records": (MIX, [(0, 0, 50, 1, [(0, 1)]), (2, 0, 100, 2, [(0, 1), (99, 2)]), (3, 40, 70, 3, [(49, 1), (57, 1), (52, 2)]), (1, 130, 180, 4, [(179, 1)])]),
    "three_alternate_bases_at_one_site": (TWO, [(0, 10, 60, 1, [(30, 1)]), (1, 10, 60, 2, [(30, 2)]), (0, 25, 35, 3, [(30, 3)]), (1, 30, 31, 4, [(30, 1)])]),
    "reads_of_zero": (TWO, [(0, 10, 60, 0, [(30, 1), (31, 1)]), (1, 10, 60, 2, [(31, 1)])]),
    "no_edit_at_all": (MIX, [(0, 5, 40, 3, []), (2, 10, 50, 4, [])]),
    "no_amplicon": (MIX, []),
}
for _w, _name in ((TWO, "all_of_two"), (MIX, "all_of_mix")):
    CASES[_name] = (_w, [t for k in sorted(CASES) if CASES[k][0] is _w for t in CASES[k][1]])
SLABS = [0, 130, 64, 7, 1]                                  # 130: between the two pieces around the deletion; 64, 7, 1: inside pieces


def rows(text):
    return [ln.split("\t") for ln in text.split("\n")[:-1]]


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("min_reads", [0, 1, 1000])
def test_body_equals_the_restatement_at_every_slab_size(case, min_reads):
    w, amps = CASES[case]
    want, arr, unl, extra = w.want(amps, min_reads)
    for slab in SLABS:
        got, gu = w.probe(amps, min_reads=min_reads, slab=slab)
        assert got == want and gu == unl, (case, slab)
    if min_reads == 1000:
        assert want == ""
    assert (arr["na"] >= 1).all() and (arr["na"] <= arr["ta"]).all() and (arr["nr"] <= arr["tr"]).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_conservation_laws(case):
    w, amps = CASES[case]
    starts, lens, reads, edits = w.inputs(amps)
    _, arr, unl, extra = w.want(amps)
    conservation(arr, unl, extra, starts, lens, len(edits), sum(reads[e[0]] for e in edits))
    # the same laws on the probe's own lines
    got, gu = w.probe(amps)
    info = [dict(kv.split("=") for kv in r[7].split(";")) for r in rows(got)]
    assert sum(int(i["NA"]) for i in info) + gu[0] == len(edits)
    assert sum(int(i["NR"]) for i in info) + gu[1] == sum(reads[e[0]] for e in edits)
    # per position: sum(NA) <= TA and sum(NR) <= TR
    per = {}
    for r, i in zip(rows(got), info):
        p = per.setdefault((r[0], r[1]), [0, 0, int(i["TA"]), int(i["TR"])])
        p[0] += int(i["NA"])
        p[1] += int(i["NR"])
        assert (p[2], p[3]) == (int(i["TA"]), int(i["TR"]))
    assert all(p[0] <= p[2] and p[1] <= p[3] for p in per.values())


def test_the_case_table_reaches_what_it_names():
    def lines(case, **kw):
        w, amps = CASES[case]
        return rows(w.probe(amps, **kw)[0]), w.probe(amps, **kw)[1]
    # one segment: section 14's table with the records renamed
    w, amps = CASES["one_segment"]
    starts, lens, reads, edits = w.inputs(amps)
    hap = scssim_amd.artefact_probe(starts, lens, reads, edits, w.hap_lens, ["chr1"], w.genome)
    assert w.probe(amps)[0] == hap and hap.count("\n") == 3
    b = int(TWO.G[50])
    r, u = lines("two_haplotypes_artefact_on_one")
    assert r == [["chr1", "51", ".", LETTERS[b], LETTERS[(b + 1) % 4], ".", ".", "NA=1;TA=3;NR=3;TR=15"]] and u == (0, 0)     # both haplotypes cover it
    r, u = lines("same_artefact_on_both_haplotypes")
    assert [x[7] for x in r] == ["NA=2;TA=2;NR=8;TR=8"]                                 # [0, 50) ends on 50: it does not cover it
    r, u = lines("het_substitution_artefact_on_each_allele")
    assert [x[1] for x in r] == ["101"] * 3 and len({x[3] for x in r}) == 2 and [LETTERS.index(x[3]) for x in r] == sorted(LETTERS.index(x[3]) for x in r)
    assert LETTERS[int(TWO.G[100])] != LETTERS[int(TWO.G[200 + 100])] and {x[7].split(";")[1] for x in r} == {"TA=3"}
    # tandem: [50, 150) of record 0 is reference [50, 100) and [40, 90); the two pieces overlap on [50, 90)
    assert pieces_of(50, 100, TANDEM.segs, TANDEM.ref_lens) == [(50, 100), (40, 90)]
    r, u = lines("tandem_copies_amplicon_spans_the_junction")
    by_pos = {x[1]: x[7] for x in r}
    assert by_pos["61"].startswith("NA=1;TA=3;") and by_pos["51"].startswith("NA=1;TA=3;") and by_pos["71"].startswith("NA=1;TA=3;")   # staged 60 -> 60; staged 110 -> 50; both pieces and record 1
    assert by_pos["61"] == "NA=1;TA=3;NR=4;TR=14"           # the amplicon's reads twice: its two pieces count separately
    # deletion: reference 120 .. 139 get nothing from record 1, whose amplicon [100, 150) is reference [100, 120) and [140, 170)
    assert pieces_of(int(MIX.hap_off[1]) + 100, 50, MIX.segs, MIX.ref_lens) == [(100, 120), (140, 170)]
    r, u = lines("deletion_inside_an_amplicon")
    assert [(x[1], x[7]) for x in r] == [("116", "NA=1;TA=2;NR=2;TR=5"), ("120", "NA=1;TA=2;NR=3;TR=5"), ("141", "NA=1;TA=2;NR=3;TR=5")]
    # the site in the gap of a het deletion gets nothing from the haplotype that deletes it: TA / TR are record 1's amplicons alone
    # (a piece that bridged the deletion would make it TA=3;TR=12); on either side of the gap that haplotype's two pieces count
    r, u = lines("het_deletion_site_in_the_gap")
    assert [(x[1], x[7]) for x in r] == [("91", "NA=1;TA=2;NR=5;TR=8"), ("121", "NA=1;TA=2;NR=3;TR=7"), ("141", "NA=1;TA=3;NR=5;TR=14")] and u == (0, 0)
    r, u = lines("insertion_under_middle_first_and_last_base")
    assert u == (3, 2 + 3 + 4) and [x[1] for x in r] == ["71", "80", "81", "86"]   # staged 85, 80 and 89 lie in the insertion [80, 90); 70, 79, 90 and 95 lift to 70, 79, 80 and 85
    r, u = lines("amplicon_wholly_in_an_insertion")
    assert r == [] and u == (3, 5 + 5 + 2) and pieces_of(82, 6, MIX.segs, MIX.ref_lens) == []
    r, u = lines("cn0_stretch")
    _, _, _, extra = MIX.want(CASES["all_of_mix"][1])
    assert (extra["ta"][120:140] == 0).all() and extra["ta"][119] > 0 and extra["ta"][140] > 0
    assert not [x for x in rows(MIX.probe(CASES["all_of_mix"][1])[0]) if x[0] == "chr1" and 121 <= int(x[1]) <= 140]
    r, u = lines("two_reference_records")
    assert [x[0] for x in r] == ["chr1", "chr1", "chr2", "chr2", "chr2", "chr2"] and [x[1] for x in r if x[0] == "chr2"] == ["1", "50", "51", "100"] and u == (1, 3)
    r, u = lines("three_alternate_bases_at_one_site")
    assert [x[1] for x in r] == ["31"] * 3 and [LETTERS.index(x[4]) for x in r] == sorted(LETTERS.index(x[4]) for x in r) and {x[7].split(";")[1] for x in r} == {"TA=4"}
    assert sorted(x[7].split(";")[0] for x in r) == ["NA=1", "NA=1", "NA=2"]
    assert [x[7] for x in lines("reads_of_zero")[0]] == ["NA=1;TA=2;NR=0;TR=2", "NA=2;TA=2;NR=2;TR=2"]
    assert [x[7] for x in lines("reads_of_zero", min_reads=1)[0]] == ["NA=2;TA=2;NR=2;TR=2"]
    assert lines("no_edit_at_all") == ([], (0, 0)) and lines("no_amplicon") == ([], (0, 0))


def test_random_haplotypes_amplicons_and_slabs():
    """Random tables: copies that jump backwards, insertions, deletions, two reference records; 300 amplicons with dense edits."""
    rng = np.random.default_rng(23)
    for trial in range(6):
        ref_lens = [int(rng.integers(300, 600)), int(rng.integers(100, 300))]
        haps = []
        for rr in (0, 0, 1, 1):
            h, total = [], 0
            while total < 500:
                if rng.random() < 0.25 and h and h[-1][0] == "R":
                    h.append(("I", int(rng.integers(1, 30))))
                else:
                    a = int(rng.integers(0, ref_lens[rr] - 1))
                    b = int(rng.integers(a + 1, min(ref_lens[rr], a + 120) + 1))
                    if h and h[-1][0] == "R" and h[-1][3] == a:
                        continue                                # (would be one segment)
                    h.append(("R", rr, a, b))
                total += h[-1][1] if h[-1][0] == "I" else h[-1][3] - h[-1][2]
            if h[0][0] == "I":
                h = h[1:]
            haps.append(h)
        w = World(ref_lens, haps, seed=trial)
        amps = []
        for _ in range(300):
            r = int(rng.integers(0, 4))
            a = int(rng.integers(0, w.hap_lens[r] - 1))
            b = int(rng.integers(a + 1, min(w.hap_lens[r], a + 150) + 1))
            pos = sorted(set(rng.integers(a, b, int(rng.integers(0, 6))).tolist()))
            amps.append((r, a, b, int(rng.integers(0, 9)), [(p, int(rng.integers(1, 4))) for p in pos]))
        for min_reads in (0, 1):
            want, arr, unl, extra = w.want(amps, min_reads)
            for slab in (0, 97, 10):
                assert w.probe(amps, min_reads=min_reads, slab=slab) == (want, unl), (trial, min_reads, slab)
        starts, lens, reads, edits = w.inputs(amps)
        conservation(*w.want(amps)[1:], starts, lens, len(edits), sum(reads[e[0]] for e in edits))
        assert unl[0] > 0 and max(len(pieces_of(s, l, w.segs, w.ref_lens)) for s, l in zip(starts, lens)) >= 3


def test_header_bytes():
    want = ("##fileformat=VCFv4.2\n##source=scssim\n##scssim_coordinates=reference\n##scssim_REF=<" + NOTE + ">\n##scssim_unlifted=<entries=3,reads=12>\n"
            "##contig=<ID=chr1,length=200>\n##contig=<ID=chr2,length=100>\n"
            '##INFO=<ID=NA,Number=1,Type=Integer,Description="edit entries (full amplicon, haplotype position) that carry the alternate base and lift to the site">\n'
            '##INFO=<ID=TA,Number=1,Type=Integer,Description="pieces of full amplicons, of any haplotype and copy, that cover the site">\n'
            '##INFO=<ID=NR,Number=1,Type=Integer,Description="reads allotted to the amplicons of the NA entries">\n'
            '##INFO=<ID=TR,Number=1,Type=Integer,Description="reads allotted to the amplicons of the TA pieces">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    assert header(MIX.ref_names, MIX.ref_lens, (3, 12)) == want and "haplotype" in NOTE and "reference FASTA" in NOTE
    w, amps = CASES["amplicon_wholly_in_an_insertion"]
    assert w.probe(amps, header=True)[0] == want                                    # a job without a site writes the header
    w, amps = CASES["two_reference_records"]
    body = w.probe(amps)[0]
    assert w.probe(amps, header=True)[0] == header(w.ref_names, w.ref_lens, (1, 3)) + body and body


BROKEN = ["amplicon_over_the_record_end", "amplicon_beyond_the_genome", "edit_outside_its_amplicon", "edit_of_no_amplicon", "alternate_base_4", "edit_twice_at_one_index",
          "records_do_not_add_up", "table_does_not_tile", "table_ends_before_the_amplicon", "segment_past_its_reference_record", "segment_of_an_unknown_reference_record",
          "segment_past_its_staged_record", "reference_of_2_58_bases"]


@pytest.mark.parametrize("what", BROKEN)
def test_inputs_that_do_not_fit_are_refused(what):
    w = MIX
    starts, lens, reads, edits = w.inputs([(0, 60, 170, 2, [(70, 1)])])
    hap_lens, ref_lens, lift_err = list(w.hap_lens), list(w.ref_lens), 0
    seg = [np.array(getattr(w.segs, k)) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")]
    if what == "amplicon_over_the_record_end":
        starts, lens, edits = [150], [60], []
    elif what == "amplicon_beyond_the_genome":
        starts, lens, edits = [int(w.hap_off[-1]) - 5], [20], []
    elif what == "edit_outside_its_amplicon":
        edits = [(0, 170, 1)]
    elif what == "edit_of_no_amplicon":
        edits = [(1, 70, 1)]
    elif what == "alternate_base_4":
        edits = [(0, 70, 4)]
    elif what == "edit_twice_at_one_index":
        edits = [(0, 70, 1), (0, 70, 2)]
    elif what == "records_do_not_add_up":
        hap_lens[-1] -= 1
    elif what == "table_does_not_tile":                         # a gap between the insertion and the segment behind it
        seg[0][2] += 1
        seg[1][2] -= 1
        lift_err = 2
    elif what == "table_ends_before_the_amplicon":
        seg = [s[:2] for s in seg]
        lift_err = 2
    elif what == "segment_past_its_reference_record":           # [140, 200) of the reference moved to [141, 201)
        seg[2][3] += 1
        lift_err = 3
    elif what == "segment_of_an_unknown_reference_record":
        seg[3][2] = 2
        lift_err = 3
    elif what == "segment_past_its_staged_record":              # the last segment of record 0 runs into record 1
        starts, lens, edits = [150], [40], []
        seg[1][3] += 5
        lift_err = 2
    else:
        ref_lens[1] = 1 << 58
    with pytest.raises(ScsError) as e:
        scssim_amd.artefact_ref_probe(starts, lens, reads, edits, hap_lens, w.genome, Segs(np.stack(seg, axis=1)), ref_lens, w.ref_names)
    assert e.value.code == SCS_EINVAL and e.value.lift_err == lift_err


def test_both_libraries_export_the_abi():
    want = {"scs_write_artefacts_ref", "scs_artefact_ref_sites", "scs_artefact_ref_kernel_time", "scs_artefact_ref_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    assert len(scssim_amd.GenReads.KERNELS) == 8            # the table's kernels have no slot of scs_kernel_time
    for m in ("write_artefacts_ref", "artefact_ref_sites", "artefact_ref_kernel_time"):
        assert callable(getattr(scssim_amd.GenReads, m))
    assert callable(scssim_amd.artefact_ref_probe)


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--artefacts-ref without --lift, with --gpus 2 or with an empty name ends the CLI with status 1 and a message before it touches
    a device (this machine may have none) or an input file (these do not exist); --artefacts-min-reads serves both tables."""
    r = _cli(["--artefacts-ref", "/nonexistent/a.vcf"])
    assert r.returncode == 1 and "--artefacts-ref needs --lift" in r.stderr, r.stderr
    r = _cli(["--artefacts-ref", "/nonexistent/a.vcf", "--lift", "/nonexistent/a.lift", "--gpus", "2"])
    assert r.returncode == 1 and "--artefacts-ref needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--artefacts-ref", ""])
    assert r.returncode == 1 and "--artefacts-ref needs the name of the file" in r.stderr, r.stderr
    r = _cli(["--artefacts-min-reads", "1"])
    assert r.returncode == 1 and "--artefacts-min-reads needs --artefacts (the file the artefact table goes to)" in r.stderr, r.stderr
    r = _cli(["--artefacts-ref", "/nonexistent/a.vcf", "--artefacts-min-reads", "1"])
    assert r.returncode == 1 and "--artefacts-ref needs --lift" in r.stderr, r.stderr   # (the min-reads option is accepted with this table alone)
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--artefacts-ref <string>" in h.stdout + h.stderr
