"""Host-side tests of the lift table (scs_lift.h): the table the simuvars plan gives against the compiled
reference's own haplotype FASTA; the true copy number per reference bin by hand; the file and its parser; the function
k_depth_lift runs on one placed read, through its host probe, against a restatement in plain Python that goes by way of POS and
CIGAR; the CLI's refusals; the stand-alone sanitizer build.  No GPU needed."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from lift_cases import copies_from_table, ref_layout
from test_depth_host import EVENTS, pos_cigar

import scssim_amd
from scssim_amd import SCS_EINVAL, SCS_EIO, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
SV = os.path.join(GOLDEN, "simuvars")


def read_fasta(data):
    """[(name, sequence bytes)] of FASTA text."""
    out = []
    for block in data.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        out.append((head.split()[0].decode(), body.replace(b"\n", b"")))
    return out


@pytest.fixture(scope="module")
def sv(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift")
    ref = str(d / "ref.fa")
    open(ref, "wb").write(gzip.open(os.path.join(SV, "ref.fa.gz")).read())
    lift = str(d / "full.lift")
    table, subst = scssim_amd.lift_plan_probe(ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"), lift)
    return dict(ref=ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), lift=lift, table=table, subst=subst, dir=d,
                ref_recs=read_fasta(open(ref, "rb").read()), hap_recs=read_fasta(gzip.open(os.path.join(SV, "expected_full.fa.gz")).read()))


def hap_record_of(t):
    """The staged record of every segment, and the records' first global indices."""
    off = np.concatenate([[0], np.cumsum(np.asarray(t.hap_lens, np.int64))])
    return np.searchsorted(off, np.asarray(t.hap_off, np.int64), side="right") - 1, off


def assert_maximal_and_anchored(t):
    """No two neighbours could be one segment; every I segment's anchor follows the rule of the contract."""
    rec, off = hap_record_of(t)
    n = len(t)
    for i in range(n):
        assert t.len[i] > 0
        assert t.hap_off[i] + t.len[i] <= off[rec[i] + 1]                                  # no segment straddles two staged records
        if i + 1 < n:
            assert t.hap_off[i] + t.len[i] == t.hap_off[i + 1]
            if rec[i] == rec[i + 1] and t.kind[i] == t.kind[i + 1]:
                assert t.kind[i] == 0 and not (t.ref_rec[i] == t.ref_rec[i + 1] and t.ref_pos[i] + t.len[i] == t.ref_pos[i + 1]), i
    assert t.hap_off[0] == 0 and t.hap_off[-1] + t.len[-1] == off[-1]
    for i in np.nonzero(np.asarray(t.kind) == 1)[0]:
        same = [j for j in range(n) if rec[j] == rec[i] and t.kind[j] == 0]
        before, after = [j for j in same if j < i], [j for j in same if j > i]
        want = t.ref_pos[before[-1]] + t.len[before[-1]] if before else (t.ref_pos[after[0]] if after else 0)
        assert t.ref_pos[i] == want and t.ref_rec[i] == rec[i] // 2, i


def test_table_against_the_reference_binarys_fasta(sv):
    """1: the segments tile every record of the compiled reference's FASTA with its lengths and names; the table is maximal; every R
    segment's text is the reference text it names except at the plan's substitutions; every I segment is a literal of vars.txt."""
    t, subst = sv["table"], set(int(x) for x in sv["subst"])
    assert t.hap_names == [n for n, _ in sv["hap_recs"]] and t.hap_lens.tolist() == [len(s) for _, s in sv["hap_recs"]]
    assert t.ref_lens.tolist() == [len(s) for _, s in sv["ref_recs"]] and len(t.ref_names) == 3
    assert_maximal_and_anchored(t)
    hap = np.frombuffer(b"".join(s for _, s in sv["hap_recs"]).upper(), np.uint8)
    refs = [np.frombuffer(s.upper(), np.uint8) for _, s in sv["ref_recs"]]
    literals = set(ln.split("\t")[3].upper().encode() for ln in open(sv["vars"]).read().split("\n") if ln.startswith("i\t"))
    n_diff = 0
    for i in range(len(t)):
        h = hap[int(t.hap_off[i]):int(t.hap_off[i] + t.len[i])]
        if t.kind[i] == 0:
            r = refs[t.ref_rec[i]][int(t.ref_pos[i]):int(t.ref_pos[i] + t.len[i])]
            assert len(r) == len(h)
            diff = np.nonzero(h != r)[0] + int(t.hap_off[i])
            assert set(diff.tolist()) <= subst, (i, diff[:5])
            n_diff += len(diff)
        else:
            assert h.tobytes() in literals, (i, h.tobytes())
    assert n_diff > 100 and (np.asarray(t.kind) == 1).sum() >= 8                             # the SNPs show, and the insertions are there
    assert len(subst) >= n_diff


@pytest.mark.parametrize("case", ["plain", "snp_only"])
def test_no_structural_variants_give_one_segment_per_record(case, sv):
    t, subst = scssim_amd.lift_plan_probe(sv["ref"], sv["snp"] if case == "snp_only" else None, None)
    assert len(t) == 6 and (t.kind == 0).all() and (t.ref_pos == 0).all()
    assert t.ref_rec.tolist() == [0, 0, 1, 1, 2, 2] and t.len.tolist() == [400000, 400000, 150000, 150000, 60000, 60000] == t.hap_lens.tolist()
    assert (len(subst) > 0) == (case == "snp_only")


@pytest.mark.parametrize("w", [1000, 37])
def test_copies_by_hand(w, sv):
    """2: the sum is the R segments' bases; CN 0, CN 8 and plain stretches of chr20 have 0, 8 and 2 copies per reference base."""
    t = sv["table"]
    copies = copies_from_table(t, t.ref_lens, w)
    off, nb = ref_layout(t.ref_lens, w)
    assert int(copies[:nb].sum()) == int(t.len[t.kind == 0].sum()) and int(copies[nb]) == int(t.len[t.kind == 1].sum()) > 0
    assert int(copies.sum()) == int(t.hap_lens.sum())
    inside = lambda a, b: np.arange(-(-a // w), b // w)                                       # bins wholly inside the 0-based [a, b) of chr20
    width = lambda bins: np.minimum((bins + 1) * w, int(t.ref_lens[0])) - bins * w
    for a, b, cn in ((149999, 160000, 0), (289999, 300000, 8), (1000, 20000, 2), (370000, 389000, 2)):
        bins = inside(a, b)
        assert len(bins) >= 8 and (copies[bins] == cn * width(bins)).all(), (a, b, cn)
    assert (copies[off[2]:off[3]] == 2 * np.minimum(w, 60000 - np.arange(off[3] - off[2]) * w)).all()   # chromosome 5: untouched


VALID = ["##scssim-lift v1", "#ref\tc1\t1000", "#hap\th1\t600", "#hap\th2\t500",
         "h1\t0\t300\tc1\t0\t300\tR", "h1\t300\t320\tc1\t300\t300\tI", "h1\t320\t600\tc1\t100\t380\tR", "h2\t0\t500\tc1\t500\t1000\tR"]


def _edit(line, text):
    v = list(VALID)
    v[line - 1] = text
    return v


BROKEN = [
    # name, lines, the line the parser must refuse it at
    ("unknown_haplotype_record", _edit(5, "hX\t0\t300\tc1\t0\t300\tR"), 5),
    ("unknown_reference_record", _edit(7, "h1\t320\t600\tcX\t100\t380\tR"), 7),
    ("gap", _edit(7, "h1\t330\t600\tc1\t110\t380\tR"), 7),
    ("overlap", _edit(7, "h1\t310\t600\tc1\t90\t380\tR"), 7),
    ("unsorted_lines", VALID[:4] + [VALID[5], VALID[4]] + VALID[6:], 5),
    ("records_out_of_order", VALID[:4] + [VALID[7]] + VALID[4:7], 5),
    ("record_not_covered", VALID[:7], 8),
    ("next_record_before_the_end", VALID[:6] + [VALID[7]], 7),
    ("past_its_haplotype_record", _edit(8, "h2\t0\t501\tc1\t499\t1000\tR"), 8),
    ("past_its_reference_record", _edit(8, "h2\t0\t500\tc1\t501\t1001\tR"), 8),
    ("r_lengths_differ", _edit(5, "h1\t0\t300\tc1\t0\t299\tR"), 5),
    ("i_with_a_reference_interval", _edit(6, "h1\t300\t320\tc1\t300\t320\tI"), 6),
    ("wrong_column_count", _edit(6, "h1\t300\t320\tc1\t300\t300"), 6),
    ("wrong_column_count_in_the_header", _edit(3, "#hap\th1"), 3),
    ("not_a_number", _edit(5, "h1\t0\t3e2\tc1\t0\t300\tR"), 5),
    ("missing_first_line", VALID[1:], 1),
    ("missing_hap_lines", [VALID[0], VALID[1]] + VALID[4:], 3),
    ("empty_file", [], 1),
]


def test_file_round_trip_and_the_small_valid_file(sv, tmp_path):
    """3: the file the plan probe writes parses back to the identical table; so does the hand-written file the broken ones derive from."""
    t, back = sv["table"], scssim_amd.lift_file_probe(sv["lift"])
    assert back.same_segments(t) and back.hap_names == t.hap_names and back.ref_names == t.ref_names
    assert back.hap_lens.tolist() == t.hap_lens.tolist() and back.ref_lens.tolist() == t.ref_lens.tolist()
    head = open(sv["lift"]).read().split("\n")
    assert head[0] == "##scssim-lift v1" and head[1] == "#ref\t20\t400000" and head[4] == "#hap\t20_1_400000\t505006" and head[-1] == ""
    assert head[10] == "20_1_400000\t0\t30099\t20\t0\t30099\tR" and len(head) == 1 + 3 + 6 + len(t) + 1
    p = str(tmp_path / "valid.lift")
    open(p, "w").write("\n".join(VALID) + "\n")
    v = scssim_amd.lift_file_probe(p)
    assert v.hap_off.tolist() == [0, 300, 320, 600] and v.len.tolist() == [300, 20, 280, 500] and v.kind.tolist() == [0, 1, 0, 0] and v.ref_pos.tolist() == [0, 300, 100, 500]
    with pytest.raises(ScsError) as e:
        scssim_amd.lift_file_probe(str(tmp_path / "missing.lift"))
    assert e.value.code == SCS_EIO and e.value.line == 0


@pytest.mark.parametrize("name,lines,line", BROKEN, ids=[b[0] for b in BROKEN])
def test_broken_files_are_refused_with_their_line(name, lines, line, tmp_path):
    p = str(tmp_path / (name + ".lift"))
    open(p, "w").write("".join(ln + "\n" for ln in lines))
    with pytest.raises(ScsError) as e:
        scssim_amd.lift_file_probe(p)
    assert e.value.code == SCS_EIO and e.value.line == line and "line %d" % line in str(e.value), str(e.value)


# ---- 4: one read through lift_read
class Layout:
    """A lift table from per-record lists of (kind, ref_rec, ref_pos, len); I segments get their anchors by the contract's rule."""

    def __init__(self, records, ref_lens):
        self.hap_off, self.len, self.ref_pos, self.ref_rec, self.kind, self.hap_lens = [], [], [], [], [], []
        at = 0
        for segs in records:
            start = at
            firsts = [s[2] for s in segs if s[0] == 0]
            anchor = firsts[0] if firsts else 0
            for kind, rr, rp, ln in segs:
                if kind == 0:
                    anchor = rp + ln
                self.hap_off.append(at); self.len.append(ln); self.ref_rec.append(rr); self.kind.append(kind); self.ref_pos.append(rp if kind == 0 else anchor)
                at += ln
            self.hap_lens.append(at - start)
        self.ref_lens = ref_lens
        self.bounds = self.hap_off[1:]


ONE = Layout([[(0, 0, 0, 100000)]], [100000])
# record A: a short insertion, a long one, copy 2 of a unit (the reference jumps backwards), a germline deletion (it jumps forwards);
# record B lies on the other reference record
MIXED = Layout([[(0, 0, 0, 2000), (1, 0, 0, 20), (0, 0, 2000, 3000), (1, 0, 0, 400), (0, 0, 5000, 2000), (0, 0, 5000, 2000), (0, 0, 7010, 1990)],
                [(0, 1, 0, 4000)]], [9000, 4001])


def restate(layout, pos, cigar, w):
    """The contract from POS (global staged index) and CIGAR, base by base: (bin of the reads increment, {bin: bases})."""
    off, nb = ref_layout(layout.ref_lens, w)
    starts = np.asarray(layout.hap_off, np.int64)
    bases, first, g = {}, None, pos
    for l, k in re.findall(r"(\d+)([MID])", cigar):
        l = int(l)
        if k == "M":
            for x in range(g, g + l):
                i = int(np.searchsorted(starts, x, side="right")) - 1
                b = nb if layout.kind[i] else int(off[layout.ref_rec[i]]) + (layout.ref_pos[i] + x - layout.hap_off[i]) // w
                bases[b] = bases.get(b, 0) + 1
                if first is None and b != nb:
                    first = b
        if k != "I":
            g += l
    return (nb if first is None else first), bases


def lefts(layout, n):
    """Leftmost window bases: every boundary exactly at the read's first base, at its last base, one past it and in its middle; for
    MIXED a read wholly inside the long insertion, one that starts inside it, and the last window of record A."""
    out = {1000}
    for b in layout.bounds:
        out |= {b, b - (n - 1), b - n, b - n // 2, b - 70}
    if layout is MIXED:
        out |= {5020 + 100, 5020 + 330, layout.hap_lens[0] - n, layout.hap_lens[0]}
    return sorted(x for x in out if x >= 0)


def check_read(layout, left, n, events, reverse, w):
    pos0 = left + n - 1 if reverse else left
    pos, cigar = pos_cigar(pos0, n, events, reverse)
    want_first, want = restate(layout, pos, cigar, w)
    first, got = scssim_amd.lift_read_probe(layout, layout.hap_lens, layout.ref_lens, pos0, n, events, reverse, bin_width=w)
    summed = {}
    for b, k in got:
        summed[b] = summed.get(b, 0) + k
    assert (first, summed) == (want_first, want), (left, reverse, cigar, w)
    assert all(got[i][0] != got[i + 1][0] for i in range(len(got) - 1)) and all(k > 0 for _, k in got)   # the pieces of one bin are summed first
    return pos, cigar, got


@pytest.mark.parametrize("w", [1, 37, 1000])
@pytest.mark.parametrize("name,n,events", EVENTS, ids=[e[0] for e in EVENTS])
def test_read_increments_match_pos_and_cigar_through_the_table(name, n, events, w):
    """4: lift_read (what k_depth_lift runs per read) against the restatement, both strands, over one segment and over the mixed
    layout: boundaries at the first base, the last base and one past it, insertions, the backwards jump, the record's end."""
    nb = ref_layout(MIXED.ref_lens, w)[1]
    seen = dict(pseudo_only=0, starts_in_insertion=0, two_bounds=0, back=0)
    for layout in (ONE, MIXED):
        for reverse in (False, True):
            for left in lefts(layout, n):
                if left < layout.hap_lens[0] < left + n:                                      # (a window over the records' junction: test_named_geometries)
                    continue
                pos, cigar, got = check_read(layout, left, n, events, reverse, w)
                if layout is MIXED:
                    bins = [b for b, _ in got]
                    seen["pseudo_only"] += bins == [nb]
                    seen["starts_in_insertion"] += len(bins) > 1 and bins[0] == nb
                    seen["two_bounds"] += pos < 2000 and pos + n - 10 > 2020
                    seen["back"] += pos < 7420 <= pos + 100
    assert seen["pseudo_only"] >= 2 and seen["starts_in_insertion"] >= 2 and seen["two_bounds"] >= 2 and seen["back"] >= 2, seen


def test_named_geometries():
    """4: the cases of the list by hand, at W = 1000 over MIXED (reference bins 0..8 on record 0, 9..13 on record 1, pseudo-bin 14)."""
    probe = lambda pos0, ev=(), rev=False, w=1000: scssim_amd.lift_read_probe(MIXED, MIXED.hap_lens, MIXED.ref_lens, pos0, 150, ev, rev, bin_width=w)
    assert probe(1950) == (1, [(1, 50), (14, 20), (2, 80)])                                   # an insertion in the middle
    assert probe(5100) == (14, [(14, 150)])                                                   # wholly inside an insertion: the pseudo-bin has the read
    assert probe(5400) == (5, [(14, 20), (5, 130)])                                           # starts inside one: the read counts where its first lifted base lies
    assert probe(7350) == (6, [(6, 70), (5, 80)])                                             # copy 2 starts where copy 1 started: 6999 -> 5000
    assert probe(7499, rev=True) == (6, [(6, 70), (5, 80)])                                   # the same bases from the other strand
    assert probe(9350) == (6, [(6, 70), (7, 80)])                                             # the germline deletion: 6999 -> 7010
    assert probe(9350, [(60, 1, 30)]) == (6, [(6, 60), (7, 60)])                              # a sequencing deletion that spans a segment end (9420): 6930 .. 6989, then 7030 .. 7089
    assert probe(11260) == (8, [(8, 150)]) and probe(11410) == (9, [(9, 150)])                # the last window of record A, the first of record B
    for pos0, rev in ((11261, False), (11409, False), (11410 + 100, True)):                   # into the other record's haplotype: never crossed, an error
        with pytest.raises(ScsError) as e:
            probe(pos0, rev=rev)
        assert e.value.code == SCS_EINVAL and e.value.lift_err == 1
    broken = Layout([[(0, 0, 0, 2000), (0, 0, 8900, 200)]], [9000])                           # a segment that lifts past its reference record
    with pytest.raises(ScsError) as e:
        scssim_amd.lift_read_probe(broken, broken.hap_lens, broken.ref_lens, 1950, 150, bin_width=1000)
    assert e.value.lift_err == 3
    short = Layout([[(0, 0, 0, 2000)]], [9000])                                               # the table ends before the record does
    with pytest.raises(ScsError) as e:
        scssim_amd.lift_read_probe(short, [3000], short.ref_lens, 1950, 150, bin_width=1000)
    assert e.value.lift_err == 2


def _cli(sub, args):
    return subprocess.run([CLI, sub] + args, capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work(tmp_path):
    """5: --depth-ref without --lift, --lift with --gpus 2 and simuvars --lift to a path that cannot be written end the CLI with their
    own message before it touches a device (this machine has none) or an input file (these do not exist)."""
    gen = ["-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"]
    r = _cli("genreads", gen + ["--depth-ref", "/nonexistent/d.tsv"])
    assert r.returncode != 0 and "--depth-ref needs --lift" in r.stderr, r.stderr
    r = _cli("genreads", gen + ["--lift", "/nonexistent/x.lift", "--gpus", "2"])
    assert r.returncode != 0 and "--lift needs --gpus 1" in r.stderr, r.stderr
    r = _cli("simuvars", ["-r", "/nonexistent/ref.fa", "-o", str(tmp_path / "o.fa"), "--lift", "/nonexistent/dir/x.lift"])
    assert r.returncode != 0 and "can not open lift file /nonexistent/dir/x.lift" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "o.fa"))
    h = _cli("genreads", ["-h"])
    assert "--lift <string>" in h.stdout + h.stderr and "--depth-ref <string>" in h.stdout + h.stderr
    h = _cli("simuvars", ["-h"])
    assert "--lift <string>" in h.stdout + h.stderr


def test_both_libraries_export_the_lift_abi():
    from conftest import SEAMS_LIB
    want = {"scs_write_lift", "scs_load_lift", "scs_lift_info", "scs_lift_segments", "scs_lift_positions", "scs_set_depth_ref", "scs_depth_ref_bins", "scs_depth_ref_record_bins",
            "scs_download_depth_ref", "scs_write_depth_ref", "scs_depth_ref_kernel_time", "scs_lift_plan_probe", "scs_lift_file_probe", "scs_lift_read_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    assert len(scssim_amd.GenReads.KERNELS) == 8                                              # scs_kernel_time keeps its slots


def host_check_rows():
    """The grid of test 4 and the parser's case table as the lines tools/lift_host_check.cpp reads."""
    rows = []
    for li, layout in enumerate((ONE, MIXED)):
        rows.append("table %d %d %d %d " % (li, len(layout.hap_off), len(layout.hap_lens), len(layout.ref_lens)) +
                    " ".join("%d %d %d %d %d" % s for s in zip(layout.hap_off, layout.len, layout.ref_pos, layout.ref_rec, layout.kind)) + " " +
                    " ".join(str(x) for x in layout.hap_lens) + " " + " ".join(str(x) for x in layout.ref_lens))
        for name, n, events in EVENTS:
            for w in (1, 37, 1000):
                for reverse in (False, True):
                    for left in lefts(layout, n):
                        if left < layout.hap_lens[0] < left + n:
                            continue
                        pos0 = left + n - 1 if reverse else left
                        first, want = restate(layout, *pos_cigar(pos0, n, events, reverse), w)
                        rows.append("read %d %d %d %d %d %d " % (li, n, pos0, int(reverse), w, len(events)) + " ".join(str(v) for e in events for v in e) +
                                    " %d %d " % (first, len(want)) + " ".join("%d %d" % kv for kv in sorted(want.items())))
    return rows


def test_sanitizer_build_of_the_host_code(tmp_path):
    """6: tools/lift_host_check.py: scs_lift.h (lift_read, the parser) as a stand-alone CPU program under AddressSanitizer and
    UndefinedBehaviorSanitizer over the grid of test 4 and the case table of test 3."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lift_host_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) reads, (\d+) files, 0 wrong", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) == len(BROKEN) + 1, r.stdout[-500:]
