"""Host-side tests of the site support (scs_set_site_support): the function the kernel runs on one placed read, through its host
probe, against a restatement in plain Python that goes by way of POS, CIGAR and SEQ; the line with its counters through the
formatter the emit kernel runs; the CLI's --support options and their refusals; the sanitizer tool.  No GPU needed."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from test_depth_host import pos_cigar, window_bases

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
REC_LEN = 100000
EVCAP = 32                                                 # TRUTH_EVCAP (scs_truth.h)
COMP = str.maketrans("ACGTN", "TGCAN")
CLS = {"A": 0, "C": 1, "G": 2, "T": 3}

EVENTS = [
    # name, n, events (window position, deletion?, length)
    ("no_events", 150, []),
    ("one_insertion", 150, [(70, 0, 3)]),
    ("one_deletion", 150, [(60, 1, 5)]),
    ("insertion_at_0", 150, [(0, 0, 2)]),
    ("insertion_at_n_minus_1", 150, [(149, 0, 3)]),
    ("deletion_clipped_at_the_window_end", 150, [(146, 1, 4)]),
    ("leading_deletion", 150, [(0, 1, 4)]),
    ("two_adjacent_events", 150, [(50, 1, 3), (53, 0, 2)]),
    ("evcap_events", 150, [(4 * i + 2, i & 1, 1 + (i % 3 == 0)) for i in range(EVCAP)]),
    ("rollback_51", 51, [(10, 1, 2)]),
]


def fastq_bases(qlen, with_n=False):
    """The read's FASTQ bases (read orientation): no period that a shifted cursor would survive; with_n: an N every 11 bases."""
    s = "".join("ACGT"[(i * i + i // 3) % 4] for i in range(qlen))
    return "".join("N" if with_n and i % 11 == 5 else ch for i, ch in enumerate(s))


def sam_fields(pos0, n, events, reverse, fq):
    """(POS - 1, CIGAR, SEQ) as the truth SAM states them: SEQ genome-forward, the complement of the reversed bases on a reverse read."""
    pos, cigar = pos_cigar(pos0, n, events, reverse)
    return pos, cigar, fq[::-1].translate(COMP) if reverse else fq


def restatement(pos, cigar, seq, positions):
    """The contract from POS, CIGAR and SEQ alone: [(position index, class)] ascending; D gives class 5, inserted bases are skipped."""
    at = {}
    g, qi = pos, 0
    for l, k in re.findall(r"(\d+)([MID])", cigar):
        l = int(l)
        for t in range(l):
            if k == "M":
                at[g + t] = CLS.get(seq[qi + t], 4)
            elif k == "D":
                at[g + t] = 5
        if k != "I":
            g += l
        if k != "D":
            qi += l
    assert qi == len(seq)
    return [(i, at[p]) for i, p in enumerate(positions) if p in at]


def position_lists(pos, cigar):
    """The lists of the grid for one alignment: none; every base of the read (and two on either side); and the special places -- the
    first and the last aligned base, one before and one after each, inside every deletion and at both of its edges, just before and
    just after every insertion."""
    g, special, ops = pos, set(), re.findall(r"(\d+)([MID])", cigar)
    hi = pos + sum(int(l) for l, k in ops if k != "I") - 1
    special |= {pos - 1, pos, pos + 1, hi - 1, hi, hi + 1}
    for l, k in ops:
        l = int(l)
        if k == "D":
            special |= {g - 1, g, g + l // 2, g + l - 1, g + l}
        if k == "I":
            special |= {g - 1, g}
        if k != "I":
            g += l
    return [[], sorted(p for p in special if 0 <= p < REC_LEN), list(range(max(0, pos - 2), min(REC_LEN, hi + 3)))]


def grid():
    """(name, n, events, reverse, pos0, fq, positions) of every probe call of the table."""
    for name, n, events in EVENTS:
        qlen = len(window_bases(n, events))
        for reverse in (False, True):
            pos0 = 1000 + n - 1 if reverse else 1000
            for with_n in (False, True):
                fq = fastq_bases(qlen, with_n)
                pos, cigar, _ = sam_fields(pos0, n, events, reverse, fq)
                for positions in position_lists(pos, cigar):
                    yield name, n, events, reverse, pos0, fq, positions


@pytest.mark.parametrize("name,n,events", EVENTS, ids=[e[0] for e in EVENTS])
def test_read_support_matches_pos_cigar_and_seq(name, n, events):
    """support_read (what k_support runs per read) reports, at every listed position, the class POS, CIGAR and SEQ give."""
    seen, classes = 0, set()
    for nm, n_, ev, reverse, pos0, fq, positions in grid():
        if nm != name:
            continue
        pos, cigar, seq = sam_fields(pos0, n, events, reverse, fq)
        want = restatement(pos, cigar, seq, positions)
        got = scssim_amd.support_read_probe(pos0, n, fq, positions, events, reverse, rec_len=REC_LEN)
        assert got == want, (name, reverse, cigar, positions[:8], got[:8], want[:8])
        seen += 1
        classes |= set(c for _, c in got)
    assert seen == 12 and {0, 1, 2, 3, 4} <= classes
    if "deletion" in name or name in ("two_adjacent_events", "evcap_events"):
        dropped = name in ("leading_deletion", "deletion_clipped_at_the_window_end")
        assert (5 in classes) == (not dropped)              # a deletion before the first or after the last aligned base is dropped: it deletes nothing
    if name == "rollback_51":
        assert pos_cigar(1000, n, events, False)[1] == "51M" and 5 not in classes
    if name == "leading_deletion":
        assert pos_cigar(1000, n, events, False) == (1004, "146M")
        assert scssim_amd.support_read_probe(1000, n, fastq_bases(146), [1000, 1003, 1004], events) == [(2, CLS[fastq_bases(146)[0]])]
    if name == "evcap_events":
        assert len(events) == EVCAP and pos_cigar(1000, n, events, False)[1].count("I") == EVCAP // 2


def test_a_read_with_an_n_gives_class_4_and_a_reverse_read_the_complement():
    fq = "ACGTN" * 30
    assert scssim_amd.support_read_probe(1000, 150, fq, [999, 1000, 1004, 1149, 1150]) == [(1, 0), (2, 4), (3, 4)]
    assert scssim_amd.support_read_probe(1149, 150, fq, [999, 1000, 1004, 1149, 1150], reverse=True) == [(1, 4), (2, 3), (3, 3)]
    assert scssim_amd.support_read_probe(1000, 150, fq, []) == []
    assert scssim_amd.support_read_probe(1000, 150, fq, [5, 999, 1150, 99999]) == []


def test_refusals():
    fq = fastq_bases(150)
    for kw in (dict(positions=[5, 5]), dict(positions=[7, 5]), dict(seq=fq[:149]), dict(pos0=REC_LEN - 149), dict(events=[(10, 0, 1), (5, 1, 2)]),
               dict(events=[(4 * i + 2, 0, 1) for i in range(EVCAP + 1)], seq=fastq_bases(150 + EVCAP + 1))):
        a = dict(pos0=1000, n=150, seq=fq, positions=[1000], events=[], rec_len=REC_LEN)
        a.update(kw)
        with pytest.raises(ScsError) as e:
            scssim_amd.support_read_probe(**a)
        assert e.value.code == SCS_EINVAL, kw


def test_line_probe():
    """The suffix text, REF = N (class 4), the largest counter values (10 digits), and stripping the suffix gives back site_line's text."""
    big = 4294967295
    plain = scssim_amd.site_support_line_probe("chr7", 41, 2, 0, 3, 9, 12, 40)
    assert plain == "chr7\t42\t.\tG\tA\t.\t.\tNA=3;TA=9;NR=12;TR=40\n"
    line = scssim_amd.site_support_line_probe("chr7", 41, 2, 0, 3, 9, 12, 40, [5, 0, 31, 1, 2, 7])
    assert line == plain[:-1] + ";DP=39;AD=31,5;DL=7\n"
    line = scssim_amd.site_support_line_probe("chr7", 41, 4, 3, 3, 9, 12, 40, [5, 0, 31, 1, 2, 7])
    assert line.endswith("\tN\tT\t.\t.\tNA=3;TA=9;NR=12;TR=40;DP=39;AD=2,1;DL=7\n")
    line = scssim_amd.site_support_line_probe("c", 0, 0, 1, big, big, 2 ** 63, 2 ** 64 - 1, [big] * 6)
    assert line == "c\t1\t.\tA\tC\t.\t.\tNA=%d;TA=%d;NR=%d;TR=%d;DP=%d;AD=%d,%d;DL=%d\n" % (big, big, 2 ** 63, 2 ** 64 - 1, 5 * big, big, big, big)
    assert re.sub(r";DP=\d+;AD=\d+,\d+;DL=\d+\n$", "\n", line) == scssim_amd.site_support_line_probe("c", 0, 0, 1, big, big, 2 ** 63, 2 ** 64 - 1)
    assert scssim_amd.site_support_line_probe("c", 0, 0, 1, 1, 1, 1, 1, [0] * 6).endswith(";DP=0;AD=0,0;DL=0\n")
    for ref, alt in ((5, 0), (0, 4)):
        with pytest.raises(ScsError):
            scssim_amd.site_support_line_probe("c", 0, ref, alt, 1, 1, 1, 1)


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--support with --gpus 2 and --support-min-reads without --support end the CLI with their own message before it touches a
    device (this machine has none) or an input file (these do not exist)."""
    r = _cli(["--support", "/nonexistent/s.vcf", "--gpus", "2"])
    assert r.returncode != 0 and "--support needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--support-min-reads", "1"])
    assert r.returncode != 0 and "--support-min-reads needs --support" in r.stderr, r.stderr
    r = _cli(["--support", "/nonexistent/s.vcf", "--support-min-reads", "-1"])
    assert r.returncode != 0 and "--support-min-reads should be a non-negative integer" in r.stderr, r.stderr
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--support <string>" in h.stdout + h.stderr and "--support-min-reads <int>" in h.stdout + h.stderr


def test_both_libraries_export_the_site_support_abi():
    from conftest import SEAMS_LIB
    want = {"scs_set_site_support", "scs_site_support", "scs_write_site_support", "scs_site_support_kernel_time", "scs_support_read_probe", "scs_site_support_line_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib


def test_sanitizer_tool_builds_and_passes(tmp_path):
    """tools/support_host_check.py: scs_support.h as a stand-alone CPU program under AddressSanitizer and UndefinedBehaviorSanitizer,
    over the grid above, every array in a heap block of exactly its size.  Skips only where the host compiler has no sanitizer runtimes."""
    probe = tmp_path / "p.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "p")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "p")]).returncode != 0:
        pytest.skip("the host compiler lacks the AddressSanitizer / UndefinedBehaviorSanitizer runtimes: " + r.stderr[-300:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "support_host_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 wrong" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
