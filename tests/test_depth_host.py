"""Host-side tests of the depth track (scs_set_depth): the function the depth kernel runs on one placed read, through its host
probe, against a restatement in plain Python that goes by way of POS and CIGAR; the bin layout the ctx uses; the CLI's --depth
options and their refusals.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import scssim_amd
from scssim_amd import SCS_EINVAL, ScsError

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
REC_LEN = 100000                                           # the record of the grid below: 100 bins of 1000, 2703 bins of 37 (the last one 26 bases)


def window_bases(n, events):
    """Profile::predict's output: per read base its window index, or -1 for an inserted base (after the n + delta < 50 rollback)."""
    if n + sum(-l if d else l for _, d, l in events) < 50:
        events = []
    ev = {p: (d, l) for p, d, l in events}
    out, j = [], 0
    while j < n:
        if j in ev and ev[j][0]:
            j += ev[j][1]
            continue
        out.append(j)
        if j in ev:
            out += [-1] * ev[j][1]
        j += 1
    return out


def pos_cigar(pos0, n, events, reverse):
    """(POS - 1, CIGAR) of the read, genome-forward, as the truth SAM states them: deletions before the first and after the last
    aligned base are dropped, an insertion at either end stays."""
    coords = [None if x < 0 else (pos0 - x if reverse else pos0 + x) for x in window_bases(n, events)]
    if reverse:
        coords = coords[::-1]
    ops, prev = [], None
    for c in coords:
        if c is None:
            k, l = "I", 1
        else:
            if prev is not None and c > prev + 1:
                ops.append(["D", c - prev - 1])
            k, l, prev = "M", 1, c
        if ops and ops[-1][0] == k:
            ops[-1][1] += l
        else:
            ops.append([k, l])
    return min(c for c in coords if c is not None), "".join("%d%s" % (l, k) for k, l in ops)


def increments(pos, cigar, w):
    """The contract, from POS and CIGAR alone: the bin of the `reads` increment, and {bin: bases} over the M operations."""
    bases, g = {}, pos
    for l, k in re.findall(r"(\d+)([MID])", cigar):
        l = int(l)
        if k == "M":
            for x in range(g, g + l):
                bases[x // w] = bases.get(x // w, 0) + 1
        if k != "I":
            g += l
    return pos // w, sorted(bases.items())


EVENTS = [
    # name, n, events (window position, deletion?, length)
    ("no_events", 150, []),
    ("insertion_at_0", 150, [(0, 0, 2)]),
    ("insertion_at_n_minus_1", 150, [(149, 0, 3)]),
    ("leading_deletion", 150, [(0, 1, 4)]),
    ("trailing_deletion", 150, [(146, 1, 4)]),
    ("deletion_over_a_boundary", 150, [(60, 1, 30)]),
    ("two_deletions_insertion_between", 150, [(20, 1, 5), (70, 0, 4), (110, 1, 12)]),
    ("rollback_51", 51, [(10, 1, 2)]),
]
WIDTHS = [1, 37, 64, 150, 1000]


def positions(n, w, reverse):
    """Window starts (record coordinate of the leftmost window base) for width w: the window ends on a bin boundary, starts on one,
    lies in the record's last (short, when w does not divide the record) bin, touches the record's last base, and one in the middle."""
    last_bin = (REC_LEN - 1) // w * w
    lefts = {5 * w - n if 5 * w >= n else (n + w - 1) // w * w - n, 7 * w, min(last_bin, REC_LEN - n), REC_LEN - n, 3 * w + w // 2}
    return sorted((l + n - 1 if reverse else l) for l in lefts)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("name,n,events", EVENTS, ids=[e[0] for e in EVENTS])
def test_read_increments_match_pos_and_cigar(name, n, events, w):
    """depth_read (what k_depth runs per read) gives the `reads` bin of POS and, per bin, the bases the CIGAR's M operations align."""
    seen = 0
    for reverse in (False, True):
        for pos0 in positions(n, w, reverse):
            pos, cigar = pos_cigar(pos0, n, events, reverse)
            want_first, want = increments(pos, cigar, w)
            first, got = scssim_amd.depth_read_probe(pos0, n, events, reverse, rec_len=REC_LEN, bin_width=w)
            assert (first, got) == (want_first, want), (name, w, reverse, pos0, cigar)
            assert sum(b for _, b in got) == sum(int(l) for l, k in re.findall(r"(\d+)([MID])", cigar) if k == "M")
            seen += 1
    assert seen == 2 * len(positions(n, w, False))
    if name == "rollback_51":
        assert pos_cigar(0, n, events, False)[1] == "51M"
    if name == "leading_deletion":
        assert pos_cigar(1000, n, events, False) == (1004, "146M") and pos_cigar(1149, n, events, True) == (1000, "146M")


def test_bins_per_read_cover_one_two_and_many():
    """The grid reaches reads inside one bin, over two bins and over three or more."""
    counts = set()
    for w in WIDTHS:
        for pos0 in positions(150, w, False):
            counts.add(min(3, len(scssim_amd.depth_read_probe(pos0, 150, [], False, rec_len=REC_LEN, bin_width=w)[1])))
    assert counts == {1, 2, 3}
    first, got = scssim_amd.depth_read_probe(REC_LEN - 150, 150, [], False, rec_len=REC_LEN, bin_width=37)
    assert got[-1] == ((REC_LEN - 1) // 37, REC_LEN % 37) and first == (REC_LEN - 150) // 37   # the short last bin, filled to the record's last base


@pytest.mark.parametrize("events", [[(10, 0, 1), (5, 1, 2)], [(10, 1, 3), (11, 0, 1)], [(148, 1, 5)], [(150, 0, 1)], [(3, 0, 0)]],
                         ids=["out_of_order", "inside_a_deletion", "deletion_past_the_window", "insertion_past_the_window", "zero_length"])
def test_invalid_event_lists_are_refused(events):
    with pytest.raises(ScsError) as e:
        scssim_amd.depth_read_probe(5000, 150, events, False, rec_len=REC_LEN, bin_width=64)
    assert e.value.code == SCS_EINVAL


def test_reads_outside_the_record_are_refused():
    for pos0, rev in ((REC_LEN - 149, False), (148, True), (-1, False)):
        with pytest.raises(ScsError) as e:
            scssim_amd.depth_read_probe(pos0, 150, [], rev, rec_len=REC_LEN, bin_width=64)
        assert e.value.code == SCS_EINVAL
    assert scssim_amd.depth_read_probe(149, 150, [], True, rec_len=150, bin_width=64) == (0, [(0, 64), (1, 64), (2, 22)])


@pytest.mark.parametrize("w", [1, 37, 1000])
def test_layout_is_the_cumulative_sum_of_the_records_bins(w):
    lens = [5 * w, 5 * w + 1, max(1, w - 1), w, 1, 12345, 3 * w]
    off, n = scssim_amd.depth_layout_probe(lens, w)
    per = [-(-l // w) for l in lens]
    assert off.dtype == np.uint64 and off.tolist() == [0] + np.cumsum(per).tolist() and n == sum(per)


def test_layout_refuses_more_than_2_to_27_bins_and_names_the_width():
    """Lengths of 2^40 at W = 1: SCS_EINVAL at once, nothing of the bins' size is allocated; the message names the smallest width that fits."""
    with pytest.raises(ScsError) as e:
        scssim_amd.depth_layout_probe([1 << 40, 1 << 40, 5], 1)
    assert e.value.code == SCS_EINVAL
    m = re.search(r"smallest bin width these records admit is (\d+)", str(e.value))
    assert m, str(e.value)
    wmin = int(m.group(1))
    assert scssim_amd.depth_layout_probe([1 << 40, 1 << 40, 5], wmin)[1] <= 1 << 27
    with pytest.raises(ScsError):
        scssim_amd.depth_layout_probe([1 << 40, 1 << 40, 5], wmin - 1)
    assert scssim_amd.depth_layout_probe([1 << 27], 1)[1] == 1 << 27      # the cap itself is admitted
    with pytest.raises(ScsError):
        scssim_amd.depth_layout_probe([(1 << 27) + 1], 1)
    with pytest.raises(ScsError):
        scssim_amd.depth_layout_probe([100], 0)


def _cli(args):
    return subprocess.run([CLI, "genreads", "-i", "/nonexistent/genome.fa", "-m", "/nonexistent/m.profile", "-o", "/nonexistent/out"] + args,
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_come_before_any_gpu_work():
    """--depth with --gpus 2 and --depth-bin without --depth end the CLI with their own message before it touches a device (this
    machine has none) or an input file (these do not exist)."""
    r = _cli(["--depth", "/nonexistent/d.tsv", "--gpus", "2"])
    assert r.returncode != 0 and "--depth needs --gpus 1" in r.stderr, r.stderr
    r = _cli(["--depth-bin", "500"])
    assert r.returncode != 0 and "--depth-bin needs --depth" in r.stderr, r.stderr
    r = _cli(["--depth", "/nonexistent/d.tsv", "--depth-bin", "0"])
    assert r.returncode != 0 and "--depth-bin should be a positive integer" in r.stderr, r.stderr
    h = subprocess.run([CLI, "genreads", "-h"], capture_output=True, text=True, timeout=60)
    assert "--depth <string>" in h.stdout + h.stderr and "--depth-bin <int>" in h.stdout + h.stderr


def test_both_libraries_export_the_depth_abi():
    from conftest import SEAMS_LIB
    want = {"scs_set_depth", "scs_depth_bins", "scs_depth_record_bins", "scs_download_depth", "scs_write_depth", "scs_depth_layout_probe", "scs_depth_read_probe"}
    for lib in (os.path.join(ROOT, "scssim_amd", "libscssim_hip.so"), SEAMS_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert want <= set(l.split()[-1] for l in out.splitlines() if " T " in l), lib
    assert "k_depth" in scssim_amd.GenReads.KERNELS and scssim_amd.GenReads.KERNELS.index("k_depth") == 7
