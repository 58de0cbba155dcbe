"""The BGZF kernels (scs_bgzf.hip) and the small scan (k_scan_small, scs_k_misc.hip) ON THE DEVICE over inputs that FASTQ text never
gives them: tests/bgzf_cases.py (short inputs, one symbol, ties, all 256 literals, trees deeper than 15, stored blocks for both
reasons, the LDS cap from both sides, mixed neighbours at every dst & 3) through scs_bgzf_device_probe, and the scan at its edge
sizes through scs_scan_probe.  References: zlib (inflate with CRC-32 and ISIZE checked) and numpy.cumsum; the device's BGZF bytes
must also equal the host emulation's (scs_bgzf_probe), which pins sizes, offsets and the stored-or-deflated decision per block.
One child process per probe does all the GPU work and writes what it got to files; every check runs here."""
import json
import os
import zlib

import numpy as np
import pytest

import bgzf_cases as bc
from gpu_child import run_child

import scssim_amd

pytestmark = pytest.mark.gpu

_BGZF_CHILD = r'''
import json, os
import scssim_amd, bgzf_cases as bc
from gpu_child import job_args
out, guards = job_args()["out"], {}
for name in bc.CASES:
    for zbase in bc.ZBASES[name]:
        z, ok = scssim_amd.bgzf_device_probe(bc.data(name), zbase)
        open(os.path.join(out, "%s.z%d.bin" % (name, zbase)), "wb").write(z)
        guards["%s.z%d" % (name, zbase)] = ok
json.dump(guards, open(os.path.join(out, "guards.json"), "w"))
print("bgzf child ok")
'''

_SCAN_CHILD = r'''
import numpy as np
import scssim_amd, bgzf_cases as t
from gpu_child import job_args
res = {}
for kind in ("small", "full"):
    for n in t.SCAN_SIZES:
        res["alone.%s.%d" % (kind, n)] = scssim_amd.scan_probe(t.scan_input(n, kind))
        o0, o1 = scssim_amd.scan_probe(t.scan_input(t.scan_partner(n), kind, 1), t.scan_input(n, kind))
        res["pair0.%s.%d" % (kind, n)], res["pair1.%s.%d" % (kind, n)] = o0, o1
    for tag, n0, n1 in (("n1_zero", 1000, 0), ("n0_zero", 0, 1000), ("both_zero", 0, 0)):
        o0, o1 = scssim_amd.scan_probe(t.scan_input(n0, kind, 2), t.scan_input(n1, kind, 3))
        res["%s0.%s" % (tag, kind)], res["%s1.%s" % (tag, kind)] = o0, o1
np.savez(job_args()["out"], **res)
print("scan child ok")
'''


@pytest.fixture(scope="module")
def device_bgzf(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bgzf_dev"))
    run_child(_BGZF_CHILD, dict(out=out), timeout=900, ok=True)
    return out, json.load(open(os.path.join(out, "guards.json")))


@pytest.fixture(scope="module")
def device_scan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scan_dev") / "scan.npz")
    run_child(_SCAN_CHILD, dict(out=out), timeout=600, ok=True)
    return np.load(out)


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return int(d[0]) if d.size else n


def check_case(name, outputs, guards):
    """outputs[zbase]: the device's bytes for the case, guards[zbase]: the probe's guards_ok"""
    data = bc.data(name)
    want = scssim_amd.bgzf_probe(data)
    for zbase in bc.ZBASES[name]:
        tag, z = "%s.z%d" % (name, zbase), outputs[zbase]
        where = ""
        if z != want:
            o = _first_diff(z, want)
            sizes = np.cumsum([len(b) for b, _ in scssim_amd.bgzf_blocks(want)])
            blk = int(np.searchsorted(sizes, o, side="right"))
            where = "%s: %d device bytes, %d expected; first difference at byte %d = block %d + %d" % (tag, len(z), len(want), o, blk, o - (int(sizes[blk - 1]) if blk else 0))
        blocks = scssim_amd.bgzf_blocks(z)
        assert len(blocks) == (len(data) + bc.BGZF_IN - 1) // bc.BGZF_IN, (tag, where)
        assert [i for _, i in blocks] == bc.cut(data), (tag, where)
        for k, (b, _) in enumerate(blocks):
            try:
                plain = zlib.decompress(b, 31)
            except zlib.error as e:
                pytest.fail("%s: zlib rejects block %d (%s); %s" % (tag, k, e, where))
            assert plain == data[k * bc.BGZF_IN:(k + 1) * bc.BGZF_IN], "%s: block %d inflates to other bytes; %s" % (tag, k, where)
        assert z == want, "zlib accepts every block, the emulation differs: " + where
        assert guards[zbase] is True, "%s: a guard byte around the output was overwritten" % tag


@pytest.mark.parametrize("name", list(bc.CASES))
def test_device_bgzf_inflates_with_zlib_and_equals_the_emulation(name, device_bgzf):
    """Every case of the table, at every zbase in 0..3 (big_text: 0): the device's output is framed into ceil(n / 64512) BGZF blocks
    whose ISIZEs are the input's cut; zlib inflates every block (gzip framing: CRC-32 and ISIZE verified) to its part of the input;
    the bytes equal the host emulation's; no guard byte around the output was touched.  On a mismatch the message names the
    block, the offset, and whether zlib rejected the block or only the emulation differs."""
    out, guards = device_bgzf
    check_case(name, {zb: open(os.path.join(out, "%s.z%d.bin" % (name, zb)), "rb").read() for zb in bc.ZBASES[name]},
               {zb: guards["%s.z%d" % (name, zb)] for zb in bc.ZBASES[name]})


def _scan_ref(a):
    ref = np.concatenate([np.zeros(1, np.uint64), np.cumsum(a.astype(np.uint64), dtype=np.uint64)])     # (a list's [0] would make it float64)
    assert ref.dtype == np.uint64
    return ref & np.uint64(0xFFFFFFFF)


def _scan_eq(got, a, what):
    ref = _scan_ref(a)
    assert got.dtype == np.uint32 and got.shape == ref.shape, what
    bad = np.flatnonzero(got.astype(np.uint64) != ref)
    assert bad.size == 0, "%s: %d of %d entries differ, the first at %d (got %d, expected %d)" % (what, bad.size, ref.size, bad[0], got[bad[0]], ref[bad[0]])


@pytest.mark.parametrize("kind", ["small", "full"])
@pytest.mark.parametrize("n", bc.SCAN_SIZES)
def test_device_scan_equals_cumsum(n, kind, device_scan):
    """exclusive_scan_u32 / exclusive_scan_u32_pair at the edge sizes of k_scan_small (uint4 tiles, per-wave segments; 262144 is the
    last size of the one-workgroup path, 262145 the first of rocPRIM's) against numpy.cumsum in uint64 masked to 32 bits, all
    n + 1 entries exactly: values below 2^12 (below 2^16, and no sum wraps) and full-range ones (sums wrap), each size alone and as the second array of
    a pair whose first array has another size (a pair with one array above the switch takes two separate scans)."""
    assert bc.scan_partner(n) != n
    if kind == "small":
        assert int(bc.scan_input(n, kind).sum(dtype=np.uint64)) < 1 << 32
    _scan_eq(device_scan["alone.%s.%d" % (kind, n)], bc.scan_input(n, kind), "alone")
    _scan_eq(device_scan["pair1.%s.%d" % (kind, n)], bc.scan_input(n, kind), "second of a pair")
    _scan_eq(device_scan["pair0.%s.%d" % (kind, n)], bc.scan_input(bc.scan_partner(n), kind, 1), "first of a pair (%d)" % bc.scan_partner(n))


@pytest.mark.parametrize("kind", ["small", "full"])
def test_device_scan_pairs_with_an_empty_array(kind, device_scan):
    """n1 == 0 (out1[0] == 0), n0 == 0, and both"""
    for tag, n0, n1 in (("n1_zero", 1000, 0), ("n0_zero", 0, 1000), ("both_zero", 0, 0)):
        _scan_eq(device_scan["%s0.%s" % (tag, kind)], bc.scan_input(n0, kind, 2), tag + " first")
        _scan_eq(device_scan["%s1.%s" % (tag, kind)], bc.scan_input(n1, kind, 3), tag + " second")
    assert device_scan["n1_zero1.%s" % kind].tolist() == [0] and device_scan["n0_zero0.%s" % kind].tolist() == [0]
