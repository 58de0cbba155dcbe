"""The read allocation's kernels (scs_k_allocate.hip) on their own, over the case table of tests/alloc_cases.py: the fixed-shape sums
and scans (scs_alloc_sums_probe), the whole allocation behind the weights on one shard and on worlds of 2, 3 and 4 shards over gloo
(scs_alloc_probe), each compared bit for bit with the oracle's serial statement of the same rule (scso_tree_sum, scso_scan_all,
scso_allocate_reads).  tests/test_alloc_host.py proves on the CPU that the table reaches the branches it names.  One child process
per group (tests/alloc_gpu_worker.py) does the GPU work under a time limit of its own; every comparison runs here."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import alloc_cases as ac
from conftest import ROOT

import scssim_amd

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "alloc_gpu_worker.py")
SMALL = 64000                                                        # sizes up to here share one worker; each larger one has its own


def _run(mode, tmp_path_factory, timeout, *args):
    out = str(tmp_path_factory.mktemp("alloc_" + mode))
    t0 = time.time()
    r = subprocess.run([sys.executable, WORKER, mode, out] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print("%s (%.1f s)" % (r.stdout.strip().splitlines()[-1], time.time() - t0))
    return np.load(os.path.join(out, mode + ".npz")), json.load(open(os.path.join(out, mode + ".json")))


def _grouped(sizes, run):
    """size -> the output of the worker that ran it: one worker for the sizes up to SMALL, one per larger size, each run once"""
    cache = {}

    def get(n):
        group = tuple(s for s in sizes if s <= SMALL) if n <= SMALL else (n,)
        if group not in cache:
            cache[group] = run(group)
        return cache[group]
    return get


@pytest.fixture(scope="module")
def sums_run(tmp_path_factory):
    return _grouped(ac.SUM_SIZES, lambda group: _run("sums", tmp_path_factory, 300, *group))


@pytest.fixture(scope="module")
def one_run(tmp_path_factory, models):
    return _grouped(ac.ONE_SIZES, lambda group: _run("one", tmp_path_factory, 300, models["Illumina_HiSeq2500"], *group))


@pytest.fixture(scope="module")
def shard_run(tmp_path_factory, models):
    """(shards, hooks) -> per rank the output of that world's workers: every layout of that size and hook kind in one world, run once"""
    cache = {}

    def get(world, hooks):
        if (world, hooks) in cache:
            return cache[world, hooks]
        layouts = [n for n in ac.LAYOUTS if ac.LAYOUTS[n][0] == world and hooks in ac.LAYOUT_HOOKS[n]]
        out = str(tmp_path_factory.mktemp("alloc_shard"))
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = str(s.getsockname()[1]); s.close()
        procs, t0 = [], time.time()
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, LOCAL_RANK="0")
            procs.append(subprocess.Popen([sys.executable, WORKER, "shard", out, models["Illumina_HiSeq2500"], hooks] + layouts, env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=300)[0] for p in procs]
        assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
        print("%d shards, %s hooks, %s (%.1f s)" % (world, hooks, layouts, time.time() - t0))
        cache[world, hooks] = [(np.load(os.path.join(out, "shard.r%d.npz" % r)), json.load(open(os.path.join(out, "shard.r%d.json" % r)))) for r in range(world)]
        return cache[world, hooks]
    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_u32(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, "%s: %s %s, expected %s" % (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d entries differ, the first at %d (got %d, expected %d)" % (what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------- a. the fixed-shape sums and scans
@pytest.mark.parametrize("n", ac.SUM_SIZES)
def test_tree_sum_and_scan_all_equal_the_oracle_bit_for_bit(n, sums_run, oracle_lib):
    """launch_tree_sum and scan_all_dev over every family at n entries, with the scratch a job reserves for n chunks (the probe guards
    what lies behind it), against scso_tree_sum / scso_scan_all: every bit of every double."""
    res, _ = sums_run(n)
    for fam in ac.SUM_FAMILIES:
        v = ac.sum_values(fam, n)
        got, want = res["sum.%s.%d" % (fam, n)], np.array([ac.oracle_tree_sum(oracle_lib, v)])
        assert _bits(got).tolist() == _bits(want).tolist(), "tree_sum of %s at %d: got %r, the oracle has %r" % (fam, n, got[0], want[0])
        got, want = res["scan.%s.%d" % (fam, n)], ac.oracle_scan_all(oracle_lib, v)
        assert got.shape == want.shape
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, "scan_all of %s at %d: %d entries differ, the first at %d (got %r, the oracle has %r)" % (fam, n, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------- b. the whole allocation on one shard
def _check_allocation(rn, po, want, reads, paired, what):
    """read numbers and pair offsets against the oracle's numbers, and the properties of the rule beside them"""
    _same_u32(rn, want, what + ": read numbers")
    _same_u32(po, ac.pair_offsets(want, paired), what + ": pair offsets")
    total = int(rn.astype(np.uint64).sum())
    if paired:
        assert not (rn & 1).any(), what + ": an odd read number on a PE job"
        assert abs(total - reads) <= 1, "%s: %d reads allocated of %d" % (what, total, reads)
    else:
        assert total == reads, "%s: %d reads allocated of %d" % (what, total, reads)
    assert int(po[-1]) == (total // 2 if paired else total) % (1 << 32), what + ": the planned pair count"


@pytest.mark.parametrize("n", ac.ONE_SIZES)
def test_one_shard_allocation_equals_the_oracle(n, one_run, oracle_lib):
    """scs_alloc_probe over every family, read count and layout at n amplicons: rn == scso_allocate_reads, pair_off == the exclusive
    cumulative sum of rn (SE) or rn / 2 (PE) of the oracle's numbers; SE: sum(rn) == reads; PE: every rn even, |sum(rn) - reads| <= 1;
    pair_off[n] is the planned pair count."""
    res, _ = one_run(n)
    cases = ac.one_cases(n)
    assert len(cases) >= 12
    for fam, reads, paired in cases:
        key = ac.one_key(n, fam, reads, paired)
        want, _ = ac.oracle_allocate(oracle_lib, ac.weights(fam, n), reads, paired)
        _check_allocation(res[key + ".rn"], res[key + ".po"], want, reads, paired, key)


def test_a_probed_ctx_still_refuses_to_yield(one_run):
    """after every probe of the small sizes, both ctxs (SE, PE) are still not allocated: scs_yield_reads is refused by name"""
    _, meta = one_run(ac.ONE_SIZES[0])
    for p in ("0", "1"):
        m = meta["yield." + p]
        assert m.get("code") == scssim_amd.SCS_EINVAL and "scs_yield_reads: call scs_allocate_reads first" in m["error"], m


# ---------------------------------------------------------------- c. shards
@pytest.mark.parametrize("name,hooks", [(n, h) for n in ac.LAYOUTS for h in ac.LAYOUT_HOOKS[n]])
def test_sharded_allocation_equals_the_one_shard_oracle(name, hooks, shard_run, oracle_lib):
    """every rank of the layout's world runs scs_alloc_probe on its slice of the whole job's weights (collectives over gloo, through
    the host or the device hooks): the ranks' read numbers, put back in list order, are the oracle's over the whole vector, and each
    rank's pair_off is the cumulative sum of its own numbers."""
    world, _ = ac.LAYOUTS[name]
    ranks = shard_run(world, hooks)
    slices = ac.layout_slices(name)
    for fam, reads, paired in ac.layout_runs(name):
        w = ac.layout_weights(name, fam)
        want, _ = ac.oracle_allocate(oracle_lib, w, reads, paired)
        got = np.zeros(w.size, np.uint32)
        for r in range(world):
            key = ac.layout_key(name, hooks, fam, reads, paired, r)
            rn, po, at = ranks[r][0][key + ".rn"], ranks[r][0][key + ".po"], 0
            assert rn.size == sum(b - a for a, b in slices[r]), key
            for a, b in slices[r]:
                got[a:b] = rn[at:at + b - a]
                at += b - a
            _same_u32(po, ac.pair_offsets(rn, paired), key + ": pair offsets")
        what = "%s under %s hooks, %s, %d reads, %s" % (name, hooks, fam, reads, "PE" if paired else "SE")
        _check_allocation(got, ac.pair_offsets(got, paired), want, reads, paired, what)
    calls = ranks[0][1]["calls"]
    assert (calls["allreduce_dev"] > 0 and calls["allgather_dev"] > 0) if hooks == "device" else (calls["allreduce"] > 0 and calls["allgatherv"] > 0 and calls["allreduce_dev"] == 0), calls
