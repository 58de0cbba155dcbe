"""Worker for tests/test_gpu_alloc.py: all the GPU work of one group of its tests in a process of its own; what the allocation's
kernels computed goes to <out>/<mode>.npz (and <out>/<mode>.json), every comparison runs in the test.
  sums OUT N...             scs_alloc_sums_probe over every family of tests/alloc_cases.py at these sizes: sum.<family>.<n>, scan.<family>.<n>
  one OUT PROFILE N...      scs_alloc_probe over every one-shard case of these sizes (largest first: a smaller case lies in buffers a larger
                            one has filled), one ctx per layout; then a yield on the probed ctx, whose refusal is recorded
  shard OUT PROFILE HOOKS LAYOUT...   one rank (RANK / WORLD_SIZE, gloo) of a sharded world: its slice of every run of these layouts
                            through scs_alloc_probe, under the host or the device hooks; <out>/shard.r<rank>.npz"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import alloc_cases as ac
import scssim_amd


def sums(out, res, meta, *sizes):
    for n in (int(x) for x in sizes):
        for fam in ac.SUM_FAMILIES:
            v = ac.sum_values(fam, n)
            res["sum.%s.%d" % (fam, n)] = np.array([scssim_amd.alloc_sums_probe(v, 0)])
            res["scan.%s.%d" % (fam, n)] = scssim_amd.alloc_sums_probe(v, 1)
    meta["cases"] = len(res)


def whole(n):
    """the segment table of one shard that holds all n amplicons in slot 0"""
    seg = np.zeros(ac.SLOTS, np.uint32)
    seg[0] = n
    return seg


def one(out, res, meta, profile, *sizes):
    ctx = {p: scssim_amd.GenReads(profile=profile, layout="PE" if p else "SE", seed=ac.SEED) for p in (0, 1)}
    for n in sorted((int(x) for x in sizes), reverse=True):
        for fam, reads, paired in ac.one_cases(n):
            rn, po = ctx[paired].alloc_probe(ac.weights(fam, n), whole(n), reads)
            key = ac.one_key(n, fam, reads, paired)
            res[key + ".rn"], res[key + ".po"] = rn, po
    for p, g in ctx.items():
        try:
            g.yield_reads(collect=False)
            meta["yield.%d" % p] = dict(error=None)
        except scssim_amd.ScsError as e:
            meta["yield.%d" % p] = dict(error=str(e), code=e.code)
        g.close()
    meta["cases"] = len(res) // 2


def shard(out, res, meta, profile, hooks, *layouts):
    import torch
    import torch.distributed as dist
    from scssim_amd.dist import Collectives
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, world = dist.get_rank(), dist.get_world_size()
    stream = torch.cuda.Stream()
    coll = Collectives(device="cpu", stream=stream)
    ctx = {}
    for p in (0, 1):
        ctx[p] = scssim_amd.GenReads(profile=profile, layout="PE" if p else "SE", seed=ac.SEED, device=0, stream=stream.cuda_stream, shard_rank=rank, shard_count=world)
        ctx[p].set_collectives(coll, device_hooks=(hooks == "device"))
    for name in layouts:
        assert ac.LAYOUTS[name][0] == world
        seg = ac.layout_counts(name)[rank].astype(np.uint32)
        for fam, reads, paired in ac.layout_runs(name):
            rn, po = ctx[paired].alloc_probe(ac.local_weights(name, fam, rank), seg, reads)
            key = ac.layout_key(name, hooks, fam, reads, paired, rank)
            res[key + ".rn"], res[key + ".po"] = rn, po
    meta["calls"] = coll.calls
    dist.barrier()
    for g in ctx.values():
        g.close()
    dist.destroy_process_group()
    return "shard.r%d" % rank


def main():
    mode, out = sys.argv[1:3]
    res, meta = {}, {}
    name = dict(sums=sums, one=one, shard=shard)[mode](out, res, meta, *sys.argv[3:]) or mode
    np.savez(os.path.join(out, name + ".npz"), **res)
    with open(os.path.join(out, name + ".json"), "w") as f:
        json.dump(meta, f)
    print("alloc worker %s: %d arrays with library %s" % (name, len(res), os.path.basename(scssim_amd.lib_path())))


if __name__ == "__main__":
    main()
