#!/usr/bin/env python3
"""What the depth track costs: a chr20-size PE150 30x job (the genome and model of tools/truth_cost.py)
written to files on tmpfs with depth off and with depth on at 1000-base bins.  Prints one JSON line per leg and repeat: wall
seconds of the yield call and the library's HIP-event times of k_reads and k_depth on the same batches.  `--slots 0` runs the
depth legs in a child process whose kernel has no LDS table (SCS_TEST_DEPTH_SLOTS=0 in the seams build: every add is a global
atomic) -- the A/B of the aggregation; `--slots 512` is the product's table through the same build."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402


def job(a, td):
    g = cj.open_ctx(a, td)
    cj.allocate(g)
    cj.warm_up(g, td, a.writers)
    for leg in cj.legs(a, td):
        g.set_depth(a.bin if leg == "on" else 0)
        t = time.time()
        g.yield_reads_files(os.path.join(td, "reads_" + leg), a.writers)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        rec = dict(leg=leg, slots=a.slots, bin=a.bin if leg == "on" else 0, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"],
                   k_reads=kt["k_reads"], k_depth=kt["k_depth"])
        if leg == "on":
            r, b, _ = g.depth()
            rec.update(bins=int(r.size), reads_sum=int(r.sum()), bases_sum=int(b.sum()), reads_max=int(r.max()))
            assert rec["reads_sum"] == st["reads_written"]
        cj.emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on", help="comma list of off, on")
    ap.add_argument("--bin", type=int, default=1000)
    cj.add_common(ap, repeats=2, slots="the kernel", writers=True)
    cj.run(ap.parse_args(), job, seam="SCS_TEST_DEPTH_SLOTS")


if __name__ == "__main__":
    main()
