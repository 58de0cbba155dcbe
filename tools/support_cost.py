#!/usr/bin/env python3
"""What the site support costs: the chr20-size PE150 30x job of tools/truth_cost.py written to files on tmpfs
on one ctx, with the site support off and on at min_reads 1 and 0.  Prints one JSON line per leg and repeat: wall seconds of the
yield call (the site table's build is part of it), the library's HIP-event times of k_reads and k_support on the same batches, the
sites, the positions the reads touched and the sums of the counters.  `--slots 0` runs the legs in a child process whose kernel
has no LDS table (SCS_TEST_SUPPORT_SLOTS=0 in the seams build: every add is a global atomic) -- the A/B of the aggregation;
`--slots 1024` is the product's table through the same build."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402

LEGS = {"off": None, "on1": 1, "on0": 0}


def job(a, td):
    g = cj.open_ctx(a, td)
    cj.allocate(g)
    cj.warm_up(g, td, a.writers)
    for leg in cj.legs(a, td):
        g.set_site_support(LEGS[leg] is not None, LEGS[leg] or 0)
        t = time.time()
        g.yield_reads_files(os.path.join(td, "reads_" + leg), a.writers)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        rec = dict(leg=leg, slots=a.slots, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"], k_reads=kt["k_reads"], k_support=g.site_support_kernel_time())
        if LEGS[leg] is not None:
            z = g.site_support()
            c = z["counts"]
            rec.update(sites=int(len(z["na"])), seen=int((c[:, :5].sum(axis=1) > 0).sum()), alt_seen=int((c[range(len(c)), z["alt"].astype(int)] > 0).sum()),
                       depth_sum=int(c[:, :5].sum()), deleted_sum=int(c[:, 5].sum()))
            t = time.time()
            w = g.write_site_support(os.path.join(td, "reads_sup.vcf"))
            rec.update(write_s=round(time.time() - t, 3), bytes=w["bytes"])
        cj.emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on1,on0", help="comma list of off, on1 (min_reads 1), on0 (min_reads 0)")
    cj.add_common(ap, repeats=3, slots="the kernel", writers=True)
    cj.run(ap.parse_args(), job, seam="SCS_TEST_SUPPORT_SLOTS")


if __name__ == "__main__":
    main()
