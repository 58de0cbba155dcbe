#!/usr/bin/env python3
"""What the coverage profile costs: a chr20-size PE150 30x job (the genome and model of tools/depth_cost.py)
written to files on tmpfs with coverage off and with coverage on at max_depth 1000.  Prints one JSON line per leg and repeat: wall
seconds of the yield call and the library's HIP-event times of k_reads, k_depth and the two coverage passes -- the per-batch
marks (k_cov_mark, on the same batches as k_reads) and the end-of-job pass (three kernels, once).  `--lds 0` runs the legs in a
child process whose end-of-job pass has no LDS histogram (SCS_TEST_COV_LDS=0 in the seams build: every count is a 64-bit global
atomic) -- the A/B of the aggregation; `--lds 4096` is the product's table through the same build."""
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
        g.set_coverage(a.max_depth if leg == "on" else 0)
        t = time.time()
        g.yield_reads_files(os.path.join(td, "reads_" + leg), a.writers)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        rec = dict(leg=leg, lds=a.slots, max_depth=a.max_depth if leg == "on" else 0, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"],
                   k_reads=kt["k_reads"], k_depth=kt["k_depth"], k_cov_mark=g.coverage_kernel_time(0), k_cov_finish=g.coverage_kernel_time(1))
        if leg == "on":
            t = g.coverage()
            h = t["hist"][-1]
            rec.update(bases=int(h.sum()), n_bases=int(t["n_bases"][-1]), aligned=int(t["sum"][-1]) + int(t["sum_n"][-1]), top_bucket=int(h[-1]),
                       mark_over_reads=round(rec["k_cov_mark"]["ms"] / max(rec["k_reads"]["ms"], 1e-9), 4))
        cj.emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on", help="comma list of off, on")
    ap.add_argument("--max-depth", type=int, default=1000)
    ap.add_argument("--lds", dest="slots", type=int, default=None, help="buckets of the end-of-job pass' LDS histogram (the seams build; 0: none).  Default: the product build")
    cj.add_common(ap, repeats=2, writers=True)
    cj.run(ap.parse_args(), job, seam="SCS_TEST_COV_LDS")


if __name__ == "__main__":
    main()
