#!/usr/bin/env python3
"""What the coverage profile on the reference costs: the chr20-size PE150 30x simuvars job of
tools/lift_cost.py written to files on tmpfs with both profiles off, with the staged profile alone (--coverage-profile), with the
reference profile alone (--coverage-profile-ref) and with both.  Prints one JSON line per leg and repeat: wall seconds of the yield
call and the library's HIP-event times of k_reads, of the per-batch marks (k_cov_mark), of the staged end-of-job pass, of the new
end-of-job kernels (k_cov_ref_lift + k_cov_ref_hist) and of the once-per-layout kernel (k_cov_ref_copies: launched in the first
yield after the switch went on, none while the layout stands); --log FILE also appends them there (profiles/).  `--lds 0` runs the
legs in a child process whose two count kernels have no LDS histogram (SCS_TEST_COV_LDS=0 in the seams build)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402


def job(a, td):
    lib = os.path.basename(os.environ.get("SCSSIM_HIP_LIB") or "libscssim_hip.so")
    g, ref, var = cj.open_ctx(a, td, True, a.cnvs, a.indels)
    t = time.time()
    g.simuvars(ref, None, var)
    cj.emit(dict(leg="simuvars", wall_s=round(time.time() - t, 3), staged_bases=g.stats()["genome_bases"], segments=g.lift_info()[0]), a.log, lib)
    cj.allocate(g)
    cj.warm_up(g, td, a.writers)
    for leg in cj.legs(a, td):
        g.set_coverage(a.max_depth if leg in ("staged", "both") else 0)
        g.set_coverage_ref(a.max_depth if leg in ("ref", "both") else 0)
        t = time.time()
        g.yield_reads_files(os.path.join(td, "reads_" + leg), a.writers)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        rec = dict(leg=leg, lds=a.slots, max_depth=a.max_depth, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"], k_reads=kt["k_reads"],
                   k_cov_mark=g.coverage_kernel_time(0), k_cov_finish=g.coverage_kernel_time(1), k_cov_ref_copies=g.coverage_ref_kernel_time(0), k_cov_ref_finish=g.coverage_ref_kernel_time(1))
        if leg in ("ref", "both"):
            tb = g.download_coverage_ref()
            rec.update(ref_bases=int(tb["hist"][-1].sum()) + int(tb["n_bases"][-1]), absent=int(tb["absent"][-1]), aligned=int(tb["sum"][-1]) + int(tb["sum_n"][-1]), unlifted=tb["unlifted"],
                       top_bucket=int(tb["hist"][-1][-1]), mean_by_cn=[round(int(s) / int(b), 3) if b else None for s, b in zip(tb["cn_sum"][-1], tb["cn_bases"][-1])],
                       ref_over_staged_finish=round(rec["k_cov_ref_finish"]["ms"] / max(rec["k_cov_finish"]["ms"], 1e-9), 3))
        cj.emit(rec, a.log, lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,staged,ref,both", help="comma list of off, staged, ref, both")
    ap.add_argument("--max-depth", type=int, default=1000)
    ap.add_argument("--lds", dest="slots", type=int, default=None, help="buckets of the count kernels' LDS histogram (the seams build; 0: none).  Default: the product build")
    cj.add_common(ap, repeats=3, writers=True, simuvars=True)
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/coverage_ref_cost_*.log)")
    cj.run(ap.parse_args(), job, seam="SCS_TEST_COV_LDS")


if __name__ == "__main__":
    main()
