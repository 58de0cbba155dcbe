#!/usr/bin/env python3
"""What the depth track by reference bin costs: a chr20-size PE150 30x job whose genome comes from
scs_simuvars -- the reference of tools/make_genome.py and a variation file of a few hundred CNVs and indels (tools/cost_job.py: write_variations) -- written to
files on tmpfs with both depth tracks off, with the haplotype track (--depth), with the reference track (--depth-ref) and with
both.  Prints one JSON line per leg and repeat: wall seconds of the yield call and the library's HIP-event times of k_reads,
k_depth and k_depth_lift on the same batches; --log FILE also appends them there (profiles/).  `--slots 0` runs the legs in a
child process whose k_depth_lift has no LDS table (SCS_TEST_LIFT_SLOTS=0 in the seams build: every add is a global atomic) -- the
A/B of the aggregation; `--slots 512` is the product's table through the same build.  `--legs off` runs on a library without the
feature too (SCSSIM_HIP_LIB = the parent commit's build): the yield time with the feature off against the parent's, back to back."""
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
    have = hasattr(g, "lift_info") and hasattr(g._L, "scs_lift_info")
    cj.emit(dict(leg="simuvars", wall_s=round(time.time() - t, 3), staged_bases=g.stats()["genome_bases"], segments=g.lift_info()[0] if have else None), a.log, lib)
    cj.allocate(g)
    cj.warm_up(g, td, a.writers)
    for leg in cj.legs(a, td):
        g.set_depth(a.bin if leg in ("depth", "both") else 0)
        if have:
            g.set_depth_ref(a.bin if leg in ("ref", "both") else 0)
        t = time.time()
        g.yield_reads_files(os.path.join(td, "reads_" + leg), a.writers)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        rec = dict(leg=leg, slots=a.slots, bin=a.bin, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"], k_reads=kt["k_reads"], k_depth=kt["k_depth"],
                   k_depth_lift=g.depth_ref_kernel_time() if have else None)
        if leg in ("ref", "both"):
            r, b, c, _ = g.depth_ref()
            rec.update(bins=int(r.size) - 1, reads_sum=int(r.sum()), bases_sum=int(b.sum()), unlifted_reads=int(r[-1]), unlifted_bases=int(b[-1]), copies_sum=int(c[:-1].sum()), inserted=int(c[-1]))
            assert rec["reads_sum"] == st["reads_written"] and rec["copies_sum"] + rec["inserted"] == st["genome_bases"]
        cj.emit(rec, a.log, lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,depth,ref,both", help="comma list of off, depth, ref, both")
    ap.add_argument("--bin", type=int, default=1000)
    cj.add_common(ap, repeats=3, slots="k_depth_lift", writers=True, simuvars=True)
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/lift_cost_*.log)")
    cj.run(ap.parse_args(), job, seam="SCS_TEST_LIFT_SLOTS")


if __name__ == "__main__":
    main()
