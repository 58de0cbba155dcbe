#!/usr/bin/env python3
"""What the site support on the original reference costs: the chr20-size PE150 30x job of tools/lift_cost.py
(the reference of tools/make_genome.py through scs_simuvars with that tool's variation file) written to files on tmpfs on one ctx.
Prints one JSON line per leg and repeat: wall seconds of the yield call (the site table's build and the expansion are part of it),
the library's HIP-event times of k_reads and k_support on the same batches and, with the table on the reference on, of the
expansion behind the site table and of the gather, the sites, the positions k_support counted at and the sums of the counters.
Legs: off; sup0 = --support at min_reads 0; ref0 / ref1 = --support-ref at min_reads 0 and 1; art0 / art1 = scs_write_artefacts_ref
at the same min_reads (the kernels the open step's site table runs, timed by a call of their own).
--parent-lib PATH: the parent commit's library runs the legs off and sup0 on the same job before and after, each in a process of
its own (a library is loaded once per process)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402

LEGS = {"off": None, "sup0": ("hap", 0), "ref0": ("ref", 0), "ref1": ("ref", 1), "art0": ("art", 0), "art1": ("art", 1)}


def job(a, td):
    lib = os.environ.get("SCSSIM_HIP_LIB") and "parent" or "this tree"
    g, ref, var = cj.open_ctx(a, td, True, a.cnvs, a.indels)
    g.simuvars(ref, None, var)
    cj.allocate(g)
    cj.emit(dict(leg="job", staged_bases=g.stats()["genome_bases"], segments=g.lift_info()[0], fulls=g.stats()["full_amplicons"]), a.log, lib)
    cj.warm_up(g, td, a.writers)
    for leg in cj.legs(a, td):
        kind, min_reads = LEGS[leg] or (None, 0)
        if kind == "art":
            t = time.time()
            r = g.write_artefacts_ref(os.path.join(td, "reads_art.vcf"), min_reads=min_reads)
            rec = dict(leg=leg, wall_s=round(time.time() - t, 3), kernels=g.artefact_ref_kernel_time(), sites=r["sites"])
        else:
            g.set_site_support(False)
            if kind == "ref":
                g.set_site_support_ref(True, min_reads)
            elif kind == "hap":
                g.set_site_support(True, min_reads)
            t = time.time()
            g.yield_reads_files(os.path.join(td, "reads_" + leg), a.writers)
            wall = time.time() - t
            st, kt = g.stats(), g.kernel_times()
            rec = dict(leg=leg, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"], k_reads=kt["k_reads"], k_support=g.site_support_kernel_time())
            if kind:
                z = g.site_support_ref() if kind == "ref" else g.site_support()
                c = z["counts"]
                rec.update(sites=int(len(z["na"])), seen=int((c[:, :5].sum(axis=1) > 0).sum()), depth_sum=int(c[:, :5].sum()), deleted_sum=int(c[:, 5].sum()))
            if kind == "ref":
                rec.update(k_open=g.site_support_ref_kernel_time(0), k_gather=g.site_support_ref_kernel_time(1))
                t = time.time()
                w = g.write_site_support_ref(os.path.join(td, "reads_sup.vcf"))
                rec.update(write_s=round(time.time() - t, 3), bytes=w["bytes"])
                g.set_site_support_ref(False)
        cj.emit(rec, a.log, lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,sup0,ref0,ref1,art0,art1", help="comma list of off, sup0, ref0, ref1, art0, art1")
    cj.add_common(ap, repeats=3, writers=True, simuvars=True)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libscssim_hip.so: it runs --legs off,sup0 before and after this tree's legs")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/support_ref_cost_*.log)")
    cj.run(ap.parse_args(), job, parent_legs="off,sup0")


if __name__ == "__main__":
    main()
