#!/usr/bin/env python3
"""What the artefact table on the original reference costs: the chr20-size PE150 30x job of tools/lift_cost.py
(the reference of tools/make_genome.py through scs_simuvars with that tool's variation file), files on tmpfs.  Prints one JSON line
per leg and repeat: wall seconds of the call, the HIP-event time of its kernels (the library sorts and scans included), the sites
and bytes written.  Legs: art0 = scs_write_artefacts (the yardstick), ref0 / ref1 / ref0_bgzf / ref1_bgzf = scs_write_artefacts_ref
at min_reads 0 and 1, plain and BGZF.  --parent-lib PATH: the parent commit's library runs art0 on the same job before and after,
each in a process of its own (a library is loaded once per process)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402

LEGS = {"ref0": (0, False), "ref1": (1, False), "ref0_bgzf": (0, True), "ref1_bgzf": (1, True)}


def job(a, td):
    lib = os.environ.get("SCSSIM_HIP_LIB") and "parent" or "this tree"
    g, ref, var = cj.open_ctx(a, td, True, a.cnvs, a.indels)
    t = time.time()
    g.simuvars(ref, None, var)
    head = dict(leg="simuvars", wall_s=round(time.time() - t, 3), staged_bases=g.stats()["genome_bases"], segments=g.lift_info()[0])
    cj.allocate(g)
    head.update(fulls=g.stats()["full_amplicons"])
    cj.emit(head, a.log, lib)
    g.write_artefacts(os.path.join(td, "art_warm.vcf"))                      # warm-up of each kind: the buffers, the page cache
    if any(l in LEGS for l in a.legs.split(",")):
        g.write_artefacts_ref(os.path.join(td, "art_warm_ref.vcf"))
    for leg in cj.legs(a, td, ("art_",)):
        t = time.time()
        if leg in LEGS:
            min_reads, bgzf = LEGS[leg]
            r = g.write_artefacts_ref(os.path.join(td, "art_" + leg + (".vcf.gz" if bgzf else ".vcf")), bgzf=bgzf, min_reads=min_reads)
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), kernels=g.artefact_ref_kernel_time(), **r)
        else:
            r = g.write_artefacts(os.path.join(td, "art_" + leg + ".vcf"))
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), kernels=g.artefact_kernel_time(), **r)
        cj.emit(rec, a.log, lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="art0,ref0,ref1,ref0_bgzf,ref1_bgzf", help="comma list of art0, ref0, ref1, ref0_bgzf, ref1_bgzf")
    cj.add_common(ap, repeats=3, warm="of each kind", simuvars=True)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libscssim_hip.so: it runs --legs art0 before and after this tree's legs")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/artefacts_ref_cost_*.log)")
    cj.run(ap.parse_args(), job, parent_legs="art0")


if __name__ == "__main__":
    main()
