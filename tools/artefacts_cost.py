#!/usr/bin/env python3
"""What the artefact table costs: the chr20-size PE150 30x job of tools/amplicons_cost.py with files on tmpfs.
Prints one JSON line per leg and repeat: wall seconds of scs_write_artefacts at min_reads 0 and 1, plain and BGZF, the HIP-event
time of its kernels (the library sorts and scans included), the sites and bytes written; beside them scs_write_amplicons (plain,
BGZF) on the same job and tree, which is what the call is expected not to exceed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402

LEGS = {"art0": (0, False), "art1": (1, False), "art0_bgzf": (0, True), "art1_bgzf": (1, True)}


def job(a, td):
    g = cj.open_ctx(a, td)
    g.create_frags()
    t = time.time(); g.amplify(); amplify_s = time.time() - t
    g.allocate_reads(0)
    st = g.stats()
    cj.emit(dict(leg="amplify", wall_s=round(amplify_s, 3), semis=st["semi_amplicons"], fulls=st["full_amplicons"]))
    g.write_artefacts(os.path.join(td, "art_warm.vcf"))                      # warm-up of each kind: the buffers, the page cache
    g.write_amplicons(os.path.join(td, "amp_warm.tsv"))
    for leg in cj.legs(a, td, ("art_", "amp_")):
        t = time.time()
        if leg in LEGS:
            min_reads, bgzf = LEGS[leg]
            r = g.write_artefacts(os.path.join(td, "art_" + leg + (".vcf.gz" if bgzf else ".vcf")), bgzf=bgzf, min_reads=min_reads)
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), sites=r["sites"], bytes=r["bytes"], kernels=g.artefact_kernel_time())
        else:
            n = g.write_amplicons(os.path.join(td, "amp_" + leg + (".tsv.gz" if leg == "amp_bgzf" else ".tsv")), bgzf=leg == "amp_bgzf")
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), bytes=n, kernels=g.amplicon_kernel_time())
        cj.emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="art0,art1,art0_bgzf,art1_bgzf,amp,amp_bgzf", help="comma list of art0, art1, art0_bgzf, art1_bgzf, amp, amp_bgzf")
    cj.add_common(ap, repeats=3, warm="of each kind")
    cj.run(ap.parse_args(), job)


if __name__ == "__main__":
    main()
