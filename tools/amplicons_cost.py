#!/usr/bin/env python3
"""What the amplicon table costs: the chr20-size PE150 30x job of tools/truth_cost.py with files on tmpfs.
Prints one JSON line per leg and repeat: wall seconds of scs_write_amplicons (plain, BGZF), the HIP-event time of its kernels,
the bytes written and the amplicons; beside them the wall seconds of scs_amplify and of scs_yield_reads_files on the same job and
box (`--legs yield` alone, run on a checkout of the parent commit, gives the parent's figures: it uses nothing the table adds)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402


def job(a, td):
    g = cj.open_ctx(a, td)
    g.create_frags()
    t = time.time(); g.amplify(); amplify_s = time.time() - t
    g.allocate_reads(0)
    st = g.stats()
    cj.emit(dict(leg="amplify", wall_s=round(amplify_s, 3), semis=st["semi_amplicons"], fulls=st["full_amplicons"]))
    legs = a.legs.split(",")
    if "yield" in legs:
        cj.warm_up(g, td)
    if "plain" in legs or "bgzf" in legs:
        g.write_amplicons(os.path.join(td, "amp_warm.tsv"))
    for leg in cj.legs(a, td, ("reads_", "amp_")):
        t = time.time()
        if leg == "yield":
            g.set_seed(220); g.yield_reads_files(os.path.join(td, "reads_" + leg), 1)
            rec = dict(leg=leg, wall_s=round(time.time() - t, 3), pairs=g.stats()["pairs_written"], k_reads=g.kernel_times()["k_reads"])
        else:
            n = g.write_amplicons(os.path.join(td, "amp_" + leg + (".tsv.gz" if leg == "bgzf" else ".tsv")), bgzf=leg == "bgzf")
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), bytes=n, kernels=g.amplicon_kernel_time(), mb_per_s=round(n / wall / 1e6, 1))
        cj.emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="yield,plain,bgzf", help="comma list of yield, plain, bgzf")
    cj.add_common(ap, repeats=3, warm="of each kind")
    cj.run(ap.parse_args(), job)


if __name__ == "__main__":
    main()
