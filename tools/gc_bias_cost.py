#!/usr/bin/env python3
"""What the GC-bias table costs: the chr20-size PE150 30x job of tools/cost_job.py written to files on tmpfs
with coverage on at max_depth 1000, then the table made at windows of 100 and 1024 bases.  Prints one JSON line per repeat: the
library's HIP-event time of the GC-bias kernel per window (scs_gc_bias_kernel_time) beside the end-of-job coverage pass of the same
yield call (scs_coverage_kernel_time(1)), the yardstick: it reads the same two arrays once and stores one of them.  After the last
repeat one line with the genome's curve at a window of 100 (normalized beside model for every bin with windows, read back from
write_gc_bias's file), and, unless --no-probe, lines for the kernel alone over the job's own arrays (downloaded, and uploaded again
by scs_gc_bias_probe) with the LDS table (lds -1, the product's choice) and without it (lds 0: every add a global atomic) -- the A/B
of the aggregation."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402

WINDOWS = (100, 1024)


def codes_of_fasta(path):
    """(codes uint8, record lengths) of a FASTA: ACGT = 0 .. 3 in either case, anything else 4"""
    import numpy as np
    lut = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = lut[ch + 32] = i
    parts, lens = [], []
    for rec in open(path, "rb").read().split(b">")[1:]:
        seq = np.frombuffer(rec[rec.index(b"\n") + 1:], np.uint8)
        seq = seq[(seq != 10) & (seq != 13)]
        parts.append(lut[seq]); lens.append(seq.size)
    return np.concatenate(parts), lens


def job(a, td):
    import scssim_amd
    g = cj.open_ctx(a, td)
    cj.allocate(g)
    cj.warm_up(g, td)
    g.set_coverage(a.max_depth)
    for rep in range(a.repeats + 1):                        # (the first one warms the table's buffer and the kernel's code up: not recorded)
        t = time.time()
        g.yield_reads_files(os.path.join(td, "reads_on"), 1)
        wall = time.time() - t
        rec = dict(leg="job", repeat=rep, wall_s=round(wall, 3), pairs=g.stats()["pairs_written"], k_cov_finish=g.coverage_kernel_time(1))
        for W in WINDOWS:
            t = time.time()
            tab = g.gc_bias(W)
            rec["w%d" % W] = dict(g.gc_bias_kernel_time(), call_s=round(time.time() - t, 4), windows=int(tab["windows"][-1].sum()), n_windows=int(tab["n_windows"][-1]),
                                  over_finish=round(g.gc_bias_kernel_time()["ms"] / max(rec["k_cov_finish"]["ms"], 1e-9), 3))
        if rep:
            cj.emit(rec)
        for f in os.listdir(td):
            if f.startswith("reads_on"):
                os.unlink(os.path.join(td, f))
    path = os.path.join(td, "gc_bias.txt")
    g.write_gc_bias(path, 100)
    rows = [ln.split("\t") for ln in open(path).read().split("\n") if ln.startswith("genome\t")]
    cj.emit(dict(leg="curve", window=100, rows=[dict(gc=int(r[1]), windows=int(r[2]), mean_depth=float(r[4]), normalized=float(r[5]), model=r[6]) for r in rows]))
    if a.no_probe:
        return
    import numpy as np
    codes, lens = codes_of_fasta(os.path.join(td, "chr20.fa"))
    depth = np.concatenate([g.coverage_range(r, 0, n) for r, n in enumerate(lens)])
    want = {W: g.gc_bias(W) for W in WINDOWS}
    for rep in range(a.repeats + 1):
        for W in WINDOWS:
            for lds in (-1, 0):
                tab = scssim_amd.gc_bias_probe(g, depth, codes, lens, W, lds)
                assert all((tab[k] == want[W][k][:-1]).all() for k in tab), (W, lds)      # (the probe has no genome row)
                if rep:
                    cj.emit(dict(leg="probe", repeat=rep, window=W, lds=lds, **g.gc_bias_kernel_time()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-depth", type=int, default=1000)
    ap.add_argument("--no-probe", action="store_true", help="skip the kernel alone with and without its LDS table")
    cj.add_common(ap, repeats=3, warm="yield and table")
    cj.run(ap.parse_args(), job)


if __name__ == "__main__":
    main()
