#!/usr/bin/env python3
"""What the amplicon table costs: the chr20-size PE150 30x job of tools/truth_cost.py with files on tmpfs.
Prints one JSON line per leg and repeat: wall seconds of scs_write_amplicons (plain, BGZF), the HIP-event time of its kernels,
the bytes written and the amplicons; beside them the wall seconds of scs_amplify and of scs_yield_reads_files on the same job and
box (`--legs yield` alone, run on a checkout of the parent commit, gives the parent's figures: it uses nothing the table adds)."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def job(a, td):
    import scssim_amd
    fa, prof = os.path.join(td, "chr20.fa"), os.path.join(td, "m.profile")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--simu-out", fa])
    src = os.path.join(td, "x.profile")
    open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
    g = scssim_amd.GenReads(profile=prof, input_fasta=fa, coverage=a.coverage, seed=220)
    g.create_frags()
    t = time.time(); g.amplify(); amplify_s = time.time() - t
    g.allocate_reads(0)
    st = g.stats()
    print(json.dumps(dict(leg="amplify", wall_s=round(amplify_s, 3), semis=st["semi_amplicons"], fulls=st["full_amplicons"])), flush=True)
    legs = a.legs.split(",")
    if "yield" in legs:
        g.yield_reads_files(os.path.join(td, "reads_warm"), 1)            # warm-up: the buffers, the pinned slots, the page cache
    if "plain" in legs or "bgzf" in legs:
        g.write_amplicons(os.path.join(td, "amp_warm.tsv"))
    for leg in [l for _ in range(a.repeats) for l in legs]:
        t = time.time()
        if leg == "yield":
            g.set_seed(220); g.yield_reads_files(os.path.join(td, "reads_" + leg), 1)
            rec = dict(leg=leg, wall_s=round(time.time() - t, 3), pairs=g.stats()["pairs_written"], k_reads=g.kernel_times()["k_reads"])
        else:
            n = g.write_amplicons(os.path.join(td, "amp_" + leg + (".tsv.gz" if leg == "bgzf" else ".tsv")), bgzf=leg == "bgzf")
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), bytes=n, kernels=g.amplicon_kernel_time(), mb_per_s=round(n / wall / 1e6, 1))
        print(json.dumps(rec), flush=True)
        for f in os.listdir(td):
            if f.startswith("reads_") or f.startswith("amp_"):
                os.unlink(os.path.join(td, f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="yield,plain,bgzf", help="comma list of yield, plain, bgzf")
    ap.add_argument("--repeats", type=int, default=3, help="runs of every leg after one unrecorded warm-up of each kind")
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        job(a, td)


if __name__ == "__main__":
    main()
