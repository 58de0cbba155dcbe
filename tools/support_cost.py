#!/usr/bin/env python3
"""What the site support costs: the chr20-size PE150 30x job of tools/truth_cost.py written to files on tmpfs
on one ctx, with the site support off and on at min_reads 1 and 0.  Prints one JSON line per leg and repeat: wall seconds of the
yield call (the site table's build is part of it), the library's HIP-event times of k_reads and k_support on the same batches, the
sites, the positions the reads touched and the sums of the counters.  `--slots 0` runs the legs in a child process whose kernel
has no LDS table (SCS_TEST_SUPPORT_SLOTS=0 in the seams build: every add is a global atomic) -- the A/B of the aggregation;
`--slots 1024` is the product's table through the same build."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"off": None, "on1": 1, "on0": 0}


def job(a, td):
    import gzip
    import scssim_amd
    fa, prof = os.path.join(td, "chr20.fa"), os.path.join(td, "m.profile")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--simu-out", fa])
    src = os.path.join(td, "x.profile")
    open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
    g = scssim_amd.GenReads(profile=prof, input_fasta=fa, coverage=a.coverage, seed=220)
    g.create_frags(); g.amplify(); g.allocate_reads(0)
    g.yield_reads_files(os.path.join(td, "reads_warm"), a.writers)      # warm-up: the buffers, the pinned slots, the page cache
    for leg in [l for _ in range(a.repeats) for l in a.legs.split(",")]:
        out = os.path.join(td, "reads_" + leg)
        g.set_site_support(LEGS[leg] is not None, LEGS[leg] or 0)
        t = time.time()
        g.yield_reads_files(out, a.writers)
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
        print(json.dumps(rec), flush=True)
        for f in os.listdir(td):
            if f.startswith("reads_"):
                os.unlink(os.path.join(td, f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on1,on0", help="comma list of off, on1 (min_reads 1), on0 (min_reads 0)")
    ap.add_argument("--repeats", type=int, default=3, help="runs of every leg after one unrecorded warm-up yield")
    ap.add_argument("--slots", type=int, default=None, help="entries of the kernel's LDS table (the seams build; 0: none).  Default: the product build")
    ap.add_argument("--writers", type=int, default=1)
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    a = ap.parse_args()
    if a.slots is not None and os.environ.get("SCS_TEST_SUPPORT_SLOTS") != str(a.slots):   # the seam is read once per process: a fresh child with it set
        env = dict(os.environ, SCS_TEST_SUPPORT_SLOTS=str(a.slots), SCSSIM_HIP_LIB=os.path.join(ROOT, "scssim_amd", "libscssim_hip_seams.so"))
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        job(a, td)


if __name__ == "__main__":
    main()
