#!/usr/bin/env python3
"""What the truth SAM costs: a chr20-size PE150 30x job (the genome and model of test_chr20_size_bit_exact)
written to files with truth off and on.  Prints one JSON line per leg: wall seconds of the yield call, the FASTQ and SAM bytes, and
the library's HIP-event times of k_reads and of the truth passes on the same batches.  Kernel-level numbers: run it under
`rocprofv3 --kernel-trace --stats -- python tools/truth_cost.py --legs on` (k_truth_size / k_truth_emit against k_reads_all)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scssim_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        fa, prof = os.path.join(td, "chr20.fa"), os.path.join(td, "m.profile")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--simu-out", fa])
        import gzip
        src = os.path.join(td, "x.profile")
        open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
        g = scssim_amd.GenReads(profile=prof, input_fasta=fa, coverage=a.coverage, seed=220)
        g.create_frags(); g.amplify(); g.allocate_reads(0)
        for leg in a.legs.split(","):
            out = os.path.join(td, "reads_" + leg)
            g.set_truth_sam(out + ".sam" if leg == "on" else None)
            t = time.time()
            g.yield_reads_files(out, 1)
            wall = time.time() - t
            st, kt = g.stats(), g.kernel_times()
            rec = dict(leg=leg, wall_s=round(wall, 3), pairs=st["pairs_written"], fastq_bytes=st["fastq_bytes"],
                       sam_bytes=g.truth_bytes() if leg == "on" else 0, k_reads=kt["k_reads"], k_truth=kt["k_truth"])
            print(json.dumps(rec), flush=True)
            for f in os.listdir(td):
                if f.startswith("reads_"):
                    os.unlink(os.path.join(td, f))


if __name__ == "__main__":
    main()
