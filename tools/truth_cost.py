#!/usr/bin/env python3
"""What the truth SAM and the truth BAM cost: a chr20-size PE150 30x job (the genome and model of
test_chr20_size_bit_exact) written to files with truth off, with the SAM on and (--bam) with the BAM on.  Prints one JSON line per
leg and repeat: wall seconds of the yield call, the FASTQ and truth bytes (BAM: compressed, and uncompressed from the blocks' ISIZE
fields), and the library's HIP-event times of k_reads and of the truth passes on the same batches.  Kernel-level numbers: run it under
`rocprofv3 --kernel-trace --stats -- python tools/truth_cost.py --legs on,bam --repeats 1` (k_truth_size / k_truth_emit,
k_truth_bam_size / k_truth_bam_emit and the BGZF kernels against k_reads_all).
With a `ref` leg (the truth SAM on the original reference) every leg runs on a genome built by scs_simuvars, as
tools/lift_cost.py builds its genome, so that a lift table exists: `--legs off,on,ref --repeats 3`.  `--legs off` runs on a library
without the feature too (SCSSIM_HIP_LIB = the parent commit's build); --log FILE appends the JSON lines there (profiles/)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import struct
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scssim_amd  # noqa: E402


def bgzf_isize_sum(path):
    """Uncompressed bytes of a BGZF file: the sum of its members' ISIZE fields, found by walking BSIZE."""
    tot, o, n = 0, 0, os.path.getsize(path)
    with open(path, "rb") as f:
        while o < n:
            f.seek(o + 16)
            bsize = struct.unpack("<H", f.read(2))[0] + 1
            f.seek(o + bsize - 4)
            tot += struct.unpack("<I", f.read(4))[0]
            o += bsize
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=None, help="comma list of off, on (the SAM), bam, ref (the SAM on the reference) [off,on; with --bam: off,on,bam]")
    ap.add_argument("--simuvars", action="store_true", help="the genome of the ref leg (scs_simuvars over the variations of tools/lift_cost.py) without that leg")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--bam", action="store_true", help="add the truth BAM leg")
    ap.add_argument("--repeats", type=int, default=1, help="runs of every leg after one unrecorded warm-up yield")
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        fa, prof = os.path.join(td, "chr20.fa"), os.path.join(td, "m.profile")
        if "ref" not in (a.legs or "").split(",") and not a.simuvars:
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--simu-out", fa])
        import gzip
        src = os.path.join(td, "x.profile")
        open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
        legs = (a.legs or ("off,on,bam" if a.bam else "off,on")).split(",")
        if "ref" in legs or a.simuvars:
            from lift_cost import write_variations
            var = os.path.join(td, "vars.txt")
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--ref-out", fa])
            write_variations(var, a.bases, 120, 150)
            g = scssim_amd.GenReads(profile=prof, coverage=a.coverage, seed=220)
            g.simuvars(fa, None, var)
        else:
            g = scssim_amd.GenReads(profile=prof, input_fasta=fa, coverage=a.coverage, seed=220)
        g.create_frags(); g.amplify(); g.allocate_reads(0)
        have_ref = hasattr(g._L, "scs_set_truth_ref_sam")
        if a.repeats > 1:                                   # warm-up: the buffers, the pinned slots and the page cache of the first yield
            g.yield_reads_files(os.path.join(td, "reads_warm"), 1)
        for leg in [l for _ in range(a.repeats) for l in legs]:
            out = os.path.join(td, "reads_" + leg)
            if have_ref:                                    # (one truth output per ctx: the last leg's is cleared before this leg's is set)
                g.set_truth_ref_sam(None)
            g.set_truth_sam(out + ".sam" if leg == "on" else None)
            g.set_truth_bam(out + ".bam" if leg == "bam" else None)
            if have_ref and leg == "ref":
                g.set_truth_ref_sam(out + ".ref.sam")
            t = time.time()
            g.yield_reads_files(out, 1)
            wall = time.time() - t
            st, kt = g.stats(), g.kernel_times()
            rec = dict(leg=leg, wall_s=round(wall, 3), pairs=st["pairs_written"], fastq_bytes=st["fastq_bytes"],
                       sam_bytes=g.truth_bytes() if leg in ("on", "ref") else 0, bam_bytes=g.truth_bytes() if leg == "bam" else 0,
                       bam_uncompressed_bytes=bgzf_isize_sum(out + ".bam") if leg == "bam" else 0, k_reads=kt["k_reads"], k_truth=kt["k_truth"])
            print(json.dumps(rec), flush=True)
            if a.log:
                with open(a.log, "a") as f:
                    f.write(json.dumps(dict(rec, lib=os.environ.get("SCSSIM_HIP_LIB") or "libscssim_hip.so")) + "\n")
            for f in os.listdir(td):
                if f.startswith("reads_"):
                    os.unlink(os.path.join(td, f))


if __name__ == "__main__":
    main()
