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
import os
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402


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


def job(a, td):
    lib = os.environ.get("SCSSIM_HIP_LIB") or "libscssim_hip.so"
    legs = (a.legs or ("off,on,bam" if a.bam else "off,on")).split(",")
    if "ref" in legs or a.simuvars:
        g, ref, var = cj.open_ctx(a, td, True)
        g.simuvars(ref, None, var)
    else:
        g = cj.open_ctx(a, td)
    cj.allocate(g)
    have_ref = hasattr(g._L, "scs_set_truth_ref_sam")
    if a.repeats > 1:                                       # (a single repeat goes without the warm-up yield, as it always has)
        cj.warm_up(g, td)
    for leg in cj.legs(a, td, names=legs):
        out = os.path.join(td, "reads_" + leg)
        if have_ref:                                        # (one truth output per ctx: the last leg's is cleared before this leg's is set)
            g.set_truth_ref_sam(None)
        g.set_truth_sam(out + ".sam" if leg == "on" else None)
        g.set_truth_bam(out + ".bam" if leg == "bam" else None)
        if have_ref and leg == "ref":
            g.set_truth_ref_sam(out + ".ref.sam")
        t = time.time()
        g.yield_reads_files(out, 1)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        cj.emit(dict(leg=leg, wall_s=round(wall, 3), pairs=st["pairs_written"], fastq_bytes=st["fastq_bytes"],
                     sam_bytes=g.truth_bytes() if leg in ("on", "ref") else 0, bam_bytes=g.truth_bytes() if leg == "bam" else 0,
                     bam_uncompressed_bytes=bgzf_isize_sum(out + ".bam") if leg == "bam" else 0, k_reads=kt["k_reads"], k_truth=kt["k_truth"]), a.log, lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=None, help="comma list of off, on (the SAM), bam, ref (the SAM on the reference) [off,on; with --bam: off,on,bam]")
    ap.add_argument("--simuvars", action="store_true", help="the genome of the ref leg (scs_simuvars over the variations of tools/lift_cost.py) without that leg")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--bam", action="store_true", help="add the truth BAM leg")
    cj.add_common(ap, repeats=1)
    cj.run(ap.parse_args(), job)


if __name__ == "__main__":
    main()
