#!/usr/bin/env python3
"""What the depth track by reference bin costs: a chr20-size PE150 30x job whose genome comes from
scs_simuvars -- the reference of tools/make_genome.py and a variation file of a few hundred CNVs and indels made here -- written to
files on tmpfs with both depth tracks off, with the haplotype track (--depth), with the reference track (--depth-ref) and with
both.  Prints one JSON line per leg and repeat: wall seconds of the yield call and the library's HIP-event times of k_reads,
k_depth and k_depth_lift on the same batches; --log FILE also appends them there (profiles/).  `--slots 0` runs the legs in a
child process whose k_depth_lift has no LDS table (SCS_TEST_LIFT_SLOTS=0 in the seams build: every add is a global atomic) -- the
A/B of the aggregation; `--slots 512` is the product's table through the same build.  `--legs off` runs on a library without the
feature too (SCSSIM_HIP_LIB = the parent commit's build): the yield time with the feature off against the parent's, back to back."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_variations(path, bases, n_cnv, n_indel, seed=16):
    """n_cnv copy-number stretches of 50 - 500 kb (CN 0 .. 8) in ascending order with plain stretches between them, n_indel
    insertions (10 - 300 bases) and as many deletions (5 - 200 bases) anywhere, half of them heterozygous."""
    import numpy as np
    rng = np.random.default_rng(seed)
    slot = bases // n_cnv
    lines = ["# tools/lift_cost.py"]
    for k in range(n_cnv):
        ln = int(rng.integers(min(50000, slot // 4), min(500000, slot // 2)))
        s = k * slot + int(rng.integers(1, slot - ln))
        cn = int(rng.choice([0, 1, 3, 4, 5, 6, 8]))
        lines.append("c\tchr20\t%d\t%d\t%d\t%d" % (s, s + ln - 1, cn, (cn + 1) // 2))
    for p in np.sort(rng.integers(1000, bases - 1000, n_indel)):
        lines.append("i\tchr20\t%d\t%s\t%s" % (p, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(10, 300)))]).decode(), "het" if rng.integers(2) else "homo"))
    for p in np.sort(rng.integers(1000, bases - 1000, n_indel)):
        lines.append("d\tchr20\t%d\t%d\t%s" % (p, int(rng.integers(5, 200)), "het" if rng.integers(2) else "homo"))
    open(path, "w").write("\n".join(lines) + "\n")


def job(a, td, log):
    import gzip
    import scssim_amd
    ref, var, prof = os.path.join(td, "chr20_ref.fa"), os.path.join(td, "vars.txt"), os.path.join(td, "m.profile")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--ref-out", ref])
    write_variations(var, a.bases, a.cnvs, a.indels)
    src = os.path.join(td, "x.profile")
    open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
    g = scssim_amd.GenReads(profile=prof, coverage=a.coverage, seed=220)
    t = time.time()
    g.simuvars(ref, None, var)
    have = hasattr(g, "lift_info") and hasattr(g._L, "scs_lift_info")
    head = dict(leg="simuvars", wall_s=round(time.time() - t, 3), staged_bases=g.stats()["genome_bases"], segments=g.lift_info()[0] if have else None)
    print(json.dumps(head), flush=True); log(head)
    g.create_frags(); g.amplify(); g.allocate_reads(0)
    g.yield_reads_files(os.path.join(td, "reads_warm"), a.writers)      # warm-up: the buffers, the pinned slots, the page cache
    for leg in [l for _ in range(a.repeats) for l in a.legs.split(",")]:
        out = os.path.join(td, "reads_" + leg)
        g.set_depth(a.bin if leg in ("depth", "both") else 0)
        if have:
            g.set_depth_ref(a.bin if leg in ("ref", "both") else 0)
        t = time.time()
        g.yield_reads_files(out, a.writers)
        wall = time.time() - t
        st, kt = g.stats(), g.kernel_times()
        rec = dict(leg=leg, slots=a.slots, bin=a.bin, writers=a.writers, wall_s=round(wall, 3), pairs=st["pairs_written"], k_reads=kt["k_reads"], k_depth=kt["k_depth"],
                   k_depth_lift=g.depth_ref_kernel_time() if have else None)
        if leg in ("ref", "both"):
            r, b, c, _ = g.depth_ref()
            rec.update(bins=int(r.size) - 1, reads_sum=int(r.sum()), bases_sum=int(b.sum()), unlifted_reads=int(r[-1]), unlifted_bases=int(b[-1]), copies_sum=int(c[:-1].sum()), inserted=int(c[-1]))
            assert rec["reads_sum"] == st["reads_written"] and rec["copies_sum"] + rec["inserted"] == st["genome_bases"]
        print(json.dumps(rec), flush=True); log(rec)
        for f in os.listdir(td):
            if f.startswith("reads_"):
                os.unlink(os.path.join(td, f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,depth,ref,both", help="comma list of off, depth, ref, both")
    ap.add_argument("--repeats", type=int, default=3, help="runs of every leg after one unrecorded warm-up yield")
    ap.add_argument("--slots", type=int, default=None, help="entries of k_depth_lift's LDS table (the seams build; 0: none).  Default: the product build")
    ap.add_argument("--bin", type=int, default=1000)
    ap.add_argument("--writers", type=int, default=1)
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--cnvs", type=int, default=120)
    ap.add_argument("--indels", type=int, default=150, help="insertions, and as many deletions")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/lift_cost_*.log)")
    a = ap.parse_args()
    if a.slots is not None and os.environ.get("SCS_TEST_LIFT_SLOTS") != str(a.slots):   # the seam is read once per process: a fresh child with it set
        env = dict(os.environ, SCS_TEST_LIFT_SLOTS=str(a.slots), SCSSIM_HIP_LIB=os.path.join(ROOT, "scssim_amd", "libscssim_hip_seams.so"))
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))

    def log(rec):
        if a.log:
            with open(a.log, "a") as f:
                f.write(json.dumps(dict(rec, lib=os.path.basename(os.environ.get("SCSSIM_HIP_LIB") or "libscssim_hip.so"))) + "\n")
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        job(a, td, log)


if __name__ == "__main__":
    main()
