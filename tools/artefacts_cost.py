#!/usr/bin/env python3
"""What the artefact table costs: the chr20-size PE150 30x job of tools/amplicons_cost.py with files on tmpfs.
Prints one JSON line per leg and repeat: wall seconds of scs_write_artefacts at min_reads 0 and 1, plain and BGZF, the HIP-event
time of its kernels (the library sorts and scans included), the sites and bytes written; beside them scs_write_amplicons (plain,
BGZF) on the same job and tree, which is what the call is expected not to exceed."""
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

LEGS = {"art0": (0, False), "art1": (1, False), "art0_bgzf": (0, True), "art1_bgzf": (1, True)}


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
    g.write_artefacts(os.path.join(td, "art_warm.vcf"))                      # warm-up of each kind: the buffers, the page cache
    g.write_amplicons(os.path.join(td, "amp_warm.tsv"))
    for leg in [l for _ in range(a.repeats) for l in legs]:
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
        print(json.dumps(rec), flush=True)
        for f in os.listdir(td):
            if f.startswith("art_") or f.startswith("amp_"):
                os.unlink(os.path.join(td, f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="art0,art1,art0_bgzf,art1_bgzf,amp,amp_bgzf", help="comma list of art0, art1, art0_bgzf, art1_bgzf, amp, amp_bgzf")
    ap.add_argument("--repeats", type=int, default=3, help="runs of every leg after one unrecorded warm-up of each kind")
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        job(a, td)


if __name__ == "__main__":
    main()
