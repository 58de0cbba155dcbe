#!/usr/bin/env python3
"""What the artefact table on the original reference costs: the chr20-size PE150 30x job of tools/lift_cost.py
(the reference of tools/make_genome.py through scs_simuvars with that tool's variation file), files on tmpfs.  Prints one JSON line
per leg and repeat: wall seconds of the call, the HIP-event time of its kernels (the library sorts and scans included), the sites
and bytes written.  Legs: art0 = scs_write_artefacts (the yardstick), ref0 / ref1 / ref0_bgzf / ref1_bgzf = scs_write_artefacts_ref
at min_reads 0 and 1, plain and BGZF.  --parent-lib PATH: the parent commit's library runs art0 on the same job before and after,
each in a process of its own (a library is loaded once per process)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEGS = {"ref0": (0, False), "ref1": (1, False), "ref0_bgzf": (0, True), "ref1_bgzf": (1, True)}


def job(a, td, log):
    import scssim_amd
    from lift_cost import write_variations
    ref, var, prof = os.path.join(td, "chr20_ref.fa"), os.path.join(td, "vars.txt"), os.path.join(td, "m.profile")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(a.bases), "--seed", "20", "--n-block", "60000", "--ref-out", ref])
    write_variations(var, a.bases, a.cnvs, a.indels)
    src = os.path.join(td, "x.profile")
    open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
    g = scssim_amd.GenReads(profile=prof, coverage=a.coverage, seed=220)
    t = time.time()
    g.simuvars(ref, None, var)
    head = dict(leg="simuvars", wall_s=round(time.time() - t, 3), staged_bases=g.stats()["genome_bases"], segments=g.lift_info()[0])
    g.create_frags(); g.amplify(); g.allocate_reads(0)
    head.update(fulls=g.stats()["full_amplicons"])
    print(json.dumps(head), flush=True); log(head)
    legs = a.legs.split(",")
    g.write_artefacts(os.path.join(td, "art_warm.vcf"))                      # warm-up of each kind: the buffers, the page cache
    if any(l in LEGS for l in legs):
        g.write_artefacts_ref(os.path.join(td, "art_warm_ref.vcf"))
    for leg in [l for _ in range(a.repeats) for l in legs]:
        t = time.time()
        if leg in LEGS:
            min_reads, bgzf = LEGS[leg]
            r = g.write_artefacts_ref(os.path.join(td, "art_" + leg + (".vcf.gz" if bgzf else ".vcf")), bgzf=bgzf, min_reads=min_reads)
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), kernels=g.artefact_ref_kernel_time(), **r)
        else:
            r = g.write_artefacts(os.path.join(td, "art_" + leg + ".vcf"))
            wall = time.time() - t
            rec = dict(leg=leg, wall_s=round(wall, 3), kernels=g.artefact_kernel_time(), **r)
        print(json.dumps(rec), flush=True); log(rec)
        for f in os.listdir(td):
            if f.startswith("art_"):
                os.unlink(os.path.join(td, f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="art0,ref0,ref1,ref0_bgzf,ref1_bgzf", help="comma list of art0, ref0, ref1, ref0_bgzf, ref1_bgzf")
    ap.add_argument("--repeats", type=int, default=3, help="runs of every leg after one unrecorded warm-up of each kind")
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--cnvs", type=int, default=120)
    ap.add_argument("--indels", type=int, default=150, help="insertions, and as many deletions")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libscssim_hip.so: it runs --legs art0 before and after this tree's legs")
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/artefacts_ref_cost_*.log)")
    a = ap.parse_args()

    if a.parent_lib:                                           # three fresh children: parent, this tree, parent
        rest = [x for i, x in enumerate(sys.argv[1:]) if x != "--parent-lib" and (i == 0 or sys.argv[i] != "--parent-lib") and not x.startswith("--parent-lib=")]
        for lib, extra in ((a.parent_lib, ["--legs", "art0"]), (None, []), (a.parent_lib, ["--legs", "art0"])):
            env = dict(os.environ)
            if lib:
                env["SCSSIM_HIP_LIB"] = os.path.abspath(lib)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__)] + rest + extra, env=env)
            if rc:
                sys.exit(rc)                                   # (nothing more is started after a failure)
        return

    def log(rec):
        if a.log:
            with open(a.log, "a") as f:
                f.write(json.dumps(dict(rec, lib=os.environ.get("SCSSIM_HIP_LIB") and "parent" or "this tree")) + "\n")
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        job(a, td, log)


if __name__ == "__main__":
    main()
