#!/usr/bin/env python3
"""What the bedGraph files of the per-base arrays cost: the chr20-size PE150 30x simuvars job of
tools/cost_job.py, one yield call with both coverage switches on, then every file -- the staged depths, the reference depths, the
reference's true copy number -- plain and as .gz, written to tmpfs.  Prints one JSON line per file and repeat: lines and text
bytes, the file's size, the writer's HIP-event time (scs_coverage_bedgraph_kernel_time: the plan passes and per slab scan, emit and
BGZF), the write call's wall seconds and the slabs at the default cap (one event pair for the plan passes, one per slab);
--log FILE also appends them there (profiles/).  A warm-up write of every file comes first: the writer's buffers, the pinned block."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_job as cj  # noqa: E402

FILES = (("staged", "write_coverage_bedgraph"), ("ref", "write_coverage_ref_bedgraph"), ("copies", "write_copy_number_ref"))


def job(a, td):
    lib = os.path.basename(os.environ.get("SCSSIM_HIP_LIB") or "libscssim_hip.so")
    g, ref, var = cj.open_ctx(a, td, True, a.cnvs, a.indels)
    g.simuvars(ref, None, var)
    cj.allocate(g)
    g.set_coverage(a.max_depth); g.set_coverage_ref(a.max_depth)
    t = time.time()
    cj.warm_up(g, td)
    cj.emit(dict(leg="yield", wall_s=round(time.time() - t, 3), staged_bases=g.stats()["genome_bases"], pairs=g.stats()["pairs_written"], k_cov_finish=g.coverage_kernel_time(1),
                 k_cov_ref_finish=g.coverage_ref_kernel_time(1)), a.log, lib)
    wanted = a.legs.split(",")
    for rep in range(a.repeats + 1):                        # (the first round is the warm-up: not recorded)
        for name, method in FILES:
            for gz in (False, True):
                if name not in wanted:
                    continue
                path = os.path.join(td, "cov_" + name + (".bg.gz" if gz else ".bg"))
                t = time.time()
                info = getattr(g, method)(path)
                wall = time.time() - t
                kt = g.coverage_bedgraph_kernel_time()
                if rep:
                    cj.emit(dict(leg=name, gz=gz, lines=info["lines"], text_bytes=info["text_bytes"], file_bytes=os.path.getsize(path), k_runs=kt, slabs=kt["launches"] - 1,
                                 wall_s=round(wall, 4), text_mb_per_s=round(info["text_bytes"] / 1e6 / wall, 1)), a.log, lib)
                os.unlink(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="staged,ref,copies", help="comma list of staged, ref, copies")
    ap.add_argument("--max-depth", type=int, default=1000)
    cj.add_common(ap, repeats=3, warm="write of every file", simuvars=True)
    ap.add_argument("--log", default=None, help="append the JSON lines to this file too (profiles/coverage_bedgraph_cost_*.log)")
    cj.run(ap.parse_args(), job)


if __name__ == "__main__":
    main()
