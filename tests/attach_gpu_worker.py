"""Worker for tests/test_gpu_attach.py: one unsharded genreads job on the GPU in a process of its own (the attach seams
SCS_ATTACH_GROUPS / SCS_ATTACH_G are read once per process), everything the test compares written beside `prefix`:
<prefix>.npz (amplicon tables, primer stock, read numbers, stock statistics) and <prefix>_1.fq / _2.fq."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    fasta, profile, prefix, coverage, seed, primers, gamma = sys.argv[1:8]
    import numpy as np
    import scssim_amd
    g = scssim_amd.GenReads(profile=profile, input_fasta=fasta, coverage=float(coverage), seed=int(seed), primers=int(primers), gamma=float(gamma))
    g.create_frags()
    g.amplify()
    st = g.stats()
    out = dict(stock=g.download_primer_stock(), stock_stats=np.array([st["stock_checks"], st["stock_exhausted_passes"], st["stock_rounds"]], np.int64))
    from scssim_amd import api
    cfg = api._Config()
    scssim_amd.load_library().scs_default_config(api.C.byref(cfg))
    out["amp_limits"] = np.array([cfg.amplicon_min_len, cfg.amplicon_max_len], np.int64)   # what the preconditions' arithmetic assumes
    for kind, name in ((0, "semis"), (1, "fulls")):
        for k, v in g.download_amplicons(kind).items():
            out[name + "_" + k] = v
    g.allocate_reads(0)
    out["readnum"] = g.download_read_numbers()
    fq1, fq2 = g.yield_reads()
    np.savez(prefix + ".npz", **out)
    with open(prefix + "_1.fq", "wb") as f:
        f.write(fq1)
    with open(prefix + "_2.fq", "wb") as f:
        f.write(fq2)
    print("library %s: %d semi + %d full amplicons, %d pairs" % (os.path.basename(scssim_amd.lib_path()), st["semi_amplicons"], st["full_amplicons"], g.stats()["pairs_written"]))


if __name__ == "__main__":
    main()
