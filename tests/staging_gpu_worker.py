"""Worker for tests/test_gpu_staging.py: all the GPU work of one group of its tests in a process of its own; what the staging
kernels left on the device (GenReads.download_genome) goes to <out>/<mode>.npz and <out>/<mode>.json, every check runs in the test.
SCS_TEST_FASTA_CHUNK is read at every load_genome call (scs_stage.cpp), so one process sets it from call to call.
  parser   the case table of tests/fasta_cases.py at every chunk size, the ragged 100 KB file at two more
  index    uploaded genomes of the edge lengths: codes, bit index, prefix arrays, pair, two-bit copy
  hasn     a genome with N blocks: fragments and has_n
  slice EOL CHUNK   sharded ctxs (no collectives) on an indexed FASTA of lf / crlf line ends: every rank's slice under one piece size
  slice_extra       the same path on a line longer than a piece, and its fallbacks to the parser
  cap     more than 2^20 headers, then a file that loads"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import fasta_cases as fc
import scssim_amd

ARRAYS = ("codes",) + fc.INDEX_KEYS


def set_chunk(chunk):
    if chunk is None:
        os.environ.pop("SCS_TEST_FASTA_CHUNK", None)
    else:
        os.environ["SCS_TEST_FASTA_CHUNK"] = str(chunk)


def write(path, data, fai=None, fai_age=0):
    """the file, and beside it no index, or `fai` (bytes), fai_age seconds older than the file when asked"""
    with open(path, "wb") as f:
        f.write(data)
    if os.path.exists(path + ".fai"):
        os.unlink(path + ".fai")
    if fai is not None:
        with open(path + ".fai", "wb") as f:
            f.write(fai)
        if fai_age:
            t = os.stat(path).st_mtime
            os.utime(path + ".fai", (t - fai_age, t - fai_age))
    return path


def take(res, meta, key, g, arrays=ARRAYS, **more):
    """one download of ctx g under `key`"""
    d = g.download_genome(**more)
    for k in arrays + (("has_n",) if more.get("has_n") else ()):
        res[key + "." + k] = d[k]
    res[key + ".rec_lens"] = d["rec_lens"]
    st = g.stats()
    meta[key] = dict(names=d["names"], slice_base=d["slice_base"], slice_len=d["slice_len"], records=st["records"], genome_bases=st["genome_bases"], staged_bases=st["staged_bases"])


def load(res, meta, key, g, path, arrays=ARRAYS):
    """load_genome + download under `key`; a refusal is recorded, not raised"""
    try:
        g.load_genome(path)
    except scssim_amd.ScsError as e:
        meta[key] = dict(error=str(e), code=e.code)
        return
    take(res, meta, key, g, arrays)
    meta[key]["fai"] = open(path + ".fai", "rb").read().decode("latin-1") if os.path.exists(path + ".fai") else None


def parser(out, res, meta):
    for chunk in fc.CHUNKS:
        set_chunk(chunk)
        g = scssim_amd.GenReads()                                   # one ctx per chunk size, loaded with file after file
        for name in fc.CASES:
            load(res, meta, "%s.%s" % (name, chunk), g, write(os.path.join(out, "%s.%s.fa" % (name, chunk)), fc.data(name)), ("codes",))
        g.close()
    for chunk in fc.RAGGED_CHUNKS:
        set_chunk(chunk)
        g = scssim_amd.GenReads()
        load(res, meta, "ragged_100k.%s" % chunk, g, write(os.path.join(out, "ragged_100k.%s.fa" % chunk), fc.ragged_100k()), ("codes",))
        g.close()


def index(out, res, meta):
    g = scssim_amd.GenReads()
    for total in sorted(fc.INDEX_TOTALS, reverse=True):                 # descending: a shorter genome lies in buffers a longer one has filled
        for variant in fc.INDEX_VARIANTS:
            seq = fc.index_genome(total, variant)
            for layout, lens in (("one", [total]), ("three", fc.split_three(total))):
                offs = np.concatenate([[0], np.cumsum(lens)])
                g.upload_genome(["r%d_1_%d" % (i, n) for i, n in enumerate(lens)], [seq[offs[i]:offs[i + 1]] for i in range(len(lens))])
                take(res, meta, "%d.%s.%s" % (total, variant, layout), g)
    with_genome = scssim_amd.GenReads()
    try:
        with_genome.download_genome()
        meta["before_staging"] = dict(error=None)
    except scssim_amd.ScsError as e:
        meta["before_staging"] = dict(error=str(e), code=e.code)


def hasn(out, res, meta):
    recs = fc.hasn_genome()
    g = scssim_amd.GenReads(seed=fc.HASN_SEED)
    g.upload_genome([n for n, _ in recs], [s for _, s in recs])
    try:
        g.download_genome(has_n=True)
        meta["before_frags"] = dict(error=None)
    except scssim_amd.ScsError as e:
        meta["before_frags"] = dict(error=str(e), code=e.code)
    g.create_frags()
    take(res, meta, "hasn", g, ("codes", "n_bits", "n_pref"), has_n=True)
    for k, v in g.download_frags().items():
        res["frags." + k] = v


def slices(out, res, meta, eol_name, chunk):
    """every rank of 2, 3 and 5 shards on the three-record file with these line ends, under pieces of `chunk` bytes"""
    recs = fc.slice_records()
    text = fc.fasta_text(recs, 70, *dict(lf=(b"\n", True), crlf=(b"\r\n", False))[eol_name])
    path = write(os.path.join(out, "slice.%s.fa" % eol_name), text)
    scssim_amd.fasta_write_index(path)                                  # the host writer's index; the test compares it with the one stated from the records
    meta["fai"] = open(path + ".fai").read()
    set_chunk(int(chunk))
    for n in fc.SLICE_SHARDS:
        for r in range(n):
            g = scssim_amd.GenReads(shard_rank=r, shard_count=n, seed=fc.SLICE_SEED)
            load(res, meta, "slice.%d.%d" % (n, r), g, path)
            g.close()


def slice_extra(out, res, meta):
    recs = fc.slice_records()
    set_chunk(256)
    # a record on one line longer than the piece buffer: one base per piece
    long_recs = fc.long_line_records()
    path = write(os.path.join(out, "long.fa"), fc.fasta_text(long_recs, 5000), fc.fai_regular(long_recs, 5000).encode())
    for r in range(2):
        g = scssim_amd.GenReads(shard_rank=r, shard_count=2, seed=fc.SLICE_SEED)
        load(res, meta, "long.2.%d" % r, g, path)
        g.close()
    # the fallbacks to the parser, each followed on the same ctx by a regular file that is sliced again; and an empty LAST record, which the index can describe
    regular = write(os.path.join(out, "regular.fa"), fc.fasta_text(recs), fc.fai_regular(recs).encode())
    with_empty = recs[:1] + [("empty_1_0", b"")] + recs[1:]
    empty_fai = fc.fai(fc.fasta_text(with_empty))
    falls = {"no_fai": (fc.fasta_text(recs), None, 0),
             "stale_fai": (fc.fasta_text(recs), fc.fai_regular(recs).encode(), 100),
             "widths_cancel_out": (fc.fasta_text(recs, widths=(71, 69, 70, 70)), fc.fai_regular(recs).encode(), 0),
             "empty_record": (fc.fasta_text(with_empty), empty_fai, 0),
             "empty_last_record": (fc.fasta_text(recs + [("empty_1_0", b"")]), fc.fai(fc.fasta_text(recs + [("empty_1_0", b"")])), 0)}
    for name, (text, fai, age) in falls.items():
        path = write(os.path.join(out, "fall.%s.fa" % name), text, fai, age)
        for n, r in ((2, 0), (2, 1), (3, 1)):
            g = scssim_amd.GenReads(shard_rank=r, shard_count=n, seed=fc.SLICE_SEED)
            load(res, meta, "fall.%s.%d.%d" % (name, n, r), g, path)
            load(res, meta, "fall.%s.%d.%d.then_regular" % (name, n, r), g, regular)
            g.close()
            if name in ("no_fai", "stale_fai"):                           # (the next rank meets the same file again: no index / the stale one)
                write(path, text, fai, age)


def cap(out, res, meta):
    path = write(os.path.join(out, "many.fa"), b">a\n" * ((1 << 20) + 1))
    g = scssim_amd.GenReads()
    load(res, meta, "many", g, path)
    load(res, meta, "then_lf", g, write(os.path.join(out, "lf.fa"), fc.data("lf")), ("codes",))


def main():
    mode, out = sys.argv[1:3]
    res, meta = {}, {}
    dict(parser=parser, index=index, hasn=hasn, slice=slices, slice_extra=slice_extra, cap=cap)[mode](out, res, meta, *sys.argv[3:])
    np.savez(os.path.join(out, mode + ".npz"), **res)
    with open(os.path.join(out, mode + ".json"), "w") as f:
        json.dump(meta, f)
    print("staging worker %s: %d downloads with library %s" % (mode, len(meta), os.path.basename(scssim_amd.lib_path())))


if __name__ == "__main__":
    main()
