"""Readers and builders the GPU test modules share: SAM / FASTQ / FASTA / BGZF readers, the downloaded lift segments, the oracle's
command line, generated genomes, the exact-placement profile and the small job of the cut-LDS checks.  No module of the suite
imports helpers from another test module; what several need lives here, a feature's restatement in its tests/*_cases.py."""
import gzip
import os
import re
import subprocess
import sys
import zlib

import numpy as np

from gpu_child import ROOT

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
SV = os.path.join(ROOT, "tests", "golden", "simuvars")
EOF_BLOCK = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
CIG = re.compile(r"(\d+)([MID])")


def _fastq(path):
    op = gzip.open if path.endswith(".gz") else open
    lines = op(path, "rb").read().split(b"\n")
    return [(lines[i][1:].decode(), lines[i + 1].decode(), lines[i + 3].decode()) for i in range(0, len(lines) - 1, 4)]


def _fasta(path):
    recs, name, parts = {}, None, []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            if name is not None:
                recs[name] = b"".join(parts).upper()
            name, parts = ln[1:].split()[0].decode(), []
        else:
            parts.append(ln.strip())
    recs[name] = b"".join(parts).upper()
    return {k: re.sub(rb"[^ACGT]", b"N", v) for k, v in recs.items()}


def _sam(path):
    hdr, recs = [], []
    for ln in open(path).read().split("\n")[:-1]:
        (hdr if ln.startswith("@") else recs).append(ln if ln.startswith("@") else ln.split("\t"))
    return hdr, recs


def _inflate(z):
    """the members of a BGZF file, one by one; the last one is the end-of-file block"""
    assert z.endswith(EOF_BLOCK)
    text, at = b"", 0
    while at < len(z):
        assert z[at:at + 4] == b"\x1f\x8b\x08\x04" and z[at + 12:at + 14] == b"BC"
        size = int.from_bytes(z[at + 16:at + 18], "little") + 1
        text += zlib.decompress(z[at + 18:at + size - 8], -15)
        at += size
    assert at == len(z)
    return text


def _same(got, want, what):
    if got != want:
        gl, wl = got.split("\n"), want.split("\n")
        bad = [i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]]
        print(what, "lines", len(gl), len(wl), "first differences", [(gl[i], wl[i]) for i in bad[:5]])
    assert got == want, what


class Segs:
    """The lift table's segments as a job's child dumped them (<out>_segs.npz)."""
    def __init__(self, out):
        z = np.load(out + "_segs.npz")
        self.hap_off, self.len, self.ref_pos, self.ref_rec, self.kind, self.ref_lens = (z[k].astype(np.int64) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind", "ref_lens"))

    def __len__(self):
        return len(self.hap_off)


def _oracle(oracle_bin, fa, prof, prefix, args, seed):
    subprocess.check_call([oracle_bin, "genreads", "-i", fa, "-m", prof, "-o", prefix, "--rng", "counter", "--seed", str(seed), "-t", "16", "-q"] + args)


def make_genome(path, lengths, seed, n_block=None, ref=False):
    """tools/make_genome.py: a staged diploid FASTA (ref: the haploid reference of a simuvars job) of records of these lengths."""
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", lengths, "--seed", str(seed), "--ref-out" if ref else "--simu-out", path]
                          + (["--n-block", str(n_block)] if n_block else []))
    return path


def _exact_profile(src, dst, ins, dele):
    """Substitution rows with all their mass on the row's own base (kmer XYZ -> Z), and the given indel rates."""
    lines = open(src).read().split("\n")
    out, i, L = [], 0, None
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("readLength:"):
            L = int(ln.split(":")[1])
        if ln in ("[Insert Rate]", "[Deletion Rate]"):
            out += [ln, "%g" % (ins if ln == "[Insert Rate]" else dele)]
            i += 2
            continue
        m = re.match(r"kmer: ([ACGTNX]{3})$", ln)
        if m:
            b = m.group(1)[2]
            out.append(ln)
            row = "\t".join("1" if c == b else "0" for c in "ACGT")
            out += [row if b in "ACGT" else r for r in lines[i + 1:i + 1 + 2 * L]]
            i += 1 + 2 * L
            continue
        out.append(ln)
        i += 1
    open(dst, "w").write("\n".join(out))
    return dst


# ---- the emit pass under a cut LDS (SCS_TEST_TRUTH_LDS).  The job: test_gpu_truth_bam.py::test_frequent_indels' genome and
# profile (insertion and deletion rates 0.01, no substitution anywhere), PE, at a coverage of 0.2: 350 kb / (2 x 125) x 0.2 = 280 pairs
CUT_JOB = dict(cov=0.2, layout="PE", seed=7, sink="callback", ber=0.0)
CUT_LDS = 256                                             # bytes: below any pair of the job (pair_floor)


def cut_job_inputs(d, models):
    return make_genome(str(d / "g.fa"), "200000,150000", 17), _exact_profile(models["Illumina_HiSeq2500"], str(d / "x.profile"), 0.01, 0.01)


def pair_floor(probe, rname, **kw):
    """Bytes of the smallest pair of records a job can hold, on the CPU, through the formatter the kernels run (`probe`: one of the
    record probes of scssim_amd).  The shortest read the profile admits has n + delta = 50 bases (fewer: the events are rolled
    back); its smallest record has every field at its narrowest: amplicon 0, count 1, a one-digit POS and PNEXT, FLAG 99, TLEN 50,
    the 75 deleted bases at the window's end (dropped from the CIGAR: "50M"), no mismatch.  A pair is two records, read 2's FLAG
    (147) a digit wider."""
    ev = [(50, 1, 75)]
    rec = probe(seq="A" * 50, qual="I" * 50, pos0=0, n=125, events=ev, reverse=False, rname=rname, amp=0, cnt=1, paired=True, is_read2=False, mate=(49, True, ev), **kw)
    return 2 * len(rec)
