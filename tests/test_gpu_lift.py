"""GPU tests of the lift table and the depth track by reference bin (scs_simuvars / scs_load_lift / scs_set_depth_ref, `scssim
simuvars --lift`, `scssim genreads --lift --depth-ref`): the per-bin counters equal what the truth SAM of the
same yield call gives, read by read, through the downloaded segment table; the copies equal the host value; a dense layout where
most reads cross segment boundaries; a plain genome against the haplotype depth track; nothing else moves; the counters do not
depend on sinks, batch cuts or the LDS table's size; positions lifted on the device; the two-step flow through the CLI; refusals
and ownership.  Each job runs in a child process under its own time limit; the checks run here.  Run with `-m gpu`."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, seams_env
from test_gpu_truth import CIG, _exact_profile, _sam
from test_lift_host import copies_from_table, ref_layout

import scssim_amd

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "scssim_amd", "bin", "scssim")
SV = os.path.join(GOLDEN, "simuvars")

# one ctx, one genome (built by simuvars, or a FASTA and its lift file), one amplified job, then a yield per leg:
# {name, wr (reference bins; 0: off), w (haplotype bins; 0: off), sink (callback / null / files / device), sam, writers, ...}
_CHILD = r'''
import json, os, sys, ctypes
sys.path.insert(0, %(root)r)
import numpy as np
import scssim_amd
a = json.loads(%(args)r)
g = scssim_amd.GenReads(profile=a["prof"], coverage=a["cov"], layout=a["layout"], seed=a["seed"], isize=a.get("isize", 260), ber=a.get("ber", 3.4e-4))
out = a["out"]
if a.get("fasta"):
    g.load_genome(a["fasta"]); g.load_lift(a["lift"])
else:
    g.simuvars(a["ref"], a.get("snp"), a.get("vars"), a.get("out_fasta"))
    g.write_lift(out + ".lift")
t = g.lift_segments()
np.savez(out + "_segs.npz", hap_off=t.hap_off, len=t.len, ref_pos=t.ref_pos, ref_rec=t.ref_rec, kind=t.kind, ref_lens=t.ref_lens)
g.create_frags(); g.amplify(); g.allocate_reads(0)
res = {}
for leg in a["legs"]:
    pre = out + "_" + leg["name"]
    g.set_seed(a["seed"])
    g.set_depth(leg.get("w", 0)); g.set_depth_ref(leg.get("wr", 0))
    g.set_truth_sam(pre + ".sam" if leg.get("sam") else None)
    kind = leg.get("sink", "callback")
    if kind == "callback":
        f1, f2 = g.yield_reads()
        open(pre + "_1.fq", "wb").write(f1); open(pre + "_2.fq", "wb").write(f2)
    elif kind == "null":
        g.yield_reads(collect=False)
    elif kind == "files":
        g.yield_reads_files(pre, leg.get("writers", 1), leg.get("generations", 1), bgzf=leg.get("bgzf", False))
    else:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]; hip.hipFree.argtypes = [ctypes.c_void_p]
        d1, d2, cap = ctypes.c_void_p(), ctypes.c_void_p(), 64 << 20
        assert hip.hipMalloc(ctypes.byref(d1), cap) == 0 and hip.hipMalloc(ctypes.byref(d2), cap) == 0
        g.yield_reads_device(d1, cap, d2, cap)
        hip.hipFree(d1); hip.hipFree(d2)
    res[leg["name"]] = dict(reads_written=g.stats()["reads_written"], k_depth_lift=g.depth_ref_kernel_time(), k_reads=g.kernel_times()["k_reads"], k_depth=g.kernel_times()["k_depth"])
    arrays = {}
    if leg.get("wr"):
        arrays["reads"], arrays["bases"], arrays["copies"], arrays["off"] = g.depth_ref()
        if leg.get("write"):
            g.write_depth_ref(pre + ".tsv")
    if leg.get("w"):
        arrays["hreads"], arrays["hbases"], arrays["hoff"] = g.depth()
    np.savez(pre + "_depth.npz", **arrays)
print("RESULT " + json.dumps(res))
'''


def _run(tmp_path, legs, env=None, timeout=300, **a):
    a.setdefault("out", str(tmp_path / "job"))
    a["legs"] = legs
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, args=json.dumps(a))], env=env or dict(os.environ),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])
    return a["out"], res


def _arrays(out, name):
    return np.load(out + "_" + name + "_depth.npz")


class Segs:
    def __init__(self, out):
        z = np.load(out + "_segs.npz")
        self.hap_off, self.len, self.ref_pos, self.ref_rec, self.kind, self.ref_lens = (z[k].astype(np.int64) for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind", "ref_lens"))

    def __len__(self):
        return len(self.hap_off)


def lift_from_sam(path, seg, w):
    """The contract from the SAM's @SQ lines, POS and CIGAR through the segment table, base by base in numpy: (reads, bases) of
    n_bins + 1 entries, the record count, the sum of the M lengths, and what the reads of the job reach (the dense case's conditions)."""
    hdr, recs = _sam(path)
    sq = [(h.split("\t")[1][3:], int(h.split("\t")[2][3:])) for h in hdr if h.startswith("@SQ")]
    start = dict(zip([n for n, _ in sq], np.concatenate([[0], np.cumsum([ln for _, ln in sq])])[:-1]))
    off, nb = ref_layout(seg.ref_lens, w)
    m_start, m_len, m_read, has_d = [], [], [], np.zeros(len(recs), bool)
    for i, r in enumerate(recs):
        g = int(start[r[2]]) + int(r[3]) - 1
        for n, k in CIG.findall(r[5]):
            n = int(n)
            if k == "M":
                m_start.append(g); m_len.append(n); m_read.append(i)
            if k == "D":
                has_d[i] = True
            if k != "I":
                g += n
    m_start, m_len, m_read = np.array(m_start, np.int64), np.array(m_len, np.int64), np.array(m_read, np.int64)
    x = np.repeat(m_start, m_len) + np.arange(m_len.sum()) - np.repeat(np.cumsum(m_len) - m_len, m_len)   # every M-aligned base, read by read, ascending
    rid = np.repeat(m_read, m_len)
    si = np.searchsorted(seg.hap_off, x, side="right") - 1
    lifted = seg.kind[si] == 0
    r = seg.ref_pos[si] + x - seg.hap_off[si]
    b = np.where(lifted, off[seg.ref_rec[si]] + r // w, nb)
    bases = np.bincount(b, minlength=nb + 1).astype(np.uint64)
    idx = np.nonzero(lifted)[0]
    u, first = np.unique(rid[idx], return_index=True)
    reads = np.bincount(b[idx[first]], minlength=nb + 1).astype(np.uint64)
    reads[nb] += len(recs) - len(u)
    # what the reads reach
    touched = np.bincount(np.unique(rid * len(seg) + si) // len(seg), minlength=len(recs))    # segments a read's M runs touch
    _, first_base = np.unique(rid, return_index=True)
    same = (rid[1:] == rid[:-1]) & (x[1:] == x[:-1] + 1) & (si[1:] != si[:-1]) & lifted[1:] & lifted[:-1]
    back = same & (seg.ref_rec[si[1:]] == seg.ref_rec[si[:-1]]) & (r[1:] < r[:-1])
    reach = dict(cross=int((touched >= 2).sum()), cross2=int((touched >= 3).sum()), wholly_inserted=len(recs) - len(u),
                 starts_inserted=int((~lifted[first_base] & np.isin(np.arange(len(recs)), u)).sum()), back=len(np.unique(rid[1:][back])),
                 deletion_and_boundary=int((has_d & (touched >= 2)).sum()), n=len(recs))
    return reads, bases, len(recs), int(m_len.sum()), reach


def check_against_sam(out, res, name, w, seg):
    z = _arrays(out, name)
    reads, bases, copies = z["reads"], z["bases"], z["copies"]
    off, nb = ref_layout(seg.ref_lens, w)
    assert reads.dtype == bases.dtype == copies.dtype == np.uint64 and len(reads) == len(bases) == len(copies) == nb + 1 and (z["off"] == off.astype(np.uint64)).all()
    want_reads, want_bases, n_recs, m_sum, reach = lift_from_sam(out + "_" + name + ".sam", seg, w)
    assert n_recs == res[name]["reads_written"] > 500 and int(reads.sum()) == n_recs and int(bases.sum()) == m_sum
    assert (reads == want_reads).all(), np.nonzero(reads != want_reads)[0][:10]
    assert (bases == want_bases).all(), np.nonzero(bases != want_bases)[0][:10]
    assert (copies == copies_from_table(seg, seg.ref_lens, w)).all()
    assert res[name]["k_depth_lift"]["launches"] >= 1 and res[name]["k_depth_lift"]["units"] > 0
    return reads, bases, reach


@pytest.fixture(scope="module")
def sv_ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("svref")
    ref = str(d / "ref.fa")
    open(ref, "wb").write(gzip.open(os.path.join(SV, "ref.fa.gz")).read())
    return ref


def test_counters_equal_the_truth_sam_through_the_table(sv_ref, models, tmp_path):
    """1: the golden simuvars genome (1.5 Mb staged, CN 0 .. 8, three reference records), PE HiSeq2500 at 2x, bins of 1000 and 37:
    reads, bases and the pseudo-bin rebuilt from the SAM's POS and CIGAR through the downloaded table, bin for bin; copies = the
    host value; the device copy of the table = the host probe's."""
    legs = [dict(name="w%d" % w, wr=w, sam=True) for w in (1000, 37)]
    out, res = _run(tmp_path, legs, prof=models["Illumina_HiSeq2500"], ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, layout="PE", seed=41)
    seg = Segs(out)
    host, _ = scssim_amd.lift_plan_probe(sv_ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"))
    assert all((getattr(seg, k) == np.asarray(getattr(host, k), np.int64)).all() for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind")) and len(seg) == len(host)
    assert open(out + ".lift").read() == open(_write_host_lift(sv_ref, tmp_path)).read()
    for w in (1000, 37):
        reads, bases, reach = check_against_sam(out, res, "w%d" % w, w, seg)
        off, nb = ref_layout(seg.ref_lens, w)
        cn0 = np.arange(-(-149999 // w), 160000 // w)
        assert (reads[cn0] == 0).all() and (bases[cn0] == 0).all() and reads[:nb].sum() > 0   # no read lifts into the CN-0 stretch


def _write_host_lift(ref, tmp_path):
    p = str(tmp_path / "host.lift")
    scssim_amd.lift_plan_probe(ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"), p)
    return p


# ---- 2: the dense case
DENSE_INS, DENSE_STEP = 130, 170                           # bases of every insertion; reference bases from one insertion to the next (a deletion 40 behind each)
DENSE_COV = 14.0                                           # of the 60 kb REFERENCE, as genreads counts it (14x and not 3x: only two junctions jump backwards, and some reads of the job must cross one)


def write_dense_inputs(d, seed=5):
    """A 60 kb one-record reference and a variation file: every 170 bases an insertion of 130 bases and, 40 bases on, a deletion
    of 5 .. 40 bases; CN 4, CN 1 and CN 0 stretches of 4, 2 and 5 kb.  (The insertions are 130 bases and not 400: with reads of 75
    bases, boundaries must lie closer than two read lengths on average for most reads to cross one; 130 still holds a read of 125.)"""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 60000)]
    ref, var = str(d / "dense_ref.fa"), str(d / "dense_vars.txt")
    with open(ref, "wb") as f:
        f.write(b">1\n")
        f.write(np.concatenate([seq.reshape(-1, 60), np.full((1000, 1), 10, np.uint8)], axis=1).tobytes())
    lines, dels = ["# dense test variations"], [5, 12, 19, 26, 33, 40]
    for k, p in enumerate(range(300, 59500, DENSE_STEP)):
        lines.append("i\tchr1\t%d\t%s\thomo" % (p, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, DENSE_INS)]).decode()))
        lines.append("d\tchr1\t%d\t%d\thomo" % (p + 40, dels[k % len(dels)]))
    lines += ["c\tchr1\t10001\t14000\t4\t2", "c\tchr1\t25001\t27000\t1\t1", "c\tchr1\t40001\t45000\t0\t0"]
    open(var, "w").write("\n".join(lines) + "\n")
    return ref, var


def expected_reach(t, L, n_reads):
    """What reads of L bases whose starts are uniform over the staged records reach in this layout (the builder's check on the CPU):
    expected reads per condition.  Amplicons of 1 - 2 kb are many boundaries long, so their ends change little."""
    kind, hap_off, ln = np.asarray(t.kind), np.asarray(t.hap_off, np.int64), np.asarray(t.len, np.int64)
    total = int(np.asarray(t.hap_lens).sum())
    x = np.arange(total - L)
    s0, s1 = np.searchsorted(hap_off, x, side="right") - 1, np.searchsorted(hap_off, x + L - 1, side="right") - 1
    rec_end = np.cumsum(np.asarray(t.hap_lens, np.int64))
    ok = np.searchsorted(rec_end, x, side="right") == np.searchsorted(rec_end, x + L - 1, side="right")   # inside one record
    rp = np.asarray(t.ref_pos, np.int64)
    jump_back = np.zeros(len(t), bool)
    jump_back[1:] = (kind[1:] == 0) & (kind[:-1] == 0) & (rp[1:] < rp[:-1] + ln[:-1])
    cum_back = np.concatenate([[0], np.cumsum(jump_back)])
    f = lambda m: float((m & ok).sum()) / ok.sum() * n_reads
    return dict(cross=f(s1 > s0), cross2=f(s1 > s0 + 1), wholly_inserted=f((s1 == s0) & (kind[s0] == 1)), starts_inserted=f((s1 > s0) & (kind[s0] == 1)),
                back=f(cum_back[s1 + 1] - cum_back[s0 + 1] > 0))


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    ref, var = write_dense_inputs(d)
    table, _ = scssim_amd.lift_plan_probe(ref, None, var)
    return dict(ref=ref, var=var, table=table, dir=d)


@pytest.mark.parametrize("model,layout,L", [("Illumina_HiSeq2000", "SE", 75), ("Illumina_HiSeq2500", "PE", 125)])
def test_dense_layout(model, layout, L, dense, models, tmp_path):
    """2: boundaries closer than a read is long: insertions, deletions, CN 4 / 1 / 0 in 60 kb, sequenced at 14x with frequent
    sequencing indels (the exact-placement model of test_gpu_truth.py).  The builder's geometry is checked on the CPU first; what
    the reads of the job really reached is computed from the SAM and asserted, so that the test cannot pass beside the branches."""
    t = dense["table"]
    n_reads = DENSE_COV * float(np.asarray(t.ref_lens).sum()) / L                               # genreads takes the coverage of the reference length the record names state
    exp = expected_reach(t, L, n_reads)
    assert exp["cross"] > 0.55 * n_reads and min(exp["cross2"], exp["wholly_inserted"], exp["starts_inserted"], exp["back"]) >= 8, exp   # safe before relying on it
    prof = _exact_profile(models[model], str(tmp_path / "x.profile"), 0.004, 0.004)
    out, res = _run(tmp_path, [dict(name="w%d" % w, wr=w, sam=True) for w in (1000, 37)], prof=prof, ref=dense["ref"], vars=dense["var"], cov=DENSE_COV, layout=layout, seed=19, ber=0.0)
    seg = Segs(out)
    assert len(seg) == len(t) > 600
    for w in (1000, 37):
        reads, bases, reach = check_against_sam(out, res, "w%d" % w, w, seg)
    assert reach["cross"] > 0.5 * reach["n"], reach                                          # most reads cross a segment boundary
    assert reach["cross2"] >= 1 and reach["starts_inserted"] >= 1 and reach["wholly_inserted"] >= 1 and reach["back"] >= 1 and reach["deletion_and_boundary"] >= 1, reach
    nb = ref_layout(seg.ref_lens, 37)[1]
    assert reads[nb] == reach["wholly_inserted"] and (reads[-(-40000 // 37):45000 // 37] == 0).all()


def test_plain_genome_agrees_with_the_haplotype_track(models, tmp_path):
    """3: simuvars without variant files: one R segment per haplotype, so the reference track is the sum of the two haplotypes'
    tracks of k_depth in the same call, nothing is unlifted and every reference base has two copies."""
    ref = str(tmp_path / "ref.fa")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", "60000,40500", "--seed", "17", "--ref-out", ref])
    out, res = _run(tmp_path, [dict(name="both", w=1000, wr=1000)], prof=models["Illumina_HiSeq2500"], ref=ref, cov=3.0, layout="PE", seed=3)
    z, seg = _arrays(out, "both"), Segs(out)
    assert len(seg) == 4 and seg.ref_lens.tolist() == [60000, 40500] and z["hoff"].tolist() == [0, 60, 120, 161, 202] and z["off"].tolist() == [0, 60, 101]
    for name in ("reads", "bases"):
        h = z["h" + name]
        want = np.concatenate([h[0:60] + h[60:120], h[120:161] + h[161:202], [0]])
        assert (z[name] == want).all() and z[name].sum() > 500
    width = np.concatenate([np.full(60, 1000), np.full(40, 1000), [500]])
    assert (z["copies"][:101] == 2 * width).all() and z["copies"][101] == 0
    assert int(z["reads"].sum()) == res["both"]["reads_written"]


INV = dict(cov=24.0, layout="PE", seed=23)                 # the dense genome at 24x of its 60 kb reference: 5760 pairs -- 23 workgroups, two batches of 4096 at SCS_TEST_BATCH_SHIFT=12


@pytest.fixture(scope="module")
def invariance_reference(dense, models, tmp_path_factory):
    """The one PE job of checks 4 and 5 with every sink the default build offers, on one ctx: computed once, shared, never changed."""
    d = tmp_path_factory.mktemp("inv")
    legs = [dict(name="cb", wr=100, sam=True), dict(name="off", w=100, sink="files"), dict(name="on", w=100, wr=100, sink="files"),
            dict(name="parts", wr=100, sink="files", writers=3, generations=2), dict(name="bgzf", wr=100, sink="files", bgzf=True),
            dict(name="null", wr=100, sink="null"), dict(name="dev", wr=100, sink="device"), dict(name="again", wr=100)]
    out, res = _run(d, legs, prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], **INV)
    return out, res


def test_nothing_else_moves_and_sinks_do_not_matter(invariance_reference):
    """4, 5: the FASTQ files and the haplotype depth arrays with the reference track on are those with it off; a callback (checked
    against its SAM), files, 3 writers x 2 generations, BGZF, a NULL sink, the text left in device memory and a second callback
    yield after set_seed give the same counters."""
    out, res = invariance_reference
    reads, bases, _ = check_against_sam(out, res, "cb", 100, Segs(out))
    assert res["cb"]["reads_written"] > 2 * 4096                                              # more than 4096 pairs: two batches at SCS_TEST_BATCH_SHIFT=12
    for name in ("on", "parts", "bgzf", "null", "dev", "again"):
        z = _arrays(out, name)
        assert (z["reads"] == reads).all() and (z["bases"] == bases).all() and (z["copies"] == _arrays(out, "cb")["copies"]).all(), name
        assert res[name]["k_depth_lift"]["launches"] == res[name]["k_reads"]["launches"] >= 1      # one event pair per batch
    assert res["off"]["k_depth_lift"]["launches"] == 0 and res["off"]["k_depth_lift"]["units"] == 0
    off, on = _arrays(out, "off"), _arrays(out, "on")
    for k in ("hreads", "hbases", "hoff"):
        assert off[k].tobytes() == on[k].tobytes() and off[k].sum() > 0
    for m in ("_1.fq", "_2.fq"):
        want = open(out + "_off" + m, "rb").read()
        assert len(want) > 100000 and open(out + "_on" + m, "rb").read() == want == open(out + "_cb" + m, "rb").read()
        k = 0 if m == "_1.fq" else 1
        assert b"".join(open(p, "rb").read() for p in scssim_amd.part_paths(out + "_parts", 6)[k]) == want
        assert gzip.open(out + "_bgzf" + m + ".gz", "rb").read() == want


@pytest.mark.parametrize("knob,value", [("SCS_TEST_BATCH_SHIFT", "12"), ("SCS_TEST_BATCH_SHIFT", "8"), ("SCS_TEST_LIFT_SLOTS", "0"), ("SCS_TEST_LIFT_SLOTS", "4")])
def test_invariance_over_batch_cuts_and_table_sizes(knob, value, invariance_reference, dense, models, tmp_path):
    """5: batches of 4096 pairs and of 256 (a workgroup each), no LDS table at all (every add goes to memory) and a table of 4 slots
    (most adds overflow into direct ones): the arrays of the default build."""
    ref_out, _ = invariance_reference
    want = _arrays(ref_out, "cb")
    out, res = _run(tmp_path, [dict(name="v", wr=100)], env=seams_env(**{knob: value}), prof=models["Illumina_HiSeq2500"], ref=dense["ref"], vars=dense["var"], **INV)
    z = _arrays(out, "v")
    assert (z["reads"] == want["reads"]).all() and (z["bases"] == want["bases"]).all() and (z["copies"] == want["copies"]).all()
    if knob == "SCS_TEST_BATCH_SHIFT":
        assert res["v"]["k_depth_lift"]["launches"] == res["v"]["k_reads"]["launches"] >= (res["v"]["reads_written"] // 2) >> int(value) >= 1


_POS = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import scssim_amd
from scssim_amd import ScsError, SCS_EINVAL
g = scssim_amd.GenReads(seed=5)
g.simuvars(%(ref)r, %(snp)r, %(vars)r)
t = g.lift_segments()
n, nr = g.lift_info()
assert n == len(t) == 92 and nr == 3 and t.ref_lens.tolist() == [400000, 150000, 60000]
hap_lens = np.array(%(hap_lens)r, np.int64)
off = np.concatenate([[0], np.cumsum(hap_lens)])
rng = np.random.default_rng(1)
x = np.concatenate([rng.integers(0, off[-1], 100000), t.hap_off.astype(np.int64), (t.hap_off + t.len - 1).astype(np.int64)])
rec = np.searchsorted(off, x, side="right") - 1
rr, rp, k = g.lift_positions(rec, x - off[rec])
si = np.searchsorted(t.hap_off.astype(np.int64), x, side="right") - 1
assert (k == t.kind[si]).all() and (rr == t.ref_rec[si]).all() and (k == 1).sum() > 10
want = np.where(t.kind[si] == 0, t.ref_pos[si].astype(np.int64) + x - t.hap_off[si].astype(np.int64), t.ref_pos[si].astype(np.int64))
assert (rp.astype(np.int64) == want).all()
for bad_rec, bad_pos in ((0, hap_lens[0]), (5, hap_lens[5]), (6, 0)):
    try:
        g.lift_positions([0, bad_rec], [5, bad_pos])
    except ScsError as e:
        assert e.code == SCS_EINVAL and "outside" in str(e), e
    else:
        raise SystemExit("a position past its record was lifted")
assert g.lift_positions([], [])[0].size == 0
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''


def test_lift_positions(sv_ref, tmp_path):
    """6: 10^5 random staged positions and every segment's first and last base through k_lift_points against numpy.searchsorted on
    the downloaded table; a position past its record is refused."""
    host, _ = scssim_amd.lift_plan_probe(sv_ref, os.path.join(SV, "snp.txt"), os.path.join(SV, "vars.txt"))
    r = subprocess.run([sys.executable, "-c", _POS % dict(root=ROOT, ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), hap_lens=host.hap_lens.tolist())],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_step_flow_through_the_cli(sv_ref, models, golden_inputs, tmp_path):
    """7: `scssim simuvars --lift`, then `scssim genreads -i simu.fa --lift --depth-ref`: the depth file is the in-process route's for
    the same seed, byte for byte; the lift file is the host probe's and loads to the table simuvars kept; a lift file of another
    genome is refused with the record named."""
    prof, simu, lift, pre = models["Illumina_HiSeq2500"], str(tmp_path / "simu.fa"), str(tmp_path / "simu.lift"), str(tmp_path / "cli")
    r = subprocess.run([CLI, "simuvars", "-r", sv_ref, "-s", os.path.join(SV, "snp.txt"), "-v", os.path.join(SV, "vars.txt"), "-o", simu, "--lift", lift], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(simu, "rb").read() == gzip.open(os.path.join(SV, "expected_full.fa.gz")).read()   # the FASTA stays the reference binary's
    assert open(lift).read() == open(_write_host_lift(sv_ref, tmp_path)).read()
    r = subprocess.run([CLI, "genreads", "-i", simu, "-m", prof, "-c", "2", "-o", pre, "--seed", "77", "--lift", lift, "--depth-ref", pre + ".tsv", "--depth-bin", "1000"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, res = _run(tmp_path, [dict(name="api", wr=1000, sink="null", write=True)], prof=prof, ref=sv_ref, snp=os.path.join(SV, "snp.txt"), vars=os.path.join(SV, "vars.txt"), cov=2.0, layout="PE", seed=77)
    text = open(pre + ".tsv").read()
    assert text == open(out + "_api.tsv").read()
    lines = text.split("\n")
    z = _arrays(out, "api")
    assert lines[0] == "#record\tstart\tend\treads\tbases\tcopies" and lines[1].split("\t")[:3] == ["20", "0", "1000"] and lines[-1] == "" and len(lines) == 1 + 610 + 1 + 1
    assert lines[-2] == "#unlifted\t%d\t%d\t%d" % (z["reads"][-1], z["bases"][-1], z["copies"][-1])
    assert [int(ln.split("\t")[3]) for ln in lines[1:-2]] == z["reads"][:-1].tolist() and [int(ln.split("\t")[5]) for ln in lines[1:-2]] == z["copies"][:-1].tolist()
    # the loaded table is the kept one
    out2, _ = _run(tmp_path, [], out=str(tmp_path / "loaded"), prof=prof, fasta=simu, lift=lift, cov=2.0, layout="PE", seed=77)
    a, b = Segs(out), Segs(out2)
    assert all((getattr(a, k) == getattr(b, k)).all() for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind", "ref_lens")) and len(a) == len(b) == 92
    # another genome
    r = subprocess.run([CLI, "genreads", "-i", golden_inputs["g1_hiseq2500_pe"], "-m", prof, "-o", pre + "_x", "--lift", lift, "--depth-ref", pre + "_x.tsv"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "belongs to another genome" in r.stderr and "20_1_400000" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(pre + "_x.tsv") and not os.path.exists(pre + "_x_1.fq")


_OWN = r'''
import sys, ctypes
sys.path.insert(0, %(root)r)
import scssim_amd
from scssim_amd import ScsError, SCS_EINVAL, SCS_EIO, SCS_EOVERFLOW
def fails(f, code, *words):
    try:
        f()
    except ScsError as e:
        assert e.code == code and all(w in str(e) for w in words), (code, words, e)
        return
    raise SystemExit("no error: " + " ".join(words))
s = scssim_amd.GenReads(shard_count=2, shard_rank=0, profile=%(prof)r, seed=5)
s.set_depth_ref(1000)
fails(s.yield_reads, SCS_EINVAL, "scs_set_depth_ref", "sharded")
s.set_depth_ref(0)
fails(s.yield_reads, SCS_EINVAL, "scs_allocate_reads")       # the refusal is gone: what is missing now is the job itself
g = scssim_amd.GenReads(profile=%(prof)r, input_fasta=%(fa)r, coverage=2.0, seed=5)
fails(g.lift_info, SCS_EINVAL, "scs_simuvars", "scs_load_lift")
fails(lambda: g.write_lift(%(tmp)r + "/none.lift"), SCS_EINVAL, "no lift table")
fails(lambda: g.load_lift(%(tmp)r + "/missing.lift"), SCS_EIO, "can not open")
g.create_frags(); g.amplify(); g.allocate_reads(0)
g.set_depth_ref(1000)
fails(lambda: g.yield_reads(collect=False), SCS_EINVAL, "scs_load_lift", "scs_simuvars")   # a staged genome without a table
g.set_depth_ref(0)
g.yield_reads(collect=False)
# a genome with its table
g.simuvars(%(ref)r, None, None)
live = scssim_amd.live_resources()
fails(g.depth_ref_bins, SCS_EINVAL, "off")
g.set_depth_ref(1)
n, w = g.depth_ref_bins()
assert (n, w) == (610000, 1)
g.set_depth_ref(1000)
fails(g.depth_ref, SCS_EINVAL, "scs_download_depth_ref")     # before any yield
g.run(collect=False)
r, b, c, off = g.depth_ref()
assert int(r.sum()) == g.stats()["reads_written"] > 0 and len(r) == 611 and r[610] == 0 and int(c.sum()) == 2 * 610000
assert g.depth_ref_kernel_time()["launches"] >= 1
buf = (ctypes.c_uint64 * 611)()
g._L.scs_download_depth_ref.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
assert g._L.scs_download_depth_ref(g._ctx, buf, None, None, 610) == SCS_EOVERFLOW
assert g._L.scs_download_depth_ref(g._ctx, None, buf, None, 611) == 0 and list(buf) == b.tolist()
g.set_depth_ref(0)
g.set_seed(5); g.yield_reads(collect=False)
assert g.depth_ref_kernel_time()["launches"] == 0
fails(g.depth_ref, SCS_EINVAL, "off")
# staging another genome drops the table
g.load_genome(%(fa)r)
fails(g.lift_info, SCS_EINVAL, "no lift table")
g.close(); s.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
# more than 2^27 bins: refused by the layout before any GPU work, with the smallest admissible width
h = scssim_amd.GenReads(profile=%(prof)r, seed=5)
h.load_genome(%(fa)r); h.load_lift(%(big)r)
h.set_depth_ref(1)
fails(h.depth_ref_bins, SCS_EINVAL, "2^27", "smallest bin width it admits is 8")
h.create_frags(); h.amplify(); h.allocate_reads(0)
fails(lambda: h.yield_reads(collect=False), SCS_EINVAL, "2^27", "smallest bin width it admits is 8")
h.set_depth_ref(8)
assert h.depth_ref_bins() == (1 << 27, 8)
h.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0), scssim_amd.live_resources()
print("ok")
'''

_OWN_LIVE = r'''
import sys
sys.path.insert(0, %(root)r)
import scssim_amd
g = scssim_amd.GenReads(profile=%(prof)r, coverage=2.0, seed=5)
g.simuvars(%(ref)r, None, None)
g.run(collect=False)
before = scssim_amd.live_resources()
g.set_depth_ref(1000); g.set_seed(5); g.yield_reads(collect=False)
during = scssim_amd.live_resources()
g.set_depth_ref(0)
after = scssim_amd.live_resources()
assert during[0] > before[0] and after == before, (before, during, after)
g.close()
assert scssim_amd.live_resources() == (0, 0, 0, 0)
print("ok")
'''


def test_refusals_and_ownership(sv_ref, models, golden_inputs, tmp_path):
    """8: a sharded ctx and a genome without a table are refused at the yield call by name; no download before a yield, none into too
    small a buffer; more than 2^27 bins name the smallest admissible width; staging a new genome drops the table; the live resources
    read the same before the feature goes on and after it goes off, and zero after scs_destroy."""
    fa = golden_inputs["g1_hiseq2500_pe"]
    names, _, _ = scssim_amd.fasta_probe(fa)
    scssim_amd.fasta_write_index(fa)
    lens = [int(ln.split("\t")[1]) for ln in open(fa + ".fai").read().split("\n") if ln]
    big = str(tmp_path / "big.lift")                       # the staged records as copies of a reference record of 2^30 bases
    with open(big, "w") as f:
        f.write("##scssim-lift v1\n#ref\tbig\t%d\n" % (1 << 30) + "".join("#hap\t%s\t%d\n" % (n, ln) for n, ln in zip(names, lens)))
        f.write("".join("%s\t0\t%d\tbig\t%d\t%d\tR\n" % (n, ln, (1 << 30) - ln, 1 << 30) for n, ln in zip(names, lens)))
    r = subprocess.run([sys.executable, "-c", _OWN % dict(root=ROOT, prof=models["Illumina_HiSeq2500"], fa=fa, ref=sv_ref, tmp=str(tmp_path), big=big)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-c", _OWN_LIVE % dict(root=ROOT, prof=models["Illumina_HiSeq2500"], ref=sv_ref)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
