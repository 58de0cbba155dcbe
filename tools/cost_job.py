"""What the tools/*_cost.py scripts share: the chr20-size inputs (the genome of tools/make_genome.py at seed 20 with an N block of
60000, the XTen model at read length 150; for the tools that go through scs_simuvars the reference and a variation file made
here), the ctx, the warm-up yield, the leg x repeat loop with its clean-up, the common arguments, the JSON line, and the two ways
a tool runs itself again in a fresh child: with a seam of the seams build set (a seam is read once per process) and with the
parent commit's library (a library is loaded once per process).  A tool keeps what its legs switch on and what they record."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def add_common(ap, repeats, warm="yield", slots=None, writers=False, simuvars=False):
    """--repeats [--slots] [--writers] --out-dir --bases --coverage [--cnvs --indels]; --legs is the tool's own"""
    ap.add_argument("--repeats", type=int, default=repeats, help="runs of every leg after one unrecorded warm-up " + warm)
    if slots:
        ap.add_argument("--slots", type=int, default=None, help="entries of %s's LDS table (the seams build; 0: none).  Default: the product build" % slots)
    if writers:
        ap.add_argument("--writers", type=int, default=1)
    ap.add_argument("--out-dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--bases", type=int, default=63025520)
    ap.add_argument("--coverage", type=float, default=30.0)
    if simuvars:
        ap.add_argument("--cnvs", type=int, default=120)
        ap.add_argument("--indels", type=int, default=150, help="insertions, and as many deletions")


def run(a, job, seam=None, parent_legs=None):
    """job(a, td) in a temporary directory under --out-dir.  seam: with --slots N the tool runs again as a fresh child with
    seam=N and the seams library set, and this process ends with its status.  parent_legs: with --parent-lib PATH three fresh
    children run instead -- the parent commit's library on these legs, this tree, the parent again."""
    if seam and a.slots is not None and os.environ.get(seam) != str(a.slots):
        env = dict(os.environ, SCSSIM_HIP_LIB=os.path.join(ROOT, "scssim_amd", "libscssim_hip_seams.so"), **{seam: str(a.slots)})
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    if parent_legs and a.parent_lib:
        rest = [x for i, x in enumerate(sys.argv[1:]) if x != "--parent-lib" and (i == 0 or sys.argv[i] != "--parent-lib") and not x.startswith("--parent-lib=")]
        for lib, extra in ((a.parent_lib, ["--legs", parent_legs]), (None, []), (a.parent_lib, ["--legs", parent_legs])):
            rc = subprocess.call([sys.executable, os.path.abspath(sys.argv[0])] + rest + extra, env=dict(os.environ, SCSSIM_HIP_LIB=os.path.abspath(lib)) if lib else dict(os.environ))
            if rc:
                sys.exit(rc)                                   # (nothing more is started after a failure)
        return
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        job(a, td)


def emit(rec, log=None, lib=None):
    """One JSON line on stdout; --log FILE: appended there too, with the library that ran."""
    print(json.dumps(rec), flush=True)
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(rec, lib=lib)) + "\n")


def _make_genome(path, bases, ref):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), "--lengths", str(bases), "--seed", "20", "--n-block", "60000", "--ref-out" if ref else "--simu-out", path])


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


def open_ctx(a, td, simuvars=False, cnvs=120, indels=150):
    """The ctx of the job at seed 220 over the inputs made in td: the staged FASTA given to the constructor, or (simuvars) the
    reference and the variation file, which the caller stages: returns (g, ref, var) then, and g alone otherwise."""
    import scssim_amd
    prof, src = os.path.join(td, "m.profile"), os.path.join(td, "x.profile")
    open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "models", "Illumina_HiSeqXTen.profile.gz")).read())
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_profile.py"), src, prof, "--read-length", "150"])
    if simuvars:
        ref, var = os.path.join(td, "chr20_ref.fa"), os.path.join(td, "vars.txt")
        _make_genome(ref, a.bases, True)
        write_variations(var, a.bases, cnvs, indels)
        return scssim_amd.GenReads(profile=prof, coverage=a.coverage, seed=220), ref, var
    fa = os.path.join(td, "chr20.fa")
    _make_genome(fa, a.bases, False)
    return scssim_amd.GenReads(profile=prof, input_fasta=fa, coverage=a.coverage, seed=220)


def allocate(g):
    g.create_frags(); g.amplify(); g.allocate_reads(0)


def warm_up(g, td, writers=1):
    g.yield_reads_files(os.path.join(td, "reads_warm"), writers)      # the buffers, the pinned slots, the page cache


def legs(a, td, prefixes=("reads_",), names=None):
    """Every leg of --legs, --repeats times over; after each, the files it left in td under these prefixes are removed."""
    for leg in [l for _ in range(a.repeats) for l in names or a.legs.split(",")]:
        yield leg
        for f in os.listdir(td):
            if f.startswith(prefixes):
                os.unlink(os.path.join(td, f))
