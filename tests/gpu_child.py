"""How the GPU tests run a job: in a fresh child process under its own time limit, the checks in the parent.  This module is the
one place that knows how.  Parent side (a test module imports it): run_child and the sv_ref fixture.  Child side (the -c script
imports it; run_child has put tests/ and the repository on its sys.path): job_args, open_job, yield_leg, device_buffers,
leg_env, fails, emit.  A module's child script keeps what is its own -- the feature's switches per leg, what it reads back, its
ownership checks -- and takes the prologue, the sinks and the protocol from here.  Not a conftest, not collected."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


# ---- parent side

def run_child(script, args=None, env=None, timeout=300, ok=False):
    """`python -c script` as a fresh child, `args` as JSON in its argv (job_args() there).  Exit status 0 is asserted, the tails
    of stdout and stderr in the message.  Returns the dict of the child's last "RESULT " line (emit() there); ok=True: the child
    prints "ok" instead, that is asserted and its stdout returned."""
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]\n" % (TESTS, ROOT) + script, json.dumps(args)],
                       env=env or dict(os.environ), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and (not ok or "ok" in r.stdout), "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    if ok:
        return r.stdout
    return json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])


if "pytest" in sys.modules:                                 # (a child has no use for it and does not pay for the import)
    import pytest

    @pytest.fixture(scope="module")
    def sv_ref(tmp_path_factory):
        """The reference of the golden simuvars genome, unpacked; a test module imports the fixture by name and gets its own copy."""
        import gzip
        ref = str(tmp_path_factory.mktemp("svref") / "ref.fa")
        open(ref, "wb").write(gzip.open(os.path.join(TESTS, "golden", "simuvars", "ref.fa.gz")).read())
        return ref


# ---- child side

def job_args():
    return json.loads(sys.argv[1])


def emit(res):
    print("RESULT " + json.dumps(res))


def open_job(a, lift_file=False, segs=False, allocate=True):
    """The ctx of a job from its arguments {prof, cov, seed, layout, isize, ber, out} and its genome by one of three routes:
    fa (a staged FASTA, given to the constructor), fasta + lift (a staged FASTA, then its lift file), ref [+ snp, vars, out_fasta]
    (scs_simuvars).  lift_file: write the table to <out>.lift; segs: dump its segments to <out>_segs.npz (both only read the
    table); allocate: fragments, amplification and read allocation, so that the next call is a yield."""
    import scssim_amd
    kw = dict(input_fasta=a["fa"]) if "fa" in a else {}
    g = scssim_amd.GenReads(profile=a["prof"], coverage=a["cov"], layout=a.get("layout", "PE"), seed=a["seed"], isize=a.get("isize", 260), ber=a.get("ber", 3.4e-4), **kw)
    if "fasta" in a:
        g.load_genome(a["fasta"]); g.load_lift(a["lift"])
    elif "ref" in a:
        g.simuvars(a["ref"], a.get("snp"), a.get("vars"), a.get("out_fasta"))
    if lift_file:
        g.write_lift(a["out"] + ".lift")
    if segs:
        import numpy as np
        t = g.lift_segments()
        np.savez(a["out"] + "_segs.npz", hap_off=t.hap_off, len=t.len, ref_pos=t.ref_pos, ref_rec=t.ref_rec, kind=t.kind, ref_lens=t.ref_lens)
    if allocate:
        g.create_frags(); g.amplify(); g.allocate_reads(0)
    return g


@contextlib.contextmanager
def device_buffers(cap, n=2):
    """n device buffers of cap bytes each from hipMalloc, as c_void_p; freed on the way out."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]; hip.hipFree.argtypes = [ctypes.c_void_p]
    ptrs = [ctypes.c_void_p() for _ in range(n)]
    try:
        for p in ptrs:
            assert hip.hipMalloc(ctypes.byref(p), cap) == 0
        yield ptrs
    finally:
        for p in ptrs:
            hip.hipFree(p)


def yield_leg(g, pre, leg):
    """One yield into the leg's sink: callback (the default: <pre>_1.fq, <pre>_2.fq written here), null, files (the names of
    yield_reads_files under <pre>; writers, generations, bgzf) or device (the text stays in two buffers of 64 MB)."""
    kind = leg.get("sink", "callback")
    if kind == "callback":
        f1, f2 = g.yield_reads()
        open(pre + "_1.fq", "wb").write(f1); open(pre + "_2.fq", "wb").write(f2)
    elif kind == "null":
        g.yield_reads(collect=False)
    elif kind == "files":
        g.yield_reads_files(pre, leg.get("writers", 1), leg.get("generations", 1), bgzf=leg.get("bgzf", False))
    else:
        assert kind == "device", kind
        with device_buffers(64 << 20) as (d1, d2):
            g.yield_reads_device(d1, 64 << 20, d2, 64 << 20)


@contextlib.contextmanager
def leg_env(env):
    """The seams of one leg or variant (the seams build reads these at every call), gone again afterwards."""
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def fails(f, code, *words):
    """f() must raise ScsError with this code and every word in its message."""
    from scssim_amd import ScsError
    try:
        f()
    except ScsError as e:
        assert e.code == code and all(w in str(e) for w in words), (code, words, str(e))
        return
    raise SystemExit("no error: " + " ".join(words))
