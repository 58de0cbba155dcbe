"""The attach kernels of the amplification stage (k_attach<FROM_FRAG, G>, k_attach_dense: scs_k_amplify.hip) outside the one regime
every other test runs them in -- a primer budget of 6.5 per template.  Five jobs (tests/attach_cases.py), each proven from the
oracle's dump to reach the branch it is named for before the GPU is touched:
  high_budget      budgets of 65: most semi amplicons span two chunks of k_attach_dense, some are abandoned (> 50 tries) in one
                   chunk with further chunks to come (carry_abort / carry_v), fragments go into a second round of 64 primers;
  three_chunks     budgets of 131: three and four chunks per template, templates that fill a whole chunk;
  dry_high_budget  the same budgets on a genome of A / T runs: primer types run dry, exact_stock's undo pass runs over cut templates;
  sparse           budgets of 0.2: more templates in a chunk than it has bitmap rows, the chunk ends early;
  row_overflow     budgets of 1.1 on 4 Mb: hundreds of such chunks, each followed by one whose first template is a new one on row 0.
                   A row 0 left uncleared there shows only when that template proposes a position the row's last owner took:
                   about 2 % of the cases (two templates of 1.6 primers, positions uniform over 1 .. 974 places), so 300 of them
                   are asked for.
high_budget and dry_high_budget run in five variants -- the dense pass, and lane groups per template of 8, 2, 4 and 16 (SCS_ATTACH_GROUPS,
SCS_ATTACH_G: k_attach<false, G>) --, three_chunks as dense and groups of 4, sparse and row_overflow as dense and groups of 8, each run
in a child process of its own (the seams are read once per process); dry_high_budget also as two shards (the segment-by-segment
re-run: launch_attach_semis on a range, with undo, at both production group widths).  Everything is compared exactly against the
oracle in counter mode: amplicon tables, primer stock, read numbers, FASTQ."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import attach_cases as ac
from conftest import ROOT, seams_env

import scssim_amd

pytestmark = pytest.mark.gpu

VARIANTS = {"dense": {},
            "groups8": dict(SCS_ATTACH_GROUPS="1"),
            "groups2": dict(SCS_ATTACH_GROUPS="1", SCS_ATTACH_G="2"),
            "groups4": dict(SCS_ATTACH_GROUPS="1", SCS_ATTACH_G="4"),
            "groups16": dict(SCS_ATTACH_GROUPS="1", SCS_ATTACH_G="16")}
RUNS = ([("high_budget", v) for v in VARIANTS] + [("dry_high_budget", v) for v in VARIANTS] +
        [("three_chunks", "dense"), ("three_chunks", "groups4"), ("sparse", "dense"), ("sparse", "groups8"),
         ("row_overflow", "dense"), ("row_overflow", "groups8")])


@pytest.fixture(scope="module")
def attach_oracle(oracle_bin, models, tmp_path_factory):
    """case -> the oracle's run of it (once per case): genome, dump read into arrays, FASTQ, and the precondition counts.  Fails when
    the dump does not show the case reaching its branch."""
    cache = {}

    def get(case):
        if case not in cache:
            d = tmp_path_factory.mktemp(case)
            fa = ac.write_genome(case, str(d / "simu.fa"))
            prefix = str(d / "orc")
            subprocess.check_call([oracle_bin, "genreads", "-i", fa, "-m", models[ac.MODEL], "-o", prefix, "--rng", "counter", "--seed", str(ac.SEED),
                                   "-t", "8", "-q", "--dump", prefix] + ac.oracle_args(case), timeout=120)
            o = dict(fasta=fa, prefix=prefix, dir=d, semis=ac.load_amps(prefix + ".semis.tsv"), fulls=ac.load_amps(prefix + ".fulls.tsv"))
            o["stock"], o["prim"] = ac.load_primer_stock(prefix + ".primers.tsv", ac.CASES[case]["primers"])
            o["readnum"] = ac.load_read_numbers(prefix + ".readnum.tsv", o["fulls"]["uid"].size)
            o["fq"] = [open(prefix + s, "rb").read() for s in ("_1.fq", "_2.fq")]
            o["counts"], o["unmet"] = ac.preconditions(case, o["semis"], o["prim"])
            cache[case] = o
        o = cache[case]
        c = o["counts"]
        print("%s: %d semis, %d fulls; budgets mean %.2f max %d, above 56 / 112 / 168: %d / %d / %d; certain aborts with carry %d (of %d unplaceable); "
              "fragment passes with a second round %d (largest primer index %d); dry types %d of %d used; most templates in a window of 56 items %d, chunks cut short by the bitmap rows %d"
              % (case, c["semis"], o["fulls"]["uid"].size, c["mean_budget"], c["max_budget"], c["above_56"], c["above_112"], c["above_168"],
                 c["certain_aborts_with_carry"], c["unplaceable"], c["fragment_second_rounds"], c["max_fragment_primer"], c["dry_types"], c["types_used"], c["densest_window"], c["row_split_restarts"]))
        assert not o["unmet"], "%s does not reach the branch it is there for: %s" % (case, "; ".join(o["unmet"]))
        return o
    return get


def _first_diff(table, column, got, want):
    assert got.shape == want.shape, "%s.%s: %s values, the oracle has %s" % (table, column, got.shape, want.shape)
    d = np.nonzero(got != want)[0]
    assert d.size == 0, "%s.%s differs in %d rows, first row %d: got %s want %s" % (table, column, d.size, d[0], got[d[0]], want[d[0]])


def _compare_tables(r, o):
    for name in ("semis", "fulls"):
        want = o[name]
        assert r[name + "_parent"].size == want["parent"].size, "%s count: %d, the oracle has %d" % (name, r[name + "_parent"].size, want["parent"].size)
        for col in ("parent", "spos", "len", "gc", "uid") + (("primers",) if name == "semis" else ()):
            _first_diff(name, col, r[name + "_" + col].astype(np.uint64), want[col])
        _first_diff(name, "error count", r[name + "_nerr"], want["nerr"])
        for k in range(4):
            has = want["nerr"] > k
            _first_diff(name, "error %d" % k, np.where(has, r[name + "_errs"][:, k], 0), want["errs"][:, k])


@pytest.mark.parametrize("case,variant", RUNS)
def test_attach_matches_oracle(case, variant, attach_oracle, models):
    o = attach_oracle(case)
    c = ac.CASES[case]
    prefix = str(o["dir"] / variant)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attach_gpu_worker.py"), o["fasta"], models[ac.MODEL], prefix, ac.COVERAGE, str(ac.SEED),
                        str(c["primers"]), repr(c["gamma"])], env=seams_env(**VARIANTS[variant]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "libscssim_hip_seams.so" in r.stdout, "the child must load the seams build: " + r.stdout[-500:]
    r = np.load(prefix + ".npz")
    assert tuple(r["amp_limits"]) == (ac.AMP_MIN, ac.AMP_MAX), "the preconditions of attach_cases.py count with other amplicon limits than the library's"
    checks, dry_passes, rounds = (int(v) for v in r["stock_stats"])
    print("%s / %s: %d stock checks, %d passes with a dry type, %d rounds" % (case, variant, checks, dry_passes, rounds))
    if case == "dry_high_budget":
        assert dry_passes >= 1 and rounds >= 1, "no pass was run again for a dry primer type"
    _compare_tables(r, o)
    _first_diff("primer stock", "copies left", r["stock"], o["stock"])
    _first_diff("read numbers", "reads", r["readnum"], o["readnum"])
    for k, suffix in enumerate(("_1.fq", "_2.fq")):
        got = open(prefix + suffix, "rb").read()
        assert len(o["fq"][k]) > 1000
        assert got == o["fq"][k], "%s differs from the oracle's (%d / %d bytes)" % (suffix, len(got), len(o["fq"][k]))


@pytest.mark.parametrize("width", ["default", "4"])
def test_dry_high_budget_sharded_equals_whole_job(width, attach_oracle, models, tmp_path):
    """Two shards, host hooks: the pass in which a type runs dry is run again segment by segment (launch_attach_semis on a range of
    the list, exact_stock's undo on it) -- with 8 lanes per template, the choice below 2^18 semi amplicons, and with 4, the choice
    above.  The merged shards equal the whole job's files, the oracle's."""
    o = attach_oracle("dry_high_budget")
    c = ac.CASES["dry_high_budget"]
    n_dry = o["counts"]["dry_types"]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = str(s.getsockname()[1]); s.close()
    knobs = {} if width == "default" else dict(SCS_ATTACH_G=width)
    procs = []
    for rank in range(2):
        env = seams_env(dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, LOCAL_RANK="0"), **knobs)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_worker.py"), o["fasta"], models[ac.MODEL], str(tmp_path / "shard"),
                                       ac.COVERAGE, "PE", str(ac.SEED), "host", "0", str(c["primers"]), repr(c["gamma"])],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    rounds = 0
    for out in outs:
        f = [l for l in out.splitlines() if l.startswith("STOCK ")][0].split()
        assert int(f[3]) >= 1 and int(f[5]) == n_dry, "every shard must see the dry types of the whole job: " + " ".join(f)
        rounds += int(f[4])
    print("sharded, width %s: %d undo rounds inside the segments (counted by their owners)" % (width, rounds))
    assert rounds >= 1, "no segment was run again with undo"
    scssim_amd.merge_fastq_shards(str(tmp_path / "shard"), 2, paired=True)
    for k, suffix in enumerate(("_1.fq", "_2.fq")):
        assert open(str(tmp_path / "shard") + suffix, "rb").read() == o["fq"][k], "sharded GPU job differs from the whole job (%s)" % suffix
