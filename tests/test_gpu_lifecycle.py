"""What a ctx holds on the device and what it leaves behind: every device buffer, stream, event and pinned block of the library is an
owning handle (csrc/scs_ctx.h) that counts itself in a process-wide census (scs_live_resources).  One child process runs small jobs
into every kind of target -- each on a GenReads of its own, so that every lazily made group of resources is created somewhere -- and
records the census before and after each close(); a second process is only the other rank of the sharded job.  The checks run here.
SCS_VMM_FROM_MB=1 puts these jobs' buffers on the mapped-range path, SCS_TEST_BATCH_SHIFT=9 gives them several batches."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT, seams_env

pytestmark = pytest.mark.gpu

_CHILD = r'''
import gzip, hashlib, json, os, sys
sys.path.insert(0, %(root)r)
import torch
import torch.distributed as dist
import scssim_amd
from scssim_amd.dist import Collectives
A = json.loads(%(args)r)
live = scssim_amd.live_resources
sha = lambda b: hashlib.sha256(b).hexdigest()
cat = lambda files: b"".join(open(f, "rb").read() for f in files)
rep = dict(start=live(), jobs=[])

def ctx(case, **kw):
    c = A["cases"][case]
    g = scssim_amd.GenReads(profile=c["prof"], input_fasta=c["fa"], coverage=2.0, layout=c["layout"], seed=c["seed"], **kw)
    return g, c["layout"] == "PE"

def to_device(g, paired, out):
    d1, d2 = (torch.empty(64 << 20, dtype=torch.uint8, device="cuda") for _ in range(2))
    n1, n2, _ = g.yield_reads_device(d1.data_ptr(), d1.numel(), d2.data_ptr(), d2.numel())
    return [bytes(d1[:n1].cpu().numpy()), bytes(d2[:n2].cpu().numpy())]

def to_callback(g, paired, out):
    return list(g.yield_reads())

def to_files(g, paired, out, bgzf=False):
    g.yield_reads_files(out, writers=3, generations=2, bgzf=bgzf)
    parts = [cat(m) for m in scssim_amd.part_paths(out, 6, paired, ".fq.gz" if bgzf else ".fq")]
    return [gzip.decompress(p) if bgzf else p for p in parts]

def to_truth(g, paired, out):
    g.set_truth_sam(out + ".sam")
    g.yield_reads_files(out)
    assert g.truth_bytes() == os.path.getsize(out + ".sam") > 0
    return [cat(m) for m in scssim_amd.part_paths(out, 1, paired)]

def job(case, target, run, setup=None, **kw):
    g, paired = ctx(case, **kw)
    if setup:
        setup(g)
    g.create_frags(); g.amplify(); g.allocate_reads(0)
    text = run(g, paired, os.path.join(A["dir"], case + "_" + target))
    before = live(); g.close()
    rep["jobs"].append(dict(case=case, target=target, before=before, after=live(), text=[sha(t) for t in (text + [b""])[:2]], bytes=sum(map(len, text))))

# the sharded job first (the other rank is waiting for this one): shard 0 of 2 on torch's stream, device hooks over gloo
dist.init_process_group("gloo")
torch.cuda.set_device(0)
stream = torch.cuda.Stream()
coll = Collectives(device="cpu", stream=stream)
shard = os.path.join(A["dir"], "shard")
job("g1", "sharded", lambda g, paired, out: g.yield_reads_files(shard) or [], setup=lambda g: g.set_collectives(coll, device_hooks=True),
    stream=stream.cuda_stream, shard_rank=0, shard_count=2)
dist.barrier()                                             # the other rank's shard is written
dist.destroy_process_group()
scssim_amd.merge_fastq_shards(shard, 2, paired=True)
rep["sharded_text"] = [sha(open(shard + s, "rb").read()) for s in ("_1.fq", "_2.fq")]

for case in ("g1", "g3"):
    job(case, "device", to_device)
    job(case, "callback", to_callback)
    job(case, "files", to_files)
    job(case, "bgzf", lambda g, paired, out: to_files(g, paired, out, bgzf=True))
    job(case, "truth", to_truth)

# a sink that fails on its second batch; the ctx must stay usable and free everything at the end
g, _ = ctx("g1")
g.create_frags(); g.amplify(); g.allocate_reads(0)
calls = [0]
def failing(_u, _p1, _n1, _p2, _n2):
    calls[0] += 1
    return 1 if calls[0] >= 2 else 0
try:
    g.yield_reads_sink(failing); code = 0
except scssim_amd.ScsError as e:
    code = e.code
again = g.run()
before = live(); g.close()
rep["failing"] = dict(code=code, calls=calls[0], text=[sha(t) for t in again], before=before, after=live())

# two contexts alive at once, closed in creation order
a, _ = ctx("g1"); b, _ = ctx("g3")
a.run(); b.run()
both = live(); a.close(); one = live(); b.close()
rep["two"] = dict(both=both, one=one, none=live())
json.dump(rep, open(os.path.join(A["dir"], "report.json"), "w"))
'''

# What each target must at least hold before close(): (streams, events).  Every job makes the semi pass' stream with its 2 events and the
# reads pre-pass' stream with its 5; a ctx on a stream of its own counts that one too; a sink adds the copy stream, 4 events and one
# event per pinned slot (writers + 2); BGZF adds 2 events, truth 1.  The kernel timers' events come on top (hence "at least").
_AT_LEAST = {"device": (3, 7), "callback": (4, 14), "files": (4, 16), "bgzf": (4, 18), "truth": (4, 15), "sharded": (3, 14)}


@pytest.fixture(scope="module")
def report(models, golden_inputs, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lifecycle"))
    cases = {"g1": dict(fa=golden_inputs["g1_hiseq2500_pe"], prof=models["Illumina_HiSeq2500"], layout="PE", seed=5),
             "g3": dict(fa=golden_inputs["g3_hiseq2000_se"], prof=models["Illumina_HiSeq2000"], layout="SE", seed=6)}
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = str(s.getsockname()[1]); s.close()
    env = lambda rank: seams_env(SCS_VMM_FROM_MB="1", SCS_TEST_BATCH_SHIFT="9", RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, LOCAL_RANK="0")
    limit = ["timeout", "-k", "10", "300"]
    g1 = cases["g1"]
    peer = subprocess.Popen(limit + [sys.executable, os.path.join(ROOT, "tests", "dist_gpu_worker.py"), g1["fa"], g1["prof"], os.path.join(d, "shard"), "2", "PE", str(g1["seed"]), "device", "0"],
                            env=env(1), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        code = _CHILD % dict(root=ROOT, args=json.dumps(dict(dir=d, cases=cases)))
        r = subprocess.run(limit + [sys.executable, "-c", code], env=env(0), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        peer_out = peer.communicate(timeout=60)[0]
        assert peer.returncode == 0, peer_out
    finally:
        if peer.poll() is None:
            peer.kill(); peer.communicate()
    return json.load(open(os.path.join(d, "report.json")))


def test_nothing_is_held_before_the_first_ctx(report):
    assert report["start"] == [0, 0, 0, 0]


@pytest.mark.parametrize("case,target", [(c, t) for c in ("g1", "g3") for t in ("device", "callback", "files", "bgzf", "truth")] + [("g1", "sharded")])
def test_close_frees_everything_the_target_made(report, case, target):
    """Before close(): device bytes, pinned bytes and at least the streams and events the target creates.  After: exactly nothing."""
    (j,) = [j for j in report["jobs"] if (j["case"], j["target"]) == (case, target)]
    dev, streams, events, pinned = j["before"]
    print(case, target, "before close:", j["before"])
    assert dev > 0 and pinned >= 256 and streams >= _AT_LEAST[target][0] and events >= _AT_LEAST[target][1]
    if target not in ("device", "sharded"):
        assert pinned >= 1 << 20, "a sink's pinned slot"
    assert j["after"] == [0, 0, 0, 0]


def test_every_target_got_the_same_text(report):
    """Not what this file is about, but free: whatever the target, the job's FASTQ text is the device target's (BGZF inflated, parts and
    shards concatenated)."""
    for case in ("g1", "g3"):
        want = [j for j in report["jobs"] if (j["case"], j["target"]) == (case, "device")][0]
        assert want["bytes"] > 100000
        for j in report["jobs"]:
            if j["case"] == case and j["target"] != "sharded":
                assert j["text"] == want["text"], (case, j["target"])
    assert report["sharded_text"] == [j for j in report["jobs"] if (j["case"], j["target"]) == ("g1", "device")][0]["text"]


def test_failing_sink_leaves_a_usable_ctx_that_frees_everything(report):
    f = report["failing"]
    assert f["code"] == 2 and f["calls"] >= 2                   # SCS_EIO, from the sink's second batch
    assert f["text"] == [j for j in report["jobs"] if (j["case"], j["target"]) == ("g1", "device")][0]["text"]
    assert f["before"][0] > 0 and f["after"] == [0, 0, 0, 0]


def test_two_contexts_free_their_own(report):
    t = report["two"]
    assert all(b > o > 0 for b, o in zip(t["both"], t["one"])), t
    assert t["none"] == [0, 0, 0, 0]
