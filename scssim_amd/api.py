import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # SCSSIM_HIP_LIB: another build of the same library (A/B measurements of a kernel change on one box: tools/ab_kernels.sh)
    return os.environ.get("SCSSIM_HIP_LIB") or os.path.join(HERE, "libscssim_hip.so")


def build(verbose=False):
    """Compile the HIP library and the CLI for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc"), "-j4"] + ([] if verbose else ["-s"]))


SCS_OK, SCS_EINVAL, SCS_EIO, SCS_EDEVICE, SCS_EOVERFLOW = 0, 1, 2, 3, 4       # include/scssim_hip.h


class ScsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("scssim_hip error %d: %s" % (code, msg))
        self.code = code


class _Config(C.Structure):
    _fields_ = [("device", C.c_int), ("stream", C.c_void_p), ("seed", C.c_uint64), ("primers", C.c_long),
                ("gamma", C.c_double), ("coverage", C.c_double), ("isize", C.c_int), ("paired", C.c_int),
                ("ber", C.c_double), ("amplicon_min_len", C.c_int), ("amplicon_max_len", C.c_int),
                ("frag_size", C.c_int), ("frag_min", C.c_int), ("frag_max", C.c_int),
                ("shard_rank", C.c_int), ("shard_count", C.c_int), ("verbose", C.c_int)]


class _Stats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("genome_bases", C.c_uint64), ("fragments", C.c_uint64),
                ("semi_amplicons", C.c_uint64), ("full_amplicons", C.c_uint64), ("primers_left", C.c_uint64),
                ("reads_requested", C.c_uint64), ("pairs_written", C.c_uint64), ("reads_written", C.c_uint64),
                ("fastq_bytes", C.c_uint64 * 2), ("algorithmic_bytes", C.c_uint64), ("t_stage", C.c_double * 8), ("sink_bytes", C.c_uint64 * 2), ("staged_bases", C.c_uint64),
                ("stock_checks", C.c_uint64), ("stock_exhausted_passes", C.c_uint64), ("stock_rounds", C.c_uint64)]


_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t)
_lib = None


def load_library():
    """dlopen the in-tree library; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError("%s is missing: run scssim_amd.build() / make -C scssim_amd/csrc (no CPU fallback exists)" % p)
    L = C.CDLL(p)
    L.scs_last_error.restype = C.c_char_p
    L.scs_last_error.argtypes = [C.c_void_p]
    L.scs_create.argtypes = [C.POINTER(_Config), C.POINTER(C.c_void_p)]
    L.scs_destroy.argtypes = [C.c_void_p]
    L.scs_set_seed.argtypes = [C.c_void_p, C.c_uint64]
    L.scs_load_profile.argtypes = [C.c_void_p, C.c_char_p]
    L.scs_read_length.argtypes = [C.c_void_p]
    L.scs_load_genome_fasta.argtypes = [C.c_void_p, C.c_char_p]
    L.scs_upload_genome.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]
    L.scs_upload_genome_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_void_p]
    for f in ("scs_create_frags", "scs_amplify"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.scs_allocate_reads.argtypes = [C.c_void_p, C.c_uint64]
    L.scs_yield_reads.argtypes = [C.c_void_p, _SINK, C.c_void_p]
    L.scs_run_genreads.argtypes = [C.c_void_p, _SINK, C.c_void_p]
    L.scs_yield_reads_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.scs_yield_reads_files.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.scs_merge_fastq_shards.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.scs_comm_unique_id.argtypes = [C.c_void_p]
    L.scs_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.scs_get_stats.argtypes = [C.c_void_p, C.POINTER(_Stats)]
    L.scs_set_collectives.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scs_set_collectives_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scs_kernel_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.scs_set_kernel_timing.argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    L.scs_predict_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.scs_philox_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.scs_detlog_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.scs_download_amplicons.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    L.scs_download_read_numbers.argtypes = [C.c_void_p, C.c_void_p]
    L.scs_download_primer_stock.argtypes = [C.c_void_p, C.c_void_p]
    L.scs_profile_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.scs_profile_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_size_t)]
    L.scs_profile_scalars.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.scs_profile_close.argtypes = [C.c_void_p]
    L.scs_fasta_probe.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.scs_fasta_write_index.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.scs_simuvars.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    L.scs_simuvars_probe.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    _lib = L
    return L


def merge_fastq_shards(prefix, nranks, paired=True, keep_shards=False):
    """Host-only: rebuild the single-job FASTQ files from the per-rank shards + indexes that a sharded job wrote with
    GenReads.yield_reads_files (byte-range copies in list order; no record is parsed)."""
    L = load_library()
    err = C.create_string_buffer(512)
    rc = L.scs_merge_fastq_shards(os.fsencode(prefix), int(nranks), int(paired), int(keep_shards), err, 512)
    if rc:
        raise ScsError(rc, err.value.decode())


def merge_fastq_parts(prefix, paired=True, keep_parts=False):
    """Host-only: <prefix>.p*_1.fq ... (written by yield_reads_files(prefix, writers=K)) -> <prefix>_1.fq ... by byte-range
    copies; the parts and <prefix>.parts are removed unless keep_parts."""
    L = load_library()
    L.scs_merge_fastq_parts.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    err = C.create_string_buffer(512)
    rc = L.scs_merge_fastq_parts(os.fsencode(prefix), int(paired), int(keep_parts), err, 512)
    if rc:
        raise ScsError(rc, err.value.decode())


def part_paths(base, parts, paired=True, suffix=".fq"):
    """The files yield_reads_files(base, writers=parts) writes, per mate, in record order."""
    mates = ("_1", "_2") if paired else ("",)
    if parts <= 1:
        return [[base + m + suffix] for m in mates]
    return [[base + ".p%02d" % k + m + suffix for k in range(parts)] for m in mates]


def gpu_local_cpus(device=0):
    """CPUs of the NUMA node the GPU hangs on, within this process's affinity mask ([]: unknown or no choice)."""
    L = load_library()
    buf = (C.c_int * 4096)()
    n = L.scs_gpu_local_cpus(int(device), buf, 4096)
    return [buf[i] for i in range(min(n, 4096))]


def text_checksum(data):
    """The library's batch checksum (scs_set_batch_checksums) of a bytes-like object, in numpy: the text as little-endian 64-bit
    words w_i (the last zero-padded), sum_i fmix64(w_i + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64."""
    import numpy as np
    b = np.frombuffer(data, np.uint8)
    pad = (-len(b)) % 8
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    w = b.view("<u8").astype(np.uint64)
    with np.errstate(over="ignore"):
        x = w + (np.arange(1, len(w) + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        x ^= x >> np.uint64(33); x *= np.uint64(0xFF51AFD7ED558CCD); x ^= x >> np.uint64(33); x *= np.uint64(0xC4CEB9FE1A85EC53); x ^= x >> np.uint64(33)
        return int(np.add.reduce(x, dtype=np.uint64)) if len(x) else 0


def bgzf_probe(data, lds_out_cap=0):
    """Host-only: the BGZF blocks the device kernels would make of `data` (their arithmetic on the CPU; no end-of-file block)."""
    L = load_library()
    L.scs_bgzf_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    data = bytes(data)
    rc = L.scs_bgzf_probe(data, len(data), lds_out_cap, None, 0, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_bgzf_probe")
    out = C.create_string_buffer(max(1, n.value))
    rc = L.scs_bgzf_probe(data, len(data), lds_out_cap, out, n.value, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_bgzf_probe")
    return out.raw[:n.value]


def batch_plan_probe(pairs, read_length=150, to_sink=False, writers=1, regions=1, batch_shift=0):
    """Host-only: (pairs per batch, order, region_of) of the batches a yield of `pairs` pairs is cut into: order[i] is the batch made
    i-th, region_of[i] the sink region its records belong to."""
    L = load_library()
    L.scs_batch_plan_probe.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    batch, n = C.c_uint64(), C.c_uint32()
    args = (int(pairs), int(read_length), int(bool(to_sink)), int(writers), int(regions), int(batch_shift), C.byref(batch), C.byref(n))
    rc = L.scs_batch_plan_probe(*args, None, None, 0)
    if rc:
        raise ScsError(rc, "scs_batch_plan_probe")
    order, region_of = (C.c_uint32 * max(1, n.value))(), (C.c_uint32 * max(1, n.value))()
    rc = L.scs_batch_plan_probe(*args, order, region_of, n.value)
    if rc:
        raise ScsError(rc, "scs_batch_plan_probe")
    return batch.value, list(order[:n.value]), list(region_of[:n.value])


def bgzf_blocks(data):
    """Split BGZF bytes into (block bytes, ISIZE) after checking every block's frame: gzip magic, the BC subfield, BSIZE."""
    out, o = [], 0
    while o < len(data):
        h = data[o:o + 18]
        assert len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00", "not a BGZF block at %d" % o
        size = int.from_bytes(h[16:18], "little") + 1
        assert o + size <= len(data) and size <= 65536
        out.append((data[o:o + size], int.from_bytes(data[o + size - 4:o + size], "little")))
        o += size
    return out


COMM_ID_BYTES = 128


def comm_unique_id():
    """RCCL communicator id (ncclGetUniqueId) as bytes: rank 0 makes it, every rank passes it to GenReads.comm_init."""
    L = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = L.scs_comm_unique_id(buf)
    if rc:
        raise ScsError(rc, L.scs_last_error(None).decode())
    return buf.raw


def simuvars_probe(ref_fasta, snp_file=None, var_file=None):
    """Host-only: (records, total haplotype bases, FNV-1a of the FASTA text) that GenReads.simuvars would produce."""
    L = load_library()
    n, tot, h = C.c_int(), C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(512)
    enc = lambda p: os.fsencode(p) if p else None
    rc = L.scs_simuvars_probe(enc(ref_fasta), enc(snp_file), enc(var_file), C.byref(n), C.byref(tot), C.byref(h), err, 512)
    if rc:
        raise ScsError(rc, err.value.decode())
    return n.value, tot.value, h.value


def fasta_write_index(path):
    """Host-only: leave <path>.fai beside the FASTA if there is none, as loading the genome does (fastahack index)."""
    L = load_library()
    err = C.create_string_buffer(512)
    rc = L.scs_fasta_write_index(os.fsencode(path), err, 512)
    if rc:
        raise ScsError(rc, err.value.decode())


def devbuf_probe(first_bytes, second_bytes, device=0):
    """Test seam (needs a GPU): capacities of a library device buffer after reserve(first) and reserve(second), and
    whether the second reserve kept the buffer's address."""
    L = load_library()
    L.scs_devbuf_probe.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    caps, same = (C.c_uint64 * 2)(), C.c_int()
    rc = L.scs_devbuf_probe(device, first_bytes, second_bytes, caps, C.byref(same))
    if rc:
        raise ScsError(rc, (L.scs_last_error(None) or b"").decode())
    return caps[0], caps[1], bool(same.value)


def live_resources():
    """Test seam: (device-buffer bytes, streams, events, pinned bytes) the library's owning handles hold right now in this
    process, by their own count (scs_live_resources).  All zero once every GenReads is closed."""
    L = load_library()
    L.scs_live_resources.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = L.scs_live_resources(out)
    if rc:
        raise ScsError(rc, "scs_live_resources")
    return tuple(out)


def bgzf_device_probe(data, zbase=0, device=0):
    """Test seam (needs a GPU): the BGZF blocks the device kernels make of `data` (plan, scan, emit -- what a batch's mate goes
    through), written from byte `zbase` (0..3) of a guarded output buffer.  Returns (blocks, guards_ok)."""
    L = load_library()
    L.scs_bgzf_device_probe.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    data = bytes(data)
    cap = len(data) + 31 * ((len(data) + 64511) // 64512) + 64
    out, n, ok = C.create_string_buffer(cap), C.c_uint64(), C.c_int()
    rc = L.scs_bgzf_device_probe(device, data, len(data), zbase, out, cap, C.byref(n), C.byref(ok))
    if rc:
        raise ScsError(rc, "scs_bgzf_device_probe: " + (L.scs_last_error(None) or b"").decode())
    return out.raw[:n.value], bool(ok.value)


def scan_probe(a0, a1=None, device=0):
    """Test seam (needs a GPU): the library's exclusive scan of the uint32 array a0 (n + 1 entries come back), or of the pair
    (a0, a1) in one call when a1 is given.  Returns out0, or (out0, out1)."""
    import numpy as np
    L = load_library()
    L.scs_scan_probe.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    a0 = np.ascontiguousarray(a0, np.uint32)
    o0 = np.empty(a0.size + 1, np.uint32)
    if a1 is None:
        rc = L.scs_scan_probe(device, a0.ctypes.data, a0.size, None, 0, o0.ctypes.data, None)
    else:
        a1 = np.ascontiguousarray(a1, np.uint32)
        o1 = np.empty(a1.size + 1, np.uint32)
        p1 = a1 if a1.size else np.zeros(1, np.uint32)                # an empty second array is still a second array: a valid pointer
        rc = L.scs_scan_probe(device, a0.ctypes.data, a0.size, p1.ctypes.data, a1.size, o0.ctypes.data, o1.ctypes.data)
    if rc:
        raise ScsError(rc, "scs_scan_probe: " + (L.scs_last_error(None) or b"").decode())
    return o0 if a1 is None else (o0, o1)


ALLOC_SLOTS = 40
ALLOC_CHUNK = 1000


def alloc_plan_probe(counts, rank):
    """Host-only: the read allocation's plan of shard `rank` over counts[R][40] amplicons per (shard, slot), as do_allocate builds it:
    dict of total, nch, n_interior, n_boundary, n_ranges, n_gseg, ac, scratch and the arrays ranges [n, 3] (q0, c0, local0),
    bchunks [n, 3] (chunk, length, owner), gsegs [n, 5] (go, lo, n, owner, slot), my_seg [40, 4] (go, lo, n, order)."""
    import numpy as np
    L = load_library()
    L.scs_alloc_plan_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    counts = np.ascontiguousarray(counts, np.uint64)
    assert counts.ndim == 2 and counts.shape[1] == ALLOC_SLOTS
    sc = (C.c_uint64 * 8)()
    rc = L.scs_alloc_plan_probe(counts.ctypes.data, counts.shape[0], int(rank), sc, None, None, None, None)
    if rc:
        raise ScsError(rc, "scs_alloc_plan_probe")
    out = dict(zip(("total", "nch", "n_interior", "n_boundary", "n_ranges", "n_gseg", "ac", "scratch"), (int(v) for v in sc)))
    rng, bch = np.zeros((out["n_ranges"], 3), np.uint32), np.zeros((out["n_boundary"], 3), np.uint32)
    gseg, mine = np.zeros((out["n_gseg"], 5), np.uint64), np.zeros((ALLOC_SLOTS, 4), np.uint64)
    rc = L.scs_alloc_plan_probe(counts.ctypes.data, counts.shape[0], int(rank), sc, rng.ctypes.data, bch.ctypes.data, gseg.ctypes.data, mine.ctypes.data)
    if rc:
        raise ScsError(rc, "scs_alloc_plan_probe")
    out.update(ranges=rng, bchunks=bch, gsegs=gseg, my_seg=mine)
    return out


def alloc_sums_probe(values, which, device=0):
    """Test seam (needs a GPU): the allocation's fixed-shape sum (which = 0: a float) or inclusive scan (which = 1: an array) of the
    float64 array `values`, with the scratch a job reserves for that many chunk partials."""
    import numpy as np
    L = load_library()
    L.scs_alloc_sums_probe.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    v = np.ascontiguousarray(values, np.float64)
    out = np.empty(v.size if which else 1, np.float64)
    rc = L.scs_alloc_sums_probe(device, v.ctypes.data, v.size, int(which), out.ctypes.data)
    if rc:
        raise ScsError(rc, "scs_alloc_sums_probe: " + (L.scs_last_error(None) or b"").decode())
    return out if which else float(out[0])


def _truth_probe(fn, seq, qual, genome, pos0, n, events, reverse, genome_start, rname, amp, cnt, paired, is_read2, mate):
    L = load_library()
    f = getattr(L, fn)
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int,
                  C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int64, C.c_uint64,
                  C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    enc = lambda x: x.encode() if isinstance(x, str) else bytes(x)
    seq, qual, genome = enc(seq), enc(qual), enc(genome)
    ev = lambda es: (C.c_int32 * max(1, 3 * len(es)))(*[int(v) for e in es for v in e])
    m_pos, m_rev, m_ev = mate if mate is not None else (0, False, ())
    args = [int(paired), int(is_read2), amp, cnt, enc(rname), n, pos0, int(reverse), ev(events), len(events),
            m_pos, int(m_rev), ev(m_ev), len(m_ev), seq, qual, len(seq), genome, genome_start, len(genome)]
    size = C.c_size_t()
    rc = f(*args, None, 0, C.byref(size))
    if rc:
        raise ScsError(rc, fn + ": not a valid alignment")
    out = C.create_string_buffer(size.value)
    rc = f(*args, out, size.value, C.byref(size))
    if rc:
        raise ScsError(rc, fn)
    return out.raw[:size.value]


def truth_bam_record_probe(seq, qual, genome, pos0, n, events=(), reverse=False, genome_start=0, rname="chr", amp=0, cnt=1,
                           paired=False, is_read2=False, mate=None):
    """Host-only: one read's truth BAM record (bytes, block_size included, uncompressed) through the formatter the truth kernels
    run; refID = 0, next_refID = 0 (paired) or -1.  The arguments are truth_record_probe's."""
    return _truth_probe("scs_truth_bam_record_probe", seq, qual, genome, pos0, n, events, reverse, genome_start, rname, amp, cnt, paired, is_read2, mate)


def truth_record_probe(seq, qual, genome, pos0, n, events=(), reverse=False, genome_start=0, rname="chr", amp=0, cnt=1,
                       paired=False, is_read2=False, mate=None):
    """Host-only: one read's truth SAM line (with its newline) through the formatter the truth kernels run.  n = window length;
    pos0 = 0-based record coordinate of window base 0 (the rightmost base when reverse); events = [(window position, deletion?,
    length), ...] in read orientation; seq / qual = the FASTQ record's; genome = the record's bases from genome_start on;
    mate = (pos0, reverse, events) of the other read of a pair (paired=True)."""
    return _truth_probe("scs_truth_record_probe", seq, qual, genome, pos0, n, events, reverse, genome_start, rname, amp, cnt, paired, is_read2, mate).decode()


def depth_layout_probe(rec_lens, bin_width):
    """Host-only: (bin_off, n_bins) of the depth track's bins for records of these lengths, through the layout function the
    library runs: bin_off[r] = first bin of record r (len(rec_lens) + 1 entries, uint64).  More than 2^27 bins: ScsError
    (SCS_EINVAL) naming the smallest admissible width."""
    import numpy as np
    L = load_library()
    L.scs_depth_layout_probe.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    lens = np.ascontiguousarray(rec_lens, np.uint64)
    off, n = np.zeros(lens.size + 1, np.uint64), C.c_uint64()
    rc = L.scs_depth_layout_probe(lens.ctypes.data, lens.size, int(bin_width), off.ctypes.data, C.byref(n))
    if rc:
        raise ScsError(rc, (L.scs_last_error(None) or b"").decode())
    return off, n.value


def depth_read_probe(pos0, n, events=(), reverse=False, rec_len=1 << 40, bin_width=1000):
    """Host-only: what one read adds to the depth track, through the function the depth kernel runs.  pos0, n, events, reverse
    as for truth_record_probe; rec_len = bases of its record.  Returns (bin of the `reads` increment, [(bin, bases), ...] in
    ascending bin order), bins counted inside the record."""
    L = load_library()
    L.scs_depth_read_probe.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32,
                                       C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    ev = (C.c_int32 * max(1, 3 * len(events)))(*[int(v) for e in events for v in e])
    first, k = C.c_uint64(), C.c_int()
    args = (int(n), int(pos0), int(bool(reverse)), ev, len(events), int(rec_len), int(bin_width), C.byref(first))
    rc = L.scs_depth_read_probe(*args, None, None, 0, C.byref(k))
    if rc not in (SCS_OK, SCS_EOVERFLOW):
        raise ScsError(rc, "scs_depth_read_probe: not a valid alignment inside the record")
    bins, bases = (C.c_uint64 * max(1, k.value))(), (C.c_uint32 * max(1, k.value))()
    rc = L.scs_depth_read_probe(*args, bins, bases, k.value, C.byref(k))
    if rc:
        raise ScsError(rc, "scs_depth_read_probe")
    return first.value, [(bins[i], bases[i]) for i in range(k.value)]


def coverage_read_probe(pos0, n, events=(), reverse=False, rec_len=1 << 40):
    """Host-only: the intervals [(start, end), ...] of record coordinates one read marks in the coverage profile, ascending, through
    the function the per-batch kernel runs.  Arguments as for depth_read_probe."""
    L = load_library()
    L.scs_coverage_read_probe.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    ev = (C.c_int32 * max(1, 3 * len(events)))(*[int(v) for e in events for v in e])
    k = C.c_int()
    args = (int(n), int(pos0), int(bool(reverse)), ev, len(events), int(rec_len))
    rc = L.scs_coverage_read_probe(*args, None, None, 0, C.byref(k))
    if rc not in (SCS_OK, SCS_EOVERFLOW):
        raise ScsError(rc, "scs_coverage_read_probe: not a valid alignment inside the record")
    a, b = (C.c_uint64 * max(1, k.value))(), (C.c_uint64 * max(1, k.value))()
    rc = L.scs_coverage_read_probe(*args, a, b, k.value, C.byref(k))
    if rc:
        raise ScsError(rc, "scs_coverage_read_probe")
    return [(a[i], b[i]) for i in range(k.value)]


def coverage_stats_probe(hist, total):
    """Host-only: dict(mean=, breadth=(at 1, 5, 10, 20), gini=) of one histogram row (max_depth + 1 buckets, the last one depth >=
    max_depth) whose depths add up to `total`, through the function write_coverage runs."""
    import numpy as np
    L = load_library()
    L.scs_coverage_stats_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    h = np.ascontiguousarray(hist, np.uint64)
    out = np.zeros(6, np.float64)
    rc = L.scs_coverage_stats_probe(h.ctypes.data, h.size - 1, int(total), out.ctypes.data)
    if rc:
        raise ScsError(rc, "scs_coverage_stats_probe: a row has 2 .. 65536 buckets")
    return dict(mean=float(out[0]), breadth=tuple(float(v) for v in out[1:5]), gini=float(out[5]))


def coverage_tile():
    """(tile, chunk): entries of the difference array per workgroup of the coverage profile's end-of-job pass, and tile sums per
    step of its tile-offset scan."""
    L = load_library()
    L.scs_coverage_tile.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.scs_coverage_tile.restype = None
    t, c = C.c_uint32(), C.c_uint32()
    L.scs_coverage_tile(C.byref(t), C.byref(c))
    return t.value, c.value


def coverage_finish_probe(ctx, diff, codes, rec_lens, max_depth, lds_buckets=-1):
    """Needs the GPU: the end-of-job kernels of the coverage profile alone, on the GenReads `ctx`.  diff: int32[G + 1], codes:
    uint8[G] (0 .. 3, 4 = N), rec_lens adding up to G; lds_buckets: buckets of a workgroup's LDS histogram (-1: the product's).
    Returns dict(depth=uint32[G], hist=uint64[records][max_depth + 1], n_bases=, sum=, sum_n=); inconsistent differences raise
    ScsError (SCS_EOVERFLOW) and leave the ctx usable."""
    import numpy as np
    d, cd, ln = np.ascontiguousarray(diff, np.int32), np.ascontiguousarray(codes, np.uint8), np.ascontiguousarray(rec_lens, np.uint64)
    G, nr, D = cd.size, ln.size, int(max_depth)
    if d.size != G + 1:
        raise ValueError("diff has G + 1 entries")
    out = dict(depth=np.zeros(G, np.uint32), hist=np.zeros((nr, D + 1), np.uint64), n_bases=np.zeros(nr, np.uint64), sum=np.zeros(nr, np.uint64), sum_n=np.zeros(nr, np.uint64))
    fn = ctx._L.scs_coverage_finish_probe
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 5
    ctx._ck(fn(ctx._ctx, d.ctypes.data, cd.ctypes.data, G, ln.ctypes.data, nr, D, int(lds_buckets), *[out[k].ctypes.data for k in ("depth", "hist", "n_bases", "sum", "sum_n")]))
    return out


def gc_bias_probe(ctx, depth, codes, rec_lens, window, lds_buckets=-1):
    """Needs the GPU: the GC-bias kernel alone, as the product launches it, on the GenReads `ctx`.  depth: uint32[G], codes: uint8[G]
    (0 .. 3 = ACGT, >= 4 = N), rec_lens adding up to G, window 1 .. 1024; lds_buckets: -1 the product's choice, 0 no LDS table (every
    add goes to memory).  Returns dict(windows=uint64[records][101], depth_sum=uint64[records][101], n_windows=uint64[records])."""
    import numpy as np
    d, cd, ln = np.ascontiguousarray(depth, np.uint32), np.ascontiguousarray(codes, np.uint8), np.ascontiguousarray(rec_lens, np.uint64)
    G, nr = cd.size, ln.size
    if d.size != G:
        raise ValueError("depth and codes have G entries each")
    out = dict(windows=np.zeros((nr, 101), np.uint64), depth_sum=np.zeros((nr, 101), np.uint64), n_windows=np.zeros(nr, np.uint64))
    fn = ctx._L.scs_gc_bias_probe
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 3
    ctx._ck(fn(ctx._ctx, d.ctypes.data, cd.ctypes.data, G, ln.ctypes.data, nr, int(window), int(lds_buckets), *[out[k].ctypes.data for k in ("windows", "depth_sum", "n_windows")]))
    return out


def coverage_ref_finish_probe(ctx, depth, codes, segs, hap_lens, ref_lens, max_depth, lds_buckets=-1):
    """Needs the GPU: the kernels of the coverage profile on the reference alone, as the product launches them, on the GenReads
    `ctx`.  depth: uint32[G] staged depths, codes: uint8[G] (0 .. 3, 4 = N), segs: (hap_off, len, ref_pos, ref_rec, kind) arrays in
    lift_segments' layout that tile staged records of hap_lens (adding up to G), ref_lens: the reference records; lds_buckets: buckets
    of the count kernel's LDS histogram (-1: the product's).  Returns dict(ref_depth=uint32[R], packed=uint32[R] (copies |
    n_copies << 16), hist=uint64[ref records][max_depth + 1], n_bases=, absent=, sum=, sum_n=, cn_bases=, cn_sum= [ref records][17],
    unlifted=int).  A segment that lifts outside its reference record raises ScsError (SCS_EOVERFLOW) and leaves the ctx usable."""
    import numpy as np
    d, cd = np.ascontiguousarray(depth, np.uint32), np.ascontiguousarray(codes, np.uint8)
    ho, ln, rp = (np.ascontiguousarray(v, np.uint64) for v in segs[:3])
    rr, kd = (np.ascontiguousarray(v, np.uint32) for v in segs[3:5])
    hl, rl = np.ascontiguousarray(hap_lens, np.uint64), np.ascontiguousarray(ref_lens, np.uint64)
    G, nf, D, R = cd.size, rl.size, int(max_depth), int(rl.sum())
    if d.size != G or not (ho.size == ln.size == rp.size == rr.size == kd.size):
        raise ValueError("depth and codes have G entries, the segment arrays one length")
    out = dict(ref_depth=np.zeros(R, np.uint32), packed=np.zeros(R, np.uint32), hist=np.zeros((nf, D + 1), np.uint64), n_bases=np.zeros(nf, np.uint64), absent=np.zeros(nf, np.uint64),
               sum=np.zeros(nf, np.uint64), sum_n=np.zeros(nf, np.uint64), cn_bases=np.zeros((nf, 17), np.uint64), cn_sum=np.zeros((nf, 17), np.uint64))
    unl = C.c_uint64()
    fn = ctx._L.scs_coverage_ref_finish_probe
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 9 + [C.POINTER(C.c_uint64)]
    ctx._ck(fn(ctx._ctx, d.ctypes.data, cd.ctypes.data, G, ho.ctypes.data, ln.ctypes.data, rp.ctypes.data, rr.ctypes.data, kd.ctypes.data, ho.size, hl.ctypes.data, hl.size, rl.ctypes.data, nf, D, int(lds_buckets),
               *[out[k].ctypes.data for k in ("ref_depth", "packed", "hist", "n_bases", "absent", "sum", "sum_n", "cn_bases", "cn_sum")], C.byref(unl)))
    out["unlifted"] = unl.value
    return out


def runs_line_probe(name, start, end, value, cap=None):
    """Host-only: one bedGraph line `name\\tstart\\tend\\tvalue\\n` as bytes, through the formatter the bedGraph writer's sizing and
    emit kernels run.  cap: room in bytes (None: enough); too little raises ScsError (SCS_EOVERFLOW) whose `needed` is the line's size."""
    L = load_library()
    L.scs_runs_line_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    nm = name if isinstance(name, bytes) else name.encode()
    room = len(nm) + 64 if cap is None else int(cap)
    buf, n = C.create_string_buffer(max(1, room)), C.c_uint64()
    rc = L.scs_runs_line_probe(nm, int(start), int(end), int(value), buf, room, C.byref(n))
    if rc:
        e = ScsError(rc, "scs_runs_line_probe: the line has %d bytes, room for %d" % (n.value, room))
        e.needed = n.value
        raise e
    return buf.raw[:n.value]


def runs_probe(ctx, values, mask, rec_lens, names, text_cap=0, bgzf=False):
    """Needs the GPU: the bedGraph writer's kernels and slab loop, as the product runs them, over values (uint32[n]) compared and
    printed under `mask`, records of rec_lens (adding up to n) named `names`, on the GenReads `ctx`.  text_cap: bytes of text a slab
    may hold (0: the product's); bgzf: BGZF blocks with the end-of-file block.  Returns dict(data=bytes a file would hold, lines=,
    slabs=).  A cap below one tile's text raises ScsError (SCS_EINVAL) and leaves the ctx usable."""
    import numpy as np
    v, ln = np.ascontiguousarray(values, np.uint32), np.ascontiguousarray(rec_lens, np.uint64)
    nm = [s if isinstance(s, bytes) else s.encode() for s in names]
    if len(nm) != ln.size:
        raise ValueError("one name per record")
    arr = (C.c_char_p * max(1, len(nm)))(*nm)
    fn = ctx._L.scs_runs_probe
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64] + [C.POINTER(C.c_uint64)] * 3
    n_out, lines, slabs = C.c_uint64(), C.c_uint64(), C.c_uint64()
    args = (ctx._ctx, v.ctypes.data, v.size, int(mask), ln.ctypes.data, ln.size, arr, int(text_cap), int(bool(bgzf)))
    rc = fn(*args, None, 0, C.byref(n_out), C.byref(lines), C.byref(slabs))            # sizes first, then the bytes
    if rc != SCS_EOVERFLOW or not n_out.value:
        ctx._ck(rc)
        return dict(data=b"", lines=lines.value, slabs=slabs.value)
    buf = np.zeros(n_out.value, np.uint8)
    ctx._ck(fn(*args, buf.ctypes.data, buf.size, C.byref(n_out), C.byref(lines), C.byref(slabs)))
    return dict(data=buf[:n_out.value].tobytes(), lines=lines.value, slabs=slabs.value)


class LiftTable:
    """A lift table as numpy arrays: per segment hap_off (global staged index), len, ref_pos, ref_rec, kind (0: R, 1: I); the
    reference records' and the staged records' names and lengths."""

    def __init__(self, hap_off, length, ref_pos, ref_rec, kind, ref_names=None, ref_lens=None, hap_names=None, hap_lens=None):
        self.hap_off, self.len, self.ref_pos, self.ref_rec, self.kind = hap_off, length, ref_pos, ref_rec, kind
        self.ref_names, self.ref_lens, self.hap_names, self.hap_lens = ref_names, ref_lens, hap_names, hap_lens

    def __len__(self):
        return len(self.hap_off)

    def same_segments(self, other):
        return all((getattr(self, k) == getattr(other, k)).all() if len(self) == len(other) else False for k in ("hap_off", "len", "ref_pos", "ref_rec", "kind"))


def _lift_probe(call):
    """The two-call pattern of scs_lift_plan_probe / scs_lift_file_probe: sizes first, then the arrays."""
    import numpy as np
    n_seg, n_hap, n_ref, n_names = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    call(None, None, None, None, None, 0, n_seg, None, None, 0, n_hap, n_ref, None, 0, n_names)
    ns, nr = n_seg.value, max(n_hap.value, n_ref.value)
    a = [np.zeros(max(ns, 1), np.uint64) for _ in range(3)] + [np.zeros(max(ns, 1), np.uint32) for _ in range(2)]
    hap_lens, ref_lens = np.zeros(max(nr, 1), np.uint64), np.zeros(max(nr, 1), np.uint64)
    names = C.create_string_buffer(max(1, n_names.value))
    call(*[x.ctypes.data for x in a], ns, n_seg, hap_lens.ctypes.data, ref_lens.ctypes.data, nr, n_hap, n_ref, names, n_names.value, n_names)
    nm = names.raw[:n_names.value].decode().split("\n")[:-1]
    return LiftTable(*[x[:ns] for x in a], ref_names=nm[:n_ref.value], ref_lens=ref_lens[:n_ref.value], hap_names=nm[n_ref.value:], hap_lens=hap_lens[:n_hap.value])


def lift_plan_probe(ref_fasta, snp_file=None, var_file=None, out_path=None):
    """Host-only: (LiftTable, substituted global staged indices) of the genome GenReads.simuvars would build for these inputs,
    through the planner and the table builder it runs; out_path: also write the lift file."""
    import numpy as np
    L = load_library()
    L.scs_lift_plan_probe.argtypes = [C.c_char_p] * 4 + [C.c_void_p] * 5 + [C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                      C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    enc = lambda p: os.fsencode(p) if p else None
    err, n_sub = C.create_string_buffer(512), C.c_uint64()
    state = dict(sub=None)

    def call(h, l, rp, rr, k, cap, n_seg, hl, rl, rcap, n_hap, n_ref, names, ncap, nlen):
        sub = state["sub"]
        rc = L.scs_lift_plan_probe(enc(ref_fasta), enc(snp_file), enc(var_file), enc(out_path) if sub is not None else None, h, l, rp, rr, k, cap, C.byref(n_seg),
                                   sub.ctypes.data if sub is not None else None, len(sub) if sub is not None else 0, C.byref(n_sub),
                                   hl, rl, rcap, C.byref(n_hap), C.byref(n_ref), names, ncap, C.byref(nlen), err, 512)
        if rc:
            raise ScsError(rc, err.value.decode() or "scs_lift_plan_probe")
        if sub is None:
            state["sub"] = np.zeros(max(1, n_sub.value), np.uint64)
    t = _lift_probe(call)
    return t, state["sub"][:n_sub.value]


def lift_file_probe(path):
    """Host-only: the LiftTable a lift file holds, through the parser scs_load_lift runs.  A refused file raises ScsError (SCS_EIO)
    whose .line is the line it was refused at."""
    L = load_library()
    L.scs_lift_file_probe.argtypes = [C.c_char_p] + [C.c_void_p] * 5 + [C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    err, line = C.create_string_buffer(1024), C.c_uint64()

    def call(h, l, rp, rr, k, cap, n_seg, hl, rl, rcap, n_hap, n_ref, names, ncap, nlen):
        rc = L.scs_lift_file_probe(os.fsencode(path), h, l, rp, rr, k, cap, C.byref(n_seg), hl, rl, rcap, C.byref(n_hap), C.byref(n_ref), names, ncap, C.byref(nlen), C.byref(line), err, 1024)
        if rc:
            e = ScsError(rc, err.value.decode() or "scs_lift_file_probe")
            e.line = line.value
            raise e
    return _lift_probe(call)


def lift_read_probe(table, hap_lens, ref_lens, pos0, n, events=(), reverse=False, bin_width=1000):
    """Host-only: what one read adds to the reference's bins through a lift table, through the function k_depth_lift runs.  table:
    a LiftTable (or any object with its five arrays); pos0 = global staged index of window base 0.  Returns (bin of the `reads`
    increment, [(bin, bases), ...] in the order made); the pseudo-bin is the number of bins.  A read that cannot be lifted raises
    ScsError (SCS_EINVAL) whose .lift_err says why (0: not a valid alignment)."""
    import numpy as np
    L = load_library()
    L.scs_lift_read_probe.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    ev = np.ascontiguousarray([v for e in events for v in e], np.int32)
    segs = [np.ascontiguousarray(getattr(table, k), dt) for k, dt in (("hap_off", np.uint64), ("len", np.uint64), ("ref_pos", np.uint64), ("ref_rec", np.uint32), ("kind", np.uint32))]
    hl, rl = np.ascontiguousarray(hap_lens, np.uint64), np.ascontiguousarray(ref_lens, np.uint64)
    first, k, le = C.c_uint64(), C.c_int(), C.c_int()
    args = (int(n), int(pos0), int(bool(reverse)), ev.ctypes.data if len(events) else None, len(events)) + tuple(x.ctypes.data for x in segs) + \
           (len(segs[0]), hl.ctypes.data, len(hl), rl.ctypes.data, len(rl), int(bin_width), C.byref(first))
    rc = L.scs_lift_read_probe(*args, None, None, 0, C.byref(k), C.byref(le))
    if rc not in (SCS_OK, SCS_EOVERFLOW):
        e = ScsError(rc, "scs_lift_read_probe: " + ("the read cannot be lifted (%d)" % le.value if le.value else "not a valid alignment"))
        e.lift_err = le.value
        raise e
    bins, bases = np.zeros(max(1, k.value), np.uint64), np.zeros(max(1, k.value), np.uint32)
    rc = L.scs_lift_read_probe(*args, bins.ctypes.data, bases.ctypes.data, k.value, C.byref(k), C.byref(le))
    if rc:
        raise ScsError(rc, "scs_lift_read_probe")
    return first.value, [(int(bins[i]), int(bases[i])) for i in range(k.value)]


def truth_ref_record_probe(table, hap_lens, ref_lens, ref_names, seq, qual, pos0, n, events=(), reverse=False, hap_names=None, rname=None,
                           amp=0, cnt=1, paired=False, is_read2=False, mate=None):
    """Host-only: one read's line (with its newline) of the truth SAM on the original reference, through the formatter its kernels
    run.  table: a LiftTable (or any object with its five arrays); hap_lens / ref_lens / ref_names: the staged and the reference
    records; pos0 = GLOBAL staged index of window base 0; n, events, reverse, seq, qual, mate as for truth_record_probe (the
    mate's pos0 global too).  rname = the staged record's name for YH (None: from hap_names).  A read that cannot be lifted
    raises ScsError (SCS_EINVAL) whose .lift_err says why (0: not a valid alignment)."""
    import numpy as np
    L = load_library()
    f = L.scs_truth_ref_record_probe
    f.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int,
                  C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int] + [C.c_void_p] * 5 + \
                 [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    enc = lambda x: x.encode() if isinstance(x, str) else bytes(x)
    seq, qual = enc(seq), enc(qual)
    ev = lambda es: (C.c_int32 * max(1, 3 * len(es)))(*[int(v) for e in es for v in e])
    m_pos, m_rev, m_ev = mate if mate is not None else (0, False, ())
    segs = [np.ascontiguousarray(getattr(table, k), dt) for k, dt in (("hap_off", np.uint64), ("len", np.uint64), ("ref_pos", np.uint64), ("ref_rec", np.uint32), ("kind", np.uint32))]
    hl, rl = np.ascontiguousarray(hap_lens, np.uint64), np.ascontiguousarray(ref_lens, np.uint64)
    names = "".join(x + "\n" for x in list(ref_names) + list(hap_names or ())).encode()
    args = [int(paired), int(is_read2), amp, cnt, enc(rname) if rname is not None else None, int(n), int(pos0), int(bool(reverse)), ev(events), len(events),
            int(m_pos), int(bool(m_rev)), ev(m_ev), len(m_ev), seq, qual, len(seq)] + [x.ctypes.data for x in segs] + \
           [len(segs[0]), hl.ctypes.data, len(hl), rl.ctypes.data, len(rl), names, len(names)]
    size, le = C.c_size_t(), C.c_int()
    rc = f(*args, None, 0, C.byref(size), C.byref(le))
    if rc:
        e = ScsError(rc, "scs_truth_ref_record_probe: " + ("the read cannot be lifted (%d)" % le.value if le.value else "not a valid alignment"))
        e.lift_err = le.value
        raise e
    out = C.create_string_buffer(size.value)
    rc = f(*args, out, size.value, C.byref(size), C.byref(le))
    if rc:
        raise ScsError(rc, "scs_truth_ref_record_probe")
    return out.raw[:size.value].decode()


def support_read_probe(pos0, n, seq, positions, events=(), reverse=False, rec_len=1 << 40):
    """Host-only: what one read shows at the listed record coordinates, through the function the site support kernel runs.  pos0, n,
    events, reverse, rec_len as for depth_read_probe; seq = the FASTQ record's bases; positions ascending and distinct.  Returns
    [(position index, class), ...] in ascending order: class 0..3 = A, C, G, T (genome-forward), 4 = other, 5 = deleted."""
    import numpy as np
    L = load_library()
    L.scs_support_read_probe.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_char_p, C.c_int,
                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    ev = (C.c_int32 * max(1, 3 * len(events)))(*[int(v) for e in events for v in e])
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    pos = np.ascontiguousarray(list(positions), np.uint64)             # (exactly its size: the sanitizer tool's twin reads no further)
    k = C.c_int()
    args = (int(n), int(pos0), int(bool(reverse)), ev, len(events), int(rec_len), seq, len(seq), pos.ctypes.data if pos.size else None, pos.size)
    rc = L.scs_support_read_probe(*args, None, None, 0, C.byref(k))
    if rc not in (SCS_OK, SCS_EOVERFLOW):
        raise ScsError(rc, "scs_support_read_probe: not a valid alignment inside the record, or positions out of order")
    idx, cls = np.zeros(max(1, k.value), np.uint64), np.zeros(max(1, k.value), np.uint8)
    rc = L.scs_support_read_probe(*args, idx.ctypes.data, cls.ctypes.data, k.value, C.byref(k))
    if rc:
        raise ScsError(rc, "scs_support_read_probe")
    return [(int(idx[i]), int(cls[i])) for i in range(k.value)]


def site_support_line_probe(name, pos, ref, alt, na, ta, nr, tr, counts=None):
    """Host-only: one site's line through the formatter the emit kernel runs; counts = its six counters (A, C, G, T, other, deleted),
    or None for the artefact table's line.  pos 0-based, ref a code 0..4, alt 0..3."""
    L = load_library()
    L.scs_site_support_line_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p,
                                              C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    cn = (C.c_uint32 * 6)(*[int(v) for v in counts]) if counts is not None else None
    args = [name.encode(), int(pos), int(ref), int(alt), int(na), int(ta), int(nr), int(tr), cn]
    n = C.c_size_t()
    rc = L.scs_site_support_line_probe(*args, None, 0, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_site_support_line_probe")
    out = C.create_string_buffer(max(1, n.value))
    rc = L.scs_site_support_line_probe(*args, out, n.value, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_site_support_line_probe")
    return out.raw[:n.value].decode()


def amplicon_line_probe(frag, semi, full, genome, genome_start=0, rec_off=0, rec_len=None, rec_name="chr", index=0, reads=0, semi_index=0):
    """Host-only: one line of the amplicon table through the functions its kernels run.  frag = (genome offset, length, strand);
    semi / full = (spos, length, [(pos, alt), ...]) with alt a base code 0..3; genome = the bases from genome index genome_start on;
    rec_off / rec_len = the record's first genome index and length.  ScsError (SCS_EINVAL): a lineage that does not fit."""
    import numpy as np
    L = load_library()
    L.scs_amplicon_line_probe.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    genome = genome.encode() if isinstance(genome, str) else bytes(genome)
    e1 = np.array([(p << 3) | a for p, a in semi[2]] or [0], np.uint32)
    e2 = np.array([(p << 3) | a for p, a in full[2]] or [0], np.uint32)
    args = [int(frag[0]), int(frag[1]), int(frag[2]), int(semi[0]), int(semi[1]), e1.ctypes.data, len(semi[2]), int(full[0]), int(full[1]), e2.ctypes.data, len(full[2]),
            genome, int(genome_start), len(genome), int(rec_off), int(len(genome) if rec_len is None else rec_len), rec_name.encode(), int(index), int(reads), int(semi_index)]
    n = C.c_size_t()
    rc = L.scs_amplicon_line_probe(*args, None, 0, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_amplicon_line_probe: the lineage does not fit its parents, its record or the genome given")
    out = C.create_string_buffer(max(1, n.value))
    rc = L.scs_amplicon_line_probe(*args, out, n.value, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_amplicon_line_probe")
    return out.raw[:n.value].decode()


def artefact_probe(starts, lens, reads, edits, rec_lens, rec_names, genome, min_reads=0, header=False):
    """Host-only: the artefact table's body (header=True: behind its header) through the functions its kernels run.  starts / lens /
    reads: the full amplicons' global genome start, length and read number; edits = [(amplicon, global genome index, alt code 0..3),
    ...]; rec_lens / rec_names: the staged records; genome = their bases, concatenated.  ScsError (SCS_EINVAL): an amplicon outside
    its record, an edit outside its amplicon."""
    import numpy as np
    L = load_library()
    L.scs_artefact_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint32, C.c_int,
                                     C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    genome = genome.encode() if isinstance(genome, str) else bytes(genome)
    n_amp, n_ed = len(starts), len(edits)
    a_s, a_l, a_r = (np.ascontiguousarray(list(starts) + [0], np.uint64), np.ascontiguousarray(list(lens) + [0], np.uint32), np.ascontiguousarray(list(reads) + [0], np.uint32))
    e_a = np.ascontiguousarray([e[0] for e in edits] + [0], np.uint32)
    e_x = np.ascontiguousarray([e[1] for e in edits] + [0], np.uint64)
    e_b = np.ascontiguousarray([e[2] for e in edits] + [0], np.uint8)
    r_l = np.ascontiguousarray(list(rec_lens), np.uint64)
    names = (C.c_char_p * len(rec_names))(*[n.encode() for n in rec_names])
    args = [a_s.ctypes.data, a_l.ctypes.data, a_r.ctypes.data, n_amp, e_a.ctypes.data, e_x.ctypes.data, e_b.ctypes.data, n_ed,
            r_l.ctypes.data, names, len(rec_names), genome, len(genome), int(min_reads), 1 if header else 0]
    n = C.c_size_t()
    rc = L.scs_artefact_probe(*args, None, 0, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_artefact_probe: an amplicon outside its record, an edit outside its amplicon, or a base that is no code 0..3")
    out = C.create_string_buffer(max(1, n.value))
    rc = L.scs_artefact_probe(*args, out, n.value, C.byref(n))
    if rc:
        raise ScsError(rc, "scs_artefact_probe")
    return out.raw[:n.value].decode()


def artefact_ref_probe(starts, lens, reads, edits, hap_lens, genome, table, ref_lens, ref_names, min_reads=0, slab=0, header=False):
    """Host-only: the body of the artefact table on the original reference (header=True: behind its header) through the functions its
    kernels run, slab by slab.  starts / lens / reads: the full amplicons' global staged start, length and read number; edits =
    [(amplicon, global staged index, alt code 0..3), ...] in any order; hap_lens: the staged records; genome = their bases,
    concatenated; table: a LiftTable (or any object with its five arrays); ref_lens / ref_names: the reference records; slab:
    reference indices per slab (0: 2^28).  Returns (text, (unlifted entries, unlifted reads)).  A refused input raises ScsError
    (SCS_EINVAL) whose .lift_err says why a walk gave up (0: it was not a walk)."""
    import numpy as np
    L = load_library()
    L.scs_artefact_ref_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64] + [C.c_void_p] * 5 + [C.c_uint32,
                                         C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                         C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int)]
    genome = genome.encode() if isinstance(genome, str) else bytes(genome)
    n_amp, n_ed = len(starts), len(edits)
    a_s, a_l, a_r = (np.ascontiguousarray(list(starts) + [0], np.uint64), np.ascontiguousarray(list(lens) + [0], np.uint32), np.ascontiguousarray(list(reads) + [0], np.uint32))
    e_a = np.ascontiguousarray([e[0] for e in edits] + [0], np.uint32)
    e_x = np.ascontiguousarray([e[1] for e in edits] + [0], np.uint64)
    e_b = np.ascontiguousarray([e[2] for e in edits] + [0], np.uint8)
    h_l = np.ascontiguousarray(list(hap_lens), np.uint64)
    r_l = np.ascontiguousarray(list(ref_lens), np.uint64)
    seg = [np.ascontiguousarray(getattr(table, k), t) for k, t in (("hap_off", np.uint64), ("len", np.uint64), ("ref_pos", np.uint64), ("ref_rec", np.uint32), ("kind", np.uint32))]
    names = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    unl = np.zeros(2, np.uint64)
    args = [a_s.ctypes.data, a_l.ctypes.data, a_r.ctypes.data, n_amp, e_a.ctypes.data, e_x.ctypes.data, e_b.ctypes.data, n_ed,
            h_l.ctypes.data, len(h_l), genome, len(genome)] + [x.ctypes.data for x in seg] + [len(seg[0]),
            r_l.ctypes.data, names, len(ref_names), int(min_reads), int(slab), 1 if header else 0]
    n, le = C.c_size_t(), C.c_int()
    rc = L.scs_artefact_ref_probe(*args, None, 0, C.byref(n), unl.ctypes.data, C.byref(le))
    if rc:
        e = ScsError(rc, "scs_artefact_ref_probe: " + ("an amplicon cannot be lifted (%d)" % le.value if le.value else "an amplicon off its record, an edit that is none of its amplicon, or tables that do not fit each other"))
        e.lift_err = le.value
        raise e
    out = C.create_string_buffer(max(1, n.value))
    rc = L.scs_artefact_ref_probe(*args, out, n.value, C.byref(n), unl.ctypes.data, C.byref(le))
    if rc:
        raise ScsError(rc, "scs_artefact_ref_probe")
    return out.raw[:n.value].decode(), (int(unl[0]), int(unl[1]))


def support_ref_probe(table, hap_lens, ref_lens, x, chunk=0, g_counts=None):
    """Host-only: the expansion of the site support table on the reference (and, with g_counts, its gather) through the functions
    the kernels run.  table: a LiftTable (or any object with its five arrays); hap_lens / ref_lens: the staged and the reference
    records; x: the listed reference positions X, ascending and distinct; chunk: output slots per fill pass (0: all at once);
    g_counts: uint32 [staged bases, 6], the counters of every staged index.  Returns (staged positions, the index into x of each,
    uint32 [len(x), 6] sums or None).  A refused input raises ScsError (SCS_EINVAL) whose .why says which check failed."""
    import numpy as np
    L = load_library()
    L.scs_support_ref_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_int)]
    seg = [np.ascontiguousarray(getattr(table, k), t) for k, t in (("hap_off", np.uint64), ("len", np.uint64), ("ref_pos", np.uint64), ("ref_rec", np.uint32), ("kind", np.uint32))]
    h_l, r_l = np.ascontiguousarray(list(hap_lens), np.uint64), np.ascontiguousarray(list(ref_lens), np.uint64)
    xs = np.ascontiguousarray(x, np.uint64).reshape(-1)
    gc = None if g_counts is None else np.ascontiguousarray(g_counts, np.uint32)
    if gc is not None and gc.shape != (int(h_l.sum()), 6):
        raise ValueError("g_counts is [staged bases, 6]")
    head = [a.ctypes.data for a in seg] + [len(seg[0]), h_l.ctypes.data, len(h_l), r_l.ctypes.data, len(r_l), xs.ctypes.data if len(xs) else None, len(xs), int(chunk),
                                           None if gc is None else gc.ctypes.data]
    n, why = C.c_uint64(), C.c_int()

    def refuse(rc):
        e = ScsError(rc, "scs_support_ref_probe: " + {2: "a segment that does not follow the last, holds no base or leaves its staged record", 3: "a segment past its reference record",
                                                      4: "listed positions out of order or outside the reference", 5: "staged positions that do not ascend",
                                                      6: "a counter past 2^32 - 1"}.get(why.value, "tables that do not fit each other"))
        e.why = why.value
        return e
    rc = L.scs_support_ref_probe(*head, None, None, 0, C.byref(n), None, C.byref(why))
    if rc and not (rc == SCS_EOVERFLOW and n.value):
        raise refuse(rc)
    pos, pos_x = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
    out = None if gc is None else np.zeros((len(xs), 6), np.uint32)
    rc = L.scs_support_ref_probe(*head, pos.ctypes.data, pos_x.ctypes.data, n.value, C.byref(n), None if out is None else out.ctypes.data, C.byref(why))
    if rc:
        raise refuse(rc)
    return pos, pos_x, out


def support_ref_header_probe(ref_names, ref_lens, unlifted=(0, 0)):
    """Host-only: the header of the site support table on the reference, as write_site_support_ref writes it."""
    import numpy as np
    L = load_library()
    L.scs_support_ref_header_probe.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    r_l = np.ascontiguousarray(list(ref_lens), np.uint64)
    names = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    n = C.c_size_t()
    args = [r_l.ctypes.data, names, len(ref_names), int(unlifted[0]), int(unlifted[1])]
    if L.scs_support_ref_header_probe(*args, None, 0, C.byref(n)):
        raise ScsError(SCS_EINVAL, "scs_support_ref_header_probe")
    out = C.create_string_buffer(max(1, n.value))
    if L.scs_support_ref_header_probe(*args, out, n.value, C.byref(n)):
        raise ScsError(SCS_EINVAL, "scs_support_ref_header_probe")
    return out.raw[:n.value].decode()


def fasta_probe(path):
    """Host-only: (names, total bases, FNV-1a checksum of the upper-cased sequence) as the library stages the file."""
    L = load_library()
    n, tot, h = C.c_int(), C.c_uint64(), C.c_uint64()
    names, err = C.create_string_buffer(1 << 16), C.create_string_buffer(512)
    rc = L.scs_fasta_probe(os.fsencode(path), C.byref(n), C.byref(tot), C.byref(h), names, 1 << 16, err, 512)
    if rc:
        raise ScsError(rc, err.value.decode())
    return names.value.decode().split("\n")[:n.value], tot.value, h.value


class Profile:
    """Host-only view of a .profile model: the exact uint32 thresholds and the double CDFs they come from
    (mirrors Profile::train(file), reference lib/profile/Profile.cpp:1432-1436).  Needs no GPU."""

    TABLES = {"subs1": 0, "subs2": 1, "qual": 2, "ins": 3, "del": 4, "isize": 5, "qual_alias": 6}

    def __init__(self, path, paired=True, isize=260):
        import numpy as np
        self._np = np
        L = load_library()
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = L.scs_profile_open(os.fsencode(path), int(paired), int(isize), C.byref(self._h), err, 512)
        if rc:
            raise ScsError(rc, err.value.decode())
        sc = (C.c_double * 10)()
        L.scs_profile_scalars(self._h, sc)
        (self.read_length, self.bins, self.t_insert, self.t_delete, self.isize_min, self.have_cdf2) = [int(v) for v in sc[:6]]
        self.insert_rate, self.del_rate = sc[6], sc[7]
        self.t_indel, self.qual_k = int(sc[8]), int(sc[9])

    def table(self, name):
        np = self._np
        thr = C.POINTER(C.c_uint32)()
        cdf = C.POINTER(C.c_double)()
        n = C.c_size_t()
        rc = load_library().scs_profile_table(self._h, self.TABLES[name], C.byref(thr), C.byref(cdf), C.byref(n))
        if rc:
            raise ScsError(rc, "bad table")
        if n.value == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.float64)
        if not cdf:                                   # tables without a double twin (compact quality rows)
            return np.ctypeslib.as_array(thr, (n.value,)).copy(), None
        return (np.ctypeslib.as_array(thr, (n.value,)).copy(), np.ctypeslib.as_array(cdf, (n.value,)).copy())

    def close(self):
        if self._h:
            load_library().scs_profile_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GenReads:
    """One `scssim genreads` job on one MI355X.  Mirrors the reference's driver (src/scssim.cpp:46-67)."""

    def __init__(self, profile=None, input_fasta=None, primers=100000, gamma=1e-9, coverage=5.0, isize=260,
                 layout="PE", seed=1, device=0, stream=None, shard_rank=0, shard_count=1, verbose=False, ber=3.4e-4):
        import numpy as np
        self._np = np
        self._L = load_library()
        cfg = _Config()
        self._L.scs_default_config.argtypes = [C.POINTER(_Config)]
        self._L.scs_default_config(C.byref(cfg))
        cfg.device, cfg.stream, cfg.seed = device, stream, seed
        cfg.primers, cfg.gamma, cfg.coverage, cfg.isize = primers, gamma, coverage, isize
        cfg.ber = ber                         # amplification error rate per base (Config "ber"); 0: no amplification errors
        if layout not in ("PE", "SE"):
            raise ValueError("Error: sequence layout incorrectly specified!")
        cfg.paired = 1 if layout == "PE" else 0
        cfg.shard_rank, cfg.shard_count, cfg.verbose = shard_rank, shard_count, int(verbose)
        self.paired = bool(cfg.paired)
        self._ctx = C.c_void_p()
        rc = self._L.scs_create(C.byref(cfg), C.byref(self._ctx))
        if rc:
            raise ScsError(rc, self._L.scs_last_error(None).decode())
        if input_fasta is not None:
            self.load_genome(input_fasta)
        if profile is not None:
            self.load_profile(profile)

    # ---- plumbing
    def _ck(self, rc):
        if rc:
            raise ScsError(rc, self._L.scs_last_error(self._ctx).decode())

    def close(self):
        if self._ctx:
            self._L.scs_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference call sequence
    def load_genome(self, path):            # Genome::loadData
        self._ck(self._L.scs_load_genome_fasta(self._ctx, os.fsencode(path)))

    def upload_genome(self, names, seqs):
        n = len(names)
        bn = [s.encode() if isinstance(s, str) else s for s in names]
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        self._ck(self._L.scs_upload_genome(self._ctx, n, (C.c_char_p * n)(*bn), (C.c_char_p * n)(*bs),
                                           (C.c_uint64 * n)(*[len(s) for s in bs])))

    def upload_genome_device(self, names, lens, d_bases):
        """Genome already in HBM: d_bases = device pointer to the records' ASCII bases, concatenated (sum(lens) bytes)."""
        n = len(names)
        bn = [s.encode() if isinstance(s, str) else s for s in names]
        self._ck(self._L.scs_upload_genome_device(self._ctx, n, (C.c_char_p * n)(*bn), (C.c_uint64 * n)(*[int(x) for x in lens]), C.c_void_p(int(d_bases))))

    def simuvars(self, ref_fasta, snp_file=None, var_file=None, out_fasta=None):
        """`scssim simuvars` on the data plane: the two haplotypes of every chromosome are built in HBM and stay resident
        as the genreads input (no intermediate FASTA); out_fasta additionally writes the reference's simuvars file."""
        enc = lambda p: os.fsencode(p) if p else None
        self._ck(self._L.scs_simuvars(self._ctx, enc(ref_fasta), enc(snp_file), enc(var_file), enc(out_fasta)))

    def load_profile(self, path):           # Profile::train(file)
        self._ck(self._L.scs_load_profile(self._ctx, os.fsencode(path)))

    @property
    def read_length(self):
        return self._L.scs_read_length(self._ctx)

    def set_collectives(self, coll, device_hooks=False):
        """Sharded single job (shard_count > 1): `coll` = scssim_amd.dist.Collectives (torch.distributed hooks).
        device_hooks=True: collectives act on the library's HBM buffers directly (create the GenReads on torch's
        current stream: stream=torch.cuda.current_stream().cuda_stream)."""
        self._coll = coll                      # keep the ctypes callbacks alive
        self._ck(self._L.scs_set_collectives(self._ctx, C.cast(coll.allreduce_cb, C.c_void_p), C.cast(coll.allgatherv_cb, C.c_void_p), None))
        if device_hooks:
            self._ck(self._L.scs_set_collectives_device(self._ctx, C.cast(coll.allreduce_dev_cb, C.c_void_p), C.cast(coll.allgather_dev_cb, C.c_void_p), None))

    def set_seed(self, seed):
        self._ck(self._L.scs_set_seed(self._ctx, seed))

    def create_frags(self):                 # Malbac::createFrags
        self._ck(self._L.scs_create_frags(self._ctx))

    def amplify(self):                      # Malbac::amplify
        self._ck(self._L.scs_amplify(self._ctx))

    def allocate_reads(self, reads=0):      # Malbac::setReadCounts
        self._ck(self._L.scs_allocate_reads(self._ctx, reads))

    def alloc_probe(self, weights, seg_counts, reads):
        """Test seam: the read allocation behind the weights on this (never amplified) ctx, over `weights` as this shard's list cut into
        segments of seg_counts[40] amplicons; layout, seed, shard and collectives are the ctx's.  Returns (read numbers, pair offsets
        [n + 1]); the ctx stays not allocated."""
        np = self._np
        self._L.scs_alloc_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        w = np.ascontiguousarray(weights, np.float64)
        sc = np.ascontiguousarray(seg_counts, np.uint32)
        assert sc.shape == (ALLOC_SLOTS,)
        rn, po = np.zeros(max(1, w.size), np.uint32), np.zeros(w.size + 1, np.uint32)
        self._ck(self._L.scs_alloc_probe(self._ctx, w.ctypes.data if w.size else None, w.size, sc.ctypes.data, int(reads), rn.ctypes.data, po.ctypes.data))
        return rn[:w.size], po

    def yield_reads(self, collect=True):    # Malbac::yieldReads -> (fastq1, fastq2) bytes
        parts1, parts2 = [], []

        def sink(_u, p1, n1, p2, n2):
            if collect:
                parts1.append(C.string_at(p1, n1) if n1 else b"")
                parts2.append(C.string_at(p2, n2) if n2 else b"")
            return 0
        cb = _SINK(sink) if collect else _SINK()   # NULL sink: generate on the device and count only
        self._ck(self._L.scs_yield_reads(self._ctx, cb, None))
        return b"".join(parts1), b"".join(parts2)

    def yield_reads_sink(self, sink=None):
        """Malbac::yieldReads with a caller-supplied sink(user, p1, n1, p2, n2) -> int (host pointers valid during the call),
        or None: the FASTQ text is generated batch by batch into HBM buffers and counted only."""
        cb = _SINK(sink) if sink is not None else _SINK()
        self._ck(self._L.scs_yield_reads(self._ctx, cb, None))

    def yield_reads_files(self, prefix, writers=0, generations=1, bgzf=False, in_place=False):
        """Malbac::yieldReads + SeqWriter: <prefix>_1.fq/_2.fq (.fq), or this shard's <prefix>.r<rank>_*.fq + .idx.
        writers = K > 1: K part files per mate (<base>.p00_1.fq ...: contiguous record ranges, one writer thread each; their
        concatenation is the single file) + <base>.parts.  generations = G > 1: K x G parts made generation by generation (part p
        is final once part p + K exists).  bgzf: <...>.fq.gz, BGZF blocks made on the GPU.  in_place: files that exist are overwritten
        where they lie and cut to length at the end, not truncated first (SCS_SINK_IN_PLACE)."""
        self._L.scs_yield_reads_files_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        self._ck(self._L.scs_yield_reads_files_ex(self._ctx, os.fsencode(prefix), int(writers), int(generations), (1 if bgzf else 0) | (2 if in_place else 0)))

    def comm_init(self, comm_id, rank, nranks):
        """RCCL inside the library: every rank of a sharded job calls this with rank 0's comm_unique_id()."""
        self._id = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._ck(self._L.scs_comm_init(self._ctx, self._id, int(rank), int(nranks)))

    def comm_count(self):
        """Ranks of the ctx's RCCL communicator as RCCL reports them (ncclCommCount); 0 without one."""
        self._L.scs_comm_count.argtypes = [C.c_void_p]
        return int(self._L.scs_comm_count(self._ctx))

    def yield_reads_device(self, d_fq1, cap1, d_fq2, cap2):
        """FASTQ pool stays in HBM: d_fq1/d_fq2 are device pointers (e.g. torch uint8 tensors' data_ptr())."""
        n1, n2, pairs = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._ck(self._L.scs_yield_reads_device(self._ctx, d_fq1, cap1, d_fq2, cap2, C.byref(n1), C.byref(n2), C.byref(pairs)))
        return n1.value, n2.value, pairs.value

    def run_genreads(self, collect=True):
        """scs_run_genreads: createFrags + amplify + allocate + yield in ONE call of the C ABI (main()'s genreads branch,
        src/scssim.cpp:59-65)."""
        out1, out2 = bytearray(), bytearray()

        def on_batch(_u, p1, n1, p2, n2):
            if collect:
                if n1:
                    out1.extend(C.string_at(p1, n1))
                if n2:
                    out2.extend(C.string_at(p2, n2))
            return 0
        cb = _SINK(on_batch)
        self._ck(self._L.scs_run_genreads(self._ctx, cb, None))
        return bytes(out1), bytes(out2)

    def run(self, collect=True):
        self.create_frags()
        self.amplify()
        self.allocate_reads(0)
        return self.yield_reads(collect)

    def run_to_files(self, prefix):
        fq1, fq2 = self.run()
        if self.paired:
            open(prefix + "_1.fq", "wb").write(fq1)
            open(prefix + "_2.fq", "wb").write(fq2)
        else:
            open(prefix + ".fq", "wb").write(fq1)

    def set_truth_sam(self, path):
        """The following yield calls also write each read's true alignment to `path` as SAM (None: off).  One GPU, one writer."""
        self._L.scs_set_truth_sam.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_set_truth_sam(self._ctx, os.fsencode(path) if path is not None else None))

    def set_truth_bam(self, path):
        """The same records as BAM, made and compressed on the GPU (None: off).  One truth output per ctx: fails while the SAM is on."""
        self._L.scs_set_truth_bam.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_set_truth_bam(self._ctx, os.fsencode(path) if path is not None else None))

    def set_truth_ref_sam(self, path):
        """The reads' true alignments on the ORIGINAL REFERENCE as SAM, lifted through the lift table on the GPU (None: off).  Needs a
        lift table (simuvars, load_lift); one truth output per ctx: fails while the SAM or the BAM is on."""
        self._L.scs_set_truth_ref_sam.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_set_truth_ref_sam(self._ctx, os.fsencode(path) if path is not None else None))

    def truth_bytes(self):
        """Bytes of the truth SAM (header included) or BAM (compressed, header and end-of-file block included) the last yield call wrote."""
        self._L.scs_truth_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        n = C.c_uint64()
        self._ck(self._L.scs_truth_bytes(self._ctx, C.byref(n)))
        return n.value

    def set_depth(self, bin_width):
        """The following yield calls also count, per bin of bin_width bases of the staged records, the reads that start in the bin
        and the bases aligned in it, on the GPU (0: off).  Any sink, any writers, the text left in HBM; not a sharded job."""
        self._L.scs_set_depth.argtypes = [C.c_void_p, C.c_uint32]
        self._ck(self._L.scs_set_depth(self._ctx, int(bin_width)))

    def depth_bins(self):
        """(number of bins, bin width) of the depth track for the staged genome."""
        self._L.scs_depth_bins.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        n, w = C.c_uint64(), C.c_uint32()
        self._ck(self._L.scs_depth_bins(self._ctx, C.byref(n), C.byref(w)))
        return n.value, w.value

    def depth(self):
        """(reads, bases, bin_off) of the last yield call: the two counters per bin (uint64) and the first bin of every staged
        record (records + 1 entries)."""
        np = self._np
        n, w = self.depth_bins()
        reads, bases = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._L.scs_download_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self._ck(self._L.scs_download_depth(self._ctx, reads.ctypes.data, bases.ctypes.data, n))
        bin_off = np.zeros(self.stats()["records"] + 1, np.uint64)
        self._L.scs_depth_record_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._ck(self._L.scs_depth_record_bins(self._ctx, bin_off.ctypes.data, bin_off.size))
        return reads, bases, bin_off

    def write_depth(self, path):
        """The depth track of the last yield call as tab-separated text: #record, start, end (BED coordinates), reads, bases."""
        self._L.scs_write_depth.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_write_depth(self._ctx, os.fsencode(path)))

    def set_coverage(self, max_depth):
        """Coverage profile: the following yield calls also keep the per-base depth of the staged genome (the M operations of the
        truth CIGAR, as the depth track's `bases`), its histogram per record with buckets 0 .. max_depth (the last one depth >=
        max_depth; N bases in none) and the exact sums.  max_depth in 1 .. 65535; 0 turns it off and releases the arrays."""
        self._L.scs_set_coverage.argtypes = [C.c_void_p, C.c_uint32]
        self._ck(self._L.scs_set_coverage(self._ctx, int(max_depth)))

    def coverage_shape(self):
        """(staged records, max_depth) of the coverage profile."""
        return self._shape("scs_coverage_shape")

    def coverage(self):
        """The tables of the last yield call as numpy uint64 arrays: dict(hist=[records + 1][max_depth + 1], n_bases=, sum=, sum_n=
        [records + 1]); the last row is the genome."""
        np = self._np
        nr, D = self.coverage_shape()
        a = dict(hist=np.zeros((nr + 1, D + 1), np.uint64), n_bases=np.zeros(nr + 1, np.uint64), sum=np.zeros(nr + 1, np.uint64), sum_n=np.zeros(nr + 1, np.uint64))
        self._L.scs_download_coverage.argtypes = [C.c_void_p] * 5 + [C.c_uint64]
        self._ck(self._L.scs_download_coverage(self._ctx, *[a[k].ctypes.data for k in ("hist", "n_bases", "sum", "sum_n")], nr + 1))
        return a

    def coverage_range(self, record, start, end):
        """The per-base depth of [start, end) of staged record `record` after the last yield call, as numpy uint32."""
        np = self._np
        out = np.zeros(max(0, int(end) - int(start)), np.uint32)
        self._L.scs_coverage_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        self._ck(self._L.scs_coverage_range(self._ctx, int(record), int(start), int(end), out.ctypes.data))
        return out

    def write_coverage(self, path):
        """The coverage profile of the last yield call as text: summary lines per record and for the genome (bases, N bases, aligned
        bases, mean depth, breadth at 1 / 5 / 10 / 20, Gini), then `bedtools genomecov`'s five columns."""
        self._L.scs_write_coverage.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_write_coverage(self._ctx, os.fsencode(path)))

    def coverage_kernel_time(self, which=0):
        """Event pairs, milliseconds and units of the last yield call's coverage passes: which=0 the per-batch marks (units: pairs),
        1 the end-of-job pass (units: staged bases)."""
        return self._kernel_time("scs_coverage_kernel_time", which)

    def set_coverage_ref(self, max_depth):
        """Coverage profile on the reference: the following yield calls also keep, per base of the reference records of the lift
        table, the summed per-base depth of every staged base that lifts to it (every haplotype and tandem copy), its histogram
        per reference record and the depth by true copy number.  max_depth in 1 .. 65535, its own; 0 turns it off and releases the
        arrays.  It brings the staged array of set_coverage with it; what set_coverage exposes still needs set_coverage."""
        self._L.scs_set_coverage_ref.argtypes = [C.c_void_p, C.c_uint32]
        self._ck(self._L.scs_set_coverage_ref(self._ctx, int(max_depth)))

    def coverage_ref_shape(self):
        """(reference records, max_depth) of the coverage profile on the reference."""
        return self._shape("scs_coverage_ref_shape")

    def download_coverage_ref(self):
        """The tables of the last yield call on the reference as numpy uint64 arrays: dict(hist=[ref records + 1][max_depth + 1],
        n_bases=, absent=, sum=, sum_n= [ref records + 1], cn_bases=, cn_sum= [ref records + 1][17], unlifted=int); the last row is the genome."""
        np = self._np
        nf, D = self.coverage_ref_shape()
        a = dict(hist=np.zeros((nf + 1, D + 1), np.uint64), n_bases=np.zeros(nf + 1, np.uint64), absent=np.zeros(nf + 1, np.uint64), sum=np.zeros(nf + 1, np.uint64), sum_n=np.zeros(nf + 1, np.uint64),
                 cn_bases=np.zeros((nf + 1, 17), np.uint64), cn_sum=np.zeros((nf + 1, 17), np.uint64))
        unl = C.c_uint64()
        self._L.scs_download_coverage_ref.argtypes = [C.c_void_p] * 8 + [C.POINTER(C.c_uint64), C.c_uint64]
        self._ck(self._L.scs_download_coverage_ref(self._ctx, *[a[k].ctypes.data for k in ("hist", "n_bases", "absent", "sum", "sum_n", "cn_bases", "cn_sum")], C.byref(unl), nf + 1))
        a["unlifted"] = unl.value
        return a

    def coverage_ref_range(self, ref_record, start, end):
        """(depth, copies) of [start, end) of reference record `ref_record` after the last yield call, as numpy uint32: the summed
        per-base depth and the staged bases that lift to each base (its true copy number)."""
        np = self._np
        n = max(0, int(end) - int(start))
        d, cp = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._L.scs_coverage_ref_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        self._ck(self._L.scs_coverage_ref_range(self._ctx, int(ref_record), int(start), int(end), d.ctypes.data, cp.ctypes.data))
        return d, cp

    def write_coverage_ref(self, path):
        """The coverage profile on the reference of the last yield call as text: write_coverage's lines per reference record (with
        `absent`), the mean depth by true copy number (#c lines), what lies in inserted sequence (#unlifted), genomecov's columns."""
        self._L.scs_write_coverage_ref.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_write_coverage_ref(self._ctx, os.fsencode(path)))

    def coverage_ref_kernel_time(self, which=0):
        """Event pairs, milliseconds and units (staged bases) of the last yield call's passes on the reference: which=0 the
        once-per-layout copies kernel (no launch while the layout stands), 1 the end-of-job lift and count."""
        return self._kernel_time("scs_coverage_ref_kernel_time", which)

    def _write_bedgraph(self, name, path):
        fn = getattr(self._L, name)
        fn.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lines, text = C.c_uint64(), C.c_uint64()
        self._ck(fn(self._ctx, os.fsencode(path), C.byref(lines), C.byref(text)))
        return dict(lines=lines.value, text_bytes=text.value)

    def write_coverage_bedgraph(self, path):
        """The per-base depth of the staged genome after the last yield call (set_coverage on) as bedGraph, encoded on the GPU: one
        line `name start end depth` per maximal run of equal depth inside a record, depth 0 included (`bedtools genomecov -bga`).
        A path ending in .gz is written in BGZF.  Returns dict(lines=, text_bytes=) (uncompressed); may be repeated."""
        return self._write_bedgraph("scs_write_coverage_bedgraph", path)

    def write_coverage_ref_bedgraph(self, path):
        """The same for the per-base depth of the original reference (set_coverage_ref on, a lift table), under the reference's
        record names."""
        return self._write_bedgraph("scs_write_coverage_ref_bedgraph", path)

    def write_copy_number_ref(self, path):
        """The per-base true copy number of the original reference as bedGraph: per maximal segment the staged bases that lift to
        each of its bases, 0 where every haplotype lost it (set_coverage_ref on, a lift table)."""
        return self._write_bedgraph("scs_write_copy_number_ref", path)

    def coverage_bedgraph_kernel_time(self):
        """Event pairs, milliseconds and units (bases) of the bedGraph writer's kernels in the last write call."""
        return self._kernel_time("scs_coverage_bedgraph_kernel_time")

    def gc_bias(self, window=100, cap_rows=None):
        """The GC-bias table of the last yield call's per-base depth (set_coverage on), made on the GPU at this call: every window
        of `window` bases (1 .. 1024) inside a staged record, sliding by one base, is counted under bin 100 * gc / window; a window
        that holds an N only in n_windows.  dict of numpy arrays with records + 1 rows, the genome's last: windows, depth_sum
        (uint64[rows][101]), n_windows (uint64[rows]) and, derived here as the file derives them, mean_depth, normalized
        (float64[rows][101]) and row_mean (float64[rows]).  May be repeated with any window; the arrays are only read.  cap_rows:
        the rows the call is told there is room for (default: all)."""
        np = self._np
        nr, _ = self.coverage_shape()
        W = int(window)
        a = dict(windows=np.zeros((nr + 1, 101), np.uint64), depth_sum=np.zeros((nr + 1, 101), np.uint64), n_windows=np.zeros(nr + 1, np.uint64))
        self._L.scs_gc_bias.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self._ck(self._L.scs_gc_bias(self._ctx, W & 0xFFFFFFFF, *[a[k].ctypes.data for k in ("windows", "depth_sum", "n_windows")], nr + 1 if cap_rows is None else int(cap_rows)))
        n, s = a["windows"].astype(np.float64), a["depth_sum"].astype(np.float64)
        tot_n, tot_s = a["windows"].sum(axis=1).astype(np.float64), a["depth_sum"].sum(axis=1).astype(np.float64)
        a["mean_depth"] = np.divide(s, n * W, out=np.zeros_like(s), where=n > 0)
        a["row_mean"] = np.divide(tot_s, W * tot_n, out=np.zeros_like(tot_s), where=tot_n > 0)
        a["normalized"] = np.divide(a["mean_depth"], a["row_mean"][:, None], out=np.zeros_like(s), where=a["row_mean"][:, None] > 0)
        return a

    def write_gc_bias(self, path, window=100):
        """gc_bias(window) as text written by the host: a `#gc_bias` line stating the window, `#s` summary lines per record and for
        the genome (windows, n_windows, mean depth), then `record gc windows depth_sum mean_depth normalized model` for every bin
        with windows, the genome's rows last; model is the loaded profile's gc_means[gc]."""
        self._L.scs_write_gc_bias.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
        self._ck(self._L.scs_write_gc_bias(self._ctx, os.fsencode(path), int(window) & 0xFFFFFFFF))

    def gc_bias_kernel_time(self):
        """Event pairs, milliseconds and units (staged bases) of the GC-bias kernel in the last gc_bias / write_gc_bias call."""
        return self._kernel_time("scs_gc_bias_kernel_time")

    def amplicon_places(self):
        """The amplified pool after allocate_reads, one entry per full amplicon in list order (the index the read names print): dict
        of numpy arrays rec (staged record), start (0-based record coordinate), len, strand (+1 / -1), n_edits (bases where the
        amplicon differs from the genome it copies).  Made on the GPU; not a sharded job."""
        np = self._np
        n = self.stats()["full_amplicons"]
        a = dict(rec=np.zeros(n, np.uint32), start=np.zeros(n, np.uint64), len=np.zeros(n, np.uint32), strand=np.zeros(n, np.int8), n_edits=np.zeros(n, np.uint32))
        self._L.scs_amplicon_places.argtypes = [C.c_void_p] * 6 + [C.c_uint64]
        self._ck(self._L.scs_amplicon_places(self._ctx, *[a[k].ctypes.data for k in ("rec", "start", "len", "strand", "n_edits")], n))
        return a

    def write_amplicons(self, path, bgzf=False):
        """The same table as tab-separated text made on the GPU: #record, start, end (BED), amplicon, strand, reads, semi, edits
        (pos:R>A joined by commas, or "."); bgzf: BGZF blocks compressed on the GPU.  Returns the file's size in bytes."""
        self._L.scs_write_amplicons.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
        n = C.c_uint64()
        self._ck(self._L.scs_write_amplicons(self._ctx, os.fsencode(path), 1 if bgzf else 0, C.byref(n)))
        return n.value

    def _kernel_time(self, symbol, which=None):
        fn = getattr(self._L, symbol)
        lead = [] if which is None else [int(which)]       # the entry points with more than one timer take its index first
        fn.argtypes = [C.c_void_p] + [C.c_int] * len(lead) + [C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        n, ms, u = C.c_uint64(), C.c_double(), C.c_uint64()
        self._ck(fn(self._ctx, *lead, C.byref(n), C.byref(ms), C.byref(u)))
        return dict(launches=n.value, ms=ms.value, units=u.value)

    def _shape(self, symbol):
        fn = getattr(self._L, symbol)
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        n, d = C.c_uint32(), C.c_uint32()
        self._ck(fn(self._ctx, C.byref(n), C.byref(d)))
        return n.value, d.value

    def amplicon_kernel_time(self):
        """Event pairs, milliseconds and amplicons of the last write_amplicons call's kernels."""
        return self._kernel_time("scs_amplicon_kernel_time")

    def write_artefacts(self, path, bgzf=False, min_reads=0):
        """The amplification's artefacts by genome site as a sorted VCF made on the GPU, after allocate_reads: per (record, coordinate,
        alternate base) NA / TA (full amplicons that carry it / that cover the site) and NR / TR (the reads allotted to them).
        min_reads: only sites with NR >= min_reads; bgzf: BGZF blocks compressed on the GPU.  Returns dict(sites=, bytes=)."""
        self._L.scs_write_artefacts.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        n, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.scs_write_artefacts(self._ctx, os.fsencode(path), 1 if bgzf else 0, int(min_reads), C.byref(n), C.byref(b)))
        return dict(sites=n.value, bytes=b.value)

    _SITE_ARRAYS = dict(pos="uint64", ref="uint8", alt="uint8", na="uint32", ta="uint32", nr="uint64", tr="uint64")

    def _sites_into_arrays(self, symbol, rec_key, head=(), counts=False, tail=()):
        """A site table's two calls: ask for the number of sites, then fill numpy arrays of that size.  rec_key: what the record
        array is called; head: the arguments between ctx and the arrays; counts: a [sites, 6] array behind the eight; tail: extra
        out-parameters behind n."""
        np = self._np
        fn = getattr(self._L, symbol)
        na = 9 if counts else 8
        fn.argtypes = [C.c_void_p] + [C.c_uint32] * len(head) + [C.c_void_p] * na + [C.c_uint64, C.POINTER(C.c_uint64)] + [C.POINTER(C.c_uint64)] * len(tail)
        n = C.c_uint64()
        rc = fn(self._ctx, *head, *([None] * na), 0, C.byref(n), *tail)
        if rc and not (rc == SCS_EOVERFLOW and n.value):
            self._ck(rc)
        a = {rec_key: np.zeros(n.value, np.uint32)}
        a.update((k, np.zeros(n.value, getattr(np, t))) for k, t in self._SITE_ARRAYS.items())
        if counts:
            a["counts"] = np.zeros((n.value, 6), np.uint32)
        if n.value:
            self._ck(fn(self._ctx, *head, *[x.ctypes.data for x in a.values()], n.value, C.byref(n), *tail))
        return a

    def artefact_sites(self, min_reads=0):
        """The same table as a dict of numpy arrays, one entry per site in file order: rec (staged record), pos (0-based record
        coordinate), ref (code 0..4), alt (0..3), na, ta, nr, tr."""
        return self._sites_into_arrays("scs_artefact_sites", "rec", head=(int(min_reads),))

    def artefact_kernel_time(self):
        """Event pairs, milliseconds and sites of the last write_artefacts call's kernels (the sorts and scans included)."""
        return self._kernel_time("scs_artefact_kernel_time")

    def write_artefacts_ref(self, path, bgzf=False, min_reads=0):
        """The amplification's artefacts by site of the ORIGINAL REFERENCE as a sorted VCF made on the GPU, after allocate_reads; needs
        a lift table (simuvars, load_lift).  Per (reference record, coordinate, the template's base, alternate base) NA / NR (the edit
        entries that lift to the site, their amplicons' reads) and TA / TR (the pieces of amplicons, of every haplotype and copy,
        that cover it, and theirs).  Returns dict(sites=, bytes=, unlifted_entries=, unlifted_reads=)."""
        self._L.scs_write_artefacts_ref.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        n, b, u = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 2)()
        self._ck(self._L.scs_write_artefacts_ref(self._ctx, os.fsencode(path), 1 if bgzf else 0, int(min_reads), C.byref(n), C.byref(b), u))
        return dict(sites=n.value, bytes=b.value, unlifted_entries=u[0], unlifted_reads=u[1])

    def artefact_ref_sites(self, min_reads=0):
        """The same table as a dict of numpy arrays, one entry per site in file order: ref_rec (reference record of the lift table), pos
        (0-based reference coordinate), ref (code 0..4), alt (0..3), na, ta, nr, tr; and unlifted = (entries, reads)."""
        u = (C.c_uint64 * 2)()
        a = self._sites_into_arrays("scs_artefact_ref_sites", "ref_rec", head=(int(min_reads),), tail=(u,))
        a["unlifted"] = (int(u[0]), int(u[1]))
        return a

    def artefact_ref_kernel_time(self):
        """Event pairs, milliseconds and sites of the last write_artefacts_ref call's kernels (the sorts and scans included)."""
        return self._kernel_time("scs_artefact_ref_kernel_time")

    def set_site_support(self, on, min_reads=0):
        """Site support on / off: every later yield call counts, on the GPU, what its reads show at the coordinates of the artefact
        sites with NR >= min_reads (artefact_sites(min_reads)): six counters per position.  Off releases every buffer of it."""
        self._L.scs_set_site_support.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        self._ck(self._L.scs_set_site_support(self._ctx, 1 if on else 0, int(min_reads)))

    def site_support(self):
        """The last yield call's sites and counters as a dict of numpy arrays, one entry per site in file order: artefact_sites' arrays
        and counts, uint32 [sites, 6]: reads that show A, C, G, T, another character, a deletion at the site's coordinate."""
        return self._sites_into_arrays("scs_site_support", "rec", counts=True)

    def write_site_support(self, path, bgzf=False):
        """The artefact VCF of the same min_reads with DP / AD / DL of the last yield call's reads at the end of every line, made on
        the GPU.  Returns dict(sites=, bytes=)."""
        self._L.scs_write_site_support.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        n, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.scs_write_site_support(self._ctx, os.fsencode(path), 1 if bgzf else 0, C.byref(n), C.byref(b)))
        return dict(sites=n.value, bytes=b.value)

    def set_site_support_ref(self, on, min_reads=0):
        """Site support by site of the ORIGINAL REFERENCE on / off (needs a lift table at the yield call): every later yield call
        counts, on the GPU, what its reads show at every staged position that lifts to a reference position of
        artefact_ref_sites(min_reads), and sums the six counters by reference position.  Not together with set_site_support."""
        self._L.scs_set_site_support_ref.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        self._ck(self._L.scs_set_site_support_ref(self._ctx, 1 if on else 0, int(min_reads)))

    def site_support_ref(self):
        """The last yield call's sites and counters as a dict of numpy arrays, one entry per site in file order: artefact_ref_sites'
        arrays (unlifted included) and counts, uint32 [sites, 6], summed over every haplotype record and copy of the site."""
        u = (C.c_uint64 * 2)()
        a = self._sites_into_arrays("scs_site_support_ref", "ref_rec", counts=True, tail=(u,))
        a["unlifted"] = (int(u[0]), int(u[1]))
        return a

    def write_site_support_ref(self, path, bgzf=False):
        """write_artefacts_ref's file of the same min_reads with DP / AD / DL of the last yield call's reads at the end of every
        line, made on the GPU.  Returns dict(sites=, bytes=)."""
        self._L.scs_write_site_support_ref.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        n, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.scs_write_site_support_ref(self._ctx, os.fsencode(path), 1 if bgzf else 0, C.byref(n), C.byref(b)))
        return dict(sites=n.value, bytes=b.value)

    def site_support_ref_kernel_time(self, step=None):
        """Event pairs (one per batch), milliseconds and pairs of the last yield call's k_support launches with the table on the
        reference on; step=0: the expansion behind the site table, step=1: the gather (units: staged positions)."""
        if step is None:
            return self._kernel_time("scs_site_support_ref_kernel_time")
        fn = self._L.scs_site_support_ref_step_time
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        n, ms, u = C.c_uint64(), C.c_double(), C.c_uint64()
        self._ck(fn(self._ctx, int(step), C.byref(n), C.byref(ms), C.byref(u)))
        return dict(launches=n.value, ms=ms.value, units=u.value)

    # ---- lift table and depth by reference bin
    def write_lift(self, path):
        """The staged genome's lift table (kept by simuvars, or read by load_lift) as text: ##scssim-lift v1."""
        self._L.scs_write_lift.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_write_lift(self._ctx, os.fsencode(path)))

    def load_lift(self, path):
        """Read the lift table `simuvars --lift` / write_lift wrote for the genome that is staged (after staging it)."""
        self._L.scs_load_lift.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_load_lift(self._ctx, os.fsencode(path)))

    def lift_info(self):
        """(segments, reference records) of the staged genome's lift table."""
        self._L.scs_lift_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        n, r = C.c_uint64(), C.c_uint32()
        self._ck(self._L.scs_lift_info(self._ctx, C.byref(n), C.byref(r)))
        return n.value, r.value

    def lift_segments(self):
        """The lift table as a LiftTable of numpy arrays, read back from the device copy (ref_lens filled in)."""
        np = self._np
        n, nr = self.lift_info()
        a = [np.zeros(max(n, 1), np.uint64) for _ in range(3)] + [np.zeros(max(n, 1), np.uint32) for _ in range(2)]
        rl = np.zeros(max(nr, 1), np.uint64)
        self._L.scs_lift_segments.argtypes = [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p, C.c_uint32]
        self._ck(self._L.scs_lift_segments(self._ctx, *[x.ctypes.data for x in a], n, rl.ctypes.data, nr))
        return LiftTable(*[x[:n] for x in a], ref_lens=rl[:nr])

    def lift_positions(self, rec, pos):
        """Staged positions (record index, 0-based coordinate) -> (ref_rec, ref_pos, kind) arrays, lifted on the GPU."""
        np = self._np
        rec, pos = np.ascontiguousarray(rec, np.uint32), np.ascontiguousarray(pos, np.uint64)
        n = len(rec)
        assert len(pos) == n
        rr, rp, k = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
        self._L.scs_lift_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self._L.scs_lift_positions(self._ctx, rec.ctypes.data, pos.ctypes.data, n, rr.ctypes.data, rp.ctypes.data, k.ctypes.data))
        return rr[:n], rp[:n], k[:n]

    def set_depth_ref(self, bin_width):
        """Depth by bin of the ORIGINAL REFERENCE through the lift table: the following yield calls count reads and aligned bases per
        bin of bin_width reference bases (0: off), plus one pseudo-bin for what has no reference coordinate."""
        self._L.scs_set_depth_ref.argtypes = [C.c_void_p, C.c_uint32]
        self._ck(self._L.scs_set_depth_ref(self._ctx, int(bin_width)))

    def depth_ref_bins(self):
        """(number of reference bins -- the pseudo-bin not counted --, bin width)."""
        self._L.scs_depth_ref_bins.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        n, w = C.c_uint64(), C.c_uint32()
        self._ck(self._L.scs_depth_ref_bins(self._ctx, C.byref(n), C.byref(w)))
        return n.value, w.value

    def depth_ref(self):
        """(reads, bases, copies, bin_off) of the last yield call: uint64 arrays of n_bins + 1 entries (the last one the pseudo-bin) and
        the first bin of every reference record (records + 1 entries)."""
        np = self._np
        n, _ = self.depth_ref_bins()
        _, nr = self.lift_info()
        reads, bases, copies, off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64), np.zeros(nr + 1, np.uint64)
        self._L.scs_download_depth_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self._ck(self._L.scs_download_depth_ref(self._ctx, reads.ctypes.data, bases.ctypes.data, copies.ctypes.data, n + 1))
        self._L.scs_depth_ref_record_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._ck(self._L.scs_depth_ref_record_bins(self._ctx, off.ctypes.data, off.size))
        return reads, bases, copies, off

    def write_depth_ref(self, path):
        """The same as text: #record, start, end (BED coordinates of the reference), reads, bases, copies; last line #unlifted."""
        self._L.scs_write_depth_ref.argtypes = [C.c_void_p, C.c_char_p]
        self._ck(self._L.scs_write_depth_ref(self._ctx, os.fsencode(path)))

    def depth_ref_kernel_time(self):
        """Event pairs (one per batch), milliseconds and pairs of the last yield call's k_depth_lift launches."""
        return self._kernel_time("scs_depth_ref_kernel_time")

    def site_support_kernel_time(self):
        """Event pairs (one per batch), milliseconds and pairs of the last yield call's k_support launches."""
        return self._kernel_time("scs_site_support_kernel_time")

    def download_frags(self):
        """The fragments of create_frags: genome offset (records concatenated in staging order), length, strand (+1 / -1)."""
        np = self._np
        n = self.stats()["fragments"]
        goff, ln, st = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.int8)
        self._L.scs_download_frags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(self._L.scs_download_frags(self._ctx, ptr(goff), ptr(ln), ptr(st)))
        return dict(goff=goff, len=ln, strand=st)

    def download_genome(self, has_n=False):
        """Test seam: what staging left on the device for the resident stretch of the genome (scs_download_genome), copied back as it
        lies: dict of slice_base, slice_len, names, rec_lens and the numpy arrays codes (uint8), gc_bits / n_bits / gc_pref / n_pref
        (uint64, words + 1), gc_pair (uint64 [words + 1, 2]), g2 (uint32, 4 x words); has_n=True, after create_frags: has_n (uint8
        per fragment of download_frags)."""
        np = self._np
        fn = self._L.scs_download_genome
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64] + [C.c_void_p] * 8
        info = np.zeros(4, np.uint64)
        self._ck(fn(self._ctx, info.ctypes.data, None, 0, None, 0, *([None] * 8)))
        base, n, nrec, nbytes = (int(v) for v in info)
        nw = (n + 63) // 64
        names, lens = C.create_string_buffer(max(1, nbytes)), np.zeros(max(1, nrec), np.uint64)
        a = dict(codes=np.zeros(n, np.uint8), gc_bits=np.zeros(nw + 1, np.uint64), n_bits=np.zeros(nw + 1, np.uint64), gc_pref=np.zeros(nw + 1, np.uint64),
                 n_pref=np.zeros(nw + 1, np.uint64), gc_pair=np.zeros((nw + 1, 2), np.uint64), g2=np.zeros(4 * nw, np.uint32))
        nf = self.stats()["fragments"] if has_n else 0
        hn = np.zeros(max(1, nf), np.uint8)                           # (a pointer even for no fragments: asking before create_frags is refused)
        ptr = lambda x: x.ctypes.data if x.size else None
        self._ck(fn(self._ctx, info.ctypes.data, names, nbytes, lens.ctypes.data, nrec, *[ptr(a[k]) for k in ("codes", "gc_bits", "n_bits", "gc_pref", "n_pref", "gc_pair", "g2")],
                    hn.ctypes.data if has_n else None))
        if has_n:
            a["has_n"] = hn[:nf]
        a.update(slice_base=base, slice_len=n, names=names.raw[:nbytes].decode("latin-1").split("\n")[:nrec], rec_lens=lens[:nrec].copy())
        return a

    def set_batch_checksums(self, on=True):
        """Every batch of the following yield_reads* calls gets a 64-bit checksum per mate, computed on the device."""
        self._L.scs_set_batch_checksums.argtypes = [C.c_void_p, C.c_int]
        self._ck(self._L.scs_set_batch_checksums(self._ctx, int(on)))

    def batch_checksums(self):
        """[(mate 1, mate 2), ...] of the last yield call's batches, in record order (see text_checksum)."""
        self._L.scs_batch_checksums.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        n = C.c_size_t()
        self._ck(self._L.scs_batch_checksums(self._ctx, None, 0, C.byref(n)))
        out = (C.c_uint64 * (2 * n.value))()
        self._ck(self._L.scs_batch_checksums(self._ctx, out, 2 * n.value, C.byref(n)))
        return [(out[2 * i], out[2 * i + 1]) for i in range(n.value)]

    # ---- introspection
    def stats(self):
        st = _Stats()
        self._ck(self._L.scs_get_stats(self._ctx, C.byref(st)))
        d = {k: getattr(st, k) for k, _ in _Stats._fields_ if k not in ("fastq_bytes", "t_stage", "sink_bytes")}
        d["fastq_bytes"] = list(st.fastq_bytes)
        d["sink_bytes"] = list(st.sink_bytes)
        d["t_stage"] = list(st.t_stage)
        return d

    def kernel_times(self):
        out = {}
        for i in range(len(self.KERNELS)):
            name, n, ms, units = C.c_char_p(), C.c_uint64(), C.c_double(), C.c_uint64()
            self._ck(self._L.scs_kernel_time(self._ctx, i, C.byref(name), C.byref(n), C.byref(ms), C.byref(units)))
            out[name.value.decode()] = dict(launches=n.value, ms=ms.value, units=units.value)
        return out

    KERNELS = ("k_errs<semi->full>", "k_errs<frag->semi>", "k_reads", "k_attach<semi>", "k_indels", "k_attach<frag>", "k_truth", "k_depth")

    def set_kernel_timing(self, names=None, every=1):
        """Keep HIP event pairs only around the named kernels (None = all eight), on every `every`-th amplify / yield call.
        Every event record is a packet on the stream (about 6 us each on the latency-bound 1 Mb job)."""
        mask = (1 << len(self.KERNELS)) - 1 if names is None else sum(1 << self.KERNELS.index(n) for n in names)
        self._ck(self._L.scs_set_kernel_timing(self._ctx, mask, every))

    def download_amplicons(self, kind):
        np = self._np
        st = self.stats()
        n = st["semi_amplicons"] if kind == 0 else st["full_amplicons"]
        a = {k: np.zeros(n, np.uint32) for k in ("parent", "spos", "len", "gc", "primers")}
        a["uid"] = np.zeros(n, np.uint64)
        a["errs"] = np.zeros((n, 4), np.uint32)
        a["nerr"] = np.zeros(n, np.uint32)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(self._L.scs_download_amplicons(self._ctx, kind, ptr(a["parent"]), ptr(a["spos"]), ptr(a["len"]), ptr(a["gc"]),
                                                ptr(a["primers"]), ptr(a["uid"]), ptr(a["errs"]), ptr(a["nerr"])))
        return a

    def download_primer_stock(self):
        """Copies of every primer type left after amplify (PrimerIndex.count, lib/malbac/Malbac.h:18-24), index = 2-bit-packed 8-mer."""
        import numpy as np
        st = np.zeros(65536, np.int64)
        self._ck(self._L.scs_download_primer_stock(self._ctx, st.ctypes.data_as(C.c_void_p)))
        return st

    def download_read_numbers(self):
        np = self._np
        rn = np.zeros(self.stats()["full_amplicons"], np.uint32)
        self._ck(self._L.scs_download_read_numbers(self._ctx, rn.ctypes.data_as(C.c_void_p)))
        return rn

    # ---- kernel-level entry points
    def predict_batch(self, windows, uids, attempts, is_read1):
        """Profile::predict for a batch of windows (n x L uint8 codes).  Returns (list of bases, list of quals)."""
        np = self._np
        w = np.ascontiguousarray(windows, np.uint8)
        n, L = w.shape
        assert L == self.read_length
        stride = ((L + 64 + 63) // 64) * 64
        u = np.ascontiguousarray(uids, np.uint64)
        a = np.ascontiguousarray(attempts, np.uint32)
        r = np.ascontiguousarray(is_read1, np.uint8)
        ob = np.zeros((n, stride), np.uint8)
        oq = np.zeros((n, stride), np.uint8)
        ol = np.zeros(n, np.int32)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        self._ck(self._L.scs_predict_batch(self._ctx, ptr(w), n, ptr(u), ptr(a), ptr(r), ptr(ob), ptr(oq), ptr(ol), stride))
        return [bytes(ob[i, :ol[i]]) for i in range(n)], [bytes(oq[i, :ol[i]]) for i in range(n)]

    def philox(self, ctr, key):
        np = self._np
        c = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
        k = np.ascontiguousarray(key, np.uint32)
        out = np.zeros_like(c)
        self._ck(self._L.scs_philox_batch(self._ctx, c.ctypes.data_as(C.c_void_p), c.shape[0], k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def det_log(self, x):
        np = self._np
        x = np.ascontiguousarray(x, np.float64)
        out = np.zeros_like(x)
        self._ck(self._L.scs_detlog_batch(self._ctx, x.ctypes.data_as(C.c_void_p), x.size, out.ctypes.data_as(C.c_void_p)))
        return out
