// scs_pipeline.cpp -- the C ABI (include/scssim_hip.h) over the host files of the library, and what they share: the mailbox.
// (The ABI's test seams and kernel-level probes are in scs_probes.cpp.)
// One scs_ctx = one HIP device + one stream; all amplicon state lives in HBM as flat SoA arrays (scs_ctx.h).
// Reference call sequence reproduced: src/scssim.cpp:46-67 (genreads branch of main()).
#include "scs_ctx.h"
#include <cerrno>

namespace scs {

std::string& create_error() { thread_local std::string e; return e; }

// ---- mailbox: device scalars -> pinned host words, no copy and no stream sync (k_mail)
void mail_post(scs_ctx* c, const Mail& m, bool last, hipStream_t st) {   // last: the post the host will wait for; st: the ctx stream unless given
    c->mail_stream = st ? st : c->stream;
    launch_mail(c->mail_stream, m.src, m.wd, m.dst, m.n, m.clear, c->d_rb, last ? ++c->mail_seq : 0ull);
}
void mail_wait(scs_ctx* c) {                                                      // everything posted so far has landed in h_rb
    volatile uint64_t* flag = c->h_rb + MAIL_SEQ_SLOT;
    // a post usually lands within tens of microseconds: spin (with the CPU's pause hint) for about that long, then back
    // off -- yield, then short sleeps -- so that a long device phase (a whole-genome pass, a collective waiting for another
    // rank) does not burn a host core; a failed or drained stream must not leave the host waiting either
    for (uint64_t spin = 1;; ++spin) {
        if (*flag == c->mail_seq) break;
        if (spin < 20000) { __builtin_ia32_pause(); continue; }
        if ((spin & 0x3F) == 0) {
            const hipError_t q = hipStreamQuery(c->mail_stream ? c->mail_stream : c->stream);
            if (q == hipSuccess) { if (*flag == c->mail_seq) break; throw ScsError(SCS_EDEVICE, "mailbox: stream drained without the expected post"); }
            if (q != hipErrorNotReady) throw ScsError(SCS_EDEVICE, std::string("mailbox: ") + hipGetErrorString(q));
        }
        if (spin < 20200) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(spin < 21000 ? 20 : 200));
    }
    std::atomic_thread_fence(std::memory_order_acquire);
}

// device-side overflow flags: slot 30 of the mailbox.  flags_eval reads what a post already brought (the caller has
// waited for that post, or synchronised the stream after it); check_flags posts and waits itself.
void flags_eval(scs_ctx* c) {
    { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("kernel launch failed: ") + hipGetErrorString(le)); }
    const uint32_t f = (uint32_t)c->h_rb[30];
    if (f) {
        HIP_OK(hipMemsetAsync(c->flags.p, 0, 4, c->stream));
        std::string m = "device work buffer overflow:";
        if (f & FLAG_ERRCAP) m += " per-amplicon error list";
        if (f & FLAG_ERRPOOL) m += " error overflow pool";
        if (f & FLAG_READSLOT) m += " read slot (indel-extended read longer than the slot)";
        if (f & FLAG_INTERNAL) m += " internal";
        if (f & FLAG_KEYSPACE) m += " primer budget of a fragment beyond 2^20 (-p / -r far outside the reference's ranges)";
        if (f & FLAG_TRUTH) m += " truth SAM / BAM (a read with more than 32 indel events, pair flags that are not a strand, a pair whose records outgrow the emit pass' LDS, or a record the two passes size differently)";
        if (f & FLAG_DEPTH) m += " depth track (a read with more than 32 indel events, pair flags that are not a strand, or a read placed outside its record)";
        if (f & FLAG_AMP) m += " amplicon table (a lineage that does not fit its parents, view flags that are not a strand, an amplicon outside its record, or a line the two passes size differently)";
        if (f & FLAG_SITE) m += " artefact table (an amplicon that cannot be placed, a slab whose entries differ from their count, site counts that contradict each other, or a line the two passes size differently)";
        if (f & FLAG_LIFT) m += " depth by reference bin / truth SAM on the reference (a read placed outside its record, an aligned run that leaves the lift table, a lifted coordinate outside its reference record, a read with more than 32 indel events, or pair flags that are not a strand; artefact table on the reference: an amplicon whose walk leaves the lift table or its record's segments, or a segment that lifts outside its reference record; coverage profile on the reference: a segment that lifts outside its reference record, or a staged base the table does not hold)";
        if (f & FLAG_SUPPORT) m += " site support (a read placed outside its record, pair flags that are not a strand, a read with more than 32 indel events, a FASTQ record that is not where the offsets say, or sites that are not in order" + std::string(c->support_ref ? "; on the reference: staged positions that do not ascend, or a reference counter past 2^32 - 1" : "") + ")";
        if (f & FLAG_COVERAGE) m += " coverage profile (a read placed outside its record, a read with more than 32 indel events, pair flags that are not a strand, a negative running depth, or a depth that is not 0 behind the genome's last base; on the reference: depth on a base no staged base lifts to)";
        if (f & FLAG_RUNS) m += " bedGraph text (a line or a tile the sizing pass and the emit pass size differently: the text would overflow its plan)";
        throw ScsError(SCS_EOVERFLOW, m);
    }
}
void check_flags(scs_ctx* c) {
    Mail m; m.add(c->flags.p, 4, 30); mail_post(c, m, true); mail_wait(c);
    flags_eval(c);
}

}  // namespace scs

// =================================================================== C ABI
extern "C" {

void scs_default_config(scs_config* cfg) {
    memset(cfg, 0, sizeof *cfg);
    cfg->device = 0; cfg->stream = nullptr; cfg->seed = 1;
    cfg->primers = 100000; cfg->gamma = 1e-9; cfg->coverage = 5; cfg->isize = 260; cfg->paired = 1;
    cfg->ber = 3.4e-4; cfg->amplicon_min_len = 1000; cfg->amplicon_max_len = 2000; cfg->frag_size = 1000;
    cfg->frag_min = 10000; cfg->frag_max = 100000; cfg->shard_rank = 0; cfg->shard_count = 1; cfg->verbose = 0;
}

int scs_create(const scs_config* cfg, scs_ctx** out) {
    if (!cfg || !out) { create_error() = "scs_create: null argument"; return SCS_EINVAL; }
    *out = nullptr;
    if (cfg->primers < 1000) { create_error() = "Error: the value of parameter \"primers\" should be at least 1000!"; return SCS_EINVAL; }
    if (cfg->gamma <= 0 || cfg->gamma > 1e-8) { create_error() = "Error: the value of parameter \"gamma\" should be in 0~1e-8!"; return SCS_EINVAL; }
    if (cfg->coverage <= 0) { create_error() = "Error: sequencing coverage not properly specified!"; return SCS_EINVAL; }
    if (cfg->shard_count < 1 || cfg->shard_rank < 0 || cfg->shard_rank >= cfg->shard_count) { create_error() = "scs_create: bad shard rank/count"; return SCS_EINVAL; }
    if (cfg->amplicon_max_len > 2047 || cfg->frag_max > 131071 || cfg->amplicon_min_len < 64) { create_error() = "scs_create: amplicon/fragment size outside the packed-record limits"; return SCS_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device) {
        create_error() = "scs_create: no HIP device " + std::to_string(cfg->device) + " (this library has no CPU fallback)"; return SCS_EDEVICE;
    }
    scs_ctx* c = new scs_ctx; c->cfg = *cfg;
    try {
        HIP_OK(hipSetDevice(cfg->device));
        if (cfg->stream) c->stream.adopt((hipStream_t)cfg->stream); else c->stream.ensure(hipStreamNonBlocking);
        c->key = RngKey{(uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32)};
        for (KernelTimer& t : c->tm) t.gate = &c->timing_gate;
        for (KernelTimer* t : c->yield_timers()) t->gate = &c->timing_gate;
        c->flags.reserve(256, c->stream); HIP_OK(hipMemsetAsync(c->flags.p, 0, 256, c->stream));
        c->dsums.reserve(256, c->stream); HIP_OK(hipMemsetAsync(c->dsums.p, 0, 256, c->stream));
        c->d_tot.reserve(256, c->stream);
        c->h_rb.reserve(256, hipHostMallocMapped | hipHostMallocCoherent); memset(c->h_rb, 0, 256);
        HIP_OK(hipHostGetDevicePointer((void**)&c->d_rb, c->h_rb, 0));
        HIP_OK(hipStreamSynchronize(c->stream));
    } catch (const std::exception& e) { create_error() = e.what(); delete c; return SCS_EDEVICE; }
    *out = c; return SCS_OK;
}

void scs_destroy(scs_ctx* c) {                              // the ctx's members free themselves (scs_ctx.h)
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
}

const char* scs_last_error(const scs_ctx* c) { return c ? c->err.c_str() : create_error().c_str(); }

int scs_set_seed(scs_ctx* c, uint64_t seed) {
    if (!c) return SCS_EINVAL;
    c->cfg.seed = seed; c->key = RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; return SCS_OK;
}

int scs_load_profile(scs_ctx* c, const char* path) { return guarded(c, [&] { if (!path) throw ScsError(SCS_EINVAL, "null path"); do_load_profile(c, path); }); }
int scs_read_length(const scs_ctx* c) { return c && c->have_profile ? c->prof.read_length : -1; }

int scs_load_genome_fasta(scs_ctx* c, const char* path) {
    return guarded(c, [&] {
        if (!path) throw ScsError(SCS_EINVAL, "null path");
        if (seam_env("SCS_HOST_FASTA")) { load_fasta(path, c->recs, true); stage_genome(c); }   // the host parser (what scs_fasta_probe checks); debugging aid
        else if (c->cfg.shard_count > 1 && !seam_env("SCS_STAGE_WHOLE") && stage_fasta_slice(c, fasta_plain_path(path))) {
            if (c->cfg.verbose) fprintf(stderr, "(shard %d of %d: %llu of %llu bases staged)\n", c->cfg.shard_rank, c->cfg.shard_count, (unsigned long long)c->slice_len, (unsigned long long)c->genome_bases);
        }
        else stage_fasta_on_device(c, path);
        if (c->cfg.verbose) fprintf(stderr, "\nReference sequence was loaded from file %s\n", path);
    });
}
int scs_upload_genome(scs_ctx* c, int n, const char* const* names, const char* const* seqs, const uint64_t* lens) {
    return guarded(c, [&] {
        if (n <= 0 || !names || !seqs || !lens) throw ScsError(SCS_EINVAL, "scs_upload_genome: bad arguments");
        c->recs.resize(n);
        for (int i = 0; i < n; ++i) encode_record(names[i], seqs[i], lens[i], c->recs[i]);
        stage_genome(c);
    });
}
int scs_upload_genome_device(scs_ctx* c, int n, const char* const* names, const uint64_t* lens, const void* d_bases) {
    return guarded(c, [&] {
        if (n <= 0 || !names || !lens || !d_bases) throw ScsError(SCS_EINVAL, "scs_upload_genome_device: bad arguments");
        c->recs.resize(n);
        for (int i = 0; i < n; ++i) encode_record(names[i], nullptr, 0, c->recs[i]);
        stage_genome(c, d_bases, lens);
    });
}
// `scssim simuvars` (src/scssim.cpp:33-38: Genome::loadData + Genome::saveSequence) on the data plane
int scs_simuvars(scs_ctx* c, const char* ref_fasta, const char* snp_file, const char* var_file, const char* out_fasta) {
    return guarded(c, [&] {
        if (!ref_fasta) throw ScsError(SCS_EINVAL, "reference sequence file not specified!");
        hipStream_t s = c->stream;
        std::vector<FastaRecord> ref; load_fasta(ref_fasta, ref, true);                // Genome::loadRefSeq (Genome.cpp:176-195): index names, .fai beside the file
        if (c->cfg.verbose) fprintf(stderr, "\nReference sequence was loaded from file %s\n", ref_fasta);
        std::vector<SvChrom> chroms; uint64_t rtot = 0;
        for (auto& r : ref) { chroms.push_back(SvChrom{r.name, rtot, (uint64_t)r.code.size()}); rtot += r.code.size(); }
        DevBuf d_ref, d_lit, d_pc, d_sb;
        d_ref.reserve(std::max<uint64_t>(rtot, 16), s);
        for (size_t i = 0; i < ref.size(); ++i) if (!ref[i].code.empty()) HIP_OK(hipMemcpyAsync((uint8_t*)d_ref.p + chroms[i].off, ref[i].code.data(), ref[i].code.size(), hipMemcpyHostToDevice, s));
        SvPlan P;
        try { simuvars_plan(chroms, snp_file ? snp_file : "", var_file ? var_file : "", c->cfg.verbose != 0, P); }
        catch (const std::exception& e) { HIP_OK(hipStreamSynchronize(s)); throw ScsError(SCS_EIO, e.what()); }
        if (P.pieces.size() > 0xFFFFFFF0ull || P.substs.size() > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, "simuvars: too many edits");
        upload(d_pc, P.pieces, s); upload(d_sb, P.substs, s);
        d_lit.reserve(std::max<size_t>(P.literals.size(), 16), s);
        if (!P.literals.empty()) HIP_OK(hipMemcpyAsync(d_lit.p, P.literals.data(), P.literals.size(), hipMemcpyHostToDevice, s));
        c->genome.reserve(std::max<uint64_t>(P.total, 16), s);
        launch_sv_build(s, d_ref.as<uint8_t>(), d_lit.as<uint8_t>(), d_pc.as<SvPiece>(), (uint32_t)P.pieces.size(), d_sb.as<SvSubst>(), (uint32_t)P.substs.size(), c->genome.as<uint8_t>(), P.total);
        HIP_OK(hipStreamSynchronize(s));                                                 // the host vectors behind the uploads may go
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("simuvars kernel launch failed: ") + hipGetErrorString(le)); }
        if (out_fasta && *out_fasta) {                                                   // Genome::saveSequence's file: >chr_hap_len, 100 columns (Genome.cpp:365-381)
            FILE* o = fopen(out_fasta, "w");
            if (!o) throw ScsError(SCS_EIO, std::string("can not open file ") + out_fasta);
            const size_t chunk = 64u << 20; Pinned<char> hb; hb.reserve(chunk, hipHostMallocDefault);
            std::vector<char> line_buf; uint64_t off = 0; bool okw = true;
            for (size_t r = 0; r < P.rec_names.size() && okw; ++r) {
                okw = fprintf(o, ">%s\n", P.rec_names[r].c_str()) > 0;
                uint64_t col = 0;
                for (uint64_t done = 0; done < P.rec_lens[r] && okw; done += chunk) {
                    const size_t n = (size_t)std::min<uint64_t>(chunk, P.rec_lens[r] - done);
                    HIP_OK(hipMemcpyAsync(hb, (uint8_t*)c->genome.p + off + done, n, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
                    line_buf.clear(); line_buf.reserve(n + n / 100 + 2);
                    for (size_t i = 0; i < n;) { const size_t take = (size_t)std::min<uint64_t>(100 - col, n - i); line_buf.insert(line_buf.end(), hb + i, hb + i + take); i += take; col += take; if (col == 100) { line_buf.push_back('\n'); col = 0; } }
                    okw = fwrite(line_buf.data(), 1, line_buf.size(), o) == line_buf.size();
                }
                if (col && okw) okw = fputc('\n', o) != EOF;
                off += P.rec_lens[r];
            }
            if (fclose(o) != 0 || !okw) throw ScsError(SCS_EIO, std::string("writing ") + out_fasta + " failed");
        }
        c->recs.resize(P.rec_names.size());
        for (size_t i = 0; i < P.rec_names.size(); ++i) encode_record(P.rec_names[i].c_str(), nullptr, 0, c->recs[i]);
        stage_genome(c, c->genome.p, P.rec_lens.data());                                 // encode + bit index in place: ready for scs_create_frags
        LiftTable T; std::string why;                                                    // the plan's map to the reference stays with the genome it built
        if (!lift_from_plan(chroms, P, T, why)) throw ScsError(SCS_EDEVICE, why);
        lift_install(c, std::move(T));
    });
}
int scs_create_frags(scs_ctx* c) { return guarded(c, [&] { double t = now_s(); do_create_frags(c); c->st.t_stage[1] = now_s() - t; }); }
int scs_amplify(scs_ctx* c) { return guarded(c, [&] { double t = now_s(); do_amplify(c); c->st.t_stage[2] = now_s() - t; }); }
int scs_allocate_reads(scs_ctx* c, uint64_t reads) { return guarded(c, [&] { do_allocate(c, reads); }); }
static int discard_sink(void*, const char*, size_t, const char*, size_t) { return 0; }
int scs_yield_reads(scs_ctx* c, scs_sink_fn sink, void* user) {
    return guarded(c, [&] {
        truth_check(c, false, 1); depth_check(c); support_check(c); coverage_check(c);
        // with truth on, a NULL sink still takes the sink path: the SAM needs its writer; the FASTQ text stays on the device
        double t = now_s(); CallbackSink cb(sink ? sink : discard_sink, user);
        OutTarget tg{false, nullptr, nullptr, 0, 0, (sink || !c->truth_path.empty()) ? &cb : nullptr}; tg.discard = !sink;
        do_yield(c, tg, nullptr, nullptr, nullptr); c->st.t_stage[5] = now_s() - t;
    });
}
int scs_yield_reads_device(scs_ctx* c, void* d1, size_t cap1, void* d2, size_t cap2, uint64_t* n1, uint64_t* n2, uint64_t* pairs) {
    return guarded(c, [&] {
        if (!d1 || (c->cfg.paired && !d2)) throw ScsError(SCS_EINVAL, "scs_yield_reads_device: null output buffer");
        truth_check(c, true, 1); depth_check(c); support_check(c); coverage_check(c);
        double t = now_s(); OutTarget tg{true, (char*)d1, (char*)d2, cap1, cap2, nullptr}; do_yield(c, tg, n1, n2, pairs); c->st.t_stage[5] = now_s() - t;
    });
}
// SeqWriter (lib/seqwriter/SeqWriter.cpp:12-64).  writers <= 1: the reference's files <prefix>_1.fq / _2.fq (.fq) -- a shard of a
// sharded job: <prefix>.r<rank>_1.fq ... + <prefix>.r<rank>.idx.  writers = K > 1: K part files per mate, each a contiguous
// range of the job's (shard's) records written by its own thread, + <base>.parts (scs_comm.h: FastqParts).
int scs_yield_reads_files_ex(scs_ctx* c, const char* prefix, int writers, int generations, int flags) {
    const int bgzf = flags & SCS_SINK_BGZF; const bool in_place = (flags & SCS_SINK_IN_PLACE) != 0;
    return guarded(c, [&] {
        if (flags & ~(SCS_SINK_BGZF | SCS_SINK_IN_PLACE)) throw ScsError(SCS_EINVAL, "scs_yield_reads_files: unknown sink flag");
        if (!prefix || !*prefix) throw ScsError(SCS_EINVAL, "scs_yield_reads_files: no output prefix");
        if (writers > 64 || generations > 64 || (int64_t)std::max(1, writers) * std::max(1, generations) > 99) throw ScsError(SCS_EINVAL, "scs_yield_reads_files: at most 64 writers and 99 parts");
        truth_check(c, false, writers); depth_check(c); support_check(c); coverage_check(c);
        const bool pe = c->cfg.paired != 0, shard = c->cfg.shard_count > 1; const std::string pre = prefix;
        const std::string base = shard ? shard_base(pre, c->cfg.shard_rank) : pre;
        FastqParts files; std::string err;
        if (!files.open(base, pe, std::max(1, writers), std::max(1, generations), bgzf ? ".fq.gz" : ".fq", bgzf != 0, err, in_place)) throw ScsError(SCS_EIO, err);
        std::vector<uint64_t> so1, so2;
        double t = now_s(); OutTarget tg{false, nullptr, nullptr, 0, 0, &files}; tg.bgzf = bgzf != 0;
        if (shard && !bgzf) { tg.seg_off1 = &so1; tg.seg_off2 = &so2; }              // (byte ranges of compressed shards cannot be spliced: BGZF shards stay shards)
        do_yield(c, tg, nullptr, nullptr, nullptr);
        if (!files.close(err)) throw ScsError(SCS_EIO, err);
        if (shard && !bgzf && !write_shard_index(shard_index_path(pre, c->cfg.shard_rank), so1, so2, err)) throw ScsError(SCS_EIO, err);
        c->st.t_stage[5] = now_s() - t;
    });
}
int scs_yield_reads_files(scs_ctx* c, const char* prefix, int writers) { return scs_yield_reads_files_ex(c, prefix, writers, 1, 0); }
int scs_merge_fastq_parts(const char* prefix, int paired, int keep_parts, char* errbuf, size_t errlen) {
    if (!prefix) return SCS_EINVAL;
    std::string err;
    if (merge_parts(prefix, paired != 0, ".fq", keep_parts != 0, err)) return SCS_OK;
    copy_err(errbuf, errlen, err.c_str());
    return SCS_EIO;
}
int scs_merge_fastq_shards(const char* prefix, int nranks, int paired, int keep_shards, char* errbuf, size_t errlen) {
    if (!prefix) return SCS_EINVAL;
    std::string err;
    if (merge_shards(prefix, nranks, paired != 0, keep_shards != 0, err)) return SCS_OK;
    copy_err(errbuf, errlen, err.c_str());
    return SCS_EIO;
}
int scs_comm_unique_id(void* id_out) {
    std::string err;
    if (!id_out) return SCS_EINVAL;
    if (rccl_unique_id(id_out, err)) { create_error() = err; return SCS_EDEVICE; }
    return SCS_OK;
}
static int rccl_allreduce_hook(void* user, void* d_vals, uint64_t n, int elem_bytes) {
    scs_ctx* c = (scs_ctx*)user; std::string err;
    if (rccl_allreduce_sum(c->rccl.get(), d_vals, n, elem_bytes, c->stream, err)) { c->err = err; return 1; }
    return 0;
}
static int rccl_allgather_hook(void* user, const void* d_send, void* d_recv, uint64_t bytes) {
    scs_ctx* c = (scs_ctx*)user; std::string err;
    if (rccl_allgather(c->rccl.get(), d_send, d_recv, bytes, c->stream, err)) { c->err = err; return 1; }
    return 0;
}
int scs_comm_init(scs_ctx* c, const void* id, int rank, int nranks) {
    return guarded(c, [&] {
        if (!id || nranks < 1 || rank < 0 || rank >= nranks) throw ScsError(SCS_EINVAL, "scs_comm_init: bad arguments");
        if (rank != c->cfg.shard_rank || nranks != c->cfg.shard_count) throw ScsError(SCS_EINVAL, "scs_comm_init: rank / size differ from the ctx's shard_rank / shard_count");
        c->rccl.reset();
        std::string err;
        c->rccl.reset(rccl_init(id, rank, nranks, err));
        if (!c->rccl) throw ScsError(SCS_EDEVICE, err);
        c->allreduce_dev = rccl_allreduce_hook; c->allgather_dev = rccl_allgather_hook; c->coll_dev_user = c;
    });
}
int scs_comm_count(const scs_ctx* c) { return c && c->rccl ? rccl_count(c->rccl.get()) : 0; }
int scs_comm_abort(scs_ctx* c) { if (!c) return SCS_EINVAL; if (c->rccl) rccl_abort(c->rccl.get()); return SCS_OK; }
int scs_run_genreads(scs_ctx* c, scs_sink_fn sink, void* user) {
    int rc; double t = now_s();
    if ((rc = scs_create_frags(c))) return rc;
    if ((rc = scs_amplify(c))) return rc;
    if ((rc = scs_allocate_reads(c, 0))) return rc;
    if ((rc = scs_yield_reads(c, sink, user))) return rc;
    c->st.t_stage[7] = now_s() - t; return SCS_OK;
}
int scs_set_collectives(scs_ctx* c, scs_allreduce_fn ar, scs_allgatherv_fn ag, void* user) {
    if (!c) return SCS_EINVAL;
    c->allreduce = ar; c->allgatherv = ag; c->coll_user = user; return SCS_OK;
}
int scs_set_collectives_device(scs_ctx* c, scs_allreduce_dev_fn ar, scs_allgather_dev_fn ag, void* user) {
    if (!c) return SCS_EINVAL;
    c->allreduce_dev = ar; c->allgather_dev = ag; c->coll_dev_user = user; return SCS_OK;
}
int scs_set_batch_checksums(scs_ctx* c, int on) { if (!c) return SCS_EINVAL; c->want_cks = on != 0; return SCS_OK; }
int scs_batch_checksums(const scs_ctx* c, uint64_t* out, size_t cap, size_t* n_batches) {
    if (!c || !n_batches) return SCS_EINVAL;
    *n_batches = c->cks.size() / 2;
    if (out) memcpy(out, c->cks.data(), std::min(cap, c->cks.size()) * 8);
    return SCS_OK;
}
int scs_get_stats(const scs_ctx* c, scs_stats* out) { if (!c || !out) return SCS_EINVAL; *out = c->st; return SCS_OK; }

// one truth output per ctx: truth_path is the SAM's, (truth_bam) the BAM's or (truth_ref) the reference SAM's; NULL clears only the caller's own
static int set_truth(scs_ctx* c, const char* path, int kind) {
    static const char* const fn[3] = {"scs_set_truth_sam", "scs_set_truth_bam", "scs_set_truth_ref_sam"};
    static const char* const what[3] = {"truth SAM", "truth BAM", "truth SAM on the reference"};
    if (!c) return SCS_EINVAL;
    const bool on = !c->truth_path.empty(); const int cur = c->truth_bam ? 1 : c->truth_ref ? 2 : 0;
    if (path && on && cur != kind) {
        c->err = std::string(fn[kind]) + ": the " + what[cur] + " is on (" + fn[cur] + "); one truth output per ctx: clear it with " + fn[cur] + "(ctx, NULL) first";
        return SCS_EINVAL;
    }
    if (path) { c->truth_path = path; c->truth_bam = kind == 1; c->truth_ref = kind == 2; }
    else if (!on || cur == kind) {
        if (c->truth_ref) truth_ref_release(c);
        c->truth_path.clear(); c->truth_bam = false; c->truth_ref = false;
    }
    return SCS_OK;
}
int scs_set_truth_sam(scs_ctx* c, const char* path) { return set_truth(c, path, 0); }
int scs_set_truth_bam(scs_ctx* c, const char* path) { return set_truth(c, path, 1); }
int scs_set_truth_ref_sam(scs_ctx* c, const char* path) { return set_truth(c, path, 2); }
int scs_truth_bytes(const scs_ctx* c, uint64_t* bytes) { if (!c || !bytes) return SCS_EINVAL; *bytes = c->truth_bytes; return SCS_OK; }
int scs_download_frags(scs_ctx* c, uint64_t* goff, uint32_t* len, int8_t* strand) {
    return guarded(c, [&] {
        if (!c->have_frags) throw ScsError(SCS_EINVAL, "scs_download_frags: call scs_create_frags first");
        const size_t n = c->f_len.size();
        if (goff && n) memcpy(goff, c->f_goff.data(), n * 8);
        if (len && n) memcpy(len, c->f_len.data(), n * 4);
        if (strand && n) memcpy(strand, c->f_strand.data(), n);
    });
}

int scs_kernel_time(const scs_ctx* c, int which, const char** name, uint64_t* launches, double* ms, uint64_t* units) {
    if (!c || which < 0 || which >= TM_COUNT) return SCS_EINVAL;
    const KernelTimer& t = c->tm[which];
    if (name) *name = t.name; if (launches) *launches = t.launches; if (ms) *ms = t.ms; if (units) *units = t.units;
    return SCS_OK;
}

int scs_set_kernel_timing(scs_ctx* c, unsigned mask, unsigned every) {
    if (!c || every == 0) return SCS_EINVAL;
    for (int i = 0; i < TM_COUNT; ++i) c->tm[i].on = (mask >> i) & 1u;
    c->timing_every = every; c->amplify_calls = 0; c->yield_calls = 0;
    return SCS_OK;
}

int scs_download_amplicons(scs_ctx* c, int kind, uint32_t* parent, uint32_t* spos, uint32_t* len, uint32_t* gc, uint32_t* primers, uint64_t* uid,
                           uint32_t* errs, uint32_t* nerr) {
    return guarded(c, [&] {
        if (!c->amplified) throw ScsError(SCS_EINVAL, "scs_download_amplicons: call scs_amplify first");
        AmpStore& A = kind == 0 ? c->semis : c->fulls; const uint32_t n = A.n; hipStream_t s = c->stream; DevAmps v = A.view();
        std::vector<uint32_t> hsl(n), hp(n); std::vector<uint16_t> hgc(n), hpr(n); std::vector<uint64_t> hu(n), he(n);
        if (n) {
            HIP_OK(hipMemcpyAsync(hp.data(), v.parent, (size_t)n * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipMemcpyAsync(hsl.data(), v.sl, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(hgc.data(), v.gc, (size_t)n * 2, hipMemcpyDeviceToHost, s)); HIP_OK(hipMemcpyAsync(hpr.data(), v.primers, (size_t)n * 2, hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(hu.data(), v.uid, (size_t)n * 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipMemcpyAsync(he.data(), v.errs, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        }
        uint32_t used = 0; HIP_OK(hipMemcpyAsync(&used, A.pool_head.p, 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        std::vector<uint32_t> pool(std::min(used, A.pool_cap));
        if (!pool.empty()) { HIP_OK(hipMemcpyAsync(pool.data(), A.pool.p, pool.size() * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s)); }
        for (uint32_t i = 0; i < n; ++i) {
            if (parent) parent[i] = hp[i]; if (spos) spos[i] = sl_spos(hsl[i]); if (len) len[i] = sl_len(hsl[i]); if (gc) gc[i] = hgc[i];
            if (primers) primers[i] = hpr[i]; if (uid) uid[i] = hu[i];
            uint32_t cnt = 0; uint32_t e4[4] = {0, 0, 0, 0};
            if (he[i] & ERR_OVERFLOW_BIT) { const uint32_t off = (uint32_t)he[i]; cnt = (uint32_t)(he[i] >> 32) & 0xFFFF; for (uint32_t k = 0; k < std::min(cnt, 4u); ++k) { uint32_t e = pool[off + k]; e4[k] = (err_pos(e) << 3) | err_alt(e); } }
            else for (int k = 0; k < 4; ++k) { uint32_t e = (uint32_t)(he[i] >> (16 * k)) & 0xFFFF; if (e) e4[cnt++] = (err_pos(e) << 3) | err_alt(e); }
            if (errs) memcpy(errs + 4 * (size_t)i, e4, 16); if (nerr) nerr[i] = cnt;
        }
    });
}
int scs_gpu_local_cpus(int device, int* cpus, int cap) {
    try { const std::vector<int> v = gpu_local_cpus(device); for (int i = 0; i < (int)v.size() && i < cap && cpus; ++i) cpus[i] = v[(size_t)i]; return (int)v.size(); } catch (...) { return 0; }
}
const char* scs_test_seam(const char* name) { return name ? seam_env(name) : nullptr; }
int scs_download_primer_stock(scs_ctx* c, int64_t* stock) {
    return guarded(c, [&] {
        if (!stock) throw ScsError(SCS_EINVAL, "null pointer");
        if (!c->amplified) throw ScsError(SCS_EINVAL, "scs_download_primer_stock: call scs_amplify first");
        HIP_OK(hipMemcpyAsync(stock, c->primer_cnt.p, 65536 * 8, hipMemcpyDeviceToHost, c->stream)); HIP_OK(hipStreamSynchronize(c->stream));
    });
}
int scs_download_read_numbers(scs_ctx* c, uint32_t* rn) {
    return guarded(c, [&] {
        if (!c->allocated) throw ScsError(SCS_EINVAL, "call scs_allocate_reads first");
        if (c->fulls.n) HIP_OK(hipMemcpyAsync(rn, c->read_numbers.p, (size_t)c->fulls.n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    });
}

int scs_fasta_write_index(const char* path, char* errbuf, size_t errlen) {
    if (!path) return SCS_EINVAL;
    std::vector<FastaRecord> recs;
    try { load_fasta(path, recs, true); }
    catch (const std::exception& e) { copy_err(errbuf, errlen, e.what()); return SCS_EIO; }
    return SCS_OK;
}

}  // extern "C"


