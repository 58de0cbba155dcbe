// scs_ctx.h -- private to the library's host side: the context behind the C ABI's opaque scs_ctx, its device buffers, and the
// functions the host files share (scs_pipeline.cpp: mailbox, C ABI; scs_stage.cpp: profile, genome, fragments; scs_amplify.cpp:
// Malbac::amplify; scs_reads.cpp: read allocation, yieldReads; scs_sink.cpp: the FASTQ sink).
#pragma once
#include "../../include/scssim_hip.h"
#include <sched.h>
#include <pthread.h>
#include "scs_device.h"
#include "scs_seams.h"
#include "scs_tables.h"
#include "scs_comm.h"
#include "scs_bgzf.h"
#include "scs_truth.h"
#include "scs_depth.h"
#include "scs_coverage.h"
#include "scs_runs.h"
#include "scs_lift.h"
#include "scs_outfile.h"

#include <atomic>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

namespace scs {

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    throw ScsError(SCS_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what the owning handles below hold at this moment, process-wide (scs_live_resources: the tests' leak check); relaxed: it orders nothing
struct Census { std::atomic<uint64_t> dev_bytes{0}, streams{0}, events{0}, pinned_bytes{0}; };
inline Census& census() { static Census c; return c; }
inline void census_add(std::atomic<uint64_t>& a, uint64_t d) { a.fetch_add(d, std::memory_order_relaxed); }   // (d = -n: n fewer)
struct LiveBytes {           // DevBuf's capacity: a size_t whose every change is also made to census().dev_bytes
    size_t v = 0;
    operator size_t() const { return v; }
    LiveBytes& operator=(size_t n) { census_add(census().dev_bytes, (uint64_t)n - v); v = n; return *this; }
    LiveBytes& operator+=(size_t n) { return *this = v + n; }
};

// growable device buffer, freed by its destructor.  Small buffers are plain hipMalloc blocks.  A buffer that grows past 64 MB moves (once) into
// a reserved virtual address range and from then on grows IN PLACE by mapping more physical memory behind it
// (hipMemAddressReserve / hipMemCreate / hipMemMap): no reallocate-copy-free cycles while the amplicon arrays of a
// whole-genome job grow cycle by cycle, no transient 2.5x footprint -- and fresh hipMalloc memory costs about 20 ms per
// GB on its first touch on this platform (measured), mapped chunks do not.
struct DevBuf {
    void* p = nullptr; LiveBytes cap;        // cap: usable (mapped) bytes
    DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete; ~DevBuf() { release(); }
    size_t va = 0;                           // reserved address range in bytes (0: plain hipMalloc block)
    bool plain = false;                      // true: always a plain hipMalloc block, whatever its size (an array of a fixed size has no use for growing in place)
    // equal-sized chunks: on ROCm 7.2 hipMemSetAccess rejects a chunk mapped right behind one of a different size (probed)
    static constexpr size_t kRange = 384ull << 30, kGran = 128ull << 20;
    static size_t virtual_from() {           // SCS_VMM_FROM_MB: tests lower it so that small jobs run on mapped buffers too
        static const size_t v = seam_env("SCS_VMM_FROM_MB") ? (size_t)atol(seam_env("SCS_VMM_FROM_MB")) << 20 : 64ull << 20;
        return v;
    }
    static bool& virtual_ok() { static bool ok = seam_env("SCS_NO_VMM") == nullptr; return ok; }
    void map_more(size_t ncap) {             // map [cap, ncap) of the reserved range, kGran at a time
        int dev = 0; HIP_OK(hipGetDevice(&dev));
        hipMemAllocationProp prop = {}; prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = dev;
        hipMemAccessDesc acc = {}; acc.location.type = hipMemLocationTypeDevice; acc.location.id = dev; acc.flags = hipMemAccessFlagsProtReadWrite;
        while (cap < ncap) {
            hipMemGenericAllocationHandle_t h;
            HIP_OK(hipMemCreate(&h, kGran, &prop, 0));
            hipError_t e = hipMemMap((char*)p + cap, kGran, 0, h, 0);
            if (e == hipSuccess) { e = hipMemSetAccess((char*)p + cap, kGran, &acc, 1); if (e != hipSuccess) (void)hipMemUnmap((char*)p + cap, kGran); }
            (void)hipMemRelease(h);          // the mapping keeps the memory alive
            if (e != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("device memory map: ") + hipGetErrorString(e));
            cap += kGran;
        }
    }
    void reserve(size_t bytes, hipStream_t s, size_t keep_bytes = 0) {
        if (bytes <= cap) return;
        // a mapped buffer grows in place, chunk by chunk: it takes what is asked for plus 3 % (growing it by half, as a block that
        // must be copied is, mapped tens of GB in the middle of a job whose amplicon count came out 0.01 % above the last one's)
        size_t ncap = va ? bytes + bytes / 32 : std::max(bytes, cap + cap / 2);
        if (va) { map_more(std::min((ncap + kGran - 1) / kGran * kGran, va)); if (bytes > cap) throw ScsError(SCS_EOVERFLOW, "device buffer larger than its address range"); return; }
        if (!plain && ncap > virtual_from() && virtual_ok()) {
            void* base = nullptr;
            if (hipMemAddressReserve(&base, kRange, kGran, nullptr, 0) == hipSuccess) {
                void* old = p; const size_t old_cap = cap;
                p = base; cap = 0; va = kRange;
                try { map_more((ncap + kGran - 1) / kGran * kGran); }
                catch (...) { (void)hipMemAddressFree(base, kRange); p = old; cap = old_cap; va = 0; throw; }
                if (old && keep_bytes) { HIP_OK(hipMemcpyAsync(p, old, keep_bytes, hipMemcpyDeviceToDevice, s)); HIP_OK(hipStreamSynchronize(s)); }
                if (old) HIP_OK(hipFree(old));
                return;
            }
            (void)hipGetLastError(); virtual_ok() = false;                        // no virtual memory management here: classic path from now on
        }
        void* np = nullptr;
        HIP_OK(hipMalloc(&np, ncap));
        if (p && keep_bytes) { HIP_OK(hipMemcpyAsync(np, p, keep_bytes, hipMemcpyDeviceToDevice, s)); HIP_OK(hipStreamSynchronize(s)); }
        if (p) HIP_OK(hipFree(p));
        p = np; cap = ncap;
    }
    void release() {
        if (p && va) { for (size_t o = 0; o < cap; o += kGran) (void)hipMemUnmap((char*)p + o, kGran); (void)hipMemAddressFree(p, va); }
        else if (p) (void)hipFree(p);
        p = nullptr; cap = 0; va = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

// The other device-side resources, owned the same way: made by ensure() / reserve() where they are first needed (a second call
// is a no-op), usable wherever the raw handle is, destroyed with their owner when they were made.
struct Stream {
    hipStream_t s = nullptr; bool owned = false;
    Stream() = default; Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s && owned) { (void)hipStreamDestroy(s); census_add(census().streams, -1); } }
    void ensure(unsigned flags) { if (s) return; HIP_OK(hipStreamCreateWithFlags(&s, flags)); owned = true; census_add(census().streams, 1); }
    void adopt(hipStream_t theirs) { s = theirs; owned = false; }                // the caller's stream (cfg->stream): used, never destroyed
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default; Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }         // (movable, for vectors of them; not copyable)
    ~Event() { release(); }
    void ensure(unsigned flags) { if (e) return; HIP_OK(hipEventCreateWithFlags(&e, flags)); census_add(census().events, 1); }
    void release() { if (e) { (void)hipEventDestroy(e); census_add(census().events, -1); } e = nullptr; }
    operator hipEvent_t() const { return e; }
};
template <class T> struct Pinned {                                               // a pinned host block of T
    T* p = nullptr; size_t bytes = 0;
    Pinned() = default; Pinned(Pinned&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~Pinned() { release(); }
    void reserve(size_t need, unsigned flags, size_t alloc = 0) {                // at least `need` bytes; a block that must grow is made max(alloc, need) large, its contents are lost
        if (need <= bytes) return;
        release(); alloc = std::max(alloc, need);
        HIP_OK(hipHostMalloc((void**)&p, alloc, flags)); bytes = alloc; census_add(census().pinned_bytes, bytes);
    }
    void release() { if (p) { (void)hipHostFree(p); census_add(census().pinned_bytes, -(uint64_t)bytes); } p = nullptr; bytes = 0; }
    operator T*() const { return p; }
};
// BGZF made on the device over one byte stream (scs_bgzf.hip; bgzf_in_place, scs_textout.h): the blocks' plans / sizes / offsets and two
// output buffers, for the users that make one batch's blocks while the last one's cross to the host
struct BgzfLane { DevBuf plan, sizes, offs, out[2]; };
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf owns its memory");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Pinned<char>>::value, "the handles own what they hold");

struct AmpStore {            // SoA amplicon arrays (DevAmps) with capacity management
    DevBuf parent, sl, gc, primers, uid, errs; uint32_t n = 0, cap = 0;
    DevBuf pool, pool_head; uint32_t pool_cap = 0;
    void reserve(uint64_t want, hipStream_t s) {
        if (want > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, "amplicon count exceeds 2^32 (reference limit: Malbac.cpp:376,386)");
        if (want <= cap) return;
        uint64_t ncap = uid.va ? want + want / 32 : std::max<uint64_t>(want, (uint64_t)cap + cap / 2);   // (mapped arrays grow in place: see DevBuf::reserve)
        ncap = std::min<uint64_t>(std::max<uint64_t>(ncap, 1u << 16), 0xFFFFFFF0ull);
        parent.reserve(ncap * 4, s, (size_t)n * 4); sl.reserve(ncap * 4, s, (size_t)n * 4);
        gc.reserve(ncap * 2, s, (size_t)n * 2); primers.reserve(ncap * 2, s, (size_t)n * 2);
        uid.reserve(ncap * 8, s, (size_t)n * 8); errs.reserve(ncap * 8, s, (size_t)n * 8);
        cap = (uint32_t)ncap;
    }
    void reserve_pool(uint32_t entries, hipStream_t s) {
        if (!pool_head.p) { pool_head.reserve(256, s); HIP_OK(hipMemsetAsync(pool_head.p, 0, 4, s)); }
        if (entries > pool_cap) {
            uint32_t used = 0;
            if (pool_cap) { HIP_OK(hipMemcpyAsync(&used, pool_head.p, 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s)); used = std::min(used, pool_cap); }
            pool.reserve((size_t)entries * 4, s, (size_t)used * 4); pool_cap = entries;
        }
    }
    DevAmps view() const { return DevAmps{parent.as<uint32_t>(), sl.as<uint32_t>(), gc.as<uint16_t>(), primers.as<uint16_t>(), uid.as<uint64_t>(), errs.as<uint64_t>()}; }
    DevErrPool pool_view() const { return DevErrPool{pool.as<uint32_t>(), pool_head.as<uint32_t>(), pool_cap}; }
    void reset(hipStream_t s) { n = 0; if (pool_head.p) HIP_OK(hipMemsetAsync(pool_head.p, 0, 4, s)); }
    void reset_counts() { n = 0; }                                                // the pool head is zeroed by k_amplify_init
};                           // (its DevBufs free themselves: not copyable, nothing to release by hand)

static const bool kAlwaysTimed = true;
struct KernelTimer {         // HIP events on the ctx stream around the launches of one kernel (scs_set_kernel_timing turns one off)
    const char* name; std::vector<std::pair<Event, Event>> ev; size_t used = 0; double ms = 0; uint64_t launches = 0; uint64_t units = 0; bool on = true; const bool* gate = &kAlwaysTimed;
    void add_units(uint64_t n) { if (on && *gate) units += n; }
    void begin(hipStream_t s) {
        if (!on || !*gate) return;
        if (used == ev.size()) { std::pair<Event, Event> p; p.first.ensure(hipEventDefault); p.second.ensure(hipEventDefault); ev.push_back(std::move(p)); }
        HIP_OK(hipEventRecord(ev[used].first, s));
    }
    void end(hipStream_t s) { if (!on || !*gate) return; HIP_OK(hipEventRecord(ev[used].second, s)); ++used; }
    void collect() {         // call after a stream sync
        for (size_t i = 0; i < used; ++i) { float t = 0; HIP_OK(hipEventElapsedTime(&t, ev[i].first, ev[i].second)); ms += t; ++launches; }
        used = 0;
    }
    void reset() { ms = 0; launches = 0; units = 0; used = 0; }
    void drop_events() { ev.clear(); used = 0; }         // a call's open events go (a failed wait); the sums stay
    void drop() { drop_events(); reset(); }              // what the timer's feature made goes with the feature
};
// One depth track of a ctx: the bin width (0: off -- no buffer of it exists, no code of it runs), the bins of its records, the
// counters of the last yield call (planes of `bins` entries, zeroed on the ctx stream at the start of every call; valid: a call with
// the track on has finished) and the kernel's tables
struct DepthTrack { uint32_t width = 0; uint64_t bins = 0; bool valid = false; DevBuf cnt, tab; };
// The coverage profile of a ctx (scs_set_coverage; scs_coverage.cpp): max_depth (0: off); the difference array of the running
// yield call, the per-base depths once it has finished (bases + 1 int32, padded to whole tiles; valid: a call with it on has
// finished); the last call's tables (CovTab's layout), the kernels' record starts and tile sums; run_depth: the max_depth the
// last end-of-job pass ran with (1: tables kept private for the profile on the reference).  Which switch owns which buffer of
// this struct and the three below: coverage_settle (scs_coverage.cpp)
struct CovTrack { uint32_t max_depth = 0, n_rec = 0, run_depth = 0; uint64_t bases = 0; bool valid = false; DevBuf diff, tab, rec, tiles; };
// The coverage profile on the reference (scs_set_coverage_ref; scs_coverage.cpp): per reference base of
// the lift table the last call's depth (uint32, padded to whole tiles) and the packed copies | n_copies << 16 (made once per
// genome and table: `copies` says that they stand); the last call's tables (CovTab's layout), the reference record starts and
// unlifted (the two per-base arrays are plain blocks: their size is the reference's, they never grow)
struct CovRefTrack { uint32_t max_depth = 0, n_ref = 0; uint64_t bases = 0, unlifted = 0; bool valid = false, copies = false; DevBuf depth, packed, tab, rec; CovRefTrack() { depth.plain = packed.plain = true; } };
// What the bedGraph writer of the per-base arrays keeps (scs_write_coverage_bedgraph ...; scs_runs.cpp): per
// tile the first run start, the next one behind it, lines and bytes; a slab's 64-bit offsets, the scan's scratch, its text (at
// most the text cap, whatever the genome's size), the BGZF lane over it and the pinned block it crosses to the host through.  Made
// by the first write call, kept for the next one, released by a change of either coverage switch (coverage_settle)
struct RunsWork {
    DevBuf first, next, lines, bytes, offs, scan, text, crc; BgzfLane z; Pinned<char> h_text; Pinned<uint32_t> h_n;
    void release() { for (DevBuf* b : {&first, &next, &lines, &bytes, &offs, &scan, &text, &crc, &z.plan, &z.sizes, &z.offs, &z.out[0], &z.out[1]}) b->release(); h_text.release(); h_n.release(); }
};
// The GC-bias table's buffer (scs_gc_bias, scs_write_gc_bias; scs_gcbias.cpp): windows and depth_sum, rows
// of 101 per staged record, and n_windows, all uint64.  Made by the first call, zeroed by every call (coverage_settle,
// coverage_invalidate)
struct GcBiasWork { DevBuf tab; void release() { tab.release(); } };
enum { TM_ERRSCAN,TM_ERRSCAN_F, TM_READS, TM_ATTACH, TM_INDELS, TM_ATTACH_F, TM_TRUTH, TM_DEPTH, TM_COUNT };   // a ctx's timers, in the order scs_kernel_time(which) documents

struct SinkPipe;             // scs_sink.h
struct SinkPipeDelete { void operator()(SinkPipe* p) const; };
struct RcclDelete { void operator()(RcclComm* r) const { rccl_destroy(r); } };   // (skips ncclCommDestroy after scs_comm_abort)
}  // namespace scs
using namespace scs;

struct Mail {                // a batch of device scalars for one k_mail post (at most 16)
    const void* src[16]; int wd[16]; int dst[16]; int n = 0; unsigned clear = 0;
    void add(const void* p, int width, int slot, bool clear_after = false) { src[n] = p; wd[n] = width; dst[n] = slot; if (clear_after) clear |= 1u << n; ++n; }
};

// Every device-side resource below is an owning handle: `delete ctx` is the whole teardown.  Members are destroyed in REVERSE order
// of declaration, and three places rely on it: the ctx stream comes first (it goes last, after everything that was ever queued on
// it), the RCCL communicator right behind it (it goes just before the stream its collectives ran on), and the sink pipe last (it
// goes first, before the pinned blocks and events of the batches it shipped; its writers are joined at the end of every yield).
struct scs_ctx {
    Stream stream;                                                                 // cfg.stream adopted, or the ctx's own
    std::unique_ptr<RcclComm, RcclDelete> rccl;            // scs_comm_init: RCCL communicator of this shard (the device collectives then run on it)
    scs_config cfg; std::string err;
    RngKey key{0, 0};
    // model
    ProfileTables prof; bool have_profile = false; DevTables dtb{};
    DevBuf d_tables, t_gap, t_qcompact, t_guide, t_ring1, t_ring2, t_ring1u, t_ring2u, t_subs1, t_subs2, t_qual, t_ins, t_del, t_isize, d_subs1, d_subs2, d_qual, d_ins, d_del, d_isize, d_gcmeans;
    // genome + fragments
    DevBuf gx_gc_bits, gx_n_bits, gx_gc_cnt, gx_n_cnt, gx_gc_pref, gx_n_pref, gx_gc_pair, d_binom;
    std::vector<FastaRecord> recs; bool have_genome = false; DevBuf genome, genome2; std::vector<uint64_t> rec_off, rec_len; uint64_t genome_bases = 0;   // recs: names only once staged
    std::vector<uint64_t> f_goff; std::vector<uint32_t> f_len; std::vector<int8_t> f_strand; std::vector<uint32_t> f_primers;
    uint64_t f_gidx_base = 0; bool have_frags = false;
    uint64_t slice_base = 0, slice_len = 0; bool sliced = false;   // sharded job staged from a FASTA: only the bases of this shard's fragments are resident (genome coordinate slice_base ..)
    DevBuf df_blob, df_primers, df_hasn; size_t df_len_off = 0, df_strand_off = 0;           // fragments: offsets | lengths | strands in one block
    Pinned<uint8_t> h_frag; bool frag_copy_pending = false;                                  // its pinned staging copy
    // amplicons
    AmpStore semis, fulls;
    DevBuf budget_f, budget_s, slot_off_f, slot_off_s, dsums, poisson_part; Pinned<uint64_t> h_rb;   // dsums: device scalars; h_rb: pinned, device-mapped mailbox (32 words)
    unsigned long long* d_rb = nullptr; uint64_t mail_seq = 0;                      // device address of h_rb; sequence of the last post
    Mail pend;                                                                     // counts of the passes launched since the last collect
    bool timing_gate = true; uint32_t timing_every = 1; uint64_t amplify_calls = 0, yield_calls = 0;   // scs_set_kernel_timing: events on every n-th call
    uint64_t frag_total_len = 0, semi_total_len = 0; uint32_t slots_f = 0, slots_s = 0, budget_ns = 0;
    uint64_t nf_all = 0, frag_len_all = 0; bool budgets_pending = false;            // sharded job: fragments of ALL shards; budgets not yet exchanged
    DevBuf primer_cnt, primer_delta, primer_cut, primer_gdelta; uint64_t total_primers = 0; bool amplified = false;   // stock, what the running pass took (this shard / all shards), the cuts k_attach reads
    DevBuf st_eidx, st_etype, st_estart, st_info, st_list, st_sorted, st_tmp, att_wave_first; uint64_t min_stock_lb = 0;   // exact_stock's work arrays; lower bound of every primer stock in use
    DevBuf slots, slot_tmpl, valid, valid_off, valid_f, valid_off_f, scan_tmp, flags;
    // allocation + reads
    DevBuf weights, read_numbers, pair_off, pairs, odd_before, a_part, a_tp, a_probs, a_quota, a_poff, a_plan, a_crn, a_scratch, a_brow, a_bmap, a_send, a_gath, a_odd; SegMap gmap{}; std::vector<uint32_t> h_read_numbers; uint64_t reads_requested = 0, n_pairs_planned = 0; bool allocated = false;
    DevBuf slot_b, slot_q, lens, ev_hdr, ev_dat, sizes[2], off[2], out[2][2], rl_cls, rl_pos, rl_lists, d_bounds;   // sizes / off: per mate; out[slot][mate]: the FASTQ text (sink mode: two slots)
    Stream errs_stream; Event ev_att, ev_errs; bool errs_pending = false;   // k_errs<semi->full> of a cycle runs beside the fragment pass that follows it
    DevBuf slots_fr, slot_tmpl_fr;                        // the fragment passes' own slot arrays (the semi pass's are still being read then)
    // BGZF made on the device (scs_bgzf.hip): a lane per byte stream (z[0], z[1]: the mates' FASTQ text; z[2]: the truth BAM's records);
    // the CRC tables; the blocks' totals per batch reach the host through a small pinned array (h_z[slot][stream]) behind the slot's
    // event, the FASTQ blocks' one batch late (see do_yield)
    BgzfLane z[3]; DevBuf z_crc; Pinned<uint32_t> h_z; Event ev_z[2];
    bool want_cks = false; DevBuf d_cks; std::vector<uint64_t> cks;   // scs_set_batch_checksums: per batch and mate, computed where the text lies in HBM
    // truth SAM (scs_set_truth_sam): the path (empty: off), per batch the pairs' SAM sizes and 64-bit offsets, two output buffers (the
    // batch's text crosses PCIe on the copy stream while the next batch is made), the record table the kernels name records from,
    // and the batch's total, read back through a pinned word behind ev_t
    std::string truth_path; uint64_t truth_bytes = 0;
    DevBuf t_sizes, t_offs, t_scan, t_out[2], t_recs; Pinned<uint64_t> h_t; Event ev_t;
    // truth BAM (scs_set_truth_bam): truth_path names a BAM; t_out then holds the batch's binary records, which become BGZF blocks in
    // z[2].out; the blocks' total reaches the host through h_z[slot][2] behind ev_z[slot]
    bool truth_bam = false;
    // truth SAM on the original reference (scs_set_truth_ref_sam): truth_path names a SAM whose records are
    // lifted through the lift table (d_lift); t_refs: the reference records' lengths, name offsets and names as the kernels read them
    bool truth_ref = false; DevBuf t_refs;
    // depth track (scs_set_depth; scs_depth.cpp): counters reads[bins] then bases[bins]; tables rec_off[nr + 1] then bin_off[nr + 1]
    DepthTrack depth;
    // coverage profile (scs_set_coverage; scs_coverage.cpp)
    CovTrack cov;
    KernelTimer tm_cov_mark{"k_cov_mark"}, tm_cov_finish{"k_cov_finish"};   // the last yield call's per-batch marks and its end-of-job pass (scs_coverage_kernel_time; not of tm[])
    // the GC-bias table of cov's depths (scs_gcbias.cpp): made on demand after a yield call
    GcBiasWork gcb;
    KernelTimer tm_gcbias{"k_gc_bias"};                   // the last scs_gc_bias / scs_write_gc_bias call's kernel (scs_gc_bias_kernel_time; not one of tm[])
    // coverage profile on the reference (scs_set_coverage_ref; scs_coverage.cpp)
    CovRefTrack cov_ref;
    KernelTimer tm_cov_ref_copies{"k_cov_ref_copies"}, tm_cov_ref_finish{"k_cov_ref_finish"};   // the once-per-layout kernel and the end-of-job lift and count (scs_coverage_ref_kernel_time)
    // the bedGraph files of the three per-base arrays above (scs_runs.cpp)
    RunsWork runs;
    KernelTimer tm_runs{"k_runs"};                        // the last bedGraph write call's kernels (scs_coverage_bedgraph_kernel_time; not one of tm[])
    // lift table (scs_lift.cpp): the staged records as stretches of the original reference -- kept by scs_simuvars
    // or read by scs_load_lift, on the host and (d_lift: the segments) on the device; tied to the staged genome: staging another drops it.
    // Depth by reference bin (scs_set_depth_ref; scs_depth.cpp): the bins of the reference records; counters reads, bases, copies of
    // bins + 1 entries each (the pseudo-bin last), copies made once per layout (dref_copies), not per call; tables: the staged record
    // starts, the reference's lengths and first bins
    bool have_lift = false; LiftTable lift; DevBuf d_lift;
    DepthTrack depth_ref; bool dref_copies = false;
    KernelTimer tm_depth_ref{"k_depth_lift"};             // the last yield call's k_depth_lift launches (scs_depth_ref_kernel_time; not one of tm[])
    // amplicon table (scs_amplicon_places / scs_write_amplicons; scs_amplicons.cpp): every buffer, stream and event of a call belongs to
    // its AmpJob and goes with it; nothing of the call stays here but the kernels' times
    KernelTimer tm_amp{"k_amplicons"};                    // the last scs_write_amplicons call's kernels (scs_amplicon_kernel_time; not one of tm[])
    // site support (scs_set_site_support; scs_support.cpp): off -- no buffer below exists, no code of it runs.  The
    // last yield call's site table (the artefact table's sites at support_min_reads, packed in order), every site's position index, the
    // distinct positions (global genome indices, ascending), six uint32 counters per position (zeroed on the ctx stream at the start
    // of every call; support_valid: a call with it on has finished) and the kernel's record starts
    bool support_on = false, support_valid = false; uint32_t support_min_reads = 0; uint64_t sp_n_sites = 0, sp_n_pos = 0;
    DevBuf sp_sites, sp_site_pos, sp_pos, sp_cnt, sp_tab;
    // the same table on the original reference (scs_set_site_support_ref): support_on with support_ref.  The
    // sites are then the reference table's (rec = reference record), sp_site_pos indexes the distinct reference positions spr_x
    // (sp_n_x of them, six counters each in spr_cnt, summed after the last batch), and sp_pos / sp_cnt are the staged positions
    // that lift to them (sp_n_pos) and their counters, sp_pos_x every staged position's reference position; spr_tab: the
    // reference records' starts; sp_unlifted: the reference table's two unlifted totals (its header states them)
    bool support_ref = false; uint64_t sp_n_x = 0, sp_unlifted[2] = {0, 0};
    DevBuf spr_x, spr_cnt, sp_pos_x, spr_tab;
    KernelTimer tm_support_ref_open{"k_support_ref_open"}, tm_support_ref_gather{"k_support_ref_gather"};   // the last yield call's expansion (heads .. fill) and gather (scs_site_support_ref_step_time)
    KernelTimer tm_support{"k_support"};                  // the last yield call's k_support launches (scs_site_support_kernel_time; not one of tm[])
    KernelTimer tm_site{"k_sites"};                       // the last scs_write_artefacts call's kernels (scs_artefact_kernel_time); the call's buffers live and die with it (scs_sites.cpp)
    KernelTimer tm_site_ref{"k_sites_ref"};               // the last scs_write_artefacts_ref call's kernels (scs_artefact_ref_kernel_time); the call's buffers live and die with it (scs_sites.cpp)
    ReadsSide reads_side;                                 // k_reads' two small class kernels run beside the big one on these (per ctx: two contexts on one device do not share events)
    Stream pre_stream; Event ev_pre[2], ev_free[2], ev_plan;   // the reads stage's pre-pass on its own stream, beside the previous batch's base pass
    hipStream_t mail_stream = nullptr;                                             // the stream of the last post (mail_wait watches it)
    Stream copy_stream; Event ev_made[2], ev_d2h[2];   // sink mode: D2H on its own stream, behind the batch's k_reads
    // sharded single job: collectives supplied by the caller + segment bookkeeping of the local amplicon lists
    scs_allreduce_fn allreduce = nullptr; scs_allgatherv_fn allgatherv = nullptr; void* coll_user = nullptr;
    scs_allreduce_dev_fn allreduce_dev = nullptr; scs_allgather_dev_fn allgather_dev = nullptr; void* coll_dev_user = nullptr;
    DevBuf d_tot, d_stage, d_mail;
    std::vector<uint32_t> semi_block_end;                  // local semi count after each fragment pass
    struct Seg { int c, p; uint32_t count; }; std::vector<Seg> full_segs;   // local fulls list = these, in order
    DevBuf d_hostred;
    uint32_t seg_lo[ALLOC_SLOTS + 1] = {0};                // first local amplicon of each list segment slot (do_allocate); [ALLOC_SLOTS] = amplicon count
    int pending_seg_cycle = -1;
    // collectives run when the job is sharded -- or whenever hooks are installed (1-shard jobs then exercise them too)
    bool sharded() const { return cfg.shard_count > 1 || allreduce || allreduce_dev; }
    void reduce(uint64_t* v, uint64_t n) {
        if (!sharded()) return;
        if (allreduce_dev) {                                                       // device hook installed: two small copies beat the host hook's round trip
            d_hostred.reserve(n * 8, stream);
            HIP_OK(hipMemcpyAsync(d_hostred.p, v, n * 8, hipMemcpyHostToDevice, stream));
            if (allreduce_dev(coll_dev_user, d_hostred.p, n, 8)) throw ScsError(SCS_EINVAL, "sharded job: device all-reduce hook failed");
            HIP_OK(hipMemcpyAsync(v, d_hostred.p, n * 8, hipMemcpyDeviceToHost, stream)); HIP_OK(hipStreamSynchronize(stream));
            return;
        }
        if (!allreduce || allreduce(coll_user, v, n)) throw ScsError(SCS_EINVAL, "sharded job: all-reduce hook missing or failed (scs_set_collectives)");
    }
    // sum a device array over all shards, in place, ordered on the ctx stream when the device hook is set
    void reduce_dev(void* d, uint64_t n, int elem_bytes) {
        if (!sharded()) return;
        if (allreduce_dev) { if (allreduce_dev(coll_dev_user, d, n, elem_bytes)) throw ScsError(SCS_EINVAL, "sharded job: device all-reduce hook failed"); return; }
        std::vector<uint64_t> v(n);                                                // fallback: stage through the host hook
        if (elem_bytes == 8) { HIP_OK(hipMemcpyAsync(v.data(), d, n * 8, hipMemcpyDeviceToHost, stream)); HIP_OK(hipStreamSynchronize(stream)); }
        else { std::vector<uint32_t> w(n); HIP_OK(hipMemcpyAsync(w.data(), d, n * 4, hipMemcpyDeviceToHost, stream)); HIP_OK(hipStreamSynchronize(stream)); for (uint64_t i = 0; i < n; ++i) v[i] = w[i]; }
        reduce(v.data(), n);
        if (elem_bytes == 8) { HIP_OK(hipMemcpyAsync(d, v.data(), n * 8, hipMemcpyHostToDevice, stream)); HIP_OK(hipStreamSynchronize(stream)); }
        else { std::vector<uint32_t> w(n); for (uint64_t i = 0; i < n; ++i) w[i] = (uint32_t)std::min<uint64_t>(v[i], 0xFFFFFFFFull);
               HIP_OK(hipMemcpyAsync(d, w.data(), n * 4, hipMemcpyHostToDevice, stream)); HIP_OK(hipStreamSynchronize(stream)); }
    }
    // every shard's `bytes` at d_send -> d_recv[r * bytes ..], ordered on the ctx stream when the device hook is set
    void gather_dev(const void* d_send, void* d_recv, uint64_t bytes) {
        if (allgather_dev) { if (allgather_dev(coll_dev_user, d_send, d_recv, bytes)) throw ScsError(SCS_EINVAL, "sharded job: device all-gather hook failed"); return; }
        std::vector<uint8_t> h(bytes), all((size_t)bytes * cfg.shard_count); std::vector<uint64_t> sizes(cfg.shard_count, 0);
        HIP_OK(hipMemcpyAsync(h.data(), d_send, bytes, hipMemcpyDeviceToHost, stream)); HIP_OK(hipStreamSynchronize(stream));
        if (!allgatherv || allgatherv(coll_user, h.data(), bytes, all.data(), bytes, sizes.data())) throw ScsError(SCS_EINVAL, "sharded job: all-gather hook missing or failed (scs_set_collectives)");
        HIP_OK(hipMemcpyAsync(d_recv, all.data(), all.size(), hipMemcpyHostToDevice, stream)); HIP_OK(hipStreamSynchronize(stream));
    }
    scs_stats st{};
    KernelTimer tm[TM_COUNT] = {{"k_errs<semi->full>"}, {"k_errs<frag->semi>"}, {"k_reads"}, {"k_attach<semi>"}, {"k_indels"}, {"k_attach<frag>"}, {"k_truth"}, {"k_depth"}};
    // the timers a yield call runs: reset at its start, collected at its end.  A new side output's timer is one more entry here
    std::array<KernelTimer*, 12> yield_timers() { return {&tm[TM_READS], &tm[TM_INDELS], &tm[TM_TRUTH], &tm[TM_DEPTH], &tm_support, &tm_depth_ref, &tm_support_ref_open, &tm_support_ref_gather, &tm_cov_mark, &tm_cov_finish, &tm_cov_ref_copies, &tm_cov_ref_finish}; }

    DevFrags frags_view() const {
        uint8_t* b = df_blob.as<uint8_t>();
        return DevFrags{(uint64_t*)b, (uint32_t*)(b + df_len_off), (int8_t*)(b + df_strand_off), df_primers.as<uint32_t>(), (uint32_t)f_len.size(), f_gidx_base, df_hasn.as<uint8_t>()};
    }
    std::unique_ptr<SinkPipe, SinkPipeDelete> pipe;        // the sink's writers and pinned slots, made by the first yield into a sink
};


namespace scs {
// ---- scs_pipeline.cpp
std::string& create_error();                // this thread's scs_last_error(NULL): what scs_create and the ctx-less entry points report
inline void copy_err(char* errbuf, size_t errlen, const char* msg) { if (errbuf && errlen) { strncpy(errbuf, msg, errlen - 1); errbuf[errlen - 1] = 0; } }
// mailbox: device scalars -> pinned host words
void mail_post(scs_ctx* c, const Mail& m, bool last, hipStream_t st = nullptr);   // last: the post the host will wait for; st: the ctx stream unless given
void mail_wait(scs_ctx* c);                                                      // everything posted so far has landed in h_rb
void flags_eval(scs_ctx* c);
void check_flags(scs_ctx* c);
template <class T>
inline void upload(DevBuf& b, const std::vector<T>& v, hipStream_t s, size_t extra = 0) {
    b.reserve(std::max<size_t>((v.size() + extra) * sizeof(T), 16), s);
    if (!v.empty()) HIP_OK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
}


// ---- scs_stage.cpp
void do_load_profile(scs_ctx* c, const char* path);
void index_genome(scs_ctx* c, uint64_t tot);
void stage_genome(scs_ctx* c, const void* d_ascii = nullptr, const uint64_t* d_lens = nullptr);
void stage_fasta_on_device(scs_ctx* c, const std::string& path_in);
bool stage_fasta_slice(scs_ctx* c, const std::string& path);
void do_create_frags(scs_ctx* c);
// ---- scs_amplify.cpp
void do_amplify(scs_ctx* c);
// ---- scs_reads.cpp
void do_allocate(scs_ctx* c, uint64_t reads);
void allocate_weighted(scs_ctx* c, uint64_t reads, uint32_t ac);   // everything of do_allocate behind the weights: over the ac weights in c->weights
struct CallbackSink : BatchSink {           // a caller's scs_sink_fn as a BatchSink: one region, the batches in record order
    scs_sink_fn fn; void* user;
    CallbackSink(scs_sink_fn f, void* u) : fn(f), user(u) {}
    int put(int, const char* a, size_t na, const char* b, size_t nb) override { return fn(user, a, na, b, nb); }
};
struct OutTarget { bool device; char* d1; char* d2; size_t cap1, cap2; BatchSink* sink;
                   std::vector<uint64_t>* seg_off1 = nullptr; std::vector<uint64_t>* seg_off2 = nullptr;   // seg_off: byte offset of each list segment's first record (shard index)
                   bool bgzf = false;                                             // bgzf: the sink gets BGZF blocks made on the device instead of the text
                   bool discard = false; };                                       // discard: the FASTQ text is not wanted on the host (a NULL sink with truth on)
// the batches of a yield: pairs per batch, their number, the order they are made in and the writer region of each (pure arithmetic: no device, no ctx)
struct BatchPlan { uint64_t batch = 1; uint32_t nbatch = 0; std::vector<uint32_t> order, region_of; };
BatchPlan plan_batches(uint64_t P, uint32_t read_length, bool to_sink, int writers, int regions, int batch_shift);

void do_yield(scs_ctx* c, const OutTarget& tg, uint64_t* n1_out, uint64_t* n2_out, uint64_t* pairs_out);
// truth SAM: refuses (SCS_EINVAL) the targets it does not apply to; device: scs_yield_reads_device, writers: the file sink's
void truth_check(scs_ctx* c, bool device, int writers);
// the truth SAM on the reference is switched off: everything its yield calls made for it goes (the truth passes' buffers, which
// the next truth output of any kind makes again)
void truth_ref_release(scs_ctx* c);
// the depth tracks (scs_depth.cpp), both at once: depth_check refuses (SCS_EINVAL) a sharded or sliced ctx, and the reference track
// without a lift table, at the yield call's entry; depth_yield_check the same and more than DEPTH_MAX_BINS bins, before the call's
// GPU work.  depth_open, one track: the kernel's tables, this call's zeroed counters and (on_ref, once per layout) the copies
void depth_check(scs_ctx* c);
void depth_yield_check(scs_ctx* c);
void depth_open(scs_ctx* c, bool on_ref);
// the coverage profile (scs_coverage.cpp): coverage_check refuses (SCS_EINVAL) a sharded or sliced ctx at the yield call's entry;
// coverage_open: the call's zeroed difference array and tables and the kernels' record starts; coverage_finish: the end-of-job
// pass on the ctx stream (lds: buckets of its LDS histogram)
void coverage_check(scs_ctx* c);
void coverage_invalidate(scs_ctx* c, bool genome_changed);   // another genome is staged, or (false) only another lift table: what was made of the old one no longer stands
void coverage_open(scs_ctx* c);
void coverage_finish(scs_ctx* c, uint32_t lds);
// ... on the reference (scs_set_coverage_ref): coverage_check refuses it too (sharded, or no lift table); coverage_ref_open, after
// coverage_open: the zeroed reference array and tables, and the packed copies where the genome or the table is new;
// coverage_ref_finish, after coverage_finish: the staged depths through the table, counted per reference record;
// coverage_ref_close, once the call's flags are clean: the sum identity (SCS_EOVERFLOW where it does not hold)
void coverage_ref_open(scs_ctx* c);
void coverage_ref_finish(scs_ctx* c, uint32_t lds);
void coverage_ref_close(scs_ctx* c);
// lift table (scs_lift.cpp): lift_install makes T the ctx's table (host and device), lift_drop forgets it (every call that stages a
// genome); need_lift refuses (SCS_EINVAL) in fn's name where there is none
void lift_install(scs_ctx* c, LiftTable&& T);
void lift_drop(scs_ctx* c);
void need_lift(const scs_ctx* c, const char* fn);
// site support (scs_support.cpp): refuses (SCS_EINVAL) a sharded or sliced ctx at the yield call; the call's site table, positions and zeroed counters
void support_check(scs_ctx* c);
void support_open(scs_ctx* c);
// the table on the reference alone, after the last batch: the staged counters summed by reference position, on the ctx stream
void support_close(scs_ctx* c);
// "site support (scs_set_site_support)", or the reference table's name: what the yield call's refusals open with
std::string support_name(const scs_ctx* c);
// the bedGraph writer (scs_runs.cpp): the run-length text of values[n] under mask -- records of the starts roff (n_rec + 1, the
// last one n) and names name(r) -- to the file at path (a name ending in .gz: BGZF made on the device); who: the entry point's name
void runs_write_file(scs_ctx* c, const std::string& who, const char* path, const uint32_t* values, uint32_t mask, uint64_t n, const std::vector<uint64_t>& roff,
                     const std::vector<std::string>& names, uint64_t* lines, uint64_t* text_bytes);
std::vector<int> gpu_local_cpus(int device);   // scs_sink.cpp

template <class F>
int guarded(scs_ctx* c, F f) {
    if (!c) return SCS_EINVAL;
    try { if (c->cfg.device >= 0) (void)hipSetDevice(c->cfg.device); f(); return SCS_OK; }
    catch (const ScsError& e) { c->err = e.what(); return e.code; }
    catch (const std::exception& e) { c->err = e.what(); return SCS_EIO; }
}

}  // namespace scs
