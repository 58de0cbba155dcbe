// scs_sitejob.h -- private to the host files of the artefact table, on the staged genome and on the original reference (scs_sites.cpp:
// the same scheme over either axis), and of the site support table (scs_support.cpp), which is the same table with the reads'
// counters: one call's pass over the amplicons slab by slab (SiteJob) and what turns a run of sites into bytes of a file (SiteOut).  Every buffer, stream and event belongs to the struct that holds it and goes with it.
#pragma once
#include "scs_textout.h"
#include "scs_site.h"
#include "scs_site_ref.h"

namespace scs {


const uint32_t kSiteChunk = 1u << 20;                      // amplicons per launch of the counting and fill passes
const uint64_t kSiteSlab = 1ull << 28;                     // genome indices per slab
const uint64_t kSitePiece = 32ull << 20;                   // bytes of the file that cross to the host at a time
const uint64_t kSiteMaxEntries = 0x7FFFFF00ull;            // edit entries (and amplicons) one slab may hold

inline void site_check(scs_ctx* c, const char* fn, bool on_ref) {   // (amp_check's refusals, scs_amplicons.cpp; on_ref: and no lift table)
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, std::string(fn) + ": not available for a sharded job (shard_count > 1)");
    if (on_ref && !c->have_lift) throw ScsError(SCS_EINVAL, std::string(fn) + ": the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
    if (!c->allocated) throw ScsError(SCS_EINVAL, std::string(fn) + ": call scs_allocate_reads first (the table states every site's read support)");
}

// A run of sites becomes bytes of the file: the emit pass over their sized lines (and BGZF over the text where it lies), then the
// bytes travel in PIECES over the copy stream into two pinned blocks, piece p + 1 on its way while the host writes piece p to the
// file.  The pinned blocks hold a piece, the device buffers a run's text: nothing holds the job's
struct SiteOut {
    uint32_t lds = 0; uint64_t piece = kSitePiece;
    Stream copy; Event ev_made, ev_d2h[2]; DevBuf out, crc; BgzfLane z; Pinned<char> h_out[2]; Pinned<uint32_t> h_z;
    SiteOut() {
        if (seam_env("SCS_TEST_SITE_LDS")) lds = (uint32_t)std::max(16, atoi(seam_env("SCS_TEST_SITE_LDS")));                            // tests: lines that straddle two LDS runs
        if (seam_env("SCS_TEST_SITE_PIECE")) piece = (uint64_t)std::max(1L, std::min(atol(seam_env("SCS_TEST_SITE_PIECE")), 1L << 30));      // tests: a run's bytes in many pieces
    }
    void open(hipStream_t s, bool bgzf) {
        copy.ensure(hipStreamNonBlocking);
        ev_made.ensure(hipEventDisableTiming | hipEventBlockingSync); for (int k = 0; k < 2; ++k) ev_d2h[k].ensure(hipEventDisableTiming | hipEventBlockingSync);
        h_z.reserve(64, hipHostMallocDefault); memset(h_z, 0, 64);
        if (bgzf) bgzf_crc_tables(crc, s);
    }
    // the t.n entries' lines (t_n bytes at the offsets offs; site_pos / counts: launch_site_emit's) made on the ctx stream; returns where
    // the bytes to ship lie and sets *n to their number, once they are made
    const char* make(hipStream_t s, KernelTimer& tm, const SiteArgs& t, const SiteRec* recs, const uint64_t* offs, uint64_t t_n, bool bgzf, void* scan_tmp, size_t scan_bytes,
                     const char* too_large, uint64_t* n, const uint32_t* site_pos = nullptr, const uint32_t* counts = nullptr) {
        out.reserve(std::max<uint64_t>(t_n + t_n / 16, 16) + 16, s);
        const char* made = out.as<char>();
        tm.begin(s);
        launch_site_emit(s, t, recs, offs, lds, out.as<char>(), site_pos, counts);
        if (bgzf) {                                        // the text becomes BGZF blocks where it lies (the FASTQ blocks' kernels); their total travels to h_z
            z.out[0].reserve(bgzf_bound(t_n), s);
            bgzf_in_place(s, z, crc, made, t_n, z.out[0].as<char>(), h_z, scan_tmp, scan_bytes, too_large);
            made = z.out[0].as<char>();
        }
        tm.end(s);
        HIP_OK(hipEventRecord(ev_made, s)); HIP_OK(hipEventSynchronize(ev_made));   // (the blocks' total has arrived; the copy stream may read what was made)
        *n = bgzf ? (uint64_t)h_z[0] : t_n;
        return made;
    }
    void ship(OutFile& fd, const char* p, uint64_t n) {
        const uint64_t P = piece, np = (n + P - 1) / P;
        for (int q = 0; q < 2; ++q) h_out[q].reserve(std::min<uint64_t>(P, std::max<uint64_t>(n, 16)), hipHostMallocDefault);
        for (uint64_t sent = 0, done = 0; done < np; ++done) {
            for (; sent < np && sent < done + 2; ++sent) {   // (piece sent - 2, the block's last user, is in the file)
                HIP_OK(hipMemcpyAsync(h_out[sent & 1], p + sent * P, std::min(P, n - sent * P), hipMemcpyDeviceToHost, copy));
                HIP_OK(hipEventRecord(ev_d2h[sent & 1], copy));
            }
            HIP_OK(hipEventSynchronize(ev_d2h[done & 1]));
            fd.write(h_out[done & 1], std::min(P, n - done * P));
        }
    }
    ~SiteOut() { if (copy.s) (void)hipStreamSynchronize(copy); }
};

// One call's work: the kernels' arguments over the ctx's tables, the per-slab counts, and everything the call allocates.  Its
// destructor ends every way out of the call: both streams drained; the members then release themselves.
// on_ref: the slabs are slabs of REFERENCE indices, the counting, fill and reduce passes are
// scs_k_sites_ref.hip's over the lift table (v), `amplicons` reads `pieces of amplicons`, t names the reference records, and the
// counting pass also finds the two unlifted totals and is followed by a check of the flags.  Everything else is one code
struct SiteJob {
    scs_ctx* const c; const hipStream_t s; const bool on_ref; const char* const what; KernelTimer idle{"k_sites"}; KernelTimer& tm; AmpArgs a{}; SiteArgs t{};   // tm: the ctx's timer (scs_write_artefacts / _ref), or one that is off
    uint32_t chunk = kSiteChunk, min_reads = 0; uint64_t slab = kSiteSlab, bases = 0; uint32_t n_slabs = 0;   // bases: of the axis the slabs cut
    std::vector<uint64_t> cnt;                             // [2 k]: edit entries of slab k, [2 k + 1]: amplicons (pieces) that overlap it; on_ref: behind them the two unlifted totals
    SiteRefView v{}; RecTable ref_rt; uint64_t unlifted[2] = {0, 0};   // on_ref: the walk's view of the lift table; the reference records' table
    uint64_t max_e = 0, max_a = 0; size_t sort_bytes = 0, scan_bytes = 0;
    Event ev_n; RecTable rt; SiteOut em;                   // em: the file's bytes (scs_write_artefacts)
    DevBuf d_cnt, cur, keys[2], kreads[2], starts[2], ends[2], areads[3], ps_start, ps_end, sort_tmp, scan_tmp, site_recs, sizes, offs, keep, keep_pos, packed;
    Pinned<uint64_t> h_n;

    SiteJob(scs_ctx* c_, uint32_t min_reads_, bool timed, bool on_ref_ = false)
        : c(c_), s(c_->stream), on_ref(on_ref_), what(on_ref_ ? "artefact table on the reference" : "artefact table"), tm(timed ? (on_ref_ ? c_->tm_site_ref : c_->tm_site) : idle), min_reads(min_reads_) {
        idle.on = false;
        if (seam_env("SCS_TEST_AMP_CHUNK")) chunk = (uint32_t)std::max(1L, std::min(atol(seam_env("SCS_TEST_AMP_CHUNK")), 1L << 30));     // tests: chunk edges
        if (seam_env("SCS_TEST_SITE_SLAB")) slab = (uint64_t)std::max(1L, std::min(atol(seam_env("SCS_TEST_SITE_SLAB")), 1L << 40));      // tests: sites and amplicons on both sides of slab borders
        tm.reset();
        rt.make(c, s); bases = rt.bases; const uint32_t nr = rt.n_rec;
        a.fr = c->frags_view(); a.semis = c->semis.view(); a.fulls = c->fulls.view(); a.spool = c->semis.pool.as<uint32_t>(); a.fpool = c->fulls.pool.as<uint32_t>();
        a.g = c->genome.as<uint8_t>(); a.read_numbers = c->read_numbers.as<uint32_t>();
        a.rec_off = rt.rec_off; a.name_off = rt.name_off; a.names = rt.names; a.n_rec = nr;
        a.flags = c->flags.as<uint32_t>();
        t.g = a.g; t.rec_off = a.rec_off; t.name_off = a.name_off; t.names = a.names; t.n_rec = nr; t.min_reads = min_reads; t.flags = a.flags;
        if (bases >> 60) throw ScsError(SCS_EOVERFLOW, "artefact table: the genome exceeds 2^60 bases");
        if (on_ref) reference();
        const uint64_t ns = t.n_rec && c->fulls.n && (!on_ref || v.n_seg) ? (bases + slab - 1) / slab : 0;
        if (ns > (1u << 24)) throw ScsError(SCS_EINVAL, std::string(what) + ": more than 2^24 slabs (SCS_TEST_SITE_SLAB too small for this genome)");
        n_slabs = (uint32_t)ns;
        count();
    }
    ~SiteJob() {
        (void)hipStreamSynchronize(s); if (em.copy.s) (void)hipStreamSynchronize(em.copy);
        tm.ev.clear(); tm.used = 0;                        // (the timer's events were this call's too; its sums stay)
    }

    // on_ref: the reference records' table (RecTable, over the lift table's names and lengths) takes the staged records' place in
    // t, and the slabs cut the reference
    void reference() {
        const LiftTable& L = c->lift; const uint32_t nf = (uint32_t)L.ref_lens.size();
        std::vector<uint64_t> roff(nf + 1, 0);
        for (uint32_t r = 0; r < nf; ++r) {
            roff[r + 1] = roff[r] + L.ref_lens[r];
            if ((L.ref_lens[r] >> 58) || (roff[r + 1] >> 58)) throw ScsError(SCS_EOVERFLOW, "artefact table on the reference: the reference exceeds 2^58 bases");
        }
        ref_rt.make(roff, [&](uint32_t r) -> const std::string& { return L.ref_names[r]; }, s);
        bases = ref_rt.bases;
        v.segs = c->d_lift.as<LiftSeg>(); v.n_seg = (uint32_t)L.segs.size(); v.ref_off = ref_rt.rec_off; v.n_ref = nf;
        t.rec_off = ref_rt.rec_off; t.name_off = ref_rt.name_off; t.names = ref_rt.names; t.n_rec = nf;
    }

    template <class F> void chunks(F f) {                  // the amplicon list, a chunk at a time
        const uint32_t N = c->fulls.n;
        for (uint32_t first = 0; first < N; first += std::min(chunk, N - first)) { a.first = first; a.n = std::min(chunk, N - first); f(); }
    }

    // the one pass over all amplicons: every slab's counts in one round trip, and the call's buffers sized by the largest slab
    void count() {
        cnt.assign((size_t)2 * n_slabs + (on_ref ? 2 : 0), 0);
        if (!n_slabs) return;
        const size_t bytes = cnt.size() * 8;
        d_cnt.reserve(bytes, s); HIP_OK(hipMemsetAsync(d_cnt.p, 0, bytes, s));
        tm.begin(s);
        chunks([&] { if (on_ref) launch_site_ref_count(s, a, v, slab, n_slabs, d_cnt.as<unsigned long long>()); else launch_site_count(s, a, slab, n_slabs, d_cnt.as<unsigned long long>()); });
        tm.end(s);
        HIP_OK(hipMemcpyAsync(cnt.data(), d_cnt.p, bytes, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string(what) + ": counting pass failed: " + hipGetErrorString(le)); }
        if (on_ref) { check_flags(c); unlifted[0] = cnt[(size_t)2 * n_slabs]; unlifted[1] = cnt[(size_t)2 * n_slabs + 1]; }   // a walk that failed is reported here, before anything is written
        for (uint32_t k = 0; k < n_slabs; ++k) if (cnt[2 * k]) { max_e = std::max(max_e, cnt[2 * k]); max_a = std::max(max_a, cnt[2 * k + 1]); }
        if (!max_e) return;
        if (max_e > kSiteMaxEntries || max_a > kSiteMaxEntries) throw ScsError(SCS_EOVERFLOW, std::string(what) + ": a slab holds more than 2^31 edit entries or amplicons");
        cur.reserve(16, s);
        for (int k = 0; k < 2; ++k) { keys[k].reserve((max_e + 1) * 8, s); kreads[k].reserve((max_e + 1) * 4, s); starts[k].reserve((max_a + 1) * 8, s); ends[k].reserve((max_a + 1) * 8, s); }
        for (int k = 0; k < 3; ++k) areads[k].reserve((max_a + 1) * 4, s);
        ps_start.reserve((max_a + 1) * 8, s); ps_end.reserve((max_a + 1) * 8, s);
        sort_bytes = std::max(site_sort_temp_bytes(max_e), site_sort_temp_bytes(max_a)); sort_tmp.reserve(sort_bytes, s);
        scan_bytes = scan_temp_bytes(std::max(max_e, max_a)); scan_tmp.reserve(scan_bytes, s);
        site_recs.reserve(max_e * sizeof(SiteRec), s); sizes.reserve((max_e + 1) * 4, s); offs.reserve((max_e + 1) * 8, s); keep.reserve((max_e + 1) * 4, s); keep_pos.reserve((max_e + 1) * 4, s);
        h_n.reserve(64, hipHostMallocDefault); memset(h_n, 0, 64);   // [0]: a slab's text bytes; [1]: its reported sites
        ev_n.ensure(hipEventDisableTiming | hipEventBlockingSync);
    }

    // the slab's reported sites packed in order into `packed` (after make: e its edit entries, kept = h_n[1])
    void compact(uint64_t e, uint64_t kept) {
        packed.reserve(std::max<uint64_t>(kept, 1) * sizeof(SiteRec), s);
        launch_site_compact(s, site_recs.as<SiteRec>(), keep.as<uint32_t>(), keep_pos.as<uint32_t>(), e, packed.as<SiteRec>());
    }

    // every slab with work, in order: made (make), then f(e, kept) -- its edit entries and its reported sites (h_n[0]: its text bytes)
    template <class F> void slabs(F f) {
        for (uint32_t k = 0; k < n_slabs; ++k) {
            if (!cnt[2 * k]) continue;                     // a slab without an entry has no site: nothing is launched for it
            const uint64_t e = make(k);
            f(e, (uint64_t)(uint32_t)h_n[1]);
        }
    }

    // slab k with work: its sorted entries, its sites and their line sizes, the text offsets and the reported sites' positions;
    // the two totals arrive in h_n[0] and h_n[1].  Returns the slab's edit entries
    uint64_t make(uint32_t k) {
        const uint64_t e = cnt[2 * k], m = cnt[2 * k + 1], x0 = (uint64_t)k * slab, x1 = std::min(bases, x0 + slab);
        const unsigned kb = site_bits(bases, on_ref ? SITE_REF_KEY_BITS : 2u), ib = site_bits(bases, 0);
        HIP_OK(hipMemsetAsync(cur.p, 0, 16, s));
        tm.begin(s);
        chunks([&] {
            if (on_ref) launch_site_ref_fill(s, a, v, x0, x1, cur.as<unsigned long long>(), e, m, keys[0].as<uint64_t>(), kreads[0].as<uint32_t>(), starts[0].as<uint64_t>(), ends[0].as<uint64_t>(), areads[0].as<uint32_t>());
            else launch_site_fill(s, a, x0, x1, cur.as<unsigned long long>(), e, m, keys[0].as<uint64_t>(), kreads[0].as<uint32_t>(), starts[0].as<uint64_t>(), ends[0].as<uint64_t>(), areads[0].as<uint32_t>());
        });
        launch_site_check(s, cur.as<unsigned long long>(), e, m, a.flags);
        launch_site_sort(s, keys[0].as<uint64_t>(), keys[1].as<uint64_t>(), kreads[0].as<uint32_t>(), kreads[1].as<uint32_t>(), e, kb, sort_tmp.p, sort_bytes);
        launch_site_sort(s, starts[0].as<uint64_t>(), starts[1].as<uint64_t>(), areads[0].as<uint32_t>(), areads[1].as<uint32_t>(), m, ib, sort_tmp.p, sort_bytes);
        launch_site_sort(s, ends[0].as<uint64_t>(), ends[1].as<uint64_t>(), areads[0].as<uint32_t>(), areads[2].as<uint32_t>(), m, ib, sort_tmp.p, sort_bytes);
        exclusive_scan_u32_to_u64(s, areads[1].as<uint32_t>(), ps_start.as<uint64_t>(), m, scan_tmp.p, scan_bytes);
        exclusive_scan_u32_to_u64(s, areads[2].as<uint32_t>(), ps_end.as<uint64_t>(), m, scan_tmp.p, scan_bytes);
        t.keys = keys[1].as<uint64_t>(); t.reads = kreads[1].as<uint32_t>(); t.n = e;
        t.starts = starts[1].as<uint64_t>(); t.ps_start = ps_start.as<uint64_t>(); t.ends = ends[1].as<uint64_t>(); t.ps_end = ps_end.as<uint64_t>(); t.m = m;
        if (on_ref) launch_site_ref_reduce(s, t, site_recs.as<SiteRec>(), sizes.as<uint32_t>(), keep.as<uint32_t>());
        else launch_site_reduce(s, t, site_recs.as<SiteRec>(), sizes.as<uint32_t>(), keep.as<uint32_t>());
        exclusive_scan_u32_to_u64(s, sizes.as<uint32_t>(), offs.as<uint64_t>(), e, scan_tmp.p, scan_bytes);
        exclusive_scan_u32(s, keep.as<uint32_t>(), keep_pos.as<uint32_t>(), e, scan_tmp.p, scan_bytes);
        tm.end(s);
        HIP_OK(hipMemcpyAsync(h_n, offs.as<uint64_t>() + e, 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(h_n + 1, keep_pos.as<uint32_t>() + e, 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipEventRecord(ev_n, s)); HIP_OK(hipEventSynchronize(ev_n));
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string(what) + ": a slab's passes failed: " + hipGetErrorString(le)); }
        return e;
    }
};

}  // namespace scs
