// scs_support.cpp -- the site support table (include/scssim_hip.h: scs_set_site_support, scs_site_support, scs_write_site_support;
// DESIGN.md section 15): the artefact table's sites (scs_sites.cpp) with what the reads of a yield call show at their coordinates.
// The sites are made on the device at the start of the yield call (support_open: the artefact table's SiteJob, slab by slab, its
// packed sites appended to a ctx-owned array that never visits the host), the counters per batch (scs_k_support.hip, launched from
// scs_reads.cpp), the file afterwards from both.  The sites, their positions and the counters belong to the ctx and go with
// scs_set_site_support(ctx, 0, ..); what a write call needs beyond them belongs to the call and goes with it.
// The same table on the ORIGINAL REFERENCE (scs_set_site_support_ref, scs_site_support_ref, scs_write_site_support_ref; DESIGN.md
// section 19) is this file's second axis, as scs_sites.cpp has one: support_ref switches the sites to the reference table's
// (SiteJob's on_ref) and the batches' position list to the staged positions that lift to the sites' reference positions
// (support_expand; scs_k_support_ref.hip: ranges, scan, fill), and adds a step behind the last batch that sums the staged counters
// by reference position (support_close).  Each entry point has one body for both.
#include "scs_sitejob.h"
#include "scs_support_ref.h"

namespace scs {

namespace {
const uint64_t kSupportChunk = 1ull << 20;                 // sites per turn of the emit and read-out loops: no buffer of theirs is sized by the job

const char* support_setter(bool on_ref) { return on_ref ? "scs_set_site_support_ref" : "scs_set_site_support"; }

void support_release(scs_ctx* c) {
    c->sp_sites.release(); c->sp_site_pos.release(); c->sp_pos.release(); c->sp_cnt.release(); c->sp_tab.release();
    c->spr_x.release(); c->spr_cnt.release(); c->sp_pos_x.release(); c->spr_tab.release();
    for (KernelTimer* t : {&c->tm_support, &c->tm_support_ref_open, &c->tm_support_ref_gather}) { t->ev.clear(); t->used = 0; t->reset(); }
    c->sp_n_sites = c->sp_n_pos = c->sp_n_x = 0; c->sp_unlifted[0] = c->sp_unlifted[1] = 0; c->support_valid = false;
}
void support_ready(scs_ctx* c, bool on_ref, const char* fn) {
    if (!c->support_on || c->support_ref != on_ref || !c->support_valid)
        throw ScsError(SCS_EINVAL, std::string(fn) + ": no yield call with the site support on (" + support_setter(on_ref) + ") has finished");
}
// the table's counters and how many positions they cover: the staged positions', or the reference positions'
const uint32_t* support_counts(const scs_ctx* c) { return (c->support_ref ? c->spr_cnt : c->sp_cnt).as<uint32_t>(); }
uint64_t support_positions(const scs_ctx* c) { return c->support_ref ? c->sp_n_x : c->sp_n_pos; }
std::vector<uint64_t> reference_starts(const scs_ctx* c) {
    const size_t nf = c->lift.ref_lens.size(); std::vector<uint64_t> roff(nf + 1, 0);
    for (size_t r = 0; r < nf; ++r) roff[r + 1] = roff[r] + c->lift.ref_lens[r];
    return roff;
}

void support_set(scs_ctx* c, bool on_ref, int on, uint32_t min_reads) {
    if (c->support_on && c->support_ref != on_ref) {       // one position list per yield call: the other table is on
        if (!on) return;                                   // (nothing of this table exists)
        throw ScsError(SCS_EINVAL, std::string(support_setter(on_ref)) + ": the site support is on through " + support_setter(!on_ref) + "; a yield call makes one of the two tables -- turn that one off first (" +
                                   support_setter(!on_ref) + "(ctx, 0, 0))");
    }
    HIP_OK(hipStreamSynchronize(c->stream));               // the last call's table and counters go: nothing may still read them
    support_release(c);
    c->support_on = on != 0; c->support_ref = on && on_ref; c->support_min_reads = on ? min_reads : 0;
}

// the reference positions spr_x expanded to the staged positions sp_pos (ascending) and every staged position's reference position
// sp_pos_x; returns their number
uint64_t support_expand(scs_ctx* c, uint64_t n_x) {
    const hipStream_t s = c->stream; const std::string what = support_name(c); const uint32_t n_seg = (uint32_t)c->lift.segs.size();
    if (!n_x || !n_seg) return 0;
    uint64_t chunk = ~0ull;
    if (seam_env("SCS_TEST_SUPPORT_REF_CHUNK")) chunk = (uint64_t)std::max(1L, atol(seam_env("SCS_TEST_SUPPORT_REF_CHUNK")));   // tests: a launch border inside a segment's range
    SupportRefView v{c->d_lift.as<LiftSeg>(), n_seg, c->sp_tab.as<uint64_t>(), (uint32_t)c->recs.size(), c->spr_tab.as<uint64_t>(), (uint32_t)c->lift.ref_lens.size(), c->spr_x.as<uint64_t>(), n_x};
    DevBuf seg_a, seg_n, off, tmp; const size_t tb = scan_temp_bytes(n_seg);
    seg_a.reserve((size_t)n_seg * 8, s); seg_n.reserve(((size_t)n_seg + 1) * 4, s); off.reserve(((size_t)n_seg + 1) * 8, s); tmp.reserve(tb, s);
    launch_support_ref_ranges(s, v, seg_a.as<uint64_t>(), seg_n.as<uint32_t>(), c->flags.as<uint32_t>());
    exclusive_scan_u32_to_u64(s, seg_n.as<uint32_t>(), off.as<uint64_t>(), n_seg, tmp.p, tb);
    uint64_t total = 0;
    HIP_OK(hipMemcpyAsync(&total, off.as<uint64_t>() + n_seg, 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
    check_flags(c);                                        // a segment that does not fit: the call fails before a slot is filled
    if (total > SUPPORT_MAX_POS) throw ScsError(SCS_EOVERFLOW, what + ": " + std::to_string(total) + " staged positions, more than 2^29 - 1; raise min_reads");
    c->sp_pos.reserve(std::max<size_t>((size_t)total * 8, 16), s); c->sp_pos_x.reserve(std::max<size_t>((size_t)total * 4, 16), s);
    for (uint64_t t0 = 0; t0 < total; t0 += std::min(chunk, total - t0))
        launch_support_ref_fill(s, v, off.as<uint64_t>(), seg_a.as<uint64_t>(), t0, std::min(chunk, total - t0), total, c->sp_pos.as<uint64_t>(), c->sp_pos_x.as<uint32_t>(), c->flags.as<uint32_t>());
    HIP_OK(hipStreamSynchronize(s));                       // (seg_a, seg_n, off and tmp go)
    return total;
}
}  // namespace

std::string support_name(const scs_ctx* c) { return c->support_ref ? "site support on the reference (scs_set_site_support_ref)" : "site support (scs_set_site_support)"; }

void support_check(scs_ctx* c) {
    if (!c->support_on) return;
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, support_name(c) + ": not available for a sharded job (shard_count > 1); turn it off with " + support_setter(c->support_ref) + "(ctx, 0, 0)");
    if (c->support_ref && !c->have_lift) throw ScsError(SCS_EINVAL, support_name(c) + ": the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
}

// The call's site table: the artefact table's slabs, each slab's reported sites packed and appended; then the distinct coordinates
// (head flags, the library's scan, a scatter) and this call's counters, zeroed on the ctx stream.  On the reference the
// coordinates are reference positions, and the staged positions that lift to them follow (support_expand)
void support_open(scs_ctx* c) {
    const hipStream_t s = c->stream; const bool on_ref = c->support_ref; const std::string what = support_name(c);
    c->sp_n_sites = c->sp_n_pos = c->sp_n_x = 0;
    uint64_t n = 0;
    {
        SiteJob J(c, c->support_min_reads, false, on_ref);
        c->sp_unlifted[0] = J.unlifted[0]; c->sp_unlifted[1] = J.unlifted[1];
        J.slabs([&](uint64_t e, uint64_t kept) {
            if (!kept) return;
            // more sites than the most positions can carry: a staged index has one REF and three ALT, a reference position up to
            // five REF (A, C, G, T, N) of the haplotypes that lift to it with the ALT that differ from each -- sixteen
            if (!on_ref && n + kept > 3ull * SUPPORT_MAX_POS) throw ScsError(SCS_EOVERFLOW, what + ": more than 2^29 - 1 distinct positions; raise min_reads");
            if (on_ref && n + kept > 16ull * SUPPORT_MAX_POS) throw ScsError(SCS_EOVERFLOW, what + ": more than 16 x (2^29 - 1) sites, more than 2^29 - 1 reference positions can carry; raise min_reads");
            J.compact(e, kept);
            c->sp_sites.reserve((n + kept) * sizeof(SiteRec), s, n * sizeof(SiteRec));
            HIP_OK(hipMemcpyAsync(c->sp_sites.as<SiteRec>() + n, J.packed.p, kept * sizeof(SiteRec), hipMemcpyDeviceToDevice, s));
            n += kept;
        });
        // the record starts for the kernels of this call (the job's own table goes with it)
        const std::vector<uint64_t> roff = record_starts(c);
        upload(c->sp_tab, roff, s);
        if (on_ref) upload(c->spr_tab, reference_starts(c), s);
        HIP_OK(hipStreamSynchronize(s));
    }
    // the sites' own records: the staged ones, or the reference's
    const uint64_t* site_off = (on_ref ? c->spr_tab : c->sp_tab).as<uint64_t>(); const uint32_t site_recs = on_ref ? (uint32_t)c->lift.ref_lens.size() : (uint32_t)c->recs.size();
    DevBuf& pos = on_ref ? c->spr_x : c->sp_pos;
    uint32_t n_pos = 0;
    if (on_ref) c->tm_support_ref_open.begin(s);
    if (n) {
        DevBuf head, e, tmp; const size_t tb = scan_temp_bytes(n);
        head.reserve((n + 1) * 4, s); e.reserve((n + 1) * 4, s); tmp.reserve(tb, s);
        c->sp_site_pos.reserve(n * 4, s);
        launch_support_heads(s, c->sp_sites.as<SiteRec>(), n, site_off, site_recs, head.as<uint32_t>(), c->flags.as<uint32_t>());
        exclusive_scan_u32(s, head.as<uint32_t>(), e.as<uint32_t>(), n, tmp.p, tb);
        HIP_OK(hipMemcpyAsync(&n_pos, e.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        if (n_pos > SUPPORT_MAX_POS) throw ScsError(SCS_EOVERFLOW, what + ": " + std::to_string(n_pos) + " distinct positions, more than 2^29 - 1; raise min_reads");
        pos.reserve(std::max<size_t>((size_t)n_pos * 8, 16), s);
        launch_support_scatter(s, c->sp_sites.as<SiteRec>(), n, site_off, head.as<uint32_t>(), e.as<uint32_t>(), pos.as<uint64_t>(), c->sp_site_pos.as<uint32_t>());
        HIP_OK(hipStreamSynchronize(s));                                           // (head, e and tmp go)
    }
    uint64_t n_staged = n_pos;
    if (on_ref) {
        check_flags(c);                                    // (sites out of order: no bisection over them)
        n_staged = support_expand(c, n_pos);
        c->tm_support_ref_open.end(s); c->tm_support_ref_open.add_units(n_staged);
        const size_t rb = std::max<size_t>((size_t)n_pos * 24, 16);
        c->spr_cnt.reserve(rb, s); HIP_OK(hipMemsetAsync(c->spr_cnt.p, 0, rb, s));
        if (!c->sp_pos.p) c->sp_pos.reserve(16, s);
    }
    const size_t cb = std::max<size_t>((size_t)n_staged * 24, 16);
    c->sp_cnt.reserve(cb, s); HIP_OK(hipMemsetAsync(c->sp_cnt.p, 0, cb, s));
    check_flags(c);
    c->sp_n_sites = n; c->sp_n_pos = n_staged; c->sp_n_x = on_ref ? n_pos : 0;
}

void support_close(scs_ctx* c) {
    if (!c->support_ref) return;
    const hipStream_t s = c->stream;
    c->tm_support_ref_gather.begin(s);
    launch_support_ref_gather(s, c->sp_cnt.as<uint32_t>(), c->sp_pos_x.as<uint32_t>(), c->sp_n_pos, c->sp_n_x, c->spr_cnt.as<uint32_t>(), c->flags.as<uint32_t>());
    c->tm_support_ref_gather.end(s); c->tm_support_ref_gather.add_units(c->sp_n_pos);
}

namespace {

void support_into(scs_ctx* c, bool on_ref, const std::string& fn, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr, uint32_t* counts,
                  uint64_t cap, uint64_t* n, uint64_t* unlifted) {
    if (!n) throw ScsError(SCS_EINVAL, fn + ": n is NULL");
    support_ready(c, on_ref, fn.c_str());
    const hipStream_t s = c->stream; const uint64_t total = c->sp_n_sites, n_pos = support_positions(c); const uint32_t* cnt = support_counts(c);
    *n = total;
    if (unlifted) { unlifted[0] = c->sp_unlifted[0]; unlifted[1] = c->sp_unlifted[1]; }
    HIP_OK(hipStreamSynchronize(s));
    if (cap < total) throw ScsError(SCS_EOVERFLOW, fn + ": " + std::to_string(total) + " sites, room for " + std::to_string(cap));
    std::vector<SiteRec> h; std::vector<uint32_t> sp, cn;
    for (uint64_t first = 0; first < total; first += kSupportChunk) {
        const uint64_t m = std::min(kSupportChunk, total - first);
        h.resize(m); sp.resize(m);
        HIP_OK(hipMemcpyAsync(h.data(), c->sp_sites.as<SiteRec>() + first, m * sizeof(SiteRec), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(sp.data(), c->sp_site_pos.as<uint32_t>() + first, m * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        const uint32_t p0 = sp[0], p1 = sp[m - 1];     // (the sites' positions ascend: the chunk's counters are one run)
        if (p1 < p0 || p1 >= n_pos) throw ScsError(SCS_EDEVICE, fn + ": the sites' positions are not in order");
        if (counts) { cn.resize(6 * (size_t)(p1 - p0 + 1)); HIP_OK(hipMemcpyAsync(cn.data(), cnt + 6 * (size_t)p0, cn.size() * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s)); }
        for (uint64_t i = 0; i < m; ++i) {
            const SiteRec& r = h[i]; const uint64_t o = first + i;
            if (rec) rec[o] = r.rec; if (pos) pos[o] = r.pos; if (ref) ref[o] = r.ref; if (alt) alt[o] = r.alt;
            if (na) na[o] = r.na; if (ta) ta[o] = r.ta; if (nr) nr[o] = r.nr; if (tr) tr[o] = r.tr;
            if (counts) { if (sp[i] < p0 || sp[i] > p1) throw ScsError(SCS_EDEVICE, fn + ": the sites' positions are not in order"); memcpy(counts + 6 * o, cn.data() + 6 * (size_t)(sp[i] - p0), 24); }
        }
    }
}

void support_write(scs_ctx* c, bool on_ref, const std::string& fn, const char* path, int flags, uint64_t* sites, uint64_t* bytes) {
    if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
    if (flags & ~1) throw ScsError(SCS_EINVAL, fn + ": unknown flag");
    support_ready(c, on_ref, fn.c_str());
    const bool bgzf = (flags & 1) != 0; const hipStream_t s = c->stream; const uint64_t total_sites = c->sp_n_sites; const uint32_t* cnt = support_counts(c);
    const std::string too_large = fn + ": a chunk's text exceeds 4 GB";
    OutFile fd; fd.open(fn, path, bgzf);
    if (on_ref) fd.header(site_ref_header(c->lift.ref_names, c->lift.ref_lens.data(), c->sp_unlifted[0], c->sp_unlifted[1], true));
    else { std::vector<std::string> names; for (const auto& r : c->recs) names.push_back(r.name); fd.header(site_header(names, c->rec_len.data(), true)); }
    // what the call needs beyond the ctx's arrays belongs to it: the record table, a chunk's line sizes and offsets, the emitter.
    // The struct's destructor ends every way out: both streams drained, then the members release themselves
    struct Call { hipStream_t s; RecTable rt; SiteOut em; DevBuf sizes, offs, scan; Pinned<uint64_t> h_n; Event ev_n; KernelTimer idle{"k_sites"};
                  ~Call() { (void)hipStreamSynchronize(s); } } W{s};
    W.idle.on = false;
    if (total_sites) {
        const uint64_t cm = std::min(kSupportChunk, total_sites); const size_t sb = scan_temp_bytes(cm);
        if (on_ref) W.rt.make(reference_starts(c), [&](uint32_t r) -> const std::string& { return c->lift.ref_names[r]; }, s); else W.rt.make(c, s);
        W.em.open(s, bgzf);
        W.sizes.reserve((cm + 1) * 4, s); W.offs.reserve((cm + 1) * 8, s); W.scan.reserve(sb, s);
        W.h_n.reserve(64, hipHostMallocDefault); W.ev_n.ensure(hipEventDisableTiming | hipEventBlockingSync);
        SiteArgs t{}; t.rec_off = W.rt.rec_off; t.name_off = W.rt.name_off; t.names = W.rt.names; t.n_rec = W.rt.n_rec; t.flags = c->flags.as<uint32_t>();
        for (uint64_t first = 0; first < total_sites; first += kSupportChunk) {
            t.n = std::min(kSupportChunk, total_sites - first);
            const SiteRec* recs = c->sp_sites.as<SiteRec>() + first; const uint32_t* sp = c->sp_site_pos.as<uint32_t>() + first;
            launch_support_size(s, t, recs, sp, cnt, W.sizes.as<uint32_t>());
            exclusive_scan_u32_to_u64(s, W.sizes.as<uint32_t>(), W.offs.as<uint64_t>(), t.n, W.scan.p, sb);
            HIP_OK(hipMemcpyAsync(W.h_n, W.offs.as<uint64_t>() + t.n, 8, hipMemcpyDeviceToHost, s));
            HIP_OK(hipEventRecord(W.ev_n, s)); HIP_OK(hipEventSynchronize(W.ev_n));
            { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("site support: the sizing pass failed: ") + hipGetErrorString(le)); }
            const uint64_t t_n = W.h_n[0]; uint64_t nb = 0;
            const char* made = W.em.make(s, W.idle, t, recs, W.offs.as<uint64_t>(), t_n, bgzf, W.scan.p, sb, too_large.c_str(), &nb, sp, cnt);
            W.em.ship(fd, made, nb);
        }
    }
    check_flags(c);                                    // (also: everything on the ctx stream is over)
    fd.finish();
    if (sites) *sites = total_sites;
    if (bytes) *bytes = fd.total;
}

}  // namespace
}  // namespace scs

extern "C" {

int scs_set_site_support(scs_ctx* c, int on, uint32_t min_reads) { return guarded(c, [&] { support_set(c, false, on, min_reads); }); }
int scs_set_site_support_ref(scs_ctx* c, int on, uint32_t min_reads) { return guarded(c, [&] { support_set(c, true, on, min_reads); }); }

int scs_site_support(scs_ctx* c, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr, uint32_t* counts,
                     uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    return guarded(c, [&] { support_into(c, false, "scs_site_support", rec, pos, ref, alt, na, ta, nr, tr, counts, cap, n, nullptr); });
}
int scs_site_support_ref(scs_ctx* c, uint32_t* ref_rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr, uint32_t* counts,
                         uint64_t cap, uint64_t* n, uint64_t unlifted[2]) {
    if (n) *n = 0;
    if (unlifted) unlifted[0] = unlifted[1] = 0;
    return guarded(c, [&] { support_into(c, true, "scs_site_support_ref", ref_rec, pos, ref, alt, na, ta, nr, tr, counts, cap, n, unlifted); });
}

int scs_write_site_support(scs_ctx* c, const char* path, int flags, uint64_t* sites, uint64_t* bytes) {
    return guarded(c, [&] { support_write(c, false, "scs_write_site_support", path, flags, sites, bytes); });
}
int scs_write_site_support_ref(scs_ctx* c, const char* path, int flags, uint64_t* sites, uint64_t* bytes) {
    return guarded(c, [&] { support_write(c, true, "scs_write_site_support_ref", path, flags, sites, bytes); });
}

int scs_site_support_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_support, launches, ms, units); }
int scs_site_support_ref_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_support, launches, ms, units); }
int scs_site_support_ref_step_time(const scs_ctx* c, int step, uint64_t* launches, double* ms, uint64_t* units) {
    if (step != 0 && step != 1) return SCS_EINVAL;
    return kernel_time_of(c, step ? &scs_ctx::tm_support_ref_gather : &scs_ctx::tm_support_ref_open, launches, ms, units);
}

}  // extern "C"
