// scs_support.cpp -- the site support table (include/scssim_hip.h: scs_set_site_support, scs_site_support, scs_write_site_support;
// DESIGN.md section 15): the artefact table's sites (scs_sites.cpp) with what the reads of a yield call show at their coordinates.
// The sites are made on the device at the start of the yield call (support_open: the artefact table's SiteJob, slab by slab, its
// packed sites appended to a ctx-owned array that never visits the host), the counters per batch (scs_k_support.hip, launched from
// scs_reads.cpp), the file afterwards from both.  The sites, their positions and the counters belong to the ctx and go with
// scs_set_site_support(ctx, 0, ..); what a write call needs beyond them belongs to the call and goes with it.
#include "scs_sitejob.h"

namespace scs {

namespace {
const uint64_t kSupportChunk = 1ull << 20;                 // sites per turn of the emit and read-out loops: no buffer of theirs is sized by the job

void support_release(scs_ctx* c) {
    c->sp_sites.release(); c->sp_site_pos.release(); c->sp_pos.release(); c->sp_cnt.release(); c->sp_tab.release();
    c->tm_support.ev.clear(); c->tm_support.used = 0; c->tm_support.reset();
    c->sp_n_sites = c->sp_n_pos = 0; c->support_valid = false;
}
void support_ready(scs_ctx* c, const char* fn) {
    if (!c->support_on || !c->support_valid) throw ScsError(SCS_EINVAL, std::string(fn) + ": no yield call with the site support on (scs_set_site_support) has finished");
}
}  // namespace

void support_check(scs_ctx* c) {
    if (!c->support_on) return;
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, "site support (scs_set_site_support): not available for a sharded job (shard_count > 1); turn it off with scs_set_site_support(ctx, 0, 0)");
}

// The call's site table: the artefact table's slabs, each slab's reported sites packed and appended; then the distinct coordinates
// (head flags, the library's scan, a scatter) and this call's counters, zeroed on the ctx stream
void support_open(scs_ctx* c) {
    const hipStream_t s = c->stream;
    c->sp_n_sites = c->sp_n_pos = 0;
    uint64_t n = 0;
    {
        SiteJob J(c, c->support_min_reads, false);
        J.slabs([&](uint64_t e, uint64_t kept) {
            if (!kept) return;
            if (n + kept > 3ull * SUPPORT_MAX_POS) throw ScsError(SCS_EOVERFLOW, "site support (scs_set_site_support): more than 2^29 - 1 distinct positions; raise min_reads");
            J.compact(e, kept);
            c->sp_sites.reserve((n + kept) * sizeof(SiteRec), s, n * sizeof(SiteRec));
            HIP_OK(hipMemcpyAsync(c->sp_sites.as<SiteRec>() + n, J.packed.p, kept * sizeof(SiteRec), hipMemcpyDeviceToDevice, s));
            n += kept;
        });
        // the record starts for the kernels of this call (the job's own table goes with it)
        const std::vector<uint64_t> roff = record_starts(c);
        upload(c->sp_tab, roff, s); HIP_OK(hipStreamSynchronize(s));
    }
    uint32_t n_pos = 0;
    if (n) {
        DevBuf head, e, tmp; const size_t tb = scan_temp_bytes(n);
        head.reserve((n + 1) * 4, s); e.reserve((n + 1) * 4, s); tmp.reserve(tb, s);
        c->sp_site_pos.reserve(n * 4, s);
        launch_support_heads(s, c->sp_sites.as<SiteRec>(), n, c->sp_tab.as<uint64_t>(), (uint32_t)c->recs.size(), head.as<uint32_t>(), c->flags.as<uint32_t>());
        exclusive_scan_u32(s, head.as<uint32_t>(), e.as<uint32_t>(), n, tmp.p, tb);
        HIP_OK(hipMemcpyAsync(&n_pos, e.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        if (n_pos > SUPPORT_MAX_POS) throw ScsError(SCS_EOVERFLOW, "site support (scs_set_site_support): " + std::to_string(n_pos) + " distinct positions, more than 2^29 - 1; raise min_reads");
        c->sp_pos.reserve(std::max<size_t>((size_t)n_pos * 8, 16), s);
        launch_support_scatter(s, c->sp_sites.as<SiteRec>(), n, c->sp_tab.as<uint64_t>(), head.as<uint32_t>(), e.as<uint32_t>(), c->sp_pos.as<uint64_t>(), c->sp_site_pos.as<uint32_t>());
        HIP_OK(hipStreamSynchronize(s));                                           // (head, e and tmp go)
    }
    const size_t cb = std::max<size_t>((size_t)n_pos * 24, 16);
    c->sp_cnt.reserve(cb, s); HIP_OK(hipMemsetAsync(c->sp_cnt.p, 0, cb, s));
    check_flags(c);
    c->sp_n_sites = n; c->sp_n_pos = n_pos;
}

}  // namespace scs

extern "C" {

int scs_set_site_support(scs_ctx* c, int on, uint32_t min_reads) {
    return guarded(c, [&] {
        HIP_OK(hipStreamSynchronize(c->stream));                                   // the last call's table and counters go: nothing may still read them
        support_release(c);
        c->support_on = on != 0; c->support_min_reads = on ? min_reads : 0;
    });
}

int scs_site_support(scs_ctx* c, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr, uint32_t* counts,
                     uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    return guarded(c, [&] {
        if (!n) throw ScsError(SCS_EINVAL, "scs_site_support: n is NULL");
        support_ready(c, "scs_site_support");
        const hipStream_t s = c->stream; const uint64_t total = c->sp_n_sites;
        *n = total;
        HIP_OK(hipStreamSynchronize(s));
        if (cap < total) throw ScsError(SCS_EOVERFLOW, "scs_site_support: " + std::to_string(total) + " sites, room for " + std::to_string(cap));
        std::vector<SiteRec> h; std::vector<uint32_t> sp, cn;
        for (uint64_t first = 0; first < total; first += kSupportChunk) {
            const uint64_t m = std::min(kSupportChunk, total - first);
            h.resize(m); sp.resize(m);
            HIP_OK(hipMemcpyAsync(h.data(), c->sp_sites.as<SiteRec>() + first, m * sizeof(SiteRec), hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(sp.data(), c->sp_site_pos.as<uint32_t>() + first, m * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
            const uint32_t p0 = sp[0], p1 = sp[m - 1];     // (the sites' positions ascend: the chunk's counters are one run)
            if (p1 < p0 || p1 >= c->sp_n_pos) throw ScsError(SCS_EDEVICE, "scs_site_support: the sites' positions are not in order");
            if (counts) { cn.resize(6 * (size_t)(p1 - p0 + 1)); HIP_OK(hipMemcpyAsync(cn.data(), c->sp_cnt.as<uint32_t>() + 6 * (size_t)p0, cn.size() * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s)); }
            for (uint64_t i = 0; i < m; ++i) {
                const SiteRec& r = h[i]; const uint64_t o = first + i;
                if (rec) rec[o] = r.rec; if (pos) pos[o] = r.pos; if (ref) ref[o] = r.ref; if (alt) alt[o] = r.alt;
                if (na) na[o] = r.na; if (ta) ta[o] = r.ta; if (nr) nr[o] = r.nr; if (tr) tr[o] = r.tr;
                if (counts) { if (sp[i] < p0 || sp[i] > p1) throw ScsError(SCS_EDEVICE, "scs_site_support: the sites' positions are not in order"); memcpy(counts + 6 * o, cn.data() + 6 * (size_t)(sp[i] - p0), 24); }
            }
        }
    });
}

int scs_write_site_support(scs_ctx* c, const char* path, int flags, uint64_t* sites, uint64_t* bytes) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_write_site_support: no path");
        if (flags & ~1) throw ScsError(SCS_EINVAL, "scs_write_site_support: unknown flag");
        support_ready(c, "scs_write_site_support");
        const bool bgzf = (flags & 1) != 0; const hipStream_t s = c->stream; const uint64_t total_sites = c->sp_n_sites;
        OutFile fd; fd.open("scs_write_site_support", path, bgzf);
        std::vector<std::string> names; for (const auto& r : c->recs) names.push_back(r.name);
        fd.header(site_header(names, c->rec_len.data(), true));
        // what the call needs beyond the ctx's arrays belongs to it: the record table, a chunk's line sizes and offsets, the emitter.
        // The struct's destructor ends every way out: both streams drained, then the members release themselves
        struct Call { hipStream_t s; RecTable rt; SiteOut em; DevBuf sizes, offs, scan; Pinned<uint64_t> h_n; Event ev_n; KernelTimer idle{"k_sites"};
                      ~Call() { (void)hipStreamSynchronize(s); } } W{s};
        W.idle.on = false;
        if (total_sites) {
            const uint64_t cm = std::min(kSupportChunk, total_sites); const size_t sb = scan_temp_bytes(cm);
            W.rt.make(c, s); W.em.open(s, bgzf);
            W.sizes.reserve((cm + 1) * 4, s); W.offs.reserve((cm + 1) * 8, s); W.scan.reserve(sb, s);
            W.h_n.reserve(64, hipHostMallocDefault); W.ev_n.ensure(hipEventDisableTiming | hipEventBlockingSync);
            SiteArgs t{}; t.rec_off = W.rt.rec_off; t.name_off = W.rt.name_off; t.names = W.rt.names; t.n_rec = W.rt.n_rec; t.flags = c->flags.as<uint32_t>();
            for (uint64_t first = 0; first < total_sites; first += kSupportChunk) {
                t.n = std::min(kSupportChunk, total_sites - first);
                const SiteRec* recs = c->sp_sites.as<SiteRec>() + first; const uint32_t* sp = c->sp_site_pos.as<uint32_t>() + first;
                launch_support_size(s, t, recs, sp, c->sp_cnt.as<uint32_t>(), W.sizes.as<uint32_t>());
                exclusive_scan_u32_to_u64(s, W.sizes.as<uint32_t>(), W.offs.as<uint64_t>(), t.n, W.scan.p, sb);
                HIP_OK(hipMemcpyAsync(W.h_n, W.offs.as<uint64_t>() + t.n, 8, hipMemcpyDeviceToHost, s));
                HIP_OK(hipEventRecord(W.ev_n, s)); HIP_OK(hipEventSynchronize(W.ev_n));
                { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("site support: the sizing pass failed: ") + hipGetErrorString(le)); }
                const uint64_t t_n = W.h_n[0]; uint64_t nb = 0;
                const char* made = W.em.make(s, W.idle, t, recs, W.offs.as<uint64_t>(), t_n, bgzf, W.scan.p, sb, "scs_write_site_support: a chunk's text exceeds 4 GB", &nb, sp, c->sp_cnt.as<uint32_t>());
                W.em.ship(fd, made, nb);
            }
        }
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        fd.finish();
        if (sites) *sites = total_sites;
        if (bytes) *bytes = fd.total;
    });
}

int scs_site_support_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_support, launches, ms, units); }

}  // extern "C"
