// scs_sites_ref.cpp -- the artefact table on the original reference (include/scssim_hip.h: scs_write_artefacts_ref,
// scs_artefact_ref_sites): the artefact table's entries lifted through the lift table and grouped by REFERENCE
// site, with the pieces of amplicons -- of every haplotype and copy -- that cover each, made on the device (scs_k_sites_ref.hip) after
// scs_allocate_reads.  The reference is worked in slabs of reference indices; one counting pass over the amplicons sizes every
// slab's buffers and finds the unlifted totals the header states.  The sorts, the scans, the emit pass, BGZF and the shipping of the
// bytes are the artefact table's (scs_k_sites.hip, SiteOut in scs_sitejob.h), called as they are, and the call's job object is the
// artefact table's SiteJob with on_ref set (scs_sitejob.h): one definition of the buffers' sizing and of a slab's passes.  Every
// buffer, stream and event of a call belongs to its SiteJob and goes with it: nothing of the call stays in the ctx but the
// kernels' times.
#include "scs_sitejob.h"

namespace scs {
namespace {

void site_ref_check(scs_ctx* c, const char* fn) {
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, std::string(fn) + ": not available for a sharded job (shard_count > 1)");
    if (!c->have_lift) throw ScsError(SCS_EINVAL, std::string(fn) + ": the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
    if (!c->allocated) throw ScsError(SCS_EINVAL, std::string(fn) + ": call scs_allocate_reads first (the table states every site's read support)");
}

}  // namespace
}  // namespace scs

extern "C" {

int scs_artefact_ref_sites(scs_ctx* c, uint32_t min_reads, uint32_t* ref_rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr,
                           uint64_t cap, uint64_t* n, uint64_t unlifted[2]) {
    if (n) *n = 0;
    if (unlifted) unlifted[0] = unlifted[1] = 0;
    return guarded(c, [&] {
        if (!n) throw ScsError(SCS_EINVAL, "scs_artefact_ref_sites: n is NULL");
        site_ref_check(c, "scs_artefact_ref_sites");
        SiteJob J(c, min_reads, false, true); const hipStream_t s = J.s;
        if (unlifted) { unlifted[0] = J.unlifted[0]; unlifted[1] = J.unlifted[1]; }
        std::vector<SiteRec> h;
        uint64_t total = 0;
        for (uint32_t k = 0; k < J.n_slabs; ++k) {
            if (!J.cnt[2 * k]) continue;
            const uint64_t e = J.make(k), kept = (uint32_t)J.h_n[1];
            const uint64_t room = cap > total ? cap - total : 0, take = std::min(kept, room);
            if (take) {                                    // (the sites are packed in order: the first `take` of them are the ones there is room for)
                J.compact(e, kept);
                h.resize(take);
                HIP_OK(hipMemcpyAsync(h.data(), J.packed.p, take * sizeof(SiteRec), hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
                for (uint64_t i = 0; i < take; ++i) {
                    const SiteRec& r = h[i]; const uint64_t o = total + i;
                    if (ref_rec) ref_rec[o] = r.rec; if (pos) pos[o] = r.pos; if (ref) ref[o] = r.ref; if (alt) alt[o] = r.alt;
                    if (na) na[o] = r.na; if (ta) ta[o] = r.ta; if (nr) nr[o] = r.nr; if (tr) tr[o] = r.tr;
                }
            }
            total += kept;
        }
        *n = total;
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        if (cap < total) throw ScsError(SCS_EOVERFLOW, "scs_artefact_ref_sites: " + std::to_string(total) + " sites, room for " + std::to_string(cap));
    });
}

int scs_write_artefacts_ref(scs_ctx* c, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes, uint64_t unlifted[2]) {
    if (unlifted) unlifted[0] = unlifted[1] = 0;
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_write_artefacts_ref: no path");
        if (flags & ~1) throw ScsError(SCS_EINVAL, "scs_write_artefacts_ref: unknown flag");
        site_ref_check(c, "scs_write_artefacts_ref");
        const bool bgzf = (flags & 1) != 0;
        OutFile fd; fd.open("scs_write_artefacts_ref", path, bgzf);
        SiteJob J(c, min_reads, true, true); const hipStream_t s = J.s; KernelTimer& tm = J.tm;
        if (unlifted) { unlifted[0] = J.unlifted[0]; unlifted[1] = J.unlifted[1]; }
        fd.header(site_ref_header(c->lift.ref_names, c->lift.ref_lens.data(), J.unlifted[0], J.unlifted[1]));   // (the counting pass is over: the unlifted totals are known)
        uint64_t n_sites = 0;
        if (J.max_e) J.em.open(s, bgzf);
        for (uint32_t k = 0; k < J.n_slabs; ++k) {
            if (!J.cnt[2 * k]) continue;                   // a slab without an entry has no site: nothing is launched for it
            J.make(k);
            const uint64_t t_n = J.h_n[0]; n_sites += (uint32_t)J.h_n[1];
            if (!t_n) continue;                            // (every site of the slab below min_reads)
            uint64_t n = 0;
            const char* made = J.em.make(s, tm, J.t, J.site_recs.as<SiteRec>(), J.offs.as<uint64_t>(), t_n, bgzf, J.scan_tmp.p, J.scan_bytes, "scs_write_artefacts_ref: a slab's text exceeds 4 GB", &n);
            J.em.ship(fd, made, n);
        }
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        tm.add_units(n_sites); tm.collect();
        fd.finish();
        if (sites) *sites = n_sites;
        if (bytes) *bytes = fd.total;
    });
}

int scs_artefact_ref_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_site_ref, launches, ms, units); }

// host-only: the table's body (flags & 1: behind its header) through the functions its kernels run (site_ref_probe, scs_site_ref.h)
int scs_artefact_ref_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                           const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                           const uint64_t* hap_len, uint32_t n_hap, const char* genome, uint64_t genome_len,
                           const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                           const uint64_t* ref_len, const char* const* ref_names, uint32_t n_ref,
                           uint32_t min_reads, uint64_t slab, int flags, char* out, size_t cap, size_t* n_out, uint64_t unlifted[2], int* lift_err) {
    if (!n_out || !ref_names || !n_ref || !ref_len || (flags & ~1) || !n_seg || !seg_hap_off || !seg_len || !seg_ref_pos || !seg_ref_rec || !seg_kind) return SCS_EINVAL;
    std::vector<std::string> names;
    for (uint32_t r = 0; r < n_ref; ++r) { if (!ref_names[r]) return SCS_EINVAL; names.push_back(ref_names[r]); }
    std::vector<LiftSeg> segs(n_seg);
    for (uint32_t i = 0; i < n_seg; ++i) segs[i] = LiftSeg{seg_hap_off[i], seg_len[i], seg_ref_pos[i], seg_ref_rec[i], seg_kind[i]};
    std::string body; uint64_t unl[2] = {0, 0};
    const int rc = site_ref_probe(amp_start, amp_len, amp_reads, n_amp, ed_amp, ed_x, ed_alt, n_ed, hap_len, n_hap, genome, genome_len, segs.data(), n_seg, ref_len, names,
                                  min_reads, slab ? slab : kSiteSlab, body, unl, lift_err);
    if (unlifted) { unlifted[0] = unl[0]; unlifted[1] = unl[1]; }
    if (rc) return rc;
    if (flags & 1) body = site_ref_header(names, ref_len, unl[0], unl[1]) + body;
    *n_out = body.size();
    if (out) { if (body.size() > cap) return SCS_EOVERFLOW; memcpy(out, body.data(), body.size()); }
    return SCS_OK;
}

}  // extern "C"
