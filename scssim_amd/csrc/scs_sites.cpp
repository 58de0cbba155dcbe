// scs_sites.cpp -- the artefact table (include/scssim_hip.h: scs_write_artefacts, scs_artefact_sites): one entry
// per (genome site, alternate base) that the amplification made, with the amplicons and reads that carry and that cover it, made
// on the device (scs_k_sites.hip) after scs_allocate_reads.  The genome is worked in slabs of genome indices; one counting pass over
// the amplicons sizes every slab's buffers, the largest slab sizes the call's.  Every buffer, stream and event of a call belongs to
// its SiteJob (scs_sitejob.h, shared with the site support table of scs_support.cpp) and goes with it: nothing of the call stays in
// the ctx but the kernels' times.
#include "scs_sitejob.h"

extern "C" {

int scs_artefact_sites(scs_ctx* c, uint32_t min_reads, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr,
                       uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    return guarded(c, [&] {
        if (!n) throw ScsError(SCS_EINVAL, "scs_artefact_sites: n is NULL");
        site_check(c, "scs_artefact_sites");
        SiteJob J(c, min_reads, false); const hipStream_t s = J.s;
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
                    if (rec) rec[o] = r.rec; if (pos) pos[o] = r.pos; if (ref) ref[o] = r.ref; if (alt) alt[o] = r.alt;
                    if (na) na[o] = r.na; if (ta) ta[o] = r.ta; if (nr) nr[o] = r.nr; if (tr) tr[o] = r.tr;
                }
            }
            total += kept;
        }
        *n = total;
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        if (cap < total) throw ScsError(SCS_EOVERFLOW, "scs_artefact_sites: " + std::to_string(total) + " sites, room for " + std::to_string(cap));
    });
}

int scs_write_artefacts(scs_ctx* c, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_write_artefacts: no path");
        if (flags & ~1) throw ScsError(SCS_EINVAL, "scs_write_artefacts: unknown flag");
        site_check(c, "scs_write_artefacts");
        const bool bgzf = (flags & 1) != 0;
        OutFile fd; fd.open("scs_write_artefacts", path, bgzf);
        SiteJob J(c, min_reads, true); const hipStream_t s = J.s; KernelTimer& tm = J.tm;
        std::vector<std::string> names; for (const auto& r : c->recs) names.push_back(r.name);
        fd.header(site_header(names, c->rec_len.data()));
        uint64_t n_sites = 0;
        if (J.max_e) J.em.open(s, bgzf);
        // Slab k: its sites and the text's size to the host (it sizes the output), emit pass (and BGZF over the text where it lies);
        // then the slab's bytes travel in pieces into the file (SiteOut)
        for (uint32_t k = 0; k < J.n_slabs; ++k) {
            if (!J.cnt[2 * k]) continue;                   // a slab without an edit has no site: nothing is launched for it
            J.make(k);
            const uint64_t t_n = J.h_n[0]; n_sites += (uint32_t)J.h_n[1];
            if (!t_n) continue;                            // (every site of the slab below min_reads)
            uint64_t n = 0;
            const char* made = J.em.make(s, tm, J.t, J.site_recs.as<SiteRec>(), J.offs.as<uint64_t>(), t_n, bgzf, J.scan_tmp.p, J.scan_bytes, "scs_write_artefacts: a slab's text exceeds 4 GB", &n);
            J.em.ship(fd, made, n);
        }
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        tm.add_units(n_sites); tm.collect();
        fd.finish();
        if (sites) *sites = n_sites;
        if (bytes) *bytes = fd.total;
    });
}

int scs_artefact_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_site, launches, ms, units); }

}  // extern "C"
