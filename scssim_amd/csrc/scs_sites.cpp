// scs_sites.cpp -- the artefact table (include/scssim_hip.h: scs_write_artefacts, scs_artefact_sites): one entry
// per (genome site, alternate base) that the amplification made, with the amplicons and reads that carry and that cover it, made
// on the device (scs_k_sites.hip) after scs_allocate_reads -- and the same table on the original reference (scs_write_artefacts_ref,
// scs_artefact_ref_sites): its entries lifted through the lift table and grouped by REFERENCE site, with the
// pieces of amplicons -- of every haplotype and copy -- that cover each (scs_k_sites_ref.hip).  The axis is worked in slabs of its
// indices; one counting pass over the amplicons sizes every slab's buffers (and finds the unlifted totals the reference table's
// header states), the largest slab sizes the call's.  The two tables differ in SiteJob's on_ref (scs_sitejob.h, shared with the site
// support table of scs_support.cpp), the header and the unlifted totals: each entry point has one body for both.  Every buffer,
// stream and event of a call belongs to its SiteJob and goes with it: nothing of the call stays in the ctx but the kernels' times.
#include "scs_sitejob.h"

namespace scs {
namespace {

// fn: the entry point's name, for the error texts; unlifted: the reference table's two totals (may be NULL; untouched when !on_ref)
void sites_into(scs_ctx* c, bool on_ref, const std::string& fn, uint32_t min_reads, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta,
                uint64_t* nr, uint64_t* tr, uint64_t cap, uint64_t* n, uint64_t* unlifted) {
    if (!n) throw ScsError(SCS_EINVAL, fn + ": n is NULL");
    site_check(c, fn.c_str(), on_ref);
    SiteJob J(c, min_reads, false, on_ref); const hipStream_t s = J.s;
    if (unlifted) { unlifted[0] = J.unlifted[0]; unlifted[1] = J.unlifted[1]; }
    std::vector<SiteRec> h;
    uint64_t total = 0;
    J.slabs([&](uint64_t e, uint64_t kept) {
        const uint64_t room = cap > total ? cap - total : 0, take = std::min(kept, room);
        if (take) {                                        // (the sites are packed in order: the first `take` of them are the ones there is room for)
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
    });
    *n = total;
    check_flags(c);                                        // (also: everything on the ctx stream is over)
    if (cap < total) throw ScsError(SCS_EOVERFLOW, fn + ": " + std::to_string(total) + " sites, room for " + std::to_string(cap));
}

void sites_write(scs_ctx* c, bool on_ref, const std::string& fn, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes, uint64_t* unlifted) {
    if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
    if (flags & ~1) throw ScsError(SCS_EINVAL, fn + ": unknown flag");
    site_check(c, fn.c_str(), on_ref);
    const bool bgzf = (flags & 1) != 0; const std::string too_large = fn + ": a slab's text exceeds 4 GB";
    OutFile fd; fd.open(fn, path, bgzf);
    SiteJob J(c, min_reads, true, on_ref); const hipStream_t s = J.s; KernelTimer& tm = J.tm;
    if (unlifted) { unlifted[0] = J.unlifted[0]; unlifted[1] = J.unlifted[1]; }
    if (on_ref) fd.header(site_ref_header(c->lift.ref_names, c->lift.ref_lens.data(), J.unlifted[0], J.unlifted[1]));   // (the counting pass is over: the unlifted totals are known)
    else { std::vector<std::string> names; for (const auto& r : c->recs) names.push_back(r.name); fd.header(site_header(names, c->rec_len.data())); }
    uint64_t n_sites = 0;
    if (J.max_e) J.em.open(s, bgzf);
    // A slab: its sites and the text's size to the host (it sizes the output), emit pass (and BGZF over the text where it lies);
    // then the slab's bytes travel in pieces into the file (SiteOut)
    J.slabs([&](uint64_t, uint64_t kept) {
        const uint64_t t_n = J.h_n[0]; n_sites += kept;
        if (!t_n) return;                                  // (every site of the slab below min_reads)
        uint64_t n = 0;
        const char* made = J.em.make(s, tm, J.t, J.site_recs.as<SiteRec>(), J.offs.as<uint64_t>(), t_n, bgzf, J.scan_tmp.p, J.scan_bytes, too_large.c_str(), &n);
        J.em.ship(fd, made, n);
    });
    check_flags(c);                                        // (also: everything on the ctx stream is over)
    tm.add_units(n_sites); tm.collect();
    fd.finish();
    if (sites) *sites = n_sites;
    if (bytes) *bytes = fd.total;
}

}  // namespace
}  // namespace scs

extern "C" {

int scs_artefact_sites(scs_ctx* c, uint32_t min_reads, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr,
                       uint64_t cap, uint64_t* n) {
    if (n) *n = 0;
    return guarded(c, [&] { sites_into(c, false, "scs_artefact_sites", min_reads, rec, pos, ref, alt, na, ta, nr, tr, cap, n, nullptr); });
}
int scs_artefact_ref_sites(scs_ctx* c, uint32_t min_reads, uint32_t* ref_rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr,
                           uint64_t cap, uint64_t* n, uint64_t unlifted[2]) {
    if (n) *n = 0;
    if (unlifted) unlifted[0] = unlifted[1] = 0;
    return guarded(c, [&] { sites_into(c, true, "scs_artefact_ref_sites", min_reads, ref_rec, pos, ref, alt, na, ta, nr, tr, cap, n, unlifted); });
}

int scs_write_artefacts(scs_ctx* c, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes) {
    return guarded(c, [&] { sites_write(c, false, "scs_write_artefacts", path, flags, min_reads, sites, bytes, nullptr); });
}
int scs_write_artefacts_ref(scs_ctx* c, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes, uint64_t unlifted[2]) {
    if (unlifted) unlifted[0] = unlifted[1] = 0;
    return guarded(c, [&] { sites_write(c, true, "scs_write_artefacts_ref", path, flags, min_reads, sites, bytes, unlifted); });
}

int scs_artefact_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_site, launches, ms, units); }
int scs_artefact_ref_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_site_ref, launches, ms, units); }

}  // extern "C"
