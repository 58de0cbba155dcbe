// scs_site_load.h -- device only: how the kernels of the two artefact tables (scs_k_sites.hip, scs_k_sites_ref.hip) resolve one full
// amplicon of the list.  Every kernel file is its own translation unit; this is the one definition both include.
#pragma once
#include "scs_device.h"
#include "scs_amp.h"
#include "scs_site.h"

namespace scs {

struct SiteGen { const uint8_t* g; __device__ uint32_t operator()(int64_t x) const { return g[x]; } };

// amplicon first + j: its index map, its two error lists, its reads, its staged record.  false: it cannot be placed (FLAG_SITE: a
// lineage that does not fit its parents, flags that are not a strand, an amplicon outside its record) -- amp_load's checks
// (scs_k_amplicons.hip)
__device__ inline bool site_load(const AmpArgs& A, uint32_t j, AmpPlace& p, AmpErrs& e1, AmpErrs& e2, uint32_t& reads, uint32_t& rec) {
    const uint32_t i = A.first + j;
    const uint32_t fsl = A.fulls.sl[i], sm = A.fulls.parent[i], ssl = A.semis.sl[sm], f = A.semis.parent[sm];
    if (!amp_resolve(A.fr.goff[f], A.fr.len[f], A.fr.strand[f], sl_spos(ssl), sl_len(ssl), sl_spos(fsl), sl_len(fsl), p) || !amp_strand(p)) { atomicOr(A.flags, (uint32_t)FLAG_SITE); return false; }
    const int64_t x0 = amp_lo(p);
    if (x0 < 0 || (uint64_t)x0 >= A.rec_off[A.n_rec]) { atomicOr(A.flags, (uint32_t)FLAG_SITE); return false; }
    const uint32_t r = rec_of(A.rec_off, A.n_rec, x0);
    if ((uint64_t)x0 < A.rec_off[r] || (uint64_t)x0 + p.len > A.rec_off[r + 1]) { atomicOr(A.flags, (uint32_t)FLAG_SITE); return false; }   // a fragment never straddles records
    rec = r;
    reads = A.read_numbers[i];
    e1 = AmpErrs{A.semis.errs[sm], A.spool}; e2 = AmpErrs{A.fulls.errs[i], A.fpool};
    return true;
}
__device__ inline bool site_load(const AmpArgs& A, uint32_t j, AmpPlace& p, AmpErrs& e1, AmpErrs& e2, uint32_t& reads) {
    uint32_t rec = 0;
    return site_load(A, j, p, e1, e2, reads, rec);
}

}  // namespace scs
