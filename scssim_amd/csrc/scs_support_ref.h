// scs_support_ref.h -- the site support table on the ORIGINAL REFERENCE (scs_set_site_support_ref): the
// reference positions X of the artefact table on the reference (scs_site_ref.h) expanded to every staged index g that lifts to one
// of them, and the staged counters of a yield call (scs_support.h) summed back by X.  X = ref_off[ref_rec] + ref_pos as there; a
// staged index g of R segment s lifts to X(g) = ref_off[s.ref_rec] + s.ref_pos + (g - s.hap_off).  The segments ascend in hap_off
// and inside an R segment g rises with X, so the listed positions inside a segment are one run [a, a + n) of the ascending list
// x[]: two bisections per segment, a scan over the segments' counts, and one output slot per staged position -- no walk, no sort.
// One definition for the kernels (scs_k_support_ref.hip) and the host probe (scs_support_ref_probe), so the test seam runs the code
// the kernels run.
#pragma once
#include <stdint.h>
#include "scs_common.h"
#include "scs_site.h"
#include "scs_lift.h"
#include "scs_support.h"

namespace scs {

// the lift table, the staged records' starts (n_rec + 1), the reference records' (n_ref + 1) and the listed reference positions
// (ascending, distinct)
struct SupportRefView { const LiftSeg* segs; uint32_t n_seg; const uint64_t* rec_off; uint32_t n_rec; const uint64_t* ref_off; uint32_t n_ref; const uint64_t* x; uint64_t n_x; };

// Segment si, checked as site_ref_seek checks the segment it enters -- it follows the one before it without a gap, holds a base,
// stays inside one staged record and, if R, inside its reference record -- and the listed positions inside it: x[a .. a + n).
// An I segment holds none.  Returns a LiftErr
SCS_HD int support_ref_range(const SupportRefView& V, uint32_t si, uint64_t& a, uint32_t& n) {
    a = 0; n = 0;
    const LiftSeg s = V.segs[si];
    const uint64_t before = si ? V.segs[si - 1u].hap_off + V.segs[si - 1u].len : 0ull;
    if (s.len == 0 || s.hap_off + s.len < s.hap_off || s.hap_off != before) return LIFT_ETABLE;
    if (V.n_rec == 0 || s.hap_off >= V.rec_off[V.n_rec]) return LIFT_ETABLE;
    if (s.hap_off + s.len > V.rec_off[rec_of(V.rec_off, V.n_rec, s.hap_off) + 1u]) return LIFT_ETABLE;
    if (s.kind != 0u) return LIFT_OK;
    if (s.ref_rec >= V.n_ref || s.ref_pos + s.len < s.ref_pos || s.ref_pos + s.len > V.ref_off[s.ref_rec + 1u] - V.ref_off[s.ref_rec]) return LIFT_EREF;
    const uint64_t x0 = V.ref_off[s.ref_rec] + s.ref_pos;
    a = support_first_ge(V.x, V.n_x, x0);
    n = (uint32_t)(support_first_ge(V.x, V.n_x, x0 + s.len) - a);   // (at most n_x <= SUPPORT_MAX_POS)
    return LIFT_OK;
}

// Output slot t < off[n_seg] (off: the exclusive scan of the segments' counts, seg_a: their a): the staged index g and the index
// xi of its reference position.  false: the slot is not where the segments say (never an index outside x[] or the segment)
SCS_HD bool support_ref_slot(const SupportRefView& V, const uint64_t* off, const uint64_t* seg_a, uint64_t t, uint64_t& g, uint32_t& xi) {
    const uint32_t si = (uint32_t)(site_rank_le(off, V.n_seg, t) - 1u);   // the last segment that starts at or before t: off[0] = 0
    const LiftSeg s = V.segs[si];
    const uint64_t i = seg_a[si] + (t - off[si]);
    g = 0; xi = 0;
    if (t >= off[si + 1u] || i >= V.n_x || s.kind != 0u || s.ref_rec >= V.n_ref) return false;
    const uint64_t x0 = V.ref_off[s.ref_rec] + s.ref_pos;
    if (V.x[i] < x0 || V.x[i] - x0 >= s.len) return false;
    g = s.hap_off + (V.x[i] - x0); xi = (uint32_t)i;
    return true;
}
// slot t as the fill pass writes it: and the slot before it lies at a smaller staged index -- found from the segments again, not
// from what another lane is writing.  support_read's bisection needs the ascending order
SCS_HD bool support_ref_fill(const SupportRefView& V, const uint64_t* off, const uint64_t* seg_a, uint64_t t, uint64_t& g, uint32_t& xi) {
    if (!support_ref_slot(V, off, seg_a, t, g, xi)) return false;
    if (t == 0) return true;
    uint64_t gp; uint32_t xp;
    return support_ref_slot(V, off, seg_a, t - 1u, gp, xp) && gp < g;
}

// Staged position t adds its non-zero counters to those of its reference position xi.  add(k, v) adds v to reference counter k and
// returns what it held before (the device's atomicAdd).  false: a counter passed 2^32 - 1
template <class Add>
SCS_HD bool support_ref_gather(const uint32_t* cnt, uint64_t t, uint32_t xi, Add add) {
    bool ok = true;
    for (uint32_t k = 0; k < 6u; ++k) {
        const uint32_t v = cnt[6ull * t + k];
        if (v && add(6ull * xi + k, v) > 0xFFFFFFFFu - v) ok = false;
    }
    return ok;
}

// ---- host-only
// The expansion and the gather as the device works them (scs_support_ref_probe; no GPU, no ctx): the range pass over every segment,
// the scan, the fill pass `chunk` slots at a time, then -- g_cnt: six counters per staged index of the whole genome, or NULL -- the
// gather.  SCS_EINVAL with *why = a LiftErr (2: a segment that does not follow the last, holds no base or leaves its staged record;
// 3: one past its reference record), 4: listed positions that do not ascend or lie outside the reference, 5: staged positions
// that do not ascend, 6: a counter past 2^32 - 1
inline int support_ref_probe(const LiftSeg* segs, uint32_t n_seg, const uint64_t* hap_len, uint32_t n_hap, const uint64_t* ref_len, uint32_t n_ref,
                             const uint64_t* x, uint64_t n_x, uint64_t chunk, const uint32_t* g_cnt,
                             std::vector<uint64_t>& sp_pos, std::vector<uint32_t>& sp_pos_x, std::vector<uint32_t>& ref_cnt, int* why) {
    if (why) *why = 0;
    sp_pos.clear(); sp_pos_x.clear(); ref_cnt.assign(6 * (size_t)n_x, 0u);
    if (!segs || !n_seg || !hap_len || !n_hap || !ref_len || !n_ref || (n_x && !x) || !chunk) return SCS_EINVAL;
    std::vector<uint64_t> rec_off(n_hap + 1, 0), ref_off(n_ref + 1, 0);
    for (uint32_t r = 0; r < n_hap; ++r) rec_off[r + 1] = rec_off[r] + hap_len[r];
    for (uint32_t r = 0; r < n_ref; ++r) { if (ref_len[r] >> 58) return SCS_EINVAL; ref_off[r + 1] = ref_off[r] + ref_len[r]; if (ref_off[r + 1] >> 58) return SCS_EINVAL; }
    auto fail = [&](int w) { if (why) *why = w; return SCS_EINVAL; };
    for (uint64_t i = 0; i < n_x; ++i) if (x[i] >= ref_off[n_ref] || (i && x[i - 1] >= x[i])) return fail(4);
    if (n_x > 0x1FFFFFFFull) return SCS_EOVERFLOW;
    const SupportRefView V{segs, n_seg, rec_off.data(), n_hap, ref_off.data(), n_ref, x, n_x};
    std::vector<uint64_t> seg_a(n_seg), off(n_seg + 1, 0);
    for (uint32_t si = 0; si < n_seg; ++si) {
        uint32_t n = 0;
        const int err = support_ref_range(V, si, seg_a[si], n);
        if (err) return fail(err);
        off[si + 1] = off[si] + n;
    }
    const uint64_t total = off[n_seg];
    if (total > 0x1FFFFFFFull) return SCS_EOVERFLOW;
    sp_pos.assign(total, 0); sp_pos_x.assign(total, 0);
    for (uint64_t t0 = 0; t0 < total; t0 += std::min(chunk, total - t0))
        for (uint64_t t = t0; t < t0 + std::min(chunk, total - t0); ++t) if (!support_ref_fill(V, off.data(), seg_a.data(), t, sp_pos[t], sp_pos_x[t])) return fail(5);
    if (g_cnt)
        for (uint64_t t = 0; t < total; ++t)
            if (!support_ref_gather(g_cnt + 6 * sp_pos[t], 0, sp_pos_x[t], [&](uint64_t k, uint32_t v) { const uint32_t was = ref_cnt[k]; ref_cnt[k] = was + v; return was; })) return fail(6);
    return SCS_OK;
}

}  // namespace scs
