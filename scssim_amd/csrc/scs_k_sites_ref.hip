// scs_k_sites_ref.hip -- gfx950 kernels of the artefact table on the original reference (scs_write_artefacts_ref /
// scs_artefact_ref_sites): the edits of the full amplicons lifted through the lift table and grouped by
// reference site (scs_site_ref.h).  The REFERENCE is worked in slabs of S reference indices, so that nothing is sized by the job:
//   k_site_ref_count   one pass over all amplicons, a thread each: one bisection for the amplicon's first segment, then a cursor
//                      that only moves forward.  Every R piece counts in every slab it overlaps, every edit in an R segment in
//                      its slab (summed per workgroup in LDS, then one atomic per slab touched); an edit in an I segment counts
//                      in the two unlifted totals.  It sizes every slab's buffers.
//   k_site_ref_fill    per slab with an entry: the same walk twice -- first the lane's entries and pieces in the slab are counted,
//                      a wave adds its totals to the two cursors once, then the lanes write behind the wave's base: (key, reads)
//                      per entry, (start, end, reads) per piece.  No per-lane arrays: a lane's piece count has no bound.
//   (scs_k_sites.hip)  the radix sorts, the cursor check, the LDS-window emit pass and the compaction are the artefact table's
//   k_site_ref_reduce  a thread per sorted entry; the one that opens a run makes the site (site_ref_make) and sizes its line
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_amp.h"
#include "scs_site_ref.h"
#include "scs_site_load.h"

namespace scs {

namespace {

// why a walk gave up, as a flag: the amplicon (or an edit of it) is not where it should be; the table or the reference is left
__device__ void site_ref_raise(uint32_t* flags, int err) {
    if (err) atomicOr(flags, (uint32_t)(err == LIFT_EPLACE ? FLAG_SITE : FLAG_LIFT));
}

}  // namespace

// cnt[2 s]: entries that lift into slab s; cnt[2 s + 1]: pieces that overlap it; cnt[2 n_slabs], cnt[2 n_slabs + 1]: the entries
// without a reference coordinate and their amplicons' reads.  Up to SITE_LDS_SLABS slabs are summed in LDS first
// A walk that gives up raises its flag; what it had added before stays in cnt -- the host checks the flags behind this pass and
// fails the call before any count is used
__global__ void __launch_bounds__(256) k_site_ref_count(AmpArgs A, SiteRefView V, uint64_t S, uint32_t n_slabs, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t s_cnt[2u * SITE_LDS_SLABS];
    const bool lds = n_slabs <= SITE_LDS_SLABS;
    if (lds) for (uint32_t k = threadIdx.x; k < 2u * n_slabs; k += 256u) s_cnt[k] = 0u;
    __syncthreads();
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    AmpPlace p; AmpErrs e1, e2; uint32_t reads = 0, rec = 0;
    if (j < A.n && site_load(A, j, p, e1, e2, reads, rec)) {
        auto add = [&](uint64_t slab, uint32_t which) {
            if (slab >= n_slabs) { atomicOr(A.flags, (uint32_t)FLAG_SITE); return; }
            if (lds) atomicAdd(&s_cnt[2u * (uint32_t)slab + which], 1u); else atomicAdd(&cnt[2u * slab + which], 1ull);
        };
        uint32_t unl = 0;
        const int err = site_ref_amp(V, (uint64_t)amp_lo(p), p.len, A.rec_off[rec], A.rec_off[rec + 1],
            [&](auto f) { amp_edits(p, e1, e2, SiteGen{A.g}, f); },
            [&](uint64_t x0, uint64_t x1) { for (uint64_t s = x0 / S; s <= (x1 - 1u) / S; ++s) add(s, 1u); },
            [&](uint64_t x, uint32_t, uint32_t) { add(x / S, 0u); },
            [&] { ++unl; });
        site_ref_raise(A.flags, err);
        if (unl) { atomicAdd(&cnt[2ull * n_slabs], (unsigned long long)unl); atomicAdd(&cnt[2ull * n_slabs + 1u], (unsigned long long)unl * reads); }
    }
    __syncthreads();
    if (lds) for (uint32_t k = threadIdx.x; k < 2u * n_slabs; k += 256u) if (s_cnt[k]) atomicAdd(&cnt[k], (unsigned long long)s_cnt[k]);
}

// the slab [x0, x1) of the reference: cur[0] / cur[1] are the cursors of the entries and of the pieces (zeroed by the host per
// slab).  Every lane of a wave takes every shuffle: no lane leaves early
__global__ void __launch_bounds__(256) k_site_ref_fill(AmpArgs A, SiteRefView V, uint64_t x0, uint64_t x1, unsigned long long* __restrict__ cur, uint64_t cap_e, uint64_t cap_p,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ kreads, uint64_t* __restrict__ starts, uint64_t* __restrict__ ends,
                                                       uint32_t* __restrict__ preads) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x; const int lane = (int)(threadIdx.x & 63u);
    AmpPlace p; AmpErrs e1, e2; uint32_t reads = 0, rec = 0;
    const bool ok = j < A.n && site_load(A, j, p, e1, e2, reads, rec);
    const uint64_t lo = ok ? (uint64_t)amp_lo(p) : 0ull;
    uint32_t ne = 0, np = 0;
    if (ok) {
        const int err = site_ref_amp(V, lo, p.len, A.rec_off[rec], A.rec_off[rec + 1],
            [&](auto f) { amp_edits(p, e1, e2, SiteGen{A.g}, f); },
            [&](uint64_t a, uint64_t b) { if (a < x1 && b > x0) ++np; },
            [&](uint64_t x, uint32_t, uint32_t) { if (x >= x0 && x < x1) ++ne; },
            [] {});
        if (err) { site_ref_raise(A.flags, err); ne = np = 0; }
    }
    const uint32_t in_e = wave_incl_scan(ne, lane), in_p = wave_incl_scan(np, lane);
    const uint32_t tot_e = __shfl(in_e, 63), tot_p = __shfl(in_p, 63);
    unsigned long long base_e = 0, base_p = 0;
    if (lane == 63) { if (tot_e) base_e = atomicAdd(&cur[0], (unsigned long long)tot_e); if (tot_p) base_p = atomicAdd(&cur[1], (unsigned long long)tot_p); }
    base_e = __shfl(base_e, 63); base_p = __shfl(base_p, 63);
    if (!ne && !np) return;                                // (the shuffles are over)
    uint64_t we = base_e + in_e - ne, wp = base_p + in_p - np;
    const uint64_t end_e = we + ne, end_p = wp + np;
    (void)site_ref_amp(V, lo, p.len, A.rec_off[rec], A.rec_off[rec + 1],
        [&](auto f) { amp_edits(p, e1, e2, SiteGen{A.g}, f); },
        [&](uint64_t a, uint64_t b) {
            if (!(a < x1 && b > x0)) return;
            if (wp < end_p && wp < cap_p) { starts[wp] = a; ends[wp] = b; preads[wp] = reads; } else atomicOr(A.flags, (uint32_t)FLAG_SITE);
            ++wp;
        },
        [&](uint64_t x, uint32_t ref, uint32_t alt) {
            if (x < x0 || x >= x1) return;
            if (we < end_e && we < cap_e && alt < 4u) { keys[we] = site_ref_key(x, ref, alt); kreads[we] = reads; } else atomicOr(A.flags, (uint32_t)FLAG_SITE);
            ++we;
        },
        [] {});
    if (we != end_e || wp != end_p) atomicOr(A.flags, (uint32_t)FLAG_SITE);   // (the two walks of one lane disagree)
}

// entry i of the sorted keys: the head of a run makes its site and sizes its line (0: the site is not reported); the others are no
// site.  T.rec_off / T.n_rec / T.names: the REFERENCE records'
__global__ void __launch_bounds__(256) k_site_ref_reduce(SiteArgs T, SiteRec* __restrict__ recs, uint32_t* __restrict__ sizes, uint32_t* __restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= T.n) return;
    uint32_t size = 0, kept = 0;
    if (site_head(T.keys, i)) {
        SiteRec r;
        if (!site_ref_make(T.keys, T.reads, T.n, i, T.starts, T.ps_start, T.ends, T.ps_end, T.m, T.rec_off, T.n_rec, r)) atomicOr(T.flags, (uint32_t)FLAG_SITE);
        else if (r.nr >= (uint64_t)T.min_reads) {
            TruthCount c; site_line(c, T.names + T.name_off[r.rec], T.name_off[r.rec + 1] - T.name_off[r.rec], r);
            size = (uint32_t)c.n; kept = 1u; recs[i] = r;
        }
    }
    sizes[i] = size; keep[i] = kept;
}

void launch_site_ref_count(hipStream_t s, const AmpArgs& a, const SiteRefView& v, uint64_t slab, uint32_t n_slabs, unsigned long long* cnt) {
    if (a.n == 0 || n_slabs == 0) return;
    hipLaunchKernelGGL(k_site_ref_count, dim3(cdiv(a.n, 256)), dim3(256), 0, s, a, v, slab, n_slabs, cnt);
    note_launch(hipGetLastError());
}
void launch_site_ref_fill(hipStream_t s, const AmpArgs& a, const SiteRefView& v, uint64_t x0, uint64_t x1, unsigned long long* cur, uint64_t cap_e, uint64_t cap_p,
                          uint64_t* keys, uint32_t* kreads, uint64_t* starts, uint64_t* ends, uint32_t* preads) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_site_ref_fill, dim3(cdiv(a.n, 256)), dim3(256), 0, s, a, v, x0, x1, cur, cap_e, cap_p, keys, kreads, starts, ends, preads);
    note_launch(hipGetLastError());
}
void launch_site_ref_reduce(hipStream_t s, const SiteArgs& t, SiteRec* recs, uint32_t* sizes, uint32_t* keep) {
    if (t.n == 0) return;
    hipLaunchKernelGGL(k_site_ref_reduce, dim3(cdiv(t.n, 256)), dim3(256), 0, s, t, recs, sizes, keep);
    note_launch(hipGetLastError());
}

}  // namespace scs
