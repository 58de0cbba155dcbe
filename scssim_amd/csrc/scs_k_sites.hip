// scs_k_sites.hip -- gfx950 kernels of the artefact table (scs_write_artefacts / scs_artefact_sites): the edits
// of the full amplicons (amp_edits, scs_amp.h) grouped by genome site, with the amplicons and reads that carry and that cover each.
// The genome is worked in SLABS of S genome indices, so that nothing is sized by the job:
//   k_site_count   one pass over all amplicons: per slab the edit entries that fall in it and the amplicons that overlap it
//                  (summed per workgroup in LDS, then one atomic per slab touched).  It sizes every slab's buffers.
//   k_site_fill    per slab: every edit in it becomes (key = index << 2 | alt, reads), every amplicon that overlaps it its start,
//                  its end and its reads.  The order is free: a wave adds its total to the cursor once and its lanes write behind it.
//   (rocPRIM)      radix sort of the keys, the starts and the ends, each with the reads; 64-bit scans of the reads in start and end order
//   k_site_reduce  a thread per sorted entry; the one that opens a run makes the site (site_make, scs_site.h) and sizes its line
//   k_site_emit    the lines, by the windowed scheme of scs_emit.h (emit_windows), as k_amp_emit
//   k_site_compact the kept sites packed for the binary form
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_amp.h"
#include "scs_site.h"
#include "scs_site_load.h"
#include "scs_emit.h"
#include <rocprim/rocprim.hpp>

namespace scs {

// cnt[2 s]: edit entries in slab s; cnt[2 s + 1]: amplicons that overlap it.  Up to SITE_LDS_SLABS slabs are summed in LDS first
__global__ void __launch_bounds__(256) k_site_count(AmpArgs A, uint64_t S, uint32_t n_slabs, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t s_cnt[2u * SITE_LDS_SLABS];
    const bool lds = n_slabs <= SITE_LDS_SLABS;
    if (lds) for (uint32_t k = threadIdx.x; k < 2u * n_slabs; k += 256u) s_cnt[k] = 0u;
    __syncthreads();
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    AmpPlace p; AmpErrs e1, e2; uint32_t reads = 0;
    if (j < A.n && site_load(A, j, p, e1, e2, reads)) {
        auto add = [&](uint64_t slab, uint32_t which) {
            if (slab >= n_slabs) { atomicOr(A.flags, (uint32_t)FLAG_SITE); return; }
            if (lds) atomicAdd(&s_cnt[2u * (uint32_t)slab + which], 1u); else atomicAdd(&cnt[2u * slab + which], 1ull);
        };
        const uint64_t lo = (uint64_t)amp_lo(p);
        for (uint64_t s = lo / S; s <= (lo + p.len - 1u) / S; ++s) add(s, 1u);
        amp_edits(p, e1, e2, SiteGen{A.g}, [&](int64_t x, uint32_t, uint32_t) { add((uint64_t)x / S, 0u); });
    }
    __syncthreads();
    if (lds) for (uint32_t k = threadIdx.x; k < 2u * n_slabs; k += 256u) if (s_cnt[k]) atomicAdd(&cnt[k], (unsigned long long)s_cnt[k]);
}

// the slab [x0, x1): cur[0] / cur[1] are the cursors of the edit entries and of the amplicons (zeroed by the host per slab).
// Every lane of a wave takes every shuffle: no lane leaves early
__global__ void __launch_bounds__(256) k_site_fill(AmpArgs A, uint64_t x0, uint64_t x1, unsigned long long* __restrict__ cur, uint64_t cap_e, uint64_t cap_a,
                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ kreads, uint64_t* __restrict__ starts, uint64_t* __restrict__ ends,
                                                   uint32_t* __restrict__ areads) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x; const int lane = (int)(threadIdx.x & 63u);
    AmpPlace p; AmpErrs e1, e2; uint32_t reads = 0;
    const bool ok = j < A.n && site_load(A, j, p, e1, e2, reads);
    const uint64_t lo = ok ? (uint64_t)amp_lo(p) : 0ull;
    const bool over = ok && lo < x1 && lo + p.len > x0;
    uint32_t ne = 0;
    if (over) amp_edits(p, e1, e2, SiteGen{A.g}, [&](int64_t x, uint32_t, uint32_t) { if ((uint64_t)x >= x0 && (uint64_t)x < x1) ++ne; });
    const uint32_t in_e = wave_incl_scan(ne, lane), in_a = wave_incl_scan(over ? 1u : 0u, lane);
    const uint32_t tot_e = __shfl(in_e, 63), tot_a = __shfl(in_a, 63);
    unsigned long long base_e = 0, base_a = 0;
    if (lane == 63) { if (tot_e) base_e = atomicAdd(&cur[0], (unsigned long long)tot_e); if (tot_a) base_a = atomicAdd(&cur[1], (unsigned long long)tot_a); }
    base_e = __shfl(base_e, 63); base_a = __shfl(base_a, 63);
    if (!over) return;                                     // (the shuffles are over)
    const uint64_t ia = base_a + in_a - 1u;
    if (ia < cap_a) { starts[ia] = lo; ends[ia] = lo + p.len; areads[ia] = reads; } else atomicOr(A.flags, (uint32_t)FLAG_SITE);
    if (!ne) return;
    uint64_t w = base_e + in_e - ne;
    amp_edits(p, e1, e2, SiteGen{A.g}, [&](int64_t x, uint32_t, uint32_t alt) {
        if ((uint64_t)x < x0 || (uint64_t)x >= x1) return;
        if (w < cap_e && alt < 4u) { keys[w] = site_key((uint64_t)x, alt); kreads[w] = reads; } else atomicOr(A.flags, (uint32_t)FLAG_SITE);
        ++w;
    });
}

// the fill pass found what the counting pass counted (else the sorted arrays hold entries nobody wrote)
__global__ void k_site_check(const unsigned long long* __restrict__ cur, unsigned long long n_e, unsigned long long n_a, uint32_t* __restrict__ flags) {
    if (cur[0] != n_e || cur[1] != n_a) atomicOr(flags, (uint32_t)FLAG_SITE);
}

// entry i of the sorted keys: the head of a run makes its site and sizes its line (0: the site is not reported); the others are no site
__global__ void __launch_bounds__(256) k_site_reduce(SiteArgs T, SiteRec* __restrict__ recs, uint32_t* __restrict__ sizes, uint32_t* __restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= T.n) return;
    uint32_t size = 0, kept = 0;
    if (site_head(T.keys, i)) {
        const uint64_t x = site_key_x(T.keys[i]);
        SiteRec r;
        if (x >= T.rec_off[T.n_rec] || !site_make(T.keys, T.reads, T.n, i, T.starts, T.ps_start, T.ends, T.ps_end, T.m, T.rec_off, T.n_rec, T.g[x], r)) atomicOr(T.flags, (uint32_t)FLAG_SITE);
        else if (r.nr >= (uint64_t)T.min_reads) {
            TruthCount c; site_line(c, T.names + T.name_off[r.rec], T.name_off[r.rec + 1] - T.name_off[r.rec], r);
            size = (uint32_t)c.n; kept = 1u; recs[i] = r;
        }
    }
    sizes[i] = size; keep[i] = kept;
}

// one workgroup per 256 entries (emit_windows): the lanes whose entry is a reported site format its line.  counts (the site
// support table; else null): the line ends with the six counters of the entry's position
__global__ void __launch_bounds__(256) k_site_emit(SiteArgs T, const SiteRec* __restrict__ recs, const uint64_t* __restrict__ offs, uint32_t lds, char* __restrict__ out,
                                                   const uint32_t* __restrict__ site_pos, const uint32_t* __restrict__ counts) {
    extern __shared__ uint4 s_run4[];
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u, j = j0 + threadIdx.x;
    const EmitSpan sp = emit_span(offs, j0, j0 + 256u < T.n ? j0 + 256u : T.n);
    const bool ok = sp.my1 > sp.my0;
    SiteRec r; const char* name = nullptr; uint32_t name_len = 0;
    if (ok) { r = recs[j]; if (r.rec < T.n_rec) { name = T.names + T.name_off[r.rec]; name_len = T.name_off[r.rec + 1] - T.name_off[r.rec]; } }
    const uint32_t* cnt = ok && counts ? counts + 6ull * site_pos[j] : nullptr;
    emit_windows(s_run4, sp, ok, lds, out, T.flags, (uint32_t)FLAG_SITE, [&](WinOut& o) { site_line(o, name, name_len, r, cnt); });
}

// the reported sites packed in order: out[pos[i]] = recs[i] where keep[i] (pos: the exclusive scan of keep)
__global__ void __launch_bounds__(256) k_site_compact(const SiteRec* __restrict__ recs, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, uint64_t n, SiteRec* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n && keep[i]) out[pos[i]] = recs[i];
}

void launch_site_count(hipStream_t s, const AmpArgs& a, uint64_t slab, uint32_t n_slabs, unsigned long long* cnt) {
    if (a.n == 0 || n_slabs == 0) return;
    hipLaunchKernelGGL(k_site_count, dim3(cdiv(a.n, 256)), dim3(256), 0, s, a, slab, n_slabs, cnt);
    note_launch(hipGetLastError());
}
void launch_site_fill(hipStream_t s, const AmpArgs& a, uint64_t x0, uint64_t x1, unsigned long long* cur, uint64_t cap_e, uint64_t cap_a,
                      uint64_t* keys, uint32_t* kreads, uint64_t* starts, uint64_t* ends, uint32_t* areads) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_site_fill, dim3(cdiv(a.n, 256)), dim3(256), 0, s, a, x0, x1, cur, cap_e, cap_a, keys, kreads, starts, ends, areads);
    note_launch(hipGetLastError());
}
void launch_site_check(hipStream_t s, const unsigned long long* cur, uint64_t n_e, uint64_t n_a, uint32_t* flags) {
    hipLaunchKernelGGL(k_site_check, dim3(1), dim3(1), 0, s, cur, (unsigned long long)n_e, (unsigned long long)n_a, flags);
    note_launch(hipGetLastError());
}
size_t site_sort_temp_bytes(size_t n) {
    size_t b = 0; (void)rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 64);
    return b + 256;
}
void launch_site_sort(hipStream_t s, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n, unsigned end_bit, void* temp, size_t temp_bytes) {
    if (n) note_launch(rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, s));
}
void launch_site_reduce(hipStream_t s, const SiteArgs& t, SiteRec* recs, uint32_t* sizes, uint32_t* keep) {
    if (t.n == 0) return;
    hipLaunchKernelGGL(k_site_reduce, dim3(cdiv(t.n, 256)), dim3(256), 0, s, t, recs, sizes, keep);
    note_launch(hipGetLastError());
}
void launch_site_emit(hipStream_t s, const SiteArgs& t, const SiteRec* recs, const uint64_t* offs, uint32_t lds, char* out, const uint32_t* site_pos, const uint32_t* counts) {
    if (t.n == 0) return;
    hipLaunchKernelGGL(k_site_emit, dim3(cdiv(t.n, 256)), dim3(256), SITE_LDS, s, t, recs, offs, emit_windows_lds(lds, SITE_LDS), out, site_pos, counts);
    note_launch(hipGetLastError());
}
void launch_site_compact(hipStream_t s, const SiteRec* recs, const uint32_t* keep, const uint32_t* pos, uint64_t n, SiteRec* out) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_site_compact, dim3(cdiv(n, 256)), dim3(256), 0, s, recs, keep, pos, n, out);
    note_launch(hipGetLastError());
}

}  // namespace scs
