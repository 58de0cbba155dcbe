// scs_k_support_ref.hip -- gfx950 kernels of the site support table on the original reference (scs_set_site_support_ref; DESIGN.md
// section 19; scs_support_ref.h): the listed reference positions expanded to the staged positions k_support counts at, and the
// staged counters summed back by reference position.
//   k_support_ref_ranges  a thread per segment of the lift table: the segment checked, two bisections of the listed positions for
//                         the run that lies inside it.  The library's scan over the counts gives every segment's first output slot
//   k_support_ref_fill    a thread per output slot [t0, t0 + n): one bisection of the segments' offsets, then its staged index and
//                         the index of its reference position.  The work is one thread per staged position whatever the segments'
//                         sizes; the output ascends, which support_read's bisection needs (every slot checks the one before it
//                         from the segments, not from memory another lane writes)
//   k_support_ref_gather  after the last batch, a thread per staged position: its non-zero counters added to its reference
//                         position's (at most a few copies share one: no aggregation); the atomic's return value tells a counter
//                         that passed 2^32 - 1
// The batches between the two run k_support (scs_k_support.hip) over the staged positions, unchanged.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_support_ref.h"

namespace scs {

__global__ void __launch_bounds__(256) k_support_ref_ranges(SupportRefView V, uint64_t* __restrict__ seg_a, uint32_t* __restrict__ seg_n, uint32_t* __restrict__ flags) {
    const uint64_t si = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (si >= V.n_seg) return;
    uint64_t a = 0; uint32_t n = 0;
    if (support_ref_range(V, (uint32_t)si, a, n)) { atomicOr(flags, (uint32_t)FLAG_LIFT); a = 0; n = 0u; }   // (the host fails the call before a slot is filled)
    seg_a[si] = a; seg_n[si] = n;
}

__global__ void __launch_bounds__(256) k_support_ref_fill(SupportRefView V, const uint64_t* __restrict__ off, const uint64_t* __restrict__ seg_a, uint64_t t0, uint64_t n, uint64_t total,
                                                          uint64_t* __restrict__ sp_pos, uint32_t* __restrict__ sp_pos_x, uint32_t* __restrict__ flags) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x, t = t0 + k;
    if (k >= n || t >= total) return;
    uint64_t g = 0; uint32_t xi = 0;
    if (!support_ref_fill(V, off, seg_a, t, g, xi)) atomicOr(flags, (uint32_t)FLAG_SUPPORT);
    sp_pos[t] = g; sp_pos_x[t] = xi;
}

__global__ void __launch_bounds__(256) k_support_ref_gather(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ sp_pos_x, uint64_t n, uint64_t n_x,
                                                            uint32_t* __restrict__ ref_cnt, uint32_t* __restrict__ flags) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const uint32_t xi = sp_pos_x[t];
    if (xi >= n_x) { atomicOr(flags, (uint32_t)FLAG_SUPPORT); return; }
    if (!support_ref_gather(cnt, t, xi, [&](uint64_t k, uint32_t v) { return atomicAdd(&ref_cnt[k], v); })) atomicOr(flags, (uint32_t)FLAG_SUPPORT);
}

void launch_support_ref_ranges(hipStream_t s, const SupportRefView& v, uint64_t* seg_a, uint32_t* seg_n, uint32_t* flags) {
    if (v.n_seg == 0) return;
    hipLaunchKernelGGL(k_support_ref_ranges, dim3(cdiv(v.n_seg, 256)), dim3(256), 0, s, v, seg_a, seg_n, flags);
    note_launch(hipGetLastError());
}
void launch_support_ref_fill(hipStream_t s, const SupportRefView& v, const uint64_t* off, const uint64_t* seg_a, uint64_t t0, uint64_t n, uint64_t total, uint64_t* sp_pos, uint32_t* sp_pos_x, uint32_t* flags) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_support_ref_fill, dim3(cdiv(n, 256)), dim3(256), 0, s, v, off, seg_a, t0, n, total, sp_pos, sp_pos_x, flags);
    note_launch(hipGetLastError());
}
void launch_support_ref_gather(hipStream_t s, const uint32_t* cnt, const uint32_t* sp_pos_x, uint64_t n, uint64_t n_x, uint32_t* ref_cnt, uint32_t* flags) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_support_ref_gather, dim3(cdiv(n, 256)), dim3(256), 0, s, cnt, sp_pos_x, n, n_x, ref_cnt, flags);
    note_launch(hipGetLastError());
}

}  // namespace scs
