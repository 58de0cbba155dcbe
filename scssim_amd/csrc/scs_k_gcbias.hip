// scs_k_gcbias.hip -- gfx950 kernel of the GC-bias table (scs_gc_bias): one pass over the per-base depths the
// coverage profile leaves on the device (scs_k_coverage.hip) and the genome's codes gives, per record, for every GC bin of the
// sliding windows of W bases the number of windows and the sum of their depths.  Both arrays are only read.
//
// k_gc_bias, a workgroup of 256 per tile of COV_TILE window starts; no workgroup ever waits for another one:
//   scan     the tile's entries and the W - 1 behind them (the halo) in strips of 1024, a thread four neighbours per strip: depths by
//            16-byte loads, codes as one uint32 per four bases.  Two exclusive prefix sums in LDS: the depths in 64 bits (a window of
//            1024 bases at a depth above 2^22 does not fit 32), and G/C count | N count << 16 in one uint32 (tile plus halo is at most
//            5119 bases).  Wave scan, the four waves through LDS, the strips by a carry.  Entries at or behind n_bases count as 0 and
//            are not loaded: no load reaches outside the arrays.
//   windows  a thread owns four neighbouring starts per strip; a window's three quantities are two LDS reads each.  The windows of
//            the record the tile begins in add to an LDS table of GCB_BINS x (count, 64-bit sum); neighbouring windows differ by at
//            most one in gc, so a thread adds once per run of equal bin among its four.  A start behind a record border inside the tile
//            bisects its own record and adds to memory.  A start whose window would pass its record's end adds nothing: windows never
//            cross a record border, and a halo is never read past the record's end.
//   flush    one 64-bit atomic per non-zero table entry; n_windows by wave reduction, one atomic per wave.
// The bin comes from a clamped count (gcb_bin), so no input can index outside a row.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_truth.h"
#include "scs_coverage.h"
#include "scs_gcbias.h"

namespace scs {

#define GCB_STRIP 1024u
#define GCB_ENTRIES (COV_TILE + GCB_MAX_WINDOW)            // 5120: tile plus the widest halo, rounded up to whole strips

__global__ void __launch_bounds__(256) k_gc_bias(GcBiasArgs A) {
    __shared__ unsigned long long s_pd[GCB_ENTRIES + 1u];  // s_pd[k] = the depths of the tile's entries before k
    __shared__ uint32_t s_pc[GCB_ENTRIES + 1u];            // ... their G/C bases | their N bases << 16
    __shared__ unsigned long long s_sum[GCB_BINS];
    __shared__ uint32_t s_cnt[GCB_BINS];
    __shared__ unsigned long long s_wd[4];
    __shared__ uint32_t s_wc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, W = A.window;
    const uint64_t base = (uint64_t)blockIdx.x * COV_TILE, G = A.n_bases;
    const uint32_t n_ent = COV_TILE + W - 1u, strips = (n_ent + GCB_STRIP - 1u) / GCB_STRIP;   // 4 (W = 1) or 5
    for (uint32_t i = tid; i < GCB_BINS; i += 256u) { s_sum[i] = 0ull; s_cnt[i] = 0u; }
    if (tid == 0u) { s_pd[0] = 0ull; s_pc[0] = 0u; }
    // ---- scan
    unsigned long long carry_d = 0; uint32_t carry_c = 0;
    for (uint32_t j = 0; j < strips; ++j) {
        const uint32_t k0 = j * GCB_STRIP + tid * 4u;
        const uint64_t i0 = base + k0;
        uint32_t d[4] = {0u, 0u, 0u, 0u}, cw = 0x04040404u;
        if (k0 < n_ent && i0 < G) {                        // (entries the tile's windows never reach stay 0 and unread)
            const uint4 v = *(const uint4*)(A.depth + i0);                         // (i0 < n_bases and both are within depth_alloc, a multiple of 4 as i0 is: the launcher checks it)
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            if (i0 + 4u <= G) cw = *(const uint32_t*)(A.codes + i0);
            else { cw = 0u; for (uint32_t e = 0; e < 4u; ++e) if (i0 + e < G) cw |= (uint32_t)A.codes[i0 + e] << (8u * e); }
        }
        unsigned long long pd[4]; uint32_t pc[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const bool in = k0 + e < n_ent && i0 + e < G;
            const uint32_t c = (cw >> (8u * e)) & 0xFFu;
            const unsigned long long de = in ? (unsigned long long)d[e] : 0ull;
            const uint32_t ce = in ? (c >= 4u ? 0x10000u : (is_gc(c) ? 1u : 0u)) : 0u;
            pd[e] = (e ? pd[e - 1u] : 0ull) + de; pc[e] = (e ? pc[e - 1u] : 0u) + ce;
        }
        const unsigned long long incl_d = wave_incl_scan_u64(pd[3], (int)lane);
        const uint32_t incl_c = wave_incl_scan(pc[3], (int)lane);
        if (lane == 63u) { s_wd[wave] = incl_d; s_wc[wave] = incl_c; }
        __syncthreads();
        unsigned long long ex_d = carry_d + incl_d - pd[3]; uint32_t ex_c = carry_c + incl_c - pc[3];
        for (uint32_t w = 0; w < wave; ++w) { ex_d += s_wd[w]; ex_c += s_wc[w]; }
        carry_d += s_wd[0] + s_wd[1] + s_wd[2] + s_wd[3]; carry_c += s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) { s_pd[k0 + e + 1u] = ex_d + pd[e]; s_pc[k0 + e + 1u] = ex_c + pc[e]; }
        __syncthreads();                                   // (s_wd, s_wc are written again in the next strip; behind the last one the prefixes stand)
    }
    // ---- windows.  The record the tile begins in uses the LDS table and the per-thread count; the others of the tile go to memory
    const uint32_t r_t = rec_of(A.rec_off, A.n_rec, (int64_t)base);
    const uint64_t r_end = A.rec_off[r_t + 1u];
    unsigned long long* const row_w = A.windows + (uint64_t)r_t * GCB_BINS;
    unsigned long long* const row_s = A.depth_sum + (uint64_t)r_t * GCB_BINS;
    const bool lds = A.lds != 0u;
    unsigned long long t_n = 0;
    auto flush = [&](uint32_t b, uint32_t n, unsigned long long sum) {
        if (!n) return;
        if (lds) { atomicAdd(&s_cnt[b], n); if (sum) atomicAdd(&s_sum[b], sum); }
        else { atomicAdd(row_w + b, (unsigned long long)n); if (sum) atomicAdd(row_s + b, sum); }
    };
    for (uint32_t j = 0; j < COV_TILE / GCB_STRIP; ++j) {
        const uint32_t k0 = j * GCB_STRIP + tid * 4u;
        uint32_t run_b = 0u, run_n = 0u; unsigned long long run_s = 0ull;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const uint32_t k = k0 + e;
            const uint64_t p = base + k;
            if (p >= G) continue;
            const bool own = p < r_end;
            uint32_t r = r_t; uint64_t end = r_end;
            if (!own) { r = rec_of(A.rec_off, A.n_rec, (int64_t)p); end = A.rec_off[r + 1u]; }
            if (p + W > end) continue;                     // the window would pass its record's end (so k + W <= n_ent, and every entry of it lies before n_bases)
            const uint32_t c = s_pc[k + W] - s_pc[k];      // (both halves ascend: no borrow from one into the other)
            const unsigned long long ds = s_pd[k + W] - s_pd[k];
            if (c >> 16) {                                 // an N in the window: counted, and in nothing else
                if (own) ++t_n; else atomicAdd(A.n_windows + r, 1ull);
                continue;
            }
            const uint32_t b = gcb_bin(c & 0xFFFFu, W);
            if (!own) { atomicAdd(A.windows + (uint64_t)r * GCB_BINS + b, 1ull); if (ds) atomicAdd(A.depth_sum + (uint64_t)r * GCB_BINS + b, ds); continue; }
            if (run_n && b == run_b) { ++run_n; run_s += ds; }
            else { flush(run_b, run_n, run_s); run_b = b; run_n = 1u; run_s = ds; }
        }
        flush(run_b, run_n, run_s);
    }
    t_n = wave_sum_u64(t_n);
    if (lane == 0u && t_n) atomicAdd(A.n_windows + r_t, t_n);
    if (!lds) return;                                      // (uniform: the whole workgroup leaves)
    __syncthreads();
    for (uint32_t i = tid; i < GCB_BINS; i += 256u) {
        if (s_cnt[i]) atomicAdd(row_w + i, (unsigned long long)s_cnt[i]);
        if (s_sum[i]) atomicAdd(row_s + i, s_sum[i]);
    }
}

void launch_gc_bias(hipStream_t s, const GcBiasArgs& a) {
    const uint64_t nt = (a.n_bases + COV_TILE - 1u) / COV_TILE;                   // (tiles of window starts: entry n_bases starts no window)
    if (a.n_rec == 0 || a.window < 1u || a.window > GCB_MAX_WINDOW || nt > 0x7FFFFFFFull || (a.depth_alloc & 3u) || a.depth_alloc < a.n_bases) { note_launch(hipErrorInvalidValue); return; }
    if (!nt) return;
    hipLaunchKernelGGL(k_gc_bias, dim3((uint32_t)nt), dim3(256), 0, s, a);
    note_launch(hipGetLastError());
}

}  // namespace scs
