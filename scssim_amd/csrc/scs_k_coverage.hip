// scs_k_coverage.hip -- gfx950 kernels of the coverage profile (scs_set_coverage): per-base depth of the staged
// genome as a difference array that every batch's reads mark, and at the end of the job one prefix sum over it with the histogram
// per record made on the way.  No FASTQ text is read; the byte genome only for its N bases.
//
// k_cov_mark, per batch: a thread per pair places its reads (for_each_placed_read, scs_place.h: the truth passes' placement) and
// adds +1 / -1 at the ends of their aligned runs (cov_read, scs_coverage.h) with int32 atomics whose result nobody reads (the
// no-return form).  A read without indel events is two atomics.  Plain global atomics: whether a workgroup-level window in LDS pays
// is a measurement, not made here.
//
// End of the job, three plain kernels over tiles of COV_TILE entries -- no workgroup ever waits for another one:
//   k_cov_tile_sums     a workgroup per tile, 16-byte loads, one int32 sum per tile
//   k_cov_tile_offsets  ONE workgroup walks the tile sums in chunks of COV_CHUNK with a carry: every tile's depth at its first entry
//   k_cov_scan_hist     a workgroup per tile loads the differences again (four strips of 1024: a thread owns four neighbours per
//                       strip), scans them (wave scan, the four waves through LDS, the strips by a carry), stores the depths in
//                       place and counts them: the bases of the record the tile begins in into an LDS histogram (a thread adds
//                       once per run of equal depth among its neighbours), flushed with one 64-bit atomic per used bucket; depths
//                       beyond the LDS table and bases behind a record border inside the tile go to memory directly.  N bases are
//                       in no bucket; the three sums per record go by wave reduction, one atomic per wave.
// The array is padded with zeros to whole tiles, so no load needs a bound.  A negative depth, or one that is not 0 at or behind entry
// G, raises FLAG_COVERAGE: the differences were not those of intervals.  Buckets are indexed by the clamped depth only.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_coverage.h"

namespace scs {

__global__ void __launch_bounds__(256) k_cov_mark(CovArgs A) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= A.np) return;
    for_each_placed_read(A, pi, (uint32_t)FLAG_COVERAGE, [&](const PairRec&, uint32_t, const TruthAln& a, int, uint32_t, int64_t r0, int64_t r1) {
        if (a.lo < r0 || a.hi >= r1) { atomicOr(A.flags, (uint32_t)FLAG_COVERAGE); return; }   // outside its record: the call fails
        cov_read(a, [&](int64_t g, int d) {
            if (g < r0 || g > r1) { atomicOr(A.flags, (uint32_t)FLAG_COVERAGE); return; }       // (r1 <= G: entry G exists)
            atomicAdd(A.diff + g, d);
        });
    });
}

void launch_cov_mark(hipStream_t s, const CovArgs& a) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_cov_mark, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a);
    note_launch(hipGetLastError());
}

__global__ void __launch_bounds__(256) k_cov_tile_sums(const int32_t* __restrict__ diff, int32_t* __restrict__ sums) {
    __shared__ uint32_t s_w[4];
    const int4* p = (const int4*)(diff + (uint64_t)blockIdx.x * COV_TILE);
    uint32_t t = 0;
#pragma unroll
    for (uint32_t j = 0; j < COV_TILE / 1024u; ++j) { const int4 v = p[j * 256u + threadIdx.x]; t += (uint32_t)v.x + (uint32_t)v.y + (uint32_t)v.z + (uint32_t)v.w; }
    t = wave_sum(t);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0u) sums[blockIdx.x] = (int32_t)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
}

// offs[i] = sums[0] + .. + sums[i - 1]: one workgroup, COV_CHUNK sums per step (four per thread), the steps joined by a carry
__global__ void __launch_bounds__(256) k_cov_tile_offsets(const int32_t* __restrict__ sums, int32_t* __restrict__ offs, uint64_t n) {
    __shared__ uint32_t s_w[4];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < n; base += COV_CHUNK) {
        const uint64_t i = base + threadIdx.x * 4u;
        uint32_t v[4], t = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) { v[e] = i + e < n ? (uint32_t)sums[i + e] : 0u; t += v[e]; }
        const uint32_t incl = block_scan_put(t, s_w);
        __syncthreads();
        uint32_t tot, ex = carry + block_scan_get(incl, t, s_w, tot);
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) if (i + e < n) { offs[i + e] = (int32_t)ex; ex += v[e]; }
        carry += tot;
        __syncthreads();                                   // (s_w is written again in the next step)
    }
}

__global__ void __launch_bounds__(256) k_cov_scan_hist(CovFinish F) {
    __shared__ uint32_t s_hist[COV_LDS_BUCKETS];
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, D = F.max_depth, nl = F.lds;
    const uint64_t base = (uint64_t)blockIdx.x * COV_TILE, G = F.n_bases;
    for (uint32_t i = tid; i < nl; i += 256u) s_hist[i] = 0u;
    // the record the tile begins in: its bases use the LDS table and the per-thread sums; the others of the tile go to memory
    const uint32_t r_t = rec_of(F.rec_off, F.n_rec, (int64_t)base);
    const uint64_t r_end = F.rec_off[r_t + 1];
    unsigned long long* const row = F.hist + (uint64_t)r_t * (D + 1u);
    uint32_t carry = (uint32_t)F.tile_offs[blockIdx.x];
    unsigned long long t_n = 0, t_sum = 0, t_sum_n = 0; bool bad = false;
    auto flush = [&](uint32_t b, uint32_t n) {
        if (!n) return;
        if (b < nl) atomicAdd(&s_hist[b], n); else atomicAdd(row + b, (unsigned long long)n);
    };
    __syncthreads();
    for (uint32_t j = 0; j < COV_TILE / 1024u; ++j) {
        const uint64_t i0 = base + j * 1024u + tid * 4u;
        const int4 d = *(const int4*)(F.diff + i0);
        uint32_t p[4]; p[0] = (uint32_t)d.x; p[1] = p[0] + (uint32_t)d.y; p[2] = p[1] + (uint32_t)d.z; p[3] = p[2] + (uint32_t)d.w;
        const uint32_t incl = block_scan_put(p[3], s_w);
        __syncthreads();
        uint32_t tot; const uint32_t ex = carry + block_scan_get(incl, p[3], s_w, tot);
        carry += tot;
        __syncthreads();                                   // (s_w is written again in the next strip)
        int32_t v[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) v[e] = (int32_t)(ex + p[e]);
        *(int4*)(F.diff + i0) = make_int4(v[0], v[1], v[2], v[3]);   // the depths, where their differences lay (non-negative, or the call fails)
        const uint32_t cw = codes4(F.codes, i0, G);
        uint32_t run_b = 0xFFFFFFFFu, run_n = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const uint64_t i = i0 + e;
            if (v[e] < 0) bad = true;
            if (i >= G) { if (v[e] != 0) bad = true; continue; }   // entry G closes the array at 0; behind it lies padding
            const uint32_t dep = v[e] < 0 ? 0u : (uint32_t)v[e], b = dep < D ? dep : D;
            const bool is_n = ((cw >> (8u * e)) & 0xFFu) >= 4u;
            if (i < r_end) {
                if (is_n) { ++t_n; t_sum_n += dep; continue; }
                t_sum += dep;
                if (b == run_b) ++run_n; else { flush(run_b, run_n); run_b = b; run_n = 1u; }
            } else {                                       // behind a record border inside the tile: under its own record
                const uint32_t r = rec_of(F.rec_off, F.n_rec, (int64_t)i);
                if (is_n) { atomicAdd(F.n_n + r, 1ull); if (dep) atomicAdd(F.sum_n + r, (unsigned long long)dep); }
                else { atomicAdd(F.hist + (uint64_t)r * (D + 1u) + b, 1ull); if (dep) atomicAdd(F.sum + r, (unsigned long long)dep); }
            }
        }
        flush(run_b, run_n);
    }
    t_n = wave_sum_u64(t_n); t_sum = wave_sum_u64(t_sum); t_sum_n = wave_sum_u64(t_sum_n);
    if (lane == 0u) {
        if (t_n) atomicAdd(F.n_n + r_t, t_n);
        if (t_sum) atomicAdd(F.sum + r_t, t_sum);
        if (t_sum_n) atomicAdd(F.sum_n + r_t, t_sum_n);
    }
    if (bad) atomicOr(F.flags, (uint32_t)FLAG_COVERAGE);
    __syncthreads();
    for (uint32_t i = tid; i < nl; i += 256u) if (s_hist[i]) atomicAdd(row + i, (unsigned long long)s_hist[i]);
}

uint64_t cov_tiles(uint64_t n_bases) { return (n_bases + 1u + COV_TILE - 1u) / COV_TILE; }

void launch_cov_finish(hipStream_t s, const CovFinish& f) {
    const uint64_t nt = cov_tiles(f.n_bases);
    if (f.n_rec == 0 || nt > 0x7FFFFFFFull) { note_launch(hipErrorInvalidValue); return; }
    CovFinish g = f; g.lds = cov_lds_buckets(f.lds, f.max_depth);
    hipLaunchKernelGGL(k_cov_tile_sums, dim3((uint32_t)nt), dim3(256), 0, s, (const int32_t*)f.diff, f.tile_sums);
    note_launch(hipGetLastError());
    hipLaunchKernelGGL(k_cov_tile_offsets, dim3(1), dim3(256), 0, s, (const int32_t*)f.tile_sums, f.tile_offs, nt);
    note_launch(hipGetLastError());
    hipLaunchKernelGGL(k_cov_scan_hist, dim3((uint32_t)nt), dim3(256), 0, s, g);
    note_launch(hipGetLastError());
}

}  // namespace scs
