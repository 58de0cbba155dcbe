// scs_k_runs.hip -- gfx950 kernels of the run-length text of a per-base uint32 array (the bedGraph files of the coverage work:
// scs_write_coverage_bedgraph, scs_write_coverage_ref_bedgraph, scs_write_copy_number_ref).  One line per
// maximal run of equal masked value inside a record (runs_line, scs_runs.h).  A RUN START is a record's first base or a base whose
// masked value differs from its left neighbour's; a line belongs to the tile its run starts in and ends at the next run start,
// wherever that lies.  Wave64, 256 lanes, a workgroup per tile of COV_TILE entries: the arrays are padded to whole tiles, so no
// load of the values needs a bound; entries at or behind n are no bases and start nothing.
//
// What every per-tile kernel does first (runs_lane): a lane owns RUNS_LANE = 16 neighbouring entries, four 16-byte loads of one
// 64-byte line, masked and put into LDS (17 words per lane, an odd stride: no bank conflict among the 32 lanes an access is
// served in); the entry left of the tile is the last word of one more 16-byte load by lane 0.  The record of the tile's first entry is one bisection; an entry behind a record
// border inside the tile that does not differ from its neighbour is bisected on its own (it starts a run where it starts a record:
// equal values on both sides of a border are two runs).  The lanes' 16 start bits lie side by side in LDS as 64 words of 64 bits,
// where a lane finds the next run start behind its own entries by counting trailing zeros: no lane walks bases.
//   k_runs_first  per tile: the local index of its first run start (COV_TILE: none)
//   k_runs_next   ONE workgroup walks those words from the last tile to the first in chunks of 1024 (four per lane, a suffix
//                 minimum through the waves, the chunks joined by a carry): every tile's next run start BEHIND it, n where none --
//                 so a run over thousands of tiles (a centromere's N block at depth 0) costs its line one load
//   k_runs_size   per tile: its lines, and their bytes through the counting sink (the sizing pass of scs_emit.h)
//   k_runs_emit   per tile of a slab, after the 64-bit exclusive scan of the slab's tile bytes: the lanes' bytes are scanned in the
//                 workgroup (a lane's lines are neighbours in the text), then emit_windows formats into LDS and copies the window
//                 out in aligned 16-byte stores.  Lanes whose bytes differ from the sizing pass', or a tile whose total does,
//                 raise FLAG_RUNS; nothing is ever written outside the tile's [offs[t], offs[t + 1]).
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_truth.h"
#include "scs_coverage.h"
#include "scs_runs.h"
#include "scs_emit.h"

namespace scs {

static_assert(RUNS_LANE * 256u == COV_TILE && RUNS_LANE == 16u, "a lane's start bits are one uint16");
#define RUNS_VAL_WORDS (COV_TILE + 256u)                   // the tile's masked values in LDS, 17 words per lane
#define RUNS_NONE 0xFFFFFFFFFFFFFFFFull

// what a lane knows of its 16 entries: bit e of m = entry i0 + e starts a run; after = the first run start behind them (runs_lane
// with want_after, and only where m != 0); r_t, r_end: the record of the tile's first entry and where it ends
struct RunsLane { uint32_t m, r_t; uint64_t i0, after, r_end; };

__device__ __forceinline__ uint32_t runs_slot(uint32_t k) { return k + (k >> 4); }

// EVERY lane of the workgroup enters (two barriers).  s_val: RUNS_VAL_WORDS words, s_st: 256 uint16, 8-byte aligned
__device__ __forceinline__ RunsLane runs_lane(const RunsArgs& A, uint32_t tile, uint32_t* s_val, uint16_t* s_st, bool want_after) {
    const uint32_t tid = threadIdx.x, k0 = tid * RUNS_LANE;
    const uint64_t base = (uint64_t)tile * COV_TILE;
    RunsLane L; L.m = 0u; L.i0 = base + k0; L.after = A.n;
    const uint4* p = reinterpret_cast<const uint4*>(A.values + L.i0);
#pragma unroll
    for (uint32_t j = 0; j < RUNS_LANE / 4u; ++j) {
        const uint4 v = p[j]; const uint32_t at = runs_slot(k0) + 4u * j;
        s_val[at] = v.x & A.mask; s_val[at + 1u] = v.y & A.mask; s_val[at + 2u] = v.z & A.mask; s_val[at + 3u] = v.w & A.mask;
    }
    uint32_t prev = 0u;
    if (tid == 0u && base) prev = reinterpret_cast<const uint4*>(A.values + base - 4u)->w & A.mask;   // (entry 0 starts its record whatever lies left of it)
    L.r_t = rec_of(A.rec_off, A.n_rec, (int64_t)base);
    const uint64_t r_start = A.rec_off[L.r_t]; L.r_end = A.rec_off[L.r_t + 1u];
    __syncthreads();
    if (tid) prev = s_val[runs_slot(k0 - 1u)];
    for (uint32_t e = 0; e < RUNS_LANE; ++e) {
        const uint64_t i = L.i0 + e;
        if (i >= A.n) break;                               // padding: not a base
        const uint32_t cur = s_val[runs_slot(k0) + e];
        bool st = cur != prev || i == r_start;
        if (!st && i >= L.r_end) st = A.rec_off[rec_of(A.rec_off, A.n_rec, (int64_t)i)] == i;   // behind a record border inside the tile
        if (st) L.m |= 1u << e;
        prev = cur;
    }
    s_st[tid] = (uint16_t)L.m;
    __syncthreads();
    if (want_after && L.m) {
        const unsigned long long* bits = reinterpret_cast<const unsigned long long*>(s_st);
        const uint32_t at = k0 + RUNS_LANE;                // the first entry behind mine: bit at & 63 of word at >> 6
        L.after = A.next[tile];
        for (uint32_t w = at >> 6; w < COV_TILE / 64u; ++w) {
            unsigned long long x = bits[w];
            if (w == at >> 6) x &= ~0ull << (at & 63u);
            if (x) { L.after = base + w * 64u + (uint32_t)(__ffsll((long long)x) - 1); break; }
        }
    }
    return L;
}

// the lines of a lane's run starts, in order, through o
template <class Out>
__device__ __forceinline__ void runs_lane_lines(const RunsArgs& A, const RunsLane& L, const uint32_t* s_val, Out& o) {
    const uint32_t k0 = threadIdx.x * RUNS_LANE;
    uint32_t m = L.m;
    while (m) {
        const uint32_t e = (uint32_t)__ffs((int)m) - 1u; m &= m - 1u;
        const uint64_t i = L.i0 + e, end = m ? L.i0 + ((uint32_t)__ffs((int)m) - 1u) : L.after;
        const uint32_t r = i < L.r_end ? L.r_t : rec_of(A.rec_off, A.n_rec, (int64_t)i);
        const uint64_t r0 = A.rec_off[r];
        runs_line(o, A.names + A.name_off[r], A.name_off[r + 1u] - A.name_off[r], i - r0, end - r0, s_val[runs_slot(k0) + e]);
    }
}

__global__ void __launch_bounds__(256) k_runs_first(RunsArgs A) {
    __shared__ uint32_t s_val[RUNS_VAL_WORDS];
    __shared__ __attribute__((aligned(8))) uint16_t s_st[256];
    __shared__ uint32_t s_first;
    if (threadIdx.x == 0u) s_first = COV_TILE;
    const RunsLane L = runs_lane(A, blockIdx.x, s_val, s_st, false);
    if (L.m) atomicMin(&s_first, threadIdx.x * RUNS_LANE + (uint32_t)__ffs((int)L.m) - 1u);
    __syncthreads();
    if (threadIdx.x == 0u) A.first[blockIdx.x] = s_first;
}

// next[t] = the first run start in a tile behind t, n where there is none: one workgroup, from the last chunk of 1024 tiles to the first
__global__ void __launch_bounds__(256) k_runs_next(const uint32_t* __restrict__ first, uint64_t* __restrict__ next, uint64_t nt, uint64_t n) {
    __shared__ unsigned long long s_w[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = n;
    for (uint64_t c = (nt + 1023u) / 1024u; c-- > 0;) {
        const uint64_t i = c * 1024u + threadIdx.x * 4u;
        uint32_t f[4]; unsigned long long own = RUNS_NONE;
#pragma unroll
        for (int e = 3; e >= 0; --e) { f[e] = i + e < nt ? first[i + e] : COV_TILE; if (f[e] < COV_TILE) own = (i + e) * COV_TILE + f[e]; }
        unsigned long long incl = own;                     // the first run start of my tiles and the lanes' right of me in the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) { const unsigned long long t = __shfl_down(incl, d); if (lane + d < 64u && t < incl) incl = t; }
        if (lane == 0u) s_w[wave] = incl;
        __syncthreads();
        unsigned long long cur = __shfl_down(incl, 1u);
        if (lane == 63u) cur = RUNS_NONE;
        unsigned long long all = s_w[0];
        for (uint32_t w = 1; w < 4u; ++w) { if (w > wave && s_w[w] < cur) cur = s_w[w]; if (s_w[w] < all) all = s_w[w]; }
        if (carry < cur) cur = carry;
#pragma unroll
        for (int e = 3; e >= 0; --e) { if (i + e < nt) next[i + e] = cur; if (f[e] < COV_TILE) cur = (i + e) * COV_TILE + f[e]; }
        if (all < carry) carry = all;
        __syncthreads();                                   // (s_w is written again in the next step)
    }
}

__global__ void __launch_bounds__(256) k_runs_size(RunsArgs A) {
    __shared__ uint32_t s_val[RUNS_VAL_WORDS];
    __shared__ __attribute__((aligned(8))) uint16_t s_st[256];
    __shared__ uint32_t s_l[4], s_b[4];
    const RunsLane L = runs_lane(A, blockIdx.x, s_val, s_st, true);
    RunsCount c; runs_lane_lines(A, L, s_val, c);
    const uint32_t nl = wave_sum((uint32_t)__popc(L.m)), nb = wave_sum((uint32_t)c.n);
    if ((threadIdx.x & 63u) == 0u) { s_l[threadIdx.x >> 6] = nl; s_b[threadIdx.x >> 6] = nb; }
    __syncthreads();
    if (threadIdx.x == 0u) { A.lines[blockIdx.x] = s_l[0] + s_l[1] + s_l[2] + s_l[3]; A.bytes[blockIdx.x] = s_b[0] + s_b[1] + s_b[2] + s_b[3]; }
}

// tile t0 + blockIdx.x of a slab; offs: the exclusive scan of the slab's tile bytes (its tiles + 1 entries), out: the slab's text
__global__ void __launch_bounds__(256) k_runs_emit(RunsArgs A, uint32_t t0, const uint64_t* __restrict__ offs, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    __shared__ uint32_t s_val[RUNS_VAL_WORDS];
    __shared__ __attribute__((aligned(8))) uint16_t s_st[256];
    __shared__ uint32_t s_w[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const RunsLane L = runs_lane(A, t0 + blockIdx.x, s_val, s_st, true);
    RunsCount c; runs_lane_lines(A, L, s_val, c);
    const uint32_t mine = (uint32_t)c.n, incl = wave_incl_scan(mine, (int)lane);
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += s_w[w];
    const uint64_t b0 = offs[blockIdx.x], b1 = offs[blockIdx.x + 1u], my0 = b0 + before + incl - mine;
    const bool fits = b1 - b0 == (uint64_t)s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (!fits && threadIdx.x == 0u) atomicOr(A.flags, (uint32_t)FLAG_RUNS);   // (the sizing pass counted another tile: its lanes keep out of the text)
    const EmitSpan sp{b0, b1, my0, my0 + mine};
    emit_windows(s_run4, sp, fits && mine != 0u, lds, out, A.flags, (uint32_t)FLAG_RUNS, [&](WinOut& o) { runs_lane_lines(A, L, s_val, o); });
}

uint64_t runs_tiles(uint64_t n) { return (n + COV_TILE - 1u) / COV_TILE; }

void launch_runs_plan(hipStream_t s, const RunsArgs& a) {
    const uint64_t nt = runs_tiles(a.n);
    if (!nt) return;
    if (a.n_rec == 0 || nt > 0x7FFFFFFFull) { note_launch(hipErrorInvalidValue); return; }
    hipLaunchKernelGGL(k_runs_first, dim3((uint32_t)nt), dim3(256), 0, s, a);
    note_launch(hipGetLastError());
    hipLaunchKernelGGL(k_runs_next, dim3(1), dim3(256), 0, s, (const uint32_t*)a.first, a.next, nt, a.n);
    note_launch(hipGetLastError());
    hipLaunchKernelGGL(k_runs_size, dim3((uint32_t)nt), dim3(256), 0, s, a);
    note_launch(hipGetLastError());
}

void launch_runs_emit(hipStream_t s, const RunsArgs& a, uint32_t t0, uint32_t tiles, const uint64_t* offs, uint32_t lds, char* out) {
    if (!tiles) return;
    if (a.n_rec == 0 || (uint64_t)t0 + tiles > runs_tiles(a.n)) { note_launch(hipErrorInvalidValue); return; }
    hipLaunchKernelGGL(k_runs_emit, dim3(tiles), dim3(256), RUNS_LDS, s, a, t0, offs, emit_windows_lds(lds, RUNS_LDS), out);
    note_launch(hipGetLastError());
}

}  // namespace scs
