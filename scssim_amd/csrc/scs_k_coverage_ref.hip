// scs_k_coverage_ref.hip -- gfx950 kernels of the coverage profile on the reference (scs_set_coverage_ref).
// Depth is linear in the (read, base) pairs, and an R segment of the lift table maps a contiguous staged stretch onto a contiguous
// reference stretch: ref_depth[p] = the sum of depth[g] over the staged bases g that lift to p.  So nothing here runs per batch:
// the batches mark the staged difference array (k_cov_mark), the end-of-job pass makes the staged depths (scs_k_coverage.hip), and
// these kernels carry them through the table once.
//
// k_cov_ref_copies, once per (genome, table): a workgroup per COV_TILE staged bases, thread tid owns base strip * 256 + tid of
//   every strip.  Its bases ascend, so it finds the segment of its first base by one bisection and the others with a cursor that
//   only moves forward.  One no-return atomicAdd of 1 | is_n << 16 into the packed word of the lifted base; I segments add nothing.
// k_cov_ref_lift, end of the job: the same mapping over the staged depths.  A zero depth costs its load and nothing else (not
//   even the bisection): that keeps a low-coverage job cheap.  A non-zero depth is one no-return uint32 atomicAdd to ref_depth;
//   depths under I segments go into a per-thread uint64 and reach *unlifted by wave reduction, one atomic per wave.
//   With this mapping one wave's atomic instruction covers 64 consecutive staged bases -- inside a segment 64 consecutive
//   reference entries, 256 contiguous bytes: the shape the float-atomic measurements found an order of magnitude faster than
//   scattered ones.  That finding is NOT measured for integer adds; the shape is taken anyway (it costs nothing).
// k_cov_ref_hist, over reference tiles: the counting half of k_cov_scan_hist without the scan -- the LDS histogram of
//   min(max_depth + 1, COV_LDS_BUCKETS) buckets, one add per run of equal depth among a thread's four neighbours, overflow to
//   64-bit global atomics, a flush of the non-zero buckets; the tile's first base bisected in the reference record starts, a
//   bisection per base behind a record border inside the tile.  N and absent come from the packed word, not from genome codes;
//   the 17 x 2 copy-number accumulators live in LDS (one add per run of equal copy number) and are flushed with one 64-bit atomic
//   per non-zero entry.
// Every segment is checked against its reference record's length when a thread enters it (one load): a segment that lifts
// outside raises FLAG_LIFT and adds nothing, so a bad table is an error and never a write outside the arrays.  Both arrays are
// padded to whole tiles, so k_cov_ref_hist's 16-byte loads need no bound.  No workgroup waits for another.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_coverage.h"
#include "scs_lift.h"

namespace scs {

// the segment of a thread's current staged base.  ok: an R segment inside its reference record, ref0 = the global reference index
// of its first base
struct SegCursor { uint32_t si = 0; LiftSeg sg{}; uint64_t ref0 = 0; bool have = false, ok = false; };

// moves c to the segment that holds g (g ascends from call to call).  false: the table does not hold g (FLAG_LIFT is raised)
__device__ __forceinline__ bool seg_at(const CovRefArgs& A, SegCursor& c, uint64_t g) {
    bool entered = false;
    if (!c.have) { c.si = lift_find(A.segs, A.n_seg, g); c.sg = A.segs[c.si]; c.have = true; entered = true; }
    while (g - c.sg.hap_off >= c.sg.len && g >= c.sg.hap_off) {
        if (c.si + 1u >= A.n_seg) { atomicOr(A.flags, (uint32_t)FLAG_LIFT); return false; }
        c.sg = A.segs[++c.si]; entered = true;
    }
    if (g < c.sg.hap_off) { atomicOr(A.flags, (uint32_t)FLAG_LIFT); return false; }
    if (entered) {
        c.ok = false;
        if (c.sg.kind == 0u) {
            const uint64_t rl = c.sg.ref_rec < A.n_ref ? A.ref_off[c.sg.ref_rec + 1u] - A.ref_off[c.sg.ref_rec] : 0u;
            if (c.sg.ref_rec < A.n_ref && c.sg.len <= rl && c.sg.ref_pos <= rl - c.sg.len) { c.ok = true; c.ref0 = A.ref_off[c.sg.ref_rec] + c.sg.ref_pos; }
            else atomicOr(A.flags, (uint32_t)FLAG_LIFT);   // lifts outside its reference record: nothing is added
        }
    }
    return true;
}

__global__ void __launch_bounds__(256) k_cov_ref_copies(CovRefArgs A) {
    const uint64_t base = (uint64_t)blockIdx.x * COV_TILE;
    SegCursor c;
    for (uint32_t j = 0; j < COV_TILE / 256u; ++j) {
        const uint64_t g = base + j * 256u + threadIdx.x;
        if (g >= A.n_staged) break;
        if (!seg_at(A, c, g) || !c.ok) continue;           // inserted sequence has no reference coordinate
        atomicAdd(A.packed + (c.ref0 + (g - c.sg.hap_off)), 1u | (A.codes[g] >= 4u ? 0x10000u : 0u));
    }
}

__global__ void __launch_bounds__(256) k_cov_ref_lift(CovRefArgs A) {
    const uint64_t base = (uint64_t)blockIdx.x * COV_TILE;
    SegCursor c; unsigned long long unl = 0;
    for (uint32_t j = 0; j < COV_TILE / 256u; ++j) {
        const uint64_t g = base + j * 256u + threadIdx.x;
        if (g >= A.n_staged) break;
        const uint32_t d = A.depth[g];
        if (!d || !seg_at(A, c, g)) continue;
        if (c.sg.kind != 0u) { unl += d; continue; }
        if (c.ok) atomicAdd(A.ref_depth + (c.ref0 + (g - c.sg.hap_off)), d);
    }
    unl = wave_sum_u64(unl);
    if ((threadIdx.x & 63u) == 0u && unl) atomicAdd(A.unlifted, unl);
}

__global__ void __launch_bounds__(256) k_cov_ref_hist(CovRefArgs A) {
    __shared__ uint32_t s_hist[COV_LDS_BUCKETS];
    __shared__ unsigned long long s_cn[2u * (COV_REF_CN + 1u)];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, D = A.max_depth, nl = A.lds, NC = COV_REF_CN + 1u;
    const uint64_t base = (uint64_t)blockIdx.x * COV_TILE, R = A.n_ref_bases;
    for (uint32_t i = tid; i < nl; i += 256u) s_hist[i] = 0u;
    if (tid < 2u * NC) s_cn[tid] = 0ull;
    // the reference record the tile begins in: its bases use the LDS tables and the per-thread sums; the others of the tile go to memory
    const uint32_t r_t = rec_of(A.ref_off, A.n_ref, (int64_t)base);
    const uint64_t r_end = A.ref_off[r_t + 1];
    unsigned long long* const row = A.hist + (uint64_t)r_t * (D + 1u);
    unsigned long long t_n = 0, t_abs = 0, t_sum = 0, t_sum_n = 0; bool bad = false;
    auto flush = [&](uint32_t b, uint32_t n) {
        if (!n) return;
        if (b < nl) atomicAdd(&s_hist[b], n); else atomicAdd(row + b, (unsigned long long)n);
    };
    auto cn_flush = [&](uint32_t cn, uint32_t n, unsigned long long s) {
        if (!n) return;
        atomicAdd(&s_cn[cn], (unsigned long long)n);
        if (s) atomicAdd(&s_cn[NC + cn], s);
    };
    __syncthreads();
    for (uint32_t j = 0; j < COV_TILE / 1024u; ++j) {
        const uint64_t i0 = base + j * 1024u + tid * 4u;
        const uint4 dv = *(const uint4*)(A.ref_depth + i0), pv = *(const uint4*)(A.packed + i0);
        const uint32_t d[4] = {dv.x, dv.y, dv.z, dv.w}, p[4] = {pv.x, pv.y, pv.z, pv.w};
        uint32_t run_b = 0xFFFFFFFFu, run_n = 0, cn_r = 0xFFFFFFFFu, cn_n = 0; unsigned long long cn_s = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const uint64_t i = i0 + e;
            if (i >= R) continue;                          // padding
            const uint32_t dep = d[e], cp = p[e] & 0xFFFFu, ncp = p[e] >> 16, b = dep < D ? dep : D, cn = cp < COV_REF_CN ? cp : COV_REF_CN;
            const bool is_n = cp > 0u && ncp == cp;        // every copy is N; mixed copies count as sequence
            if (!cp && dep) bad = true;                    // depth where no staged base lifts to
            if (i < r_end) {
                if (is_n) { ++t_n; t_sum_n += dep; continue; }
                t_sum += dep; if (!cp) ++t_abs;
                if (b == run_b) ++run_n; else { flush(run_b, run_n); run_b = b; run_n = 1u; }
                if (cn == cn_r) { ++cn_n; cn_s += dep; } else { cn_flush(cn_r, cn_n, cn_s); cn_r = cn; cn_n = 1u; cn_s = dep; }
            } else {                                       // behind a record border inside the tile: under its own record
                const uint32_t r = rec_of(A.ref_off, A.n_ref, (int64_t)i);
                if (is_n) { atomicAdd(A.n_n + r, 1ull); if (dep) atomicAdd(A.sum_n + r, (unsigned long long)dep); continue; }
                atomicAdd(A.hist + (uint64_t)r * (D + 1u) + b, 1ull); atomicAdd(A.cn_bases + (uint64_t)r * NC + cn, 1ull);
                if (!cp) atomicAdd(A.absent + r, 1ull);
                if (dep) { atomicAdd(A.sum + r, (unsigned long long)dep); atomicAdd(A.cn_sum + (uint64_t)r * NC + cn, (unsigned long long)dep); }
            }
        }
        flush(run_b, run_n); cn_flush(cn_r, cn_n, cn_s);
    }
    t_n = wave_sum_u64(t_n); t_abs = wave_sum_u64(t_abs); t_sum = wave_sum_u64(t_sum); t_sum_n = wave_sum_u64(t_sum_n);
    if (lane == 0u) {
        if (t_n) atomicAdd(A.n_n + r_t, t_n);
        if (t_abs) atomicAdd(A.absent + r_t, t_abs);
        if (t_sum) atomicAdd(A.sum + r_t, t_sum);
        if (t_sum_n) atomicAdd(A.sum_n + r_t, t_sum_n);
    }
    if (bad) atomicOr(A.flags, (uint32_t)FLAG_COVERAGE);
    __syncthreads();
    for (uint32_t i = tid; i < nl; i += 256u) if (s_hist[i]) atomicAdd(row + i, (unsigned long long)s_hist[i]);
    if (tid < 2u * NC && s_cn[tid]) atomicAdd((tid < NC ? A.cn_bases : A.cn_sum) + (uint64_t)r_t * NC + (tid < NC ? tid : tid - NC), s_cn[tid]);
}

uint64_t cov_ref_tiles(uint64_t n_ref_bases) { return (n_ref_bases + COV_TILE - 1u) / COV_TILE; }

static bool cov_ref_grids(const CovRefArgs& a, uint64_t& staged_tiles, uint64_t& ref_tiles) {
    staged_tiles = (a.n_staged + COV_TILE - 1u) / COV_TILE; ref_tiles = cov_ref_tiles(a.n_ref_bases);
    return a.n_ref != 0 && a.n_seg != 0 && staged_tiles <= 0x7FFFFFFFull && ref_tiles <= 0x7FFFFFFFull;
}

void launch_cov_ref_copies(hipStream_t s, const CovRefArgs& a) {
    uint64_t st, rt;
    if (!cov_ref_grids(a, st, rt)) { note_launch(hipErrorInvalidValue); return; }
    if (!st) return;
    hipLaunchKernelGGL(k_cov_ref_copies, dim3((uint32_t)st), dim3(256), 0, s, a);
    note_launch(hipGetLastError());
}

void launch_cov_ref_finish(hipStream_t s, const CovRefArgs& a) {
    uint64_t st, rt;
    if (!cov_ref_grids(a, st, rt)) { note_launch(hipErrorInvalidValue); return; }
    CovRefArgs g = a; g.lds = cov_lds_buckets(a.lds, a.max_depth);
    if (st) { hipLaunchKernelGGL(k_cov_ref_lift, dim3((uint32_t)st), dim3(256), 0, s, g); note_launch(hipGetLastError()); }
    if (rt) { hipLaunchKernelGGL(k_cov_ref_hist, dim3((uint32_t)rt), dim3(256), 0, s, g); note_launch(hipGetLastError()); }
}

}  // namespace scs
