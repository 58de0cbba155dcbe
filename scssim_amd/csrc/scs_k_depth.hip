// scs_k_depth.hip -- gfx950 kernel of the depth track (scs_set_depth): per bin of the staged genome the
// reads that start in it and the bases aligned in it, summed over a batch's reads right after its base pass from what the device
// holds anyway -- the pair records and the indel pass' events.  No FASTQ text, no byte genome.
//
// A thread per pair places its reads (read_place: the truth passes' placement) and cuts their M runs at the bin boundaries
// (depth_read, scs_depth.h).  Neighbouring pairs of the list are reads of one amplicon, so the 256 pairs of a workgroup hit the
// same few bins: the workgroup first sums into an open-addressing table in LDS (key = the global bin, < 2^27; two uint32 sums per
// slot, at most 512 reads x L bases each: no overflow) and then adds every used slot to memory once, one 64-bit atomic per
// counter.  A lane that finds no free slot within DEPTH_PROBES steps adds to memory itself, so a full table costs time, never a
// count (DepthTable, scs_depth_table.h: shared with k_depth_lift).  slots = 0 (SCS_TEST_DEPTH_SLOTS): no table, every add goes to
// memory -- the un-aggregated kernel of the A/B.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_depth.h"
#include "scs_depth_table.h"

namespace scs {

__device__ void depth_pair(const DepthArgs& A, uint32_t pi, const DepthTable& T) {
    const PairRec pr = A.pairs[pi];
    if (pr.isz == 0) return;                               // hole: no FASTQ record
    uint32_t ev[TRUTH_EVCAP];
    for (uint32_t rd = 0; rd < (A.paired ? 2u : 1u); ++rd) {
        TruthAln a; int n_out;
        if (!read_place(A, pr, pi, rd, ev, a, n_out, (uint32_t)FLAG_DEPTH)) continue;
        uint32_t lo = 0, hi = A.n_rec;                     // the record: rec_off[lo] <= a.lo < rec_off[lo + 1]
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)A.rec_off[mid] <= a.lo) lo = mid; else hi = mid; }
        const int64_t r0 = (int64_t)A.rec_off[lo], r1 = (int64_t)A.rec_off[lo + 1];
        if (a.lo < r0 || a.hi >= r1) { atomicOr(A.flags, (uint32_t)FLAG_DEPTH); continue; }   // outside its record: the call fails
        const uint64_t b0 = A.bin_off[lo], nb = A.bin_off[lo + 1] - b0;
        depth_read(a, r0, A.bin_width,
                   [&](uint64_t bin) { T.add((uint32_t)(b0 + bin), 1u, 0u); },
                   [&](uint64_t bin, uint32_t n) { if (bin < nb) T.add((uint32_t)(b0 + bin), 0u, n); else atomicOr(A.flags, (uint32_t)FLAG_DEPTH); });
    }
}

__global__ void __launch_bounds__(256) k_depth(DepthArgs A) {
    __shared__ uint32_t s_key[DEPTH_LDS_SLOTS], s_reads[DEPTH_LDS_SLOTS], s_bases[DEPTH_LDS_SLOTS];
    for (uint32_t i = threadIdx.x; i < A.slots; i += 256u) { s_key[i] = DEPTH_EMPTY; s_reads[i] = 0u; s_bases[i] = 0u; }
    __syncthreads();
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi < A.np) depth_pair(A, pi, DepthTable{s_key, s_reads, s_bases, A.slots, A.reads, A.bases});   // (no lane leaves before the barriers)
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < A.slots; i += 256u) {
        const uint32_t bin = s_key[i];
        if (bin == DEPTH_EMPTY) continue;
        if (s_reads[i]) atomicAdd(&A.reads[bin], (unsigned long long)s_reads[i]);
        if (s_bases[i]) atomicAdd(&A.bases[bin], (unsigned long long)s_bases[i]);
    }
}

void launch_depth(hipStream_t s, const DepthArgs& a) {
    if (a.np == 0) return;
    DepthArgs b = a;
    b.slots = b.slots > DEPTH_LDS_SLOTS ? DEPTH_LDS_SLOTS : b.slots;
    while (b.slots & (b.slots - 1u)) b.slots &= b.slots - 1u;                      // a power of two (the table's index mask), or 0
    hipLaunchKernelGGL(k_depth, dim3(cdiv(a.np, 256)), dim3(256), 0, s, b);
    note_launch(hipGetLastError());
}

}  // namespace scs
