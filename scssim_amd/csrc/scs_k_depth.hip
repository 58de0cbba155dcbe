// scs_k_depth.hip -- gfx950 kernel of the depth track (scs_set_depth): per bin of the staged genome the
// reads that start in it and the bases aligned in it, summed over a batch's reads right after its base pass from what the device
// holds anyway -- the pair records and the indel pass' events.  No FASTQ text, no byte genome.
//
// A thread per pair places its reads (for_each_placed_read, scs_place.h: the truth passes' placement) and cuts their M runs at the bin boundaries
// (depth_read, scs_depth.h).  Neighbouring pairs of the list are reads of one amplicon, so the 256 pairs of a workgroup hit the
// same few bins: the workgroup first sums into an open-addressing table in LDS (key = the global bin, < 2^27; two uint32 sums per
// slot, at most 512 reads x L bases each: no overflow) and then adds every used slot to memory once, one 64-bit atomic per
// counter.  A lane that finds no free slot within DEPTH_PROBES steps adds to memory itself, so a full table costs time, never a
// count (DepthTable and the kernel's shell, scs_depth_table.h: shared with k_depth_lift).  slots = 0 (SCS_TEST_DEPTH_SLOTS): no table, every add goes to
// memory -- the un-aggregated kernel of the A/B.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_depth.h"
#include "scs_depth_table.h"

namespace scs {

__device__ void depth_pair(const DepthArgs& A, uint32_t pi, const DepthTable& T) {
    for_each_placed_read(A, pi, (uint32_t)FLAG_DEPTH, [&](const PairRec&, uint32_t, const TruthAln& a, int, uint32_t lo, int64_t r0, int64_t r1) {
        if (a.lo < r0 || a.hi >= r1) { atomicOr(A.flags, (uint32_t)FLAG_DEPTH); return; }   // outside its record: the call fails
        const uint64_t b0 = A.bin_off[lo], nb = A.bin_off[lo + 1] - b0;
        depth_read(a, r0, A.bin_width,
                   [&](uint64_t bin) { T.add((uint32_t)(b0 + bin), 1u, 0u); },
                   [&](uint64_t bin, uint32_t n) { if (bin < nb) T.add((uint32_t)(b0 + bin), 0u, n); else atomicOr(A.flags, (uint32_t)FLAG_DEPTH); });
    });
}

__global__ void __launch_bounds__(256) k_depth(DepthArgs A) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    depth_table_run(A.slots, A.reads, A.bases, [&](const DepthTable& T) { if (pi < A.np) depth_pair(A, pi, T); });
}

void launch_depth(hipStream_t s, const DepthArgs& a) {
    if (a.np == 0) return;
    DepthArgs b = a; b.slots = table_slots(a.slots, DEPTH_LDS_SLOTS);
    hipLaunchKernelGGL(k_depth, dim3(cdiv(a.np, 256)), dim3(256), 0, s, b);
    note_launch(hipGetLastError());
}

}  // namespace scs
