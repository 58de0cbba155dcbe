// scs_k_lift.hip -- gfx950 kernels of the lift table (scs_lift.h).
//
// k_depth_lift: per bin of the ORIGINAL REFERENCE the reads and aligned bases of a batch, right after its base pass, from what
// k_depth reads -- the pair records and the indel pass' events; no FASTQ text, no byte genome.  A thread per pair places its reads
// (for_each_placed_read), finds the segment of the leftmost aligned base by one bisection of the table and walks the truth CIGAR with a
// segment cursor (lift_read): every M run is cut at segment ends and reference bin boundaries; what lies in an inserted segment
// goes to the pseudo-bin n_bins.  The table is small and read-only: plain loads that L2 keeps.  Aggregation is k_depth's
// (DepthTable and depth_table_run, scs_depth_table.h): an LDS table per workgroup, then one 64-bit atomic per used slot and counter; the pseudo-bin is
// an ordinary key.  The lanes diverge on the CIGAR walk and the segment cursor, as k_depth's do on the walk.
// k_lift_copies: a workgroup per segment, its lanes over the reference bins the segment covers, one atomicAdd per (segment, bin).
// k_lift_points: a thread per staged position, a bisection of the table, coalesced in and out.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_depth.h"
#include "scs_depth_table.h"
#include "scs_lift.h"

namespace scs {

__device__ void depth_lift_pair(const LiftArgs& A, const LiftView& V, uint32_t pi, const DepthTable& T) {
    for_each_placed_read(A, pi, (uint32_t)FLAG_LIFT, [&](const PairRec&, uint32_t, const TruthAln& a, int, uint32_t, int64_t r0, int64_t r1) {
        const uint32_t nb = (uint32_t)A.n_bins;            // (at most 2^27: the pseudo-bin is a uint32 key like the others)
        const int err = lift_read(a, r0, r1, V,
                                  [&](uint64_t bin) { if (bin <= nb) T.add((uint32_t)bin, 1u, 0u); else atomicOr(A.flags, (uint32_t)FLAG_LIFT); },
                                  [&](uint64_t bin, uint32_t n) { if (bin <= nb) T.add((uint32_t)bin, 0u, n); else atomicOr(A.flags, (uint32_t)FLAG_LIFT); });
        if (err) atomicOr(A.flags, (uint32_t)FLAG_LIFT);   // placed outside its record, off the table, or lifted outside the reference: the call fails
    });
}

__global__ void __launch_bounds__(256) k_depth_lift(LiftArgs A) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    const LiftView V{A.segs, A.n_seg, A.ref_len, A.ref_bin_off, A.n_ref, A.bin_width, A.n_bins};
    depth_table_run(A.slots, A.reads, A.bases, [&](const DepthTable& T) { if (pi < A.np) depth_lift_pair(A, V, pi, T); });
}

void launch_depth_lift(hipStream_t s, const LiftArgs& a) {
    if (a.np == 0) return;
    LiftArgs b = a; b.slots = table_slots(a.slots, DEPTH_LDS_SLOTS);
    hipLaunchKernelGGL(k_depth_lift, dim3(cdiv(a.np, 256)), dim3(256), 0, s, b);
    note_launch(hipGetLastError());
}

__global__ void __launch_bounds__(256) k_lift_copies(const LiftSeg* segs, uint32_t n_seg, const uint64_t* ref_len, const uint64_t* ref_bin_off, uint32_t n_ref, uint32_t bin_width,
                                                     uint64_t n_bins, unsigned long long* copies, uint32_t* flags) {
    const uint32_t si = blockIdx.x;
    if (si >= n_seg) return;
    const LiftSeg sg = segs[si];
    if (sg.len == 0) return;
    if (sg.kind != 0u) { if (threadIdx.x == 0) atomicAdd(&copies[n_bins], (unsigned long long)sg.len); return; }   // inserted bases: the pseudo-bin
    if (sg.ref_rec >= n_ref || sg.ref_pos + sg.len > ref_len[sg.ref_rec]) { if (threadIdx.x == 0) atomicOr(flags, (uint32_t)FLAG_LIFT); return; }
    const uint64_t w = bin_width, r0 = sg.ref_pos, r1 = sg.ref_pos + sg.len, q0 = r0 / w, q1 = (r1 - 1u) / w, b0 = ref_bin_off[sg.ref_rec];
    for (uint64_t q = q0 + threadIdx.x; q <= q1; q += 256u) {
        const uint64_t lo = q * w > r0 ? q * w : r0, hi = (q + 1u) * w < r1 ? (q + 1u) * w : r1;
        if (b0 + q < n_bins) atomicAdd(&copies[b0 + q], (unsigned long long)(hi - lo)); else atomicOr(flags, (uint32_t)FLAG_LIFT);
    }
}

void launch_lift_copies(hipStream_t s, const LiftSeg* segs, uint32_t n_seg, const uint64_t* ref_len, const uint64_t* ref_bin_off, uint32_t n_ref, uint32_t bin_width,
                        uint64_t n_bins, unsigned long long* copies, uint32_t* flags) {
    if (n_seg == 0) return;
    hipLaunchKernelGGL(k_lift_copies, dim3(n_seg), dim3(256), 0, s, segs, n_seg, ref_len, ref_bin_off, n_ref, bin_width, n_bins, copies, flags);
    note_launch(hipGetLastError());
}

__global__ void __launch_bounds__(256) k_lift_points(const LiftSeg* segs, uint32_t n_seg, const uint64_t* rec_off, uint32_t n_rec, const uint32_t* rec, const uint64_t* pos, uint64_t n,
                                                     uint32_t* ref_rec, uint64_t* ref_pos, uint32_t* kind, uint32_t* bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rec[i]; const uint64_t p = pos[i];
    if (r >= n_rec || p >= rec_off[r + 1] - rec_off[r]) { atomicOr(bad, 1u); return; }   // outside its record: the call fails
    uint32_t rr, k; uint64_t rp;
    lift_point(segs, n_seg, rec_off[r] + p, rr, rp, k);
    ref_rec[i] = rr; ref_pos[i] = rp; kind[i] = k;
}

void launch_lift_points(hipStream_t s, const LiftSeg* segs, uint32_t n_seg, const uint64_t* rec_off, uint32_t n_rec, const uint32_t* rec, const uint64_t* pos, uint64_t n,
                        uint32_t* ref_rec, uint64_t* ref_pos, uint32_t* kind, uint32_t* bad) {
    if (n == 0 || n_seg == 0) return;
    hipLaunchKernelGGL(k_lift_points, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, segs, n_seg, rec_off, n_rec, rec, pos, n, ref_rec, ref_pos, kind, bad);
    note_launch(hipGetLastError());
}

}  // namespace scs
