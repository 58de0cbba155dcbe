// scs_k_truth_ref.hip -- gfx950 kernels of the truth SAM on the original reference (scs_set_truth_ref_sam):
// each read's true alignment lifted through the lift table, one SAM record per FASTQ record, made per batch after k_reads from
// what the truth SAM's passes read (truth_load: pair records, indel events, the FASTQ text) and the segment table -- no byte genome,
// the record has no NM / MD.  The two passes of scs_k_truth.hip with the formatter of scs_truth_ref.h: the SIZING pass counts the
// bytes of the pair's records, a 64-bit exclusive scan gives their offsets, the EMIT pass (emit_runs, scs_emit.h) writes them.  Both mates are lifted
// (lift_align) before either line is made: each line names its mate's block.  The table is small and read-only: plain loads that
// L2 keeps; a lane's walk costs one bisection and a cursor that moves forward.  The lanes diverge on the CIGAR walk and the cursor.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_truth_ref.h"
#include "scs_emit.h"

namespace scs {

#define TRUTH_REF_LDS 61440u                               // bytes of one workgroup's run of records (dynamic LDS: 2 workgroups per CU)

struct RefSrc {                                            // a read's FASTQ bases and qualities
    const char* s; const char* q;
    __device__ char seq(int i) const { return s[i]; }
    __device__ char qual(int i) const { return q[i]; }
};

// both records of pair pi into o.  A read that cannot be lifted raises FLAG_LIFT and the pair writes nothing: the call fails
template <class Out>
__device__ void truth_ref_pair(const TruthArgs& A, uint32_t pi, Out& o) {
    const PairRec pr = A.pairs[pi];
    if (pr.isz == 0) return;                               // hole: no FASTQ record either
    uint32_t ev1[TRUTH_EVCAP], ev2[TRUTH_EVCAP];
    TruthAln a1, a2; RefSrc s1, s2;
    if (!truth_load(A, pr, pi, 0, ev1, a1, s1.s, s1.q)) return;
    if (A.paired && !truth_load(A, pr, pi, 1, ev2, a2, s2.s, s2.q)) return;
    const uint32_t lo = rec_of(A.rec_off, A.n_rec, a1.lo);   // the staged record
    const int64_t r0 = (int64_t)A.rec_off[lo], r1 = (int64_t)A.rec_off[lo + 1];
    const LiftTab T{A.segs, A.n_seg, A.ref_len, A.n_ref};
    LiftAln l1{}, l2{};
    int err = lift_align(a1, r0, r1, T, l1);
    if (!err && A.paired) err = lift_align(a2, r0, r1, T, l2);
    if (err) { atomicOr(A.flags, (uint32_t)FLAG_LIFT); return; }
    TruthRefLine li{pr.amp, pr.att + 1u, A.paired, 0, A.paired ? a2.rev : 0, A.names + A.name_off[lo], A.name_off[lo + 1] - A.name_off[lo], r0, r1, A.ref_name_off, A.ref_names};
    // one call site for the formatter: the second turn is the mate's line
    for (int rd = 0; rd < (A.paired ? 2 : 1); ++rd) {
        li.read2 = rd; li.mate_rev = A.paired ? (rd ? a1.rev : a2.rev) : 0;
        if (truth_ref_record(o, rd ? a2 : a1, li, T, rd ? l2 : l1, rd ? l1 : l2, rd ? s2 : s1)) atomicOr(A.flags, (uint32_t)FLAG_LIFT);
    }
}

__global__ void __launch_bounds__(256) k_truth_ref_size(TruthArgs A, uint32_t* __restrict__ sizes) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= A.np) return;
    TruthCount c; truth_ref_pair(A, pi, c);
    sizes[pi] = (uint32_t)c.n;
}

// one wave per `ppb` <= 64 pairs (emit_runs), as k_truth_bam_emit.  A pair that alone outgrows the LDS raises FLAG_TRUTH
__global__ void __launch_bounds__(64) k_truth_ref_emit(TruthArgs A, const uint64_t* __restrict__ offs, uint32_t ppb, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    const uint32_t p0 = blockIdx.x * ppb;
    emit_runs(s_run4, offs, p0, min(ppb, A.np - p0), lds, out, A.flags, (uint32_t)FLAG_TRUTH, [&](uint32_t pi, RunOut& o) { truth_ref_pair(A, pi, o); });
}

void launch_truth_ref_size(hipStream_t s, const TruthArgs& a, uint32_t* sizes) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_ref_size, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
uint32_t truth_ref_pairs_per_block(uint64_t fq_bytes, uint32_t np) {
    // a record is its FASTQ record (name, bases, qualities) plus about 100 bytes of fields, clips and tags
    return pairs_per_block(fq_bytes, np, TRUTH_REF_LDS, 1, 1, 256);
}
void launch_truth_ref_emit(hipStream_t s, const TruthArgs& a, const uint64_t* offs, uint32_t ppb, uint32_t lds, char* out) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_ref_emit, dim3(cdiv(a.np, ppb)), dim3(64), TRUTH_REF_LDS, s, a, offs, ppb, emit_runs_lds(lds, TRUTH_REF_LDS), out);
    note_launch(hipGetLastError());
}

}  // namespace scs
