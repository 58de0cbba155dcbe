// scs_k_truth.hip -- gfx950 kernels of the truth SAM (scs_set_truth_sam): each read's true alignment as one SAM record, made per
// batch after k_reads from what the device holds -- the pair records (PairRec: the amplicon as an index map of the genome), the
// indel pass' events, the FASTQ text k_reads has just written and the byte genome.  Two passes over the batch's pairs, a thread per
// pair, both running the formatter of scs_truth.h: the SIZING pass counts the bytes of the pair's records (NM / MD need the genome
// comparison already), a 64-bit exclusive scan gives their offsets, and the EMIT pass writes them by the wave scheme of scs_emit.h
// (emit_runs: a pair's ~390-byte records built in LDS, the run copied out in aligned 16-byte stores).
// The truth BAM (scs_set_truth_bam) runs the same two passes over the same loads with the BAM formatter (k_truth_bam_size,
// k_truth_bam_emit); its records then become BGZF blocks through the kernels of scs_bgzf.hip.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_emit.h"

namespace scs {

#define TRUTH_LDS 61440u                                   // bytes of one workgroup's run of records (dynamic LDS: 2 workgroups per CU)

struct DevSrc {                                            // a read's FASTQ bases and qualities, the genome as characters
    const char* s; const char* q; const uint8_t* g;
    __device__ char seq(int i) const { return s[i]; }
    __device__ char qual(int i) const { return q[i]; }
    __device__ char gen(int64_t x) const { const uint32_t c = g[x]; return (char)(c < 4u ? (0x54474341u >> (8u * c)) & 255u : 'N'); }
};

// both records of pair pi through fmt(alignment, line, source, index of the record): the SAM's formatter or the BAM's
template <class Fmt>
__device__ void truth_pair(const TruthArgs& A, uint32_t pi, Fmt fmt) {
    const PairRec pr = A.pairs[pi];
    if (pr.isz == 0) return;                               // hole: no FASTQ record either
    uint32_t ev1[TRUTH_EVCAP], ev2[TRUTH_EVCAP];
    TruthAln a1, a2; DevSrc s1, s2; s1.g = s2.g = A.g;
    if (!truth_load(A, pr, pi, 0, ev1, a1, s1.s, s1.q)) return;
    if (A.paired && !truth_load(A, pr, pi, 1, ev2, a2, s2.s, s2.q)) return;
    const uint32_t lo = rec_of(A.rec_off, A.n_rec, a1.lo);
    const int64_t r0 = (int64_t)A.rec_off[lo], r1 = (int64_t)A.rec_off[lo + 1];
    if (a1.lo < r0 || a1.hi >= r1 || (A.paired && (a2.lo < r0 || a2.hi >= r1))) { atomicOr(A.flags, (uint32_t)FLAG_TRUTH); return; }
    TruthLine li{pr.amp, pr.att + 1u, 0u, A.paired, A.names + A.name_off[lo], A.name_off[lo + 1] - A.name_off[lo], r0, 0, 0};
    if (!A.paired) {
        li.flag = a1.rev ? 0x10u : 0u;
        fmt(a1, li, s1, lo);
        return;
    }
    const int64_t left = a1.lo < a2.lo ? a1.lo : a2.lo, right = a1.hi > a2.hi ? a1.hi : a2.hi, t = right - left + 1;
    li.flag = 0x43u | (a1.rev ? 0x10u : 0u) | (a2.rev ? 0x20u : 0u); li.mate_lo = a2.lo; li.tlen = a1.lo <= a2.lo ? t : -t;
    fmt(a1, li, s1, lo);
    li.flag = 0x83u | (a2.rev ? 0x10u : 0u) | (a1.rev ? 0x20u : 0u); li.mate_lo = a1.lo; li.tlen = a1.lo <= a2.lo ? -t : t;
    fmt(a2, li, s2, lo);
}

__global__ void __launch_bounds__(256) k_truth_size(TruthArgs A, uint32_t* __restrict__ sizes) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= A.np) return;
    TruthCount c; truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t) { truth_record(c, a, li, src); });
    sizes[pi] = (uint32_t)c.n;
}

// one wave per `ppb` <= 64 pairs: lane i formats pair p0 + i at its place in the run's LDS image, then the wave copies the run out
// (scs_emit.h; the one turn of emit_runs).  A run that outgrows `lds` bytes (very long reads; SCS_TEST_TRUTH_LDS) is written lane
// by lane straight to memory instead: the truth SAM refuses no pair
__global__ void __launch_bounds__(64) k_truth_emit(TruthArgs A, const uint64_t* __restrict__ offs, uint32_t ppb, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    const uint32_t p0 = blockIdx.x * ppb, p1 = min(p0 + ppb, A.np), pi = p0 + threadIdx.x;
    const uint64_t b0 = offs[p0], b1 = offs[p1], wa = emit_base(b0);
    const bool in_lds = b1 - wa <= (uint64_t)lds;
    if (threadIdx.x < ppb && pi < p1 && offs[pi + 1] > offs[pi]) {
        RunOut o{in_lds ? reinterpret_cast<char*>(s_run4) + (offs[pi] - wa) : out + offs[pi], 0u};
        truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t) { truth_record(o, a, li, src); });
        if (o.n != (uint32_t)(offs[pi + 1] - offs[pi])) atomicOr(A.flags, (uint32_t)FLAG_TRUTH);   // (the sizing pass and the formatter disagree)
    }
    if (!in_lds) return;
    __syncthreads();
    emit_copy_out<64>(s_run4, wa, b0, b1, out);
}

// ---- the truth BAM (scs_set_truth_bam): the same two passes over the same loads, the records in BAM's encoding
#define TRUTH_BAM_LDS 49152u                               // bytes of one workgroup's run of BAM records (3 workgroups per CU)

__global__ void __launch_bounds__(256) k_truth_bam_size(TruthArgs A, uint32_t* __restrict__ sizes) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= A.np) return;
    uint32_t n = 0;
    truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t) { n += truth_bam_size(a, li, src); });
    sizes[pi] = n;
}

// one wave per `ppb` <= 64 pairs (emit_runs).  A pair that alone outgrows the LDS raises FLAG_TRUTH
__global__ void __launch_bounds__(64) k_truth_bam_emit(TruthArgs A, const uint64_t* __restrict__ offs, uint32_t ppb, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    const uint32_t p0 = blockIdx.x * ppb;
    emit_runs(s_run4, offs, p0, min(ppb, A.np - p0), lds, out, A.flags, (uint32_t)FLAG_TRUTH, [&](uint32_t pi, RunOut& o) {
        truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t ref) { truth_bam_record(o, a, li, src, (int32_t)ref); });
    });
}

void launch_truth_bam_size(hipStream_t s, const TruthArgs& a, uint32_t* sizes) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_bam_size, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
uint32_t truth_bam_pairs_per_block(uint64_t fq_bytes, uint32_t np) {
    // a record is 36 bytes of head, name, CIGAR and tags (about 90 with a short MD string) plus 1.5 bytes per base; its FASTQ record 2 per base
    return pairs_per_block(fq_bytes, np, TRUTH_BAM_LDS, 3, 4, 192);
}
void launch_truth_bam_emit(hipStream_t s, const TruthArgs& a, const uint64_t* offs, uint32_t ppb, uint32_t lds, char* out) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_bam_emit, dim3(cdiv(a.np, ppb)), dim3(64), TRUTH_BAM_LDS, s, a, offs, ppb, emit_runs_lds(lds, TRUTH_BAM_LDS), out);
    note_launch(hipGetLastError());
}

void launch_truth_size(hipStream_t s, const TruthArgs& a, uint32_t* sizes) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_size, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
uint32_t truth_pairs_per_block(uint64_t fq_bytes, uint32_t np) {
    // a record is its FASTQ record (name, bases, qualities) plus about 80 bytes of fields and tags (and the MD string)
    uint32_t ppb = pairs_per_block(fq_bytes, np, TRUTH_LDS, 5, 4, 192);
    while (ppb & (ppb - 1u)) ppb &= ppb - 1u;              // 64, 32, 16, ...: the power of two at or below
    return ppb;
}
void launch_truth_emit(hipStream_t s, const TruthArgs& a, const uint64_t* offs, uint32_t ppb, uint32_t lds, char* out) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_emit, dim3(cdiv(a.np, ppb)), dim3(64), TRUTH_LDS, s, a, offs, ppb, emit_runs_lds(lds, TRUTH_LDS), out);
    note_launch(hipGetLastError());
}

}  // namespace scs
