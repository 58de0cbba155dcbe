// scs_k_truth_ref.hip -- gfx950 kernels of the truth SAM on the original reference (scs_set_truth_ref_sam):
// each read's true alignment lifted through the lift table, one SAM record per FASTQ record, made per batch after k_reads from
// what the truth SAM's passes read (truth_load: pair records, indel events, the FASTQ text) and the segment table -- no byte genome,
// the record has no NM / MD.  The two passes of scs_k_truth.hip with the formatter of scs_truth_ref.h: the SIZING pass counts the
// bytes of the pair's records, a 64-bit exclusive scan gives their offsets, the EMIT pass writes them.  Both mates are lifted
// (lift_align) before either line is made: each line names its mate's block.  The table is small and read-only: plain loads that
// L2 keeps; a lane's walk costs one bisection and a cursor that moves forward.  The lanes diverge on the CIGAR walk and the cursor.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_truth_ref.h"

namespace scs {

#define TRUTH_REF_LDS 61440u                               // bytes of one workgroup's run of records (dynamic LDS: 2 workgroups per CU)

struct RefSrc {                                            // a read's FASTQ bases and qualities
    const char* s; const char* q;
    __device__ char seq(int i) const { return s[i]; }
    __device__ char qual(int i) const { return q[i]; }
};
struct RefOut { char* p; uint32_t n; __device__ void put(char ch) { p[n++] = ch; } };

// read rd of pair pi: its events into ev and its placement (read_place), then its FASTQ text.  false: as truth_load
__device__ bool truth_ref_load(const TruthArgs& A, const PairRec& pr, uint32_t pi, uint32_t rd, uint32_t* ev, TruthAln& a, RefSrc& src) {
    int n_out;
    if (!read_place(A, pr, pi, rd, ev, a, n_out, (uint32_t)FLAG_TRUTH)) return false;
    src.s = read_text(A.off1, A.off2, A.fq1, A.fq2, A.paired, pr, pi, rd);
    src.q = src.s + n_out + 3;
    return true;
}

// both records of pair pi into o.  A read that cannot be lifted raises FLAG_LIFT and the pair writes nothing: the call fails
template <class Out>
__device__ void truth_ref_pair(const TruthArgs& A, uint32_t pi, Out& o) {
    const PairRec pr = A.pairs[pi];
    if (pr.isz == 0) return;                               // hole: no FASTQ record either
    uint32_t ev1[TRUTH_EVCAP], ev2[TRUTH_EVCAP];
    TruthAln a1, a2; RefSrc s1, s2;
    if (!truth_ref_load(A, pr, pi, 0, ev1, a1, s1)) return;
    if (A.paired && !truth_ref_load(A, pr, pi, 1, ev2, a2, s2)) return;
    uint32_t lo = 0, hi = A.n_rec;                         // the staged record: rec_off[lo] <= a1.lo < rec_off[lo + 1]
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)A.rec_off[mid] <= a1.lo) lo = mid; else hi = mid; }
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

// one workgroup (one wave) per `ppb` <= 64 pairs, as k_truth_bam_emit: lane i formats pair p0 + i into LDS at its offset inside the
// run (the run starts at LDS byte (run start & 15), so 16-byte aligned text is 16-byte aligned in LDS), then the wave copies the
// run out: whole aligned 16-byte chunks, single bytes at the two ends (shared with the neighbouring runs).  The run is cut where it
// would outgrow `lds` bytes: the wave takes the lanes that fit, copies them out and goes on with the rest (one turn for the
// shipped read lengths; SCS_TEST_TRUTH_LDS makes it several).  A pair that alone outgrows the LDS raises FLAG_TRUTH, and so does a
// lane whose formatter wrote another number of bytes than the sizing pass counted.
__global__ void __launch_bounds__(64) k_truth_ref_emit(TruthArgs A, const uint64_t* __restrict__ offs, uint32_t ppb, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    char* s_run = reinterpret_cast<char*>(s_run4);
    const uint32_t p0 = blockIdx.x * ppb, p1 = min(p0 + ppb, A.np), nl = p1 - p0;
    const uint32_t pi = p0 + threadIdx.x; const bool mine = threadIdx.x < nl;
    const uint64_t my0 = mine ? offs[pi] : 0, my1 = mine ? offs[pi + 1] : 0;
    for (uint32_t first = 0; first < nl;) {
        const uint64_t b0 = offs[p0 + first];
        const uint32_t sh = (uint32_t)(b0 & 15u);
        const bool fits = mine && threadIdx.x >= first && my1 - b0 + sh <= (uint64_t)lds;   // (offsets ascend: the lanes that fit are first, first + 1, ...)
        const uint32_t last = first + (uint32_t)__popcll(__ballot(fits));
        if (last == first) { if (threadIdx.x == 0) atomicOr(A.flags, (uint32_t)FLAG_TRUTH); return; }
        const uint64_t b1 = offs[p0 + last];
        if (fits && threadIdx.x < last && my1 > my0) {
            RefOut o{s_run + sh + (uint32_t)(my0 - b0), 0u};
            truth_ref_pair(A, pi, o);
            if (o.n != (uint32_t)(my1 - my0)) atomicOr(A.flags, (uint32_t)FLAG_TRUTH);   // (the sizing pass and the formatter disagree: never a silent wrong file)
        }
        __syncthreads();
        const uint64_t a0 = (b0 + 15u) & ~15ull, a1 = b1 & ~15ull;
        if (a0 >= a1) { for (uint64_t x = b0 + threadIdx.x; x < b1; x += 64u) out[x] = s_run[sh + (x - b0)]; }
        else {
            for (uint64_t x = b0 + threadIdx.x; x < a0; x += 64u) out[x] = s_run[sh + (x - b0)];
            for (uint64_t x = a1 + threadIdx.x; x < b1; x += 64u) out[x] = s_run[sh + (x - b0)];
            for (uint64_t x = a0 + 16u * threadIdx.x; x < a1; x += 1024u) *reinterpret_cast<uint4*>(out + x) = s_run4[(sh + (x - b0)) >> 4];
        }
        __syncthreads();                                   // (the next turn writes the LDS this one has just read)
        first = last;
    }
}

void launch_truth_ref_size(hipStream_t s, const TruthArgs& a, uint32_t* sizes) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_ref_size, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
uint32_t truth_ref_pairs_per_block(uint64_t fq_bytes, uint32_t np) {
    // a record is its FASTQ record (name, bases, qualities) plus about 100 bytes of fields, clips and tags
    const uint64_t est = (np ? fq_bytes / np : 0) + 256;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, TRUTH_REF_LDS / est));
}
void launch_truth_ref_emit(hipStream_t s, const TruthArgs& a, const uint64_t* offs, uint32_t ppb, uint32_t lds, char* out) {
    if (a.np == 0) return;
    lds = lds ? std::min(lds, TRUTH_REF_LDS) : TRUTH_REF_LDS;
    hipLaunchKernelGGL(k_truth_ref_emit, dim3(cdiv(a.np, ppb)), dim3(64), TRUTH_REF_LDS, s, a, offs, ppb, lds, out);
    note_launch(hipGetLastError());
}

}  // namespace scs
