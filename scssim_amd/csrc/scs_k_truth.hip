// scs_k_truth.hip -- gfx950 kernels of the truth SAM (scs_set_truth_sam): each read's true alignment as one SAM record, made per
// batch after k_reads from what the device holds -- the pair records (PairRec: the amplicon as an index map of the genome), the
// indel pass' events, the FASTQ text k_reads has just written and the byte genome.  Two passes over the batch's pairs, a thread per
// pair, both running the formatter of scs_truth.h: the SIZING pass counts the bytes of the pair's records (NM / MD need the genome
// comparison already), a 64-bit exclusive scan gives their offsets, and the EMIT pass writes them.  The emit pass builds a
// workgroup's contiguous run of records in LDS and copies it out in whole 16-byte aligned stores (a lane writing its ~390-byte
// records byte by byte would leave partial sectors all over the text: the cost k_reads pays for its lane-private records).
// The truth BAM (scs_set_truth_bam) runs the same two passes over the same loads with the BAM formatter (k_truth_bam_size,
// k_truth_bam_emit); its records then become BGZF blocks through the kernels of scs_bgzf.hip.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"

namespace scs {

#define TRUTH_LDS 61440u                                   // bytes of one workgroup's run of records (dynamic LDS: 2 workgroups per CU)

struct DevSrc {                                            // a read's FASTQ bases and qualities, the genome as characters
    const char* s; const char* q; const uint8_t* g;
    __device__ char seq(int i) const { return s[i]; }
    __device__ char qual(int i) const { return q[i]; }
    __device__ char gen(int64_t x) const { const uint32_t c = g[x]; return (char)(c < 4u ? (0x54474341u >> (8u * c)) & 255u : 'N'); }
};
struct PtrOut { char* p; __device__ void put(char ch) { *p++ = ch; } };

// read rd of pair pi: its events into ev and its placement (read_place, scs_place.h), then its FASTQ text.  false: it has no record
// (a hole, or a read the indel pass flagged), or it cannot be made right (FLAG_TRUTH)
__device__ bool truth_load(const TruthArgs& A, const PairRec& pr, uint32_t pi, uint32_t rd, uint32_t* ev, TruthAln& a, DevSrc& src) {
    int n_out;
    if (!read_place(A, pr, pi, rd, ev, a, n_out, (uint32_t)FLAG_TRUTH)) return false;
    src.s = read_text(A.off1, A.off2, A.fq1, A.fq2, A.paired, pr, pi, rd);
    src.q = src.s + n_out + 3; src.g = A.g;
    return true;
}

// both records of pair pi through fmt(alignment, line, source, index of the record): the SAM's formatter or the BAM's
template <class Fmt>
__device__ void truth_pair(const TruthArgs& A, uint32_t pi, Fmt fmt) {
    const PairRec pr = A.pairs[pi];
    if (pr.isz == 0) return;                               // hole: no FASTQ record either
    uint32_t ev1[TRUTH_EVCAP], ev2[TRUTH_EVCAP];
    TruthAln a1, a2; DevSrc s1, s2;
    if (!truth_load(A, pr, pi, 0, ev1, a1, s1)) return;
    if (A.paired && !truth_load(A, pr, pi, 1, ev2, a2, s2)) return;
    uint32_t lo = 0, hi = A.n_rec;                         // the record: rec_off[lo] <= a1.lo < rec_off[lo + 1]
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)A.rec_off[mid] <= a1.lo) lo = mid; else hi = mid; }
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

// one workgroup (one wave) per `ppb` pairs: lane i formats pair p0 + i into LDS at its offset inside the run (the run starts at
// LDS byte (run start & 15), so 16-byte aligned text is 16-byte aligned in LDS), then the wave copies the run out: whole aligned
// 16-byte chunks, single bytes at the two ends (shared with the neighbouring runs).  A run longer than the LDS (very long reads)
// is written lane by lane straight to memory instead.
__global__ void __launch_bounds__(64) k_truth_emit(TruthArgs A, const uint64_t* __restrict__ offs, uint32_t ppb, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    char* s_run = reinterpret_cast<char*>(s_run4);
    const uint32_t p0 = blockIdx.x * ppb, p1 = min(p0 + ppb, A.np);
    const uint64_t b0 = offs[p0], b1 = offs[p1];
    const uint32_t sh = (uint32_t)(b0 & 15u);
    const bool in_lds = b1 - b0 + sh <= (uint64_t)TRUTH_LDS;
    const uint32_t pi = p0 + threadIdx.x;
    if (threadIdx.x < ppb && pi < p1 && offs[pi + 1] > offs[pi]) {
        PtrOut o{in_lds ? s_run + sh + (offs[pi] - b0) : out + offs[pi]};
        truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t) { truth_record(o, a, li, src); });
    }
    if (!in_lds) return;
    __syncthreads();
    const uint64_t a0 = (b0 + 15u) & ~15ull, a1 = b1 & ~15ull;
    if (a0 >= a1) { for (uint64_t x = b0 + threadIdx.x; x < b1; x += 64u) out[x] = s_run[sh + (x - b0)]; return; }
    for (uint64_t x = b0 + threadIdx.x; x < a0; x += 64u) out[x] = s_run[sh + (x - b0)];
    for (uint64_t x = a1 + threadIdx.x; x < b1; x += 64u) out[x] = s_run[sh + (x - b0)];
    for (uint64_t x = a0 + 16u * threadIdx.x; x < a1; x += 1024u) *reinterpret_cast<uint4*>(out + x) = s_run4[(sh + (x - b0)) >> 4];
}

// ---- the truth BAM (scs_set_truth_bam): the same two passes over the same loads, the records in BAM's encoding
#define TRUTH_BAM_LDS 49152u                               // bytes of one workgroup's run of BAM records (3 workgroups per CU)

struct BamOut {                                            // a pair's records into LDS
    uint8_t* b; uint32_t n;
    __device__ void put(uint8_t v) { b[n++] = v; }
    __device__ uint32_t pos() const { return n; }
    __device__ void poke32(uint32_t at, uint32_t v) { b[at] = (uint8_t)v; b[at + 1] = (uint8_t)(v >> 8); b[at + 2] = (uint8_t)(v >> 16); b[at + 3] = (uint8_t)(v >> 24); }
};

__global__ void __launch_bounds__(256) k_truth_bam_size(TruthArgs A, uint32_t* __restrict__ sizes) {
    const uint32_t pi = blockIdx.x * 256u + threadIdx.x;
    if (pi >= A.np) return;
    uint32_t n = 0;
    truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t) { n += truth_bam_size(a, li, src); });
    sizes[pi] = n;
}

// one workgroup (one wave) per `ppb` <= 64 pairs, as k_truth_emit: lane i formats pair p0 + i into LDS at its offset inside the run,
// the wave copies the run out in whole aligned 16-byte chunks (single bytes at the two ends).  The run is cut where it would outgrow
// `lds` bytes: the wave then takes the lanes that fit, copies them out and goes on with the rest (one turn of the loop for the
// shipped read lengths; SCS_TEST_TRUTH_LDS makes it several).  A pair that alone outgrows the LDS raises FLAG_TRUTH.
__global__ void __launch_bounds__(64) k_truth_bam_emit(TruthArgs A, const uint64_t* __restrict__ offs, uint32_t ppb, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    uint8_t* s_run = reinterpret_cast<uint8_t*>(s_run4);
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
        if (fits && my1 > my0) {
            BamOut o{s_run + sh + (uint32_t)(my0 - b0), 0u};
            truth_pair(A, pi, [&](const TruthAln& a, const TruthLine& li, const DevSrc& src, uint32_t ref) { truth_bam_record(o, a, li, src, (int32_t)ref); });
            if (o.n != (uint32_t)(my1 - my0)) atomicOr(A.flags, (uint32_t)FLAG_TRUTH);   // (the sizing pass and the formatter disagree: never a silent wrong file)
        }
        __syncthreads();
        const uint64_t a0 = (b0 + 15u) & ~15ull, a1 = b1 & ~15ull;
        if (a0 >= a1) { for (uint64_t x = b0 + threadIdx.x; x < b1; x += 64u) out[x] = (char)s_run[sh + (x - b0)]; }
        else {
            for (uint64_t x = b0 + threadIdx.x; x < a0; x += 64u) out[x] = (char)s_run[sh + (x - b0)];
            for (uint64_t x = a1 + threadIdx.x; x < b1; x += 64u) out[x] = (char)s_run[sh + (x - b0)];
            for (uint64_t x = a0 + 16u * threadIdx.x; x < a1; x += 1024u) *reinterpret_cast<uint4*>(out + x) = s_run4[(sh + (x - b0)) >> 4];
        }
        __syncthreads();                                   // (the next turn writes the LDS this one has just read)
        first = last;
    }
}

void launch_truth_bam_size(hipStream_t s, const TruthArgs& a, uint32_t* sizes) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_bam_size, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
uint32_t truth_bam_pairs_per_block(uint64_t fq_bytes, uint32_t np) {
    // a record is 36 bytes of head, name, CIGAR and tags (about 90 with a short MD string) plus 1.5 bytes per base; its FASTQ record 2 per base
    const uint64_t est = (np ? fq_bytes / np : 0) * 3 / 4 + 192;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, TRUTH_BAM_LDS / est));
}
void launch_truth_bam_emit(hipStream_t s, const TruthArgs& a, const uint64_t* offs, uint32_t ppb, uint32_t lds, char* out) {
    if (a.np == 0) return;
    lds = lds ? std::min(lds, TRUTH_BAM_LDS) : TRUTH_BAM_LDS;
    hipLaunchKernelGGL(k_truth_bam_emit, dim3(cdiv(a.np, ppb)), dim3(64), TRUTH_BAM_LDS, s, a, offs, ppb, lds, out);
    note_launch(hipGetLastError());
}

void launch_truth_size(hipStream_t s, const TruthArgs& a, uint32_t* sizes) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_size, dim3(cdiv(a.np, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
uint32_t truth_pairs_per_block(uint64_t fq_bytes, uint32_t np) {
    // a record is its FASTQ record (name, bases, qualities) plus about 80 bytes of fields and tags (and the MD string)
    const uint64_t est = (np ? fq_bytes / np : 0) * 5 / 4 + 192;
    uint32_t ppb = 64;
    while (ppb > 1 && ppb * est > TRUTH_LDS) ppb >>= 1;
    return ppb;
}
void launch_truth_emit(hipStream_t s, const TruthArgs& a, const uint64_t* offs, uint32_t ppb, char* out) {
    if (a.np == 0) return;
    hipLaunchKernelGGL(k_truth_emit, dim3(cdiv(a.np, ppb)), dim3(64), TRUTH_LDS, s, a, offs, ppb, out);
    note_launch(hipGetLastError());
}

}  // namespace scs
