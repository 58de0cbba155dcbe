// scs_k_amplicons.hip -- gfx950 kernels of the amplicon table (scs_amplicon_places / scs_write_amplicons):
// one entry per full amplicon of the list, made after scs_allocate_reads from what the device holds -- the fragment and amplicon
// tables, both error pools, the read numbers, the byte genome.  A thread per amplicon resolves it to an index map of the genome
// (amp_resolve: k_plan_pairs' resolution), finds its record by bisection and walks its edits (scs_amp.h).
//
// k_amp_place writes the binary form.  The text takes two passes over a chunk of amplicons, both running amp_line: the SIZING
// pass counts each line's bytes, a 64-bit exclusive scan gives the offsets, and the EMIT pass writes the lines.  The emit pass
// builds a workgroup's contiguous run of lines in LDS and copies it out in whole 16-byte aligned stores (a lane writing its ~45-byte
// line byte by byte would leave partial sectors all over the text: the cost k_reads pays for its lane-private records).  The run is
// a WINDOW of `lds` bytes over the workgroup's text: a lane formats its line once per window the line touches and keeps the bytes
// that fall inside, so a line may straddle two windows and no line is too long for the LDS.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_amp.h"

namespace scs {

struct AmpGen { const uint8_t* g; __device__ uint32_t operator()(int64_t x) const { return g[x]; } };

// amplicon first + j: its index map, its line's fields, its two error lists.  false: it cannot be made right (FLAG_AMP: a lineage
// that does not fit its parents, flags that are not a strand, an amplicon outside its record)
__device__ bool amp_load(const AmpArgs& A, uint32_t j, AmpPlace& p, AmpLine& li, AmpErrs& e1, AmpErrs& e2, uint32_t& rec) {
    const uint32_t i = A.first + j;
    const uint32_t fsl = A.fulls.sl[i], sm = A.fulls.parent[i], ssl = A.semis.sl[sm], f = A.semis.parent[sm];
    if (!amp_resolve(A.fr.goff[f], A.fr.len[f], A.fr.strand[f], sl_spos(ssl), sl_len(ssl), sl_spos(fsl), sl_len(fsl), p) || !amp_strand(p)) { atomicOr(A.flags, (uint32_t)FLAG_AMP); return false; }
    const int64_t x0 = amp_lo(p);
    uint32_t lo = 0, hi = A.n_rec;                         // the record: rec_off[lo] <= x0 < rec_off[lo + 1]
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)A.rec_off[mid] <= x0) lo = mid; else hi = mid; }
    const int64_t r0 = (int64_t)A.rec_off[lo], r1 = (int64_t)A.rec_off[lo + 1];
    if (x0 < r0 || x0 + (int64_t)p.len > r1) { atomicOr(A.flags, (uint32_t)FLAG_AMP); return false; }   // a fragment never straddles records
    rec = lo;
    li = AmpLine{A.names + A.name_off[lo], A.name_off[lo + 1] - A.name_off[lo], r0, i, sm, A.read_numbers[i]};
    e1 = AmpErrs{A.semis.errs[sm], A.spool}; e2 = AmpErrs{A.fulls.errs[i], A.fpool};
    return true;
}

__global__ void __launch_bounds__(256) k_amp_place(AmpArgs A, uint32_t* __restrict__ rec, uint64_t* __restrict__ start, uint32_t* __restrict__ len,
                                                   int8_t* __restrict__ strand, uint32_t* __restrict__ n_edits) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= A.n) return;
    AmpPlace p; AmpLine li; AmpErrs e1, e2; uint32_t r = 0;
    const bool ok = amp_load(A, j, p, li, e1, e2, r);
    if (rec) rec[j] = ok ? r : 0u;
    if (start) start[j] = ok ? (uint64_t)(amp_lo(p) - li.rec0) : 0ull;
    if (len) len[j] = ok ? p.len : 0u;
    if (strand) strand[j] = ok ? (int8_t)(p.dir > 0 ? 1 : -1) : (int8_t)0;
    if (n_edits) n_edits[j] = ok ? amp_edits(p, e1, e2, AmpGen{A.g}, [](int64_t, uint32_t, uint32_t) {}) : 0u;
}

__global__ void __launch_bounds__(256) k_amp_size(AmpArgs A, uint32_t* __restrict__ sizes) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= A.n) return;
    AmpPlace p; AmpLine li; AmpErrs e1, e2; uint32_t r = 0; TruthCount c;
    if (amp_load(A, j, p, li, e1, e2, r)) amp_line(c, li, p, e1, e2, AmpGen{A.g});
    sizes[j] = (uint32_t)c.n;
}

// a line into the window [w0, w1) of the chunk's text, which lies in LDS from s on: the bytes outside are counted, not kept
struct AmpWinOut {
    char* s; uint64_t pos, w0, w1;
    __device__ void put(char ch) { if (pos >= w0 && pos < w1) s[pos - w0] = ch; ++pos; }
};

// one workgroup per 256 amplicons: window by window (wa: 16-byte aligned, so aligned text is aligned in LDS) the lanes format the
// lines that touch the window, then the workgroup copies the window's part of its text out: whole aligned 16-byte chunks, single
// bytes at the two ends (shared with the neighbouring workgroups' text).  One window for most workgroups (256 lines of ~45 bytes)
__global__ void __launch_bounds__(256) k_amp_emit(AmpArgs A, const uint64_t* __restrict__ offs, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    char* s_run = reinterpret_cast<char*>(s_run4);
    const uint32_t j0 = blockIdx.x * 256u, j1 = min(j0 + 256u, A.n), j = j0 + threadIdx.x;
    const bool mine = j < j1;
    const uint64_t b0 = offs[j0], b1 = offs[j1], my0 = mine ? offs[j] : 0ull, my1 = mine ? offs[j + 1] : 0ull;
    AmpPlace p; AmpLine li; AmpErrs e1, e2; uint32_t r = 0;
    const bool ok = mine && my1 > my0 && amp_load(A, j, p, li, e1, e2, r);
    for (uint64_t wa = b0 & ~15ull; wa < b1; wa += lds) {  // (b0, b1 and lds are the workgroup's: every lane takes every turn)
        const uint64_t c0 = wa > b0 ? wa : b0, c1 = wa + lds < b1 ? wa + lds : b1;
        if (ok && my0 < c1 && my1 > c0) {
            AmpWinOut o{s_run, my0, wa, wa + lds};
            amp_line(o, li, p, e1, e2, AmpGen{A.g});
            if (o.pos != my1) atomicOr(A.flags, (uint32_t)FLAG_AMP);   // (the sizing pass and the formatter disagree: never a silent wrong file)
        }
        __syncthreads();
        const uint64_t a0 = (c0 + 15u) & ~15ull, a1 = c1 & ~15ull;
        if (a0 >= a1) { for (uint64_t x = c0 + threadIdx.x; x < c1; x += 256u) out[x] = s_run[x - wa]; }
        else {
            for (uint64_t x = c0 + threadIdx.x; x < a0; x += 256u) out[x] = s_run[x - wa];
            for (uint64_t x = a1 + threadIdx.x; x < c1; x += 256u) out[x] = s_run[x - wa];
            for (uint64_t x = a0 + 16u * threadIdx.x; x < a1; x += 4096u) *reinterpret_cast<uint4*>(out + x) = s_run4[(x - wa) >> 4];
        }
        __syncthreads();                                   // (the next turn writes the LDS this one has just read)
    }
}

void launch_amp_place(hipStream_t s, const AmpArgs& a, uint32_t* rec, uint64_t* start, uint32_t* len, int8_t* strand, uint32_t* n_edits) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_amp_place, dim3(cdiv(a.n, 256)), dim3(256), 0, s, a, rec, start, len, strand, n_edits);
    note_launch(hipGetLastError());
}
void launch_amp_size(hipStream_t s, const AmpArgs& a, uint32_t* sizes) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_amp_size, dim3(cdiv(a.n, 256)), dim3(256), 0, s, a, sizes);
    note_launch(hipGetLastError());
}
void launch_amp_emit(hipStream_t s, const AmpArgs& a, const uint64_t* offs, uint32_t lds, char* out) {
    if (a.n == 0) return;
    lds = lds ? std::min(lds, AMP_LDS) & ~15u : AMP_LDS;   // whole 16-byte chunks, at least one
    if (lds < 16u) lds = 16u;
    hipLaunchKernelGGL(k_amp_emit, dim3(cdiv(a.n, 256)), dim3(256), AMP_LDS, s, a, offs, lds, out);
    note_launch(hipGetLastError());
}

}  // namespace scs
