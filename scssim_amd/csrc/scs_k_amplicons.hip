// scs_k_amplicons.hip -- gfx950 kernels of the amplicon table (scs_amplicon_places / scs_write_amplicons):
// one entry per full amplicon of the list, made after scs_allocate_reads from what the device holds -- the fragment and amplicon
// tables, both error pools, the read numbers, the byte genome.  A thread per amplicon resolves it to an index map of the genome
// (amp_resolve: k_plan_pairs' resolution), finds its record by bisection and walks its edits (scs_amp.h).
//
// k_amp_place writes the binary form.  The text takes two passes over a chunk of amplicons, both running amp_line: the SIZING
// pass counts each line's bytes, a 64-bit exclusive scan gives the offsets, and the EMIT pass writes the ~45-byte lines by the
// windowed scheme of scs_emit.h (emit_windows): a line may straddle two windows and no line is too long for the LDS.
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_amp.h"
#include "scs_emit.h"

namespace scs {

struct AmpGen { const uint8_t* g; __device__ uint32_t operator()(int64_t x) const { return g[x]; } };

// amplicon first + j: its index map, its line's fields, its two error lists.  false: it cannot be made right (FLAG_AMP: a lineage
// that does not fit its parents, flags that are not a strand, an amplicon outside its record)
__device__ bool amp_load(const AmpArgs& A, uint32_t j, AmpPlace& p, AmpLine& li, AmpErrs& e1, AmpErrs& e2, uint32_t& rec) {
    const uint32_t i = A.first + j;
    const uint32_t fsl = A.fulls.sl[i], sm = A.fulls.parent[i], ssl = A.semis.sl[sm], f = A.semis.parent[sm];
    if (!amp_resolve(A.fr.goff[f], A.fr.len[f], A.fr.strand[f], sl_spos(ssl), sl_len(ssl), sl_spos(fsl), sl_len(fsl), p) || !amp_strand(p)) { atomicOr(A.flags, (uint32_t)FLAG_AMP); return false; }
    const int64_t x0 = amp_lo(p);
    const uint32_t lo = rec_of(A.rec_off, A.n_rec, x0);
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

// one workgroup per 256 amplicons (emit_windows): lane i formats the line of amplicon j0 + i
__global__ void __launch_bounds__(256) k_amp_emit(AmpArgs A, const uint64_t* __restrict__ offs, uint32_t lds, char* __restrict__ out) {
    extern __shared__ uint4 s_run4[];
    const uint32_t j0 = blockIdx.x * 256u;
    const EmitSpan sp = emit_span(offs, j0, min(j0 + 256u, A.n));
    AmpPlace p; AmpLine li; AmpErrs e1, e2; uint32_t r = 0;
    const bool ok = sp.my1 > sp.my0 && amp_load(A, j0 + threadIdx.x, p, li, e1, e2, r);
    emit_windows(s_run4, sp, ok, lds, out, A.flags, (uint32_t)FLAG_AMP, [&](WinOut& o) { amp_line(o, li, p, e1, e2, AmpGen{A.g}); });
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
    hipLaunchKernelGGL(k_amp_emit, dim3(cdiv(a.n, 256)), dim3(256), AMP_LDS, s, a, offs, emit_windows_lds(lds, AMP_LDS), out);
    note_launch(hipGetLastError());
}

}  // namespace scs
