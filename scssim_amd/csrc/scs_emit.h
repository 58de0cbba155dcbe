// scs_emit.h -- the emit pass of every text or record stream the GPU formats (truth SAM / BAM / reference SAM, amplicon table,
// artefact and support tables).  Each stream takes the same three steps: a SIZING pass counts every record's bytes with a counting
// sink (TruthCount), a 64-bit exclusive scan turns the counts into offsets, and the EMIT pass formats the records again, now into
// LDS, and copies a workgroup's contiguous run out in whole 16-byte aligned stores (a lane writing its record byte by byte would
// leave partial sectors all over the text: the cost k_reads pays for its lane-private records).  The LDS image of a run begins at
// the 16-byte aligned text byte `wa` at or below the run's first byte, so text byte x lies at LDS byte x - wa and aligned text is
// aligned in LDS.  Two schemes share the copy-out:
//   emit_runs     one wave per up to 64 records, each formatted ONCE at its place in LDS; the run is cut where it would outgrow
//                 the LDS (the truth BAM and reference SAM: a pair's records are some hundred bytes and costly to format).  The
//                 truth SAM's k_truth_emit takes its run in one turn, or writes it lane by lane straight to memory: the cut-run
//                 loop around its formatter needs 195 VGPRs or more where the one turn needs 162 (3 waves per SIMD)
//   emit_windows  256 lanes, a WINDOW of the LDS' size moved over the workgroup's text; a lane formats its line once per window
//                 the line touches and keeps the bytes that fall inside (the tables: short lines, none too long for the LDS)
// Both compare what a lane wrote with what the sizing pass counted and raise the caller's flag on a difference: never a silent
// wrong file.  Device only; needs scs_device.h before it.
#pragma once

namespace scs {

// [c0, c1) of the text from the LDS image whose byte 0 is text byte wa (16-byte aligned, wa <= c0) to out, by the NT lanes of the
// workgroup: single bytes up to the first aligned address and from the last one (those chunks are shared with the neighbouring
// runs), whole uint4 stores between.  out itself is 16-byte aligned.  The caller puts a barrier before it and one behind it
template <uint32_t NT>
__device__ __forceinline__ void emit_copy_out(const uint4* s_run4, uint64_t wa, uint64_t c0, uint64_t c1, char* __restrict__ out) {
    const char* s_run = reinterpret_cast<const char*>(s_run4);
    const uint64_t a0 = (c0 + 15u) & ~15ull, a1 = c1 & ~15ull;
    if (a0 >= a1) { for (uint64_t x = c0 + threadIdx.x; x < c1; x += NT) out[x] = s_run[x - wa]; return; }
    for (uint64_t x = c0 + threadIdx.x; x < a0; x += NT) out[x] = s_run[x - wa];
    for (uint64_t x = a1 + threadIdx.x; x < c1; x += NT) out[x] = s_run[x - wa];
    for (uint64_t x = a0 + 16u * threadIdx.x; x < a1; x += 16u * NT) *reinterpret_cast<uint4*>(out + x) = s_run4[(x - wa) >> 4];
}

// where the LDS image of a run that starts at text byte b0 begins: the 16-byte aligned text byte at or below it
__device__ __forceinline__ uint64_t emit_base(uint64_t b0) { return b0 & ~15ull; }

// a record's bytes from p on (LDS, or the output itself): what the formatters of scs_truth.h and scs_truth_ref.h write through
struct RunOut {
    char* p; uint32_t n;
    __device__ void put(char ch) { p[n++] = ch; }
    __device__ uint32_t pos() const { return n; }
    __device__ void poke32(uint32_t at, uint32_t v) { p[at] = (char)v; p[at + 1] = (char)(v >> 8); p[at + 2] = (char)(v >> 16); p[at + 3] = (char)(v >> 24); }
};

// a line into the window [w0, w1) of the text, which lies in LDS from s on: the bytes outside are counted, not kept
struct WinOut {
    char* s; uint64_t pos, w0, w1;
    __device__ void put(char ch) { if (pos >= w0 && pos < w1) s[pos - w0] = ch; ++pos; }
};

// EVERY lane of the workgroup enters emit_runs, whether or not it has a record: the loop holds ballots and barriers.
// The workgroup is ONE WAVE (64 lanes) that owns the nl <= 64 records p0 .. p0 + nl - 1; record p0 + i lies at offs[p0 + i] ..
// offs[p0 + i + 1] of out and is lane i's.  Per turn the wave takes the lanes whose records fit `lds` bytes behind wa (a ballot
// over the ascending offsets: they are first, first + 1, ...); each formats its record through fmt(record, RunOut&) at its place
// in LDS; then barrier, copy-out, barrier, and the next turn starts behind the last lane taken (one turn for the shipped read
// lengths).  A record that alone outgrows `lds` raises `flag` and the workgroup leaves.  lds: at most the dynamic LDS behind s_run4
template <class Fmt>
__device__ __forceinline__ void emit_runs(uint4* s_run4, const uint64_t* __restrict__ offs, uint32_t p0, uint32_t nl, uint32_t lds, char* __restrict__ out,
                                          uint32_t* flags, uint32_t flag, Fmt fmt) {
    char* s_run = reinterpret_cast<char*>(s_run4);
    const uint32_t pi = p0 + threadIdx.x; const bool mine = threadIdx.x < nl;
    const uint64_t my0 = mine ? offs[pi] : 0, my1 = mine ? offs[pi + 1] : 0;
    for (uint32_t first = 0; first < nl;) {
        const uint64_t b0 = offs[p0 + first], wa = emit_base(b0);
        const bool fits = mine && threadIdx.x >= first && my1 - wa <= (uint64_t)lds;   // (offsets ascend: the lanes that fit are first, first + 1, ...)
        const uint32_t last = first + (uint32_t)__popcll(__ballot(fits));
        if (last == first) { if (threadIdx.x == 0) atomicOr(flags, flag); return; }    // (the wave's: every lane sees the same ballot)
        if (fits && my1 > my0) {
            RunOut o{s_run + (uint32_t)(my0 - wa), 0u};
            fmt(pi, o);
            if (o.n != (uint32_t)(my1 - my0)) atomicOr(flags, flag);   // (the sizing pass and the formatter disagree)
        }
        __syncthreads();
        emit_copy_out<64>(s_run4, wa, b0, offs[p0 + last], out);
        __syncthreads();                                   // (the next turn writes the LDS this one has just read)
        first = last;
    }
}

// the workgroup's text [b0, b1) and this lane's line [my0, my1) in it (my0 == my1: the lane has none): entries j0 .. j1 - 1 of offs
struct EmitSpan { uint64_t b0, b1, my0, my1; };
__device__ __forceinline__ EmitSpan emit_span(const uint64_t* __restrict__ offs, uint64_t j0, uint64_t j1) {
    const uint64_t j = j0 + threadIdx.x; const bool mine = j < j1;
    return EmitSpan{offs[j0], offs[j1], mine ? offs[j] : 0ull, mine ? offs[j + 1] : 0ull};
}

// EVERY lane of the workgroup (256) enters emit_windows: sp.b0, sp.b1 and lds are the workgroup's, so every lane takes every turn
// and its two barriers.  Window by window (lds bytes from wa on; lds a multiple of 16) the lanes with ok whose line touches the
// window format it through fmt(WinOut&), then the workgroup copies the window's part of its text out.  One window for most
// workgroups
template <class Fmt>
__device__ __forceinline__ void emit_windows(uint4* s_run4, const EmitSpan& sp, bool ok, uint32_t lds, char* __restrict__ out, uint32_t* flags, uint32_t flag, Fmt fmt) {
    for (uint64_t wa = emit_base(sp.b0); wa < sp.b1; wa += lds) {
        const uint64_t c0 = wa > sp.b0 ? wa : sp.b0, c1 = wa + lds < sp.b1 ? wa + lds : sp.b1;
        if (ok && sp.my0 < c1 && sp.my1 > c0) {
            WinOut o{reinterpret_cast<char*>(s_run4), sp.my0, wa, wa + lds};
            fmt(o);
            if (o.pos != sp.my1) atomicOr(flags, flag);    // (the sizing pass and the formatter disagree)
        }
        __syncthreads();
        emit_copy_out<256>(s_run4, wa, c0, c1, out);
        __syncthreads();                                   // (the next turn writes the LDS this one has just read)
    }
}

}  // namespace scs
