// scs_runs.h -- the run-length text of a per-base uint32 array (scs_write_coverage_bedgraph, scs_write_coverage_ref_bedgraph,
// scs_write_copy_number_ref): one bedGraph line `name\tstart\tend\tvalue\n` (0-based, half-open) per maximal
// run of equal masked value inside a record.  One definition of the line for the kernels (scs_k_runs.hip: the sizing pass through a
// counting sink, the emit pass into LDS) and the host probe (scs_runs_line_probe; tools/runs_host_check.cpp builds it alone under
// the sanitizers), so the test seam runs the code the product runs.  Nothing but scs_common.h is needed.
#pragma once
#include <stdint.h>
#include "scs_common.h"

namespace scs {

#define RUNS_LDS 16384u                                    // bytes of the emit pass' LDS window (emit_windows, scs_emit.h)
#define RUNS_LANE 16u                                      // neighbouring entries a lane owns: COV_TILE / 256
#define RUNS_NAME_MAX 65535u                               // the longest record name: a tile's 4096 lines then stay below 2^32 bytes
#define RUNS_TEXT_CAP (128ull << 20)                       // bytes of text a slab holds on the device (the seams build: SCS_TEST_RUNS_TEXT_CAP)

struct RunsCount { uint64_t n = 0; SCS_HD void put(char) { ++n; } };

template <class Out>
SCS_HD void runs_num(Out& o, uint64_t v) {
    char d[20]; int n = 0;
    if (v >> 32) { do { d[n++] = (char)('0' + v % 10u); v /= 10u; } while (v >> 32); }   // (positions beyond 2^32 are rare: the 64-bit division is theirs alone)
    uint32_t w = (uint32_t)v;
    do { d[n++] = (char)('0' + w % 10u); w /= 10u; } while (w);
    while (n) o.put(d[--n]);
}

// the line of the run [start, end) of record `name` at `value`, with its newline, through o.put(char)
template <class Out>
SCS_HD void runs_line(Out& o, const char* name, uint32_t name_len, uint64_t start, uint64_t end, uint32_t value) {
    for (uint32_t i = 0; i < name_len; ++i) o.put(name[i]);
    o.put('\t'); runs_num(o, start); o.put('\t'); runs_num(o, end); o.put('\t'); runs_num(o, value); o.put('\n');
}

// into out[0 .. cap): the bytes written, or (cap too small) the bytes the line needs with nothing trusted in out
struct RunsBuf { char* p; uint64_t cap, n; SCS_HD void put(char c) { if (n < cap) p[n] = c; ++n; } };

#if defined(__HIPCC__)
// ---- the kernels (scs_k_runs.hip).  values: n entries, readable up to runs_tiles(n) whole tiles of COV_TILE; the records' starts
// (n_rec + 1, the last one n), name offsets and names as RecTable lays them out (scs_textout.h).  Per tile: first (the local index
// of its first run start, COV_TILE: none), next (the first run start behind it, n: none), lines and bytes (tiles + 1 entries each:
// the scan reads one more).  launch_runs_plan fills all four; launch_runs_emit writes the text of tiles t0 .. t0 + tiles - 1 to out
// (16-byte aligned) at offs, the exclusive_scan_u32_to_u64 of bytes + t0; lds: the LDS window in bytes (0: RUNS_LDS).  FLAG_RUNS:
// the two passes sized a line differently
struct RunsArgs {
    const uint32_t* values; uint32_t mask; uint64_t n;
    const uint64_t* rec_off; const uint32_t* name_off; const char* names; uint32_t n_rec;
    uint32_t* first; uint64_t* next; uint32_t* lines; uint32_t* bytes; uint32_t* flags;
};
uint64_t runs_tiles(uint64_t n);
void launch_runs_plan(hipStream_t s, const RunsArgs& a);
void launch_runs_emit(hipStream_t s, const RunsArgs& a, uint32_t t0, uint32_t tiles, const uint64_t* offs, uint32_t lds, char* out);
#endif

}  // namespace scs
