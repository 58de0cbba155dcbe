// scs_gcbias.h -- the GC-bias table of the per-base depth (scs_gc_bias ...): which row a window of the staged
// genome adds to, and what the host derives from a row.  One definition for the kernel (scs_k_gcbias.hip) and for the file
// (scs_gcbias.cpp), so a table and its file cannot disagree about a bin.
//
// A window is W neighbouring bases of one staged record, W in 1 .. GCB_MAX_WINDOW; windows slide by one base.  One that holds an N
// is counted in n_windows and nowhere else.  Every other one adds 1 to windows[b] and the sum of its W depths to depth_sum[b],
// b = gcb_bin(gc, W), gc its G or C bases: the simulator's own formula for an amplicon (100 * gc / len; k_weights,
// scs_k_allocate.hip), so row b stands beside the model's gc_means[b].
#pragma once
#include <stdint.h>
#include "scs_common.h"

namespace scs {

#define GCB_BINS 101u                                      // rows of a table: b = 0 .. 100
#define GCB_MAX_WINDOW 1024u                               // the widest window; tile plus halo then is COV_TILE + 1023 entries

// gc is clamped to the window: whatever the arrays hold, b indexes inside a row
SCS_HD uint32_t gcb_bin(uint32_t gc, uint32_t window) { return 100u * (gc < window ? gc : window) / window; }

// What the host derives from one row (windows[b], depth_sum[b], b = 0 .. 100) at window W, as doubles:
//   mean[b]        depth_sum[b] / (windows[b] * W), 0 for an empty bin
//   row_mean       sum_b depth_sum / (W * sum_b windows), 0 for an empty row
//   normalized[b]  mean[b] / row_mean (Picard's normalized coverage, on aligned bases), 0 where row_mean is 0
struct GcbRow { uint64_t n; double row_mean, mean[GCB_BINS], normalized[GCB_BINS]; };
inline GcbRow gcb_row(const uint64_t* windows, const uint64_t* depth_sum, uint32_t window) {
    GcbRow o; o.n = 0; o.row_mean = 0.0;
    uint64_t all = 0;
    for (uint32_t b = 0; b < GCB_BINS; ++b) { o.n += windows[b]; all += depth_sum[b]; }
    if (o.n) o.row_mean = (double)all / ((double)window * (double)o.n);
    for (uint32_t b = 0; b < GCB_BINS; ++b) {
        o.mean[b] = windows[b] ? (double)depth_sum[b] / ((double)windows[b] * (double)window) : 0.0;
        o.normalized[b] = o.row_mean > 0.0 ? o.mean[b] / o.row_mean : 0.0;
    }
    return o;
}

#if defined(__HIPCC__)
// ---- the kernel (scs_k_gcbias.hip).  depth: n_bases entries, readable up to depth_alloc (a multiple of 4: the array's padding);
// codes: n_bases bytes and nothing behind them; rec_off: the records' starts (n_rec + 1, the last one n_bases).  windows and
// depth_sum: n_rec rows of GCB_BINS, n_windows: n_rec entries, all zeroed by the caller and added to.  lds: 0 -- a workgroup keeps
// no table in LDS, every add goes to memory.  Both arrays are only read
struct GcBiasArgs {
    const uint32_t* depth; uint64_t depth_alloc; const uint8_t* codes; uint64_t n_bases; const uint64_t* rec_off; uint32_t n_rec, window, lds;
    unsigned long long* windows; unsigned long long* depth_sum; unsigned long long* n_windows;
};
void launch_gc_bias(hipStream_t s, const GcBiasArgs& a);
#endif

}  // namespace scs
