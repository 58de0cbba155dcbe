// scs_depth.h -- the depth track (scs_set_depth): the bins of the staged records and what one placed read
// adds to them.  One definition for the ctx and its host probe (depth_layout / scs_depth_layout_probe) and for the kernel and its
// host probe (depth_read: scs_k_depth.hip / scs_depth_read_probe), so the test seams run the code the product runs.
//
// Bins of `bin_width` bases, record by record in staging order; a record's last bin may be short, no bin straddles two records.
// Per bin: `reads` = the reads whose leftmost aligned genome base (SAM POS - 1, TruthAln::lo) lies in it; `bases` = the genome
// bases in it that an M operation of the truth CIGAR aligns to a read base (D and I count nothing).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "scs_truth.h"

namespace scs {

#define DEPTH_MAX_BINS (1ull << 27)                        // two uint64 counters per bin: 2 GB at the cap
#define DEPTH_LDS_SLOTS 512u                               // entries of a workgroup's LDS table

// bins of all records at this width, or DEPTH_MAX_BINS + 1 when there are more (no overflow whatever the lengths)
inline uint64_t depth_count_bins(const uint64_t* lens, size_t n, uint64_t w) {
    uint64_t b = 0;
    for (size_t r = 0; r < n; ++r) {
        const uint64_t k = lens[r] / w + (lens[r] % w ? 1u : 0u);
        if (k > DEPTH_MAX_BINS || b + k > DEPTH_MAX_BINS) return DEPTH_MAX_BINS + 1;
        b += k;
    }
    return b;
}
// the layout: bin_off[r] = first bin of record r (n + 1 entries; may be NULL), *n_bins = their total.  false: bin_width is 0, or
// there are more than DEPTH_MAX_BINS bins; *min_width then receives the smallest admissible width (0: none below 2^32)
inline bool depth_layout(const uint64_t* lens, size_t n, uint32_t bin_width, uint64_t* bin_off, uint64_t* n_bins, uint32_t* min_width) {
    if (min_width) *min_width = 1;
    if (bin_width == 0) return false;
    if (depth_count_bins(lens, n, bin_width) > DEPTH_MAX_BINS) {
        uint64_t lo = (uint64_t)bin_width + 1, hi = 0xFFFFFFFFull;                  // the count does not grow with the width: bisect
        if (depth_count_bins(lens, n, hi) > DEPTH_MAX_BINS) lo = 0;
        else while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (depth_count_bins(lens, n, mid) <= DEPTH_MAX_BINS) hi = mid; else lo = mid + 1; }
        if (min_width) *min_width = (uint32_t)lo;
        return false;
    }
    uint64_t b = 0;
    for (size_t r = 0; r < n; ++r) { if (bin_off) bin_off[r] = b; b += lens[r] / bin_width + (lens[r] % bin_width ? 1u : 0u); }
    if (bin_off) bin_off[n] = b;
    if (n_bins) *n_bins = b;
    return true;
}

// What a placed read (truth_place has run) adds to the bins of its record: first(bin) once, the bin of its leftmost aligned base,
// then run(bin, bases) for every bin it has aligned bases in, in ascending order, each bin once.  rec0 = genome index of the
// record's first base; bins are counted inside the record.  The M runs of the truth CIGAR (truth_cigar_walk: leading and trailing
// deletions dropped) are cut at the bin boundaries; one division per read, and one more per deletion that leaves its bin.
template <class First, class Run>
SCS_HD void depth_read(const TruthAln& a, int64_t rec0, uint32_t bin_width, First first, Run run) {
    const uint64_t w = bin_width;
    uint64_t g = (uint64_t)(a.lo - rec0), bin = g / w, next = (bin + 1) * w;       // next: first coordinate of the following bin
    uint64_t cur = bin; uint32_t acc = 0;
    first(bin);
    truth_cigar_walk(a, [&](char k, uint32_t l) {
        if (k == 'I') return;
        if (k == 'D') { g += l; if (g >= next) { bin = g / w; next = (bin + 1) * w; } return; }
        while (l) {
            const uint32_t take = (uint64_t)l < next - g ? l : (uint32_t)(next - g);
            if (bin != cur) { if (acc) run(cur, acc); cur = bin; acc = 0; }
            acc += take; g += take; l -= take;
            if (g == next) { ++bin; next += w; }
        }
    });
    if (acc) run(cur, acc);
}

}  // namespace scs
