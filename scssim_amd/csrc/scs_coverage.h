// scs_coverage.h -- the coverage profile (scs_set_coverage): per-base depth of the staged genome, its histogram
// per record and the summary a Lorenz curve is drawn from.  One definition for the per-batch kernel and its host probe (cov_read:
// k_cov_mark, scs_k_coverage.hip / scs_coverage_read_probe) and for the file and its host probe (cov_stats: scs_write_coverage /
// scs_coverage_stats_probe), so the test seams run the code the product runs.
//
// depth[g] = the (read, base) pairs an M operation of the truth CIGAR aligns to genome base g (D and I count nothing; the rules are
// the depth track's `bases`, scs_depth.h).  A read marks a difference array of G + 1 int32 entries: +1 where a run of aligned bases
// begins, -1 behind its last base; the end-of-job pass turns the array into depths with one prefix sum.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "scs_truth.h"

namespace scs {

#define COV_MAX_DEPTH 65535u                               // the largest max_depth (histogram rows of max_depth + 1 uint64)
#define COV_TILE 4096u                                     // entries of the difference array per workgroup of the end-of-job pass
#define COV_CHUNK 1024u                                    // tile sums per step of the one-workgroup offset scan
#define COV_LDS_BUCKETS 4096u                              // a workgroup's LDS histogram holds min(max_depth + 1, this) buckets
#define COV_REF_CN 16u                                     // on the reference (scs_set_coverage_ref): depth by copy number 0 .. this, the last one copies >= this
#define COV_REF_MAX_COPIES 65535u                          // ... and the staged bases that may lift to one reference base (16 bits of its packed word)

// the buckets of a workgroup's LDS histogram for a caller's `lds` (the launchers' clamp; 0: every count goes to memory)
inline uint32_t cov_lds_buckets(uint32_t lds, uint32_t max_depth) {
    const uint32_t n = lds < max_depth + 1u ? lds : max_depth + 1u;
    return n < COV_LDS_BUCKETS ? n : COV_LDS_BUCKETS;
}

// What a placed read (truth_place has run) marks: mark(g, +1), mark(g + l, -1) for every maximal run [g, g + l) of genome bases
// aligned to read bases, g a global genome index.  M runs that only an insertion separates are one run (an I moves nothing on the
// genome); a deletion ends a run.  Leading and trailing deletions are truth_cigar_walk's to drop.  Every index lies in
// [a.lo, a.hi + 1]
template <class Mark>
SCS_HD void cov_read(const TruthAln& a, Mark mark) {
    int64_t g = a.lo, run0 = -1;
    truth_cigar_walk(a, [&](char k, uint32_t l) {
        if (k == 'I') return;
        if (k == 'D') { if (run0 >= 0) { mark(run0, 1); mark(g, -1); run0 = -1; } g += l; return; }
        if (run0 < 0) run0 = g;
        g += l;
    });
    if (run0 >= 0) { mark(run0, 1); mark(g, -1); }
}

// The summary of one histogram row: hist[k], k = 0 .. D, counts the non-N bases of depth k, the last bucket those of depth >= D;
// sum = the exact sum of their depths, so the top bucket's mass is sum - sum_{k < D} k hist[k] whatever lies in it.
//   mean        sum / bases
//   breadth[i]  the fraction of bases at depth >= {1, 5, 10, 20}[i]; a threshold above D counts the top bucket (all that is known of
//               it is depth >= D: an upper bound)
//   gini        of the Lorenz curve over the buckets, the top bucket taken at its mean depth: 1 - sum_k n_k (S_{k-1} + S_k) / (n S)
//               with S_k the mass of the buckets up to k.  Exact when no base reaches D (every bucket then holds one depth); a lower
//               bound otherwise (bases of unequal depth are taken at their mean).  0 when all depths are 0 or there are no bases
struct CovStats { double mean, breadth[4], gini; };
inline CovStats cov_stats(const uint64_t* hist, uint32_t D, uint64_t sum) {
    CovStats s{0.0, {0.0, 0.0, 0.0, 0.0}, 0.0};
    uint64_t n = 0, below = 0;
    for (uint32_t k = 0; k <= D; ++k) { n += hist[k]; if (k < D) below += (uint64_t)k * hist[k]; }
    if (!n) return s;
    s.mean = (double)sum / (double)n;
    const uint32_t at[4] = {1u, 5u, 10u, 20u};
    for (int i = 0; i < 4; ++i) {
        uint64_t c = 0;
        for (uint32_t k = at[i] < D ? at[i] : D; k <= D; ++k) c += hist[k];
        s.breadth[i] = (double)c / (double)n;
    }
    if (!sum || sum < below) return s;                     // (sum < below: not a row of this layout; no Gini is better than a wrong one)
    double acc = 0.0; uint64_t S = 0;
    for (uint32_t k = 0; k <= D; ++k) {
        if (!hist[k]) continue;
        const uint64_t mass = k < D ? (uint64_t)k * hist[k] : sum - below;
        acc += (double)hist[k] * ((double)S + (double)(S + mass));
        S += mass;
    }
    s.gini = 1.0 - acc / ((double)n * (double)sum);
    return s;
}

}  // namespace scs
