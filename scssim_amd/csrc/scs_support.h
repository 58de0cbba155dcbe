// scs_support.h -- the site support counters (scs_set_site_support): what one placed read shows at the listed
// genome positions (the artefact sites' coordinates).  One definition for the kernel (scs_k_support.hip) and its host probe
// (scs_support_read_probe), so the test seam runs the code the product runs.
//
// Per position six classes: 0..3 the read's aligned base there is A, C, G, T (genome-forward: a read whose window runs backwards
// shows the complement of its FASTQ base, as the truth SAM's SEQ does), 4 any other character, 5 the position lies inside a D of
// the truth CIGAR (truth_cigar_walk: leading and trailing deletions dropped).  Inserted bases align to no position.
#pragma once
#include <stdint.h>
#include "scs_truth.h"

namespace scs {

SCS_HD uint32_t support_class(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// the first of the n ascending values that is >= x (n: none)
SCS_HD uint64_t support_first_ge(const uint64_t* v, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (v[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// What a placed read (truth_place has run; a.lo >= 0) shows at the listed positions pos[0 .. n_pos) (global genome indices,
// ascending, distinct): rep(position index, class) for every listed position in [a.lo, a.hi], in ascending order, each once.
// seq(i) = the FASTQ record's base i (read orientation).  One bisection, then the operations of the CIGAR and the positions they
// cover: never a loop over the read's bases
template <class Seq, class Rep>
SCS_HD void support_read(const TruthAln& a, const uint64_t* pos, uint64_t n_pos, Seq seq, Rep rep) {
    uint64_t i = support_first_ge(pos, n_pos, (uint64_t)a.lo);
    if (i >= n_pos || pos[i] > (uint64_t)a.hi) return;
    uint64_t g = (uint64_t)a.lo; uint32_t qi = 0; const uint32_t q = (uint32_t)a.qlen;
    truth_cigar_walk(a, [&](char k, uint32_t l) {
        if (k == 'I') { qi += l; return; }
        const uint64_t end = g + l;
        for (; i < n_pos && pos[i] < end; ++i) {
            if (k == 'D') { rep(i, 5u); continue; }
            const uint32_t at = qi + (uint32_t)(pos[i] - g);
            rep(i, support_class(a.rev ? truth_comp(seq((int)(q - 1u - at))) : seq((int)at)));
        }
        g = end; if (k == 'M') qi += l;
    });
}

}  // namespace scs
