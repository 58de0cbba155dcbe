// scs_alloc_plan.h -- the read allocation's host plan: where the chunks of the whole job's amplicon list lie relative to one
// shard's list.  Plain host code: no device, no ctx; do_allocate (scs_reads.cpp) and scs_alloc_plan_probe run it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace scs {
// ---- read allocation over the whole job's amplicon list, computed by the shards (scs_k_allocate.hip, K3) ---------------
// The list is cut into chunks of 1000 (randIndx_hp's chunks, MyDefine.cpp:203-253).  A shard's local list is the
// concatenation of its segments (cycle ascending, fragment pass descending: slot = cycle * 8 + (7 - pass)); the whole
// job's list interleaves the shards' segments slot by slot (order = slot * shards + rank).
#define ALLOC_CHUNK 1000u
enum { ALLOC_SLOTS = 40 };
struct AllocRange { uint32_t q0, c0, local0; };            // work chunks q0.. (up to the next range) = whole-job chunks c0.., in place at local0 + 1000 (q - q0)
struct AllocBChunk { uint32_t c, n, owner; };              // a chunk that straddles a segment boundary: materialised row; owner: this shard holds its first amplicon
struct AllocGSeg { unsigned long long go; uint32_t lo, n, owner, slot; };   // every non-empty segment of every shard, in list order
struct AllocMySeg { unsigned long long go; uint32_t lo, n, order, pad; };  // this shard's segment of slot s

// doubles of scratch that launch_tree_sum and launch_alloc_quota's scan_all share, for nch chunk partials
inline size_t alloc_tree_scratch(size_t nch) { return nch / ALLOC_CHUNK * 3 + 4096; }

// the plan of shard `me`: total amplicons and chunks of the job, this shard's amplicons (ac), its interior ranges (n_interior whole
// chunks read in place), its boundary chunks, every shard's segments in list order, and its own segment of every slot
struct AllocHostPlan {
    uint64_t total = 0; uint32_t nch = 0, n_interior = 0, ac = 0;
    std::vector<AllocRange> rng; std::vector<AllocBChunk> bch; std::vector<AllocGSeg> gseg;
    AllocMySeg my_seg[ALLOC_SLOTS];
};
// segc[r * ALLOC_SLOTS + slot] = amplicons of shard r in that slot, R shards.  false: more than 2^32 amplicons in the whole job
inline bool alloc_plan_build(const uint64_t* segc, int R, int me, AllocHostPlan& P) {
    std::vector<AllocGSeg>& gseg = P.gseg; std::vector<uint32_t> loff((size_t)R, 0); uint64_t total = 0;
    gseg.clear(); P.rng.clear(); P.bch.clear();
    for (int sl = 0; sl < ALLOC_SLOTS; ++sl) for (int r = 0; r < R; ++r) {
        const uint64_t n = segc[(size_t)r * ALLOC_SLOTS + sl];
        if (r == me) P.my_seg[sl] = AllocMySeg{total, loff[r], (uint32_t)n, (uint32_t)(sl * R + r), 0};
        if (!n) continue;
        gseg.push_back(AllocGSeg{total, loff[r], (uint32_t)n, (uint32_t)r, (uint32_t)sl});
        loff[r] += (uint32_t)n; total += n;
        if (total > 0xFFFFFFF0ull) return false;
    }
    P.total = total; P.ac = loff[me];
    const uint32_t nch = P.nch = (uint32_t)((total + ALLOC_CHUNK - 1) / ALLOC_CHUNK);
    std::vector<AllocRange>& rng = P.rng; std::vector<AllocBChunk>& bch = P.bch; uint32_t nq = 0;
    auto owner_of = [&](uint64_t gi) { size_t lo = 0, hi = gseg.size(); while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (gseg[mid].go <= gi) lo = mid; else hi = mid; } return gseg[lo].owner; };
    auto add_boundary = [&](uint32_t ch) { for (auto& b : bch) if (b.c == ch) return; bch.push_back(AllocBChunk{ch, (uint32_t)std::min<uint64_t>(ALLOC_CHUNK, total - (uint64_t)ch * ALLOC_CHUNK), owner_of((uint64_t)ch * ALLOC_CHUNK) == (uint32_t)me ? 1u : 0u}); };
    for (size_t k = 0; k < gseg.size();) {                                    // my segments, merged while they are contiguous in the whole list
        if (gseg[k].owner != (uint32_t)me) { ++k; continue; }
        uint64_t go = gseg[k].go, n = gseg[k].n; const uint32_t lo = gseg[k].lo; size_t j = k + 1;
        while (j < gseg.size() && gseg[j].owner == (uint32_t)me && gseg[j].go == go + n) { n += gseg[j].n; ++j; }
        k = j;
        const uint64_t cA = (go + ALLOC_CHUNK - 1) / ALLOC_CHUNK, cB = go + n == total ? nch : (go + n) / ALLOC_CHUNK;   // whole chunks inside [go, go+n)
        if (cA < cB) { rng.push_back(AllocRange{nq, (uint32_t)cA, (uint32_t)(lo + (cA * ALLOC_CHUNK - go))}); nq += (uint32_t)(cB - cA); }
        if (cA >= cB) { for (uint64_t ch = go / ALLOC_CHUNK; ch <= (go + n - 1) / ALLOC_CHUNK; ++ch) add_boundary((uint32_t)ch); }   // shorter than a chunk (or two partial ones)
        else {
            if (go % ALLOC_CHUNK) add_boundary((uint32_t)(go / ALLOC_CHUNK));
            if (cB * ALLOC_CHUNK < go + n) add_boundary((uint32_t)cB);
        }
    }
    P.n_interior = nq;
    return true;
}
}  // namespace scs
