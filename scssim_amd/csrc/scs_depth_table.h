// scs_depth_table.h -- the per-workgroup sum table of the depth kernels (k_depth, scs_k_depth.hip; k_depth_lift, scs_k_lift.hip):
// an open-addressing table in LDS (key = the global bin, < 2^27 + 1; two uint32 sums per slot, at most 512 reads x L bases each:
// no overflow).  A lane that finds no free slot within DEPTH_PROBES steps adds to memory itself, so a full table costs time, never
// a count.  slots = 0: no table, every add goes to memory.  Device code only: include it behind scs_device.h.
#pragma once
#include <stdint.h>

namespace scs {

#define DEPTH_EMPTY 0xFFFFFFFFu                            // (a bin index is at most 2^27)
#define DEPTH_PROBES 16u

struct DepthTable {
    uint32_t* key; uint32_t* reads; uint32_t* bases; uint32_t slots;
    unsigned long long* g_reads; unsigned long long* g_bases;
    __device__ void add(uint32_t bin, uint32_t dr, uint32_t db) const {
        uint32_t h = bin & (slots - 1u);                   // neighbouring bins in neighbouring slots (slots = 0: no turn of the loop)
        for (uint32_t p = 0; p < DEPTH_PROBES && p < slots; ++p, h = (h + 1u) & (slots - 1u)) {
            const uint32_t was = atomicCAS(&key[h], DEPTH_EMPTY, bin);
            if (was != DEPTH_EMPTY && was != bin) continue;
            if (dr) atomicAdd(&reads[h], dr);
            if (db) atomicAdd(&bases[h], db);
            return;
        }
        if (dr) atomicAdd(&g_reads[bin], (unsigned long long)dr);
        if (db) atomicAdd(&g_bases[bin], (unsigned long long)db);
    }
};

}  // namespace scs
