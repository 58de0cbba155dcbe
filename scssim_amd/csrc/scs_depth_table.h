// scs_depth_table.h -- the per-workgroup sum table of the depth kernels (k_depth, scs_k_depth.hip; k_depth_lift, scs_k_lift.hip):
// an open-addressing table in LDS (key = the global bin, < 2^27 + 1; two uint32 sums per slot, at most 512 reads x L bases each:
// no overflow).  A lane that finds no free slot within DEPTH_PROBES steps adds to memory itself, so a full table costs time, never
// a count.  slots = 0: no table, every add goes to memory.  depth_table_run is the two kernels' shell: the table cleared, the
// per-pair body, every used slot added to memory once.  Device code only: include it behind scs_device.h.
#pragma once
#include <stdint.h>
#include "scs_depth.h"

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

// A workgroup of 256 threads: its table of `slots` entries (a power of two up to DEPTH_LDS_SLOTS, or 0: table_slots) cleared,
// body(T) in every lane (no lane leaves before the barriers: a lane without work does nothing in body), then one 64-bit atomic per
// used slot and counter
template <class Body>
__device__ __forceinline__ void depth_table_run(uint32_t slots, unsigned long long* g_reads, unsigned long long* g_bases, Body body) {
    __shared__ uint32_t s_key[DEPTH_LDS_SLOTS], s_reads[DEPTH_LDS_SLOTS], s_bases[DEPTH_LDS_SLOTS];
    for (uint32_t i = threadIdx.x; i < slots; i += 256u) { s_key[i] = DEPTH_EMPTY; s_reads[i] = 0u; s_bases[i] = 0u; }
    __syncthreads();
    body(DepthTable{s_key, s_reads, s_bases, slots, g_reads, g_bases});
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < slots; i += 256u) {
        const uint32_t bin = s_key[i];
        if (bin == DEPTH_EMPTY) continue;
        if (s_reads[i]) atomicAdd(&g_reads[bin], (unsigned long long)s_reads[i]);
        if (s_bases[i]) atomicAdd(&g_bases[bin], (unsigned long long)s_bases[i]);
    }
}

}  // namespace scs
