// scs_indel.h -- phase 1 of Profile::predict on the device: the indel events of a read, drawn from its stream A.  Shared by
// k_indels / k_reads (scs_k_reads.hip) and the truth passes (scs_k_truth.hip), which re-draw the events of replayed reads with
// the same code.  Needs scs_device.h and scs_kernels_common.h before it.
#pragma once
namespace scs {
#define EV_MAX 8
// indel events, 16 bits: pos:10 | del:1 | len:5.  A read with an event that does not fit (position >= 1024, length
// >= 32, more than EV_MAX events) is "replayed": phase 2 re-draws its indel tests from stream A as it goes.
__device__ __forceinline__ uint32_t ev_pack(uint32_t pos, uint32_t del, uint32_t len) { return pos | (del << 10) | (len << 11); }
__device__ __forceinline__ uint32_t ev_pos(uint32_t v) { return v & 1023u; }
__device__ __forceinline__ uint32_t ev_del(uint32_t v) { return (v >> 10) & 1u; }
__device__ __forceinline__ uint32_t ev_len(uint32_t v) { return v >> 11; }

// [REMAP] number of event-free bases before the next indel event among the `rem` bases left: the per-base tests of
// getIndelSeq (Profile.cpp:1552-1570) are i.i.d. with probability p = t_indel / 2^32, so the gap is geometric and ONE draw
// x gives it: gap >= g <=> x < T[g], T[g] = floor((1-p)^g 2^32) (non-increasing, host-built: scs_tables.h).  Returns rem when
// no event falls among the bases left (86 % of 150-base reads with the shipped models: one compare).
__device__ __forceinline__ uint32_t indel_gap(const uint32_t* __restrict__ T, uint32_t x, uint32_t rem) {
    if (x < T[rem]) return rem;
    uint32_t lo = 1, hi = rem;                                                     // first g in [1, rem] with x >= T[g] (g = rem qualifies)
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (x >= T[mid]) hi = mid; else lo = mid + 1; }
    return lo - 1;
}
// phase 1 of Profile::predict: the indel events of a read (getIndelSeq, Profile.cpp:1552-1570 / loop 1606-1630): stream A
// gives, event by event, the gap to the next event and its kind; the length is a keyed Philox draw.
// put(i, v) stores event i (16 bits).  Returns n' (0 = the read does not fit its slot), the event count and the replay flag.
struct IndelPass { int n_out; int nev; bool replay; };
// RAW: every event goes to put(i, pos, del, len), whatever its position or length (the truth passes re-draw the events of a
// replayed read with it: the same draws by construction); the caps and the replay flag are the packed form's
template <bool RAW = false, class Put>
__device__ __forceinline__ IndelPass indel_pass(const DevTables& tb, RngKey key, uint32_t aux, uint64_t uid, uint32_t force_replay, uint32_t slot,
                                                uint32_t* __restrict__ flags, Put put) {
    const int n = tb.L; const uint32_t t_kind = tb.t_kind;
    int nev = 0, delta = 0; bool replay = false;
    Xoshiro xa; xa.seed(draw4(key, ST_READ, aux, uid, 0));                         // stream A: gap, kind, gap, kind, ...
    if (tb.t_indel) for (int ji = 0; ji < n;) {
        ji += (int)indel_gap(tb.gap_t, xa.next(), (uint32_t)(n - ji));
        if (ji >= n) break;
        const uint32_t y = xa.next();                                              // an event at base ji: insertion | deletion in the ratio of their rates
        const uint32_t x = draw4(key, ST_INDEL_LEN, aux, uid, (uint32_t)ji).w[0];
        if (y < t_kind) {
            const uint32_t k = rand_indx_thr(tb.ins_t, tb.ins_d, (uint32_t)tb.n_ins, x);
            if (k > 0) {
                if constexpr (RAW) put(nev, (uint32_t)ji, 0u, k);
                else if (nev < EV_MAX && ji < 1024 && k < 32u) put(nev, ev_pack((uint32_t)ji, 0u, k)); else replay = true;
                ++nev; delta += (int)k;
            }
            ++ji;
        } else {
            const uint32_t k = rand_indx_thr(tb.del_t, tb.del_d, (uint32_t)tb.n_del, x);
            if (k > 0) {
                const int kk = (int)k < n - ji ? (int)k : n - ji;
                if constexpr (RAW) put(nev, (uint32_t)ji, 1u, (uint32_t)kk);
                else if (nev < EV_MAX && ji < 1024 && kk < 32) put(nev, ev_pack((uint32_t)ji, 1u, (uint32_t)kk)); else replay = true;
                ++nev; delta -= kk; ji += kk;
            }
            else ++ji;
        }
    }
    if ((force_replay & 1u) && nev > 0) replay = true;
    if (n + delta < 50) { nev = 0; delta = 0; replay = false; }                    // Profile.cpp:1623-1630: drop all indels
    int n_out = n + delta;
    if (n_out > (int)slot) { atomicOr(flags, (uint32_t)FLAG_READSLOT); n_out = 0; nev = 0; replay = false; }
    if (replay) nev = 0;                                                           // phase 2 draws the tests again
    return IndelPass{n_out, nev, replay};
}

}  // namespace scs
