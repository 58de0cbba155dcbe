// scs_place.h -- where a read of a batch lies on the genome: its indel events (the indel pass' packed ones, or drawn again for a
// replayed read) and its placement (truth_place, scs_truth.h).  The one definition behind the truth passes (scs_k_truth.hip),
// which go on to the read's FASTQ text (read_text), the site support pass (scs_k_support.hip), which reads its bases there, and the
// depth passes (scs_k_depth.hip, scs_k_lift.hip), which need neither.  The three side passes walk a pair's reads through one loop
// (for_each_placed_read); the truth passes place a pair's two mates together and keep their own.
// Needs scs_device.h and scs_kernels_common.h before it.
#pragma once
#include "scs_indel.h"
#include "scs_truth.h"

namespace scs {

// read rd of pair pi: its events into ev (TRUTH_EVCAP entries), its placement into a, its length into n_out.  false: it has no
// record (a read the indel pass flagged), or it cannot be placed right (`flag` is raised: FLAG_TRUTH / FLAG_DEPTH)
__device__ __forceinline__ bool read_place(const PlaceArgs& A, const PairRec& pr, uint32_t pi, uint32_t rd, uint32_t* ev, TruthAln& a, int& n_out, uint32_t flag) {
    const uint32_t r = A.paired ? 2u * pi + rd : pi, hdr = A.ev_hdr[r];
    n_out = (int)(hdr & 0xFFFFu);
    if (n_out == 0) return false;
    int nev = (int)((hdr >> 16) & 0xFFu);
    if ((hdr >> 24) & 1u) {                                // replayed read: its events again, drawn by the indel pass' own code
        bool over = false;
        const IndelPass ip = indel_pass<true>(A.tb, A.key, rd | (pr.att << 1), pr.uid, 0u, A.slot, A.flags, [&](int i, uint32_t pos, uint32_t del, uint32_t len) {
            if (i < TRUTH_EVCAP) ev[i] = tev_pack(pos, del, len); else over = true;
        });
        if (over && ip.nev > 0) { atomicOr(A.flags, flag); return false; }
        nev = ip.nev;
    } else if (nev > 0) {
        const uint4 d = A.ev_dat[r]; const uint32_t w[4] = {d.x, d.y, d.z, d.w};
        for (int i = 0; i < nev; ++i) { const uint32_t v = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; ev[i] = tev_pack(ev_pos(v), ev_del(v), ev_len(v)); }
    }
    // a full amplicon is a forward copy (direction +1, no complement) or a reverse complement (-1, complement) of the genome
    const uint32_t comp = pr.flags & 1u, back = (pr.flags >> 1) & 1u;
    if (comp != back) { atomicOr(A.flags, flag); return false; }
    const int64_t dir = back ? -1 : 1;
    a.g0 = rd == 0 ? pr.base + dir * (int64_t)pr.pos : pr.base + dir * (int64_t)(pr.pos + pr.isz - 1);   // read 2 = revcomp of the far end
    a.rev = rd == 0 ? (int)back : (int)(back ^ 1u);
    a.n = A.tb.L; a.nev = nev; a.ev = ev;
    if (!truth_place(a) || a.qlen != n_out) { atomicOr(A.flags, flag); return false; }
    return true;
}

// every placed read of pair pi (A: PlaceArgs with the staged record starts rec_off[n_rec + 1]): f(pr, rd, a, n, lo, r0, r1) with the
// pair's record, the read's number, placement and length, and the staged record of its leftmost aligned base: lo, its first base r0
// = rec_off[lo] <= a.lo and its end r1 = rec_off[lo + 1].  A hole and a read that read_place gives up on (it raises `flag`) are
// passed over.  Whether the read ends inside [r0, r1) is not checked here: k_depth and k_support check before they use the record,
// lift_read reports it itself
template <class Args, class F>
__device__ __forceinline__ void for_each_placed_read(const Args& A, uint32_t pi, uint32_t flag, F f) {
    const PairRec pr = A.pairs[pi];
    if (pr.isz == 0) return;                               // hole: no FASTQ record
    uint32_t ev[TRUTH_EVCAP];
    for (uint32_t rd = 0; rd < (A.paired ? 2u : 1u); ++rd) {
        TruthAln a; int n_out;
        if (!read_place(A, pr, pi, rd, ev, a, n_out, flag)) continue;
        const uint32_t lo = rec_of(A.rec_off, A.n_rec, a.lo);
        f(pr, rd, a, n_out, lo, (int64_t)A.rec_off[lo], (int64_t)A.rec_off[lo + 1]);
    }
}

// where the bases of read rd of pair pi lie in the batch's FASTQ text: behind the record's name line "@amp#cnt[/r]\n" (off1 / off2:
// the mates' record offsets, OFF_MASK; fq1 / fq2: their text).  *rec receives the record's first byte, its '@'
__device__ __forceinline__ const char* read_text(const uint64_t* off1, const uint64_t* off2, const char* fq1, const char* fq2, int paired, const PairRec& pr, uint32_t pi, uint32_t rd,
                                                 const char** rec = nullptr) {
    const char* r = (rd ? fq2 : fq1) + ((rd ? off2 : off1)[pi] & OFF_MASK);
    if (rec) *rec = r;
    return r + 1u + truth_digits(pr.amp) + 1u + truth_digits(pr.att + 1u) + (paired ? 2u : 0u) + 1u;
}

// read rd of pair pi for a truth pass: its events into ev and its placement (read_place), then its FASTQ text: s its bases, q its
// qualities.  false: it has no record (a read the indel pass flagged), or it cannot be made right (FLAG_TRUTH)
__device__ inline bool truth_load(const TruthArgs& A, const PairRec& pr, uint32_t pi, uint32_t rd, uint32_t* ev, TruthAln& a, const char*& s, const char*& q) {
    int n_out;
    if (!read_place(A, pr, pi, rd, ev, a, n_out, (uint32_t)FLAG_TRUTH)) return false;
    s = read_text(A.off1, A.off2, A.fq1, A.fq2, A.paired, pr, pi, rd);
    q = s + n_out + 3;
    return true;
}

}  // namespace scs
