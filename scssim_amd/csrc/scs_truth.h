// scs_truth.h -- the SAM record of a read's true alignment (scs_set_truth_sam).  One formatter for the
// device passes (scs_k_truth.hip: sizing with a counting sink, emit into LDS) and the host probe (scs_truth_record_probe), so the
// test seam runs the code the kernels run.  The BAM record of the same alignment (scs_set_truth_bam) is at the end: the same walks,
// BAM's encoding, and its own probe (scs_truth_bam_record_probe).
//
// A read's alignment comes from its indel events alone (Profile::predict, Profile.cpp:1605-1650): in read orientation the window
// bases cur .. j of an insertion at j are M, then its k inserted bases I; a deletion of k bases at j is j - cur bases M, then k D
// (already clipped to the window end).  Op 2 i is the M run before event i, op 2 i + 1 the event, op 2 nev the M run after the
// last one, so the ops can be walked in either orientation without storing them.  The record is written genome-forward: a read
// whose window runs backwards on the genome (bit 0x10) walks its ops from the last; D runs before the first M or after the last M
// are dropped (POS moves past a leading one), equal neighbours merge, and an I at either end stays.
#pragma once
#include <stdint.h>
#include "scs_common.h"

namespace scs {

#define TRUTH_EVCAP 32                                     // indel events per read the passes hold (more: FLAG_TRUTH, never a wrong record)

// an event: window position | length << 16 | deletion << 31
SCS_HD uint32_t tev_pack(uint32_t pos, uint32_t del, uint32_t len) { return pos | (len << 16) | (del << 31); }
SCS_HD uint32_t tev_pos(uint32_t e) { return e & 0xFFFFu; }
SCS_HD uint32_t tev_len(uint32_t e) { return (e >> 16) & 0x7FFFu; }
SCS_HD uint32_t tev_del(uint32_t e) { return e >> 31; }
SCS_HD uint32_t tev_end(uint32_t e) { return tev_pos(e) + (tev_del(e) ? tev_len(e) : 1u); }   // first window base after the event

// one read: g0 = genome index of window base 0, rev = the window runs backwards (and complemented) on the genome
struct TruthAln {
    int64_t g0; int rev; int n; int nev; const uint32_t* ev;
    int64_t lo, hi;                                        // leftmost / rightmost aligned genome index
    int qlen;                                              // bases of the read (M + I)
};

// op k (read orientation) of 2 nev + 1: kind 'M', 'I' or 'D' and its length (an M run may be empty)
SCS_HD void truth_op(const TruthAln& a, int k, char& kind, uint32_t& len) {
    if (k & 1) { const uint32_t e = a.ev[k >> 1]; kind = tev_del(e) ? 'D' : 'I'; len = tev_len(e); return; }
    const int i = k >> 1;
    const uint32_t cur = i ? tev_end(a.ev[i - 1]) : 0u;
    const uint32_t stop = i < a.nev ? tev_pos(a.ev[i]) + (tev_del(a.ev[i]) ? 0u : 1u) : (uint32_t)a.n;
    kind = 'M'; len = stop - cur;
}

// checks the event list, applies the n + delta < 50 rollback (Profile.cpp:1623-1630; a no-op on the device's lists, which are
// rolled back already) and places the read.  false: not a valid alignment
SCS_HD bool truth_place(TruthAln& a) {
    int delta = 0; uint32_t cur = 0;
    for (int i = 0; i < a.nev; ++i) {
        const uint32_t e = a.ev[i];
        if (tev_pos(e) < cur || tev_len(e) == 0 || tev_end(e) > (uint32_t)a.n || (!tev_del(e) && tev_pos(e) >= (uint32_t)a.n)) return false;
        delta += tev_del(e) ? -(int)tev_len(e) : (int)tev_len(e);
        cur = tev_end(e);
    }
    if (a.n + delta < 50) { a.nev = 0; delta = 0; }
    a.qlen = a.n + delta;
    int first = -1, last = -1;                             // window bases of the first and the last M
    for (int k = 0; k <= 2 * a.nev; k += 2) {
        char kind; uint32_t len; truth_op(a, k, kind, len);
        const uint32_t cur0 = (k >> 1) ? tev_end(a.ev[(k >> 1) - 1]) : 0u;
        if (len) { if (first < 0) first = (int)cur0; last = (int)(cur0 + len - 1); }
    }
    if (first < 0) return false;
    if (a.rev) { a.lo = a.g0 - last; a.hi = a.g0 - first; } else { a.lo = a.g0 + first; a.hi = a.g0 + last; }
    return true;
}

// which staged record holds genome index x: rec_off[r] <= x < rec_off[r + 1] (n_rec + 1 ascending starts, n_rec >= 1).  An x outside
// the genome gives record 0 or n_rec - 1: the caller checks x against the record's bounds before it trusts the answer
SCS_HD uint32_t rec_of(const uint64_t* rec_off, uint32_t n_rec, int64_t x) {
    uint32_t lo = 0, hi = n_rec;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)rec_off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// the CIGAR ops genome-forward, leading / trailing D dropped, neighbours of one kind merged: f(kind, len)
template <class F>
SCS_HD void truth_cigar_walk(const TruthAln& a, F f) {
    char lk = 0; uint32_t ll = 0, pend_d = 0; bool seen_m = false;
    auto push = [&](char k, uint32_t l) { if (k == lk) ll += l; else { if (lk) f(lk, ll); lk = k; ll = l; } };
    const int nops = 2 * a.nev + 1;
    for (int j = 0; j < nops; ++j) {
        char kind; uint32_t len; truth_op(a, a.rev ? nops - 1 - j : j, kind, len);
        if (!len) continue;
        if (kind == 'D') { if (seen_m) pend_d += len; continue; }
        if (pend_d) { push('D', pend_d); pend_d = 0; }
        if (kind == 'M') seen_m = true;
        push(kind, len);
    }
    if (lk) f(lk, ll);
}

SCS_HD char truth_comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

template <class Out>
SCS_HD void truth_num(Out& o, uint64_t v) {
    char d[20]; int n = 0;
    do { d[n++] = (char)('0' + v % 10u); v /= 10u; } while (v);
    while (n) o.put(d[--n]);
}
template <class Out>
SCS_HD void truth_snum(Out& o, int64_t v) { if (v < 0) { o.put('-'); truth_num(o, (uint64_t)(-v)); } else truth_num(o, (uint64_t)v); }

// the rest of a record: who it is and where its mate lies
struct TruthLine {
    uint32_t amp, cnt, flag; int paired;
    const char* rname; uint32_t rname_len; int64_t rec0;   // rec0: genome index of the record's first base
    int64_t mate_lo; int64_t tlen;
};

// src: seq(i) / qual(i) = the FASTQ record's base / quality i (read orientation), gen(g) = genome base g as 'A' 'C' 'G' 'T' 'N'.
// Writes the record with its newline through o.put(char).
template <class Out, class Src>
SCS_HD void truth_record(Out& o, const TruthAln& a, const TruthLine& li, const Src& src) {
    const int q = a.qlen;
    truth_num(o, li.amp); o.put('#'); truth_num(o, li.cnt); o.put('\t');
    truth_num(o, li.flag); o.put('\t');
    for (uint32_t i = 0; i < li.rname_len; ++i) o.put(li.rname[i]);
    o.put('\t'); truth_num(o, (uint64_t)(a.lo - li.rec0 + 1)); o.put('\t');
    o.put('2'); o.put('5'); o.put('5'); o.put('\t');
    truth_cigar_walk(a, [&](char k, uint32_t l) { truth_num(o, l); o.put(k); });
    o.put('\t');
    if (li.paired) { o.put('='); o.put('\t'); truth_num(o, (uint64_t)(li.mate_lo - li.rec0 + 1)); o.put('\t'); truth_snum(o, li.tlen); }
    else { o.put('*'); o.put('\t'); o.put('0'); o.put('\t'); o.put('0'); }
    o.put('\t');
    for (int i = 0; i < q; ++i) o.put(a.rev ? truth_comp(src.seq(q - 1 - i)) : src.seq(i));
    o.put('\t');
    for (int i = 0; i < q; ++i) o.put(src.qual(a.rev ? q - 1 - i : i));
    // NM / MD against the genome: one walk counts, the second prints
    uint32_t nm = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int64_t g = a.lo; int qi = 0; uint32_t run = 0;
        if (pass == 1) { o.put('\t'); o.put('N'); o.put('M'); o.put(':'); o.put('i'); o.put(':'); truth_num(o, nm); o.put('\t'); o.put('M'); o.put('D'); o.put(':'); o.put('Z'); o.put(':'); }
        truth_cigar_walk(a, [&](char k, uint32_t l) {
            if (k == 'I') { qi += (int)l; if (!pass) nm += l; return; }
            if (k == 'D') {
                if (!pass) { nm += l; g += l; return; }
                truth_num(o, run); run = 0; o.put('^');
                for (uint32_t t = 0; t < l; ++t) o.put(src.gen(g++));
                return;
            }
            for (uint32_t t = 0; t < l; ++t, ++qi, ++g) {
                const char r = a.rev ? truth_comp(src.seq(q - 1 - qi)) : src.seq(qi), gc = src.gen(g);
                if (r == gc) { ++run; continue; }
                if (!pass) ++nm; else { truth_num(o, run); o.put(gc); }
                run = 0;
            }
        });
        if (pass == 1) truth_num(o, run);
    }
    o.put('\n');
}

struct TruthCount { uint64_t n = 0; SCS_HD void put(char) { ++n; } };

// ---- the same alignment as one BAM record (scs_set_truth_bam): the SAM's values in BAM's encoding, from the same walks
// a read's MD string through o.put; returns its NM (the SAM record's second walk, counting as it prints)
template <class Out, class Src>
SCS_HD uint32_t truth_md(Out& o, const TruthAln& a, const Src& src) {
    const int q = a.qlen; uint32_t nm = 0, run = 0; int64_t g = a.lo; int qi = 0;
    truth_cigar_walk(a, [&](char k, uint32_t l) {
        if (k == 'I') { qi += (int)l; nm += l; return; }
        if (k == 'D') {
            nm += l; truth_num(o, run); run = 0; o.put('^');
            for (uint32_t t = 0; t < l; ++t) o.put(src.gen(g++));
            return;
        }
        for (uint32_t t = 0; t < l; ++t, ++qi, ++g) {
            const char r = a.rev ? truth_comp(src.seq(q - 1 - qi)) : src.seq(qi), gc = src.gen(g);
            if (r == gc) { ++run; continue; }
            ++nm; truth_num(o, run); o.put(gc); run = 0;
        }
    });
    truth_num(o, run);
    return nm;
}

SCS_HD uint32_t truth_digits(uint32_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; ++d; } return d; }
// bin of the 0-based region [beg, end) (SAM specification, section 5.3)
SCS_HD uint32_t truth_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
SCS_HD uint32_t truth_base4(char c) { return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : 15u; }

// bytes of the record below (block_size included): closed-form but for the CIGAR's op count and the MD string's length
template <class Src>
SCS_HD uint32_t truth_bam_size(const TruthAln& a, const TruthLine& li, const Src& src) {
    uint32_t ncig = 0; truth_cigar_walk(a, [&](char, uint32_t) { ++ncig; });
    TruthCount md; truth_md(md, a, src);
    const uint32_t q = (uint32_t)a.qlen;
    return 36u + truth_digits(li.amp) + 1u + truth_digits(li.cnt) + 1u + 4u * ncig + (q + 1u) / 2u + q + 7u + 3u + (uint32_t)md.n + 1u;
}

template <class Out> SCS_HD void truth_le16(Out& o, uint32_t v) { o.put((uint8_t)v); o.put((uint8_t)(v >> 8)); }
template <class Out> SCS_HD void truth_le32(Out& o, uint32_t v) { truth_le16(o, v); truth_le16(o, v >> 16); }

// The BAM record of a read, block_size first.  o: put(uint8_t), pos() = bytes put so far, poke32(at, v) = four little-endian
// bytes over the ones put at `at` (block_size and NM are known once the tags are written).  ref_id: index of li's record
template <class Out, class Src>
SCS_HD void truth_bam_record(Out& o, const TruthAln& a, const TruthLine& li, const Src& src, int32_t ref_id) {
    const int q = a.qlen; const uint32_t at0 = o.pos();
    uint32_t ncig = 0; truth_cigar_walk(a, [&](char, uint32_t) { ++ncig; });
    const int64_t pos = a.lo - li.rec0;
    truth_le32(o, 0u); truth_le32(o, (uint32_t)ref_id); truth_le32(o, (uint32_t)pos);
    o.put((uint8_t)(truth_digits(li.amp) + 1u + truth_digits(li.cnt) + 1u)); o.put((uint8_t)255);
    truth_le16(o, truth_reg2bin(pos, a.hi - li.rec0 + 1)); truth_le16(o, ncig); truth_le16(o, li.flag); truth_le32(o, (uint32_t)q);
    truth_le32(o, li.paired ? (uint32_t)ref_id : 0xFFFFFFFFu); truth_le32(o, li.paired ? (uint32_t)(li.mate_lo - li.rec0) : 0xFFFFFFFFu);
    truth_le32(o, li.paired ? (uint32_t)(int32_t)li.tlen : 0u);
    truth_num(o, li.amp); o.put('#'); truth_num(o, li.cnt); o.put((uint8_t)0);
    truth_cigar_walk(a, [&](char k, uint32_t l) { truth_le32(o, (l << 4) | (k == 'M' ? 0u : k == 'I' ? 1u : 2u)); });
    for (int i = 0; i < q; i += 2) {
        const uint32_t hi4 = truth_base4(a.rev ? truth_comp(src.seq(q - 1 - i)) : src.seq(i));
        const uint32_t lo4 = i + 1 < q ? truth_base4(a.rev ? truth_comp(src.seq(q - 2 - i)) : src.seq(i + 1)) : 0u;
        o.put((uint8_t)((hi4 << 4) | lo4));
    }
    for (int i = 0; i < q; ++i) o.put((uint8_t)(src.qual(a.rev ? q - 1 - i : i) - 33));
    o.put('N'); o.put('M'); o.put('i'); const uint32_t at_nm = o.pos(); truth_le32(o, 0u);
    o.put('M'); o.put('D'); o.put('Z'); const uint32_t nm = truth_md(o, a, src); o.put((uint8_t)0);
    o.poke32(at_nm, nm); o.poke32(at0, o.pos() - at0 - 4u);
}

}  // namespace scs
