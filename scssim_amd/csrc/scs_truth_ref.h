// scs_truth_ref.h -- the SAM record of a read's true alignment ON THE ORIGINAL REFERENCE (scs_set_truth_ref_sam; DESIGN.md section
// 17): the haplotype alignment of scs_truth.h lifted through the lift table (scs_lift.h).  One definition for the device passes
// (scs_k_truth_ref.hip: sizing with a counting sink, emit into LDS) and the host probe (scs_truth_ref_record_probe).
//
// The haplotype CIGAR is walked genome-forward (truth_cigar_walk) with a haplotype cursor that starts at a.lo, runs through the
// segment table and is cut at segment ends (lift_pieces).  M in an R segment stays M, at ref_pos + (g - hap_off); M in an I
// segment and a sequencing insertion are I; D in an R segment stays D, D in an I segment is nothing.  Where the walk goes from R
// segment s to the next R segment t it touches (I segments between them skipped), the two are collinear iff t.ref_rec == s.ref_rec
// and t.ref_pos >= s.ref_pos + s.len: then a D of the reference bases between them stands in front of t's first piece (the planted
// deletion, a CN-0 stretch).  Any other junction (the backwards jump between tandem copies, another reference record) is a cut;
// cuts split the read into blocks.  The record shows the PRIMARY block, the one with the most M bases (the first on a tie): the read
// indices [q0, q1) from its first to its last M base keep their ops, merged by kind; everything outside is soft-clipped, D at the
// block's edges is dropped.  A read with no lifted M base is unmapped.
// There is no NM / MD: against the reference they need the reference's bases under the planted SNPs and deletions, which genreads
// never stages.  YH:Z / YP:i (haplotype record and POS) join the record to the haplotype SAM, YB:i counts the blocks.
#pragma once
#include "scs_lift.h"

namespace scs {

struct LiftTab { const LiftSeg* segs; uint32_t n_seg; const uint64_t* ref_len; uint32_t n_ref; };

// The genome-forward ops of a placed read cut at segment ends: f(k, len, sg, si, g) -- k 'M' / 'D': len haplotype bases from global
// index g, all inside segment sg = segs[si]; k 'I': a sequencing insertion of len read bases (sg, si, g: where the cursor stands).
// [rec0, rec1): the read's staged record.  One bisection for a.lo, then a cursor that only moves forward; no loop over bases.
// Returns why it gave up, as lift_read does: placed outside its record, off the table or its record's segments, a segment that
// lifts outside its reference record
template <class F>
SCS_HD int lift_pieces(const TruthAln& a, int64_t rec0, int64_t rec1, const LiftTab& T, F f) {
    if (T.n_seg == 0 || a.lo < rec0 || a.hi >= rec1 || a.lo > a.hi) return LIFT_EPLACE;
    uint64_t g = (uint64_t)a.lo;
    uint32_t si = lift_find(T.segs, T.n_seg, g);
    LiftSeg sg = T.segs[si];
    bool checked = false; int err = LIFT_OK;
    truth_cigar_walk(a, [&](char k, uint32_t l) {
        if (err) return;
        if (k == 'I') { f('I', l, sg, si, g); return; }
        while (l) {
            while (g >= sg.hap_off + sg.len) { if (++si >= T.n_seg) { err = LIFT_ETABLE; return; } sg = T.segs[si]; checked = false; }
            if (!checked) {
                if (g < sg.hap_off || sg.hap_off < (uint64_t)rec0 || sg.hap_off + sg.len > (uint64_t)rec1) { err = LIFT_ETABLE; return; }
                if (sg.kind == 0u && (sg.ref_rec >= T.n_ref || sg.ref_pos + sg.len > T.ref_len[sg.ref_rec])) { err = LIFT_EREF; return; }
                checked = true;
            }
            const uint64_t room = sg.hap_off + sg.len - g;
            const uint32_t take = (uint64_t)l < room ? l : (uint32_t)room;
            f(k, take, sg, si, g);
            g += take; l -= take;
        }
    });
    return err;
}

// a read on the reference: its primary block.  mapped 0: no lifted M base (rec, pos, end, q0, q1 are 0 then, blocks too)
struct LiftAln {
    uint32_t mapped, rec, blocks;                          // rec: the reference record; blocks: 1 + the cuts the read crosses
    uint64_t pos, end;                                     // 0-based reference coordinate of the block's first M base; one past its last
    uint32_t q0, q1, m;                                    // read indices (SEQ order) of the block's first M base and one past its last; its M bases
};

#define LIFT_NO_SEG 0xFFFFFFFFu

// the first walk: the running block's M bases against the best block so far; no per-read arrays
SCS_HD int lift_align(const TruthAln& a, int64_t rec0, int64_t rec1, const LiftTab& T, LiftAln& out) {
    LiftAln best{0u, 0u, 0u, 0, 0, 0u, 0u, 0u}, cur = best;
    uint32_t qi = 0, prev_si = LIFT_NO_SEG, prev_rec = 0, blocks = 0; uint64_t prev_end = 0;
    const int err = lift_pieces(a, rec0, rec1, T, [&](char k, uint32_t l, const LiftSeg& sg, uint32_t si, uint64_t g) {
        if (k == 'I') { qi += l; return; }
        if (sg.kind != 0u) { if (k == 'M') qi += l; return; }
        if (si != prev_si) {
            const bool cut = prev_si != LIFT_NO_SEG && !(sg.ref_rec == prev_rec && sg.ref_pos >= prev_end);
            if (prev_si == LIFT_NO_SEG) blocks = 1;
            else if (cut) { if (cur.m > best.m) best = cur; cur.m = 0u; ++blocks; }
            prev_si = si; prev_rec = sg.ref_rec; prev_end = sg.ref_pos + sg.len;
        }
        if (k != 'M') return;
        const uint64_t r = sg.ref_pos + (g - sg.hap_off);
        if (cur.m == 0u) { cur.q0 = qi; cur.rec = sg.ref_rec; cur.pos = r; }
        cur.m += l; qi += l; cur.q1 = qi; cur.end = r + l;
    });
    if (err) return err;
    if (cur.m > best.m) best = cur;
    out = best;
    if (best.m) { out.mapped = 1u; out.blocks = blocks; }
    return LIFT_OK;
}

// the second walk: the primary block's ops between its first and its last M base, merged by kind: f(kind, len).  A D stands
// between two read bases: it is shown iff q0 < (read bases before it) < q1 -- so the D runs at the block's edges go
template <class F>
SCS_HD int lift_align_ops(const TruthAln& a, int64_t rec0, int64_t rec1, const LiftTab& T, const LiftAln& L, F f) {
    char lk = 0; uint32_t qi = 0, prev_si = LIFT_NO_SEG, prev_rec = 0; uint64_t ll = 0, prev_end = 0;
    auto push = [&](char k, uint64_t l) { if (k == lk) ll += l; else { if (lk) f(lk, ll); lk = k; ll = l; } };
    const int err = lift_pieces(a, rec0, rec1, T, [&](char k, uint32_t l, const LiftSeg& sg, uint32_t si, uint64_t) {
        const bool in = qi >= L.q0 && qi < L.q1, between = qi > L.q0 && qi < L.q1;
        if (k == 'I' || (sg.kind != 0u && k == 'M')) { if (in) push('I', l); qi += l; return; }
        if (sg.kind != 0u) return;
        if (si != prev_si) {
            if (prev_si != LIFT_NO_SEG && between && sg.ref_rec == prev_rec && sg.ref_pos > prev_end) push('D', sg.ref_pos - prev_end);
            prev_si = si; prev_rec = sg.ref_rec; prev_end = sg.ref_pos + sg.len;
        }
        if (k == 'M') { if (in) push('M', l); qi += l; }
        else if (between) push('D', l);
    });
    if (!err && lk) f(lk, ll);
    return err;
}

// the rest of a record: who it is, its haplotype record (YH / YP) and the reference's names
struct TruthRefLine {
    uint32_t amp, cnt; int paired, read2, mate_rev;
    const char* hname; uint32_t hname_len; int64_t rec0, rec1;   // the staged record: its name, its global indices
    const uint32_t* ref_name_off; const char* ref_names;   // reference record r: ref_names[ref_name_off[r] .. ref_name_off[r + 1])
};

// src: seq(i) / qual(i) = the FASTQ record's base / quality i (read orientation).  L: the read's primary block, M: its mate's (PE).
// Writes the record with its newline through o.put(char); returns lift_align_ops' error (the record is then not to be used)
template <class Out, class Src>
SCS_HD int truth_ref_record(Out& o, const TruthAln& a, const TruthRefLine& li, const LiftTab& T, const LiftAln& L, const LiftAln& M, const Src& src) {
    const int q = a.qlen;
    const bool mate_mapped = li.paired && M.mapped, same = L.mapped && mate_mapped && L.rec == M.rec;
    auto name = [&](uint32_t r) { for (uint32_t i = li.ref_name_off[r]; i < li.ref_name_off[r + 1]; ++i) o.put(li.ref_names[i]); };
    uint32_t flag = a.rev ? 0x10u : 0u;
    if (li.paired) flag |= 0x1u | (li.read2 ? 0x80u : 0x40u) | (li.mate_rev ? 0x20u : 0u) | (M.mapped ? 0u : 0x8u) | (same ? 0x2u : 0u);
    if (!L.mapped) flag |= 0x4u;
    // where the record stands: its own block, else its mate's
    const bool placed = L.mapped || mate_mapped; const uint32_t rec = L.mapped ? L.rec : M.rec; const uint64_t pos = L.mapped ? L.pos : M.pos;
    truth_num(o, li.amp); o.put('#'); truth_num(o, li.cnt); o.put('\t');
    truth_num(o, flag); o.put('\t');
    if (placed) { name(rec); o.put('\t'); truth_num(o, pos + 1u); } else { o.put('*'); o.put('\t'); o.put('0'); }
    o.put('\t');
    if (L.mapped) { o.put('2'); o.put('5'); o.put('5'); } else o.put('0');
    o.put('\t');
    int err = LIFT_OK;
    if (L.mapped) {
        if (L.q0) { truth_num(o, L.q0); o.put('S'); }
        err = lift_align_ops(a, li.rec0, li.rec1, T, L, [&](char k, uint64_t l) { truth_num(o, l); o.put(k); });
        if ((uint32_t)q > L.q1) { truth_num(o, (uint32_t)q - L.q1); o.put('S'); }
    } else o.put('*');
    o.put('\t');
    if (li.paired && placed) {
        const uint32_t mrec = mate_mapped ? M.rec : L.rec; const uint64_t mpos = mate_mapped ? M.pos : L.pos;
        int64_t tlen = 0;
        if (same) {
            const uint64_t left = L.pos < M.pos ? L.pos : M.pos, right = L.end > M.end ? L.end : M.end;
            const bool first = L.pos < M.pos || (L.pos == M.pos && !li.read2);
            tlen = first ? (int64_t)(right - left) : -(int64_t)(right - left);
        }
        if (mrec == rec) o.put('='); else name(mrec);
        o.put('\t'); truth_num(o, mpos + 1u); o.put('\t'); truth_snum(o, tlen);
    } else { o.put('*'); o.put('\t'); o.put('0'); o.put('\t'); o.put('0'); }
    o.put('\t');
    for (int i = 0; i < q; ++i) o.put(a.rev ? truth_comp(src.seq(q - 1 - i)) : src.seq(i));
    o.put('\t');
    for (int i = 0; i < q; ++i) o.put(src.qual(a.rev ? q - 1 - i : i));
    o.put('\t'); o.put('Y'); o.put('H'); o.put(':'); o.put('Z'); o.put(':');
    for (uint32_t i = 0; i < li.hname_len; ++i) o.put(li.hname[i]);
    o.put('\t'); o.put('Y'); o.put('P'); o.put(':'); o.put('i'); o.put(':'); truth_num(o, (uint64_t)(a.lo - li.rec0 + 1));
    o.put('\t'); o.put('Y'); o.put('B'); o.put(':'); o.put('i'); o.put(':'); truth_num(o, L.blocks);
    o.put('\n');
    return err;
}

}  // namespace scs
