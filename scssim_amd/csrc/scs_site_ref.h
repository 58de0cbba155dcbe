// scs_site_ref.h -- the artefact table on the ORIGINAL REFERENCE (scs_write_artefacts_ref / scs_artefact_ref_sites; DESIGN.md section
// 18): the edits of the full amplicons (amp_edits, scs_amp.h) lifted through the lift table (scs_lift.h) and grouped by reference
// site.  X = ref_off[ref_rec] + ref_pos indexes the reference records of the table, concatenated in table order.  A site is
// (X, the template's base, alternate base); per site NA / NR count the edit entries that lift to it and their amplicons' reads,
// TA / TR the PIECES that contain X and theirs -- a piece being the part of an amplicon's interval that lies in one R segment, as
// a reference interval.  An entry in inserted sequence has no reference coordinate: it is counted, and makes no line.  One
// definition for the device passes (scs_k_sites_ref.hip: the walk, the sort keys, the cover count) and the host probe
// (scs_artefact_ref_probe), so the test seam runs the code the kernels run -- with std::sort where the device has the radix sort.
#pragma once
#include <stdint.h>
#include "scs_common.h"
#include "scs_site.h"
#include "scs_lift.h"

namespace scs {

// the sort key of a lifted entry: ascending keys are ascending (X, REF A < C < G < T < N, ALT A < C < G < T)
#define SITE_REF_KEY_BITS 5u
SCS_HD uint64_t site_ref_key(uint64_t x, uint32_t ref, uint32_t alt) { return (x << 5) | ((uint64_t)(ref < 4u ? ref : 4u) << 2) | (uint64_t)(alt & 3u); }
SCS_HD uint64_t site_ref_key_x(uint64_t key) { return key >> 5; }
SCS_HD uint32_t site_ref_key_ref(uint64_t key) { return (uint32_t)(key >> 2) & 7u; }
SCS_HD uint32_t site_ref_key_alt(uint64_t key) { return (uint32_t)(key & 3u); }

// the table as the walk sees it: the segments, and where every reference record starts among the reference's bases (n_ref + 1)
struct SiteRefView { const LiftSeg* segs; uint32_t n_seg; const uint64_t* ref_off; uint32_t n_ref; };

// A cursor over the segments under one amplicon [lo, hi): it only moves forward.  Whenever it ENTERS a segment it checks it -- the
// segment follows the last one without a gap, stays inside the amplicon's staged record [.., rec1) and, if R, inside its reference
// record (as lift_read checks a segment on entry) -- and reports the R segment's piece.  err: a LiftErr
struct SiteRefCursor { uint64_t lo, hi, rec1; uint32_t si; LiftSeg sg; int err; };

template <class Piece>
SCS_HD void site_ref_enter(const SiteRefView& V, SiteRefCursor& c, Piece piece) {
    const LiftSeg& s = c.sg;
    if (s.len == 0 || s.hap_off + s.len < s.hap_off || s.hap_off + s.len > c.rec1) { c.err = LIFT_ETABLE; return; }
    if (s.kind != 0u) return;
    if (s.ref_rec >= V.n_ref || s.ref_pos + s.len < s.ref_pos || s.ref_pos + s.len > V.ref_off[s.ref_rec + 1] - V.ref_off[s.ref_rec]) { c.err = LIFT_EREF; return; }
    const uint64_t g0 = c.lo > s.hap_off ? c.lo : s.hap_off, g1 = c.hi < s.hap_off + s.len ? c.hi : s.hap_off + s.len;
    const uint64_t x0 = V.ref_off[s.ref_rec] + s.ref_pos + (g0 - s.hap_off);
    piece(x0, x0 + (g1 - g0));
}
// the cursor on the segment of lo: one bisection.  [rec0, rec1): the amplicon's staged record
template <class Piece>
SCS_HD void site_ref_begin(const SiteRefView& V, uint64_t lo, uint64_t len, uint64_t rec0, uint64_t rec1, SiteRefCursor& c, Piece piece) {
    c.lo = lo; c.hi = lo + len; c.rec1 = rec1; c.si = 0; c.err = LIFT_OK;
    if (V.n_seg == 0 || len == 0 || lo < rec0 || lo + len > rec1 || lo + len < lo) { c.err = LIFT_EPLACE; return; }
    c.si = lift_find(V.segs, V.n_seg, lo); c.sg = V.segs[c.si];
    if (lo < c.sg.hap_off || lo >= c.sg.hap_off + c.sg.len || c.sg.hap_off < rec0) { c.err = LIFT_ETABLE; return; }
    site_ref_enter(V, c, piece);
}
// forward to the segment of g (lo <= g < hi, not before the last g)
template <class Piece>
SCS_HD void site_ref_seek(const SiteRefView& V, SiteRefCursor& c, uint64_t g, Piece piece) {
    while (!c.err && g >= c.sg.hap_off + c.sg.len) {
        const uint64_t end = c.sg.hap_off + c.sg.len;
        if (++c.si >= V.n_seg) { c.err = LIFT_ETABLE; return; }
        c.sg = V.segs[c.si];
        if (c.sg.hap_off != end) { c.err = LIFT_ETABLE; return; }
        site_ref_enter(V, c, piece);
    }
    if (!c.err && g < c.sg.hap_off) c.err = LIFT_ETABLE;
}

// One amplicon through the table.  edits(f) delivers its edits f(g, ref, alt) in ascending staged order, each index once (amp_edits);
// piece(x0, x1) per R segment it touches, in staged order; entry(x, ref, alt) per edit in an R segment, unlifted() per edit in an
// I segment.  Returns a LiftErr.  The callbacks made before an error have been made: the caller drops what they gave (the host
// probe adds an amplicon's counts only after its walk has succeeded) or fails the whole call (the kernels)
template <class Edits, class Piece, class Entry, class Unlifted>
SCS_HD int site_ref_amp(const SiteRefView& V, uint64_t lo, uint64_t len, uint64_t rec0, uint64_t rec1, Edits edits, Piece piece, Entry entry, Unlifted unlifted) {
    SiteRefCursor c;
    site_ref_begin(V, lo, len, rec0, rec1, c, piece);
    if (c.err) return c.err;
    uint64_t prev = lo; bool any = false;
    edits([&](int64_t gx, uint32_t ref, uint32_t alt) {
        if (c.err) return;
        const uint64_t g = (uint64_t)gx;
        if (gx < 0 || g < c.lo || g >= c.hi || (any && g <= prev)) { c.err = LIFT_EPLACE; return; }
        prev = g; any = true;
        site_ref_seek(V, c, g, piece);
        if (c.err) return;
        if (c.sg.kind == 0u) entry(V.ref_off[c.sg.ref_rec] + c.sg.ref_pos + (g - c.sg.hap_off), ref, alt); else unlifted();
    });
    if (!c.err) site_ref_seek(V, c, c.hi - 1u, piece);
    return c.err;
}

// site_make (scs_site.h) over lifted entries and pieces: the run that opens at entry i of the sorted (key, reads) pairs; starts /
// ends: the ascending starts and (exclusive) ends of the pieces, ps_*: the prefix sums of their reads.  REF and ALT come from the
// key, the reference record from ref_off.  false: X outside the reference, or counts that contradict each other
SCS_HD bool site_ref_make(const uint64_t* keys, const uint32_t* reads, uint64_t n, uint64_t i, const uint64_t* starts, const uint64_t* ps_start,
                          const uint64_t* ends, const uint64_t* ps_end, uint64_t m, const uint64_t* ref_off, uint32_t n_ref, SiteRec& r) {
    const uint64_t key = keys[i], x = site_ref_key_x(key);
    if (n_ref == 0 || x >= ref_off[n_ref]) return false;
    uint32_t na = 0; uint64_t nr = 0;
    for (uint64_t j = i; j < n && keys[j] == key; ++j) { ++na; nr += reads[j]; }
    const uint64_t rs = site_rank_le(starts, m, x), re = site_rank_le(ends, m, x);
    r.rec = rec_of(ref_off, n_ref, x); r.pos = x - ref_off[r.rec]; r.ref = (uint8_t)site_ref_key_ref(key); r.alt = (uint8_t)site_ref_key_alt(key); r.pad[0] = r.pad[1] = 0;
    r.na = na; r.nr = nr; r.ta = (uint32_t)(rs - re); r.tr = ps_start[rs] - ps_end[re];
    return rs >= re && rs - re >= na && rs - re <= 0xFFFFFFFFull && ps_start[rs] >= ps_end[re] && r.tr >= nr && r.ref <= 4u;
}

// ---- host-only
#define SITE_REF_NOTE "the base of the haplotype the amplicon copied (the template the polymerase misread); it differs from the reference FASTA where a substitution was planted"
// the file's header: the unlifted totals, one contig line per REFERENCE record of the lift table, in its order (support: the site
// support table's on the reference, three more INFO lines)
inline std::string site_ref_header(const std::vector<std::string>& ref_names, const uint64_t* ref_len, uint64_t unl_entries, uint64_t unl_reads, bool support = false) {
    std::string h = "##fileformat=VCFv4.2\n##source=scssim\n##scssim_coordinates=reference\n##scssim_REF=<" SITE_REF_NOTE ">\n";
    h += "##scssim_unlifted=<entries=" + std::to_string(unl_entries) + ",reads=" + std::to_string(unl_reads) + ">\n";
    for (size_t r = 0; r < ref_names.size(); ++r) h += "##contig=<ID=" + ref_names[r] + ",length=" + std::to_string(ref_len[r]) + ">\n";
    h += "##INFO=<ID=NA,Number=1,Type=Integer,Description=\"edit entries (full amplicon, haplotype position) that carry the alternate base and lift to the site\">\n"
         "##INFO=<ID=TA,Number=1,Type=Integer,Description=\"pieces of full amplicons, of any haplotype and copy, that cover the site\">\n"
         "##INFO=<ID=NR,Number=1,Type=Integer,Description=\"reads allotted to the amplicons of the NA entries\">\n"
         "##INFO=<ID=TR,Number=1,Type=Integer,Description=\"reads allotted to the amplicons of the TA pieces\">\n";
    if (support) h += SITE_SUPPORT_INFO;                   // (scs_write_site_support_ref)
    h += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    return h;
}

// The table's body from amplicon intervals (global staged start, length, reads), edit entries (amplicon, global staged index,
// alternate base) in any order, the staged records and bases, and the lift table -- slab by slab as the device works it: a counting
// walk over all amplicons, then per slab of `slab` reference indices a fill walk, three sorts, the prefix sums and the reduce
// (scs_artefact_ref_probe; no GPU, no ctx).  SCS_EINVAL: an amplicon off its record, an edit outside its amplicon or twice at one
// index, a base that is no code 0..3, records that do not add up to the genome, a walk that leaves the table (it does not tile), a
// segment past its reference record, a reference of 2^58 bases; SCS_EDEVICE: the two walks or the two sinks disagree, or
// site_ref_make refuses.  *lift_err (may be NULL): why a walk gave up.  unlifted[2]: entries and reads without a reference coordinate
inline int site_ref_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                          const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                          const uint64_t* hap_len, uint32_t n_hap, const char* genome, uint64_t genome_len,
                          const LiftSeg* segs, uint32_t n_seg, const uint64_t* ref_len, const std::vector<std::string>& ref_names,
                          uint32_t min_reads, uint64_t slab, std::string& body, uint64_t unlifted[2], int* lift_err,
                          std::vector<SiteRec>* sites = nullptr) {
    const uint32_t n_ref = (uint32_t)ref_names.size();
    if (lift_err) *lift_err = 0;
    unlifted[0] = unlifted[1] = 0; body.clear();
    if (!n_hap || !hap_len || !genome || !n_ref || !ref_len || !n_seg || !segs || !slab || (n_amp && (!amp_start || !amp_len || !amp_reads)) || (n_ed && (!ed_amp || !ed_x || !ed_alt))) return SCS_EINVAL;
    std::vector<uint64_t> rec_off(n_hap + 1, 0), ref_off(n_ref + 1, 0);
    for (uint32_t r = 0; r < n_hap; ++r) rec_off[r + 1] = rec_off[r] + hap_len[r];
    for (uint32_t r = 0; r < n_ref; ++r) { if (ref_len[r] >> 58) return SCS_EINVAL; ref_off[r + 1] = ref_off[r] + ref_len[r]; if (ref_off[r + 1] >> 58) return SCS_EINVAL; }
    if (rec_off[n_hap] != genome_len || genome_len >> 60 || ref_off[n_ref] == 0) return SCS_EINVAL;
    const uint64_t ref_bases = ref_off[n_ref], n_slabs = (ref_bases + slab - 1) / slab;
    if (n_slabs > (1u << 24)) return SCS_EINVAL;
    // the edits of every amplicon, ascending
    std::vector<uint64_t> order(n_ed), first(n_amp + 1, 0);
    for (uint64_t e = 0; e < n_ed; ++e) {
        const uint32_t a = ed_amp[e];
        if (a >= n_amp || ed_alt[e] > 3u || ed_x[e] < amp_start[a] || ed_x[e] >= amp_start[a] + amp_len[a]) return SCS_EINVAL;
        order[e] = e; ++first[a + 1];
    }
    for (uint64_t a = 0; a < n_amp; ++a) first[a + 1] += first[a];
    std::sort(order.begin(), order.end(), [&](uint64_t p, uint64_t q) { return ed_amp[p] != ed_amp[q] ? ed_amp[p] < ed_amp[q] : ed_x[p] < ed_x[q]; });
    for (uint64_t e = 1; e < n_ed; ++e) if (ed_amp[order[e]] == ed_amp[order[e - 1]] && ed_x[order[e]] == ed_x[order[e - 1]]) return SCS_EINVAL;
    std::vector<uint64_t> a_rec0(n_amp), a_rec1(n_amp);
    for (uint64_t a = 0; a < n_amp; ++a) {
        if (!amp_len[a] || amp_start[a] >= genome_len || amp_start[a] + amp_len[a] > genome_len) return SCS_EINVAL;
        const uint32_t r = rec_of(rec_off.data(), n_hap, amp_start[a]);
        if (amp_start[a] + amp_len[a] > rec_off[r + 1]) return SCS_EINVAL;         // a fragment never straddles records
        a_rec0[a] = rec_off[r]; a_rec1[a] = rec_off[r + 1];
    }
    auto code = [&](uint64_t g) -> uint32_t { const char ch = genome[g]; return ch == 'A' || ch == 'a' ? 0u : ch == 'C' || ch == 'c' ? 1u : ch == 'G' || ch == 'g' ? 2u : ch == 'T' || ch == 't' ? 3u : 4u; };
    const SiteRefView V{segs, n_seg, ref_off.data(), n_ref};
    // walk(a, piece, entry, unl): amplicon a through site_ref_amp
    auto walk = [&](uint64_t a, auto piece, auto entry, auto unl) {
        return site_ref_amp(V, amp_start[a], amp_len[a], a_rec0[a], a_rec1[a],
                            [&](auto f) { for (uint64_t k = first[a]; k < first[a + 1]; ++k) { const uint64_t e = order[k]; f((int64_t)ed_x[e], code(ed_x[e]), (uint32_t)ed_alt[e]); } },
                            piece, entry, unl);
    };
    // the counting pass
    std::vector<uint64_t> cnt(2 * n_slabs, 0);
    for (uint64_t a = 0; a < n_amp; ++a) {
        uint64_t ue = 0; std::vector<uint64_t> add;              // (an amplicon that fails counts for nothing)
        const int err = walk(a, [&](uint64_t x0, uint64_t x1) { for (uint64_t s = x0 / slab; s <= (x1 - 1) / slab; ++s) add.push_back(2 * s + 1); },
                             [&](uint64_t x, uint32_t, uint32_t) { add.push_back(2 * (x / slab)); }, [&] { ++ue; });
        if (err) { if (lift_err) *lift_err = err; return SCS_EINVAL; }
        for (uint64_t k : add) { if (k >= cnt.size()) return SCS_EDEVICE; ++cnt[k]; }
        unlifted[0] += ue; unlifted[1] += ue * amp_reads[a];
    }
    struct StrOut { std::string* t; void put(char ch) { t->push_back(ch); } } o{&body};
    uint64_t counted = 0;
    typedef std::pair<uint64_t, uint32_t> KV;
    auto by_key = [](const KV& p, const KV& q) { return p.first < q.first; };
    for (uint64_t k = 0; k < n_slabs; ++k) {
        if (!cnt[2 * k]) continue;                               // a slab without an entry has no site
        const uint64_t s0 = k * slab, s1 = std::min(ref_bases, s0 + slab);
        std::vector<KV> ent, st, en;
        for (uint64_t a = 0; a < n_amp; ++a)
            (void)walk(a, [&](uint64_t x0, uint64_t x1) { if (x0 < s1 && x1 > s0) { st.push_back({x0, amp_reads[a]}); en.push_back({x1, amp_reads[a]}); } },
                       [&](uint64_t x, uint32_t ref, uint32_t alt) { if (x >= s0 && x < s1) ent.push_back({site_ref_key(x, ref, alt), amp_reads[a]}); }, [] {});
        if (ent.size() != cnt[2 * k] || st.size() != cnt[2 * k + 1]) return SCS_EDEVICE;   // (the fill pass found what the counting pass counted)
        std::sort(ent.begin(), ent.end(), by_key); std::sort(st.begin(), st.end(), by_key); std::sort(en.begin(), en.end(), by_key);
        const uint64_t e = ent.size(), m = st.size();
        std::vector<uint64_t> keys(e + 1, 0), starts(m + 1, 0), ends(m + 1, 0), ps_start(m + 1, 0), ps_end(m + 1, 0); std::vector<uint32_t> reads(e + 1, 0);
        for (uint64_t i = 0; i < e; ++i) { keys[i] = ent[i].first; reads[i] = ent[i].second; }
        for (uint64_t i = 0; i < m; ++i) { starts[i] = st[i].first; ends[i] = en[i].first; ps_start[i + 1] = ps_start[i] + st[i].second; ps_end[i + 1] = ps_end[i] + en[i].second; }
        for (uint64_t i = 0; i < e; ++i) {
            if (!site_head(keys.data(), i)) continue;
            SiteRec r;
            if (!site_ref_make(keys.data(), reads.data(), e, i, starts.data(), ps_start.data(), ends.data(), ps_end.data(), m, ref_off.data(), n_ref, r)) return SCS_EDEVICE;
            if (r.nr < min_reads) continue;
            TruthCount c; site_line(c, ref_names[r.rec].data(), (uint32_t)ref_names[r.rec].size(), r); counted += c.n;
            site_line(o, ref_names[r.rec].data(), (uint32_t)ref_names[r.rec].size(), r);
            if (sites) sites->push_back(r);
        }
    }
    return counted == body.size() ? SCS_OK : SCS_EDEVICE;       // (the sizing pass' sink and the emit pass' must agree)
}

}  // namespace scs
