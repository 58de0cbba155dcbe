// scs_lift.h -- the lift table: the staged haplotype records as stretches of the original reference, kept from
// the plan `simuvars` builds them by (SvPlan::pieces), and what one placed read adds to the bins of the REFERENCE through it.  One
// definition for the ctx and its host probes (lift_from_plan / lift_write / lift_parse: scs_lift_plan_probe, scs_lift_file_probe)
// and for the kernels and their host probe (lift_read, lift_point: scs_k_lift.hip / scs_lift_read_probe), so the test seams run the
// code the product runs.
//
// A segment is `len` haplotype bases from global genome index `hap_off` (records concatenated, as rec_off counts them).  kind 0 (R):
// copies of reference record ref_rec, 0-based [ref_pos, ref_pos + len) -- substitutions do not break a segment.  kind 1 (I): inserted
// sequence; ref_rec = the chromosome of its haplotype record, ref_pos = an anchor for information only (the end of the R segment
// before it in its record; none: the start of the next one; no R segment in the record: 0).  Segments ascend, tile [0, total), never
// straddle two haplotype records, and are maximal: no two neighbours could be one.  Consecutive R segments may jump backwards in
// the reference (copy 2 of a duplicated unit starts where copy 1 started): nothing here assumes monotone reference coordinates.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <fstream>
#include <map>
#include <string>
#include <vector>
#include "scs_truth.h"
#include "scs_simuvars.h"

namespace scs {

struct LiftSeg { uint64_t hap_off; uint64_t len; uint64_t ref_pos; uint32_t ref_rec; uint32_t kind; };
static_assert(sizeof(LiftSeg) == 32, "LiftSeg is 32 bytes");

// why lift_read gives up (the kernel raises FLAG_LIFT for each): the read is placed outside its record; an M run leaves the table
// or its record's segments; a segment lifts outside its reference record
enum LiftErr { LIFT_OK = 0, LIFT_EPLACE = 1, LIFT_ETABLE = 2, LIFT_EREF = 3 };

// the table and the reference's bins as lift_read sees them: ref_bin_off[r] = first bin of reference record r (depth_layout over
// the reference lengths), pseudo = their total = the bin of everything without a reference coordinate
struct LiftView { const LiftSeg* segs; uint32_t n_seg; const uint64_t* ref_len; const uint64_t* ref_bin_off; uint32_t n_ref; uint32_t bin_width; uint64_t pseudo; };

// the segment that holds global index x (n >= 1, segs[0].hap_off = 0): the last one that starts at or before it
SCS_HD uint32_t lift_find(const LiftSeg* segs, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].hap_off <= x) lo = mid; else hi = mid; }
    return lo;
}
// one staged position -> its reference record, coordinate (I: the anchor) and kind
SCS_HD void lift_point(const LiftSeg* segs, uint32_t n, uint64_t x, uint32_t& ref_rec, uint64_t& ref_pos, uint32_t& kind) {
    const LiftSeg s = segs[lift_find(segs, n, x)];
    ref_rec = s.ref_rec; kind = s.kind; ref_pos = s.kind ? s.ref_pos : s.ref_pos + (x - s.hap_off);
}

// What a placed read (truth_place has run) adds to the reference's bins: run(bin, bases) for the bases its M operations align, cut
// at segment ends and, inside an R segment, at the reference's bin boundaries (the pieces of one bin that follow one another are
// summed first; a bin met again after a jump is reported again), an I segment's bases in V.pseudo; then first(bin) once -- the bin
// of its first aligned base that has a reference coordinate, V.pseudo when it has none.  [rec0, rec1): its record's global indices.
// One bisection for a.lo, then a cursor that only moves forward; one division per R segment entered (and per deletion that leaves
// its piece), none per base.
template <class First, class Run>
SCS_HD int lift_read(const TruthAln& a, int64_t rec0, int64_t rec1, const LiftView& V, First first, Run run) {
    if (V.n_seg == 0 || a.lo < rec0 || a.hi >= rec1 || a.lo > a.hi) return LIFT_EPLACE;
    const uint64_t w = V.bin_width;
    uint64_t g = (uint64_t)a.lo, lim = 0, bin = 0, cur = 0, first_bin = V.pseudo;   // lim: first index behind the piece (segment and bin) g lies in
    uint32_t si = lift_find(V.segs, V.n_seg, g), acc = 0;
    LiftSeg sg = V.segs[si];
    bool fresh = true, have_cur = false, have_first = false; int err = LIFT_OK;      // fresh: bin and lim are not those of g
    truth_cigar_walk(a, [&](char k, uint32_t l) {
        if (err || k == 'I') return;
        if (k == 'D') { g += l; if (g >= lim) fresh = true; return; }
        while (l) {
            if (fresh || g == lim) {
                const bool same = !fresh && g < sg.hap_off + sg.len;                // the next bin of the R segment it is in
                if (!same) {
                    while (g >= sg.hap_off + sg.len) { if (++si >= V.n_seg) { err = LIFT_ETABLE; return; } sg = V.segs[si]; }
                    if (g < sg.hap_off || sg.hap_off + sg.len > (uint64_t)rec1) { err = LIFT_ETABLE; return; }
                }
                const uint64_t s_end = sg.hap_off + sg.len;
                if (same) { ++bin; lim += w; }
                else if (sg.kind == 0u) {
                    if (sg.ref_rec >= V.n_ref || sg.ref_pos + sg.len > V.ref_len[sg.ref_rec]) { err = LIFT_EREF; return; }
                    const uint64_t r = sg.ref_pos + (g - sg.hap_off), q = r / w;
                    bin = V.ref_bin_off[sg.ref_rec] + q; lim = g + ((q + 1u) * w - r);
                } else { bin = V.pseudo; lim = s_end; }
                if (lim > s_end) lim = s_end;
                fresh = false;
            }
            const uint32_t take = (uint64_t)l < lim - g ? l : (uint32_t)(lim - g);
            if (!have_first && bin != V.pseudo) { first_bin = bin; have_first = true; }
            if (!have_cur || bin != cur) { if (acc) run(cur, acc); cur = bin; acc = 0; have_cur = true; }
            acc += take; g += take; l -= take;
        }
    });
    if (err) return err;
    if (acc) run(cur, acc);
    first(first_bin);
    return LIFT_OK;
}

// ---- the table on the host: built from a plan, written, parsed
struct LiftTable {
    std::vector<LiftSeg> segs;
    std::vector<std::string> ref_names, hap_names; std::vector<uint64_t> ref_lens, hap_lens;   // reference records in order; staged records in staging order
    uint64_t total() const { uint64_t t = 0; for (uint64_t l : hap_lens) t += l; return t; }
    void clear() { segs.clear(); ref_names.clear(); hap_names.clear(); ref_lens.clear(); hap_lens.clear(); }
};

// the anchors of the I segments, by the rule above (hap_rec_of: the staged record of every segment)
inline void lift_set_anchors(LiftTable& T, const std::vector<uint32_t>& hap_rec_of) {
    const size_t n = T.segs.size();
    for (size_t i = 0; i < n;) {
        size_t j = i; while (j < n && hap_rec_of[j] == hap_rec_of[i]) ++j;              // [i, j): one staged record
        uint64_t anchor = 0;
        for (size_t k = i; k < j; ++k) if (T.segs[k].kind == 0u) { anchor = T.segs[k].ref_pos; break; }   // before the first R: its start
        for (size_t k = i; k < j; ++k) {
            LiftSeg& s = T.segs[k];
            if (s.kind == 0u) anchor = s.ref_pos + s.len; else s.ref_pos = anchor;
        }
        i = j;
    }
}

// The plan's pieces (ascending dst, covering the output) as segments: zero-length pieces dropped, neighbours of one record and kind
// that continue one another merged (the cuts Rope::split_at leaves; two insertions that abut are one I segment).  Plans are two
// staged records per chromosome, in chromosome order.  false: the plan is not what the comment of SvPlan says (why)
inline bool lift_from_plan(const std::vector<SvChrom>& chroms, const SvPlan& P, LiftTable& T, std::string& why) {
    T.clear();
    for (const SvChrom& c : chroms) { T.ref_names.push_back(c.name); T.ref_lens.push_back(c.len); }
    T.hap_names = P.rec_names; T.hap_lens = P.rec_lens;
    std::vector<uint64_t> hap_end(P.rec_lens.size() + 1, 0);
    for (size_t r = 0; r < P.rec_lens.size(); ++r) hap_end[r + 1] = hap_end[r] + P.rec_lens[r];
    if (P.rec_lens.size() != 2 * chroms.size()) { why = "lift table: the plan does not hold two haplotype records per chromosome"; return false; }
    std::vector<uint32_t> hap_rec_of; uint64_t at = 0; size_t rec = 0;
    for (const SvPiece& pc : P.pieces) {
        if (!pc.len) continue;
        if (pc.dst != at) { why = "lift table: the plan's pieces do not tile the output"; return false; }
        while (rec < P.rec_lens.size() && at >= hap_end[rec + 1]) ++rec;
        if (rec >= P.rec_lens.size() || at + pc.len > hap_end[rec + 1]) { why = "lift table: a piece of the plan straddles two haplotype records"; return false; }
        LiftSeg s{at, pc.len, 0, (uint32_t)(rec / 2), pc.lit ? 1u : 0u};
        if (!pc.lit) {
            size_t ci = (size_t)(std::upper_bound(chroms.begin(), chroms.end(), pc.src, [](uint64_t x, const SvChrom& c) { return x < c.off; }) - chroms.begin());
            if (ci == 0) { why = "lift table: a piece of the plan lies before the reference"; return false; }
            --ci;                                                                      // the last record that starts at or before src
            if (pc.src + pc.len > chroms[ci].off + chroms[ci].len) { why = "lift table: a piece of the plan leaves its reference record"; return false; }
            s.ref_rec = (uint32_t)ci; s.ref_pos = pc.src - chroms[ci].off;
        }
        at += pc.len;
        if (!T.segs.empty() && hap_rec_of.back() == (uint32_t)rec) {
            LiftSeg& p = T.segs.back();
            if (p.kind == s.kind && (s.kind == 1u || (p.ref_rec == s.ref_rec && p.ref_pos + p.len == s.ref_pos))) { p.len += s.len; continue; }
        }
        T.segs.push_back(s); hap_rec_of.push_back((uint32_t)rec);
    }
    if (at != P.total || at != hap_end.back()) { why = "lift table: the plan's pieces do not cover the output"; return false; }
    lift_set_anchors(T, hap_rec_of);
    return true;
}

// the file: "##scssim-lift v1", "#ref\t<name>\t<length>" per reference record, "#hap\t<name>\t<length>" per staged record, then per
// segment <hap name> <hap start> <hap end> <ref name> <ref start> <ref end> R|I, tab-separated, BED coordinates inside the records
inline bool lift_write(const LiftTable& T, const std::string& path) {
    FILE* o = fopen(path.c_str(), "w");
    if (!o) return false;
    bool ok = fputs("##scssim-lift v1\n", o) != EOF;
    for (size_t r = 0; r < T.ref_names.size() && ok; ++r) ok = fprintf(o, "#ref\t%s\t%llu\n", T.ref_names[r].c_str(), (unsigned long long)T.ref_lens[r]) > 0;
    for (size_t r = 0; r < T.hap_names.size() && ok; ++r) ok = fprintf(o, "#hap\t%s\t%llu\n", T.hap_names[r].c_str(), (unsigned long long)T.hap_lens[r]) > 0;
    uint64_t rec0 = 0; size_t rec = 0;
    for (const LiftSeg& s : T.segs) {
        if (!ok) break;
        while (rec < T.hap_lens.size() && s.hap_off >= rec0 + T.hap_lens[rec]) rec0 += T.hap_lens[rec++];
        if (rec >= T.hap_lens.size() || s.ref_rec >= T.ref_names.size()) { ok = false; break; }
        const unsigned long long h0 = s.hap_off - rec0, r0 = s.ref_pos;
        ok = fprintf(o, "%s\t%llu\t%llu\t%s\t%llu\t%llu\t%c\n", T.hap_names[rec].c_str(), h0, h0 + (unsigned long long)s.len, T.ref_names[s.ref_rec].c_str(), r0,
                     s.kind ? r0 : r0 + (unsigned long long)s.len, s.kind ? 'I' : 'R') > 0;
    }
    return (fclose(o) == 0) && ok;
}

// Parses the file into T.  false: it cannot be opened (line = 0) or is malformed -- `why` says how, `line` where (1-based; one past
// the last line when the file ends too early).  Malformed: a missing header; a wrong column count; a number that is none; an
// unknown record name; lines that leave a gap, overlap or are not in staging order; a segment of no bases, past its haplotype
// record or past its reference record; an R line whose two lengths differ; an I line whose reference interval is not empty
inline bool lift_parse(const std::string& path, LiftTable& T, std::string& why, uint64_t& line) {
    T.clear(); line = 0;
    std::ifstream in(path);
    if (!in.is_open()) { why = "can not open " + path; return false; }
    auto split = [](const std::string& s) { std::vector<std::string> f; size_t b = 0; for (;;) { const size_t e = s.find('\t', b); if (e == std::string::npos) { f.push_back(s.substr(b)); break; } f.push_back(s.substr(b, e - b)); b = e + 1; } return f; };
    auto num = [](const std::string& s, uint64_t& v) { if (s.empty() || s.size() > 19) return false; v = 0; for (char ch : s) { if (ch < '0' || ch > '9') return false; v = v * 10 + (uint64_t)(ch - '0'); } return true; };
    std::string ln; std::map<std::string, uint32_t> ref_of, hap_of;
    bool data = false; size_t rec = 0; uint64_t rec0 = 0, at = 0;                  // at: where the next segment must start inside record `rec`
    std::vector<uint32_t> hap_rec_of;
    auto bad = [&](const std::string& m) { why = m; return false; };
    while (std::getline(in, ln)) {
        ++line;
        if (!ln.empty() && ln.back() == '\r') ln.pop_back();
        if (line == 1) { if (ln != "##scssim-lift v1") return bad("missing header: the first line is not \"##scssim-lift v1\""); continue; }
        const std::vector<std::string> f = split(ln);
        if (f[0] == "#ref" || f[0] == "#hap") {
            uint64_t len = 0;
            if (data) return bad("a header line behind the first segment");
            if (f.size() != 3) return bad("wrong column count: a " + f[0] + " line has 3 columns");
            if (!num(f[2], len)) return bad("not a length: " + f[2]);
            const bool ref = f[0] == "#ref"; auto& names = ref ? T.ref_names : T.hap_names; auto& idx = ref ? ref_of : hap_of;
            if (ref && !T.hap_names.empty()) return bad("a #ref line behind the #hap lines");
            if (idx.count(f[1])) return bad("record " + f[1] + " is named twice");
            idx[f[1]] = (uint32_t)names.size(); names.push_back(f[1]); (ref ? T.ref_lens : T.hap_lens).push_back(len);
            continue;
        }
        if (T.ref_names.empty() || T.hap_names.empty()) return bad("missing header: no #ref / #hap lines before the first segment");
        data = true;
        if (f.size() != 7) return bad("wrong column count: a segment line has 7 columns");
        uint64_t h0, h1, r0, r1;
        if (!num(f[1], h0) || !num(f[2], h1) || !num(f[4], r0) || !num(f[5], r1)) return bad("not a coordinate");
        if (f[6] != "R" && f[6] != "I") return bad("the kind is neither R nor I: " + f[6]);
        const auto hi = hap_of.find(f[0]); const auto ri = ref_of.find(f[3]);
        if (hi == hap_of.end()) return bad("unknown haplotype record " + f[0]);
        if (ri == ref_of.end()) return bad("unknown reference record " + f[3]);
        while (rec < T.hap_lens.size() && at == T.hap_lens[rec] && hi->second != rec) { rec0 += T.hap_lens[rec++]; at = 0; }   // the record is tiled: on to the next
        if (rec >= T.hap_lens.size() || hi->second != rec) return bad(hi->second < rec ? "lines are not in staging order: record " + f[0] + " again" : "a gap: record " + T.hap_names[std::min(rec, T.hap_names.size() - 1)] + " is not covered to its end");
        if (h0 != at) return bad(h0 < at ? "an overlap (or unsorted lines): the segment starts before the last one's end" : "a gap before the segment");
        if (h1 <= h0) return bad("a segment of no bases");
        if (h1 > T.hap_lens[rec]) return bad("the segment ends past its haplotype record");
        const bool ins = f[6] == "I";
        if (r1 < r0 || r1 > T.ref_lens[ri->second]) return bad("the segment ends past its reference record");
        if (!ins && r1 - r0 != h1 - h0) return bad("an R line whose two lengths differ");
        if (ins && r1 != r0) return bad("an I line whose reference interval is not empty");
        T.segs.push_back(LiftSeg{rec0 + h0, h1 - h0, r0, ri->second, ins ? 1u : 0u}); hap_rec_of.push_back((uint32_t)rec);
        at = h1;
    }
    ++line;
    if (line == 1) return bad("missing header: the file is empty");
    if (T.ref_names.empty() || T.hap_names.empty()) return bad("missing header: no #ref / #hap lines");
    while (rec < T.hap_lens.size() && at == T.hap_lens[rec]) { rec0 += T.hap_lens[rec++]; at = 0; }
    if (rec < T.hap_lens.size()) return bad("a gap: record " + T.hap_names[rec] + " is not covered to its end");
    if (T.segs.size() > 0xFFFFFFF0ull) return bad("more than 2^32 segments");
    return true;
}

}  // namespace scs
