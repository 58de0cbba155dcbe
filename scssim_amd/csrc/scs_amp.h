// scs_amp.h -- one line of the amplicon table (scs_write_amplicons / scs_amplicon_places): where a full
// amplicon lies on the genome, which strand it copies, and every base where it differs from the genome it copies.  One definition
// for the device passes (scs_k_amplicons.hip: placement, sizing with a counting sink, emit into LDS) and the host probe
// (scs_amplicon_line_probe), so the test seam runs the code the kernels run.
//
// The full amplicon sequence is U[t] = maybe_comp(G[base + dir * t]), t in [0, len), patched by the semi's errors (at
// t = k1 - pos(e), value comp(alt)) and then by the full's own (at t = pos(e), value alt) -- PairRec in scs_device.h, resolved the
// way k_plan_pairs resolves it: the fragment's template view, the semi's template strand on it, shifted by the full's start.
#pragma once
#include <stdint.h>
#include "scs_common.h"
#include "scs_truth.h"
#include "../../include/scssim_hip.h"
#include <string.h>
#include <string>
#include <vector>

namespace scs {

// the amplicon as an index map of the genome
struct AmpPlace { int64_t base; int32_t dir; uint32_t comp; int32_t k1; uint32_t len; };

// false: the lineage does not fit its parents (the semi inside the fragment, the full inside the semi)
SCS_HD bool amp_resolve(uint64_t goff, uint32_t flen, int fstrand, uint32_t s_spos, uint32_t s_len, uint32_t f_spos, uint32_t f_len, AmpPlace& p) {
    if (f_len == 0 || (uint64_t)s_spos + s_len > flen || (uint64_t)f_spos + f_len > s_len) return false;
    // template strand of the fragment: strand > 0 runs backwards and complemented over the slice, else forwards
    int64_t base = fstrand > 0 ? (int64_t)goff + flen - 1 : (int64_t)goff; int32_t dir = fstrand > 0 ? -1 : 1; uint32_t comp = fstrand > 0 ? 1u : 0u;
    // template strand c(S) of the semi (s, l) made on it, then the full's window from f_spos on
    base += (int64_t)dir * (int64_t)(s_spos + s_len - 1); dir = -dir; comp ^= 1u;
    base += (int64_t)dir * (int64_t)f_spos;
    p.base = base; p.dir = dir; p.comp = comp; p.k1 = (int32_t)(s_len - 1 - f_spos); p.len = f_len;
    return true;
}
SCS_HD int64_t amp_lo(const AmpPlace& p) { return p.dir > 0 ? p.base : p.base - (int64_t)(p.len - 1); }   // leftmost genome index
// '+': a forward copy of the genome; '-': its reverse complement; 0: the two flags are not a strand
SCS_HD char amp_strand(const AmpPlace& p) { return p.dir > 0 && !p.comp ? '+' : p.dir < 0 && p.comp ? '-' : (char)0; }

// an amplicon's error list as the amplification leaves it: four inline 16-bit entries (0 = empty), or bit 63 set: `count` entries
// of the overflow pool from `offset` on (scs_common.h)
struct AmpErrs {
    uint64_t w; const uint32_t* pool;
    SCS_HD uint32_t slots() const { return (w & ERR_OVERFLOW_BIT) ? (uint32_t)(w >> 32) & 0xFFFFu : (w ? 4u : 0u); }
    SCS_HD uint32_t at(uint32_t i) const { return (w & ERR_OVERFLOW_BIT) ? pool[(uint32_t)w + i] : (uint32_t)(w >> (16u * i)) & 0xFFFFu; }
};

// The edits in ascending genome coordinate, each coordinate once: f(x, ref, alt) with x the genome index, ref = gen(x) (code 0..4)
// and alt the amplicon's base read genome-forward.  Selection by repeated minimum over the two lists: no buffer, no cap (the mean
// count is below 1).  key(t) = the position's rank in genome order.  Returns the number of edits.
template <class Gen, class F>
SCS_HD uint32_t amp_edits(const AmpPlace& p, const AmpErrs& e1, const AmpErrs& e2, Gen gen, F f) {
    const int64_t len = (int64_t)p.len, none = (int64_t)1 << 40;
    const uint32_t n1 = e1.slots(), n2 = e2.slots();
    uint32_t n = 0;
    for (int64_t prev = -1;;) {
        int64_t best = none;
        for (uint32_t i = 0; i < n1; ++i) {
            const uint32_t v = e1.at(i); if (!v) continue;
            const int64_t t = (int64_t)p.k1 - (int64_t)err_pos(v); if (t < 0 || t >= len) continue;
            const int64_t key = p.dir > 0 ? t : len - 1 - t; if (key > prev && key < best) best = key;
        }
        for (uint32_t i = 0; i < n2; ++i) {
            const uint32_t v = e2.at(i); if (!v) continue;
            const int64_t t = (int64_t)err_pos(v); if (t >= len) continue;
            const int64_t key = p.dir > 0 ? t : len - 1 - t; if (key > prev && key < best) best = key;
        }
        if (best == none) break;
        prev = best;
        const int64_t t = p.dir > 0 ? best : len - 1 - best;
        uint32_t c = 255u;                                 // the patched base: the semi's entry, then the full's (it wins)
        for (uint32_t i = 0; i < n1; ++i) { const uint32_t v = e1.at(i); if (v && (int64_t)p.k1 - (int64_t)err_pos(v) == t) c = 3u - err_alt(v); }
        for (uint32_t i = 0; i < n2; ++i) { const uint32_t v = e2.at(i); if (v && (int64_t)err_pos(v) == t) c = err_alt(v); }
        const int64_t x = p.base + (int64_t)p.dir * t;
        const uint32_t g = gen(x), u = p.comp ? (uint32_t)comp_code((uint8_t)g) : g;
        if (c == u) continue;                              // (a full's error that restores the genome base)
        f(x, g, p.comp ? 3u - c : c); ++n;
    }
    return n;
}

SCS_HD char amp_letter(uint32_t c) { return c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : c == 3 ? 'T' : 'N'; }

// who the amplicon is: its record (name, genome index of its first base), its index in the job's list, its semi, its reads
struct AmpLine { const char* rname; uint32_t rname_len; int64_t rec0; uint32_t index, semi, reads; };

// "record\tstart\tend\tamplicon\tstrand\treads\tsemi\tedits\n" through o.put(char); edits = pos:R>A joined by commas, or "."
template <class Out, class Gen>
SCS_HD void amp_line(Out& o, const AmpLine& li, const AmpPlace& p, const AmpErrs& e1, const AmpErrs& e2, Gen gen) {
    const uint64_t start = (uint64_t)(amp_lo(p) - li.rec0);
    for (uint32_t i = 0; i < li.rname_len; ++i) o.put(li.rname[i]);
    o.put('\t'); truth_num(o, start); o.put('\t'); truth_num(o, start + p.len); o.put('\t'); truth_num(o, li.index);
    o.put('\t'); o.put(amp_strand(p)); o.put('\t'); truth_num(o, li.reads); o.put('\t'); truth_num(o, li.semi); o.put('\t');
    bool first = true;
    const uint32_t n = amp_edits(p, e1, e2, gen, [&](int64_t x, uint32_t ref, uint32_t alt) {
        if (!first) o.put(',');
        first = false;
        truth_num(o, (uint64_t)(x - li.rec0)); o.put(':'); o.put(amp_letter(ref)); o.put('>'); o.put(amp_letter(alt));
    });
    if (!n) o.put('.');
    o.put('\n');
}

// ---- host-only: one amplicon's line from its lineage, through the functions above (scs_amplicon_line_probe; no GPU, no ctx).
// Error entries are (pos << 3) | alt, as scs_download_amplicons reports them; they are packed the way the amplification leaves
// them -- up to four inline, more in an overflow pool -- so both forms of the list take part.  genome: the bases from genome index
// genome_start on (any case; anything but ACGT is N).  SCS_EINVAL: a lineage that does not fit its parents, its record or the
// genome given, or an entry that is no error of its amplicon
inline int amp_line_probe(uint64_t frag_goff, uint32_t frag_len, int frag_strand, uint32_t semi_spos, uint32_t semi_len, const uint32_t* semi_errs, uint32_t n_semi_errs,
                          uint32_t full_spos, uint32_t full_len, const uint32_t* full_errs, uint32_t n_full_errs,
                          const char* genome, uint64_t genome_start, uint64_t genome_len, uint64_t rec_off, uint64_t rec_len, const char* rec_name,
                          uint32_t index, uint32_t reads, uint32_t semi, std::string& line) {
    if (!genome || !rec_name || (n_semi_errs && !semi_errs) || (n_full_errs && !full_errs) || n_semi_errs > 0xFFFFu || n_full_errs > 0xFFFFu) return SCS_EINVAL;
    if ((frag_strand != 1 && frag_strand != -1) || frag_len > 131071u || semi_len > 2047u || full_len > 2047u) return SCS_EINVAL;
    AmpPlace p;
    if (!amp_resolve(frag_goff, frag_len, frag_strand, semi_spos, semi_len, full_spos, full_len, p) || !amp_strand(p)) return SCS_EINVAL;
    const int64_t lo = amp_lo(p);
    if (lo < (int64_t)rec_off || (uint64_t)lo + p.len > rec_off + rec_len) return SCS_EINVAL;
    if (frag_goff < rec_off || frag_goff + frag_len > rec_off + rec_len) return SCS_EINVAL;        // a fragment never straddles records
    if (lo < (int64_t)genome_start || (uint64_t)lo + p.len > genome_start + genome_len) return SCS_EINVAL;
    std::vector<uint32_t> pool;
    auto pack = [&](const uint32_t* e, uint32_t n, uint32_t alen, uint64_t& w) {
        w = 0;
        if (n > 4) { w = ERR_OVERFLOW_BIT | ((uint64_t)n << 32) | (uint64_t)pool.size(); }
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t pos = e[i] >> 3, alt = e[i] & 7u, v = err_pack(pos, alt);
            if (pos >= alen || alt > 3u || v == 0) return false;
            if (n > 4) pool.push_back(v); else w |= (uint64_t)v << (16u * i);
        }
        return true;
    };
    uint64_t w1 = 0, w2 = 0;
    if (!pack(semi_errs, n_semi_errs, semi_len, w1) || !pack(full_errs, n_full_errs, full_len, w2)) return SCS_EINVAL;
    pool.push_back(0);                                     // (never an empty pool behind the pointer)
    const AmpErrs e1{w1, pool.data()}, e2{w2, pool.data()};
    struct StrOut { std::string* t; void put(char ch) { t->push_back(ch); } } o{&line};
    const AmpLine li{rec_name, (uint32_t)strlen(rec_name), (int64_t)rec_off, index, semi, reads};
    line.clear();
    amp_line(o, li, p, e1, e2, [&](int64_t x) -> uint32_t {
        const char ch = genome[x - (int64_t)genome_start];
        return ch == 'A' || ch == 'a' ? 0u : ch == 'C' || ch == 'c' ? 1u : ch == 'G' || ch == 'g' ? 2u : ch == 'T' || ch == 't' ? 3u : 4u;
    });
    TruthCount cnt; amp_line(cnt, li, p, e1, e2, [&](int64_t x) -> uint32_t {
        const char ch = genome[x - (int64_t)genome_start];
        return ch == 'A' || ch == 'a' ? 0u : ch == 'C' || ch == 'c' ? 1u : ch == 'G' || ch == 'g' ? 2u : ch == 'T' || ch == 't' ? 3u : 4u;
    });
    return cnt.n == line.size() ? SCS_OK : SCS_EDEVICE;      // (the sizing pass' sink and the emit pass' must agree)
}

}  // namespace scs
