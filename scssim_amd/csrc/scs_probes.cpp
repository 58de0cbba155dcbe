// scs_probes.cpp -- the test seams and kernel-level entry points of the C ABI: host-only probes of the formatters, parsers and
// planners the product runs (truth SAM, FASTA, simuvars, BGZF, the profile tables), device probes of single kernels (BGZF, the
// scans, DevBuf, Philox, det_log, Profile::predict), and the census of live device resources.  Nothing here is on a job's path.
#include "scs_sitejob.h"
#include "scs_amp.h"
#include "scs_support.h"
#include "scs_support_ref.h"
#include "scs_truth_ref.h"

// host-only: one read's record through the formatter the truth kernels run (scs_truth.h), as SAM text or as a BAM record
static int truth_probe(bool bam, int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                       int64_t pos0, int reverse, const int32_t* events, int nev,
                       int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                       const char* seq, const char* qual, int len, const char* genome, int64_t genome_start, uint64_t genome_len,
                       char* out, size_t cap, size_t* n_out) {
    if (!rname || !seq || !qual || !genome || !n_out || n <= 0 || nev < 0 || mate_nev < 0 || (nev && !events) || (paired && mate_nev && !mate_events)) return SCS_EINVAL;
    auto pack = [](const int32_t* e, int k, std::vector<uint32_t>& v) {
        for (int i = 0; i < k; ++i) {
            if (e[3 * i] < 0 || e[3 * i] > 0xFFFF || e[3 * i + 2] <= 0 || e[3 * i + 2] > 0x7FFF) return false;
            v.push_back(tev_pack((uint32_t)e[3 * i], e[3 * i + 1] ? 1u : 0u, (uint32_t)e[3 * i + 2]));
        }
        return true;
    };
    std::vector<uint32_t> e1, e2;
    if (!pack(events, nev, e1) || (paired && !pack(mate_events, mate_nev, e2))) return SCS_EINVAL;
    TruthAln a{pos0, reverse ? 1 : 0, n, nev, e1.data(), 0, 0, 0}, m{mate_pos0, mate_reverse ? 1 : 0, n, mate_nev, e2.data(), 0, 0, 0};
    if (!truth_place(a) || a.qlen != len || (paired && !truth_place(m))) return SCS_EINVAL;
    if (a.lo < genome_start || a.hi >= genome_start + (int64_t)genome_len) return SCS_EINVAL;
    TruthLine li{amp, cnt, 0u, paired ? 1 : 0, rname, (uint32_t)strlen(rname), 0, 0, 0};
    if (paired) {
        const int64_t left = std::min(a.lo, m.lo), right = std::max(a.hi, m.hi), t = right - left + 1;
        li.flag = 0x3u | (is_read2 ? 0x80u : 0x40u) | (a.rev ? 0x10u : 0u) | (m.rev ? 0x20u : 0u);
        li.mate_lo = m.lo;
        li.tlen = (a.lo < m.lo || (a.lo == m.lo && !is_read2)) ? t : -t;   // positive on the leftmost read (read 1 on a tie, as the kernels)
    } else li.flag = a.rev ? 0x10u : 0u;
    struct Src {
        const char* s; const char* q; const char* g; int64_t g0;
        char seq(int i) const { return s[i]; } char qual(int i) const { return q[i]; }
        char gen(int64_t x) const { const char ch = g[x - g0]; return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' ? ch : ch == 'a' ? 'A' : ch == 'c' ? 'C' : ch == 'g' ? 'G' : ch == 't' ? 'T' : 'N'; }
    } src{seq, qual, genome, genome_start};
    struct VecOut {
        std::string t;
        void put(char ch) { t.push_back(ch); }
        uint32_t pos() const { return (uint32_t)t.size(); }
        void poke32(uint32_t at, uint32_t v) { for (int k = 0; k < 4; ++k) t[at + k] = (char)(v >> (8 * k)); }
    } o;
    if (bam) {
        truth_bam_record(o, a, li, src, 0);
        if (o.t.size() != truth_bam_size(a, li, src)) return SCS_EDEVICE;              // (the sizing pass' arithmetic and the formatter must agree)
    } else truth_record(o, a, li, src);
    *n_out = o.t.size();
    if (out) { if (o.t.size() > cap) return SCS_EOVERFLOW; memcpy(out, o.t.data(), o.t.size()); }
    return SCS_OK;
}

extern "C" {

int scs_truth_record_probe(int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                           int64_t pos0, int reverse, const int32_t* events, int nev,
                           int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                           const char* seq, const char* qual, int len, const char* genome, int64_t genome_start, uint64_t genome_len,
                           char* out, size_t cap, size_t* n_out) {
    return truth_probe(false, paired, is_read2, amp, cnt, rname, n, pos0, reverse, events, nev, mate_pos0, mate_reverse, mate_events, mate_nev,
                       seq, qual, len, genome, genome_start, genome_len, out, cap, n_out);
}
int scs_truth_bam_record_probe(int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                               int64_t pos0, int reverse, const int32_t* events, int nev,
                               int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                               const char* seq, const char* qual, int len, const char* genome, int64_t genome_start, uint64_t genome_len,
                               char* out, size_t cap, size_t* n_out) {
    return truth_probe(true, paired, is_read2, amp, cnt, rname, n, pos0, reverse, events, nev, mate_pos0, mate_reverse, mate_events, mate_nev,
                       seq, qual, len, genome, genome_start, genome_len, out, cap, n_out);
}

// host-only: one read's record on the original reference through the formatter the kernels of scs_k_truth_ref.hip run
// (scs_truth_ref.h), the sizing pass' counting sink checked against it.  names: the reference records' names, then the staged
// records', a newline behind each (rname NULL: the staged record's name from there)
int scs_truth_ref_record_probe(int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                               int64_t pos0, int reverse, const int32_t* events, int nev,
                               int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                               const char* seq, const char* qual, int len,
                               const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                               const uint64_t* hap_lens, uint32_t n_hap, const uint64_t* ref_lens, uint32_t n_ref, const char* names, size_t names_len,
                               char* out, size_t cap, size_t* n_out, int* lift_err) {
    if (lift_err) *lift_err = 0;
    if (!seq || !qual || !n_out || n <= 0 || nev < 0 || mate_nev < 0 || nev > TRUTH_EVCAP || mate_nev > TRUTH_EVCAP || (nev && !events) || (paired && mate_nev && !mate_events) ||
        !n_hap || !hap_lens || (n_ref && !ref_lens) || !names || (n_seg && (!seg_hap_off || !seg_len || !seg_ref_pos || !seg_ref_rec || !seg_kind))) return SCS_EINVAL;
    auto pack = [](const int32_t* e, int k, std::vector<uint32_t>& v) {
        for (int i = 0; i < k; ++i) {
            if (e[3 * i] < 0 || e[3 * i] > 0xFFFF || e[3 * i + 2] <= 0 || e[3 * i + 2] > 0x7FFF) return false;
            v.push_back(tev_pack((uint32_t)e[3 * i], e[3 * i + 1] ? 1u : 0u, (uint32_t)e[3 * i + 2]));
        }
        return true;
    };
    std::vector<uint32_t> e1, e2;
    if (!pack(events, nev, e1) || (paired && !pack(mate_events, mate_nev, e2))) return SCS_EINVAL;
    TruthAln a{pos0, reverse ? 1 : 0, n, nev, e1.data(), 0, 0, 0}, m{mate_pos0, mate_reverse ? 1 : 0, n, mate_nev, e2.data(), 0, 0, 0};
    if (!truth_place(a) || a.qlen != len || (paired && !truth_place(m))) return SCS_EINVAL;
    std::vector<std::string> nm; { std::string cur; for (size_t i = 0; i < names_len; ++i) { if (names[i] == '\n') { nm.push_back(cur); cur.clear(); } else cur.push_back(names[i]); } }
    if (nm.size() < n_ref || (!rname && nm.size() < (size_t)n_ref + n_hap)) return SCS_EINVAL;
    std::vector<uint32_t> noff(n_ref + 1, 0); std::string text;
    for (uint32_t r = 0; r < n_ref; ++r) { text += nm[r]; noff[r + 1] = (uint32_t)text.size(); }
    std::vector<LiftSeg> segs(n_seg);
    for (uint32_t i = 0; i < n_seg; ++i) segs[i] = LiftSeg{seg_hap_off[i], seg_len[i], seg_ref_pos[i], seg_ref_rec[i], seg_kind[i]};
    std::vector<uint64_t> roff(n_hap + 1, 0);
    for (uint32_t r = 0; r < n_hap; ++r) roff[r + 1] = roff[r] + hap_lens[r];
    const uint32_t lo = rec_of(roff.data(), n_hap, paired && is_read2 ? m.lo : a.lo);  // the staged record, as the kernel finds it (read 1's; the mate must lie there too)
    const int64_t r0 = (int64_t)roff[lo], r1 = (int64_t)roff[lo + 1];
    const LiftTab T{segs.data(), n_seg, ref_lens, n_ref};
    LiftAln la{}, lm{};
    int err = lift_align(a, r0, r1, T, la);
    if (!err && paired) err = lift_align(m, r0, r1, T, lm);
    if (err) { if (lift_err) *lift_err = err; return SCS_EINVAL; }
    const std::string hname = rname ? std::string(rname) : nm[n_ref + lo];
    const TruthRefLine li{amp, cnt, paired ? 1 : 0, is_read2 ? 1 : 0, paired ? m.rev : 0, hname.data(), (uint32_t)hname.size(), r0, r1, noff.data(), text.data()};
    struct Src { const char* s; const char* q; char seq(int i) const { return s[i]; } char qual(int i) const { return q[i]; } } src{seq, qual};
    struct VecOut { std::string t; void put(char ch) { t.push_back(ch); } } o;
    TruthCount cn;
    if ((err = truth_ref_record(o, a, li, T, la, lm, src)) || (err = truth_ref_record(cn, a, li, T, la, lm, src))) { if (lift_err) *lift_err = err; return SCS_EINVAL; }
    if (cn.n != o.t.size()) return SCS_EDEVICE;                                        // (the sizing pass' sink and the formatter must agree)
    *n_out = o.t.size();
    if (out) { if (o.t.size() > cap) return SCS_EOVERFLOW; memcpy(out, o.t.data(), o.t.size()); }
    return SCS_OK;
}

// host-only: the depth track's bin layout through the function the ctx runs (depth_layout, scs_depth.h); nothing of the bins' size is allocated
int scs_depth_layout_probe(const uint64_t* rec_lens, int n_records, uint32_t bin_width, uint64_t* bin_off, uint64_t* n_bins) {
    if (n_records < 0 || (n_records && !rec_lens)) return SCS_EINVAL;
    uint32_t min_w = 0;
    if (depth_layout(rec_lens, (size_t)n_records, bin_width, bin_off, n_bins, &min_w)) return SCS_OK;
    create_error() = bin_width ? "scs_depth_layout_probe: more than 2^27 bins; " + (min_w ? "the smallest bin width these records admit is " + std::to_string(min_w) : std::string("no bin width below 2^32 is enough"))
                               : std::string("scs_depth_layout_probe: bin_width is 0");
    return SCS_EINVAL;
}
// host-only: one read through the function the depth kernel runs (depth_read, scs_depth.h) after the truth passes' placement
int scs_depth_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev, uint64_t rec_len, uint32_t bin_width,
                         uint64_t* reads_bin, uint64_t* bins, uint32_t* bases, int cap, int* n_out) {
    if (!n_out || n <= 0 || nev < 0 || (nev && !events) || bin_width == 0 || cap < 0 || (cap && (!bins || !bases))) return SCS_EINVAL;
    std::vector<uint32_t> ev;
    for (int i = 0; i < nev; ++i) {
        if (events[3 * i] < 0 || events[3 * i] > 0xFFFF || events[3 * i + 2] <= 0 || events[3 * i + 2] > 0x7FFF) return SCS_EINVAL;
        ev.push_back(tev_pack((uint32_t)events[3 * i], events[3 * i + 1] ? 1u : 0u, (uint32_t)events[3 * i + 2]));
    }
    TruthAln a{pos0, reverse ? 1 : 0, n, nev, ev.data(), 0, 0, 0};
    if (!truth_place(a) || a.lo < 0 || a.hi >= (int64_t)rec_len) return SCS_EINVAL;
    std::vector<std::pair<uint64_t, uint32_t>> runs; uint64_t first = 0;
    depth_read(a, 0, bin_width, [&](uint64_t b) { first = b; }, [&](uint64_t b, uint32_t k) { runs.push_back({b, k}); });
    if (reads_bin) *reads_bin = first;
    *n_out = (int)runs.size();
    if ((int)runs.size() > cap) return SCS_EOVERFLOW;
    for (size_t i = 0; i < runs.size(); ++i) { bins[i] = runs[i].first; bases[i] = runs[i].second; }
    return SCS_OK;
}

// host-only: one read through the function k_cov_mark runs (cov_read, scs_coverage.h) after the truth passes' placement: the
// intervals [starts[i], ends[i]) of record coordinates it marks, ascending
int scs_coverage_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev, uint64_t rec_len, uint64_t* starts, uint64_t* ends, int cap, int* n_out) {
    if (!n_out || n <= 0 || nev < 0 || nev > TRUTH_EVCAP || (nev && !events) || cap < 0 || (cap && (!starts || !ends))) return SCS_EINVAL;   // (more events: the kernel raises FLAG_COVERAGE)
    std::vector<uint32_t> ev;
    for (int i = 0; i < nev; ++i) {
        if (events[3 * i] < 0 || events[3 * i] > 0xFFFF || events[3 * i + 2] <= 0 || events[3 * i + 2] > 0x7FFF) return SCS_EINVAL;
        ev.push_back(tev_pack((uint32_t)events[3 * i], events[3 * i + 1] ? 1u : 0u, (uint32_t)events[3 * i + 2]));
    }
    TruthAln a{pos0, reverse ? 1 : 0, n, nev, ev.data(), 0, 0, 0};
    if (!truth_place(a) || a.lo < 0 || a.hi >= (int64_t)rec_len) return SCS_EINVAL;
    std::vector<int64_t> up, down;
    cov_read(a, [&](int64_t g, int d) { (d > 0 ? up : down).push_back(g); });
    if (up.size() != down.size()) return SCS_EDEVICE;
    *n_out = (int)up.size();
    if ((int)up.size() > cap) return SCS_EOVERFLOW;
    for (size_t i = 0; i < up.size(); ++i) { starts[i] = (uint64_t)up[i]; ends[i] = (uint64_t)down[i]; }
    return SCS_OK;
}
// host-only: one histogram row (max_depth + 1 buckets) and its exact sum through the function scs_write_coverage runs (cov_stats,
// scs_coverage.h): out = mean, breadth at 1, 5, 10, 20, gini
int scs_coverage_stats_probe(const uint64_t* hist, uint32_t max_depth, uint64_t sum, double out[6]) {
    if (!hist || !out || max_depth < 1u || max_depth > COV_MAX_DEPTH) return SCS_EINVAL;
    const CovStats s = cov_stats(hist, max_depth, sum);
    out[0] = s.mean; for (int i = 0; i < 4; ++i) out[1 + i] = s.breadth[i]; out[5] = s.gini;
    return SCS_OK;
}
// the end-of-job pass' tile and the chunk of its tile-offset scan: where the tests aim
void scs_coverage_tile(uint32_t* tile, uint32_t* chunk) { if (tile) *tile = COV_TILE; if (chunk) *chunk = COV_CHUNK; }
// host-only: one read through the function the site support kernel runs (support_read, scs_support.h) after the truth passes'
// placement: seq = the FASTQ record's `len` bases, positions = the listed record coordinates, ascending and distinct
int scs_support_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev, uint64_t rec_len, const char* seq, int len,
                           const uint64_t* positions, uint64_t n_pos, uint64_t* index, uint8_t* cls, int cap, int* n_out) {
    if (!n_out || !seq || n <= 0 || nev < 0 || (nev && !events) || (n_pos && !positions) || cap < 0 || (cap && (!index || !cls))) return SCS_EINVAL;
    for (uint64_t i = 1; i < n_pos; ++i) if (positions[i] <= positions[i - 1]) return SCS_EINVAL;
    std::vector<uint32_t> ev;
    for (int i = 0; i < nev; ++i) {
        if (events[3 * i] < 0 || events[3 * i] > 0xFFFF || events[3 * i + 2] <= 0 || events[3 * i + 2] > 0x7FFF) return SCS_EINVAL;
        ev.push_back(tev_pack((uint32_t)events[3 * i], events[3 * i + 1] ? 1u : 0u, (uint32_t)events[3 * i + 2]));
    }
    if (nev > TRUTH_EVCAP) return SCS_EINVAL;                                        // (the kernel raises FLAG_SUPPORT there)
    TruthAln a{pos0, reverse ? 1 : 0, n, nev, ev.data(), 0, 0, 0};
    if (!truth_place(a) || a.lo < 0 || a.hi >= (int64_t)rec_len || a.qlen != len) return SCS_EINVAL;
    std::vector<std::pair<uint64_t, uint32_t>> got;
    support_read(a, positions, n_pos, [&](int i) { return seq[i]; }, [&](uint64_t i, uint32_t k) { got.push_back({i, k}); });
    *n_out = (int)got.size();
    if ((int)got.size() > cap) return SCS_EOVERFLOW;
    for (size_t i = 0; i < got.size(); ++i) { index[i] = got[i].first; cls[i] = (uint8_t)got[i].second; }
    return SCS_OK;
}
// host-only: one site's line through the formatter the emit kernel runs (site_line, scs_site.h); counts: its six counters (the site
// support table's line), or NULL (the artefact table's)
int scs_site_support_line_probe(const char* name, uint64_t pos, uint32_t ref, uint32_t alt, uint32_t na, uint32_t ta, uint64_t nr, uint64_t tr, const uint32_t* counts,
                                char* out, size_t cap, size_t* n_out) {
    if (!name || !n_out || ref > 4u || alt > 3u) return SCS_EINVAL;
    SiteRec r{pos, nr, tr, 0u, na, ta, (uint8_t)ref, (uint8_t)alt, {0, 0}};
    struct StrOut { std::string t; void put(char ch) { t.push_back(ch); } } o;
    TruthCount cnt; site_line(cnt, name, (uint32_t)strlen(name), r, counts); site_line(o, name, (uint32_t)strlen(name), r, counts);
    if (cnt.n != o.t.size()) return SCS_EDEVICE;                                      // (the sizing pass' sink and the emit pass' must agree)
    *n_out = o.t.size();
    if (out) { if (o.t.size() > cap) return SCS_EOVERFLOW; memcpy(out, o.t.data(), o.t.size()); }
    return SCS_OK;
}

// host-only: one amplicon's line of the amplicon table through the functions its kernels run (amp_line_probe, scs_amp.h)
int scs_amplicon_line_probe(uint64_t frag_goff, uint32_t frag_len, int frag_strand, uint32_t semi_spos, uint32_t semi_len, const uint32_t* semi_errs, uint32_t n_semi_errs,
                            uint32_t full_spos, uint32_t full_len, const uint32_t* full_errs, uint32_t n_full_errs,
                            const char* genome, uint64_t genome_start, uint64_t genome_len, uint64_t rec_off, uint64_t rec_len, const char* rec_name,
                            uint32_t index, uint32_t reads, uint32_t semi, char* out, size_t cap, size_t* n_out) {
    if (!n_out) return SCS_EINVAL;
    std::string line;
    const int rc = amp_line_probe(frag_goff, frag_len, frag_strand, semi_spos, semi_len, semi_errs, n_semi_errs, full_spos, full_len, full_errs, n_full_errs,
                                  genome, genome_start, genome_len, rec_off, rec_len, rec_name, index, reads, semi, line);
    if (rc) return rc;
    *n_out = line.size();
    if (out) { if (line.size() > cap) return SCS_EOVERFLOW; memcpy(out, line.data(), line.size()); }
    return SCS_OK;
}

// host-only: the artefact table's body (flags & 1: behind its header) through the functions its kernels run (site_probe, scs_site.h)
int scs_artefact_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                       const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                       const uint64_t* rec_len, const char* const* rec_names, uint32_t n_rec, const char* genome, uint64_t genome_len,
                       uint32_t min_reads, int flags, char* out, size_t cap, size_t* n_out) {
    if (!n_out || !rec_names || !n_rec || (flags & ~1)) return SCS_EINVAL;
    std::vector<std::string> names;
    for (uint32_t r = 0; r < n_rec; ++r) { if (!rec_names[r]) return SCS_EINVAL; names.push_back(rec_names[r]); }
    std::string body;
    const int rc = site_probe(amp_start, amp_len, amp_reads, n_amp, ed_amp, ed_x, ed_alt, n_ed, rec_len, names, genome, genome_len, min_reads, body);
    if (rc) return rc;
    if (flags & 1) body = site_header(names, rec_len) + body;
    *n_out = body.size();
    if (out) { if (body.size() > cap) return SCS_EOVERFLOW; memcpy(out, body.data(), body.size()); }
    return SCS_OK;
}

// host-only: the reference table's body (flags & 1: behind its header) through the functions its kernels run (site_ref_probe, scs_site_ref.h)
int scs_artefact_ref_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                           const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                           const uint64_t* hap_len, uint32_t n_hap, const char* genome, uint64_t genome_len,
                           const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                           const uint64_t* ref_len, const char* const* ref_names, uint32_t n_ref,
                           uint32_t min_reads, uint64_t slab, int flags, char* out, size_t cap, size_t* n_out, uint64_t unlifted[2], int* lift_err) {
    if (!n_out || !ref_names || !n_ref || !ref_len || (flags & ~1) || !n_seg || !seg_hap_off || !seg_len || !seg_ref_pos || !seg_ref_rec || !seg_kind) return SCS_EINVAL;
    std::vector<std::string> names;
    for (uint32_t r = 0; r < n_ref; ++r) { if (!ref_names[r]) return SCS_EINVAL; names.push_back(ref_names[r]); }
    std::vector<LiftSeg> segs(n_seg);
    for (uint32_t i = 0; i < n_seg; ++i) segs[i] = LiftSeg{seg_hap_off[i], seg_len[i], seg_ref_pos[i], seg_ref_rec[i], seg_kind[i]};
    std::string body; uint64_t unl[2] = {0, 0};
    const int rc = site_ref_probe(amp_start, amp_len, amp_reads, n_amp, ed_amp, ed_x, ed_alt, n_ed, hap_len, n_hap, genome, genome_len, segs.data(), n_seg, ref_len, names,
                                  min_reads, slab ? slab : kSiteSlab, body, unl, lift_err);
    if (unlifted) { unlifted[0] = unl[0]; unlifted[1] = unl[1]; }
    if (rc) return rc;
    if (flags & 1) body = site_ref_header(names, ref_len, unl[0], unl[1]) + body;
    *n_out = body.size();
    if (out) { if (body.size() > cap) return SCS_EOVERFLOW; memcpy(out, body.data(), body.size()); }
    return SCS_OK;
}

// host-only: the expansion of the site support table on the reference and its gather through the functions the kernels run
// (support_ref_probe, scs_support_ref.h)
int scs_support_ref_probe(const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                          const uint64_t* hap_len, uint32_t n_hap, const uint64_t* ref_len, uint32_t n_ref, const uint64_t* x, uint64_t n_x, uint64_t chunk, const uint32_t* g_counts,
                          uint64_t* sp_pos, uint32_t* sp_pos_x, uint64_t cap, uint64_t* n_staged, uint32_t* ref_counts, int* why) {
    if (why) *why = 0;
    if (!n_staged || !n_seg || !seg_hap_off || !seg_len || !seg_ref_pos || !seg_ref_rec || !seg_kind) return SCS_EINVAL;
    std::vector<LiftSeg> segs(n_seg);
    for (uint32_t i = 0; i < n_seg; ++i) segs[i] = LiftSeg{seg_hap_off[i], seg_len[i], seg_ref_pos[i], seg_ref_rec[i], seg_kind[i]};
    std::vector<uint64_t> pos; std::vector<uint32_t> pos_x, rc;
    const int rv = support_ref_probe(segs.data(), n_seg, hap_len, n_hap, ref_len, n_ref, x, n_x, chunk ? chunk : ~0ull, g_counts, pos, pos_x, rc, why);
    if (rv) return rv;
    *n_staged = pos.size();
    if (pos.size() > cap) return SCS_EOVERFLOW;
    if (sp_pos && !pos.empty()) memcpy(sp_pos, pos.data(), pos.size() * 8);
    if (sp_pos_x && !pos.empty()) memcpy(sp_pos_x, pos_x.data(), pos.size() * 4);
    if (ref_counts && g_counts && !rc.empty()) memcpy(ref_counts, rc.data(), rc.size() * 4);
    return SCS_OK;
}
// host-only: the header of the site support table on the reference (site_ref_header with the three more lines)
int scs_support_ref_header_probe(const uint64_t* ref_len, const char* const* ref_names, uint32_t n_ref, uint64_t unl_entries, uint64_t unl_reads, char* out, size_t cap, size_t* n_out) {
    if (!n_out || !ref_names || !ref_len) return SCS_EINVAL;
    std::vector<std::string> names;
    for (uint32_t r = 0; r < n_ref; ++r) { if (!ref_names[r]) return SCS_EINVAL; names.push_back(ref_names[r]); }
    const std::string h = site_ref_header(names, ref_len, unl_entries, unl_reads, true);
    *n_out = h.size();
    if (out) { if (h.size() > cap) return SCS_EOVERFLOW; memcpy(out, h.data(), h.size()); }
    return SCS_OK;
}

int scs_predict_batch(scs_ctx* c, const uint8_t* windows, size_t n_reads, const uint64_t* uids, const uint32_t* attempts, const uint8_t* is_read1,
                      char* out_bases, char* out_quals, int32_t* out_len, int out_stride) {
    return guarded(c, [&] {
        if (!c->have_profile) throw ScsError(SCS_EINVAL, "scs_predict_batch: load a profile first");
        if (n_reads > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, "too many reads");
        hipStream_t s = c->stream; const uint32_t L = (uint32_t)c->prof.read_length, slot = ((L + 64 + 63) / 64) * 64, n = (uint32_t)n_reads;
        if (out_stride < (int)slot) throw ScsError(SCS_EINVAL, "out_stride must be >= " + std::to_string(slot));
        DevBuf dw, du, da, dr; dw.reserve(std::max<size_t>((size_t)n * L, 16), s); du.reserve(std::max<size_t>((size_t)n * 8, 16), s);
        da.reserve(std::max<size_t>((size_t)n * 4, 16), s); dr.reserve(std::max<size_t>(n, 16), s);
        HIP_OK(hipMemcpyAsync(dw.p, windows, (size_t)n * L, hipMemcpyHostToDevice, s)); HIP_OK(hipMemcpyAsync(du.p, uids, (size_t)n * 8, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(da.p, attempts, (size_t)n * 4, hipMemcpyHostToDevice, s)); HIP_OK(hipMemcpyAsync(dr.p, is_read1, n, hipMemcpyHostToDevice, s));
        c->slot_b.reserve((size_t)n * slot, s); c->slot_q.reserve((size_t)n * slot, s); c->lens.reserve(std::max<size_t>((size_t)n * 4, 16), s);
        launch_predict_windows(s, dw.as<uint8_t>(), n, du.as<uint64_t>(), da.as<uint32_t>(), dr.as<uint8_t>(), c->dtb, c->d_tables.as<DevTables>(), c->key, slot, c->slot_b.as<char>(),
                               c->slot_q.as<char>(), c->lens.as<uint32_t>(), c->flags.as<uint32_t>());
        std::vector<char> hb((size_t)n * slot), hq((size_t)n * slot); std::vector<uint32_t> hl(n);
        HIP_OK(hipMemcpyAsync(hb.data(), c->slot_b.p, hb.size(), hipMemcpyDeviceToHost, s)); HIP_OK(hipMemcpyAsync(hq.data(), c->slot_q.p, hq.size(), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(hl.data(), c->lens.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        check_flags(c);
        for (uint32_t i = 0; i < n; ++i) { out_len[i] = (int32_t)hl[i]; memcpy(out_bases + (size_t)i * out_stride, hb.data() + (size_t)i * slot, hl[i]); memcpy(out_quals + (size_t)i * out_stride, hq.data() + (size_t)i * slot, hl[i]); }
    });
}

int scs_philox_batch(scs_ctx* c, const uint32_t* ctr, size_t n, const uint32_t* key, uint32_t* out) {
    return guarded(c, [&] {
        hipStream_t s = c->stream; DevBuf a, b; a.reserve(std::max<size_t>(n * 16, 16), s); b.reserve(std::max<size_t>(n * 16, 16), s);
        HIP_OK(hipMemcpyAsync(a.p, ctr, n * 16, hipMemcpyHostToDevice, s));
        launch_philox(s, a.as<uint32_t>(), (uint32_t)n, RngKey{key[0], key[1]}, b.as<uint32_t>());
        HIP_OK(hipMemcpyAsync(out, b.p, n * 16, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
    });
}
int scs_detlog_batch(scs_ctx* c, const double* x, size_t n, double* out) {
    return guarded(c, [&] {
        hipStream_t s = c->stream; DevBuf a, b; a.reserve(std::max<size_t>(n * 8, 16), s); b.reserve(std::max<size_t>(n * 8, 16), s);
        HIP_OK(hipMemcpyAsync(a.p, x, n * 8, hipMemcpyHostToDevice, s));
        launch_detlog(s, a.as<double>(), (uint32_t)n, b.as<double>());
        HIP_OK(hipMemcpyAsync(out, b.p, n * 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
    });
}

// what staging left on the device for the resident stretch of the genome, copied back as it lies: no kernel runs, no state changes
int scs_download_genome(scs_ctx* c, uint64_t info[4], char* names, size_t names_cap, uint64_t* rec_lens, uint64_t rec_cap, uint8_t* codes,
                        uint64_t* gc_bits, uint64_t* n_bits, uint64_t* gc_pref, uint64_t* n_pref, uint64_t* gc_pair, uint32_t* g2, uint8_t* has_n) {
    return guarded(c, [&] {
        if (!info) throw ScsError(SCS_EINVAL, "scs_download_genome: null info");
        if (!c->have_genome) throw ScsError(SCS_EINVAL, "scs_download_genome: no genome loaded");
        if (has_n && !c->have_frags) throw ScsError(SCS_EINVAL, "scs_download_genome: has_n needs scs_create_frags first");
        std::string nm; for (auto& r : c->recs) { nm += r.name; nm += '\n'; }
        const uint64_t n = c->slice_len, nw = (n + 63) / 64;
        info[0] = c->slice_base; info[1] = n; info[2] = c->recs.size(); info[3] = nm.size();
        if ((names && names_cap < nm.size()) || (rec_lens && rec_cap < c->rec_len.size())) throw ScsError(SCS_EOVERFLOW, "scs_download_genome: names or rec_lens too small");
        if (names) memcpy(names, nm.data(), nm.size());
        if (rec_lens) std::copy(c->rec_len.begin(), c->rec_len.end(), rec_lens);
        hipStream_t s = c->stream;
        auto down = [&](void* dst, const void* src, size_t bytes) { if (dst && bytes) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s)); };
        down(codes, c->genome.p, n);
        down(gc_bits, c->gx_gc_bits.p, (nw + 1) * 8); down(n_bits, c->gx_n_bits.p, (nw + 1) * 8);
        down(gc_pref, c->gx_gc_pref.p, (nw + 1) * 8); down(n_pref, c->gx_n_pref.p, (nw + 1) * 8);
        down(gc_pair, c->gx_gc_pair.p, (nw + 1) * 16);
        down(g2, c->genome2.as<uint32_t>() + 16, nw * 16);                             // (behind the 64 bytes of slack in front: index_genome)
        down(has_n, c->df_hasn.p, c->f_len.size());
        HIP_OK(hipStreamSynchronize(s));
    });
}

int scs_fasta_probe(const char* path, int* n_records, uint64_t* total_bases, uint64_t* checksum, char* names_buf, size_t names_len, char* errbuf, size_t errlen) {
    if (!path) return SCS_EINVAL;
    std::vector<FastaRecord> recs;
    try { load_fasta(path, recs); }
    catch (const std::exception& e) { copy_err(errbuf, errlen, e.what()); return SCS_EIO; }
    uint64_t tot = 0, h = 1469598103934665603ull; std::string names;
    for (auto& r : recs) {
        tot += r.code.size(); names += r.name; names += '\n';
        for (uint8_t b : r.code) { h ^= (uint64_t)(b >= 'a' && b <= 'z' ? b - 32 : b); h *= 1099511628211ull; }
    }
    if (n_records) *n_records = (int)recs.size(); if (total_bases) *total_bases = tot; if (checksum) *checksum = h;
    if (names_buf && names_len) { strncpy(names_buf, names.c_str(), names_len - 1); names_buf[names_len - 1] = 0; }
    return SCS_OK;
}
int scs_devbuf_probe(int device, uint64_t first_bytes, uint64_t second_bytes, uint64_t* caps, int* in_place) {
    if (!caps) return SCS_EINVAL;
    try {
        HIP_OK(hipSetDevice(device));
        DevBuf b;
        b.reserve((size_t)first_bytes, nullptr); caps[0] = b.cap;
        const void* at = b.p;
        b.reserve((size_t)second_bytes, nullptr); caps[1] = b.cap;
        if (in_place) *in_place = b.p == at ? 1 : 0;
        return SCS_OK;
    } catch (const std::exception& e) { create_error() = e.what(); return SCS_EDEVICE; }
}
// host-only: the simuvars plan applied to the host copy of the reference, folded into a checksum of the FASTA text that
// scs_simuvars would write (test seam for the planner; the product builds the sequences on the device)
int scs_simuvars_probe(const char* ref_fasta, const char* snp_file, const char* var_file, int* n_records, uint64_t* total_bases, uint64_t* checksum, char* errbuf, size_t errlen) {
    if (!ref_fasta) return SCS_EINVAL;
    try {
        std::vector<FastaRecord> ref; load_fasta(ref_fasta, ref);
        std::vector<SvChrom> chroms; std::vector<uint8_t> flat;
        for (auto& r : ref) { chroms.push_back(SvChrom{r.name, (uint64_t)flat.size(), (uint64_t)r.code.size()}); flat.insert(flat.end(), r.code.begin(), r.code.end()); }
        SvPlan P; simuvars_plan(chroms, snp_file ? snp_file : "", var_file ? var_file : "", false, P);
        std::vector<uint8_t> out(P.total);
        for (const SvPiece& pc : P.pieces) for (uint32_t i = 0; i < pc.len; ++i) { uint8_t ch = pc.lit ? (uint8_t)P.literals[pc.src + i] : flat[pc.src + i]; out[pc.dst + i] = (uint8_t)(ch >= 'a' && ch <= 'z' ? ch - 32 : ch); }
        for (const SvSubst& sb : P.substs) out[sb.dst] = (uint8_t)sb.ch;
        uint64_t h = 1469598103934665603ull, off = 0;
        auto eat = [&](const char* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= (uint8_t)p[i]; h *= 1099511628211ull; } };
        for (size_t r = 0; r < P.rec_names.size(); ++r) {
            const std::string hd = ">" + P.rec_names[r] + "\n"; eat(hd.data(), hd.size());
            for (uint64_t x = 0; x < P.rec_lens[r]; x += 100) { eat((const char*)out.data() + off + x, (size_t)std::min<uint64_t>(100, P.rec_lens[r] - x)); eat("\n", 1); }
            off += P.rec_lens[r];
        }
        if (n_records) *n_records = (int)P.rec_names.size(); if (total_bases) *total_bases = P.total; if (checksum) *checksum = h;
        return SCS_OK;
    } catch (const std::exception& e) { copy_err(errbuf, errlen, e.what()); return SCS_EIO; }
}
// host-only test seam: the BGZF kernels' arithmetic run on the CPU ("thread" by "thread" over the same functions: scs_bgzf.hip)
int scs_bgzf_probe(const void* text, uint64_t nbytes, uint32_t lds_out_cap, void* out, uint64_t cap, uint64_t* n_out) {
    if ((!text && nbytes) || !n_out) return SCS_EINVAL;
    std::vector<uint8_t> z; bgzf_compress_host((const uint8_t*)text, nbytes, lds_out_cap ? lds_out_cap : BGZF_LDS_OUT, z);
    *n_out = z.size();
    if (out) { if (z.size() > cap) return SCS_EOVERFLOW; memcpy(out, z.data(), z.size()); }
    return SCS_OK;
}
// host-only test seam: the batches scs_yield_reads would cut `pairs` pairs into, and the order it would make them in (plan_batches)
int scs_batch_plan_probe(uint64_t pairs, uint32_t read_length, int to_sink, int writers, int regions, int batch_shift, uint64_t* batch, uint32_t* nbatch,
                         uint32_t* order, uint32_t* region_of, uint32_t cap) {
    if (!batch || !nbatch || batch_shift < 0 || batch_shift > 40) return SCS_EINVAL;
    const BatchPlan pl = plan_batches(pairs, read_length, to_sink != 0, writers, regions, batch_shift);
    *batch = pl.batch; *nbatch = pl.nbatch;
    if (!order && !region_of) return SCS_OK;
    if (pl.nbatch > cap) return SCS_EOVERFLOW;
    if (order) std::copy(pl.order.begin(), pl.order.end(), order);
    if (region_of) std::copy(pl.region_of.begin(), pl.region_of.end(), region_of);
    return SCS_OK;
}
namespace {
struct ProbeMem {                                         // plain hipMalloc blocks of a device probe, freed on every way out (no seam: not a DevBuf)
    std::vector<void*> blocks;
    void* get(size_t bytes) { void* p = nullptr; HIP_OK(hipMalloc(&p, std::max<size_t>((bytes + 15) & ~(size_t)15, 16))); blocks.push_back(p); return p; }
    ~ProbeMem() { for (void* p : blocks) (void)hipFree(p); }
};
constexpr size_t kProbeGuard = 64;                        // guard bytes on each side of a probe's output
constexpr int kProbeFill = 0xA5;
void probe_sync() {
    HIP_OK(hipDeviceSynchronize());
    const hipError_t le = take_launch_error();                                    // hipGetLastError + what the launchers noted
    if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("probe kernel failed: ") + hipGetErrorString(le));
}
}  // namespace
// device test seam: plan, scan and emit over a fresh text buffer, exactly the calls scs_reads.cpp makes per mate
int scs_bgzf_device_probe(int device, const void* text, uint64_t nbytes, uint32_t zbase, void* out, uint64_t cap, uint64_t* n_out, int* guards_ok) {
    if ((!text && nbytes) || (!out && nbytes) || !n_out || !guards_ok || zbase > 3 || bgzf_bound(nbytes) > 0xFFFFFFF0ull) return SCS_EINVAL;
    *n_out = 0; *guards_ok = 1;
    if (!nbytes) return SCS_OK;
    try {
        HIP_OK(hipSetDevice(device));
        ProbeMem mem;
        const uint32_t nblk = bgzf_blocks(nbytes);
        const size_t zcap = kProbeGuard + 4 + (size_t)bgzf_bound(nbytes) + kProbeGuard;   // [guard | zbase | the blocks, at most bgzf_bound | guard]
        char* d_text = (char*)mem.get(nbytes);
        uint8_t* d_plan = (uint8_t*)mem.get((size_t)nblk * BGZF_PLAN_BYTES);
        uint32_t* d_sizes = (uint32_t*)mem.get(((size_t)nblk + 2) * 4); uint32_t* d_offs = (uint32_t*)mem.get(((size_t)nblk + 2) * 4);
        uint32_t* d_crc = (uint32_t*)mem.get(512 * 4);
        char* d_z = (char*)mem.get(zcap);
        uint32_t tabs[512]; bgzf_host_tables(tabs, tabs + 256);
        HIP_OK(hipMemcpy(d_text, text, nbytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_crc, tabs, sizeof tabs, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_sizes, 0, ((size_t)nblk + 2) * 4));
        HIP_OK(hipMemset(d_z, kProbeFill, zcap));
        HIP_OK(hipDeviceSynchronize());
        launch_bgzf_plan(nullptr, d_text, nbytes, d_plan, d_sizes);
        exclusive_scan_u32(nullptr, d_sizes, d_offs, nblk, nullptr, 0);
        launch_bgzf_emit(nullptr, d_text, nbytes, d_plan, d_sizes, d_offs, d_crc, d_crc + 256, d_z + kProbeGuard, zbase);
        probe_sync();
        uint32_t total = 0;
        HIP_OK(hipMemcpy(&total, d_offs + nblk, 4, hipMemcpyDeviceToHost));
        *n_out = total;
        if (total > bgzf_bound(nbytes)) throw ScsError(SCS_EDEVICE, "BGZF probe: the blocks' total exceeds bgzf_bound");
        std::vector<uint8_t> z(zcap);
        HIP_OK(hipMemcpy(z.data(), d_z, zcap, hipMemcpyDeviceToHost));
        const size_t lo = kProbeGuard + zbase, hi = lo + total;                       // everything outside [lo, hi) is guard
        for (size_t i = 0; i < zcap; ++i) if ((i < lo || i >= hi) && z[i] != (uint8_t)kProbeFill) { *guards_ok = 0; break; }
        if (total > cap) return SCS_EOVERFLOW;
        memcpy(out, z.data() + lo, total);
        return SCS_OK;
    } catch (const std::exception& e) { create_error() = e.what(); return SCS_EDEVICE; }
}
// device test seam: the exclusive scans of scs_k_misc.hip over uploaded arrays
int scs_scan_probe(int device, const uint32_t* in0, uint64_t n0, const uint32_t* in1, uint64_t n1, uint32_t* out0, uint32_t* out1) {
    if ((!in0 && n0) || !out0 || (in1 && !out1) || (!in1 && n1) || n0 > 0x7FFFFFF0ull || n1 > 0x7FFFFFF0ull) return SCS_EINVAL;
    try {
        HIP_OK(hipSetDevice(device));
        ProbeMem mem;
        const uint32_t* hin[2] = {in0, in1}; const uint64_t n[2] = {n0, n1}; uint32_t* hout[2] = {out0, out1};
        uint32_t* din[2] = {nullptr, nullptr}; uint32_t* dout[2] = {nullptr, nullptr};
        const int arrays = in1 ? 2 : 1;
        const size_t guard_words = kProbeGuard / 4;
        for (int a = 0; a < arrays; ++a) {
            din[a] = (uint32_t*)mem.get((n[a] + 2) * 4); dout[a] = (uint32_t*)mem.get((n[a] + 1 + guard_words) * 4);
            HIP_OK(hipMemset(din[a], kProbeFill, (n[a] + 2) * 4));                    // in[n] is readable and must be ignored: it is not zero
            if (n[a]) HIP_OK(hipMemcpy(din[a], hin[a], n[a] * 4, hipMemcpyHostToDevice));
            HIP_OK(hipMemset(dout[a], kProbeFill, (n[a] + 1 + guard_words) * 4));
        }
        const size_t tb = scan_temp_bytes((size_t)std::max(n0, n1));
        void* temp = (char*)mem.get(tb);
        HIP_OK(hipDeviceSynchronize());
        if (in1) exclusive_scan_u32_pair(nullptr, din[0], dout[0], n0, din[1], dout[1], n1, temp, tb);
        else exclusive_scan_u32(nullptr, din[0], dout[0], n0, temp, tb);
        probe_sync();
        for (int a = 0; a < arrays; ++a) {
            std::vector<uint32_t> h(n[a] + 1 + guard_words);
            HIP_OK(hipMemcpy(h.data(), dout[a], h.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = n[a] + 1; i < h.size(); ++i) if (h[i] != 0xA5A5A5A5u) throw ScsError(SCS_EDEVICE, "scan probe: a scan wrote behind out[n]");
            memcpy(hout[a], h.data(), (n[a] + 1) * 4);
        }
        return SCS_OK;
    } catch (const std::exception& e) { create_error() = e.what(); return SCS_EDEVICE; }
}
// host-only test seam: the read allocation's plan of shard `rank` (alloc_plan_build, scs_alloc_plan.h: what do_allocate runs) over the
// table counts[r * 40 + slot], R shards.  scalars: total, chunks of the job, n_interior, n_boundary, n_ranges, n_gseg, this shard's
// amplicons, the scratch doubles reserved for that many chunks.  The arrays (all NULL: the scalars alone; else each at least as long
// as the scalars say): ranges as q0, c0, local0; bchunks as c, n, owner; gsegs as go, lo, n, owner, slot; my_seg[40] as go, lo, n, order
int scs_alloc_plan_probe(const uint64_t* counts, int R, int rank, uint64_t scalars[8], uint32_t* ranges, uint32_t* bchunks, uint64_t* gsegs, uint64_t* my_seg) {
    if (!counts || !scalars || R < 1 || R > 4096 || rank < 0 || rank >= R) return SCS_EINVAL;
    AllocHostPlan P;
    if (!alloc_plan_build(counts, R, rank, P)) return SCS_EOVERFLOW;
    scalars[0] = P.total; scalars[1] = P.nch; scalars[2] = P.n_interior; scalars[3] = P.bch.size(); scalars[4] = P.rng.size(); scalars[5] = P.gseg.size();
    scalars[6] = P.ac; scalars[7] = alloc_tree_scratch(P.nch);
    if (ranges) for (size_t i = 0; i < P.rng.size(); ++i) { ranges[3 * i] = P.rng[i].q0; ranges[3 * i + 1] = P.rng[i].c0; ranges[3 * i + 2] = P.rng[i].local0; }
    if (bchunks) for (size_t i = 0; i < P.bch.size(); ++i) { bchunks[3 * i] = P.bch[i].c; bchunks[3 * i + 1] = P.bch[i].n; bchunks[3 * i + 2] = P.bch[i].owner; }
    if (gsegs) for (size_t i = 0; i < P.gseg.size(); ++i) { const AllocGSeg& g = P.gseg[i]; gsegs[5 * i] = g.go; gsegs[5 * i + 1] = g.lo; gsegs[5 * i + 2] = g.n; gsegs[5 * i + 3] = g.owner; gsegs[5 * i + 4] = g.slot; }
    if (my_seg) for (int sl = 0; sl < ALLOC_SLOTS; ++sl) { const AllocMySeg& m = P.my_seg[sl]; my_seg[4 * sl] = m.go; my_seg[4 * sl + 1] = m.lo; my_seg[4 * sl + 2] = m.n; my_seg[4 * sl + 3] = m.order; }
    return SCS_OK;
}
// device test seam: the allocation's fixed-shape sums over n uploaded doubles, with the scratch do_allocate reserves for n chunk
// partials (alloc_tree_scratch) and guards behind it and behind the output.  which = 0: launch_tree_sum, one double out;
// which = 1: launch_scan_all, n doubles out
int scs_alloc_sums_probe(int device, const double* in, uint64_t n, int which, double* out) {
    if (!in || !out || !n || n > 0x7FFFFFF0ull || (which != 0 && which != 1)) return SCS_EINVAL;
    try {
        HIP_OK(hipSetDevice(device));
        ProbeMem mem;
        const size_t n_out = which ? (size_t)n : 1, n_scr = alloc_tree_scratch((size_t)n), guard = kProbeGuard / 8;
        double* d_in = (double*)mem.get((size_t)n * 8); double* d_out = (double*)mem.get((n_out + guard) * 8); double* d_scr = (double*)mem.get((n_scr + guard) * 8);
        HIP_OK(hipMemcpy(d_in, in, (size_t)n * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, kProbeFill, (n_out + guard) * 8)); HIP_OK(hipMemset(d_scr, kProbeFill, (n_scr + guard) * 8));
        HIP_OK(hipDeviceSynchronize());
        if (which) launch_scan_all(nullptr, d_in, (uint32_t)n, d_out, d_scr);
        else launch_tree_sum(nullptr, d_in, (uint32_t)n, d_scr, d_out);
        probe_sync();
        std::vector<uint64_t> h(n_out + guard), g(guard);
        HIP_OK(hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(g.data(), d_scr + n_scr, guard * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < guard; ++i) if (h[n_out + i] != 0xA5A5A5A5A5A5A5A5ull || g[i] != 0xA5A5A5A5A5A5A5A5ull) throw ScsError(SCS_EDEVICE, "allocation sums probe: a kernel wrote behind its output or behind the scratch");
        memcpy(out, h.data(), n_out * 8);
        return SCS_OK;
    } catch (const std::exception& e) { create_error() = e.what(); return SCS_EDEVICE; }
}
// device test seam: the allocation (allocate_weighted: everything of scs_allocate_reads behind the weights) over n_local given weights as
// this shard's list, cut into segments of seg_counts[slot] amplicons, on a ctx that was never amplified -- its layout, seed, shard rank
// and collectives are the job's.  rn_out[n_local], pair_off_out[n_local + 1].  The ctx is left as it was: not allocated
int scs_alloc_probe(scs_ctx* c, const double* w_local, uint64_t n_local, const uint32_t* seg_counts, uint64_t reads, uint32_t* rn_out, uint32_t* pair_off_out) {
    return guarded(c, [&] {
        if (!seg_counts || !pair_off_out || (n_local && (!w_local || !rn_out)) || n_local > 0xFFFFFFF0ull || reads > 0x7FFFFFFFFFFFFFFFull) throw ScsError(SCS_EINVAL, "scs_alloc_probe: bad argument");
        if (c->amplified || c->allocated) throw ScsError(SCS_EINVAL, "scs_alloc_probe: the ctx holds a job");
        uint64_t sum = 0; for (int sl = 0; sl < ALLOC_SLOTS; ++sl) sum += seg_counts[sl];
        if (sum != n_local) throw ScsError(SCS_EINVAL, "scs_alloc_probe: the segments do not add up to n_local");
        hipStream_t s = c->stream; const uint32_t ac = (uint32_t)n_local;
        struct Keep {                                                              // what allocate_weighted leaves on the ctx, put back on every way out
            scs_ctx* c; std::vector<scs_ctx::Seg> segs; SegMap gmap; uint64_t pairs; uint32_t seg_lo[ALLOC_SLOTS + 1];
            explicit Keep(scs_ctx* x) : c(x), segs(x->full_segs), gmap(x->gmap), pairs(x->n_pairs_planned) { memcpy(seg_lo, x->seg_lo, sizeof seg_lo); }
            ~Keep() { c->full_segs.swap(segs); c->gmap = gmap; c->n_pairs_planned = pairs; memcpy(c->seg_lo, seg_lo, sizeof seg_lo); }
        } keep(c);
        c->full_segs.clear();
        for (int sl = 0; sl < ALLOC_SLOTS; ++sl) if (seg_counts[sl]) c->full_segs.push_back(scs_ctx::Seg{sl / 8, 7 - sl % 8, seg_counts[sl]});
        c->weights.reserve(std::max<size_t>((size_t)ac * 8, 16), s);
        c->read_numbers.reserve(((size_t)ac + 1) * 4, s); c->pair_off.reserve(((size_t)ac + 1) * 4, s);
        if (ac) HIP_OK(hipMemcpyAsync(c->weights.p, w_local, (size_t)ac * 8, hipMemcpyHostToDevice, s));
        allocate_weighted(c, reads, ac);
        if (ac) HIP_OK(hipMemcpyAsync(rn_out, c->read_numbers.p, (size_t)ac * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(pair_off_out, c->pair_off.p, ((size_t)ac + 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        const hipError_t le = take_launch_error();
        if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("scs_alloc_probe: kernel launch failed: ") + hipGetErrorString(le));
    });
}
int scs_profile_open(const char* path, int paired, int isize, void** handle, char* errbuf, size_t errlen) {
    if (!path || !handle) return SCS_EINVAL;
    ProfileTables* T = new ProfileTables;
    try { load_profile(path, paired != 0, isize, *T); }
    catch (const std::exception& e) { copy_err(errbuf, errlen, e.what()); delete T; *handle = nullptr; return SCS_EIO; }
    *handle = T; return SCS_OK;
}
int scs_profile_table(void* handle, int which, const uint32_t** thr, const double** cdf, size_t* n) {
    if (!handle) return SCS_EINVAL;
    ProfileTables* T = (ProfileTables*)handle;
    const std::vector<uint32_t>* t; const std::vector<double>* d;
    switch (which) {
        case 0: t = &T->subs1_t; d = &T->subs1; break; case 1: t = &T->subs2_t; d = &T->subs2; break; case 2: t = &T->qual_t; d = &T->qual; break;
        case 3: t = &T->ins_t; d = &T->ins_cdf; break; case 4: t = &T->del_t; d = &T->del_cdf; break; case 5: t = &T->isize_t; d = &T->isize_cdf; break;
        case 6: if (thr) *thr = T->qual_alias.data(); if (cdf) *cdf = nullptr; if (n) *n = T->qual_alias.size(); return SCS_OK;   // alias quality rows
        default: return SCS_EINVAL;
    }
    if (thr) *thr = t->data(); if (cdf) *cdf = d->data(); if (n) *n = t->size();
    return SCS_OK;
}
int scs_profile_scalars(void* handle, double* out) {
    if (!handle || !out) return SCS_EINVAL;
    ProfileTables* T = (ProfileTables*)handle;
    out[0] = T->read_length; out[1] = T->bins; out[2] = T->t_insert; out[3] = T->t_delete; out[4] = T->isize_min; out[5] = T->have_cdf2; out[6] = T->insert_rate; out[7] = T->del_rate;
    out[8] = T->t_indel; out[9] = T->qual_k;
    return SCS_OK;
}
void scs_profile_close(void* handle) { delete (ProfileTables*)handle; }

// what this library's owning handles (scs_ctx.h) hold right now, in the whole process: DevBuf bytes, streams, events, pinned bytes
int scs_live_resources(uint64_t out[4]) {
    if (!out) return SCS_EINVAL;
    const std::atomic<uint64_t>* n[4] = {&census().dev_bytes, &census().streams, &census().events, &census().pinned_bytes};
    for (int i = 0; i < 4; ++i) out[i] = n[i]->load(std::memory_order_relaxed);
    return SCS_OK;
}

}  // extern "C"
