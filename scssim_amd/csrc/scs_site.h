// scs_site.h -- one line of the artefact table (scs_write_artefacts / scs_artefact_sites): the edits of the
// full amplicons (amp_edits, scs_amp.h) grouped by genome site.  A site is (genome index, alternate base); per site NA / NR count
// the amplicons that carry the base and their reads, TA / TR the amplicons whose interval contains the index and theirs.  One
// definition for the device passes (scs_k_sites.hip: the sort keys, the run heads, the cover count, the line) and the host probe
// (scs_artefact_probe), so the test seam runs the code the kernels run -- with std::sort where the device has the radix sort.
#pragma once
#include <stdint.h>
#include "scs_common.h"
#include "scs_truth.h"
#include "scs_amp.h"
#include <algorithm>
#include <string>
#include <vector>

namespace scs {

// the sort key of an edit entry: ascending keys are ascending (genome index, alternate base A < C < G < T)
SCS_HD uint64_t site_key(uint64_t x, uint32_t alt) { return (x << 2) | (uint64_t)(alt & 3u); }
SCS_HD uint64_t site_key_x(uint64_t key) { return key >> 2; }
SCS_HD uint32_t site_key_alt(uint64_t key) { return (uint32_t)(key & 3u); }
// bits of a key over a genome of `bases` indices (the radix sort's end_bit); `extra` = 2 for keys, 0 for plain indices up to `bases`
inline unsigned site_bits(uint64_t bases, unsigned extra) { unsigned b = 1; while (b < 62 && (bases >> b)) ++b; return b + extra; }

// entry i of the sorted keys opens a run (a site)
SCS_HD bool site_head(const uint64_t* keys, uint64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

// how many of the n ascending values are <= x
SCS_HD uint64_t site_rank_le(const uint64_t* v, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (v[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

// one site.  pos: 0-based record coordinate; ref 0..4, alt 0..3
struct SiteRec { uint64_t pos, nr, tr; uint32_t rec, na, ta; uint8_t ref, alt, pad[2]; };

// Over the run that opens at entry i of the sorted (key, reads) pairs: NA and NR from the run; TA = #(starts <= x) - #(ends <= x)
// over the ascending starts and (exclusive) ends of the amplicons, TR the difference of the two prefix sums of their reads at
// those ranks (ps_*[k] = reads of the first k).  false: the counts contradict each other (NA > TA or NR > TR): never a wrong line
SCS_HD bool site_make(const uint64_t* keys, const uint32_t* reads, uint64_t n, uint64_t i, const uint64_t* starts, const uint64_t* ps_start,
                      const uint64_t* ends, const uint64_t* ps_end, uint64_t m, const uint64_t* rec_off, uint32_t n_rec, uint32_t ref, SiteRec& r) {
    const uint64_t key = keys[i], x = site_key_x(key);
    uint32_t na = 0; uint64_t nr = 0;
    for (uint64_t j = i; j < n && keys[j] == key; ++j) { ++na; nr += reads[j]; }
    const uint64_t rs = site_rank_le(starts, m, x), re = site_rank_le(ends, m, x);
    r.rec = rec_of(rec_off, n_rec, x); r.pos = x - rec_off[r.rec]; r.ref = (uint8_t)ref; r.alt = (uint8_t)site_key_alt(key); r.pad[0] = r.pad[1] = 0;
    r.na = na; r.nr = nr; r.ta = (uint32_t)(rs - re); r.tr = ps_start[rs] - ps_end[re];
    return rs >= re && rs - re >= na && ps_start[rs] >= ps_end[re] && r.tr >= nr && x < rec_off[n_rec];
}

// "NAME\tPOS\t.\tR\tA\t.\t.\tNA=..;TA=..;NR=..;TR=..\n" through o.put(char); POS = record coordinate + 1 (VCF 4.2).  cnt (the site
// support table; else NULL): the six read counters of the site's coordinate -- A, C, G, T, other, deleted --
// which add ";DP=..;AD=ref,alt;DL=.." to INFO: DP their first five, AD the classes of REF (N: class 4) and of ALT, DL the sixth
template <class Out>
SCS_HD void site_line(Out& o, const char* name, uint32_t name_len, const SiteRec& r, const uint32_t* cnt = nullptr) {
    for (uint32_t i = 0; i < name_len; ++i) o.put(name[i]);
    o.put('\t'); truth_num(o, r.pos + 1); o.put('\t'); o.put('.'); o.put('\t'); o.put(amp_letter(r.ref)); o.put('\t'); o.put(amp_letter(r.alt));
    o.put('\t'); o.put('.'); o.put('\t'); o.put('.'); o.put('\t');
    o.put('N'); o.put('A'); o.put('='); truth_num(o, r.na); o.put(';'); o.put('T'); o.put('A'); o.put('='); truth_num(o, r.ta); o.put(';');
    o.put('N'); o.put('R'); o.put('='); truth_num(o, r.nr); o.put(';'); o.put('T'); o.put('R'); o.put('='); truth_num(o, r.tr);
    if (cnt) {
        const uint64_t dp = (uint64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4];
        o.put(';'); o.put('D'); o.put('P'); o.put('='); truth_num(o, dp);
        o.put(';'); o.put('A'); o.put('D'); o.put('='); truth_num(o, cnt[r.ref < 4u ? r.ref : 4u]); o.put(','); truth_num(o, cnt[r.alt & 3u]);
        o.put(';'); o.put('D'); o.put('L'); o.put('='); truth_num(o, cnt[5]);
    }
    o.put('\n');
}

// ---- host-only
// the three ##INFO lines both site support tables (DESIGN.md sections 15 and 19) add behind the artefact table's four
#define SITE_SUPPORT_INFO "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"reads of the job with a base aligned at the site\">\n" \
                          "##INFO=<ID=AD,Number=2,Type=Integer,Description=\"reads that show the reference base, reads that show the alternate base\">\n" \
                          "##INFO=<ID=DL,Number=1,Type=Integer,Description=\"reads whose alignment deletes the site\">\n"
// the file's header: one contig line per staged record, in staging order (support: the site support table's, three more INFO lines)
inline std::string site_header(const std::vector<std::string>& names, const uint64_t* rec_len, bool support = false) {
    std::string h = "##fileformat=VCFv4.2\n##source=scssim\n";
    for (size_t r = 0; r < names.size(); ++r) h += "##contig=<ID=" + names[r] + ",length=" + std::to_string(rec_len[r]) + ">\n";
    h += "##INFO=<ID=NA,Number=1,Type=Integer,Description=\"full amplicons that carry the alternate base\">\n"
         "##INFO=<ID=TA,Number=1,Type=Integer,Description=\"full amplicons that cover the site\">\n"
         "##INFO=<ID=NR,Number=1,Type=Integer,Description=\"reads allotted to the NA amplicons\">\n"
         "##INFO=<ID=TR,Number=1,Type=Integer,Description=\"reads allotted to the TA amplicons\">\n";
    if (support) h += SITE_SUPPORT_INFO;                   // the site support table's three (scs_write_site_support)
    h += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    return h;
}

// The table's body from amplicon intervals (global start, length, reads) and edit entries (amplicon, global index, alternate base)
// through the functions above (scs_artefact_probe; no GPU, no ctx).  genome: the bases of every record, concatenated (any case;
// anything but ACGT is N).  SCS_EINVAL: an amplicon outside its record, an edit outside its amplicon, a base that is no code 0..3,
// records that do not add up to the genome; SCS_EDEVICE: the counting sink and the writing sink disagree, or site_make refuses
inline int site_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                      const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                      const uint64_t* rec_len, const std::vector<std::string>& names, const char* genome, uint64_t genome_len,
                      uint32_t min_reads, std::string& body) {
    const uint32_t n_rec = (uint32_t)names.size();
    if (!n_rec || !rec_len || !genome || (n_amp && (!amp_start || !amp_len || !amp_reads)) || (n_ed && (!ed_amp || !ed_x || !ed_alt))) return SCS_EINVAL;
    std::vector<uint64_t> rec_off(n_rec + 1, 0);
    for (uint32_t r = 0; r < n_rec; ++r) rec_off[r + 1] = rec_off[r] + rec_len[r];
    if (rec_off[n_rec] != genome_len || genome_len >> 60) return SCS_EINVAL;
    for (uint64_t a = 0; a < n_amp; ++a) {
        if (!amp_len[a] || amp_start[a] >= genome_len || amp_start[a] + amp_len[a] > genome_len) return SCS_EINVAL;
        const uint32_t r = rec_of(rec_off.data(), n_rec, amp_start[a]);
        if (amp_start[a] + amp_len[a] > rec_off[r + 1]) return SCS_EINVAL;       // a fragment never straddles records
    }
    std::vector<std::pair<uint64_t, uint32_t>> ent(n_ed), st(n_amp), en(n_amp);
    for (uint64_t e = 0; e < n_ed; ++e) {
        const uint32_t a = ed_amp[e];
        if (a >= n_amp || ed_alt[e] > 3u || ed_x[e] < amp_start[a] || ed_x[e] >= amp_start[a] + amp_len[a]) return SCS_EINVAL;
        ent[e] = {site_key(ed_x[e], ed_alt[e]), amp_reads[a]};
    }
    for (uint64_t a = 0; a < n_amp; ++a) { st[a] = {amp_start[a], amp_reads[a]}; en[a] = {amp_start[a] + amp_len[a], amp_reads[a]}; }
    auto by_key = [](const std::pair<uint64_t, uint32_t>& p, const std::pair<uint64_t, uint32_t>& q) { return p.first < q.first; };
    std::sort(ent.begin(), ent.end(), by_key); std::sort(st.begin(), st.end(), by_key); std::sort(en.begin(), en.end(), by_key);
    std::vector<uint64_t> keys(n_ed + 1, 0), starts(n_amp + 1, 0), ends(n_amp + 1, 0), ps_start(n_amp + 1, 0), ps_end(n_amp + 1, 0); std::vector<uint32_t> reads(n_ed + 1, 0);
    for (uint64_t e = 0; e < n_ed; ++e) { keys[e] = ent[e].first; reads[e] = ent[e].second; }
    for (uint64_t a = 0; a < n_amp; ++a) { starts[a] = st[a].first; ends[a] = en[a].first; ps_start[a + 1] = ps_start[a] + st[a].second; ps_end[a + 1] = ps_end[a] + en[a].second; }
    struct StrOut { std::string* t; void put(char ch) { t->push_back(ch); } } o{&body};
    body.clear();
    uint64_t counted = 0;
    for (uint64_t i = 0; i < n_ed; ++i) {
        if (!site_head(keys.data(), i)) continue;
        const char ch = genome[site_key_x(keys[i])];
        const uint32_t ref = ch == 'A' || ch == 'a' ? 0u : ch == 'C' || ch == 'c' ? 1u : ch == 'G' || ch == 'g' ? 2u : ch == 'T' || ch == 't' ? 3u : 4u;
        SiteRec r;
        if (!site_make(keys.data(), reads.data(), n_ed, i, starts.data(), ps_start.data(), ends.data(), ps_end.data(), n_amp, rec_off.data(), n_rec, ref, r)) return SCS_EDEVICE;
        if (r.nr < min_reads) continue;
        TruthCount cnt; site_line(cnt, names[r.rec].data(), (uint32_t)names[r.rec].size(), r); counted += cnt.n;
        site_line(o, names[r.rec].data(), (uint32_t)names[r.rec].size(), r);
    }
    return counted == body.size() ? SCS_OK : SCS_EDEVICE;   // (the sizing pass' sink and the emit pass' must agree)
}

}  // namespace scs
