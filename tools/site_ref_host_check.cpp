// site_ref_host_check.cpp -- the host code of the artefact table on the original reference (scs_site_ref.h: site_ref_probe and
// everything it runs -- the segment cursor, the pieces, the keys, the cover count) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on a CPU box (tools/site_ref_host_check.py builds it, replays the case table of
// tests/test_artefacts_ref_host.py through it and compares every body with the restatement's).  No GPU, no HIP.
// Input (stdin), per case:
//   case <min_reads> <slab> <expected return code> <expected lift_err> <unlifted entries> <unlifted reads> <genome>
//        <n_hap> <length> ... <n_ref> <name> <length> ... <n_seg> <hap_off> <len> <ref_pos> <ref_rec> <kind> ...
//        <n_amp> <start> <len> <reads> ... <n_ed> <amplicon> <staged index> <alt> ... <lines>
//   followed by the <lines> expected lines of the body (when the return code is 0).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_site_ref.h"

int main() {
    std::string ln; int n_cases = 0, bad = 0;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string kind; in >> kind;
        if (kind != "case") continue;
        uint32_t min_reads; uint64_t slab, want_unl[2], n_amp, n_ed; int want_rc, want_err; size_t lines, n_hap, n_ref, n_seg; std::string genome;
        in >> min_reads >> slab >> want_rc >> want_err >> want_unl[0] >> want_unl[1] >> genome;
        // every array in a heap block of exactly its size: a read outside it is the sanitizer's to report
        in >> n_hap; std::vector<uint64_t> hap_len(n_hap); for (auto& v : hap_len) in >> v;
        in >> n_ref; std::vector<std::string> names(n_ref); std::vector<uint64_t> ref_len(n_ref); for (size_t r = 0; r < n_ref; ++r) in >> names[r] >> ref_len[r];
        in >> n_seg; std::vector<scs::LiftSeg> segs(n_seg); for (auto& s : segs) in >> s.hap_off >> s.len >> s.ref_pos >> s.ref_rec >> s.kind;
        in >> n_amp; std::vector<uint64_t> st(n_amp); std::vector<uint32_t> len(n_amp), reads(n_amp);
        for (uint64_t a = 0; a < n_amp; ++a) in >> st[a] >> len[a] >> reads[a];
        in >> n_ed; std::vector<uint32_t> ea(n_ed); std::vector<uint64_t> ex(n_ed); std::vector<uint8_t> eb(n_ed);
        for (uint64_t e = 0; e < n_ed; ++e) { unsigned b; in >> ea[e] >> ex[e] >> b; eb[e] = (uint8_t)b; }
        in >> lines;
        std::vector<char> g(genome.begin(), genome.end());
        std::string body, want; uint64_t unl[2] = {0, 0}; int err = 0;
        const int rc = scs::site_ref_probe(st.data(), len.data(), reads.data(), n_amp, ea.data(), ex.data(), eb.data(), n_ed, hap_len.data(), (uint32_t)n_hap, g.data(), g.size(),
                                           segs.data(), (uint32_t)n_seg, ref_len.data(), names, min_reads, slab, body, unl, &err);
        if (want_rc == 0) for (size_t k = 0; k < lines; ++k) { std::getline(std::cin, ln); want += ln + "\n"; }
        ++n_cases;
        if (rc != want_rc || err != want_err || (rc == 0 && (body != want || unl[0] != want_unl[0] || unl[1] != want_unl[1]))) {
            ++bad; fprintf(stderr, "case %d: rc %d (want %d), lift_err %d (want %d), unlifted %llu %llu\n got  %s want %s", n_cases, rc, want_rc, err, want_err,
                           (unsigned long long)unl[0], (unsigned long long)unl[1], body.c_str(), want.c_str());
        }
    }
    printf("%d cases, %d wrong\n", n_cases, bad);
    return bad || !n_cases ? 1 : 0;
}
