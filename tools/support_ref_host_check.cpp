// support_ref_host_check.cpp -- the host code of the site support table on the original reference (scs_support_ref.h:
// support_ref_probe and everything it runs -- the range of a segment, the output slots, the gather) as a stand-alone program, to be
// built with -fsanitize=address,undefined and run on a CPU box (tools/support_ref_host_check.py builds it, replays the case table
// of tests/test_support_ref_host.py through it and compares every array with the restatement's).  No GPU, no HIP.
// Input (stdin), whitespace-separated, per case:
//   case <chunk> <expected return code> <expected why> <n_hap> <length> ... <n_ref> <length> ... <n_seg> <hap_off> <len> <ref_pos>
//        <ref_rec> <kind> ... <n_x> <x> ... <counters: 0 | 1> [6 counters per staged index] <n_staged> [<staged position> <index of
//        its x> ...] [6 sums per x]
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_support_ref.h"

int main() {
    std::string kind; int n_cases = 0, bad = 0;
    while (std::cin >> kind) {
        if (kind != "case") { fprintf(stderr, "not a case: %s\n", kind.c_str()); return 1; }
        uint64_t chunk, n_x, n_staged; int want_rc, want_why, with_counts; size_t n_hap, n_ref, n_seg;
        std::cin >> chunk >> want_rc >> want_why;
        // every array in a heap block of exactly its size: a read outside it is the sanitizer's to report
        std::cin >> n_hap; std::vector<uint64_t> hap_len(n_hap); for (auto& v : hap_len) std::cin >> v;
        std::cin >> n_ref; std::vector<uint64_t> ref_len(n_ref); for (auto& v : ref_len) std::cin >> v;
        std::cin >> n_seg; std::vector<scs::LiftSeg> segs(n_seg); for (auto& s : segs) std::cin >> s.hap_off >> s.len >> s.ref_pos >> s.ref_rec >> s.kind;
        std::cin >> n_x; std::vector<uint64_t> x(n_x); for (auto& v : x) std::cin >> v;
        uint64_t total = 0; for (uint64_t l : hap_len) total += l;
        std::cin >> with_counts; std::vector<uint32_t> g_cnt(with_counts ? 6 * total : 0); for (auto& v : g_cnt) std::cin >> v;
        std::cin >> n_staged; std::vector<uint64_t> want_pos(n_staged); std::vector<uint32_t> want_px(n_staged), want_sum(with_counts && want_rc == 0 ? 6 * n_x : 0);
        for (uint64_t t = 0; t < n_staged; ++t) std::cin >> want_pos[t] >> want_px[t];
        for (auto& v : want_sum) std::cin >> v;
        std::vector<uint64_t> pos; std::vector<uint32_t> px, sum; int why = 0;
        const int rc = scs::support_ref_probe(segs.data(), (uint32_t)n_seg, hap_len.data(), (uint32_t)n_hap, ref_len.data(), (uint32_t)n_ref, x.data(), n_x, chunk ? chunk : ~0ull,
                                              with_counts ? g_cnt.data() : nullptr, pos, px, sum, &why);
        ++n_cases;
        if (rc != want_rc || why != want_why || (rc == 0 && (pos != want_pos || px != want_px || (with_counts && sum != want_sum)))) {
            ++bad; fprintf(stderr, "case %d: rc %d (want %d), why %d (want %d), %zu staged positions (want %zu)\n", n_cases, rc, want_rc, why, want_why, pos.size(), want_pos.size());
        }
    }
    printf("%d cases, %d wrong\n", n_cases, bad);
    return bad || !n_cases ? 1 : 0;
}
