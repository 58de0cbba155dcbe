// site_host_check.cpp -- the artefact table's host code (scs_site.h: site_probe and everything it runs) as a stand-alone program,
// to be built with -fsanitize=address,undefined and run on a CPU box (tools/site_host_check.py builds it, replays the case table
// of tests/test_artefacts_host.py through it and compares every body with the restatement's).  No GPU, no HIP.
// Input (stdin):  genome <bases>  and  records <n> <name> <length> ...  once, then per case
//   case <min_reads> <expected return code> <n_amp> <start> <len> <reads> ... <n_ed> <amplicon> <genome index> <alt> ... <lines>
//   followed by the <lines> expected lines of the body (when the return code is 0).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_site.h"

int main() {
    std::string genome, ln; std::vector<std::string> names; std::vector<uint64_t> rec_len; int n_cases = 0, bad = 0;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string kind; in >> kind;
        if (kind == "genome") { in >> genome; continue; }
        if (kind == "records") { size_t n; in >> n; names.resize(n); rec_len.resize(n); for (size_t r = 0; r < n; ++r) in >> names[r] >> rec_len[r]; continue; }
        if (kind != "case") continue;
        uint32_t min_reads; int want_rc; uint64_t n_amp, n_ed; size_t lines;
        in >> min_reads >> want_rc >> n_amp;
        // every array in a heap block of exactly its size: a read outside it is the sanitizer's to report
        std::vector<uint64_t> st(n_amp); std::vector<uint32_t> len(n_amp), reads(n_amp);
        for (uint64_t a = 0; a < n_amp; ++a) in >> st[a] >> len[a] >> reads[a];
        in >> n_ed;
        std::vector<uint32_t> ea(n_ed); std::vector<uint64_t> ex(n_ed); std::vector<uint8_t> eb(n_ed);
        for (uint64_t e = 0; e < n_ed; ++e) { unsigned b; in >> ea[e] >> ex[e] >> b; eb[e] = (uint8_t)b; }
        in >> lines;
        std::vector<char> g(genome.begin(), genome.end());
        std::string body, want;
        const int rc = scs::site_probe(st.data(), len.data(), reads.data(), n_amp, ea.data(), ex.data(), eb.data(), n_ed, rec_len.data(), names, g.data(), g.size(), min_reads, body);
        if (want_rc == 0) for (size_t k = 0; k < lines; ++k) { std::getline(std::cin, ln); want += ln + "\n"; }
        ++n_cases;
        if (rc != want_rc || (rc == 0 && body != want)) { ++bad; fprintf(stderr, "case %d: rc %d (want %d)\n got  %s want %s", n_cases, rc, want_rc, body.c_str(), want.c_str()); }
    }
    printf("%d cases, %d wrong\n", n_cases, bad);
    return bad || !n_cases ? 1 : 0;
}
