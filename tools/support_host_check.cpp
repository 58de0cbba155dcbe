// support_host_check.cpp -- the site support's host code (scs_support.h: support_read and everything it runs) as a stand-alone
// program, to be built with -fsanitize=address,undefined and run on a CPU box (tools/support_host_check.py builds it and replays
// the grid of tests/test_support_host.py through it).  No GPU, no HIP.
// Input (stdin), per case:
//   case <n> <pos0> <reverse> <rec_len> <bases> <nev> <position> <deletion> <length> ... <n_pos> <position> ... <n_want> <index> <class> ...
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_support.h"

int main() {
    std::string ln; int n_cases = 0, bad = 0;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string kind, bases; in >> kind;
        if (kind != "case") continue;
        int n, reverse, nev; int64_t pos0; uint64_t rec_len, n_pos, n_want;
        in >> n >> pos0 >> reverse >> rec_len >> bases >> nev;
        // every array in a heap block of exactly its size: a read outside it is the sanitizer's to report
        std::vector<uint32_t> ev(nev);
        for (int i = 0; i < nev; ++i) { uint32_t p, d, l; in >> p >> d >> l; ev[i] = scs::tev_pack(p, d, l); }
        in >> n_pos; std::vector<uint64_t> pos(n_pos); for (uint64_t i = 0; i < n_pos; ++i) in >> pos[i];
        in >> n_want; std::vector<std::pair<uint64_t, uint32_t>> want(n_want), got; for (uint64_t i = 0; i < n_want; ++i) in >> want[i].first >> want[i].second;
        std::vector<char> seq(bases.begin(), bases.end());
        scs::TruthAln a{pos0, reverse, n, nev, ev.data(), 0, 0, 0};
        ++n_cases;
        if (!scs::truth_place(a) || a.lo < 0 || a.hi >= (int64_t)rec_len || a.qlen != (int)seq.size()) { ++bad; fprintf(stderr, "case %d: not placed\n", n_cases); continue; }
        scs::support_read(a, pos.data(), n_pos, [&](int i) { return seq[(size_t)i]; }, [&](uint64_t i, uint32_t k) { got.push_back({i, k}); });
        if (got != want) { ++bad; fprintf(stderr, "case %d: %zu reports, %zu wanted\n", n_cases, got.size(), want.size()); }
    }
    printf("%d cases, %d wrong\n", n_cases, bad);
    return bad || !n_cases ? 1 : 0;
}
