// amp_host_check.cpp -- the amplicon table's host code (scs_amp.h: amp_line_probe and everything it runs) as a stand-alone program,
// to be built with -fsanitize=address,undefined and run on a CPU box (tools/amp_host_check.py builds it, replays the case table
// of tests/test_amplicons_host.py through it and compares every line with the restatement's).  No GPU, no HIP.
// Input (stdin), per case:  genome <bases> once, then
//   case <frag_goff> <frag_len> <frag_strand> <semi_spos> <semi_len> <n1> <e...> <full_spos> <full_len> <n2> <e...> <genome_start> <genome_len>
//        <rec_off> <rec_len> <rec_name> <index> <reads> <semi> <expected return code>
//   followed by the expected line (when the return code is 0).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_amp.h"

int main() {
    std::string genome, ln; int n_cases = 0, bad = 0;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string kind; in >> kind;
        if (kind == "genome") { in >> genome; continue; }
        if (kind != "case") continue;
        uint64_t goff, gs, gl, ro, rl; uint32_t fl, ss, sl, n1, fs, fln, n2, index, reads, semi; int st, want_rc; std::string name;
        in >> goff >> fl >> st >> ss >> sl >> n1; std::vector<uint32_t> e1(n1); for (auto& e : e1) in >> e;
        in >> fs >> fln >> n2; std::vector<uint32_t> e2(n2); for (auto& e : e2) in >> e;
        in >> gs >> gl >> ro >> rl >> name >> index >> reads >> semi >> want_rc;
        // the window of the genome in a heap block of exactly its size: a read outside it is the sanitizer's to report
        std::vector<char> win(genome.begin() + (long)gs, genome.begin() + (long)(gs + gl));
        std::string line, want;
        const int rc = scs::amp_line_probe(goff, fl, st, ss, sl, e1.data(), n1, fs, fln, e2.data(), n2, win.data(), gs, gl, ro, rl, name.c_str(), index, reads, semi, line);
        if (want_rc == 0) { std::getline(std::cin, want); want += "\n"; }
        ++n_cases;
        if (rc != want_rc || (rc == 0 && line != want)) { ++bad; fprintf(stderr, "case %d: rc %d (want %d)\n got  %s want %s", n_cases, rc, want_rc, line.c_str(), want.c_str()); }
    }
    printf("%d cases, %d wrong\n", n_cases, bad);
    return bad || !n_cases ? 1 : 0;
}
