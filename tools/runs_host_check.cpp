// runs_host_check.cpp -- the bedGraph line of the per-base arrays' writer (scs_runs.h: runs_line, the counting sink of the sizing
// pass, the capped buffer of scs_runs_line_probe) as a stand-alone program, to be built with -fsanitize=address,undefined and run on
// a CPU box (tools/runs_host_check.py builds it and replays the host table of tests/test_runs_host.py through it).  No GPU, no HIP.
// Input (stdin), per line: <name, @ for the empty one> <start> <end> <value>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_runs.h"

int main() {
    std::string ln; int n_lines = 0, bad = 0;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string name; unsigned long long start, end, value;
        if (!(in >> name >> start >> end >> value)) continue;
        if (name == "@") name.clear();
        ++n_lines;
        char want[512];
        const int nw = snprintf(want, sizeof want, "%s\t%llu\t%llu\t%llu\n", name.c_str(), start, end, value);
        std::vector<char> nm(name.begin(), name.end());                            // the name without a terminator, in a block of exactly its size
        scs::RunsCount cnt; scs::runs_line(cnt, nm.data(), (uint32_t)nm.size(), start, end, (uint32_t)value);
        std::vector<char> out(cnt.n);                                              // a heap block of exactly the counted size
        scs::RunsBuf b{out.data(), out.size(), 0}; scs::runs_line(b, nm.data(), (uint32_t)nm.size(), start, end, (uint32_t)value);
        bool ok = nw > 0 && (uint64_t)nw == cnt.n && b.n == cnt.n && !memcmp(out.data(), want, cnt.n);
        std::vector<char> shorter(cnt.n - 1, '#');                                 // one byte short: the size is still reported, nothing is written past the block
        scs::RunsBuf s{shorter.data(), shorter.size(), 0}; scs::runs_line(s, nm.data(), (uint32_t)nm.size(), start, end, (uint32_t)value);
        ok = ok && s.n == cnt.n && !memcmp(shorter.data(), want, shorter.size());
        if (!ok) { ++bad; fprintf(stderr, "line %d (%s): got %llu bytes, wanted %d\n", n_lines, ln.c_str(), (unsigned long long)b.n, nw); }
    }
    printf("%d lines, %d wrong\n", n_lines, bad);
    return bad || !n_lines ? 1 : 0;
}
