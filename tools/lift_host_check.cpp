// lift_host_check.cpp -- the lift table's host code (scs_lift.h: lift_read with everything it runs, and the file's parser) as a
// stand-alone program, to be built with -fsanitize=address,undefined and run on a CPU box (tools/lift_host_check.py builds it and
// replays the grid and the case table of tests/test_lift_host.py through it).  No GPU, no HIP.
// Input (stdin), per line:
//   table <id> <n_seg> <n_hap> <n_ref> <hap_off> <len> <ref_pos> <ref_rec> <kind> ... <hap length> ... <ref length> ...
//   read <table id> <n> <pos0> <reverse> <bin width> <nev> <position> <deletion> <length> ... <reads bin> <n_want> <bin> <bases> ...
//   file <path> <line it must be refused at, 0: it must parse>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_lift.h"
#include "../scssim_amd/csrc/scs_depth.h"

struct Table { std::vector<scs::LiftSeg> segs; std::vector<uint64_t> hap_off, ref_len; };

int main() {
    std::string ln; int n_reads = 0, n_files = 0, bad = 0; std::map<int, Table> tables;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string kind; in >> kind;
        if (kind == "table") {
            int id; size_t ns, nh, nr; in >> id >> ns >> nh >> nr;
            Table& T = tables[id]; T.segs.resize(ns); T.hap_off.assign(nh + 1, 0); T.ref_len.resize(nr);   // every array in a heap block of exactly its size
            for (auto& s : T.segs) in >> s.hap_off >> s.len >> s.ref_pos >> s.ref_rec >> s.kind;
            for (size_t r = 0; r < nh; ++r) { uint64_t l; in >> l; T.hap_off[r + 1] = T.hap_off[r] + l; }
            for (auto& l : T.ref_len) in >> l;
        } else if (kind == "read") {
            int id, n, reverse, nev; int64_t pos0; uint32_t w; uint64_t want_first, n_want;
            in >> id >> n >> pos0 >> reverse >> w >> nev;
            std::vector<uint32_t> ev(nev);
            for (int i = 0; i < nev; ++i) { uint32_t p, d, l; in >> p >> d >> l; ev[i] = scs::tev_pack(p, d, l); }
            in >> want_first >> n_want; std::map<uint64_t, uint64_t> want, got;
            for (uint64_t i = 0; i < n_want; ++i) { uint64_t b, k; in >> b >> k; want[b] = k; }
            const Table& T = tables[id]; ++n_reads;
            std::vector<uint64_t> boff(T.ref_len.size() + 1); uint64_t nb = 0;
            scs::TruthAln a{pos0, reverse, n, nev, ev.data(), 0, 0, 0};
            if (!scs::truth_place(a) || !scs::depth_layout(T.ref_len.data(), T.ref_len.size(), w, boff.data(), &nb, nullptr)) { ++bad; fprintf(stderr, "read %d: not placed\n", n_reads); continue; }
            size_t rec = 0; while (rec + 2 < T.hap_off.size() && (int64_t)T.hap_off[rec + 1] <= a.lo) ++rec;
            const scs::LiftView V{T.segs.data(), (uint32_t)T.segs.size(), T.ref_len.data(), boff.data(), (uint32_t)T.ref_len.size(), w, nb};
            uint64_t first = ~0ull;
            const int err = scs::lift_read(a, (int64_t)T.hap_off[rec], (int64_t)T.hap_off[rec + 1], V, [&](uint64_t b) { first = b; }, [&](uint64_t b, uint32_t k) { got[b] += k; });
            if (err || first != want_first || got != want) { ++bad; fprintf(stderr, "read %d: error %d, reads bin %llu (wanted %llu), %zu bins (wanted %zu)\n", n_reads, err, (unsigned long long)first, (unsigned long long)want_first, got.size(), want.size()); }
        } else if (kind == "file") {
            std::string path; uint64_t want_line; in >> path >> want_line;
            scs::LiftTable T; std::string why; uint64_t line = 0; ++n_files;
            const bool ok = scs::lift_parse(path, T, why, line);
            if (ok != (want_line == 0) || (!ok && line != want_line)) { ++bad; fprintf(stderr, "file %s: %s at line %llu (wanted %llu)\n", path.c_str(), ok ? "parsed" : why.c_str(), (unsigned long long)line, (unsigned long long)want_line); }
            if (ok) {                                                               // what parses writes back and parses again to the same table
                const std::string again = path + ".again"; scs::LiftTable U;
                if (!scs::lift_write(T, again) || !scs::lift_parse(again, U, why, line) || U.segs.size() != T.segs.size() || memcmp(U.segs.data(), T.segs.data(), T.segs.size() * sizeof(scs::LiftSeg))) { ++bad; fprintf(stderr, "file %s: no round trip\n", path.c_str()); }
            }
        }
    }
    printf("%d reads, %d files, %d wrong\n", n_reads, n_files, bad);
    return bad || !n_reads || !n_files ? 1 : 0;
}
