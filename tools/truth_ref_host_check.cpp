// truth_ref_host_check.cpp -- the formatter of the truth SAM on the original reference (scs_truth_ref.h: lift_align, lift_align_ops,
// truth_ref_record with everything they run) as a stand-alone program, to be built with -fsanitize=address,undefined and run on a
// CPU box (tools/truth_ref_host_check.py builds it and replays the grid of tests/test_truth_ref_host.py through it).  No GPU, no HIP.
// Input (stdin), per line:
//   table <id> <n_seg> <n_hap> <n_ref> <hap_off> <len> <ref_pos> <ref_rec> <kind> ... <hap length> ... <ref length> ... <ref name> ... <hap name> ...
//   read <table id> <paired> <is read 2> <n> <pos0> <reverse> <nev> <position> <deletion> <length> ... <mate pos0> <mate reverse> <mate nev> ... <seq> <qual> <the line, '|' for tabs>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../scssim_amd/csrc/scs_truth_ref.h"

struct Table { std::vector<scs::LiftSeg> segs; std::vector<uint64_t> hap_off, ref_len; std::vector<uint32_t> name_off; std::vector<char> names; std::vector<std::string> hap_names; };
struct Src { const char* s; const char* q; char seq(int i) const { return s[i]; } char qual(int i) const { return q[i]; } };
struct VecOut { std::string t; void put(char ch) { t.push_back(ch); } };

int main() {
    std::string ln; int n_reads = 0, bad = 0; std::map<int, Table> tables;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln); std::string kind; in >> kind;
        if (kind == "table") {
            int id; size_t ns, nh, nr; in >> id >> ns >> nh >> nr;
            Table& T = tables[id]; T.segs.resize(ns); T.hap_off.assign(nh + 1, 0); T.ref_len.resize(nr); T.name_off.assign(nr + 1, 0); T.hap_names.resize(nh);   // every array in a heap block of exactly its size
            for (auto& s : T.segs) in >> s.hap_off >> s.len >> s.ref_pos >> s.ref_rec >> s.kind;
            for (size_t r = 0; r < nh; ++r) { uint64_t l; in >> l; T.hap_off[r + 1] = T.hap_off[r] + l; }
            for (auto& l : T.ref_len) in >> l;
            std::string text;
            for (size_t r = 0; r < nr; ++r) { std::string nm; in >> nm; text += nm; T.name_off[r + 1] = (uint32_t)text.size(); }
            T.names.assign(text.begin(), text.end());
            for (auto& nm : T.hap_names) in >> nm;
        } else if (kind == "read") {
            int id, paired, read2, n; int64_t pos[2]; int rev[2], nev[2]; std::vector<uint32_t> ev[2];
            in >> id >> paired >> read2 >> n;
            for (int k = 0; k < 2; ++k) {
                in >> pos[k] >> rev[k] >> nev[k]; ev[k].resize((size_t)nev[k]);
                for (int i = 0; i < nev[k]; ++i) { uint32_t p, d, l; in >> p >> d >> l; ev[k][(size_t)i] = scs::tev_pack(p, d, l); }
            }
            std::string seq, qual, want; in >> seq >> qual >> want;
            for (char& ch : want) if (ch == '|') ch = '\t';
            want.push_back('\n');
            const Table& T = tables[id]; ++n_reads;
            const std::vector<char> s(seq.begin(), seq.end()), q(qual.begin(), qual.end());   // (no terminator: a read past the end is a report)
            scs::TruthAln a{pos[0], rev[0], n, nev[0], ev[0].data(), 0, 0, 0}, m{pos[1], rev[1], n, nev[1], ev[1].data(), 0, 0, 0};
            if (!scs::truth_place(a) || a.qlen != (int)s.size() || (paired && !scs::truth_place(m))) { ++bad; fprintf(stderr, "read %d: not placed\n", n_reads); continue; }
            const int64_t first_lo = paired && read2 ? m.lo : a.lo;
            size_t rec = 0; while (rec + 2 < T.hap_off.size() && (int64_t)T.hap_off[rec + 1] <= first_lo) ++rec;
            const int64_t r0 = (int64_t)T.hap_off[rec], r1 = (int64_t)T.hap_off[rec + 1];
            const scs::LiftTab V{T.segs.data(), (uint32_t)T.segs.size(), T.ref_len.data(), (uint32_t)T.ref_len.size()};
            scs::LiftAln la{}, lm{};
            int err = scs::lift_align(a, r0, r1, V, la);
            if (!err && paired) err = scs::lift_align(m, r0, r1, V, lm);
            const std::string& hn = T.hap_names[rec];
            const scs::TruthRefLine li{7u, 3u, paired, read2, paired ? m.rev : 0, hn.data(), (uint32_t)hn.size(), r0, r1, T.name_off.data(), T.names.data()};
            VecOut o; scs::TruthCount cnt;
            if (!err) err = scs::truth_ref_record(o, a, li, V, la, lm, Src{s.data(), q.data()});
            if (!err) err = scs::truth_ref_record(cnt, a, li, V, la, lm, Src{s.data(), q.data()});
            if (err || o.t != want || cnt.n != o.t.size()) { ++bad; fprintf(stderr, "read %d: error %d, counted %llu\n got    %s wanted %s", n_reads, err, (unsigned long long)cnt.n, o.t.c_str(), want.c_str()); }
        }
    }
    printf("%d reads, %d wrong\n", n_reads, bad);
    if (!bad && n_reads) printf("ok\n");
    return bad || !n_reads ? 1 : 0;
}
