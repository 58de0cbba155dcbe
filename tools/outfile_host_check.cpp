// outfile_host_check.cpp -- the output file of everything the device makes and the host writes (scs_outfile.h: OutFile and the
// write loop) as a stand-alone program, to be built with -fsanitize=address,undefined and run on a CPU box
// (tools/outfile_host_check.py builds and runs it, and inflates the BGZF file with zlib).  No GPU, no HIP: the library's
// bgzf_compress_host lives beside the kernels, so a stand-in that stores its input in BGZF blocks takes its place here.
// Usage: outfile_host_check <directory>; leaves plain.txt and blocks.gz there.
#include <cstdio>
#include <fstream>
#include <sstream>
#include "../scssim_amd/csrc/scs_outfile.h"

namespace scs {
static uint32_t crc32_of(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    return ~c;
}
void bgzf_compress_host(const uint8_t* text, uint64_t nbytes, uint32_t, std::vector<uint8_t>& out) {   // stored blocks of at most 65280 bytes
    auto le = [&](uint32_t v, int bytes) { for (int k = 0; k < bytes; ++k) out.push_back((uint8_t)(v >> (8 * k))); };
    for (uint64_t at = 0; at < nbytes; at += 65280) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(65280, nbytes - at);
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        out.insert(out.end(), head, head + 16); le(n + 5 + 25, 2);
        out.push_back(1); le(n, 2); le(~n & 0xFFFFu, 2); out.insert(out.end(), text + at, text + at + n);
        le(crc32_of(text + at, n), 4); le(n, 4);
    }
}
}  // namespace scs
using namespace scs;

static std::string slurp(const std::string& path) { std::ifstream f(path, std::ios::binary); std::ostringstream o; o << f.rdbuf(); return o.str(); }

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { ++bad; fprintf(stderr, "wrong: %s\n", what); } }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1], header = "#record\tstart\tend\n";
    // a few buffers, each in a heap block of exactly its size: a read outside one is the sanitizer's to report
    std::vector<std::vector<char>> bufs;
    for (size_t n : {size_t(1), size_t(4099), size_t(0), size_t(3) << 20}) { std::vector<char> b(n); for (size_t i = 0; i < n; ++i) b[i] = (char)('a' + (i * 7 + n) % 26); bufs.push_back(b); }
    std::string body; for (const auto& b : bufs) body.append(b.data(), b.size());
    for (int bgzf = 0; bgzf < 2; ++bgzf) {
        const std::string path = dir + (bgzf ? "/blocks.gz" : "/plain.txt");
        OutFile f; f.open("outfile_host_check", path, bgzf != 0);
        f.header(header);
        std::string want = header;
        if (bgzf) { std::vector<uint8_t> z; bgzf_compress_host((const uint8_t*)header.data(), header.size(), kBgzfHostCap, z); want.assign((const char*)z.data(), z.size()); }
        expect(f.total == want.size(), "the total after the header");
        for (const auto& b : bufs) {                        // (BGZF: the caller's bytes are blocks already, as the device's are)
            std::vector<uint8_t> z; if (bgzf) bgzf_compress_host((const uint8_t*)b.data(), b.size(), kBgzfHostCap, z);
            const std::vector<char> w = bgzf ? std::vector<char>(z.begin(), z.end()) : b;
            f.write(w.data(), w.size()); want.append(w.data(), w.size());
        }
        if (bgzf) want.append((const char*)kBgzfEof, 28);
        f.finish();
        expect(f.fd == -1, "finish closes the file");
        expect(f.total == want.size(), "the total is the file's size");
        expect(slurp(path) == want, bgzf ? "the BGZF file's bytes" : "the plain file's bytes");
    }
    { OutFile f; f.open("outfile_host_check", dir + "/plain.txt", false); f.finish(); expect(slurp(dir + "/plain.txt").empty(), "open truncates"); f.open("outfile_host_check", dir + "/plain.txt", false); f.header(header); for (const auto& b : bufs) f.write(b.data(), b.size()); }   // (left open: its owner closes it)
    expect(slurp(dir + "/plain.txt") == header + body, "a file closed with its owner holds what was written");
    const std::string absent = dir + "/no_such_dir/a.tsv";
    try { OutFile f; f.open("scs_write_amplicons", absent, true); expect(false, "a path in a directory that does not exist opens"); }
    catch (const ScsError& e) { expect(e.code == SCS_EIO && e.what() == "scs_write_amplicons: can not open " + absent + ": No such file or directory", "the open error's text"); }
    { OutFile f; f.who = "truth BAM"; f.path = "x.bam"; expect(f.failed("writing") == "truth BAM: writing x.bam failed" && f.failed("closing") == "truth BAM: closing x.bam failed", "the write and close errors' texts"); }
    { OutFile f; f.open("scs_write_artefacts", dir + "/plain.txt", false); ::close(f.fd);   // a descriptor that is no longer one: the write fails
      try { f.write("x", 1); expect(false, "a write to a closed descriptor succeeds"); }
      catch (const ScsError& e) { expect(e.code == SCS_EIO && e.what() == "scs_write_artefacts: writing " + dir + "/plain.txt failed", "the write error's text"); }
      f.fd = -1; }
    { OutFile f; f.open("outfile_host_check", dir + "/plain.txt", false); f.header(header); for (const auto& b : bufs) f.write(b.data(), b.size()); f.finish(); }
    printf("outfile_host_check: %d wrong\n", bad);
    return bad ? 1 : 0;
}
