// scs_outfile.h -- the library's error type and the one output file of everything that is made on the device and written by the
// host (the truth SAM / BAM, the amplicon, artefact and site support tables): open, header, the bytes, the BGZF end-of-file block,
// a checked close.  No HIP here: tools/outfile_host_check.cpp builds it alone, under the sanitizers.
#pragma once
#include "../../include/scssim_hip.h"
#include <cerrno>
#include <cstring>
#include <fcntl.h>
#include <stdexcept>
#include <string>
#include <unistd.h>
#include <vector>

namespace scs {

struct ScsError : std::runtime_error { int code; ScsError(int c, const std::string& m) : std::runtime_error(m), code(c) {} };

// the BGZF end-of-file block (SAM specification, section 4.1.2)
static const unsigned char kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void bgzf_compress_host(const uint8_t* text, uint64_t nbytes, uint32_t lds_out_cap, std::vector<uint8_t>& out);   // (scs_bgzf.h)
const uint32_t kBgzfHostCap = 40960u;                      // BGZF_LDS_OUT: a header's blocks are made as the device's are (scs_textout.h holds the two equal)

inline bool write_all(int fd, const char* p, size_t n) {
    while (n) { const ssize_t w = ::write(fd, p, n); if (w < 0 && errno == EINTR) continue; if (w <= 0) return false; p += w; n -= (size_t)w; }
    return true;
}

// who: what the error texts begin with (the entry point's name, "truth SAM"); total: the bytes in the file so far -- a caller whose
// bytes reach the file by another road (the sink pipe's writer, through fd) adds them itself.  Closed by finish, or with its owner
struct OutFile {
    int fd = -1; bool bgzf = false; uint64_t total = 0; std::string who, path;
    OutFile() = default; OutFile(const OutFile&) = delete; OutFile& operator=(const OutFile&) = delete;
    ~OutFile() { if (fd >= 0) ::close(fd); }
    std::string failed(const char* doing) const { return who + ": " + doing + " " + path + " failed"; }
    void open(const std::string& who_, const std::string& path_, bool bgzf_) {
        who = who_; path = path_; bgzf = bgzf_; total = 0;
        fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (fd < 0) throw ScsError(SCS_EIO, who + ": can not open " + path + ": " + strerror(errno));
    }
    void write(const char* p, size_t n) { if (!write_all(fd, p, n)) throw ScsError(SCS_EIO, failed("writing")); total += n; }
    void header(const std::string& hd) {                       // BGZF: compressed on the host
        if (!bgzf) return write(hd.data(), hd.size());
        std::vector<uint8_t> z; bgzf_compress_host((const uint8_t*)hd.data(), hd.size(), kBgzfHostCap, z); write((const char*)z.data(), z.size());
    }
    void finish(const char* closing = "writing") {           // the end-of-file block when BGZF; closing: what the close's error text says was being done
        if (bgzf) write((const char*)kBgzfEof, sizeof kBgzfEof);
        const int f = fd; fd = -1;
        if (::close(f) != 0) throw ScsError(SCS_EIO, failed(closing));
    }
};

}  // namespace scs
