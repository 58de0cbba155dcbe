// scs_textout.h -- private to the host files whose kernels make a file's bytes (scs_reads.cpp: FASTQ blocks, truth SAM / BAM;
// scs_amplicons.cpp, scs_sites.cpp, scs_support.cpp: the tables): the staged records as the kernels read them, and BGZF over bytes
// where they lie on the device.  The file itself is scs_outfile.h's.
#pragma once
#include "scs_ctx.h"
#include <cstdarg>

namespace scs {

static_assert(kBgzfHostCap == BGZF_LDS_OUT, "a header's BGZF blocks are made as the device's are");

// where every staged record starts among the genome's bases, and behind the last one where it ends: nr + 1 entries
inline std::vector<uint64_t> record_starts(const scs_ctx* c) {
    const size_t nr = c->recs.size(); std::vector<uint64_t> roff(nr + 1, 0);
    for (size_t r = 0; r < nr; ++r) { roff[r] = c->rec_off[r]; roff[r + 1] = c->rec_off[r] + c->rec_len[r]; }
    return roff;
}

// the same from any records' lengths
inline std::vector<uint64_t> starts_of(const std::vector<uint64_t>& lens) {
    std::vector<uint64_t> roff(lens.size() + 1, 0);
    for (size_t r = 0; r < lens.size(); ++r) roff[r + 1] = roff[r] + lens[r];
    return roff;
}

// printf behind o: a line's numbers (at most 511 bytes a call; names of any length are appended as they are)
inline void text_printf(std::string& o, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline void text_printf(std::string& o, const char* fmt, ...) {
    char buf[512]; va_list ap; va_start(ap, fmt); const int n = vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (n > 0) o.append(buf, std::min<size_t>((size_t)n, sizeof buf - 1));
}

// the kernels' record table on the device: record starts (n + 1), name offsets (n + 1), names, 16 bytes of slack.  It lies in the
// table's own buffer, which goes with it, or in `into` (the truth passes' t_recs, which the ctx keeps between yield calls).  Over
// any records -- roff: their n + 1 starts, name(r): record r's name -- or over the staged ones
struct RecTable {
    DevBuf tab; const uint64_t* rec_off = nullptr; const uint32_t* name_off = nullptr; const char* names = nullptr; uint32_t n_rec = 0; uint64_t bases = 0;
    template <class Name> void make(const std::vector<uint64_t>& roff, Name name, hipStream_t s, DevBuf* into = nullptr) {
        DevBuf& d = into ? *into : tab;
        const uint32_t nr = (uint32_t)roff.size() - 1u;
        std::vector<uint32_t> noff(nr + 1, 0); std::string text;
        for (uint32_t r = 0; r < nr; ++r) { text += name(r); noff[r + 1] = (uint32_t)text.size(); }
        bases = roff[nr];
        const size_t o_name = (size_t)(nr + 1) * 8, o_text = o_name + (size_t)(nr + 1) * 4; std::vector<uint8_t> blob(o_text + text.size() + 16, 0);
        memcpy(blob.data(), roff.data(), o_name); memcpy(blob.data() + o_name, noff.data(), (size_t)(nr + 1) * 4); memcpy(blob.data() + o_text, text.data(), text.size());
        upload(d, blob, s); HIP_OK(hipStreamSynchronize(s));                          // (the host blob goes)
        const uint8_t* tb = d.as<uint8_t>();
        rec_off = (const uint64_t*)tb; name_off = (const uint32_t*)(tb + o_name); names = (const char*)(tb + o_text); n_rec = nr;
    }
    void make(const scs_ctx* c, hipStream_t s, DevBuf* into = nullptr) { make(record_starts(c), [&](uint32_t r) -> const std::string& { return c->recs[r].name; }, s, into); }
};

// the BGZF kernels' CRC tables in `crc`: uploaded (and waited for) where it holds none yet
inline void bgzf_crc_tables(DevBuf& crc, hipStream_t s) {
    if (crc.p) return;
    std::vector<uint32_t> tabs(512); bgzf_host_tables(tabs.data(), tabs.data() + 256); upload(crc, tabs, s); HIP_OK(hipStreamSynchronize(s));
}

// n bytes at `text` become BGZF blocks at `dst` (the caller's, bgzf_bound(n) bytes) where they lie: plan (code lengths, exact block
// sizes), prefix sum (scan_tmp / scan_bytes: exclusive_scan_u32's scratch; nullptr, 0: its one-workgroup form, no scratch), emit at
// the final offsets.  The blocks' total is only known on the device: it travels to the pinned word h_total, behind everything here
inline void bgzf_in_place(hipStream_t s, BgzfLane& z, const DevBuf& crc, const char* text, uint64_t n, char* dst, uint32_t* h_total, void* scan_tmp, size_t scan_bytes, const char* too_large) {
    if (bgzf_bound(n) > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, too_large);
    const uint32_t nblk = bgzf_blocks(n);
    z.plan.reserve(std::max<size_t>((size_t)nblk * BGZF_PLAN_BYTES, 16), s); z.sizes.reserve(((size_t)nblk + 2) * 4, s); z.offs.reserve(((size_t)nblk + 2) * 4, s);
    launch_bgzf_plan(s, text, n, z.plan.as<uint8_t>(), z.sizes.as<uint32_t>());
    exclusive_scan_u32(s, z.sizes.as<uint32_t>(), z.offs.as<uint32_t>(), nblk, scan_tmp, scan_bytes);
    launch_bgzf_emit(s, text, n, z.plan.as<uint8_t>(), z.sizes.as<uint32_t>(), z.offs.as<uint32_t>(), crc.as<uint32_t>(), crc.as<uint32_t>() + 256, dst, 0);
    HIP_OK(hipMemcpyAsync(h_total, z.offs.as<uint32_t>() + nblk, 4, hipMemcpyDeviceToHost, s));
}

// what the scs_*_kernel_time entry points answer from their timer
inline int kernel_time_of(const scs_ctx* c, const KernelTimer scs_ctx::* tm, uint64_t* launches, double* ms, uint64_t* units) {
    if (!c) return SCS_EINVAL;
    const KernelTimer& t = c->*tm;
    if (launches) *launches = t.launches; if (ms) *ms = t.ms; if (units) *units = t.units;
    return SCS_OK;
}

}  // namespace scs
