// scs_runs.cpp -- the bedGraph writer of the per-base arrays the coverage work leaves on the device (include/scssim_hip.h:
// scs_write_coverage_bedgraph, scs_write_coverage_ref_bedgraph, scs_write_copy_number_ref): one run-length
// text writer over a uint32 array, its slab plan, file and probes.  The entry points and their refusals are scs_coverage.cpp's (they
// know which array stands); the line is scs_runs.h's, the kernels are scs_k_runs.hip's.
//
// A call: the plan pass leaves every tile's lines and bytes; the host cuts the tiles into SLABS whose text fits the cap (cut at
// tile borders: a line lies wholly in the slab of its first base); per slab a 64-bit scan of its tile bytes, the emit pass, BGZF
// where the bytes lie (.gz), one copy through pinned memory, the flags, the file.  Device memory for text never passes the cap,
// whatever the genome's size.  The arrays are only read.
#include "scs_textout.h"
#include <functional>

namespace scs {
namespace {

uint64_t runs_text_cap() {                                 // the product reads nothing from the environment (scs_seams.h)
    const char* e = seam_env("SCS_TEST_RUNS_TEXT_CAP");
    return e ? (uint64_t)std::max(1ll, atoll(e)) : RUNS_TEXT_CAP;
}

struct RunsSlab { uint32_t t0, t1; uint64_t bytes; };
// greedy: a slab takes tiles while their text fits `cap`.  A tile that alone does not is the caller's error, not a loop
std::vector<RunsSlab> runs_slabs(const std::string& who, const std::vector<uint32_t>& bytes, uint64_t cap) {
    std::vector<RunsSlab> out; RunsSlab cur{0, 0, 0};
    for (uint32_t t = 0; t < bytes.size(); ++t) {
        if (bytes[t] > cap) throw ScsError(SCS_EINVAL, who + ": the text of tile " + std::to_string(t) + " alone is " + std::to_string(bytes[t]) + " bytes, the text cap " + std::to_string(cap));
        if (cur.bytes + bytes[t] > cap) { out.push_back(cur); cur = RunsSlab{t, t, 0}; }
        cur.bytes += bytes[t]; cur.t1 = t + 1;
    }
    if (cur.t1 > cur.t0) out.push_back(cur);
    return out;
}

// ends every way out of a write: the ctx stream drained before anyone touches the buffers again; the timer's open events dropped
struct RunsCall {
    scs_ctx* c;
    ~RunsCall() { (void)hipStreamSynchronize(c->stream); c->tm_runs.drop_events(); }
};

using RunsPut = std::function<void(const char*, size_t)>;

// the text (bgzf: its BGZF blocks, every slab's on a block border, without the end-of-file block) of values[n] through put
void runs_write(scs_ctx* c, const std::string& who, const uint32_t* values, uint32_t mask, uint64_t n, const RecTable& rt, uint64_t cap, bool bgzf, const RunsPut& put,
                uint64_t* lines_out, uint64_t* text_out, uint64_t* slabs_out) {
    RunsWork& W = c->runs; KernelTimer& tm = c->tm_runs; const hipStream_t s = c->stream;
    tm.reset();
    uint64_t lines = 0, text = 0, n_slabs = 0;
    const uint64_t nt = runs_tiles(n);
    if (nt > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, who + ": the array has more tiles than a grid holds");
    if (nt) {
        RunsCall call{c};
        W.first.reserve((size_t)nt * 4, s); W.next.reserve((size_t)nt * 8, s); W.lines.reserve(((size_t)nt + 1) * 4, s); W.bytes.reserve(((size_t)nt + 1) * 4, s);
        W.offs.reserve(((size_t)nt + 1) * 8, s); W.scan.reserve(scan_temp_bytes(nt), s);
        const RunsArgs a{values, mask, n, rt.rec_off, rt.name_off, rt.names, rt.n_rec, W.first.as<uint32_t>(), W.next.as<uint64_t>(), W.lines.as<uint32_t>(), W.bytes.as<uint32_t>(), c->flags.as<uint32_t>()};
        tm.begin(s);
        launch_runs_plan(s, a);
        tm.end(s); tm.add_units(n);
        std::vector<uint32_t> t_lines(nt), t_bytes(nt);
        HIP_OK(hipMemcpyAsync(t_lines.data(), W.lines.p, (size_t)nt * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipMemcpyAsync(t_bytes.data(), W.bytes.p, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, who + ": the plan pass failed: " + hipGetErrorString(le)); }
        for (uint64_t t = 0; t < nt; ++t) { lines += t_lines[t]; text += t_bytes[t]; }
        const std::vector<RunsSlab> slabs = runs_slabs(who, t_bytes, cap);
        uint64_t most = 0; for (const RunsSlab& sl : slabs) most = std::max(most, sl.bytes);
        if (bgzf && bgzf_bound(most) > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, who + ": a slab's text exceeds 4 GB");
        W.text.reserve((size_t)most + 16, s);
        W.h_text.reserve(std::max<size_t>(bgzf ? bgzf_bound(most) : most, 16), hipHostMallocDefault);
        W.h_n.reserve(64, hipHostMallocDefault);
        if (bgzf) { bgzf_crc_tables(W.crc, s); W.z.out[0].reserve(bgzf_bound(most), s); }
        for (const RunsSlab& sl : slabs) {
            if (!sl.bytes) continue;
            const uint32_t tiles = sl.t1 - sl.t0;
            tm.begin(s);
            exclusive_scan_u32_to_u64(s, W.bytes.as<uint32_t>() + sl.t0, W.offs.as<uint64_t>(), tiles, W.scan.p, W.scan.cap);
            launch_runs_emit(s, a, sl.t0, tiles, W.offs.as<uint64_t>(), 0, W.text.as<char>());
            const char* made = W.text.as<char>(); uint64_t n_made = sl.bytes;
            if (bgzf) {                                    // the text becomes BGZF blocks where it lies; their total is only known on the device
                bgzf_in_place(s, W.z, W.crc, made, sl.bytes, W.z.out[0].as<char>(), W.h_n, nullptr, 0, "a slab's text exceeds 4 GB");
                tm.end(s);
                HIP_OK(hipStreamSynchronize(s));
                made = W.z.out[0].as<char>(); n_made = W.h_n[0];
                if (n_made > bgzf_bound(sl.bytes)) throw ScsError(SCS_EDEVICE, who + ": the BGZF blocks of a slab outgrow their bound");
            } else tm.end(s);
            HIP_OK(hipMemcpyAsync(W.h_text, made, n_made, hipMemcpyDeviceToHost, s));
            check_flags(c);                                // (waits for everything on the ctx stream; a text that left its plan never reaches the file)
            put(W.h_text, n_made);
            ++n_slabs;
        }
        HIP_OK(hipStreamSynchronize(s));
        tm.collect();
    }
    if (lines_out) *lines_out = lines;
    if (text_out) *text_out = text;
    if (slabs_out) *slabs_out = n_slabs;
}

void runs_names_fit(const std::string& who, const std::vector<std::string>& names) {
    for (const std::string& nm : names) if (nm.size() > RUNS_NAME_MAX) throw ScsError(SCS_EINVAL, who + ": a record name of " + std::to_string(nm.size()) + " bytes (at most 65535)");
}

}  // namespace

void runs_write_file(scs_ctx* c, const std::string& who, const char* path, const uint32_t* values, uint32_t mask, uint64_t n, const std::vector<uint64_t>& roff,
                     const std::vector<std::string>& names, uint64_t* lines, uint64_t* text_bytes) {
    const std::string p = path; const bool bgzf = p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0;
    runs_names_fit(who, names);
    OutFile fd; fd.open(who, p, bgzf);                     // (an unwritable path fails here, before any GPU work)
    HIP_OK(hipStreamSynchronize(c->stream));
    RecTable rt; rt.make(roff, [&](uint32_t r) -> const std::string& { return names[r]; }, c->stream);
    runs_write(c, who, values, mask, n, rt, runs_text_cap(), bgzf, [&](const char* b, size_t k) { fd.write(b, k); }, lines, text_bytes, nullptr);
    fd.finish();
}

}  // namespace scs

extern "C" {

int scs_coverage_bedgraph_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_runs, launches, ms, units); }

int scs_runs_probe(scs_ctx* c, const uint32_t* values, uint64_t n, uint32_t mask, const uint64_t* rec_lens, uint32_t n_rec, const char* const* names, uint64_t text_cap, int bgzf,
                   char* out, uint64_t out_cap, uint64_t* n_out, uint64_t* lines, uint64_t* slabs) {
    return guarded(c, [&] {
        const std::string fn = "scs_runs_probe";
        if (!values || !n || !rec_lens || !n_rec || !names || (!out && out_cap)) throw ScsError(SCS_EINVAL, fn + ": bad argument");
        std::vector<uint64_t> roff(n_rec + 1, 0); std::vector<std::string> nm(n_rec);
        for (uint32_t r = 0; r < n_rec; ++r) { if (!names[r]) throw ScsError(SCS_EINVAL, fn + ": bad argument"); roff[r + 1] = roff[r] + rec_lens[r]; nm[r] = names[r]; }
        if (roff[n_rec] != n) throw ScsError(SCS_EINVAL, fn + ": the records' lengths add up to " + std::to_string(roff[n_rec]) + ", the array has " + std::to_string(n) + " entries");
        runs_names_fit(fn, nm);
        const hipStream_t s = c->stream; DevBuf d_val; const size_t padded = (size_t)runs_tiles(n) * COV_TILE * 4;
        d_val.reserve(padded, s);
        HIP_OK(hipMemsetAsync(d_val.p, 0, padded, s)); HIP_OK(hipMemcpyAsync(d_val.p, values, (size_t)n * 4, hipMemcpyHostToDevice, s));
        RecTable rt; rt.make(roff, [&](uint32_t r) -> const std::string& { return nm[r]; }, s);
        std::string made;
        runs_write(c, fn, d_val.as<uint32_t>(), mask, n, rt, text_cap ? text_cap : runs_text_cap(), bgzf != 0, [&](const char* b, size_t k) { made.append(b, k); }, lines, nullptr, slabs);
        if (bgzf) made.append((const char*)kBgzfEof, sizeof kBgzfEof);
        if (n_out) *n_out = made.size();
        if (made.size() > out_cap) throw ScsError(SCS_EOVERFLOW, fn + ": " + std::to_string(made.size()) + " bytes, room for " + std::to_string(out_cap));
        if (!made.empty()) memcpy(out, made.data(), made.size());
    });
}

int scs_runs_line_probe(const char* name, uint64_t start, uint64_t end, uint32_t value, char* out, uint64_t cap, uint64_t* n_out) {
    if (!name || (!out && cap)) return SCS_EINVAL;
    RunsBuf b{out, cap, 0};
    runs_line(b, name, (uint32_t)strlen(name), start, end, value);
    if (n_out) *n_out = b.n;
    return b.n > cap ? SCS_EOVERFLOW : SCS_OK;
}

}  // extern "C"
