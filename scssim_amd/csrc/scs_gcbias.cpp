// scs_gcbias.cpp -- the GC-bias table of the per-base depth (include/scssim_hip.h: scs_gc_bias, scs_write_gc_bias; DESIGN.md section
// 23): depth as a function of the GC content of sliding windows, per staged record and for the genome, made on demand from the
// arrays a yield call with the coverage profile on leaves on the device (scs_coverage.cpp).  The bin and the row statistics are
// scs_gcbias.h's, the kernel is scs_k_gcbias.hip's.  Nothing here runs unless one of the entry points below is called.
#include "scs_textout.h"
#include "scs_gcbias.h"

namespace scs {
namespace {

void gcb_window_ok(const std::string& fn, uint32_t window) {
    if (window < 1u || window > GCB_MAX_WINDOW) throw ScsError(SCS_EINVAL, fn + ": a window of " + std::to_string(window) + " bases (1 to 1024)");
}
void gcb_ready(const scs_ctx* c, const std::string& fn) {
    if (!c->cov.max_depth || !c->cov.valid) throw ScsError(SCS_EINVAL, fn + ": no yield call with the coverage profile on (scs_set_coverage) has finished");
}

// a call's tables on the host: windows and depth_sum, rows of GCB_BINS, and n_windows; nr rows, or nr + 1 with the genome's last
struct GcbTables { uint32_t nr; std::vector<uint64_t> windows, depth_sum, n_windows; };

// The kernel over depth (readable up to depth_alloc entries) and codes of n bases and the device record starts rec (nr + 1), as
// every caller launches it; the tables in `tab` (zeroed here), timed by the ctx's timer; genome: one more row, the records' sum
GcbTables gcb_run(scs_ctx* c, DevBuf& tab, const uint32_t* depth, uint64_t depth_alloc, const uint8_t* codes, uint64_t n, const uint64_t* rec, uint32_t nr, uint32_t window, uint32_t lds, bool genome) {
    const hipStream_t s = c->stream; KernelTimer& tm = c->tm_gcbias;
    const size_t nb = (size_t)nr * GCB_BINS, words = 2 * nb + nr;
    tab.reserve(std::max<size_t>(words * 8, 16), s);
    HIP_OK(hipMemsetAsync(tab.p, 0, std::max<size_t>(words * 8, 16), s));
    unsigned long long* t = tab.as<unsigned long long>();
    tm.reset();
    tm.begin(s);
    launch_gc_bias(s, GcBiasArgs{depth, depth_alloc, codes, n, rec, nr, window, lds, t, t + nb, t + 2 * nb});
    tm.end(s); tm.add_units(n);
    std::vector<uint64_t> all(words);
    if (words) HIP_OK(hipMemcpyAsync(all.data(), tab.p, words * 8, hipMemcpyDeviceToHost, s));
    const hipError_t se = hipStreamSynchronize(s);
    if (se != hipSuccess) { tm.drop_events(); throw ScsError(SCS_EDEVICE, std::string("GC-bias table: ") + hipGetErrorString(se)); }
    tm.collect();
    { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("GC-bias table: the kernel was not launched: ") + hipGetErrorString(le)); }
    const size_t rows = (size_t)nr + (genome ? 1u : 0u);
    GcbTables o{nr, std::vector<uint64_t>(rows * GCB_BINS, 0), std::vector<uint64_t>(rows * GCB_BINS, 0), std::vector<uint64_t>(rows, 0)};
    std::copy(all.begin(), all.begin() + nb, o.windows.begin()); std::copy(all.begin() + nb, all.begin() + 2 * nb, o.depth_sum.begin()); std::copy(all.begin() + 2 * nb, all.end(), o.n_windows.begin());
    if (genome) for (size_t r = 0; r < nr; ++r) {
        for (size_t b = 0; b < GCB_BINS; ++b) { o.windows[nb + b] += o.windows[r * GCB_BINS + b]; o.depth_sum[nb + b] += o.depth_sum[r * GCB_BINS + b]; }
        o.n_windows[nr] += o.n_windows[r];
    }
    return o;
}

// the table of the last yield call's depths at this window
GcbTables gcb_of_ctx(scs_ctx* c, uint32_t window) {
    const CovTrack& T = c->cov;
    return gcb_run(c, c->gcb.tab, T.diff.as<uint32_t>(), cov_tiles(T.bases) * COV_TILE, c->genome.as<uint8_t>(), T.bases, T.rec.as<uint64_t>(), T.n_rec, window, 1u, true);
}

}  // namespace
}  // namespace scs

extern "C" {

int scs_gc_bias(scs_ctx* c, uint32_t window, uint64_t* windows, uint64_t* depth_sum, uint64_t* n_windows, uint64_t cap_rows) {
    return guarded(c, [&] {
        const std::string fn = "scs_gc_bias";
        gcb_window_ok(fn, window); gcb_ready(c, fn);
        const uint64_t rows = (uint64_t)c->cov.n_rec + 1;
        if (cap_rows < rows) throw ScsError(SCS_EOVERFLOW, fn + ": " + std::to_string(rows) + " rows (the records and the genome), room for " + std::to_string(cap_rows));
        const GcbTables t = gcb_of_ctx(c, window);
        if (windows) std::copy(t.windows.begin(), t.windows.end(), windows);
        if (depth_sum) std::copy(t.depth_sum.begin(), t.depth_sum.end(), depth_sum);
        if (n_windows) std::copy(t.n_windows.begin(), t.n_windows.end(), n_windows);
    });
}

int scs_write_gc_bias(scs_ctx* c, const char* path, uint32_t window) {
    return guarded(c, [&] {
        const std::string fn = "scs_write_gc_bias";
        if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
        gcb_window_ok(fn, window); gcb_ready(c, fn);
        OutFile fd; fd.open(fn, path, false);              // (an unwritable path fails here, before any GPU work)
        const GcbTables t = gcb_of_ctx(c, window); const uint32_t nr = t.nr;
        auto name = [&](uint32_t r) { return r < nr ? c->recs[r].name.c_str() : "genome"; };
        std::vector<GcbRow> rows; for (uint32_t r = 0; r <= nr; ++r) rows.push_back(gcb_row(t.windows.data() + (size_t)r * GCB_BINS, t.depth_sum.data() + (size_t)r * GCB_BINS, window));
        std::string o;
        text_printf(o, "#gc_bias\twindow=%u\tstep=1\texcluded=windows_with_N\tbin=100*gc/window\n", window);
        o += "#summary\trecord\twindows\tn_windows\tmean_depth\n";
        for (uint32_t r = 0; r <= nr; ++r) { o += "#s\t"; o += name(r); text_printf(o, "\t%llu\t%llu\t%.6f\n", (unsigned long long)rows[r].n, (unsigned long long)t.n_windows[r], rows[r].row_mean); }
        o += "#record\tgc\twindows\tdepth_sum\tmean_depth\tnormalized\tmodel\n";
        for (uint32_t r = 0; r <= nr; ++r)
            for (uint32_t b = 0; b < GCB_BINS; ++b) {
                const uint64_t w = t.windows[(size_t)r * GCB_BINS + b];
                if (!w) continue;
                o += name(r);
                text_printf(o, "\t%u\t%llu\t%llu\t%.6f\t%.6f\t", b, (unsigned long long)w, (unsigned long long)t.depth_sum[(size_t)r * GCB_BINS + b], rows[r].mean[b], rows[r].normalized[b]);
                if (c->have_profile) text_printf(o, "%.6g\n", c->prof.gc_means[b]); else o += ".\n";   // (the value k_weights reads for an amplicon of this bin)
            }
        fd.write(o.data(), o.size());
        fd.finish();
    });
}

int scs_gc_bias_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_gcbias, launches, ms, units); }

// device test seam: the kernel alone, as the product launches it, over a caller's depths and codes of n_bases bases and records of
// rec_lens (adding up to n_bases), on the ctx's stream; the depths padded to whole tiles as the coverage profile's array is, nothing
// behind the codes.  lds < 0: the product's choice; 0: no LDS table.  n_records rows, no genome row; any output may be NULL
int scs_gc_bias_probe(scs_ctx* c, const uint32_t* depth, const uint8_t* codes, uint64_t n_bases, const uint64_t* rec_lens, uint32_t n_records, uint32_t window, int lds,
                      uint64_t* windows, uint64_t* depth_sum, uint64_t* n_windows) {
    return guarded(c, [&] {
        const std::string fn = "scs_gc_bias_probe";
        if (!depth || !codes || !n_bases || !rec_lens || !n_records) throw ScsError(SCS_EINVAL, fn + ": bad argument");
        gcb_window_ok(fn, window);
        const std::vector<uint64_t> roff = starts_of(std::vector<uint64_t>(rec_lens, rec_lens + n_records));
        if (roff[n_records] != n_bases) throw ScsError(SCS_EINVAL, fn + ": the records' lengths add up to " + std::to_string(roff[n_records]) + ", the arrays have " + std::to_string(n_bases) + " entries");
        const uint64_t nt = cov_tiles(n_bases);
        if (nt > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, fn + ": too many tiles");
        const hipStream_t s = c->stream; DevBuf d_depth, d_codes, d_rec, d_tab; const size_t padded = (size_t)nt * COV_TILE * 4;
        d_depth.plain = d_codes.plain = true;              // (arrays of a fixed size that live for this call: plain blocks, as CovRefTrack's)
        d_depth.reserve(padded, s); d_codes.reserve(std::max<size_t>(n_bases, 16), s); upload(d_rec, roff, s);
        HIP_OK(hipMemsetAsync(d_depth.p, 0, padded, s)); HIP_OK(hipMemcpyAsync(d_depth.p, depth, (size_t)n_bases * 4, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(d_codes.p, codes, n_bases, hipMemcpyHostToDevice, s));
        const GcbTables t = gcb_run(c, d_tab, d_depth.as<uint32_t>(), nt * COV_TILE, d_codes.as<uint8_t>(), n_bases, d_rec.as<uint64_t>(), n_records, window, lds < 0 ? 1u : (uint32_t)lds, false);
        if (windows) std::copy(t.windows.begin(), t.windows.end(), windows);
        if (depth_sum) std::copy(t.depth_sum.begin(), t.depth_sum.end(), depth_sum);
        if (n_windows) std::copy(t.n_windows.begin(), t.n_windows.end(), n_windows);
    });
}

}  // extern "C"
