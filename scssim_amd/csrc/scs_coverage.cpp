// scs_coverage.cpp -- the coverage profile (include/scssim_hip.h: scs_set_coverage ...): the state of a ctx's
// profile (CovTrack, scs_ctx.h), its refusals, the buffers of a yield call, the end-of-job pass, read-out and file.  What a read
// marks and the file's summary are scs_coverage.h's; the kernels are scs_k_coverage.hip's, the per-batch one launched from
// scs_reads.cpp.
#include "scs_textout.h"
#include <cerrno>

namespace scs {
namespace {

const char* const kLabel = "coverage profile (scs_set_coverage)";

void ready(const scs_ctx* c, const std::string& fn) {
    if (!c->cov.max_depth || !c->cov.valid) throw ScsError(SCS_EINVAL, fn + ": no yield call with the coverage profile on (scs_set_coverage) has finished");
}
// the last call's tables on the host: hist (n_rec + 1 rows of D + 1, the genome's last), n_bases, sum, sum_n (n_rec + 1 each)
struct CovTables { uint32_t nr, D; std::vector<uint64_t> hist, n_n, sum, sum_n; };
CovTables tables(scs_ctx* c) {
    const CovTrack& T = c->cov; const uint32_t nr = T.n_rec, D = T.max_depth; const size_t row = (size_t)D + 1, nh = (size_t)nr * row;
    std::vector<uint64_t> all(nh + 3 * (size_t)nr);
    if (!all.empty()) HIP_OK(hipMemcpyAsync(all.data(), T.tab.p, all.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    CovTables t{nr, D, std::vector<uint64_t>(nh + row, 0), std::vector<uint64_t>(nr + 1, 0), std::vector<uint64_t>(nr + 1, 0), std::vector<uint64_t>(nr + 1, 0)};
    std::copy(all.begin(), all.begin() + nh, t.hist.begin());
    for (uint32_t r = 0; r < nr; ++r) {
        for (size_t k = 0; k < row; ++k) t.hist[nh + k] += t.hist[r * row + k];
        t.n_n[r] = all[nh + r]; t.sum[r] = all[nh + nr + r]; t.sum_n[r] = all[nh + 2 * (size_t)nr + r];
        t.n_n[nr] += t.n_n[r]; t.sum[nr] += t.sum[r]; t.sum_n[nr] += t.sum_n[r];
    }
    return t;
}

}  // namespace

void coverage_check(scs_ctx* c) {
    if (!c->cov.max_depth) return;
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, std::string(kLabel) + ": not available for a sharded job (shard_count > 1); turn it off with scs_set_coverage(ctx, 0)");
}

// This call's difference array and tables, zeroed on the ctx stream, and the kernels' record starts (nr + 1) and tile sums
void coverage_open(scs_ctx* c) {
    CovTrack& T = c->cov; const hipStream_t s = c->stream;
    const std::vector<uint64_t> roff = record_starts(c); const uint32_t nr = (uint32_t)c->recs.size(), D = T.max_depth;
    if (!nr) throw ScsError(SCS_EINVAL, std::string(kLabel) + ": no genome is staged");
    const uint64_t G = roff[nr], nt = cov_tiles(G);
    if (nt > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, std::string(kLabel) + ": the staged genome has more tiles than a grid holds");
    const size_t diff_bytes = (size_t)nt * COV_TILE * 4, tab_bytes = ((size_t)nr * ((size_t)D + 1) + 3 * (size_t)nr) * 8;
    try { T.diff.reserve(diff_bytes, s); }
    catch (const ScsError& e) { throw ScsError(e.code, std::string(kLabel) + ": the per-base array of " + std::to_string(G) + " + 1 entries needs " + std::to_string(diff_bytes) + " bytes of device memory: " + e.what()); }
    T.tab.reserve(std::max<size_t>(tab_bytes, 16), s); T.tiles.reserve((size_t)nt * 8, s);
    upload(T.rec, roff, s);
    HIP_OK(hipMemsetAsync(T.diff.p, 0, diff_bytes, s)); HIP_OK(hipMemsetAsync(T.tab.p, 0, std::max<size_t>(tab_bytes, 16), s));
    T.bases = G; T.n_rec = nr;
    HIP_OK(hipStreamSynchronize(s));                                               // (the host table goes)
}

// After the last batch: the differences become the depths, counted into the tables; the kernels' errors reach the call through the flags word
void coverage_finish(scs_ctx* c, uint32_t lds) {
    CovTrack& T = c->cov; const hipStream_t s = c->stream; const uint32_t nr = T.n_rec, D = T.max_depth; const uint64_t nt = cov_tiles(T.bases);
    unsigned long long* tab = T.tab.as<unsigned long long>(); const size_t nh = (size_t)nr * ((size_t)D + 1);
    const CovFinish f{T.diff.as<int32_t>(), c->genome.as<uint8_t>(), T.bases, T.rec.as<uint64_t>(), nr, D, lds, T.tiles.as<int32_t>(), T.tiles.as<int32_t>() + nt,
                      tab, tab + nh, tab + nh + nr, tab + nh + 2 * (size_t)nr, c->flags.as<uint32_t>()};
    c->tm_cov_finish.begin(s);
    launch_cov_finish(s, f);
    c->tm_cov_finish.end(s); c->tm_cov_finish.add_units(T.bases);
}

}  // namespace scs

extern "C" {

int scs_set_coverage(scs_ctx* c, uint32_t max_depth) {
    return guarded(c, [&] {
        if (max_depth > COV_MAX_DEPTH) throw ScsError(SCS_EINVAL, "scs_set_coverage: max_depth is at most 65535 (0: off)");
        CovTrack& T = c->cov;
        if (max_depth == T.max_depth) return;
        HIP_OK(hipStreamSynchronize(c->stream));                                   // the last call's arrays go: nothing may still read them
        T.diff.release(); T.tab.release(); T.rec.release(); T.tiles.release(); T.valid = false; T.bases = 0; T.n_rec = 0; T.max_depth = max_depth;
        if (!max_depth) for (KernelTimer* t : {&c->tm_cov_mark, &c->tm_cov_finish}) { t->ev.clear(); t->used = 0; t->reset(); }
    });
}

int scs_coverage_shape(const scs_ctx* c, uint32_t* records, uint32_t* max_depth) {
    if (!c) return SCS_EINVAL;
    if (!c->cov.max_depth || !c->have_genome) { const_cast<scs_ctx*>(c)->err = "scs_coverage_shape: the coverage profile is off (scs_set_coverage), or no genome is staged"; return SCS_EINVAL; }
    if (records) *records = (uint32_t)c->recs.size();
    if (max_depth) *max_depth = c->cov.max_depth;
    return SCS_OK;
}

int scs_download_coverage(scs_ctx* c, uint64_t* hist, uint64_t* n_bases, uint64_t* sum, uint64_t* sum_n, uint64_t cap_rows) {
    return guarded(c, [&] {
        ready(c, "scs_download_coverage");
        const uint64_t rows = (uint64_t)c->cov.n_rec + 1;
        if (cap_rows < rows) throw ScsError(SCS_EOVERFLOW, "scs_download_coverage: " + std::to_string(rows) + " rows (the records and the genome), room for " + std::to_string(cap_rows));
        const CovTables t = tables(c);
        if (hist) std::copy(t.hist.begin(), t.hist.end(), hist);
        if (n_bases) std::copy(t.n_n.begin(), t.n_n.end(), n_bases);
        if (sum) std::copy(t.sum.begin(), t.sum.end(), sum);
        if (sum_n) std::copy(t.sum_n.begin(), t.sum_n.end(), sum_n);
    });
}

int scs_coverage_range(scs_ctx* c, uint32_t record, uint64_t start, uint64_t end, uint32_t* out) {
    return guarded(c, [&] {
        ready(c, "scs_coverage_range");
        if (record >= c->cov.n_rec || record >= c->rec_len.size() || start > end || end > c->rec_len[record])
            throw ScsError(SCS_EINVAL, "scs_coverage_range: [" + std::to_string(start) + ", " + std::to_string(end) + ") of record " + std::to_string(record) + " is not inside a staged record");
        if (end > start && !out) throw ScsError(SCS_EINVAL, "scs_coverage_range: no output array");
        if (end > start) HIP_OK(hipMemcpyAsync(out, c->cov.diff.as<uint32_t>() + c->rec_off[record] + start, (size_t)(end - start) * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    });
}

int scs_write_coverage(scs_ctx* c, const char* path) {
    return guarded(c, [&] {
        const std::string fn = "scs_write_coverage";
        if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
        ready(c, fn);
        const CovTables t = tables(c); const uint32_t nr = t.nr, D = t.D; const size_t row = (size_t)D + 1;
        FILE* o = fopen(path, "w");
        if (!o) throw ScsError(SCS_EIO, fn + ": can not open " + path + ": " + strerror(errno));
        auto name = [&](uint32_t r) { return r < nr ? c->recs[r].name.c_str() : "genome"; };
        auto size = [&](uint32_t r) { uint64_t n = 0; for (size_t k = 0; k < row; ++k) n += t.hist[r * row + k]; return n; };   // the non-N bases
        bool okw = fprintf(o, "#coverage\tmax_depth=%u\tthe last bucket (depth %u) counts depth >= %u; gini takes it at its mean depth: exact when it is empty, a lower bound otherwise\n", D, D, D) > 0 &&
                   fputs("#summary\trecord\tbases\tn_bases\taligned\tmean\tbreadth1\tbreadth5\tbreadth10\tbreadth20\tgini\n", o) != EOF;
        for (uint32_t r = 0; r <= nr && okw; ++r) {
            const CovStats s = cov_stats(t.hist.data() + r * row, D, t.sum[r]);
            okw = fprintf(o, "#s\t%s\t%llu\t%llu\t%llu\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\n", name(r), (unsigned long long)(size(r) + t.n_n[r]), (unsigned long long)t.n_n[r],
                          (unsigned long long)(t.sum[r] + t.sum_n[r]), s.mean, s.breadth[0], s.breadth[1], s.breadth[2], s.breadth[3], s.gini) > 0;
        }
        if (okw) okw = fputs("#record\tdepth\tcount\tsize\tfraction\n", o) != EOF;
        for (uint32_t r = 0; r <= nr && okw; ++r) {
            const uint64_t n = size(r);
            for (size_t k = 0; k < row && okw; ++k)
                if (t.hist[r * row + k]) okw = fprintf(o, "%s\t%llu\t%llu\t%llu\t%.10g\n", name(r), (unsigned long long)k, (unsigned long long)t.hist[r * row + k], (unsigned long long)n, (double)t.hist[r * row + k] / (double)n) > 0;
        }
        if (fclose(o) != 0 || !okw) throw ScsError(SCS_EIO, fn + ": writing " + path + " failed");
    });
}

int scs_coverage_kernel_time(const scs_ctx* c, int which, uint64_t* launches, double* ms, uint64_t* units) {
    if (which != 0 && which != 1) return SCS_EINVAL;
    return kernel_time_of(c, which ? &scs_ctx::tm_cov_finish : &scs_ctx::tm_cov_mark, launches, ms, units);
}

}  // extern "C"
