// scs_coverage.cpp -- the coverage profile (include/scssim_hip.h: scs_set_coverage ...): the state of a ctx's
// profile (CovTrack, scs_ctx.h), its refusals, the buffers of a yield call, the end-of-job pass, read-out and file.  What a read
// marks and the file's summary are scs_coverage.h's; the kernels are scs_k_coverage.hip's, the per-batch one launched from
// scs_reads.cpp.  With it the profile on the original reference (scs_set_coverage_ref ...; CovRefTrack): the
// staged depths carried through the lift table at the end of the job (scs_k_coverage_ref.hip), with the same read-out and file.
// Either switch brings the staged array and its end-of-job pass; what a switch EXPOSES is its own (coverage_settle).
#include "scs_textout.h"

namespace scs {
namespace {

const char* const kLabel = "coverage profile (scs_set_coverage)";
const char* const kRefLabel = "coverage profile on the reference (scs_set_coverage_ref)";

void ready(const scs_ctx* c, const std::string& fn) {
    if (!c->cov.max_depth || !c->cov.valid) throw ScsError(SCS_EINVAL, fn + ": no yield call with the coverage profile on (scs_set_coverage) has finished");
}
void ref_ready(const scs_ctx* c, const std::string& fn) {
    if (!c->cov_ref.max_depth || !c->cov_ref.valid) throw ScsError(SCS_EINVAL, fn + ": no yield call with the coverage profile on the reference on (scs_set_coverage_ref) has finished");
}

// where the tables lie in CovTrack::tab and CovRefTrack::tab, in uint64 words: hist[n][D + 1], n_n [n], sum, sum_n [n]; ref: absent
// [n] behind n_n, and behind sum_n cn_bases, cn_sum [n][17] and unlifted
struct CovTab {
    size_t n, row, nc, nn, ab, sum, sumn, cnb, cns, unl, words;
    CovTab(uint32_t n_rec, uint32_t D, bool ref) : n(n_rec), row((size_t)D + 1), nc(ref ? COV_REF_CN + 1u : 0u), nn(n * row), ab(nn + n), sum(ab + (ref ? n : 0)), sumn(sum + n), cnb(sumn + n),
                                                    cns(cnb + n * nc), unl(cns + n * nc), words(unl + (ref ? 1 : 0)) {}
    size_t bytes() const { return std::max<size_t>(words * 8, 16); }
};
// a block of that layout on the host, n + 1 rows each (the genome's last); the staged track's has no absent, cn_bases, cn_sum
struct CovTables { uint32_t n, D; std::vector<uint64_t> hist, n_n, absent, sum, sum_n, cn_bases, cn_sum; uint64_t unlifted; };
CovTables cov_tables(const DevBuf& tab, uint32_t n_rec, uint32_t D, bool ref, hipStream_t s) {
    const CovTab t(n_rec, D, ref); const size_t n = t.n, xr = ref ? n + 1 : 0;
    std::vector<uint64_t> all(t.words);
    if (t.words) HIP_OK(hipMemcpyAsync(all.data(), tab.p, t.words * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    CovTables o{n_rec, D, std::vector<uint64_t>((n + 1) * t.row, 0), std::vector<uint64_t>(n + 1, 0), std::vector<uint64_t>(xr, 0), std::vector<uint64_t>(n + 1, 0), std::vector<uint64_t>(n + 1, 0),
                std::vector<uint64_t>(xr * t.nc, 0), std::vector<uint64_t>(xr * t.nc, 0), ref ? all[t.unl] : 0};
    std::copy(all.begin(), all.begin() + t.nn, o.hist.begin());
    std::copy(all.begin() + t.cnb, all.begin() + t.cns, o.cn_bases.begin()); std::copy(all.begin() + t.cns, all.begin() + t.unl, o.cn_sum.begin());
    for (size_t r = 0; r < n; ++r) {
        for (size_t k = 0; k < t.row; ++k) o.hist[n * t.row + k] += o.hist[r * t.row + k];
        for (size_t k = 0; k < t.nc; ++k) { o.cn_bases[n * t.nc + k] += o.cn_bases[r * t.nc + k]; o.cn_sum[n * t.nc + k] += o.cn_sum[r * t.nc + k]; }
        o.n_n[r] = all[t.nn + r]; o.sum[r] = all[t.sum + r]; o.sum_n[r] = all[t.sumn + r];
        o.n_n[n] += o.n_n[r]; o.sum[n] += o.sum[r]; o.sum_n[n] += o.sum_n[r];
        if (ref) { o.absent[r] = all[t.ab + r]; o.absent[n] += o.absent[r]; }
    }
    return o;
}
CovTables tables(scs_ctx* c) { return cov_tables(c->cov.tab, c->cov.n_rec, c->cov.max_depth, false, c->stream); }
CovTables ref_tables(scs_ctx* c) { return cov_tables(c->cov_ref.tab, c->cov_ref.n_ref, c->cov_ref.max_depth, true, c->stream); }
// the first `rows` rows of a block's tables to a caller's arrays, any of which may be NULL
void tables_out(const CovTables& t, size_t rows, uint64_t* hist, uint64_t* n_n, uint64_t* absent, uint64_t* sum, uint64_t* sum_n, uint64_t* cn_bases, uint64_t* cn_sum, uint64_t* unlifted) {
    const size_t row = (size_t)t.D + 1, nc = COV_REF_CN + 1u;
    if (hist) std::copy(t.hist.begin(), t.hist.begin() + rows * row, hist);
    if (n_n) std::copy(t.n_n.begin(), t.n_n.begin() + rows, n_n);
    if (absent) std::copy(t.absent.begin(), t.absent.begin() + rows, absent);
    if (sum) std::copy(t.sum.begin(), t.sum.begin() + rows, sum);
    if (sum_n) std::copy(t.sum_n.begin(), t.sum_n.begin() + rows, sum_n);
    if (cn_bases) std::copy(t.cn_bases.begin(), t.cn_bases.begin() + rows * nc, cn_bases);
    if (cn_sum) std::copy(t.cn_sum.begin(), t.cn_sum.begin() + rows * nc, cn_sum);
    if (unlifted) *unlifted = t.unlifted;
}

// T's arrays for records of the starts roff and max_depth D: reserved (an allocation failure states the bytes), the record starts
// uploaded (the caller waits before roff goes); nothing is zeroed here
void reserve(CovTrack& T, const std::vector<uint64_t>& roff, uint32_t D, hipStream_t s) {
    const uint32_t nr = (uint32_t)roff.size() - 1u;
    if (!nr) throw ScsError(SCS_EINVAL, std::string(kLabel) + ": no genome is staged");
    const uint64_t G = roff[nr], nt = cov_tiles(G);
    if (nt > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, std::string(kLabel) + ": the staged genome has more tiles than a grid holds");
    const size_t diff_bytes = (size_t)nt * COV_TILE * 4;
    try { T.diff.reserve(diff_bytes, s); }
    catch (const ScsError& e) { throw ScsError(e.code, std::string(kLabel) + ": the per-base array of " + std::to_string(G) + " + 1 entries needs " + std::to_string(diff_bytes) + " bytes of device memory: " + e.what()); }
    T.tab.reserve(CovTab(nr, D, false).bytes(), s); T.tiles.reserve((size_t)nt * 8, s);
    upload(T.rec, roff, s);
    T.bases = G; T.n_rec = nr; T.run_depth = D;
}
void zero(const CovTrack& T, hipStream_t s) {
    HIP_OK(hipMemsetAsync(T.diff.p, 0, (size_t)cov_tiles(T.bases) * COV_TILE * 4, s)); HIP_OK(hipMemsetAsync(T.tab.p, 0, CovTab(T.n_rec, T.run_depth, false).bytes(), s));
}
CovFinish args(const CovTrack& T, const uint8_t* codes, uint32_t lds, uint32_t* flags) {
    const CovTab t(T.n_rec, T.run_depth, false); unsigned long long* tab = T.tab.as<unsigned long long>(); const uint64_t nt = cov_tiles(T.bases);
    return CovFinish{T.diff.as<int32_t>(), codes, T.bases, T.rec.as<uint64_t>(), T.n_rec, T.run_depth, lds, T.tiles.as<int32_t>(), T.tiles.as<int32_t>() + nt, tab, tab + t.nn, tab + t.sum, tab + t.sumn, flags};
}

// ---- on the reference
// a table that could put more than COV_REF_MAX_COPIES staged bases on one reference base is refused: the packed word's 16 bits
// never wrap silently.  A sweep over the R segments' ends per reference record
void ref_copies_fit(const LiftSeg* segs, size_t n) {
    std::vector<std::pair<std::pair<uint32_t, uint64_t>, int>> ev; ev.reserve(2 * n);
    for (size_t i = 0; i < n; ++i) if (segs[i].kind == 0u && segs[i].len) { ev.push_back({{segs[i].ref_rec, segs[i].ref_pos}, 1}); ev.push_back({{segs[i].ref_rec, segs[i].ref_pos + segs[i].len}, -1}); }
    std::sort(ev.begin(), ev.end());                                               // (an end sorts before a start at the same coordinate)
    int64_t run = 0;
    for (const auto& e : ev) { run += e.second; if (run > (int64_t)COV_REF_MAX_COPIES) throw ScsError(SCS_EOVERFLOW, std::string(kRefLabel) + ": more than 65535 staged bases lift to one reference base (record " + std::to_string(e.first.first) + ", position " + std::to_string(e.first.second) + "); the per-base copies are 16 bits wide"); }
}
// R's arrays for reference records of these lengths and max_depth D, beside a staged array of `staged` bases: reserved (an
// allocation failure states the bytes), the record starts uploaded; nothing is zeroed here
void ref_reserve(CovRefTrack& R, const std::vector<uint64_t>& ref_lens, uint32_t D, uint64_t staged, hipStream_t s) {
    const uint32_t nf = (uint32_t)ref_lens.size();
    if (!nf) throw ScsError(SCS_EINVAL, std::string(kRefLabel) + ": the lift table names no reference record");
    const std::vector<uint64_t> roff = starts_of(ref_lens);
    const uint64_t nt = cov_ref_tiles(roff[nf]);
    if (nt > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, std::string(kRefLabel) + ": the reference has more tiles than a grid holds");
    const size_t arr = std::max<size_t>((size_t)nt * COV_TILE * 4, 16);
    try { R.depth.reserve(arr, s); R.packed.reserve(arr, s); }
    catch (const ScsError& e) {
        throw ScsError(e.code, std::string(kRefLabel) + ": the two per-base arrays of " + std::to_string(roff[nf]) + " reference bases need " + std::to_string(2 * arr) + " bytes of device memory (8 per reference base), beside " +
                       std::to_string((size_t)cov_tiles(staged) * COV_TILE * 4) + " bytes of the staged array (4 per staged base): " + e.what());
    }
    R.tab.reserve(CovTab(nf, D, true).words * 8, s);
    upload(R.rec, roff, s);
    R.n_ref = nf; R.bases = roff[nf];
    HIP_OK(hipStreamSynchronize(s));                                               // (the host table goes)
}
void ref_zero(const CovRefTrack& R, uint32_t D, bool packed_too, hipStream_t s) {
    const size_t arr = std::max<size_t>((size_t)cov_ref_tiles(R.bases) * COV_TILE * 4, 16);
    HIP_OK(hipMemsetAsync(R.depth.p, 0, arr, s)); HIP_OK(hipMemsetAsync(R.tab.p, 0, CovTab(R.n_ref, D, true).words * 8, s));
    if (packed_too) HIP_OK(hipMemsetAsync(R.packed.p, 0, arr, s));
}
CovRefArgs ref_args(const CovRefTrack& R, uint32_t D, const LiftSeg* segs, uint32_t n_seg, const uint32_t* depth, const uint8_t* codes, uint64_t staged, uint32_t lds, uint32_t* flags) {
    const CovTab t(R.n_ref, D, true); unsigned long long* tab = R.tab.as<unsigned long long>();
    return CovRefArgs{segs, n_seg, R.rec.as<uint64_t>(), R.n_ref, staged, R.bases, depth, codes, R.depth.as<uint32_t>(), R.packed.as<uint32_t>(), D, lds,
                      tab, tab + t.nn, tab + t.ab, tab + t.sum, tab + t.sumn, tab + t.cnb, tab + t.cns, tab + t.unl, flags};
}
// sum ref_depth + unlifted = sum staged depth, uint64 on both sides: the reads' aligned bases all arrived somewhere.  It is also
// the net under a uint32 wrap of one reference base's depth (many copies of a deep base): FLAG_COVERAGE's error
void ref_identity(const CovTables& t, uint64_t staged_sum) {
    const uint64_t got = t.sum[t.n] + t.sum_n[t.n] + t.unlifted;
    if (got != staged_sum) throw ScsError(SCS_EOVERFLOW, "device work buffer overflow: coverage profile (on the reference: the depths of the reference bases and of inserted sequence add up to " + std::to_string(got) +
                                          ", the staged depths to " + std::to_string(staged_sum) + " -- a reference base's depth passed 2^32 - 1, or the lift table does not cover the staged genome)");
}

// ---- the file of either profile: header, a summary line per record and the genome, (inserted: on the reference) the copy-number
// table and the unlifted line, the histogram's non-empty buckets
const char kCovHeader[] = "#coverage\tmax_depth=%u\tthe last bucket (depth %u) counts depth >= %u; gini takes it at its mean depth: exact when it is empty, a lower bound otherwise\n";
template <class Name>
void write_profile(const std::string& fn, const char* path, const CovTables& t, Name name, const uint64_t* inserted) {
    const bool ref = inserted != nullptr; const uint32_t n = t.n, D = t.D; const size_t row = (size_t)D + 1, nc = COV_REF_CN + 1u;
    OutFile fd; fd.open(fn, path, false);
    auto size = [&](uint32_t r) { uint64_t b = 0; for (size_t k = 0; k < row; ++k) b += t.hist[r * row + k]; return b; };   // the non-N bases (on the reference the absent ones among them)
    std::string o;
    text_printf(o, kCovHeader, D, D, D);
    o += "#summary\trecord\tbases\tn_bases\t"; if (ref) o += "absent\t"; o += "aligned\tmean\tbreadth1\tbreadth5\tbreadth10\tbreadth20\tgini\n";
    for (uint32_t r = 0; r <= n; ++r) {
        const CovStats s = cov_stats(t.hist.data() + r * row, D, t.sum[r]);
        o += "#s\t"; o += name(r); text_printf(o, "\t%llu\t%llu", (unsigned long long)(size(r) + t.n_n[r]), (unsigned long long)t.n_n[r]);
        if (ref) text_printf(o, "\t%llu", (unsigned long long)t.absent[r]);
        text_printf(o, "\t%llu\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\t%.10g\n", (unsigned long long)(t.sum[r] + t.sum_n[r]), s.mean, s.breadth[0], s.breadth[1], s.breadth[2], s.breadth[3], s.gini);
    }
    if (ref) {
        o += "#cn\trecord\tcopies\tbases\taligned\tmean\n";
        for (uint32_t r = 0; r <= n; ++r)
            for (size_t k = 0; k < nc; ++k) {
                const uint64_t b = t.cn_bases[r * nc + k], a = t.cn_sum[r * nc + k];
                if (b) { o += "#c\t"; o += name(r); text_printf(o, "\t%llu\t%llu\t%llu\t%.10g\n", (unsigned long long)k, (unsigned long long)b, (unsigned long long)a, (double)a / (double)b); }
            }
        text_printf(o, "#unlifted\t%llu\t%llu\n", (unsigned long long)t.unlifted, (unsigned long long)*inserted);
    }
    o += "#record\tdepth\tcount\tsize\tfraction\n";
    for (uint32_t r = 0; r <= n; ++r) {
        const uint64_t b = size(r);
        for (size_t k = 0; k < row; ++k) {
            const uint64_t h = t.hist[r * row + k];
            if (h) { o += name(r); text_printf(o, "\t%llu\t%llu\t%llu\t%.10g\n", (unsigned long long)k, (unsigned long long)h, (unsigned long long)b, (double)h / (double)b); }
        }
    }
    fd.write(o.data(), o.size());
    fd.finish();
}

// ---- The family's ownership rule, applied behind either setter (its new max_depth stored, the stream drained: nothing may
// still read what goes).  staged_changed: scs_set_coverage called, else scs_set_coverage_ref
//   the staged array (diff, rec, tiles), tm_cov_mark / tm_cov_finish and tm_runs: while either switch is on; the array is made
//     anew too where scs_set_coverage changes with the reference switch off
//   the bedGraph writer's buffers: released on every change of either switch (they only grow, to the largest array written so
//     far: kept, what a ctx holds in a state would depend on the way into it); the next write makes them again
//   cov.tab: released whenever cov.max_depth changes (the reference switch alone: the next call makes a private run_depth = 1 block)
//   the GC-bias table and tm_gcbias: while cov.max_depth is not 0
//   the reference arrays, their flags and tm_cov_ref_*: cov_ref.max_depth's alone, reset on every change of it
void coverage_settle(scs_ctx* c, bool staged_changed) {
    CovTrack& T = c->cov; CovRefTrack& R = c->cov_ref; const bool staged = T.max_depth != 0, ref = R.max_depth != 0;
    if (staged_changed) { T.tab.release(); T.valid = false; }
    else { R.depth.release(); R.packed.release(); R.tab.release(); R.rec.release(); R.valid = false; R.copies = false; R.bases = 0; R.n_ref = 0; R.unlifted = 0; }
    if (!ref) { c->tm_cov_ref_copies.drop(); c->tm_cov_ref_finish.drop(); }
    if (!staged) { c->gcb.release(); c->tm_gcbias.drop(); }
    if (!ref && (staged_changed || !staged)) { T.diff.release(); T.rec.release(); T.tiles.release(); T.bases = 0; T.n_rec = 0; }
    if (!ref && !staged) { T.tab.release(); c->tm_cov_mark.drop(); c->tm_cov_finish.drop(); c->tm_runs.drop(); }
    c->runs.release();
}
void set_switch(scs_ctx* c, const char* fn, uint32_t& slot, uint32_t max_depth, bool staged) {
    if (max_depth > COV_MAX_DEPTH) throw ScsError(SCS_EINVAL, std::string(fn) + ": max_depth is at most 65535 (0: off)");
    if (max_depth == slot) return;
    HIP_OK(hipStreamSynchronize(c->stream));
    slot = max_depth;
    coverage_settle(c, staged);
}

}  // namespace

void coverage_check(scs_ctx* c) {
    const bool sharded = c->cfg.shard_count > 1 || c->sliced;
    if (c->cov.max_depth && sharded) throw ScsError(SCS_EINVAL, std::string(kLabel) + ": not available for a sharded job (shard_count > 1); turn it off with scs_set_coverage(ctx, 0)");
    if (!c->cov_ref.max_depth) return;
    if (sharded) throw ScsError(SCS_EINVAL, std::string(kRefLabel) + ": not available for a sharded job (shard_count > 1); turn it off with scs_set_coverage_ref(ctx, 0)");
    if (!c->have_lift) throw ScsError(SCS_EINVAL, std::string(kRefLabel) + ": the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
}

void coverage_invalidate(scs_ctx* c, bool genome_changed) {
    c->cov_ref.valid = false; c->cov_ref.copies = false;
    if (genome_changed) { c->cov.valid = false; c->gcb.release(); }                // (the GC-bias table's rows were the last genome's records)
}

// This call's difference array and tables, zeroed on the ctx stream, and the kernels' record starts (nr + 1) and tile sums
void coverage_open(scs_ctx* c) {
    CovTrack& T = c->cov; const std::vector<uint64_t> roff = record_starts(c);
    reserve(T, roff, T.max_depth ? T.max_depth : 1u, c->stream);                   // (only the profile on the reference is on: any valid max_depth, the tables stay private)
    zero(T, c->stream);
    HIP_OK(hipStreamSynchronize(c->stream));                                       // (the host table goes)
}

// After the last batch: the differences become the depths, counted into the tables; the kernels' errors reach the call through the flags word
void coverage_finish(scs_ctx* c, uint32_t lds) {
    const hipStream_t s = c->stream;
    c->tm_cov_finish.begin(s);
    launch_cov_finish(s, args(c->cov, c->genome.as<uint8_t>(), lds, c->flags.as<uint32_t>()));
    c->tm_cov_finish.end(s); c->tm_cov_finish.add_units(c->cov.bases);
}

// The call's reference array and tables, zeroed on the ctx stream; the packed copies where the genome or the table is new (the
// staged array is open: coverage_open has run)
void coverage_ref_open(scs_ctx* c) {
    CovRefTrack& R = c->cov_ref; const hipStream_t s = c->stream;
    need_lift(c, "scs_set_coverage_ref");
    if (c->lift.total() != c->cov.bases) throw ScsError(SCS_EINVAL, std::string(kRefLabel) + ": the lift table covers " + std::to_string(c->lift.total()) + " staged bases, " + std::to_string(c->cov.bases) + " are staged");
    if (!R.copies) ref_copies_fit(c->lift.segs.data(), c->lift.segs.size());
    ref_reserve(R, c->lift.ref_lens, R.max_depth, c->cov.bases, s);
    ref_zero(R, R.max_depth, !R.copies, s);
    if (!R.copies) {
        c->tm_cov_ref_copies.begin(s);
        launch_cov_ref_copies(s, ref_args(R, R.max_depth, c->d_lift.as<LiftSeg>(), (uint32_t)c->lift.segs.size(), nullptr, c->genome.as<uint8_t>(), c->cov.bases, 0, c->flags.as<uint32_t>()));
        c->tm_cov_ref_copies.end(s); c->tm_cov_ref_copies.add_units(c->cov.bases);
    }
    HIP_OK(hipStreamSynchronize(s));                                               // (the host table goes)
    if (!R.copies) { check_flags(c); R.copies = true; }
}

// After coverage_finish: the staged depths lie where their differences lay
void coverage_ref_finish(scs_ctx* c, uint32_t lds) {
    CovRefTrack& R = c->cov_ref; const hipStream_t s = c->stream;
    c->tm_cov_ref_finish.begin(s);
    launch_cov_ref_finish(s, ref_args(R, R.max_depth, c->d_lift.as<LiftSeg>(), (uint32_t)c->lift.segs.size(), c->cov.diff.as<uint32_t>(), c->genome.as<uint8_t>(), c->cov.bases, lds, c->flags.as<uint32_t>()));
    c->tm_cov_ref_finish.end(s); c->tm_cov_ref_finish.add_units(c->cov.bases);
}

void coverage_ref_close(scs_ctx* c) {
    const CovTrack& T = c->cov; const CovTab w(T.n_rec, T.run_depth, false);
    std::vector<uint64_t> st(2 * w.n);
    if (w.n) HIP_OK(hipMemcpyAsync(st.data(), T.tab.as<uint64_t>() + w.sum, st.size() * 8, hipMemcpyDeviceToHost, c->stream));   // the staged pass' sum and sum_n
    const CovTables t = ref_tables(c);                                             // (synchronises)
    uint64_t staged = 0; for (uint64_t v : st) staged += v;
    ref_identity(t, staged);
    c->cov_ref.unlifted = t.unlifted;
}

}  // namespace scs

extern "C" {

int scs_set_coverage(scs_ctx* c, uint32_t max_depth) {
    return guarded(c, [&] { set_switch(c, "scs_set_coverage", c->cov.max_depth, max_depth, true); });
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
        tables_out(tables(c), rows, hist, n_bases, nullptr, sum, sum_n, nullptr, nullptr, nullptr);
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
        const CovTables t = tables(c);
        write_profile(fn, path, t, [&](uint32_t r) { return r < t.n ? c->recs[r].name.c_str() : "genome"; }, nullptr);
    });
}

int scs_write_coverage_bedgraph(scs_ctx* c, const char* path, uint64_t* lines, uint64_t* text_bytes) {
    return guarded(c, [&] {
        const std::string fn = "scs_write_coverage_bedgraph";
        if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
        ready(c, fn);
        std::vector<std::string> names; for (const FastaRecord& r : c->recs) names.push_back(r.name);
        runs_write_file(c, fn, path, c->cov.diff.as<uint32_t>(), 0xFFFFFFFFu, c->cov.bases, record_starts(c), names, lines, text_bytes);
    });
}

int scs_coverage_kernel_time(const scs_ctx* c, int which, uint64_t* launches, double* ms, uint64_t* units) {
    if (which != 0 && which != 1) return SCS_EINVAL;
    return kernel_time_of(c, which ? &scs_ctx::tm_cov_finish : &scs_ctx::tm_cov_mark, launches, ms, units);
}

// ---- on the reference
int scs_set_coverage_ref(scs_ctx* c, uint32_t max_depth) {
    return guarded(c, [&] { set_switch(c, "scs_set_coverage_ref", c->cov_ref.max_depth, max_depth, false); });
}

int scs_coverage_ref_shape(const scs_ctx* c, uint32_t* ref_records, uint32_t* max_depth) {
    if (!c) return SCS_EINVAL;
    if (!c->cov_ref.max_depth || !c->have_lift) { const_cast<scs_ctx*>(c)->err = "scs_coverage_ref_shape: the coverage profile on the reference is off (scs_set_coverage_ref), or the staged genome has no lift table (scs_simuvars, scs_load_lift)"; return SCS_EINVAL; }
    if (ref_records) *ref_records = (uint32_t)c->lift.ref_lens.size();
    if (max_depth) *max_depth = c->cov_ref.max_depth;
    return SCS_OK;
}

int scs_download_coverage_ref(scs_ctx* c, uint64_t* hist, uint64_t* n_bases, uint64_t* absent, uint64_t* sum, uint64_t* sum_n, uint64_t* cn_bases, uint64_t* cn_sum, uint64_t* unlifted, uint64_t cap_rows) {
    return guarded(c, [&] {
        ref_ready(c, "scs_download_coverage_ref");
        const uint64_t rows = (uint64_t)c->cov_ref.n_ref + 1;
        if (cap_rows < rows) throw ScsError(SCS_EOVERFLOW, "scs_download_coverage_ref: " + std::to_string(rows) + " rows (the reference records and the genome), room for " + std::to_string(cap_rows));
        tables_out(ref_tables(c), rows, hist, n_bases, absent, sum, sum_n, cn_bases, cn_sum, unlifted);
    });
}

int scs_coverage_ref_range(scs_ctx* c, uint32_t ref_record, uint64_t start, uint64_t end, uint32_t* depth_out, uint32_t* copies_out) {
    return guarded(c, [&] {
        ref_ready(c, "scs_coverage_ref_range"); need_lift(c, "scs_coverage_ref_range");
        const std::vector<uint64_t>& lens = c->lift.ref_lens;
        if (ref_record >= c->cov_ref.n_ref || ref_record >= lens.size() || start > end || end > lens[ref_record])
            throw ScsError(SCS_EINVAL, "scs_coverage_ref_range: [" + std::to_string(start) + ", " + std::to_string(end) + ") of reference record " + std::to_string(ref_record) + " is not inside a reference record");
        const uint64_t off = starts_of(lens)[ref_record] + start;
        const size_t n = (size_t)(end - start);
        if (n && depth_out) HIP_OK(hipMemcpyAsync(depth_out, c->cov_ref.depth.as<uint32_t>() + off, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (n && copies_out) HIP_OK(hipMemcpyAsync(copies_out, c->cov_ref.packed.as<uint32_t>() + off, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (copies_out) for (size_t i = 0; i < n; ++i) copies_out[i] &= 0xFFFFu;      // (the packed word's other half counts the N copies)
    });
}

int scs_write_coverage_ref(scs_ctx* c, const char* path) {
    return guarded(c, [&] {
        const std::string fn = "scs_write_coverage_ref";
        if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
        ref_ready(c, fn); need_lift(c, fn.c_str());
        const CovTables t = ref_tables(c);
        uint64_t inserted = 0; for (const LiftSeg& sg : c->lift.segs) if (sg.kind != 0u) inserted += sg.len;
        write_profile(fn, path, t, [&](uint32_t r) { return r < t.n ? c->lift.ref_names[r].c_str() : "genome"; }, &inserted);
    });
}

// the reference's two per-base arrays as bedGraph: the depths, or (copies) the packed word's lower half
static void write_ref_bedgraph(scs_ctx* c, const std::string& fn, const char* path, bool copies, uint64_t* lines, uint64_t* text_bytes) {
    if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
    ref_ready(c, fn); need_lift(c, fn.c_str());
    const CovRefTrack& R = c->cov_ref; const std::vector<uint64_t>& lens = c->lift.ref_lens; const std::vector<uint64_t> roff = starts_of(lens);
    if (lens.size() != R.n_ref || roff[lens.size()] != R.bases || c->lift.ref_names.size() != lens.size()) throw ScsError(SCS_EINVAL, fn + ": the lift table is not the one the arrays were made with");
    runs_write_file(c, fn, path, copies ? R.packed.as<uint32_t>() : R.depth.as<uint32_t>(), copies ? 0xFFFFu : 0xFFFFFFFFu, R.bases, roff, c->lift.ref_names, lines, text_bytes);
}

int scs_write_coverage_ref_bedgraph(scs_ctx* c, const char* path, uint64_t* lines, uint64_t* text_bytes) {
    return guarded(c, [&] { write_ref_bedgraph(c, "scs_write_coverage_ref_bedgraph", path, false, lines, text_bytes); });
}

int scs_write_copy_number_ref(scs_ctx* c, const char* path, uint64_t* lines, uint64_t* text_bytes) {
    return guarded(c, [&] { write_ref_bedgraph(c, "scs_write_copy_number_ref", path, true, lines, text_bytes); });
}

int scs_coverage_ref_kernel_time(const scs_ctx* c, int which, uint64_t* launches, double* ms, uint64_t* units) {
    if (which != 0 && which != 1) return SCS_EINVAL;
    return kernel_time_of(c, which ? &scs_ctx::tm_cov_ref_finish : &scs_ctx::tm_cov_ref_copies, launches, ms, units);
}

// device test seam: the end-of-job kernels of the coverage profile alone (launch_cov_finish, scs_k_coverage.hip) over a given
// difference array diff[n_bases + 1], the bases' codes[n_bases] (0 .. 3, 4: N) and records of rec_lens (they add up to n_bases), on
// the ctx's stream and flags word, in a CovTrack of its own through the yield call's reserve / zero / args; lds_buckets < 0: the
// product's.  depth[n_bases], hist[n_records][max_depth + 1], n_n / sum / sum_n[n_records]; any output may be NULL.  Differences
// that are not those of intervals: the flag's error (SCS_EOVERFLOW)
int scs_coverage_finish_probe(scs_ctx* c, const int32_t* diff, const uint8_t* codes, uint64_t n_bases, const uint64_t* rec_lens, uint32_t n_records, uint32_t max_depth, int lds_buckets,
                              uint32_t* depth, uint64_t* hist, uint64_t* n_n, uint64_t* sum, uint64_t* sum_n) {
    return guarded(c, [&] {
        if (!diff || (n_bases && !codes) || !rec_lens || !n_records || max_depth < 1u || max_depth > COV_MAX_DEPTH) throw ScsError(SCS_EINVAL, "scs_coverage_finish_probe: bad argument");
        const std::vector<uint64_t> roff = starts_of(std::vector<uint64_t>(rec_lens, rec_lens + n_records));
        if (roff[n_records] != n_bases) throw ScsError(SCS_EINVAL, "scs_coverage_finish_probe: the records do not add up to n_bases");
        if (cov_tiles(n_bases) > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, "scs_coverage_finish_probe: too many tiles");
        const hipStream_t s = c->stream; CovTrack T; DevBuf d_codes;
        reserve(T, roff, max_depth, s); d_codes.reserve(std::max<size_t>(n_bases, 16), s);
        zero(T, s);
        HIP_OK(hipMemcpyAsync(T.diff.p, diff, (size_t)(n_bases + 1) * 4, hipMemcpyHostToDevice, s));
        if (n_bases) HIP_OK(hipMemcpyAsync(d_codes.p, codes, n_bases, hipMemcpyHostToDevice, s));
        launch_cov_finish(s, args(T, d_codes.as<uint8_t>(), lds_buckets < 0 ? COV_LDS_BUCKETS : (uint32_t)lds_buckets, c->flags.as<uint32_t>()));
        check_flags(c);                                                            // (waits for the kernels; the flag's error where the differences are inconsistent)
        if (depth && n_bases) HIP_OK(hipMemcpyAsync(depth, T.diff.p, (size_t)n_bases * 4, hipMemcpyDeviceToHost, s));
        tables_out(cov_tables(T.tab, n_records, max_depth, false, s), n_records, hist, n_n, nullptr, sum, sum_n, nullptr, nullptr, nullptr);   // (synchronises)
    });
}

// device test seam: the kernels of the profile on the reference alone (launch_cov_ref_copies, launch_cov_ref_finish: what the
// product launches) over a caller's staged depths, codes and table, on the ctx's stream and flags word.  Rows are the reference
// records' (no genome row); any output may be NULL
int scs_coverage_ref_finish_probe(scs_ctx* c, const uint32_t* depth, const uint8_t* codes, uint64_t n_staged,
                                  const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                                  const uint64_t* hap_lens, uint32_t n_hap, const uint64_t* ref_lens, uint32_t n_ref, uint32_t max_depth, int lds_buckets,
                                  uint32_t* ref_depth, uint32_t* packed, uint64_t* hist, uint64_t* n_n, uint64_t* absent, uint64_t* sum, uint64_t* sum_n, uint64_t* cn_bases, uint64_t* cn_sum, uint64_t* unlifted) {
    return guarded(c, [&] {
        const std::string fn = "scs_coverage_ref_finish_probe";
        if (!depth || !codes || !n_staged || !n_seg || !seg_hap_off || !seg_len || !seg_ref_pos || !seg_ref_rec || !seg_kind || !hap_lens || !n_hap || !ref_lens || !n_ref || max_depth < 1u || max_depth > COV_MAX_DEPTH)
            throw ScsError(SCS_EINVAL, fn + ": bad argument");
        // the table as lift_parse leaves it: segments that ascend, tile the staged genome and straddle no staged record.  Where a
        // segment lifts to is the kernels' to check
        std::vector<LiftSeg> segs(n_seg); uint64_t at = 0, rec_end = 0; uint32_t rec = 0;
        for (uint32_t i = 0; i < n_seg; ++i) {
            segs[i] = LiftSeg{seg_hap_off[i], seg_len[i], seg_ref_pos[i], seg_ref_rec[i], seg_kind[i]};
            while (rec < n_hap && at == rec_end) rec_end += hap_lens[rec++];
            if (seg_hap_off[i] != at || !seg_len[i] || seg_len[i] > rec_end - at || seg_kind[i] > 1u) throw ScsError(SCS_EINVAL, fn + ": the segments do not tile the staged records");
            at += seg_len[i];
        }
        while (rec < n_hap && at == rec_end) rec_end += hap_lens[rec++];
        if (at != n_staged || rec != n_hap || rec_end != n_staged) throw ScsError(SCS_EINVAL, fn + ": the segments do not tile the staged records");
        ref_copies_fit(segs.data(), segs.size());
        const hipStream_t s = c->stream; CovRefTrack R; DevBuf d_depth, d_codes, d_segs;
        ref_reserve(R, std::vector<uint64_t>(ref_lens, ref_lens + n_ref), max_depth, n_staged, s);
        d_depth.reserve((size_t)n_staged * 4, s); d_codes.reserve(std::max<size_t>(n_staged, 16), s); upload(d_segs, segs, s);
        HIP_OK(hipMemcpyAsync(d_depth.p, depth, (size_t)n_staged * 4, hipMemcpyHostToDevice, s)); HIP_OK(hipMemcpyAsync(d_codes.p, codes, n_staged, hipMemcpyHostToDevice, s));
        ref_zero(R, max_depth, true, s);
        const CovRefArgs a = ref_args(R, max_depth, d_segs.as<LiftSeg>(), n_seg, d_depth.as<uint32_t>(), d_codes.as<uint8_t>(), n_staged, lds_buckets < 0 ? COV_LDS_BUCKETS : (uint32_t)lds_buckets, c->flags.as<uint32_t>());
        launch_cov_ref_copies(s, a);
        launch_cov_ref_finish(s, a);
        check_flags(c);                                                            // (waits for the kernels; FLAG_LIFT's error where a segment lifts outside its reference record)
        const CovTables t = cov_tables(R.tab, n_ref, max_depth, true, s);
        uint64_t staged = 0; for (uint64_t i = 0; i < n_staged; ++i) staged += depth[i];
        ref_identity(t, staged);
        if (ref_depth && R.bases) HIP_OK(hipMemcpyAsync(ref_depth, R.depth.p, (size_t)R.bases * 4, hipMemcpyDeviceToHost, s));
        if (packed && R.bases) HIP_OK(hipMemcpyAsync(packed, R.packed.p, (size_t)R.bases * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        tables_out(t, n_ref, hist, n_n, absent, sum, sum_n, cn_bases, cn_sum, unlifted);
    });
}

}  // extern "C"
