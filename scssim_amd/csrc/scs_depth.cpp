// scs_depth.cpp -- the two depth tracks (include/scssim_hip.h): per bin of the staged genome (scs_set_depth ...; DESIGN.md section
// 12) and per bin of the original reference, through the lift table (scs_set_depth_ref ...).  One definition
// of a track's state (DepthTrack, scs_ctx.h), refusals, layout, tables and counters, read-out and file; what differs between the
// two is DepthKind.  The bins and what a read adds to them are scs_depth.h's and scs_lift.h's; the per-batch kernels are launched
// from scs_reads.cpp.
#include "scs_textout.h"
#include <cerrno>

namespace scs {
namespace {

struct DepthKind {
    bool on_ref;               // by reference bin: needs the lift table; a third counter plane (copies), a pseudo-bin behind the bins and an "#unlifted" line
    const char* set_fn;        // what the messages name: the switch,
    const char* feature;       // the feature,
    const char* axis;          // what the bins cut,
    const char* recs;          // and its records
    DepthTrack& track(scs_ctx* c) const { return on_ref ? c->depth_ref : c->depth; }
    const DepthTrack& track(const scs_ctx* c) const { return on_ref ? c->depth_ref : c->depth; }
    const std::vector<uint64_t>& lens(const scs_ctx* c) const { return on_ref ? c->lift.ref_lens : c->rec_len; }
    const std::string& name(const scs_ctx* c, size_t r) const { return on_ref ? c->lift.ref_names[r] : c->recs[r].name; }
    std::string label() const { return std::string(feature) + " (" + set_fn + ")"; }
    int planes() const { return on_ref ? 3 : 2; }
    uint64_t entries(const DepthTrack& T) const { return T.bins + (on_ref ? 1u : 0u); }   // of one counter plane
};
const DepthKind kHap{false, "scs_set_depth", "depth track", "the staged genome", "records"};
const DepthKind kRef{true, "scs_set_depth_ref", "depth by reference bin", "the reference", "reference records"};

void check(scs_ctx* c, const DepthKind& K) {
    if (!K.track(c).width) return;
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, K.label() + ": not available for a sharded job (shard_count > 1); turn it off with " + K.set_fn + "(ctx, 0)");
    if (K.on_ref && !c->have_lift) throw ScsError(SCS_EINVAL, K.label() + ": the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
}
// the records' bins (SCS_EINVAL: no lift table, or beyond DEPTH_MAX_BINS); bin_off: every record's first bin, n + 1 entries
uint64_t layout(const scs_ctx* c, const DepthKind& K, std::vector<uint64_t>* bin_off) {
    if (K.on_ref && !c->have_lift) throw ScsError(SCS_EINVAL, K.label() + ": the staged genome has no lift table (scs_simuvars, scs_load_lift)");
    const std::vector<uint64_t>& lens = K.lens(c); const uint32_t w = K.track(c).width; const size_t nr = lens.size(); uint64_t nb = 0; uint32_t min_w = 0;
    if (bin_off) bin_off->assign(nr + 1, 0);
    if (depth_layout(lens.data(), nr, w, bin_off ? bin_off->data() : nullptr, &nb, &min_w)) return nb;
    throw ScsError(SCS_EINVAL, K.label() + ": bins of " + std::to_string(w) + " bases give more than 2^27 bins for " + K.axis + "; " +
                   (min_w ? "the smallest bin width it admits is " + std::to_string(min_w) : std::string("no bin width below 2^32 is enough")));
}
void ready(const scs_ctx* c, const DepthKind& K, const std::string& fn) {
    const DepthTrack& T = K.track(c);
    if (!T.width || !T.valid) throw ScsError(SCS_EINVAL, fn + ": no yield call with the " + K.feature + " on (" + K.set_fn + ") has finished");
}
// the entry points that take a const ctx: the error text is the only thing written
template <class F> int answered(const scs_ctx* c, F f) {
    try { f(); return SCS_OK; } catch (const ScsError& e) { const_cast<scs_ctx*>(c)->err = e.what(); return e.code; }
}

int set_width(scs_ctx* c, const DepthKind& K, uint32_t bin_width) {
    return guarded(c, [&] {
        DepthTrack& T = K.track(c);
        if (bin_width == T.width) return;
        HIP_OK(hipStreamSynchronize(c->stream));                                   // the last call's counters go: nothing may still read them
        T.cnt.release(); T.tab.release(); T.valid = false; T.bins = 0; T.width = bin_width;
        if (K.on_ref) c->dref_copies = false;
        if (K.on_ref && !bin_width) { c->tm_depth_ref.ev.clear(); c->tm_depth_ref.used = 0; c->tm_depth_ref.reset(); }
    });
}
int bins(const scs_ctx* c, const DepthKind& K, const std::string& fn, uint64_t* n_bins, uint32_t* bin_width) {
    if (!c) return SCS_EINVAL;
    return answered(c, [&] {
        if (!K.track(c).width) throw ScsError(SCS_EINVAL, fn + ": the " + K.feature + " is off (" + K.set_fn + ")");
        if (!K.on_ref && !c->have_genome) throw ScsError(SCS_EINVAL, fn + ": no genome is staged");
        const uint64_t nb = layout(c, K, nullptr);
        if (n_bins) *n_bins = nb; if (bin_width) *bin_width = K.track(c).width;
    });
}
int record_bins(const scs_ctx* c, const DepthKind& K, const std::string& fn, uint64_t* bin_off, uint64_t cap) {
    if (!c || !bin_off) return SCS_EINVAL;
    return answered(c, [&] {
        if (K.on_ref) { if (!K.track(c).width) throw ScsError(SCS_EINVAL, fn + ": the " + K.feature + " is off (" + K.set_fn + ")"); }
        else if (!K.track(c).width || !c->have_genome) throw ScsError(SCS_EINVAL, fn + ": the " + K.feature + " is off (" + K.set_fn + "), or no genome is staged");
        const ScsError small(SCS_EOVERFLOW, fn + ": " + K.recs + " + 1 entries are needed");
        if (!K.on_ref && cap < c->rec_len.size() + 1) throw small;                 // (the staged records are known before their layout, the reference's with it)
        std::vector<uint64_t> off; (void)layout(c, K, &off);
        if (cap < off.size()) throw small;
        std::copy(off.begin(), off.end(), bin_off);
    });
}
// out[k]: plane k of the counters (NULL: not wanted)
int download_track(scs_ctx* c, const DepthKind& K, const std::string& fn, uint64_t* const* out, uint64_t cap) {
    return guarded(c, [&] {
        ready(c, K, fn);
        const DepthTrack& T = K.track(c); const uint64_t n = K.entries(T);
        if (cap < n) throw ScsError(SCS_EOVERFLOW, fn + ": " + std::to_string(n) + (K.on_ref ? " entries (the bins and the pseudo-bin)" : " bins") + ", room for " + std::to_string(cap));
        for (int k = 0; k < K.planes(); ++k) if (out[k] && n) HIP_OK(hipMemcpyAsync(out[k], T.cnt.as<uint64_t>() + k * n, n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    });
}
int write_track(scs_ctx* c, const DepthKind& K, const std::string& fn, const char* path) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, fn + ": no path");
        ready(c, K, fn); if (K.on_ref) need_lift(c, fn.c_str());
        const DepthTrack& T = K.track(c); const uint64_t nb = T.bins, n = K.entries(T), w = T.width; const int np = K.planes();
        std::vector<uint64_t> cnt(std::max<uint64_t>(np * n, 1));
        if (n) HIP_OK(hipMemcpyAsync(cnt.data(), T.cnt.p, np * n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        FILE* o = fopen(path, "w");
        if (!o) throw ScsError(SCS_EIO, fn + ": can not open " + path + ": " + strerror(errno));
        auto counters = [&](uint64_t b) { bool ok = true; for (int k = 0; k < np && ok; ++k) ok = fprintf(o, "\t%llu", (unsigned long long)cnt[k * n + b]) > 0; return ok && fputc('\n', o) != EOF; };
        bool okw = fputs(K.on_ref ? "#record\tstart\tend\treads\tbases\tcopies\n" : "#record\tstart\tend\treads\tbases\n", o) != EOF; uint64_t b = 0;
        const std::vector<uint64_t>& lens = K.lens(c);
        for (size_t r = 0; r < lens.size() && okw; ++r)
            for (uint64_t x = 0; x < lens[r] && okw; x += w, ++b)
                okw = fprintf(o, "%s\t%llu\t%llu", K.name(c, r).c_str(), (unsigned long long)x, (unsigned long long)std::min<uint64_t>(x + w, lens[r])) > 0 && counters(b);
        if (okw && K.on_ref) okw = fputs("#unlifted", o) != EOF && counters(nb);
        if (fclose(o) != 0 || !okw || b != nb) throw ScsError(SCS_EIO, fn + ": writing " + path + " failed");
    });
}

}  // namespace

void depth_check(scs_ctx* c) { check(c, kRef); check(c, kHap); }
void depth_yield_check(scs_ctx* c) {
    if (c->depth.width) (void)layout(c, kHap, nullptr);                            // more than 2^27 bins: refused before any GPU work
    if (c->depth_ref.width) { check(c, kRef); (void)layout(c, kRef, nullptr); }    // no lift table, or more than 2^27 bins: the same
}

// The kernel's tables -- the staged record starts (nr + 1), on_ref: the reference's lengths (nf), the first bins (n + 1) -- and this
// call's counters, zeroed on the ctx stream; on_ref: the copies where the layout is new
void depth_open(scs_ctx* c, bool on_ref) {
    const DepthKind& K = on_ref ? kRef : kHap; DepthTrack& T = K.track(c); const hipStream_t s = c->stream;
    std::vector<uint64_t> boff; const uint64_t nb = T.bins = layout(c, K, &boff);
    std::vector<uint64_t> tab = record_starts(c); const size_t nr = c->recs.size(), nf = K.lens(c).size();
    if (on_ref) tab.insert(tab.end(), c->lift.ref_lens.begin(), c->lift.ref_lens.end());
    tab.insert(tab.end(), boff.begin(), boff.end());
    upload(T.tab, tab, s);
    const bool copies_stand = on_ref && c->dref_copies;
    const size_t one = (size_t)K.entries(T) * 8, all = std::max<size_t>(K.planes() * one, 16);
    T.cnt.reserve(all, s, copies_stand ? all : 0);                                 // (a layout that stands keeps its size: nothing moves)
    HIP_OK(hipMemsetAsync(T.cnt.p, 0, copies_stand ? 2 * one : all, s));
    if (on_ref && !copies_stand) {
        const uint64_t* t = T.tab.as<uint64_t>();
        launch_lift_copies(s, c->d_lift.as<LiftSeg>(), (uint32_t)c->lift.segs.size(), t + nr + 1, t + nr + 1 + nf, (uint32_t)nf, T.width, nb,
                           T.cnt.as<unsigned long long>() + 2 * (nb + 1), c->flags.as<uint32_t>());
    }
    HIP_OK(hipStreamSynchronize(s));                                               // (the host table goes)
    if (on_ref && !copies_stand) { check_flags(c); c->dref_copies = true; }
}

}  // namespace scs

extern "C" {

int scs_set_depth(scs_ctx* c, uint32_t bin_width) { return set_width(c, kHap, bin_width); }
int scs_depth_bins(const scs_ctx* c, uint64_t* n_bins, uint32_t* bin_width) { return bins(c, kHap, "scs_depth_bins", n_bins, bin_width); }
int scs_depth_record_bins(const scs_ctx* c, uint64_t* bin_off, uint64_t cap) { return record_bins(c, kHap, "scs_depth_record_bins", bin_off, cap); }
int scs_download_depth(scs_ctx* c, uint64_t* reads, uint64_t* bases, uint64_t cap) { uint64_t* const out[3] = {reads, bases, nullptr}; return download_track(c, kHap, "scs_download_depth", out, cap); }
int scs_write_depth(scs_ctx* c, const char* path) { return write_track(c, kHap, "scs_write_depth", path); }

int scs_set_depth_ref(scs_ctx* c, uint32_t bin_width) { return set_width(c, kRef, bin_width); }
int scs_depth_ref_bins(const scs_ctx* c, uint64_t* n_bins, uint32_t* bin_width) { return bins(c, kRef, "scs_depth_ref_bins", n_bins, bin_width); }
int scs_depth_ref_record_bins(const scs_ctx* c, uint64_t* bin_off, uint64_t cap) { return record_bins(c, kRef, "scs_depth_ref_record_bins", bin_off, cap); }
int scs_download_depth_ref(scs_ctx* c, uint64_t* reads, uint64_t* bases, uint64_t* copies, uint64_t cap) { uint64_t* const out[3] = {reads, bases, copies}; return download_track(c, kRef, "scs_download_depth_ref", out, cap); }
int scs_write_depth_ref(scs_ctx* c, const char* path) { return write_track(c, kRef, "scs_write_depth_ref", path); }
int scs_depth_ref_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_depth_ref, launches, ms, units); }

}  // extern "C"
