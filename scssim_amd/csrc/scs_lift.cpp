// scs_lift.cpp -- the lift table and the depth track by reference bin (include/scssim_hip.h: scs_write_lift, scs_load_lift,
// scs_lift_info, scs_lift_segments, scs_lift_positions, scs_set_depth_ref ...).  The table itself -- built from
// the simuvars plan, written, parsed -- is scs_lift.h's; here it becomes the ctx's (host vector + device copy), the ctx's entry
// points run over it, and the host-only probes expose what they run.  The per-batch kernel is launched from scs_reads.cpp.
#include "scs_textout.h"
#include <cerrno>

namespace scs {

void lift_drop(scs_ctx* c) {
    if (!c->have_lift && !c->d_lift.p) return;
    c->have_lift = false; c->lift.clear(); c->d_lift.release();
    c->dref_valid = false; c->dref_copies = false; c->dref_bins = 0;
}
void lift_install(scs_ctx* c, LiftTable&& T) {
    lift_drop(c);
    if (T.segs.size() > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, "lift table: more than 2^32 segments");
    c->lift = std::move(T);
    upload(c->d_lift, c->lift.segs, c->stream);
    HIP_OK(hipStreamSynchronize(c->stream));
    c->have_lift = true;
}

void depth_ref_check(scs_ctx* c) {
    if (!c->dref_width) return;
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, "depth by reference bin (scs_set_depth_ref): not available for a sharded job (shard_count > 1); turn it off with scs_set_depth_ref(ctx, 0)");
    if (!c->have_lift) throw ScsError(SCS_EINVAL, "depth by reference bin (scs_set_depth_ref): the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
}
uint64_t depth_ref_layout(const scs_ctx* c, std::vector<uint64_t>* bin_off) {
    if (!c->have_lift) throw ScsError(SCS_EINVAL, "depth by reference bin (scs_set_depth_ref): the staged genome has no lift table (scs_simuvars, scs_load_lift)");
    const size_t nr = c->lift.ref_lens.size(); uint64_t nb = 0; uint32_t min_w = 0;
    if (bin_off) bin_off->assign(nr + 1, 0);
    if (depth_layout(c->lift.ref_lens.data(), nr, c->dref_width, bin_off ? bin_off->data() : nullptr, &nb, &min_w)) return nb;
    throw ScsError(SCS_EINVAL, "depth by reference bin (scs_set_depth_ref): bins of " + std::to_string(c->dref_width) + " bases give more than 2^27 bins for the reference; " +
                   (min_w ? "the smallest bin width it admits is " + std::to_string(min_w) : std::string("no bin width below 2^32 is enough")));
}
void depth_ref_open(scs_ctx* c) {
    const hipStream_t s = c->stream;
    const size_t nr = c->recs.size(), nf = c->lift.ref_lens.size(); std::vector<uint64_t> boff;
    const uint64_t nb = c->dref_bins = depth_ref_layout(c, &boff);
    std::vector<uint64_t> tab = record_starts(c); tab.resize(nr + 1 + nf + nf + 1, 0);
    std::copy(c->lift.ref_lens.begin(), c->lift.ref_lens.end(), tab.begin() + (long)(nr + 1));
    std::copy(boff.begin(), boff.end(), tab.begin() + (long)(nr + 1 + nf));
    upload(c->dr_tab, tab, s);
    const size_t one = (size_t)(nb + 1) * 8;
    c->dr_cnt.reserve(3 * one, s, c->dref_copies ? 3 * one : 0);                    // (a layout that stands keeps its size: nothing moves)
    HIP_OK(hipMemsetAsync(c->dr_cnt.p, 0, (c->dref_copies ? 2 : 3) * one, s));
    if (!c->dref_copies) {
        const uint64_t* t = c->dr_tab.as<uint64_t>();
        launch_lift_copies(s, c->d_lift.as<LiftSeg>(), (uint32_t)c->lift.segs.size(), t + nr + 1, t + nr + 1 + nf, (uint32_t)nf, c->dref_width, nb,
                           c->dr_cnt.as<unsigned long long>() + 2 * (nb + 1), c->flags.as<uint32_t>());
    }
    HIP_OK(hipStreamSynchronize(s));                                               // (the host table goes)
    if (!c->dref_copies) { check_flags(c); c->dref_copies = true; }
}

namespace {
void need_lift(const scs_ctx* c, const char* fn) {
    if (!c->have_lift) throw ScsError(SCS_EINVAL, std::string(fn) + ": the staged genome has no lift table (scs_simuvars keeps one, scs_load_lift reads one)");
}
void need_dref(const scs_ctx* c, const char* fn) {
    if (!c->dref_width || !c->dref_valid) throw ScsError(SCS_EINVAL, std::string(fn) + ": no yield call with the depth by reference bin on (scs_set_depth_ref) has finished");
}
// a table into a caller's arrays (any pointer may be NULL): SCS_EOVERFLOW when one is too small; names: the reference records'
// then the staged records', each followed by a newline
int export_table(const LiftTable& T, uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t seg_cap, uint64_t* n_seg,
                 uint64_t* hap_lens, uint64_t* ref_lens, uint32_t rec_cap, uint32_t* n_hap, uint32_t* n_ref, char* names, size_t names_cap, size_t* names_len) {
    std::string nm; for (auto& s : T.ref_names) nm += s + "\n"; for (auto& s : T.hap_names) nm += s + "\n";
    if (n_seg) *n_seg = T.segs.size(); if (n_hap) *n_hap = (uint32_t)T.hap_lens.size(); if (n_ref) *n_ref = (uint32_t)T.ref_lens.size(); if (names_len) *names_len = nm.size();
    const bool want_segs = hap_off || len || ref_pos || ref_rec || kind;
    if ((want_segs && seg_cap < T.segs.size()) || (hap_lens && rec_cap < T.hap_lens.size()) || (ref_lens && rec_cap < T.ref_lens.size()) || (names && names_cap < nm.size())) return SCS_EOVERFLOW;
    for (size_t i = 0; i < T.segs.size() && want_segs; ++i) {
        const LiftSeg& s = T.segs[i];
        if (hap_off) hap_off[i] = s.hap_off; if (len) len[i] = s.len; if (ref_pos) ref_pos[i] = s.ref_pos; if (ref_rec) ref_rec[i] = s.ref_rec; if (kind) kind[i] = s.kind;
    }
    if (hap_lens) std::copy(T.hap_lens.begin(), T.hap_lens.end(), hap_lens);
    if (ref_lens) std::copy(T.ref_lens.begin(), T.ref_lens.end(), ref_lens);
    if (names) memcpy(names, nm.data(), nm.size());
    return SCS_OK;
}
}  // namespace
}  // namespace scs

extern "C" {

int scs_write_lift(scs_ctx* c, const char* path) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_write_lift: no path");
        need_lift(c, "scs_write_lift");
        if (!lift_write(c->lift, path)) throw ScsError(SCS_EIO, std::string("scs_write_lift: writing ") + path + " failed: " + strerror(errno));
    });
}
int scs_load_lift(scs_ctx* c, const char* path) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_load_lift: no path");
        if (!c->have_genome) throw ScsError(SCS_EINVAL, "scs_load_lift: no genome is staged (the table is read after staging)");
        LiftTable T; std::string why; uint64_t line = 0;
        if (!lift_parse(path, T, why, line)) throw ScsError(SCS_EIO, std::string("scs_load_lift: ") + path + (line ? ", line " + std::to_string(line) + ": " : ": ") + why);
        const size_t nr = c->recs.size();
        for (size_t r = 0; r < std::max(nr, T.hap_names.size()); ++r) {
            if (r < nr && r < T.hap_names.size() && T.hap_names[r] == c->recs[r].name && T.hap_lens[r] == c->rec_len[r]) continue;
            const std::string staged = r < nr ? c->recs[r].name + " (" + std::to_string(c->rec_len[r]) + " bases)" : std::string("nothing"),
                              file = r < T.hap_names.size() ? T.hap_names[r] + " (" + std::to_string(T.hap_lens[r]) + " bases)" : std::string("nothing");
            throw ScsError(SCS_EINVAL, std::string("scs_load_lift: ") + path + " belongs to another genome: record " + std::to_string(r + 1) + " is " + file + " in the file, " + staged + " is staged");
        }
        lift_install(c, std::move(T));
    });
}
int scs_lift_info(const scs_ctx* c, uint64_t* n_segments, uint32_t* n_ref_records) {
    if (!c) return SCS_EINVAL;
    if (!c->have_lift) { const_cast<scs_ctx*>(c)->err = "scs_lift_info: the staged genome has no lift table (scs_simuvars keeps one, scs_load_lift reads one)"; return SCS_EINVAL; }
    if (n_segments) *n_segments = c->lift.segs.size(); if (n_ref_records) *n_ref_records = (uint32_t)c->lift.ref_lens.size();
    return SCS_OK;
}
// the device copy, so that the copy is what a caller (and the tests) sees
int scs_lift_segments(scs_ctx* c, uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t cap, uint64_t* ref_lens, uint32_t ref_cap) {
    return guarded(c, [&] {
        need_lift(c, "scs_lift_segments");
        const size_t n = c->lift.segs.size();
        if (cap < n) throw ScsError(SCS_EOVERFLOW, "scs_lift_segments: " + std::to_string(n) + " segments, room for " + std::to_string(cap));
        if (ref_lens && ref_cap < c->lift.ref_lens.size()) throw ScsError(SCS_EOVERFLOW, "scs_lift_segments: " + std::to_string(c->lift.ref_lens.size()) + " reference records, room for " + std::to_string(ref_cap));
        std::vector<LiftSeg> h(n);
        if (n) HIP_OK(hipMemcpyAsync(h.data(), c->d_lift.p, n * sizeof(LiftSeg), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n; ++i) {
            if (hap_off) hap_off[i] = h[i].hap_off; if (len) len[i] = h[i].len; if (ref_pos) ref_pos[i] = h[i].ref_pos; if (ref_rec) ref_rec[i] = h[i].ref_rec; if (kind) kind[i] = h[i].kind;
        }
        if (ref_lens) std::copy(c->lift.ref_lens.begin(), c->lift.ref_lens.end(), ref_lens);
    });
}
int scs_lift_positions(scs_ctx* c, const uint32_t* rec, const uint64_t* pos, uint64_t n, uint32_t* ref_rec, uint64_t* ref_pos, uint32_t* kind) {
    return guarded(c, [&] {
        need_lift(c, "scs_lift_positions");
        if (n && (!rec || !pos || !ref_rec || !ref_pos || !kind)) throw ScsError(SCS_EINVAL, "scs_lift_positions: null array");
        if (!n) return;
        const hipStream_t s = c->stream; const size_t nr = c->recs.size();
        DevBuf d_in, d_out, d_tab;                                                     // the call's buffers: they go with it
        const std::vector<uint64_t> roff = record_starts(c);
        upload(d_tab, roff, s, 2);                                                     // (+ the `bad` word behind the record starts)
        uint32_t* bad = (uint32_t*)(d_tab.as<uint64_t>() + nr + 1);
        HIP_OK(hipMemsetAsync(bad, 0, 8, s));
        d_in.reserve(n * 12, s); d_out.reserve(n * 16, s);
        uint64_t* d_pos = d_in.as<uint64_t>(); uint32_t* d_rec = (uint32_t*)(d_pos + n);
        uint64_t* d_rp = d_out.as<uint64_t>(); uint32_t* d_rr = (uint32_t*)(d_rp + n); uint32_t* d_k = d_rr + n;
        HIP_OK(hipMemcpyAsync(d_pos, pos, n * 8, hipMemcpyHostToDevice, s)); HIP_OK(hipMemcpyAsync(d_rec, rec, n * 4, hipMemcpyHostToDevice, s));
        launch_lift_points(s, c->d_lift.as<LiftSeg>(), (uint32_t)c->lift.segs.size(), d_tab.as<uint64_t>(), (uint32_t)nr, d_rec, d_pos, n, d_rr, d_rp, d_k, bad);
        uint32_t h_bad = 0;
        HIP_OK(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("scs_lift_positions: kernel launch failed: ") + hipGetErrorString(le)); }
        if (h_bad || c->lift.segs.empty()) throw ScsError(SCS_EINVAL, "scs_lift_positions: a position lies outside its staged record (or names a record that is not staged)");
        HIP_OK(hipMemcpyAsync(ref_pos, d_rp, n * 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipMemcpyAsync(ref_rec, d_rr, n * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(kind, d_k, n * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
    });
}

// ---- depth by reference bin
int scs_set_depth_ref(scs_ctx* c, uint32_t bin_width) {
    return guarded(c, [&] {
        if (bin_width == c->dref_width) return;
        HIP_OK(hipStreamSynchronize(c->stream));                                   // the last call's counters go: nothing may still read them
        c->dr_cnt.release(); c->dr_tab.release(); c->dref_valid = false; c->dref_copies = false; c->dref_bins = 0; c->dref_width = bin_width;
        if (!bin_width) { c->tm_depth_ref.ev.clear(); c->tm_depth_ref.used = 0; c->tm_depth_ref.reset(); }
    });
}
int scs_depth_ref_bins(const scs_ctx* c, uint64_t* n_bins, uint32_t* bin_width) {
    if (!c) return SCS_EINVAL;
    scs_ctx* m = const_cast<scs_ctx*>(c);                                          // (the error text is the only thing written)
    try {
        if (!c->dref_width) throw ScsError(SCS_EINVAL, "scs_depth_ref_bins: the depth by reference bin is off (scs_set_depth_ref)");
        const uint64_t nb = depth_ref_layout(c, nullptr);
        if (n_bins) *n_bins = nb; if (bin_width) *bin_width = c->dref_width;
        return SCS_OK;
    } catch (const ScsError& e) { m->err = e.what(); return e.code; }
}
int scs_depth_ref_record_bins(const scs_ctx* c, uint64_t* bin_off, uint64_t cap) {
    if (!c || !bin_off) return SCS_EINVAL;
    scs_ctx* m = const_cast<scs_ctx*>(c);
    try {
        if (!c->dref_width) throw ScsError(SCS_EINVAL, "scs_depth_ref_record_bins: the depth by reference bin is off (scs_set_depth_ref)");
        std::vector<uint64_t> off; (void)depth_ref_layout(c, &off);
        if (cap < off.size()) throw ScsError(SCS_EOVERFLOW, "scs_depth_ref_record_bins: reference records + 1 entries are needed");
        std::copy(off.begin(), off.end(), bin_off);
        return SCS_OK;
    } catch (const ScsError& e) { m->err = e.what(); return e.code; }
}
int scs_download_depth_ref(scs_ctx* c, uint64_t* reads, uint64_t* bases, uint64_t* copies, uint64_t cap) {
    return guarded(c, [&] {
        need_dref(c, "scs_download_depth_ref");
        const uint64_t n = c->dref_bins + 1;
        if (cap < n) throw ScsError(SCS_EOVERFLOW, "scs_download_depth_ref: " + std::to_string(n) + " entries (the bins and the pseudo-bin), room for " + std::to_string(cap));
        uint64_t* out[3] = {reads, bases, copies};
        for (int k = 0; k < 3; ++k) if (out[k]) HIP_OK(hipMemcpyAsync(out[k], c->dr_cnt.as<uint64_t>() + k * n, n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    });
}
int scs_write_depth_ref(scs_ctx* c, const char* path) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_write_depth_ref: no path");
        need_dref(c, "scs_write_depth_ref"); need_lift(c, "scs_write_depth_ref");
        const uint64_t nb = c->dref_bins, n = nb + 1, w = c->dref_width; std::vector<uint64_t> cnt(3 * n);
        HIP_OK(hipMemcpyAsync(cnt.data(), c->dr_cnt.p, 3 * n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        FILE* o = fopen(path, "w");
        if (!o) throw ScsError(SCS_EIO, std::string("scs_write_depth_ref: can not open ") + path + ": " + strerror(errno));
        bool okw = fputs("#record\tstart\tend\treads\tbases\tcopies\n", o) != EOF; uint64_t b = 0;
        for (size_t r = 0; r < c->lift.ref_lens.size() && okw; ++r)
            for (uint64_t x = 0; x < c->lift.ref_lens[r] && okw; x += w, ++b)
                okw = fprintf(o, "%s\t%llu\t%llu\t%llu\t%llu\t%llu\n", c->lift.ref_names[r].c_str(), (unsigned long long)x, (unsigned long long)std::min<uint64_t>(x + w, c->lift.ref_lens[r]),
                              (unsigned long long)cnt[b], (unsigned long long)cnt[n + b], (unsigned long long)cnt[2 * n + b]) > 0;
        if (okw) okw = fprintf(o, "#unlifted\t%llu\t%llu\t%llu\n", (unsigned long long)cnt[nb], (unsigned long long)cnt[n + nb], (unsigned long long)cnt[2 * n + nb]) > 0;
        if (fclose(o) != 0 || !okw || b != nb) throw ScsError(SCS_EIO, std::string("scs_write_depth_ref: writing ") + path + " failed");
    });
}
int scs_depth_ref_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_depth_ref, launches, ms, units); }

// ---- host-only seams (no GPU, no ctx)
// plan -> table -> optionally the file; subst_pos: the global haplotype indices the plan substitutes (SNP / SNV alleles)
int scs_lift_plan_probe(const char* ref_fasta, const char* snp_file, const char* var_file, const char* out_path,
                        uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t seg_cap, uint64_t* n_seg,
                        uint64_t* subst_pos, uint64_t subst_cap, uint64_t* n_subst,
                        uint64_t* hap_lens, uint64_t* ref_lens, uint32_t rec_cap, uint32_t* n_hap, uint32_t* n_ref,
                        char* names, size_t names_cap, size_t* names_len, char* errbuf, size_t errlen) {
    if (!ref_fasta) return SCS_EINVAL;
    try {
        std::vector<FastaRecord> ref; load_fasta(ref_fasta, ref);
        std::vector<SvChrom> chroms; uint64_t rtot = 0;
        for (auto& r : ref) { chroms.push_back(SvChrom{r.name, rtot, (uint64_t)r.code.size()}); rtot += r.code.size(); }
        SvPlan P; simuvars_plan(chroms, snp_file ? snp_file : "", var_file ? var_file : "", false, P);
        LiftTable T; std::string why;
        if (!lift_from_plan(chroms, P, T, why)) { copy_err(errbuf, errlen, why.c_str()); return SCS_EDEVICE; }
        if (out_path && *out_path && !lift_write(T, out_path)) { copy_err(errbuf, errlen, (std::string("can not write ") + out_path).c_str()); return SCS_EIO; }
        if (n_subst) *n_subst = P.substs.size();
        if (subst_pos) { if (subst_cap < P.substs.size()) return SCS_EOVERFLOW; for (size_t i = 0; i < P.substs.size(); ++i) subst_pos[i] = P.substs[i].dst; }
        return export_table(T, hap_off, len, ref_pos, ref_rec, kind, seg_cap, n_seg, hap_lens, ref_lens, rec_cap, n_hap, n_ref, names, names_cap, names_len);
    } catch (const std::exception& e) { copy_err(errbuf, errlen, e.what()); return SCS_EIO; }
}
// the parser scs_load_lift runs: SCS_EIO with *line (0: the file cannot be opened) and the reason when the file is malformed
int scs_lift_file_probe(const char* path, uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t seg_cap, uint64_t* n_seg,
                        uint64_t* hap_lens, uint64_t* ref_lens, uint32_t rec_cap, uint32_t* n_hap, uint32_t* n_ref,
                        char* names, size_t names_cap, size_t* names_len, uint64_t* line, char* errbuf, size_t errlen) {
    if (!path) return SCS_EINVAL;
    LiftTable T; std::string why; uint64_t ln = 0;
    const bool ok = lift_parse(path, T, why, ln);
    if (line) *line = ok ? 0 : ln;
    if (!ok) { copy_err(errbuf, errlen, (std::string(path) + (ln ? ", line " + std::to_string(ln) + ": " : ": ") + why).c_str()); return SCS_EIO; }
    return export_table(T, hap_off, len, ref_pos, ref_rec, kind, seg_cap, n_seg, hap_lens, ref_lens, rec_cap, n_hap, n_ref, names, names_cap, names_len);
}
// one read through the function k_depth_lift runs (lift_read) after the truth passes' placement.  pos0: the global staged index of
// window base 0; the table as arrays; hap_lens / ref_lens: the staged and the reference records.  *lift_err: 0, or why lift_read
// gave up (1 placed outside its record, 2 off the table, 3 lifted outside the reference; the call then returns SCS_EINVAL).
// *reads_bin and bins[]: reference bins as depth_layout numbers them over ref_lens, the pseudo-bin = their total
int scs_lift_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev,
                        const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                        const uint64_t* hap_lens, uint32_t n_hap, const uint64_t* ref_lens, uint32_t n_ref, uint32_t bin_width,
                        uint64_t* reads_bin, uint64_t* bins, uint32_t* bases, int cap, int* n_out, int* lift_err) {
    if (!n_out || n <= 0 || nev < 0 || nev > TRUTH_EVCAP || (nev && !events) || bin_width == 0 || cap < 0 || (cap && (!bins || !bases)) || !n_hap || !hap_lens || (n_ref && !ref_lens) ||
        (n_seg && (!seg_hap_off || !seg_len || !seg_ref_pos || !seg_ref_rec || !seg_kind))) return SCS_EINVAL;
    if (lift_err) *lift_err = 0;
    std::vector<uint32_t> ev;
    for (int i = 0; i < nev; ++i) {
        if (events[3 * i] < 0 || events[3 * i] > 0xFFFF || events[3 * i + 2] <= 0 || events[3 * i + 2] > 0x7FFF) return SCS_EINVAL;
        ev.push_back(tev_pack((uint32_t)events[3 * i], events[3 * i + 1] ? 1u : 0u, (uint32_t)events[3 * i + 2]));
    }
    TruthAln a{pos0, reverse ? 1 : 0, n, nev, ev.data(), 0, 0, 0};
    if (!truth_place(a)) return SCS_EINVAL;
    std::vector<LiftSeg> segs(n_seg);
    for (uint32_t i = 0; i < n_seg; ++i) segs[i] = LiftSeg{seg_hap_off[i], seg_len[i], seg_ref_pos[i], seg_ref_rec[i], seg_kind[i]};
    std::vector<uint64_t> roff(n_hap + 1, 0), rl(ref_lens, ref_lens + n_ref), boff(n_ref + 1, 0); uint64_t nb = 0;
    for (uint32_t r = 0; r < n_hap; ++r) roff[r + 1] = roff[r] + hap_lens[r];
    if (!depth_layout(rl.data(), n_ref, bin_width, boff.data(), &nb, nullptr)) return SCS_EINVAL;
    uint32_t lo = 0, hi = n_hap;                                                       // the record, as the kernel finds it
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if ((int64_t)roff[mid] <= a.lo) lo = mid; else hi = mid; }
    const LiftView V{segs.data(), n_seg, rl.data(), boff.data(), n_ref, bin_width, nb};
    std::vector<std::pair<uint64_t, uint32_t>> runs; uint64_t first = 0;
    const int err = lift_read(a, (int64_t)roff[lo], (int64_t)roff[lo + 1], V, [&](uint64_t b) { first = b; }, [&](uint64_t b, uint32_t k) { runs.push_back({b, k}); });
    if (err) { if (lift_err) *lift_err = err; return SCS_EINVAL; }
    if (reads_bin) *reads_bin = first;
    *n_out = (int)runs.size();
    if ((int)runs.size() > cap) return SCS_EOVERFLOW;
    for (size_t i = 0; i < runs.size(); ++i) { bins[i] = runs[i].first; bases[i] = runs[i].second; }
    return SCS_OK;
}

}  // extern "C"
