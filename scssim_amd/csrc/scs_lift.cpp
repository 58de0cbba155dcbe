// scs_lift.cpp -- the lift table (include/scssim_hip.h: scs_write_lift, scs_load_lift, scs_lift_info, scs_lift_segments,
// scs_lift_positions).  The table itself -- built from the simuvars plan, written, parsed -- is scs_lift.h's;
// here it becomes the ctx's (host vector + device copy), the ctx's entry points run over it, and the host-only probes expose what
// they run.  The depth track over it is scs_depth.cpp's.
#include "scs_textout.h"
#include <cerrno>

namespace scs {

void lift_drop(scs_ctx* c) {
    if (!c->have_lift && !c->d_lift.p) return;
    c->have_lift = false; c->lift.clear(); c->d_lift.release();
    c->depth_ref.valid = false; c->dref_copies = false; c->depth_ref.bins = 0;   // (the reference track's layout was this table's)
    coverage_invalidate(c, false);                                               // (and so were the coverage profile's reference array and its copies)
}
void lift_install(scs_ctx* c, LiftTable&& T) {
    lift_drop(c);
    if (T.segs.size() > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, "lift table: more than 2^32 segments");
    c->lift = std::move(T);
    upload(c->d_lift, c->lift.segs, c->stream);
    HIP_OK(hipStreamSynchronize(c->stream));
    c->have_lift = true;
}

void need_lift(const scs_ctx* c, const char* fn) {
    if (!c->have_lift) throw ScsError(SCS_EINVAL, std::string(fn) + ": the staged genome has no lift table (scs_simuvars keeps one, scs_load_lift reads one)");
}

namespace {
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
    const uint32_t lo = rec_of(roff.data(), n_hap, a.lo);                              // the record, as the kernel finds it
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
