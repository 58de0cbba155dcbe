// scs_amplicons.cpp -- the amplicon table (include/scssim_hip.h: scs_amplicon_places, scs_write_amplicons):
// one entry per full amplicon of the list, made on the device (scs_k_amplicons.hip) a chunk of amplicons at a time after
// scs_allocate_reads.  Nothing here is sized by the job: the kernels' work arrays, the two text buffers and their pinned twins
// hold one chunk, and all of them are released when the call returns.
#include "scs_ctx.h"
#include "scs_amp.h"
#include <cerrno>

namespace {

const uint32_t kAmpChunk = 1u << 20;                       // amplicons per chunk: about 48 MB of text

void amp_check(scs_ctx* c, const char* fn) {
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, std::string(fn) + ": not available for a sharded job (shard_count > 1)");
    if (!c->allocated) throw ScsError(SCS_EINVAL, std::string(fn) + ": call scs_allocate_reads first (the table states every amplicon's read number)");
}

struct AmpFd {
    int fd = -1; ~AmpFd() { if (fd >= 0) ::close(fd); }
    bool write_all(const char* p, size_t n) {
        while (n) { const ssize_t w = ::write(fd, p, n); if (w < 0) { if (errno == EINTR) continue; return false; } p += w; n -= (size_t)w; }
        return true;
    }
};

// what both entry points share: the kernels' arguments over the ctx's tables and the record table they name records from.
// Its destructor ends every way out of the call: both streams drained, every buffer of the call released
struct AmpJob {
    scs_ctx* const c; const hipStream_t s; AmpArgs a{}; uint32_t chunk = kAmpChunk, lds = 0;
    explicit AmpJob(scs_ctx* c_) : c(c_), s(c_->stream) {
        if (seam_env("SCS_TEST_AMP_CHUNK")) chunk = (uint32_t)std::max(1L, std::min(atol(seam_env("SCS_TEST_AMP_CHUNK")), 1L << 30));   // tests: chunk edges
        if (seam_env("SCS_TEST_AMP_LDS")) lds = (uint32_t)std::max(16, atoi(seam_env("SCS_TEST_AMP_LDS")));                             // tests: lines that straddle two LDS runs
        const uint32_t nr = (uint32_t)c->recs.size();      // record starts, name offsets, names: the truth passes' table
        std::vector<uint64_t> roff(nr + 1, 0); std::vector<uint32_t> noff(nr + 1, 0); std::string names;
        for (uint32_t r = 0; r < nr; ++r) { roff[r] = c->rec_off[r]; roff[r + 1] = c->rec_off[r] + c->rec_len[r]; names += c->recs[r].name; noff[r + 1] = (uint32_t)names.size(); }
        const size_t o_name = (size_t)(nr + 1) * 8, o_text = o_name + (size_t)(nr + 1) * 4; std::vector<uint8_t> blob(o_text + names.size() + 16, 0);
        memcpy(blob.data(), roff.data(), o_name); memcpy(blob.data() + o_name, noff.data(), (size_t)(nr + 1) * 4); memcpy(blob.data() + o_text, names.data(), names.size());
        upload(c->am_recs, blob, s); HIP_OK(hipStreamSynchronize(s));                // (the host blob goes)
        const uint8_t* tb = c->am_recs.as<uint8_t>();
        a.fr = c->frags_view(); a.semis = c->semis.view(); a.fulls = c->fulls.view(); a.spool = c->semis.pool.as<uint32_t>(); a.fpool = c->fulls.pool.as<uint32_t>();
        a.g = c->genome.as<uint8_t>(); a.read_numbers = c->read_numbers.as<uint32_t>();
        a.rec_off = (const uint64_t*)tb; a.name_off = (const uint32_t*)(tb + o_name); a.names = (const char*)(tb + o_text); a.n_rec = nr;
        a.flags = c->flags.as<uint32_t>();
    }
    ~AmpJob() {
        (void)hipStreamSynchronize(s); if (c->copy_stream.s) (void)hipStreamSynchronize(c->copy_stream);
        c->am_recs.release(); c->am_sizes.release(); c->am_offs.release(); c->am_scan.release(); c->am_bin.release();
        c->am_z.plan.release(); c->am_z.sizes.release(); c->am_z.offs.release();
        for (int k = 0; k < 2; ++k) { c->am_out[k].release(); c->am_z.out[k].release(); c->h_am[k].release(); }
    }
};

}  // namespace

extern "C" {

int scs_amplicon_places(scs_ctx* c, uint32_t* rec, uint64_t* start, uint32_t* len, int8_t* strand, uint32_t* n_edits, uint64_t cap) {
    return guarded(c, [&] {
        amp_check(c, "scs_amplicon_places");
        const uint32_t N = c->fulls.n;
        if (cap < N) throw ScsError(SCS_EOVERFLOW, "scs_amplicon_places: " + std::to_string(N) + " full amplicons, room for " + std::to_string(cap));
        AmpJob J(c); const hipStream_t s = J.s;
        for (uint32_t first = 0; first < N; first += std::min(J.chunk, N - first)) {
            const uint32_t n = std::min(J.chunk, N - first);
            c->am_bin.reserve((size_t)n * 21 + 16, s);     // starts | records | lengths | edit counts | strands
            uint64_t* d_start = c->am_bin.as<uint64_t>(); uint32_t* d_rec = (uint32_t*)(d_start + n); uint32_t* d_len = d_rec + n; uint32_t* d_ne = d_len + n; int8_t* d_str = (int8_t*)(d_ne + n);
            J.a.first = first; J.a.n = n;
            launch_amp_place(s, J.a, rec ? d_rec : nullptr, start ? d_start : nullptr, len ? d_len : nullptr, strand ? d_str : nullptr, n_edits ? d_ne : nullptr);
            if (rec) HIP_OK(hipMemcpyAsync(rec + first, d_rec, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            if (start) HIP_OK(hipMemcpyAsync(start + first, d_start, (size_t)n * 8, hipMemcpyDeviceToHost, s));
            if (len) HIP_OK(hipMemcpyAsync(len + first, d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            if (strand) HIP_OK(hipMemcpyAsync(strand + first, d_str, (size_t)n, hipMemcpyDeviceToHost, s));
            if (n_edits) HIP_OK(hipMemcpyAsync(n_edits + first, d_ne, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
        }
        check_flags(c);
    });
}

int scs_write_amplicons(scs_ctx* c, const char* path, int flags, uint64_t* bytes) {
    return guarded(c, [&] {
        if (!path || !*path) throw ScsError(SCS_EINVAL, "scs_write_amplicons: no path");
        if (flags & ~1) throw ScsError(SCS_EINVAL, "scs_write_amplicons: unknown flag");
        amp_check(c, "scs_write_amplicons");
        const bool bgzf = (flags & 1) != 0; const uint32_t N = c->fulls.n;
        AmpFd fd; fd.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (fd.fd < 0) throw ScsError(SCS_EIO, std::string("scs_write_amplicons: can not open ") + path + ": " + strerror(errno));
        const std::string failed = std::string("scs_write_amplicons: writing ") + path + " failed";
        AmpJob J(c); const hipStream_t s = J.s; KernelTimer& tm = c->tm_amp; tm.reset();
        std::string hd = "#record\tstart\tend\tamplicon\tstrand\treads\tsemi\tedits\n";
        if (bgzf) { std::vector<uint8_t> z; bgzf_compress_host((const uint8_t*)hd.data(), hd.size(), BGZF_LDS_OUT, z); hd.assign((const char*)z.data(), z.size()); }
        if (!fd.write_all(hd.data(), hd.size())) throw ScsError(SCS_EIO, failed);
        uint64_t total = hd.size();
        c->copy_stream.ensure(hipStreamNonBlocking); c->ev_am_n.ensure(hipEventDisableTiming | hipEventBlockingSync);
        for (int k = 0; k < 2; ++k) { c->ev_am_made[k].ensure(hipEventDisableTiming | hipEventBlockingSync); c->ev_am_d2h[k].ensure(hipEventDisableTiming | hipEventBlockingSync); }
        c->h_am_n.reserve(64, hipHostMallocDefault); memset(c->h_am_n, 0, 64);      // [0]: a chunk's text bytes; [1 + slot]: its BGZF blocks' bytes
        if (bgzf && !c->z_crc.p) { std::vector<uint32_t> tabs(512); bgzf_host_tables(tabs.data(), tabs.data() + 256); upload(c->z_crc, tabs, s); HIP_OK(hipStreamSynchronize(s)); }
        // Chunk k: sizing pass and scan, its total to the host (it sizes the output), emit pass (and BGZF over the text where it
        // lies), D2H on the copy stream into the slot's pinned twin.  The host then writes chunk k - 1 to the file while the device
        // works on chunk k: two device buffers, two pinned ones.
        struct Made { const char* p = nullptr; uint64_t n = 0; bool z = false; int slot = 0; bool have = false; } prev;
        auto d2h = [&](const Made& m, uint64_t n) {
            c->h_am[m.slot].reserve(std::max<uint64_t>(n, 16), hipHostMallocDefault, (size_t)(n + n / 16 + 16));
            HIP_OK(hipStreamWaitEvent(c->copy_stream, c->ev_am_made[m.slot], 0));
            if (n) HIP_OK(hipMemcpyAsync(c->h_am[m.slot], m.p, n, hipMemcpyDeviceToHost, c->copy_stream));
            HIP_OK(hipEventRecord(c->ev_am_d2h[m.slot], c->copy_stream));
        };
        auto drain = [&](Made& m) {
            if (!m.have) return;
            if (m.z) { HIP_OK(hipEventSynchronize(c->ev_am_made[m.slot])); m.n = (uint32_t)c->h_am_n[1 + m.slot]; d2h(m, m.n); }   // the blocks' total has arrived
            HIP_OK(hipEventSynchronize(c->ev_am_d2h[m.slot]));
            if (m.n && !fd.write_all(c->h_am[m.slot], m.n)) throw ScsError(SCS_EIO, failed);
            total += m.n; m.have = false;
        };
        uint32_t k = 0;
        for (uint32_t first = 0; first < N; ++k) {
            const uint32_t n = std::min(J.chunk, N - first); const int slot = (int)(k & 1u);
            J.a.first = first; J.a.n = n; first += n;
            c->am_sizes.reserve(((size_t)n + 1) * 4, s); c->am_offs.reserve(((size_t)n + 1) * 8, s); c->am_scan.reserve(scan_temp_bytes(n), s);
            tm.begin(s);
            launch_amp_size(s, J.a, c->am_sizes.as<uint32_t>());
            exclusive_scan_u32_to_u64(s, c->am_sizes.as<uint32_t>(), c->am_offs.as<uint64_t>(), n, c->am_scan.p, c->am_scan.cap);
            tm.end(s);
            HIP_OK(hipMemcpyAsync(c->h_am_n, c->am_offs.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipEventRecord(c->ev_am_n, s));
            HIP_OK(hipEventSynchronize(c->ev_am_n));
            { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("amplicon table: sizing pass failed: ") + hipGetErrorString(le)); }
            const uint64_t t_n = c->h_am_n[0];
            // (the slot's last user, chunk k - 2, has left the device: the host wrote it to the file before it came here)
            c->am_out[slot].reserve(std::max<uint64_t>(t_n + t_n / 16, 16) + 16, s);
            Made cur; cur.p = c->am_out[slot].as<char>(); cur.n = t_n; cur.slot = slot; cur.have = true;
            tm.begin(s);
            launch_amp_emit(s, J.a, c->am_offs.as<uint64_t>(), J.lds, c->am_out[slot].as<char>());
            if (bgzf && t_n) {                             // the text becomes BGZF blocks where it lies (the FASTQ blocks' kernels); their total travels to h_am_n[1 + slot]
                if (bgzf_bound(t_n) > 0xFFFFFFF0ull) throw ScsError(SCS_EOVERFLOW, "scs_write_amplicons: a chunk's text exceeds 4 GB");
                scs_ctx::BgzfLane& z = c->am_z; const uint32_t nblk = bgzf_blocks(t_n);
                z.plan.reserve(std::max<size_t>((size_t)nblk * BGZF_PLAN_BYTES, 16), s); z.sizes.reserve(((size_t)nblk + 2) * 4, s); z.offs.reserve(((size_t)nblk + 2) * 4, s);
                z.out[slot].reserve(bgzf_bound(t_n), s);
                launch_bgzf_plan(s, cur.p, t_n, z.plan.as<uint8_t>(), z.sizes.as<uint32_t>());
                exclusive_scan_u32(s, z.sizes.as<uint32_t>(), z.offs.as<uint32_t>(), nblk, nullptr, 0);
                launch_bgzf_emit(s, cur.p, t_n, z.plan.as<uint8_t>(), z.sizes.as<uint32_t>(), z.offs.as<uint32_t>(), c->z_crc.as<uint32_t>(), c->z_crc.as<uint32_t>() + 256, z.out[slot].as<char>(), 0);
                HIP_OK(hipMemcpyAsync(c->h_am_n + 1 + slot, z.offs.as<uint32_t>() + nblk, 4, hipMemcpyDeviceToHost, s));
                cur.p = z.out[slot].as<char>(); cur.z = true;
            }
            tm.end(s); tm.add_units(n);
            HIP_OK(hipEventRecord(c->ev_am_made[slot], s));
            if (!cur.z) d2h(cur, cur.n);
            drain(prev); prev = cur;
        }
        drain(prev);
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        tm.collect();
        if (bgzf) {                                        // the BGZF end-of-file block (SAM specification, section 4.1.2)
            static const unsigned char eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (!fd.write_all((const char*)eof, 28)) throw ScsError(SCS_EIO, failed);
            total += 28;
        }
        { const int f = fd.fd; fd.fd = -1; if (::close(f) != 0) throw ScsError(SCS_EIO, failed); }
        if (bytes) *bytes = total;
    });
}

int scs_amplicon_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) {
    if (!c) return SCS_EINVAL;
    if (launches) *launches = c->tm_amp.launches; if (ms) *ms = c->tm_amp.ms; if (units) *units = c->tm_amp.units;
    return SCS_OK;
}

}  // extern "C"
