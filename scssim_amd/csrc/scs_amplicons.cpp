// scs_amplicons.cpp -- the amplicon table (include/scssim_hip.h: scs_amplicon_places, scs_write_amplicons):
// one entry per full amplicon of the list, made on the device (scs_k_amplicons.hip) a chunk of amplicons at a time after
// scs_allocate_reads.  Nothing here is sized by the job: the kernels' work arrays, the two text buffers and their pinned twins
// hold one chunk, and all of them are released when the call returns.
#include "scs_textout.h"
#include "scs_amp.h"

namespace {

const uint32_t kAmpChunk = 1u << 20;                       // amplicons per chunk: about 48 MB of text

void amp_check(scs_ctx* c, const char* fn) {
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, std::string(fn) + ": not available for a sharded job (shard_count > 1)");
    if (!c->allocated) throw ScsError(SCS_EINVAL, std::string(fn) + ": call scs_allocate_reads first (the table states every amplicon's read number)");
}

// One call's work: the kernels' arguments over the ctx's tables, the record table they name records from, and everything the call
// allocates -- a chunk's line sizes and 64-bit offsets, the binary form's arrays, two text buffers (and the BGZF lane over them) with
// their pinned twins, the copy stream, the chunk's totals in pinned words behind ev_n / ev_made.  Its destructor ends every way out of
// the call: both streams drained; the members then release themselves
struct AmpJob {
    scs_ctx* const c; const hipStream_t s; AmpArgs a{}; uint32_t chunk = kAmpChunk, lds = 0;
    RecTable rt; DevBuf sizes, offs, scan, bin, out[2], crc; BgzfLane z; Pinned<char> h_out[2]; Pinned<uint64_t> h_n;
    Stream copy; Event ev_n, ev_made[2], ev_d2h[2];
    explicit AmpJob(scs_ctx* c_) : c(c_), s(c_->stream) {
        if (seam_env("SCS_TEST_AMP_CHUNK")) chunk = (uint32_t)std::max(1L, std::min(atol(seam_env("SCS_TEST_AMP_CHUNK")), 1L << 30));   // tests: chunk edges
        if (seam_env("SCS_TEST_AMP_LDS")) lds = (uint32_t)std::max(16, atoi(seam_env("SCS_TEST_AMP_LDS")));                             // tests: lines that straddle two LDS runs
        rt.make(c, s);
        a.fr = c->frags_view(); a.semis = c->semis.view(); a.fulls = c->fulls.view(); a.spool = c->semis.pool.as<uint32_t>(); a.fpool = c->fulls.pool.as<uint32_t>();
        a.g = c->genome.as<uint8_t>(); a.read_numbers = c->read_numbers.as<uint32_t>();
        a.rec_off = rt.rec_off; a.name_off = rt.name_off; a.names = rt.names; a.n_rec = rt.n_rec;
        a.flags = c->flags.as<uint32_t>();
    }
    ~AmpJob() {
        (void)hipStreamSynchronize(s); if (copy.s) (void)hipStreamSynchronize(copy);
        c->tm_amp.ev.clear(); c->tm_amp.used = 0;          // (the timer's events were this call's too; its sums stay)
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
            J.bin.reserve((size_t)n * 21 + 16, s);         // starts | records | lengths | edit counts | strands
            uint64_t* d_start = J.bin.as<uint64_t>(); uint32_t* d_rec = (uint32_t*)(d_start + n); uint32_t* d_len = d_rec + n; uint32_t* d_ne = d_len + n; int8_t* d_str = (int8_t*)(d_ne + n);
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
        OutFile fd; fd.open("scs_write_amplicons", path, bgzf);
        AmpJob J(c); const hipStream_t s = J.s; KernelTimer& tm = c->tm_amp; tm.reset();
        fd.header("#record\tstart\tend\tamplicon\tstrand\treads\tsemi\tedits\n");
        J.copy.ensure(hipStreamNonBlocking); J.ev_n.ensure(hipEventDisableTiming | hipEventBlockingSync);
        for (int k = 0; k < 2; ++k) { J.ev_made[k].ensure(hipEventDisableTiming | hipEventBlockingSync); J.ev_d2h[k].ensure(hipEventDisableTiming | hipEventBlockingSync); }
        J.h_n.reserve(64, hipHostMallocDefault); memset(J.h_n, 0, 64);              // [0]: a chunk's text bytes; [1 + slot]: its BGZF blocks' bytes
        if (bgzf) bgzf_crc_tables(J.crc, s);
        // Chunk k: sizing pass and scan, its total to the host (it sizes the output), emit pass (and BGZF over the text where it
        // lies), D2H on the copy stream into the slot's pinned twin.  The host then writes chunk k - 1 to the file while the device
        // works on chunk k: two device buffers, two pinned ones.
        struct Made { const char* p = nullptr; uint64_t n = 0; bool z = false; int slot = 0; bool have = false; } prev;
        auto d2h = [&](const Made& m, uint64_t n) {
            J.h_out[m.slot].reserve(std::max<uint64_t>(n, 16), hipHostMallocDefault, (size_t)(n + n / 16 + 16));
            HIP_OK(hipStreamWaitEvent(J.copy, J.ev_made[m.slot], 0));
            if (n) HIP_OK(hipMemcpyAsync(J.h_out[m.slot], m.p, n, hipMemcpyDeviceToHost, J.copy));
            HIP_OK(hipEventRecord(J.ev_d2h[m.slot], J.copy));
        };
        auto drain = [&](Made& m) {
            if (!m.have) return;
            if (m.z) { HIP_OK(hipEventSynchronize(J.ev_made[m.slot])); m.n = (uint32_t)J.h_n[1 + m.slot]; d2h(m, m.n); }   // the blocks' total has arrived
            HIP_OK(hipEventSynchronize(J.ev_d2h[m.slot]));
            if (m.n) fd.write(J.h_out[m.slot], m.n);
            m.have = false;
        };
        uint32_t k = 0;
        for (uint32_t first = 0; first < N; ++k) {
            const uint32_t n = std::min(J.chunk, N - first); const int slot = (int)(k & 1u);
            J.a.first = first; J.a.n = n; first += n;
            J.sizes.reserve(((size_t)n + 1) * 4, s); J.offs.reserve(((size_t)n + 1) * 8, s); J.scan.reserve(scan_temp_bytes(n), s);
            tm.begin(s);
            launch_amp_size(s, J.a, J.sizes.as<uint32_t>());
            exclusive_scan_u32_to_u64(s, J.sizes.as<uint32_t>(), J.offs.as<uint64_t>(), n, J.scan.p, J.scan.cap);
            tm.end(s);
            HIP_OK(hipMemcpyAsync(J.h_n, J.offs.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipEventRecord(J.ev_n, s));
            HIP_OK(hipEventSynchronize(J.ev_n));
            { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("amplicon table: sizing pass failed: ") + hipGetErrorString(le)); }
            const uint64_t t_n = J.h_n[0];
            // (the slot's last user, chunk k - 2, has left the device: the host wrote it to the file before it came here)
            J.out[slot].reserve(std::max<uint64_t>(t_n + t_n / 16, 16) + 16, s);
            Made cur; cur.p = J.out[slot].as<char>(); cur.n = t_n; cur.slot = slot; cur.have = true;
            tm.begin(s);
            launch_amp_emit(s, J.a, J.offs.as<uint64_t>(), J.lds, J.out[slot].as<char>());
            if (bgzf && t_n) {                             // the text becomes BGZF blocks where it lies (the FASTQ blocks' kernels); their total travels to h_n[1 + slot]
                J.z.out[slot].reserve(bgzf_bound(t_n), s);
                bgzf_in_place(s, J.z, J.crc, cur.p, t_n, J.z.out[slot].as<char>(), (uint32_t*)(J.h_n + 1 + slot), nullptr, 0, "scs_write_amplicons: a chunk's text exceeds 4 GB");
                cur.p = J.z.out[slot].as<char>(); cur.z = true;
            }
            tm.end(s); tm.add_units(n);
            HIP_OK(hipEventRecord(J.ev_made[slot], s));
            if (!cur.z) d2h(cur, cur.n);
            drain(prev); prev = cur;
        }
        drain(prev);
        check_flags(c);                                    // (also: everything on the ctx stream is over)
        tm.collect();
        fd.finish();
        if (bytes) *bytes = fd.total;
    });
}

int scs_amplicon_kernel_time(const scs_ctx* c, uint64_t* launches, double* ms, uint64_t* units) { return kernel_time_of(c, &scs_ctx::tm_amp, launches, ms, units); }

}  // extern "C"
