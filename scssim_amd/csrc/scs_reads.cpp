// scs_reads.cpp -- Malbac::setReadCounts and Malbac::yieldReads on the device
#include "scs_sink.h"

namespace scs {
// ---------------------------------------------------------------- a8 + a9: Malbac::setReadCounts (Malbac.cpp:370-408) on the device
void do_allocate(scs_ctx* c, uint64_t reads) {
    if (!c->amplified) throw ScsError(SCS_EINVAL, "scs_allocate_reads: call scs_amplify first");
    hipStream_t s = c->stream;
    if (reads == 0) {                                                             // Malbac::yieldReads, Malbac.cpp:413-420
        uint64_t ref_len = 0;
        for (auto& r : c->recs) { size_t p = r.name.rfind('_'); ref_len += (uint64_t)atoi(r.name.c_str() + (p == std::string::npos ? 0 : p + 1)); }
        ref_len /= 2;
        reads = (uint64_t)(ref_len * c->cfg.coverage / (long)c->prof.read_length);
    }
    if (c->cfg.verbose) fprintf(stderr, "\nNumber of reads to generate: %llu\n", (unsigned long long)reads);
    c->reads_requested = reads; c->st.reads_requested = reads;
    const uint32_t ac = c->fulls.n;
    double t0 = now_s();
    c->weights.reserve(std::max<size_t>((size_t)ac * 8, 16), s);
    c->read_numbers.reserve(((size_t)ac + 1) * 4, s); c->pair_off.reserve(((size_t)ac + 1) * 4, s);
    launch_weights(s, c->fulls.view(), ac, c->dtb, c->key, (uint32_t)c->cfg.frag_size, c->weights.as<double>());
    allocate_weighted(c, reads, ac);
    c->st.t_stage[3] = 0; c->st.t_stage[4] = now_s() - t0;
    c->allocated = true;
}

// the allocation over the weights already in c->weights (ac of them, this shard's list segments in c->full_segs): everything of
// setReadCounts behind the weights.  do_allocate runs it on a job's weights, scs_alloc_probe on given ones
void allocate_weighted(scs_ctx* c, uint64_t reads, uint32_t ac) {
    hipStream_t s = c->stream;
    double* d_w = c->weights.as<double>(); uint32_t* d_rn = c->read_numbers.as<uint32_t>();

    // ---- the plan: where the chunks of the whole job's list lie relative to this shard's list (alloc_plan_build, scs_alloc_plan.h).
    // slot = cycle * 8 + (7 - fragment pass): this shard's segments in local order; the whole job's list takes the
    // shards' segments slot by slot, shard by shard
    const int R = c->cfg.shard_count, me = c->cfg.shard_rank; const bool multi = c->sharded();
    std::vector<uint64_t> segc((size_t)R * ALLOC_SLOTS, 0);
    for (auto& sg : c->full_segs) { if (sg.c < 0 || sg.c >= 5 || sg.p < 0 || sg.p >= 8) throw ScsError(SCS_EINVAL, "allocation: segment out of range"); segc[(size_t)me * ALLOC_SLOTS + sg.c * 8 + (7 - sg.p)] += sg.count; }
    if (multi) c->reduce(segc.data(), segc.size());
    AllocHostPlan hp;
    if (!alloc_plan_build(segc.data(), R, me, hp)) throw ScsError(SCS_EOVERFLOW, "more than 2^32 amplicons in the whole job");
    if (hp.ac != ac) throw ScsError(SCS_EINVAL, "sharded allocation: segment bookkeeping mismatch");
    const std::vector<AllocRange>& rng = hp.rng; const std::vector<AllocBChunk>& bch = hp.bch; const std::vector<AllocGSeg>& gseg = hp.gseg;
    const uint64_t total = hp.total; const uint32_t nch = hp.nch, nq = hp.n_interior;
    AllocPlan pl{}; pl.rank = (uint32_t)me;
    for (int sl = 0; sl < ALLOC_SLOTS; ++sl) pl.my_seg[sl] = hp.my_seg[sl];
    pl.total = total; pl.n_interior = nq; pl.n_boundary = (uint32_t)bch.size(); pl.n_ranges = (uint32_t)rng.size(); pl.n_gseg = (uint32_t)gseg.size();
    const uint32_t nwork = pl.n_interior + pl.n_boundary;
    {   // the plan's arrays: one small upload
        const size_t o_b = rng.size() * sizeof(AllocRange), o_g = o_b + bch.size() * sizeof(AllocBChunk), bytes = o_g + gseg.size() * sizeof(AllocGSeg);
        std::vector<uint8_t> blob(std::max<size_t>(bytes, 16));
        if (!rng.empty()) memcpy(blob.data(), rng.data(), o_b);
        if (!bch.empty()) memcpy(blob.data() + o_b, bch.data(), o_g - o_b);
        if (!gseg.empty()) memcpy(blob.data() + o_g, gseg.data(), bytes - o_g);
        c->a_plan.reserve(blob.size(), s);
        HIP_OK(hipMemcpyAsync(c->a_plan.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s)); HIP_OK(hipStreamSynchronize(s));
        pl.rng = (const AllocRange*)c->a_plan.p; pl.bchunk = (const AllocBChunk*)((char*)c->a_plan.p + o_b); pl.gseg = (const AllocGSeg*)((char*)c->a_plan.p + o_g);
    }
    for (int sl = 0; sl < ALLOC_SLOTS; ++sl) c->seg_lo[sl] = pl.my_seg[sl].lo;
    c->seg_lo[ALLOC_SLOTS] = ac;
    c->gmap = SegMap{};
    if (multi) { uint32_t k = 0; for (int sl = 0; sl < ALLOC_SLOTS; ++sl) if (pl.my_seg[sl].n) { c->gmap.lo[k] = pl.my_seg[sl].lo; c->gmap.cnt[k] = pl.my_seg[sl].n; c->gmap.go[k] = pl.my_seg[sl].go; ++k; } c->gmap.n = k; }

    // ---- buffers: per-chunk partials of the WHOLE job (8 B per 1000 amplicons), per-work-chunk partials of this shard
    const size_t tree_scratch = alloc_tree_scratch(nch);
    c->a_part.reserve(((size_t)nch + 2) * 8, s); c->a_tp.reserve(((size_t)nch + 2) * 8, s); c->a_probs.reserve(((size_t)nch + 2) * 8, s);
    c->a_quota.reserve(((size_t)nch + 2) * 4, s); c->a_crn.reserve(((size_t)nwork + 2) * 4, s); c->a_scratch.reserve(tree_scratch * 8, s);
    c->a_brow.reserve(std::max<size_t>((size_t)pl.n_boundary * ALLOC_CHUNK * 8, 16), s); c->a_bmap.reserve(std::max<size_t>((size_t)pl.n_boundary * ALLOC_CHUNK * 4, 16), s);
    c->odd_before.reserve(((size_t)ac + 1) * 4, s); c->scan_tmp.reserve(scan_temp_bytes(ac), s);
    AllocState* st = (AllocState*)((char*)c->dsums.p + 128);
    double* d_part = c->a_part.as<double>(); double* d_tp = c->a_tp.as<double>();
    unsigned long long* d_sum_rn = (unsigned long long*)(d_tp + nch);               // rides behind tp[] on the same all-reduce
    if (R > 1) {   // first / last 1000 weights of every segment of every shard: what the boundary rows of the others need
        const size_t per = (size_t)ALLOC_SLOTS * 2 * ALLOC_CHUNK * 8;
        c->a_send.reserve(per, s); c->a_gath.reserve(per * R, s);
        launch_alloc_bpack(s, d_w, pl, c->a_send.as<double>());
        c->gather_dev(c->a_send.p, c->a_gath.p, per);
    }
    launch_alloc_bgather(s, d_w, pl, c->a_gath.as<double>(), c->a_brow.as<double>(), c->a_bmap.as<int>());
    if (multi) HIP_OK(hipMemsetAsync(d_part, 0, (size_t)nch * 8, s));               // owners fill their chunks; the all-reduce sums disjoint entries (x + 0 = x)
    launch_alloc_chunk_sum(s, d_w, c->a_brow.as<double>(), pl, d_part);
    if (multi) c->reduce_dev(d_part, nch, 8);
    launch_tree_sum(s, d_part, nch, c->a_scratch.as<double>(), &st->total);
    if (multi) HIP_OK(hipMemsetAsync(d_tp, 0, ((size_t)nch + 1) * 8, s));
    launch_alloc_norm(s, d_w, c->a_brow.as<double>(), c->a_bmap.as<int>(), pl, &st->total, reads, d_rn, d_tp, c->a_crn.as<uint32_t>(), d_sum_rn);
    if (multi) c->reduce_dev(d_tp, (uint64_t)nch + 1, 8);
    launch_alloc_quota(s, d_tp, nch, reads, d_sum_rn, &st->sum_quota, c->a_quota.as<uint32_t>(), c->a_probs.as<double>(), c->a_scratch.as<double>(), c->key);
    launch_alloc_sample(s, d_w, c->a_brow.as<double>(), c->a_bmap.as<int>(), pl, d_tp, c->a_quota.as<uint32_t>(), c->key, d_rn);
    if (c->cfg.paired && !multi) launch_parity_pair_offsets(s, d_rn, ac, c->pair_off.as<uint32_t>(), c->scan_tmp.p, c->scan_tmp.cap);
    else if (c->cfg.paired) {
        launch_alloc_odd_scan(s, d_rn, ac, c->odd_before.as<uint32_t>(), c->scan_tmp.p, c->scan_tmp.cap);
        unsigned long long* table = nullptr;
        if (multi) {   // odd entries of every segment of every shard, in list order
            c->a_odd.reserve((size_t)R * ALLOC_SLOTS * 8, s); table = c->a_odd.as<unsigned long long>();
            HIP_OK(hipMemsetAsync(table, 0, (size_t)R * ALLOC_SLOTS * 8, s));
            launch_alloc_odd_counts(s, c->odd_before.as<uint32_t>(), pl, table);
            c->reduce_dev(table, (uint64_t)R * ALLOC_SLOTS, 8);
        }
        launch_alloc_parity(s, d_rn, c->odd_before.as<uint32_t>(), ac, pl, table);
    }
    if (!c->cfg.paired || multi) launch_pair_offsets(s, d_rn, ac, c->cfg.paired != 0, c->pair_off.as<uint32_t>(), c->scan_tmp.p, c->scan_tmp.cap);
    { Mail m; m.add(ac ? (const void*)(c->pair_off.as<uint32_t>() + ac) : nullptr, 4, 0); mail_post(c, m, true); }
    mail_wait(c);
    c->n_pairs_planned = (uint32_t)c->h_rb[0];
}

// ---------------------------------------------------------------- a10/a11/a13/a16: yieldReads
BatchPlan plan_batches(uint64_t P, uint32_t L, bool to_sink, int writers, int regions, int batch_shift) {
    BatchPlan pl; regions = to_sink ? std::max(1, regions) : 1;
    // pairs per batch: 8 M with the text staying in HBM (5 GB of text per batch: the base pass' grids are long enough for their tails and
    // the per-batch pre-pass not to matter: 2 M -> 8 M gave -11 % on the stage).  Towards a sink a batch fills a pinned slot and every
    // writer holds one: as large as leaves each part file of each generation a couple of batches -- 2 M pairs (1.3 GB of text) on a
    // whole-genome job, where the base pass then runs at the rate it has in HBM (256 k-pair launches ran at 0.09 of the HBM roofline
    // with the chip half empty through their tails, 2 M-pair ones at 0.15: profiles/r04_sink_batch_sizes.log; the job, bound by the
    // host's copies, is the same to within its run-to-run spread) --, never fewer than 256 k (512 k with few writers)
    uint64_t sink_batch = 1ull << 19;
    if (to_sink && writers > 4) {
        const uint64_t per_part = P / (2ull * (uint64_t)regions);                  // two batches per part file
        sink_batch = 1ull << 18; while (sink_batch < (1ull << 21) && sink_batch * 2 <= per_part) sink_batch <<= 1;
        // writers + 2 pinned slots of two mates each stay allocated until the ctx goes: at most 24 GB of them per ctx (12 writers x 2 M pairs of
        // PE150 = 19.5 GB; 64 writers would pin 92 GB per rank)
        const uint64_t per_pair = 4ull * L + 64ull;
        while (sink_batch > (1ull << 18) && ((uint64_t)writers + 2ull) * sink_batch * per_pair > (24ull << 30)) sink_batch >>= 1;
    }
    pl.batch = std::min<uint64_t>(std::max<uint64_t>(P, 1), batch_shift ? (1ull << batch_shift) : to_sink ? sink_batch : (1ull << 23));
    const uint32_t nbatch = pl.nbatch = (uint32_t)((P + pl.batch - 1) / pl.batch);
    // The order the batches are made in.  One region: record order.  Several (a sink with `writers` threads and regions = writers x
    // generations): region r owns the contiguous batches [r nbatch / regions, (r + 1) nbatch / regions); generation after generation,
    // the `writers` regions of a generation are visited round-robin, so every writer always has a batch of its own range on the way
    // while each range still arrives in record order -- and a generation's parts are complete when the next one starts.
    const int n_writers = to_sink ? std::max(1, std::min(writers, regions)) : 1;
    pl.order.reserve(nbatch); pl.region_of.reserve(nbatch);
    for (int g0 = 0; g0 < regions; g0 += n_writers) {
        const int g1 = std::min(regions, g0 + n_writers);
        std::vector<uint32_t> next((size_t)(g1 - g0)), end((size_t)(g1 - g0)); size_t left = 0;
        for (int r = g0; r < g1; ++r) { next[(size_t)(r - g0)] = (uint32_t)((uint64_t)nbatch * r / regions); end[(size_t)(r - g0)] = (uint32_t)((uint64_t)nbatch * (r + 1) / regions); left += end[(size_t)(r - g0)] - next[(size_t)(r - g0)]; }
        while (left) for (int r = g0; r < g1; ++r) if (next[(size_t)(r - g0)] < end[(size_t)(r - g0)]) { pl.order.push_back(next[(size_t)(r - g0)]++); pl.region_of.push_back((uint32_t)r); --left; }
    }
    return pl;
}

namespace {
struct Ship { char* p[3]; uint64_t n[3]; int dsl; uint32_t region; };   // [0], [1]: the mates' text (or its blocks); [2]: the batch's truth SAM (BAM: its blocks, n[2] known once their total has arrived)
// one iteration of do_yield's loop: which pairs, which buffer set (k) and output slot (dsl), what the pre-pass mailed, where its text lies
struct Batch { uint64_t it, p0; uint32_t bidx, np; int k, dsl; const PairRec* pr; const BatchSet* B; BatchCounts n; char* out[2]; char* t_text; uint64_t t_n; };
struct SegAt { size_t seg; uint32_t b; uint64_t o[2]; };
struct PipeGuard { SinkPipe* p; ~PipeGuard() { if (p) (void)p->finish(); } };

struct Yield {               // the state of one do_yield call
    scs_ctx* const c; const OutTarget& tg;
    const hipStream_t s = c->stream; hipStream_t ps = s; const int paired = c->cfg.paired != 0; const uint64_t P = c->n_pairs_planned; const uint32_t L = (uint32_t)c->prof.read_length, slot = ((L + 64 + 63) / 64) * 64;
    const bool to_sink = !tg.device && tg.sink, truth = !c->truth_path.empty(), bam = truth && c->truth_bam, tref = truth && c->truth_ref, bgzf = to_sink && tg.bgzf, depth = c->depth.width != 0, depth_ref = c->depth_ref.width != 0, support = c->support_on, coverage = c->cov.max_depth != 0, coverage_ref = c->cov_ref.max_depth != 0, cov_array = coverage || coverage_ref; const std::string tname = bam ? "truth BAM" : tref ? "truth SAM on the reference" : "truth SAM";
    BatchPlan plan; std::vector<uint32_t> bounds; BatchSet bs[2]; ReadsJob job;
    uint64_t tot[2] = {0, 0}, sunk[2] = {0, 0}, bi = 0;                           // sunk: bytes handed to the sink (= the text's, or its BGZF blocks'); bi: batches handed to the sink so far
    bool d2h_rec[2] = {false, false}, free_rec[2] = {false, false}; Ship pending{}; bool have_pending = false;
    OutFile truth_fd;                                                              // (closed after the pipe's writers have ended: declared first); its total: the header, every batch's bytes, the end-of-file block
    PipeGuard guard{nullptr}; RecTable rt; TruthArgs ta{}; DepthArgs da{}; LiftArgs la{}; SupportArgs sa{}; CovArgs ca{};
    // shard index: the pair index at which each list segment starts (pair_off at the segment's first amplicon); the byte offset of
    // that record = the bytes of the batches before its batch (known once every batch is made) + its offset inside the batch
    std::vector<uint64_t> bpair, bb[2]; std::vector<SegAt> seg_at;
    // what every pass that places reads takes (PlaceArgs): of the job, and of a batch
    void place_job(PlaceArgs& a) const { a.paired = paired; a.tb = c->dtb; a.key = c->key; a.slot = slot; a.flags = c->flags.as<uint32_t>(); }
    static void place_batch(PlaceArgs& a, const Batch& b) { a.pairs = b.pr; a.np = b.np; a.ev_hdr = b.B->ev_hdr; a.ev_dat = b.B->ev_dat; }
    // a test seam that holds a number (SCS_TEST_*_SLOTS: a small LDS table overflows, 0 = no table), or what the product runs with
    static uint32_t seam_u32(const char* name, uint32_t product) { return seam_env(name) ? (uint32_t)atoi(seam_env(name)) : product; }
    void truth_open() {
        // the header first, then the batches' records from the pipe's writer; the kernels' record table: starts, name offsets, names
        truth_fd.open(tname, c->truth_path, bam);
        std::string hd = "@HD\tVN:1.6\tSO:unsorted\n"; const uint32_t nr = (uint32_t)c->recs.size();
        if (tref) for (size_t r = 0; r < c->lift.ref_names.size(); ++r) hd += "@SQ\tSN:" + c->lift.ref_names[r] + "\tLN:" + std::to_string(c->lift.ref_lens[r]) + "\n";   // (the records of the reference the table names)
        else for (uint32_t r = 0; r < nr; ++r) hd += "@SQ\tSN:" + c->recs[r].name + "\tLN:" + std::to_string(c->rec_len[r]) + "\n";
        hd += "@PG\tID:scssim\tPN:scssim\n";
        if (bam) {                                                                 // magic, l_text, the SAM's header text, n_ref, per record l_name / name / l_ref: BGZF made on the host (OutFile::header)
            std::string bh = "BAM\1";
            auto le32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) bh.push_back((char)(v >> (8 * k))); };
            le32((uint32_t)hd.size()); bh += hd; le32(nr);
            for (uint32_t r = 0; r < nr; ++r) { le32((uint32_t)c->recs[r].name.size() + 1u); bh += c->recs[r].name; bh.push_back('\0'); le32((uint32_t)c->rec_len[r]); }
            hd.swap(bh);
        }
        truth_fd.header(hd);
        c->t_sizes.reserve((plan.batch + 1) * 4, s); c->t_offs.reserve((plan.batch + 1) * 8, s); c->t_scan.reserve(scan_temp_bytes(plan.batch), s);
        c->h_t.reserve(64, hipHostMallocDefault); c->ev_t.ensure(hipEventDisableTiming | hipEventBlockingSync);
        rt.make(c, s, &c->t_recs);                                                 // (in the ctx's buffer: it stays allocated between yield calls)
        ta.g = c->genome.as<uint8_t>(); ta.rec_off = rt.rec_off; ta.name_off = rt.name_off; ta.names = rt.names; ta.n_rec = nr;
        place_job(ta);
        if (tref) {                                                                // the reference's table, made as RecTable is: lengths (nf), name offsets (nf + 1), names, 16 bytes of slack
            const uint32_t nf = (uint32_t)c->lift.ref_lens.size(); std::vector<uint32_t> noff(nf + 1, 0); std::string text;
            for (uint32_t r = 0; r < nf; ++r) { text += c->lift.ref_names[r]; noff[r + 1] = (uint32_t)text.size(); }
            const size_t o_name = (size_t)nf * 8, o_text = o_name + (size_t)(nf + 1) * 4; std::vector<uint8_t> blob(o_text + text.size() + 16, 0);
            memcpy(blob.data(), c->lift.ref_lens.data(), o_name); memcpy(blob.data() + o_name, noff.data(), (size_t)(nf + 1) * 4); memcpy(blob.data() + o_text, text.data(), text.size());
            upload(c->t_refs, blob, s); HIP_OK(hipStreamSynchronize(s));          // (the host blob goes)
            const uint8_t* tb = c->t_refs.as<uint8_t>();
            ta.segs = c->d_lift.as<LiftSeg>(); ta.n_seg = (uint32_t)c->lift.segs.size(); ta.ref_len = (const uint64_t*)tb; ta.n_ref = nf;
            ta.ref_name_off = (const uint32_t*)(tb + o_name); ta.ref_names = (const char*)(tb + o_text);
        }
    }
    void depth_open() {
        // the kernel's record table (record starts, first bins) and this call's counters, zeroed on the ctx stream (scs_depth.cpp)
        static const uint32_t slots = seam_u32("SCS_TEST_DEPTH_SLOTS", DEPTH_LDS_SLOTS);
        scs::depth_open(c, false);
        const uint32_t nr = (uint32_t)c->recs.size(); const uint64_t nb = c->depth.bins;
        da.rec_off = c->depth.tab.as<uint64_t>(); da.bin_off = da.rec_off + nr + 1; da.n_rec = nr; da.bin_width = c->depth.width; da.slots = slots;
        da.reads = c->depth.cnt.as<unsigned long long>(); da.bases = da.reads + nb;
        place_job(da);
    }
    void depth_ref_open() {
        // the kernel's tables (staged record starts, the reference's lengths and first bins), this call's counters zeroed on the ctx
        // stream, the copies where the layout is new (scs_depth.cpp)
        static const uint32_t slots = seam_u32("SCS_TEST_LIFT_SLOTS", DEPTH_LDS_SLOTS);
        scs::depth_open(c, true);
        const uint32_t nr = (uint32_t)c->recs.size(), nf = (uint32_t)c->lift.ref_lens.size(); const uint64_t nb = c->depth_ref.bins;
        la.rec_off = c->depth_ref.tab.as<uint64_t>(); la.n_rec = nr; la.ref_len = la.rec_off + nr + 1; la.ref_bin_off = la.ref_len + nf; la.n_ref = nf;
        la.segs = c->d_lift.as<LiftSeg>(); la.n_seg = (uint32_t)c->lift.segs.size(); la.bin_width = c->depth_ref.width; la.slots = slots; la.n_bins = nb;
        la.reads = c->depth_ref.cnt.as<unsigned long long>(); la.bases = la.reads + nb + 1;
        place_job(la);
    }
    void support_open() {
        // the call's site table, its distinct positions and this call's counters, zeroed on the ctx stream (scs_support.cpp)
        static const uint32_t slots = seam_u32("SCS_TEST_SUPPORT_SLOTS", SUPPORT_LDS_SLOTS);
        scs::support_open(c);
        sa.rec_off = c->sp_tab.as<uint64_t>(); sa.n_rec = (uint32_t)c->recs.size(); sa.sp_pos = c->sp_pos.as<uint64_t>(); sa.n_pos = c->sp_n_pos;
        sa.counts = c->sp_cnt.as<uint32_t>(); sa.slots = slots;
        place_job(sa);
    }
    void coverage_open() {
        // this call's difference array and tables, zeroed on the ctx stream, and the kernels' record starts (scs_coverage.cpp)
        // (the profile on the reference needs the same array: one array and one k_cov_mark launch per batch whichever switches are on)
        scs::coverage_open(c);
        if (coverage_ref) scs::coverage_ref_open(c);
        ca.rec_off = c->cov.rec.as<uint64_t>(); ca.n_rec = c->cov.n_rec; ca.diff = c->cov.diff.as<int32_t>();
        place_job(ca);
    }
    void setup() {           // the batches' bounds; the truth file; the pipe's writers; the BGZF totals' pinned words and events, the BGZF kernels' CRC tables; the batches' two buffer sets; the pre-pass' stream; the shard index
        // The pairs are planned (k_plan_pairs: insert sizes, positions, the amplicon resolved to an index map) batch by batch, at the
        // head of each batch's pre-pass: bounds[b] = the amplicon that holds the batch's first pair.
        bounds.assign(plan.nbatch + 1, 0);
        if (P) {
            c->d_bounds.reserve(((size_t)plan.nbatch + 1) * 4, s);
            launch_batch_bounds(s, c->pair_off.as<uint32_t>(), c->fulls.n, plan.batch, plan.nbatch, c->d_bounds.as<uint32_t>());
            HIP_OK(hipMemcpyAsync(bounds.data(), c->d_bounds.p, ((size_t)plan.nbatch + 1) * 4, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s));
        }
        if (truth) truth_open();
        if (depth) depth_open();
        if (depth_ref) depth_ref_open();
        if (support) support_open();
        if (cov_array) coverage_open();
        if (to_sink) {
            if (!c->pipe) c->pipe.reset(new SinkPipe);
            c->copy_stream.ensure(hipStreamNonBlocking); for (int k = 0; k < 2; ++k) { c->ev_made[k].ensure(hipEventDisableTiming); c->ev_d2h[k].ensure(hipEventDisableTiming); }
            c->pipe->truth_fd = truth_fd.fd; c->pipe->start(tg.sink, paired != 0, c->cfg.device); guard.p = c->pipe.get();
        }
        if (bgzf || bam) { c->h_z.reserve(64, hipHostMallocDefault); memset(c->h_z, 0, 64); for (int k = 0; k < 2; ++k) c->ev_z[k].ensure(hipEventDisableTiming | hipEventBlockingSync); }
        if (bgzf || bam) bgzf_crc_tables(c->z_crc, s);                             // (FASTQ blocks and the truth BAM's)
        // Per batch a PRE-PASS (indel events -> record sizes -> offsets, class lists; k_indels + scans) must finish before the host
        // can launch the base pass (it needs the batch's byte counts and class counts).  The pre-pass of batch i+1 is therefore
        // queued BEFORE the base pass of batch i, into a second set of buffers: while the host waits for its mail the GPU
        // still has a base pass to run.
        const uint64_t batch = plan.batch, nreads_b = paired ? 2 * batch : batch;
        c->ev_hdr.reserve(2 * nreads_b * 4, s); c->ev_dat.reserve(2 * nreads_b * 16, s);
        for (int m = 0; m < 2; ++m) c->sizes[m].reserve(2 * (batch + 1) * 4, s);
        for (int m = 0; m < 2; ++m) c->off[m].reserve(2 * (batch + 1) * 8, s);
        c->scan_tmp.reserve(scan_temp_bytes(batch), s);
        // the reads of a batch split by class (with / without indel events): flags, their scans, four lists of pair indices
        c->rl_cls.reserve(2 * (batch + 1) * 2 * 4, s); c->rl_pos.reserve(2 * (batch + 1) * 2 * 4, s); c->rl_lists.reserve(2 * batch * 6 * 4, s);
        for (int k = 0; k < 2; ++k) {
            BatchSet& B = bs[k]; B.ev_hdr = c->ev_hdr.as<uint32_t>() + k * nreads_b; B.ev_dat = c->ev_dat.as<uint4>() + k * nreads_b;
            for (int m = 0; m < 2; ++m) {                                          // (the six lists lie behind one another: slist, clist, dlist, mate 1 then mate 2 of each)
                B.sizes[m] = c->sizes[m].as<uint32_t>() + k * (batch + 1); B.off[m] = c->off[m].as<uint64_t>() + k * (batch + 1);
                B.d1f[m] = c->rl_cls.as<uint32_t>() + (k * 2 + m) * (batch + 1); B.d1p[m] = c->rl_pos.as<uint32_t>() + (k * 2 + m) * (batch + 1);
                B.slist[m] = c->rl_lists.as<uint32_t>() + (k * 6 + m) * batch; B.clist[m] = B.slist[m] + 2 * batch; B.dlist[m] = B.slist[m] + 4 * batch;
            }
        }
        job = ReadsJob{c->genome.as<uint8_t>(), c->genome2.as<uint32_t>() + 16, c->semis.pool_view(), c->fulls.pool_view(), c->dtb, c->key, paired, slot, c->flags.as<uint32_t>(), &c->reads_side};
        // The pre-pass runs on a stream of its own, BESIDE the previous batch's base pass (it is memory-bound and short, the base pass
        // compute-bound).  Its buffer set must be free (the base pass two batches back, which read it, is over: ev_free) and the
        // base pass of its batch starts when the host has seen its mail.  SCS_READS_SERIAL=1: everything on the ctx stream.
        static const bool serial_pre = seam_env("SCS_READS_SERIAL") != nullptr;
        if (!serial_pre) {
            c->pre_stream.ensure(hipStreamNonBlocking); c->ev_plan.ensure(hipEventDisableTiming); for (int k = 0; k < 2; ++k) { c->ev_pre[k].ensure(hipEventDisableTiming); c->ev_free[k].ensure(hipEventDisableTiming); }
            ps = c->pre_stream; HIP_OK(hipEventRecord(c->ev_plan, s)); HIP_OK(hipStreamWaitEvent(ps, c->ev_plan, 0));   // the pair records (and everything before) are made
        }
        bb[0].assign(plan.nbatch, 0); bb[1].assign(plan.nbatch, 0);
        if (!tg.seg_off1) return;
        std::vector<uint32_t> v(ALLOC_SLOTS + 1, 0);
        for (int k = 0; k <= ALLOC_SLOTS; ++k) HIP_OK(hipMemcpyAsync(&v[k], c->pair_off.as<uint32_t>() + c->seg_lo[k], 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        bpair.assign(v.begin(), v.end()); tg.seg_off1->assign(ALLOC_SLOTS + 1, 0); if (tg.seg_off2) tg.seg_off2->assign(ALLOC_SLOTS + 1, 0);
    }
    void prepass(uint64_t it) {
        hipStream_t s = ps;                                                        // (shadows the ctx stream inside the pre-pass)
        const int k = (int)(it & 1); const BatchSet& B = bs[k]; const uint64_t batch = plan.batch, p0 = (uint64_t)plan.order[it] * batch;
        if (ps != c->stream && free_rec[k]) HIP_OK(hipStreamWaitEvent(ps, c->ev_free[k], 0));
        const uint32_t np = (uint32_t)std::min<uint64_t>(batch, P - p0);
        const PairRec* pr = c->pairs.as<PairRec>() + p0;
        // this batch's pair records: its amplicons, the one that straddles the next batch's start included
        const uint32_t b = (uint32_t)(p0 / batch), a_lo = bounds[b], a_hi = std::min<uint32_t>(c->fulls.n, bounds[b + 1] + 1u);
        launch_plan_pairs(s, c->frags_view(), c->semis.view(), c->fulls.view(), a_lo, a_hi - a_lo, (uint32_t)p0, (uint32_t)(p0 + np), c->read_numbers.as<uint32_t>(), c->pair_off.as<uint32_t>(),
                          c->gmap, c->dtb, c->key, paired, c->pairs.as<PairRec>(), c->dsums.as<unsigned long long>() + DS_HOLES);
        // the indel pass fixes every read's length, hence the record sizes and (prefix sums) the record offsets
        c->tm[TM_INDELS].begin(s);
        launch_indels(s, job, pr, np, B);
        c->tm[TM_INDELS].end(s); c->tm[TM_INDELS].add_units(np);
        for (int m = 0; m < (paired ? 2 : 1); ++m) exclusive_scan_sizes(s, B.sizes[m], B.off[m], np, c->scan_tmp.p, c->scan_tmp.cap);   // byte offsets + positions in the class lists: one scan per mate
        launch_read_lists(s, np, paired, B, c->scan_tmp.p, c->scan_tmp.cap);
        Mail m; m.add(B.off[0] + np, 8, 0); m.add(paired ? (const void*)(B.off[1] + np) : nullptr, 8, 1);
        m.add(B.d1p[0] + np, 4, 2); m.add(paired ? (const void*)(B.d1p[1] + np) : nullptr, 4, 3); mail_post(c, m, true, s);
        if (ps != c->stream) HIP_OK(hipEventRecord(c->ev_pre[k], ps));
    }
    Batch decode(uint64_t it) const {                                              // (after mail_wait: the mailbox holds this batch's byte and class counts)
        Batch b{}; b.it = it; b.k = (int)(it & 1); b.bidx = plan.order[it]; b.p0 = (uint64_t)b.bidx * plan.batch; b.np = (uint32_t)std::min<uint64_t>(plan.batch, P - b.p0);
        b.pr = c->pairs.as<PairRec>() + b.p0; b.B = &bs[b.k]; b.dsl = (int)(bi & 1);
        for (int m = 0; m < 2; ++m) { b.n.bytes[m] = c->h_rb[m] & OFF_MASK; b.n.n_general[m] = (uint32_t)(c->h_rb[m] >> OFF_BITS); b.n.n_one_event[m] = (uint32_t)c->h_rb[2 + m]; }
        if (seam_env("SCS_DEBUG_CLASSES")) fprintf(stderr, "[classes] batch of %u pairs: general %u / %u, one-event %u / %u\n", b.np, b.n.n_general[0], b.n.n_general[1], b.n.n_one_event[0], b.n.n_one_event[1]);
        return b;
    }
    void index_batch(const Batch& b) {
        for (int m = 0; m < 2; ++m) bb[m][b.bidx] = b.n.bytes[m];
        for (size_t j = (size_t)(std::lower_bound(bpair.begin(), bpair.end(), b.p0) - bpair.begin()); j < bpair.size() && bpair[j] < b.p0 + b.np; ++j) {   // segments that start inside this batch
            uint64_t ov[2] = {0, 0}; const uint64_t idx = bpair[j] - b.p0;
            for (int m = 0; m < (paired ? 2 : 1); ++m) HIP_OK(hipMemcpyAsync(&ov[m], b.B->off[m] + idx, 8, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s)); seg_at.push_back(SegAt{j, b.bidx, {ov[0] & OFF_MASK, ov[1] & OFF_MASK}});
        }
    }
    // reserves the nb double-buffered outputs of slot dsl that a batch writes together (need: what it writes; room: what a grown buffer gets).  If
    // one must grow (move) and a D2H was recorded on the slot, its last copy must be out -- the host waits; else, where asked, the stream waits (ev_d2h)
    void reserve_slot(DevBuf* d, int nb, const uint64_t* need, const uint64_t* room, int dsl, bool stream_wait) {
        bool grows = false; for (int i = 0; i < nb; ++i) grows |= need[i] > d[i].cap;
        if (d2h_rec[dsl] && grows) HIP_OK(hipEventSynchronize(c->ev_d2h[dsl]));
        else if (d2h_rec[dsl] && stream_wait) HIP_OK(hipStreamWaitEvent(s, c->ev_d2h[dsl], 0));
        for (int i = 0; i < nb; ++i) d[i].reserve(room[i], s);
    }
    void base_pass(Batch& b) {
        if (tg.device) {
            if (tot[0] + b.n.bytes[0] > tg.cap1 || tot[1] + b.n.bytes[1] > tg.cap2) throw ScsError(SCS_EOVERFLOW, "scs_yield_reads_device: output buffer too small");
            b.out[0] = tg.d1 + tot[0]; b.out[1] = tg.d2 ? tg.d2 + tot[1] : nullptr;
        } else {
            // sink mode: two device buffers.  One is free for this batch's k_reads once the D2H of the batch two back has left it
            // (ev_d2h: the stream waits, not the host), so the text of a batch crosses PCIe beside the next batch's kernels.
            DevBuf* d = c->out[b.dsl];
            const uint64_t want[2] = {std::max<uint64_t>(b.n.bytes[0] + b.n.bytes[0] / 16, 16), std::max<uint64_t>(b.n.bytes[1] + b.n.bytes[1] / 16, 16)};
            reserve_slot(d, 2, want, want, b.dsl, true);
            b.out[0] = d[0].as<char>(); b.out[1] = d[1].as<char>();
        }
        c->tm[TM_READS].begin(s);                                                      // the base pass writes the FASTQ text at the record offsets
        launch_reads(s, job, b.pr, b.np, *b.B, b.n, b.out);
        c->tm[TM_READS].end(s); c->tm[TM_READS].add_units(b.np);
        if (c->want_cks && !tg.device) for (int m = 0; m < 2; ++m) launch_text_checksum(s, b.out[m], m && !paired ? 0 : b.n.bytes[m], c->d_cks.as<unsigned long long>() + 2 * (size_t)b.bidx + m);
    }
    // a byte stream becomes BGZF blocks where it lies (scs_textout.h), in the lane's output of slot dsl; the blocks' total travels to the
    // pinned word h_z[dsl][lane].  Returns where the blocks lie
    char* bgzf_in_place(int lane, const char* text, uint64_t n, int dsl, const char* too_large) {
        DevBuf& zo = c->z[lane].out[dsl]; const uint64_t zb = bgzf_bound(n);
        reserve_slot(&zo, 1, &zb, &zb, dsl, false);
        scs::bgzf_in_place(s, c->z[lane], c->z_crc, text, n, zo.as<char>(), c->h_z + (dsl * 3 + lane), nullptr, 0, too_large);   // (at most 256 k blocks: the one-workgroup scan, no scratch)
        return zo.as<char>();
    }
    void truth_batch(Batch& b) {
        // the batch's SAM: sizing pass + 64-bit offsets, the total to the host (it sizes the output), emit pass.  Before ev_free: the
        // passes read the batch's indel events and record offsets
        static const uint32_t lds = seam_u32("SCS_TEST_TRUTH_LDS", 0u);       // tests: the emit pass cuts its runs
        struct Pass {                                                            // the three truth outputs' passes (scs_device.h)
            void (*size)(hipStream_t, const TruthArgs&, uint32_t*); uint32_t (*ppb)(uint64_t, uint32_t);
            void (*emit)(hipStream_t, const TruthArgs&, const uint64_t*, uint32_t, uint32_t, char*);
        };
        static const Pass passes[3] = {{launch_truth_size, truth_pairs_per_block, launch_truth_emit}, {launch_truth_bam_size, truth_bam_pairs_per_block, launch_truth_bam_emit},
                                       {launch_truth_ref_size, truth_ref_pairs_per_block, launch_truth_ref_emit}};
        const Pass& P = passes[bam ? 1 : tref ? 2 : 0];
        const uint32_t np = b.np; const uint64_t fq_bytes = b.n.bytes[0] + b.n.bytes[1];
        place_batch(ta, b); ta.off1 = b.B->off[0]; ta.off2 = b.B->off[1]; ta.fq1 = b.out[0]; ta.fq2 = b.out[1];
        c->tm[TM_TRUTH].begin(s);
        P.size(s, ta, c->t_sizes.as<uint32_t>());
        exclusive_scan_u32_to_u64(s, c->t_sizes.as<uint32_t>(), c->t_offs.as<uint64_t>(), np, c->t_scan.p, c->t_scan.cap);
        HIP_OK(hipMemcpyAsync(c->h_t, c->t_offs.as<uint64_t>() + np, 8, hipMemcpyDeviceToHost, s)); HIP_OK(hipEventRecord(c->ev_t, s));
        c->tm[TM_TRUTH].end(s);
        HIP_OK(hipEventSynchronize(c->ev_t));
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("truth sizing pass failed: ") + hipGetErrorString(le)); }
        DevBuf& to = c->t_out[b.dsl]; const uint64_t t_n = *c->h_t, need = std::max<uint64_t>(t_n, 16), room = std::max<uint64_t>(t_n + t_n / 16, 16);
        reserve_slot(&to, 1, &need, &room, b.dsl, false);
        c->tm[TM_TRUTH].begin(s);
        if (!bam || t_n) P.emit(s, ta, c->t_offs.as<uint64_t>(), P.ppb(fq_bytes, np), lds, to.as<char>());
        if (!bam) { b.t_text = to.as<char>(); b.t_n = t_n; truth_fd.total += t_n; }
        else if (t_n) {
            // BGZF over the batch's records where they lie (the FASTQ blocks' kernels); ship reads n[2] from h_z[dsl][2], behind ev_z
            b.t_text = bgzf_in_place(2, to.as<char>(), t_n, b.dsl, "truth BAM: a batch's records exceed 4 GB");
            if (!bgzf) HIP_OK(hipEventRecord(c->ev_z[b.dsl], s));
        }
        c->tm[TM_TRUTH].end(s); c->tm[TM_TRUTH].add_units(np);
    }
    void depth_batch(const Batch& b) {
        // the batch's reads into the depth counters, from its pair records and indel events alone.  Before ev_free, as truth_batch
        place_batch(da, b);
        c->tm[TM_DEPTH].begin(s);
        launch_depth(s, da);
        c->tm[TM_DEPTH].end(s); c->tm[TM_DEPTH].add_units(b.np);
    }
    void depth_ref_batch(const Batch& b) {
        // the batch's reads into the reference's bins through the lift table, from what depth_batch reads.  Before ev_free, as truth_batch
        place_batch(la, b);
        c->tm_depth_ref.begin(s);
        launch_depth_lift(s, la);
        c->tm_depth_ref.end(s); c->tm_depth_ref.add_units(b.np);
    }
    void support_batch(const Batch& b) {
        // the batch's reads into the site counters, from its pair records, indel events and FASTQ text.  Before ev_free, as truth_batch,
        // and before the sink takes the text
        place_batch(sa, b); sa.off1 = b.B->off[0]; sa.off2 = b.B->off[1]; sa.fq1 = b.out[0]; sa.fq2 = b.out[1];
        c->tm_support.begin(s);
        launch_support(s, sa);
        c->tm_support.end(s); c->tm_support.add_units(b.np);
    }
    void coverage_batch(const Batch& b) {
        // the batch's reads into the difference array, from what depth_batch reads.  Before ev_free, as truth_batch
        place_batch(ca, b);
        c->tm_cov_mark.begin(s);
        launch_cov_mark(s, ca);
        c->tm_cov_mark.end(s); c->tm_cov_mark.add_units(b.np);
    }
    void coverage_finish() {
        // after the last batch: the differences become depths, counted per record (three kernels on the ctx stream, scs_k_coverage.hip)
        const uint32_t lds = seam_u32("SCS_TEST_COV_LDS", COV_LDS_BUCKETS);      // (read at every call: the legs of one test job differ in it)
        scs::coverage_finish(c, lds);
        if (coverage_ref) scs::coverage_ref_finish(c, lds);                        // the staged depths through the lift table, counted per reference record
    }
    void ship(Ship sh) {                                                           // D2H on the copy stream into a free pinned slot, then to the region's writer
        if (bgzf || (bam && sh.p[2])) HIP_OK(hipEventSynchronize(c->ev_z[sh.dsl]));   // the blocks' totals have arrived
        if (bgzf) { sh.n[0] = c->h_z[sh.dsl * 3]; sh.n[1] = c->h_z[sh.dsl * 3 + 1]; }
        if (bam && sh.p[2]) { sh.n[2] = c->h_z[sh.dsl * 3 + 2]; truth_fd.total += sh.n[2]; }
        const int hs = c->pipe->acquire(sh.n[0], sh.n[1], sh.n[2]);                     // (a pinned slot no writer holds: the host waits here when the sink is the slower side)
        if (hs < 0) throw ScsError(SCS_EIO, "sink aborted");
        SinkPipe::Slot& H = c->pipe->slots[(size_t)hs];
        HIP_OK(hipStreamWaitEvent(c->copy_stream, c->ev_made[sh.dsl], 0));          // ... and crosses PCIe on the copy stream, beside the next batch's kernels
        for (int f = 0; f < 3; ++f) if (sh.n[f]) HIP_OK(hipMemcpyAsync(H.h[f], sh.p[f], sh.n[f], hipMemcpyDeviceToHost, c->copy_stream));
        HIP_OK(hipEventRecord(H.ev, c->copy_stream));
        HIP_OK(hipEventRecord(c->ev_d2h[sh.dsl], c->copy_stream)); d2h_rec[sh.dsl] = true;
        c->pipe->submit((int)sh.region, hs, sh.n[0], sh.n[1], sh.n[2]);
        sunk[0] += sh.n[0]; sunk[1] += sh.n[1];
    }
    void sink_batch(const Batch& b) {
        Ship sh{{b.out[0], b.out[1], b.t_text}, {tg.discard ? 0 : b.n.bytes[0], tg.discard ? 0 : b.n.bytes[1], b.t_n}, b.dsl, plan.region_of[b.it]};
        if (bgzf) {
            // the text becomes BGZF blocks where it lies; their totals travel to pinned words behind ev_z, and the batch is shipped ONE
            // ITERATION LATER, when the host reads them without waiting while the GPU works on the next batch.
            for (int m = 0; m < (paired ? 2 : 1); ++m) sh.p[m] = bgzf_in_place(m, b.out[m], b.n.bytes[m], b.dsl, "BGZF: a batch's text exceeds 4 GB");
            if (!paired) { c->h_z[b.dsl * 3 + 1] = 0; sh.p[1] = nullptr; }
            HIP_OK(hipEventRecord(c->ev_z[b.dsl], s));
        }
        HIP_OK(hipEventRecord(c->ev_made[b.dsl], s));                               // the batch's text (its blocks) is complete ...
        if (bgzf) { if (have_pending) ship(pending); pending = sh; have_pending = true; } else ship(sh);
        ++bi;
    }
    void finish(uint64_t* n1_out, uint64_t* n2_out, uint64_t* pairs_out) {
        std::vector<uint64_t>* so[2] = {tg.seg_off1, tg.seg_off2};
        for (int m = 0; m < 2 && tg.seg_off1; ++m) {                               // the shard index.  Record order = batch order: the bytes before each batch
            if (!so[m]) continue;
            std::vector<uint64_t> pre(plan.nbatch + 1, 0);
            for (uint32_t b = 0; b < plan.nbatch; ++b) pre[b + 1] = pre[b] + bb[m][b];
            for (size_t j = 0; j < bpair.size(); ++j) (*so[m])[j] = tot[m];       // segments that start behind the last pair
            for (const SegAt& a : seg_at) (*so[m])[a.seg] = pre[a.b] + a.o[m];
        }
        // pairs produced = planned - holes; a hole arises only when > 1000 insert sizes in a row miss [readLength, ampliconLen]
        // (Amplicon.cpp:484-489): k_plan_pairs counted them on the device
        { Mail m; m.add(c->flags.p, 4, 30); m.add(c->dsums.as<unsigned long long>() + DS_HOLES, 8, 2); mail_post(c, m, true); }   // flags + hole count land before the final synchronize: no second round trip
        HIP_OK(hipStreamSynchronize(s));
        if (to_sink) { HIP_OK(hipStreamSynchronize(c->copy_stream)); guard.p = nullptr; const bool ok = c->pipe->finish(); c->pipe->truth_fd = -1; if (!ok) throw ScsError(SCS_EIO, truth ? "sink aborted (or the " + tname + " could not be written)" : std::string("sink aborted")); }
        if (truth) { truth_fd.finish("closing"); c->truth_bytes = truth_fd.total; }   // (BAM: the end-of-file block first)
        mail_wait(c); flags_eval(c);
        if (coverage_ref) coverage_ref_close(c);                                   // the sum identity: the net under a uint32 wrap of a reference base's depth
        if (c->want_cks && !tg.device && plan.nbatch) { c->cks.assign((size_t)plan.nbatch * 2, 0); HIP_OK(hipMemcpyAsync(c->cks.data(), c->d_cks.p, (size_t)plan.nbatch * 16, hipMemcpyDeviceToHost, s)); HIP_OK(hipStreamSynchronize(s)); }
        const uint64_t pairs_written = P - c->h_rb[2];
        for (KernelTimer* t : c->yield_timers()) t->collect();
        c->depth.valid = depth; c->support_valid = support; c->depth_ref.valid = depth_ref; c->cov.valid = coverage; c->cov_ref.valid = coverage_ref;
        c->st.pairs_written = pairs_written; c->st.reads_written = paired ? 2 * pairs_written : pairs_written;
        for (int m = 0; m < 2; ++m) { c->st.fastq_bytes[m] = tot[m]; c->st.sink_bytes[m] = to_sink ? sunk[m] : 0; }
        // 1526 B per created amplicon + per pair (insert size + FASTQ bytes of both records)
        const uint64_t per_pair_tmpl = paired ? (uint64_t)(c->cfg.isize + 1) : (uint64_t)L;
        c->st.algorithmic_bytes = 1526ull * (c->st.semi_amplicons + c->st.full_amplicons) + pairs_written * per_pair_tmpl + tot[0] + tot[1];
        if (n1_out) *n1_out = tot[0]; if (n2_out) *n2_out = tot[1]; if (pairs_out) *pairs_out = pairs_written;
        if (seam_env("SCS_PHASE_CLOCK")) phase_clock_report();                     // (prints only in a -DSCS_PHASE_CLOCK build)
        if (c->cfg.verbose) fprintf(stderr, "\nReads generation done!\n");
    }
};
}  // namespace

void do_yield(scs_ctx* c, const OutTarget& tg, uint64_t* n1_out, uint64_t* n2_out, uint64_t* pairs_out) {
    if (!c->allocated) throw ScsError(SCS_EINVAL, "scs_yield_reads: call scs_allocate_reads first");
    Yield y{c, tg}; const hipStream_t s = y.s; const uint64_t P = y.P;
    if (c->cfg.verbose) fprintf(stderr, "\n*****Producing reads*****\n");
    c->timing_gate = (c->yield_calls++ % c->timing_every) == 0;
    for (KernelTimer* t : c->yield_timers()) t->reset();
    c->depth.valid = false; c->support_valid = false; c->depth_ref.valid = false; c->cov.valid = false; c->cov_ref.valid = false;
    depth_yield_check(c);                                  // more than 2^27 bins, no lift table: refused before any GPU work
    // A paired-end job on a model whose [Insert Size Standard Deviation] is 0 has no insert-size alphabet (Profile.cpp:908: built only when
    // stdISize > 0); the reference's first yieldInsertSize then asks its Config for a parameter that does not exist and exit(1)s
    // (Profile.cpp:1482-1485 -> Config.cpp:85-93) -- after the amplification, with the output files opened and empty.  Same here, as an error code.
    if (y.paired && P > 0 && c->prof.isize_t.empty()) throw ScsError(SCS_EIO, "Error: unrecognized parameter name \"insertSize\"");
    c->pairs.reserve(std::max<size_t>(P * sizeof(PairRec), 16), s); HIP_OK(hipMemsetAsync(c->dsums.as<unsigned long long>() + DS_HOLES, 0, 8, s));
    if (y.truth) { truth_check(c, tg.device, y.to_sink ? tg.sink->writers : 1); if (!y.to_sink) throw ScsError(SCS_EINVAL, y.tname + ": the reads must go to a sink"); }
    if (y.bam) {                                                                   // what BAM's int32 fields and its bin scheme cannot hold: refused before any GPU work
        for (size_t r = 0; r < c->rec_len.size(); ++r)
            if (c->rec_len[r] >= (1ull << 29)) throw ScsError(SCS_EINVAL, "truth BAM (scs_set_truth_bam): record " + c->recs[r].name + " has 2^29 bases or more (the BAM bin scheme ends there); the truth SAM (scs_set_truth_sam) has no such limit");
        if ((y.paired ? 2 * P : P) > 0x7FFFFFFFull) throw ScsError(SCS_EINVAL, "truth BAM (scs_set_truth_bam): more than 2^31 - 1 records");
    }
    if (y.support) {                                                               // refused before any GPU work: a 32-bit counter could wrap
        support_check(c);
        if ((y.paired ? 2 * P : P) >> 32) throw ScsError(SCS_EINVAL, support_name(c) + ": 2^32 reads or more are planned (the counters are 32 bits wide)");
    }
    static const int batch_shift = seam_env("SCS_TEST_BATCH_SHIFT") ? atoi(seam_env("SCS_TEST_BATCH_SHIFT")) : 0;   // tests: many small batches
    y.plan = plan_batches(P, y.L, y.to_sink, y.to_sink ? tg.sink->writers : 1, y.to_sink ? tg.sink->regions : 1, batch_shift);
    y.setup();
    c->cks.clear(); if (c->want_cks && !tg.device) c->d_cks.reserve(std::max<size_t>((size_t)y.plan.nbatch * 16, 16), s);
    if (P) y.prepass(0);
    for (uint64_t it = 0; it < y.plan.nbatch; ++it) {
        mail_wait(c);                                                              // this batch's byte and class counts
        Batch b = y.decode(it);
        if (y.ps != s) HIP_OK(hipStreamWaitEvent(s, c->ev_pre[b.k], 0));           // (the host has seen the pre-pass' mail already: ordering for the device's sake)
        if (it + 1 < y.plan.nbatch) y.prepass(it + 1);                             // the next batch's pre-pass starts now, beside this batch's base pass
        y.index_batch(b);
        y.base_pass(b);
        if (y.truth) y.truth_batch(b);
        if (y.depth) y.depth_batch(b);
        if (y.depth_ref) y.depth_ref_batch(b);
        if (y.support) y.support_batch(b);
        if (y.cov_array) y.coverage_batch(b);
        if (y.ps != s) { HIP_OK(hipEventRecord(c->ev_free[b.k], s)); y.free_rec[b.k] = true; }   // this batch's buffer set is free for the pre-pass after next
        { const hipError_t le = take_launch_error(); if (le != hipSuccess) throw ScsError(SCS_EDEVICE, std::string("k_reads launch failed: ") + hipGetErrorString(le)); }
        if (y.to_sink) y.sink_batch(b);                                            // BGZF where asked; then to the region's writer (with BGZF: the batch before)
        for (int m = 0; m < 2; ++m) y.tot[m] += b.n.bytes[m];
    }
    if (y.have_pending) y.ship(y.pending);
    if (y.support) support_close(c);                                               // (the table on the reference: the staged counters summed by reference position)
    if (y.cov_array) y.coverage_finish();                                          // (the per-base depths and their histogram, before the call's last synchronise)
    y.finish(n1_out, n2_out, pairs_out);
}

void truth_check(scs_ctx* c, bool device, int writers) {
    if (c->truth_path.empty()) return;
    const std::string fn = c->truth_bam ? "scs_set_truth_bam" : c->truth_ref ? "scs_set_truth_ref_sam" : "scs_set_truth_sam",
                      what = (c->truth_bam ? "truth BAM (" : c->truth_ref ? "truth SAM on the reference (" : "truth SAM (") + fn + ")";
    if (device) throw ScsError(SCS_EINVAL, what + ": not available with scs_yield_reads_device; turn it off with " + fn + "(ctx, NULL)");
    if (c->cfg.shard_count > 1 || c->sliced) throw ScsError(SCS_EINVAL, what + ": not available for a sharded job (shard_count > 1)");
    if (writers > 1) throw ScsError(SCS_EINVAL, what + ": needs writers <= 1 (part files are made out of record order)");
    if (c->truth_ref && !c->have_lift) throw ScsError(SCS_EINVAL, what + ": the staged genome has no lift table; stage it with scs_simuvars, or read its table with scs_load_lift after staging");
}

void truth_ref_release(scs_ctx* c) {
    (void)hipStreamSynchronize(c->stream); if (c->copy_stream.s) (void)hipStreamSynchronize(c->copy_stream);   // nothing may still read them
    c->t_sizes.release(); c->t_offs.release(); c->t_scan.release(); c->t_out[0].release(); c->t_out[1].release(); c->t_recs.release(); c->t_refs.release();
    c->h_t.release(); c->ev_t.release();
    c->tm[TM_TRUTH].ev.clear(); c->tm[TM_TRUTH].used = 0; c->tm[TM_TRUTH].reset();
    if (c->pipe) for (auto& sl : c->pipe->slots) sl.h[2].release();                // (no writer runs between two yield calls)
}

}  // namespace scs
