/* scssim_hip.h -- C ABI of the MI355X-native `genreads` hot path.
 *
 * Drop-in boundary for qasimyu/scssim (reference paths below are relative to
 * the reference root).  The reference has no plugin/FFI layer: its genreads
 * driver (src/scssim.cpp:46-67) calls five methods on global objects.  Each
 * entry point here replaces one of those calls (or the pool job behind it), so
 * a maintainer swaps the bodies of those five calls for the functions below
 * (INTEGRATION.md shows the patch).  Plain C types only; every function
 * returns 0 on success or an SCS_E* code and never throws or exits.
 * One scs_ctx per host thread; a ctx owns one HIP device and one stream.
 */
#ifndef SCSSIM_HIP_H
#define SCSSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCS_OK          0
#define SCS_EINVAL      1   /* bad argument / call order                         */
#define SCS_EIO         2   /* file could not be opened / malformed (the reference exit(1)/exit(-1)s) */
#define SCS_EDEVICE     3   /* HIP error, no device, out of memory               */
#define SCS_EOVERFLOW   4   /* a fixed-size device work buffer overflowed (never silent) */

typedef struct scs_ctx scs_ctx;

/* Mirrors the reference's Config defaults (lib/config/Config.cpp:13-49) and the
 * genreads options (src/scssim.cpp:285-404). */
typedef struct scs_config {
    int      device;            /* HIP device ordinal                                  */
    void*    stream;            /* hipStream_t to run on, or NULL = ctx-owned stream   */
    uint64_t seed;              /* counter-RNG seed (the reference seeds from time(): scssim.cpp:47) */
    long     primers;           /* -p  [100000]                                        */
    double   gamma;             /* -r  [1e-9]                                          */
    double   coverage;          /* -c  [5]                                             */
    int      isize;             /* -s  [260]                                           */
    int      paired;            /* -l  PE=1 / SE=0 [1]                                 */
    double   ber;               /* Config "ber" 3.4e-4                                 */
    int      amplicon_min_len;  /* 1000                                                */
    int      amplicon_max_len;  /* 2000                                                */
    int      frag_size;         /* Config "fragSize" 1000 (weight denominator)         */
    int      frag_min;          /* Fragment::minSize 10000 (lib/fragment/Fragment.cpp:15-16) */
    int      frag_max;          /* Fragment::maxSize 100000                            */
    int      shard_rank;        /* this process' shard (fragment-lineage sharding)     */
    int      shard_count;       /* number of shards; 1 = whole job                     */
    int      verbose;           /* progress lines on stderr as the reference prints    */
} scs_config;

typedef struct scs_stats {
    uint64_t records, genome_bases, fragments, semi_amplicons, full_amplicons;
    uint64_t primers_left;       /* Malbac::totalPrimers after amplify                 */
    uint64_t reads_requested, pairs_written, reads_written;
    uint64_t fastq_bytes[2];
    uint64_t algorithmic_bytes;  /* 1526 B per created amplicon + per pair (isize + FASTQ bytes) */
    double   t_stage[8];         /* seconds: load, frags, amplify, weights, allocate, yield, -, total */
    uint64_t sink_bytes[2];      /* bytes handed to the sink per mate: fastq_bytes, or their BGZF blocks' (scs_yield_reads_files_ex) */
    uint64_t staged_bases;       /* bases resident on this GPU: genome_bases, or -- a shard of a sharded job loaded from an indexed FASTA --
                                    only the stretch its own fragments cover (scs_load_genome_fasta) */
    /* the primer stock of scs_amplify (Malbac::updatePrimerCount, lib/malbac/Malbac.cpp:91-103): passes whose demand was compared
     * with the stock (a pass that cannot reach the smallest stock is not), passes in which a primer type ran dry, and the
     * rounds it took to give such a type to exactly its first `stock` attachments in list order */
    uint64_t stock_checks, stock_exhausted_passes, stock_rounds;
} scs_stats;

void        scs_default_config(scs_config* cfg);
int         scs_create(const scs_config* cfg, scs_ctx** out);
void        scs_destroy(scs_ctx* ctx);
/* message of the last failure on ctx (or of the last failed scs_create when ctx == NULL) */
const char* scs_last_error(const scs_ctx* ctx);
int         scs_set_seed(scs_ctx* ctx, uint64_t seed);

/* Profile::train(file) = load + normParas(true) + initCDFs  (lib/profile/Profile.cpp:1432-1436).
 * Parses the .profile text, builds the CDF tables in double exactly as the reference, converts
 * every CDF entry to the exact uint32 draw threshold, uploads them.  Sets the read length. */
int         scs_load_profile(scs_ctx* ctx, const char* profile_path);
int         scs_read_length(const scs_ctx* ctx);

/* Genome::loadData for genreads = Genome::loadRefSeq (lib/genome/Genome.cpp:18-25,176-195):
 * simuvars-style FASTA (records <chr>_<hap>_<reflen>); ".gz" is inflated with `gzip -cd` as there. */
int         scs_load_genome_fasta(scs_ctx* ctx, const char* fasta_path);
/* A shard of a sharded job (shard_count > 1) stages only ITS OWN stretch of the genome when the file has a fastahack index beside
 * it (<fasta>.fai, not older than the file) that describes it (regular lines): the fragment split needs the record lengths alone
 * (lib/genome/Genome.cpp:753-782), so the shard reads, uploads, encodes and indexes just the byte ranges its fragments cover
 * (scs_stats.staged_bases).  The split depends on the seed: after scs_set_seed load the genome again (scs_create_frags says so).
 * Without a usable index the whole file is staged, which also writes the index. */
/* Same, from memory: names[i] as they appear after '>' ; seqs[i] = lens[i] ASCII bases. */
int         scs_upload_genome(scs_ctx* ctx, int n_records, const char* const* names,
                              const char* const* seqs, const uint64_t* lens);

/* Same, with the bases already in device memory (HBM-resident producers: a genome edited on the GPU, a synthetic
 * benchmark genome): d_bases = the records' ASCII bases concatenated without separators, sum(lens) bytes, readable
 * on the ctx device; copied, the caller keeps ownership. */
int         scs_upload_genome_device(scs_ctx* ctx, int n_records, const char* const* names, const uint64_t* lens,
                                     const void* d_bases);

/* `scssim simuvars` (src/scssim.cpp:33-38, 108-170) on the data plane: Genome::loadData (loadAbers lib/genome/Genome.cpp:35-165,
 * loadSNPs -> lib/snp/snp.cpp:147-203, loadRefSeq 176-195) + Genome::saveSequence (329-384) / generateSegment (386-691).
 * ref_fasta: plain reference (records chr<k>); snp_file / var_file: the reference's formats, either may be NULL.
 * The host only plans (segments, copies, substitutions, insertions, deletions as a list of pieces; the reference's rand()
 * draws reproduced); the two haplotypes of every chromosome are built in HBM from the resident reference and stay resident
 * exactly as if scs_load_genome_fasta had read the simuvars output -- genreads can follow with no intermediate FASTA.
 * out_fasta != NULL additionally writes that file, byte-identical to the reference's (records <chr>_<hap>_<reflen>, 100 columns). */
int         scs_simuvars(scs_ctx* ctx, const char* ref_fasta, const char* snp_file, const char* var_file, const char* out_fasta);

/* Malbac::createFrags -> Genome::splitToFrags + Fragment::createSequence
 * (lib/malbac/Malbac.cpp:143-145, lib/genome/Genome.cpp:753-782, lib/fragment/Fragment.cpp:40-50) */
int         scs_create_frags(scs_ctx* ctx);

/* Malbac::amplify (lib/malbac/Malbac.cpp:173-201): createPrimers, setPrimers, and the 1+5 cycles of
 * Fragment::batchAmplify / Amplicon::batchAmplify pool jobs (Fragment.cpp:52-152, Amplicon.cpp:156-253).
 * Amplicons stay resident in HBM. */
int         scs_amplify(scs_ctx* ctx);

/* Malbac::setReadCounts (Malbac.cpp:370-408) incl. Amplicon::getWeightedLength (Amplicon.cpp:396-400),
 * Profile::getGCFactor (Profile.cpp:1503-1513) and randIndx_hp/batchSampling (MyDefine.cpp:191-272).
 * reads == 0: derive it from the record names and coverage as Malbac::yieldReads does (Malbac.cpp:413-420). */
int         scs_allocate_reads(scs_ctx* ctx, uint64_t reads);

/* Sink = SeqWriter::write(char*) / write(char*,char*) (lib/seqwriter/SeqWriter.cpp:41-54).
 * Called in output order with host buffers valid only during the call; fq2/n2 are NULL/0 for SE.
 * Return non-zero to abort. */
typedef int (*scs_sink_fn)(void* user, const char* fq1, size_t n1, const char* fq2, size_t n2);

/* Malbac::yieldReads fan-out + Amplicon::yieldReads jobs (Malbac.cpp:436-457, Amplicon.cpp:402-565)
 * with Profile::predict (Profile.cpp:1582-1697) per read.  FASTQ text is produced on the device
 * and handed to `sink` batch by batch (sink may be NULL: generate and count only). */
int         scs_yield_reads(scs_ctx* ctx, scs_sink_fn sink, void* user);

/* Same, but the FASTQ pool stays in HBM in caller-owned device buffers (for the RCCL gather of the
 * read pool).  Fails with SCS_EOVERFLOW if a capacity is too small; n1 / n2 receive the byte counts. */
int         scs_yield_reads_device(scs_ctx* ctx, void* d_fq1, size_t cap1, void* d_fq2, size_t cap2,
                                   uint64_t* n1, uint64_t* n2, uint64_t* pairs);

/* createFrags + amplify + allocate + yield in one call (the body of main()'s genreads branch,
 * src/scssim.cpp:59-65). */
int         scs_run_genreads(scs_ctx* ctx, scs_sink_fn sink, void* user);

int         scs_get_stats(const scs_ctx* ctx, scs_stats* out);

/* Integrity of text that never leaves the GPU (a NULL sink) or crosses PCIe: with on != 0 every batch of the next scs_yield_reads /
 * scs_yield_reads_files gets a 64-bit checksum per mate, computed by a kernel where the text lies in HBM -- the text as
 * little-endian 64-bit words w_i (the last zero-padded): sum_i fmix64(w_i + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64, fmix64 = the
 * MurmurHash3 finaliser.  scs_batch_checksums: out[2 b], out[2 b + 1] = batch b's two mates, in record order (cap: entries of
 * out); *n_batches = batches of the last call.  Not computed for scs_yield_reads_device. */
int         scs_set_batch_checksums(scs_ctx* ctx, int on);
int         scs_batch_checksums(const scs_ctx* ctx, uint64_t* out, size_t cap, size_t* n_batches);

/* ---- one job over several GPUs (scs_config.shard_rank / shard_count: fragment-lineage sharding) -------------
 * The reference is single-process; these are the exchange steps its globals imply once fragments are split over
 * ranks: Malbac::setPrimers totals (Malbac.cpp:242-262,282), the primer stock (Malbac.cpp:91-103) and the weight
 * normalisation / chunked sampling of Malbac::setReadCounts (Malbac.cpp:370-408).  The caller supplies them
 * (torch.distributed over RCCL or gloo: scssim_amd/dist.py); buffers are host memory.
 *   allreduce : element-wise sum of n uint64 values in place over all shards
 *   allgatherv: every shard sends send_bytes; recv has shard_count slots of stride_bytes; sizes[r] = bytes of shard r
 * With the hooks set, a sharded job writes record names / read counts identical to the unsharded job; each shard's
 * FASTQ pool is sorted by the amplicon index in the record name, so the writer k-way merges the pools. */
typedef int (*scs_allreduce_fn)(void* user, uint64_t* vals, uint64_t n);
typedef int (*scs_allgatherv_fn)(void* user, const void* send, uint64_t send_bytes, void* recv, uint64_t stride_bytes, uint64_t* sizes);
int         scs_set_collectives(scs_ctx* ctx, scs_allreduce_fn allreduce, scs_allgatherv_fn allgatherv, void* user);
/* Device-memory variants, ordered on the ctx stream (no host sync): used for the per-cycle scalars, the per-pass
 * primer-stock decrements and the weight gather when set; the host hooks above remain the fallback.
 *   allreduce_dev: sum n elements of elem_bytes (4 = uint32, 8 = uint64) in place
 *   allgather_dev: d_recv[r * bytes_per_rank ..] = shard r's d_send[0 .. bytes_per_rank) */
typedef int (*scs_allreduce_dev_fn)(void* user, void* d_vals, uint64_t n, int elem_bytes);
typedef int (*scs_allgather_dev_fn)(void* user, const void* d_send, void* d_recv, uint64_t bytes_per_rank);
int         scs_set_collectives_device(scs_ctx* ctx, scs_allreduce_dev_fn allreduce_dev, scs_allgather_dev_fn allgather_dev, void* user);

/* RCCL inside the library (one process per GPU; no caller-side hooks needed).  Rank 0 obtains an id (ncclGetUniqueId) and
 * hands its SCS_COMM_ID_BYTES to the other ranks by any means (a pipe, a file, MPI, torch.distributed); every rank then
 * calls scs_comm_init on its ctx (ncclCommInitRank on the ctx device).  From then on the exchanges above run as RCCL
 * all-reduce / all-gather on the ctx stream.  RCCL is bound at run time (dlopen), so the library loads without it. */
#define SCS_COMM_ID_BYTES 128
int         scs_comm_unique_id(void* id_out);
int         scs_comm_init(scs_ctx* ctx, const void* id, int rank, int nranks);
/* ranks of the ctx's communicator as RCCL reports them (ncclCommCount); 0 without a communicator */
int         scs_comm_count(const scs_ctx* ctx);
/* ncclCommAbort on the ctx's communicator, callable from ANOTHER thread than the one blocked in a collective: how a driver
 * that has seen a rank die releases its own rank before it leaves (the ctx is only good for scs_destroy afterwards) */
int         scs_comm_abort(scs_ctx* ctx);

/* ---- FASTQ straight to files (SeqWriter, lib/seqwriter/SeqWriter.cpp:12-64; opened by Malbac::yieldReads, Malbac.cpp:426-435)
 * writers <= 1: the reference's files.  Whole job (shard_count == 1): <prefix>_1.fq / <prefix>_2.fq, or <prefix>.fq for SE.
 * Sharded job: this shard's records go to <prefix>.r<rank>_1.fq / _2.fq (.fq) and <prefix>.r<rank>.idx lists the byte offset
 * at which each of the shard's list segments starts.  The whole job's file is the shards' segments interleaved in list
 * order, so scs_merge_fastq_shards rebuilds it by copying byte ranges (copy_file_range, a few threads) -- it parses no
 * record -- and the result equals the unsharded job's files byte for byte.
 * writers = K > 1 (at most 64): buffered writes into ONE file serialise on its inode lock (5.7 GB/s per file on the GPU
 * box's tmpfs whatever the thread count), so the job's (shard's) records are cut into K contiguous ranges, made round-robin,
 * and written by K threads into K PART files per mate: <base>.p00_1.fq ... <base>.p<K-1>_1.fq (+ _2.fq; .p<kk>.fq for SE),
 * base = <prefix> or <prefix>.r<rank>.  Their concatenation in that order IS the single file (`cat <base>.p*_1.fq`);
 * <base>.parts lists their sizes; scs_merge_fastq_parts / scs_merge_fastq_shards read parts and single files alike. */
int         scs_yield_reads_files(scs_ctx* ctx, const char* prefix, int writers);
/* The same with two more choices.
 * generations = G > 1: writers x G parts per mate, made generation by generation (the first `writers` parts, then the next ...):
 *   part p is complete -- closed, final -- as soon as part p + writers exists, so a consumer can stream the early parts while the
 *   job runs and the page cache holds a couple of generations instead of the whole job's text (at most 99 parts).
 * bgzf != 0: the files are <...>.fq.gz in BGZF (blocked gzip: what `bgzip` writes; gzip / zcat, htslib, bwa, samtools read it).
 *   The blocks are made ON THE GPU from the text where it lies in HBM (scs_bgzf.hip: one dynamic-Huffman deflate block of
 *   literals per 63 KB of text, CRC-32 included), so 3-4x fewer bytes cross PCIe and reach the file system -- the two walls of a
 *   job.  `zcat` of a part is the text of that part; every part ends with the BGZF end-of-file block.  An extension: the
 *   reference writes plain text only.  The shards of a sharded job stay shards (compressed byte ranges cannot be spliced).
 * flags: SCS_SINK_BGZF (1; `bgzf` was this argument's name when it was the only choice) | SCS_SINK_IN_PLACE (2): output files that
 *   exist already are not truncated when they are opened (what `ofstream` does, SeqWriter.cpp:17-30) but overwritten where they lie
 *   and cut to their new length when they are finished -- the same files in the end, and a job that replaces the files of an earlier
 *   one does not pay for giving their pages back and taking them again.  Until a file is finished its tail is the old file's.
 *   With generations > 1 the "part p + writers exists => part p is final" signal is kept: the call first renames the earlier job's
 *   files of the LATER generations to <name>.prev, and each comes back under its name (its pages kept) when its part's first batch
 *   arrives; no .prev file is left when the call returns. */
#define SCS_SINK_BGZF     1
#define SCS_SINK_IN_PLACE 2
int         scs_yield_reads_files_ex(scs_ctx* ctx, const char* prefix, int writers, int generations, int flags);
int         scs_merge_fastq_shards(const char* prefix, int nranks, int paired, int keep_shards, char* errbuf, size_t errlen);
/* host only: <prefix>.p*_1.fq ... -> <prefix>_1.fq ... (byte-range copies; parts removed unless keep_parts) */
int         scs_merge_fastq_parts(const char* prefix, int paired, int keep_parts, char* errbuf, size_t errlen);

/* ---- truth SAM: where every read came from --------------------------------------------------------------------------
 * scs_set_truth_sam(ctx, path): the following yield calls also write each read's true alignment to `path` as plain-text SAM
 * (NULL: off, the default).  Header: @HD VN:1.6 SO:unsorted, one @SQ per staged genome record (staging order), @PG ID:scssim.
 * One record per FASTQ record, in FASTQ order (read 1 then its read 2): QNAME = the FASTQ name without '@' and /1 /2; FLAG
 * 0x1|0x2|0x40/0x80 (+0x10 reverse, +0x20 mate reverse) for PE, 0 / 0x10 for SE; RNAME / POS in the staged (haplotype) records;
 * MAPQ 255; CIGAR from the read's indel events (Profile::predict), genome-forward; RNEXT '=' / PNEXT / TLEN (+ on the leftmost
 * read) for PE, '*' 0 0 for SE; SEQ / QUAL the FASTQ's, reverse-complemented / reversed for 0x10; NM:i and MD:Z against the
 * staged record (amplification and sequencing errors alike).  The records are made on the GPU after each batch's reads and
 * written by the sink's writer thread.  Applies to scs_yield_reads (any sink, NULL included), scs_yield_reads_files(_ex) with
 * writers <= 1 and scs_run_genreads; a sharded ctx, writers > 1 and scs_yield_reads_device fail with SCS_EINVAL.
 * scs_truth_bytes: SAM bytes of the last yield call (header included). */
int         scs_set_truth_sam(scs_ctx* ctx, const char* path);
int         scs_truth_bytes(const scs_ctx* ctx, uint64_t* bytes);
/* scs_set_truth_bam(ctx, path): the same records, in the same order, from the same calls, as BAM (NULL: off, the default).  The
 * header (magic, the SAM's header text, the record table) is made on the host, the records on the GPU, where they also become
 * BGZF blocks; the file ends with the 28-byte BGZF end-of-file block (a job with no reads writes the header and that block).
 * refID = index of the staged record, pos = POS - 1, mapq 255, bin = reg2bin(pos, end), CIGAR ops len << 4 | (M 0, I 1, D 2),
 * next_refID / next_pos = refID / PNEXT - 1 (PE) or -1 / -1 (SE), SEQ 4 bits per base, QUAL = Phred, tags NM:i (int32) and MD:Z.
 * At most one truth output per ctx: setting one while the other is on fails with SCS_EINVAL; NULL clears only its own.  A staged
 * record of 2^29 bases or more (the BAM bin scheme ends there) and more than 2^31 - 1 records fail with SCS_EINVAL before any
 * GPU work.  scs_truth_bytes then reports the BAM file's size (compressed; header and end-of-file block included), and
 * scs_kernel_time(which = 6) the BAM passes with their BGZF launches. */
int         scs_set_truth_bam(scs_ctx* ctx, const char* path);
/* scs_set_truth_ref_sam(ctx, path): a third truth output (NULL: off, the default -- no code of it runs): a plain-text SAM whose
 * records are aligned to the ORIGINAL REFERENCE the lift table names (see "lift table" below), made on the GPU from the
 * haplotype alignment and the table.  Still at most one truth output per ctx: setting one while another is on fails with
 * SCS_EINVAL and names both; NULL clears only its own (and frees what its yield calls allocated).  It applies where the truth
 * SAM does; a sharded ctx, writers > 1, scs_yield_reads_device and a ctx without a lift table (scs_simuvars keeps one,
 * scs_load_lift reads one) fail the yield call with SCS_EINVAL.  It works beside the depth tracks and the site support.
 * scs_truth_bytes and scs_kernel_time(which = 6) report it as they do the SAM.
 * Header: @HD VN:1.6 SO:unsorted, one @SQ SN LN per reference record of the table in its order, @PG ID:scssim PN:scssim.
 * One record per FASTQ record, in FASTQ order; QNAME, SEQ, QUAL, their orientation and the 0x10 / 0x20 bits are the haplotype
 * SAM's (simuvars makes no inversions).  The haplotype CIGAR is walked with a cursor through the segment table: M in an R
 * segment stays M at ref_pos + (g - hap_off), M in an I segment and a sequencing insertion are I, D in an R segment stays D, D in
 * an I segment is nothing.  Going from R segment s to the next R segment t it touches, the walk emits D of t.ref_pos - (s.ref_pos +
 * s.len) bases when t.ref_rec == s.ref_rec and that is >= 0 (collinear: a planted deletion, a CN-0 stretch); any other junction
 * (the jump back between tandem copies, another reference record) is a cut, and cuts split the read into blocks.  The record
 * shows the PRIMARY block -- the one with the most M bases, the first on a tie: the read bases from its first to its last M base
 * keep their ops (merged by kind), every base outside is soft-clipped (S), D at the block's edges is dropped; POS = the first M
 * base's reference coordinate + 1, RNAME its reference record, MAPQ 255.  A read with no lifted M base (wholly in inserted
 * sequence) is unmapped: FLAG |= 0x4, MAPQ 0, CIGAR *, RNAME / POS the mate's when that is mapped, else * 0.  Mate fields come
 * from the two primary blocks: 0x1, 0x40 / 0x80; 0x8 when the mate is unmapped; 0x2 only when both are mapped to one reference
 * record; RNEXT '=' on the same record, the mate's name on another, '*' when neither is mapped; PNEXT the mate's POS (the read's
 * own when only the mate is unmapped); TLEN +-(rightmost reference end - leftmost reference start + 1) when both are mapped to
 * one record (+ on the smaller POS, on read 1 on a tie), else 0.  SE: '*' 0 0.  Tags: YH:Z the haplotype record's name and YP:i
 * the haplotype POS (the join key to the haplotype SAM and the amplicon table), YB:i the number of blocks (0: unmapped).  There
 * is no NM / MD: against the reference they need the reference's bases under the planted SNPs and deletions, which genreads
 * never stages.  A read that cannot be lifted (placed outside its record, a walk that leaves the table or its record's segments,
 * a segment that lifts outside its reference record) fails the call (SCS_EOVERFLOW), never writes a wrong record. */
int         scs_set_truth_ref_sam(scs_ctx* ctx, const char* path);
/* ---- depth track: binned read and base counts of the job, made on the GPU ----------------------------------------------
 * scs_set_depth(ctx, bin_width): the following yield calls also count, per bin of bin_width >= 1 bases of the staged genome, the
 * reads that start in the bin and the bases aligned in it (0: off, the default -- no buffer exists, no depth code runs).  Record r
 * of len_r bases has ceil(len_r / bin_width) bins, bin k covering record coordinates [k bin_width, min((k + 1) bin_width, len_r));
 * no bin straddles two records; bins are numbered record by record in staging order.  More than 2^27 bins (two uint64 counters
 * each: 2 GB) fail the yield call with SCS_EINVAL before any GPU work; the message names the smallest admissible width.
 * Both counters follow the alignment the truth SAM writes: `reads` = FASTQ records whose leftmost aligned genome base (POS - 1)
 * lies in the bin; `bases` = (record, genome base) pairs aligned by an M operation with the base in the bin -- deleted and
 * inserted bases count nothing.  Reads without a FASTQ record count nothing; both mates of a pair count.  So the sum of `reads`
 * is scs_stats.reads_written.  The counters are sums of integers: they do not depend on batch cuts, the sink, its writers or
 * whether the text leaves the GPU.  Zeroed at the start of every yield call, they hold that call's job afterwards.
 * Applies to every yield entry point and sink (scs_yield_reads with any sink or NULL, scs_yield_reads_files(_ex) with any
 * writers / generations / flags, scs_yield_reads_device, scs_run_genreads), beside either truth output.  A sharded ctx
 * (shard_count > 1) fails the yield call with SCS_EINVAL; scs_set_depth(ctx, 0) makes it usable again.
 * scs_depth_bins: the layout for the staged genome (SCS_EINVAL: depth off, no genome staged, or too many bins).
 * scs_depth_record_bins: bin_off[r] = first bin of staged record r, records + 1 entries (SCS_EOVERFLOW: cap is smaller).
 * scs_download_depth: the counters of the last yield call, n_bins entries each; either pointer may be NULL; SCS_EINVAL before a
 * yield call with depth on has finished, SCS_EOVERFLOW when cap < n_bins; synchronises the ctx stream itself.
 * scs_write_depth: the same as tab-separated text written by the host: the line "#record\tstart\tend\treads\tbases", then one
 * line per bin, start 0-based and end exclusive (BED coordinates), record names as scs_fasta_probe reports them.
 * scs_kernel_time(which = 7) is the depth kernel: one event pair per batch, units = pairs. */
int         scs_set_depth(scs_ctx* ctx, uint32_t bin_width);
int         scs_depth_bins(const scs_ctx* ctx, uint64_t* n_bins, uint32_t* bin_width);
int         scs_depth_record_bins(const scs_ctx* ctx, uint64_t* bin_off, uint64_t cap);
int         scs_download_depth(scs_ctx* ctx, uint64_t* reads, uint64_t* bases, uint64_t cap);
int         scs_write_depth(scs_ctx* ctx, const char* path);
/* Host-only test seams of the depth track (no GPU, no ctx).  scs_depth_layout_probe: the layout function the ctx runs, the 2^27
 * refusal included (SCS_EINVAL; the text in scs_last_error(NULL)): bin_off[r] = first bin of record r (n_records + 1 entries; may
 * be NULL), *n_bins their total.  It allocates nothing that grows with the number of bins.
 * scs_depth_read_probe: one read through the function the kernel runs.  n, pos0, reverse, events, nev as for
 * scs_truth_record_probe (pos0 = 0-based record coordinate of window base 0); rec_len = bases of the record.  *reads_bin = the bin
 * (inside the record) that receives the `reads` increment; bins[i] / bases[i], i < *n_out: the `bases` increments in ascending
 * bin order, each bin once.  SCS_EINVAL: not a valid alignment, or not inside the record; SCS_EOVERFLOW: cap entries are too few
 * (*n_out is set). */
int         scs_depth_layout_probe(const uint64_t* rec_lens, int n_records, uint32_t bin_width, uint64_t* bin_off, uint64_t* n_bins);
int         scs_depth_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev, uint64_t rec_len, uint32_t bin_width,
                                 uint64_t* reads_bin, uint64_t* bins, uint32_t* bases, int cap, int* n_out);
/* ---- coverage profile: per-base depth of the job, its histogram per record and a Lorenz summary, made on the GPU ---------
 * scs_set_coverage(ctx, max_depth): the following yield calls also keep depth[g] for every base g of the staged genome: the
 * (read, base) pairs an M operation of the truth CIGAR aligns to g (0: off, the default -- no buffer exists, no coverage code
 * runs; max_depth D in 1 .. 65535).  The rules are those of the depth track's `bases`: D and I count nothing, leading and trailing
 * deletions are dropped, reads without a FASTQ record count nothing, both mates of a pair count.  So the depths of a bin of
 * scs_set_depth add up to its `bases`, those of the genome to the sum of the M lengths.  Per staged record r, hist[r][k], k = 0 ..
 * D, counts its non-N bases of depth k, the last bucket those of depth >= D; N bases are in no bucket.  n_bases[r] = its N bases,
 * sum[r] / sum_n[r] = the exact sum of the depths over its non-N / its N bases (so the top bucket's mass is
 * sum - sum_{k < D} k hist[k]).  One more row, the genome, is the sum of the records' rows.  Sums of integers: nothing depends on
 * batch cuts, the sink, its writers or whether the text leaves the GPU.  The arrays are zeroed on the ctx stream at the start of
 * every yield call and valid once it has returned; scs_set_coverage(ctx, 0) (or another max_depth) releases them.  Device memory:
 * 4 bytes per staged base, rounded up to 16 KB; where it cannot be had the yield call fails as any allocation does, its message
 * stating the bytes.  Applies to every yield entry point and sink, beside either truth output, both depth tracks and the site
 * support.  A sharded ctx (shard_count > 1) fails the yield call with SCS_EINVAL naming this setter, before any GPU work.  A
 * read outside its record, a read with more than 32 indel events, a negative running depth or one that is not 0 behind the
 * last base fail the call (SCS_EOVERFLOW), never give a wrong count.
 * scs_coverage_shape: the staged records and max_depth (SCS_EINVAL: off, or no genome staged).
 * scs_download_coverage: records + 1 rows, the genome's last; hist row-major, max_depth + 1 values per row; any pointer may be
 * NULL; SCS_EINVAL before a yield call with coverage on has finished, SCS_EOVERFLOW when cap_rows < records + 1; synchronises the
 * ctx stream itself.
 * scs_coverage_range: the depths of [start, end) of staged record `record`, copied from the device array (SCS_EINVAL: not inside
 * the record, or no finished call).
 * scs_write_coverage: text written by the host.  "#coverage\tmax_depth=D\t..." states that the last bucket counts depth >= D;
 * "#summary\trecord\tbases\tn_bases\taligned\tmean\tbreadth1\tbreadth5\tbreadth10\tbreadth20\tgini" heads one "#s\t..." line per
 * record and one for `genome`: bases = all its bases, aligned = sum + sum_n, mean and the breadths (fractions at depth >= 1, 5,
 * 10, 20; a threshold above D counts the top bucket) over the non-N bases; then "#record\tdepth\tcount\tsize\tfraction" and
 * `bedtools genomecov`'s five columns for every bucket with count > 0 (size = the record's non-N bases), the genome's rows last.
 * gini is computed from the histogram with the top bucket at its mean depth: exact when no base reaches D, a lower bound
 * otherwise; 0 when all depths are 0 or the record has no non-N base.
 * scs_coverage_kernel_time: which = 0 the per-batch pass (one event pair per batch, units = pairs), 1 the end-of-job pass (one
 * pair, units = staged bases) of the last yield call; not part of scs_kernel_time's table. */
int         scs_set_coverage(scs_ctx* ctx, uint32_t max_depth);
int         scs_coverage_shape(const scs_ctx* ctx, uint32_t* records, uint32_t* max_depth);
int         scs_download_coverage(scs_ctx* ctx, uint64_t* hist, uint64_t* n_bases, uint64_t* sum, uint64_t* sum_n, uint64_t cap_rows);
int         scs_coverage_range(scs_ctx* ctx, uint32_t record, uint64_t start, uint64_t end, uint32_t* out);
int         scs_write_coverage(scs_ctx* ctx, const char* path);
int         scs_coverage_kernel_time(const scs_ctx* ctx, int which, uint64_t* launches, double* ms, uint64_t* units);
/* Test seams of the coverage profile.  scs_coverage_read_probe (host only): one read through the function the per-batch kernel
 * runs; arguments as scs_depth_read_probe; [starts[i], ends[i]), i < *n_out: the intervals of record coordinates it marks,
 * ascending (SCS_EINVAL: not a valid alignment inside the record, or more than 32 events; SCS_EOVERFLOW: cap is too small, *n_out
 * is set).  scs_coverage_stats_probe (host only): one histogram row of max_depth + 1 buckets and its sum through the function
 * scs_write_coverage runs; out = mean, the four breadths, gini.  scs_coverage_tile: the end-of-job pass' tile and the chunk of
 * its tile-offset scan.  scs_coverage_finish_probe (needs the GPU): the end-of-job kernels alone over diff[n_bases + 1],
 * codes[n_bases] (0 .. 3, 4 = N) and records of rec_lens (adding up to n_bases); lds_buckets: buckets of a workgroup's LDS
 * histogram (< 0: the product's; 0: none); depth[n_bases], hist[n_records][max_depth + 1], n_n / sum / sum_n[n_records], any of
 * them NULL.  Differences that are not those of intervals give the flag's error (SCS_EOVERFLOW), and the ctx stays usable. */
int         scs_coverage_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev, uint64_t rec_len,
                                    uint64_t* starts, uint64_t* ends, int cap, int* n_out);
int         scs_coverage_stats_probe(const uint64_t* hist, uint32_t max_depth, uint64_t sum, double out[6]);
void        scs_coverage_tile(uint32_t* tile, uint32_t* chunk);
int         scs_coverage_finish_probe(scs_ctx* ctx, const int32_t* diff, const uint8_t* codes, uint64_t n_bases, const uint64_t* rec_lens, uint32_t n_records,
                                      uint32_t max_depth, int lds_buckets, uint32_t* depth, uint64_t* hist, uint64_t* n_n, uint64_t* sum, uint64_t* sum_n);
/* ---- coverage profile on the reference: the per-base depth an aligner's pile-up is compared with --------------------------
 * scs_set_coverage_ref(ctx, max_depth): the following yield calls also keep, for every base p of the reference records the lift
 * table names (scs_simuvars, scs_load_lift), ref_depth[p] (uint32) = the sum of the staged depths (scs_set_coverage's depth[g]) of
 * every staged base in an R segment that lifts to p: every haplotype and every tandem copy counts, and a read over two copies of
 * p counts twice, as its pieces do in scs_set_depth_ref's `bases`.  0: off, the default -- no buffer exists, no code of it runs;
 * max_depth D in 1 .. 65535, independent of scs_set_coverage's.  The depths are lifted ONCE, at the end of the job: the batches
 * mark the staged difference array, the staged end-of-job pass makes the staged depths, two more kernels carry them through the
 * table and count them.  So this switch brings the staged array and its pass whether or not scs_set_coverage is on (one array,
 * one marking pass per batch with both on); scs_download_coverage, scs_coverage_range and scs_write_coverage still need
 * scs_set_coverage (and while this switch is on, scs_set_coverage with another max_depth releases the staged tables only: the
 * array stays).  Staged bases of I segments have no reference coordinate: their depths are summed into `unlifted`, so
 * sum ref_depth + unlifted = sum of the staged depths = sum of the truth CIGARs' M lengths.  The host checks this equality
 * (uint64 on both sides) when the call ends and fails the call with the coverage profile's flag error (SCS_EOVERFLOW) where it
 * does not hold: that check is also the net under a uint32 wrap of one reference base's depth.
 * Per reference base, made once per (genome, lift table): copies[p] = the staged bases that lift to p (the per-base true copy
 * number), n_copies[p] = those of them that are N; 16 bits each in one uint32.  A table that could put more than 65535 staged
 * bases on one reference base fails the call (SCS_EOVERFLOW) before any kernel runs.  Classes: N -- copies > 0 and every copy
 * is N, in no bucket; absent -- copies = 0 (copy number 0 on every haplotype), counted in bucket 0 because no read can cover it
 * and `genomecov` on aligned reads shows it so, and reported as `absent`, so hist[0] - absent is the uncovered present sequence;
 * counted -- everything else (mixed N and non-N copies count as sequence).  The reference's own bases are never staged: an N gap
 * under a CN-0 stretch cannot be told from sequence.
 * Tables per reference record and a last `genome` row: hist[r][0 .. D] (the last bucket depth >= D), n_bases, absent, sum, sum_n
 * (exact), and depth by copy number: cn_bases[r][c], cn_sum[r][c], c = 0 .. 16 (the last one copies >= 16) over the non-N bases,
 * cn_sum / cn_bases the mean depth at true copy number c; cn_bases[r][0] = absent[r].
 * Device memory: 8 bytes per reference base beside scs_set_coverage's 4 per staged base; an allocation that fails states the
 * bytes.  Every yield entry point and sink; one GPU.  A sharded ctx, or a ctx without a lift table, fails the yield call with
 * SCS_EINVAL naming this setter (and scs_load_lift / scs_simuvars) before any GPU work.  A segment that lifts outside its
 * reference record adds nothing and fails the call (the lift flag's error).  Staging another genome or installing another table
 * invalidates the arrays and has the copies remade; scs_set_coverage_ref(ctx, 0) (or another max_depth) releases them.
 * scs_coverage_ref_shape: the reference records and max_depth (SCS_EINVAL: off, or no lift table).
 * scs_download_coverage_ref: ref_records + 1 rows, the genome's last; hist max_depth + 1 values per row, cn_bases / cn_sum 17;
 * any pointer may be NULL; errors as scs_download_coverage.
 * scs_coverage_ref_range: ref_depth and copies of [start, end) of reference record ref_record, from the device arrays; either
 * output may be NULL.
 * scs_write_coverage_ref: scs_write_coverage's text with the reference's record names: the "#coverage" line;
 * "#summary\trecord\tbases\tn_bases\tabsent\taligned\tmean\tbreadth1\tbreadth5\tbreadth10\tbreadth20\tgini" and a "#s" line per
 * record and for `genome`; "#cn\trecord\tcopies\tbases\taligned\tmean" and a "#c" line for every (record, c) with bases;
 * "#unlifted\t<aligned bases>\t<inserted bases>"; then genomecov's five columns.
 * scs_coverage_ref_kernel_time: which = 0 the once-per-layout copies kernel (no launch when the layout stands), 1 the end-of-job
 * lift and count, units = staged bases; not part of scs_kernel_time's table.
 * scs_coverage_ref_finish_probe (test seam, needs the GPU): the three kernels alone, as the product launches them, over staged
 * depths and codes of n_staged bases, a table in scs_lift_segments' layout that tiles staged records of hap_lens, and reference
 * records of ref_lens; lds_buckets as scs_coverage_finish_probe.  ref_depth / packed (copies | n_copies << 16) per reference
 * base, the tables with n_ref rows, *unlifted; any output may be NULL.  The sum identity is checked as in a yield call. */
int         scs_set_coverage_ref(scs_ctx* ctx, uint32_t max_depth);
int         scs_coverage_ref_shape(const scs_ctx* ctx, uint32_t* ref_records, uint32_t* max_depth);
int         scs_download_coverage_ref(scs_ctx* ctx, uint64_t* hist, uint64_t* n_bases, uint64_t* absent, uint64_t* sum, uint64_t* sum_n,
                                      uint64_t* cn_bases, uint64_t* cn_sum, uint64_t* unlifted, uint64_t cap_rows);
int         scs_coverage_ref_range(scs_ctx* ctx, uint32_t ref_record, uint64_t start, uint64_t end, uint32_t* depth_out, uint32_t* copies_out);
int         scs_write_coverage_ref(scs_ctx* ctx, const char* path);
int         scs_coverage_ref_kernel_time(const scs_ctx* ctx, int which, uint64_t* launches, double* ms, uint64_t* units);
int         scs_coverage_ref_finish_probe(scs_ctx* ctx, const uint32_t* depth, const uint8_t* codes, uint64_t n_staged,
                                          const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                                          const uint64_t* hap_lens, uint32_t n_hap, const uint64_t* ref_lens, uint32_t n_ref, uint32_t max_depth, int lds_buckets,
                                          uint32_t* ref_depth, uint32_t* packed, uint64_t* hist, uint64_t* n_n, uint64_t* absent, uint64_t* sum, uint64_t* sum_n,
                                          uint64_t* cn_bases, uint64_t* cn_sum, uint64_t* unlifted);
/* ---- the per-base arrays as bedGraph: depth and true copy number as files a genome browser and bedtools read ---------------
 * After a yield call the device holds three per-base uint32 arrays: the staged depths (scs_set_coverage), the reference depths and
 * the per-base true copy number of the reference (scs_set_coverage_ref: the packed word's lower 16 bits).  Each write call below
 * encodes one of them on the GPU as plain bedGraph: lines "name\tstart\tend\tvalue\n", 0-based and half-open, no `track` line, no
 * header; one line per maximal run of equal value inside a record, runs of value 0 included (`bedtools genomecov -bga`), so the
 * lines of a record tile it exactly -- the first starts at 0, consecutive lines abut, the last ends at the record's length,
 * neighbouring lines of one record differ in value -- and a run never crosses a record border, even between equal values.
 * Records in staged (reference) order; N bases carry their depth like any base; values are exact, never clamped by max_depth.
 * The value is compared and printed under a mask (0xFFFFFFFF for depths, 0xFFFF for copies: neighbours that differ only in the
 * packed word's upper half are one run).  A path ending in .gz is written in BGZF made on the GPU, ending with BGZF's end-of-file
 * block.  lines / text_bytes (either may be NULL): the lines written and their uncompressed bytes.
 * scs_write_coverage_bedgraph: the staged depths under the staged record names; needs a finished yield call with scs_set_coverage
 * on (else SCS_EINVAL, as scs_write_coverage).  scs_write_coverage_ref_bedgraph: the reference depths under the lift table's
 * reference names; scs_write_copy_number_ref: the staged bases that lift to each reference base (copy number 0 on every haplotype
 * is a run of 0); both need scs_set_coverage_ref and the lift table, as scs_write_coverage_ref.
 * The calls synchronise the ctx stream themselves, only read the arrays and may be repeated after one yield: identical files.
 * Device memory for text is bounded by a cap (128 MB) that does not depend on the genome: the tiles of the array are cut into
 * slabs whose text fits it, each slab is sized, scanned, formatted, compressed where asked, copied through pinned memory and
 * written.  The writer's buffers belong to the ctx: kept for the next write, released with it or when both coverage switches are
 * off.  Errors: an unwritable path is SCS_EIO before any GPU work and the ctx stays usable; text that would leave its plan
 * raises a device flag and fails the call (SCS_EOVERFLOW), never a wrong file; a tile (4096 bases) whose text alone exceeds the
 * cap, or a record name beyond 65535 bytes, is SCS_EINVAL stating the bytes.  One GPU.
 * scs_coverage_bedgraph_kernel_time: the writer's kernels (plan passes, per slab scan, emit and BGZF) in the last write call,
 * units = bases; not part of scs_kernel_time's table.
 * Test seams.  scs_runs_probe (needs the GPU): the same kernels and the same slab loop over a caller's values[n] under mask, records
 * of rec_lens[n_rec] (adding up to n) named names[n_rec]; text_cap: the cap in bytes (0: the product's); bgzf != 0: BGZF blocks
 * and the end-of-file block.  out[out_cap] gets the bytes a file would hold, *n_out their number (SCS_EOVERFLOW when out_cap is
 * too small, *n_out set), *lines the lines, *slabs the slabs written; a cap below one tile's text is SCS_EINVAL and the ctx stays
 * usable.  scs_runs_line_probe (host only): one line through the formatter the sizing and emit kernels run; *n_out = its bytes
 * (SCS_EOVERFLOW when cap is too small, *n_out set, out not to be trusted). */
int         scs_write_coverage_bedgraph(scs_ctx* ctx, const char* path, uint64_t* lines, uint64_t* text_bytes);
int         scs_write_coverage_ref_bedgraph(scs_ctx* ctx, const char* path, uint64_t* lines, uint64_t* text_bytes);
int         scs_write_copy_number_ref(scs_ctx* ctx, const char* path, uint64_t* lines, uint64_t* text_bytes);
int         scs_coverage_bedgraph_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
int         scs_runs_probe(scs_ctx* ctx, const uint32_t* values, uint64_t n, uint32_t mask, const uint64_t* rec_lens, uint32_t n_records, const char* const* names,
                           uint64_t text_cap, int bgzf, char* out, uint64_t out_cap, uint64_t* n_out, uint64_t* lines, uint64_t* slabs);
int         scs_runs_line_probe(const char* name, uint64_t start, uint64_t end, uint32_t value, char* out, uint64_t cap, uint64_t* n_out);
/* ---- GC bias: the per-base depth as a function of GC content, the curve Picard's CollectGcBiasMetrics draws -----------------
 * After a yield call with scs_set_coverage on the device holds the staged depths, the genome's codes and the record starts.  The
 * calls below make one pass over them, on demand, and count sliding windows by their GC content.
 * Window: W bases, 1 .. 1024.  For every staged record r of length len and every start p with p + W <= len the window is the W
 * bases [p, p + W) of r: windows slide by one base, never cross a record border, and a record shorter than W has none.
 * Excluded: a window that holds at least one N base is counted in n_windows[r] and in nothing else.
 * Bin: a counted window with gc bases of G or C adds to row b = 100 * gc / W (integer division, 0 .. 100): the simulator's own
 * formula for an amplicon, so row b stands beside gc_means[b] of the loaded profile.  W = 100: b = gc; W < 100: some rows stay
 * empty.
 * Tables, per record and one last row `genome` which is the host's sum of the records' rows; all uint64 and exact for every
 * uint32 depth (a window's sum may pass 2^32): windows[r][b] the counted windows of bin b, depth_sum[r][b] the sum over them of
 * the sum of depth[g] over the window's W bases, n_windows[r] the excluded windows.  Derived by the host, as doubles:
 * mean_depth[r][b] = depth_sum / (windows * W); row_mean[r] = sum_b depth_sum / (W * sum_b windows); normalized[r][b] =
 * mean_depth / row_mean, 0 where row_mean is 0 -- Picard's normalized coverage, on aligned bases instead of read starts.
 * scs_gc_bias: records + 1 rows (records: scs_coverage_shape), windows and depth_sum row-major with 101 values per row; any
 * pointer may be NULL.  SCS_EINVAL for a window outside 1 .. 1024 and before a yield call with scs_set_coverage on has finished
 * (the message names scs_set_coverage; a sharded ctx keeps no array, so its yield call is refused as before); SCS_EOVERFLOW when
 * cap_rows < records + 1.  It synchronises the ctx stream, may be repeated with any W, and only reads the arrays:
 * scs_download_coverage and scs_coverage_range answer the same before and after.
 * scs_write_gc_bias: the table as text written by the host (no .gz):
 *   "#gc_bias\twindow=W\tstep=1\texcluded=windows_with_N\tbin=100*gc/window"
 *   "#summary\trecord\twindows\tn_windows\tmean_depth", then "#s\tNAME\t<sum_b windows>\t<n_windows>\t<row_mean>" per record and
 *   for `genome`
 *   "#record\tgc\twindows\tdepth_sum\tmean_depth\tnormalized\tmodel", then "NAME\tb\t..." for every b with windows > 0, the
 *   genome's rows last.  Doubles as %.6f; model = the loaded profile's gc_means[b] as %.6g, `.` when the ctx has no profile.
 * An unwritable path is SCS_EIO before any GPU work.
 * scs_gc_bias_kernel_time: the last call's launches, HIP-event milliseconds and units (staged bases); not part of
 * scs_kernel_time's table.
 * The table's buffer belongs to the ctx: released with it, when scs_set_coverage goes off and when another genome is staged.
 * scs_gc_bias_probe (test seam, needs the GPU): the kernel alone, as the product launches it, over depth[n_bases], codes[n_bases]
 * (0 .. 3 = ACGT, >= 4 = N) and records of rec_lens (adding up to n_bases); lds as scs_coverage_finish_probe's lds_buckets: < 0
 * the product's choice, 0 no LDS table, every add goes to memory.  n_records rows, no genome row; any output may be NULL. */
int         scs_gc_bias(scs_ctx* ctx, uint32_t window, uint64_t* windows, uint64_t* depth_sum, uint64_t* n_windows, uint64_t cap_rows);
int         scs_write_gc_bias(scs_ctx* ctx, const char* path, uint32_t window);
int         scs_gc_bias_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
int         scs_gc_bias_probe(scs_ctx* ctx, const uint32_t* depth, const uint8_t* codes, uint64_t n_bases, const uint64_t* rec_lens, uint32_t n_records,
                              uint32_t window, int lds, uint64_t* windows, uint64_t* depth_sum, uint64_t* n_windows);
/* ---- lift table and depth by reference bin: the job in the coordinates of the original reference ---------------------------
 * Every other truth product lives in the coordinates of the staged haplotype records.  The lift table maps them to the reference
 * `simuvars` built them from: segments that ascend and tile the staged genome, none straddling two staged records, each `len`
 * bases from global index hap_off (records concatenated in staging order).  kind 0 (R): copies of reference record ref_rec,
 * 0-based [ref_pos, ref_pos + len); SNP / SNV substitutions do not break a segment.  kind 1 (I): inserted sequence, no reference
 * coordinate; ref_rec = the chromosome of its staged record, ref_pos = an anchor for information only (the end of the R segment
 * before it in its record; none: the start of the next; no R segment in the record: 0).  The table is maximal (no two
 * neighbours could be one) and belongs to the staged genome: every call that stages another genome drops it.
 * scs_simuvars keeps the table of the genome it builds (nothing else about that call changes).
 * scs_write_lift: the table as tab-separated text with BED coordinates inside the records:
 *     ##scssim-lift v1
 *     #ref  <name> <length>                         one per reference record, in order
 *     #hap  <name> <length>                         one per staged record, in staging order
 *     <hap name> <hap start> <hap end> <ref name> <ref start> <ref end> R|I         (I: ref start = ref end = the anchor)
 * scs_load_lift: reads such a file for the genome that is staged (the two-step flow: `scssim simuvars --lift`, later `genreads
 * -i simu.fa --lift`).  SCS_EINVAL: its #hap names and lengths are not the staged records' (the first record that differs is
 * named).  SCS_EIO with the line number: a missing header, a wrong column count, an unknown record name, a gap, an overlap or
 * lines out of order, a segment past its staged or its reference record, an R line whose two lengths differ.
 * scs_lift_info: the table's size.  scs_lift_segments: the table as arrays (any may be NULL), read back from the device copy;
 * ref_lens: the reference records' lengths (ref_cap entries of room).  SCS_EOVERFLOW: cap / ref_cap is too small.
 * scs_lift_positions: n staged positions (rec[i] = staged record, pos[i] = 0-based coordinate in it; host arrays) lifted on the
 * device: ref_rec / ref_pos / kind per position (I: the anchor).  How POS columns of the truth SAM, the amplicon table and the
 * artefact VCF are lifted.  SCS_EINVAL: a position outside its record.
 *
 * scs_set_depth_ref(ctx, bin_width): the following yield calls also count the job per bin of bin_width >= 1 bases of the REFERENCE
 * records (0: off, the default -- no buffer exists, no code of it runs).  Bins are numbered as scs_set_depth numbers them, over the
 * reference lengths (the same 2^27 cap); one extra pseudo-bin at index n_bins collects what has no reference coordinate.  Placement
 * is the truth SAM's.  bases[b] = (read, haplotype base) pairs an M operation aligns whose base lies in an R segment and lifts into
 * bin b (in an I segment: the pseudo-bin).  reads[b] = FASTQ records whose first M-aligned base with a reference coordinate, in
 * ascending haplotype order, lifts into b (no such base: the pseudo-bin).  So the sum of reads is scs_stats.reads_written and the
 * sum of bases is the sum of the CIGARs' M lengths.  copies[b] = haplotype bases of R segments that lift into b, made once per
 * layout, independent of the reads: copies[b] / (end - start) is the bin's true copy number; copies[n_bins] = inserted bases.
 * Which reads, the counters' lifetime and where it works: as scs_set_depth, beside it and beside the site support.  A sharded ctx,
 * or a staged genome without a lift table, fails the yield call with SCS_EINVAL.
 * scs_depth_ref_bins / scs_depth_ref_record_bins: the layout (bin_off: reference records + 1 entries).
 * scs_download_depth_ref: n_bins + 1 entries each (any pointer may be NULL); SCS_EINVAL before a yield call with it on has finished.
 * scs_write_depth_ref: "#record\tstart\tend\treads\tbases\tcopies", one line per bin with the reference's record names, then
 * "#unlifted\t<reads>\t<bases>\t<inserted bases>".
 * scs_depth_ref_kernel_time: event pairs (one per batch), milliseconds and pairs of the last yield call's k_depth_lift launches
 * (scs_kernel_time keeps its slots). */
int         scs_write_lift(scs_ctx* ctx, const char* path);
int         scs_load_lift(scs_ctx* ctx, const char* path);
int         scs_lift_info(const scs_ctx* ctx, uint64_t* n_segments, uint32_t* n_ref_records);
int         scs_lift_segments(scs_ctx* ctx, uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t cap, uint64_t* ref_lens, uint32_t ref_cap);
int         scs_lift_positions(scs_ctx* ctx, const uint32_t* rec, const uint64_t* pos, uint64_t n, uint32_t* ref_rec, uint64_t* ref_pos, uint32_t* kind);
int         scs_set_depth_ref(scs_ctx* ctx, uint32_t bin_width);
int         scs_depth_ref_bins(const scs_ctx* ctx, uint64_t* n_bins, uint32_t* bin_width);
int         scs_depth_ref_record_bins(const scs_ctx* ctx, uint64_t* bin_off, uint64_t cap);
int         scs_download_depth_ref(scs_ctx* ctx, uint64_t* reads, uint64_t* bases, uint64_t* copies, uint64_t cap);
int         scs_write_depth_ref(scs_ctx* ctx, const char* path);
int         scs_depth_ref_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
/* Host-only test seams of the lift table (no GPU, no ctx).  scs_lift_plan_probe: plans scs_simuvars for these inputs, builds the
 * table and (out_path) writes the file; the table comes back as arrays (any may be NULL; *n_seg, *n_hap, *n_ref are always set;
 * SCS_EOVERFLOW: a cap is too small), names = the reference records' names then the staged records', a newline behind each;
 * subst_pos = the global staged indices the plan substitutes.  scs_lift_file_probe: the parser scs_load_lift runs; SCS_EIO with
 * *line (0: the file cannot be opened) when it is refused.  scs_lift_read_probe: one read through the function k_depth_lift runs;
 * n, reverse, events, nev as for scs_truth_record_probe, pos0 = GLOBAL staged index of window base 0; the table and the records as
 * arrays.  *reads_bin and bins[i] / bases[i], i < *n_out: the increments in the order the kernel makes them (a bin met again after a
 * jump comes again), bins numbered over ref_lens, the pseudo-bin = their total.  SCS_EINVAL: not a valid alignment, or the read
 * cannot be lifted -- *lift_err then says why (1 placed outside its record, 2 off the table, 3 lifted outside the reference). */
int         scs_lift_plan_probe(const char* ref_fasta, const char* snp_file, const char* var_file, const char* out_path,
                                uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t seg_cap, uint64_t* n_seg,
                                uint64_t* subst_pos, uint64_t subst_cap, uint64_t* n_subst,
                                uint64_t* hap_lens, uint64_t* ref_lens, uint32_t rec_cap, uint32_t* n_hap, uint32_t* n_ref,
                                char* names, size_t names_cap, size_t* names_len, char* errbuf, size_t errlen);
int         scs_lift_file_probe(const char* path, uint64_t* hap_off, uint64_t* len, uint64_t* ref_pos, uint32_t* ref_rec, uint32_t* kind, uint64_t seg_cap, uint64_t* n_seg,
                                uint64_t* hap_lens, uint64_t* ref_lens, uint32_t rec_cap, uint32_t* n_hap, uint32_t* n_ref,
                                char* names, size_t names_cap, size_t* names_len, uint64_t* line, char* errbuf, size_t errlen);
int         scs_lift_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev,
                                const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                                const uint64_t* hap_lens, uint32_t n_hap, const uint64_t* ref_lens, uint32_t n_ref, uint32_t bin_width,
                                uint64_t* reads_bin, uint64_t* bins, uint32_t* bases, int cap, int* n_out, int* lift_err);
/* Host-only test seam of the truth SAM on the reference: one read's line through the formatter its kernels run.  The arguments of
 * scs_truth_record_probe without the genome, pos0 / mate_pos0 = GLOBAL staged indices of window base 0; the table and the records
 * as arrays (scs_lift_read_probe); names = the reference records' names then the staged records', a newline behind each
 * (scs_lift_plan_probe); rname = the staged record's name for YH (NULL: taken from names).  SCS_EINVAL: not a valid alignment, or
 * the read cannot be lifted -- *lift_err then says why, as scs_lift_read_probe's. */
int         scs_truth_ref_record_probe(int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                                       int64_t pos0, int reverse, const int32_t* events, int nev,
                                       int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                                       const char* seq, const char* qual, int len,
                                       const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                                       const uint64_t* hap_lens, uint32_t n_hap, const uint64_t* ref_lens, uint32_t n_ref, const char* names, size_t names_len,
                                       char* out, size_t cap, size_t* n_out, int* lift_err);
/* ---- amplicon table: the amplified pool the reads were drawn from, made on the GPU ---------------------------------------
 * One entry per FULL amplicon, in list order: entry i is the amplicon whose index the FASTQ / SAM record names print.
 *   rec          the staged record the amplicon lies in (a fragment never straddles records)
 *   start, end   0-based, end-exclusive record coordinates of the genome interval it copies; end - start = its length
 *   strand       '+' (+1) when its sequence is a forward copy of the genome, '-' (-1) when it is the reverse complement
 *   semi         index of its parent semi amplicon;  reads: the read number scs_allocate_reads gave it
 *   edits        every base where it differs from the genome it copies: the polymerase errors of its semi amplicon that fall
 *                inside it, then its own (which win at a shared base); a base the second error restores is no edit.  Each is
 *                stated genome-forward -- record coordinate, the genome's base (N for a non-ACGT one), the amplicon's base
 *                complemented on '-' -- in ascending coordinate order, each coordinate once, at any count (never truncated).
 * An edit is shared by every read of the amplicon that covers it (a semi's by the reads of all its fulls): what tells an
 * amplification artefact from a sequencing error, which the truth SAM's NM / MD count alike.
 * Both calls need scs_allocate_reads to have run (SCS_EINVAL before, the message names it) and refuse a sharded ctx (shard_count > 1)
 * with SCS_EINVAL.  A lineage that cannot be placed fails the call with SCS_EOVERFLOW ("amplicon table"), never a wrong line.  They
 * work a chunk of amplicons at a time: no buffer is sized by the job, and every buffer is released when the call returns.
 * scs_amplicon_places: the binary form, arrays of scs_stats.full_amplicons entries (strand +1 / -1, start a record coordinate,
 * len = end - start); any pointer may be NULL; SCS_EOVERFLOW when cap is smaller than the number of full amplicons; synchronises
 * the ctx stream itself.
 * scs_write_amplicons: the table as text, made on the GPU: the line "#record\tstart\tend\tamplicon\tstrand\treads\tsemi\tedits",
 * then one line per amplicon -- the record's name (as scs_fasta_probe reports it), BED coordinates, and edits as pos:R>A joined by
 * commas, "." when there are none.  flags & 1: BGZF, compressed on the GPU, the file ending with the end-of-file block.  *bytes
 * (may be NULL) receives the file's size.  SCS_EIO: the file cannot be opened or written; the ctx stays usable.
 * scs_amplicon_kernel_time: event pairs, milliseconds and amplicons of the last scs_write_amplicons call's kernels (not a slot
 * of scs_kernel_time). */
int         scs_amplicon_places(scs_ctx* ctx, uint32_t* rec, uint64_t* start, uint32_t* len, int8_t* strand, uint32_t* n_edits, uint64_t cap);
int         scs_write_amplicons(scs_ctx* ctx, const char* path, int flags, uint64_t* bytes);
int         scs_amplicon_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
/* Host-only test seam of the amplicon table (no GPU, no ctx): one amplicon's line through the functions its kernels run.  The
 * lineage: the fragment's genome offset / length / strand (scs_download_frags), the semi's and the full's start and length with
 * their error lists as (pos << 3) | alt entries (scs_download_amplicons' form; more than four go through an overflow pool as on
 * the device); genome = the bases from genome index genome_start on (genome_len of them, covering the amplicon); the record's
 * first genome index, length and name; the line's index, reads and semi fields.  out receives the line with its newline (NULL:
 * only *n_out).  SCS_EINVAL: a lineage that does not fit its parents, its record or the genome given; SCS_EOVERFLOW: cap too small. */
int         scs_amplicon_line_probe(uint64_t frag_goff, uint32_t frag_len, int frag_strand, uint32_t semi_spos, uint32_t semi_len,
                                    const uint32_t* semi_errs, uint32_t n_semi_errs, uint32_t full_spos, uint32_t full_len,
                                    const uint32_t* full_errs, uint32_t n_full_errs, const char* genome, uint64_t genome_start, uint64_t genome_len,
                                    uint64_t rec_off, uint64_t rec_len, const char* rec_name, uint32_t index, uint32_t reads, uint32_t semi,
                                    char* out, size_t cap, size_t* n_out);

/* ---- artefact table: the amplification's errors by genome site, made on the GPU -------------------------------------------
 * The false-positive truth set of the experiment: one entry per ARTEFACT SITE, a triple (staged record, record coordinate,
 * alternate base), wherever at least one full amplicon has an edit (the amplicon table's edits above: genome-forward, the semi's
 * errors then the full's own, which win at a shared base; a restored base is no edit).  Two alternate bases at one coordinate
 * are two sites.  Per site, exact integers:
 *   NA   full amplicons that carry this alternate base at this coordinate
 *   TA   full amplicons whose interval [start, end) contains the coordinate, whatever they carry there
 *   NR   sum of the read numbers (scs_download_read_numbers) of the NA amplicons;  TR: of the TA amplicons
 * so 1 <= NA <= TA, NR <= TR, and NR / TR is the artefact's expected allele fraction in the reads.  The sites come in ascending
 * (record in staging order, coordinate, alternate base A < C < G < T), each once.  min_reads: only sites with NR >= min_reads are
 * reported (0: every site; most sites of a low-coverage job have NR = 0).
 * Both calls need scs_allocate_reads to have run and an unsharded ctx (SCS_EINVAL otherwise, as for the amplicon table).  A lineage
 * that cannot be placed fails the call with SCS_EOVERFLOW ("artefact table"), never a wrong line.  The genome is worked in slabs
 * of 2^28 genome indices: the call's buffers hold one slab's edit entries and amplicons, not the job's, and every buffer, stream
 * and event of the call is released when it returns, on every way out.
 * scs_write_artefacts: VCF 4.2, made on the GPU: ##fileformat=VCFv4.2, ##source=scssim, one ##contig=<ID=NAME,length=LEN> per
 * staged record (names as scs_fasta_probe reports them), the four ##INFO lines, the #CHROM line, then per site
 * NAME, POS (coordinate + 1), ".", REF (the genome's base, N for a non-ACGT one), ALT, ".", ".", "NA=..;TA=..;NR=..;TR=..".
 * flags: 1 = BGZF (header block made on the host, body blocks on the GPU, the 28-byte end-of-file block last: the file is sorted,
 * so bgzip- and tabix-style tools read it); any other bit is SCS_EINVAL.  A job without a site writes the header (and in BGZF the
 * end-of-file block).  *sites / *bytes (may be NULL) receive the sites written and the file's size.  SCS_EIO: the file cannot be
 * opened or written; the ctx stays usable.
 * scs_artefact_sites: the binary form; ref codes 0..4, alt 0..3, pos 0-based; any array may be NULL; *n is always set to the number
 * of sites, SCS_EOVERFLOW when cap < *n (cap = 0 asks for the count; the first cap sites are still stored); synchronises the ctx
 * stream itself.
 * scs_artefact_kernel_time: event pairs, milliseconds and sites of the last scs_write_artefacts call's kernels, the library sorts
 * and scans included (not a slot of scs_kernel_time). */
int         scs_write_artefacts(scs_ctx* ctx, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes);
int         scs_artefact_sites(scs_ctx* ctx, uint32_t min_reads, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta,
                               uint64_t* nr, uint64_t* tr, uint64_t cap, uint64_t* n);
int         scs_artefact_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
/* Host-only test seam of the artefact table (no GPU, no ctx): the table's body through the functions its kernels run (key packing,
 * run heads, the cover count by bisection, the record lookup, the line formatter under a counting and a writing sink), with
 * std::sort where the device has the radix sort.  n_amp amplicon intervals (global genome start, length, reads), n_ed edit
 * entries (amplicon, global genome index, alternate base code 0..3), the staged records' lengths and names, genome = the bases
 * of all records concatenated (genome_len = the sum of the lengths).  flags & 1: the header goes in front.  out receives the text
 * (NULL: only *n_out).  SCS_EINVAL: an amplicon outside its record, an edit outside its amplicon, an alternate base above 3;
 * SCS_EOVERFLOW: cap too small. */
int         scs_artefact_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                               const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                               const uint64_t* rec_len, const char* const* rec_names, uint32_t n_rec, const char* genome, uint64_t genome_len,
                               uint32_t min_reads, int flags, char* out, size_t cap, size_t* n_out);
/* ---- artefact table on the ORIGINAL REFERENCE: the same artefacts where a caller's VCF has them, made on the GPU -------------
 * The table above is keyed by staged haplotype record.  This one is keyed by the reference the lift table (scs_simuvars,
 * scs_load_lift) maps the staged records to, so that a caller's VCF can be intersected with it.  X = the index of a reference
 * base among the reference records of the lift table, concatenated in table order.
 *   entry  a (full amplicon, staged index g) pair with an edit -- the edits of the tables above.  With g in an R segment it belongs
 *          to the SITE (X(g), REF, ALT); with g in an I segment (inserted sequence) it has no reference coordinate: it is counted
 *          in unlifted[0] (entries) and unlifted[1] (their amplicons' read numbers) and makes no line.
 *   REF    the base of the staged haplotype at g: the template the polymerase misread.  It is part of the site's identity: where a
 *          heterozygous substitution was planted the two haplotypes hold different bases at one reference position, and one POS
 *          may carry lines with different REF.  It differs from the reference FASTA's base exactly there.
 *   piece  the part of a full amplicon's interval that lies in one R segment, as a reference interval [X0, X1): one per R segment
 *          the amplicon touches, none for an amplicon wholly in inserted sequence.  Two pieces of one amplicon may overlap on the
 *          reference (an amplicon longer than a tandem copy unit); they count separately.
 *   NA / NR  the site's entries and the sum of their amplicons' read numbers;
 *   TA / TR  the pieces, of any haplotype record and copy, with X0 <= X < X1, and the sum of their amplicons' read numbers.
 * So 1 <= NA, and over the lines of one position sum(NA) <= TA and sum(NR) <= TR; NR / TR is the artefact's expected allele
 * fraction among the reads that align to the reference position.  The counters are exact and do not depend on slab, chunk or LDS
 * sizes.  The sites come in ascending (reference record in table order, coordinate, REF A < C < G < T < N, ALT A < C < G < T), each
 * once; min_reads keeps the sites with NR >= min_reads.
 * Both calls need a lift table, scs_allocate_reads to have run and an unsharded ctx (SCS_EINVAL otherwise; the message names the
 * missing step).  An amplicon that cannot be placed, a walk that leaves the table or its record's segments, a segment that lifts
 * outside its reference record, counts that contradict each other or a line the two passes size differently fail the call with
 * SCS_EOVERFLOW ("artefact table" / "artefact table on the reference"), never a wrong line.  The reference is worked in slabs of
 * 2^28 reference indices; every buffer, stream and event of the call is released when it returns, on every way out.  A reference
 * of 2^58 bases or more is refused (SCS_EOVERFLOW).
 * scs_write_artefacts_ref: VCF 4.2, made on the GPU: ##fileformat=VCFv4.2, ##source=scssim, ##scssim_coordinates=reference,
 * ##scssim_REF=<what REF is>, ##scssim_unlifted=<entries=E,reads=R>, one ##contig=<ID=NAME,length=LEN> per REFERENCE record of the
 * lift table in its order, the four ##INFO lines, the #CHROM line, then per site NAME, POS (reference coordinate + 1), ".", REF,
 * ALT, ".", ".", "NA=..;TA=..;NR=..;TR=..".  flags: 1 = BGZF exactly as scs_write_artefacts; any other bit is SCS_EINVAL.  A job
 * without a site writes the header.  *sites / *bytes / unlifted (each may be NULL) receive the sites written, the file's size and
 * the two unlifted totals.  SCS_EIO: the file cannot be opened or written; the ctx stays usable.
 * scs_artefact_ref_sites: the binary form, as scs_artefact_sites (ref_rec: the reference record; the cap / SCS_EOVERFLOW protocol
 * is the same); unlifted may be NULL.
 * scs_artefact_ref_kernel_time: event pairs, milliseconds and sites of the last scs_write_artefacts_ref call's kernels. */
int         scs_write_artefacts_ref(scs_ctx* ctx, const char* path, int flags, uint32_t min_reads, uint64_t* sites, uint64_t* bytes, uint64_t unlifted[2]);
int         scs_artefact_ref_sites(scs_ctx* ctx, uint32_t min_reads, uint32_t* ref_rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta,
                                   uint64_t* nr, uint64_t* tr, uint64_t cap, uint64_t* n, uint64_t unlifted[2]);
int         scs_artefact_ref_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
/* Host-only test seam of that table (no GPU, no ctx): the table's body through the functions its kernels run (the segment cursor,
 * the pieces, key packing, run heads, the cover count by bisection, the line formatter under a counting and a writing sink), slab
 * by slab as the device works it, with std::sort where the device has the radix sort.  The amplicons and edit entries as for
 * scs_artefact_probe (staged indices; the entries in any order), the staged records' lengths and bases, the lift table as five
 * arrays (scs_lift_segments' layout), the reference records' lengths and names.  slab: reference indices per slab (0: 2^28).
 * flags & 1: the header goes in front.  unlifted / lift_err may be NULL.  SCS_EINVAL: an amplicon off its record, an edit outside
 * its amplicon, twice at one index or with an alternate base above 3, records that do not add up to the genome, a reference of 2^58
 * bases, or a walk that gives up (*lift_err: 1 the amplicon, 2 the table does not tile under it, 3 a segment past its reference
 * record); SCS_EOVERFLOW: cap too small. */
int         scs_artefact_ref_probe(const uint64_t* amp_start, const uint32_t* amp_len, const uint32_t* amp_reads, uint64_t n_amp,
                                   const uint32_t* ed_amp, const uint64_t* ed_x, const uint8_t* ed_alt, uint64_t n_ed,
                                   const uint64_t* hap_len, uint32_t n_hap, const char* genome, uint64_t genome_len,
                                   const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                                   const uint64_t* ref_len, const char* const* ref_names, uint32_t n_ref,
                                   uint32_t min_reads, uint64_t slab, int flags, char* out, size_t cap, size_t* n_out, uint64_t unlifted[2], int* lift_err);
/* ---- site support: what the reads of a yield call show at the artefact sites, counted on the GPU ----------------------------
 * The artefact table's NR / TR is the EXPECTED allele fraction; these counters are the OBSERVED one, after fragment sampling,
 * sequencing errors, indels and trimming.  scs_set_site_support(ctx, 1, min_reads): every later yield call first makes the site
 * table scs_artefact_sites(ctx, min_reads, ..) reports (same sites, order, NA / TA / NR / TR; kept on the device) and the distinct
 * genome positions of its sites (two alternate bases at one coordinate share a position; at most 2^29 - 1 positions, SCS_EOVERFLOW
 * beyond -- raise min_reads), then counts per batch, right after the base pass: per position six uint32 counters,
 *   0..3  reads whose aligned base there is A, C, G, T     4  any other character (N)     5  reads whose CIGAR deletes the position
 * The alignment is the truth SAM's (POS, CIGAR, SEQ: genome-forward, a read with flag 0x10 shows the complement of its FASTQ base;
 * inserted bases align to no position; leading and trailing deletions are dropped).  Every read with a FASTQ record counts, both
 * mates of a pair separately, also where they overlap.  Per site DP = classes 0..4, AD = (class of REF -- N: class 4 --, class of
 * ALT), DL = class 5.  The counters are zeroed on the ctx stream at the start of every yield call and hold that call's job; they do
 * not depend on batch cuts, the sink, its writers or whether the text leaves the GPU, and work beside either truth output and the
 * depth track.  A sharded ctx fails the yield call (SCS_EINVAL, naming this setter); 2^32 planned reads or more: SCS_EINVAL.  A read
 * that cannot be counted right fails the call with SCS_EOVERFLOW ("site support"), never a wrong count.  Off (the default): no
 * buffer exists and no code of it runs.  scs_set_site_support(ctx, 0, ..) releases every buffer of the feature.
 * scs_site_support: the sites and their counters after a yield call with the feature on (SCS_EINVAL before one has finished); the
 * arrays as scs_artefact_sites', counts = 6 per site (A, C, G, T, other, deleted at the site's coordinate); any array may be NULL;
 * *n is always set, SCS_EOVERFLOW when cap < *n (cap = 0 asks for the count); synchronises the ctx stream itself.
 * scs_write_site_support: scs_write_artefacts' file at the same min_reads with three more ##INFO lines (DP, AD with Number=2, DL)
 * behind the four and ";DP=d;AD=r,a;DL=x" at the end of every line, made on the GPU; flags: 1 = BGZF as there, any other bit
 * SCS_EINVAL; SCS_EIO: the file cannot be opened or written, the ctx stays usable.
 * scs_site_support_kernel_time: event pairs (one per batch), milliseconds and pairs of the last yield call's k_support launches
 * (not a slot of scs_kernel_time). */
int         scs_set_site_support(scs_ctx* ctx, int on, uint32_t min_reads);
int         scs_site_support(scs_ctx* ctx, uint32_t* rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr,
                             uint32_t* counts /* 6 per site: A,C,G,T,other,deleted at the site's coordinate */, uint64_t cap, uint64_t* n);
int         scs_write_site_support(scs_ctx* ctx, const char* path, int flags, uint64_t* sites, uint64_t* bytes);
int         scs_site_support_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
/* Host-only test seams of the site support (no GPU, no ctx).  scs_support_read_probe: one read through the function the kernel runs;
 * n, pos0, reverse, events, nev, rec_len as for scs_depth_read_probe; seq = the FASTQ record's len bases (read orientation);
 * positions = n_pos record coordinates, ascending and distinct.  index / cls receive (position index, class) in ascending order
 * (cap entries; *n_out their number).  SCS_EINVAL: not a valid alignment inside the record, more than 32 events, len is not the
 * read's length, positions out of order; SCS_EOVERFLOW: cap too small.  scs_site_support_line_probe: one site's line through the
 * formatter the emit kernel runs; counts = its six counters, or NULL for the artefact table's line. */
int         scs_support_read_probe(int n, int64_t pos0, int reverse, const int32_t* events, int nev, uint64_t rec_len, const char* seq, int len,
                                   const uint64_t* positions, uint64_t n_pos, uint64_t* index, uint8_t* cls, int cap, int* n_out);
int         scs_site_support_line_probe(const char* name, uint64_t pos, uint32_t ref, uint32_t alt, uint32_t na, uint32_t ta, uint64_t nr, uint64_t tr,
                                        const uint32_t* counts, char* out, size_t cap, size_t* n_out);
/* ---- site support on the original reference: the same counters at the sites of scs_artefact_ref_sites, by reference position -----
 * scs_set_site_support_ref(ctx, 1, min_reads): every later yield call makes the site table scs_artefact_ref_sites(ctx, min_reads, ..)
 * reports (same sites, order, REF, ALT, NA / TA / NR / TR and unlifted totals; kept on the device), the distinct reference positions
 * X = ref_off[ref_rec] + pos of its sites, and every staged index g that lies in an R segment of the lift table and lifts to one of
 * them -- on every haplotype record and tandem copy, with or without an artefact there (at most 2^29 - 1 staged positions,
 * SCS_EOVERFLOW beyond -- raise min_reads).  The batches count at the staged positions exactly as scs_set_site_support's do; after the
 * last batch the six counters of a reference position are the sums over the staged positions under it.  So a read that covers two
 * tandem copies of X counts once per copy (as its pieces count in TA); a read on a haplotype where X is deleted by a planted variant
 * or lies in a CN-0 stretch has no staged base under X and counts nowhere, not in DL either (DL: sequencing deletions only); bases in
 * inserted sequence count nowhere; bases the truth SAM on the reference soft-clips still count.  Needs a lift table and an unsharded
 * ctx: otherwise the yield call fails with SCS_EINVAL naming this setter; 2^32 planned reads or more: SCS_EINVAL.  A segment that
 * lifts outside its reference record, staged positions that do not ascend or a reference counter that would pass 2^32 - 1 fail the
 * call with SCS_EOVERFLOW, never a wrong or wrapped count.  One table per yield call: switching this one on while
 * scs_set_site_support is on, or the other way round, is SCS_EINVAL naming both setters; switching one off does not touch the other.
 * Lifetime, ownership and where it works: as scs_set_site_support; (ctx, 0, ..) releases every buffer of it.
 * scs_site_support_ref: as scs_site_support (ref_rec: the reference record); unlifted (may be NULL) as scs_artefact_ref_sites.
 * scs_write_site_support_ref: scs_write_artefacts_ref's file at the same min_reads with the three ##INFO lines DP, AD, DL behind its
 * four and ";DP=d;AD=r,a;DL=x" at the end of every line; flags and errors as scs_write_site_support.
 * scs_site_support_ref_kernel_time: the last yield call's k_support launches, as scs_site_support_kernel_time.
 * scs_site_support_ref_step_time: step 0 the expansion behind the site table (position list, ranges, scan, fill; units: staged
 * positions) -- ONE event pair around the whole stretch, with the host's waits for its two totals and its stream synchronisations
 * inside it, so its milliseconds are an upper bound of the kernels' time, not their sum; step 1 the gather, one launch (units:
 * staged positions); any other step is SCS_EINVAL.
 * Memory: beside what scs_set_site_support holds per site, 36 bytes per STAGED position (its index, its reference position, six
 * counters) and 32 per reference position stay allocated from the first yield call until the feature is switched off. */
int         scs_set_site_support_ref(scs_ctx* ctx, int on, uint32_t min_reads);
int         scs_site_support_ref(scs_ctx* ctx, uint32_t* ref_rec, uint64_t* pos, uint8_t* ref, uint8_t* alt, uint32_t* na, uint32_t* ta, uint64_t* nr, uint64_t* tr,
                                 uint32_t* counts /* 6 per site */, uint64_t cap, uint64_t* n, uint64_t unlifted[2]);
int         scs_write_site_support_ref(scs_ctx* ctx, const char* path, int flags, uint64_t* sites, uint64_t* bytes);
int         scs_site_support_ref_kernel_time(const scs_ctx* ctx, uint64_t* launches, double* ms, uint64_t* units);
int         scs_site_support_ref_step_time(const scs_ctx* ctx, int step, uint64_t* launches, double* ms, uint64_t* units);
/* Host-only test seams of that table (no GPU, no ctx).  scs_support_ref_probe: the expansion and the gather through the functions the
 * kernels run: the lift table as five arrays, the staged and the reference records' lengths, x = the n_x listed reference positions
 * (ascending, distinct), chunk = output slots per fill pass (0: all), g_counts = six counters per staged index of the whole genome
 * (or NULL: no gather).  sp_pos / sp_pos_x receive the staged positions and the index of each one's reference position (cap entries;
 * *n_staged their number, SCS_EOVERFLOW when cap is too small), ref_counts 6 n_x sums.  SCS_EINVAL with *why: 2 a segment that does not
 * follow the last, holds no base or leaves its staged record, 3 a segment past its reference record, 4 listed positions out of order or
 * outside the reference, 5 staged positions that do not ascend, 6 a counter past 2^32 - 1.  scs_support_ref_header_probe: the file's
 * header. */
int         scs_support_ref_probe(const uint64_t* seg_hap_off, const uint64_t* seg_len, const uint64_t* seg_ref_pos, const uint32_t* seg_ref_rec, const uint32_t* seg_kind, uint32_t n_seg,
                                  const uint64_t* hap_len, uint32_t n_hap, const uint64_t* ref_len, uint32_t n_ref, const uint64_t* x, uint64_t n_x, uint64_t chunk, const uint32_t* g_counts,
                                  uint64_t* sp_pos, uint32_t* sp_pos_x, uint64_t cap, uint64_t* n_staged, uint32_t* ref_counts, int* why);
int         scs_support_ref_header_probe(const uint64_t* ref_len, const char* const* ref_names, uint32_t n_ref, uint64_t unl_entries, uint64_t unl_reads, char* out, size_t cap, size_t* n_out);
/* The fragments of scs_create_frags (Fragment, lib/fragment/Fragment.h:20-31): genome offset of each slice (records concatenated
 * in staging order), its length and strand (+1 / -1); arrays of scs_stats.fragments entries, any pointer may be NULL. */
int         scs_download_frags(scs_ctx* ctx, uint64_t* goff, uint32_t* len, int8_t* strand);
/* Test seam of the staging kernels (the FASTA parser, the slice gather, the genome index): what they left on the device for the
 * resident stretch of the genome, copied back as it lies -- no kernel is launched, no state changes.  info[0..3] = slice_base (genome
 * coordinate of the first resident base; 0 unless a sharded ctx staged only its own stretch), slice_len (resident bases), the number
 * of records, the bytes of their names.  names: the index names, each followed by '\n' (names_cap bytes); rec_lens: the records'
 * lengths (rec_cap entries); SCS_EOVERFLOW with info filled in when either is too small.  With nwords = (slice_len + 63) / 64:
 * codes: slice_len base codes (0..3 = ACGT, 4 = anything else); gc_bits / n_bits: nwords + 1 words, bit i & 63 of word i >> 6 set for a
 * G or C / for a code 4, word nwords zero; gc_pref / n_pref: nwords + 1 exclusive running popcounts of them; gc_pair: nwords + 1 pairs
 * {gc_bits, gc_pref}; g2: 4 nwords words, base i in bits 2 (i & 15) of word i >> 4, a code 4 as 0; has_n: after scs_create_frags, one
 * byte per fragment of scs_download_frags, 1 when it holds a code 4.  Any pointer but info may be NULL.  SCS_EINVAL: no genome
 * staged, or has_n asked for before scs_create_frags. */
int         scs_download_genome(scs_ctx* ctx, uint64_t info[4], char* names, size_t names_cap, uint64_t* rec_lens, uint64_t rec_cap, uint8_t* codes,
                                uint64_t* gc_bits, uint64_t* n_bits, uint64_t* gc_pref, uint64_t* n_pref, uint64_t* gc_pair, uint32_t* g2, uint8_t* has_n);
/* Host-only test seam of the truth kernels: one read's SAM record through their formatter.  n = window length (the model's read
 * length); pos0 = 0-based record coordinate of window base 0 (the rightmost base when reverse); events = nev triples {window
 * position, deletion?, length} in read orientation, as Profile::predict draws them (a deletion clipped to the window end); the
 * mate (PE) likewise; seq / qual = the FASTQ record's len bases and qualities; genome = the record's bases from coordinate
 * genome_start on (genome_len of them, covering the read).  out receives the line with its newline (out may be NULL to ask for
 * its size *n_out); SCS_EINVAL: not a valid alignment, SCS_EOVERFLOW: cap too small. */
int         scs_truth_record_probe(int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                                   int64_t pos0, int reverse, const int32_t* events, int nev,
                                   int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                                   const char* seq, const char* qual, int len, const char* genome, int64_t genome_start, uint64_t genome_len,
                                   char* out, size_t cap, size_t* n_out);
/* The same seam for the truth BAM: out receives the one BAM record the kernels would make, block_size included, uncompressed;
 * refID = 0, next_refID = 0 (PE) or -1 (SE).  Same arguments, same error codes. */
int         scs_truth_bam_record_probe(int paired, int is_read2, uint32_t amp, uint32_t cnt, const char* rname, int n,
                                       int64_t pos0, int reverse, const int32_t* events, int nev,
                                       int64_t mate_pos0, int mate_reverse, const int32_t* mate_events, int mate_nev,
                                       const char* seq, const char* qual, int len, const char* genome, int64_t genome_start, uint64_t genome_len,
                                       char* out, size_t cap, size_t* n_out);

/* ---- kernel-level entry points (unit parity tests; same kernels as the pipeline) ------------ */

/* char* Profile::predict(char* refSeq, int isRead1)  (lib/profile/Profile.cpp:1582-1697) for a batch:
 * windows = n_reads x L base codes (0..3 = ACGT, 4 = N) on the HOST; per read the lineage uid,
 * the attempt number and the read-1 flag select the counter-RNG substream.  out_bases/out_quals:
 * n_reads x out_stride chars; out_len[i] = produced length n'. */
int         scs_predict_batch(scs_ctx* ctx, const uint8_t* windows, size_t n_reads,
                              const uint64_t* uids, const uint32_t* attempts, const uint8_t* is_read1,
                              char* out_bases, char* out_quals, int32_t* out_len, int out_stride);

/* Philox4x32-10 on the device for n counters (ctr: n x 4, key: 2, out: n x 4; host pointers). */
int         scs_philox_batch(scs_ctx* ctx, const uint32_t* ctr, size_t n, const uint32_t* key, uint32_t* out);
/* det_log on the device (host pointers); an argument <= 0 is evaluated as det_exp instead (the product-form Poisson's
 * exp(-lambda), -256 <= x <= 0), so one entry point serves both deterministic functions. */
int         scs_detlog_batch(scs_ctx* ctx, const double* x, size_t n, double* out);

/* Download the amplicon tables (kind 0 = semi, 1 = full) for stage-level parity tests.  Any pointer
 * may be NULL.  Arrays must hold scs_stats.{semi,full}_amplicons entries; errs: up to 4 packed
 * (pos<<3|alt) entries per amplicon in errs[4*i..], count in nerr[i] (>4 = overflow list truncated). */
int         scs_download_amplicons(scs_ctx* ctx, int kind, uint32_t* parent, uint32_t* spos, uint32_t* len,
                                   uint32_t* gc, uint32_t* primers, uint64_t* uid, uint32_t* errs, uint32_t* nerr);
int         scs_download_read_numbers(scs_ctx* ctx, uint32_t* read_numbers);
/* The primer pool after scs_amplify: stock[65536], copies left of every primer type (PrimerIndex.count, lib/malbac/Malbac.h:18-24;
 * index = the 8-mer at two bits per base, first base in the top bits). */
int         scs_download_primer_stock(scs_ctx* ctx, int64_t* stock);
/* The CPUs of the NUMA node `device` hangs on that this process may run on (cpus[0..cap), returns their number; 0: unknown, or the
 * whole affinity mask is local).  The library's sink threads and pinned buffers bind themselves to them; a caller with host threads of
 * its own around the sink (bench.py's cleaners) can do the same. */
int         scs_gpu_local_cpus(int device, int* cpus, int cap);
/* Test seams (csrc/scs_seams.h: small batches, forced kernel variants, injected failures) exist only in libscssim_hip_seams.so, the
 * build the tests load; there this returns the seam's value.  In libscssim_hip.so it returns NULL for every name: the product reads
 * no such knob. */
const char* scs_test_seam(const char* name);

/* ---- host-only table access (no GPU needed): the thresholds scs_load_profile uploads -------------
 * which: 0 subs read1 [84][bins][4], 1 subs read2, 2 quality [16][bins][94], 3 insert length,
 *        4 deletion length, 5 insert size, 6 the alias rows of the quality tables that the inject_errors kernel draws from
 *        (uint32 words, K + K/4 per row, K = 16 / 64 / 128 columns: scssim_amd/csrc/scs_tables.h; no cdf).
 *        thr/cdf point into memory owned by the handle. */
int         scs_profile_open(const char* profile_path, int paired, int isize, void** handle, char* errbuf, size_t errlen);
int         scs_profile_table(void* handle, int which, const uint32_t** thr, const double** cdf, size_t* n);
/* out[0..9] = read length, bins, t_insert, t_delete, isize_min, have_cdf2, insert_rate, del_rate, t_indel (one-draw
 * insertion/deletion test), columns per alias quality row (16, 64 or 128) */
int         scs_profile_scalars(void* handle, double* out);
void        scs_profile_close(void* handle);

/* Host-only: parse a FASTA exactly as scs_load_genome_fasta stages it (no GPU).  names_buf receives the index
 * names joined by '\n'; checksum = FNV-1a over the upper-cased sequence bytes of all records in order. */
int         scs_fasta_probe(const char* fasta_path, int* n_records, uint64_t* total_bases, uint64_t* checksum,
                            char* names_buf, size_t names_len, char* errbuf, size_t errlen);
/* Host-only: plan scs_simuvars for these inputs and return the record count, the total haplotype bases and the FNV-1a
 * checksum of the FASTA text scs_simuvars would write (no GPU; the test seam of the planner). */
int         scs_simuvars_probe(const char* ref_fasta, const char* snp_file, const char* var_file, int* n_records, uint64_t* total_bases,
                               uint64_t* checksum, char* errbuf, size_t errlen);
/* Test seam of the device-buffer policy (needs a GPU, touches no ctx): a library buffer is reserved with first_bytes, then
 * with second_bytes; caps[0..1] receive its usable capacity after each step and *in_place whether the second step kept its
 * address.  Buffers above 64 MB (SCS_VMM_FROM_MB) live in a reserved address range and grow in place, by the request + 3 %. */
int         scs_devbuf_probe(int device, uint64_t first_bytes, uint64_t second_bytes, uint64_t* caps, int* in_place);
/* Host-only test seam of the BGZF kernels (scs_yield_reads_files_ex, bgzf): their arithmetic -- Huffman lengths, header, chunked
 * bit packing, chunked CRC-32 combined by carry-less multiplication, the stored fallback when a block's deflate data exceeds
 * lds_out_cap (0 = the kernels' limit) -- run on the CPU over the same functions; out receives the BGZF blocks of the text
 * (no end-of-file block), *n_out their size (out may be NULL to ask for it).  The checker is zlib. */
int         scs_bgzf_probe(const void* text, uint64_t nbytes, uint32_t lds_out_cap, void* out, uint64_t cap, uint64_t* n_out);
/* Host-only test seam of the reads stage's batch plan (no GPU, no ctx, reads no environment variable): how scs_yield_reads cuts
 * `pairs` planned pairs of reads of read_length bases into batches and in which order it makes them.  to_sink = 0: the text stays in
 * device memory (writers / regions are ignored); else the sink's writers and regions (regions = writers x generations).  batch_shift:
 * 0, or the tests' SCS_TEST_BATCH_SHIFT (batches of 2^shift pairs).  *batch = pairs per batch, *nbatch = their number; order[i] = the
 * batch made i-th, region_of[i] = the region its records belong to (nbatch entries each; both may be NULL to ask for the sizes only;
 * SCS_EOVERFLOW: cap entries are too few). */
int         scs_batch_plan_probe(uint64_t pairs, uint32_t read_length, int to_sink, int writers, int regions, int batch_shift,
                                 uint64_t* batch, uint32_t* nbatch, uint32_t* order, uint32_t* region_of, uint32_t cap);
/* Test seam of the BGZF kernels themselves (needs a GPU, touches no ctx, reads no environment variable): text[0..nbytes) is
 * copied to a fresh device buffer -- 16-byte aligned, as the product's text buffers are -- and goes through exactly what a
 * batch's mate goes through: the plan kernel, the one-workgroup exclusive scan of the block sizes (no scratch), the emit kernel
 * with the tables of bgzf_host_tables, the blocks written from byte zbase (0..3) of a 4-byte aligned output buffer.  out
 * receives the blocks (no end-of-file block), *n_out their size; cap >= nbytes + 31 per 64512-byte block is always enough
 * (SCS_EOVERFLOW otherwise, with *n_out set).  The output buffer has at least 64 guard bytes below byte zbase (the bytes below
 * zbase down to the dword boundary are guard too) and 64 behind the last block, filled with a fixed non-zero pattern before the
 * launches: *guards_ok = 1 when every guard byte is untouched, 0 otherwise.  nbytes == 0: 0 bytes, nothing is launched.
 * The stream is synchronised and hipGetLastError checked before any result is read; a device error is SCS_EDEVICE with its
 * text in scs_last_error(NULL), as for scs_devbuf_probe.  The checkers are zlib and scs_bgzf_probe (byte for byte). */
int         scs_bgzf_device_probe(int device, const void* text, uint64_t nbytes, uint32_t zbase, void* out, uint64_t cap, uint64_t* n_out, int* guards_ok);
/* Test seam of the library's 32-bit exclusive scans (needs a GPU, touches no ctx, reads no environment variable): in0[0..n0)
 * (and in1[0..n1) unless in1 is NULL) are uploaded into buffers with n + 1 readable entries, as the scans require -- entry n
 * holds a non-zero word that must not reach any sum --; exclusive_scan_u32_pair runs (exclusive_scan_u32 when in1 is NULL) with
 * scratch sized by scan_temp_bytes: arrays up to 262144 entries take the one-workgroup kernel, longer ones rocPRIM.
 * out0[0..n0] and out1[0..n1] (n + 1 entries each, out[n] = the total mod 2^32) come back.  A scan that writes behind out[n] is
 * reported as SCS_EDEVICE.  Errors as for scs_devbuf_probe. */
int         scs_scan_probe(int device, const uint32_t* in0, uint64_t n0, const uint32_t* in1, uint64_t n1, uint32_t* out0, uint32_t* out1);
/* Test seams of the read allocation (scs_k_allocate.hip, scs_alloc_plan.h).  scs_alloc_plan_probe: host-only, the plan of shard `rank`
 * of R over counts[r * 40 + slot] amplicons (slot = cycle * 8 + 7 - pass).  scalars: total, chunks, n_interior, n_boundary, n_ranges,
 * n_gseg, the shard's amplicons, scratch doubles; all arrays NULL: the scalars alone (the sizes of a second call); ranges: 3 words
 * each (q0, c0, local0); bchunks: 3 (chunk, length, owner); gsegs: 5 (go, lo, n, owner, slot); my_seg: 40 x 4 (go, lo, n, order).
 * scs_alloc_sums_probe (needs a GPU): the fixed-shape sum (which = 0: one double) or scan (which = 1: n doubles) of n doubles with the
 * scratch a job reserves for n chunks.  scs_alloc_probe (needs a GPU): the whole allocation behind the weights on a ctx that was never
 * amplified, over n_local given weights cut into segments of seg_counts[40]; layout, seed, shard and collectives are the ctx's;
 * rn_out[n_local], pair_off_out[n_local + 1]; the ctx stays not allocated.  In contract: finite weights >= 0 whose sum over the
 * whole job is at least 1e-3. */
int         scs_alloc_plan_probe(const uint64_t* counts, int R, int rank, uint64_t scalars[8], uint32_t* ranges, uint32_t* bchunks, uint64_t* gsegs, uint64_t* my_seg);
int         scs_alloc_sums_probe(int device, const double* in, uint64_t n, int which, double* out);
int         scs_alloc_probe(scs_ctx* ctx, const double* w_local, uint64_t n_local, const uint32_t* seg_counts, uint64_t reads, uint32_t* rn_out, uint32_t* pair_off_out);
/* Test seam of the library's resource ownership (no ctx; process-wide): what its owning handles hold at this moment --
 * out[0] = bytes of device buffers, out[1] = streams it created (a caller's cfg.stream is not one), out[2] = events, out[3] = bytes
 * of pinned host memory.  Counted by the handles themselves as they allocate and free, not asked of the driver, so other
 * processes on the card do not show; the two side streams and three events of a ctx's k_reads class kernels are outside the count.
 * All four are zero once every ctx is destroyed. */
int         scs_live_resources(uint64_t out[4]);
/* Host-only: leave <fasta_path>.fai beside the file if there is none, exactly as scs_load_genome_fasta does (the
 * reference indexes its input through fastahack, lib/fastahack/Fasta.cpp:241-249: name, length, offset, bases per
 * line, bytes per line). */
int         scs_fasta_write_index(const char* fasta_path, char* errbuf, size_t errlen);

/* Per-kernel timing (HIP events recorded on the ctx stream around every launch, accumulated over the
 * last scs_amplify / scs_yield_reads call): name, launches, total milliseconds, and the units the
 * launches processed (amplicons created for the errscan kernels, read pairs for k_reads/k_indels,
 * templates for the two k_attach instances).  which = 0..7: k_errs<semi->full>, k_errs<frag->semi>, k_reads,
 * k_attach<semi>, k_indels, k_attach<frag>, k_truth (the truth SAM's sizing + scan and emit passes, two event pairs per batch),
 * k_depth (the depth track's pass, one event pair per batch, units = pairs). */
int         scs_kernel_time(const scs_ctx* ctx, int which, const char** name, uint64_t* launches, double* ms, uint64_t* units);
/* Which of the eight kernels get their HIP event pairs: bit `which` of mask (default: all), and on which calls: every
 * `every`-th scs_amplify / scs_yield_reads call counted from this call (default 1 = all).  Every event record is a
 * packet on the stream (about 6 us each on the latency-bound 1 Mb configuration), so a measurement run times only the
 * kernel of interest, on a sample of the steps.  scs_kernel_time reports an untimed call as 0 launches / 0 units. */
int         scs_set_kernel_timing(scs_ctx* ctx, unsigned mask, unsigned every);

#ifdef __cplusplus
}
#endif
#endif /* SCSSIM_HIP_H */
