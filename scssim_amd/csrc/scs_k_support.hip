// scs_k_support.hip -- gfx950 kernels of the site support counters (scs_set_site_support): per listed genome
// position (the artefact sites' coordinates) the reads of the job that show A, C, G, T, another character or a deletion there,
// summed over a batch's reads right after its base pass from what the device holds: the pair records, the indel pass' events and
// the FASTQ text.
//
// k_support: a thread per pair places its reads (for_each_placed_read, scs_place.h: the truth passes' placement), finds their bases in the text (read_text)
// and walks the truth CIGAR over the listed positions (support_read, scs_support.h).  Neighbouring pairs of the list are reads of
// one amplicon, so the 256 pairs of a workgroup hit the same few positions: the workgroup first sums into an open-addressing table
// in LDS (key = position index << 3 | class; one uint32 sum per slot, at most 512 reads each: no overflow) and then adds every used
// slot to memory once.  A lane that finds no free slot within SUPPORT_PROBES steps adds to memory itself, so a full table costs
// time, never a count.  slots = 0 (SCS_TEST_SUPPORT_SLOTS): no table, every add goes to memory -- the un-aggregated kernel of the A/B.
//
// k_support_heads / k_support_scatter: the distinct coordinates of the sorted sites (the scan between them is the library's).
// k_support_size: the bytes of every site's line with its counters (the emit pass is k_site_emit, scs_k_sites.hip).
#include "scs_device.h"
#include "scs_kernels_common.h"
#include "scs_place.h"
#include "scs_support.h"
#include "scs_site.h"

namespace scs {

constexpr uint32_t kSupportBlock = 256u;                   // threads of a k_support workgroup: one pair each
#define SUPPORT_EMPTY 0xFFFFFFFFu                          // (class 7 of the last position index: never a key)
#define SUPPORT_PROBES 16u
static_assert((SUPPORT_LDS_SLOTS & (SUPPORT_LDS_SLOTS - 1u)) == 0u && SUPPORT_LDS_SLOTS >= SUPPORT_PROBES && SUPPORT_LDS_SLOTS % kSupportBlock == 0u,
              "the table's index mask needs a power of two; its set-up and flush loops stride by the block");
static_assert(((uint64_t)(SUPPORT_MAX_POS - 1u) << 3 | 5u) < SUPPORT_EMPTY, "every key is below the empty key");

struct SupportTable {
    uint32_t* key; uint32_t* sum; uint32_t slots; uint32_t* counts;
    __device__ void add(uint32_t idx, uint32_t cls) const {
        const uint32_t k = (idx << 3) | cls;
        uint32_t h = k & (slots - 1u);                     // the classes of a position in neighbouring slots (slots = 0: no turn of the loop)
        for (uint32_t p = 0; p < SUPPORT_PROBES && p < slots; ++p, h = (h + 1u) & (slots - 1u)) {
            const uint32_t was = atomicCAS(&key[h], SUPPORT_EMPTY, k);
            if (was != SUPPORT_EMPTY && was != k) continue;
            atomicAdd(&sum[h], 1u);
            return;
        }
        atomicAdd(&counts[6ull * idx + cls], 1u);
    }
};

__device__ void support_pair(const SupportArgs& A, uint32_t pi, const SupportTable& T) {
    for_each_placed_read(A, pi, (uint32_t)FLAG_SUPPORT, [&](const PairRec& pr, uint32_t rd, const TruthAln& a, int n_out, uint32_t, int64_t r0, int64_t r1) {
        if (a.lo < r0 || a.hi >= r1) { atomicOr(A.flags, (uint32_t)FLAG_SUPPORT); return; }   // outside its record: the call fails
        const char* rec; const char* s = read_text(A.off1, A.off2, A.fq1, A.fq2, A.paired, pr, pi, rd, &rec);
        if (rec[0] != '@' || s[-1] != '\n' || s[n_out] != '\n') { atomicOr(A.flags, (uint32_t)FLAG_SUPPORT); return; }   // the record is not where the offsets say
        support_read(a, A.sp_pos, A.n_pos, [&](int i) { return s[i]; }, [&](uint64_t idx, uint32_t cls) { T.add((uint32_t)idx, cls); });
    });
}

__global__ void __launch_bounds__(kSupportBlock) k_support(SupportArgs A) {
    __shared__ uint32_t s_key[SUPPORT_LDS_SLOTS], s_sum[SUPPORT_LDS_SLOTS];
    for (uint32_t i = threadIdx.x; i < A.slots; i += kSupportBlock) { s_key[i] = SUPPORT_EMPTY; s_sum[i] = 0u; }
    __syncthreads();
    const uint32_t pi = blockIdx.x * kSupportBlock + threadIdx.x;
    if (pi < A.np) support_pair(A, pi, SupportTable{s_key, s_sum, A.slots, A.counts});   // (no lane leaves before the barriers)
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < A.slots; i += kSupportBlock) {
        const uint32_t k = s_key[i];
        if (k != SUPPORT_EMPTY && s_sum[i]) atomicAdd(&A.counts[6ull * (k >> 3) + (k & 7u)], s_sum[i]);
    }
}

// site i of the sorted sites opens a coordinate (two alternate bases at one coordinate share a position)
__device__ __forceinline__ uint64_t support_gidx(const SiteRec* sites, const uint64_t* rec_off, uint64_t i) { return rec_off[sites[i].rec] + sites[i].pos; }

__global__ void __launch_bounds__(256) k_support_heads(const SiteRec* __restrict__ sites, uint64_t n, const uint64_t* __restrict__ rec_off, uint32_t n_rec, uint32_t* __restrict__ head, uint32_t* __restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (sites[i].rec >= n_rec || (i && sites[i - 1].rec >= n_rec)) { atomicOr(flags, (uint32_t)FLAG_SUPPORT); head[i] = 0u; return; }
    const uint64_t x = support_gidx(sites, rec_off, i), before = i ? support_gidx(sites, rec_off, i - 1) : 0ull;
    if (i && before > x) atomicOr(flags, (uint32_t)FLAG_SUPPORT);   // (the sites are not in ascending order: never a wrong bisection)
    head[i] = i == 0 || before != x ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_support_scatter(const SiteRec* __restrict__ sites, uint64_t n, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ head,
                                                         const uint32_t* __restrict__ e, uint64_t* __restrict__ pos, uint32_t* __restrict__ site_pos) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (head[i]) { pos[e[i]] = support_gidx(sites, rec_off, i); site_pos[i] = e[i]; }
    else site_pos[i] = e[i] ? e[i] - 1u : 0u;              // (e[i] >= 1 behind a head; site 0 is one)
}

__global__ void __launch_bounds__(256) k_support_size(SiteArgs T, const SiteRec* __restrict__ sites, const uint32_t* __restrict__ site_pos, const uint32_t* __restrict__ counts, uint32_t* __restrict__ sizes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= T.n) return;
    const SiteRec r = sites[i];
    if (r.rec >= T.n_rec) { atomicOr(T.flags, (uint32_t)FLAG_SUPPORT); sizes[i] = 0u; return; }
    TruthCount c; site_line(c, T.names + T.name_off[r.rec], T.name_off[r.rec + 1] - T.name_off[r.rec], r, counts + 6ull * site_pos[i]);
    sizes[i] = (uint32_t)c.n;
}

void launch_support(hipStream_t s, const SupportArgs& a) {
    if (a.np == 0 || a.n_pos == 0) return;
    SupportArgs b = a; b.slots = table_slots(a.slots, SUPPORT_LDS_SLOTS);
    hipLaunchKernelGGL(k_support, dim3(cdiv(a.np, kSupportBlock)), dim3(kSupportBlock), 0, s, b);
    note_launch(hipGetLastError());
}
void launch_support_heads(hipStream_t s, const SiteRec* sites, uint64_t n, const uint64_t* rec_off, uint32_t n_rec, uint32_t* head, uint32_t* flags) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_support_heads, dim3(cdiv(n, 256)), dim3(256), 0, s, sites, n, rec_off, n_rec, head, flags);
    note_launch(hipGetLastError());
}
void launch_support_scatter(hipStream_t s, const SiteRec* sites, uint64_t n, const uint64_t* rec_off, const uint32_t* head, const uint32_t* e, uint64_t* pos, uint32_t* site_pos) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_support_scatter, dim3(cdiv(n, 256)), dim3(256), 0, s, sites, n, rec_off, head, e, pos, site_pos);
    note_launch(hipGetLastError());
}
void launch_support_size(hipStream_t s, const SiteArgs& t, const SiteRec* sites, const uint32_t* site_pos, const uint32_t* counts, uint32_t* sizes) {
    if (t.n == 0) return;
    hipLaunchKernelGGL(k_support_size, dim3(cdiv(t.n, 256)), dim3(256), 0, s, t, sites, site_pos, counts, sizes);
    note_launch(hipGetLastError());
}

}  // namespace scs
