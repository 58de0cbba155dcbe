// scs_sink.cpp -- the FASTQ sink (SeqWriter's replacement): where its host work runs, and the pipeline of pinned slots and writer threads
#include "scs_sink.h"

namespace scs {
// FASTQ sink pipeline (replaces the mutexed ofstream of lib/seqwriter/SeqWriter.cpp:41-54).  A batch's text is
// copied D2H on the copy stream into a free pinned slot and handed to the writer thread of its REGION (BatchSink: the job's
// records are cut into `regions` contiguous ranges, visited round-robin, one writer thread and one pair of files each), which
// waits for the copy's event, writes, and frees the slot -- while the GPU already produces the next batches.  writers + 2
// slots: every writer can hold one while one is being filled and one crosses PCIe.  (regions = writers x generations: writer w
// serves the regions r = w mod writers, one after the other.)
// ---- where the sink's host work runs.  A GPU hangs on one NUMA node of the host; a copy into pinned memory of the OTHER node runs at
// half the rate (profiles/r03_numa_probe.log: 29 against 57 GB/s), and on a node with several GPUs every rank's writers should stay
// on their own GPU's node.  gpu_local_cpus: the CPUs of the ctx device's node that this process may run on (empty: unknown, or no
// choice to make); NumaScope binds the calling thread to them for its lifetime (pinned allocations: first touch).
std::vector<int> gpu_local_cpus(int device) {
    std::vector<int> out; char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) return out;
    for (char* q = bdf; *q; ++q) *q = (char)tolower(*q);
    int node = -1;
    { FILE* f = fopen((std::string("/sys/bus/pci/devices/") + bdf + "/numa_node").c_str(), "r"); if (!f) return out; if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
    if (node < 0) return out;
    char list[4096] = {0};
    { FILE* f = fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r"); if (!f) return out; if (!fgets(list, sizeof list, f)) list[0] = 0; fclose(f); }
    cpu_set_t allowed; CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return out;
    char* save = nullptr;                                                          // (strtok_r: two ctxs on two host threads come through here at once)
    for (char* tok = strtok_r(list, ",\n", &save); tok; tok = strtok_r(nullptr, ",\n", &save)) {
        int a = 0, b = 0; const int k = sscanf(tok, "%d-%d", &a, &b); if (k < 1) continue; if (k == 1) b = a;
        for (int c = a; c <= b && c < CPU_SETSIZE; ++c) if (CPU_ISSET(c, &allowed)) out.push_back(c);
    }
    if ((int)out.size() == CPU_COUNT(&allowed)) out.clear();                       // the whole mask is local already
    return out;
}
struct NumaScope {
    cpu_set_t old; bool on = false;
    explicit NumaScope(const std::vector<int>& cpus) {
        if (cpus.empty() || pthread_getaffinity_np(pthread_self(), sizeof old, &old) != 0) return;
        cpu_set_t s; CPU_ZERO(&s); for (int c : cpus) CPU_SET(c, &s);
        on = pthread_setaffinity_np(pthread_self(), sizeof s, &s) == 0;
    }
    ~NumaScope() { if (on) (void)pthread_setaffinity_np(pthread_self(), sizeof old, &old); }
};
void SinkPipe::start(BatchSink* f, bool pe, int dev) {
    sink = f; paired = pe; device = dev; done = failed = false;
    local_cpus = gpu_local_cpus(dev);
    const size_t nw = (size_t)std::max(1, f->writers), want = nw + 2;
    // (blocking events: a writer that waits for its batch's copy sleeps instead of spinning -- the host's cores are the sink's bottleneck)
    while (slots.size() < want) { Slot sl; sl.ev.ensure(hipEventDisableTiming | hipEventBlockingSync); slots.push_back(std::move(sl)); }
    for (auto& sl : slots) sl.busy = false;
    writers = std::vector<Writer>(nw);
    for (size_t w = 0; w < writers.size(); ++w) writers[w].th = std::thread([this, w] {
        (void)hipSetDevice(device);
        if (!local_cpus.empty()) { cpu_set_t cs; CPU_ZERO(&cs); for (int c : local_cpus) CPU_SET(c, &cs); (void)pthread_setaffinity_np(pthread_self(), sizeof cs, &cs); }   // a writer stays on its GPU's node
        Writer& W = writers[w];
        for (;;) {
            Job j;
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !W.q.empty() || done; }); if (W.q.empty()) return; j = W.q.front(); W.q.erase(W.q.begin()); }
            Slot& sl = slots[(size_t)j.slot];
            bool bad = hipEventSynchronize(sl.ev) != hipSuccess;
            if (!bad && !failed) bad = sink->put(j.region, sl.h[0], j.n1, paired ? sl.h[1] : nullptr, j.n2) != 0;
            if (!bad && !failed && j.n3) bad = !write_all(truth_fd, sl.h[2], j.n3);   // (scs_outfile.h)
            { std::lock_guard<std::mutex> lk(mu); sl.busy = false; if (bad) failed = true; }
            cv.notify_all();
        }
    });
}
int SinkPipe::acquire(size_t need1, size_t need2, size_t need3) {
    int k = -1;
    { std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { if (failed) return true; for (size_t i = 0; i < slots.size(); ++i) if (!slots[i].busy) { k = (int)i; return true; } return false; });
      if (failed) return -1;
      slots[(size_t)k].busy = true; }
    Slot& sl = slots[(size_t)k];
    for (int f = 0; f < 3; ++f) {
        const size_t need = f == 0 ? need1 : f == 1 ? need2 : need3;
        if (f == 2 && need == 0) continue;
        if (need > sl.h[f].bytes) {
            NumaScope here(local_cpus);                                        // the slot's pages on the GPU's node
            sl.h[f].reserve(need, hipHostMallocDefault, std::max<size_t>(need + need / 8, 1 << 20));
        }
    }
    return k;
}
void SinkPipe::submit(int region, int slot, size_t n1, size_t n2, size_t n3) { { std::lock_guard<std::mutex> lk(mu); writers[(size_t)region % writers.size()].q.push_back(Job{slot, region, n1, n2, n3}); } cv.notify_all(); }
bool SinkPipe::finish() { { std::lock_guard<std::mutex> lk(mu); done = true; } cv.notify_all(); for (auto& W : writers) if (W.th.joinable()) W.th.join(); writers.clear(); return !failed; }
void SinkPipeDelete::operator()(SinkPipe* p) const { delete p; }                   // (the slots' pinned blocks and events free themselves)
}  // namespace scs
