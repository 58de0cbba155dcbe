// scs_sink.h -- the FASTQ sink pipeline (scs_sink.cpp): pinned slots, one writer thread per region of the job's records
#pragma once
#include "scs_textout.h"
namespace scs {
struct SinkPipe {
    std::vector<int> local_cpus;                                                   // of the device's NUMA node (gpu_local_cpus)
    struct Slot { Pinned<char> h[3]; Event ev; bool busy = false; };               // h[2]: the batch's truth SAM (or its BAM blocks)
    struct Job { int slot, region; size_t n1, n2, n3; };
    struct Writer { std::thread th; std::vector<Job> q; };
    std::vector<Slot> slots; std::vector<Writer> writers;
    std::mutex mu; std::condition_variable cv; bool done = false, failed = false;
    BatchSink* sink = nullptr; bool paired = true; int device = 0;
    int truth_fd = -1;                                                             // the truth SAM / BAM (one writer: batch order), or -1
    void start(BatchSink* f, bool pe, int dev);
    // a free pinned slot with room for the batch (blocks while every slot is with a writer); -1: the sink failed
    int acquire(size_t need1, size_t need2, size_t need3 = 0);
    void submit(int region, int slot, size_t n1, size_t n2, size_t n3 = 0);
    bool finish();
};
}  // namespace scs
