#include "host_mem.hpp"

#include <sched.h>

#include <algorithm>
#include <cstring>

#include "device_abi_weak.hpp"

namespace cli {

HostBuffer &HostBuffer::operator=(HostBuffer &&o) noexcept {
    if (this != &o) {
        reset();
        p = o.p, cap = o.cap, pinned = o.pinned;
        o.p = nullptr, o.cap = 0, o.pinned = false;
    }
    return *this;
}

void HostBuffer::reset() {
    if (pinned) mk_host_free(p);
    else free(p);
    p = nullptr, cap = 0, pinned = false;
}

bool HostBuffer::grow(size_t n, size_t headroom, bool or_malloc) {
    if (n <= cap) return true;
    reset();
    const size_t want = n + n / 8 + headroom;
    void *q = nullptr;
    if (mk_host_alloc && mk_host_alloc(want, &q) == MK_OK) pinned = true;
    else q = or_malloc ? malloc(want) : nullptr;
    if (!q) return false;
    p = (uint8_t *)q, cap = want;
    return true;
}

static unsigned g_io_threads_cap = 0;  // 0 = no cap
void set_io_threads_cap(unsigned n) { g_io_threads_cap = n; }

unsigned io_threads() {
    static const unsigned cached = [] {
        if (const char *e = getenv("MERKURIO_IO_THREADS")) return (unsigned)std::max(1, atoi(e));
        unsigned hw = std::thread::hardware_concurrency();
        if (hw == 0) hw = 1;
        // containers: the cgroup CPU quota, not the machine's core count, is what this process gets
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32] = {0};
            long long period = 0;
            if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
                hw = std::min<unsigned>(hw, (unsigned)std::max<long long>(1, atoll(q) / period));
            fclose(f);
        }
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) hw = std::min<unsigned>(hw, (unsigned)std::max(1, CPU_COUNT(&set)));
        return std::min(hw, 32u);
    }();
    return g_io_threads_cap ? std::min(cached, g_io_threads_cap) : cached;
}

// Host memory this process may still take: MemAvailable, capped by the cgroup limit.  0 = unknown.
static uint64_t host_memory_available() {
    uint64_t avail = 0;
    if (FILE *f = fopen("/proc/meminfo", "r")) {
        char line[256];
        while (fgets(line, sizeof(line), f)) {
            unsigned long long kb = 0;
            if (sscanf(line, "MemAvailable: %llu kB", &kb) == 1) avail = (uint64_t)kb << 10;
        }
        fclose(f);
    }
    unsigned long long lim = 0, cur = 0;
    FILE *fl = fopen("/sys/fs/cgroup/memory.max", "r"), *fc = fopen("/sys/fs/cgroup/memory.current", "r");
    if (fl && fc && fscanf(fl, "%llu", &lim) == 1 && fscanf(fc, "%llu", &cur) == 1 && lim > cur) {
        const uint64_t room = lim - cur;
        if (avail == 0 || room < avail) avail = room;
    }
    if (fl) fclose(fl);
    if (fc) fclose(fc);
    return avail;
}

// This build holds a decompressed input (and its record index) in host memory; the reference streams
// it.  Fail early and say so instead of being killed by the kernel half way through.
void require_host_memory(uint64_t need, const std::string &path) {
    const uint64_t avail = host_memory_available();
    if (avail == 0 || need <= avail) return;
    char buf[256];
    snprintf(buf, sizeof(buf), " needs about %.1f GiB of host memory once decompressed, %.1f GiB are available. ",
             need / 1073741824.0, avail / 1073741824.0);
    bail(path + buf +
         "This build keeps a compressed input in memory while it is processed (plain-text inputs are memory-mapped and do not "
         "count): decompress it first, split it, or run on a host with more memory.");
}

}  // namespace cli
