// host_mem.hpp -- the host's threads and memory as the CLI's readers and writers use them
#pragma once
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "util.hpp"

namespace cli {

// host threads for ingest / codec work: hardware concurrency, capped at 32, MERKURIO_IO_THREADS overrides
unsigned io_threads();
// `tag -p N` given explicitly: at most N host threads for the codec work (the reference's meaning of -p:
// BAM (de)compression threads, src/cmd_tag.rs:102-104,506); without it every core the process may use
void set_io_threads_cap(unsigned n);

// runs fn(t) for t in [0, T) on T host threads; the first cli::Error is re-raised on the caller
template <class F>
void run_threads(size_t T, F fn) {
    if (T <= 1) {
        fn((size_t)0);
        return;
    }
    std::vector<std::string> errs(T);
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            try {
                fn(t);
            } catch (const Error &e) {
                errs[t] = e.what()[0] ? e.what() : "error";
            }
        });
    for (auto &x : th) x.join();
    for (auto &e : errs)
        if (!e.empty()) bail(e);
}

// Host memory with one owner, page-locked where it can be (mk_host_alloc: the device copies from and into it directly).  Move-only;
// the destructor frees it, except in a process that is about to end (g_process_is_ending: unpinning costs more than the process
// has left to live).
struct HostBuffer {
    uint8_t *p = nullptr;
    size_t cap = 0;
    bool pinned = false;  // mk_host_alloc's (else malloc's)
    HostBuffer() = default;
    HostBuffer(HostBuffer &&o) noexcept : p(o.p), cap(o.cap), pinned(o.pinned) { o.p = nullptr, o.cap = 0, o.pinned = false; }
    HostBuffer &operator=(HostBuffer &&o) noexcept;
    HostBuffer(const HostBuffer &) = delete;
    HostBuffer &operator=(const HostBuffer &) = delete;
    ~HostBuffer() {
        if (!g_process_is_ending) reset();
    }
    // at least n bytes: a smaller buffer is freed and n + n / 8 + headroom bytes take its place (the contents are not kept), page-locked
    // or, with or_malloc, from malloc where page-locked memory cannot be had.  false: no memory, the buffer is empty (mk_last_error()
    // says why page-locking failed)
    bool grow(size_t n, size_t headroom, bool or_malloc = false);
    void reset();  // frees the memory now
};

// raises cli::Error if `need` bytes of host memory are not available (decompressed inputs are held in memory)
void require_host_memory(uint64_t need, const std::string &path);

}  // namespace cli
