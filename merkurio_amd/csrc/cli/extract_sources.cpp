// extract_sources.cpp -- the sources of the extract window driver whose bodies the host makes: host text (a plain file staged with
// pread() into the pool of page-locked buffers, or text the host inflated; the first window prepare() read and the rest behind the last
// record included) and BGZF members as stored.  Owns the pin pool.  The sources whose text lies on the device: extract_device_text.cpp.
#include <unistd.h>

#include "extract_sources.hpp"

namespace cli {
namespace xw {

static void grow_pin(HostBuffer &b, uint64_t n) {
    if (!b.grow(n, 4096)) bail(std::string("Error allocating page-locked memory: ") + mk_last_error());
}

void PinPool::make(Gate &g, uint64_t bytes) {
    for (size_t q = 0; q < bufs.size(); ++q) {
        grow_pin(bufs[q], bytes);
        std::lock_guard<std::mutex> lk(g.mu);
        free.push_back((int)q);
        g.cv.notify_all();
    }
}

int PinPool::take(Gate &g) {
    std::unique_lock<std::mutex> lk(g.mu);
    g.cv.wait(lk, [&] { return g.failed || !free.empty(); });
    if (g.failed) return -1;
    const int pin = free.front();
    free.pop_front();
    return pin;
}

namespace {

// the window's bytes into pinned memory, on all host threads (page-cache pages cannot be DMA sources).  A plain file is read with
// pread() -- the kernel copies from the page cache without a page fault per 4 KiB of a mapping --, inflated text is copied.
void stage(int fd, HostBuffer &dst, const char *src, uint64_t n, uint64_t file_off) {
    grow_pin(dst, n);
    const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), (size_t)(n >> 22) + 1));
    run_threads(T, [&](size_t t) {
        const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
        uint64_t done_ = lo;
        while (fd >= 0 && done_ < hi) {
            const ssize_t got = pread(fd, (char *)dst.p + done_, (size_t)(hi - done_), (off_t)(file_off + done_));
            if (got <= 0) break;
            done_ += (uint64_t)got;
        }
        if (done_ < hi) memcpy((char *)dst.p + done_, src + done_, (size_t)(hi - done_));  // (no descriptor, or a short read)
    });
}

struct HostText : Source {
    InputFile &f;
    const int i;
    Gate &g;
    PinPool pool;  // (no buffers: a source that took over from a gzip stream -- its bodies stay where the reader left them)
    bool done = false;
    HostText(InputFile &f_, int i_, Gate &g_) : f(f_), i(i_), g(g_) {}
    bool ended() const override { return done; }
    PinPool *pins() override { return &pool; }
    void window_left_device(Side &S) override {
        if (S.pin >= 0) pool.free.push_back(S.pin);
        S.pin = -1;
    }
    // window 0 -- the one prepare() has read -- goes up from where it lies; the ones behind it are staged and sent ahead
    void next(uint64_t k, Side &S, uint64_t target, mk_matcher *m_ahead) override {
        if (done) return;
        const char *text = nullptr;
        uint64_t n = 0, resume = 0;
        bool more;
        if (f.have_first) {
            more = true, text = f.first_text, n = f.first_n, resume = f.first_resume;
            f.have_first = false;
        } else {
            more = f.s.raw_fill(target, &text, &n, &resume);
        }
        if (!more) {
            // nothing, or text that does not start like a record (garbage behind the last record): the rest goes out as one last body,
            // the device refuses it and the host parser words the reference's error
            done = true;
            if (f.s.raw_rest(&text, &n) && n) {
                S.own.assign(text, text + n);
                S.body = S.own.data(), S.n_body = n;
            }
            return;
        }
        f.s.raw_consume();
        if (k == 0 || pool.bufs.empty()) {
            if (f.s.raw_is_plain() || f.s.source().mapped()) {
                S.body = text;  // (a mapping, or a whole inflated bzip2 / xz / zstd text: stays where it is)
            } else {
                S.own.assign(text, text + n);  // (the reader's buffers are recycled two windows on)
                S.body = S.own.data();
            }
            S.n_body = n;
            return;
        }
        const int pin = pool.take(g);
        if (pin < 0) return;
        const double t_stage = PhaseTimer::now();
        stage(f.fd, pool.bufs[pin], text, n, resume - n);
        S.pin = pin, S.body = (const char *)pool.bufs[pin].p, S.n_body = n;
        if (m_ahead) mk_check(mk_upload_text_ahead(m_ahead, (const uint8_t *)S.body, n), "Error uploading the next window");
        if (g.timing) fprintf(stderr, "[timing]   reader: input %d, %.0f MB staged + sent ahead in %.1f ms\n", i, n / 1e6, (PhaseTimer::now() - t_stage) * 1e3);
    }
};

struct Members : Source {
    InputFile &f;
    size_t next_member = 0;
    explicit Members(InputFile &f_) : f(f_) {}
    bool ended() const override { return next_member >= f.s.source().bgzf_members().size(); }
    bool on_device() const override { return true; }
    void next(uint64_t, Side &S, uint64_t target, mk_matcher *) override {
        if (ended()) return;
        const std::vector<mk_bgzf_member> &mem = f.s.source().bgzf_members();
        const size_t g0 = next_member, g = bgzf_run_end(mem, g0, mem.size(), target);
        if (g > g0) S.grp = bgzf_rebased(mem.data() + g0, g - g0, 0, mem[g0].out_off);  // (data_off stays absolute in the file)
        next_member = g;
        S.ends = ended();
    }
    void body_to_host(const Side &S, char *dst) const override {  // (zlib on the host threads)
        inflate_bgzf_members_host(f.s.source().file_bytes(), S.grp.data(), S.grp.size(), dst, f.path);
    }
};

}  // namespace

std::unique_ptr<Source> host_text_source(InputFile &f, int i, Gate &g) { return std::unique_ptr<Source>(new HostText(f, i, g)); }
std::unique_ptr<Source> members_source(InputFile &f) { return std::unique_ptr<Source>(new Members(f)); }

}  // namespace xw
}  // namespace cli
