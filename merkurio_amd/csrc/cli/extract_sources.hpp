// extract_sources.hpp -- what the stages of the extract window driver (extract_windows.cpp) hand to each other: an input file as
// prepare() opened it, one input's part of a window (Side), a window (Win), and the producer of window bodies of one input (Source),
// one small type per kind of input behind one interface:
//   host text      a plain file staged with pread() into page-locked buffers, or text the host inflated      (extract_sources.cpp)
//   BGZF members   the members go to the device as they are                                                  (extract_sources.cpp)
//   device text    a gzip file (one member or several) or a bzip2 file whose text the device has made        (extract_device_text.cpp)
//   device stream  a gzip or bzip2 file the device decodes window by window, and may hand back mid-way       (extract_device_text.cpp)
// No HIP header here: everything but extract_device_text.cpp compiles for a CPU test (tests/helpers/extract_windows_harness.cpp).
#pragma once
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>

#include "extract_common.hpp"

namespace cli {
namespace xw {

constexpr uint64_t kFirstWindow = 8ull << 20;  // (page-locked staging needs the HIP runtime, which is still starting: a small first window)

// what the threads of a job wait on: one lock, one condition; whether the job has failed, and how far the device loops are
struct Gate {
    std::mutex mu;
    std::condition_variable cv;
    bool failed = false;
    std::string failure;
    uint64_t n_done = 0;  // windows the device loops are through with (chained inputs: in order)
    // an xz stream handed its file back and liblzma then refused it: --host-codec would have met that error at load, before it opened
    // the kept records' files or wrote a log row, so the driver removes the former and cuts the logs back before it reports the
    // failure (Sink::discard, Sink::rollback)
    bool discard_kept = false;
    const bool timing = getenv("MERKURIO_TIMING") != nullptr;
    void fail_all(const std::string &msg) {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed) failure = msg;
        failed = true;
        cv.notify_all();
    }
};

struct InputFile {  // one input file as prepare() opened it
    std::string path;
    FastxStream s;
    int fd = -1;                       // plain file: windows are staged with pread()
    const char *first_text = nullptr;  // the first raw window (prepare())
    uint64_t first_n = 0, first_resume = 0;
    bool have_first = false;
    uint32_t xz_spread = 0;    // --xz-spread for an .xz input under --device-xz (0 = the library's default)
    bool zstd_stream = false;  // --zstd-stream and more compressed bytes than --zstd-window: take_on_device opens a stream
    bool xz_stream = false;    // --xz-stream and more compressed bytes than --xz-window: likewise
    uint64_t xz_text_cap = 0;  // --xz-text-cap for that stream (0 = the library's default)
};

struct Source;

struct Side {  // one input's part of a window
    // ---- what the reader sets: the head, the body in one of three forms, where it ends and where its text lives
    std::vector<char> head;
    const char *body = nullptr;  // plain text body ...
    uint64_t n_body = 0;
    int pin = -1;                 // ... in this page-locked buffer of its source (-1: where the reader left it)
    std::vector<char> own;        // (first window of a compressed input: a copy of its own)
    std::vector<mk_bgzf_member> grp;  // ... or BGZF members
    const uint8_t *dev_body = nullptr;  // ... or a range of text that lies on the device
    uint64_t n_dev_body = 0, dev_off = 0;
    bool ends = true;             // the body ends at a record end
    Source *from = nullptr;       // the source that cut the body
    // the source was device text when this window was cut (a streamed gzip input is device text up to where its stream hands the file
    // back, host text behind): its tail and kept records come back from the device
    bool on_device = false;
    bool has_body() const { return n_body || !grp.empty() || n_dev_body; }
    uint64_t body_bytes() const {
        uint64_t n = n_body + n_dev_body;
        for (auto &e : grp) n += e.isize;
        return n;
    }
    // ---- what comes back from the device or the host call
    struct Result {
        std::vector<uint64_t> rec_start;
        uint64_t n_window = 0, n_used = 0;
        std::vector<char> tail;  // the text behind the processed records: the next window's head
        // MEMBERS / WRITTEN (-z, mk_extract_window_members; --zstd-output, mk_extract_window_frames): the kept records came down as BGZF
        // members (zstd frames) of their written form / as that
        // text (a window below --z-members-from), the ids of the kept records beside them -- the writer needs no stored text
        enum Layout { HEAD_BODY, PACKED_KEPT, WHOLE, MEMBERS, WRITTEN } layout = HEAD_BODY;
        std::vector<char> text;  // what the writer reads from unless HEAD_BODY: the kept records, the whole window, the host parser's text
        std::vector<char> ids;   // MEMBERS / WRITTEN with logs: the kept records' ids back to back, id_end[q] = where the q-th one's ends
        std::vector<uint64_t> id_end;
        uint64_t n_members = 0;
        FastxFile parsed;  // host-parsed window: the records (parsed.data = text)
    } out;
};

struct Win {
    uint64_t k = 0;
    int dev = 0;
    Side side[2];
    std::string error;  // a window that only carries a message: raised when the writer reaches it (after everything in front of it)
    uint64_t n_rec = 0, n_rows = 0;
    std::vector<uint8_t> keep;
    std::vector<uint64_t> kept;  // the indices of the kept records, built once where `keep` becomes final (the end of the device / host call)
    std::vector<mk_row> rows;
    mk_counters cb;
    std::vector<uint32_t> cnt;
    bool by_host = false;
    // --open-windows: `open` -- the window starts at a member, not at a record: the call finds its first record and `front` is the text
    // in front of it; `probe` -- a seam, tail(k - 1) ++ front(k) as host text; `refused` -- an open window or a seam the device did
    // not take as it is (the guess is disproved: the window is run again the chained way); `job` -- the writer waits for this one
    bool open = false, probe = false, refused = false, job = false;
    std::vector<char> front;
    float z_ms[4] = {0, 0, 0, 0};  // -z on the device: written form (select, scan, gather), cut, deflate, download (--zstd-output: cut is in deflate)
    void index_kept() {
        kept.clear();
        for (uint64_t r = 0; r < n_rec; ++r)
            if (keep[r]) kept.push_back(r);
    }
};

// page-locked staging buffers of a host-text source: one being filled, one per device in flight, one being written out
struct PinPool {
    std::vector<HostBuffer> bufs;
    std::deque<int> free;
    // page-locks every buffer (bytes each) and hands them to take() as they appear; raises cli::Error.  On a thread of its own
    void make(Gate &g, uint64_t bytes);
    int take(Gate &g);  // waits for a free buffer; -1: the job has failed
};

struct Source {
    virtual ~Source() = default;
    // fills S with the next body of about `target` bytes, for text window k; nothing: the input has no more.  m_ahead: the matcher window
    // k will run on (a staged body is sent ahead to it), or null
    virtual void next(uint64_t k, Side &S, uint64_t target, mk_matcher *m_ahead) = 0;
    virtual bool ended() const = 0;
    // the host never holds this source's text: windows are sized for the device, tails and kept records come back from it
    virtual bool on_device() const { return false; }
    // S's body (S.body_bytes() of it, S cut by this source) to dst on the host
    virtual void body_to_host(const Side &S, char *dst) const { memcpy(dst, S.body, (size_t)S.n_body); }
    // the window of S has left its device loop (called under the gate's lock): a page-locked buffer goes back to its pool
    virtual void window_left_device(Side &) {}
    virtual PinPool *pins() { return nullptr; }
    // the source has changed kind (a gzip stream that handed the file back to zlib): the source that reads on in its place, positioned
    // behind what the windows have used -- the chain's tail S.head is dropped, the caller asks the new source once more.  Else null
    virtual std::unique_ptr<Source> hand_back(Side &) { return nullptr; }
};

std::unique_ptr<Source> host_text_source(InputFile &f, int i, Gate &g);
std::unique_ptr<Source> members_source(InputFile &f);

// ---- extract_device_text.cpp (a CPU harness brings its own: no device, nothing taken)
uint64_t device_free_bytes(int device);  // 0: unknown
// Once the HIP runtime is up: tries to make input i's text on `device` -- a gzip or bzip2 file of more compressed bytes than
// stream_window (the window of its format: --gzip-window, --bzip2-window) window by window, a smaller one in one call -- and prints the
// [timing] rows.  -> the device source, or nothing: the host library reads the file
std::unique_ptr<Source> take_on_device(InputFile &f, int i, int device, uint64_t stream_window, Gate &g);

}  // namespace xw
}  // namespace cli
