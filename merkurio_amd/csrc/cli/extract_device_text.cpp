// extract_device_text.cpp -- the sources of the extract window driver whose text the device makes and keeps: the text of a gzip file
// inflated in one piece or member by member, or of a bzip2, (--device-zstd) zstd or (--device-xz) xz file (windows are ranges of it), and a gzip, bzip2, (--zstd-stream) zstd or (--xz-stream) xz file decoded window by
// window (mk_gzip_stream_*, mk_bzip2_stream_*, mk_zstd_stream_*, mk_xz_stream_*: one class over a table of calls), which may hand the file back to zlib / libbz2 / libzstd / liblzma mid-way.  Owns the step that tries the device for an input and the
// "free bytes on this device" helper.  Every HIP runtime call of the extract driver is in this file.
#include <hip/hip_runtime_api.h>

#include "extract_sources.hpp"

namespace cli {
namespace xw {

uint64_t device_free_bytes(int device) {
    size_t free_b = 0, total_b = 0;
    return hipSetDevice(device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (uint64_t)free_b : 0;
}

namespace {

struct DeviceText : Source {
    mk_codec *codec;
    const uint8_t *text = nullptr;  // (of a stream: the latest window's)
    uint64_t bytes = 0, at = 0;     // windows are text[at, ...) in turn
    explicit DeviceText(mk_codec *c) : codec(c) {}
    // (codec handles, like the page-locked buffers, are not released at the end of the run: that costs more than the process has left to live)
    ~DeviceText() override {
        if (!g_process_is_ending) mk_codec_destroy(codec);
    }
    bool on_device() const override { return true; }
    bool ended() const override { return at >= bytes; }
    void cut(Side &S, uint64_t target) {
        const uint64_t n = std::min<uint64_t>(target, bytes - at);
        S.dev_body = text + at, S.n_dev_body = n, S.dev_off = at;
        at += n;
    }
    void next(uint64_t, Side &S, uint64_t target, mk_matcher *) override {
        if (ended()) return;
        cut(S, target);
        S.ends = ended();
    }
    void body_to_host(const Side &S, char *dst) const override {
        mk_check(mk_gzip_text_read(codec, S.dev_off, (uint8_t *)dst, S.n_dev_body), "Error reading the inflated text back");
    }
};

// What differs between the formats the device decodes window by window: the library calls, and the wording of the [timing] rows
struct StreamCalls {
    const char *format, *host_library;  // "gzip" / "zlib"
    int (*begin)(mk_codec *, const uint8_t *file, uint64_t n, uint64_t window_bytes, uint32_t *taken);
    int (*next)(mk_codec *, uint64_t *text_bytes, uint32_t *state);
    int (*end)(mk_codec *);
    // the stream's own figures: compressed bytes consumed, what it counted, its phases and its peak
    void (*figures)(mk_codec *, uint64_t *consumed, std::string *counts, std::string *phases);
    // (may be null) the phases summed so far, for a window's row to show what each cost in that window
    void (*phase_ms)(mk_codec *, float ms[6]);
    const char *phase_names[6];
    bool discard_kept_on_error = false;  // the host library's error behind a hand-back leaves no kept records' file (Gate::discard_kept)
    void (*knobs)(mk_codec *, const InputFile &) = nullptr;  // the input's options that the stream takes when it begins
    std::string (*why_not)(mk_codec *) = nullptr;           // what the NOT taken row says of a refusal at _begin (the codec may be null)
    bool needs_codec = false;  // no codec handle is the run's error, not the host library's file
};

template <class... A>
std::string fmt(const char *f, A... a) {
    char buf[512];
    snprintf(buf, sizeof buf, f, a...);
    return buf;
}

const StreamCalls kGzipCalls = {"gzip", "zlib", mk_gzip_stream_begin, mk_gzip_stream_next, mk_gzip_stream_end, [](mk_codec *c, uint64_t *consumed, std::string *counts, std::string *phases) {
                                    mk_gzip_stream_stats st;
                                    memset(&st, 0, sizeof(st));
                                    (void)mk_gzip_stream_info(c, &st);
                                    *consumed = st.consumed_bytes;
                                    *counts = fmt("%llu windows, %llu members proved, %llu grown, %llu rounds repeated", (unsigned long long)st.windows, (unsigned long long)st.members,
                                                  (unsigned long long)st.windows_grown, (unsigned long long)st.rounds_repeated);
                                    *phases = fmt("upload %.1f, block search %.1f, pieces %.1f, resolution %.1f, CRC %.1f ms; peak %llu device bytes", st.ms[0], st.ms[1], st.ms[2],
                                                  st.ms[3], st.ms[4], (unsigned long long)st.peak_device_bytes);
                                }, nullptr, {}, false, nullptr, nullptr, true};
const StreamCalls kBzip2Calls = {"bzip2", "libbz2", mk_bzip2_stream_begin, mk_bzip2_stream_next, mk_bzip2_stream_end, [](mk_codec *c, uint64_t *consumed, std::string *counts, std::string *phases) {
                                     mk_bzip2_stream_stats st;
                                     memset(&st, 0, sizeof(st));
                                     (void)mk_bzip2_stream_info(c, &st);
                                     *consumed = st.consumed_bytes;
                                     *counts = fmt("%llu windows, %llu streams closed, %llu blocks, %llu grown", (unsigned long long)st.windows, (unsigned long long)st.streams,
                                                   (unsigned long long)st.blocks, (unsigned long long)st.windows_grown);
                                     *phases = fmt("upload %.1f, marker search %.1f, block decode %.1f, text %.1f, CRC %.1f ms; peak %llu device bytes", st.ms[0], st.ms[1], st.ms[2],
                                                   st.ms[3], st.ms[4], (unsigned long long)st.peak_device_bytes);
                                 }, nullptr, {}};
const StreamCalls kZstdCalls = {"zstd", "libzstd", mk_zstd_stream_begin, mk_zstd_stream_next, mk_zstd_stream_end, [](mk_codec *c, uint64_t *consumed, std::string *counts, std::string *phases) {
                                    mk_zstd_stream_stats st;
                                    memset(&st, 0, sizeof(st));
                                    (void)mk_zstd_stream_info(c, &st);
                                    *consumed = st.consumed_bytes;
                                    *counts = fmt("%llu windows, %llu frames closed, %llu blocks, %llu rounds, largest history %llu bytes", (unsigned long long)st.windows,
                                                  (unsigned long long)st.frames, (unsigned long long)st.blocks, (unsigned long long)st.rounds, (unsigned long long)st.max_history);
                                    *phases = fmt("upload %.1f, tables + entropy decode %.1f, walk + scans %.1f, execution %.1f, cross-block rounds %.1f, checksum %.1f ms; peak %llu device bytes",
                                                  st.ms[0], st.ms[1], st.ms[2], st.ms[3], st.ms[4], st.ms[5], (unsigned long long)st.peak_device_bytes);
                                }, [](mk_codec *c, float ms[6]) {
                                    mk_zstd_stream_stats st;
                                    memset(&st, 0, sizeof(st));
                                    (void)mk_zstd_stream_info(c, &st);
                                    for (int k = 0; k < 6; ++k) ms[k] = st.ms[k];
                                }, {"upload", "tables + entropy decode", "walk + scans", "execution", "cross-block rounds", "checksum"}};

const StreamCalls kXzCalls = {"xz", "liblzma", mk_xz_stream_begin, mk_xz_stream_next, mk_xz_stream_end, [](mk_codec *c, uint64_t *consumed, std::string *counts, std::string *phases) {
                                  mk_xz_stream_stats st;
                                  memset(&st, 0, sizeof(st));
                                  (void)mk_xz_stream_info(c, &st);
                                  *consumed = st.consumed_bytes;
                                  *counts = fmt("%llu planned windows, %llu windows, %llu blocks, %llu streams closed, largest block %llu text bytes, status %d", (unsigned long long)st.planned_windows,
                                                (unsigned long long)st.windows, (unsigned long long)st.blocks, (unsigned long long)st.streams, (unsigned long long)st.largest_block_text, (int)st.status);
                                  *phases = fmt("upload %.1f, decode %.1f, check %.1f, calls %.1f ms; peak %llu device bytes", st.ms[0], st.ms[1], st.ms[2], st.ms[3],
                                                (unsigned long long)st.peak_device_bytes);
                              }, nullptr, {}, true, [](mk_codec *c, const InputFile &f) {
                                  if (f.xz_spread) (void)mk_codec_set_xz_spread(c, f.xz_spread);
                                  if (f.xz_text_cap) (void)mk_codec_set_xz_text_cap(c, f.xz_text_cap);
                              }, [](mk_codec *c) {
                                  mk_xz_stream_stats st;
                                  memset(&st, 0, sizeof(st));
                                  if (c) (void)mk_xz_stream_info(c, &st);
                                  return fmt("status %d, largest block %llu text bytes; ", (int)st.status, (unsigned long long)st.largest_block_text);
                              }};

// A file the device decodes window by window (mk_gzip_stream_*, mk_bzip2_stream_*, mk_zstd_stream_*, mk_xz_stream_*).  Window w of the stream lies in text buffer w & 1
struct DeviceStream : DeviceText {
    const StreamCalls &calls;
    InputFile &f;
    const int i;
    Gate &g;
    uint64_t windows = 0;                 // windows the stream has produced
    uint64_t last_k[2] = {~0ull, ~0ull};  // the last text window whose body lies in either buffer
    uint64_t delivered = 0;               // text bytes of all its windows
    float seen_ms[6] = {0, 0, 0, 0, 0, 0};  // the stream's phases up to the window before (calls.phase_ms)
    enum { RUNNING, ENDED, HANDED_BACK } state = RUNNING;  // HANDED_BACK (the stream's state 2): the host library takes the file from the chain's tail on
    const double t0;
    DeviceStream(const StreamCalls &calls_, mk_codec *c, InputFile &f_, int i_, Gate &g_, double t0_) : DeviceText(c), calls(calls_), f(f_), i(i_), g(g_), t0(t0_) {}
    bool ended() const override { return state == ENDED; }

    // the next window of the stream; false: there is none -- the file has ended, or the stream has handed it back (what does not add
    // up, no room, any error of the device -- the codec rule).  Window w + 2 takes the text buffer of window w: not before every text
    // window over w has left its device loop
    bool next_window(uint64_t k) {
        for (;;) {
            const uint64_t last = last_k[windows & 1];
            if (last != ~0ull) {
                std::unique_lock<std::mutex> lk(g.mu);
                g.cv.wait(lk, [&] { return g.failed || g.n_done > last; });
                if (g.failed) return false;
            }
            const double t_win = PhaseTimer::now();
            uint64_t text_bytes = 0, consumed = 0;
            uint32_t st_now = 2;
            if (calls.next(codec, &text_bytes, &st_now) != MK_OK) st_now = 2;
            std::string counts, phases;
            calls.figures(codec, &consumed, &counts, &phases);
            std::string window_phases;
            if (calls.phase_ms) {
                float ms[6];
                calls.phase_ms(codec, ms);
                for (int p = 0; p < 6; ++p) window_phases += fmt("%s%s %.1f", p ? ", " : "; ", calls.phase_names[p], ms[p] - seen_ms[p]), seen_ms[p] = ms[p];
                window_phases += " ms";
            }
            if (st_now == 0) {
                if (g.timing)
                    fprintf(stderr, "[timing]   %s input %d on the device: window %llu taken, %llu text bytes, %llu compressed bytes consumed, %.1f ms (in front of text window %llu%s)\n",
                            calls.format, i, (unsigned long long)windows, (unsigned long long)text_bytes, (unsigned long long)consumed, (PhaseTimer::now() - t_win) * 1e3,
                            (unsigned long long)k, window_phases.c_str());
                ++windows;
                delivered += text_bytes;
                text = (const uint8_t *)mk_gzip_text_device(codec, &bytes);
                at = 0;
                if (bytes != text_bytes) st_now = 2;
                else if (text_bytes) return true;
                else continue;  // (a window of empty members / streams)
            }
            if (g.timing)
                fprintf(stderr, "[timing]   %s input %d on the device, window by window: %s, handed back at %s, %.3f s (%s)\n", calls.format, i, counts.c_str(),
                        st_now == 1 ? "-" : std::to_string(delivered).append(" text bytes (").append(calls.host_library).append(" reads on)").c_str(), PhaseTimer::now() - t0,
                        phases.c_str());
            bytes = at = 0;
            state = st_now == 1 ? ENDED : HANDED_BACK;
            return false;
        }
    }

    void next(uint64_t k, Side &S, uint64_t target, mk_matcher *) override {
        if (state != RUNNING) return;
        if (at >= bytes && !next_window(k)) return;  // (its end, or handed back)
        cut(S, target);
        // (that the text ends here is known only when the stream says so: the last window is then the chain's tail alone)
        last_k[(windows - 1) & 1] = k;
        S.ends = false;
    }
    // (mk_gzip_text_read refers to the stream's latest window, which S's may no longer be)
    void body_to_host(const Side &S, char *dst) const override {
        if (hipMemcpy(dst, S.dev_body, S.n_dev_body, hipMemcpyDeviceToHost) != hipSuccess) bail("Error reading the inflated text back");
    }
    // every text window over the stream's text is through: the host library reads the file from the front (a bzip2 file: libbz2
    // inflates it now, whole), drops what the windows have used -- all that was delivered but the chain's tail S.head, which starts at a
    // record start -- and is this input's reader from here on
    std::unique_ptr<Source> hand_back(Side &S) override {
        if (state != HANDED_BACK) return nullptr;
        const uint64_t used = delivered - std::min<uint64_t>(delivered, S.head.size());
        S.head.clear();
        (void)calls.end(codec);
        g.discard_kept = calls.discard_kept_on_error;  // (until the host library has read what the windows used)
        f.s.raw_settle();
        if (used) {
            f.have_first = false;
            if (!f.s.raw_skip(used)) bail("Error while decompressing " + f.path);
        }
        g.discard_kept = false;
        return host_text_source(f, i, g);
    }
};

}  // namespace

std::unique_ptr<Source> take_on_device(InputFile &f, int i, int device, uint64_t stream_window, Gate &g) {
    const bool bz = f.s.raw_is_bzip2(), zs = f.s.raw_is_zstd(), xz = f.s.raw_is_xz();
    if (!bz && !zs && !xz && !f.s.raw_is_gzip()) return nullptr;
    const uint8_t *z = f.s.source().file_bytes();
    const uint64_t n = f.s.source().file_size();
    double t0 = PhaseTimer::now();
    mk_codec *codec = nullptr;
    uint64_t text_bytes = 0;
    uint32_t taken = 0;
    // (the codec rule: whatever a call reports other than "taken" -- an error of the device included -- the file is the host library's)
    // A stream: --xz-stream / --zstd-stream, or a gzip or bzip2 file of more compressed bytes than one window.  It is decoded window by
    // window as the text windows reach it, device memory bounded by the window (xz: windows of whole blocks planned when the stream
    // begins; stream_window = 0: bounded by the text cap only).  What the stream does not take -- at its begin or from whichever window
    // on -- is the host library's, which also words the error
    const StreamCalls *sc = xz ? (f.xz_stream ? &kXzCalls : nullptr) : zs ? (f.zstd_stream ? &kZstdCalls : nullptr) : n <= stream_window ? nullptr : bz ? &kBzip2Calls : &kGzipCalls;
    if (sc) {
        const int made = mk_codec_create(device, &codec);
        if (sc->needs_codec) mk_check(made, "Error setting up the gzip codec");
        if (made != MK_OK) codec = nullptr;
        t0 = PhaseTimer::now();
        if (codec && sc->knobs) sc->knobs(codec, f);
        if (codec && sc->begin(codec, z, n, stream_window, &taken) != MK_OK) taken = 0;
        if (taken) return std::unique_ptr<Source>(new DeviceStream(*sc, codec, f, i, g, t0));
        if (g.timing)
            fprintf(stderr, "[timing]   %s input %d on the device, window by window: NOT taken (%s%s reads it)\n", sc->format, i, sc->why_not ? sc->why_not(codec).c_str() : "",
                    sc->host_library);
    } else if (xz) {
        // --device-xz: its blocks are decoded on the device, a wave each, in one call.  What the call does not take -- a file of one huge
        // block (the spread rule), anything else it refuses, a damaged file, no room -- and a file of more compressed bytes than
        // --xz-window, liblzma reads whole, as without the flag, and words the error
        uint64_t blocks = 0;
        if (n <= stream_window && mk_codec_create(device, &codec) != MK_OK) codec = nullptr;
        if (codec && f.xz_spread) (void)mk_codec_set_xz_spread(codec, f.xz_spread);
        if (codec && mk_xz_inflate_device(codec, z, n, &text_bytes, &taken, &blocks) != MK_OK) taken = 0;
        float ms4[4] = {0, 0, 0, 0};
        uint32_t streams = 0, status = 0;
        uint64_t largest = 0;
        if (codec) (void)mk_xz_info(codec, nullptr, &streams, &status, &largest, ms4);
        if (g.timing && taken) {
            fprintf(stderr, "[timing]   xz on the device: %llu blocks, %u streams, largest block %llu text bytes, upload %.1f, decode %.1f, check %.1f, total %.1f ms (input %d: %llu text bytes, %.3f s)\n",
                    (unsigned long long)blocks, streams, (unsigned long long)largest, ms4[0], ms4[1], ms4[2], ms4[3], i, (unsigned long long)text_bytes, PhaseTimer::now() - t0);
        } else if (g.timing) {
            char why[96];
            snprintf(why, sizeof why, "handed back, status %d, largest block %llu text bytes", (int)status, (unsigned long long)largest);
            fprintf(stderr, "[timing]   xz input %d: NOT taken by the device after %.3f s (%s; liblzma reads it)\n", i, PhaseTimer::now() - t0,
                    n > stream_window ? "more compressed bytes than --xz-window" : why);
        }
    } else if (zs) {
        // --device-zstd: its blocks are decoded on the device, a wave each, in one call.  What the call does not take -- anything it
        // refuses, a damaged file, no room -- and a file of more compressed bytes than --zstd-window, libzstd reads whole, as
        // without the flag, and words the error
        uint64_t blocks = 0;
        if (n <= stream_window && mk_codec_create(device, &codec) != MK_OK) codec = nullptr;
        if (codec && mk_zstd_inflate_device(codec, z, n, &text_bytes, &taken, &blocks) != MK_OK) taken = 0;
        if (g.timing && taken) {
            float ms6[6] = {0, 0, 0, 0, 0, 0};
            uint32_t frames = 0, rounds = 0;
            (void)mk_zstd_info(codec, nullptr, &frames, &rounds, ms6);
            fprintf(stderr, "[timing]   zstd on the device: %llu blocks, %u frames, %u rounds, upload %.1f, tables + entropy decode %.1f, scans %.1f, execution %.1f, cross-block rounds %.1f, checksum %.1f ms (input %d: %llu text bytes, %.3f s)\n",
                    (unsigned long long)blocks, frames, rounds, ms6[0], ms6[1], ms6[2], ms6[3], ms6[4], ms6[5], i, (unsigned long long)text_bytes, PhaseTimer::now() - t0);
        } else if (g.timing) {
            fprintf(stderr, "[timing]   zstd input %d: NOT taken by the device after %.3f s (%s; libzstd reads it)\n", i, PhaseTimer::now() - t0,
                    n > stream_window ? "more compressed bytes than --zstd-window" : "handed back");
        }
    } else if (bz) {
        // its blocks are decoded on the device, a wave each.  What the call does not take -- anything it refuses, a damaged file, no room
        // -- libbz2 reads whole, as under --host-codec, and words the error
        uint64_t blocks = 0;
        if (mk_codec_create(device, &codec) != MK_OK) codec = nullptr;
        if (codec && mk_bzip2_inflate_device(codec, z, n, &text_bytes, &taken, &blocks) != MK_OK) taken = 0;
        if (g.timing && taken) {
            float ms5[5] = {0, 0, 0, 0, 0};
            (void)mk_bzip2_info(codec, nullptr, ms5);
            fprintf(stderr, "[timing]   bzip2 on the device: %llu blocks, upload %.1f, marker search %.1f, block decode %.1f, text %.1f, CRC %.1f ms (input %d: %llu text bytes, %.3f s)\n",
                    (unsigned long long)blocks, ms5[0], ms5[1], ms5[2], ms5[3], ms5[4], i, (unsigned long long)text_bytes, PhaseTimer::now() - t0);
        } else if (g.timing) {
            fprintf(stderr, "[timing]   bzip2 input %d: NOT taken by the device after %.3f s (libbz2 reads it)\n", i, PhaseTimer::now() - t0);
        }
    } else {
        // ONE DEFLATE stream, which zlib walks from the front at 0.5 GB/s -- the device inflates it in parallel pieces and keeps the
        // text; a file of several members (`cat a.gz b.gz`) goes to mk_gzip_members_inflate_device, which cuts all of them into pieces
        // at once.  What neither takes (no findable block starts, a stream the buffers do not hold, bytes behind the last member, a
        // damaged file) stays with the zlib reader, which also words the errors
        mk_check(mk_codec_create(device, &codec), "Error setting up the gzip codec");
        t0 = PhaseTimer::now();
        mk_check(mk_gzip_inflate_device(codec, z, n, &text_bytes, &taken), "Error inflating the input");
        uint64_t members = taken ? 1 : 0, guesses = 0;
        if (!taken && mk_gzip_member_guesses(z, n, nullptr, 0, &guesses) == MK_OK && guesses > 1) {
            if (mk_gzip_members_inflate_device(codec, z, n, &text_bytes, &taken, &members) != MK_OK) taken = 0;
            if (!taken) members = 0;
        }
        if (g.timing) {
            uint32_t seg = 0;
            float ms5[5] = {0, 0, 0, 0, 0};
            (void)mk_gzip_info(codec, &seg, ms5);
            fprintf(stderr, "[timing]   gzip input %d on the device: %s, %llu members proved, %.3f s (%u pieces; upload %.1f, block search %.1f, pieces %.1f, resolution %.1f, CRC %.1f ms)\n", i,
                    taken ? "taken" : "NOT taken (zlib reads it)", (unsigned long long)members, PhaseTimer::now() - t0, seg, ms5[0], ms5[1], ms5[2], ms5[3], ms5[4]);
        }
    }
    if (!taken) {
        if (codec) mk_codec_destroy(codec);
        return nullptr;
    }
    std::unique_ptr<DeviceText> d(new DeviceText(codec));
    d->text = (const uint8_t *)mk_gzip_text_device(codec, &d->bytes);
    return d;
}

}  // namespace xw
}  // namespace cli
