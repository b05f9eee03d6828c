// extract_windows.hpp -- the state of one `merkurio extract` job over text windows, shared by the stages of its driver: the pipeline
// (extract_windows.cpp), the window call (extract_window_call.cpp) and the writer (extract_write.cpp).
#pragma once
#include <atomic>
#include <functional>
#include <map>

#include "extract_sources.hpp"

namespace cli {

struct WindowExtract::Impl {
    using Side = xw::Side;
    using Win = xw::Win;
    ExtractArgs a;
    std::vector<int> devs;
    int n_in = 1;
    xw::InputFile in[2];
    std::unique_ptr<xw::Source> src[2];  // the reader's: one per input (device threads go through Side::from)
    std::vector<std::unique_ptr<xw::Source>> retired;  // sources that changed kind: windows in flight still name them
    bool fastq = true;
    bool chained = false;
    uint64_t plain_target = 128ull << 20, bgzf_target = 1ull << 30;
    bool whole_text = false;  // -v with a log: the rows name records that are not kept -- BGZF windows hand their whole text back

    // ---- set by run()
    const Patterns *pats = nullptr;
    Loggers *lg = nullptr;
    std::vector<mk_matcher *> ms;
    std::vector<mk_codec *> codecs;
    uint64_t batch_bytes = 128ull << 20;

    // ---- pipeline state (under gate.mu)
    xw::Gate gate;
    std::vector<std::deque<std::unique_ptr<Win>>> queue;  // per device
    std::map<uint64_t, std::unique_ptr<Win>> done;        // finished windows by number
    std::map<uint64_t, std::vector<std::vector<char>>> tails;  // tails of finished windows (chained inputs)
    bool reader_done = false;
    uint64_t n_windows = 0;  // (valid once reader_done)
    uint64_t last_head[2] = {0, 0};  // (the reader's)
    // --open-windows (one BGZF input, plain-text output).  Under gate.mu: windows the writer is through with, whether
    // it has ended, whether the rest of the file is chained (4 disproved windows in a row), the seam / re-run the writer waits for
    bool open_mode = false, open_off = false, writer_done = false;
    uint64_t written = 0;
    std::unique_ptr<Win> job_done;
    uint64_t n_open = 0, n_seams = 0, n_reruns = 0;  // (the writer's)
    std::atomic<uint64_t> rec_cap_seen{0};
    // -z / --zstd-output: the kept records leave the device as BGZF members (mk_extract_window_members) / zstd frames
    // (mk_extract_window_frames) -- not with --host-codec, and not with logs under -v, whose rows name records that are not kept
    bool z_members = false;
    // the last window's needs, carried forward as rec_cap_seen is: bytes of members (or of text, for a window that came back as text)
    // and of ids per KiB of window text
    std::atomic<uint64_t> members_share_seen{0}, ids_share_seen{0};
    std::atomic<uint64_t> z_repeats{0};  // window calls made again because the members' or the ids' buffer was too small
    uint64_t z_member_windows = 0, z_text_windows = 0;  // (the writer's)
    double z_ms[4] = {0, 0, 0, 0};

    // ---- extract_windows.cpp
    bool members_input(int i) const { return !a.host_codec && in[i].s.raw_is_bgzf(); }
    void bound_device_windows();
    void take_inputs_on_device();
    // a .bz2 input of more compressed bytes than --bzip2-window: decoded window by window (under --host-codec no input is_bzip2)
    bool bzip2_streamed(int i) const { return in[i].s.raw_is_bzip2() && in[i].s.source().file_size() > a.bzip2_window; }
    // a .zst input of more compressed bytes than --zstd-window under --zstd-stream: likewise (without the flag it is libzstd's)
    bool zstd_streamed(int i) const { return a.zstd_stream && in[i].s.raw_is_zstd() && in[i].s.source().file_size() > a.zstd_window; }
    // an .xz input of more compressed bytes than --xz-window under --xz-stream: likewise (without the flag it is liblzma's)
    bool xz_streamed(int i) const { return a.xz_stream && in[i].s.raw_is_xz() && in[i].s.source().file_size() > a.xz_window; }
    void settle_bzip2(xw::InputFile &I);
    void reader_loop();
    void device_loop(size_t d);
    // ---- extract_window_call.cpp
    struct Call;
    void side_text(Side &S, std::vector<char> &out);
    void host_window(Win &W, mk_matcher *m);
    void device_window(Win &W, mk_matcher *m, mk_codec *codec);
    uint64_t bind_outputs(Win &W, Call &c);
    void guess_member_buffers(Win &W, Call &c);
    bool grow_named(Win &W, Call &c);
    void collect(Win &W, Call &c, mk_codec *codec);
    void pack_host_text(const Win &W, Side &S);
    // ---- extract_write.cpp
    void write_window(Win &W, Sink &w1, Sink &w2, const std::string &name1, const std::string &name2, PhaseTimer &tm);
    void write_members_window(Win &W, Sink **w, const std::string **names, PhaseTimer &tm);
    // (--open-windows: the writer's seam and re-run steps)
    std::unique_ptr<Win> run_job(std::unique_ptr<Win> W);
    std::unique_ptr<Win> settle_open_window(std::unique_ptr<Win> W, const std::vector<char> &prev_tail, int &disproved_in_a_row,
                                            const std::function<void(Win &)> &emit);
};

}  // namespace cli
