// bgzf_out.hpp -- `extract -z`: the kept records written as BGZF members that end at record ends
#pragma once
#include "extract_common.hpp"

namespace cli {

// extract -z: the kept records of a Sink leave as BGZF members that end at record ends (the cut rule of include/merkurio_hip.h) --
// cut and deflated on the device (mk_bgzf_deflate_records), or, with --host-codec, cut by mk_bgzf_record_cuts and deflated by zlib at
// level 6 on the host threads (the checker: same cuts, same text).  The record text gathers in the Sink (Sink::z_text / z_ends);
// window_done() compresses what has gathered once it is worth a launch, finish() the rest and ends the output with the EOF member.
// extract --zstd-output: the same gathering, and the records leave as zstd frames that end at record ends (the rule with MK_ZSTD_CUT_GRID
// / MK_ZSTD_FRAME_TEXT_MAX): cut and compressed on the device (mk_zstd_deflate_records), or, with --host-codec, cut by
// mk_zstd_record_cuts and compressed by libzstd at level 3 on the host threads, every range a frame of its own with a checksum (the
// checker).  No end marker; a job that kept nothing writes one empty frame, so that the file is a valid .zst.
// On the window path a window whose kept records take --z-members-from bytes or more does not gather: it arrives as members / frames
// made on its own device (mk_extract_window_members / mk_extract_window_frames) and is passed through (put_members).
struct RecordGzip {
    void attach(Sink &sink, int device, bool zstd = false);  // device < 0: zlib / libzstd on the host threads
    void window_done(bool force = false);
    // members / frames made on the device (mk_extract_window_members / mk_extract_window_frames): whatever text has gathered is forced out
    // first, so that record order holds, then they are written through (frames: their block kinds are counted from their headers)
    void put_members(const uint8_t *p, uint64_t n, uint64_t count);
    void finish();
    uint64_t members = 0;          // BGZF members, or zstd frames
    uint64_t window_members = 0;   // ... of them through put_members: made on the windows' devices (the rest: from gathered text)
    uint64_t kinds[3] = {0, 0, 0};  // zstd frames of the device codec: Raw, RLE, Compressed blocks
    double upload_ms = 0;           // zstd frames of the device codec (cut_ms stays 0: the library times the cut kernel with the deflate)
    double cut_ms = 0, deflate_ms = 0, download_ms = 0;  // device codec: summed over the calls; host codec: deflate_ms alone

   private:
    void zstd_window();
    bool zstd_ = false;
    Sink *sink_ = nullptr;
    int device_ = -1;
    mk_codec *codec_ = nullptr;
    std::string text_;
    std::vector<uint64_t> ends_;
    std::vector<uint8_t> out_;
};

// decompress.cpp: src[0, n) as ONE zstd frame with a content checksum at `level`, by libzstd (bound with dlopen beside the decoder's symbols)
void zstd_compress_frame(const uint8_t *src, size_t n, int level, std::vector<uint8_t> &out);

}  // namespace cli
