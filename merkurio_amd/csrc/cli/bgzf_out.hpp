// bgzf_out.hpp -- `extract -z`: the kept records written as BGZF members that end at record ends
#pragma once
#include "extract_common.hpp"

namespace cli {

// extract -z: the kept records of a Sink leave as BGZF members that end at record ends (the cut rule of include/merkurio_hip.h) --
// cut and deflated on the device (mk_bgzf_deflate_records), or, with --host-codec, cut by mk_bgzf_record_cuts and deflated by zlib at
// level 6 on the host threads (the checker: same cuts, same text).  The record text gathers in the Sink (Sink::z_text / z_ends);
// window_done() compresses what has gathered once it is worth a launch, finish() the rest and ends the output with the EOF member.
struct RecordGzip {
    void attach(Sink &sink, int device);  // device < 0: zlib on the host threads
    void window_done(bool force = false);
    // members made on the device (mk_extract_window_members): whatever text has gathered is forced out first, so that record order
    // holds, then the members are written through
    void put_members(const uint8_t *p, uint64_t n, uint64_t count);
    void finish();
    uint64_t members = 0;
    double cut_ms = 0, deflate_ms = 0, download_ms = 0;  // device codec: summed over the calls; host codec: deflate_ms alone

   private:
    Sink *sink_ = nullptr;
    int device_ = -1;
    mk_codec *codec_ = nullptr;
    std::string text_;
    std::vector<uint64_t> ends_;
    std::vector<uint8_t> out_;
};

}  // namespace cli
