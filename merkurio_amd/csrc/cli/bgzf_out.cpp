// bgzf_out.cpp -- `extract -z` and `extract --zstd-output` (bgzf_out.hpp).  The reference writes plain text only (src/cmd_extract.rs:297-318).
#include "bgzf_out.hpp"

#include <chrono>

namespace cli {

void RecordGzip::attach(Sink &sink, int device, bool zstd) {
    sink_ = &sink, device_ = device, zstd_ = zstd;
    sink.flush();
    sink.z_text = &text_, sink.z_ends = &ends_;
    sink.z_window = [this] { window_done(); };
    sink.z_members = [this](const uint8_t *p, uint64_t n, uint64_t count) { put_members(p, n, count); };
}

void RecordGzip::window_done(bool force) {
    if (!sink_ || text_.empty() || (!force && text_.size() < (64u << 20))) return;
    if (ends_.empty() || ends_.back() != text_.size()) ends_.push_back(text_.size());  // (text behind the last marked record end: its own record)
    if (zstd_) return zstd_window();
    FILE *f = sink_->f;
    const auto t0 = std::chrono::steady_clock::now();
    if (device_ >= 0) {
        if (!codec_) mk_check(mk_codec_create(device_, &codec_), "Error setting up the BGZF codec");
        uint64_t need = 0, n_members = 0;
        // (every member stored: its text + 31 bytes -- the call then never has to run twice)
        out_.resize(std::max<size_t>(out_.size(), text_.size() + 31 * (text_.size() / MK_BGZF_CUT_GRID + 1)));
        for (int attempt = 0; attempt < 2; ++attempt) {
            const int rc = mk_bgzf_deflate_records(codec_, (const uint8_t *)text_.data(), text_.size(), ends_.data(), ends_.size(), out_.data(), out_.size(), &need,
                                                   &n_members);
            if (rc == MK_E_CAPACITY && attempt == 0) {
                out_.resize(need);
                continue;
            }
            mk_check(rc, "Error compressing the output");
            break;
        }
        float ms[3] = {0, 0, 0};
        (void)mk_codec_cut_times(codec_, nullptr, ms);
        cut_ms += ms[0], deflate_ms += ms[1], download_ms += ms[2];
        members += n_members;
        if (f && fwrite(out_.data(), 1, need, f) != need) bail("Error writing the compressed output");
    } else {
        uint64_t n_cuts = 0;
        std::vector<uint64_t> cut(text_.size() / MK_BGZF_CUT_GRID + 3);
        mk_check(mk_bgzf_record_cuts(ends_.data(), ends_.size(), cut.data(), cut.size(), &n_cuts), "Error compressing the output");
        const size_t blocks = (size_t)n_cuts - 1;
        std::vector<std::vector<uint8_t>> outs(blocks);
        const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), blocks));
        run_threads(T, [&](size_t t) {
            for (size_t i = t; i < blocks; i += T) bgzf_compress((const uint8_t *)text_.data() + cut[i], (size_t)(cut[i + 1] - cut[i]), outs[i]);
        });
        deflate_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        members += blocks;
        for (auto &o : outs)
            if (f && fwrite(o.data(), 1, o.size(), f) != o.size()) bail("Error writing the compressed output");
    }
    text_.clear(), ends_.clear();
}

// --zstd-output: what has gathered -> frames (on the one device codec of this output, whatever --gpus says: the windows that are worth
// a launch of their own have left as frames from their own devices, put_members)
void RecordGzip::zstd_window() {
    FILE *f = sink_->f;
    const auto t0 = std::chrono::steady_clock::now();
    if (device_ >= 0) {
        if (!codec_) mk_check(mk_codec_create(device_, &codec_), "Error setting up the zstd codec");
        uint64_t need = 0, n_frames = 0;
        out_.resize(std::max<size_t>(out_.size(), mk_zstd_deflate_bound(text_.size())));  // (every block raw: the call never has to run twice)
        mk_check(mk_zstd_deflate_records(codec_, (const uint8_t *)text_.data(), text_.size(), ends_.data(), ends_.size(), out_.data(), out_.size(), &need, &n_frames),
                 "Error compressing the output");
        uint32_t k[3] = {0, 0, 0};
        float ms[3] = {0, 0, 0};
        (void)mk_zstd_deflate_info(codec_, nullptr, k, ms);
        upload_ms += ms[0], deflate_ms += ms[1], download_ms += ms[2];
        for (int i = 0; i < 3; ++i) kinds[i] += k[i];
        members += n_frames;
        if (f && fwrite(out_.data(), 1, need, f) != need) bail("Error writing the compressed output");
    } else {
        uint64_t n_cuts = 0;
        std::vector<uint64_t> cut(text_.size() / MK_ZSTD_CUT_GRID + 3);
        mk_check(mk_zstd_record_cuts(ends_.data(), ends_.size(), cut.data(), cut.size(), &n_cuts), "Error compressing the output");
        const size_t blocks = (size_t)n_cuts - 1;
        std::vector<std::vector<uint8_t>> outs(blocks);
        const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), blocks));
        run_threads(T, [&](size_t t) {
            for (size_t i = t; i < blocks; i += T) zstd_compress_frame((const uint8_t *)text_.data() + cut[i], (size_t)(cut[i + 1] - cut[i]), 3, outs[i]);
        });
        deflate_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        members += blocks;
        for (auto &o : outs)
            if (f && fwrite(o.data(), 1, o.size(), f) != o.size()) bail("Error writing the compressed output");
    }
    text_.clear(), ends_.clear();
}

void RecordGzip::put_members(const uint8_t *p, uint64_t n, uint64_t count) {
    if (!sink_) return;
    window_done(true);
    if (sink_->f && n && fwrite(p, 1, n, sink_->f) != n) bail("Error writing the compressed output");
    members += count, window_members += count;
    if (!zstd_) return;
    // the kind of every frame's one block, from its header (include/merkurio_hip.h: 4 bytes of magic, the descriptor, 4 bytes of
    // content size, the 3-byte block header -- type in bits 1-2, size above --, the block, 4 bytes of checksum)
    uint64_t at = 0, seen = 0;
    for (; n - at >= 16; ++seen) {
        const uint32_t bh = p[at + 9] | (uint32_t)p[at + 10] << 8 | (uint32_t)p[at + 11] << 16, type = bh >> 1 & 3;
        if (type > 2) break;
        const uint64_t size = 16 + (type == 1 ? 1 : bh >> 3);
        if (size > n - at) break;
        kinds[type] += 1, at += size;
    }
    if (at != n || seen != count) bail("Error writing the compressed output: the frames of a window do not add up to its bytes");
}

void RecordGzip::finish() {
    if (!sink_) return;
    window_done(true);
    // (an empty frame: magic, descriptor 0xA4, content size 0, an empty last Raw block, the low 32 bits of XXH64 of nothing)
    static const uint8_t kEmptyFrame[16] = {0x28, 0xB5, 0x2F, 0xFD, 0xA4, 0, 0, 0, 0, 0x01, 0, 0, 0x99, 0xE9, 0xD8, 0x51};
    if (zstd_) {
        if (!members && sink_->f && fwrite(kEmptyFrame, 1, 16, sink_->f) != 16) bail("Error writing the compressed output");
        if (!members) members = 1, kinds[0] += 1;
    } else if (sink_->f && fwrite(mk_bgzf_eof(), 1, 28, sink_->f) != 28) bail("Error writing the compressed output");
    if (sink_->f) fflush(sink_->f);
    sink_->z_text = nullptr, sink_->z_ends = nullptr, sink_->z_window = nullptr, sink_->z_members = nullptr;
    if (codec_ && !g_process_is_ending) mk_codec_destroy(codec_);
    codec_ = nullptr, sink_ = nullptr;
}

}  // namespace cli
