// codec_stream.hpp -- what the entry points of the four streams (mk_gzip_stream_*, mk_bzip2_stream_*, mk_zstd_stream_*, mk_xz_stream_*)
// share: the frame of _next, _info and _end, and the close.  A stream is named by its member of the handle (&mk_codec::bzs); what a
// format decides about a window stays in its *_chain.hpp, what it does on the device in its *_host.cpp.  _begin is each format's own.
#pragma once
#include <algorithm>

#include "codec_internal.h"

namespace mkz {

// what only one format holds on the device beside the two text windows
inline void free_extra(mk_gzip_stream &S) {
    for (void *&p : S.d_carry) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
}
template <class Stream>
void free_extra(Stream &) {}

// An open stream ends: its device memory and the handle's scratch go back, its figures stay (mk_*_stream_info without an open stream:
// what the last one left)
template <class Stream>
void stream_close(mk_codec *c, Stream &S) {
    if (!S.active) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_extra(S);
    S.text.free_all();
    c->d_gz_text = nullptr, c->gz_text_cap = 0;  // (it pointed into one of the stream's two)
    gz_release(c);
    const auto last = S.info();
    S = Stream();
    S.info() = last;
}

inline uint64_t stream_held(const mk_codec *c, const TextWindows &text) { return c->gz_in_cap + c->gz_sym_cap + c->gz_tab_cap + c->gz_ctx_cap + text.held(); }

// mk_*_stream_next up to the format's own part: the arguments, *text_bytes = 0 and *state = 2, the lock, "no open stream"; then
// body(S), with the handle's mutex held
template <class Stream, class Body>
int stream_next(mk_codec *c, Stream mk_codec::*which, uint64_t *text_bytes, uint32_t *state, Body body) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !state) return mk::fail(MK_E_INVALID_ARG, "mk_%s_stream_next: NULL argument", Stream::format);
    *text_bytes = 0, *state = 2;
    std::lock_guard<std::mutex> lock(c->mu);
    Stream &S = c->*which;
    if (!S.active) return mk::fail(MK_E_INVALID_ARG, "mk_%s_stream_next: no open stream (mk_%s_stream_begin)", Stream::format, Stream::format);
    body(S);
    return MK_OK;
    MK_ABI_END
}

// ... of a stream whose windows a chain header decides (S.s: bzip2, zstd, xz): no text while the call runs, the device set -- or the
// stream handed back: no_device(S) may note why --, window(S) = the chain's *_stream_next over the format's Dev, then the window's text
// published on state 0 and the peak of what the stream holds
template <class Stream, class Window, class NoDevice>
int chain_stream_next(mk_codec *c, Stream mk_codec::*which, uint64_t *text_bytes, uint32_t *state, Window window, NoDevice no_device) {
    return stream_next(c, which, text_bytes, state, [&](Stream &S) {
        c->gz_text_bytes = 0;
        if (hipSetDevice(c->device) != hipSuccess) {
            (void)hipGetLastError();
            S.s.dead = true;
            no_device(S);
            return;
        }
        window(S);
        if (*state == 0) c->gz_text_bytes = *text_bytes;
        S.s.stats.peak_device_bytes = std::max<uint64_t>(S.s.stats.peak_device_bytes, stream_held(c, S.text));
    });
}
template <class Stream, class Window>
int chain_stream_next(mk_codec *c, Stream mk_codec::*which, uint64_t *text_bytes, uint32_t *state, Window window) {
    return chain_stream_next(c, which, text_bytes, state, window, [](Stream &) {});
}

// mk_*_stream_info.  It takes the lock that _next writes the figures under: a call beside it waits for the window.  No stream open:
// what the last one left (a refusal at _begin included, where the format notes one), zeros if there was none
template <class Stream, class Stats>
int stream_info(const mk_codec *c, Stream mk_codec::*which, Stats *out) {
    MK_ABI_BEGIN
    if (!c || !out) return mk::fail(MK_E_INVALID_ARG, "mk_%s_stream_info: NULL argument", Stream::format);
    mk_codec *m = const_cast<mk_codec *>(c);
    std::lock_guard<std::mutex> lock(m->mu);
    *out = (m->*which).info();
    return MK_OK;
    MK_ABI_END
}

// mk_*_stream_end
template <class Stream>
int stream_end(mk_codec *c, Stream mk_codec::*which) {
    MK_ABI_BEGIN
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_%s_stream_end: NULL handle", Stream::format);
    std::lock_guard<std::mutex> lock(c->mu);
    stream_close(c, c->*which);
    return MK_OK;
    MK_ABI_END
}

}  // namespace mkz
