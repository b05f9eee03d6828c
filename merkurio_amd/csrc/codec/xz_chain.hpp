// xz_chain.hpp -- an .xz file of any size decoded window by window (mk_xz_stream_*, include/merkurio_hip.h): everything the host
// decides about a window.  No HIP in it: xz_host.cpp runs it with the kernels of xz_inflate.hip behind `Dev`,
// tests/helpers/xz_windows_harness.cpp with the serial decoder of lzma_serial.hpp.  Host code only.
//
// xz is the easy format to window.  Blocks need nothing from each other, and the Index states every block's stored size and text size
// (xz_plan.hpp: xz_walk), so the WHOLE list of windows is made when the stream begins, before a bit is decoded: nothing grows, nothing
// is guessed, no history or table crosses a seam.  The plan is greedy and deterministic: a window is the longest run of consecutive
// blocks from the cursor whose text is at most the text cap T and whose compressed span -- from the first block's Block Header to the
// end of the last block's check -- is at most window_bytes (0 = no bound); one block at the least.  A window may run across stream
// boundaries, Stream Padding and streams of other check kinds: the span is uploaded as it lies in the file.
//
// What needs thought is the spread rule.  A window's decode costs as long as its slowest block (a block is one wave's serial decode:
// largest / r_wave), and liblzma would take text / r_lzma for it on the host, so many small windows cost more than one large one.
// With K = ceil(2 r_lzma / r_wave) (xz_plan.hpp: kXzSpreadDefault) the file is taken when
//      K x sum over the windows of (that window's largest block's text) <= the whole text,
// which with one window is the one-shot call's rule exactly.  KNOWN APPROXIMATION: the rule ignores that a window may hold more blocks
// than the device has resident waves (8 per CU at lc + lp = 3, by LDS); the one-shot rule ignores it too, and it is not modelled.
// The rule's consequence: with 24 MiB blocks and K = 107 a window must hold about 2.5 GiB of text or the file is refused, so
// window_bytes = 0 means "bounded by the text cap only", and the default T comes from the free device memory (xz_host.cpp), an
// unmeasured choice (profiles/e2e_unxz_windows.txt).
//
// A window's launch order: its blocks sorted by text size, largest first, so that in a window of more blocks than resident waves the
// longest block is not the last to start.  ASSUMPTION: that the dispatcher starts workgroups in index order.  Nothing depends on it
// for correctness: statuses and text positions go by block, not by workgroup.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../../include/merkurio_hip.h"
#include "lzma_serial.hpp"
#include "xz_plan.hpp"

namespace mkz {

// a block whose text alone exceeds the text cap (behind the container's -1 .. -19 and a block's -20 .. -32)
constexpr int kXzBlockOverCap = -33;

struct XzWindow {
    uint32_t first = 0, count = 0;  // blocks [first, first + count) of the plan
    uint64_t from = 0, to = 0;      // the compressed span in the file: first Block Header .. end of the last check
    uint64_t text = 0, largest = 0; // text bytes of the window, of its largest block
};

// the windows of a block table under (window_bytes, T): 0, or kXzBlockOverCap
inline int xz_windows(const XzPlan &P, uint64_t window_bytes, uint64_t T, std::vector<XzWindow> &out) {
    out.clear();
    const size_t B = P.blocks.size();
    for (size_t k = 0; k < B;) {
        XzWindow W;
        W.first = (uint32_t)k, W.from = P.head_off[k];
        for (; k < B; ++k) {
            const XzBlock &b = P.blocks[k];
            if (b.text_bytes > T) return kXzBlockOverCap;
            const uint64_t to = b.check_off + xz_check_bytes(b.check_kind);
            if (W.count && (b.text_bytes > T - W.text || (window_bytes && to - W.from > window_bytes))) break;
            W.count += 1, W.to = to, W.text += b.text_bytes, W.largest = std::max(W.largest, b.text_bytes);
        }
        out.push_back(W);
    }
    return 0;
}

// the spread rule over a list of windows
inline bool xz_windows_spread_ok(const XzPlan &P, const std::vector<XzWindow> &W, uint32_t spread) {
    uint64_t sum = 0;
    for (const XzWindow &w : W) sum += w.largest;  // (at most the whole text: below 2^62)
    return sum <= P.text_total / std::max(1u, spread);
}

// what a window's launch reads: its blocks with in_off / check_off counted from the upload's first byte and text_off from the window's
// text, the launch order, and the largest lc + lp of ITS chunks
struct XzWork {
    std::vector<XzBlock> blocks;
    std::vector<uint32_t> order;
    uint32_t lclp = 0;
    uint64_t from = 0, bytes = 0, text = 0;
};

struct XzStream {
    const uint8_t *xz = nullptr;  // the whole file, the caller's
    uint64_t n = 0;
    XzPlan P;
    std::vector<XzWindow> windows;
    size_t next = 0;
    bool dead = false;
    XzWork work;
    mk_xz_stream_stats stats{};
};

// mk_xz_stream_begin: the walk, the windows, the rules.  0: S is open; else the refusal (S.stats.status says it too, with what the
// walk found so far)
inline int xz_stream_open(XzStream &S, const uint8_t *xz, uint64_t n, uint64_t window_bytes, uint64_t T, uint32_t spread) {
    S = XzStream();
    S.xz = xz, S.n = n;
    int st = xz_walk(xz, n, S.P);
    if (!st) {
        S.stats.largest_block_text = S.P.largest_block_text;
        st = xz_windows(S.P, window_bytes, T, S.windows);
    }
    if (!st && !xz_windows_spread_ok(S.P, S.windows, spread)) st = kXzSpread;
    S.stats.status = st;
    if (st) {  // (only the figures are needed from here on: a table of up to 2^20 blocks does not stay with the handle)
        S.P = XzPlan(), std::vector<XzWindow>().swap(S.windows);
        return st;
    }
    S.stats.planned_windows = S.windows.size();
    return 0;
}

// the largest upload and table a planned window needs, beside two text buffers of the largest window's text (xz_host.cpp's room check)
inline void xz_stream_needs(const XzStream &S, uint64_t *text, uint64_t *upload, uint64_t *blocks) {
    *text = *upload = *blocks = 0;
    for (const XzWindow &w : S.windows)
        *text = std::max(*text, w.text), *upload = std::max(*upload, w.to - w.from), *blocks = std::max<uint64_t>(*blocks, w.count);
}

// window W of S rebased to its own upload and its own text -> K.  false: a Block Header that does not stand at a multiple of 4 of the
// file (the format puts every one there, and the walk's sizes are multiples of 4: the device reads dwords from the upload's first byte)
inline bool xz_window_work(const XzStream &S, const XzWindow &W, XzWork &K) {
    K.blocks.assign(S.P.blocks.begin() + W.first, S.P.blocks.begin() + W.first + W.count);
    K.from = W.from, K.bytes = W.to - W.from, K.text = W.text;
    if ((W.from & 3) || (K.bytes & 3)) return false;
    const uint64_t text0 = K.blocks.empty() ? 0 : K.blocks[0].text_off;
    for (size_t k = 0; k < K.blocks.size(); ++k) {
        XzBlock &b = K.blocks[k];
        if (S.P.head_off[W.first + k] & 3) return false;
        b.in_off -= W.from, b.check_off -= W.from, b.text_off -= text0;
    }
    K.lclp = xz_blocks_lclp(S.xz + W.from, K.blocks.data(), K.blocks.size());
    K.order.resize(K.blocks.size());
    for (uint32_t k = 0; k < K.order.size(); ++k) K.order[k] = k;
    std::stable_sort(K.order.begin(), K.order.end(), [&](uint32_t a, uint32_t b) { return K.blocks[a].text_bytes > K.blocks[b].text_bytes; });
    return true;
}

// streams closed once blocks [0, upto) are delivered: a stream without blocks closes with the blocks in front of it
inline uint64_t xz_streams_closed(const XzPlan &P, uint64_t upto) {
    uint64_t closed = 0;
    for (uint32_t e : P.stream_end) closed += e <= upto;
    return closed;
}

// One call of mk_xz_stream_next.  Dev is the device (or the harness's stand-in):
//   int decode(const XzWork &K)
//        K.bytes bytes of the file from K.from go up, K's blocks are decoded in K.order into the text buffer that does not hold the
//        latest window and their checks compared -> 0, or the status of the first block in FILE order that failed, or kXzTooLarge
//        (no room), kXzDevice
//   void commit(uint64_t text)
//        the window stands: that buffer is the latest window's, `text` bytes
// *state as the header says: 0 = *text_bytes of text stand in that buffer, 1 = end of file, 2 = handed back (S.stats.status: why).
template <class Dev>
void xz_stream_next(XzStream &S, Dev &dev, uint64_t *text_bytes, uint32_t *state) {
    *text_bytes = 0, *state = 2;
    if (S.dead) return;
    if (S.next == S.windows.size()) {
        S.stats.streams = S.P.streams, S.stats.consumed_bytes = S.n;
        *state = 1;
        return;
    }
    S.dead = true;  // (until the window stands)
    const XzWindow &W = S.windows[S.next];
    if (!xz_window_work(S, W, S.work)) {
        S.stats.status = kXzBlockHeader;
        return;
    }
    const int st = dev.decode(S.work);
    if (st) {
        S.stats.status = st;
        return;
    }
    dev.commit(W.text);
    ++S.next;
    S.stats.windows += 1, S.stats.blocks += W.count, S.stats.text_bytes += W.text;
    S.stats.consumed_bytes = S.next < S.windows.size() ? S.windows[S.next].from : S.n;
    S.stats.streams = S.next < S.windows.size() ? xz_streams_closed(S.P, (uint64_t)W.first + W.count) : S.P.streams;
    S.dead = false;
    *text_bytes = W.text, *state = 0;
}

}  // namespace mkz
