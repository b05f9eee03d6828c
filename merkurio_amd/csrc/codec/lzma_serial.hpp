// lzma_serial.hpp -- what one block of an .xz file means: its LZMA2 chunks and the LZMA packets inside them, written once for g++
// and hipcc from the xz file format specification 1.0.4 and the public-domain LZMA description (the range coder, the probability
// layout and the packet set of the LZMA SDK's specification).  The kernel of xz_inflate.hip runs lzma2_decode_block with a wave's
// policies, tests/helpers/xz_harness.cpp with the host's below; the container around the blocks is xz_plan.hpp's.
//
// Policies:
//   In      byte(i): byte i of the block's stored bytes (the decoder asks for no i at or past their count)
//   Probs   get(i) / set(i, v): the 11-bit probabilities; fill(n): entries [0, n) = 1024
//   Out     lit(pos, b), copy(pos, dist, len), stored(pos, in, at, n): text bytes from pos on; back(pos, dist): the text byte at
//           pos - dist, which must be the byte most recently written there; finish(pos): everything up to pos is in place
//   Census  hit(k): a counter of the harness (kLzCensus* below); nothing on the device
//
// A block is proved by three facts together: the control byte 0x00 sits exactly at its stored end, its text has exactly the length
// the Index states, and (the check kernel, or the harness) its check matches.  Everything else is a refusal with a name.
#pragma once
#include <stdint.h>

#include "deflate_common.hpp"

namespace mkz {

// ---- the probability model: 1846 entries and the literal coder's 768 << (lc + lp) behind them
constexpr uint32_t kLzIsMatch = 0, kLzIsRep = 192, kLzIsRepG0 = 204, kLzIsRepG1 = 216, kLzIsRepG2 = 228, kLzIsRep0Long = 240, kLzPosSlot = 432,
                   kLzSpecPos = 688, kLzAlign = 802, kLzLenCoder = 818, kLzRepLenCoder = 1332, kLzLiteral = 1846;
constexpr uint32_t kLzLenChoice = 0, kLzLenChoice2 = 1, kLzLenLow = 2, kLzLenMid = 130, kLzLenHigh = 258, kLzLenProbs = 514;
constexpr uint32_t kLzProbInit = 1024, kLzMaxLcLp = 4;
MKZ_HD uint32_t lzma_probs(uint32_t lclp) { return kLzLiteral + (768u << lclp); }
constexpr uint32_t kLzChunkTextMax = 2u << 20, kLzChunkStoredMax = 64u << 10;

// ---- refusals of a block (the container's are xz_plan.hpp's, -1 .. -19)
constexpr int kLzControl = -20, kLzNoDictReset = -21, kLzNoProps = -22, kLzProps = -23, kLzStoredPast = -24, kLzTextPast = -25, kLzRcInit = -26,
              kLzDistance = -27, kLzEndMarker = -28, kLzChunkEnd = -29, kLzBlockEnd = -30, kLzCheck = -31, kLzModelRoom = -32;

// ---- the census of the harness: what a file's blocks exercised
enum LzCensusKey {
    kLzcLit, kLzcMatchedLit, kLzcMatch, kLzcRep0, kLzcRep1, kLzcRep2, kLzcRep3, kLzcShortRep,
    kLzcLenLow, kLzcLenMid, kLzcLenHigh,
    kLzcSlotDirect, kLzcSlotTree, kLzcSlotAlign,
    kLzcChunkStoredReset, kLzcChunkStored, kLzcChunkLzma, kLzcChunkState, kLzcChunkProps, kLzcChunkAll,
    kLzcDistLtLen, kLzcDistAtDictStart, kLzcDistAtDictSize,
    kLzcKeys
};
struct LzNoCensus {
    MKZ_HD void hit(int) {}
};

// ---- the range decoder: 11-bit probabilities, shift 5, normalised below 2^24 in front of every bit
template <class In, class Probs>
struct LzRc {
    In &in;
    Probs &p;
    uint32_t range, code;
    uint64_t at, end;  // the chunk's stored bytes [at, end) still to read
    bool over;         // a byte past `end` was asked for (zeros are read instead, the chunk is refused at its end)
    MKZ_HD uint32_t next() {
        if (at >= end) {
            over = true;
            return 0;
        }
        return in.byte(at++);
    }
    MKZ_HD void norm() {
        if (range < (1u << 24)) range <<= 8, code = code << 8 | next();
    }
    MKZ_HD uint32_t bit(uint32_t i) {
        norm();
        const uint32_t pv = p.get(i), bound = (range >> 11) * pv;
        if (code < bound) {
            range = bound;
            p.set(i, pv + ((2048u - pv) >> 5));
            return 0;
        }
        range -= bound, code -= bound;
        p.set(i, pv - (pv >> 5));
        return 1;
    }
    MKZ_HD uint32_t direct(uint32_t n) {
        uint32_t r = 0;
        for (; n; --n) {
            norm();
            range >>= 1;
            code -= range;
            const uint32_t t = 0u - (code >> 31);
            code += range & t;
            r = (r << 1) + (t + 1);
        }
        return r;
    }
    MKZ_HD uint32_t tree(uint32_t base, uint32_t bits) {
        uint32_t m = 1;
        for (uint32_t k = 0; k < bits; ++k) m = m << 1 | bit(base + m);
        return m - (1u << bits);
    }
    MKZ_HD uint32_t tree_reverse(uint32_t base, uint32_t bits) {
        uint32_t m = 1, r = 0;
        for (uint32_t k = 0; k < bits; ++k) {
            const uint32_t b = bit(base + m);
            m = m << 1 | b, r |= b << k;
        }
        return r;
    }
    MKZ_HD uint32_t length(uint32_t base, uint32_t pos_state, uint32_t *range_class) {
        if (!bit(base + kLzLenChoice)) return *range_class = 0, 2 + tree(base + kLzLenLow + (pos_state << 3), 3);
        if (!bit(base + kLzLenChoice2)) return *range_class = 1, 10 + tree(base + kLzLenMid + (pos_state << 3), 3);
        return *range_class = 2, 18 + tree(base + kLzLenHigh, 8);
    }
};

// ---- host policies ---------------------------------------------------------------------------------------------------------------
struct LzSerialIn {
    const uint8_t *p;
    MKZ_HD uint32_t byte(uint64_t i) const { return p[i]; }
};
struct LzSerialProbs {
    uint16_t *v;
    MKZ_HD uint32_t get(uint32_t i) const { return v[i]; }
    MKZ_HD void set(uint32_t i, uint32_t x) { v[i] = (uint16_t)x; }
    MKZ_HD void fill(uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) v[i] = (uint16_t)kLzProbInit;
    }
};
struct LzSerialOut {
    uint8_t *text;
    MKZ_HD void lit(uint64_t pos, uint32_t b) { text[pos] = (uint8_t)b; }
    MKZ_HD uint32_t back(uint64_t pos, uint64_t dist) const { return text[pos - dist]; }
    MKZ_HD void copy(uint64_t pos, uint64_t dist, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k) text[pos + k] = text[pos + k - dist];
    }
    template <class In>
    MKZ_HD void stored(uint64_t pos, In &in, uint64_t at, uint32_t n) {
        for (uint32_t k = 0; k < n; ++k) text[pos + k] = (uint8_t)in.byte(at + k);
    }
    MKZ_HD void finish(uint64_t) {}
};

// the block's stored bytes in[0, in_bytes) -> its text of exactly text_bytes bytes.  dict_size: of the block's filter; lclp_room: the
// largest lc + lp the probabilities have room for.  0, or the refusal; *text_made = the text bytes in place either way
template <class In, class Probs, class Out, class Census>
MKZ_HD int lzma2_decode_block(In &in, uint64_t in_bytes, Probs &pr, Out &out, uint64_t text_bytes, uint32_t dict_size, uint32_t lclp_room, Census &cs,
                              uint64_t *text_made) {
    uint64_t at = 0, pos = 0, dict_start = 0;
    bool need_dict_reset = true, need_props = true;
    uint32_t lc = 0, lp = 0, pb = 0, state = 0, rep0 = 0, rep1 = 0, rep2 = 0, rep3 = 0, prev = 0;
    int st = 0;
    for (;;) {
        if (at >= in_bytes) {
            st = kLzStoredPast;
            break;
        }
        const uint32_t c = in.byte(at++);
        if (c == 0) break;
        if (c > 2 && c < 0x80) {
            st = kLzControl;
            break;
        }
        if (c >= 0xE0 || c == 1) {
            need_props = true, need_dict_reset = false;
            dict_start = pos, prev = 0;
        } else if (need_dict_reset) {
            st = kLzNoDictReset;
            break;
        }
        if (c < 0x80) {  // ---- a stored chunk
            if (at + 2 > in_bytes) {
                st = kLzStoredPast;
                break;
            }
            const uint32_t n = ((in.byte(at) << 8) | in.byte(at + 1)) + 1;
            at += 2;
            if (at + n > in_bytes) {
                st = kLzStoredPast;
                break;
            }
            if (pos + n > text_bytes) {
                st = kLzTextPast;
                break;
            }
            cs.hit(c == 1 ? kLzcChunkStoredReset : kLzcChunkStored);
            out.stored(pos, in, at, n);
            prev = in.byte(at + n - 1);
            at += n, pos += n;
            continue;
        }
        // ---- an LZMA chunk
        if (at + 4 + (c >= 0xC0 ? 1u : 0u) > in_bytes) {
            st = kLzStoredPast;
            break;
        }
        const uint32_t usize = (((c & 0x1fu) << 16) | (in.byte(at) << 8) | in.byte(at + 1)) + 1, csize = ((in.byte(at + 2) << 8) | in.byte(at + 3)) + 1;
        at += 4;
        if (c >= 0xC0) {
            uint32_t props = in.byte(at++);
            if (props > 224) {
                st = kLzProps;
                break;
            }
            pb = props / 45, props -= pb * 45, lp = props / 9, lc = props - lp * 9;
            if (lc + lp > kLzMaxLcLp) {
                st = kLzProps;
                break;
            }
            if (lc + lp > lclp_room) {
                st = kLzModelRoom;
                break;
            }
            need_props = false;
        } else if (need_props) {
            st = kLzNoProps;
            break;
        }
        if (c >= 0xA0) {
            state = 0, rep0 = rep1 = rep2 = rep3 = 0;
            pr.fill(lzma_probs(lc + lp));
        }
        cs.hit(c >= 0xE0 ? kLzcChunkAll : c >= 0xC0 ? kLzcChunkProps : c >= 0xA0 ? kLzcChunkState : kLzcChunkLzma);
        if (at + csize > in_bytes) {
            st = kLzStoredPast;
            break;
        }
        if (pos + usize > text_bytes) {
            st = kLzTextPast;
            break;
        }
        if (csize < 5) {
            st = kLzChunkEnd;
            break;
        }
        if (in.byte(at) != 0) {
            st = kLzRcInit;
            break;
        }
        LzRc<In, Probs> rc{in, pr, 0xffffffffu, 0, at + 5, at + csize, false};
        rc.code = in.byte(at + 1) << 24 | in.byte(at + 2) << 16 | in.byte(at + 3) << 8 | in.byte(at + 4);
        const uint64_t chunk_end = pos + usize;
        const uint32_t pos_mask = (1u << pb) - 1, lp_mask = (1u << lp) - 1;
        while (pos < chunk_end && !rc.over) {
            const uint32_t p = (uint32_t)(pos - dict_start), pos_state = p & pos_mask;
            if (!rc.bit(kLzIsMatch + (state << 4) + pos_state)) {
                const uint32_t probs = kLzLiteral + 0x300u * (((p & lp_mask) << lc) + (prev >> (8 - lc)));
                uint32_t sym = 1;
                if (state >= 7) {
                    // (a state of 7 and more was left by a match or a rep, whose distance was valid: rep0 + 1 <= pos - dict_start)
                    uint32_t mb = out.back(pos, (uint64_t)rep0 + 1), offs = 0x100;
                    cs.hit(kLzcMatchedLit);
                    do {
                        mb <<= 1;
                        const uint32_t bit = offs;
                        offs &= mb;
                        const uint32_t b = rc.bit(probs + offs + bit + sym);
                        sym = sym << 1 | b;
                        if (!b) offs ^= bit;
                    } while (sym < 0x100);
                } else {
                    do sym = sym << 1 | rc.bit(probs + sym);
                    while (sym < 0x100);
                }
                cs.hit(kLzcLit);
                prev = sym & 0xffu;
                out.lit(pos, prev);
                ++pos;
                state = state < 4 ? 0 : state < 10 ? state - 3 : state - 6;
                continue;
            }
            uint32_t len, len_class = 0;
            if (!rc.bit(kLzIsRep + state)) {
                rep3 = rep2, rep2 = rep1, rep1 = rep0;
                len = rc.length(kLzLenCoder, pos_state, &len_class);
                state = state < 7 ? 7 : 10;
                const uint32_t slot = rc.tree(kLzPosSlot + ((len < 6 ? len - 2 : 3u) << 6), 6);
                if (slot < 4) {
                    rep0 = slot;
                    cs.hit(kLzcSlotDirect);
                } else {
                    const uint32_t nd = (slot >> 1) - 1;
                    rep0 = (2u | (slot & 1u)) << nd;
                    if (slot < 14) {
                        rep0 += rc.tree_reverse(kLzSpecPos + rep0 - slot - 1, nd);
                        cs.hit(kLzcSlotTree);
                    } else {
                        rep0 += rc.direct(nd - 4) << 4;
                        rep0 += rc.tree_reverse(kLzAlign, 4);
                        cs.hit(kLzcSlotAlign);
                        if (rep0 == 0xffffffffu) {
                            st = kLzEndMarker;
                            break;
                        }
                    }
                }
                cs.hit(kLzcMatch);
            } else {
                if (!rc.bit(kLzIsRepG0 + state)) {
                    if (!rc.bit(kLzIsRep0Long + (state << 4) + pos_state)) {
                        if (rep0 >= p || rep0 >= dict_size) {
                            st = kLzDistance;
                            break;
                        }
                        cs.hit(kLzcShortRep);
                        state = state < 7 ? 9 : 11;
                        prev = out.back(pos, (uint64_t)rep0 + 1);
                        out.lit(pos, prev);
                        ++pos;
                        continue;
                    }
                    cs.hit(kLzcRep0);
                } else {
                    uint32_t d;
                    if (!rc.bit(kLzIsRepG1 + state)) {
                        d = rep1;
                        cs.hit(kLzcRep1);
                    } else {
                        if (!rc.bit(kLzIsRepG2 + state)) {
                            d = rep2;
                            cs.hit(kLzcRep2);
                        } else {
                            d = rep3, rep3 = rep2;
                            cs.hit(kLzcRep3);
                        }
                        rep2 = rep1;
                    }
                    rep1 = rep0, rep0 = d;
                }
                len = rc.length(kLzRepLenCoder, pos_state, &len_class);
                state = state < 7 ? 8 : 11;
            }
            cs.hit(kLzcLenLow + len_class);
            if (rep0 >= p || rep0 >= dict_size) {
                st = kLzDistance;
                break;
            }
            if (pos + len > chunk_end) {
                st = kLzTextPast;
                break;
            }
            if (rep0 + 1 < len) cs.hit(kLzcDistLtLen);
            if (rep0 + 1 == p) cs.hit(kLzcDistAtDictStart);
            if (rep0 + 1 == dict_size) cs.hit(kLzcDistAtDictSize);
            out.copy(pos, (uint64_t)rep0 + 1, len);
            pos += len;
            prev = out.back(pos, 1);
        }
        if (st) break;
        rc.norm();
        if (rc.over || pos != chunk_end || rc.at != rc.end || rc.code != 0) {
            st = kLzChunkEnd;
            break;
        }
        at = rc.end;
    }
    out.finish(pos);
    *text_made = pos;
    if (!st && (at != in_bytes || pos != text_bytes)) st = kLzBlockEnd;
    return st;
}

}  // namespace mkz
