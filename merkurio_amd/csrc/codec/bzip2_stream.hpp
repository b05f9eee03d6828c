// bzip2_stream.hpp -- the host's walk over a .bz2 file: from the table of magics found in it (every bit offset tested: the marker
// kernel of bzip2_inflate.hip, or bz2_find_markers below for the test harness) to the blocks and streams that table implies.  Shared
// by mk_bzip2_inflate_device (bzip2_host.cpp) and tests/helpers/bzip2_harness.cpp.  Host code only.
//
// The file is "BZh" + level at byte 0, the first magic at bit 32, then magic after magic: a block magic opens a block that must end
// exactly on the next magic of the table (which the decode proves or disproves), an end magic is followed by the stream's CRC, padding
// to the byte, and either the file's end or another "BZh" + level (pbzip2 output, `cat a.bz2 b.bz2`).  A table that does not chain this
// way -- a magic that is missing, one too many (a false hit inside a block's data: 2^-48 per bit), bytes behind the last stream -- is
// not walked any further: the caller leaves the file to libbz2.
#pragma once
#include <stdint.h>

#include <vector>

#include "bzip2_serial.hpp"

namespace mkz {

struct BzMarker {
    uint64_t bit;   // of the magic's first bit
    uint32_t kind;  // 0 = block, 1 = end of stream
};
struct BzPlanBlock {
    uint64_t bit, end_bit;  // its magic, and the magic it must end on
    uint32_t level, stream;
};
struct BzPlanStream {
    uint32_t level, first_block, n_blocks, crc;
};

inline void bz2_find_markers(const uint8_t *bz, uint64_t n, std::vector<BzMarker> &out) {
    const uint64_t mask = (1ull << 48) - 1;
    uint64_t v = 0;
    for (uint64_t i = 0; i < n; ++i)
        for (int k = 7; k >= 0; --k) {
            v = (v << 1 | (bz[i] >> k & 1u)) & mask;
            const uint64_t bit = i * 8 + (7 - k);
            if (bit >= 47 && (v == kBzBlockMagic || v == kBzEndMagic)) out.push_back(BzMarker{bit - 47, v == kBzEndMagic ? 1u : 0u});
        }
}

// markers: sorted by bit.  false = the table does not chain over bz[0, n)
inline bool bz2_plan(const uint8_t *bz, uint64_t n, const std::vector<BzMarker> &markers, std::vector<BzPlanBlock> &blocks, std::vector<BzPlanStream> &streams) {
    blocks.clear(), streams.clear();
    size_t m = 0;
    uint64_t pos = 0;
    if (n == 0) return false;
    while (pos < n) {
        if (n - pos < 14 || bz[pos] != 'B' || bz[pos + 1] != 'Z' || bz[pos + 2] != 'h' || bz[pos + 3] < '1' || bz[pos + 3] > '9') return false;
        BzPlanStream s{(uint32_t)(bz[pos + 3] - '0'), (uint32_t)blocks.size(), 0, 0};
        uint64_t at = pos * 8 + 32;
        for (;; ++m) {
            if (m >= markers.size() || markers[m].bit != at) return false;
            if (markers[m].kind == 1) break;
            if (m + 1 >= markers.size()) return false;
            at = markers[m + 1].bit;
            blocks.push_back(BzPlanBlock{markers[m].bit, at, s.level, (uint32_t)streams.size()});
            ++s.n_blocks;
        }
        const uint64_t crc_bit = markers[m++].bit + 48;
        if (crc_bit + 32 > n * 8) return false;
        for (uint32_t k = 0; k < 32; ++k) s.crc = s.crc << 1 | (bz[(crc_bit + k) >> 3] >> (7 - ((crc_bit + k) & 7)) & 1u);
        streams.push_back(s);
        pos = (crc_bit + 32 + 7) >> 3;
    }
    return m == markers.size();
}

}  // namespace mkz
