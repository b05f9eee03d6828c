// tile_geometry.hpp -- how a text of n_bytes is cut into wave tiles for one scan launch (plain arithmetic, no host or
// device dependency: matcher.cpp fills ScanParams from it, mk_scan_tile_geometry exposes it to tests and tools).
//
// A tile is a whole number of four-chunk load groups: its scanned 1 KiB chunks plus ONE halo chunk (the next tile's
// first chunk, fetched so that the last lanes' q-grams can run over the tile's end).  The shorter the tile, the larger
// the share of the stream that is fetched twice: 1 chunk in 32 with 31-chunk tiles, 1 in 32 R with tiles of 32 R - 1.
// Tiles are dealt round-robin to the W scan waves, so a region of tiles is scanned evenly only if it is a whole number
// of rounds -- a last round that few waves take part in streams at a fraction of the bandwidth.  Hence two regions:
//
//   [0, n_long * long_bytes)                 first region: floor(n_main / (W * long_bytes)) whole rounds of long tiles
//   [.., tail_start)                         second region: less than one long round, cut into short tiles of
//                                            4 k - 1 chunks, k in 4..8 (15 .. 31 chunks), dealt round-robin as well
//   [tail_start, n_bytes)                    the kernel's guarded tail phase (less than 32 chunks)
//
// The short tiles' length is picked per launch too.  A last round that a third of the waves take part in does not
// keep enough loads in flight to fill HBM (4 KiB per wave; about 10 MB must be under way), so with 31-chunk tiles only,
// 10 M x 150 bp reads (R = 2: 5 long rounds, then 1.36 rounds of short tiles) ran 1 % slower than runs of two tiles
// had (profiles/r06_tile_geometry.txt).  Of the five lengths the one is taken that gives the busiest wave the fewest
// loads in the second region, the longer one on a tie: 23-chunk tiles in that case, two rounds, the last 84 % full.
//
// n_main = the bytes covered by the 31-chunk tiles whose 32 loads lie inside the text.  Tile i of the launch (both
// regions numbered through) belongs to wave i mod W; n_long is a multiple of W, so inside either region the waves'
// tile counts differ by at most one.  R = 1, or a text of less than one long round: one region of 31-chunk tiles
// (n_long = 0).
#pragma once
#include <stdint.h>

#include "filter.hpp"

namespace mk {

struct TileGeometry {
    uint64_t n_long, long_bytes;    // first region: tiles and scanned bytes per tile ((32 R - 1) chunks)
    uint64_t n_short, short_bytes;  // second region (15 .. kTileChunks chunks per tile)
    uint64_t tail_start;            // = n_long * long_bytes + n_short * short_bytes
    uint32_t long_loads, short_loads;  // chunk loads per tile, halo included: multiples of four
};

constexpr uint32_t kMaxTileRun = 8;

// R when the caller does not force one, from the 31-chunk tiles available per wave: long tiles where a wave has many
// (a wave gets at least four of them), short ones on small batches so that every wave still gets some.  On the 15 GB
// batch R = 4 takes 4 % off R = 1 (profiles/r02_tile_run.txt) and R = 8 another 1.6 % off R = 4: the slowest of eight
// runs at R = 8 beats the fastest of eight at R = 4 (profiles/r06_tile_geometry.txt)
MK_HD uint32_t tile_run_rule(uint64_t n_bytes, uint64_t n_waves) {
    const uint64_t tile_bytes = (uint64_t)kTileChunks * kChunkBytes;
    const uint64_t tiles_per_wave = n_waves ? (n_bytes + tile_bytes - 1) / tile_bytes / n_waves : 0;
    return tiles_per_wave >= 32 ? 8 : tiles_per_wave >= 16 ? 4 : tiles_per_wave >= 8 ? 2 : 1;
}

MK_HD TileGeometry tile_geometry(uint64_t n_bytes, uint64_t n_waves, uint32_t run) {
    TileGeometry g{};
    if (run < 1) run = 1;
    g.short_bytes = (uint64_t)kTileChunks * kChunkBytes;
    g.short_loads = (uint32_t)kTileChunks + 1;
    g.long_loads = run * g.short_loads;
    g.long_bytes = (uint64_t)(g.long_loads - 1) * kChunkBytes;
    const uint64_t n_main_tiles = n_bytes >= (uint64_t)kChunkBytes ? (n_bytes - kChunkBytes) / g.short_bytes : 0;
    if (run > 1 && n_waves) g.n_long = n_main_tiles * g.short_bytes / (n_waves * g.long_bytes) * n_waves;
    // (a long tile's halo load ends at n_long * long_bytes + 1 chunk <= n_main + 1 chunk <= n_bytes)
    const uint64_t long_end = g.n_long * g.long_bytes;
    const uint64_t rest = n_bytes >= (uint64_t)kChunkBytes ? n_bytes - kChunkBytes - long_end : 0;
    if (g.n_long) {  // short tiles of 4 k loads: the k that gives the busiest wave the fewest loads
        uint64_t best = ~0ull;
        for (uint32_t k = g.short_loads / 4; k >= 4; --k) {
            const uint64_t tiles = rest / ((uint64_t)(4 * k - 1) * kChunkBytes);
            const uint64_t loads = (tiles + n_waves - 1) / n_waves * (4 * k);
            if (loads < best) {
                best = loads;
                g.short_loads = 4 * k;
            }
        }
        g.short_bytes = (uint64_t)(g.short_loads - 1) * kChunkBytes;
    }
    g.n_short = rest / g.short_bytes;
    g.tail_start = long_end + g.n_short * g.short_bytes;
    return g;
}

}  // namespace mk
