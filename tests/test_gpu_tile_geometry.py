"""The scan's tile geometry (merkurio_amd/csrc/tile_geometry.hpp): a launch cuts its text into whole rounds of long
tiles (32 R - 1 KiB + a 1 KiB halo), then less than one such round in tiles of 15 .. 31 KiB, then the guarded tail.  The
arithmetic is checked on the CPU through mk_scan_tile_geometry; the kernels are checked on texts whose occurrences sit
on the boundaries that the geometry of the launch itself reports (mk_matcher_scan_geometry)."""
import random

import numpy as np
import pytest

import oracle_binding as ob

CHUNK = 1024
SHORT = 31 * CHUNK


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    return native


@pytest.fixture(scope="module")
def gpu(mk):
    if mk.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return mk


# ------------------------------------------------------------------ the arithmetic, no device
def _triples():
    rnd = random.Random(31)
    out = []
    for W in (1, 16, 48, 4096, 4864):
        for R in (1, 2, 4, 8):
            T = (32 * R - 1) * CHUNK
            sizes = {0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 15 * 10**9}
            for tile in (SHORT, T):
                sizes |= {tile - 1, tile, tile + 1, tile + CHUNK - 1, tile + CHUNK, tile + CHUNK + 1}
                sizes |= {W * tile - 1, W * tile, W * tile + 1, W * tile + CHUNK - 1, W * tile + CHUNK, W * tile + CHUNK + 1}
            sizes |= {rnd.randrange(0, 3 * W * T + 2) for _ in range(4)}
            out += [(n, W, R) for n in sorted(sizes)]
    return out


def test_tile_geometry_arithmetic(mk):
    """both regions and the tail cover [0, n_bytes) exactly once, the first region is whole rounds, the waves' tile
    counts differ by at most one inside a region, every tile is a whole number of four-load groups whose loads lie
    inside the text, the short tiles have the length that gives the busiest wave the fewest loads, and R = 1 is the
    single region of 31-chunk tiles"""
    triples = _triples()
    assert len(triples) >= 300
    for n, W, R in triples:
        g = mk.scan_tile_geometry(n, W, R)
        ctx = (n, W, R, g)
        T = (32 * R - 1) * CHUNK
        assert (g["n_waves"], g["tile_run"]) == (W, R), ctx
        S = g["short_tile_bytes"]
        assert (g["long_tile_bytes"], g["long_tile_loads"]) == (T, 32 * R), ctx
        assert g["short_tile_loads"] in (16, 20, 24, 28, 32), ctx
        assert g["long_tile_loads"] % 4 == 0 and g["short_tile_loads"] % 4 == 0, ctx
        assert g["long_tile_loads"] * CHUNK == T + CHUNK and g["short_tile_loads"] * CHUNK == S + CHUNK, ctx  # one halo chunk each
        # the regions are consecutive: [0, long_end) [long_end, tail_start) [tail_start, n)
        long_end = g["n_long_tiles"] * T
        assert g["tail_start"] == long_end + g["n_short_tiles"] * S, ctx
        assert g["tail_start"] <= n and n - g["tail_start"] < S + CHUNK <= 32 * CHUNK, ctx  # the tail: fewer than 32 chunks
        if g["n_long_tiles"] + g["n_short_tiles"]:
            assert g["tail_start"] + CHUNK <= n, ctx  # the last tile's halo load lies inside the text
        # the first region: the largest whole number of rounds that fits the 31-chunk tiles' bytes
        n_main = (n - CHUNK) // SHORT * SHORT if n >= CHUNK else 0
        assert g["n_long_tiles"] % W == 0, ctx
        if R > 1:
            assert g["n_long_tiles"] // W == n_main // (W * T), ctx
        # the second region ends with its last whole tile and is (but for a 31-chunk tile) less than one long round
        rest = n - CHUNK - long_end if n >= CHUNK else 0
        assert g["n_short_tiles"] == rest // S, ctx
        if R > 1:
            assert g["n_short_tiles"] * S < W * T + SHORT, ctx
        # (tile i belongs to wave i mod W and n_long_tiles is a multiple of W: per-wave counts differ by at most one)
        # the short tiles' length: behind long tiles the one of 15, 19 .. 31 chunks with which the busiest wave has the
        # fewest loads in the second region, the longest such; 31 chunks where there are no long tiles
        loads = {k: -(-(rest // ((4 * k - 1) * CHUNK)) // W) * 4 * k for k in (8, 7, 6, 5, 4)}
        best = min(loads, key=lambda k: (loads[k], -k)) if g["n_long_tiles"] else 8
        assert g["short_tile_loads"] == 4 * best, (ctx, loads)
        if R == 1:
            assert g["n_long_tiles"] == 0 and g["n_short_tiles"] == n_main // SHORT and g["tail_start"] == n_main, ctx
    # the headline batch at R = 4: 115 342 long tiles' worth of text, 28 whole rounds of 4096, the rest in short tiles
    g = mk.scan_tile_geometry(15 * 10**9, 4096, 4)
    assert g["n_long_tiles"] == 28 * 4096 and 0 < g["n_short_tiles"] * g["short_tile_bytes"] < 4096 * 127 * CHUNK
    # 10 M x 150 bp reads, R = 2: 5 long rounds, then 23-chunk tiles in two rounds (31-chunk ones: 1.36 rounds)
    g = mk.scan_tile_geometry(15 * 10**8, 4096, 2)
    assert (g["n_long_tiles"], g["short_tile_loads"], -(-g["n_short_tiles"] // 4096)) == (5 * 4096, 24, 2)
    # R = 0: the rule a scan applies by itself -- long tiles only where a wave has many 31-chunk tiles
    assert mk.scan_tile_geometry(15 * 10**9, 4096, 0) == mk.scan_tile_geometry(15 * 10**9, 4096, 8)
    assert [mk.scan_tile_geometry(n * 10**8, 4096, 0)["tile_run"] for n in (1, 10, 11, 20, 21, 41, 42)] == [1, 1, 2, 2, 4, 4, 8]
    for bad in ((10, 0, 1), (10, 16, 9)):
        with pytest.raises(mk.MerkurioError):
            mk.scan_tile_geometry(*bad)


# ------------------------------------------------------------------ small texts: every forced tile length
_Z = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(61).integers(0, 4, 61)])
_PATTERNS31 = sorted({_Z[i:i + 31] for i in range(31)})  # planting _Z at b - 30 puts an occurrence on each of the 30 bytes before b and on b


def _tiles(g):
    T, S, n_long = g["long_tile_bytes"], g["short_tile_bytes"], g["n_long_tiles"]
    return [(i * T, T) for i in range(n_long)] + [(n_long * T + j * S, S) for j in range(g["n_short_tiles"])]


def _small_case(mk, R, delta, options):
    """text of 19 forced tile lengths + delta; -> (records, plants' boundaries)"""
    T = (32 * R - 1) * CHUNK
    n = 19 * T + delta
    rnd = np.random.default_rng(1000 * R + delta)
    seq = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rnd.integers(0, 4, n)].tobytes())
    m = mk.Matcher(_PATTERNS31, algo=mk.MK_ALGO_AC, options=options)
    cut = 40001  # a record border inside a tile
    m.scan([bytes(seq[:cut]), bytes(seq[cut:])], mk.MK_MODE_ANY)  # the geometry depends on the text's length alone
    g = m.scan_geometry()
    assert g["tile_run"] == R and g["long_tile_bytes"] == T
    tiles = _tiles(g)
    if R > 1:  # the forced length is what runs: one round of long tiles, the rest short, every wave at most one long tile
        assert g["n_long_tiles"] == g["n_waves"] > 0 and g["n_short_tiles"] > 0
    assert g["tail_start"] == tiles[-1][0] + tiles[-1][1] and g["tail_start"] + CHUNK <= n
    ends = [tiles[1][0] + tiles[1][1],                      # a tile of the forced length (first region, or R = 1's only one)
            tiles[5][0] + tiles[5][1],
            g["n_long_tiles"] * T if R > 1 else tiles[9][0],  # first region / second region
            tiles[-2][0] + tiles[-2][1],                    # between two short tiles
            g["tail_start"],                                # the last main tile / the guarded tail
            tiles[2][0] + 36 * CHUNK]                       # a load-group border inside a tile
    for b in ends:
        assert b - 30 >= 0 and b + 31 <= n
        seq[b - 30:b + 31] = _Z
    seq[0:31] = _PATTERNS31[3]        # the first byte of the first tile
    seq[n - 31:n] = _PATTERNS31[7]    # ends on the last byte of the text
    return m, g, [bytes(seq[:cut]), bytes(seq[cut:])], len(ends)


@pytest.mark.gpu
@pytest.mark.parametrize("R,options", [
    (1, {}), (2, {}), (4, {}), (8, {}),
    (2, dict(force_global_filter=True, force_stride=8)), (8, dict(force_global_filter=True, force_stride=8)),  # context kernel <8,24>
], ids=["R1", "R2", "R4", "R8", "R2-ctx", "R8-ctx"])
def test_small_texts_every_tile_length(gpu, R, options):
    """occurrences starting on the first byte of a tile, on each of its last 30 bytes (they need the halo chunk), astride
    the two regions, astride the last main tile and the guarded tail, and ending on the text's last byte: flags and
    tuples as the CPU oracle gives them, for text lengths of k T + {0, 1, 1023, 1024, 1025}"""
    mk = gpu
    om = ob.Matcher(_PATTERNS31, True, 0, False)
    for delta in (0, 1, 1023, 1024, 1025):
        m, g, recs, n_ends = _small_case(mk, R, delta, dict(tile_run=R, **options))
        if options:
            assert m.filter_mode()["in_lds"] is False
        _, rows, _, found = ob.tag_records(om, recs, logging=True)
        exp = [(r, p, pos) for (_, r, p, pos) in rows]
        assert len(exp) >= 31 * n_ends + 2
        flags, hits = m.scan(recs, mk.MK_MODE_HITS, hits_cap=len(exp) + 16)
        assert m.scan_geometry() == g
        assert flags.tolist() == [bool(f) for f in found], (R, delta)
        assert list(zip(hits["rec"].tolist(), hits["pat"].tolist(), hits["pos"].tolist())) == exp, (R, delta)
        flags, _ = m.scan(recs, mk.MK_MODE_ANY)
        assert flags.tolist() == [bool(f) for f in found], (R, delta)


# ------------------------------------------------------------------ several rounds, both regions
@pytest.mark.gpu
def test_several_rounds_both_regions(gpu):
    """about 2.3 rounds of 63 KiB tiles (forced R = 2) of 150-byte records generated on the device, known 31-mers
    written astride the boundaries that the launch's own geometry reports: the flagged records are exactly the
    planted ones, MK_SUM_HITS counts them, flags and tuples equal those of the same text scanned with R = 1"""
    mk = gpu
    import torch
    dev = torch.device("cuda:0")
    lib = mk.load()
    rnd = np.random.default_rng(77)
    patterns = sorted({bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rnd.integers(0, 4, 31)]) for _ in range(24)})
    npat, L, R = len(patterns), 150, 2
    m2 = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=dict(tile_run=R))
    m1 = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=dict(tile_run=1))
    W = torch.cuda.get_device_properties(0).multi_processor_count * 16
    T = (32 * R - 1) * CHUNK
    n_rec = int(2.3 * W * T) // L
    n_bytes = n_rec * L
    st = torch.cuda.current_stream().cuda_stream
    d_seq = torch.empty(n_bytes + 64, dtype=torch.uint8, device=dev)
    d_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    assert lib.mk_synth_reads_device(m2.handle, 0xBEEF, n_rec, L, 0, d_seq.data_ptr(), d_off.data_ptr(), st) == 0  # nothing planted

    def scan(m, mode, cap=0):
        flags = torch.empty((n_rec + 7) // 4 * 4, dtype=torch.uint8, device=dev)
        hits = torch.empty(max(cap, 1) * 2, dtype=torch.int64, device=dev)
        nh = torch.zeros(1, dtype=torch.int64, device=dev)
        cnt = torch.zeros(npat + mk.MK_NUM_SUMMARY, dtype=torch.int64, device=dev)
        rc = lib.mk_scan_device(m.handle, d_seq.data_ptr(), n_bytes, d_off.data_ptr(), n_rec, mode, flags.data_ptr(), hits.data_ptr(), cap,
                                nh.data_ptr(), cnt.data_ptr(), st)
        assert rc == 0, lib.mk_last_error()
        torch.cuda.synchronize()
        h = np.frombuffer(hits[:2 * min(int(nh.item()), cap)].cpu().numpy().tobytes(), dtype=mk.HIT_DTYPE)
        return flags[:n_rec], np.sort(h, order=["rec", "pat", "pos"]), int(nh.item()), cnt.cpu().numpy()[npat:]

    f0, _, _, c0 = scan(m2, mk.MK_MODE_ANY)
    assert int(f0.sum(dtype=torch.int64).item()) == 0 and c0[mk.MK_SUM_HITS] == 0  # random text holds none of the 31-mers
    g = m2.scan_geometry()
    assert (g["n_waves"], g["tile_run"], g["long_tile_bytes"]) == (W, R, T)
    S = g["short_tile_bytes"]
    assert g["n_long_tiles"] == 2 * W and 1000 < g["n_short_tiles"] < W * T // S + 1  # two whole rounds, then less than one in short tiles
    long_end = g["n_long_tiles"] * T
    # (boundary, what to move it by if it falls on a record border, where no occurrence can lie astride it)
    bounds = [(long_end, 0),                                      # first region / second region
              (W * T, 0), (W * T - T, -T), (W * T + T, T),        # a round's end: the tiles of the last wave, of wave 0, and their neighbours
              (1000 * T, T), ((W + 1777) * T, T), (T, T),         # long tiles' ends in both rounds
              (long_end + S, S), (long_end + 1000 * S, S),  # short tiles' ends
              (g["tail_start"] - S, -S), (g["tail_start"], 0)]  # the second region's last tile / the tail
    assert g["tail_start"] + CHUNK <= n_bytes
    bounds = [b + step if b % L == 0 else b for b, step in bounds]
    assert len(set(bounds)) == len(bounds) and all(b % L for b in bounds), "a region boundary on a record border: choose another text length"
    exp = []
    for i, b in enumerate(bounds):
        # the occurrence starts `o` bytes before the boundary and stays inside one record
        o = next(o for o in (15, 1, 30, 8, 23, 4, 27, *range(1, 31)) if (b - o) % L <= L - 31)
        at = b - o
        assert at < b < at + 31
        pat = (5 * i) % npat
        d_seq[at:at + 31] = torch.frombuffer(bytearray(patterns[pat]), dtype=torch.uint8).to(dev)
        exp.append((at // L, pat, at % L))
    assert len({r for r, _, _ in exp}) == len(exp)
    exp_h = np.sort(np.array(exp, dtype=mk.HIT_DTYPE), order=["rec", "pat", "pos"])
    exp_f = torch.zeros(n_rec, dtype=torch.uint8, device=dev)
    exp_f[torch.tensor([r for r, _, _ in exp], device=dev)] = 1

    f2, _, _, c2 = scan(m2, mk.MK_MODE_ANY)
    assert m2.scan_geometry() == g
    assert torch.equal(f2, exp_f) and c2[mk.MK_SUM_HITS] == len(exp) and c2[mk.MK_SUM_RECORDS_HIT] == len(exp)
    f1, _, _, c1 = scan(m1, mk.MK_MODE_ANY)
    assert m1.scan_geometry()["n_long_tiles"] == 0
    same = [mk.MK_SUM_HITS, mk.MK_SUM_RECORDS_HIT, mk.MK_SUM_RECORDS, mk.MK_SUM_BASES]
    assert torch.equal(f1, f2) and np.array_equal(c1[same], c2[same])
    # hits mode: the same, and the tuples
    f2h, h2, nh2, c2h = scan(m2, mk.MK_MODE_HITS, 1024)
    f1h, h1, nh1, c1h = scan(m1, mk.MK_MODE_HITS, 1024)
    assert torch.equal(f2h, exp_f) and torch.equal(f1h, exp_f)
    assert nh2 == nh1 == len(exp) == c2h[mk.MK_SUM_HITS] == c1h[mk.MK_SUM_HITS]
    assert np.array_equal(h2, exp_h) and np.array_equal(h1, exp_h)
