"""tests/deflate_read.py (the token-level DEFLATE reader) against zlib, and tests/deflate_texts.py (the crafted texts of the deflate
writer's GPU tests) against what they claim about themselves.  No GPU: when an assertion of test_gpu_deflate_craft.py fails, the
reader and the texts have been checked here, and the fault is the kernel's."""
import collections
import zlib

import pytest

import deflate_craft as craft
import deflate_read as dr
import deflate_texts as dt
from test_codec_cpu import corpora, raw_deflate

SETTINGS = {"level-0": {"level": 0}, "level-1": {"level": 1}, "level-6": {"level": 6}, "level-9": {"level": 9},
            "fixed": {"strategy": zlib.Z_FIXED}, "huffman-only": {"strategy": zlib.Z_HUFFMAN_ONLY}, "rle": {"strategy": zlib.Z_RLE},
            "flush-5000": {"flush_every": 5000}}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_reader_renders_what_zlib_wrote(setting):
    for name, data in corpora().items():
        z = raw_deflate(data, **SETTINGS[setting])
        blocks = dr.read(z)
        assert dr.render(blocks) == data, name
        assert blocks[-1]["final"] and 0 <= 8 * len(z) - blocks[-1]["end"] <= 7, name
        assert all(b["start"] == a["end"] for a, b in zip(blocks, blocks[1:]))
        found = [t for b in blocks for t in dr.matches(b["tokens"])]
        if setting == "huffman-only":
            assert not found, name
        if setting == "rle":
            assert all(d == 1 for _, d in found), name
        if setting == "level-0":
            assert all(b["type"] == 0 for b in blocks), name
        if setting == "fixed":
            assert all(b["type"] in (0, 1) for b in blocks), name  # (zlib still stores what fixed codes would grow)
        for b in blocks:
            if b["type"] == 2:
                assert len(b["ll"]) == b["hlit"] and len(b["d"]) == b["hdist"] and dr.kraft(b["ll"]) == 1 << 15


def test_reader_reads_back_the_hand_made_tokens():
    """the `ok-` streams of the catalogue are written from token lists: the same lists come back, block by block, with the code
    lengths of the dynamic blocks; what zlib refuses (`bad-`) raises"""
    builders = {}
    real_ok = craft.stream

    def spy(blocks, tail=b""):  # the catalogue keeps the bytes only: build it once more and keep the block lists
        raw = real_ok(blocks, tail)
        builders[raw] = blocks
        return raw
    craft.stream = spy
    try:
        written_before = dict(craft.WRITTEN)
        cat = craft._catalogue()
    finally:
        craft.stream = real_ok
        craft.WRITTEN.clear()
        craft.WRITTEN.update(written_before)
    assert [(n, r) for n, r, _ in cat] == [(n, r) for n, r, _ in craft.CATALOGUE]
    n_ok = 0
    for name, raw, _ in cat:
        if name.startswith("bad-"):
            with pytest.raises(dr.DeflateError):
                dr.read(raw)
            continue
        n_ok += 1
        blocks, made = dr.read(raw), builders[raw]
        assert len(blocks) == len(made), name
        for got, want in zip(blocks, made):
            assert got["type"] == want["type"], name
            if want["type"] == 0:
                assert got["data"] == want["data"], name
            else:
                assert got["tokens"] == want["tokens"], name
            if want["type"] == 2:
                assert got["ll"] == want["ll"] and got["d"] == want["d"], name
        assert dr.render(blocks) == craft.verdict(raw)[0], name
    assert n_ok >= 15


def test_reader_refuses_a_stream_that_ends_early():
    z = raw_deflate(corpora()["fastq"][:5000], level=6)
    for cut in (1, 2, len(z) // 2, len(z) - 1):
        with pytest.raises(dr.DeflateError):
            dr.read(z[:cut])
    with pytest.raises(dr.DeflateError):
        dr.read(b"")


def test_a_64k_member_parses_in_about_a_second():
    import time
    z = raw_deflate(dt.no_repeat_text(dt.MEMBER), strategy=zlib.Z_HUFFMAN_ONLY)
    t0 = time.perf_counter()
    blocks = dr.read(z)
    assert time.perf_counter() - t0 < 2.0
    assert sum(len(b["tokens"]) for b in blocks) == dt.MEMBER


# ---- what the texts claim ---------------------------------------------------------------------------------------------------------------------
def test_de_bruijn_prefix_has_every_4_bytes_once():
    text = dt.no_repeat_text(dt.MEMBER)
    assert len(set(text)) == 16 and len({text[i:i + 4] for i in range(len(text) - 3)}) == 65277 and dt.repeats(text) == []
    assert len(raw_deflate(text, strategy=zlib.Z_HUFFMAN_ONLY)) == 31001
    for n in dt.NO_REPEAT_SIZES:  # the depth stays below 15: the unrestricted code is the best a writer can do
        hist = collections.Counter(dt.no_repeat_text(n))
        hist[256] = 1
        assert dt.huffman_cost(hist)[1] < 15


def test_noise_has_no_4_bytes_twice():
    for values, n in ((16, 4096), (64, 40000)):
        assert dt.repeats(dt.noise(n, values=values)) == []
    sep = dt.run_text(0, dt.RUN_SEPARATOR)
    assert dt.repeats(sep) == [] and dt.RUN_BYTE not in sep and len(sep) == dt.RUN_SEPARATOR
    assert dt.RUN_BYTE not in dt.PERM[:255]


def test_run_texts():
    for length in dt.RUN_LENGTHS + (dt.MEMBER,):
        for sep in (0, dt.RUN_SEPARATOR):
            text = dt.run_text(length, sep)[:dt.MEMBER]
            run = len(text) - sep
            assert text[sep:] == bytes([dt.RUN_BYTE]) * run and dt.repeats(text) == list(range(sep + 1, len(text) - 3))
    # the rule's token list is the text's: zlib's Z_RLE writes the same lengths for a run (its shortest match is 3, so from 4 up)
    for length in (5, 8, 257, 263, 518):
        tokens = dr.read(raw_deflate(dt.run_text(length), strategy=zlib.Z_RLE))[0]["tokens"]
        if (length - 1) % 258 >= 4 or (length - 1) % 258 == 0:
            dt.check_run_tokens(tokens, length)


def test_distance_texts():
    for d in dt.FAR_DISTANCES + dt.TOO_FAR_DISTANCES:
        text = dt.distance_text(d)
        assert len(text) == d + dt.COPY <= dt.MEMBER and text[:dt.COPY] == text[d:] and dt.repeats(text[:dt.COPY]) == []
        assert set(text[dt.COPY:d]) <= {dt.RUN_BYTE} and dt.RUN_BYTE not in text[:dt.COPY]
    for d in dt.NEAR_DISTANCES:
        text = dt.near_text(d)
        assert len(text) == dt.NEAR_LEAD + 4 * d and dt.repeats(text) == list(range(dt.NEAR_LEAD + d, len(text) - 3))
        assert text[dt.NEAR_LEAD:dt.NEAR_LEAD + d] * 4 == text[dt.NEAR_LEAD:]


def test_lazy_texts():
    for lane in dt.LAZY_LANES:
        text, q = dt.lazy_text(lane)
        assert q == 64 + lane and text[q:q + 4] == text[10:14] and text[q + 1:q + 24] == text[34:57]
        assert text[q + 4] != text[14] and text[q + 24] != text[57] and text[q - 1] != text[9] and text[33] != text[10]
        assert dt.repeats(text) == list(range(q, q + 21))
        assert dt.lookup_survives(text, 10, q) and (lane == 63 or dt.lookup_survives(text, 34, q + 1))


def test_symbols_text():
    text, plan = dt.symbols_text()
    assert len(text) <= dt.MEMBER and dt.repeats(text[:dt.SYMBOLS_NOISE]) == []
    assert {l for _, l, _, _ in plan} == set(dr.LEN_BASE[1:]) and {craft.distance_symbol(d)[0] for _, _, d, _ in plan} == set(range(30))
    planted = set()
    for pos, length, dist, exact in plan:
        assert text[pos:pos + length] == dr.render(list(text[:pos]) + [(length, dist)])[pos:]
        assert text[pos + length] != text[pos - dist + length]  # the copy ends where it was planted to end
        planted |= set(range(pos, pos + length - 3))
        if exact:
            assert dist >= 128 and pos - dist + length <= dt.SYMBOLS_NOISE and text[pos - 1] != text[pos - dist - 1]
            assert dt.lookup_survives(text, pos - dist, pos)
    assert set(dt.repeats(text)) == planted  # nothing repeats but the copies
    exact = [(l, d) for _, l, d, e in plan if e]
    assert {l for l, _ in exact} == set(dr.LEN_BASE[1:]) and max(d for _, d in exact) > 24577 and len(exact) >= 30


def test_bucket_is_the_kernels_hash():
    src = open(__file__.replace("tests/test_deflate_read_cpu.py", "merkurio_amd/csrc/codec/bgzf_deflate.hip")).read()
    assert "constexpr int kHashBits = %d;" % dt.HASH_BITS in src and "h = (w * 0x9E3779B1u) >> (32 - kHashBits);" in src
    assert dt.bucket(b"\x01\0\0\0") == 0x9E3779B1 >> 22


def test_stored_edge_sweep_lies_on_both_sides():
    """evenly drawn bytes over 200 .. 256 values never shrink at 64 .. 1024 bytes; the weighted draws of the sweep do and do not"""
    for values in (200, 256):
        for n in (64, 256, 1024):
            flat = bytes(dt.PERM[(k * 7919 + k // values) % values] for k in range(n))
            assert len(raw_deflate(flat, strategy=zlib.Z_HUFFMAN_ONLY)) == n + 5
    below = above = 0
    for n in dt.EDGE_SIZES:
        for values in dt.EDGE_VALUES:
            for seed in range(dt.EDGE_SEEDS):
                z = len(raw_deflate(dt.edge_noise(n, values, seed), strategy=zlib.Z_HUFFMAN_ONLY))
                assert z <= n + 5
                below += z < n + 5
                above += z == n + 5
    assert below >= 100 and above >= 100, (below, above)
    assert len(dt.edge_text(400)) == 400 * len(dt.EDGE_VALUES) * dt.EDGE_SEEDS


def test_mixed_members_and_the_period_text():
    kinds = collections.Counter()
    seen = set()
    for k in range(0, dt.MIXED_MEMBERS, 37):
        kind, text = dt.mixed_member(k)
        kinds[kind] += 1
        assert len(text) == dt.MIXED_BYTES and text not in seen
        seen.add(text)
        if kind == "a":
            assert dt.repeats(text) == []
        if kind == "b":
            assert dt.repeats(text) == list(range(dt.MIXED_SEPARATOR + 1, dt.MIXED_BYTES - 3))
    assert set(kinds) == set("abgn")
    text = dt.period_text()
    assert text[13:] == text[:-13] and len(set(text[:13])) == 13
