"""mk_bzip2_stream_*: a .bz2 file decoded on the device window by window -- the compressed bytes go up a window at a time, the cut is
the window's last magic, an end magic is consumed only with what decides the bytes behind it, the open stream's CRC is folded across
windows, a window's text arrives as one or several text windows in two buffers.  The checker is libbz2 through Python's bz2; the
files are those of bzip2_cases.py and bzip2_craft.py (test_bunzip2_windows_cpu.py runs the same window logic on the host at every
window size).  One codec per test."""
import bz2
import ctypes as C
import functools
import random

import numpy as np
import pytest

import bzip2_cases as cases
import bzip2_craft as craft
from merkurio_amd import native as mk

pytestmark = pytest.mark.gpu


@pytest.fixture()
def codec():
    c = mk.Codec()
    yield c
    c.close()


def four_block_stream():
    text = random.Random(31).randbytes(330000)
    return bz2.compress(text, 1), text


def six_block_file():
    text = cases.fastq(4000, seed=3)[:560000]
    blob = bz2.compress(text, 1)
    magics = cases.find_magics(blob)
    assert [k for _, k in magics] == [0] * 6 + [1]
    return blob, text, magics


def libbz2_prefix(blob):
    """what a BZ2Decompressor returns, fed byte by byte from the front and stream behind stream, before it raises (or the data ends):
    the call that raises returns nothing, so it is given one byte"""
    out, data = [], blob
    while data:
        d = bz2.BZ2Decompressor()
        try:
            for at in range(len(data)):
                out.append(d.decompress(data[at:at + 1]))
                if d.eof:
                    break
        except (OSError, ValueError, EOFError):
            break
        if not d.eof:
            break
        data = d.unused_data
    return b"".join(out)


def stream(codec, blob, window):
    """-> (the text windows, the state the stream ended in, its stats)"""
    parts = list(codec.bunzip2_stream(blob, window))
    stats = codec.stream_stats
    if stats is not None:
        assert stats["text_bytes"] == sum(len(p) for p in parts) and stats["windows"] == len(parts), stats
    return parts, codec.stream_state, stats


def exact(codec, blob, text, window):
    parts, state, stats = stream(codec, blob, window)
    assert state == 1 and b"".join(parts) == text and stats["consumed_bytes"] == len(blob), (window, state, stats)
    return parts, stats


VALID = sorted(cases.valid()) + ["four-random-blocks"]


def _file(name):
    return four_block_stream() if name == "four-random-blocks" else cases.valid()[name]


@pytest.mark.parametrize("name", VALID)
def test_a_third_and_a_seventh_of_the_file_per_window(codec, name):
    blob, text = _file(name)
    assert bz2.decompress(blob) == text
    for window in (max(1, len(blob) // 3), len(blob) // 7 + 1):
        exact(codec, blob, text, window)


@functools.lru_cache(maxsize=None)
def magics_of(name):
    """[(bit, kind)] as cases.find_magics gives them, by a byte search in the file shifted left by 0 .. 7 bits"""
    blob = _file(name)[0]
    whole, out = int.from_bytes(blob, "big"), []
    for r in range(8):
        shifted = ((whole << r) & ((1 << 8 * len(blob)) - 1)).to_bytes(len(blob), "big")
        for kind, magic in enumerate((cases.BLOCK_MAGIC, cases.END_MAGIC)):
            at = shifted.find(magic.to_bytes(6, "big"))
            while at >= 0:
                if at * 8 + r + 48 <= len(blob) * 8:
                    out.append((at * 8 + r, kind))
                at = shifted.find(magic.to_bytes(6, "big"), at + 1)
    return sorted(out)


def seam_of(name):
    """the magic the sixteen windows walk over: a file's first BLOCK magic behind its first block that starts inside a byte, where
    it has one (a stream of several blocks); else its second magic (an end magic, in the files of several streams with another stream
    behind it); else its only one"""
    magics = magics_of(name)
    inner = [(bit, kind) for bit, kind in magics[1:] if kind == 0 and bit & 7]
    return inner[0] if inner else magics[1] if len(magics) > 1 else magics[0]


# every block magic behind the first of the two four-block streams: six seams, all inside a byte
BLOCK_SEAMS = [(name, k) for name in ("four-blocks-l1", "four-random-blocks") for k in (1, 2, 3)]


def test_the_seams_are_what_they_are_meant_to_be():
    assert magics_of("golden-sample") == cases.find_magics(_file("golden-sample")[0])
    assert magics_of("rle-l1") == cases.find_magics(_file("rle-l1")[0])
    assert [k for _, k in magics_of("four-random-blocks")] == [k for _, k in magics_of("four-blocks-l1")] == [0, 0, 0, 0, 1]
    for name in ("four-random-blocks", "four-blocks-l1", "fastq-l1", "rle-l1"):  # a block magic inside a byte
        bit, kind = seam_of(name)
        assert kind == 0 and bit & 7 and bit > 32, (name, bit, kind)
    for name in ("two-streams", "three-streams", "streams-with-an-empty-one"):  # an end magic inside a byte, a stream behind it
        bit, kind = seam_of(name)
        assert kind == 1 and bit & 7 and (bit + 80 + 7) // 8 + 14 < len(_file(name)[0]), (name, bit, kind)
    phases = [magics_of(name)[k][0] & 7 for name, k in BLOCK_SEAMS]
    assert all(phases) and len(set(phases)) >= 4 and all(magics_of(name)[k][1] == 0 for name, k in BLOCK_SEAMS), phases


def walk_over(codec, blob, text, bit):
    """sixteen windows: the first upload (it starts at byte 4) ends 4 bytes in front of the first byte of the magic at `bit`, inside its
    6 or 7 bytes, and up to 11 bytes behind that first byte.  While the magic does not lie whole inside the upload the block in front
    of it is not decoded: the cut falls one magic earlier, or the window grows"""
    first = max(1, bit // 8 - 4 - 4)
    for window in range(first, first + 16):
        parts, _ = exact(codec, blob, text, window)
    return parts


@pytest.mark.parametrize("name", VALID)
def test_sixteen_window_sizes_around_a_seam(codec, name):
    """the first upload's end walks byte by byte over a magic of the file: a block magic that starts inside a byte wherever the file has
    one, else an end magic (seam_of)"""
    blob, text = _file(name)
    walk_over(codec, blob, text, seam_of(name)[0])


@pytest.mark.parametrize("name,k", BLOCK_SEAMS)
def test_sixteen_window_sizes_around_every_block_magic(codec, name, k):
    """... and over each block magic of the four-block streams, at bit phases 1, 2, 3, 5 and 7 of a byte"""
    blob, text = _file(name)
    bit, kind = magics_of(name)[k]
    assert kind == 0 and bit & 7
    walk_over(codec, blob, text, bit)


def test_a_window_smaller_than_a_block_grows(codec):
    blob, text = four_block_stream()
    parts, stats = exact(codec, blob, text, 4096)
    assert stats["windows_grown"] > 0 and stats["blocks"] == 4 and stats["streams"] == 1, stats


def test_window_w_is_still_there_after_window_w_plus_1(codec):
    """read through the pointer of mk_gzip_text_device with a device-to-host copy of this test's own"""
    blob, text = four_block_stream()
    L = codec._L
    src = np.frombuffer(blob, dtype=np.uint8)
    taken, n, state = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    assert L.mk_bzip2_stream_begin(codec._h, src.ctypes.data, src.size, len(blob) // 4, C.byref(taken)) == 0 and taken.value == 1
    # (the HIP runtime the library itself runs on: the one this process has mapped)
    with open("/proc/self/maps") as maps:
        hip = C.CDLL(next(ln.split()[-1] for ln in maps if "libamdhip64" in ln))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def copy_out(ptr, size):
        out = np.empty(size, dtype=np.uint8)
        assert hip.hipMemcpy(out.ctypes.data, ptr, size, 2) == 0 and hip.hipDeviceSynchronize() == 0  # (2 = device to host)
        return out.tobytes()
    held, at, checked = [], 0, 0
    try:
        while True:
            assert L.mk_bzip2_stream_next(codec._h, C.byref(n), C.byref(state)) == 0
            if state.value != 0:
                break
            ptr = L.mk_gzip_text_device(codec._h, None)
            if held:  # the window before this one, after this one was produced
                p_ptr, p_at, p_n = held[-1]
                assert p_ptr != ptr and copy_out(p_ptr, p_n) == text[p_at:p_at + p_n]
                checked += 1
            held.append((ptr, at, n.value))
            at += n.value
    finally:
        assert L.mk_bzip2_stream_end(codec._h) == 0
    assert state.value == 1 and at == len(text) and checked >= 2


def test_a_small_text_cap_gives_several_text_windows(codec):
    """600 KB of zeros and 200 KB of random bytes at level 1: three blocks in one window, the first of 688 KB of text"""
    text = bytes(600000) + random.Random(2).randbytes(200000)
    blob = bz2.compress(text, 1)
    whole, _ = exact(codec, blob, text, len(blob) + 1)
    assert len(whole) == 1
    codec.set_bzip2_text_cap(65536)
    parts, stats = exact(codec, blob, text, len(blob) + 1)
    assert len(parts) == 3 and stats["blocks"] == 3, [len(p) for p in parts]
    codec.set_bzip2_text_cap(0)
    codec.set_bzip2_pass_blocks(1)  # (and the pass hook applies to a window's passes)
    exact(codec, blob, text, len(blob) + 1)


def test_device_memory_is_bounded_by_the_window_not_the_file(codec):
    one = bz2.compress(cases.fastq(300, seed=4)[:40000], 1)
    text = bz2.decompress(one)
    window = 2 * len(one) + 64
    _, short = exact(codec, one * 8, text * 8, window)
    _, long = exact(codec, one * 64, text * 64, window)
    print(short, long)
    assert long["windows"] > 3 * short["windows"] and long["streams"] == 64
    assert 0 < long["peak_device_bytes"] <= short["peak_device_bytes"], (short, long)


def test_a_flipped_bit_in_the_last_block(codec):
    """six blocks, windows of two: the windows in front of the damage are delivered whole, and of the damaged window the whole block
    in front of the damaged one -- libbz2 has written it by then.  Exactly the text of blocks 0 .. 4"""
    blob, text, magics = six_block_file()
    window = (magics[2][0] - magics[0][0]) // 8 + 16  # two blocks
    good, _ = exact(codec, blob, text, window)
    codec.set_bzip2_text_cap(1)  # (a block per text window: the blocks' text lengths)
    blocks, _ = exact(codec, blob, text, len(blob) + 1)
    codec.set_bzip2_text_cap(0)
    assert len(blocks) == 6
    five = sum(len(p) for p in blocks[:5])
    assert sum(len(p) for p in good[:2]) < five  # (the first whole windows, and more)
    bad = cases.flip(blob, (magics[5][0] + magics[6][0]) // 2)
    parts, state, stats = stream(codec, bad, window)
    assert state == 2 and b"".join(parts) == text[:five] and stats["blocks"] == 5, (stats, [len(p) for p in parts])
    assert parts[:2] == good[:2]


def test_a_wrong_stream_crc_is_found_after_all_the_text(codec):
    blob, text, magics = six_block_file()
    bad = cases.flip(blob, magics[6][0] + 48 + 3)
    for window in (len(blob) // 3, len(blob) + 1):
        parts, state, stats = stream(codec, bad, window)
        assert state == 2 and b"".join(parts) == text and stats["streams"] == 0, (window, stats)
    parts, state, stats = stream(codec, blob + b"\x00\x01\x02\x03", len(blob) // 3)  # (and four bytes behind the stream likewise)
    assert state == 2 and b"".join(parts) == text, stats


def test_the_bad_catalogue_at_a_small_window(codec):
    """the verdict is libbz2's: state 2, and what was delivered in front of it is a prefix of libbz2's text"""
    bad = sorted(n for n in craft.CASES if n.startswith("bad-"))
    assert len(bad) >= 10
    for name in bad:
        blob = craft.CASES[name][0]
        assert craft.libbz2_says(blob) is None
        parts, state, stats = stream(codec, blob, 64)
        assert state == 2, (name, stats)
        assert libbz2_prefix(blob).startswith(b"".join(parts)), name
    two_blocks = cases.two_block_file()[1]
    for name, blob in cases.damaged().items():
        parts, state, stats = stream(codec, blob, 4096)
        assert state == 2, (name, stats)
        assert name.startswith("patched") and not parts or two_blocks.startswith(b"".join(parts)), name


def test_guards(codec):
    blob, text = cases.valid()["fastq-l1"]
    L, h = codec._L, codec._h
    src = np.frombuffer(blob, dtype=np.uint8)
    gz = np.frombuffer(__import__("gzip").compress(b"ACGT\n" * 4000), dtype=np.uint8)
    taken, n, state, blocks = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    INVALID = mk.MK_E_INVALID_ARG
    assert L.mk_bzip2_stream_next(h, C.byref(n), C.byref(state)) == INVALID  # no stream
    assert L.mk_bzip2_stream_begin(h, src.ctypes.data, src.size, 8192, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_bzip2_inflate_device(h, src.ctypes.data, src.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken)) == INVALID
    assert L.mk_gzip_members_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_stream_begin(h, gz.ctypes.data, gz.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_bzip2_stream_begin(h, src.ctypes.data, src.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_bzip2_stream_next(h, C.byref(n), C.byref(state)) == 0 and state.value == 0 and n.value > 0  # the stream is untouched by them
    assert L.mk_bzip2_stream_end(h) == 0
    assert codec.bunzip2(blob)[:2] == (True, text)  # after _end the one-shot call works
    # the reverse: a gzip stream open
    assert L.mk_gzip_stream_begin(h, gz.ctypes.data, gz.size, 8192, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_bzip2_stream_begin(h, src.ctypes.data, src.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_bzip2_inflate_device(h, src.ctypes.data, src.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_stream_end(h) == 0
    # mk_gzip_text_release ends a bzip2 stream as _end does
    assert L.mk_bzip2_stream_begin(h, src.ctypes.data, src.size, 8192, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_gzip_text_release(h) == 0
    assert L.mk_bzip2_stream_next(h, C.byref(n), C.byref(state)) == INVALID
    # no "BZh1-9" in front: not taken, and the handle lives on
    for junk in (b"", b"BZ", b"BZh0" + blob[4:], b"not a bzip2 file\n" * 9, bytes(gz)):
        assert list(codec.bunzip2_stream(junk, 4096)) == [] and codec.stream_state == 2 and codec.stream_stats is None
    assert b"".join(codec.bunzip2_stream(blob, 8192)) == text and codec.stream_state == 1
