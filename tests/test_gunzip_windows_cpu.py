"""The host side of mk_gzip_stream_* (a gzip file of any size inflated on the device window by window) that needs no device: the
entries are declared, bound and exported and refuse NULL; mk_crc32_combine -- the fold of a member's CRC-32 across windows -- against
zlib.crc32; and zlib's own verdict on every file of tests/gunzip_windows_cases.py: what test_gpu_gunzip_windows.py expects of a file is
what zlib says about it."""
import ctypes as C
import os
import random
import re
import struct
import zlib

import gunzip_members_cases as gm
import gunzip_windows_cases as gw
from merkurio_amd import native as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mk_gzip_stream_begin", "mk_gzip_stream_next", "mk_gzip_stream_info", "mk_gzip_stream_end", "mk_crc32_combine"]


def test_the_entries_are_declared_bound_exported_and_refuse_null():
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"int mk_gzip_stream_begin\(mk_codec \*c, const uint8_t \*gz, uint64_t n, uint64_t window_bytes, uint32_t \*taken\);", hdr)
    assert re.search(r"int mk_gzip_stream_next\(mk_codec \*c, uint64_t \*text_bytes, uint32_t \*state\);", hdr)
    assert re.search(r"int mk_gzip_stream_info\(const mk_codec \*c, mk_gzip_stream_stats \*out\);", hdr)
    assert re.search(r"int mk_gzip_stream_end\(mk_codec \*c\);", hdr)
    assert re.search(r"uint32_t mk_crc32_combine\(uint32_t crc_a, uint32_t crc_b, uint64_t len_b\);", hdr)
    assert re.search(r"\}\s*mk_gzip_stream_stats\s*;", hdr)
    L = mk.load()
    for name in ENTRIES:
        assert name in mk.EXPORTS and hasattr(L, name), name
    assert hasattr(mk.Codec, "gunzip_stream")
    assert L.mk_abi_version() == 7
    taken, n, state, stats = C.c_uint32(7), C.c_uint64(7), C.c_uint32(7), mk.GzipStreamStats()
    blob = (C.c_uint8 * 32)()
    assert L.mk_gzip_stream_begin(None, blob, 32, 0, C.byref(taken)) == mk.MK_E_INVALID_ARG
    assert L.mk_gzip_stream_next(None, C.byref(n), C.byref(state)) == mk.MK_E_INVALID_ARG
    assert L.mk_gzip_stream_info(None, C.byref(stats)) == mk.MK_E_INVALID_ARG
    assert L.mk_gzip_stream_end(None) == mk.MK_E_INVALID_ARG
    # the stats struct as the header lays it out: seven 64-bit counters, five floats, one reserved word
    fields = re.search(r"typedef struct mk_gzip_stream_stats \{(.*?)\}", hdr, re.S).group(1)
    assert len(re.findall(r"uint64_t \w+;", fields)) == 7 and "float ms[5];" in fields
    assert C.sizeof(mk.GzipStreamStats) == 7 * 8 + 5 * 4 + 4


def test_crc32_combine_on_random_splits():
    L = mk.load()
    rnd = random.Random(1)
    for k in range(60):
        data = rnd.randbytes(rnd.choice((0, 1, 2, 7, 255, 4096, 65280, 65281, 200_000)))
        cut = rnd.randrange(len(data) + 1)
        a, b = data[:cut], data[cut:]
        assert L.mk_crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), (k, len(data), cut)
    # a fold over many windows, as the stream runs it
    data = rnd.randbytes(300_000)
    crc, at = 0, 0
    while at < len(data):
        step = rnd.randrange(1, 40_000)
        crc = L.mk_crc32_combine(crc, zlib.crc32(data[at:at + step]), len(data[at:at + step]))
        at += step
    assert crc == zlib.crc32(data)


def test_crc32_combine_with_a_second_part_of_no_and_of_one_byte():
    L = mk.load()
    a = b"the first part\n" * 9
    assert L.mk_crc32_combine(zlib.crc32(a), zlib.crc32(b""), 0) == zlib.crc32(a)
    assert L.mk_crc32_combine(zlib.crc32(a), 0, 0) == zlib.crc32(a)
    for b in (b"\0", b"\n", b"\xff"):
        assert L.mk_crc32_combine(zlib.crc32(a), zlib.crc32(b), 1) == zlib.crc32(a + b)
    assert L.mk_crc32_combine(0, zlib.crc32(a), len(a)) == zlib.crc32(a)


def test_crc32_combine_over_more_than_4_gib_and_isize_modulo_2_32():
    """|B| = 2^32 + 5 zero bytes: the length is a 64-bit one, zlib.crc32 is fed in chunks.  The same length against ISIZE: what RFC 1952
    stores is the length modulo 2^32, which is what the stream compares"""
    L = mk.load()
    a = b"text in front of 4 GiB and five bytes of zeros\n"
    n = (1 << 32) + 5
    zeros = bytes(64 << 20)
    crc_b, crc_ab, left = 0, zlib.crc32(a), n
    while left:
        piece = zeros if left >= len(zeros) else zeros[:left]
        crc_b, crc_ab, left = zlib.crc32(piece, crc_b), zlib.crc32(piece, crc_ab), left - len(piece)
    assert L.mk_crc32_combine(zlib.crc32(a), crc_b, n) == crc_ab
    assert L.mk_crc32_combine(zlib.crc32(a), crc_b, 5) != crc_ab  # (a length cut to 32 bits folds another CRC)
    isize = struct.unpack("<I", struct.pack("<Q", len(a) + n)[:4])[0]
    assert isize == (len(a) + n) % (1 << 32) == len(a) + 5 and isize != len(a) + n


def test_what_the_gpu_tests_expect_is_what_zlib_says():
    """every file of gunzip_windows_cases.py: "taken" files are files zlib reads to their end, "handed-back" files are files zlib
    refuses; and zlib_prefix agrees with gunzip_members_cases.zlib_walk on every file of both modules"""
    verdicts = gw.verdicts()
    for name, (blob, expect) in gw.files().items():
        text, ok, members = verdicts[name]
        assert ok == (expect == "taken"), name
        assert (gm.zlib_walk(blob)[0] is not None) == ok, name
        if ok:
            assert gm.zlib_walk(blob) == (text, members), name
    for name, blob, expect in gm.cases():
        text, ok, members = verdicts[name]
        walked = gm.zlib_walk(blob)
        assert ok == (walked[0] is not None), name
        if ok:
            assert walked == (text, members), name
        if expect != "either":
            assert ok == (expect == "taken"), name
    f = gw.files()
    assert len(f["fastq-one-member-2mb"][0]) >= 6 * gw.WINDOWS[2]
    assert f["fastq-one-member-2mb"][0].startswith(f["fastq-one-member-quarter"][0][:10])
    # the damaged file: zlib hands out a prefix of the whole file's text, and stops inside window 3 of 8 or behind it
    whole = verdicts["fastq-one-member-2mb"][0]
    part = verdicts["bit-flipped-in-window-3-of-8"][0]
    assert 0 < len(part) < len(whole)
    for name in ("last-crc-wrong", "last-isize-wrong", "bytes-behind-the-last-member"):
        assert verdicts[name][0] == whole, name
    # the match of 32 000 reaches in front of the member's first byte (28 000 bytes of text lie in front of it), the one of 27 000 does not
    assert len(verdicts["match-reaches-in-front-of-a-continued-member"][0]) == 28000
    assert len(verdicts["match-reaches-the-members-early-text"][0]) == 28041


def test_the_sync_flushed_stream_has_dynamic_blocks():
    """Z_SYNC_FLUSH every 3 KiB of text: every block behind a flush marker (an empty stored block, 00 00 ff ff, byte-aligned) is a
    dynamic one (BTYPE = 2) -- the kind the block-start search finds; it passes over fixed-code blocks"""
    blob, _ = gw.files()["sync-flush-every-3k"]
    assert gw.SYNC_FLUSH_EVERY == 3072
    marks = [m.end() for m in re.finditer(rb"\x00\x00\xff\xff", blob[10:-8])]
    text = gw.verdicts()["sync-flush-every-3k"][0]
    assert len(marks) >= len(text) // gw.SYNC_FLUSH_EVERY
    dynamic = sum((blob[10 + at] >> 1) & 3 == 2 for at in marks if 10 + at < len(blob) - 8)
    assert dynamic >= 0.95 * len(marks), (dynamic, len(marks))  # (the marker's four bytes can occur inside a block too)
    # and a start of such a block every 4 KiB chunk at least: pieces shorter than 32 KiB of text
    assert len(blob) / len(marks) < 2048
