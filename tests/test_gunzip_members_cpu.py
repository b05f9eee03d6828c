"""mk_gzip_member_guesses (host code, no device): where RFC 1952 headers parse in a file of gzip members -- the guesses that
mk_gzip_members_inflate_device proves or drops on the device (test_gpu_gunzip_members.py).  And zlib's own verdict on every file
of tests/gunzip_members_cases.py: what the GPU tests expect of a file is what zlib says about it."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as craft
import gunzip_members_cases as gm
from merkurio_amd import native as mk


def guesses(blob):
    return [(int(g["header_off"]), int(g["data_off"]), int(g["crc"]), int(g["isize"])) for g in mk.gzip_member_guesses(blob)]


def expected(members, texts, header_bytes=None):
    """the table of a file that is `members` back to back, with headers of header_bytes[k] (10 where not given)"""
    out, at = [], 0
    for k, (m, t) in enumerate(zip(members, texts)):
        out.append((at, at + (header_bytes[k] if header_bytes else 10), zlib.crc32(t), len(t)))
        at += len(m)
    return out


@pytest.mark.parametrize("n", [1, 2, 5])
def test_offsets_and_trailer_fields_of_one_two_and_five_members(n):
    texts = [gm.fastq(20 + k, 300 + k) for k in range(n)]
    members = [gm.member(t, (1, 6, 9)[k % 3]) for k, t in enumerate(texts)]
    assert guesses(b"".join(members)) == expected(members, texts)


def test_optional_header_fields_are_walked():
    texts = [gm.fastq(10, 1), gm.fastq(11, 2), b"third\n", gm.fastq(5, 3)]
    headers = [dict(fextra=b"AB\x03\x00xyz", fname=b"reads.fastq", fcomment=b"a comment", fhcrc=True), dict(fname=b"n"), dict(fextra=b"", fhcrc=True), dict(fcomment=b"")]
    members = [gm.member(t, **h) for t, h in zip(texts, headers)]
    sizes = [10 + 2 + 7 + 12 + 10 + 2, 10 + 2, 10 + 2 + 2, 10 + 1]
    assert guesses(b"".join(members)) == expected(members, texts, sizes)
    # the name of a file that looks like a header is part of the header in front of it, and a guess all the same
    inner = gm.member(b"x", fname=b"\x1f\x8b\x08\x01" + bytes(range(1, 20)))
    got = guesses(inner + members[1])
    assert [g[0] for g in got] == [0, 10, len(inner)] and got[0][1] == 10 + 4 + 19 + 1


@pytest.mark.parametrize("place", ["first", "middle", "last"])
def test_an_empty_member_is_found(place):
    a, b = gm.fastq(30, 4), gm.fastq(31, 5)
    members, texts = [gm.member(a), gm.member(b, 1)], [a, b]
    k = {"first": 0, "middle": 1, "last": 2}[place]
    members.insert(k, gm.EMPTY), texts.insert(k, b"")
    assert zlib.decompress(gm.EMPTY, 31) == b""
    assert guesses(b"".join(members)) == expected(members, texts)


def test_a_file_that_does_not_start_with_a_header_has_no_guesses():
    m = gm.member(gm.fastq(10, 6))
    for blob in (b"", b"\x1f", b"x" + m, m[1:], b"\x1f\x8b\x07" + m[3:], b"plain text\n" * 30 + m, bytes(40)):
        assert guesses(blob) == [], blob[:12]


def test_reserved_flag_bits_are_refused():
    t = gm.fastq(10, 7)
    m = gm.member(t)
    for bit in (0x20, 0x40, 0x80):
        bad = m[:3] + bytes([bit]) + m[4:]
        assert guesses(bad + m) == []                                  # the file's first header
        assert guesses(m + bad) == [(0, 10, zlib.crc32(t), len(t))]    # a later one: the bytes are the first member's to explain
    assert len(guesses(m + m)) == 2


def test_a_header_cut_off_by_the_files_end_is_no_guess():
    t = gm.fastq(10, 8)
    m = gm.member(t)
    tail = gm.member(b"second\n", fextra=b"AB\x02\x00xy", fname=b"name", fhcrc=True)
    head = tail.index(b"name\0") + 5 + 2
    two = len(guesses(m + tail))
    assert two == 2
    for cut in range(1, head + 2 + 8):  # magic alone, FEXTRA's length, inside the name, no room for 2 bytes of stream and a trailer
        got = guesses(m + tail[:cut])
        assert [g[0] for g in got] == [0], cut
        assert got[0][2:] == struct.unpack("<II", (m + tail[:cut])[-8:])  # (the last guess's trailer is read at the file's end)
    assert len(guesses(m + tail[:head + 2 + 8])) == 2
    assert guesses(m[:19]) == [] and len(guesses(gm.EMPTY)) == 1


def test_magic_bytes_inside_a_payload_are_reported():
    """the walker guesses, the device proves: a header that parses inside a stored block is in the table, with the 8 bytes in front of
    it as the trailer of the guess before"""
    t = gm.fastq(10, 9)
    plant = b"\x1f\x8b\x08\x00\0\0\0\0\0\x03"
    text = t[:400] + plant + t[400:]
    m, second = gm.stored_member(text), gm.member(b"second\n")
    at = 10 + 5 + 400
    got = guesses(m + second)
    assert [g[:2] for g in got] == [(0, 10), (at, at + 10), (len(m), len(m) + 10)]
    assert got[0][2:] == struct.unpack("<II", text[392:400]) and got[1][2:] == (zlib.crc32(text), len(text))
    whole = gm.member(t[:300])  # a whole member as text
    got = guesses(gm.stored_member(whole) + second)
    assert [g[0] for g in got] == [0, 15, 15 + len(whole) + 8]


def test_a_table_one_short_gets_the_true_count_and_no_write_past_it():
    texts = [gm.fastq(5, 20 + k) for k in range(5)]
    blob = b"".join(gm.member(t) for t in texts)
    L = mk.load()
    buf = np.frombuffer(blob, dtype=np.uint8)
    full = mk.gzip_member_guesses(blob)
    assert len(full) == 5
    for cap in (4, 1, 0):
        raw = np.full(6 * mk.GUESS_DTYPE.itemsize, 0xAB, dtype=np.uint8)
        n = C.c_uint64(0)
        assert L.mk_gzip_member_guesses(buf.ctypes.data, buf.size, raw.ctypes.data, cap, C.byref(n)) == 0
        assert n.value == 5
        item = mk.GUESS_DTYPE.itemsize
        assert raw[:cap * item].tobytes() == full[:cap].tobytes()
        assert (raw[cap * item:] == 0xAB).all()
    assert L.mk_gzip_member_guesses(buf.ctypes.data, buf.size, None, 0, None) == mk.MK_E_INVALID_ARG
    assert mk.GUESS_DTYPE.itemsize == 24


def test_what_the_gpu_tests_expect_is_what_zlib_says():
    """every file of gunzip_members_cases.py: "taken" files are files zlib reads (and the walker finds at least zlib's members in them:
    no member start is missed), "handed-back" files are files zlib refuses"""
    for name, blob, expect in gm.cases():
        text, members = gm.zlib_walk(blob)
        table = guesses(blob)
        if expect == "handed-back":
            assert text is None, name
            continue
        assert text is not None and members >= 2, name
        starts, at, data = [], 0, blob
        while data:
            d = zlib.decompressobj(31)
            d.decompress(data)
            starts.append(at)
            at, data = at + len(data) - len(d.unused_data), d.unused_data
        assert set(starts) <= {g[0] for g in table}, name
        if name.startswith("false-guess"):
            assert len(table) > members, name
    assert sum(e == "taken" for _, _, e in gm.cases()) >= 30
    planted = [blob for name, blob, _ in gm.cases() if name == "false-guess-magic-bytes-end-a-payload"][0]
    at = guesses(planted)[1][0]  # the three bytes in front of the first member's trailer
    assert planted[at:at + 3] == b"\x1f\x8b\x08" and at + 3 + 8 == guesses(planted)[2][0]
