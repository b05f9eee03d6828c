"""What the four streams of the codec share (codec_stream.hpp): the two text windows that take turns, the figures that outlive the
stream, one stream per handle whatever its format, mk_gzip_text_release ending whichever is open, and a handle that goes on after a
stream left in mid-file.  One FASTQ text of about 330 KB in four files, each cut so that its stream delivers three windows or more
(then both text buffers have been written and the first one used again); the text itself is what must come back, and zlib, libbz2,
libzstd and liblzma agree that the files hold it."""
import bz2
import ctypes as C
import gzip
import lzma
import random
import zlib

import numpy as np
import pytest

import xz_cases
import xz_craft
import zstd_cases
from merkurio_amd.native import MK_E_INVALID_ARG, MK_OK

pytestmark = pytest.mark.gpu

FORMATS = ("gzip", "bzip2", "zstd", "xz")
XZ_BLOCK = 40000


def _fastq(n, seed):
    rnd = random.Random(seed)
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(rnd.choices(b"ACGT", k=100)), bytes(rnd.choices(b"FFFF:,#", k=100))) for i in range(n))


TEXT = _fastq(1600, 11)


class Format:
    """a file of TEXT, how its stream is opened (window bytes, text cap) and the names of its calls"""

    def __init__(self, name, blob, window, cap, stats, one_shots):
        self.name, self.blob, self.window, self.cap, self.stats, self.one_shots = name, blob, window, cap, stats, one_shots
        self.src = np.frombuffer(blob, dtype=np.uint8)

    def call(self, codec, entry, *args):
        return getattr(codec._L, "mk_%s_stream_%s" % (self.name, entry))(codec._h, *args)

    def generator(self, codec):
        method = {"gzip": codec.gunzip_stream, "bzip2": codec.bunzip2_stream, "zstd": codec.unzstd_stream, "xz": codec.unxz_stream}[self.name]
        return method(self.blob, self.window, self.cap) if self.cap is not None else method(self.blob, self.window)

    def begin(self, codec, taken):
        set_cap = getattr(codec._L, "mk_codec_set_%s_text_cap" % self.name) if self.cap is not None else None
        if set_cap:
            assert set_cap(codec._h, self.cap) == MK_OK
        rc = self.call(codec, "begin", self.src.ctypes.data, self.src.size, self.window, C.byref(taken))
        if set_cap:
            assert set_cap(codec._h, 0) == MK_OK  # (the stream took it when it began)
        return rc

    def info(self, codec):
        st = self.stats()
        assert self.call(codec, "info", C.byref(st)) == MK_OK
        return bytes(st)

    def one_shot(self, codec, entry, text_bytes, taken):
        extra = () if entry == "mk_gzip_inflate_device" else (C.byref(C.c_uint64(0)),)
        return getattr(codec._L, entry)(codec._h, self.src.ctypes.data, self.src.size, C.byref(text_bytes), C.byref(taken), *extra)


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def formats(mk):
    assert 300 << 10 <= len(TEXT) <= 400 << 10
    gz = gzip.compress(TEXT, 6)
    bz = bz2.compress(TEXT, 1)  # blocks of 100 kB of text: four of them
    zs = zstd_cases.compress(TEXT, checksum=True, pieces=[TEXT[k:k + (64 << 10)] for k in range(0, len(TEXT), 64 << 10)])  # a block per piece
    xz = xz_craft.stream([xz_cases.real_block(TEXT[k:k + XZ_BLOCK], 4) for k in range(0, len(TEXT), XZ_BLOCK)], 4)[0]
    assert zlib.decompress(gz, 31) == bz2.decompress(bz) == zstd_cases.libzstd_says(zs) == lzma.decompress(xz) == TEXT
    # gzip: 32 KiB of the file per window.  bzip2: 40 000 bytes, which hold one whole block.  zstd: a block per window.  xz: no bound on
    # the compressed span, two blocks of text per window
    return {"gzip": Format("gzip", gz, 32768, None, mk.GzipStreamStats, ("mk_gzip_inflate_device", "mk_gzip_members_inflate_device")),
            "bzip2": Format("bzip2", bz, 40000, None, mk.Bzip2StreamStats, ("mk_bzip2_inflate_device",)),
            "zstd": Format("zstd", zs, 1, 0, mk.ZstdStreamStats, ("mk_zstd_inflate_device",)),
            "xz": Format("xz", xz, 0, 2 * XZ_BLOCK, mk.XzStreamStats, ("mk_xz_inflate_device",))}


def new_codec(mk):
    c = mk.Codec(0)
    c.set_xz_spread(1)  # (the default asks for a hundred blocks and more; the xz file here has nine)
    return c


@pytest.fixture
def codec(mk):
    c = new_codec(mk)
    yield c
    c.close()


def next_window(codec, fmt):
    """one call of _next -> (state, the window's text read back, where it lies on the device)"""
    n, state, m = C.c_uint64(0), C.c_uint32(7), C.c_uint64(0)
    assert fmt.call(codec, "next", C.byref(n), C.byref(state)) == MK_OK
    if state.value != 0:
        assert n.value == 0
        return state.value, b"", None
    ptr = codec._L.mk_gzip_text_device(codec._h, C.byref(m))
    out = np.empty(n.value, dtype=np.uint8)
    assert m.value == n.value and codec._L.mk_gzip_text_read(codec._h, 0, out.ctypes.data if out.size else None, out.size) == MK_OK
    return 0, out.tobytes(), ptr


def one_shot_text(codec, fmt):
    got = {"gzip": codec.gunzip, "bzip2": codec.bunzip2, "zstd": codec.unzstd, "xz": codec.unxz}[fmt.name](fmt.blob)
    return got if fmt.name == "gzip" else (got[1] if got[0] else None)


@pytest.mark.parametrize("name", FORMATS)
def test_windows_alternate_and_join(codec, formats, name):
    fmt = formats[name]
    parts = list(fmt.generator(codec))
    print(name, [len(p) for p in parts], codec.stream_stats)
    assert len(parts) >= 3 and all(parts), [len(p) for p in parts]
    assert b"".join(parts) == TEXT and codec.stream_state == 1
    assert codec.stream_stats["windows"] == len(parts) and codec.stream_stats["text_bytes"] == len(TEXT)
    # and window by window through the C calls: a window never lies where the one before it does
    taken = C.c_uint32(0)
    assert fmt.begin(codec, taken) == MK_OK and taken.value == 1
    state, at, before, windows = 0, 0, None, 0
    while True:
        state, text, ptr = next_window(codec, fmt)
        if state != 0:
            break
        assert text == TEXT[at:at + len(text)] and ptr and ptr != before, (windows, at)
        at, before, windows = at + len(text), ptr, windows + 1
    assert fmt.call(codec, "end") == MK_OK
    assert state == 1 and at == len(TEXT) and windows == len(parts)


@pytest.mark.parametrize("name", FORMATS)
def test_info_survives_end(mk, codec, formats, name):
    fmt = formats[name]
    zeros = bytes(C.sizeof(fmt.stats))
    assert fmt.info(codec) == zeros, "a fresh handle"
    taken = C.c_uint32(0)
    assert fmt.begin(codec, taken) == MK_OK and taken.value == 1
    windows = 0
    while True:
        state, _, _ = next_window(codec, fmt)
        if state != 0:
            break
        windows += 1
    assert state == 1 and windows >= 3
    last = fmt.info(codec)
    st = fmt.stats.from_buffer_copy(last)
    assert st.windows == windows and st.text_bytes == len(TEXT) and st.peak_device_bytes > 0
    assert fmt.call(codec, "end") == MK_OK
    assert fmt.info(codec) == last, "mk_%s_stream_info behind _end: the last stream's figures" % name
    for other in FORMATS:  # the other formats' figures are their own: no stream of theirs has run on this handle
        if other != name:
            assert formats[other].info(codec) == bytes(C.sizeof(formats[other].stats)), other


@pytest.mark.parametrize("name", FORMATS)
def test_exclusion_is_format_blind(mk, codec, formats, name):
    fmt = formats[name]
    L = codec._L
    taken = C.c_uint32(0)
    assert fmt.begin(codec, taken) == MK_OK and taken.value == 1
    state, first, _ = next_window(codec, fmt)
    assert state == 0 and first and TEXT.startswith(first)
    for other in FORMATS:
        o = formats[other]
        taken = C.c_uint32(77)
        assert o.begin(codec, taken) == MK_E_INVALID_ARG and b"open stream" in L.mk_last_error() and taken.value == 0, other
        assert L.mk_last_error().startswith(b"mk_%s_stream_begin: " % other.encode())
        for entry in o.one_shots:
            text_bytes, taken = C.c_uint64(77), C.c_uint32(77)
            assert o.one_shot(codec, entry, text_bytes, taken) == MK_E_INVALID_ARG and b"open stream" in L.mk_last_error(), entry
            assert L.mk_last_error().startswith(entry.encode() + b": ") and (text_bytes.value, taken.value) == (0, 0), entry
    # the open stream has not noticed
    at = len(first)
    state, text, _ = next_window(codec, fmt)
    assert state == 0 and text and text == TEXT[at:at + len(text)]
    rest = [text]
    while state == 0:
        state, text, _ = next_window(codec, fmt)
        rest.append(text)
    assert fmt.call(codec, "end") == MK_OK
    assert state == 1 and first + b"".join(rest) == TEXT


@pytest.mark.parametrize("name", FORMATS)
def test_release_ends_any_stream(mk, codec, formats, name):
    fmt = formats[name]
    L = codec._L
    taken = C.c_uint32(0)
    assert fmt.begin(codec, taken) == MK_OK and taken.value == 1
    state, first, _ = next_window(codec, fmt)
    assert state == 0 and first and TEXT.startswith(first)
    assert L.mk_gzip_text_release(codec._h) == MK_OK
    n, state = C.c_uint64(77), C.c_uint32(77)
    assert fmt.call(codec, "next", C.byref(n), C.byref(state)) == MK_E_INVALID_ARG and b"no open stream" in L.mk_last_error()
    assert (n.value, state.value) == (0, 2)
    m = C.c_uint64(77)
    assert L.mk_gzip_text_device(codec._h, C.byref(m)) is None and m.value == 0
    other = formats[FORMATS[(FORMATS.index(name) + 1) % 4]]
    assert one_shot_text(codec, other) == TEXT, other.name
    assert fmt.call(codec, "end") == MK_OK  # (no stream open: nothing to do)


@pytest.mark.parametrize("name", FORMATS)
def test_abandon_and_reuse(mk, formats, name):
    fmt, other = formats[name], formats[FORMATS[(FORMATS.index(name) + 1) % 4]]
    codec = new_codec(mk)
    it = fmt.generator(codec)
    first = next(it)
    it.close()  # _end in mid-file
    assert first and TEXT.startswith(first) and len(first) < len(TEXT)
    parts = list(other.generator(codec))
    assert len(parts) >= 3 and b"".join(parts) == TEXT and codec.stream_state == 1, (other.name, [len(p) for p in parts])
    codec.close()
