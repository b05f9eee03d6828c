"""mk_xz_inflate_device (Codec.unxz): an .xz file decoded on the device, a wave per block -- the host's walk over streams, Index and
block headers, the LZMA2 decode kernel, the check kernel.  The files are those of tests/xz_cases.py and xz_craft.py
(test_unxz_cpu.py runs the same decoder on the host under the sanitizers); liblzma is the checker: a valid file is taken with
liblzma's text and the host harness's number of blocks and streams, a damaged one is handed back -- never another text."""
import bz2
import gzip

import numpy as np
import pytest

import xz_cases as cases
from test_unxz_cpu import NAMED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def codec(mk):
    c = mk.Codec()
    c.set_xz_spread(1)  # (every file is tried: most cases are one block; the rule has tests of its own below)
    yield c
    c.close()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """report(file) as lzma_serial.hpp makes it on the host: tests/helpers/xz_harness.cpp, built once without the sanitizers"""
    work = tmp_path_factory.mktemp("xz")
    exe = cases.build_harness(work, sanitize=False)
    return lambda blob, spread=1: cases.run_harness(exe, work, blob, spread)[0]


@pytest.mark.parametrize("name", sorted(cases.valid()))
def test_valid_file_is_taken_byte_for_byte(codec, harness, name):
    blob, text = cases.valid()[name]
    taken, got, n_blocks = codec.unxz(blob)
    info = codec.unxz_info()
    print(name, len(blob), "->", taken, n_blocks, info)
    assert taken is True and info[2] == 0
    assert got == text == cases.liblzma_says(blob)
    rep = harness(blob)
    assert n_blocks == int(rep["blocks"]) == info[0]
    assert info[1] == int(rep["streams"]) and info[3] == int(rep["largest"])


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_file_is_handed_back(mk, codec, harness, name):
    blob = cases.damaged()[name]
    assert cases.liblzma_says(blob) is None
    taken, got, n_blocks = codec.unxz(blob)
    assert taken is False and got is None and n_blocks == 0
    status = codec.unxz_info()[2]
    assert status == int(harness(blob)["status"]) and status == NAMED.get(name, status) and status < 0, (name, status)
    n = mk.C.c_uint64(7)
    assert mk.load().mk_gzip_text_device(codec._h, mk.C.byref(n)) is None and n.value == 0


@pytest.mark.parametrize("name", sorted(cases.handed_back()))
def test_valid_file_of_another_kind_is_handed_back_by_name(codec, name):
    blob, text, status = cases.handed_back()[name]
    assert cases.liblzma_says(blob) == text
    assert codec.unxz(blob) == (False, None, 0)
    assert codec.unxz_info()[2] == status


def test_the_spread_rule(mk):
    c = mk.Codec()
    try:
        single, text = cases.valid()["preset-6"]
        assert c.unxz(single) == (False, None, 0) and c.unxz_info()[2] == cases.XZ_SPREAD  # the default K: a single block is liblzma's
        assert c.unxz_info()[3] == len(text)
        c.set_xz_spread(1)
        assert c.unxz(single)[:2] == (True, text)
        blob, text = cases.blocks_of([3000, 1000])
        assert c.unxz(blob) == (True, text, 2)
        c.set_xz_spread(2)
        assert c.unxz(blob) == (False, None, 0) and c.unxz_info()[2] == cases.XZ_SPREAD
        even, text = cases.blocks_of([2000, 2000])
        assert c.unxz(even) == (True, text, 2)  # just admitted
        assert c.unxz(cases.blocks_of([2001, 1999])[0]) == (False, None, 0)  # just refused
        c.set_xz_spread(0)  # the default again
        assert c.unxz(even) == (False, None, 0)
        assert c.unxz(cases.valid()["40-blocks"][0])[0] is False and c.unxz(cases.valid()["3000-blocks"][0])[0] is True
    finally:
        c.close()


def test_what_is_no_xz_file_is_handed_back_and_the_handle_lives_on(codec):
    for blob in (b"", b"\xfd7zXZ\0", b"not an xz file at all, just text\n" * 10, gzip.compress(b"gzip"), bz2.compress(b"bzip2")):
        assert codec.unxz(blob) == (False, None, 0)
    blob, text = cases.valid()["preset-9e"]
    assert codec.unxz(blob)[:2] == (True, text)


def test_a_second_call_reuses_the_buffers_and_the_codecs_take_turns(mk, codec):
    text = cases.fastq(1300)
    gz = gzip.compress(text, 6)
    blob, want = cases.valid()["40-blocks"]
    L = mk.load()
    seen = set()
    for _ in range(3):
        assert codec.unxz(blob) == (True, want, 40)
        n = mk.C.c_uint64(0)
        seen.add(L.mk_gzip_text_device(codec._h, mk.C.byref(n)))
        assert n.value == len(want)
    assert len(seen) == 1  # the text buffer of the first call serves the next ones
    for _ in range(2):
        assert codec.gunzip(gz) == text
        assert codec.bunzip2(bz2.compress(text[:120000], 1))[:2] == (True, text[:120000])
        assert codec.unxz(blob)[:2] == (True, want)


def test_an_open_stream_on_the_handle_refuses_the_call(mk):
    L = mk.load()
    src = np.frombuffer(cases.valid()["text-1"][0], dtype=np.uint8)
    text = cases.fastq(400)
    streams = (("mk_bzip2_stream", bz2.compress(text, 1)), ("mk_gzip_stream", gzip.compress(text, 6)), ("mk_zstd_stream", None))
    for prefix, data in streams:
        if data is None:
            import zstd_cases
            data = zstd_cases.compress(text, 3, True)
        c = mk.Codec()
        try:
            z = np.frombuffer(data, dtype=np.uint8)
            taken = mk.C.c_uint32(0)
            assert getattr(L, prefix + "_begin")(c._h, z.ctypes.data, z.size, 1 << 20, mk.C.byref(taken)) == mk.MK_OK and taken.value == 1, prefix
            n, blocks = mk.C.c_uint64(0), mk.C.c_uint64(0)
            assert L.mk_xz_inflate_device(c._h, src.ctypes.data, src.size, mk.C.byref(n), mk.C.byref(taken), mk.C.byref(blocks)) == mk.MK_E_INVALID_ARG, prefix
            assert getattr(L, prefix + "_end")(c._h) == mk.MK_OK
            assert L.mk_xz_inflate_device(c._h, src.ctypes.data, src.size, mk.C.byref(n), mk.C.byref(taken), mk.C.byref(blocks)) == mk.MK_OK
        finally:
            c.close()
