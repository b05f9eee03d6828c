"""mk_zstd_inflate_device (Codec.unzstd): a .zst file decoded on the device, a wave per block -- the host's walk over frames and block
headers, tables and entropy decoding, the scans, execution, the rounds of cross-block resolution, the content checksum.  The files are
those of tests/zstd_cases.py and zstd_craft.py (test_unzstd_cpu.py runs the same decoder on the host under the sanitizers); libzstd is
the checker: a valid file is taken with libzstd's text and the host harness's number of blocks and rounds, a damaged one is handed back
-- never another text."""
import bz2
import gzip

import numpy as np
import pytest

import zstd_cases as cases

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
    yield c
    c.close()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """report(file) as zstd_serial.hpp makes it on the host: tests/helpers/zstd_harness.cpp, built once without the sanitizers"""
    work = tmp_path_factory.mktemp("zstd")
    exe = cases.build_harness(work, sanitize=False)
    return lambda blob: cases.run_harness(exe, work, blob)[0]


@pytest.mark.parametrize("name", sorted(cases.valid()))
def test_valid_file_is_taken_byte_for_byte(codec, harness, name):
    blob, text = cases.valid()[name]
    taken, got, n_blocks = codec.unzstd(blob)
    info = codec.unzstd_info()
    print(name, len(blob), "->", taken, n_blocks, info)
    assert taken is True
    assert got == text == cases.libzstd_says(blob)
    rep = harness(blob)
    assert n_blocks == int(rep["blocks"]) == info[0]
    assert info[1] == int(rep["frames"]) and info[2] == int(rep["rounds"])


def test_a_chain_of_40_blocks_takes_six_rounds(codec):
    blob, text = cases.valid()["chain-40"]
    taken, got, n_blocks = codec.unzstd(blob)
    assert taken is True and got == text and n_blocks == 40
    assert codec.unzstd_info()[2] == 6


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_file_is_handed_back(mk, codec, name):
    taken, got, n_blocks = codec.unzstd(cases.damaged()[name])
    assert taken is False and got is None and n_blocks == 0
    n = mk.C.c_uint64(7)
    assert mk.load().mk_gzip_text_device(codec._h, mk.C.byref(n)) is None and n.value == 0


def test_what_is_no_zstd_file_is_handed_back_and_the_handle_lives_on(codec):
    for blob in (b"", b"\x28\xb5", b"\x28\xb5\x2f\xfd", b"not a zstd file at all, just text\n" * 10, gzip.compress(b"gzip"), bz2.compress(b"bzip2")):
        assert codec.unzstd(blob) == (False, None, 0)
    assert codec.unzstd(cases.damaged()["flip-sequences"]) == (False, None, 0)
    # the handle is none the worse for it
    blob, text = cases.valid()["fastq-l19-checksum"]
    assert codec.unzstd(blob)[:2] == (True, text)


def test_gunzip_bunzip2_and_unzstd_in_turn_on_one_handle(codec):
    text = cases.fastq(1300)
    gz = gzip.compress(text, 6)  # (a stream of this length has block starts to find: the device takes it)
    for _ in range(2):
        assert codec.gunzip(gz) == text
        assert codec.bunzip2(bz2.compress(text[:120000], 1))[:2] == (True, text[:120000])
        assert codec.unzstd(cases.compress(text, 3, True))[:2] == (True, text)


def test_a_bzip2_stream_open_on_the_handle_refuses_the_call(mk):
    c = mk.Codec()
    try:
        bz = np.frombuffer(bz2.compress(cases.fastq(400), 1), dtype=np.uint8)
        taken = mk.C.c_uint32(0)
        L = mk.load()
        assert L.mk_bzip2_stream_begin(c._h, bz.ctypes.data, bz.size, 1 << 20, mk.C.byref(taken)) == mk.MK_OK and taken.value == 1
        src = np.frombuffer(cases.valid()["size-1"][0], dtype=np.uint8)
        n, blocks = mk.C.c_uint64(0), mk.C.c_uint64(0)
        assert L.mk_zstd_inflate_device(c._h, src.ctypes.data, src.size, mk.C.byref(n), mk.C.byref(taken), mk.C.byref(blocks)) == mk.MK_E_INVALID_ARG
    finally:
        c.close()
