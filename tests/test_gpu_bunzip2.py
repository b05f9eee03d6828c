"""mk_bzip2_inflate_device (Codec.bunzip2): a .bz2 file decoded on the device, a wave per block -- magics searched at every bit
offset, every block decoded from its guessed start and proved by where it ends, inverse BWT, the run-length step, block and stream
CRCs.  The files are those of tests/bzip2_cases.py (test_bunzip2_cpu.py runs the same decoder on the host under the sanitizers);
Python's bz2 is the checker: a valid file is taken with libbz2's text and the host harness's number of blocks, a damaged one is
handed back -- never another text."""
import bz2

import numpy as np
import pytest

import bzip2_cases as cases

pytestmark = pytest.mark.gpu
P = b"ACGTTGCAAGGCTTAACGGAT"


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
def harness_blocks(tmp_path_factory):
    """blocks of every valid file as the host harness counts them (bzip2_serial.hpp on the host), computed once"""
    return cases.block_counter(tmp_path_factory.mktemp("bzip2"))


@pytest.fixture(scope="module")
def seven_blocks():
    text = cases.fastq(2200, seed=9)[:650000]
    return bz2.compress(text, 1), text


@pytest.mark.parametrize("name", sorted(cases.valid()))
def test_valid_file_is_taken_byte_for_byte(codec, harness_blocks, name):
    blob, text = cases.valid()[name]
    taken, got, n_blocks = codec.bunzip2(blob)
    print(name, len(blob), "->", taken, n_blocks, codec.bunzip2_info())
    assert taken is True
    assert got == text == bz2.decompress(blob)
    assert n_blocks == harness_blocks(blob) == codec.bunzip2_info()[0]


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_file_is_handed_back(mk, codec, name):
    taken, got, n_blocks = codec.bunzip2(cases.damaged()[name])
    assert taken is False and got is None and n_blocks == 0
    n = mk.C.c_uint64(7)
    assert mk.load().mk_gzip_text_device(codec._h, mk.C.byref(n)) is None and n.value == 0


def test_what_is_no_bzip2_file_is_handed_back_and_the_handle_lives_on(codec):
    for blob in (b"", b"BZ", b"BZh9", b"not a bzip2 file at all, just text\n" * 10):
        assert codec.bunzip2(blob) == (False, None, 0)
    assert codec.bunzip2(cases.damaged()["flip-symbols"]) == (False, None, 0)
    # the handle is none the worse for it
    blob, text = cases.valid()["fastq-l9"]
    assert codec.bunzip2(blob)[:2] == (True, text)


def test_pass_size_does_not_change_the_text(codec, harness_blocks, seven_blocks):
    blob, text = seven_blocks
    assert harness_blocks(blob) == 7
    try:
        for pass_blocks in (1, 2, 3, 0):
            codec.set_bzip2_pass_blocks(pass_blocks)
            taken, got, n_blocks = codec.bunzip2(blob)
            assert (taken, n_blocks) == (True, 7), pass_blocks
            assert got == text, pass_blocks
    finally:
        codec.set_bzip2_pass_blocks(0)


def test_a_full_block_and_a_short_one_at_level_9(codec):
    """1.0 MB at level 9: a block of all 900 000 symbols (less the 19 the writer leaves) and a short one"""
    text = cases.fastq(3300, seed=21)[:1000000]
    assert len(text) == 1000000
    blob = bz2.compress(text, 9)
    taken, got, n_blocks = codec.bunzip2(blob)
    print(codec.bunzip2_info())
    assert (taken, n_blocks) == (True, 2)
    assert got == text


def test_a_gzip_stream_open_on_the_handle_refuses_the_call(mk):
    import gzip
    c = mk.Codec()
    try:
        gz = np.frombuffer(gzip.compress(cases.fastq(400)), dtype=np.uint8)
        taken = mk.C.c_uint32(0)
        L = mk.load()
        assert L.mk_gzip_stream_begin(c._h, gz.ctypes.data, gz.size, 1 << 20, mk.C.byref(taken)) == mk.MK_OK and taken.value == 1
        src = np.frombuffer(cases.valid()["one-l9"][0], dtype=np.uint8)
        n, blocks = mk.C.c_uint64(0), mk.C.c_uint64(0)
        assert L.mk_bzip2_inflate_device(c._h, src.ctypes.data, src.size, mk.C.byref(n), mk.C.byref(taken), mk.C.byref(blocks)) == mk.MK_E_INVALID_ARG
    finally:
        c.close()


def test_the_text_is_a_window_source_like_uploaded_text(mk, codec):
    """a FASTQ decoded this way, handed to mk_extract_window as device_text in three windows: keep, rows and counters are those of the
    same windows uploaded as plain text"""
    import random
    rng = random.Random(3)
    recs = []
    for i in range(900):
        s = bytearray(rng.choices(b"ACGT", k=120))
        if i % 7 == 0:
            s[30:30 + len(P)] = P
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, bytes(s), b"F" * 120))
    text = b"".join(recs)
    taken, got, _ = codec.bunzip2(bz2.compress(text, 1))
    assert taken and got == text
    n = mk.C.c_uint64(0)
    d_text = mk.load().mk_gzip_text_device(codec._h, mk.C.byref(n))
    assert d_text and n.value == len(text)
    matcher = mk.Matcher(mk.parse_pattern_list(kmer_seq=[P], reverse_complement=True))
    cuts = [0, sum(len(r) for r in recs[:300]), sum(len(r) for r in recs[:600]), len(text)]
    kept = 0
    for a, b in zip(cuts, cuts[1:]):
        dev = matcher.extract_window([{"device_text": (d_text + a, b - a)}], codec=codec)
        host = matcher.extract_window([{"text": text[a:b]}])
        assert dev["status"] == host["status"] == 0
        for key in ("n_rec", "keep", "rows", "counters"):
            assert dev[key] == host[key], key
        assert dev["n_rec"] == 300
        kept += sum(dev["keep"])
    assert kept == len(range(0, 900, 7))
