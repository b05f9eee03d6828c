"""mk_bzip2_inflate_device (Codec.bunzip2) on the hand-made streams of tests/bzip2_craft.py and on sweeps aimed at the edges of the
kernels of bzip2_inflate.hip: the reader's window of 64 dwords, the move-to-front list held four entries per lane, the scatter's turn
of 64, the carry byte of the expand kernel, the 64 pieces of the CRC kernel, the 32 bit phases and the grid-stride loop of the marker
kernel.  libbz2 is the judge (test_bunzip2_craft_cpu.py runs the same files through the host harness under the sanitizers): an `ok-`
file is taken with libbz2's text and the stated blocks, a `bad-` or `host-` file is handed back with no text on the handle.  All on
one handle, every handed-back file followed by one that is taken."""
import os
import subprocess

import numpy as np
import pytest

import bzip2_cases as cases
import bzip2_craft as craft

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def compute_units(work_dir):
    """of device 0, as the runtime states them: tests/helpers/cu_count.cpp"""
    from merkurio_amd import build
    exe = os.path.join(str(work_dir), "cu_count")
    subprocess.run([build.HIPCC, "-O1", "-o", exe, os.path.join(ROOT, "tests/helpers/cu_count.cpp")], check=True)
    n = int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert 1 <= n <= 4096
    return n


def taken(codec, label, blob, text, blocks):
    got = codec.bunzip2(blob)
    assert got[0] is True and got[2] == blocks == codec.bunzip2_info()[0], (label, got[0], got[2], blocks)
    assert got[1] == text, label


def handed_back(mk, codec, label, blob):
    assert codec.bunzip2(blob) == (False, None, 0), label
    n = mk.C.c_uint64(7)
    assert mk.load().mk_gzip_text_device(codec._h, mk.C.byref(n)) is None and n.value == 0, label


@pytest.mark.parametrize("name", craft.ordered())
def test_case(mk, codec, name):
    blob, blocks, _ = craft.CASES[name]
    if name.startswith("ok-"):
        taken(codec, name, blob, craft.text_of(name), blocks)
    else:
        handed_back(mk, codec, name, blob)


def test_every_handed_back_case_is_followed_by_one_that_is_taken():
    order = craft.ordered()
    assert sorted(order) == sorted(craft.CASES) and order[-1].startswith("ok-")
    assert all(b.startswith("ok-") for a, b in zip(order, order[1:]) if not a.startswith("ok-"))


def test_cases_of_several_blocks_a_block_per_pass(codec):
    assert len(craft.MULTI) >= 2
    try:
        codec.set_bzip2_pass_blocks(1)
        for name in craft.MULTI:
            taken(codec, name, craft.CASES[name][0], craft.text_of(name), craft.CASES[name][1])
        for label, blob, text, blocks in craft.sweep_spare_selectors():
            taken(codec, label, blob, text, blocks)
    finally:
        codec.set_bzip2_pass_blocks(0)


def test_second_block_at_every_bit_phase(codec):
    for label, blob, text, blocks in craft.sweep_spare_selectors():
        taken(codec, label, blob, text, blocks)


def test_end_magic_and_crc_end_the_file_at_every_bit_phase(mk, codec):
    for label, blob, text, blocks in craft.sweep_end_magic():
        taken(codec, label, blob, text, blocks)
    # and with the file's last byte gone the end magic still lies inside it, its CRC does not
    handed_back(mk, codec, "cut", craft.sweep_end_magic()[0][1][:-1])
    taken(codec, "again", *craft.sweep_end_magic()[0][1:])


def test_second_block_around_bytes_256_and_1024(codec):
    """the reader's window of 64 dwords, and the 256 threads x 4 bytes of a workgroup of the marker kernel"""
    for label, blob, text, blocks in craft.sweep_window_seams():
        taken(codec, label, blob, text, blocks)


def test_runs_and_counts_around_a_turn_of_64_and_short_texts(codec):
    """the expand kernel's carry byte and a count in lane 0; the CRC kernel's empty lanes, full lanes and short last piece"""
    for label, blob, text, blocks in craft.sweep_expand():
        taken(codec, label, blob, text, blocks)


def test_a_file_longer_than_one_sweep_of_the_marker_grid(codec, tmp_path_factory):
    """the marker kernel's grid is at most 16 workgroups per CU, 1 KiB each: a longer file takes its grid-stride loop round again"""
    d = tmp_path_factory.mktemp("bzip2long")
    sweep_bytes = compute_units(d) * 16 * 1024
    blob, text = craft.long_file(sweep_bytes * 3 // 2)
    assert len(blob) > sweep_bytes * 3 // 2 > sweep_bytes
    blocks = cases.block_counter(d)(blob)
    assert craft.libbz2_says(blob) == text and blocks > 30
    got = codec.bunzip2(blob)
    print(len(blob), "bytes,", blocks, "blocks", codec.bunzip2_info(), "%.3f s" % codec.last_call_s)
    assert got[0] is True and got[2] == blocks == codec.bunzip2_info()[0]
    assert np.array_equal(np.frombuffer(got[1], dtype=np.uint8), np.frombuffer(text, dtype=np.uint8))
