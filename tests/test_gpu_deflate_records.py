"""mk_bgzf_deflate_records on the device: BGZF members that end at record ends.  The device cut kernel against the host rule
(mk_bgzf_record_cuts, itself checked against numpy in test_bgzf_cuts_cpu.py): the members' ISIZE sequence is the differences of the
host's cuts.  The range deflate kernel against zlib: every member inflates to its range of the text, CRC-32 and ISIZE agree."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import bgzf_cut_cases as cc
from merkurio_amd import native as mk

pytestmark = pytest.mark.gpu

G, L = cc.G, cc.L
LINE = np.frombuffer(b"@read/1 ACGTTGCAACGTACGTTTGACCA+IIIIIIIIIIFFFFFFFFFF#####::::::,,\n"[:64], dtype=np.uint8)


@pytest.fixture(scope="module")
def codec():
    c = mk.Codec()
    yield c
    c.close()


def fastq_like(ends, seed=1):
    """low-entropy text (zlib stays fast) of ends[-1] bytes whose records end in a line end; a few bytes differ from record to record"""
    ends = np.asarray(ends, dtype=np.int64)
    T = int(ends[-1]) if ends.size else 0
    text = np.tile(LINE, T // 64 + 1)[:T].copy()
    rng = np.random.default_rng(seed)
    at = rng.integers(0, max(T, 1), size=T // 50)
    text[at] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=at.size)
    text[ends[ends > 0] - 1] = 10
    return text.tobytes()


def check(codec, text, ends, every_member=True):
    """-> the members' bytes; asserted: the cuts are the host rule's, every member is a valid BGZF member of its range"""
    blob = codec.deflate_records(text, ends)
    cuts = mk.bgzf_record_cuts(ends)
    mem, used, total = mk.bgzf_members(blob)
    assert used == len(blob) and total == len(text) and codec.last_members == len(mem) == len(cuts) - 1
    assert mem["isize"].tolist() == np.diff(cuts).tolist()  # the device's cuts against the host's
    at = 0
    for k, m in enumerate(mem):
        start, lo, hi = int(m["data_off"]) - 18, int(cuts[k]), int(cuts[k + 1])
        assert blob[start:start + 16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) and start == at
        bsize = struct.unpack_from("<H", blob, start + 16)[0]
        assert bsize + 1 == 18 + int(m["data_len"]) + 8
        assert int(m["crc"]) == zlib.crc32(text[lo:hi]), k
        if every_member:
            d = zlib.decompressobj(-15)
            got = d.decompress(blob[int(m["data_off"]):int(m["data_off"]) + int(m["data_len"])])
            assert d.eof and d.unused_data == b"" and got == text[lo:hi], k
        at += bsize + 1
    assert at == len(blob)
    assert gzip.decompress(blob + mk.bgzf_eof()) == text  # the whole file, as a reader sees it (zlib checks every CRC-32 and ISIZE)
    return blob


def test_no_text_gives_no_member(codec):
    assert codec.deflate_records(b"", []) == b"" and codec.last_members == 0
    assert codec.deflate_records(b"", [0, 0]) == b"" and codec.last_members == 0


@pytest.mark.parametrize("name", sorted(cc.fixed_shapes()))
def test_fixed_shapes(codec, name):
    ends = cc.ends(cc.fixed_shapes()[name])
    check(codec, fastq_like(ends), ends)


def test_random_length_mixes(codec):
    for k, lens in enumerate(cc.random_shapes(12, seed=77)):
        ends = cc.ends(lens)
        check(codec, fastq_like(ends, seed=k), ends)


def test_records_that_are_not_kept_repeat_an_end(codec):
    """the window path hands the cut kernel the ends of ALL records: one that is not kept ends where the one in front of it does"""
    ends = np.repeat(cc.ends(cc.fixed_shapes()["fastq_331_over_3G_100"]), 2)
    ends = np.concatenate([np.zeros(5, dtype=np.uint64), ends])
    check(codec, fastq_like(ends), ends)


def test_incompressible_text_gives_stored_members(codec):
    ends = cc.ends(cc.fixed_shapes()["fastq_331_over_3G_100"])
    text = np.random.default_rng(5).integers(0, 256, size=int(ends[-1]), dtype=np.uint8).tobytes()
    blob = check(codec, text, ends)
    mem, _, _ = mk.bgzf_members(blob)
    assert (mem["data_len"] == mem["isize"] + 5).all()  # BTYPE 00: 1 + LEN + NLEN + the text


@pytest.mark.parametrize("points", [1023, 1025])
def test_grid_points_around_the_cut_kernels_grid(codec, points):
    """the cut kernel launches at most 8 blocks of 128 lanes, which stride over the grid points: one point fewer and one more than
    16 waves of them (test_fixed_shapes has 65: one more than a wave)"""
    lens = [331] * ((points * G - 5000) // 331)
    ends = cc.ends(lens)
    assert -(-int(ends[-1]) // G) == points
    check(codec, fastq_like(ends), ends, every_member=False)


def test_capacity_one_short_and_exact_fit(codec):
    ends = cc.ends(cc.fixed_shapes()["fastq_331_over_3G_100"])
    text = fastq_like(ends)
    blob = codec.deflate_records(text, ends)
    with pytest.raises(mk.MerkurioError) as e:
        codec.deflate_records(text, ends, out_cap=len(blob) - 1)
    assert e.value.code == mk.MK_E_CAPACITY and codec.last_need == len(blob)
    assert codec.deflate_records(text, ends, out_cap=len(blob)) == blob


def test_pass_limit_does_not_change_the_bytes(codec):
    ends = cc.ends([331] * ((10 * G - 1000) // 331))
    text = fastq_like(ends)
    blob = check(codec, text, ends)
    assert codec.last_members == 10
    codec.set_pass_limits(deflate_members=3)
    try:
        assert codec.deflate_records(text, ends) == blob
        with pytest.raises(mk.MerkurioError) as e:  # the need is the sum over the passes
            codec.deflate_records(text, ends, out_cap=len(blob) - 1)
        assert e.value.code == mk.MK_E_CAPACITY and codec.last_need == len(blob)
    finally:
        codec.set_pass_limits()


def test_record_ends_are_validated(codec):
    with pytest.raises(mk.MerkurioError) as e:
        codec.deflate_records(b"abc\n", [3])  # the last record does not end where the text does
    assert e.value.code == mk.MK_E_INVALID_ARG
    with pytest.raises(mk.MerkurioError) as e:
        codec.deflate_records(b"abc\n", [3, 2, 4])
    assert e.value.code == mk.MK_E_INVALID_ARG
