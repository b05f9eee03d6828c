"""mk_zstd_deflate_records on the device (zstd_deflate.hip, a wave per frame) through native.py.  Every text: its frames decode ALONE
with libzstd to the text; mk_zstd_inflate_device takes the file (taken == 1) and gives the text; the frames' text lengths are the
differences of mk_zstd_record_cuts (host), so the device cut kernel agrees with the host rule; every frame ends at a record end or holds
a piece of a record no frame could hold; the block kinds reported are the ones each case is built to force.

Not forced here, because no text can: RLE literals inside a Compressed block (the first occurrence of every byte value is a literal, so
one distinct literal means one distinct byte, which is an RLE block; the writer has no such branch), and an offset above 131 068 (a
frame holds 131 071 bytes at most: see zstd_out_cases.far_offset_text)."""
import functools
import random

import numpy as np
import pytest

import zstd_cases as zc
import zstd_out_cases as zo
from merkurio_amd import native as mk

pytestmark = pytest.mark.gpu
G, M = zo.GRID, zo.TEXT_MAX
RAW, RLE, COMP = 0, 1, 2


@pytest.fixture(scope="module")
def codec():
    c = mk.Codec()
    yield c
    c.close()


def line_ends(text):
    e = [i + 1 for i, b in enumerate(text) if b == 10]
    if not e or e[-1] != len(text):
        e.append(len(text))
    return e


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (text, record ends, the kind of every frame's block or None where the case does not force it)"""
    rng = random.Random(17)
    rnd = bytes(rng.getrandbits(8) for _ in range(6000))
    fq = zc.fastq(420)
    wide = bytes(rng.sample(range(127, 256), 129))
    out = {}
    for n in (1, 2, 3, 4, 63, 64, 65, 4095, 4096, 4097):
        t = fq[:n]
        # (63 to 65 bytes of a FASTQ record: no kind is forced -- a tree description alone outweighs what Huffman saves on them)
        out["size-%d" % n] = (t, line_ends(t), [RLE] if n == 1 else [RAW] if n < 5 else [COMP] if n > 4000 else None)
    out["record-131072"] = (fq[:M], [M], [COMP, COMP])
    out["record-131073"] = (fq[:M + 1], [M + 1], [COMP, COMP])
    out["one-byte"] = (b"G" * 5000, [5000], [RLE])
    out["random"] = (rnd, [len(rnd)], [RAW])
    out["two-symbols"] = (b"aaababbbaa", [10], [RAW])
    t = wide + b"Z" * 3000 + wide[:64]
    out["wide-literals"] = (t, [len(t)], [COMP])
    for n in (1023, 1024, 16383, 16384):
        out["literals-%d" % n] = (zc.match_free_text(n), [n], [COMP])
    t = zc.short_matches_text()
    out["short-matches"] = (t, [len(t)], [COMP, COMP])
    # the three forms of the sequence count, one frame each (a record of 131 071 bytes is one frame): a unit of quad_units is one sequence
    for k in (127, 128, 32767):
        out["quads-%d" % k] = (zo.quad_units(k), [4 * k], [COMP])
    out["many-sequences"] = (t[:M - 1], [M - 1], [COMP])
    out["long-match"] = (b"x" + b"G" * (G - 1), [G], [COMP])
    t = zo.match_free_bytes(66000) + fq[:3000] * 3
    out["long-literals"] = (t, [len(t)], [COMP])
    out["far-offset"] = (zo.far_offset_text(), [M - 1], [COMP])
    # sixty runs of fresh bytes: every sequence is two literals and a match of 20 at offset 1 (the wave's parse sees a run inside a
    # window; what repeats at a distance is found only from the window before)
    t = b"".join(bytes([2 * i + 1]) + bytes([2 * i + 2]) * 21 for i in range(60))
    out["one-code-each"] = (t, [len(t)], [COMP])
    t = b"A" * 10 + b"xy" + b"B" * 25 + b"C" * 40 + b"pqr" + b"D" * 70 + b"E" * 9
    out["few-sequences"] = (t, [len(t)], [COMP])
    out["fastq-skewed"] = (fq[:G], [G], [COMP])  # a full frame: tens of thousands of sequences
    return out


def check(codec, text, ends, kinds=None, blob=None):
    blob = codec.zstd_records(text, ends) if blob is None else blob
    frames = zo.frames_by_libzstd(blob)
    assert b"".join(t for _, t in frames) == text
    cuts = mk.zstd_record_cuts(ends).tolist()
    assert cuts == zo.rule(ends)
    at = [0]
    for _, t in frames:
        at.append(at[-1] + len(t))
    assert at == cuts and codec.last_frames == len(frames)
    kept = set(int(e) for e in ends) | {0}
    assert all(c in kept or c % G == 0 for c in cuts)
    shapes = [zo.shape(f) for f, _ in frames]
    n, k, ms = codec.zstd_records_info()
    assert n == len(frames) and list(k) == [sum(s["block"] == b for s in shapes) for b in (RAW, RLE, COMP)]
    if kinds is not None:
        assert [s["block"] for s in shapes] == kinds, shapes
    assert all(len(f) <= len(t) + 16 for f, t in frames), "a compressed block is never larger than the raw form"
    taken, got, _ = codec.unzstd(blob)
    assert taken and bytes(got) == text
    return shapes


@pytest.mark.parametrize("name", sorted(cases()))
def test_frames_round_trip_with_the_kinds_the_case_forces(codec, name):
    text, ends, kinds = cases()[name]
    s = check(codec, text, ends, kinds)
    print(name, [(x["block"], x.get("lit"), x.get("n_lit"), x.get("n_seq"), x.get("modes")) for x in s])
    if name == "wide-literals":
        assert s[0]["lit"] == 0
    if name.startswith("literals-"):
        n = int(name.split("-")[1])
        assert (s[0]["lit"], s[0]["n_lit"], s[0]["n_seq"], s[0]["lit_format"]) == (2, n, 0, {1023: 0, 1024: 2, 16383: 2, 16384: 3}[n])
    if name == "long-match":
        assert (s[0]["n_seq"], s[0]["n_lit"], s[0]["modes"]) == (1, 2, (1, 1, 1))  # match-length code 52: one match of 114 686 bytes
    if name == "long-literals":
        assert s[0]["n_lit"] > 65536  # literal-length code 35 in front of the first match
    if name == "one-code-each":
        assert s[0]["modes"] == (1, 1, 1) and s[0]["n_seq"] == 60
    if name == "few-sequences":
        assert set(s[0]["modes"]) <= {0, 1} and 0 in s[0]["modes"]
    if name == "fastq-skewed":
        # (matches among four bases and seven qualities are short: 114 688 bytes are more than 10 000 sequences, and from 2 048 on the
        # described tables take their largest accuracy logs, 9 / 8 / 9)
        assert s[0]["modes"] == (2, 2, 2) and s[0]["n_seq"] >= 10000 and s[0]["ll_log"] == 9
    if name.startswith("quads-"):
        k = int(name.split("-")[1])
        assert s[0]["n_seq"] == k if k < 200 else 0x7F00 <= s[0]["n_seq"] <= k
    if name == "many-sequences":
        # the 1 Ki-entry table loses words that the harness's 64 Ki entries keep (32 668 sequences there): no count is forced here
        assert 20000 < s[0]["n_seq"] <= M // 3
    if name == "far-offset":
        assert (s[0]["n_lit"], s[0]["n_seq"], s[0]["text"]) == (4, 2, M - 1)
    if name == "short-matches":
        assert s[0]["n_seq"] > 20000 and s[0]["lit"] == 0


def test_empty_text_writes_nothing(codec):
    assert codec.zstd_records(b"", []) == b"" and codec.last_frames == 0
    assert codec.zstd_records(b"", [0, 0]) == b"" and codec.last_frames == 0


def test_forty_frames_in_passes_of_seven(codec):
    fq = zc.fastq(16000)
    ends = line_ends(fq)
    n_frames = len(mk.zstd_record_cuts(ends)) - 1
    assert n_frames >= 40
    whole = codec.zstd_records(fq, ends)
    codec.set_pass_limits(deflate_members=7)
    try:
        blob = codec.zstd_records(fq, ends)
        assert blob == whole
        check(codec, fq, ends, [COMP] * n_frames, blob=blob)
        with pytest.raises(mk.MerkurioError) as e:
            codec.zstd_records(fq, ends, out_cap=len(blob) - 1)
        assert e.value.code == mk.MK_E_CAPACITY and codec.last_need == len(blob)
        assert codec.zstd_records(fq, ends, out_cap=len(blob)) == blob
    finally:
        codec.set_pass_limits()


def test_bad_record_tables_are_refused(codec):
    with pytest.raises(mk.MerkurioError) as e:
        codec.zstd_records(b"abc\n", [3])  # the last record does not end where the text does
    assert e.value.code == mk.MK_E_INVALID_ARG
    with pytest.raises(mk.MerkurioError) as e:
        codec.zstd_records(b"abc\n", [3, 2, 4])
    assert e.value.code == mk.MK_E_INVALID_ARG
