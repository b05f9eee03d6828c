"""The device's deflate writer (merkurio_amd/csrc/codec/bgzf_deflate.hip) on crafted texts, its members read back TOKEN BY TOKEN.
zlib's round trip (test_gpu_codec.py) proves that a member is valid; it cannot show which tokens the kernel chose.  Here every member
is checked three ways: its fields and zlib's text as check_members of test_gpu_codec.py does; its tokens, read by tests/deflate_read.py,
against what the kernel's parse rule promises of the text (tests/deflate_texts.py, each text's claims checked on the CPU by
test_deflate_read_cpu.py); and the stream's last bit against the member's size.  Every member of every case also obeys the stored
rule read off the output: data_len <= isize + 5, with equality if and only if the block is stored."""
import collections
import struct
import zlib

import numpy as np
import pytest

import deflate_read as dr
import deflate_texts as dt
from merkurio_amd import native as mk
from test_codec_cpu import corpora

pytestmark = pytest.mark.gpu

HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])


@pytest.fixture(scope="module")
def codec():
    c = mk.Codec()
    yield c
    c.close()


def read_members(blob, texts):
    """-> the one block of every member.  Asserted for each: header, BSIZE, CRC-32, ISIZE, zlib's text; one final block that
    renders the member's own text (a distance in front of the member raises in the reader); matches of 4 .. 258 bytes at most
    32 768 back; the stored rule; for a dynamic block complete codes and the end-of-block symbol in the member's last byte"""
    mem, used, total = mk.bgzf_members(blob)
    assert used == len(blob) and len(mem) == len(texts) and total == sum(map(len, texts))
    at, out = 0, []
    for k, (m, text) in enumerate(zip(mem, texts)):
        start, n = int(m["data_off"]) - 18, int(m["data_len"])
        assert start == at and blob[start:start + 16] == HEADER
        bsize = struct.unpack_from("<H", blob, start + 16)[0]
        assert bsize + 1 == 18 + n + 8
        payload = blob[start + 18:start + 18 + n]
        z = zlib.decompressobj(-15)
        assert z.decompress(payload) == text and z.eof and z.unused_data == b"", k
        assert int(m["crc"]) == zlib.crc32(text) and int(m["isize"]) == len(text)
        blocks = dr.read(payload)
        assert len(blocks) == 1 and blocks[0]["final"] and dr.render(blocks) == text, k
        b = blocks[0]
        assert all(4 <= l <= 258 and 1 <= d <= 32768 for l, d in dr.matches(b["tokens"])), k
        assert n <= len(text) + 5 and (n == len(text) + 5) == (b["type"] == 0), (k, n, len(text), b["type"])
        assert b["type"] in (0, 2)
        if b["type"] == 2:
            assert 0 <= 8 * n - b["end"] <= 7, k
            assert dr.kraft(b["ll"]) == 1 << 15 and dr.kraft(b["d"]) == 1 << 15 and max(b["ll"] + b["d"]) <= 15, k
        out.append(b)
        at += bsize + 1
    assert at == len(blob)
    return out


def one_member(codec, text):
    assert 0 < len(text) <= dt.MEMBER
    return read_members(codec.deflate(text), [text])[0]


def literal_cost(b, text):
    """(bits the block spends on the literals of `text` and the end-of-block symbol, bits of an unrestricted Huffman code for them)"""
    hist = collections.Counter(text)
    hist[256] = 1
    return sum(b["ll"][s] * c for s, c in hist.items()), dt.huffman_cost(hist)[0]


# ---- a. no 4 bytes twice ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dt.NO_REPEAT_SIZES)
def test_text_without_a_repeat_is_all_literals(codec, n):
    """n literals and the end-of-block symbol, 63 / 64 / 65 ... tokens either side of a group of the bit packer; 65 281 tokens (the
    token scratch holds 65 536) in 1 021 rounds of it.  No match to pay for, so the body costs what the best prefix code costs"""
    text = dt.no_repeat_text(n)
    b = one_member(codec, text)
    assert b["type"] == 2 and b["tokens"] == list(text)
    spent, best = literal_cost(b, text)
    assert spent == best, (spent, best)
    assert b["end"] - b["start"] == b["header_bits"] + spent


# ---- b. runs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", dt.RUN_LENGTHS)
def test_runs_behind_a_separator_and_alone(codec, length):
    text = dt.run_text(length, dt.RUN_SEPARATOR)
    b = one_member(codec, text)
    assert b["type"] == 2 and b["tokens"][:dt.RUN_SEPARATOR] == list(text[:dt.RUN_SEPARATOR])
    dt.check_run_tokens(b["tokens"][dt.RUN_SEPARATOR:], length)
    b = one_member(codec, dt.run_text(length))  # (the shortest runs are stored: then the text is all there is to check)
    if b["type"] == 2:
        dt.check_run_tokens(b["tokens"], length)
    assert b["type"] == 2 or length < 64


def test_run_of_a_whole_member(codec):
    b = one_member(codec, dt.run_text(dt.MEMBER))
    assert b["type"] == 2 and len(b["tokens"]) == 1 + (dt.MEMBER - 1) // 258 + 1
    dt.check_run_tokens(b["tokens"], dt.MEMBER)
    sep = dt.RUN_SEPARATOR
    b = one_member(codec, dt.run_text(dt.MEMBER - sep, sep))
    assert b["type"] == 2
    dt.check_run_tokens(b["tokens"][sep:], dt.MEMBER - sep)


# ---- c. distance edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dt.FAR_DISTANCES)
def test_copy_at_a_distance_the_window_allows(codec, d):
    """matches of distance exactly d stand for at least 300 - 64 - 8 bytes of the second copy.
    Seen on an MI355X: 299 bytes at d = 300, 296 at 32 767, 300 at 32 768."""
    text = dt.distance_text(d)
    b = one_member(codec, text)
    got = dt.covered(b["tokens"], d, d + dt.COPY, distance=d)
    print("distance %d: %d of %d bytes of the second copy in matches of that distance" % (d, got, dt.COPY))
    assert b["type"] == 2 and got >= dt.COPY - 64 - 8, got


@pytest.mark.parametrize("d", dt.TOO_FAR_DISTANCES)
def test_copy_beyond_the_window_is_no_match(codec, d):
    text = dt.distance_text(d)
    b = one_member(codec, text)  # (valid, renders the text)
    assert b["type"] == 2 and max(dist for _, dist in dr.matches(b["tokens"])) <= 32768
    assert b["tokens"][-dt.COPY:] == list(text[-dt.COPY:])  # the second copy has nothing in reach: literals


@pytest.mark.parametrize("d", dt.NEAR_DISTANCES)
def test_repeats_nearer_than_a_window(codec, d):
    """256 bytes, then d bytes four times, the first at a window's first lane.  A window looks its candidates up before it enters any:
    the issue's bound -- d - 64 - 8 bytes of the last copy in matches -- is below zero for every d here, so it holds of any valid
    stream.  What the rule does promise: behind the first window of the repeats (64 positions, 8 for collisions in the table)
    every byte is part of a match"""
    text = dt.near_text(d)
    b = one_member(codec, text)
    assert b["type"] == 2
    assert dt.covered(b["tokens"], len(text) - d, len(text)) >= d - 64 - 8
    first = dt.NEAR_LEAD + d  # the first byte that repeats
    literals = (len(text) - first) - dt.covered(b["tokens"], first, len(text))
    print("period %d: %d literals behind the first copy" % (d, literals))
    assert literals <= 64 + 8, literals


# ---- d. the lazy step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane", dt.LAZY_LANES)
def test_one_step_lazy_rule(codec, lane):
    text, q = dt.lazy_text(lane)
    b = one_member(codec, text)
    assert b["type"] == 2
    if lane == 63:  # the next position lies in the next window: the walk cannot look at it.  A valid stream is all that is promised
        return
    at = dict(dr.positions(b["tokens"]))
    assert at.get(q) == text[q] and at.get(q + 1) == (23, q + 1 - 34), (at.get(q), at.get(q + 1))
    assert dr.matches(b["tokens"]) == [(23, q + 1 - 34)]


# ---- e. every symbol ----------------------------------------------------------------------------------------------------------------------------
def test_every_length_and_distance_symbol(codec):
    text, plan = dt.symbols_text()
    b = one_member(codec, text)
    assert b["type"] == 2 and b["hlit"] == 286 and b["hdist"] == 30
    at = dict(dr.positions(b["tokens"]))
    missing = [(pos, length, dist, at.get(pos)) for pos, length, dist, exact in plan if exact and at.get(pos) != (length, dist)]
    assert not missing, missing
    assert b["tokens"][:dt.SYMBOLS_NOISE] == list(text[:dt.SYMBOLS_NOISE])
    used = {dr.LEN_BASE.index(max(x for x in dr.LEN_BASE if x <= l)) for l, _ in dr.matches(b["tokens"])}
    assert used >= set(range(1, 29))


# ---- f. deep codes ------------------------------------------------------------------------------------------------------------------------------
FIBONACCI_SEED = 0


def test_deep_codes_are_limited_to_15_bits(codec):
    """complete codes and no length above 15: read_members.  Whether a codeword of 15 bits is reached depends on the matches the
    kernel takes (they thin out the literals' counts).  Of the shuffles 0 .. 15 of the Fibonacci text, 0, 6, 10, 11 and 15 reach
    15 on an MI355X, the others 14 or 13 (the CPU test's shuffle, 3: 14): shuffle 0 is kept and must reach it.  corpora()["skew"]
    reached 15 as well (printed, not asserted)"""
    b = one_member(codec, dt.fibonacci_text(FIBONACCI_SEED))
    print("fibonacci seed %d: longest literal / length codeword %d, distance %d" % (FIBONACCI_SEED, max(b["ll"]), max(b["d"])))
    assert b["type"] == 2 and max(b["ll"]) == 15
    skew = one_member(codec, corpora()["skew"])
    print("skew: longest literal / length codeword %d, distance %d" % (max(skew["ll"]), max(skew["d"])))
    assert skew["type"] == 2


# ---- g. the stored edge -------------------------------------------------------------------------------------------------------------------------
def test_stored_edge_sweep(codec):
    """the rule itself is asserted of every member by read_members; here texts on either side of it, a byte or two apart"""
    kinds = collections.Counter()
    for n in dt.EDGE_SIZES:
        text = dt.edge_text(n)
        for b in read_members(codec.deflate(text, n), [text[i:i + n] for i in range(0, len(text), n)]):
            kinds[b["type"]] += 1
    print("stored edge sweep: %d stored, %d dynamic" % (kinds[0], kinds[2]))
    assert kinds[0] >= 20 and kinds[2] >= 20, kinds


# ---- h. seams -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb", dt.SEAM_BLOCKS)
def test_period_13_cut_into_members(codec, bb):
    """every member's tokens render its own block: no distance reaches in front of the member (the reader starts each with no text)"""
    text = dt.period_text()
    blocks = read_members(codec.deflate(text, bb), [text[i:i + bb] for i in range(0, len(text), bb)])
    if bb >= 259:
        assert all(b["type"] == 2 and dr.matches(b["tokens"]) for b in blocks[:-1])


def test_more_members_than_resident_waves(codec):
    """4 160 members of 256 bytes in one call, unlike neighbours in turn: a wave that takes a second member finds the table, the
    counts and the staging words of the first"""
    members = [dt.mixed_member(k) for k in range(dt.MIXED_MEMBERS)]
    texts = [t for _, t in members]
    blocks = read_members(codec.deflate(b"".join(texts), dt.MIXED_BYTES), texts)
    kinds = collections.Counter()
    for (kind, text), b in zip(members, blocks):
        kinds[kind, b["type"]] += 1
        if kind == "a":
            assert b["type"] == 2 and b["tokens"] == list(text)
            spent, best = literal_cost(b, text)
            assert spent == best
        if kind == "b":
            sep = dt.MIXED_SEPARATOR
            assert b["type"] == 2 and b["tokens"][:sep] == list(text[:sep])
            dt.check_run_tokens(b["tokens"][sep:], dt.MIXED_BYTES - sep)
    assert kinds["g", 0] == dt.MIXED_MEMBERS // 4, kinds  # flat noise: stored


# ---- the same edges in front of the range kernel (mk_bgzf_deflate_records) -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no-repeat", "run"])
def test_largest_member_of_the_cut_rule(codec, case):
    """a record that ends one byte short of a grid point's reach: member 0 holds 65 279 bytes, the most the cut rule yields"""
    big = dt.MEMBER - 1
    head = dt.no_repeat_text(big) if case == "no-repeat" else dt.run_text(big)
    text = head + dt.noise(100, seed=9)
    ends = np.array([big, len(text)], dtype=np.uint64)
    assert mk.bgzf_record_cuts(ends).tolist() == [0, big, len(text)]
    blocks = read_members(codec.deflate_records(text, ends), [text[:big], text[big:]])
    assert blocks[0]["type"] == 2
    if case == "no-repeat":
        assert blocks[0]["tokens"] == list(head)
        spent, best = literal_cost(blocks[0], head)
        assert spent == best
    else:
        dt.check_run_tokens(blocks[0]["tokens"], big)
