"""Hand-made DEFLATE streams (tests/deflate_craft.py) through the device's inflaters, against zlib's verdict -- the checker for
RFC 1951 / RFC 1952 here, as in test_gpu_codec.py, whose streams are all zlib's or the device's own writing.  What a compressor
never writes: matches back to byte 0 and at distance 32 768, 15-bit codewords, dynamic blocks without a distance code, empty blocks;
and streams that are ILLEGAL although their trailer (CRC-32, ISIZE) agrees with what a lenient decoder would write -- there the
decoder itself must refuse, not the checksum.  BGZF members on all seven selections of the inflate kernel (where a member stands in a
call, the edges of the wave decoders' LDS rings and flushes, the largest and the empty member), one gzip stream in parallel pieces on
both piece decoders."""
import re
import zlib

import numpy as np
import pytest

import deflate_craft as craft
from merkurio_amd import native as mk
from test_codec_cpu import corpora, raw_deflate

pytestmark = pytest.mark.gpu

RINGS = (2048, 4096, 8192, 16384, 32768)
STREAM_ERRORS = range(-6, 0)  # inflate_serial.hpp: truncated, block type, stored LEN, code lengths, symbol, distance (-7 / -8: ISIZE)


@pytest.fixture(scope="module", params=[0, 1, 2, 3, 4, 5, 6], ids=["kernel-by-size", "lane-per-member", "wave-per-member", "wave-8k-ring", "wave-16k-ring", "wave-4k-ring", "wave-2k-ring"])
def codec(request):
    """the seven selections of test_gpu_codec.py's fixture (mk_codec_set_inflate_kernel)"""
    c = mk.Codec()
    c.set_inflate_kernel(request.param)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["wave-per-piece", "lane-per-piece"])
def gunzip_codec(request):
    c = mk.Codec()
    c.set_inflate_kernel(request.param)
    c.set_gzip_chunk(craft.GUNZIP_CHUNK)
    yield c
    c.close()


def neighbours():
    """zlib-written members of other sizes: 1 byte, 777, a full block, 12 345 -- (raw stream, text) each"""
    fastq = corpora()["fastq"]
    return [(raw_deflate(t, level=lv), t) for t, lv in ((fastq[:1], 6), (fastq[100:877], 1), (fastq[:65280], 6), (fastq[5000:17345], 9))]


def inflate(codec, members):
    """members: [(raw stream, the text its trailer speaks of)] -> the text of the call.  The member table is written here (a stream of
    stored blocks for 64 KiB of text is longer than BSIZE can say), the text back to back as mk_bgzf_members lays it out"""
    blob = b"".join(craft.bgzf_member(raw, text) for raw, text in members)
    table = np.zeros(len(members), dtype=mk.MEMBER_DTYPE)
    at = out = 0
    for k, (raw, text) in enumerate(members):
        table[k]["data_off"], table[k]["out_off"], table[k]["data_len"], table[k]["isize"], table[k]["crc"] = at + 18, out, len(raw), len(text), zlib.crc32(text)
        at += 18 + len(raw) + 8
        out += len(text)
    if all(len(raw) + 25 <= 0xffff for raw, _ in members):  # (the walk of the headers gives the same table)
        walked, used, n_text = mk.bgzf_members(blob)
        assert used == len(blob) and n_text == out and walked.tobytes() == table.tobytes()
    return codec.inflate(blob, table, out)


def ok_streams():
    return [(name, raw, craft.verdict(raw)[0]) for name, raw, _ in craft.CATALOGUE if name.startswith("ok-")]


def test_ok_streams_wherever_they_stand_in_a_call(codec):
    """every `ok-` stream as the only member, as member 0, in the middle and last among zlib-written members: its out_off is then not 0
    and not aligned, a neighbour's text lies directly in front of its own -- zlib's text, byte for byte"""
    nb = neighbours()
    for name, raw, text in ok_streams():
        m = (raw, text)
        assert inflate(codec, [m]) == text, (name, "alone")
        assert inflate(codec, [m, nb[1], nb[3]]) == text + nb[1][1] + nb[3][1], (name, "first")
        assert inflate(codec, [nb[0], nb[1], m]) == nb[0][1] + nb[1][1] + text, (name, "last")
    # in the middle: all of them in one call, a neighbour of another size between every two (and once more in the opposite order)
    for streams in (ok_streams(), ok_streams()[::-1]):
        members = [nb[2]]
        for k, (name, raw, text) in enumerate(streams):
            members += [(raw, text), nb[k % len(nb)]]
        got = inflate(codec, members)
        at = len(nb[2][1])
        for k, (name, raw, text) in enumerate(streams):
            assert got[at:at + len(text)] == text, (name, "middle")
            at += len(text) + len(nb[k % len(nb)][1])
        assert got == b"".join(t for _, t in members)


def refused(codec, members, k, name):
    with pytest.raises(mk.MerkurioError) as e:
        inflate(codec, members)
    msg = str(e.value)
    assert e.value.code == mk.MK_E_CORRUPT and "member %d" % k in msg, (name, msg)
    assert "CRC" not in msg, (name, msg)  # the decoder, not the checksum
    status = re.search(r"decoder status (-?\d+)", msg)
    assert status and int(status.group(1)) in STREAM_ERRORS, (name, msg)  # ... and not the ISIZE check (-7, -8)


def test_bad_streams_are_refused_by_the_decoder_not_by_the_trailer(codec):
    """every `bad-` stream as member 2 of an otherwise valid call, its trailer the CRC-32 / ISIZE of what zlib had written when it
    stopped -- for a match that reaches in front of the member, of the lenient reading: with zeros there, and with the text of
    member 1, which is what lies in front of it in the output buffer and what a decoder without the check would copy"""
    nb = neighbours()
    front_text = nb[3][1]
    for name, raw, lenient in craft.CATALOGUE:
        if not name.startswith("bad-"):
            continue
        texts = [craft.WRITTEN[name]]
        if lenient is not None:
            blocks = [craft.fixed([(3, 1), 65])] if name == "bad-fixed-match-first" else [craft.fixed([0x41, 0x80, 0xff, (10, 4), 0x42])]
            assert craft.stream(blocks) == raw
            texts = [lenient, craft.render(blocks, before=front_text)]
            assert texts[0] != texts[1]
        for text in texts:
            refused(codec, [nb[0], nb[3], (raw, text), nb[1]], 2, name)


def test_bytes_behind_the_final_block_are_ignored(codec):
    """bytes inside data_len behind the stream's final block: zlib leaves them unread (unused_data) and gives the text; so does every
    selection (include/merkurio_hip.h, mk_bgzf_inflate)"""
    nb = neighbours()
    text = corpora()["fastq"][:3000]
    for raw in (raw_deflate(text, level=6), raw_deflate(text, level=0), craft.stream([craft.fixed(list(text[:50]))])):
        want = craft.verdict(raw)[0]
        for tail in (b"\0", b"\xde\xad\xbe\xef", bytes(range(256)) * 2):
            assert craft.verdict(raw + tail) == (want, len(tail))
            assert inflate(codec, [nb[1], (raw + tail, want), nb[0]]) == nb[1][1] + want + nb[0][1], len(tail)


@pytest.mark.parametrize("ring", RINGS)
def test_matches_at_the_ring_and_flush_edges(codec, ring):
    """the wave decoders keep the last `ring` bytes of a member in LDS and send text to memory 4 KiB (or half a ring) at a time; a match
    whose source has left the ring reads it back.  Distances around the ring's size, lengths around a wave's 64 lanes and the longest,
    the match's first byte around multiples of 4 096 and of the ring: one member per combination (craft.ring_edge_members), all of
    one ring size in one call, on every selection -- zlib's text"""
    members = craft.ring_edge_members(ring)
    got = inflate(codec, [(raw, text) for _, raw, text in members])
    at = 0
    for label, _, text in members:
        assert got[at:at + len(text)] == text, (ring, label)
        at += len(text)
    assert at == len(got)


def test_largest_and_empty_members(codec):
    """ISIZE 65 536 (the most mk_bgzf_members lets through) as stored blocks and as one literal and a run; ISIZE 0 as a dynamic block
    that holds its end-of-block code alone; a member whose last block is an empty stored one"""
    big = craft.noise(65536, 5)
    cases = [craft.stored_run(big[:65535]) + [craft.stored(big[65535:])],
             craft.stored_run(big, 4097),
             [craft.fixed([0x80] + [(258, 1)] * 254 + [(3, 1)])],
             [craft.dynamic([0] * 256 + [1], [0], [])],
             [craft.fixed(list(big[:100])), craft.stored()],
             [craft.stored(big[:70]), craft.stored(), craft.stored()]]
    members = []
    for blocks in cases:
        raw = craft.stream(blocks)
        text, unused = craft.verdict(raw)
        assert text is not None and unused == 0
        members.append((raw, text))
    assert [len(t) for _, t in members] == [65536, 65536, 65536, 0, 100, 70]
    for m in members:
        assert inflate(codec, [m]) == m[1]
    assert inflate(codec, members) == b"".join(t for _, t in members)
    assert inflate(codec, members[::-1]) == b"".join(t for _, t in members[::-1])


# ---- one gzip stream in parallel pieces ------------------------------------------------------------------------------------------------
def test_gunzip_takes_every_hand_made_stream_zlib_takes(gunzip_codec):
    """pieces that begin with a match of distance 32 768, with a run of a place-holder, with a match that overlaps out of the context
    into the piece; bytes carried on by matches through twelve pieces shorter than 32 KiB; pieces of 32 767 / 32 768 / 32 769 bytes;
    text of 0xFF / 0x80 (a place-holder is told from a byte by bit 15 of a 16-bit element); a header with FEXTRA, FNAME, FCOMMENT and
    FHCRC: every one is TAKEN (test_codec_cpu.py shows the serial form takes them in that many pieces), in at least the pieces it
    was built to have, and gives zlib's text"""
    left_out = []
    for name, gz, text, pieces in craft.gunzip_streams():
        if text is None:
            continue
        got = gunzip_codec.gunzip(gz)
        if got is None:
            left_out.append((name, gunzip_codec.gzip_info))
            continue
        assert got == text, name
        assert gunzip_codec.gzip_info[0] >= pieces, (name, gunzip_codec.gzip_info, pieces)
    assert not left_out, left_out


def test_gunzip_hands_back_a_match_in_front_of_the_stream(gunzip_codec):
    """a match that reaches in front of the stream's first byte -- the first token of piece 0; in piece 1 through place-holders of the
    32 KiB in front; three pieces on, through copies of that place-holder -- with the CRC-32 / ISIZE of the lenient reading (zeros in
    front of the stream): zlib says "invalid distance too far back", the device hands the file back.  Reserved FLG bits: handed back"""
    for name, gz, text, pieces in craft.gunzip_streams():
        if text is not None:
            continue
        with pytest.raises(zlib.error, match="too far back"):
            zlib.decompress(gz, 31)
        assert gunzip_codec.gunzip(gz) is None, (name, gunzip_codec.gzip_info)
        assert gunzip_codec.gzip_info[0] >= pieces, (name, gunzip_codec.gzip_info)  # (cut and decoded as built: the resolution refused it)
    name, gz, text, _ = craft.gunzip_streams()[1]
    assert gunzip_codec.gunzip(gz) == text
    for bit in (0x20, 0x40, 0x80):
        assert gunzip_codec.gunzip(gz[:3] + bytes([gz[3] | bit]) + gz[4:]) is None, bit
