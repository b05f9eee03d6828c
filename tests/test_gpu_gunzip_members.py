"""mk_gzip_members_inflate_device: a gzip file of SEVERAL members (`cat a.gz b.gz`) inflated on the device in one batch of pieces --
member starts guessed by the host's header walker and proved by the decode, the context chain restarting at every member, CRC-32 and
ISIZE per member.  The files are those of tests/gunzip_members_cases.py, zlib is the checker (test_gunzip_members_cpu.py shows that
what is expected of each file here is what zlib says about it): a file comes back with zlib's text and zlib's number of members, or
it is handed back -- never with another text.  Both piece decoders, cuts every 4 KiB (the smallest mk_codec_set_gzip_chunk takes:
members of tens of KB have several pieces).  Then `extract` on such files against --host-codec."""
import gzip
import os
import random
import subprocess

import pytest

import deflate_craft as craft
import gunzip_members_cases as gm
from merkurio_amd import native as mk
from test_cli_gpu import BIN, json_stable, log_body

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, 1], ids=["wave-per-piece", "lane-per-piece"])
def codec(request):
    c = mk.Codec()
    c.set_inflate_kernel(request.param)
    c.set_gzip_chunk(craft.GUNZIP_CHUNK)
    yield c
    c.close()


@pytest.fixture(scope="module")
def verdicts():
    """zlib's (text, members) of every case, computed once"""
    return {name: gm.zlib_walk(blob) for name, blob, _ in gm.cases()}


def by_prefix(*prefixes):
    return [(name, blob, expect) for name, blob, expect in gm.cases() if name.startswith(prefixes)]


def check(codec, verdicts, selection, pieces_at_least=None):
    assert selection
    for name, blob, expect in selection:
        text, members = verdicts[name]
        got = codec.gunzip_members(blob)
        print(name, expect, "->", None if got is None else (len(got[0]), got[1]), codec.gzip_info)
        if expect == "handed-back":
            assert text is None and got is None, name
        elif expect == "taken":
            assert got is not None, (name, "not taken", codec.gzip_info)
        if got is not None:
            assert text is not None and got[0] == text and got[1] == members, name  # never another text
            assert mk.load().mk_gzip_text_device(codec._h, None) is not None or not text
        if pieces_at_least and got is not None:
            assert codec.gzip_info[0] >= pieces_at_least, (name, codec.gzip_info)


def test_members_of_fastq_text_at_three_levels(codec, verdicts):
    """2, 3 and 17 members written by zlib at levels 1 / 6 / 9: byte-exact, the right number of members, a piece per member at least"""
    sel = by_prefix("fastq-")
    assert len(sel) == 9
    check(codec, verdicts, sel, pieces_at_least=2)
    codec.gunzip_members([b for n, b, _ in gm.cases() if n == "fastq-17-members-level-6"][0])
    assert codec.gzip_info[0] >= 17, codec.gzip_info


def test_tiny_and_empty_members(codec, verdicts):
    """members of one byte; `gzip < /dev/null` in first, middle and last place; a file of nothing else: zero bytes of text, taken"""
    check(codec, verdicts, by_prefix("members-of-one-byte", "empty-member", "only-empty"))
    assert codec.gunzip_members(gm.EMPTY * 3) == (b"", 3)
    assert codec.gunzip_members(gm.EMPTY) == (b"", 1)


def test_block_types_headers_and_a_member_of_many_pieces(codec, verdicts):
    """stored, fixed and dynamic members in one file; headers with every optional field; ~200 KB of stream -- six or seven of zlib's
    blocks, a piece each where the search finds them -- between two members of one piece; text that begins with runs and far matches
    into its own first bytes, behind another member's text"""
    check(codec, verdicts, by_prefix("stored-fixed", "every-optional", "text-that-begins", "three-members", "one-member-twice"))
    check(codec, verdicts, by_prefix("a-member-of-many-pieces"), pieces_at_least=6)


def test_hand_made_members_in_the_middle_of_a_file(codec, verdicts):
    """the hand-made streams of several pieces (matches of distance 32 768 at a piece's start, bytes carried through twelve pieces,
    text of 0xff / 0x80) as the middle member: their place-holders resolve inside the member, at a text offset that is not 0"""
    check(codec, verdicts, by_prefix("hand-made-"), pieces_at_least=4)


def test_the_context_restarts_at_every_member(codec, verdicts):
    """a match that reaches in front of its member's first byte -- as the first token, through place-holders in a later piece, carried
    on by later matches -- with the trailer a reader would agree with that let member k's text (zeros) stand in front: zlib refuses
    ("too far back"), the device hands the file back"""
    sel = by_prefix("context-restarts-")
    assert len(sel) == 4
    check(codec, verdicts, sel)


def test_false_guesses_are_dropped(codec, verdicts):
    """whole valid members as the text of a stored block (one, two back to back, two apart): headers that parse, streams that decode,
    trailers that agree -- and no member starts.  Taken, within the four rounds, with zlib's two members.  Magic bytes at the end of and
    inside a payload: zlib's text or handed back"""
    sel = by_prefix("false-guess-")
    assert sum(e == "taken" for _, _, e in sel) == 3 and len(sel) == 5
    check(codec, verdicts, sel)


def test_files_zlib_refuses_are_handed_back(codec, verdicts):
    """trailing bytes, a flipped CRC-32, an ISIZE off by one, a member cut short, a damaged bit, bytes between a stream and its
    trailer: not taken, and the handle's text is what it was (none)"""
    sel = by_prefix("trailing-", "last-crc", "middle-", "damaged-", "bytes-between")
    assert len(sel) == 8 and all(e == "handed-back" for _, _, e in sel)
    ok = [b for n, b, _ in gm.cases() if n == "three-members-as-they-are"][0]
    for name, blob, _ in sel:
        assert codec.gunzip_members(ok) is not None
        assert codec.gunzip_members(blob) is None, name
        n = mk.C.c_uint64(77)
        assert mk.load().mk_gzip_text_device(codec._h, mk.C.byref(n)) is None and n.value == 0, name
    rnd = random.Random(11)
    for k in range(6):  # damage anywhere: never another text
        bad = bytearray(ok)
        bad[rnd.randrange(len(bad))] ^= 1 << rnd.randrange(8)
        got, (text, members) = codec.gunzip_members(bytes(bad)), gm.zlib_walk(bytes(bad))
        assert got is None or got == (text, members), k


def test_the_one_member_entry_keeps_handing_several_members_back(codec):
    """mk_gzip_inflate_device: one member is taken, two are not -- two different ones, and the same one twice (whose last trailer
    agrees with the first member's text); the new entry takes the one-member file with the same text"""
    a, b = gm.fastq(60, 1), gm.fastq(50, 2)
    one = gzip.compress(a, 6)
    assert codec.gunzip(one) == a
    assert codec.gunzip_members(one) == (a, 1)
    assert codec.gunzip(one + gzip.compress(b, 6)) is None
    assert codec.gunzip(one + one) is None
    assert codec.gunzip(gm.EMPTY + gm.EMPTY) is None
    assert codec.gunzip_members(one + one) == (a + a, 2)
    assert codec.gunzip_members(b"no gzip file\n" * 5) is None and codec.gunzip_members(b"") is None


# ---- extract ---------------------------------------------------------------------------------------------------------------------------
def _extract(tmp, name, inputs, extra):
    d = tmp / name
    d.mkdir()
    args = ["extract", "-i", str(inputs[0])] + (["-2", str(inputs[1])] if len(inputs) > 1 else [])
    p = subprocess.run([BIN] + args + ["-f", str(tmp / "k.txt"), "-r", "-o", str(d / "o"), "-l", str(d / "x.log"), "-j", str(d / "x.json"), *extra],
                       capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))
    return p, d


def test_extract_reads_files_of_several_members_on_the_device(tmp_path):
    """a .fastq.gz of three members, alone and as a pair: kept records, text log and JSON log equal --host-codec's, and the timing line
    says that the device took the file and proved three members (without it zlib alone would pass).  Bytes behind the last member: the
    same exit status and message as --host-codec"""
    rnd = random.Random(23)
    kmers = ["".join(rnd.choices("ACGT", k=25)) for _ in range(20)]
    (tmp_path / "k.txt").write_text("\n".join(kmers) + "\n")

    def reads(tag, n):
        out = []
        for i in range(n):
            s = "".join(rnd.choices("ACGT", k=rnd.choice((60, 100, 151))))
            if i % 9 == 0:
                o = rnd.randrange(len(s) - 25)
                s = s[:o] + rnd.choice(kmers) + s[o + 25:]
            out.append(f"@p{i}/{tag}\n{s}\n+\n{'I' * len(s)}\n".encode())
        return out

    files = []
    for tag in (1, 2):
        r = reads(tag, 3000)
        blob = gzip.compress(b"".join(r[:1000]), 6) + gzip.compress(b"".join(r[1000:1001]), 1) + gzip.compress(b"".join(r[1001:]), 9)
        assert gm.zlib_walk(blob) == (b"".join(r), 3)
        files.append(tmp_path / f"m_{tag}.fastq.gz")
        files[-1].write_bytes(blob)
    for name, inputs in (("single", files[:1]), ("pair", files)):
        dev, d_dev = _extract(tmp_path, name + "-dev", inputs, [])
        host, d_host = _extract(tmp_path, name + "-host", inputs, ["--host-codec"])
        assert dev.returncode == 0 and host.returncode == 0, (dev.stderr, host.stderr)
        outs = ["o.fastq"] if len(inputs) == 1 else ["o_1.fastq", "o_2.fastq"]
        for o in outs:
            assert (d_dev / o).read_bytes() == (d_host / o).read_bytes() != b"", (name, o)
        assert log_body(d_dev / "x.log") == log_body(d_host / "x.log")
        assert json_stable(d_dev / "x.json")[:2] == json_stable(d_host / "x.json")[:2]
        lines = [ln for ln in dev.stderr.decode().splitlines() if "gzip input" in ln]
        assert len(lines) == len(inputs) and all("on the device: taken, 3 members proved" in ln for ln in lines), dev.stderr.decode()
        assert not [ln for ln in host.stderr.decode().splitlines() if "gzip input" in ln]
    bad = tmp_path / "bad.fastq.gz"
    bad.write_bytes(files[0].read_bytes() + b"bytes behind the last member\n")
    dev, _ = _extract(tmp_path, "bad-dev", [bad], [])
    host, _ = _extract(tmp_path, "bad-host", [bad], ["--host-codec"])
    assert dev.returncode == host.returncode != 0
    mine = lambda p: [ln for ln in p.stderr.decode().splitlines() if not ln.startswith("[timing]")]
    assert mine(dev) == mine(host)
