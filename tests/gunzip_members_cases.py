"""Files of several gzip members for test_gunzip_members_cpu.py (the host's guess walker and zlib's verdict on every file) and
test_gpu_gunzip_members.py (mk_gzip_members_inflate_device on the same files).  zlib is the checker: members are written by zlib, or
by tests/deflate_craft.py where a compressor would never write them, and what a file's text is -- or that it has none -- is what
zlib says (zlib_text), walking the members as the reference's reader does.

A case is (name, file, expect): "taken" (the device must take it: zlib's text, as many members as zlib walks), "handed-back"
(zlib refuses the file: the device must not take it) or "either" (taken with zlib's text, or not taken)."""
import random
import struct
import zlib

import deflate_craft as craft

EMPTY = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3, 3, 0]) + bytes(8)  # `gzip < /dev/null`: a final fixed block of nothing but its end


def zlib_walk(blob):
    """-> (text, members) as zlib reads the file member by member, or (None, 0) where zlib refuses it (bytes that are no member included)"""
    out, members, data = [], 0, bytes(blob)
    if not data:
        return None, 0
    while data:
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(data))
        except zlib.error:
            return None, 0
        if not d.eof:
            return None, 0
        members, data = members + 1, d.unused_data
    return b"".join(out), members


def fastq(n, seed):
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        s = "".join(rnd.choices("ACGT", k=150))
        q = "".join(rnd.choices("FFFF:,#", k=150))
        out.append(f"@read{seed}.{i} lane={i % 8}\n{s}\n+\n{q}\n")
    return "".join(out).encode()


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **header):
    """one gzip member around zlib's stream of `text`"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return craft.gzip_member(co.compress(text) + co.flush(), text, **header)


def stored_member(text):
    """a member whose stream is stored blocks: `text` lies in the file verbatim"""
    return craft.gzip_member(craft.stream(craft.stored_run(text) if text else [craft.stored(b"")]), text)


def _cases():
    out = []
    small = [fastq(40 + 7 * k, 100 + k) for k in range(17)]  # 13-50 KB of text each
    for n in (2, 3, 17):
        for level in (1, 6, 9):
            out.append((f"fastq-{n}-members-level-{level}", b"".join(member(t, level) for t in small[:n]), "taken"))
    out.append(("members-of-one-byte", member(b"A") + member(b"\n", 1) + stored_member(b"\xff"), "taken"))
    a, b = member(small[0]), member(small[1], 9)
    out.append(("empty-member-first", EMPTY + a + b, "taken"))
    out.append(("empty-member-in-the-middle", a + EMPTY + b, "taken"))
    out.append(("empty-member-last", a + b + EMPTY, "taken"))
    out.append(("only-empty-members", EMPTY * 3, "taken"))
    out.append(("stored-fixed-and-dynamic-members", member(small[2], 0) + member(small[3], 6, zlib.Z_FIXED) + member(small[4], 6) + member(small[5], 1, zlib.Z_FIXED)
                + stored_member(small[6][:3000]), "taken"))
    out.append(("every-optional-header-field", member(small[0], fextra=b"AB\x03\x00xyz", fname=b"lane1.fastq", fcomment=b"a comment", fhcrc=True)
                + member(small[1], fname=b"lane2.fastq") + member(small[2], fhcrc=True), "taken"))
    # ~200 KB of stream (a piece can be no smaller than a block of zlib's: half a dozen pieces) between two members of one piece
    big = fastq(2000, 7)
    mid = member(big, 6)
    assert 150_000 < len(mid) < 300_000
    out.append(("a-member-of-many-pieces-between-two-of-one", member(small[0][:6000]) + mid + member(small[1][:6000], 1), "taken"))
    # a member whose text begins with runs and far matches into its own first bytes -- behind another member's text, where "in front
    # of the member" and "in front of the file" are different things
    runs = craft.stream([craft.fixed([0x41] + [(258, 1)] * 6 + [0x43, 0x47, (258, 3), (200, 1500), (3, 1549 + 258 + 200)])])
    runs_text, _ = craft.verdict(runs)
    assert runs_text is not None and runs_text.startswith(b"A" * 1549)
    out.append(("text-that-begins-with-matches-into-its-own-first-bytes", member(small[0]) + craft.gzip_member(runs, runs_text) + member(bytes(3000) + small[1], 9)
                + member(b"A" * 70000 + small[2], 9), "taken"))
    for name, gz, text, _ in craft.gunzip_streams():  # every hand-made stream of several pieces zlib takes, as a middle member
        if text is not None:
            out.append((f"hand-made-{name}-in-the-middle", member(small[3]) + gz + member(small[4], 1), "taken"))
    # the context restarts: a match that reaches in front of member k + 1's first byte finds member k's text there in a reader that
    # carries its window on -- 33 000 zeros, which is what the hand-made members' trailers were computed with.  zlib refuses.
    zeros_last = member(small[5] + bytes(33000))
    for name, gz, text, _ in craft.gunzip_streams():
        if text is None:
            out.append((f"context-restarts-{name}", zeros_last + gz + member(small[6]), "handed-back"))
    reach = [craft.fixed([(10, 5), 0x42, 0x0a])]
    out.append(("context-restarts-first-token", a + craft.gzip_member(craft.stream(reach), craft.render(reach, before=small[0])) + b, "handed-back"))
    # false guesses: whole, valid gzip members as the TEXT of a stored block -- headers that parse, streams that decode, trailers that agree
    fake1, fake2 = member(small[7][:5000]), member(small[8][:4000], 1)
    out.append(("false-guess-a-whole-member-in-a-stored-block", stored_member(fake1) + b, "taken"))
    out.append(("false-guess-two-whole-members-back-to-back", stored_member(fake1 + fake2) + b, "taken"))
    out.append(("false-guess-two-whole-members-apart", stored_member(fake1 + small[9][:700] + fake2 + b"tail\n") + b, "taken"))
    # ID1 ID2 CM as the last three bytes of a payload: the trailer's first byte is then read as FLG.  A text whose CRC-32 begins with
    # a byte that passes for one (no reserved bits, no optional fields) makes the walker guess a member there
    planted = next(small[9][:900 + k] + b"\x1f\x8b\x08" for k in range(5000) if zlib.crc32(small[9][:900 + k] + b"\x1f\x8b\x08") & 0xfe == 0)
    out.append(("false-guess-magic-bytes-end-a-payload", stored_member(planted) + b + a, "either"))
    out.append(("false-guess-magic-bytes-inside-a-payload", stored_member(small[9][:900] + b"\x1f\x8b\x08\x00" + small[9][900:2000]) + b, "either"))
    # handed back: zlib refuses every one of these
    three = [member(small[10]), member(small[11], 1), member(small[12], 9)]
    ok = b"".join(three)
    out.append(("three-members-as-they-are", ok, "taken"))
    out.append(("trailing-garbage", ok + b"garbage behind the last member\n", "handed-back"))
    out.append(("trailing-zeros", ok + bytes(16), "handed-back"))  # (zlib says "incorrect header check"; a reader that allows padding is lenient)
    bad = bytearray(ok)
    bad[-6] ^= 0x40
    out.append(("last-crc-flipped", bytes(bad), "handed-back"))
    isize_at = len(three[0]) + len(three[1]) - 4
    out.append(("middle-isize-off-by-one", ok[:isize_at] + struct.pack("<I", len(small[11]) + 1) + ok[isize_at + 4:], "handed-back"))
    out.append(("middle-member-truncated-by-one-byte", three[0] + three[1][:-1] + three[2], "handed-back"))
    out.append(("middle-member-stream-one-byte-short", three[0] + three[1][:-9] + three[1][-8:] + three[2], "handed-back"))
    bad = bytearray(ok)
    bad[len(three[0]) // 2] ^= 0x04
    out.append(("damaged-bit-in-the-first-member", bytes(bad), "handed-back"))
    out.append(("bytes-between-a-stream-and-its-trailer", three[0][:-8] + b"\0\0\0" + three[0][-8:] + three[1], "handed-back"))
    out.append(("one-member-twice", three[0] * 2, "taken"))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES
