"""Files for test_gunzip_windows_cpu.py (zlib's verdict on every one of them) and test_gpu_gunzip_windows.py (mk_gzip_stream_* on the
same files, window by window).  zlib is the checker, as in gunzip_members_cases.py: what a file's text is, how many members it has,
and -- for a file zlib refuses -- which text zlib hands out before it stops (zlib_prefix).

files() -> {name: (blob, expect)}, expect = "taken" (the stream must deliver zlib's text whole, state 1) or "handed-back" (zlib
refuses the file: state 2, what was delivered before is zlib's prefix)."""
import random
import struct
import zlib

import deflate_craft as craft
import gunzip_members_cases as gm

WINDOWS = (16 << 10, 64 << 10, 256 << 10)
MARGIN = 64  # bytes a window uploads behind its nominal size (codec/gzip_chain.hpp: kGzStreamMargin)
SYNC_FLUSH_EVERY = 3 << 10  # bytes of text between two Z_SYNC_FLUSH of "sync-flush-every-3k": zlib's blocks are dynamic at this interval


def zlib_prefix(blob):
    """-> (text zlib hands out before it refuses the file -- all of it for a file it reads --, whether it reads the file, members).
    The call that meets the error hands out nothing, so that call is repeated byte by byte on a copy of the reader."""
    blob = bytes(blob)
    out, pos, members = [], 0, 0
    if not blob:
        return b"", False, 0
    while pos < len(blob):
        d = zlib.decompressobj(31)
        while not d.eof:
            if pos >= len(blob):
                return b"".join(out), False, members
            chunk = blob[pos:pos + 4096]
            pos += len(chunk)
            before = d.copy()
            try:
                out.append(d.decompress(chunk))
            except zlib.error:
                try:
                    for b in chunk:
                        out.append(before.decompress(bytes([b])))
                except zlib.error:
                    pass
                return b"".join(out), False, members
        members += 1
        pos -= len(d.unused_data)
    return b"".join(out), True, members


def fastq_names(n, seed):
    """FASTQ whose every read name copies most of the previous one: a chain of matches back to the file's first bytes"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        s = "".join(rnd.choices("ACGT", k=150))
        q = "".join(rnd.choices("FFFF:,#", k=150))
        out.append(f"@A00123:45:HXXXXXXXX:1:1101:{1000 + i % 30000}:{i} 1:N:0:ACGTACGT+TGCATGCA\n{s}\n+\n{q}\n")
    return "".join(out).encode()


def far_matches(n, period=32400, seed=5):
    """every 1 024 bytes: 512 copied from `period` bytes back (zlib's farthest match is 32 506 back), 512 fresh random ones"""
    rnd = random.Random(seed)
    t = bytearray(rnd.randbytes(period))
    while len(t) < n:
        t += t[len(t) - period:len(t) - period + 512]
        t += rnd.randbytes(512)
    return bytes(t[:n])


def sync_flushed(text, every=SYNC_FLUSH_EVERY):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(co.compress(text[i:i + every]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(text), every)) + co.flush()
    return craft.gzip_member(raw, text)


def raw_part(text, last=False):
    """a raw DEFLATE stream of `text` that ends on a byte boundary without a final block (last: with one)"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(text) + (co.flush() if last else co.flush(zlib.Z_SYNC_FLUSH))


def planted_headers(parts, plant, behind):
    """one member: zlib's blocks of parts[0], zlib's blocks of parts[1], ... with a stored block whose text is `plant` behind the parts
    whose index is in `behind` -> (member, text)"""
    raw, text = b"", b""
    for k, p in enumerate(parts):
        last = k + 1 == len(parts)
        raw += raw_part(p, last)
        text += p
        if k in behind:
            raw += craft.stream([craft.stored(plant, final=False)])
            text += plant
    return craft.gzip_member(raw, text), text


def reach_in_front(distance):
    """one member: ~28 KB of text in zlib's blocks (two of them: the first window of 16 KiB is cut at the second one's start), then
    a fixed block with one match of `distance` -- inside the member's text, or in front of its first byte.
    -> (member, the text a lenient reader would write)"""
    rnd = random.Random(77)
    text = bytes(rnd.choices(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/", k=28000))
    tail = [craft.fixed([(40, distance), 0x0a])]
    raw = raw_part(text) + craft.stream(tail)
    full = text + craft.render(tail, before=text)  # (zeros stand in front of the member for the lenient reader)
    return craft.gzip_member(raw, full), full


def _files():
    out = {}
    big = gm.fastq(21000, 3)  # ~7 MB of text, ~2 MB compressed
    one = gm.member(big)
    assert 1_700_000 < len(one) < 2_600_000, len(one)
    out["fastq-one-member-2mb"] = (one, "taken")
    quarter = gm.member(gm.fastq(5250, 3))
    out["fastq-one-member-quarter"] = (quarter, "taken")
    far = far_matches(600_000)
    m = gm.member(far)
    assert len(m) < 0.62 * len(far), (len(m), len(far))  # (the copied halves went as matches)
    out["far-matches"] = (m, "taken")
    names = fastq_names(2500, 9)
    out["sync-flush-every-3k"] = (sync_flushed(names), "taken")
    out["names-copy-the-previous"] = (gm.member(fastq_names(6000, 10)), "taken")
    # members and windows
    small = [gm.fastq(40 + 7 * k, 500 + k) for k in range(4)]
    mid = gm.member(gm.fastq(2000, 7))  # ~200 KB
    out["member-boundary-inside-a-window"] = (gm.member(small[0]) + gm.member(small[1], 9) + mid + gm.member(small[2], 1), "taken")
    for w in WINDOWS[:2]:
        # member A ends 13 bytes in front of the first upload's end: B's header (10 bytes + a name) straddles it
        n = w // 100
        while len(gm.member(gm.fastq(n, 40))) >= w + MARGIN - 13 - 2:  # (~100 bytes of stream per record: A fills the window, several blocks)
            n -= 5
        t = gm.fastq(n, 40)
        a0 = gm.member(t)
        assert w - 2000 < len(a0) < w + MARGIN - 13 - 2, (w, len(a0))
        a = gm.member(t, fname=b"x" * (w + MARGIN - 13 - len(a0) - 1))
        assert len(a) == w + MARGIN - 13
        out[f"header-straddles-the-upload-end-{w >> 10}k"] = (a + gm.member(small[1], fname=b"a-name-behind-the-upload.fastq") + gm.member(small[2]), "taken")
    half = gm.member(gm.fastq(1000, 8))
    out["empty-members-among-long-ones"] = (gm.EMPTY + half + gm.EMPTY + gm.EMPTY + mid + gm.EMPTY, "taken")
    out["many-windows-between-two-of-one-piece"] = (gm.member(small[0][:6000]) + gm.member(gm.fastq(5000, 11)) + gm.member(small[1][:6000], 1), "taken")
    fake = gm.member(small[3][:3000])  # a whole valid member as text: its header parses wherever it lies
    parts = [gm.fastq(100, 600 + k) for k in range(12)]  # ~10 KB of stream each
    # two plants, ~10 KB of stream apart, around the first cut of a 16 KiB window (at ~10 and ~20 KB) and of a 64 KiB one (~60, ~70 KB):
    # one false header on each side of the cut (a window drops three false guesses at most, as the one-shot call does)
    for w, behind in ((16, {0, 1}), (64, {5, 6})):
        member, _ = planted_headers(parts, fake, behind)
        out[f"false-headers-on-both-sides-of-the-{w}k-cut"] = (member + gm.member(small[0]), "taken")
    # hand-backs
    bad = bytearray(one)
    bad[len(one) * 5 // 16] ^= 0x10  # window 3 of 8 at 256 KiB
    out["bit-flipped-in-window-3-of-8"] = (bytes(bad), "handed-back")
    bad = bytearray(one)
    bad[-7] ^= 1
    out["last-crc-wrong"] = (bytes(bad), "handed-back")
    out["last-isize-wrong"] = (one[:-4] + struct.pack("<I", (len(big) + 1) & 0xffffffff), "handed-back")
    out["bytes-behind-the-last-member"] = (one + b"bytes behind the last member\n", "handed-back")
    ok, _ = reach_in_front(27000)
    out["match-reaches-the-members-early-text"] = (ok, "taken")
    refused, _ = reach_in_front(32000)
    out["match-reaches-in-front-of-a-continued-member"] = (refused, "handed-back")
    out["match-reaches-in-front-behind-another-member"] = (gm.member(small[0] + bytes(33000)) + refused, "handed-back")
    return out


_FILES = None
_VERDICTS = None


def files():
    global _FILES
    if _FILES is None:
        _FILES = _files()
    return _FILES


def verdicts():
    """{name: zlib_prefix(blob)} of files() and of every case of gunzip_members_cases.py, computed once"""
    global _VERDICTS
    if _VERDICTS is None:
        _VERDICTS = {name: zlib_prefix(blob) for name, (blob, _) in files().items()}
        _VERDICTS.update({name: zlib_prefix(blob) for name, blob, _ in gm.cases()})
    return _VERDICTS
