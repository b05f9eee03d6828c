"""mk_gzip_stream_*: a gzip file inflated on the device window by window -- the compressed bytes go up a window at a time, a window
ends at the last block start that is proved, the 32 KiB of text in front of the next one are carried on the device, an open member's
CRC-32 and length are folded across windows.  The files are those of tests/gunzip_members_cases.py and tests/gunzip_windows_cases.py,
zlib is the checker (test_gunzip_windows_cpu.py shows that what is expected of a file here is what zlib says about it): a file comes
back with zlib's text and zlib's number of members, or it is handed back (state 2) -- never with another text, and what was delivered
before a hand-back is zlib's prefix of that length.  Both piece decoders, cuts every 4 KiB, windows of 16, 64 and 256 KiB."""
import pytest

import deflate_craft as craft
import gunzip_members_cases as gm
import gunzip_windows_cases as gw
from merkurio_amd import native as mk

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
    return gw.verdicts()


def stream(codec, blob, window):
    """-> (the windows' texts joined, state the stream ended in, its stats)"""
    parts = list(codec.gunzip_stream(blob, window))
    stats = codec.stream_stats
    if stats is not None:
        assert stats["text_bytes"] == sum(len(p) for p in parts)  # exact, whatever the end
        assert stats["windows"] == len(parts)
    return b"".join(parts), codec.stream_state, stats


def check(codec, verdicts, name, blob, expect, window):
    text, ok, members = verdicts[name]
    got, state, stats = stream(codec, blob, window)
    print(name, window, expect, "-> state", state, len(got), "of", len(text), stats)
    assert state in (1, 2), name
    assert got == text[:len(got)], (name, window)  # never another text; before a hand-back: zlib's prefix
    if state == 1:
        assert ok and got == text and stats["members"] == members and stats["consumed_bytes"] == len(blob), (name, window, stats)
    if expect == "taken":
        assert state == 1, (name, window, stats)
    elif expect == "handed-back":
        assert state == 2 and not ok, (name, window, stats)
    return got, state, stats


def test_every_file_of_several_members_at_each_window(codec, verdicts):
    """every case of gunzip_members_cases.py through the stream: zlib's verdict, taken files whole with zlib's number of members"""
    assert len(gm.cases()) >= 40
    for window in gw.WINDOWS:
        for name, blob, expect in gm.cases():
            check(codec, verdicts, name, blob, expect, window)
    assert list(codec.gunzip_stream(b"no gzip file\n" * 5, 16384)) == [] and codec.stream_state == 2
    assert list(codec.gunzip_stream(b"", 16384)) == [] and codec.stream_state == 2


def test_one_member_of_fastq_in_many_windows(codec, verdicts):
    """~2 MB of stream, one member: six windows at least at 256 KiB, zlib's text; at 16 KiB a window without a block start grows"""
    blob, expect = gw.files()["fastq-one-member-2mb"]
    for window in gw.WINDOWS:
        got, state, stats = check(codec, verdicts, "fastq-one-member-2mb", blob, expect, window)
        if window == 256 << 10:
            assert stats["windows"] >= 6, stats
        if window == 16 << 10:
            assert stats["windows_grown"] > 0, stats
        assert stats["members"] == 1


def test_context_across_cuts(codec, verdicts):
    """matches just under 32 KiB back into the window before; pieces shorter than 32 KiB (Z_SYNC_FLUSH every 3 KiB of text) whose
    place-holders travel through several pieces into the carry; read names that copy the previous one, back to the file's first bytes"""
    for name in ("far-matches", "sync-flush-every-3k", "names-copy-the-previous"):
        blob, expect = gw.files()[name]
        for window in gw.WINDOWS:
            got, state, stats = check(codec, verdicts, name, blob, expect, window)
            if window == 16 << 10:
                assert stats["windows"] >= 4, (name, stats)


def test_members_and_windows(codec, verdicts):
    """a member boundary inside a window; a header that straddles a window's upload end; empty members first, in the middle and last;
    a member of many windows between two of one piece; false headers in stored blocks on both sides of the cuts"""
    names = ["member-boundary-inside-a-window", "header-straddles-the-upload-end-16k", "header-straddles-the-upload-end-64k", "empty-members-among-long-ones",
             "many-windows-between-two-of-one-piece", "false-headers-on-both-sides-of-the-16k-cut", "false-headers-on-both-sides-of-the-64k-cut"]
    for name in names:
        blob, expect = gw.files()[name]
        for window in gw.WINDOWS:
            check(codec, verdicts, name, blob, expect, window)
    got, state, stats = stream(codec, gw.files()["many-windows-between-two-of-one-piece"][0], 64 << 10)
    assert stats["members"] == 3 and stats["windows"] >= 6, stats
    got, state, stats = stream(codec, gw.files()["empty-members-among-long-ones"][0], 16 << 10)
    assert stats["members"] == 6, stats


def test_hand_backs_deliver_zlibs_prefix(codec, verdicts):
    """a bit flipped in window 3 of 8, a wrong CRC-32 or ISIZE in the last trailer, bytes behind the last member: state 2 at that window
    or at the end, the text before it is zlib's prefix, `text bytes delivered` is exact (stream())"""
    whole = verdicts["fastq-one-member-2mb"][0]
    for name in ("bit-flipped-in-window-3-of-8", "last-crc-wrong", "last-isize-wrong", "bytes-behind-the-last-member"):
        blob, expect = gw.files()[name]
        for window in (64 << 10, 256 << 10):
            got, state, stats = check(codec, verdicts, name, blob, expect, window)
            assert got == whole[:len(got)] and len(got) < len(whole), name
            if name.startswith("bit-flipped") and window == 256 << 10:
                assert 1 <= stats["windows"] <= 3, stats  # windows 1 and 2 stand, the damage lies in window 3
            if not name.startswith("bit-flipped"):
                assert stats["windows"] >= (5 if window == 256 << 10 else 20), (name, stats)  # (the end is where it shows)


def test_a_distance_in_front_of_a_continued_member_is_refused(codec, verdicts):
    """28 000 bytes of text, the first 16 KiB window is cut inside them; behind the cut a match of 27 000 (inside the member's text, in
    the carry: taken) or of 32 000 (in front of the member's first byte, where the carry holds nothing -- or, behind another member,
    that member's zeros: refused, as zlib refuses it)"""
    f = gw.files()
    got, state, stats = check(codec, verdicts, "match-reaches-the-members-early-text", *f["match-reaches-the-members-early-text"], 16 << 10)
    assert stats["windows"] >= 2, stats  # (the match was resolved through the carry)
    for name in ("match-reaches-in-front-of-a-continued-member", "match-reaches-in-front-behind-another-member"):
        got, state, stats = check(codec, verdicts, name, *f[name], 16 << 10)
        assert stats["windows"] >= 1 and 0 < len(got) < 28000 + 50000, (name, stats)
        check(codec, verdicts, name, *f[name], 256 << 10)


def test_device_memory_is_bounded_by_the_window(codec, verdicts):
    """the same text at 1x and at 4x the length, the same window: the same peak of device bytes (a condition, not a measurement)"""
    peaks = []
    for name in ("fastq-one-member-quarter", "fastq-one-member-2mb"):
        got, state, stats = check(codec, verdicts, name, *gw.files()[name], 256 << 10)
        assert stats["windows_grown"] == 0, stats
        peaks.append(stats["peak_device_bytes"])
    assert len(gw.files()["fastq-one-member-2mb"][0]) > 3.5 * len(gw.files()["fastq-one-member-quarter"][0])
    assert peaks[0] == peaks[1] > 0, peaks


def test_the_one_shot_calls_work_after_a_stream(codec, verdicts):
    blob, _ = gw.files()["fastq-one-member-quarter"]
    text = verdicts["fastq-one-member-quarter"][0]
    assert stream(codec, blob, 64 << 10)[1] == 1
    name, case, _ = [c for c in gm.cases() if c[0] == "fastq-3-members-level-6"][0]
    assert codec.gunzip_members(case) == verdicts[name][::2]
    assert codec.gunzip(blob) == text
    # a stream that is left open is closed by the handle's release of the text
    L = mk.load()
    import numpy as np
    src = np.frombuffer(blob, dtype=np.uint8)
    taken = mk.C.c_uint32(0)
    assert L.mk_gzip_stream_begin(codec._h, src.ctypes.data, src.size, 65536, mk.C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_gzip_inflate_device(codec._h, src.ctypes.data, src.size, mk.C.byref(mk.C.c_uint64(0)), mk.C.byref(taken)) == mk.MK_E_INVALID_ARG
    assert L.mk_gzip_text_release(codec._h) == 0
    assert codec.gunzip(blob) == text
