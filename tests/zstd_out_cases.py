"""What the tests of the zstd frame writer share (test_zstd_deflate_cpu.py: zstd_enc_serial.hpp on the host; test_gpu_zstd_deflate.py:
mk_zstd_deflate_records on the device): libzstd frame by frame through ctypes, the cut rule restated, the shape of a written frame."""
import ctypes

import numpy as np

import zstd_cases as zc

GRID, TEXT_MAX = 114688, 131072
REACH = TEXT_MAX - GRID


def frames_by_libzstd(blob):
    """[(frame bytes, its text)]: every frame found by ZSTD_findFrameCompressedSize and decoded ALONE by ZSTD_decompress"""
    z = zc.lib()
    z.ZSTD_findFrameCompressedSize.restype = ctypes.c_size_t
    z.ZSTD_findFrameCompressedSize.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    out, at = [], 0
    dst = ctypes.create_string_buffer(TEXT_MAX + 8)
    while at < len(blob):
        rest = blob[at:]
        k = z.ZSTD_findFrameCompressedSize(rest, len(rest))
        assert not z.ZSTD_isError(k), "no frame at byte %d" % at
        r = z.ZSTD_decompress(dst, len(dst), rest[:k], k)
        assert not z.ZSTD_isError(r), "libzstd refuses the frame at byte %d" % at
        out.append((rest[:k], dst.raw[:r]))
        at += k
    return out


def rule(ends):
    """the cut rule in Python: 0, snap(k * GRID) for every grid point below the text's end, the end; distinct"""
    ends = np.asarray(ends, dtype=np.uint64)
    total = int(ends[-1]) if ends.size else 0
    cuts = [0]
    for x in range(GRID, total, GRID):
        e = int(ends[np.searchsorted(ends, x, side="left")])
        cuts.append(e if e - x < REACH else x)
    cuts.append(total)
    return sorted(set(cuts))


def shape(frame):
    """of a frame of this writer: block type (0 raw, 1 rle, 2 compressed), and for a compressed block the literals type (0 raw, 1 rle,
    2 huffman), their size format, their count, the sequence count and the three table modes (LL, OF, ML: 0 predefined, 1 rle, 2 fse)"""
    assert frame[:5] == b"\x28\xb5\x2f\xfd\xa4", frame[:5]
    bh = int.from_bytes(frame[9:12], "little")
    assert bh & 1, "Last_Block"
    out = {"block": bh >> 1 & 3, "size": bh >> 3, "text": int.from_bytes(frame[5:9], "little")}
    assert len(frame) == 16 + (1 if out["block"] == 1 else out["size"])
    if out["block"] != 2:
        return out
    p = 12
    lt, fmt = frame[p] & 3, frame[p] >> 2 & 3
    if lt < 2:
        hdr = 1 if fmt in (0, 2) else 2 if fmt == 1 else 3
        regen = int.from_bytes(frame[p:p + hdr], "little") >> (3 if hdr == 1 else 4)
        p += hdr + (regen if lt == 0 else 1)
    else:
        hdr, w = (3, 10) if fmt < 2 else (4, 14) if fmt == 2 else (5, 18)
        v = int.from_bytes(frame[p:p + hdr], "little") >> 4
        regen, comp = v & ((1 << w) - 1), v >> w
        p += hdr + comp
    b0 = frame[p]
    if b0 < 128:
        n_seq, p = b0, p + 1
    elif b0 < 255:
        n_seq, p = ((b0 - 128) << 8) + frame[p + 1], p + 2
    else:
        n_seq, p = int.from_bytes(frame[p + 1:p + 3], "little") + 0x7F00, p + 3
    modes = (frame[p] >> 6, frame[p] >> 4 & 3, frame[p] >> 2 & 3) if n_seq else None
    out.update(lit=lt, lit_format=fmt, n_lit=regen, n_seq=n_seq, modes=modes)
    if modes and modes[0] == 2:
        out["ll_log"] = (frame[p + 1] & 15) + 5  # the accuracy log of the first described table
    return out


def match_free_bytes(n, symbols=128, seed=3):
    """n bytes below `symbols`, uniform, in which no three bytes occur twice: all literals to any parser"""
    import random
    rng = random.Random(seed)
    out, seen = bytearray(), set()
    while len(out) < n:
        b = rng.randrange(symbols)
        gram = bytes(out[-2:]) + bytes([b])
        if len(gram) == 3 and gram in seen:
            continue
        seen.add(gram)
        out.append(b)
    return bytes(out)


def quad_units(k):
    """k units of one byte four times; the byte steps by an odd d for 256 units, then by the next odd d, so that no byte follows another
    twice (k <= 32 768).  A unit is one sequence to a parser with a minimum match of three, however it finds it (the run inside the
    unit, or an earlier unit of the same byte, where the match ends with the unit: what followed then differs): k sequences in 4 k bytes"""
    out, cur = bytearray(), 0
    for i in range(k):
        cur = (cur + 2 * (i // 256) + 1) % 256
        out += bytes([cur]) * 4
    return bytes(out)


def far_offset_text():
    """131 071 bytes, the most a frame holds (a grid point snaps to a record end less than 16 384 bytes behind it): xyz, zeros, xyz.  The
    last three bytes can only be a match at offset 131 068 -- offset + 3 = 2^17 - 1, offset code 16 with all of its 16 extra bits set, the
    widest field this writer's frames can hold (code 17 would need a frame of 131 072 bytes)"""
    return b"xyz" + b"\0" * (TEXT_MAX - 7) + b"xyz"
