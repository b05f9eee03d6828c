"""The .zst files of test_unzstd_cpu.py (zstd_serial.hpp and zstd_plan.hpp on the host) and test_gpu_unzstd.py (the same code on a
wave per block): valid files that must be taken, damaged ones that must be handed back.  libzstd (the system's libzstd.so.1, what the
CLI's host path binds) writes and checks them through ctypes; what no compressor can be made to emit comes from zstd_craft.py."""
import ctypes
import ctypes.util
import functools
import os
import random
import struct
import subprocess

import zstd_craft as craft

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
C_LEVEL, C_WINDOW_LOG, C_CONTENT_SIZE, C_CHECKSUM = 100, 101, 200, 201
E_CONTINUE, E_FLUSH, E_END = 0, 1, 2


class _Buf(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


@functools.lru_cache(maxsize=None)
def lib():
    z = ctypes.CDLL(ctypes.util.find_library("zstd") or "libzstd.so.1")
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf), ctypes.POINTER(_Buf), ctypes.c_int]
    z.ZSTD_compressStream2.restype = ctypes.c_size_t
    z.ZSTD_createDStream.restype = ctypes.c_void_p
    z.ZSTD_freeDStream.argtypes = [ctypes.c_void_p]
    z.ZSTD_decompressStream.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf), ctypes.POINTER(_Buf)]
    z.ZSTD_decompressStream.restype = ctypes.c_size_t
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    return z


def compress(text, level=3, checksum=False, window_log=0, pieces=None, content_size=True):
    """one frame; pieces: the text in these parts with a flush behind each (a flush ends a block; the frame then has no content size)"""
    z = lib()
    c = z.ZSTD_createCCtx()
    for param, value in ((C_LEVEL, level), (C_CHECKSUM, int(checksum)), (C_WINDOW_LOG, window_log), (C_CONTENT_SIZE, int(content_size))):
        assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(c, param, value))
    parts = pieces if pieces is not None else [text]
    dst = ctypes.create_string_buffer(z.ZSTD_compressBound(len(text)) + 64 * len(parts) + 64)
    ob = _Buf(ctypes.cast(dst, ctypes.c_void_p), len(dst), 0)
    for k, part in enumerate(parts):
        src = ctypes.create_string_buffer(bytes(part), len(part))
        ib = _Buf(ctypes.cast(src, ctypes.c_void_p), len(part), 0)
        op = E_END if k == len(parts) - 1 else E_FLUSH
        while True:
            r = z.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(ib), op)
            assert not z.ZSTD_isError(r)
            if r == 0 and ib.pos == ib.size:
                break
    z.ZSTD_freeCCtx(c)
    return dst.raw[:ob.pos]


def libzstd_says(blob):
    """the text ZSTD_decompressStream makes of blob the way the CLI's host path drives it, or None where it refuses or the data ends early"""
    z = lib()
    d = z.ZSTD_createDStream()
    src = ctypes.create_string_buffer(bytes(blob), len(blob))
    ib = _Buf(ctypes.cast(src, ctypes.c_void_p), len(blob), 0)
    room = ctypes.create_string_buffer(1 << 20)
    out, last = [], 0
    try:
        if len(blob) < 4:
            return None
        while ib.pos < ib.size or last != 0:
            ob = _Buf(ctypes.cast(room, ctypes.c_void_p), len(room), 0)
            before = ib.pos
            last = z.ZSTD_decompressStream(d, ctypes.byref(ob), ctypes.byref(ib))
            out.append(room.raw[:ob.pos])
            if z.ZSTD_isError(last) or (ib.pos == before and ob.pos == 0 and ib.pos >= ib.size):
                return None
        return b"".join(out)
    finally:
        z.ZSTD_freeDStream(d)


def fastq(n, seed=5):
    rng = random.Random(seed)
    return b"".join(b"@read%d lane=%d\n%s\n+\n%s\n" % (i, i % 8, bytes(rng.choices(b"ACGT", k=150)), bytes(rng.choices(b"FFFF:,#", k=150)))
                    for i in range(n))


def match_free_text(n, seed=77):
    """n skewed bytes of a 64-symbol alphabet in which no three bytes occur twice: no compressor finds a match, so the block's
    literals are the text and its Huffman coding pays"""
    rng = random.Random(seed)
    out, seen = bytearray(), set()
    syms, weights = list(range(40, 104)), [1.0 / (1 + i) ** 1.3 for i in range(64)]
    while len(out) < n:
        b = rng.choices(syms, weights=weights)[0]
        gram = bytes(out[-2:]) + bytes([b])
        if len(gram) == 3 and gram in seen:
            continue
        seen.add(gram)
        out.append(b)
    return bytes(out)


def short_matches_text(n_seq=0x8000):
    """a text of many short matches: 3-byte words drawn from 64, each followed by a fresh byte pair now and then, so that one 128 KiB
    block holds 0x7F00 sequences and more (the count is checked on the CPU)"""
    rng = random.Random(9)
    words = [bytes(rng.choices(range(256), k=3)) for _ in range(64)]
    out = bytearray()
    while len(out) < 4 * n_seq:
        out += words[rng.randrange(64)] + bytes([rng.randrange(256)])
    return bytes(out[:131072])


@functools.lru_cache(maxsize=None)
def valid():
    """name -> (file, text)"""
    rng = random.Random(23)
    fq = fastq(1300)[:400000]
    rnd = bytes(rng.getrandbits(8) for _ in range(131072))
    out = {}
    for size in (0, 1, 255, 256, 257, 131071, 131072, 131073):
        t = fq[:size]
        out["size-%d" % size] = (compress(t, 3, True), t)
    for size in (255, 256, 257):  # (the stream count goes by the LITERALS: these texts are all literals)
        t = match_free_text(size)
        out["literals-%d" % size] = (compress(t, 3, True), t)
    for level in (1, 3, 19):
        for ck in (False, True):
            out["fastq-l%d%s" % (level, "-checksum" if ck else "")] = (compress(fq, level, ck), fq)
    out["raw-block"] = (compress(rnd[:70000], 3, True), rnd[:70000])
    t = b"A" * 5000 + fq[:300] + b"C" * 70000
    out["rle-literals"] = (compress(t, 3, True), t)
    t = bytes(rng.choices(b"ACGT", k=3000)) + rnd[:900] + fq[:2000]
    out["mixed-small"] = (compress(t, 1, False), t)
    t = short_matches_text()
    out["many-sequences"] = (compress(t, 19, True), t)  # (level 19 takes matches of three bytes)
    t = bytes(rng.choices(range(8), weights=[1, 2, 4, 8, 16, 1, 2, 4], k=6000))
    out["direct-weights"] = (compress(t, 3, True), t)
    t = fq[:100] + b"G" * 70000 + fq[100:200]
    out["long-match"] = (compress(t, 19, True), t)
    t = rnd[:66000] + fq[:3000] * 3  # (what repeats pays for a compressed block around 66 000 literals)
    out["long-literals"] = (compress(t, 1, True), t)  # (level 1 finds no three-byte matches among random bytes)
    # repeat offsets at a block start: records of one length, a flush (= a block end) between them
    rec = [b"@r%04d\n%s\n+\n%s\n" % (i, bytes(rng.choices(b"ACGT", k=40)), bytes(rng.choices(b"F:,", k=40))) for i in range(400)]
    t = b"".join(rec)
    out["flushed-records"] = (compress(t, 3, True, pieces=[b"".join(rec[i:i + 25]) for i in range(0, 400, 25)]), t)
    out["flushed-records-l19"] = (compress(t, 19, False, pieces=[b"".join(rec[i:i + 7]) for i in range(0, 400, 7)]), t)
    # a match at distance exactly the window: 1 KiB window, a unit of 1 024 random bytes twice
    t = rnd[:1024] + rnd[:1024] + rnd[2000:2100]
    out["far-match"] = (compress(t, 19, True, window_log=10, pieces=[t[:1500], t[1500:]]), t)
    # chain depth 40: every block copies the one before it
    t = rnd * 40
    out["chain-40"] = (compress(t, 3, True, window_log=18), t)
    # frame forms
    out["fcs-1"] = (compress(fq[:200], 3), fq[:200])
    out["fcs-2"] = (compress(fq[:3000], 3), fq[:3000])
    out["fcs-4"] = (compress(fq[:70000], 3), fq[:70000])
    out["fcs-none"] = (compress(fq[:70000], 3, True, content_size=False), fq[:70000])
    a, b, c = compress(fq[:50000], 3, True), compress(fq[50000:140000], 19, False), compress(fq[140000:150000], 1, True)
    skip = struct.pack("<II", 0x184D2A53, 11) + b"hello world"
    out["three-frames"] = (a + b + c, fq[:150000])
    out["skippable-around"] = (skip + a + skip + b + skip, fq[:140000])
    out["empty-frame-among"] = (a + compress(b"", 3, True) + b, fq[:140000])
    with open(os.path.join(GOLDEN, "sample.fasta"), "rb") as f:
        t = f.read()
    out["golden-sample"] = (compress(t, 3, True), t)
    out.update(craft.valid())
    return out


def flip(b, bit):
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


def first_block(blob):
    """(offset of the first block header, Block_Size, type) of a file that starts with a zstd frame"""
    fhd = blob[4]
    at = 5 + (0 if fhd >> 5 & 1 else 1) + (0, 1, 2, 4)[fhd & 3] + ((fhd >> 5 & 1), 2, 4, 8)[fhd >> 6]
    bh = int.from_bytes(blob[at:at + 3], "little")
    return at, bh >> 3, bh >> 1 & 3


def sections(blob):
    """byte offsets inside the first (compressed, Huffman-coded) block of blob: literals header, tree, streams, sequences header, bitstream end"""
    at, size, typ = first_block(blob)
    assert typ == 2
    p = at + 3
    b0 = blob[p]
    assert b0 & 3 == 2
    sf = b0 >> 2 & 3
    hdr = 3 if sf < 2 else 4 if sf == 2 else 5
    w = 10 if sf < 2 else 14 if sf == 2 else 18
    v = int.from_bytes(blob[p:p + hdr], "little") >> 4
    comp = v >> w & ((1 << w) - 1)
    return {"block": at, "literals": p, "tree": p + hdr, "streams": p + hdr + comp // 2, "sequences": p + hdr + comp, "end": p + size}


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> file: every one must be handed back, and be an error to libzstd"""
    fq = fastq(300)[:60000]
    blob = compress(fq, 3, True)  # one block, content size, checksum
    s = sections(blob)
    out = {"flip-huffman-stream": flip(blob, s["streams"] * 8 + 3), "flip-sequences": flip(blob, (s["sequences"] + s["end"]) // 2 * 8 + 2),
           "flip-block-size": flip(blob, s["block"] * 8 + 9), "flip-content-size": flip(blob, 5 * 8 + 3), "flip-checksum": flip(blob, len(blob) * 8 - 5),
           "trailing-garbage": blob + b"garbage-behind-the-frame", "trailing-byte": blob + b"\n"}
    for name in ("block", "literals", "tree", "streams", "sequences", "end"):
        out["cut-at-%s" % name] = blob[:s[name]]
    out["cut-in-header"] = blob[:5]
    out["cut-in-checksum"] = blob[:-2]
    # patched headers (a frame without checksum, so that only the patched field is wrong)
    plain = compress(fq, 3, False, content_size=False)
    at, size, _ = first_block(plain)
    p = bytearray(plain)
    p[at] |= 6
    out["patched-reserved-block-type"] = bytes(p)
    out["patched-dictionary-id"] = plain[:4] + bytes([plain[4] | 1]) + plain[5:6] + b"\x07" + plain[6:]
    out["patched-window-log-28"] = plain[:5] + bytes([(28 - 10) << 3]) + plain[6:]
    out["patched-reserved-bit"] = plain[:4] + bytes([plain[4] | 8]) + plain[5:]
    out.update(craft.damaged())
    return out


PATCHED_STATUS = {"patched-reserved-block-type": -7, "patched-dictionary-id": -4, "patched-window-log-28": -5, "patched-reserved-bit": -3}


def build_harness(work_dir, sanitize):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(work_dir), "zstd_harness")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(root, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(root, "tests/helpers/zstd_harness.cpp")], check=True)
    return exe


def run_harness(exe, work_dir, blob):
    """-> (the report's fields, the text written)"""
    src, out = os.path.join(str(work_dir), "in.zst"), os.path.join(str(work_dir), "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    rep = dict(f.split("=") for f in p.stdout.split())
    with open(out, "rb") as f:
        return rep, f.read()
