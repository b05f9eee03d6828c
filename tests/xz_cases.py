"""The .xz files of the xz tests: valid() -> {name: (blob, text)}, damaged() -> {name: blob}, handed_back() -> {name: (blob, text, status)}.
Crafted ones come from xz_craft.py (explicit packets, chosen control bytes), real-encoder payloads from lzma.compress(FORMAT_RAW).
The checker is liblzma through the stdlib's lzma module: liblzma_says()."""
import functools
import lzma
import os
import random
import re
import subprocess

import xz_craft as craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel's buffer edges, read from its header (not retyped)
_EDGES = dict((k, int(v)) for k, v in re.findall(r"constexpr uint32_t (kXz\w+) = (\d+);", open(os.path.join(ROOT, "merkurio_amd/csrc/codec/xz_kernel_edges.h")).read()))
REFILL_BYTES, LIT_STAGE, RING = 4 * _EDGES["kXzRefillDwords"], _EDGES["kXzLitStage"], _EDGES["kXzRing"]

# statuses (xz_plan.hpp, lzma_serial.hpp)
XZ_CHECK_KIND, XZ_FILTER, XZ_SPREAD = -12, -13, -17


def liblzma_says(blob):
    """the text liblzma makes of blob read as concatenated streams with Stream Padding (LZMA_CONCATENATED, what the CLI's host path asks
    for), or None where it refuses: every stream through lzma.LZMADecompressor, the padding rule of the format between them"""
    out, data = [], bytes(blob)
    if not data:
        return None
    while data:
        d = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
        try:
            out.append(d.decompress(data))
        except lzma.LZMAError:
            return None
        if not d.eof:
            return None
        data = d.unused_data
        pad = len(data) - len(data.lstrip(b"\0"))
        if pad % 4:
            return None
        data = data[pad:]
    return b"".join(out)


def fastq(n, seed=5):
    rng = random.Random(seed)
    return b"".join(b"@read%d lane=%d\n%s\n+\n%s\n" % (i, i % 8, bytes(rng.choices(b"ACGT", k=150)), bytes(rng.choices(b"FFFF:,#", k=150)))
                    for i in range(n))


def rnd(n, seed=3):
    return random.Random(seed).randbytes(n)


def lits(data):
    return [("lit", b) for b in data]


def raw(text, preset=6, dict_size=1 << 20, **kw):
    f = {"id": lzma.FILTER_LZMA2, "preset": preset, "dict_size": dict_size}
    f.update(kw)
    return lzma.compress(text, format=lzma.FORMAT_RAW, filters=[f])


def real_block(text, kind, **kw):
    return craft.block(raw(text, **kw), text, kind), len(text)


def _crafted(name, build, kind=4, dict_size=1 << 20, **kw):
    w = craft.Lzma2Writer()
    build(w)
    data, text = w.end()
    blob, _ = craft.single(data, text, kind, dict_size=dict_size, **kw)
    return blob, text


def _props(lc, lp, pb):
    def build(w):
        w.lzma(lits(rnd(70, lc + lp)) + [("match", 5, 7), ("lit", 65), ("rep", 0, 3), ("lit", 66), ("shortrep",), ("lit", 67), ("match", 12, 33), ("lit", 1)] + lits(rnd(20, 9)),
               0xE0, (lc, lp, pb))
    return build


def _lengths(w):
    p = lits(rnd(300, 11))
    for n in (2, 9, 10, 17, 18, 272, 273):
        p += [("match", n, 200), ("lit", n & 0xFF), ("rep", 0, n), ("lit", 7)]
    w.lzma(p, 0xE0, (3, 0, 2))


def _distances(w):
    """256 KiB stored, then one match in each slot class; every match is followed by a matched literal"""
    for k in range(4):
        w.stored(rnd(65536, 20 + k), k == 0)
    p = []
    for d in (1, 2, 3, 4):
        p += [("match", 4, d), ("lit", 0x55)]
    for slot in list(range(4, 14)) + [14, 20]:
        p += [("match", 3 + slot % 3, ((2 | slot & 1) << ((slot >> 1) - 1)) + 1 + (slot % 2)), ("lit", slot)]
    p += [("match", 8, 8), ("lit", 2), ("match", 9, 8), ("lit", 3), ("match", 273, 1), ("lit", 4), ("match", 6, 1 << 18), ("lit", 5)]
    w.lzma(p, 0xC0, (3, 0, 2))


def _dict_4k(w):
    """a distance that reaches exactly the block's first byte, which is also exactly the dictionary size (4 KiB); then, further on, the
    dictionary size again"""
    w.stored(rnd(4096, 31), True)
    w.lzma([("match", 10, 4096), ("lit", 9)] + lits(rnd(900, 32)) + [("match", 20, 4096), ("lit", 1)], 0xC0, (3, 0, 2))


def _reps(w):
    p = lits(rnd(64, 41))
    for d in (10, 20, 30, 40):
        p += [("match", 3, d), ("lit", d)]
    kinds = [("rep", 0, 4), ("rep", 1, 5), ("rep", 2, 11), ("rep", 3, 19), ("shortrep",)]
    for k in kinds:  # from a state below 7 (three literals in front)
        p += lits(b"xyz") + [k, ("lit", 0x41)]
    for k in kinds:  # from a state of 7 and more (a match in front)
        p += [("match", 3, 17), k, ("lit", 0x42)]
    for k in kinds:  # a rep behind a rep, a rep behind a short rep
        p += [("rep", 1, 2), k, ("shortrep",), k, ("lit", 0x43)]
    w.lzma(p, 0xE0, (3, 0, 2))


def _turns(w):
    p = lits(rnd(200, 51))
    pos = 200
    for off in (0, 1, 63):
        for n in (63, 64, 65, 127, 128, 129):
            while pos % 64 != off:
                p.append(("lit", pos & 0xFF))
                pos += 1
            p += [("match", n, 70), ("lit", 0x30 + off)]
            pos += n + 1
            p += [("match", n, 150)]  # (dist >= len too)
            pos += n
    w.lzma(p, 0xE0, (3, 0, 2))


def _literal_runs(w):
    p = lits(rnd(10, 61))
    for n in (63, 64, 65, 127, 128, 129):
        p += [("match", 4, 3)] + lits(rnd(n, n))
    p += [("match", 5, 2)]
    w.lzma(p, 0xE0, (3, 0, 2))


def _ring_edges(w):
    """match sources that start on, before and behind the ring's reach, and dist + len on, before and behind the ring's size"""
    p = lits(rnd(64, 71))
    w.stored(rnd(2 * RING, 72), True)
    for edge in (LIT_STAGE, REFILL_BYTES, RING):
        for dist in (edge - 1, edge, edge + 1):
            p += [("match", 5, dist), ("lit", dist & 0xFF), ("match", 70, dist), ("lit", 1)]
    for total in (RING - 1, RING, RING + 1):
        for n in (2, 40, 273):
            p += [("match", n, total - n), ("lit", n & 0xFF)]
    p += [("lit", 1)] * 3 + [("match", 2, RING + 1), ("lit", 8), ("shortrep",), ("lit", 9)]  # a far matched literal, a far short rep
    w.lzma(p, 0xC0, (3, 0, 2))


def _chunk_edges(w):
    """chunk boundaries in the text on, one before and one behind each edge (0x80 continuations), and control bytes that stand on, one
    before and one behind a refill granule of the compressed bytes (stored chunks sized for it; the payload starts at file byte 24)"""
    pos, first = 0, True
    for edge in (LIT_STAGE, REFILL_BYTES, RING):
        for at in (edge - 1, edge, edge + 1):
            while at <= pos:
                at += RING
            p = lits(rnd(at - pos - 9, at)) + [("match", 9, 5)] if at - pos > 9 else lits(rnd(at - pos, at))
            w.lzma(p, 0xE0 if first else 0x80, (3, 0, 2))
            pos, first = at, False
    for want in (REFILL_BYTES - 1, 0, 1):
        n = (want - (24 + len(w.out) + 3)) % REFILL_BYTES
        w.stored(rnd(n + REFILL_BYTES, want), False)
        assert (24 + len(w.out)) % REFILL_BYTES == want
        w.lzma(lits(rnd(30, want)) + [("match", 30, 12)], 0x80)


def _stored_only(w):
    w.stored(rnd(1000, 81), True).stored(rnd(77, 82), False)


def _mixed_chunks(w):
    w.lzma(lits(rnd(100, 83)) + [("match", 20, 50)], 0xE0, (3, 0, 2))
    w.stored(rnd(300, 84), False)
    w.lzma([("match", 30, 350), ("lit", 3)] + lits(rnd(50, 85)), 0x80)  # (state and probabilities live on across the stored chunk)
    w.lzma([("match", 7, 100), ("lit", 1)] + lits(rnd(50, 86)), 0xA0)  # state reset
    w.lzma(lits(rnd(90, 87)) + [("match", 7, 100), ("lit", 1)], 0xC0, (0, 4, 1))  # new props: lc + lp 3 -> 4
    w.lzma(lits(rnd(90, 88)) + [("match", 7, 100), ("lit", 1)], 0xC0, (1, 0, 0))  # and down to 1
    w.stored(rnd(40, 89), True)  # dictionary reset by a stored chunk: the next LZMA chunk must bring props
    w.lzma(lits(rnd(40, 90)) + [("match", 7, 60), ("lit", 1)], 0xC0, (2, 2, 2))
    w.lzma(lits(rnd(40, 91)) + [("match", 7, 30), ("lit", 1)], 0xE0, (3, 0, 2))  # dictionary reset by an LZMA chunk


def _stored_64k(w):
    w.stored(rnd(65536, 92), True).stored(rnd(5, 93), False)


def _zeros_2m(w):
    n = 2 << 20
    p = [("lit", 0)] + [("match", 273, 1)] * ((n - 1) // 273)
    p.append(("match", n - 1 - 273 * ((n - 1) // 273), 1))
    w.lzma(p, 0xE0, (3, 0, 2))


@functools.lru_cache(maxsize=None)
def valid():
    v = {}
    for lc, lp, pb in ((3, 0, 2), (0, 0, 0), (4, 0, 0), (0, 4, 4), (2, 2, 2), (1, 3, 0)):
        v["props-%d-%d-%d" % (lc, lp, pb)] = _crafted("props", _props(lc, lp, pb))
    v["lengths"] = _crafted("lengths", _lengths)
    v["distances"] = _crafted("distances", _distances, kind=1, dict_size=1 << 18)
    v["dict-4k"] = _crafted("dict-4k", _dict_4k, dict_size=4096)
    v["reps"] = _crafted("reps", _reps)
    v["turns"] = _crafted("turns", _turns, kind=1)
    v["literal-runs"] = _crafted("literal-runs", _literal_runs, kind=0)
    v["ring-edges"] = _crafted("ring-edges", _ring_edges, sizes=True)
    v["chunk-edges"] = _crafted("chunk-edges", _chunk_edges)
    v["stored-only"] = _crafted("stored-only", _stored_only)
    v["mixed-chunks"] = _crafted("mixed-chunks", _mixed_chunks, header_pad=1)
    v["stored-65536"] = _crafted("stored-65536", _stored_64k, kind=1)
    v["chunk-2MiB-zeros"] = _crafted("chunk-2MiB-zeros", _zeros_2m, kind=1, dict_size=4096)
    text = fastq(700)
    for n in (1, 63, 64, 65, 4097):
        v["text-%d" % n] = (craft.stream([real_block(text[:n], 4)], 4)[0], text[:n])
    v["empty"] = (craft.stream([], 4)[0], b"")
    v["empty-block"] = (craft.stream([real_block(b"", 1)], 1)[0], b"")
    for name, preset in (("preset-0", 0), ("preset-6", 6), ("preset-9e", 9 | lzma.PRESET_EXTREME)):
        v[name] = (craft.stream([real_block(text, 4, preset=preset)], 4)[0], text)
    v["liblzma-own-container"] = (lzma.compress(text[:50000]), text[:50000])
    with open(os.path.join(ROOT, "tests", "golden", "data", "sample.fasta.xz"), "rb") as f:  # written by the xz tool itself: its header, Index and padding choices
        golden = f.read()
    with open(os.path.join(ROOT, "tests", "golden", "data", "sample.fasta"), "rb") as f:
        v["golden-sample-fasta-xz"] = (golden, f.read())
    a, b = text[:30000], text[30000:70000]
    for pad in (0, 4, 8):
        v["two-streams-pad-%d" % pad] = (craft.stream([real_block(a, 4)], 4)[0] + b"\0" * pad + craft.stream([real_block(b, 1)], 1)[0] + b"\0" * pad, a + b)
    v["mixed-checks"] = (b"".join(craft.stream([real_block(text[k * 5000:(k + 1) * 5000], kind)], kind)[0] for k, kind in enumerate((0, 1, 4, 1, 0))), text[:25000])
    rng = random.Random(7)
    cuts = sorted(rng.sample(range(1, len(text)), 39))
    parts = [text[i:j] for i, j in zip([0] + cuts, cuts + [len(text)])]
    v["40-blocks"] = (craft.stream([(craft.block(raw(p), p, 4, sizes=k % 2 == 0), len(p)) for k, p in enumerate(parts)], 4)[0], text)
    many = fastq(900, 8)[:3000 * 64]
    v["3000-blocks"] = (craft.stream([real_block(many[k * 64:(k + 1) * 64], 1, preset=0) for k in range(3000)], 1)[0], many)
    return v


def flip(b, bit):
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


def _base():
    """one stream of two real-encoder blocks, sizes in the headers, CRC-64: what most damaged files are made of"""
    text = fastq(120)
    a, b = text[:20000], text[20000:]
    return craft.stream([(craft.block(raw(a), a, 4, sizes=True), len(a)), (craft.block(raw(b), b, 4, sizes=True), len(b))], 4), a, b


def _bad_chunk(build, **kw):
    return _crafted("damaged", build, **kw)[0]


@functools.lru_cache(maxsize=None)
def damaged():
    (blob, lay), a, b = _base()
    b0 = lay["blocks"][0]
    d = {}
    places = {"stream-header": 7, "block-header": b0["at"] + 1, "payload-early": b0["payload"] + 8, "payload-middle": (b0["payload"] + b0["padding"]) // 2,
              "payload-last": b0["padding"] - 2, "check": b0["check"] + 3, "index": lay["index"] + 2, "footer": lay["footer"] + 5}
    for name, at in places.items():
        d["flip-" + name] = flip(blob, at * 8 + 2)
        d["cut-" + name] = blob[:at]
    d["trailing-bytes"] = blob + b"xz"
    d["trailing-zeros-not-a-multiple-of-4"] = blob + b"\0\0"
    ra = craft.block(raw(a), a, 4, sizes=True), len(a)
    d["index-stored-size-off-by-one"] = craft.stream([ra], 4, index_delta=(1, 0))[0]
    d["index-text-size-off-by-one"] = craft.stream([ra], 4, index_delta=(0, 1))[0]
    d["index-text-size-one-short"] = craft.stream([(craft.block(raw(a), a, 4), len(a))], 4, index_delta=(0, -1))[0]
    d["backward-size-wrong"] = craft.stream([ra], 4, backward_delta=1)[0]
    odd = next(t for t in (a[:n] for n in range(19000, 19040)) if len(raw(t)) % 4)  # (a payload whose length leaves block padding to damage)
    d["block-padding-not-zero"] = craft.stream([(craft.block(raw(odd), odd, 4, pad_byte=1), len(odd))], 4)[0]
    pre = lits(rnd(100, 1))
    d["distance-one-past-the-text"] = _bad_chunk(lambda w: w.lzma(pre + [("match", 4, 101), ("lit", 1)], 0xE0, (3, 0, 2)))
    d["shortrep-at-the-first-byte"] = _bad_chunk(lambda w: w.lzma([("shortrep",), ("lit", 1)], 0xE0, (3, 0, 2)))
    d["distance-one-past-the-dictionary"] = _bad_chunk(lambda w: (w.stored(rnd(5000, 2), True), w.lzma([("match", 4, 4097), ("lit", 1)], 0xC0, (3, 0, 2))), dict_size=4096)
    d["chunk-states-one-byte-less"] = _bad_chunk(lambda w: w.lzma(pre + [("match", 4, 9)], 0xE0, (3, 0, 2), usize_delta=-1))
    d["chunk-states-one-byte-more"] = _bad_chunk(lambda w: w.lzma(pre + [("match", 4, 9)], 0xE0, (3, 0, 2), usize_delta=1))

    def patched(build, patch):
        w = craft.Lzma2Writer()
        build(w)
        patch(w)
        data, text = w.end()
        return craft.single(data, text, 4)[0]

    ok = lambda w: w.lzma(pre + [("match", 4, 9), ("lit", 3)], 0xE0, (3, 0, 2))

    def final_code(w):
        w.out[w.chunks[0][1] + w.chunks[0][2] - 1] ^= 1

    def first_byte(w):
        w.out[w.chunks[0][1]] = 1

    def control_3(w):
        w.out[w.chunks[1][0]] = 3

    def props_5(w):
        w.out[w.chunks[0][1] - 1] = (2 * 5 + 2) * 9 + 3  # lc 3, lp 2

    d["final-code-not-zero"] = patched(ok, final_code)
    d["first-range-coder-byte-not-zero"] = patched(ok, first_byte)
    d["control-byte-0x03"] = patched(lambda w: (ok(w), w.stored(b"abc", False)), control_3)
    d["lc-plus-lp-5"] = patched(ok, props_5)
    d["first-chunk-without-dictionary-reset"] = _bad_chunk(lambda w: w.stored(b"abcdef", False))
    d["first-lzma-chunk-without-props"] = _bad_chunk(lambda w: (w.stored(b"abcdef", True), w.lzma(lits(b"abc"), 0xA0)))
    d["end-of-payload-marker"] = _bad_chunk(lambda w: w.lzma(pre + [("match", 2, 1 << 32)], 0xE0, (3, 0, 2), usize_delta=-2))
    d["end-of-payload-marker-mid-chunk"] = _bad_chunk(lambda w: w.lzma(pre + [("match", 2, 1 << 32), ("match", 3, 5)], 0xE0, (3, 0, 2), usize_delta=-2))
    return d


@functools.lru_cache(maxsize=None)
def handed_back():
    """valid files this path leaves to liblzma: {name: (blob, text, status)}"""
    text = fastq(60)
    x86 = lzma.compress(text, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 6}])
    delta = lzma.compress(text, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_DELTA, "dist": 4}, {"id": lzma.FILTER_LZMA2, "preset": 6}])
    lz = (0x21, bytes([craft.dict_byte(8 << 20)]))
    return {
        "sha-256": (craft.stream([real_block(text, 10)], 10)[0], text, XZ_CHECK_KIND),
        "liblzma-sha-256": (lzma.compress(text, check=lzma.CHECK_SHA256), text, XZ_CHECK_KIND),
        "x86-bcj": (craft.stream([(craft.block(x86, text, 4, filters=[(0x04, b""), lz]), len(text))], 4)[0], text, XZ_FILTER),
        "delta": (craft.stream([(craft.block(delta, text, 4, filters=[(0x03, b"\x03"), lz]), len(text))], 4)[0], text, XZ_FILTER),
    }


def blocks_of(sizes, seed=9):
    """one stream of real-encoder blocks of these text sizes -> (blob, text)"""
    text = fastq(sum(sizes) // 300 + 2, seed)[:sum(sizes)]
    parts, at = [], 0
    for s in sizes:
        parts.append(text[at:at + s])
        at += s
    return craft.stream([real_block(p, 4) for p in parts], 4)[0], text


def build_harness(work_dir, sanitize):
    exe = os.path.join(str(work_dir), "xz_harness")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(ROOT, "tests/helpers/xz_harness.cpp")], check=True)
    return exe


def run_harness(exe, work_dir, blob, spread=1):
    """-> (the report's fields, the text written)"""
    src, out = os.path.join(str(work_dir), "in.xz"), os.path.join(str(work_dir), "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, src, out, str(spread)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    rep = dict(f.split("=") for f in p.stdout.split())
    with open(out, "rb") as f:
        return rep, f.read()
