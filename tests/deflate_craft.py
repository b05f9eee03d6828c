"""Hand-made DEFLATE streams (RFC 1951) and the members that carry them (RFC 1952, BGZF), bit by bit -- what no compressor here
writes: the corners of the format that are legal but outside zlib's dialect (`ok-`), and streams that are illegal although their
trailer agrees with what a lenient decoder would write (`bad-`).  The judge is zlib (`verdict`): the module checks at import that
every name's prefix is zlib's verdict, so a slip in a builder fails here and cannot turn a corner case into an ordinary one.

A stream is a list of blocks -- stored(...), fixed(...), dynamic(...) -- given to stream().  Tokens of a compressed block:
    an int                     a literal byte
    (length, distance)         a match
    ("ll", symbol, extra, n)   a raw literal / length symbol with n extra bits of value `extra` (symbols 286 / 287 ...)
    ("d", symbol, extra, n)    a raw distance symbol (30 / 31 ...)
    ("bits", value, n)         n raw bits, first bit of the stream lowest (a codeword that no symbol owns)
Literal filler belongs in stored blocks (a byte copy), the tokens under test in a short compressed block behind it.
Used by test_codec_cpu.py and test_gpu_codec_streams.py; plain Python, nothing but zlib / struct."""
import struct
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
# a complete code over all 19 code-length symbols: thirteen codewords of 4 bits, six of 5
CL_FLAT = [4] * 13 + [5] * 6
# complete codes over the whole alphabets: 286 literal / length symbols in 8 / 9 bits, 30 distance symbols in 4 / 5
LL_FLAT = [8] * 226 + [9] * 60
D_FLAT = [4] * 2 + [5] * 28


class BitWriter:
    """bits of the stream, first bit lowest; whole bytes leave the accumulator as they fill"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        assert 0 <= value < (1 << count) or count == 0 and value == 0, (value, count)
        self.acc |= value << self.n
        self.n += count
        if self.n >= 512:
            whole = self.n >> 3
            self.out += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.n -= 8 * whole

    def align(self):
        self.bits(0, -self.n % 8)

    def raw(self, data):
        assert self.n % 8 == 0
        self._spill()
        self.out += data

    def _spill(self):
        whole = self.n >> 3
        self.out += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
        self.acc >>= 8 * whole
        self.n -= 8 * whole

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        self.align()
        self._spill()
        return bytes(self.out)


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: (codeword as it enters the stream -- its most significant bit first, i.e. bit-reversed --, length)}
    of the symbols whose length is not 0"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for sym, l in enumerate(lens):
        if l:
            out[sym] = (int(format(nxt[l], "0%db" % l)[::-1], 2), l)
            nxt[l] += 1
    return out


def length_symbol(length):
    assert 3 <= length <= 258
    idx = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + idx, length - LEN_BASE[idx], LEN_EXTRA[idx]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    idx = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return idx, dist - DIST_BASE[idx], DIST_EXTRA[idx]


# ---- blocks ------------------------------------------------------------------------------------------------------------------------
def stored(data=b"", final=None, nlen=None):
    """one stored block (at most 65 535 bytes); nlen: a complement that is not one"""
    assert len(data) <= 65535
    return {"type": 0, "data": bytes(data), "final": final, "nlen": nlen}


def stored_run(data, piece=65535):
    """as many stored blocks as `data` needs"""
    return [stored(data[i:i + piece]) for i in range(0, len(data), piece)]


def fixed(tokens, final=None, eob=True):
    return {"type": 1, "tokens": list(tokens), "final": final, "eob": eob}


def dynamic(ll_lens, d_lens, tokens, final=None, eob=True, code_length_symbols=None, cl_lens=None, hclen=None, hlit=None, hdist=None,
            bad_header=False):
    """a dynamic block.  ll_lens / d_lens: code lengths by symbol (as many as are sent: HLIT / HDIST follow from the lists unless
    given).  code_length_symbols: the run-length coded lengths as the header spells them -- a list of (symbol, extra value) of
    the code-length alphabet, by default every length sent on its own; cl_lens: the 19 lengths of the code-length code (default: a
    complete code over all of them); hclen: how many of those are sent (default: up to the last one that is not 0, at least 4);
    bad_header: the builder's word that the header is illegal (written() stops in front of such a block)"""
    return {"type": 2, "ll": list(ll_lens), "d": list(d_lens), "tokens": list(tokens), "final": final, "eob": eob,
            "cls": code_length_symbols, "cl_lens": list(cl_lens or CL_FLAT), "hclen": hclen, "hlit": hlit, "hdist": hdist, "bad_header": bad_header}


def reserved_block(final=None):
    """block type 3"""
    return {"type": 3, "final": final}


def _tokens(w, ll, d, tokens, eob):
    for t in tokens:
        if isinstance(t, int):
            w.bits(*ll[t])
        elif t[0] == "ll":
            w.bits(*ll[t[1]])
            w.bits(t[2], t[3])
        elif t[0] == "d":
            w.bits(*d[t[1]])
            w.bits(t[2], t[3])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        else:
            sym, extra, n = length_symbol(t[0])
            w.bits(*ll[sym])
            w.bits(extra, n)
            sym, extra, n = distance_symbol(t[1])
            w.bits(*d[sym])
            w.bits(extra, n)
    if eob:
        w.bits(*ll[256])


def write_block(w, b, final):
    w.bits(1 if final else 0, 1)
    w.bits(b["type"], 2)
    if b["type"] == 0:
        w.align()
        n = len(b["data"])
        w.bits(n, 16)
        w.bits((n ^ 0xffff) if b["nlen"] is None else b["nlen"], 16)
        w.raw(b["data"])
    elif b["type"] == 1:
        _tokens(w, canonical(FIXED_LL), canonical(FIXED_D), b["tokens"], b["eob"])
    elif b["type"] == 2:
        ll_lens, d_lens, cl_lens = b["ll"], b["d"], b["cl_lens"]
        w.bits((len(ll_lens) if b["hlit"] is None else b["hlit"]) - 257, 5)
        w.bits((len(d_lens) if b["hdist"] is None else b["hdist"]) - 1, 5)
        hclen = b["hclen"] or max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        cl = canonical(cl_lens)
        cls = b["cls"] if b["cls"] is not None else [(l, 0) for l in ll_lens + d_lens]
        for sym, extra in cls:
            w.bits(*cl[sym])
            w.bits(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
        _tokens(w, canonical(ll_lens), canonical(d_lens), b["tokens"], b["eob"])


def stream(blocks, tail=b""):
    """the blocks as one raw DEFLATE stream; the last block is the final one unless the blocks say otherwise; tail: bytes behind it"""
    return stream_and_starts(blocks, tail)[0]


def stream_and_starts(blocks, tail=b""):
    """-> (stream, [bit position of every block's first bit])"""
    w = BitWriter()
    starts = []
    for i, b in enumerate(blocks):
        starts.append(w.bit_length())
        write_block(w, b, (i == len(blocks) - 1) if b["final"] is None else b["final"])
    return w.getvalue() + tail, starts


def render(blocks, before=b"", strict=False):
    """the text of the blocks (or of a bare token list) under a LENIENT reading: a match may reach in front of the stream, where
    `before` lies -- zeros, or a neighbour's text (what the bytes in front of it are is the reader's guess: zeros where `before`
    ends).  Only used to make trailers that agree with what a decoder without the distance check would write.
    strict: the text a strict reader has written when it stops -- in front of the first illegal block, raw token or match that
    reaches in front of the stream"""
    if blocks and not isinstance(blocks[0], dict):
        blocks = [fixed(blocks)]
    room = 32768 + 258
    buf = bytearray(room - min(room, len(before))) + bytearray(before[-room:])
    for b in blocks:
        if strict and (b["type"] == 3 or b.get("bad_header") or b.get("nlen") is not None):
            break
        if b["type"] == 0:
            buf += b["data"]
            continue
        for t in b["tokens"]:
            if isinstance(t, int):
                buf.append(t)
            else:
                if strict and (isinstance(t[0], str) or t[1] > len(buf) - room):
                    return bytes(buf[room:])
                length, dist = t  # (raw escapes have no text)
                if dist >= length:
                    buf += buf[len(buf) - dist:len(buf) - dist + length]
                else:
                    pat = bytes(buf[len(buf) - dist:])
                    buf += (pat * (length // dist + 1))[:length]
    return bytes(buf[room:])


def written(blocks):
    """what a strict reader (zlib) has written when it refuses the stream, or when the stream's bytes end"""
    return render(blocks, strict=True)


# ---- zlib's verdict, members ---------------------------------------------------------------------------------------------------------
def verdict(raw):
    """-> (text, unused bytes) if zlib inflates the raw stream to its end without an error, else (None, what it handed out
    before it stopped: a prefix of what it had written -- WRITTEN holds all of that, by the builder's count)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error:
        return None, written_before_zlib_stops(raw)
    if not d.eof:
        return None, written_before_zlib_stops(raw)
    return out, len(d.unused_data)


def written_before_zlib_stops(raw):
    """zlib hands out nothing of a call that fails, so the text is drawn a byte per call: the call that meets the error can keep
    back one token's bytes at most"""
    d = zlib.decompressobj(-15)
    out, data = bytearray(), raw
    try:
        while not d.eof:
            piece = d.decompress(data, 1)
            if not piece and d.unconsumed_tail == data:
                break
            out += piece
            data = d.unconsumed_tail
            if not piece and not data:
                break
    except zlib.error:
        pass
    return bytes(out)


def bgzf_member(raw, text):
    """18-byte BGZF header + stream + CRC-32 + ISIZE of `text` (which need not be what the stream inflates to).  BSIZE is a 16-bit
    field: a stream of more than 65 510 bytes (stored blocks of 64 KiB of text) does not fit it -- such a member can only be named by
    an explicit member table (data_off = 18 behind the member's first byte, data_len = len(raw)), its BSIZE is cut to 16 bits"""
    return bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", (len(raw) + 25) & 0xffff) + raw + \
        struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def gzip_member(raw, text, fextra=None, fname=None, fcomment=None, fhcrc=False, flg_extra=0):
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0) | flg_extra
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff])
    if fextra is not None:
        head += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        head += fname + b"\0"
    if fcomment is not None:
        head += fcomment + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


# ---- one gzip stream in pieces: dynamic blocks of a little over 4 KiB of compressed bytes (cuts every 4 KiB find each of them) --------
GUNZIP_CHUNK = 4096


def piece(head=(), literals=4300, seed=0, tail=(), alphabet=None):
    """a dynamic block with complete codes over both alphabets (what the block-start search believes): `head` tokens, `literals`
    bytes of noise (from `alphabet` if given), `tail` tokens"""
    fill = noise(literals, 1000 + seed)
    if alphabet:
        fill = bytes(alphabet[b % len(alphabet)] for b in fill)
    return dynamic(LL_FLAT, D_FLAT, list(head) + list(fill) + list(tail))


def runs_to(total, literals=4300):
    """tail tokens that bring a piece of `literals` bytes to exactly `total` bytes of text: runs of the last byte"""
    rest, out = total - literals, []
    while rest:
        n = 258 if rest >= 261 or rest == 258 else min(rest, 255) if rest > 258 else rest  # (never leaves 1 or 2 bytes over)
        out.append((n, 1))
        rest -= n
    return out


def expected_pieces(blocks, starts, n_in, chunk=GUNZIP_CHUNK):
    """how many pieces the block-start search cuts the stream into, at least: a wave per nominal chunk takes the first start in its
    range, and a start is a non-final, non-empty dynamic block with complete codes followed by a dynamic or a stored block"""
    n_chunks = max(1, n_in // chunk)
    windows = set()
    for i in range(1, len(blocks) - 1):
        b, nxt = blocks[i], blocks[i + 1]
        if b["type"] != 2 or not b["tokens"] or nxt["type"] not in (0, 2) or starts[i] + 64 > n_in * 8:
            continue
        k = min(starts[i] // (8 * chunk), n_chunks - 1)
        if k >= 1:
            windows.add(k)
    return 1 + len(windows)


def _gunzip_streams():
    """-> [(name, gzip member, zlib's text or None, pieces at least)]"""
    out = []

    def add(name, blocks, **header):
        blocks = blocks + [dynamic(LL_FLAT, D_FLAT, [0x0a])]  # (a short final block: no start is searched in it)
        raw, starts = stream_and_starts(blocks)
        text, _ = verdict(raw)
        assert (text is not None) == name.startswith("ok-"), name
        for a, b in zip(starts[1:], starts[2:]):
            assert b - a > 8 * GUNZIP_CHUNK, (name, "a block of less than 4 KiB")
        trailer_text = text if text is not None else render(blocks)  # (bad-: the trailer of the lenient reading, zeros in front)
        if text is None:
            assert trailer_text != written(blocks)
        out.append((name, gzip_member(raw, trailer_text, **header), text, expected_pieces(blocks, starts, len(raw))))

    front = [piece(seed=k) for k in range(8)]  # 34 400 bytes of text in eight pieces
    add("ok-piece-starts-with-258-32768", front + [piece([(258, 32768)], seed=8), piece(seed=9)])
    add("ok-piece-starts-with-a-run", [piece(seed=10), piece([(258, 1)], seed=11), piece([(258, 1), (3, 1)], seed=12)])
    add("ok-match-overlaps-out-of-the-context", [piece(seed=13), piece([(100, 40)], seed=14), piece([(258, 7), (258, 3)], seed=15)])
    # the first three bytes of the text, copied on by the first token of every piece: a place-holder that is resolved through
    # eleven maps, every piece shorter than 32 KiB (4 303 bytes: the match's distance)
    add("ok-bytes-carried-through-twelve-pieces", [piece(seed=16)] + [piece([(3, 4300 if k == 0 else 4303)], seed=17 + k) for k in range(11)]
        + [piece(seed=29)])
    sizes = []
    for k, total in enumerate((32767, 32768, 32769)):
        sizes += [piece(seed=30 + 2 * k, tail=runs_to(total)), piece([(258, 32768), (258, 32768), (9, 32767)], seed=31 + 2 * k)]
    add("ok-pieces-of-32767-32768-32769-bytes", [piece(seed=36)] + sizes + [piece(seed=37)])
    add("ok-text-of-0xff-0x80", [piece(seed=40, alphabet=b"\xff\x80")] + [piece([(258, 4000), (100, 1)], seed=41 + k, alphabet=b"\xff\x80\xff\xfe\x7f")
                                                                          for k in range(9)] + [piece(seed=50, alphabet=b"\x80")])
    add("ok-header-with-every-optional-field", [piece(seed=51), piece([(258, 1)], seed=52), piece([(3, 4000)], seed=53)],
        fextra=b"AB\x03\x00xyz", fname=b"reads.fastq", fcomment=b"a comment", fhcrc=True)
    add("bad-piece-0-starts-in-front-of-byte-0", [piece([(10, 4)], seed=60), piece(seed=61), piece(seed=62)])
    add("bad-piece-1-reaches-byte-0-through-place-holders", [piece(literals=5120, seed=63), piece([(3, 32768)], seed=64), piece(seed=65)])
    add("bad-place-holder-copied-on-through-three-pieces", [piece(literals=5120, seed=66), piece([(3, 32768)], seed=67)]
        + [piece([(3, 4303)], seed=68 + k) for k in range(3)] + [piece(seed=71)])
    return out


_GUNZIP = None


def gunzip_streams():
    global _GUNZIP
    if _GUNZIP is None:
        _GUNZIP = _gunzip_streams()
    return _GUNZIP


# ---- ring and flush edges of the wave-per-member decoders ---------------------------------------------------------------------------
def ring_edge_members(ring):
    """-> [(label, raw stream, text)]: one member per combination of a match's distance, its length and where its first byte falls --
    one byte in front of, on, and one byte behind a multiple of 4 096 (the flush unit) and of `ring` (the bytes of text a wave keeps
    in LDS) --, stored blocks of noise in front, the match the last token: it ends on the member's last byte"""
    dists = sorted(d for d in {1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, ring - 258, ring - 257, ring - 1, ring, ring + 1, 32768} if 1 <= d <= 32768)
    fill = noise(66000, 7)
    out = []
    for unit in sorted({4096, ring}):
        for delta in (-1, 0, 1):
            for dist in dists:
                pos = max(1, -(-(dist - delta) // unit)) * unit + delta  # the first multiple of unit (+ delta) that `dist` bytes lie in front of
                for length in (3, 4, 63, 64, 65, 257, 258):
                    if pos + length > 65536:  # (a BGZF member's text: 64 KiB at most -- distance 32 768 where the position allows it)
                        continue
                    off = (dist * 7 + length) % 400
                    blocks = stored_run(fill[off:off + pos]) + [fixed([(length, dist)])]
                    raw = stream(blocks)
                    text, unused = verdict(raw)
                    assert text is not None and unused == 0 and len(text) == pos + length
                    out.append(("unit %d%+d dist %d len %d" % (unit, delta, dist, length), raw, text))
    return out


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------
def noise(n, seed=1):
    """n bytes that do not repeat within 32 KiB and take values on both sides of 0x80: a wrong source byte shows"""
    out = bytearray(n)
    x = (seed * 2654435761 + 12345) & 0xffffffff
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        out[i] = (x >> 24) ^ (i & 0xff) ^ ((i >> 8) * 37 & 0xff)
    return bytes(out)


def _ll_only(symbols):
    """code lengths 0 but for `symbols`: {symbol: length}"""
    lens = [0] * (max(symbols) + 1 if max(symbols) >= 257 else 257)
    for s, l in symbols.items():
        lens[s] = l
    return lens


def _catalogue():
    cat = []

    def ok(name, blocks, tail=b""):
        cat.append(("ok-" + name, stream(blocks, tail), None))

    def bad(name, blocks, lenient=False):
        cat.append(("bad-" + name, stream(blocks), render(blocks) if lenient else None))
        WRITTEN["bad-" + name] = written(blocks)

    lit4 = _ll_only({65: 2, 66: 2, 67: 2, 256: 2})  # A B C end-of-block: a complete code without any length symbol
    ok("stored-empty-final", [stored()])
    ok("stored-0-then-65535", [stored(), stored(noise(65535, 2))])
    ok("fixed-literal-then-runs", [fixed([0x41, (258, 1), (258, 1), (3, 1)])])
    ok("fixed-match-to-byte-0", [fixed([0x80, 0xfe, 0x03, (258, 3)])])
    ok("fixed-three-blocks-last-empty", [fixed([1, 2, 3]), fixed([(3, 3), 0xff]), fixed([])])
    ok("fixed-distance-32768-twice", stored_run(noise(32768, 3)) + [fixed([(258, 32768), (258, 32768)])])
    ok("dynamic-no-distance-code", [dynamic(lit4, [0], [65, 66, 67, 67, 66])])
    ok("dynamic-one-1-bit-distance-code", [dynamic(_ll_only({65: 1, 256: 2, 257: 2}), [1], [65, (3, 1), 65])])
    # lengths 1, 2, ..., 14, 15, 15: a complete code whose last two codewords are 15 bits long
    ramp = {s: l for s, l in zip((256, 0x80, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 0xff, 257), list(range(1, 16)) + [15])}
    ok("dynamic-lengths-1-to-15", [dynamic(_ll_only(ramp), [1, 1], [0xff, 76, 0x80, 65, (3, 2), 0xff, 0xff, (3, 1), 75])])
    ok("dynamic-only-end-of-block", [dynamic(_ll_only({256: 1}), [0], [])])
    ok("dynamic-hlit-286-hdist-30", [dynamic(LL_FLAT, D_FLAT, list(noise(600, 4)) + [(258, 1), (3, 600), (258, 599), (285 - 200, 24), (4, 17)])])
    ok("valid-then-four-bytes", [fixed([0x41, 0x80, (5, 2)])], tail=b"\xde\xad\xbe\xef")
    # a repeat (symbol 16) whose run begins at the last literal / length length and ends among the distance lengths: HLIT 258,
    # lengths 257 .. 260 of the sequence = ll[257] d[0] d[1] d[2] -- "2, then repeat the previous length 3 times"
    ll = _ll_only({65: 1, 256: 2, 257: 2})
    cls = [(l, 0) for l in ll[:257]] + [(2, 0), (16, 1)]
    assert len(ll) == 258
    ok("dynamic-repeat-crosses-into-distances", [dynamic(ll, [2, 2, 2, 2], [65, (3, 1), 65, (3, 3), (3, 2), (3, 4)], code_length_symbols=cls)])
    # HCLEN 5, the smallest count that can carry a block: the lengths of 16 17 18 0 8 are sent, so a code length is 0 or 8 -- 256
    # codewords of 8 bits (literals 0 .. 254 and the end-of-block code) are a complete code.  (HCLEN 4 sends 16 17 18 0 alone: every
    # code length is then 0, no end-of-block codeword exists and zlib refuses the block: bad-dynamic-hclen-4 below)
    cl5 = [0] * 19
    cl5[0], cl5[8], cl5[16], cl5[17] = 1, 2, 3, 3
    ok("dynamic-hclen-5-smallest-usable", [dynamic([8] * 255 + [0, 8], [0], [0, 0x7f, 0x80, 0xfe, 0x41], cl_lens=cl5)])
    cl18 = [0] * 19
    cl18[18], cl18[1], cl18[0] = 1, 2, 2   # 18: 1 bit; lengths 1 and 0: 2 bits
    # code-length symbol 18 with 138 zeros (literals 0 .. 137), 18 again with 62, literal 200, 18 with 55, the end-of-block code
    ll = _ll_only({200: 1, 256: 1})
    cls = [(18, 127), (18, 62 - 11), (1, 0), (18, 55 - 11), (1, 0), (0, 0)]
    assert 138 + 62 + 1 + 55 + 1 == 257
    ok("dynamic-18-with-138-zeros", [dynamic(ll, [0], [200, 200], code_length_symbols=cls, cl_lens=cl18)])

    bad("stored-len-nlen-mismatch", [stored(b"abc", nlen=0x1234)])
    bad("block-type-3", [fixed([65]), reserved_block()])
    bad("fixed-match-first", [fixed([(3, 1), 65])], lenient=True)
    bad("fixed-3-literals-then-10-4", [fixed([0x41, 0x80, 0xff, (10, 4), 0x42])], lenient=True)
    bad("fixed-length-symbol-286", [fixed([65, ("ll", 286, 0, 0), ("d", 0, 0, 0)])])
    bad("fixed-distance-symbol-30", [fixed([65, 66, 67, ("ll", 257, 0, 0), ("d", 30, 0, 0)])])
    bad("fixed-no-end-of-block", [fixed([65, 66, 67, 68, 0x80], eob=False)])
    bad("dynamic-length-without-distance-code", [dynamic(_ll_only({65: 1, 256: 2, 257: 2}), [0], [65, ("ll", 257, 0, 0), ("bits", 0, 1)])])
    bad("dynamic-unassigned-distance-codeword", [dynamic(_ll_only({65: 1, 256: 2, 257: 2}), [1], [65, ("ll", 257, 0, 0), ("bits", 1, 1)])])
    bad("dynamic-oversubscribed-literal-code", [dynamic(_ll_only({65: 1, 66: 1, 256: 1}), [0], [], bad_header=True)])
    bad("dynamic-incomplete-literal-code", [dynamic(_ll_only({65: 2, 256: 2}), [0], [65], bad_header=True)])
    bad("dynamic-no-end-of-block-code", [dynamic(_ll_only({65: 1, 66: 1, 256: 0}), [0], [65, 66], eob=False, bad_header=True)])
    ll = _ll_only({65: 1, 256: 1})
    bad("dynamic-repeat-16-first", [dynamic(ll, [0], [65], code_length_symbols=[(16, 0)] + [(l, 0) for l in ll[3:]] + [(0, 0)], bad_header=True)])
    bad("dynamic-repeat-past-the-lengths", [dynamic(ll, [0], [65], code_length_symbols=[(l, 0) for l in ll] + [(17, 0)], bad_header=True)])
    cl4 = [0] * 19
    cl4[16] = cl4[17] = cl4[18] = cl4[0] = 2
    bad("dynamic-hclen-4", [dynamic(ll, [0], [65], code_length_symbols=[(18, 127), (18, 120 - 11)], cl_lens=cl4, bad_header=True)])
    bad("dynamic-hlit-287", [dynamic(LL_FLAT + [0], D_FLAT, [65], bad_header=True)])
    bad("dynamic-hdist-31", [dynamic(LL_FLAT, D_FLAT + [0], [65], bad_header=True)])
    incomplete = [0] * 19
    incomplete[0], incomplete[1] = 1, 2
    bad("dynamic-incomplete-code-length-code", [dynamic(ll, [0], [65], cl_lens=incomplete, bad_header=True)])
    return cat


WRITTEN = {}  # name of a bad- stream -> the text a strict reader has written when it stops
CATALOGUE = _catalogue()


def _check_catalogue():
    names = set()
    for name, raw, lenient in CATALOGUE:
        assert name not in names, name
        names.add(name)
        text, rest = verdict(raw)
        assert (text is not None) == name.startswith("ok-"), (name, "zlib's verdict differs from the name's")
        assert name.startswith(("ok-", "bad-"))
        if text is None:
            wrote = WRITTEN[name]
            assert wrote.startswith(rest) and len(wrote) - len(rest) <= 258, (name, rest, wrote)  # (zlib keeps back one token at most)
            if lenient is not None:
                assert lenient.startswith(wrote) and len(lenient) > len(wrote), name  # (the lenient reading goes on where zlib stops)


_check_catalogue()
