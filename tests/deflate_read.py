"""A DEFLATE reader (RFC 1951) in plain Python that keeps what an inflater throws away: the blocks' headers, their code lengths and
the TOKENS -- which literals and which (length, distance) pairs the writer chose.  The counterpart of deflate_craft.py's writer: zlib
says whether a stream is valid and what it inflates to, this module says how it was spelled (tests of the device's deflate writer,
merkurio_amd/csrc/codec/bgzf_deflate.hip, compare the token list with what the kernel's parse rule promises).

read(raw) -> a list of blocks, each a dict:
    "type" 0 / 1 / 2, "final", "start" / "end" (bit positions of the block's first bit and of the bit behind its last one),
    "tokens": an int per literal, (length, distance) per match (a stored block: its bytes as literals, also under "data"),
    a dynamic block also "hlit", "hdist", "hclen", "ll" / "d" (the code lengths as sent: hlit / hdist of them) and "header_bits"
    (BFINAL up to the last code length).
render(blocks) -> the text.

The reader is strict, as zlib is: an over-subscribed code, an incomplete one (but for zlib's one exception: a literal / length or
distance code of a single 1-bit codeword), a missing end-of-block code, an unassigned codeword or symbol 286 / 287 / 30 / 31 in
use, a distance that reaches in front of the stream, a stored block whose NLEN is not LEN's complement, block type 3 and a stream
that ends inside a block raise DeflateError.  A reader that guessed would hide a writer's bugs.  Bytes behind the final block are
the caller's business (compare blocks[-1]["end"] with 8 * len(raw)).

Symbols are decoded through one table per code (2^longest-codeword entries), not bit by bit: 64 KiB of literals parse in well under a
second."""
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class DeflateError(ValueError):
    pass


def kraft(lens, unit=15):
    """the Kraft sum of a code's lengths in units of 2^-unit: 1 << unit for a complete code"""
    return sum(1 << (unit - l) for l in lens if l)


def decode_table(lens, what, lone_codeword_ok):
    """(table, mask): table[next bits of the stream & mask] = symbol << 4 | length of its codeword, 0 where no codeword matches"""
    longest = max(lens) if lens else 0
    if longest > 15:
        raise DeflateError("%s code: a length above 15" % what)
    if longest == 0:
        return [0], 0  # no codeword at all: legal as long as none is used
    k = kraft(lens)
    if k > 1 << 15:
        raise DeflateError("%s code is over-subscribed" % what)
    if k < 1 << 15 and not (lone_codeword_ok and longest == 1):
        raise DeflateError("%s code is incomplete" % what)
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    size = 1 << longest
    table = [0] * size
    for sym, l in enumerate(lens):
        if l:
            c = nxt[l]
            nxt[l] += 1
            r = int(format(c, "0%db" % l)[::-1], 2)  # the codeword as it lies in the stream: its first bit lowest
            table[r::1 << l] = [sym << 4 | l] * (size >> l)
    return table, size - 1


class _Bits:
    """the stream's bits, first bit lowest, through an accumulator that is refilled eight bytes at a time"""

    def __init__(self, raw):
        self.raw = raw
        self.at = 0       # bytes loaded
        self.acc = 0
        self.n = 0        # bits in acc
        self.pad = 0      # of them zeros from behind the stream's end

    def fill(self):
        piece = self.raw[self.at:self.at + 8]
        if piece:
            self.acc |= int.from_bytes(piece, "little") << self.n
            self.n += 8 * len(piece)
            self.at += len(piece)
        if self.n < 48:  # the stream has ended: zeros, so that a token that straddles the end is read and then refused by pos()
            if self.pad > 4096:
                raise DeflateError("the stream ends inside a block")
            self.pad += 64
            self.n += 64

    def take(self, k):
        if self.n < 48:
            self.fill()
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def pos(self):
        p = 8 * self.at + self.pad - self.n
        if p > 8 * len(self.raw):
            raise DeflateError("the stream ends inside a block")
        return p

    def to_byte(self):
        k = self.n % 8
        self.acc >>= k
        self.n -= k


def _read_lengths(b):
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise DeflateError("HLIT %d / HDIST %d" % (hlit, hdist))
    cl = [0] * 19
    for s in CL_ORDER[:hclen]:
        cl[s] = b.take(3)
    table, mask = decode_table(cl, "code-length", False)
    lens = []
    while len(lens) < hlit + hdist:
        if b.n < 48:
            b.fill()
        e = table[b.acc & mask]
        if not e:
            raise DeflateError("an unassigned code-length codeword")
        b.acc >>= e & 15
        b.n -= e & 15
        s = e >> 4
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise DeflateError("a repeat with no length in front of it")
            run, v = 3 + b.take(2), lens[-1]
        elif s == 17:
            run, v = 3 + b.take(3), 0
        else:
            run, v = 11 + b.take(7), 0
        if len(lens) + run > hlit + hdist:
            raise DeflateError("a repeat runs past the last code length")
        lens += [v] * run
    if lens[256] == 0:
        raise DeflateError("no end-of-block codeword")
    return hlit, hdist, hclen, lens[:hlit], lens[hlit:]


def _read_tokens(b, ll, d, n_text):
    """the tokens of one compressed block up to its end-of-block symbol -> (tokens, bytes of text behind them)"""
    ll_tab, ll_mask = decode_table(ll, "literal / length", True)
    d_tab, d_mask = decode_table(d, "distance", True)
    tokens = []
    put = tokens.append
    raw, total = b.raw, len(b.raw)
    acc, n, at = b.acc, b.n, b.at
    while True:
        if n < 48:
            if at < total:
                piece = raw[at:at + 8]
                acc |= int.from_bytes(piece, "little") << n
                n += 8 * len(piece)
                at += len(piece)
            if n < 48:
                b.acc, b.n, b.at = acc, n, at
                b.fill()
                b.pos()  # (raises once the block has read past the stream's end)
                acc, n, at = b.acc, b.n, b.at
        e = ll_tab[acc & ll_mask]
        if not e:
            raise DeflateError("an unassigned literal / length codeword")
        acc >>= e & 15
        n -= e & 15
        s = e >> 4
        if s < 256:
            put(s)
            continue
        if s == 256:
            break
        s -= 257
        if s > 28:
            raise DeflateError("length symbol %d" % (s + 257))
        x = LEN_EXTRA[s]
        length = LEN_BASE[s] + (acc & ((1 << x) - 1))
        acc >>= x
        n -= x
        e = d_tab[acc & d_mask]
        if not e:
            raise DeflateError("an unassigned distance codeword")
        acc >>= e & 15
        n -= e & 15
        s = e >> 4
        if s > 29:
            raise DeflateError("distance symbol %d" % s)
        x = DIST_EXTRA[s]
        dist = DIST_BASE[s] + (acc & ((1 << x) - 1))
        acc >>= x
        n -= x
        put((length, dist))
    b.acc, b.n, b.at = acc, n, at
    # distances against the text in front of each match: a second, cheap pass (the hot loop above stays small)
    for t in tokens:
        if t.__class__ is int:
            n_text += 1
        else:
            if t[1] > n_text:
                raise DeflateError("a distance of %d with %d bytes of text in front of it" % (t[1], n_text))
            n_text += t[0]
    return tokens, n_text


def read(raw):
    """every block of the raw DEFLATE stream `raw`, up to and including the final one"""
    raw = bytes(raw)
    b = _Bits(raw)
    blocks, n_text = [], 0
    while True:
        start = b.pos()
        final, btype = b.take(1), b.take(2)
        blk = {"type": btype, "final": bool(final), "start": start}
        if btype == 0:
            b.to_byte()
            n, nn = b.take(16), b.take(16)
            if n ^ nn != 0xffff:
                raise DeflateError("stored block: NLEN is not the complement of LEN")
            at = b.pos() >> 3
            if at + n > len(raw):
                raise DeflateError("the stream ends inside a stored block")
            blk["data"] = raw[at:at + n]
            blk["tokens"] = list(blk["data"])
            b.at, b.acc, b.n, b.pad = at + n, 0, 0, 0
            n_text += n
        elif btype == 1:
            blk["tokens"], n_text = _read_tokens(b, FIXED_LL, FIXED_D, n_text)
        elif btype == 2:
            blk["hlit"], blk["hdist"], blk["hclen"], blk["ll"], blk["d"] = _read_lengths(b)
            blk["header_bits"] = b.pos() - start
            blk["tokens"], n_text = _read_tokens(b, blk["ll"], blk["d"], n_text)
        else:
            raise DeflateError("block type 3")
        blk["end"] = b.pos()
        blocks.append(blk)
        if final:
            return blocks


def render(blocks):
    """the text of the blocks of read() (or of one bare token list)"""
    if blocks and not isinstance(blocks[0], dict):
        blocks = [{"tokens": blocks}]
    out = bytearray()
    for blk in blocks:
        for t in blk["tokens"]:
            if t.__class__ is int:
                out.append(t)
                continue
            length, dist = t
            if dist > len(out):
                raise DeflateError("a distance of %d with %d bytes of text in front of it" % (dist, len(out)))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                pat = bytes(out[len(out) - dist:])
                out += (pat * (length // dist + 1))[:length]
    return bytes(out)


def matches(tokens):
    return [t for t in tokens if t.__class__ is not int]


def positions(tokens):
    """[(position in the text, token)] of a token list"""
    out, at = [], 0
    for t in tokens:
        out.append((at, t))
        at += 1 if t.__class__ is int else t[0]
    return out
