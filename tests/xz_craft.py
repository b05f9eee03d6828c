"""A writer of .xz files for the tests of the device's xz path (tests/xz_cases.py): the container of the xz file format 1.0.4 -- stream
header, block headers with and without the optional sizes, block padding, Index, footer, stream padding, checks 0 / 1 / 4 / 10 -- and
a small LZMA range ENCODER that takes an explicit packet list, so that a case decides every packet the decoder meets:

    ("lit", byte)   ("match", length, distance)   ("rep", i, length)   ("shortrep",)

wrapped into LZMA2 chunks with chosen control bytes.  Nothing here is clever: the encoder mirrors the decoder of
merkurio_amd/csrc/codec/lzma_serial.hpp bit for bit, and test_unxz_cpu.py pins every file it writes to liblzma's text."""
import hashlib
import struct
import zlib

IS_MATCH, IS_REP, IS_REP_G0, IS_REP_G1, IS_REP_G2, IS_REP0_LONG, POS_SLOT, SPEC_POS, ALIGN, LEN_CODER, REP_LEN_CODER, LITERAL = (
    0, 192, 204, 216, 228, 240, 432, 688, 802, 818, 1332, 1846)


class RangeEncoder:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()

    def shift_low(self):
        if self.low < 0xFF000000 or self.low >= 1 << 32:
            carry, temp = self.low >> 32, self.cache
            while self.cache_size:
                self.out.append((temp + carry) & 0xFF)
                temp = 0xFF
                self.cache_size -= 1
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, probs, i, b):
        p = probs[i]
        bound = (self.range >> 11) * p
        if b:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        else:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.shift_low()

    def direct(self, v, n):
        for i in range(n - 1, -1, -1):
            self.range >>= 1
            if v >> i & 1:
                self.low += self.range
            while self.range < 1 << 24:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self.shift_low()

    def finish(self):
        for _ in range(5):
            self.shift_low()
        return bytes(self.out)


def slot_of(rep0):
    if rep0 < 4:
        return rep0
    n = rep0.bit_length()
    return 2 * (n - 1) + (rep0 >> (n - 2) & 1)


class Lzma2Writer:
    """the LZMA2 bytes of one block, chunk by chunk; .text is what they decode to (where every distance is valid)"""

    def __init__(self):
        self.out, self.text, self.dict_start = bytearray(), bytearray(), 0
        self.lc = self.lp = self.pb = 0
        self.probs, self.state, self.reps = [], 0, [0, 0, 0, 0]
        self.chunks = []  # (offset of the control byte, offset of the payload, payload bytes) per chunk

    def stored(self, data, reset_dict):
        assert 1 <= len(data) <= 65536
        if reset_dict:
            self.dict_start = len(self.text)
        self.chunks.append((len(self.out), len(self.out) + 3, len(data)))
        self.out += bytes([1 if reset_dict else 2]) + struct.pack(">H", len(data) - 1) + data
        self.text += data
        return self

    def _reset_state(self):
        self.state, self.reps = 0, [0, 0, 0, 0]
        self.probs = [1024] * (LITERAL + (768 << (self.lc + self.lp)))

    def lzma(self, packets, control=0xE0, props=None, usize_delta=0):
        """control: 0xE0 all reset, 0xC0 state reset + new props, 0xA0 state reset, 0x80 nothing reset"""
        if control >= 0xE0:
            self.dict_start = len(self.text)
        if control >= 0xC0:
            self.lc, self.lp, self.pb = props
        if control >= 0xA0:
            self._reset_state()
        rc, start = RangeEncoder(), len(self.text)
        for p in packets:
            self._packet(rc, p)
        payload = rc.finish()
        usize, csize = len(self.text) - start + usize_delta - 1, len(payload) - 1
        assert 0 <= usize < 1 << 21 and 0 <= csize < 1 << 16, (usize, csize)
        head = bytes([control | usize >> 16]) + struct.pack(">HH", usize & 0xFFFF, csize)
        if control >= 0xC0:
            head += bytes([(self.pb * 5 + self.lp) * 9 + self.lc])
        self.chunks.append((len(self.out), len(self.out) + len(head), len(payload)))
        self.out += head + payload
        return self

    def end(self):
        return bytes(self.out) + b"\0", bytes(self.text)

    # ---- one packet
    def _tree(self, rc, base, bits, v):
        m = 1
        for i in range(bits - 1, -1, -1):
            b = v >> i & 1
            rc.bit(self.probs, base + m, b)
            m = m << 1 | b

    def _tree_reverse(self, rc, base, bits, v):
        m = 1
        for i in range(bits):
            b = v >> i & 1
            rc.bit(self.probs, base + m, b)
            m = m << 1 | b

    def _length(self, rc, base, n, ps):
        n -= 2
        if n < 8:
            rc.bit(self.probs, base, 0)
            self._tree(rc, base + 2 + (ps << 3), 3, n)
        elif n < 16:
            rc.bit(self.probs, base, 1)
            rc.bit(self.probs, base + 1, 0)
            self._tree(rc, base + 130 + (ps << 3), 3, n - 8)
        else:
            rc.bit(self.probs, base, 1)
            rc.bit(self.probs, base + 1, 1)
            self._tree(rc, base + 258, 8, n - 16)

    def _copy(self, n):
        d = self.reps[0] + 1
        for _ in range(n):
            self.text.append(self.text[-d] if d <= len(self.text) else 0)

    def _packet(self, rc, p):
        P, st = self.probs, self.state
        pos = len(self.text) - self.dict_start
        ps = pos & ((1 << self.pb) - 1)
        if p[0] == "lit":
            rc.bit(P, IS_MATCH + (st << 4) + ps, 0)
            prev = self.text[-1] if pos else 0
            base = LITERAL + 0x300 * (((pos & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc)))
            sym, byte = 1, p[1]
            if st >= 7:
                mb, offs = self.text[-self.reps[0] - 1], 0x100
                for i in range(7, -1, -1):
                    mb <<= 1
                    bit = offs
                    offs &= mb
                    b = byte >> i & 1
                    rc.bit(P, base + offs + bit + sym, b)
                    sym = sym << 1 | b
                    if not b:
                        offs ^= bit
            else:
                for i in range(7, -1, -1):
                    b = byte >> i & 1
                    rc.bit(P, base + sym, b)
                    sym = sym << 1 | b
            self.text.append(byte)
            self.state = 0 if st < 4 else st - 3 if st < 10 else st - 6
            return
        rc.bit(P, IS_MATCH + (st << 4) + ps, 1)
        if p[0] == "match":
            _, n, dist = p
            rc.bit(P, IS_REP + st, 0)
            self._length(rc, LEN_CODER, n, ps)
            rep0 = dist - 1
            slot = slot_of(rep0)
            self._tree(rc, POS_SLOT + (min(n - 2, 3) << 6), 6, slot)
            if slot >= 4:
                nd = (slot >> 1) - 1
                base = (2 | slot & 1) << nd
                if slot < 14:
                    self._tree_reverse(rc, SPEC_POS + base - slot - 1, nd, rep0 - base)
                else:
                    rc.direct((rep0 - base) >> 4, nd - 4)
                    self._tree_reverse(rc, ALIGN, 4, (rep0 - base) & 15)
            self.reps = [rep0] + self.reps[:3]
            self.state = 7 if st < 7 else 10
            self._copy(n)
            return
        rc.bit(P, IS_REP + st, 1)
        if p[0] == "shortrep":
            rc.bit(P, IS_REP_G0 + st, 0)
            rc.bit(P, IS_REP0_LONG + (st << 4) + ps, 0)
            self.state = 9 if st < 7 else 11
            self._copy(1)
            return
        _, i, n = p
        if i == 0:
            rc.bit(P, IS_REP_G0 + st, 0)
            rc.bit(P, IS_REP0_LONG + (st << 4) + ps, 1)
        else:
            rc.bit(P, IS_REP_G0 + st, 1)
            rc.bit(P, IS_REP_G1 + st, 0 if i == 1 else 1)
            if i > 1:
                rc.bit(P, IS_REP_G2 + st, 0 if i == 2 else 1)
            self.reps = [self.reps[i]] + self.reps[:i] + self.reps[i + 1:]
        self._length(rc, REP_LEN_CODER, n, ps)
        self.state = 8 if st < 7 else 11
        self._copy(n)


# ---- the container ------------------------------------------------------------------------------------------------------------------

_CRC64_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xC96C5795D7870F42 if _c & 1 else _c >> 1
    _CRC64_TABLE.append(_c)


def crc64(data):
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = _CRC64_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def crc32le(b):
    return struct.pack("<I", zlib.crc32(b))


def check_of(kind, text):
    if kind == 0:
        return b""
    if kind == 1:
        return crc32le(text)
    if kind == 4:
        return struct.pack("<Q", crc64(text))
    if kind == 10:
        return hashlib.sha256(text).digest()
    raise ValueError(kind)


def dict_byte(size):
    for b in range(41):
        if (0xFFFFFFFF if b == 40 else (2 | b & 1) << (b // 2 + 11)) >= size:
            return b
    raise ValueError(size)


def block(data, text, kind, dict_size=1 << 20, sizes=False, filters=None, pad_byte=0, header_pad=0):
    """-> (the block's bytes with padding and check, its Unpadded Size, offsets inside it: payload, padding, check)"""
    flt = filters if filters is not None else [(0x21, bytes([dict_byte(dict_size)]))]
    body = bytes([len(flt) - 1 | (0xC0 if sizes else 0)])
    if sizes:
        body += vli(len(data)) + vli(len(text))
    for fid, props in flt:
        body += vli(fid) + vli(len(props)) + props
    total = (1 + len(body) + 4 + 3) // 4 * 4 + 4 * header_pad
    head = bytes([total // 4 - 1]) + body
    head += b"\0" * (total - 4 - len(head))
    head += crc32le(head)
    pad = -(len(head) + len(data)) % 4
    chk = check_of(kind, text)
    return head + data + bytes([pad_byte]) * pad + chk, len(head) + len(data) + len(chk), (len(head), len(head) + len(data), len(head) + len(data) + pad)


def stream(blocks, kind, index_delta=(0, 0), backward_delta=0):
    """blocks: what block() returns, with each block's text length -> (the stream, its layout: header / blocks / index / footer offsets)"""
    flags = bytes([0, kind])
    out = bytearray(b"\xfd7zXZ\0" + flags + crc32le(flags))
    layout = {"header": 0, "blocks": []}
    index = b"\0" + vli(len(blocks))
    for k, ((raw, unpadded, offs), text_len) in enumerate(blocks):
        layout["blocks"].append({"at": len(out), "payload": len(out) + offs[0], "padding": len(out) + offs[1], "check": len(out) + offs[2]})
        out += raw
        du, dt = index_delta if k == 0 else (0, 0)
        index += vli(unpadded + du) + vli(text_len + dt)
    index += b"\0" * (-len(index) % 4)
    index += crc32le(index)
    layout["index"] = len(out)
    out += index
    layout["footer"] = len(out)
    tail = struct.pack("<I", len(index) // 4 - 1 + backward_delta) + flags
    out += crc32le(tail) + tail + b"YZ"
    return bytes(out), layout


def single(data, text, kind=4, **kw):
    """one stream of one block"""
    skw = {k: kw.pop(k) for k in ("index_delta", "backward_delta") if k in kw}
    return stream([(block(data, text, kind, **kw), len(text))], kind, **skw)
