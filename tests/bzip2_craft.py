"""Hand-made bzip2 streams, bit by bit -- what libbz2's encoder never writes: the corners of the format that its decoder takes but
that lie outside the encoder's dialect (`ok-`), streams that it refuses (`bad-`), and streams that it takes while the project's
decoder documents that it hands them back to libbz2 (`host-`: the `randomised` bit, more than 18 002 selectors, a magic too many in
the table of markers -- a closed list).  The judge is libbz2 through Python's bz2 (`libbz2_says`): the module checks at import that
every name's prefix is libbz2's verdict and that the text it makes is the text of the small model of the decoder below, so a slip
in a builder fails here and cannot turn a corner case into an ordinary one.

A block is given at the level the case needs: a last column and origPtr, or the raw symbols (RUNA / RUNB / move-to-front index + 1 /
end of block) with the bytes in use.  Where no CRC is given it comes from the model: un-MTF, the counting-sort vector, the walk, the
last run-length step, bzip2's CRC.  Used by test_bunzip2_craft_cpu.py, test_gpu_bunzip2_craft.py and test_cli_bunzip2_gpu.py; plain
Python, nothing but bz2 / struct."""
import bz2
import functools
import random
import struct

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
RUNA, RUNB = 0, 1
# status of a refused block (bzip2_serial.hpp)
RANDOMISED, ORIG_PTR, GROUPS, SELECTORS, CODE_LENGTH, CODE, SELECTOR, TOO_MANY, NO_BYTES, RUN_TOO_LONG, RUN_CUT = -2, -3, -4, -5, -6, -7, -8, -9, -10, -11, -12


class BitWriter:
    """bits of the stream, first bit on top"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        assert 0 <= value < (1 << count) or count == 0 and value == 0, (value, count)
        self.acc = self.acc << count | value
        self.n += count
        if self.n >= 512:
            self._spill()

    def _spill(self):
        whole, rest = self.n >> 3, self.n & 7
        self.out += (self.acc >> rest).to_bytes(whole, "big")
        self.acc &= (1 << rest) - 1
        self.n = rest

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        self.bits(0, -self.n % 8)
        self._spill()
        return bytes(self.out)


# ---- bzip2's CRC: polynomial 0x04c11db7, first bit on top ----------------------------------------------------------------------------
def _crc_entry(i):
    c = i << 24
    for _ in range(8):
        c = (c << 1 ^ 0x04c11db7 if c & 0x80000000 else c << 1) & 0xffffffff
    return c


CRC_TABLE = [_crc_entry(i) for i in range(256)]


def _mulmod(a, b):
    r = 0
    for i in range(31, -1, -1):
        r = (r << 1 ^ 0x04c11db7 if r & 0x80000000 else r << 1) & 0xffffffff
        if b >> i & 1:
            r ^= a
    return r


def _x_pow_bytes(n):
    r, sq = 1, 0x100
    while n:
        if n & 1:
            r = _mulmod(r, sq)
        sq = _mulmod(sq, sq)
        n >>= 1
    return r


def _crc_run(c, byte, k):
    """the register after k more copies of byte: state(A + B, c) = state(B, 0) ^ state(A, c) * x^(8 |B|), B doubled up"""
    if k < 64:
        for _ in range(k):
            c = (c << 8 & 0xffffffff) ^ CRC_TABLE[c >> 24 ^ byte]
        return c
    r, n = 0, 0
    for bit in bin(k)[2:]:
        r, n = _mulmod(r, _x_pow_bytes(n)) ^ r, 2 * n
        if bit == "1":
            r, n = (r << 8 & 0xffffffff) ^ CRC_TABLE[r >> 24 ^ byte], n + 1
    return _mulmod(c, _x_pow_bytes(k)) ^ r


def crc_of_runs(runs):
    """runs: [(byte, count)]"""
    c, at = 0xffffffff, 0
    while at < len(runs):  # (neighbours of one byte as one run: a block of 100 000 equal symbols is a single one)
        byte, k, at = runs[at][0], runs[at][1], at + 1
        while at < len(runs) and runs[at][0] == byte:
            k, at = k + runs[at][1], at + 1
        c = _crc_run(c, byte, k)
    return c ^ 0xffffffff


def fold(stream_crc, block_crc):
    return ((stream_crc << 1 | stream_crc >> 31) ^ block_crc) & 0xffffffff


# ---- the model of the decoder ---------------------------------------------------------------------------------------------------------
def symbols_of(last, in_use):
    """the last column as the encoder codes it: zero runs in bijective base 2, move-to-front index + 1, end of block"""
    mtf, out, run = list(range(len(in_use))), [], 0
    where = {b: i for i, b in enumerate(in_use)}

    def flush():
        nonlocal run
        while run:
            out.append(RUNA if run & 1 else RUNB)
            run = (run - 1) >> 1 if run & 1 else (run - 2) >> 1
    for b in last:
        at = mtf.index(where[b])
        if at == 0:
            run += 1
            continue
        flush()
        out.append(at + 1)
        mtf.insert(0, mtf.pop(at))
    flush()
    return out + [len(in_use) + 1]


def run_symbols(n):
    """a zero run of n"""
    out = []
    while n:
        out.append(RUNA if n & 1 else RUNB)
        n = (n - 1) >> 1 if n & 1 else (n - 2) >> 1
    return out


def last_of(symbols, in_use):
    """symbols (up to the first end of block) -> the last column, or None where they name no byte"""
    if not in_use:
        return None
    mtf, out, run, weight = list(in_use), bytearray(), 0, 1
    for s in symbols:
        if isinstance(s, tuple):
            return None
        if s <= RUNB:
            run, weight = run + (weight << s), weight << 1
            if run > 1000000:
                return None
            continue
        out += bytes([mtf[0]]) * run
        run, weight = 0, 1
        if s == len(in_use) + 1:
            return bytes(out)
        if s > len(in_use) + 1:
            return None
        mtf.insert(0, mtf.pop(s - 1))
        out.append(mtf[0])
    return None


def walk(last, orig_ptr):
    """the inverse transform as the project does it: the bytes in front of the last run-length step"""
    n = len(last)
    if orig_ptr >= n:
        return None
    order = sorted(range(n), key=last.__getitem__)  # (stable) row j starts with last[order[j]] and is followed by row order[j]
    p, pre = orig_ptr, bytearray()
    for _ in range(n):
        p = order[p]
        pre.append(last[p])
    return bytes(pre)


def expand(pre):
    """the last run-length step -> [(byte, count)], or None where four equal bytes end the block with no count behind them"""
    runs, run, prev = [], 0, -1
    for b in pre:
        if run == 4:
            runs.append((prev, b))
            run, prev = 0, -1
        elif b == prev:
            run += 1
            runs.append((b, 1))
        else:
            run, prev = 1, b
            runs.append((b, 1))
    return None if run == 4 else runs


def model(last, orig_ptr):
    """-> (text, crc) or None"""
    pre = walk(last, orig_ptr) if last else None
    runs = expand(pre) if pre is not None else None
    if runs is None:
        return None
    return b"".join(bytes([b]) * k for b, k in runs), crc_of_runs(runs)


def bwt(pre):
    """-> (last column, origPtr) of the sorted rotations of pre"""
    n = len(pre)
    rows = sorted(range(n), key=lambda i: pre[i:] + pre[:i])
    return bytes(pre[i - 1] for i in rows), rows.index(0)


def some_orig_ptr(last):
    """the first origPtr from which the walk of this (arbitrary) last column does not end inside a run"""
    for p in range(len(last)):
        if model(last, p):
            return p
    raise AssertionError("no origPtr gives a text")


# ---- codes ----------------------------------------------------------------------------------------------------------------------------
def flat(alpha):
    """every symbol in the same number of bits (complete only where alpha is a power of two)"""
    return [max(1, (alpha - 1).bit_length())] * alpha


def codewords(lens):
    """BZ2_hbAssignCodes: by length, then by symbol.  A codeword that outgrows its length (an over-subscribed code) keeps its low bits"""
    code, out = 0, {}
    for l in range(min(lens), max(lens) + 1):
        for s, ls in enumerate(lens):
            if ls == l:
                out[s] = (code & ((1 << l) - 1), l)
                code += 1
        code <<= 1
    return out


def steps_to(lens):
    """the delta coding of code lengths as the encoder writes it: (start, one string of '+' / '-' per symbol)"""
    cur, steps = lens[0], []
    for l in lens:
        steps.append(("+" if l > cur else "-") * abs(l - cur))
        cur = l
    return lens[0], steps


def lengths_of(start, steps):
    """what a (start, steps) coding says, values outside 1 .. 20 clamped (such a block is refused before a symbol is read)"""
    cur, out = start, []
    for s in steps:
        cur += s.count("+") - s.count("-")
        out.append(min(20, max(1, cur)))
    return out


# ---- blocks and streams ---------------------------------------------------------------------------------------------------------------
def block(last=None, orig_ptr=0, symbols=None, in_use=None, lengths=None, n_tables=2, selectors=None, selector_codes=None, spare=0, n_selectors=None,
          randomised=0, crc=None, length_steps=None, empty_rows=(), table_order=None):
    """one block.  last + orig_ptr, or symbols (end of block included; a tuple (value, bits) stands for raw bits in a symbol's place) + in_use.
    in_use: the bytes in use (default: those of last); lengths: one list for all tables or one per table (default: flat);
    length_steps: {table: (start, steps per symbol)} instead of the encoder's coding of that table's lengths;
    selectors: the table of every group of 50 (default: table 0, as many as the symbols need); selector_codes: the unary codes
    themselves, whatever they say; spare: further selectors (1 bit each) behind them; n_selectors: the field, where it is to
    disagree; empty_rows: rows of the map flagged although none of their 16 bytes is in use"""
    if symbols is None:
        in_use = sorted(set(last)) if in_use is None else sorted(in_use)
        symbols = symbols_of(last, in_use)
    else:
        in_use = sorted(in_use)
        last = last_of(symbols, in_use)
    alpha = len(in_use) + 2
    if lengths is None:
        lengths = flat(alpha)
    tables = [list(l) for l in lengths] if isinstance(lengths[0], (list, tuple)) else [list(lengths)] * n_tables
    n_tables = len(tables)
    length_steps = dict(length_steps or {})
    for t, (start, steps) in length_steps.items():
        tables[t] = lengths_of(start, steps)
    assert all(len(t) == alpha for t in tables), (alpha, [len(t) for t in tables])
    groups = (len(symbols) + 49) // 50
    if selectors is None:
        selectors = [0] * groups
    m = model(last, orig_ptr) if last else None
    text = m[0] if m else None
    if crc is None:
        crc = m[1] if m else 0
    w = []
    w.append((BLOCK_MAGIC, 48)), w.append((crc, 32)), w.append((randomised, 1)), w.append((orig_ptr, 24))
    rows = [0] * 16
    for b in in_use:
        rows[b >> 4] |= 0x8000 >> (b & 15)
    flagged = [bool(rows[i]) or i in empty_rows for i in range(16)]
    w.append((sum(0x8000 >> i for i in range(16) if flagged[i]), 16))
    w += [(rows[i], 16) for i in range(16) if flagged[i]]
    if selector_codes is None:
        pos, selector_codes = list(range(n_tables)), []
        for s in selectors:
            selector_codes.append(pos.index(s))
            pos.insert(0, pos.pop(pos.index(s)))
    selector_codes = list(selector_codes) + [0] * spare
    w.append((n_tables, 3)), w.append((len(selector_codes) if n_selectors is None else n_selectors, 15))
    w += [((1 << j) - 1 << 1, j + 1) for j in selector_codes]
    for t, lens in enumerate(tables):
        start, steps = length_steps.get(t) or steps_to(lens)
        w.append((start, 5))
        for s in steps:
            w += [(2 if c == "+" else 3, 2) for c in s]
            w.append((0, 1))
    # the selectors as the decoder will read them: the symbols' codes follow those
    pos, read = list(range(n_tables)), []
    for j in selector_codes:
        if j >= n_tables:
            break
        pos.insert(0, pos.pop(j))
        read.append(pos[0])
    codes = [codewords(lens) for lens in tables]
    for k, s in enumerate(symbols):
        w.append(s if isinstance(s, tuple) else codes[read[k // 50] if k // 50 < len(read) else 0][s])
    return {"bits": w, "crc": crc, "text": text}


def stream(level, blocks, crc=None):
    w = BitWriter()
    for ch in b"BZh" + bytes([48 + level]):
        w.bits(ch, 8)
    total = 0
    for b in blocks:
        for v, n in b["bits"]:
            w.bits(v, n)
        total = fold(total, b["crc"])
    w.bits(END_MAGIC, 48)
    w.bits(total if crc is None else crc, 32)
    return w.getvalue()


def block_bits(b):
    return sum(n for _, n in b["bits"])


def libbz2_says(blob):
    """the text libbz2 makes of the WHOLE of blob, stream behind stream, or None where it refuses any of it"""
    out, data = [], blob
    if not data:
        return None
    while data:
        d = bz2.BZ2Decompressor()
        try:
            out.append(d.decompress(data))
        except (OSError, ValueError, EOFError):
            return None
        if not d.eof:
            return None
        data = d.unused_data
    return b"".join(out)


def find_magics(b):
    """[(bit, kind)] of every block (0) / end (1) magic, every bit offset tested"""
    v, out = 0, []
    for i in range(len(b) * 8):
        v = (v << 1 | (b[i >> 3] >> (7 - (i & 7)) & 1)) & ((1 << 48) - 1)
        if i >= 47 and v in (BLOCK_MAGIC, END_MAGIC):
            out.append((i - 47, int(v == END_MAGIC)))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
BANANA = bwt(b"banana")  # (b"nnbaaa", 3): a zero run stands directly in front of its end of block
CASES = {}    # name -> (file, blocks, text or None as the model has it)
WHY = {}      # name -> (the harness's refusal word, status or None), for the cases that aim at one rule
MULTI = []    # names of the ok- cases of more than one block


def add(name, blob, blocks=1, text=None, why=None):
    assert name not in CASES, name
    CASES[name] = (blob, blocks, text)
    if why:
        WHY[name] = why
    if name.startswith("ok-") and blocks > 1:
        MULTI.append(name)


def one(name, level=1, why=None, **kw):
    b = block(**kw)
    add(name, stream(level, [b]), 1, b["text"], why)


def by_verdict(name, blob, otherwise, why=None):
    """a case whose prefix is libbz2's verdict, because versions of it differ: `otherwise` where it takes the file"""
    add(("bad-" if libbz2_says(blob) is None else otherwise) + name, blob, 1, None, why)


def unary_codes(value, bits):
    """value's bits read as selector codes (ones closed by a zero); a last code left open is closed by the next selector"""
    s = format(value, "0%db" % bits)
    codes = [len(c) for c in s.split("0")]
    if s.endswith("0"):
        codes.pop()
    return codes


def _build():
    ban = dict(last=BANANA[0], orig_ptr=BANANA[1])  # bytes a b n: alphabet 5
    rng = random.Random(41)
    # ---- code tables
    one("ok-banana-flat-code", **ban)
    one("ok-lengths-all-20", lengths=[20] * 5, **ban)
    one("ok-minimum-length-1", lengths=[1, 2, 3, 4, 4], **ban)
    one("ok-length-steps-touch-1-and-20", length_steps={0: (10, ["-" * 9 + "+" * 19 + "-" * 17, "", "", "", ""])}, **ban)
    one("ok-start-length-1-and-20", lengths=[[1, 2, 3, 4, 4], [20] * 5], selectors=[1], **ban)
    one("bad-start-length-0", why=("block", CODE_LENGTH), length_steps={0: (0, [""] * 5)}, **ban)
    one("bad-start-length-21", why=("block", CODE_LENGTH), length_steps={0: (21, [""] * 5)}, **ban)
    one("bad-length-step-through-0", why=("block", CODE_LENGTH), length_steps={0: (2, ["", "--++", "", "", ""])}, **ban)
    one("bad-length-step-through-21", why=("block", CODE_LENGTH), length_steps={0: (19, ["", "+++-", "", "", ""])}, **ban)
    one("bad-length-step-through-0-in-second-table", why=("block", CODE_LENGTH), length_steps={1: (1, ["", "", "", "", "-+"])}, **ban)
    one("ok-under-subscribed-code", lengths=[4] * 5, **ban)
    one("bad-codeword-that-no-symbol-owns", why=("block", CODE), symbols=[2, (15, 4), 4], in_use=b"abn", lengths=[4] * 5)
    one("bad-codeword-of-20-ones-that-no-symbol-owns", why=("block", CODE), symbols=[2, ((1 << 20) - 1, 20), 4], in_use=b"abn", lengths=[20] * 5)
    # bytes a b n z, z never occurs: symbol 4 (index 3 = z, always at the list's end) gets the codeword that does not fit
    one("ok-over-subscribed-surplus-unused", in_use=b"abnz", lengths=[1, 2, 3, 4, 5, 4], **ban)
    b = block(lengths=[1, 2, 3, 3, 3], **ban)  # the end of block's codeword would be 1000
    by_verdict("over-subscribed-end-of-block-does-not-fit", stream(1, [b]), "ok-")
    six = [[3] * 5, [1, 2, 3, 4, 4], [4, 4, 3, 2, 1], [2, 2, 2, 3, 3], [20, 19, 18, 17, 16], [5, 4, 3, 2, 1]]
    one("ok-six-tables-one-used", lengths=six, selectors=[3], **ban)
    noise = bytes(rng.choices(b"acgtn", k=170))
    one("ok-two-tables-alternating", last=noise, orig_ptr=some_orig_ptr(noise), lengths=[[2, 3, 3, 3, 3, 3, 3], [6, 5, 4, 3, 2, 2, 2]],
        selectors=[k & 1 for k in range((len(symbols_of(noise, sorted(set(noise)))) + 49) // 50)])
    one("bad-selector-equals-ngroups", why=("block", SELECTOR), selector_codes=[2], **ban)
    one("bad-selector-equals-ngroups-of-6", why=("block", SELECTOR), lengths=six, selector_codes=[0, 6], **ban)
    for g in (1, 7):
        one("bad-ngroups-%d" % g, why=("block", GROUPS), lengths=[[3] * 5] * g, **ban)
    # ---- alphabet
    for byte in (0x00, 0x41, 0xff):
        one("ok-one-byte-in-use-%02x" % byte, last=bytes([byte]) * 3)
    seams = [256, 253, 252, 5, 4, 2, 257]  # indices 255, 252, 251, 4, 3, 1: either side of a lane's four entries, and the list's end
    one("ok-all-256-mtf-lane-seams", symbols=seams, in_use=range(256), orig_ptr=some_orig_ptr(last_of(seams, list(range(256)))))
    many = [rng.choice((RUNA, RUNB)) if rng.random() < 0.1 else rng.randrange(2, 257) for _ in range(700)]
    many = many + [4 * k + j + 1 for k in (0, 1, 31, 62, 63) for j in range(4) if 4 * k + j] + [257]  # every place of lanes 0, 1, 31, 62, 63
    one("ok-all-256-mtf-every-seam", symbols=many, in_use=range(256), orig_ptr=some_orig_ptr(last_of(many, list(range(256)))), n_tables=3,
        selectors=[k % 3 for k in range((len(many) + 49) // 50)])
    one("ok-map-row-flagged-and-empty", empty_rows=(0, 5, 15), **ban)
    one("bad-no-byte-in-use", why=("block", NO_BYTES), symbols=[1], in_use=b"")
    one("bad-no-byte-in-use-rows-flagged", why=("block", NO_BYTES), symbols=[1], in_use=b"", empty_rows=(3, 4))
    # ---- runs
    one("ok-run-100000-fills-level-1-ff", symbols=run_symbols(100000) + [2], in_use=b"\xff")
    one("ok-run-100000-fills-level-1-41", symbols=run_symbols(100000) + [2], in_use=b"A")
    one("bad-run-100001-at-level-1", why=("block", TOO_MANY), symbols=run_symbols(100001) + [2], in_use=b"A")
    one("bad-run-99999-ends-in-four-equal-bytes", why=("walk", RUN_CUT), symbols=run_symbols(99999) + [2], in_use=b"A")
    one("ok-symbol-behind-a-run-of-100000-at-level-2", level=2, symbols=run_symbols(100000) + [2, 3], in_use=b"AB", orig_ptr=100000)
    one("bad-symbol-behind-a-full-block", why=("block", TOO_MANY), symbols=run_symbols(100000) + [2, 3], in_use=b"AB", orig_ptr=100000)
    first = b"aaabnbn"
    one("ok-run-as-first-symbols", last=first, orig_ptr=some_orig_ptr(first))
    one("ok-run-in-front-of-end-of-block", lengths=[2, 2, 3, 3, 3], **ban)
    g49, g50 = (b"bca" * 17)[:49], (b"bca" * 17)[:50]
    assert len(symbols_of(g49, b"abc")) == 50 and len(symbols_of(g50, b"abc")) == 51 and RUNA not in symbols_of(g50, b"abc")
    one("ok-end-of-block-is-symbol-50", last=g49, orig_ptr=some_orig_ptr(g49))
    one("ok-end-of-block-opens-a-group", last=g50, orig_ptr=some_orig_ptr(g50))
    one("bad-end-of-block-opens-a-group-nselectors-short", why=("block", SELECTOR), last=g50, orig_ptr=some_orig_ptr(g50), selectors=[0])
    one("bad-nselectors-field-one-short", why=("block", None), last=g50, orig_ptr=some_orig_ptr(g50), n_selectors=1)
    one("ok-end-of-block-opens-a-group-spares", last=g50, orig_ptr=some_orig_ptr(g50), spare=3)
    one("bad-nselectors-0", why=("block", SELECTORS), n_selectors=0, selector_codes=[], **ban)
    one("bad-22-runa", why=("block", RUN_TOO_LONG), level=9, symbols=[RUNA] * 22 + [2], in_use=b"A")
    one("bad-21-runb", why=("block", TOO_MANY), level=9, symbols=[RUNB] * 21 + [2], in_use=b"A")
    # ---- selectors
    one("ok-selectors-18002-one-needed", spare=18001, **ban)
    by_verdict("selectors-18003", stream(1, [block(spare=18002, **ban)]), "host-", why=("block", SELECTORS))
    one("host-randomised", why=("block", RANDOMISED), randomised=1, **ban)
    # ---- the vector
    for p in range(6):
        one("ok-not-one-cycle-abcabc-origptr-%d" % p, last=b"abcabc", orig_ptr=p)
    for p in (1, 2, 3):
        one("ok-not-one-cycle-abba-origptr-%d" % p, last=b"abba", orig_ptr=p)
    one("bad-abba-origptr-0-four-equal-bytes", why=("walk", RUN_CUT), last=b"abba", orig_ptr=0)
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        pre = bytes(rng.choices(b"ACGTN\n@", k=n))
        last, p = bwt(pre)
        one("ok-nblock-%d" % n, last=last, orig_ptr=p)
        if n in (1, 64, 129):
            q = max(i for i in range(n) if model(last, i))
            one("ok-nblock-%d-some-last-origptr" % n, last=last, orig_ptr=q)
            one("bad-origptr-is-nblock-%d" % n, why=("block", ORIG_PTR), last=last, orig_ptr=n)
    one("ok-origptr-nblock-less-1", last=b"abcabd", orig_ptr=5)
    one("bad-origptr-nblock", why=("block", ORIG_PTR), last=b"abcabd", orig_ptr=6)
    one("bad-origptr-all-ones", why=("block", ORIG_PTR), last=b"abcabd", orig_ptr=(1 << 24) - 1)
    # true transforms whose rows starting with 'a' all end in 'x' (or x / y in turn): 64 equal bytes in one turn of the scatter
    xa = b"".join(bytes([120, 97, 128 + i]) for i in range(64))
    last, p = bwt(xa)
    assert last[:64] == b"x" * 64
    one("ok-scatter-64-equal-bytes-in-one-turn", last=last, orig_ptr=p)
    last, p = bwt(b"\x01\x02" + xa)
    assert last[2:66] == b"x" * 64
    one("ok-scatter-equal-bytes-across-two-turns", last=last, orig_ptr=p)
    last, p = bwt(b"".join(bytes([120 + (i & 1), 97, 128 + i]) for i in range(80)))
    assert last[:80] == b"xy" * 40
    one("ok-scatter-two-bytes-interleaved", last=last, orig_ptr=p)
    one("ok-scatter-one-byte-65-times", last=b"a" * 65, orig_ptr=7)
    # ---- the last run-length step
    for name, pre in (("ok-count-0-then-the-same-byte", b"aaaa\0aaaa\0"), ("ok-count-0-inside", b"aaaa\0b"), ("ok-count-is-the-last-byte", b"baaaa\x03"),
                      ("bad-four-equal-bytes-end-the-block", b"baaaa"), ("ok-count-then-four-equal-counts", b"aaaa\x04\x04\x04\x04\x02z"),
                      ("ok-count-255-twice", b"aaaa\xffaaaa\xffb")):
        last, p = bwt(pre)
        one(name, last=last, orig_ptr=p, why=("walk", RUN_CUT) if name.startswith("bad-") else None)
    for byte in (0, 1, 4, 5, 255):
        last, p = bwt(bytes([byte]) * 5 + b"Zq")
        one("ok-count-equals-its-byte-%d" % byte, last=last, orig_ptr=p)
    # ---- magics where no block starts: 14 bytes in use, alphabet 16, every code 4 bits, the symbols are the magics' nibbles.  The table
    # of magics then does not chain: behind a false end magic the walk over it finds no "BZh" (status 0); a false block magic passes
    # the walk and the block in front of it disproves it by not ending there (status 1)
    for kind, magic in (("block", BLOCK_MAGIC), ("end", END_MAGIC)):
        nib = [magic >> (44 - 4 * i) & 15 for i in range(12)] + [15]
        last = last_of(nib, list(range(65, 79)))
        for spare in (0, 1):
            one("host-%s-magic-in-the-symbols-%s" % (kind, "one-bit-on" if spare else "nibble-aligned"), why=("chain", int(kind == "block")), symbols=nib, in_use=range(65, 79),
                lengths=[4] * 16, orig_ptr=some_orig_ptr(last), spare=spare)
    codes = unary_codes(BLOCK_MAGIC, 48)
    one("host-block-magic-in-the-selectors", why=("chain", 1), lengths=six, selector_codes=[0] + codes + [0, 0], **ban)
    # ---- levels
    small, big = block(**ban), block(symbols=run_symbols(100001) + [2], in_use=b"A")
    add("ok-level-1-then-level-9-with-100001-symbols", stream(1, [small]) + stream(9, [big]), 2, small["text"] + big["text"])
    add("ok-level-2-holds-100001-symbols", stream(2, [big]), 1, big["text"])
    add("ok-three-blocks-of-three-kinds", stream(1, [small, block(last=b"abcabc", orig_ptr=4, spare=5), block(last=b"\xff" * 3)]), 3,
        small["text"] + model(b"abcabc", 4)[0] + b"\xff" * 3)
    # ---- the stream's frame
    good = stream(1, [small])
    add("bad-stream-crc", stream(1, [small], crc=small["crc"] ^ 1), why=("stream-crc", None))
    add("bad-block-crc", stream(1, [block(crc=small["crc"] ^ 0x80000000, **ban)]), why=("block-crc", None))
    add("bad-cut-behind-the-end-magic", good[:-4], why=("chain", 0))
    add("bad-cut-inside-the-end-magic", good[:-5], why=("chain", 0))
    add("bad-cut-inside-the-stream-crc", good[:-1], why=("chain", 0))
    add("bad-first-symbol-is-end-of-block", stream(1, [block(symbols=[4], in_use=b"abn")]), why=("block", ORIG_PTR))


_build()


def _self_check():
    for name, (blob, blocks, text) in CASES.items():
        says = libbz2_says(blob)
        assert name[:name.index("-") + 1] in ("ok-", "bad-", "host-"), name
        assert (says is None) == name.startswith("bad-"), "%s: libbz2 %s it" % (name, "refuses" if says is None else "takes")
        if name.startswith("ok-"):
            assert text == says, "%s: the model's text is not libbz2's" % name
    host = sorted(n for n in CASES if n.startswith("host-"))
    assert all("randomised" in n or "selectors-18003" in n or "magic-in-the" in n for n in host), host


_self_check()


def text_of(name):
    """libbz2's text of a case (None: it refuses)"""
    return libbz2_says(CASES[name][0])


def counts():
    return {p: sum(1 for n in CASES if n.startswith(p)) for p in ("ok-", "bad-", "host-")}


def ordered():
    """the cases in an order in which every bad- / host- one is followed by an ok- one"""
    ok = sorted(n for n in CASES if n.startswith("ok-"))
    rest = sorted(n for n in CASES if not n.startswith("ok-"))
    assert len(ok) > len(rest)
    out = []
    for k, name in enumerate(ok):
        if k < len(rest):
            out.append(rest[k])
        out.append(name)
    return out


# ---- sweeps: lists of (label, file, libbz2's text, blocks) ------------------------------------------------------------------------------
def _checked(label, blob, blocks):
    text = libbz2_says(blob)
    assert text is not None, label
    assert sum(1 for _, k in find_magics(blob) if k == 0) == blocks, label
    return label, blob, text, blocks


def _pair(k):
    """two blocks, the first with k spare selectors: every one pushes the second's magic a bit further back"""
    return [block(last=BANANA[0], orig_ptr=BANANA[1], spare=k), block(last=b"abcabc", orig_ptr=2)]


@functools.lru_cache(maxsize=None)
def sweep_spare_selectors():
    """the second block's magic (and the end magic behind it) at every bit phase of a dword"""
    out = [_checked("spare-%d" % k, stream(1, _pair(k)), 2) for k in range(64)]
    assert {find_magics(blob)[1][0] & 31 for _, blob, _, _ in out} == set(range(32))
    return out


@functools.lru_cache(maxsize=None)
def sweep_end_magic():
    """one block and the end magic + CRC as the file's last 10 bytes (and a padded 11th), at every bit phase of a dword"""
    out = [_checked("end-%d" % k, stream(1, [block(last=BANANA[0], orig_ptr=BANANA[1], spare=k)]), 1) for k in range(64)]
    ends = [find_magics(blob)[-1][0] for _, blob, _, _ in out]
    assert {e & 31 for e in ends} == set(range(32)) and all(len(blob) * 8 - e - 80 < 8 for e, (_, blob, _, _) in zip(ends, out))
    return out


@functools.lru_cache(maxsize=None)
def sweep_window_seams():
    """the pair pushed back by whole streams in front of it (empty ones of 14 bytes, one crafted filler whose spare selectors make up
    the odd bytes): the second block's magic starts at every bit from 48 in front of to 32 behind byte 256 (the reader's window of
    64 dwords) and byte 1024 (a workgroup of the marker kernel)"""
    empty = bz2.compress(b"")
    assert len(empty) == 14
    filler = {}
    for j in range(0, 160, 8):
        f = stream(1, [block(last=b"\xff" * 3, spare=j)])
        filler.setdefault(len(f), f)
    filler[0] = b""
    gap = block_bits(_pair(0)[0])
    out = []
    for seam in (256, 1024):
        for bit in range(seam * 8 - 48, seam * 8 + 33):
            k = (bit - 32 - gap) % 8
            lead = (bit - 32 - gap - k) // 8
            fit = [(a, f) for f in sorted(filler) for a in [(lead - f) // 14] if a >= 0 and 14 * a + f == lead]
            a, f = fit[0]
            blob = empty * a + filler[f] + stream(1, _pair(k))
            label, blob, text, blocks = _checked("seam-%d-bit-%+d" % (seam, bit - seam * 8), blob, 2 + (f > 0))
            assert find_magics(blob)[-2][0] == bit, label
            out.append((label, blob, text, blocks))
    return out


@functools.lru_cache(maxsize=None)
def sweep_expand():
    """libbz2's own files: s distinct bytes, a run of r, a tail -- the four equal bytes and their count on every side of a turn of 64
    of the expand kernel -- and texts whose lengths give the CRC kernel empty lanes, full lanes and a short last piece"""
    out = []
    for s in range(56, 69):
        for r in (4, 5, 68, 259, 260):
            text = bytes(range(33, 33 + s)) + b"\xee" * r + b"tail\n"
            out.append(("prefix-%d-run-%d" % (s, r), bz2.compress(text, 1), text, 1))
    rng = random.Random(8)
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097):
        text = bytes(rng.choices(b"ACGTN\n", k=n))
        out.append(("text-%d" % n, bz2.compress(text, 9), text, 1))
    return out


def unaligned_blocks(blob):
    return sum(1 for bit, kind in find_magics(blob) if kind == 0 and bit & 7)


def long_file(min_bytes):
    """distinct valid streams of incompressible text behind each other, more than min_bytes in all -> (file, text)"""
    rng = random.Random(77)
    files, texts, size, k = [], [], 0, 0
    while size <= min_bytes:
        text = struct.pack("<I", k) + rng.randbytes(150000 + 7919 * (k % 5))
        blob = bz2.compress(text, (1, 9, 2)[k % 3])
        files.append(blob), texts.append(text)
        size, k = size + len(blob), k + 1
    return b"".join(files), b"".join(texts)
