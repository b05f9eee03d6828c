"""Texts made for the device's deflate writer (merkurio_amd/csrc/codec/bgzf_deflate.hip), each with what the kernel's parse rule
promises of it.  The rule, as the kernel documents it: 64 positions (a window, one per lane) at a time; every position with 4 bytes
left hashes them into a table of 1 Ki entries that keeps the MOST RECENT position of a hash -- all lookups of a window happen
before any of its positions is entered; the candidate (at most 32 768 back) is compared byte by byte, at most 258, at least 4; a
position whose 4 bytes equal the 4 bytes one position back also tries distance 1, unless the table's candidate already reached the
longest length the position allows, and takes it on a tie; the walk over the window takes the first match, unless the next position
holds a longer one (then a literal and that match); windows a match has covered are skipped and enter nothing.

All texts are seeded and deterministic.  What they claim about themselves -- no 4 bytes twice but for the planted copies, table
entries that survive until they are looked up -- is checked on the CPU by test_deflate_read_cpu.py, so that a failing assertion of
test_gpu_deflate_craft.py is the kernel's."""
import heapq
import random

from deflate_read import DIST_BASE, LEN_BASE

PERM = random.Random(5).sample(range(256), 256)  # arbitrary byte values, both sides of 0x80: an alphabet of k values is PERM[:k]
RUN_BYTE = PERM[255]                             # the byte of runs and fillers: in no alphabet of fewer than 256 values
MEMBER = 65280                                   # the most text a member holds
HASH_BITS = 10


def bucket(four):
    """the kernel's table entry of 4 bytes of text"""
    return ((int.from_bytes(four, "little") * 0x9E3779B1) & 0xffffffff) >> (32 - HASH_BITS)


def repeats(text):
    """the positions whose 4 bytes stand at an earlier position too"""
    seen, out = set(), []
    for i in range(len(text) - 3):
        g = text[i:i + 4]
        if g in seen:
            out.append(i)
        seen.add(g)
    return out


def lookup_survives(text, src, at):
    """the lookup of position `at` finds position `src`: src was entered by a window in front of at's, and no position between it
    and that window has its table entry (every position counted as entered: skipped windows only enter fewer)"""
    base = at & ~63
    b = bucket(text[src:src + 4])
    return src < base and all(bucket(text[p:p + 4]) != b for p in range(src + 1, base))


def huffman_cost(hist):
    """(bits of the text under an unrestricted Huffman code of the histogram {symbol: count}, its longest codeword)"""
    heap = [(c, 0, 0) for c in hist.values() if c]  # (weight, depth below, tie-break)
    heapq.heapify(heap)
    cost, k = 0, 1
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, k))
        k += 1
    return cost, heap[0][1]


class Builder:
    """a text written piece by piece: fresh() bytes never complete 4 bytes the text already holds (nor an entry of self.protected),
    copy() repeats earlier text, and the byte behind a copy differs from the byte behind its source, so that the copy's length is
    exact"""

    def __init__(self, seed, values):
        self.rng = random.Random(seed)
        self.alphabet = PERM[:values]
        self.text = bytearray()
        self.seen = set()
        self.protected = set()
        self.not_next = None

    def _push(self, byte):
        self.text.append(byte)
        if len(self.text) >= 4:
            self.seen.add(bytes(self.text[-4:]))

    def fresh(self, n, not_last=None):
        for k in range(n):
            for _ in range(10000):
                c = self.rng.choice(self.alphabet)
                g = bytes(self.text[-3:]) + bytes([c])
                if c == self.not_next or (k == n - 1 and c == not_last):
                    continue
                if len(g) == 4 and (g in self.seen or bucket(g) in self.protected):
                    continue
                break
            else:
                raise RuntimeError("no fresh byte left")
            self._push(c)
            self.not_next = None
        return self

    def raw(self, data):
        for c in data:
            self._push(c)
        self.not_next = None
        return self

    def copy(self, start, length):
        assert 0 <= start < len(self.text)
        for k in range(length):
            self._push(self.text[start + k])
        self.not_next = self.text[start + length]
        return self

    def protect(self, pos):
        self.protected.add(bucket(self.text[pos:pos + 4]))

    def bytes(self):
        return bytes(self.text)


def noise(n, seed=0, values=16):
    """n bytes over `values` byte values, no 4 of them twice"""
    return Builder(1000 + seed, values).fresh(n).bytes()


# ---- a. no 4 bytes twice: a de Bruijn sequence B(16, 4) ---------------------------------------------------------------------------------
def _de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence: the Lyndon words whose length divides n, in order"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


_DB = None
NO_REPEAT_SIZES = (63, 64, 127, 128, 4095, 4096, 4097, MEMBER)  # tokens (one more: the end of the block) either side of a group of 64


def no_repeat_text(n, at=0):
    """n bytes from position `at` of B(16, 4) on 16 arbitrary byte values: every 4 bytes once.  The kernel's shortest match is 4:
    exactly n literals and the end-of-block symbol"""
    global _DB
    if _DB is None:
        _DB = bytes(PERM[s] for s in _de_bruijn(16, 4))
        assert len(_DB) == 65536
    assert at + n <= len(_DB)
    return _DB[at:at + n]


# ---- b. runs ------------------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = tuple(range(1, 9)) + tuple(range(257, 264)) + (516, 517, 518)
RUN_SEPARATOR = 300  # bytes over 16 values: 4 bits each, so that a member of separator and run is never stored


def run_text(length, separator=0):
    return noise(separator, seed=7) + bytes([RUN_BYTE]) * length


def check_run_tokens(tokens, length, byte=RUN_BYTE):
    """the tokens of a run of `length` bytes that no equal byte precedes.  The run's first byte is a literal (nothing to copy from).
    From its second byte on: matches of 258 while 258 bytes are left, then one match if 4 or more are left, else literals.
    The first match has distance 1 exactly: the table holds no position of the run when it is looked up (or, a window on, only the
    run's first byte).  A LATER match has any distance back into the run: by then the table holds a position of the run, that
    candidate reaches the longest length the position allows, and the kernel tries distance 1 only where the table's candidate
    falls short of it.  (The issue expected distance 1 throughout; that is not the kernel's rule -- `len < maxlen` in front of the
    run candidate -- and costs a 64 KiB run some 200 bytes, see DESIGN.md.)"""
    want = [1] if length else []
    rest = length - 1
    while rest >= 4:
        want.append(min(rest, 258))
        rest -= want[-1]
    want += [1] * max(rest, 0)
    got = [1 if t.__class__ is int else t[0] for t in tokens]
    assert got == want, (length, got[:8], want[:8], len(got), len(want))
    at, first = 0, True
    for t in tokens:
        if t.__class__ is int:
            assert t == byte
            at += 1
            continue
        assert 1 <= t[1] <= at, (length, at, t)
        if first:
            assert t[1] == 1, (length, t)
        first = False
        at += t[0]


# ---- c. distance edges ----------------------------------------------------------------------------------------------------------------------
COPY = 300
FAR_DISTANCES = (300, 32767, 32768)
TOO_FAR_DISTANCES = (32769, 40000)
NEAR_DISTANCES = (5, 17, 63, 64, 65)
NEAR_LEAD = 256


def distance_text(d):
    """X (300 bytes over 64 values, no 4 twice), a run as filler, X again d bytes behind the first: the filler's positions share one
    table entry (and windows its matches cover enter nothing), so X's entries are there when the second copy looks them up"""
    b = Builder(2000 + d, 64).fresh(COPY)
    b.raw(bytes([RUN_BYTE]) * (d - COPY))
    return b.copy(0, COPY).bytes()[:d + COPY]


def covered(tokens, lo, hi, distance=None):
    """bytes of text[lo, hi) that match tokens (of that distance) stand for"""
    n, at = 0, 0
    for t in tokens:
        if t.__class__ is int:
            at += 1
            continue
        if distance is None or t[1] == distance:
            n += max(0, min(hi, at + t[0]) - max(lo, at))
        at += t[0]
    return n


def near_text(d):
    """256 bytes over 16 values, then d more of them four times over: repeats nearer than a window is wide"""
    b = Builder(3000 + d, 16).fresh(NEAR_LEAD + d)
    return b.copy(NEAR_LEAD, 3 * d).bytes()


# ---- d. the lazy step -----------------------------------------------------------------------------------------------------------------------
LAZY_LANES = (0, 31, 62, 63)
LAZY_TAIL = 20


def lazy_text(lane):
    """-> (text, q): window 0 holds `wxyz` at 10 and, apart from it, `xyz` and 20 fresh bytes at 34; the byte at q = 64 + lane is `w`
    again, followed by `xyz` and the same 20 bytes.  At q the table offers a match of 4 (`wxyz`, then the texts differ), at q + 1 one of
    23: the kernel's one-step lazy rule writes `w` as a literal and the match of 23.  Both table entries survive until they are looked
    up (checked on the CPU; the seed is the first for which they do)"""
    for seed in range(4000, 4100):
        b = Builder(seed + 100 * lane, 16).fresh(14)  # wxyz = text[10:14]
        b.fresh(20, not_last=b.text[10])              # (no `w` in front of the second xyz)
        b.copy(11, 3).fresh(LAZY_TAIL)                # xyz at 34, the 20 bytes at 37 (the first of them differs from text[14])
        b.fresh(7 + lane, not_last=b.text[9])         # (the byte in front of the second w differs from the one in front of the first)
        q = len(b.text)
        b.copy(10, 4).copy(37, LAZY_TAIL).fresh(64)
        text = b.bytes()
        assert q == 64 + lane
        if repeats(text) == list(range(q, q + 21)) and lookup_survives(text, 10, q) and lookup_survives(text, 34, q + 1):
            return text, q
    raise RuntimeError("no seed gives the lazy text")


# ---- e. every symbol ------------------------------------------------------------------------------------------------------------------------
SYMBOLS_NOISE = 33 * 1024
SYMBOLS_GAP = 8


def symbols_copies():
    """(length, distance): every distance code with some length base, then every length base from 4 up at a distance with extra bits
    set.  The distances rise by more than a copy and its gap take, so a copy planted later has its source EARLIER in the noise: the
    noise behind a source avoids the table entry of the source's first 4 bytes, and so does every copy of such noise"""
    out = [(LEN_BASE[1 + k % 28], DIST_BASE[k]) for k in range(30)]
    out += [(LEN_BASE[1 + j], 24900 + 280 * j) for j in range(28)]
    assert all(b[1] - a[1] > a[0] + SYMBOLS_GAP for a, b in zip(out, out[1:]) if a[1] >= 128)
    return out


_SYMBOLS = None


def symbols_text():
    """-> (text, [(position, length, distance, exact)]): 33 KiB over 64 values with no 4 bytes twice, then the copies of
    symbols_copies(), each behind 8 fresh bytes (a match that runs a byte or two into them never reaches the next copy).  exact: the
    distance is 128 or more and the source lies in the noise, where every window is parsed and entered -- and no later position
    takes the table entry of the source's first 4 bytes (the noise is drawn that way; checked on the CPU), so the lookup at the
    copy's first byte finds the source and the token is exactly (length, distance)"""
    global _SYMBOLS
    if _SYMBOLS is not None:
        return _SYMBOLS
    copies = symbols_copies()
    at, plan = SYMBOLS_NOISE, []
    for length, dist in copies:
        at += SYMBOLS_GAP
        plan.append((at, length, dist, dist >= 128 and at - dist + length <= SYMBOLS_NOISE))
        at += length
    sources = sorted(pos - dist for pos, length, dist, exact in plan if exact)
    for seed in range(5000, 5100):
        b = Builder(seed, 64)
        for s in sources:
            b.fresh(s + 4 - len(b.text))
            b.protect(s)
        b.fresh(SYMBOLS_NOISE - len(b.text))
        for pos, length, dist, exact in plan:
            b.fresh(SYMBOLS_GAP, not_last=b.text[pos - dist - 1] if dist > SYMBOLS_GAP else None)  # (no longer a copy than planted)
            assert len(b.text) == pos
            b.copy(pos - dist, length)
        text = b.fresh(SYMBOLS_GAP).bytes()
        if all(lookup_survives(text, pos - dist, pos) for pos, length, dist, exact in plan if exact):
            _SYMBOLS = (text, plan)
            return _SYMBOLS
    raise RuntimeError("no seed gives the text of every symbol")


# ---- f. deep codes --------------------------------------------------------------------------------------------------------------------------
def fibonacci_text(seed=3):
    """the text of test_length_limited_code_on_a_fibonacci_histogram (its seed is 3): 24 byte values whose counts grow like Fibonacci
    numbers, shuffled -- the unrestricted Huffman tree is 20 and more levels deep"""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    data = b"".join(bytes([65 + i]) * f for i, f in enumerate(fib))
    return bytes(random.Random(seed).sample(data, len(data)))[:65000]


# ---- g. the stored edge ---------------------------------------------------------------------------------------------------------------------
# Bytes drawn EVENLY from 200 .. 256 values never beat a stored block at 64 .. 1024 bytes (a dynamic header of that many lengths
# costs more than 1024 bytes of such text save: zlib's Z_HUFFMAN_ONLY stores every one of them, test_deflate_read_cpu.py), so the sweep
# the issue asks for would hold stored members only.  Drawn with weights 1 / (rank + 4) the same alphabets and sizes cross the edge
# between 384 and 640 bytes; the sweep covers that range in steps of 4.
EDGE_VALUES = (200, 216, 232, 248, 256)
EDGE_SIZES = tuple(range(384, 641, 4))
EDGE_SEEDS = 2


def edge_noise(n, values, seed):
    rng = random.Random(6000 + 1000 * values + seed)
    return bytes(rng.choices(PERM[:values], weights=[1.0 / (k + 4) for k in range(values)], k=n))


def edge_text(n):
    """members of n bytes back to back: every alphabet of EDGE_VALUES, EDGE_SEEDS draws each"""
    return b"".join(edge_noise(n, v, s) for v in EDGE_VALUES for s in range(EDGE_SEEDS))


# ---- h. seams -------------------------------------------------------------------------------------------------------------------------------
SEAM_BLOCKS = (4, 5, 8, 63, 64, 65, 259, 1000)


def period_text(n=3000):
    return (bytes(PERM[20:33]) * (n // 13 + 1))[:n]


# ---- one call of more members than waves are resident -----------------------------------------------------------------------------------------
MIXED_MEMBERS, MIXED_BYTES = 4160, 256  # (a 256-CU card holds 4 096 waves of the deflate kernel)
MIXED_SEPARATOR = 100


def mixed_member(k):
    """member k of the mixed call: (kind, text) -- a (every 4 bytes once), b (such bytes, then a run), g (flat noise: stored), and
    text over 64 values in turn, no two members alike"""
    kind = "abgn"[k % 4]
    at = (k * 97) % (MEMBER - MIXED_BYTES)
    if kind == "a":
        return kind, no_repeat_text(MIXED_BYTES, at)
    if kind == "b":
        return kind, no_repeat_text(MIXED_SEPARATOR, at) + bytes([RUN_BYTE]) * (MIXED_BYTES - MIXED_SEPARATOR)
    rng = random.Random(7000 + k)
    return kind, bytes(rng.choice(PERM[:256 if kind == "g" else 64]) for _ in range(MIXED_BYTES))
