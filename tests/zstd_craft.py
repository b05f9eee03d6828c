"""A bit-level writer of Zstandard frames (RFC 8878) for what no compressor can be made to emit: RLE blocks, every literals header
width, every sequence-table mode for each of the three tables (Repeat of an RLE and of a predefined table among them), chosen repeat
offsets at a block start, an 8-byte content size -- and damaged files that hit one field.  It plays the role bzip2_craft.py plays.
The FSE decoding tables are built as the RFC says (4.1.1); sequences are encoded by walking those tables backwards."""
import functools
import struct

LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
PREDEFINED = ((LL_NORM, 6), (OF_NORM, 5), (ML_NORM, 6))


def fse_table(norm, log):
    """[(symbol, bits, base)] per state"""
    size = 1 << log
    sym, high = [0] * size, size - 1
    nxt = []
    for s, p in enumerate(norm):
        nxt.append(1 if p == -1 else p)
        if p == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    out = []
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb = log - (x.bit_length() - 1)
        out.append((sym[u], nb, (x << nb) - size))
    return out


def fse_description(norm, log):
    """the table description (4.1.1) as bytes"""
    acc, pos = log - 5, 4
    remaining, s = 1 << log, 0
    while remaining > 0:
        p = norm[s]
        val, mx = p + 1, remaining + 1
        nb = mx.bit_length()
        lower = (1 << nb) - 1 - mx
        if val < lower:
            acc |= val << pos
            pos += nb - 1
        else:
            acc |= (val + lower if val >= 1 << (nb - 1) else val) << pos
            pos += nb
        remaining -= 1 if p < 0 else p
        s += 1
        if p == 0:
            run = 0
            while s + run < len(norm) and norm[s + run] == 0 and remaining > 0:
                run += 1
            s += run
            while run >= 3:
                acc |= 3 << pos
                pos, run = pos + 2, run - 3
            acc |= run << pos
            pos += 2
    return acc.to_bytes((pos + 7) // 8, "little")


def code_of(value, base, bits):
    for c in range(len(base) - 1, -1, -1):
        if base[c] <= value:
            assert value - base[c] < 1 << bits[c]
            return c, value - base[c], bits[c]
    raise ValueError(value)


def back_stream(items):
    """items in the order the decoder reads them, (value, bits) each -> the bytes, end mark included"""
    acc, pos = 0, 0
    for v, k in reversed(items):
        assert 0 <= v < 1 << k or (k == 0 and v == 0)
        acc |= v << pos
        pos += k
    acc |= 1 << pos
    return acc.to_bytes(pos // 8 + 1, "little")


def encode_states(table, symbols):
    """-> (initial state, [bits read behind every symbol but the last as (value, bits)])"""
    state = next(u for u, e in enumerate(table) if e[0] == symbols[-1])
    steps = []
    for s in reversed(symbols[:-1]):
        u = next(u for u, e in enumerate(table) if e[0] == s and e[2] <= state < e[2] + (1 << e[1]))
        steps.append((state - table[u][2], table[u][1]))
        state = u
    return state, steps[::-1]


def sequences_section(seqs, modes, tables, logs, descriptions):
    """seqs: [(literals length, offset VALUE, match length)]; modes: three of 0..3; tables / logs: the tables in force; descriptions:
    what stands behind the modes byte for every table (b"" for predefined and repeat)"""
    n = len(seqs)
    if n == 0:
        return b"\x00"
    head = bytes([n]) if n < 128 else bytes([128 + (n >> 8), n & 255]) if n < 0x7F00 else b"\xff" + struct.pack("<H", n - 0x7F00)
    head += bytes([modes[0] << 6 | modes[1] << 4 | modes[2] << 2]) + b"".join(descriptions)
    llc = [code_of(l, LL_BASE, LL_BITS) for l, _, _ in seqs]
    mlc = [code_of(m, ML_BASE, ML_BITS) for _, _, m in seqs]
    ofc = [(o.bit_length() - 1, o - (1 << (o.bit_length() - 1)), o.bit_length() - 1) for _, o, _ in seqs]
    s_ll, u_ll = encode_states(tables[0], [c[0] for c in llc])
    s_of, u_of = encode_states(tables[1], [c[0] for c in ofc])
    s_ml, u_ml = encode_states(tables[2], [c[0] for c in mlc])
    items = [(s_ll, logs[0]), (s_of, logs[1]), (s_ml, logs[2])]
    for i in range(n):
        items += [ofc[i][1:], mlc[i][1:], llc[i][1:]]
        if i + 1 < n:
            items += [u_ll[i], u_ml[i], u_of[i]]
    return head + back_stream(items)


def literals_raw(lits, width=None):
    n = len(lits)
    width = width or (1 if n < 32 else 2 if n < 4096 else 3)
    if width == 1:
        return bytes([n << 3]) + lits
    return ((n << 4) | (1 if width == 2 else 3) << 2).to_bytes(width, "little") + lits


def literals_rle(byte, n, width=None):
    width = width or (1 if n < 32 else 2 if n < 4096 else 3)
    if width == 1:
        return bytes([n << 3 | 1, byte])
    return ((n << 4) | (1 if width == 2 else 3) << 2 | 1).to_bytes(width, "little") + bytes([byte])


def block(kind, payload, last=False, size=None):
    """kind: 0 raw, 1 RLE (payload: the byte; size: how many), 2 compressed"""
    size = len(payload) if size is None else size
    return (size << 3 | kind << 1 | int(last)).to_bytes(3, "little") + payload


def frame(blocks, window_log=17, content_size=None, fcs_bytes=0, checksum=None):
    """a frame header with a window descriptor (or, fcs_bytes given, that width of content size) and the blocks"""
    fhd = {0: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6 | (4 if checksum is not None else 0)
    head = struct.pack("<IB", 0xFD2FB528, fhd) + bytes([(window_log - 10) << 3])
    if fcs_bytes:
        head += (content_size - (256 if fcs_bytes == 2 else 0)).to_bytes(fcs_bytes, "little")
    return head + b"".join(blocks) + (struct.pack("<I", checksum) if checksum is not None else b"")


def execute(blocks_spec):
    """the text of [(literals, [(ll, offset value, ml)])] by the rules of 3.1.1.5 -- the crafted files' expected text (libzstd checks it)"""
    out, rep = bytearray(), [1, 4, 8]
    for lits, seqs in blocks_spec:
        at = 0
        for ll, ov, ml in seqs:
            out += lits[at:at + ll]
            at += ll
            if ov > 3:
                off = ov - 3
                rep = [off, rep[0], rep[1]]
            else:
                idx = ov - 1 + (ll == 0)
                if idx == 0:
                    off = rep[0]
                elif idx == 1:
                    off, rep = rep[1], [rep[1], rep[0], rep[2]]
                else:
                    off = rep[2] if idx == 2 else rep[0] - 1
                    rep = [off, rep[0], rep[1]]
            for _ in range(ml):
                out.append(out[-off])
        out += lits[at:]
    return bytes(out)


def compressed_blocks(spec):
    """spec: [(literals, seqs, modes, given)] -- given: for a mode 1 table its symbol, for mode 2 (norm, log).  Repeat (3) takes what
    the block before it left in force -> the blocks' payloads"""
    force = [None, None, None]
    out = []
    for lits, seqs, modes, given in spec:
        desc = []
        for t in range(3):
            if modes[t] == 0:
                force[t] = (fse_table(*PREDEFINED[t]), PREDEFINED[t][1])
                desc.append(b"")
            elif modes[t] == 1:
                force[t] = ([(given[t], 0, 0)], 0)
                desc.append(bytes([given[t]]))
            elif modes[t] == 2:
                force[t] = (fse_table(*given[t]), given[t][1])
                desc.append(fse_description(*given[t]))
            else:
                desc.append(b"")
        lit = lits if isinstance(lits, tuple) else ("raw", lits)
        lit_bytes = literals_rle(lit[1][0], len(lit[1])) if lit[0] == "rle" else literals_raw(lit[1], lit[2] if len(lit) > 2 else None)
        out.append(lit_bytes + sequences_section(seqs, modes, [f[0] for f in force], [f[1] for f in force], desc))
    return out


def _flat(n_sym, log, keep):
    """a distribution over codes 0 .. n_sym - 1 in which every code of `keep` has weight and the rest shares what is left"""
    norm = [0] * n_sym
    for s in keep:
        norm[s] = 1
    left = (1 << log) - len(keep)
    norm[sorted(keep)[0]] += left
    return norm


@functools.lru_cache(maxsize=None)
def valid():
    lits = bytes(range(65, 91)) * 8
    out = {}
    # an RLE block between two raw ones
    out["crafted-rle-block"] = (frame([block(0, b"head "), block(1, b"A", size=1000), block(0, b" tail", last=True)]), b"head " + b"A" * 1000 + b" tail")
    t = b"eight-byte content size"
    out["crafted-fcs-8"] = (frame([block(0, t, last=True)], content_size=len(t), fcs_bytes=8), t)
    # literals headers of every width, no sequences
    for kind in ("raw", "rle"):
        for width, n in ((1, 20), (2, 20), (3, 20), (2, 3000), (3, 70000)):
            body = (lits * 400)[:n] if kind == "raw" else b"Q" * n
            payload = (literals_raw(body, width) if kind == "raw" else literals_rle(81, n, width)) + b"\x00"
            out["crafted-literals-%s-w%d-%d" % (kind, width, n)] = (frame([block(2, payload, last=True)]), body)
    # every table mode for every table; the second block repeats what the first left, the third describes anew
    seqs = [(8, 7 + 3, 5), (0, 1, 4), (3, 2, 6), (0, 3, 3), (2, 3, 9), (1, 1, 3), (0, 2, 8), (5, 40 + 3, 7)]
    for name, modes, given in (("predefined", (0, 0, 0), (None, None, None)),
                               ("rle", (1, 1, 1), (8, 3, 4)),
                               ("fse", (2, 2, 2), ((_flat(36, 6, {0, 1, 2, 3, 4, 5, 8}), 6), (_flat(32, 5, {0, 1, 2, 3, 5}), 5), (_flat(53, 7, {0, 1, 2, 3, 4, 5, 6}), 7)))):
        s = [(8, 8 + 2, 7)] * 6 if name == "rle" else seqs  # (one symbol per table: every sequence has the same codes)
        spec = [(lits[:60], s, modes, given), (lits[60:120], s, (3, 3, 3), None), (lits[120:180], seqs, (0, 0, 0), None), (lits[:40], seqs, (3, 3, 3), None)]
        payloads = compressed_blocks(spec)
        text = execute([(l, q) for l, q, _, _ in spec])
        out["crafted-modes-%s-then-repeat" % name] = (frame([block(2, p, last=k == len(payloads) - 1) for k, p in enumerate(payloads)]), text)
    # the repeat offsets at a block start: the second block's first sequence takes value v with and without literals
    for v in (1, 2, 3):
        for ll in (0, 3):
            first = [(10, 9 + 3, 4), (5, 17 + 3, 4), (9, 30 + 3, 5)]
            spec = [(lits[:40], first, (0, 0, 0), None), (lits[40:80], [(ll, v, 6), (2, 1, 3)], (0, 0, 0), None)]
            payloads = compressed_blocks(spec)
            out["crafted-repeat-%d-%s-at-block-start" % (v, "ll0" if ll == 0 else "ll")] = (
                frame([block(2, p, last=k == 1) for k, p in enumerate(payloads)]), execute([(l, q) for l, q, _, _ in spec]))
    # 127 and 128 sequences (the count's one- and two-byte form), and a raw block between two blocks of which the second repeats
    for n in (127, 128):
        s = [(4, 3 + 3, 3)] + [(1, 3 + 3, 3)] * (n - 1)
        spec = [((lits * 2)[:n + 7], s, (0, 0, 0), None)]
        out["crafted-%d-sequences" % n] = (frame([block(2, compressed_blocks(spec)[0], last=True)]), execute([(spec[0][0], s)]))
    same_ll = [(8, 7 + 3, 5), (8, 1, 4), (8, 2, 6), (8, 40 + 3, 7)]
    spec = [(lits[:50], same_ll, (1, 0, 2), (8, None, (_flat(53, 6, {0, 1, 2, 3, 4, 5, 6}), 6))), (lits[50:90], same_ll, (3, 3, 3), None)]
    p = compressed_blocks(spec)
    full = execute([(spec[0][0], same_ll), (b"raw block in between", []), (spec[1][0], same_ll)])
    out["crafted-repeat-across-a-raw-block"] = (frame([block(2, p[0]), block(0, b"raw block in between"), block(2, p[1], last=True)]), full)
    return out


@functools.lru_cache(maxsize=None)
def damaged():
    lits = bytes(range(65, 91)) * 4
    out = {}
    one = [(8, 7 + 3, 5)]
    # Repeat in a frame's first block
    good = compressed_blocks([(lits[:20], one, (0, 0, 0), None)])[0]
    at = len(literals_raw(lits[:20])) + 1
    bad = bytearray(good)
    bad[at] = 0xFC
    out["crafted-repeat-in-first-block"] = frame([block(2, bytes(bad), last=True)])
    # an accuracy log above the table's limit (LL: 9)
    desc = bytearray(fse_description(_flat(36, 6, {0, 1, 2, 3, 4}), 6))
    desc[0] = (desc[0] & 0xF0) | (10 - 5)
    payload = literals_raw(lits[:20]) + bytes([1, 2 << 6]) + bytes(desc) + b"\x01\x01"
    out["crafted-accuracy-log-10"] = frame([block(2, payload, last=True)])
    # Huffman weights 3 and 1: they sum to 5, what is missing to 8 is no power of two
    payload = (2 | 0 << 2 | 4 << 4 | 3 << 14).to_bytes(3, "little") + bytes([129, 3 << 4 | 1, 0x01]) + b"\x00"
    out["crafted-weights-do-not-sum"] = frame([block(2, payload, last=True)])
    # an offset one byte in front of the frame: 4 literals, then offset 5
    out["crafted-offset-in-front-of-frame"] = frame([block(2, compressed_blocks([(lits[:20], [(4, 5 + 3, 5)], (0, 0, 0), None)])[0], last=True)])
    # treeless literals with no tree before them
    payload = (3 | 0 << 2 | 4 << 4 | 1 << 14).to_bytes(3, "little") + b"\x01" + b"\x00"
    out["crafted-treeless-first"] = frame([block(2, payload, last=True)])
    # libzstd's bounds on a compressed block: 3 bytes at the least, less than 128 KiB
    out["crafted-compressed-block-of-2-bytes"] = frame([block(2, b"\x00\x00", last=True)])
    big = (bytes(range(256)) * 512)[:131068]
    out["crafted-compressed-block-of-128-kib"] = frame([block(2, literals_raw(big, 3) + b"\x00", last=True)], window_log=18)
    return out


PATCHED_STATUS = {"crafted-compressed-block-of-2-bytes": -6, "crafted-compressed-block-of-128-kib": -6,
                  "crafted-repeat-in-first-block": -13, "crafted-accuracy-log-10": -10, "crafted-weights-do-not-sum": -8,
                  "crafted-offset-in-front-of-frame": -17, "crafted-treeless-first": -13}
