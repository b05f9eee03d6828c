"""`tag` SAM text -> BAM with the records encoded on the device (mk_tag_sam_bam_window, an addition to ABI v7; kernels: sam.hip).
The expected bytes come from `encode` below: a restatement of the SAM specification's BAM record layout (section 4.2) and of the
entry point's contract in include/merkurio_hip.h, written here in Python with exact rational arithmetic for the floats -- it shares
no code with the library.  The oracle's tag_records + tag_value supply keep, values, rows and counters, as in test_gpu_sam_window.py.
Every input outside test_refusals is one the device takes: each test asserts status == 0."""
import random
import struct

import numpy as np
import pytest

import oracle_binding as ob
from tag_windows import existing_value, inflate, patterns31, records_of

pytestmark = pytest.mark.gpu
REFS = [b"chr1", b"chr2", b"chrM", b"chr2", b"HLA-A*01:01", b"="]  # (a duplicate: the first one counts)


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def codec(mk):
    c = mk.Codec(0)
    yield c
    c.close()


# ---- the BAM record of a SAM line (SAM specification 4.2, 4.2.4 for the optional fields, 5.3 for the bin)
def f32_bits(spelling):
    """the IEEE single nearest (ties to even) to the decimal number `spelling`, by integer arithmetic"""
    s = spelling.decode().lower()
    neg = s.startswith("-")
    s = s.lstrip("+-")
    mant, _, ex = s.partition("e")
    ip, _, fp = mant.partition(".")
    num, den = int(ip + fp), 1
    e10 = int(ex or 0) - len(fp)
    if e10 >= 0:
        num *= 10 ** e10
    else:
        den = 10 ** -e10
    sign = 0x80000000 if neg else 0
    if num == 0:
        return sign
    e = num.bit_length() - den.bit_length() - 24
    while True:  # q = num / den / 2^e in [2^23, 2^24)
        n2, d2 = (num << -e, den) if e < 0 else (num, den << e)
        q, r = divmod(n2, d2)
        if q >= 1 << 24:
            e += 1
        elif q < 1 << 23:
            e -= 1
        else:
            break
    if 2 * r > d2 or (2 * r == d2 and q & 1):
        q += 1
        if q == 1 << 24:
            q, e = 1 << 23, e + 1
    assert -126 <= e + 23 <= 127
    return sign | (e + 23 + 127) << 23 | (q & 0x7FFFFF)


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


NIB = {c: k for k, c in enumerate(b"=ACMGRSVTWYHKDBN")}
NIB.update({c + 32: k for c, k in list(NIB.items()) if 65 <= c <= 90})
INT_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}


def encode(line, refs):
    """line = the SAM line with the tag field appended -> block_size | record"""
    f = line.split(b"\t")
    assert len(f) >= 11
    ids = {}
    for k, nm in enumerate(refs):
        ids.setdefault(nm, k)
    rid = -1 if f[2] == b"*" else ids.get(f[2], -1)
    nrid = rid if f[6] == b"=" else (-1 if f[6] == b"*" else ids.get(f[6], -1))
    pos, npos = int(f[3]) - 1, int(f[7]) - 1
    ops, span = [], 0
    if f[5] != b"*":
        num = b""
        for ch in f[5]:
            if 48 <= ch <= 57:
                num += bytes([ch])
            else:
                op = b"MIDNSHP=X".index(bytes([ch]))
                ops.append((int(num) << 4 | op) & 0xFFFFFFFF)
                if op in (0, 2, 3, 7, 8):
                    span += int(num)
                num = b""
        assert num == b""
    seq = b"" if f[9] == b"*" else f[9]
    packed = bytearray((len(seq) + 1) // 2)
    for k, ch in enumerate(seq):
        packed[k >> 1] |= NIB.get(ch, 15) << (4 if k % 2 == 0 else 0)
    qual = b"\xff" * len(seq) if f[10] == b"*" else bytes((q - 33) & 255 for q in f[10])
    assert len(qual) == len(seq)
    body = struct.pack("<iiBBHHHiiii", rid, pos, len(f[0]) + 1, int(f[4]) & 255, reg2bin(pos, pos + (span or 1)) & 0xFFFF, len(ops), int(f[1]) & 0xFFFF,
                       len(seq), nrid, npos, int(f[8]))
    body += f[0] + b"\0" + b"".join(struct.pack("<I", o) for o in ops) + bytes(packed) + qual
    for t in f[11:]:
        assert len(t) >= 5 and t[2:3] == b":" and t[4:5] == b":"
        ty, v = t[3:4], t[5:]
        body += t[:2]
        if ty == b"A":
            body += b"A" + (v[:1] or b"\0")
        elif ty == b"i":
            x = int(v)
            if x >= 0:
                body += b"C" + struct.pack("<B", x) if x <= 0xff else b"S" + struct.pack("<H", x) if x <= 0xffff else b"I" + struct.pack("<I", x & 0xFFFFFFFF)
            else:
                body += b"c" + struct.pack("<b", x) if x >= -128 else b"s" + struct.pack("<h", x) if x >= -32768 else b"i" + struct.pack("<I", x & 0xFFFFFFFF)
        elif ty == b"f":
            body += b"f" + struct.pack("<I", f32_bits(v))
        elif ty in (b"Z", b"H"):
            body += ty + v + b"\0"
        elif ty == b"B":
            sub, items = v[:1], v[2:].split(b",") if len(v) > 1 else []
            body += b"B" + sub + struct.pack("<i", len(items))
            for it in items:
                if sub == b"f":
                    body += struct.pack("<I", f32_bits(it))
                else:
                    size = struct.calcsize(INT_FMT[sub])
                    body += (int(it) & ((1 << 8 * size) - 1)).to_bytes(size, "little")
        else:
            raise AssertionError(t)
    return struct.pack("<i", len(body)) + body


# ---- lines
def float_spelling(rnd):
    """a float inside the device's rule: digits with the point dropped below 2^24, net power of ten within +-10"""
    m = rnd.choice((0, 1, 5, 15, 123, 9999, rnd.randrange(1 << 24), rnd.randrange(1000)))
    d = str(m)
    kind = rnd.randrange(4)
    sign = rnd.choice(("", "", "-", "+"))
    if kind == 0:
        return (sign + d).encode()
    if kind == 1:  # a point inside or in front of the digits, at most 10 digits behind it
        k = rnd.randrange(0, min(10, len(d)) + 1)
        k = max(k, 1)
        d = d.rjust(k + 1, "0")
        return (sign + d[:-k] + "." + d[-k:]).encode()
    if kind == 2:
        return ("%s%s%s%d" % (sign, d, rnd.choice("eE"), rnd.randrange(-10, 11))).encode()
    k = rnd.randrange(1, min(5, len(d)) + 1)
    d = d.rjust(k + 1, "0")
    return ("%s%s.%se%s%02d" % (sign, d[:-k], d[-k:], rnd.choice(("-", "+", "")), rnd.randrange(0, 6))).encode()


def int_spelling(rnd):
    x = rnd.choice((0, 1, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 32 - 1, -1, -128, -129, -32768, -32769, -2 ** 31, rnd.randrange(-10 ** 6, 10 ** 6)))
    return (rnd.choice(("", "", "+")) + str(x)).encode() if x >= 0 else str(x).encode()


def aux_fields(rnd, many=False):
    kinds = [lambda: b"NM:i:" + int_spelling(rnd), lambda: b"AS:i:%d" % rnd.randrange(1000), lambda: b"RG:Z:grp%d" % rnd.randrange(4),
             lambda: b"XA:A:" + rnd.choice((b"q", b"", b"!", b"xyz")), lambda: b"XH:H:" + rnd.choice((b"0AFF", b"", b"1a")),
             lambda: b"XF:f:" + float_spelling(rnd), lambda: b"XZ:Z:" + rnd.choice((b"", b"a b:c;d", b"z" * rnd.randrange(300))),
             lambda: b"MD:Z:%d" % rnd.randrange(200)]
    for sub, lo, hi in ((b"c", -128, 127), (b"C", 0, 255), (b"s", -32768, 32767), (b"S", 0, 65535), (b"i", -2 ** 31, 2 ** 31 - 1), (b"I", 0, 2 ** 32 - 1)):
        kinds.append(lambda sub=sub, lo=lo, hi=hi: b"B%s:B:%s" % (sub, sub) + b"".join(b",%d" % rnd.choice((lo, hi, rnd.randrange(lo, hi + 1)))
                                                                                       for _ in range(rnd.choice((0, 1, 3, 40)))))
    kinds.append(lambda: b"Bf:B:f" + b"".join(b"," + float_spelling(rnd) for _ in range(rnd.choice((0, 1, 5)))))
    n = rnd.randrange(33, 60) if many else rnd.randrange(0, 8)
    return [rnd.choice(kinds)() for _ in range(n)]


def cigar(rnd, n_ops):
    return b"".join(b"%d%c" % (rnd.choice((0, 1, 7, 150, 999999999, rnd.randrange(1000))), rnd.choice(b"MIDNSHP=X")) for _ in range(n_ops)) or b"*"


def sam_line(rnd, i, patterns, lens=(150,), hit=0.2, alpha=b"ACGT", lower=0.0, eol=b"\n", refs=REFS, aux=True, n_ops=None, star_qual=0.1):
    L = rnd.choice(lens)
    s = bytearray(rnd.choice(alpha) for _ in range(L))
    if patterns and rnd.random() < hit:
        for _ in range(rnd.choice((1, 1, 2, 3))):
            p = rnd.choice(patterns)
            if len(p) <= L:
                k = rnd.randrange(0, L - len(p) + 1)
                s[k:k + len(p)] = p
    if rnd.random() < lower:
        s = bytearray(bytes(s).lower())
    unmapped = rnd.random() < 0.15
    rname = b"*" if unmapped else rnd.choice(list(refs) + [b"unknown_contig"])
    qual = b"*" if (L == 0 or rnd.random() < star_qual) else bytes(rnd.randrange(33, 127) for _ in range(L))
    f = [b"read%d_%d" % (i, rnd.randrange(10 ** 6)), b"%d" % rnd.choice((0, 4, 99, 147, 65535, 2048)), rname, b"0" if unmapped else b"%d" % rnd.randrange(1, 2 ** 29),
         b"%d" % rnd.choice((0, 60, 255)), b"*" if unmapped else cigar(rnd, rnd.choice((0, 1, 1, 2, 5)) if n_ops is None else n_ops),
         rnd.choice((b"=", b"*", b"chr2", b"nope")), b"%d" % rnd.randrange(0, 2 ** 29), b"%d" % rnd.randrange(-10 ** 6, 10 ** 6), bytes(s) if L else b"*", qual]
    if aux:
        f += aux_fields(rnd, many=rnd.random() < 0.03)
    return b"\t".join(f) + eol


def expected(om, patterns, text, tag, logging, fm, inv, refs=REFS, last=True):
    recs, _ = records_of(text, last)
    keep, rows, c, found = ob.tag_records(om, [r[2] for r in recs], logging=logging, filter_matching=fm, invert=inv)
    out = bytearray()
    for (ln, _, _, aux), k, f in zip(recs, keep, found):
        if k:
            ex = existing_value(aux, tag)
            out += encode(ln + b"\t" + tag + b":Z:" + ob.tag_value(patterns, f, ex if ex else None), refs)
    return keep, [(recs[rec][1], rec, pat, pos) for (_, rec, pat, pos) in rows], c, bytes(out), len(recs)


def first_difference(got, want):
    """which record differs, for the failure message"""
    a = b = k = 0
    while a < len(got) and b < len(want):
        la, lb = struct.unpack_from("<i", got, a)[0] + 4, struct.unpack_from("<i", want, b)[0] + 4
        if got[a:a + la] != want[b:b + lb]:
            return f"record {k}: got {got[a:a + la][:400]!r} want {want[b:b + lb][:400]!r}"
        a, b, k = a + la, b + lb, k + 1
    return f"{len(got)} / {len(want)} bytes"


def check(res, keep, rows, c, out, n_rec, logging):
    assert all(x["status"] == 0 for x in res), [x["status"] for x in res]
    assert sum(x["n_rec"] for x in res) == n_rec and sum(x["n_kept"] for x in res) == sum(keep)
    got = b"".join(inflate(x["out"]) for x in res)
    assert got == out, first_difference(got, out)
    assert sum(x["out_text_bytes"] for x in res) == len(out)
    if logging:
        got_rows, base = [], 0
        for x in res:
            got_rows += [(nm, rec + base, pat, pos) for (nm, rec, pat, pos) in x["rows"]]
            base += x["n_rec"]
        assert got_rows == rows
        for k in ("records", "bases"):
            assert sum(x["counters"][k] for x in res) == c[k]
        assert sum(x["counters"]["hits"][0] for x in res) == c["hits"][0] and sum(x["counters"]["records_hit"][0] for x in res) == c["records_hit"][0]
        assert np.array_equal(np.sum([x["counters"]["pattern_hit_counts"] for x in res], axis=0), c["pattern_hit_counts"])
    assert sum(x["counters"]["extracted"] for x in res) == sum(keep)


def run_windows(m, codec, text, cuts, **kw):
    head, res = b"", []
    for i in range(len(cuts) - 1):
        r = m.tag_sam_bam_window(codec, head, text[cuts[i]:cuts[i + 1]], last=(i == len(cuts) - 2), **kw)
        res.append(r)
        if r["status"]:
            break
        head = r["tail"]
    return res


def test_the_restatement_knows_a_record_by_hand():
    """(no device) one record checked against bytes written out by hand from the specification"""
    line = b"r1\t99\tchr2\t100\t60\t3M1D2S\t=\t200\t-50\tACgTN\tI!~JK\tNM:i:-1\tXF:f:1.5\tkm:Z:AC"
    want = struct.pack("<iiBBHHHiiii", 1, 99, 3, 60, 4681, 3, 99, 5, 1, 199, -50) + b"r1\0" + struct.pack("<III", 3 << 4, 1 << 4 | 2, 2 << 4 | 4)
    want += bytes([0x12, 0x48, 0xF0]) + bytes([40, 0, 93, 41, 42]) + b"NMc\xff" + b"XFf" + struct.pack("<f", 1.5) + b"kmZAC\0"
    assert encode(line, REFS) == struct.pack("<i", len(want)) + want
    assert f32_bits(b"0.1") == 0x3DCCCCCD and f32_bits(b"-0") == 0x80000000 and f32_bits(b"16777215e10") == struct.unpack("<I", struct.pack("<f", 16777215e10))[0]


@pytest.mark.parametrize("filter_matching,invert", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("logging", [True, False])
def test_window_matches_the_host_encoding(mk, codec, filter_matching, invert, logging):
    rnd = random.Random(11)
    pats = patterns31(mk)
    text = b"".join(sam_line(rnd, i, pats) for i in range(3000))
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", logging, filter_matching, invert)
    r = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, logging=logging, filter_matching=filter_matching, invert=invert)
    assert r["n_rec"] == n_rec == 3000 and r["n_window"] == r["n_used"] == len(text) and r["tail"] == b""
    check([r], keep, rows, c, out, n_rec, logging)
    if logging:
        got, want = dict(r["counters"]), dict(c)
        got.pop("extracted"), want.pop("extracted")
        assert got == want


def test_bndmq_counts(mk, codec):
    rnd = random.Random(9)
    pats = mk.parse_pattern_list(kmer_seq=[b"ACGTACG", b"NNRYK", b"GATTACA", b"TTT"])
    text = b"".join(sam_line(rnd, i, pats, lens=(40, 41, 90), hit=0.5, alpha=b"ACGTNRYKMSWBDHV") for i in range(800))
    m = mk.Matcher(pats, device=0)
    assert not m.use_ac
    om = ob.Matcher(pats, False, 0, False)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, True, False)
    r = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, filter_matching=True)
    check([r], keep, rows, c, out, n_rec, True)
    assert r["counters"]["pattern_hit_counts"] == c["pattern_hit_counts"] and r["counters"]["hits"] == c["hits"]


def test_every_optional_field_type(mk, codec):
    """A (with and without a value), i at every width boundary, f, Z, H, B of every subtype with 0 ... 40 items, records with more
    than 32 optional fields"""
    rnd = random.Random(21)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    lines = []
    for i in range(1500):
        base = sam_line(rnd, i, pats, lens=(50,), hit=0.5, aux=False, eol=b"")
        lines.append(b"\t".join([base] + aux_fields(rnd, many=(i % 10 == 0))) + b"\n")
    boundary = [b"%s:i:%d" % (b"X%c" % (65 + k % 26), x) for k, x in enumerate((0, 255, 256, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 10 ** 18 - 1, -1, -128, -129, -32768,
                                                                               -32769, -2 ** 31, -2 ** 31 - 1, -10 ** 18 + 1))]
    lines.append(b"\t".join([sam_line(rnd, 9999, pats, lens=(50,), aux=False, eol=b"")] + boundary) + b"\n")
    assert max(ln.count(b"\t") for ln in lines) > 10 + 32
    text = b"".join(lines)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, False, False)
    check([m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS)], keep, rows, c, out, n_rec, True)


def test_existing_tag_values_are_merged_and_the_old_field_stays(mk, codec):
    rnd = random.Random(8)
    pats = patterns31(mk, 30)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    values = [b"", b"ZZZ", b"TTT,AAA,CCC", b"AAA,AAA,AAA", b",,", b"x,", b",x", pats[3], pats[5] + b"," + pats[1], b"a," + pats[0] + b",B,b,A", b"ACGT" * 100]
    lines = []
    for i in range(600):
        base = sam_line(rnd, i, pats[:8], lens=(120,), hit=0.7, aux=False, eol=b"")
        mine = [b"km:Z:" + rnd.choice(values)] if i % 3 else []
        aux = [[b"NM:i:2"] + mine, mine + [b"AS:i:%d" % i], [b"XL:Z:" + b"q" * 300] + mine + [b"NM:i:1"], mine][i % 4]
        lines.append(b"\t".join([base] + aux) + b"\n")
    text = b"".join(lines)
    for fm in (False, True):
        keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, fm, False)
        check([m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, filter_matching=fm)], keep, rows, c, out, n_rec, True)
    assert out.count(b"kmZ") > sum(keep)  # (old fields are still there beside the new ones)


def test_seq_and_qual_shapes(mk, codec):
    """SEQ '*', QUAL '*', every length 0 ... 70 and odd / even lengths up to 2 500, lower case, IUPAC and other bytes"""
    rnd = random.Random(5)
    pats = patterns31(mk, 50)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    lens = list(range(0, 71)) + [127, 128, 129, 255, 256, 257, 271, 272, 273, 511, 512, 513, 1000, 1001, 2499, 2500]
    lines = []
    for rep in range(3):
        for i, L in enumerate(lens):
            lines.append(sam_line(rnd, i, pats, lens=(L,), hit=0.5, alpha=b"ACGTNacgtn=RYKMSWBDHVrykmswbdhvXxEe.-", lower=0.3, star_qual=(0.0, 1.0, 0.3)[rep]))
    text = b"".join(lines)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, False, False)
    check([m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS)], keep, rows, c, out, n_rec, True)


def test_cigars(mk, codec):
    """0 ('*'), 1, 64, 65 and 3 000 ops, every op, lengths 0 and 999 999 999 (whose << 4 wraps in 32 bits), an empty CIGAR field"""
    rnd = random.Random(6)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    lines = [sam_line(rnd, i, pats, lens=(60,), hit=0.5, n_ops=n) for i, n in enumerate([0, 1, 2, 9, 63, 64, 65, 66, 200, 3000] * 8)]
    f = lines[0].split(b"\t")
    lines.append(b"\t".join(f[:5] + [b"1M2I3D4N5S6H7P8=9X"] + f[6:]))
    lines.append(b"\t".join(f[:2] + [b"chr1", b"7", b"60", b""] + f[6:]))
    text = b"".join(lines)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, False, False)
    check([m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS)], keep, rows, c, out, n_rec, True)


def test_reference_names(mk, codec):
    """unmapped records (POS 0, RNAME '*': bin 4680), RNEXT '=', unknown names, of duplicate names the first, a name that is '=',
    no names at all; then 100 000 names"""
    rnd = random.Random(7)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    lines = []
    for i in range(800):
        f = sam_line(rnd, i, pats, lens=(40,), hit=0.5, eol=b"").split(b"\t")
        f[2] = rnd.choice(REFS + [b"*", b"chr", b"chr11", b"CHR1", b""])
        f[6] = rnd.choice(REFS + [b"*", b"=", b"chr", b""])
        if f[2] == b"*":
            f[3], f[5] = b"0", b"*"
        lines.append(b"\t".join(f) + b"\n")
    text = b"".join(lines)
    unmapped = encode(b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\tkm:Z:", REFS)
    assert struct.unpack_from("<iiBBH", unmapped, 4) == (-1, -1, 2, 0, 4680)
    for refs in (REFS, [], [b"chr1"]):
        keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, False, False, refs=refs)
        check([m.tag_sam_bam_window(codec, b"", text, last=True, refs=refs)], keep, rows, c, out, n_rec, True)
    many = [b"contig_%d_%d" % (k, (k * 7919) % 1000) for k in range(100000)]
    many[500], many[70000] = many[400], many[3]  # duplicates
    lines = []
    for i in range(3000):
        f = sam_line(rnd, i, pats, lens=(40,), hit=0.5, eol=b"").split(b"\t")
        f[2] = rnd.choice((many[rnd.randrange(100000)], many[400], many[3], many[99999], many[0], b"contig_1", b"*"))
        f[6] = rnd.choice((many[rnd.randrange(100000)], b"=", b"*"))
        if f[2] == b"*":
            f[3], f[5] = b"0", b"*"
        lines.append(b"\t".join(f) + b"\n")
    text = b"".join(lines)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, False, False, refs=many)
    check([m.tag_sam_bam_window(codec, b"", text, last=True, refs=many)], keep, rows, c, out, n_rec, True)


def ragged_text(rnd, pats, n=1200):
    parts = []
    for i in range(n):
        parts.append(sam_line(rnd, i, pats, lens=(0, 1, 31, 150, 2500), hit=0.4, alpha=b"ACGTN", lower=0.3, eol=rnd.choice((b"\n", b"\r\n"))))
        if i % 97 == 5:
            parts.append(rnd.choice((b"\n", b"\r\n", b"@CO\ta comment in the middle\n", b"@SQ\tSN:chr1\tLN:5\r\n")))
    return b"".join(parts)


def test_ragged_lines_window_cuts_and_block_bytes(mk, codec):
    """CRLF mixed with LF, header and empty lines between records, a last line without a line end; windows cut at arbitrary bytes
    with the tail carried as the next head; members of 300 bytes, 4 KiB and the default"""
    rnd = random.Random(5)
    pats = patterns31(mk, 50)
    text = ragged_text(rnd, pats)[:-1]
    assert not text.endswith(b"\n")
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"XK", True, False, False)
    for bb in (0, 300, 4096):
        one = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, tag=b"XK", block_bytes=bb)
        check([one], keep, rows, c, out, n_rec, True)
        n_members = len(mk.bgzf_members(one["out"])[0])
        assert n_members == (len(out) + (bb or 65280) - 1) // (bb or 65280)
    keep2, rows2, c2, out2, n_rec2 = expected(om, pats, text, b"XK", True, False, False, last=False)
    part = m.tag_sam_bam_window(codec, b"", text, last=False, refs=REFS, tag=b"XK")
    check([part], keep2, rows2, c2, out2, n_rec2, True)
    cut = text.rfind(b"\n") + 1
    assert n_rec2 == n_rec - 1 and part["n_used"] == cut and part["tail"] == text[cut:]
    for n_cuts in (1, 7, 60):
        cuts = [0] + sorted(rnd.randrange(1, len(text)) for _ in range(n_cuts)) + [len(text)]
        check(run_windows(m, codec, text, cuts, refs=REFS, tag=b"XK"), keep, rows, c, out, n_rec, True)


def test_no_output_and_empty_windows(mk, codec):
    rnd = random.Random(4)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    text = b"".join(sam_line(rnd, i, pats, hit=0.0) for i in range(300))
    r = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, filter_matching=True)
    assert r["status"] == 0 and r["n_kept"] == 0 and r["out"] == b"" and r["n_rec"] == 300 and r["counters"]["records"] == 300
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, False, False)
    r = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, write=False)  # out == NULL: the checks run, sizes are reported
    assert r["status"] == 0 and r["out"] == b"" and r["n_kept"] == 300 and r["out_text_bytes"] == len(out) and r["counters"]["records"] == 300
    r = m.tag_sam_bam_window(codec, b"", b"", last=True, refs=REFS)
    assert r["status"] == 0 and r["n_rec"] == 0 and r["n_window"] == 0
    r = m.tag_sam_bam_window(codec, b"", b"@HD\tVN:1.6\n\n\r\n", last=True, refs=REFS)
    assert r["status"] == 0 and r["n_rec"] == 0 and r["n_used"] == 14 and r["out"] == b""


def test_capacity_exact_fit_and_one_short(mk, codec):
    """out, rows and names: a buffer of exactly the need is taken, one entry / byte less returns MK_E_CAPACITY with the need and
    counts nothing"""
    import ctypes as C
    rnd = random.Random(12)
    pats = patterns31(mk, 40)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    text = b"".join(sam_line(rnd, i, pats, hit=0.6) for i in range(500))
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, True, False)
    full = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, filter_matching=True)
    check([full], keep, rows, c, out, n_rec, True)
    tb = np.frombuffer(text, dtype=np.uint8)
    ref_bytes = np.frombuffer(b"".join(REFS), dtype=np.uint8)
    ref_off = np.array([0] + list(np.cumsum([len(r) for r in REFS])), dtype=np.uint64)

    def call(out_cap, rows_cap, names_cap):
        w = mk.SamBamWindow()
        w.text, w.n_text, w.last, w.filter_matching = tb.ctypes.data, len(tb), 1, 1
        w.tag[0], w.tag[1] = b"km"
        w.ref_names, w.ref_off, w.n_refs = ref_bytes.ctypes.data, ref_off.ctypes.data, len(REFS)
        bufs = (np.zeros(max(out_cap, 1) + 8, dtype=np.uint8), np.zeros(max(rows_cap, 1) + 1, dtype=mk.ROW_DTYPE), np.zeros(max(rows_cap, 1) + 1, dtype=np.uint64),
                np.zeros(max(names_cap, 1) + 8, dtype=np.uint8), np.zeros(64, dtype=np.uint8))
        bufs[0][out_cap:] = 0xA5
        bufs[3][names_cap:] = 0xA5
        w.out, w.out_cap, w.rows, w.rows_cap, w.row_name, w.names, w.names_cap = (bufs[0].ctypes.data, out_cap, bufs[1].ctypes.data, rows_cap, bufs[2].ctypes.data,
                                                                                  bufs[3].ctypes.data, names_cap)
        w.tail, w.tail_cap = bufs[4].ctypes.data, 64
        cnt, k2, status = mk.Counters(), np.zeros(len(pats), dtype=np.uint32), C.c_uint32()
        rc = mk.load().mk_tag_sam_bam_window(m._h, codec._h, C.byref(w), 1, C.byref(cnt), k2.ctypes.data, C.byref(status))
        assert bytes(bufs[0][out_cap:]) == b"\xa5" * 8 and bytes(bufs[3][names_cap:]) == b"\xa5" * 8  # nothing behind the capacity was touched
        return rc, w, cnt, k2, status.value, bufs

    rc, w, cnt, k2, status, bufs = call(1 << 22, 1 << 16, 1 << 20)
    assert rc == 0 and status == 0
    need = dict(out=int(w.out_len), rows=int(w.n_rows), names=int(w.n_names_bytes))
    assert need["out"] == len(full["out"]) and need["rows"] == len(rows)
    rc, w, cnt, k2, status, bufs = call(need["out"], need["rows"], need["names"])
    assert rc == 0 and status == 0 and inflate(bytes(bufs[0][:need["out"]])) == out and cnt.nb_records_tot == 500
    for short in ("out", "rows", "names"):
        caps = dict(need)
        caps[short] -= 1
        rc, w, cnt, k2, status, bufs = call(caps["out"], caps["rows"], caps["names"])
        assert rc == mk.MK_E_CAPACITY and status == 0
        assert (int(w.out_len), int(w.n_rows), int(w.n_names_bytes))[("out", "rows", "names").index(short)] == need[short]
        assert cnt.nb_records_tot == 0 and cnt.nb_records_extracted == 0 and cnt.nb_hits_tot[0] == 0 and not k2.any()


def test_refusals(mk, codec):
    """one case per refusal of the contract: the status bit, nothing produced, nothing counted -- and the same line is taken when
    the record that carries it is dropped"""
    rnd = random.Random(2)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    good = [sam_line(rnd, i, pats, hit=0.5) for i in range(50)]
    hit_seq = pats[0] + b"A" * 40

    def line(aux=(), n_fields=11, **over):
        f = [b"name", b"0", b"chr1", b"100", b"60", b"71M", b"*", b"0", b"0", hit_seq, b"F" * len(hit_seq)]
        for k, v in over.items():
            f[int(k[1:])] = v
        return b"\t".join(f[:n_fields] + list(aux)) + b"\n"

    def run(lines, **kw):
        return m.tag_sam_bam_window(codec, b"", b"".join(lines), last=True, refs=REFS, **kw)

    def refused(bad, bit, has_hit=True):
        r = run(good + [bad] + good)
        assert r["status"] == bit, (bad, r["status"])
        assert r["out"] == b"" and r["n_kept"] == 0 and r["out_text_bytes"] == 0
        assert r["counters"]["records"] == 0 and r["counters"]["extracted"] == 0 and r["counters"]["hits"][0] == 0 and not any(r["counters"]["pattern_hit_counts"])
        # (a record with a hit: -v drops it, and a dropped record is not looked at -- unless the line itself is too short)
        assert run(good + [bad] + good, invert=True)["status"] == (1 if bad.count(b"\t") < 9 else 0 if has_hit else bit)

    assert run(good + [line([b"NM:i:1"])] + good)["status"] == 0
    refused(line(n_fields=9), 1)                       # fewer than 10 fields
    refused(line(n_fields=10), 1)                      # a kept line with fewer than 11
    refused(line(f0=b"q" * 255), 2)                    # QNAME longer than 254 bytes
    assert run(good + [line(f0=b"q" * 254)])["status"] == 0
    for cig in (b"71", b"M", b"7M1", b"71Q", b"71m", b"1234567890M", b"-1M", b"7 M", b"1M" * 65536):
        refused(line(f5=cig), 2)                       # a byte that is no op, a length that is not 1-9 digits, more than 65 535 ops
    assert run(good + [line(f5=b"1M" * 65535)])["status"] == 0
    refused(line(f10=b"F" * 70), 2)                    # QUAL of another length than SEQ
    refused(line(f9=b"*", f10=b"F"), 2, has_hit=False)  # (no SEQ, no hit: -v keeps it)
    for k in (1, 3, 4, 7, 8):                          # FLAG POS MAPQ PNEXT TLEN that are not plain integers
        for v in (b"", b"x", b"1x", b" 1", b"1.0", b"0x10", b"1234567890123456789"):
            refused(line(**{"f%d" % k: v}), 2)
    for aux in (b"NM:i:", b"NM:i:x", b"NM:i:1 ", b"NM:i:1e3", b"NM:i:1234567890123456789",                # integers
                b"XF:f:inf", b"XF:f:nan", b"XF:f:0x1p3", b"XF:f:16777216", b"XF:f:1e11", b"XF:f:1e-11", b"XF:f:", b"XF:f:1.5x", b"XF:f:.5", b"XF:f: 1",
                b"XX:i", b"XX:", b"X", b"", b"XXi:1:", b"XX:i1:", b"XX;i:1",                              # shorter than 5 bytes, colons
                b"XX:q:1", b"XX:I:1", b"XX:z:a",                                                          # unknown types
                b"XB:B:", b"XB:B:q,1", b"XB:B:Z,1", b"XB:B:c1,2", b"XB:B:c,", b"XB:B:c,1,", b"XB:B:c,,1", b"XB:B:c,x", b"XB:B:f,nan", b"XB:B:f,1e11"):
        refused(line([b"AS:i:5", aux]), 2)
        refused(line([aux, b"AS:i:5"]), 2)
    refused(line([b"AS:i:5"])[:-1] + b"\t\n", 2)       # an empty field behind a final tab
    refused(line()[:-1] + b"\t\n", 2)
    refused(line([b"NM:i:1", b"km:i:5"]), 4)           # as in mk_tag_sam_window
    r = run(good + [line([b"XF:f:inf"])] + good, write=False)
    assert r["status"] == 2                            # no output asked for: the checks still run


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_windows_against_the_restatement(mk, codec, seed):
    rnd = random.Random(7000 + seed)
    few = rnd.random() < 0.3
    if few:
        pats = mk.parse_pattern_list(kmer_seq=[bytes(rnd.choice(b"ACGT") for _ in range(rnd.choice((5, 9, 21)))) for _ in range(rnd.randrange(1, 9))])
    else:
        pats = patterns31(mk, rnd.choice((20, 300)), seed=seed)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, m.use_ac, 0, False)
    n = rnd.choice((1, 40, 700, 2500))
    lens = rnd.choice(((150,), (0, 1, 2, 33, 150, 151), (100, 3000), (75,)))
    alpha = rnd.choice((b"ACGT", b"ACGTN", b"ACGTNRYKM=xq"))
    hit, lower, crlf = rnd.choice((0.0, 0.1, 0.9)), rnd.choice((0.0, 0.2)), rnd.choice((0.0, 0.0, 0.5, 1.0))
    tag = rnd.choice((b"km", b"XK"))
    carry = rnd.random() < 0.5
    parts = []
    for i in range(n):
        ln = sam_line(rnd, i, pats, lens=lens, hit=hit, alpha=alpha, lower=lower, eol=b"")
        if carry and rnd.random() < 0.3:
            ln += b"\t" + tag + b":Z:" + rnd.choice((b"", b"AAA", b"T,A,T", pats[0], pats[-1] + b",zz", b",", b"b,a,,c"))
        parts.append(ln + (b"\r\n" if rnd.random() < crlf else b"\n"))
        if rnd.random() < 0.02:
            parts.append(rnd.choice((b"\n", b"@CO\tx\n", b"\r\n")))
    text = b"".join(parts)
    if rnd.random() < 0.5 and text.endswith(b"\n") and not text.endswith(b"\r\n"):
        text = text[:-1]
    fm, inv = rnd.choice(((False, False), (True, False), (False, True)))
    logging = rnd.random() < 0.7
    keep, rows, c, out, n_rec = expected(om, pats, text, tag, logging, fm, inv)
    n_cuts = rnd.choice((0, 1, 5, 40))
    cuts = [0] + sorted(rnd.randrange(0, len(text) + 1) for _ in range(n_cuts)) + [len(text)]
    res = run_windows(m, codec, text, cuts, refs=REFS, tag=tag, logging=logging, filter_matching=fm, invert=inv, block_bytes=rnd.choice((0, 0, 1000)))
    assert len(res) == len(cuts) - 1
    check(res, keep, rows, c, out, n_rec, logging)


def test_one_large_window(mk, codec):
    """one window of more than 100 MB: 2 000 distinct lines repeated"""
    rnd = random.Random(13)
    pats = patterns31(mk, 100)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    block = b"".join(sam_line(rnd, i, pats, hit=0.2) for i in range(2000))
    reps = (100 << 20) // len(block) + 1
    text = block * reps
    assert len(text) >= 100 * 10 ** 6
    keep, rows, c, out, n_rec = expected(om, pats, block, b"km", False, True, False)
    r = m.tag_sam_bam_window(codec, b"", text, last=True, refs=REFS, logging=False, filter_matching=True)
    assert r["status"] == 0 and r["n_rec"] == n_rec * reps and r["n_kept"] == sum(keep) * reps and r["out_text_bytes"] == len(out) * reps
    got = inflate(r["out"])
    assert len(got) == len(out) * reps
    assert all(got[k * len(out):(k + 1) * len(out)] == out for k in range(reps))
