"""`tag` BAM -> SAM text with the lines formatted on the device (mk_tag_bam_sam_window, an addition to ABI v7; kernels: bam.hip).
The expected lines come from `sam_line` below, a restatement of the entry point's header comment written from the SAM specification
(§1.4 and §4.2) that shares no code with the library; floats are CPython's '%g' of the unpacked single (correctly rounded).  Keep,
tag values, rows and counters come from the oracle's tag_records + tag_value, as in test_gpu_bam_window.py.  Every input outside the
refusal tests is one the device takes: each such test asserts status == 0."""
import gzip
import os
import random
import struct

import numpy as np
import pytest

import oracle_binding as ob
from tag_windows import NIB, _bgzf, bam_record, patterns31

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFS = [b"chr1", b"2", b"a_rather_long_reference_name.17", b"MT"]
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


# ---- the restatement
def g(b4):
    return ("%g" % struct.unpack("<f", b4)[0]).encode()


INT_TYPES = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}


def sam_line(rec, refs):
    """(line without tag and line end, name, sequence as the matcher sees it) of block_size + record"""
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    p = 36
    name = rec[p:p + l_name - 1]
    p += l_name
    cig = b""
    for k in range(n_cig):
        v = struct.unpack_from("<I", rec, p + 4 * k)[0]
        cig += b"%d" % (v >> 4) + (b"MIDNSHP=X"[v & 15:(v & 15) + 1] if (v & 15) < 9 else b"?")
    p += 4 * n_cig
    seq = bytes(NIB[(rec[p + (k >> 1)] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(l_seq))
    p += (l_seq + 1) // 2
    q = rec[p:p + l_seq]
    p += l_seq
    qual = b"*" if l_seq == 0 or q[0] == 0xFF else bytes((x + 33) & 0xFF for x in q)
    rname = refs[ref] if 0 <= ref < len(refs) else b"*"
    rnext = b"*" if nref < 0 else b"=" if nref == ref else refs[nref] if nref < len(refs) else b"*"
    f = [name, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cig or b"*", rnext, b"%d" % (npos + 1), b"%d" % tlen, seq or b"*", qual]
    while p < len(rec):
        tag, ty = rec[p:p + 2], rec[p + 2]
        p += 3
        if ty == ord("A"):
            f.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif ty in INT_TYPES:
            fmt = INT_TYPES[ty]
            f.append(tag + b":i:%d" % struct.unpack_from(fmt, rec, p)[0])
            p += struct.calcsize(fmt)
        elif ty == ord("f"):
            f.append(tag + b":f:" + g(rec[p:p + 4]))
            p += 4
        elif ty in (ord("Z"), ord("H")):
            e = rec.index(b"\0", p)
            f.append(tag + b":" + bytes([ty]) + b":" + rec[p:e])
            p = e + 1
        elif ty == ord("B"):
            sub, cnt = rec[p], struct.unpack_from("<i", rec, p + 1)[0]
            p += 5
            items = []
            for _ in range(cnt):
                if sub == ord("f"):
                    items.append(g(rec[p:p + 4]))
                    p += 4
                else:
                    items.append(b"%d" % struct.unpack_from(INT_TYPES[sub], rec, p)[0])
                    p += struct.calcsize(INT_TYPES[sub])
            f.append(tag + b":B:" + bytes([sub]) + b"".join(b"," + x for x in items))
        else:
            raise AssertionError("the tests build no such field")
    assert p == len(rec)
    return b"\t".join(f), name, seq


def expected(om, patterns, recs, refs, tag, logging, filter_matching, invert, existing=None):
    dec = [sam_line(r, refs) for r in recs]
    keep, rows, c, found = ob.tag_records(om, [s for _, _, s in dec], logging=logging, filter_matching=filter_matching, invert=invert)
    out = bytearray()
    for i, (k, f) in enumerate(zip(keep, found)):
        if k:
            out += dec[i][0] + b"\t" + tag + b":Z:" + ob.tag_value(patterns, f, existing[i] if existing and existing[i] else None) + b"\n"
    return keep, [(dec[rec][1], rec, pat, pos) for (_, rec, pat, pos) in rows], c, bytes(out)


def check(r, keep, rows, c, out, logging=True):
    assert r["status"] == 0 and r["rc"] == 0
    assert r["n_kept"] == sum(keep) and r["out_len"] == len(out)
    if r["out"] != out:  # (which line differs, for the failure message)
        a, b = r["out"].split(b"\n"), out.split(b"\n")
        bad = [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:2]
        raise AssertionError(f"{len(a)} / {len(b)} lines; first differences {[(a[k], b[k]) for k in bad]}")
    if logging:
        assert r["rows"] == rows
        got, want = dict(r["counters"]), dict(c)
        assert got.pop("extracted") == sum(keep)
        want.pop("extracted")
        assert got == want


def fl(x):
    return struct.pack("<f", x)


# floats inside the rule: ties, both ends, zeros, one digit, six digits, values that round up to the next power of ten
IN_RULE = [fl(131072.5), fl(131073.5), fl(0.0001), fl(999999.4375), fl(0.0), fl(-0.0), fl(1.0), fl(-1.5), fl(0.1), fl(3.14159274), fl(100000.0), fl(99999.95),
           fl(9.9999995), fl(0.00012345), fl(-524292.0), fl(0.5), fl(2.5), fl(1234.5), fl(0.001), fl(65504.0), struct.pack("<I", 0x38D1B714)]
SEQ_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 150, 255, 256, 257, 271, 272, 273, 2500)


def rand_float(rnd):
    if rnd.random() < 0.4:
        return rnd.choice(IN_RULE)
    return struct.pack("<I", rnd.randrange(2) << 31 | rnd.randrange(115, 145) << 23 | rnd.randrange(1 << 23))  # (2^-12 ... 2^18: inside)


def rand_aux(rnd, with_tag=None):
    """optional fields of every type; with_tag: (name, value) of an existing Z field placed somewhere among them"""
    kinds = []
    for _ in range(rnd.randrange(0, 7)):
        t = rnd.choice("AcCsSiIfZHB")
        nm = bytes(rnd.choice(b"XYZN") for _ in range(1)) + bytes([rnd.choice(b"abcdeMD0")])
        if nm == b"km" or nm == b"XK":
            continue
        if t == "A":
            kinds.append(nm + b"A" + bytes([rnd.randrange(33, 127)]))
        elif t in "cCsSiI":
            fmt = INT_TYPES[ord(t)]
            lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (INT32_MIN, INT32_MAX), "I": (0, (1 << 32) - 1)}[t]
            kinds.append(nm + t.encode() + struct.pack(fmt, rnd.choice((lo, hi, 0, rnd.randrange(lo, hi + 1), rnd.randrange(-9, 11) if lo < 0 else rnd.randrange(0, 11)))))
        elif t == "f":
            kinds.append(nm + b"f" + rand_float(rnd))
        elif t in "ZH":
            kinds.append(nm + t.encode() + bytes(rnd.choice(b"0123456789ABCDEF") for _ in range(rnd.choice((0, 1, 8, 40)))) + b"\0")
        else:
            sub = rnd.choice("cCsSiIf")
            cnt = rnd.choice((0, 1, 3, 300))
            if sub == "f":
                items = b"".join(rand_float(rnd) for _ in range(cnt))
            else:
                fmt = INT_TYPES[ord(sub)]
                lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (INT32_MIN, INT32_MAX), "I": (0, (1 << 32) - 1)}[sub]
                items = b"".join(struct.pack(fmt, rnd.choice((lo, hi, rnd.randrange(lo, hi + 1)))) for _ in range(cnt))
            kinds.append(nm + b"B" + sub.encode() + struct.pack("<i", cnt) + items)
    if with_tag is not None:
        kinds.insert(rnd.randrange(len(kinds) + 1), with_tag[0] + b"Z" + with_tag[1] + b"\0")
    return b"".join(kinds)


def rand_record(rnd, pats, i, tag=b"km", hit=0.35, lens=SEQ_LENS, alpha=b"ACGTN"):
    """one record with everything the header comment restates; -> (record, existing value of the tag or None)"""
    L = rnd.choice(lens)
    s = bytearray(rnd.choice(alpha) for _ in range(L))
    if rnd.random() < hit:
        for _ in range(rnd.choice((1, 1, 2, 3))):
            p = rnd.choice(pats)
            if len(p) <= L:
                k = rnd.randrange(0, L - len(p) + 1)
                s[k:k + len(p)] = p
    pick = rnd.randrange(4)
    if pick == 0 or L == 0:
        qual = bytes(rnd.randrange(0, 94) for _ in range(L))
    elif pick == 1:
        qual = b"\xff" * L
    elif pick == 2:  # bytes whose + 33 wraps, and 0xFF behind the first byte
        qual = bytes([rnd.choice((0, 40, 222, 223, 250, 254))]) + bytes(rnd.choice((0, 93, 94, 200, 222, 223, 254, 255)) for _ in range(L - 1))
    else:
        qual = bytes(rnd.randrange(256) for _ in range(L))
        if qual[0] == 0xFF:
            qual = b"\0" + qual[1:]
    ncig = rnd.choice((0, 1, 3, 3, 1000 if i % 97 == 0 else 2))
    cigar = tuple(rnd.choice((1, 9, 10, 150, (1 << 28) - 1, rnd.randrange(1 << 28))) << 4 | rnd.choice((0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 15)) for _ in range(ncig))
    ref = rnd.choice((-1, 0, 1, 2, 3, 4, 1000))
    nref = rnd.choice((-1, -1, ref, 0, 3, 4, 77))
    existing = None
    with_tag = None
    if rnd.random() < 0.25:
        existing = rnd.choice((b"", b"ZZZ", b"TTT,AAA,CCC", b",,", pats[3 % len(pats)], pats[5 % len(pats)] + b"," + pats[1], b"a," + pats[0] + b",B"))
        with_tag = (tag, existing)
    name = bytes(rnd.choice(b"abcXYZ019_:/") for _ in range(254 if i % 89 == 0 else rnd.randrange(1, 30)))
    rec = bam_record(name, bytes(s), qual, rand_aux(rnd, with_tag), cigar, ref=ref, pos=rnd.choice((-1, 0, 99, INT32_MAX - 1, rnd.randrange(1 << 30))),
                     flag=rnd.choice((0, 4, 99, 65535)), mapq=rnd.choice((0, 60, 255)), nref=nref, npos=rnd.choice((-1, 0, INT32_MAX - 1, rnd.randrange(1 << 30))),
                     tlen=rnd.choice((0, -1, 1, INT32_MIN, INT32_MAX, rnd.randrange(-1000, 1000))))
    return rec, existing


def make(rnd, pats, n, **kw):
    pairs = [rand_record(rnd, pats, i, **kw) for i in range(n)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def window(mk, recs, block=0xff00):
    text = b"".join(recs)
    blob = _bgzf(text, block)
    members, used, tb = mk.bgzf_members(blob)
    assert used == len(blob) and tb == len(text)
    return text, blob, members


@pytest.mark.parametrize("filter_matching,invert", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("logging", [True, False])
def test_lines_match_the_restatement(mk, filter_matching, invert, logging):
    """every sequence length of the nibble parity and 16-lane step edges, every kind of quality, fixed and optional fields of every kind"""
    rnd = random.Random(11)
    pats = patterns31(mk, 100)
    recs, existing = make(rnd, pats, 600)
    text, blob, members = window(mk, recs)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    keep, rows, c, out = expected(om, pats, recs, REFS, b"km", logging, filter_matching, invert, existing)
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, logging=logging, filter_matching=filter_matching, invert=invert)
    assert r["n_rec"] == len(recs) and r["n_used"] == len(text) and r["tail"] == b""
    check(r, keep, rows, c, out, logging)
    assert 0 < sum(keep) and (sum(keep) < len(recs) or not (filter_matching or invert))
    codec.close()


def test_fixed_fields_one_by_one(mk):
    pats = patterns31(mk, 20)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    s = b"ACGTNACGTA"
    recs = [bam_record(b"r", s, ref=-1), bam_record(b"r", s, ref=3), bam_record(b"r", s, ref=4), bam_record(b"r", s, ref=INT32_MAX),
            bam_record(b"r", s, ref=1, nref=-1), bam_record(b"r", s, ref=1, nref=1), bam_record(b"r", s, ref=1, nref=2), bam_record(b"r", s, ref=1, nref=4),
            bam_record(b"r", s, ref=-1, nref=-1), bam_record(b"r", s, ref=7, nref=7), bam_record(b"r", s, ref=-5, nref=-5),
            bam_record(b"r", s, pos=-1, npos=-1), bam_record(b"r", s, pos=INT32_MAX - 1, npos=INT32_MAX - 1), bam_record(b"r", s, pos=INT32_MIN, npos=INT32_MIN),
            bam_record(b"r", s, tlen=-1), bam_record(b"r", s, tlen=INT32_MIN), bam_record(b"r", s, tlen=INT32_MAX),
            bam_record(b"r", s, flag=65535, mapq=255), bam_record(b"r", s, flag=0, mapq=0),
            bam_record(b"r", s, cigar=()), bam_record(b"r", s, cigar=(10 << 4 | 9, 5 << 4 | 15, 0 << 4 | 8, ((1 << 28) - 1) << 4 | 7)),
            bam_record(b"r", s, cigar=tuple((k + 1) << 4 | k % 9 for k in range(1000))),
            bam_record(b"n" * 254, s), bam_record(b"", s), bam_record(b"x", b""), bam_record(b"x", b"", cigar=(3 << 4,)),
            bam_record(b"q", s, qual=b"\xff" * 10), bam_record(b"q", s, qual=b"\x00" + b"\xff" * 9), bam_record(b"q", s, qual=bytes([222, 223, 254, 255, 93, 94, 0, 1, 128, 127]))]
    text, blob, members = window(mk, recs)
    keep, rows, c, out = expected(om, pats, recs, REFS, b"km", True, False, False)
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS)
    check(r, keep, rows, c, out)
    lines = r["out"].split(b"\n")
    assert lines[0].split(b"\t")[:4] == [b"r", b"0", b"*", b"101"] and lines[15].split(b"\t")[8] == b"-2147483648"
    assert lines[20].split(b"\t")[5] == b"10?5?0X268435455=" and lines[13].split(b"\t")[3] == b"-2147483647"
    # no reference names at all: every RNAME is "*"
    keep, rows, c, out = expected(om, pats, recs, [], b"km", True, False, False)
    check(m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=[]), keep, rows, c, out)
    codec.close()


def test_optional_fields_of_every_type(mk):
    pats = patterns31(mk, 20)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    hit = pats[0] + b"ACGT"
    aux = [b"XAA" + b"~", b"XAA" + b"!", b"Xcc" + struct.pack("<b", -128), b"Xcc" + struct.pack("<b", 127), b"XCC" + b"\xff", b"XCC" + b"\0",
           b"Xss" + struct.pack("<h", -32768), b"Xss" + struct.pack("<h", 32767), b"XSS" + struct.pack("<H", 65535), b"Xii" + struct.pack("<i", INT32_MIN),
           b"Xii" + struct.pack("<i", INT32_MAX), b"XII" + struct.pack("<I", (1 << 32) - 1), b"XII" + struct.pack("<I", 0),
           b"XZZ" + b"\0", b"XZZ" + b"some text: with\ttab" + b"\0", b"XHH" + b"00FFAB" + b"\0", b"XHH" + b"\0"]
    aux += [b"Xff" + x for x in IN_RULE]
    for sub in "cCsSiI":
        fmt = INT_TYPES[ord(sub)]
        lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (INT32_MIN, INT32_MAX), "I": (0, (1 << 32) - 1)}[sub]
        for cnt in (0, 1, 300):
            aux.append(b"XBB" + sub.encode() + struct.pack("<i", cnt) + b"".join(struct.pack(fmt, (lo, hi, 0, 7)[k % 4]) for k in range(cnt)))
    for cnt in (0, 1, 300):
        aux.append(b"XBB" + b"f" + struct.pack("<i", cnt) + b"".join(IN_RULE[k % len(IN_RULE)] for k in range(cnt)))
    aux.append(b"XBB" + b"?" + struct.pack("<i", 0))  # (an unknown subtype without items prints as it is)
    recs = [bam_record(b"o%d" % k, hit, aux=a) for k, a in enumerate(aux)]
    recs.append(bam_record(b"all", hit, aux=b"".join(aux)))
    # an existing tag that is merged, in the middle of the fields; an empty existing value; a second field of the name
    existing = [None] * len(recs)
    for v in (b"ZZZ,AAA", b"", pats[0], b"x," + pats[0] + b",A"):
        recs.append(bam_record(b"e", hit, aux=b"NMC\x02" + b"kmZ" + v + b"\0" + b"Xff" + fl(0.25) + b"kmZ" + b"second" + b"\0"))
        existing.append(v)
    text, blob, members = window(mk, recs)
    keep, rows, c, out = expected(om, pats, recs, REFS, b"km", True, True, False, existing)
    assert all(keep)
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, filter_matching=True)
    check(r, keep, rows, c, out)
    lines = r["out"].split(b"\n")
    assert lines[0].endswith(b"\tXA:A:~\tkm:Z:" + pats[0]) and lines[9].split(b"\t")[11] == b"Xi:i:-2147483648"
    assert lines[len(aux) + 1].endswith(b"\tNM:i:2\tkm:Z:ZZZ,AAA\tXf:f:0.25\tkm:Z:second\tkm:Z:" + b",".join(sorted([b"ZZZ", b"AAA", pats[0]])))
    codec.close()


def test_bndmq_counts(mk):
    rnd = random.Random(9)
    pats = mk.parse_pattern_list(kmer_seq=[b"ACGTACG", b"NNRYK", b"GATTACA", b"TTT"])
    recs, existing = make(rnd, pats, 400, hit=0.5, lens=(17, 40, 41, 90), alpha=b"ACGTNRYKMSWBDHV=")
    text, blob, members = window(mk, recs)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    assert not m.use_ac
    om = ob.Matcher(pats, False, 0, False)
    keep, rows, c, out = expected(om, pats, recs, REFS, b"km", True, True, False, existing)
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, filter_matching=True)
    check(r, keep, rows, c, out)
    assert r["counters"]["pattern_hit_counts"] == c["pattern_hit_counts"] and r["counters"]["hits"] == c["hits"]
    codec.close()


def run_windows(m, codec, blob, members, cuts, **kw):
    head, res = b"", []
    for i in range(len(cuts) - 1):
        r = m.tag_bam_sam_window(codec, head, blob, members[cuts[i]:cuts[i + 1]], last=(i == len(cuts) - 2), **kw)
        res.append(r)
        if r["status"]:
            break
        head = r["tail"]
    return res


def test_members_that_end_anywhere_tails_and_pieces(mk):
    rnd = random.Random(5)
    pats = patterns31(mk, 50)
    recs, existing = make(rnd, pats, 700)
    text, blob, members = window(mk, recs, block=7001)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    keep, rows, c, out = expected(om, pats, recs, REFS, b"XK", True, False, False, existing=None)
    n_win = 9
    cuts = [len(members) * k // n_win for k in range(n_win + 1)]
    assert len(set(cuts)) == n_win + 1
    for piece in (256, 4096, 65536):
        res = run_windows(m, codec, blob, members, cuts, refs=REFS, tag=b"XK", piece_bytes=piece)
        assert all(x["status"] == 0 and x["rc"] == 0 for x in res) and len(res) == n_win
        assert any(x["tail"] for x in res[:-1]) and res[-1]["tail"] == b""
        assert sum(x["n_rec"] for x in res) == len(recs)
        assert b"".join(x["out"] for x in res) == out
        got_rows, base = [], 0
        for x in res:
            got_rows += [(nm, rec + base, pat, pos) for (nm, rec, pat, pos) in x["rows"]]
            base += x["n_rec"]
        assert got_rows == rows
        assert sum(x["counters"]["records"] for x in res) == c["records"] and sum(x["counters"]["hits"][0] for x in res) == c["hits"][0]
        assert np.array_equal(np.sum([x["counters"]["pattern_hit_counts"] for x in res], axis=0), c["pattern_hit_counts"])
    codec.close()


def test_no_output_and_output_capacity(mk):
    rnd = random.Random(4)
    pats = patterns31(mk, 20)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    recs, existing = make(rnd, pats, 300)
    text, blob, members = window(mk, recs)
    keep, rows, c, out = expected(om, pats, recs, REFS, b"km", True, False, False, existing)
    # out == NULL: nothing is formatted, the checks still run and the window is counted
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, write=False)
    assert r["status"] == 0 and r["rc"] == 0 and r["n_kept"] == len(recs) and r["out"] == b"" and r["out_len"] == 0
    assert r["rows"] == rows and r["counters"]["records"] == len(recs)
    # an exact fit
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, out_cap=len(out), guard=64)
    check(r, keep, rows, c, out)
    assert r["guard"] == b"\xa5" * 64
    # one byte short: MK_E_CAPACITY, out_len = the need, nothing counted, the bytes behind out untouched
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, out_cap=len(out) - 1, guard=64)
    assert r["rc"] == mk.MK_E_CAPACITY and r["status"] == 0 and r["out_len"] == len(out) and r["guard"] == b"\xa5" * 64
    assert r["counters"]["records"] == 0 and r["counters"]["extracted"] == 0 and not any(r["counters"]["pattern_hit_counts"])
    # nothing kept
    none = [bam_record(b"n%d" % k, b"N" * 40) for k in range(50)]
    text, blob, members = window(mk, none)
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, filter_matching=True)
    assert r["status"] == 0 and r["rc"] == 0 and r["n_kept"] == 0 and r["out"] == b"" and r["n_rec"] == 50
    codec.close()


def test_refusals(mk):
    rnd = random.Random(2)
    pats = patterns31(mk, 20)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    good, good_ex = make(rnd, pats, 60, hit=0.0)
    hit_seq = pats[0] + b"A" * 40

    def run(recs, **kw):
        text, blob, members = window(mk, recs)
        return m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS, **kw)

    inf = float("inf")
    for bad in (fl(1e-5), fl(1e6), fl(inf), fl(-inf), struct.pack("<I", 0x7FC00000), struct.pack("<I", 1), fl(999999.5), fl(9.99994e-05)):
        for aux in (b"XFf" + bad, b"XBBf" + struct.pack("<i", 3) + fl(1.0) + bad + fl(2.0)):
            r = run(good + [bam_record(b"f", hit_seq, aux=aux)] + good)  # kept: bit 2, nothing produced or counted
            assert r["status"] == 2 and r["out"] == b"" and r["counters"]["records"] == 0
            # the same in a dropped record (-v drops the records with a hit): taken
            recs = good + [bam_record(b"f", hit_seq, aux=aux)] + good
            keep, rows, c, out = expected(om, pats, recs, REFS, b"km", True, False, True, good_ex + [None] + good_ex)
            assert sum(keep) == 2 * len(good)
            check(run(recs, invert=True), keep, rows, c, out)
    # POS / PNEXT = INT32_MAX: the host path's 32-bit + 1 is not imitated
    assert run(good + [bam_record(b"p", hit_seq, pos=INT32_MAX)])["status"] == 2
    assert run(good + [bam_record(b"p", hit_seq, npos=INT32_MAX)])["status"] == 2
    assert run(good + [bam_record(b"p", hit_seq, pos=INT32_MAX)], invert=True)["status"] == 0
    # today's bit 2: optional fields that do not parse; an unknown B subtype with items
    assert run(good + [bam_record(b"odd", b"ACGT" * 10, aux=b"XX?" + b"1234")])["status"] == 2
    assert run(good + [bam_record(b"odd", b"ACGT" * 10, aux=b"XXZ" + b"no terminator")])["status"] == 2
    assert run(good + [bam_record(b"odd", b"ACGT" * 10, aux=b"XXB?" + struct.pack("<i", 1) + b"abcd")])["status"] == 2
    # bit 4: a field of the tag's name that is not a string, not plain ASCII, very long
    assert run(good + [bam_record(b"old", hit_seq, aux=b"kmi" + struct.pack("<i", 5))])["status"] == 4
    assert run(good + [bam_record(b"old", hit_seq, aux=b"kmZ" + "AAA,é".encode() + b"\0")])["status"] == 4
    assert run(good + [bam_record(b"old", hit_seq, aux=b"kmZ" + b"ACGT," * 500 + b"\0")])["status"] == 4
    assert run(good + [bam_record(b"old", hit_seq, aux=b"kmi" + struct.pack("<i", 5))], invert=True)["status"] == 0
    # bit 1: sizes that do not add up
    bad = bytearray(good[3])
    struct.pack_into("<i", bad, 0, 20)
    assert run(good[:3] + [bytes(bad)] + good[4:])["status"] == 1
    # bit 8: the file ends inside a record (last); not last: the unfinished record is the tail
    text = b"".join(good)
    blob = _bgzf(text[:-7])
    members, _, _ = mk.bgzf_members(blob)
    assert m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=REFS)["status"] == 8
    r = m.tag_bam_sam_window(codec, b"", blob, members, last=False, refs=REFS)
    assert r["status"] == 0 and r["n_rec"] == len(good) - 1 and r["tail"] == good[-1][:-7]
    # a damaged member
    blob = bytearray(_bgzf(text))
    blob[len(blob) // 2] ^= 0x55
    members, _, _ = mk.bgzf_members(bytes(blob))
    with pytest.raises(mk.MerkurioError) as e:
        m.tag_bam_sam_window(codec, b"", bytes(blob), members, last=True, refs=REFS)
    assert e.value.code == mk.MK_E_CORRUPT
    codec.close()


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_against_the_restatement(mk, seed):
    rnd = random.Random(1000 + seed)
    pats = patterns31(mk, rnd.choice((15, 60)), seed=seed)
    tag = rnd.choice((b"km", b"XK"))
    recs, existing = make(rnd, pats, rnd.randrange(1, 500), tag=tag, hit=rnd.choice((0.1, 0.6)))
    text, blob, members = window(mk, recs, block=rnd.choice((3001, 20000, 0xff00)))
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    fm, inv, logging = rnd.choice(((False, False), (True, False), (False, True))) + (rnd.random() < 0.7,)
    refs = rnd.choice((REFS, REFS[:2], []))
    keep, rows, c, out = expected(om, pats, recs, refs, tag, logging, fm, inv, existing)
    n_win = min(len(members), rnd.choice((1, 2, 5)))
    cuts = sorted(set([0, len(members)] + [rnd.randrange(len(members) + 1) for _ in range(n_win - 1)]))
    res = run_windows(m, codec, blob, members, cuts, refs=refs, tag=tag, logging=logging, filter_matching=fm, invert=inv, piece_bytes=rnd.choice((0, 256, 4096)))
    assert all(x["status"] == 0 and x["rc"] == 0 for x in res) and len(res) == len(cuts) - 1
    assert sum(x["n_rec"] for x in res) == len(recs) and sum(x["n_kept"] for x in res) == sum(keep)
    got = b"".join(x["out"] for x in res)
    if got != out:
        a, b = got.split(b"\n"), out.split(b"\n")
        bad = [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:2]
        raise AssertionError(f"{len(a)} / {len(b)} lines; {[(a[k], b[k]) for k in bad]}")
    if logging:
        got_rows, base = [], 0
        for x in res:
            got_rows += [(nm, rec + base, pat, pos) for (nm, rec, pat, pos) in x["rows"]]
            base += x["n_rec"]
        assert got_rows == rows
        assert np.array_equal(np.sum([x["counters"]["pattern_hit_counts"] for x in res], axis=0), c["pattern_hit_counts"])
    codec.close()


def test_reference_bam_fixture(mk):
    """tests/fixtures/input/simple.bam of the reference through the window path: names, sequences and km values of
    tests/fixtures/tag/simple.tagged.extracted.sam (the comparison test_gpu_bam_window.py makes), and the whole record lines, which the
    host path gives byte for byte as well (test_cli_gpu.py: test_tag_fixtures compares that file whole)"""
    blob = open(os.path.join(GOLDEN, "fixtures", "input", "simple.bam"), "rb").read()
    members, used, _ = mk.bgzf_members(blob)
    text = gzip.decompress(blob)
    l_text = struct.unpack_from("<i", text, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", text, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", text, p)[0]
        refs.append(text[p + 4:p + 4 + ln - 1])
        p += 4 + ln + 4
    import textio
    _, sam = textio.read_sam(os.path.join(GOLDEN, "fixtures", "tag", "simple.tagged.extracted.sam"))
    pats = mk.parse_pattern_list(kmer_seq=[b"CTC"], reverse_complement=True)  # tag ... -s CTC -r
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    # head = the record bytes (as the CLI hands over what its header parser has already inflated), no members at all
    r = m.tag_bam_sam_window(codec, text[p:], b"", members[:0], last=True, refs=refs, logging=True)
    assert r["status"] == 0 and r["rc"] == 0
    got = [ln.split(b"\t") for ln in r["out"].split(b"\n") if ln]
    assert len(got) == len(sam) == r["n_rec"]
    for fields, want in zip(got, sam):
        assert fields[0] == want[0] and fields[9] == want[9]
        assert [f for f in fields[11:] if f.startswith(b"km:Z:")][-1] == [f for f in want[11:] if f.startswith(b"km:Z:")][-1]
        assert fields == list(want)
    codec.close()
