"""Crafted SAM lines and BAM records for the kernels behind `tag` (merkurio_amd/csrc/sam.hip, bam.hip): every byte that matters is
put at an edge of the kernels' own geometry -- a lane's 16 bytes and a step's 256 in the line kernels (8 / 128 in the gathers, 4 / 64
in the BAM emit), the 64 lanes of a wave, a piece of the BAM record chain.  Pure Python: no device, no library.  Every builder returns
what it built together with a small description of what it placed where; tests/test_tag_edge_cases_cpu.py proves those descriptions
from the bytes, tests/test_gpu_tag_edges.py runs the families through the four window entry points.

A SAM family is a list of (line without line end, line end, description); a BAM family a list of (record, description)."""
import itertools
import struct

from tag_windows import NIB, bam_record

LANE, STEP = 16, 256
STEP_EDGES = (255, 256, 257, 511, 512, 513)
CONFOUNDERS = (0x40, 0x5B, 0x60, 0x7B, 0xE1, 0xFA, 0xFF)  # the bytes next to 'A' 'Z' 'a' 'z', and 'a' 'z' DEL with the top bit set
RECORD_COUNTS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)
NON_RECORDS = ((b"@CO\tnot a record", b"\n"), (b"", b"\n"), (b"", b"\r\n"))
MERGE_MAX = 2048  # tag_merge.hpp: kBamMergeBytes


def kmers4():
    return [bytes(p) for p in itertools.product(b"ACGT", repeat=4)]


def bases(n, salt=0):
    """n bases in which every 4-mer window is told from its neighbours (no period below n for the lengths used here)"""
    return bytes(b"ACGT"[((k * k + 3 * k) // 2 + salt * (k + 1) + (k >> 3)) & 3] for k in range(n))


# ---- SAM lines -----------------------------------------------------------------------------------------------------------------
def sam_line(qname, seq, qual=None, aux=(), rname=b"chr1", cigar=None):
    """a line that is valid SAM: FLAG 0, POS 100, MAPQ 60, CIGAR <len>M, RNEXT *, PNEXT 0, TLEN 0; seq = the field as written"""
    L = 0 if seq == b"*" else len(seq)
    if qual is None:
        qual = b"I" * L if L else b"*"
    if cigar is None:
        cigar = b"%dM" % L if L else b"*"
    return b"\t".join([qname, b"0", rname, b"100", b"60", cigar, b"*", b"0", b"0", seq, qual] + list(aux))


def tab_offset(line, which):
    """offset of the which-th tab (1-based) from the line's first byte; None: the line has fewer"""
    p = -1
    for _ in range(which):
        p = line.find(b"\t", p + 1)
        if p < 0:
            return None
    return p


def line_with_tab_at(which, offset, qname=b"q", seq=b"ACGTTGCA", aux=(b"NM:i:1",)):
    """tab `which` (1, 9, 10 or 11) at `offset`: QNAME padded for tab 1, RNAME for the others"""
    if which == 1:
        return sam_line(b"q" * offset, seq, aux=aux)
    base = sam_line(qname, seq, aux=aux, rname=b"c")
    pad = offset - tab_offset(base, which)
    assert pad >= 0, (which, offset)
    return sam_line(qname, seq, aux=aux, rname=b"c" * (1 + pad))


def _both_ends(items):
    return [(ln, eol, dict(d, eol=eol)) for ln, d in items for eol in (b"\n", b"\r\n")]


def sam_tab_family():
    """tabs 1, 9, 10, 11 at every offset of a lane and at the step edges (tab 1: up to QNAME's 254 bytes), each with LF and CRLF"""
    items = []
    for off in list(range(1, 17)) + [31, 32, 254]:
        items.append((line_with_tab_at(1, off), dict(tab=1, off=off)))
    for which in (9, 10, 11):
        for off in list(range(48, 64)) + list(STEP_EDGES):
            items.append((line_with_tab_at(which, off), dict(tab=which, off=off)))
    return _both_ends(items)


def sam_long_qname_family():
    """QNAME longer than the specification's 254 bytes (the device has no such limit): the only way tab 1 leaves the first step"""
    items = [(line_with_tab_at(1, off), dict(tab=1, off=off)) for off in (255, 256, 257, 300, 511, 512, 513)]
    return _both_ends(items)


def sam_lane_family():
    """several wanted tabs in one lane; lines of exactly 11 and 12 fields; an empty CIGAR field"""
    items = []
    for pad in range(0, 18):  # tabs 9, 10, 11 within four bytes, at every position of a lane
        items.append((sam_line(b"s%d" % pad, b"*", rname=b"c" * (1 + pad), aux=(b"NM:i:1",)), dict(kind="star", fields=12)))
        items.append((sam_line(b"o%d" % pad, b"A", b"*", rname=b"c" * (1 + pad), aux=(b"NM:i:1",)), dict(kind="one-star-qual", fields=12)))
        items.append((sam_line(b"a%d" % pad, b"A", b"!", rname=b"c" * (1 + pad), aux=(b"NM:i:1",)), dict(kind="one", fields=12)))
        items.append((sam_line(b"e%d" % pad, b"*", rname=b"c" * (1 + pad)), dict(kind="star", fields=11)))
        items.append((sam_line(b"b%d" % pad, b"a", b"~", rname=b"c" * (1 + pad)), dict(kind="one", fields=11)))
    items.append((sam_line(b"emptycigar", b"ACGTACGTAC", cigar=b""), dict(kind="empty-cigar", fields=11)))
    items.append((sam_line(b"emptycigar2", b"*", cigar=b"", aux=(b"NM:i:1", b"AS:i:2")), dict(kind="empty-cigar", fields=13)))
    return _both_ends(items)


def sam_odd_family():
    """SAM -> SAM only (the host refuses these as BAM): 10 fields, runs of one-byte and of empty fields (more than 11 tabs in a
    lane), a line that ends on a tab, '\\r' directly behind a tab.  -> items, and the refusal bits SAM -> BAM answers with"""
    items = []
    ten = b"\t".join(sam_line(b"ten", b"ACGTACGTACGT").split(b"\t")[:10])
    items.append((ten, dict(kind="ten", fields=10)))
    items.append((b"\t".join(sam_line(b"ten2", b"*").split(b"\t")[:10]), dict(kind="ten", fields=10)))
    for pad in (0, 5, 11):  # a run of one-byte fields: eight tabs within a lane, wherever the lane starts
        ln = sam_line(b"m%d" % pad, b"ACGTAC", rname=b"c" * (1 + pad)) + b"\tx" * 20
        items.append((ln, dict(kind="many", fields=31)))
    # more than 11 tabs in a lane takes empty fields: fields 2 ... 9 empty puts tabs 1, 9, 10 and 11 into the line's first lane
    # (13 tabs in it); a run of empty optional fields fills later lanes with tabs, in front of nothing and of a field of the tag
    for seq, qual in ((b"A", b"!"), (b"*", b"*")):
        items.append((b"q" + b"\t" * 9 + seq + b"\t" + qual + b"\t" * 4 + b"NM:i:1", dict(kind="crowded", fields=15, wanted_in_lane0=True)))
    items.append((b"q" + b"\t" * 9 + bases(9, 2) + b"\t" + b"I" * 9 + b"\t" * 18 + b"x", dict(kind="crowded", fields=29, wanted_in_lane0=False)))
    for pad in (0, 7):
        ln = sam_line(b"w%d" % pad, bases(8, pad), rname=b"c" * (1 + pad)) + b"\t" * 20 + b"km:Z:TTTT,zz"
        items.append((ln, dict(kind="crowded", fields=31, wanted_in_lane0=False)))
    items.append((sam_line(b"endtab", b"ACGTACGT") + b"\t", dict(kind="end-tab", fields=12)))
    items.append((sam_line(b"endtab2", b"ACGTACGT", aux=(b"NM:i:1",)) + b"\t", dict(kind="end-tab", fields=13)))
    items.append((b"\t".join(sam_line(b"endtab3", b"ACGTACGT").split(b"\t")[:10]) + b"\t", dict(kind="end-tab", fields=11)))
    return _both_ends(items), 1 | 2


def sam_length_family(lo=230, hi=540):
    """every line length in [lo, hi], reached by an XL:Z: filler; and one long read of 10 000 bases"""
    items = []
    base = len(sam_line(b"len", bases(20), aux=(b"XL:Z:",)))
    for n in range(lo, hi + 1):
        ln = sam_line(b"len", bases(20, n), aux=(b"XL:Z:" + b"f" * (n - base),))
        items.append((ln, b"\n", dict(length=len(ln))))
    seq = bases(10000, 7)
    items.append((sam_line(b"longread", seq, bytes(33 + k % 90 for k in range(10000)), aux=(b"NM:i:3",)), b"\n", dict(length=None, long=10000)))
    return items


def seq_start(line):
    return tab_offset(line, 9) + 1


def sam_seq_family(aligns, lens=range(0, 301)):
    """every SEQ length at every start alignment (SEQ's offset in the line mod 16), shifted by QNAME's length"""
    items = []
    for a in aligns:
        for L in lens:
            seq = bases(L, L + a) if L else b"*"
            qual = bytes(33 + (k + L) % 94 for k in range(L)) if L and L % 7 else None
            qn = (a - seq_start(sam_line(b"", seq, qual))) % 16 or 16  # (the CIGAR in front of SEQ grows with the length)
            ln = sam_line(b"q" * qn, seq, qual)
            items.append((ln, b"\n", dict(seq_len=L, align=seq_start(ln) % 16)))
    return items


def sam_case_family():
    """lower case at every position of an eight-byte group, alone and as a whole group; the confounder bytes next to a / z, in the
    eight-byte groups and in the byte-wise tail"""
    items = []
    core = bases(40, 5)
    for start in (0, 3):  # (two alignments of SEQ: the groups of eight start at SEQ's first byte, wherever that lies)
        for k in range(8, 24):
            s = bytearray(core)
            s[k] |= 0x20
            items.append((sam_line(b"l" * (1 + start), bytes(s)), dict(kind="lower", at=k)))
        items.append((sam_line(b"L" * (1 + start), core.lower()), dict(kind="lower-all")))
        for c in CONFOUNDERS:
            for k in range(8, 16):  # inside a group of eight: [.. a c z ..]
                s = bytearray(core)
                s[k - 1:k + 2] = bytes([ord("a"), c, ord("z")])
                items.append((sam_line(b"c" * (1 + start), bytes(s)), dict(kind="confounder", byte=c, at=k)))
            s = bytearray(core[:13])  # the tail: 13 = one group of eight and five single bytes
            s[10:13] = bytes([ord("a"), c, ord("z")])
            items.append((sam_line(b"t" * (1 + start), bytes(s)), dict(kind="confounder", byte=c, at=11)))
    return [(ln, b"\n", d) for ln, d in items]


def aux_start(line):
    return tab_offset(line, 11) + 1


def sam_existing_family(tag=b"km"):
    """a line that already carries the tag: the tab in front of the field at every offset of a lane of the optional-field area and
    at its step edge, the field as field 12 and as the last field, two fields of the name in different lanes and steps, a value of
    exactly MERGE_MAX bytes"""
    items = []
    mine = tag + b":Z:TTTT,ACGT,zz"
    seq = bases(12, 3)
    for off in list(range(16, 32)) + [255, 256, 257]:
        ln = sam_line(b"x%d" % off, seq, aux=(b"XL:Z:" + b"f" * (off - 5), mine, b"NM:i:1"))
        items.append((ln, dict(kind="at", off=off, value=b"TTTT,ACGT,zz")))
    items.append((sam_line(b"f12", seq, aux=(mine, b"NM:i:1")), dict(kind="field12", value=b"TTTT,ACGT,zz")))
    items.append((sam_line(b"only", seq, aux=(mine,)), dict(kind="field12", value=b"TTTT,ACGT,zz")))
    for v in (b"", b"A"):  # as the last field: 5 bytes (an empty value: nothing to merge) and 6
        items.append((sam_line(b"last%d" % len(v), seq, aux=(b"NM:i:1", tag + b":Z:" + v)), dict(kind="last", value=v)))
    for gap in (40, 300):  # the first of two wins: in another lane, in another step
        ln = sam_line(b"two%d" % gap, seq, aux=(tag + b":Z:first", b"XL:Z:" + b"f" * gap, tag + b":i:5", b"NM:i:1"))
        items.append((ln, dict(kind="two", gap=gap, value=b"first")))
        ln = sam_line(b"twoz%d" % gap, seq, aux=(b"NM:i:1", tag + b":Z:first", b"XL:Z:" + b"f" * gap, tag + b":Z:second"))
        items.append((ln, dict(kind="two", gap=gap, value=b"first")))
    big = (b"ACGT," * 410)[:MERGE_MAX]
    items.append((sam_line(b"big", seq, aux=(b"NM:i:1", tag + b":Z:" + big)), dict(kind="big", value=big)))
    return _both_ends(items)


def sam_short_tag_family(tag=b"km"):
    """SAM -> SAM only: `km:Z` as the last field is four bytes -- not a field of that name (and not one the BAM encoder takes)"""
    seq = bases(12, 3)
    items = [(sam_line(b"four", seq, aux=(b"NM:i:1", tag + b":Z")), dict(kind="last", value=None)),
             (sam_line(b"four2", seq, aux=(tag + b":Z",)), dict(kind="last", value=None)),
             (sam_line(b"four3", seq, aux=(tag + b":", tag + b":Z:real")), dict(kind="last", value=b"real"))]
    return _both_ends(items), 2


def sam_refusal_texts(tag=b"km"):
    """the three documented refusals: name -> (text, status)"""
    seq = bases(12, 3)
    good = [sam_line(b"g%d" % i, bases(12, i)) for i in range(67)]
    out = {}
    over = sam_line(b"over", seq, aux=(b"NM:i:1", tag + b":Z:" + (b"ACGT," * 410)[:MERGE_MAX + 1]))
    out["value-2049"] = (b"\n".join(good[:5] + [over] + good[5:9]) + b"\n", 4)
    for gap in (40, 300):
        ifirst = sam_line(b"ifirst", seq, aux=(tag + b":i:5", b"XL:Z:" + b"f" * gap, tag + b":Z:second"))
        out["i-first-%d" % gap] = (b"\n".join(good[:3] + [ifirst] + good[3:6]) + b"\n", 4)
    nine = b"\t".join(sam_line(b"nine", seq).split(b"\t")[:9])
    out["nine-fields-last"] = (b"\n".join(good + [nine]) + b"\n", 1)  # 68 lines: the last line of the last wave (4 lines a wave)
    return out


def count_record(i):
    """record i of the count and compaction texts: every third one has three bases (no 4-mer: not kept under filter_matching)"""
    return sam_line(b"r%d" % i, bases(3 if i % 3 == 1 else 9 + i % 5, i))


def sam_count_texts():
    """name -> (items, n_rec): n records plain, and with non-record lines first, last and in runs of 1, 4, 16 between records; one
    record among 40 non-record lines"""
    out = {}

    def non(k):
        return [(ln, eol, dict(rec=False)) for ln, eol in (NON_RECORDS[j % 3] for j in range(k))]

    for n in RECORD_COUNTS:
        recs = [(count_record(i), b"\n", dict(rec=True)) for i in range(n)]
        out["n%d-plain" % n] = (recs, n)
        out["n%d-first" % n] = (non(2) + recs, n)
        out["n%d-last" % n] = (recs + non(3), n)
        for run in (1, 4, 16):
            at = sorted({n // 2, n - 1} | ({1} if n > 1 else set()))
            items = []
            for i, r in enumerate(recs):
                if i in at:
                    items += non(run)
                items.append(r)
            out["n%d-run%d" % (n, run)] = (items, n)
    out["one-among-40"] = (non(23) + [(count_record(0), b"\n", dict(rec=True))] + non(17), 1)
    return out


def last_wave_lane0(n, per_wave=4):
    """index of the record that lane 0 of the last wave holds (16 lanes a record: four records a wave)"""
    return (n - 1) // per_wave * per_wave


def stats_variants(n):
    """(label, index of the odd record or None, its SEQ length or None for '*'): all equal; one shorter / longer / '*' record at
    index 0, n - 1 and as lane 0 of the last wave"""
    out = [("equal", None, 12)]
    for where in sorted({0, n - 1, last_wave_lane0(n)}):
        for L in (5, 40, None):
            out.append(("odd", where, L))
    return out


def sam_stats_texts(base_len=12):
    out = {}
    for n in (4, 64, 257):
        for label, where, L in stats_variants(n):
            items = []
            for i in range(n):
                ln_ = base_len if i != where else L
                items.append((sam_line(b"s%d" % i, bases(ln_, i) if ln_ else b"*"), b"\n", dict(seq_len=ln_ or 0)))
            out["n%d-%s-%s-%s" % (n, label, where, L)] = (items, n, where)
    return out


def text_of(items):
    return b"".join(ln + eol for ln, eol, _ in items)


# ---- what the 4-mer rows say -------------------------------------------------------------------------------------------------------
def upper(seq):
    return bytes(c - 32 if 97 <= c <= 122 else c for c in seq)


def spelled(seq_upper):
    """the bytes of a sequence that some window of four plain bases covers, '.' elsewhere"""
    ok = [all(c in b"ACGT" for c in seq_upper[p:p + 4]) for p in range(max(0, len(seq_upper) - 3))]
    out = bytearray(b"." * len(seq_upper))
    for p, hit in enumerate(ok):
        if hit:
            out[p:p + 4] = seq_upper[p:p + 4]
    return bytes(out)


def spell_back(rows, patterns, lengths):
    """rows [(name, rec, pat, pos)] of a matcher over all 4-mers -> per record the text the rows spell ('.' where none says anything);
    AssertionError where two rows disagree about a byte"""
    out = [bytearray(b"." * n) for n in lengths]
    for _, rec, pat, pos in rows:
        s, p = out[rec], patterns[pat]
        assert pos + 4 <= len(s), (rec, pos, len(s))
        for k in range(4):
            assert s[pos + k] in (46, p[k]), (rec, pos)
        s[pos:pos + 4] = p
    return [bytes(s) for s in out]


# ---- BAM records ------------------------------------------------------------------------------------------------------------------
def bam_seq(L, salt=0):
    """mostly plain bases, every 11th letter walks the 16-letter alphabet"""
    b = bytearray(bases(L, salt))
    for k in range(5, L, 11):
        b[k] = NIB[(k + salt) % 16]
    return bytes(b)


def bam_qual(L, kind):
    if kind == 0 or L == 0:
        return bytes((k * 7 + L) % 94 for k in range(L))
    if kind == 1:
        return b"\xff" * L
    if kind == 2:  # 0xFF behind the first byte
        return bytes([40]) + b"\xff" * (L - 1)
    return bytes([223]) + bytes((222, 223, 254, 93, 94, 200, 250)[(k + L) % 7] for k in range(1, L))  # + 33 wraps


def bam_seq_offset(rec):
    """offset of the packed sequence from the record's block_size field"""
    return 36 + rec[12] + 4 * struct.unpack_from("<H", rec, 16)[0]


def bam_lseq_family(lens=range(0, 531)):
    """every l_seq, the four kinds of quality, names of 1 ... 16 bytes and 0 ... 3 CIGAR ops (where the packed sequence starts)"""
    out = []
    for L in lens:
        name_len, ops, kind = 1 + (L * 5) % 16, (L // 16 + L) % 4, (L // 4 + L) % 4
        rec = bam_record(b"n" * name_len, bam_seq(L, L), bam_qual(L, kind), aux=b"NMC\x01" if L % 3 else b"", cigar=tuple((k + 1) << 4 | k for k in range(ops)))
        out.append((rec, dict(l_seq=L, kind=kind if L else 0, name_len=name_len, ops=ops, seq_at=bam_seq_offset(rec) % 4)))
    return out


def bam_length_family(n=140):
    """4 + block_size at n consecutive values, reached by an XL:Z: filler"""
    out = []
    for k in range(n):
        rec = bam_record(b"len", bam_seq(21, k), aux=b"XLZ" + b"f" * k + b"\0")
        out.append((rec, dict(length=len(rec))))
    return out


def _std(i):
    return bam_record(b"p%03d" % (i % 1000), bases(10, i))


def _sized(i, size):
    """a record of exactly `size` bytes (4 + block_size)"""
    n = size - len(_std(i)) - 4
    assert n >= 0, size
    return bam_record(b"p%03d" % (i % 1000), bases(10, i), aux=b"XLZ" + b"f" * n + b"\0")


def bam_piece_records(piece, n_pieces, span3_at=None):
    """records whose chain meets the first bytes of the pieces: a record starts one byte before, exactly on and one byte behind the
    first byte of pieces 1, 2, 3, ... in turn; with span3_at, one record there is longer than three pieces.
    -> (records, [(piece, delta, index of the record that starts at piece * piece_bytes + delta)], total length)"""
    recs, placed, pos = [], [], 0
    s0 = len(_std(0))
    j = 1
    while j < n_pieces:
        if span3_at is not None and j == span3_at:
            recs.append(_sized(len(recs), 4 * piece + 2 * s0))  # (from inside one piece, over three whole ones, into a fifth)
            pos += len(recs[-1])
            j = pos // piece + 2
            continue
        delta = (-1, 0, 1)[j % 3]
        target = j * piece + delta
        while target - pos >= 2 * s0 + 4:
            recs.append(_std(len(recs)))
            pos += s0
        recs.append(_sized(len(recs), target - pos))
        pos = target
        placed.append((j, delta, len(recs)))
        j += 1
    recs.append(_std(len(recs)))  # (the record the last target names)
    pos += s0
    return recs, placed, pos


def bam_piece_count_records(piece, count):
    """a text of exactly `count` pieces: the last piece holds 1 ... piece bytes"""
    recs, placed, pos = bam_piece_records(piece, count - 1)
    while (pos + piece - 1) // piece < count:
        recs.append(_std(len(recs)))
        pos += len(recs[-1])
    assert (pos + piece - 1) // piece == count
    return recs, pos


WINDOW_CUTS = (1, 2, 3, 4, 35, 36, 37)


def bam_cut_cases(recs, placed):
    """[(bytes of text in the first window, index of the record it ends in, bytes of that record it holds)] for WINDOW_CUTS, each in a
    record that starts one byte before a piece's first byte: from two bytes on, the unfinished record starts in the piece before the
    one the text ends in"""
    starts = [0]
    for r in recs:
        starts.append(starts[-1] + len(r))
    before = [k for _, delta, k in placed if delta == -1]
    assert len(before) >= len(WINDOW_CUTS)
    out = []
    for k, d in zip(before, WINDOW_CUTS):
        assert d < len(recs[k])
        out.append((starts[k] + d, k, d))
    return out


def bam_long_tail_case(piece, n_span=12):
    """a window that ends deep inside a long record: -> (records, index of the long record, bytes of text in the first window); the
    unfinished record starts n_span pieces in front of the piece the text ends in -- more than the rounds in which the record index
    could repair piece starts one by one, so only the walk's "the text ends inside this record" stops the search"""
    recs = [_std(i) for i in range(7)]
    start = sum(len(r) for r in recs)
    recs.append(_sized(7, (n_span + 2) * piece))
    recs += [_std(i) for i in range(8, 12)]
    return recs, 7, start + n_span * piece + piece // 2


AUX_KINDS = (b"XAAq", b"Xcc\xfe", b"XCC\x07", b"Xss" + struct.pack("<h", -300), b"XSS" + struct.pack("<H", 65535), b"Xii" + struct.pack("<i", -70000),
             b"XII" + struct.pack("<I", 1 << 31), b"Xff" + struct.pack("<f", 1.5), b"XZZtext\0", b"XHH0AFF\0", b"XBBc" + struct.pack("<i", 0),
             b"XBBs" + struct.pack("<i", 300) + struct.pack("<h", -2) * 300, b"XBBf" + struct.pack("<i", 0), b"XBBI" + struct.pack("<i", 300) + struct.pack("<I", 7) * 300)


def bam_existing_family(tag=b"km"):
    """-> [(record, dict(existing=value, where=...))]: the tag's Z field first, in the middle and last among fields of every type
    (B arrays of 0 and 300 items in front of it), and a value of exactly MERGE_MAX bytes"""
    out = []
    seq = bases(12, 3)
    value = b"TTTT,ACGT,zz"
    mine = tag + b"Z" + value + b"\0"
    for k, other in enumerate(AUX_KINDS):
        out.append((bam_record(b"f%d" % k, seq, aux=mine + other), dict(existing=value, where="first")))
        out.append((bam_record(b"m%d" % k, seq, aux=other + mine + AUX_KINDS[(k + 1) % len(AUX_KINDS)]), dict(existing=value, where="middle")))
        out.append((bam_record(b"l%d" % k, seq, aux=other + mine), dict(existing=value, where="last")))
    out.append((bam_record(b"all", seq, aux=b"".join(AUX_KINDS) + mine), dict(existing=value, where="last")))
    out.append((bam_record(b"two", seq, aux=mine + AUX_KINDS[11] + tag + b"Zsecond\0"), dict(existing=value, where="first")))
    out.append((bam_record(b"none", seq, aux=b"".join(AUX_KINDS)), dict(existing=None, where=None)))
    big = (b"ACGT," * 410)[:MERGE_MAX]
    out.append((bam_record(b"big", seq, aux=AUX_KINDS[13] + tag + b"Z" + big + b"\0"), dict(existing=big, where="last")))
    return out


def bam_over_record(tag=b"km"):
    return bam_record(b"over", bases(12, 3), aux=AUX_KINDS[11] + tag + b"Z" + (b"ACGT," * 410)[:MERGE_MAX + 1] + b"\0")


def bam_stats_records(base_len=12):
    """name -> (records, index of the odd one): the variants of sam_stats_texts as BAM records ('*' = l_seq 0)"""
    out = {}
    for n in (4, 64, 257):
        for label, where, L in stats_variants(n):
            recs = [bam_record(b"s%d" % i, bases((base_len if i != where else (L or 0)), i)) for i in range(n)]
            out["n%d-%s-%s-%s" % (n, label, where, L)] = (recs, where)
    return out
