"""mk_extract_window_members: a window's kept records leave the device as BGZF members of their WRITTEN form (include/merkurio_hip.h).
The expected text is a Python restatement of the rule, `written_fastq` / `written_fasta` below (the CLI test pins it against the host
writer); the members are read with mk.bgzf_members and zlib, their ISIZE sequence is mk.bgzf_record_cuts of the written record ends.
keep, rows and counters are mk_extract_window's."""
import ctypes as C
import random
import struct
import zlib

import numpy as np
import pytest

from guarded import HostBuf

pytestmark = pytest.mark.gpu

P = b"ACGTTGCAAGGCTTAACGGAT"  # what a kept record holds (the other sequences are random: 4^-21 per place)


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def codec(mk):
    c = mk.Codec()
    yield c
    c.close()


@pytest.fixture(scope="module")
def matcher(mk):
    return mk.Matcher(mk.parse_pattern_list(kmer_seq=[P], reverse_complement=True))


def _rand(rnd, n, alpha=b"ACGT"):
    return bytes(rnd.choices(alpha, k=n))


def _seq(rnd, n, hit):
    s = bytearray(_rand(rnd, n))
    if hit:
        k = rnd.randrange(0, n - len(P) + 1)
        s[k:k + len(P)] = P
    return bytes(s)


# ---- the rule, restated -----------------------------------------------------------------------------------------------------------
def _strip(line):
    return line[:-1] if line.endswith(b"\r") else line


def fastq_records(text):
    """the stored records of a FASTQ text: lists of four lines without '\\n' (a '\\r' in front of it is still there)"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [lines[k:k + 4] for k in range(0, len(lines), 4)]


def written_fastq(rec):
    eol = b"\r\n" if len(rec[0]) > 1 and rec[0].endswith(b"\r") else b"\n"
    return _strip(rec[0]) + eol + _strip(rec[1]) + eol + b"+" + eol + _strip(rec[3]) + eol


def fasta_records(text):
    starts = [0] + [k + 1 for k in range(len(text) - 1) if text[k] == 10 and text[k + 1] == 62]
    return [text[a:b] for a, b in zip(starts, starts[1:] + [len(text)])]


def written_fasta(rec):
    """None: a record the device may refuse (its written form is not its bytes with the final line end fixed)"""
    h = rec.find(b"\n")
    if h < 0:
        return None
    eol = b"\r\n" if h > 1 and rec[h - 1:h] == b"\r" else b"\n"
    body = rec[:-2] if rec.endswith(b"\r\n") else rec[:-1] if rec.endswith(b"\n") else rec
    if len(body) <= h + 1 or body[-1:] in (b"\n", b"\r"):
        return None
    return body + eol


def check_members(mk, S, written, n_members=None):
    """S: a source of extract_window_members; written: the written forms of its kept records, in order"""
    text = b"".join(written)
    assert not S["as_text"] and S["n_written"] == len(text) and S["n_kept"] == len(written)
    blob = S["members"]
    if not text:
        assert blob == b"" and S["n_members"] == 0
        return
    mem, used, total = mk.bgzf_members(blob)
    assert used == len(blob) and total == len(text) and S["n_members"] == len(mem)
    cuts = mk.bgzf_record_cuts(np.cumsum([len(w) for w in written]))
    assert mem["isize"].tolist() == np.diff(cuts).tolist()
    if n_members is not None:
        assert len(mem) == n_members
    got = []
    for m in mem:
        start = int(m["data_off"]) - 18
        assert blob[start:start + 16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
        d = zlib.decompressobj(-15)
        t = d.decompress(blob[int(m["data_off"]):int(m["data_off"]) + int(m["data_len"])])
        assert d.eof and zlib.crc32(t) == int(m["crc"]) and len(t) == int(m["isize"])
        got.append(t)
    got = b"".join(got)
    assert len(got) == len(text)
    if got != text:
        k = next(i for i in range(len(text)) if got[i] != text[i])
        raise AssertionError("written text differs at byte %d: %r, expected %r" % (k, got[max(0, k - 40):k + 20], text[max(0, k - 40):k + 20]))
    assert blob[-28:] != mk.bgzf_eof()  # no EOF member


def same_answers(r, old):
    assert r["status"] == old["status"] == 0 and r["n_rec"] == old["n_rec"]
    assert r["keep"] == old["keep"] and r["rows"] == old["rows"] and r["counters"] == old["counters"]
    for a, b in zip(r["sources"], old["sources"]):
        assert all(a[k] == b[k] for k in ("n_window", "n_used", "n_rec_seen", "rec_start", "tail"))


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------------
def mixed_fastq(n, seed=3):
    """bare '+', '+id', CRLF, LF header with CRLF body lines, CRLF header with LF body lines; every third record holds P (kept_of),
    the last one among them, which has no line end"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        L = rnd.choice([21, 22, 36, 63, 64, 65, 100, 151, 250])
        rid = b"r%d/%d x" % (i, L) if i % 7 else b""  # (an empty id now and then: "@\r\n" is a header the index takes, "@\n" is not)
        s, q = _seq(rnd, L, (n - 1 - i) % 3 == 0), _rand(rnd, L, b"@+IJ#5ACGT>")
        shape = i % 5
        if not rid and shape not in (2, 4):
            rid = b"e"
        plus = b"+" + rid if shape == 1 else b"+"
        h_eol = b"\r\n" if shape in (2, 4) else b"\n"
        b_eol = b"\r\n" if shape in (2, 3) else b"\n"
        out.append(b"@" + rid + h_eol + s + b_eol + plus + b_eol + q + b_eol)
    text = b"".join(out)
    return text[:-1]


def kept_of(n):
    return [(n - 1 - i) % 3 == 0 for i in range(n)]


def test_fastq_mixed_shapes(mk, codec, matcher):
    """9 000 records: more than a 256-lane block, the 4 096 scan tile and several 49 152-byte grid points"""
    text = mixed_fastq(9000)
    recs = fastq_records(text)
    assert len(recs) == 9000
    r = matcher.extract_window_members([{"text": text}], codec)
    same_answers(r, matcher.extract_window([{"text": text}], logging=False))
    assert r["keep"] == kept_of(9000)
    w = [written_fastq(rec) for rec, k in zip(recs, kept_of(9000)) if k]
    assert w[-1] == written_fastq(recs[-1]) and not text.endswith(b"\n") and any(x.endswith(b"\r\n") for x in w) and sum(map(len, w)) > 5 * 49152
    check_members(mk, r["sources"][0], w)


@pytest.fixture(scope="module")
def fastq_331():
    rnd = random.Random(5)
    recs = [b"@r%06d\n" % i + _seq(rnd, 159, i == 4097) + b"\n+\n" + _rand(rnd, 159, b"IJ#5F:,") + b"\n" for i in range(6000)]
    assert all(len(x) == 331 for x in recs)
    return recs


@pytest.mark.parametrize("kept", ["all", "one", "none"])
def test_fastq_of_one_length(mk, codec, matcher, fastq_331, kept):
    text = b"".join(fastq_331)
    # ("all": -v keeps the 5 999 records without P; test_fastq_where_every_record_is_kept has all 6 000)
    if kept == "all":
        r = matcher.extract_window_members([{"text": text}], codec, invert=True)
        want = [x for i, x in enumerate(fastq_331) if i != 4097]
        old = matcher.extract_window([{"text": text}], logging=False, invert=True)
    elif kept == "one":
        r = matcher.extract_window_members([{"text": text}], codec)
        want = [fastq_331[4097]]
        old = matcher.extract_window([{"text": text}], logging=False)
    else:
        none = b"".join(x for i, x in enumerate(fastq_331) if i != 4097)
        r = matcher.extract_window_members([{"text": none}], codec)
        want = []
        old = matcher.extract_window([{"text": none}], logging=False)
    same_answers(r, old)
    check_members(mk, r["sources"][0], want)
    if kept == "none":
        assert r["sources"][0]["members"] == b"" and r["sources"][0]["n_members"] == 0


def test_fastq_where_every_record_is_kept(mk, codec, fastq_331):
    """all 6 000 kept (a pattern every record holds): the stored form is the written form, member for member"""
    recs = [x[:8] + b"\n" + P + x[9 + len(P):] for x in fastq_331]
    assert all(len(x) == 331 for x in recs)
    m = mk.Matcher(mk.parse_pattern_list(kmer_seq=[P]))
    r = m.extract_window_members([{"text": b"".join(recs)}], codec)
    assert all(r["keep"])
    check_members(mk, r["sources"][0], recs, n_members=-(-6000 * 331 // 49152))


# ---- FASTA ------------------------------------------------------------------------------------------------------------------------
def _fasta_rec(rid, seq, width, eol=b"\n"):
    return b">" + rid + eol + b"".join(seq[k:k + width] + eol for k in range(0, len(seq), width))


def test_fasta(mk, codec, matcher):
    rnd = random.Random(9)
    recs = []
    for i in range(700):
        L = rnd.choice([21, 59, 60, 61, 120, 500, 3000])
        recs.append(_fasta_rec(b"chr%d len=%d" % (i, L), _seq(rnd, L, i % 3 == 0), 60, b"\r\n" if i % 4 == 1 else b"\n"))
    recs[300] = _fasta_rec(b"long", _seq(rnd, 40000, True), 70)  # a raw cut inside (longer than 16 128 bytes)
    big = _seq(rnd, (1 << 20) + 5000, True)
    recs[600] = _fasta_rec(b"big", big, len(big))  # one line of more than 1 MiB: the record that is copied on its own
    recs[601] = _fasta_rec(b"behind the big one", _seq(rnd, 100, True), 60)
    recs[-1] = _fasta_rec(b"last", _seq(rnd, 130, True), 60)[:-1]  # no line end
    assert len(recs[300]) > 40000 and len(recs[600]) > 1 << 20
    text = b"".join(recs)
    assert fasta_records(text) == recs
    r = matcher.extract_window_members([{"text": text}], codec, fmt=mk.MK_TEXT_FASTA)
    same_answers(r, matcher.extract_window([{"text": text}], fmt=mk.MK_TEXT_FASTA, logging=False))
    keep = [i % 3 == 0 or i in (601, 699) for i in range(700)]
    assert r["keep"] == keep
    w = [written_fasta(x) for x, k in zip(recs, keep) if k]
    assert None not in w and w[-1] == recs[-1] + b"\n" and w[:5] == [x for x, k in zip(recs, keep) if k][:5]
    check_members(mk, r["sources"][0], w)


@pytest.mark.parametrize("shape", ["crlf_header_lf_last_line", "lf_header_crlf_last_line", "crlf_header_lf_lines", "blank_line_at_the_end", "no_sequence"])
def test_fasta_of_mixed_line_ends_gives_the_written_bytes_or_status_2(mk, codec, matcher, shape):
    rnd = random.Random(13)
    s = _seq(rnd, 150, True)
    odd = {"crlf_header_lf_last_line": b">odd one\r\n" + s[:60] + b"\r\n" + s[60:120] + b"\r\n" + s[120:] + b"\n",
           "lf_header_crlf_last_line": b">odd one\n" + s[:60] + b"\n" + s[60:] + b"\r\n",
           "crlf_header_lf_lines": b">odd one\r\n" + s[:60] + b"\n" + s[60:] + b"\n",
           "blank_line_at_the_end": b">odd one\n" + s + b"\n\n",
           "no_sequence": b">" + P + b"\n"}[shape]
    want = {"crlf_header_lf_last_line": odd[:-1] + b"\r\n", "lf_header_crlf_last_line": odd[:-2] + b"\n", "crlf_header_lf_lines": odd[:-1] + b"\r\n",
            "blank_line_at_the_end": odd[:-1], "no_sequence": None}[shape]  # (what FastxFile::write makes of it)
    recs = [_fasta_rec(b"a", _seq(rnd, 100, True), 60), odd, _fasta_rec(b"b", _seq(rnd, 100, True), 60)]
    text = b"".join(recs)
    inv = shape == "no_sequence"  # (a record without sequence has no hit: it is kept under -v, with nothing else)
    r = matcher.extract_window_members([{"text": text}], codec, fmt=mk.MK_TEXT_FASTA, invert=inv)
    S = r["sources"][0]
    if r["status"] == 2:
        assert S["members"] == b"" and S["n_members"] == 0 and S["n_written"] == 0 and written_fasta(odd) is None
    else:
        assert r["status"] == 0 and want is not None
        check_members(mk, S, [want] if inv else [recs[0], want, recs[2]])
    if written_fasta(odd) is not None:  # what the header promises the device writes
        assert r["status"] == 0 and written_fasta(odd) == want


# ---- records around the size from which a kept record is copied on its own (1 MiB of stored bytes) ----------------------------------
BIG = 1 << 20


def _one_line_fasta(rnd, rid, stored, hit):
    """a single-line LF record of exactly `stored` bytes (header line + sequence line, line ends included)"""
    rec = b">" + rid + b"\n" + _seq(rnd, stored - len(rid) - 3, hit) + b"\n"
    assert len(rec) == stored
    return rec


@pytest.mark.parametrize("kept_big", ["below_and_above", "below_and_exactly"])
def test_fasta_records_of_one_mebibyte_less_one_exactly_and_plus_one(mk, codec, matcher, kept_big):
    """stored sizes 2^20 - 1, 2^20 and 2^20 + 1 among small records: the kernel's share and the one-by-one copies meet here.  Kept: the
    2^20 - 1 record, one small record and either the 2^20 + 1 record (2^20 dropped) or the 2^20 record (2^20 + 1 dropped)."""
    rnd = random.Random(101 if kept_big == "below_and_above" else 103)
    exact, above = kept_big == "below_and_exactly", kept_big == "below_and_above"
    recs = []
    for i in range(3):
        recs.append(_one_line_fasta(rnd, b"s%d" % i, rnd.choice([40, 100, 333]), False))
    recs.append(_one_line_fasta(rnd, b"below", BIG - 1, True))
    recs.append(_one_line_fasta(rnd, b"small and kept", 200, True))
    recs.append(_one_line_fasta(rnd, b"small and dropped", 77, False))
    recs.append(_one_line_fasta(rnd, b"exactly", BIG, exact))
    recs.append(_one_line_fasta(rnd, b"between", 150, False))
    recs.append(_one_line_fasta(rnd, b"above", BIG + 1, above))
    for i in range(3):
        recs.append(_one_line_fasta(rnd, b"t%d" % i, rnd.choice([40, 100, 333]), False))
    keep = [False] * 3 + [True, True, False, exact, False, above] + [False] * 3
    assert [len(recs[k]) for k in (3, 6, 8)] == [BIG - 1, BIG, BIG + 1]
    text = b"".join(recs)
    assert text.endswith(b"\n") and b"\r" not in text
    stored = b"".join(x for x, k in zip(recs, keep) if k)
    w = [written_fasta(x) for x, k in zip(recs, keep) if k]
    assert None not in w and b"".join(w) == stored  # (LF line ends and a final line end: the written form is the stored one)
    old = matcher.extract_window([{"text": text}], fmt=mk.MK_TEXT_FASTA, logging=False, want=("kept",))
    assert old["status"] == 0 and old["n_rec"] == len(recs) and old["keep"] == keep
    assert old["sources"][0]["kept"] == stored
    r = matcher.extract_window_members([{"text": text}], codec, fmt=mk.MK_TEXT_FASTA, text_below=0)
    assert r["status"] == 0 and r["keep"] == keep
    check_members(mk, r["sources"][0], w)
    r = matcher.extract_window_members([{"text": text}], codec, fmt=mk.MK_TEXT_FASTA, text_below=1 << 30)
    S = r["sources"][0]
    assert r["status"] == 0 and r["keep"] == keep
    assert S["as_text"] and S["n_members"] == 0 and S["n_written"] == len(stored) and S["n_kept"] == len(w) and S["members"] == stored


def test_fastq_record_of_just_over_one_mebibyte(mk, codec, matcher):
    """a sequence of 2^19 bases: 2^20 + 9 stored bytes among small records.  The kept text copies it on its own; the members path
    copies no FASTQ record on its own."""
    rnd = random.Random(107)

    def rec(rid, L, hit):
        return b"@" + rid + b"\n" + _seq(rnd, L, hit) + b"\n+\n" + _rand(rnd, L, b"IJ#5F:,") + b"\n"

    recs = [rec(b"q%d" % i, rnd.choice([36, 100, 151]), i % 2 == 0) for i in range(6)]
    recs.insert(3, rec(b"big", 1 << 19, True))
    keep = [True, False, True, True, False, True, False]
    assert len(recs[3]) == BIG + 9
    text = b"".join(recs)
    stored = b"".join(x for x, k in zip(recs, keep) if k)
    old = matcher.extract_window([{"text": text}], logging=False, want=("kept",))
    assert old["status"] == 0 and old["n_rec"] == len(recs) and old["keep"] == keep
    assert old["sources"][0]["kept"] == stored
    r = matcher.extract_window_members([{"text": text}], codec)
    assert r["status"] == 0 and r["keep"] == keep
    w = [written_fastq(x) for x, k in zip(fastq_records(text), keep) if k]
    assert b"".join(w) == stored
    check_members(mk, r["sources"][0], w)


# ---- two sources, the other body kinds ----------------------------------------------------------------------------------------------
def _pair(n, seed):
    rnd = random.Random(seed)
    a, b = [], []
    for i in range(n):
        L = rnd.choice([40, 75, 100])
        a.append(b"@p%d/1\n" % i + _seq(rnd, L, i % 4 == 0) + b"\n+p%d/1\n" % i + _rand(rnd, L, b"IJ#5") + b"\n")
        b.append(b"@p%d/2\r\n" % i + _seq(rnd, L + 3, i % 6 == 1) + b"\r\n+\r\n" + _rand(rnd, L + 3, b"IJ#5") + b"\r\n")
    return a, b


def test_paired_sources_have_members_of_their_own(mk, codec, matcher):
    a, b = _pair(5000, 21)
    src = [{"text": b"".join(a)}, {"text": b"".join(b)}]
    r = matcher.extract_window_members(src, codec)
    same_answers(r, matcher.extract_window(src, logging=False))
    keep = [i % 4 == 0 or i % 6 == 1 for i in range(5000)]
    assert r["keep"] == keep
    for S, recs in zip(r["sources"], (a, b)):
        check_members(mk, S, [written_fastq(fastq_records(x)[0]) for x, k in zip(recs, keep) if k])
    assert r["sources"][0]["n_written"] != r["sources"][1]["n_written"]


def _bgzf(data, block):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def test_bgzf_body_and_device_text_body(mk, codec, matcher):
    import torch
    text = mixed_fastq(2000, seed=31)
    w = [written_fastq(rec) for rec, k in zip(fastq_records(text), kept_of(2000)) if k]
    blob = _bgzf(text, 60000)
    mem, _, _ = mk.bgzf_members(blob)
    r = matcher.extract_window_members([{"blob": blob, "members": mem}], codec)
    assert r["status"] == 0 and r["keep"] == kept_of(2000)
    check_members(mk, r["sources"][0], w)
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    r = matcher.extract_window_members([{"head": text[:1000], "device_text": (t.data_ptr() + 1000, len(text) - 1000)}], codec)
    assert r["status"] == 0 and r["keep"] == kept_of(2000)
    check_members(mk, r["sources"][0], w)


# ---- logging, text_below, capacities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fastq", "fasta", "paired"])
def test_with_logging_the_ids_are_the_header_lines_and_the_rows_mk_extract_windows(mk, codec, matcher, fmt):
    if fmt == "fastq":
        text = mixed_fastq(5000, seed=41)
        src, f = [{"text": text}], mk.MK_TEXT_FASTQ
        heads = [[_strip(rec[0])[1:] for rec in fastq_records(text)]]
    elif fmt == "paired":
        a, b = _pair(3000, 43)
        src, f = [{"text": b"".join(a)}, {"text": b"".join(b)}], mk.MK_TEXT_FASTQ
        heads = [[_strip(fastq_records(x)[0][0])[1:] for x in side] for side in (a, b)]
    else:
        rnd = random.Random(47)
        recs = [_fasta_rec(b"chr%d some words" % i, _seq(rnd, 200, i % 3 == 0), 60, b"\r\n" if i % 2 else b"\n") for i in range(1500)]
        src, f = [{"text": b"".join(recs)}], mk.MK_TEXT_FASTA
        heads = [[_strip(x[1:x.find(b"\n")]) for x in recs]]
    r = matcher.extract_window_members(src, codec, fmt=f, logging=True)
    old = matcher.extract_window(src, fmt=f, logging=True)
    same_answers(r, old)
    assert len(r["rows"]) > 100
    for S, h in zip(r["sources"], heads):
        kept = [x for x, k in zip(h, r["keep"]) if k]
        assert S["ids"] == b"".join(kept) and S["id_end"] == np.cumsum([len(x) for x in kept]).tolist()
    # every row's record is a kept one: its id is found by the record's rank among the kept
    rank = np.cumsum(r["keep"]) - 1
    for file, rec, _, _ in r["rows"][:50]:
        S = r["sources"][file]
        q = int(rank[rec])
        assert r["keep"][rec] and S["ids"][(S["id_end"][q - 1] if q else 0):S["id_end"][q]] == heads[file][rec]


def test_text_below(mk, codec, matcher):
    text = mixed_fastq(3000, seed=51)
    recs = [written_fastq(rec) for rec, k in zip(fastq_records(text), kept_of(3000)) if k]
    w = b"".join(recs)
    r = matcher.extract_window_members([{"text": text}], codec, text_below=len(w) + 1)
    S = r["sources"][0]
    assert S["as_text"] and S["members"] == w and S["n_members"] == 0 and S["n_written"] == len(w) and S["n_kept"] == 1000
    r = matcher.extract_window_members([{"text": text}], codec, text_below=len(w))  # "shorter than": not this one
    S = r["sources"][0]
    check_members(mk, S, recs)


def _raw_call(mk, matcher, codec, text, caps, logging, text_below=0, invert=False):
    """the entry point itself with guarded outputs -> (rc, the mk_window_members, the buffers)"""
    L = mk.load()
    arr, hold, bound = matcher._window_sources([{"text": text}])
    cap = bound // 8 + 2
    bufs = {"members": HostBuf(np.uint8, caps["members"]), "ids": HostBuf(np.uint8, caps["ids"]), "id_end": HostBuf(np.uint64, cap),
            "rec_start": HostBuf(np.uint64, cap + 1), "keep": HostBuf(np.uint8, cap), "tail": HostBuf(np.uint8, 64)}
    arr[0].rec_start, arr[0].tail, arr[0].tail_cap = bufs["rec_start"].ptr, bufs["tail"].ptr, 64
    M = (mk.WindowMembers * 1)()
    M[0].members, M[0].members_cap, M[0].ids, M[0].ids_cap = bufs["members"].ptr, caps["members"], bufs["ids"].ptr, caps["ids"]
    M[0].id_end, M[0].text_below = bufs["id_end"].ptr, text_below
    rows = np.zeros(1 << 16, dtype=mk.ROW_DTYPE)
    n_rec, status, n_rows, c2, k2 = C.c_uint64(), C.c_uint32(), C.c_uint64(), mk.Counters(), np.zeros(len(matcher.patterns), dtype=np.uint32)
    rc = L.mk_extract_window_members(matcher._h, codec._h, mk.MK_TEXT_FASTQ, 1, arr, M, int(logging), int(invert), cap, C.byref(n_rec),
                                     bufs["keep"].ptr, rows.ctypes.data, len(rows), C.byref(n_rows), C.byref(c2), k2.ctypes.data, C.byref(status))
    assert status.value == 0
    return rc, M[0], bufs


@pytest.mark.parametrize("text_below", [0, 1 << 30])
def test_capacity_exact_fit_one_short_and_guards(mk, codec, matcher, text_below):
    text = mixed_fastq(3000, seed=61)
    rc, M, bufs = _raw_call(mk, matcher, codec, text, {"members": 1 << 20, "ids": 1 << 16}, True, text_below)
    assert rc == mk.MK_OK and M.n_member_bytes > 1000 and M.n_id_bytes > 1000 and M.n_kept == 1000 and bool(M.as_text) == bool(text_below)
    need = {"members": int(M.n_member_bytes), "ids": int(M.n_id_bytes)}
    want = {k: bufs[k].view(need[k]).tobytes() for k in need}
    id_end = bufs["id_end"].view(1000).tolist()
    assert bufs["members"].untouched_from(need["members"]) and bufs["ids"].untouched_from(need["ids"]) and bufs["id_end"].untouched_from(1000)
    rc, M, bufs = _raw_call(mk, matcher, codec, text, need, True, text_below)  # exact fit
    assert rc == mk.MK_OK and {k: bufs[k].view(need[k]).tobytes() for k in need} == want and bufs["id_end"].view(1000).tolist() == id_end
    assert all(b.guard_intact() for b in bufs.values())
    for short in ("members", "ids", "both"):
        caps = {k: need[k] - (1 if short in (k, "both") else 0) for k in need}
        rc, M, bufs = _raw_call(mk, matcher, codec, text, caps, True, text_below)
        assert rc == mk.MK_E_CAPACITY, short
        err = mk.load().mk_last_error()
        if short != "ids":
            assert M.n_member_bytes == need["members"]
        if short != "members":
            assert M.n_id_bytes == need["ids"] and str(need["ids"]).encode() in err
        else:
            assert str(need["members"]).encode() in err
        for k in need:
            assert bufs[k].guard_intact() and bufs[k].untouched_from(caps[k]), (short, k)
        assert all(b.guard_intact() for b in bufs.values())
    rc, M, bufs = _raw_call(mk, matcher, codec, text, need, True, text_below)  # the handles afterwards
    assert rc == mk.MK_OK and {k: bufs[k].view(need[k]).tobytes() for k in need} == want


def test_logging_with_invert_and_other_arguments_are_refused(mk, codec, matcher):
    text = mixed_fastq(40, seed=71)
    rc, _, bufs = _raw_call(mk, matcher, codec, text, {"members": 1 << 16, "ids": 1 << 12}, True, invert=True)
    assert rc == mk.MK_E_INVALID_ARG and all(b.untouched_from(0) for b in bufs.values())
    with pytest.raises(mk.MerkurioError) as e:  # the codec is required
        matcher.extract_window_members([{"text": text}], None)
    assert e.value.code == mk.MK_E_INVALID_ARG


def test_cut_times_are_this_calls(mk, codec, matcher):
    text = mixed_fastq(3000, seed=81)
    r = matcher.extract_window_members([{"text": text}], codec)
    n, ms = codec.cut_times()
    assert n == r["sources"][0]["n_members"] > 0 and all(x > 0 for x in ms) and r["sources"][0]["written_ms"] > 0
