"""mk_extract_window_open on the device (an addition to ABI v7): a text window that may start anywhere.  The call names the start the
Python restatement of the rule names (tests/open_start.py) and, from there on, returns what mk_extract_window returns for the text
behind that start, shifted by n_front -- at every cut byte across several records, at the kernels' thread (64 bytes), wave (4 096) and
block (16 384) edges and at the search kernel's own wave and block edges (lines 256, 4 096).  A file cut into windows at arbitrary
bytes -- window 0 ordinary, the others open, a seam call for tail(k - 1) ++ front(k) between them -- joins to what one whole-file call
and the oracle's extract loop give.  On reads made to fool the rule the seam call refuses every false start and passes no false one.

The module needs Matcher.extract_window_open: on a build without the entry point it fails at import."""
import zlib

import pytest

import open_start as osr
import oracle_binding as ob
from merkurio_amd.native import Matcher

assert hasattr(Matcher, "extract_window_open"), "this build has no mk_extract_window_open"

pytestmark = pytest.mark.gpu
FMT = {"fastq": 0, "fasta": 1}


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def patterns(mk):
    return mk.parse_pattern_list(kmer_seq=osr.kmers(), reverse_complement=True)


@pytest.fixture(scope="module")
def matcher(mk, patterns):
    return mk.Matcher(patterns)


def _open(m, text, fmt, ends=True, **kw):
    return m.extract_window_open([{"text": text, "ends_at_record": ends}], fmt=FMT[fmt], **kw)


def _plain(m, text, fmt, ends=True, head=b"", **kw):
    return m.extract_window([{"head": head, "text": text, "ends_at_record": ends}], fmt=FMT[fmt], **kw)


def _assert_shifted(r, o, f, text):
    """r: the open call on `text`; o: the ordinary call on text[f:]"""
    assert r["status"] == 0 and o["status"] == 0 and r["n_front"] == f and r["front"] == text[:f]
    assert r["n_rec"] == o["n_rec"] and r["keep"] == o["keep"] and r["rows"] == o["rows"] and r["counters"] == o["counters"]
    S, T = r["sources"][0], o["sources"][0]
    assert S["rec_start"] == [x + f for x in T["rec_start"]] and S["n_used"] == T["n_used"] + f and S["n_window"] == len(text)
    assert S["tail"] == T["tail"] and S["n_rec_seen"] == T["n_rec_seen"]


def _sweep(m, text, fmt, cuts_at, ends=False):
    """every cut of cuts_at: the start the rule names, then the ordinary call's results behind it (one ordinary call per start)"""
    cuts = osr.Cuts(text, fmt)
    plain = {}
    starts = set()
    for c in cuts_at:
        f = cuts.n_front(c)
        assert f is not None
        if c + f not in plain:
            plain[c + f] = _plain(m, text[c + f:], fmt, ends)
        _assert_shifted(_open(m, text[c:], fmt, ends), plain[c + f], f, text[c:])
        starts.add(c + f)
    return starts


def _swept_records(text, fmt, first=2, n=4):
    """every byte of n consecutive records (four, or five) from record `first` on, and the byte behind them"""
    rs = sorted(osr.record_starts(text, fmt))
    return range(rs[first], rs[first + n] + 1)


@pytest.mark.parametrize("eol,final_eol,plus_id", [(osr.LF, True, False), (osr.CRLF, True, True), (osr.LF, False, True), (osr.CRLF, False, False)])
def test_every_cut_byte_fastq(matcher, patterns, eol, final_eol, plus_id):
    text, _ = osr.sweep_fastq(eol, final_eol, plus_id, planted=patterns)
    sweep = _swept_records(text, "fastq")
    assert len(_sweep(matcher, text, "fastq", sweep, ends=True)) >= 4
    # the same cuts in a window that ends anywhere: the unfinished record stays behind as the tail
    assert len(_sweep(matcher, text[:len(text) - 77], "fastq", list(sweep)[::9], ends=False)) >= 4


@pytest.mark.parametrize("width", [0, 60, 80])
def test_every_cut_byte_fasta(matcher, patterns, width):
    text, _ = osr.sweep_fasta(width, planted=patterns)
    starts = _sweep(matcher, text, "fasta", _swept_records(text, "fasta", 3, 5), ends=True)
    # ... and a cut one byte in front of four later records per residue mod 16 of their starts (the FASTA kernel's loads stay aligned)
    by_residue = {}
    for s in sorted(osr.record_starts(text, "fasta"))[20:]:
        if len(by_residue.setdefault(s % 16, [])) < 4:
            by_residue[s % 16].append(s)
    assert len(by_residue) == 16
    later = [s for group in by_residue.values() for s in group]
    assert _sweep(matcher, text, "fasta", [s - 1 for s in later], ends=(width == 60)) == set(later)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_kernel_edges(matcher, fmt):
    for at in osr.EDGE_BYTES:
        text = osr.start_at_byte(at, fmt)
        _assert_shifted(_open(matcher, text, fmt), _plain(matcher, text[at:], fmt), at, text)
    for line in osr.EDGE_LINES:
        text = osr.start_at_line(line, fmt)
        assert osr.open_start(text, fmt) == (line, 3 * line)
        _assert_shifted(_open(matcher, text, fmt), _plain(matcher, text[3 * line:], fmt), 3 * line, text)


def test_one_shape_alone_is_passed_over_and_line_0_is_not_taken(matcher):
    text = osr.one_shape_alone()
    f = osr.open_start(text)[1]
    assert f == text.index(b"@b0\n") and f > text.index(b"@lone")
    _assert_shifted(_open(matcher, text, "fastq"), _plain(matcher, text[f:], "fastq"), f, text)
    for fmt, body in (("fastq", osr.body_fastq()), ("fasta", osr.body_fasta())):
        f = osr.open_start(body, fmt)[1]
        assert f == sorted(osr.record_starts(body, fmt))[1]  # the SECOND record: line 0 begins with the marker and is not taken
        _assert_shifted(_open(matcher, body, fmt), _plain(matcher, body[f:], fmt), f, body)


# ---- a whole file from windows ---------------------------------------------------------------------------------------------------------
def _add(total, c):
    for k, v in c.items():
        if k not in total:
            total[k] = v
        elif isinstance(v, (tuple, list)):
            total[k] = type(v)(a + b for a, b in zip(total[k], v))
        else:
            total[k] += v


def _join(m, text, cuts, fmt, invert=False):
    """window 0 ordinary, windows 1 .. open, a seam call between neighbours; a disproved guess is run again the chained way.
    -> (keep, kept text, rows with file-wide record numbers, summed counters, re-runs)"""
    bounds = [0] + list(cuts) + [len(text)]
    keep, kept, rows, total, reruns = [], [], [], {}, 0

    def take(r):
        base = len(keep)
        keep.extend(r["keep"])
        kept.append(r["sources"][0]["kept"])
        rows.extend((f, rec + base, p, pos) for f, rec, p, pos in r["rows"])
        _add(total, r["counters"])

    tail = b""
    for k in range(len(bounds) - 1):
        body, last = text[bounds[k]:bounds[k + 1]], k == len(bounds) - 2
        if k == 0:
            r = _plain(m, body, fmt, last, invert=invert, want=("tail", "kept"))
        else:
            r = _open(m, body, fmt, last, invert=invert, want=("tail", "kept"))
            ok = r["status"] == 0
            if ok:
                seam_text = tail + r["front"]
                seam = _plain(m, seam_text, fmt, True, invert=invert, want=("tail", "kept"))
                ok = seam["status"] == 0 and seam["sources"][0]["n_used"] == len(seam_text)
            if ok:
                take(seam)
            else:  # disproved: the chained way, head = the tail of the window in front
                reruns += 1
                r = _plain(m, body, fmt, last, head=tail, invert=invert, want=("tail", "kept"))
        assert r["status"] == 0
        take(r)
        tail = r["sources"][0]["tail"]
    assert tail == b""
    return keep, b"".join(kept), rows, total, reruns


@pytest.mark.parametrize("fmt,algo,invert", [("fastq", "ac", False), ("fastq", "bndmq", False), ("fastq", "ac", True), ("fasta", "ac", False),
                                             ("fasta", "bndmq", True)])
def test_whole_file_from_windows(mk, patterns, fmt, algo, invert):
    pats = patterns if algo == "ac" else patterns[:2]  # (two patterns: the reference's rule selects BNDMq)
    m = mk.Matcher(pats)
    assert m.use_ac == (algo == "ac")
    text, seqs = osr.sweep_fastq(osr.LF, True, True, planted=pats) if fmt == "fastq" else osr.sweep_fasta(60, planted=pats)
    whole = _plain(m, text, fmt, True, invert=invert, want=("tail", "kept"))
    k_o, r_o, c_o = ob.extract_single(ob.Matcher(pats, m.use_ac, 0, False), seqs, logging=True, invert=invert)
    assert whole["keep"] == k_o and whole["rows"] == r_o and whole["counters"] == c_o and any(k_o) and not all(k_o)
    n = len(text)
    for cuts in ([n // 2 + 3], [n // 3 + 1, 2 * n // 3 + 29], [n * k // 7 + 13 * k for k in range(1, 7)]):
        keep, kept, rows, total, reruns = _join(m, text, cuts, fmt, invert)
        assert reruns == 0  # ordinary reads: every guess is true
        assert keep == whole["keep"] and kept == whole["sources"][0]["kept"] and rows == whole["rows"] and total == whole["counters"]
        assert total["pattern_hit_counts"] == c_o["pattern_hit_counts"]


# ---- a guess made to fail ----------------------------------------------------------------------------------------------------------------
def test_false_starts_are_refused_by_the_seam_and_no_false_one_passes(mk):
    text, seqs = osr.adversarial()
    pats = mk.parse_pattern_list(kmer_seq=[b"ACG", b"TTA", b"GGC"])
    m = mk.Matcher(pats)
    whole = _plain(m, text, "fastq", True, want=("tail", "kept"))
    k_o, r_o, c_o = ob.extract_single(ob.Matcher(pats, m.use_ac, 0, False), seqs, logging=True)
    assert whole["keep"] == k_o and whole["rows"] == r_o and whole["counters"] == c_o
    true = sorted(osr.record_starts(text))
    cuts = osr.Cuts(text)
    seams = {}
    refused = passed = none = 0
    for c in range(1, len(text)):
        r = _open(m, text[c:], "fastq", False)  # a window in mid-file: it may end anywhere
        f = cuts.n_front(c)
        if f is None:
            assert r["status"] == 2 and r["n_front"] == len(text) - c
            none += 1
            continue
        assert r["status"] == 0 and r["n_front"] == f  # (these reads have the shape at the false starts too: nothing is refused here)
        # the file's last window from the same byte: its lines behind a false start are no whole records, which the index says itself
        r = _open(m, text[c:], "fastq", True)
        assert r["n_front"] == f and r["status"] == (0 if c + f in true else 1)
        # the tail of the window in front, text[:c] read from the file's start: from its last whole record on
        lines_before = text[:c].count(b"\n")
        tail_from = true[lines_before // 4] if lines_before // 4 < len(true) else len(text)
        key = (tail_from, c + f)
        if key not in seams:
            seam_text = text[tail_from:c + f]
            s = _plain(m, seam_text, "fastq", True)
            seams[key] = s["status"] == 0 and s["sources"][0]["n_used"] == len(seam_text)
        assert seams[key] == (c + f in true)  # refused exactly when the named start is false
        refused += not seams[key]
        passed += seams[key]
    assert refused > passed > 50 and none > 0
    # cuts at false starts: the chained re-run gives the whole file's result
    false_cuts = [c for c in range(len(text) // 4, len(text) // 2) if cuts.n_front(c) is not None and c + cuts.n_front(c) not in true]
    for c in false_cuts[::23]:
        keep, kept, rows, total, reruns = _join(m, text, [c], "fastq")
        assert reruns == 1
        assert keep == whole["keep"] and kept == whole["sources"][0]["kept"] and rows == whole["rows"] and total == whole["counters"]


# ---- status 2, capacity ------------------------------------------------------------------------------------------------------------------
def test_status_2(matcher):
    body = osr.body_fastq()
    start = osr.line_starts(body)
    for text, fmt in ((b"III\n" + body[:start[8] - 1], "fastq"), (body[:start[8]], "fastq"), (body[:start[12] - 1], "fastq"), (b"", "fastq"), (b"", "fasta"),
                      (b"ACGT\n" * 5000 + b"ACG", "fasta"), (b">only\n" + b"ACGT\n" * 5000, "fasta")):
        assert osr.open_start(text, fmt) is None
        for ends in (True, False):
            r = _open(matcher, text, fmt, ends)
            assert r["status"] == 2 and r["n_rec"] == 0 and r["n_front"] == len(text) and r["keep"] == [] and r["rows"] == []
    # one line more and there is a start
    r = _open(matcher, b"III\n" + body[:start[8]], "fastq", False)
    assert r["status"] == 0 and r["n_front"] == 4 and r["n_rec"] == 2


def test_front_capacity_is_stated_and_a_second_call_succeeds(mk, matcher):
    text = osr.start_at_byte(4097)
    for cap in (0, 1, 4096):
        with pytest.raises(mk.MerkurioError) as e:
            _open(matcher, text, "fastq", front_cap=cap)
        assert e.value.code == mk.MK_E_CAPACITY and e.value.n_front == 4097
    r = _open(matcher, text, "fastq", front_cap=4097)  # an exact fit
    _assert_shifted(r, _plain(matcher, text[4097:], "fastq"), 4097, text)
    # front is reported in front of tail: a call whose tail does not fit either names the front
    L = mk.load()
    import ctypes as C
    import numpy as np
    cut = text[:len(text) - 5]
    buf = np.frombuffer(cut, dtype=np.uint8)
    arr = (mk.WindowSource * 1)()
    tail = np.zeros(1, dtype=np.uint8)
    arr[0].text, arr[0].n_text, arr[0].ends_at_record = buf.ctypes.data, len(cut), 0
    arr[0].tail, arr[0].tail_cap = tail.ctypes.data, 1
    F = mk.WindowFront()
    keep = np.zeros(64, dtype=np.uint8)
    n_rec, n_rows, status, cnt = C.c_uint64(), C.c_uint64(), C.c_uint32(), mk.Counters()
    rc = L.mk_extract_window_open(matcher.handle, None, 0, 1, arr, 0, 0, 64, C.byref(n_rec), keep.ctypes.data, None, 0, C.byref(n_rows), C.byref(cnt), None,
                                  C.byref(status), C.addressof(F))
    assert rc == mk.MK_E_CAPACITY and F.n_front == 4097 and b"front" in L.mk_last_error()


# ---- BGZF body ------------------------------------------------------------------------------------------------------------------------------
def _bgzf(data, sizes, level=6):
    import struct
    out, pos, k = bytearray(), 0, 0
    while pos < len(data):
        chunk = data[pos:pos + sizes[k % len(sizes)]]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
        pos += len(chunk)
        k += 1
    return bytes(out)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_a_window_of_members_that_starts_in_mid_record_equals_the_plain_text_call(mk, matcher, patterns, fmt):
    text, _ = osr.sweep_fastq(osr.LF, True, False, planted=patterns) if fmt == "fastq" else osr.sweep_fasta(80, planted=patterns)
    blob = _bgzf(text, [777, 20000, 4099, 12345])
    members, _, n_text = mk.bgzf_members(blob)
    assert n_text == len(text) and len(members) >= 8
    true = osr.record_starts(text, fmt)
    codec = mk.Codec(0)
    tried = 0
    for first in range(1, len(members) - 2):
        at = int(members["out_off"][first])
        if at in true:
            continue
        tried += 1
        r = matcher.extract_window_open([{"blob": blob, "members": members[first:], "ends_at_record": True}], fmt=FMT[fmt], codec=codec, want=("tail", "kept"))
        o = _open(matcher, text[at:], fmt, True, want=("tail", "kept"))
        assert r == o and r["status"] == 0 and at + r["n_front"] in true
    assert tried >= 5
    codec.close()
