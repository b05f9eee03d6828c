"""mk_extract_window_frames: a window's kept records leave the device as zstd frames of their WRITTEN form (include/merkurio_hip.h) --
mk_extract_window_members with the other codec.  The expected text is the restatement of the written form in window_frames_cases.py;
every frame is decoded ALONE by libzstd, its content size is the matching difference of mk.zstd_record_cuts of the written record ends,
and the blob is byte for byte Codec.zstd_records of the written text and ends (the same kernels on the same ranges).  keep, rows and
counters are mk_extract_window's.  New here for the cut kernel: the end table is the offsets scan of the window, in which a record
that is not kept repeats the end in front of it -- the sparse cases make every search land in such a run."""
import ctypes as C
import random
import struct
import zlib

import numpy as np
import pytest

import window_frames_cases as wf
import zstd_out_cases as zo
from guarded import HostBuf
from window_frames_cases import P, fasta_rec, fasta_records, fastq_records, kept_of, mixed_fastq, one_line_fasta, rand, seq, written_fasta, written_fastq

pytestmark = pytest.mark.gpu

G, M = zo.GRID, zo.TEXT_MAX


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
def checker(mk):
    """a second handle for Codec.zstd_records: the first keeps what mk_zstd_deflate_info says about the window call"""
    c = mk.Codec()
    yield c
    c.close()


@pytest.fixture(scope="module")
def matcher(mk):
    return mk.Matcher(mk.parse_pattern_list(kmer_seq=[P], reverse_complement=True))


def check_frames(mk, checker, S, written, n_frames=None):
    """S: a source of extract_window_frames; written: the written forms of its kept records, in order.  -> the frames' text sizes"""
    text = b"".join(written)
    assert not S["as_text"] and S["n_written"] == len(text) and S["n_kept"] == len(written)
    blob = S["members"]
    if not text:
        assert blob == b"" and S["n_members"] == 0
        return []
    frames = zo.frames_by_libzstd(blob)  # (every frame decoded alone)
    ends = np.cumsum([len(w) for w in written])
    cuts = mk.zstd_record_cuts(ends)
    sizes = np.diff(cuts).tolist()
    assert cuts.tolist() == zo.rule(ends)
    assert S["n_members"] == len(frames) == len(sizes)
    assert [zo.shape(f)["text"] for f, _ in frames] == sizes and [len(t) for _, t in frames] == sizes
    if n_frames is not None:
        assert len(frames) == n_frames
    got = b"".join(t for _, t in frames)
    if got != text:
        k = next(i for i in range(min(len(text), len(got))) if got[i] != text[i])
        raise AssertionError("written text differs at byte %d: %r, expected %r" % (k, got[max(0, k - 40):k + 20], text[max(0, k - 40):k + 20]))
    assert blob == checker.zstd_records(text, ends), "the frames differ from mk_zstd_deflate_records' of the same text and ends"
    return sizes


def same_answers(r, old):
    assert r["status"] == old["status"] == 0 and r["n_rec"] == old["n_rec"]
    assert r["keep"] == old["keep"] and r["rows"] == old["rows"] and r["counters"] == old["counters"]
    for a, b in zip(r["sources"], old["sources"]):
        assert all(a[k] == b[k] for k in ("n_window", "n_used", "n_rec_seen", "rec_start", "tail"))


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------------
def test_fastq_mixed_shapes(mk, codec, checker, matcher):
    """600 records of mixed lengths and line ends; the last kept one has no line end"""
    text = mixed_fastq(600)
    recs = fastq_records(text)
    assert len(recs) == 600
    r = matcher.extract_window_frames([{"text": text}], codec)
    same_answers(r, matcher.extract_window([{"text": text}], logging=False))
    assert r["keep"] == kept_of(600)
    w = [written_fastq(rec) for rec, k in zip(recs, kept_of(600)) if k]
    assert w[-1] == written_fastq(recs[-1]) and not text.endswith(b"\n") and any(x.endswith(b"\r\n") for x in w)
    check_frames(mk, checker, r["sources"][0], w)


@pytest.fixture(scope="module")
def fastq_331():
    rnd = random.Random(5)
    recs = [b"@r%06d\n" % i + seq(rnd, 159, i == 257) + b"\n+\n" + rand(rnd, 159, b"IJ#5F:,") + b"\n" for i in range(800)]
    assert all(len(x) == 331 for x in recs)
    return recs


@pytest.mark.parametrize("kept", ["all", "one", "none"])
def test_fastq_all_one_none_kept(mk, codec, checker, matcher, fastq_331, kept):
    text = b"".join(fastq_331)
    if kept == "all":  # (-v keeps the 799 records without P: 264 469 bytes, three frames)
        r = matcher.extract_window_frames([{"text": text}], codec, invert=True)
        want = [x for i, x in enumerate(fastq_331) if i != 257]
        old = matcher.extract_window([{"text": text}], logging=False, invert=True)
    elif kept == "one":
        r = matcher.extract_window_frames([{"text": text}], codec)
        want = [fastq_331[257]]
        old = matcher.extract_window([{"text": text}], logging=False)
    else:
        none = b"".join(x for i, x in enumerate(fastq_331) if i != 257)
        r = matcher.extract_window_frames([{"text": none}], codec)
        want = []
        old = matcher.extract_window([{"text": none}], logging=False)
    same_answers(r, old)
    sizes = check_frames(mk, checker, r["sources"][0], want)
    if kept == "all":
        assert len(sizes) == 3
    if kept == "none":
        S = r["sources"][0]
        assert S["members"] == b"" and S["n_members"] == 0 and not S["as_text"] and S["n_written"] == 0


# ---- sparse keeps: runs of equal ends in the table the cut kernel searches -----------------------------------------------------------
@pytest.mark.parametrize("only", [None, "first", "last"], ids=["all_over", "first_grid_bytes", "last_grid_bytes"])
def test_sparse_keeps_of_3000_records(mk, codec, checker, matcher, only):
    """every 50th of 3 000 records of 313 bytes: 49 ends repeat between two that move; then the kept ones only in the first / only in
    the last 114 688 bytes of the window, so that the run of equal ends is the table's tail / its head"""
    text, keep, rec = wf.sparse_fastq(3000, 50, only)
    assert 0 < sum(keep) <= 60 and (only is None) == (sum(keep) == 60)
    r = matcher.extract_window_frames([{"text": text}], codec)
    same_answers(r, matcher.extract_window([{"text": text}], logging=False))
    assert r["keep"] == keep
    check_frames(mk, checker, r["sources"][0], [rec[i].tobytes() for i in np.flatnonzero(keep)], n_frames=1)


def test_sparse_keeps_where_every_grid_point_lands_in_a_run_of_equal_ends(mk, codec, checker, matcher):
    """40 000 records with every 50th kept: 800 x 313 = 250 400 written bytes, two inner grid points -- and in the end table 49 of 50
    entries repeat their neighbour, so both searches end inside a run (the smallest end >= x is the run's value)"""
    text, keep, rec = wf.sparse_fastq(40000, 50, None, seed=19)
    assert sum(keep) == 800 and 800 * wf.SPARSE_REC > 2 * G
    r = matcher.extract_window_frames([{"text": text}], codec)
    assert r["status"] == 0 and r["keep"] == keep
    sizes = check_frames(mk, checker, r["sources"][0], [rec[i].tobytes() for i in np.flatnonzero(keep)], n_frames=3)
    assert all(s % wf.SPARSE_REC == 0 for s in sizes)  # every frame is whole records


# ---- record ends around the rule's edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("edge", list(wf.EDGES))
def test_record_ends_at_the_rules_edges(mk, codec, checker, matcher, edge, delta):
    ends = wf.edge_ends(edge, delta)
    text, keep, written = wf.fasta_with_written_ends(ends)
    target = wf.EDGES[edge] + delta
    assert target in ends
    r = matcher.extract_window_frames([{"text": text}], codec, fmt=mk.MK_TEXT_FASTA)
    assert r["status"] == 0 and r["keep"] == keep
    check_frames(mk, checker, r["sources"][0], written)
    cuts = mk.zstd_record_cuts(ends).tolist()
    assert (target in cuts) == wf.edge_is_cut(edge, delta)


@pytest.mark.parametrize("length", [M - 1, M, M + 1])
def test_fasta_record_longer_than_the_reach(mk, codec, checker, matcher, length):
    """one kept record of 131 071 / 131 072 / 131 073 written bytes behind a small one: the grid points inside it find no end within
    reach and cut on the grid, inside the record"""
    rnd = random.Random(200 + length - M)
    recs = [one_line_fasta(rnd, b"small", 300, True), one_line_fasta(rnd, b"dropped", 100, False), one_line_fasta(rnd, b"long", length, True),
            one_line_fasta(rnd, b"behind", 250, True)]
    keep = [True, False, True, True]
    r = matcher.extract_window_frames([{"text": b"".join(recs)}], codec, fmt=mk.MK_TEXT_FASTA)
    assert r["status"] == 0 and r["keep"] == keep
    sizes = check_frames(mk, checker, r["sources"][0], [x for x, k in zip(recs, keep) if k])
    assert sizes[0] == G and max(sizes) <= M  # the first cut is the grid point inside the long record


BIG = 1 << 20


@pytest.mark.parametrize("stored", [BIG - 1, BIG, BIG + 1])
def test_fasta_record_of_one_mebibyte(mk, codec, checker, matcher, stored):
    """the size from which a kept record is copied on its own, and one byte either side, kept next to small ones"""
    rnd = random.Random(300 + stored - BIG)
    recs = [one_line_fasta(rnd, b"s0", 333, True), one_line_fasta(rnd, b"s1", 77, False), one_line_fasta(rnd, b"big", stored, True),
            one_line_fasta(rnd, b"s2", 150, False), one_line_fasta(rnd, b"s3", 200, True)]
    keep = [True, False, True, False, True]
    r = matcher.extract_window_frames([{"text": b"".join(recs)}], codec, fmt=mk.MK_TEXT_FASTA)
    assert r["status"] == 0 and r["keep"] == keep
    check_frames(mk, checker, r["sources"][0], [x for x, k in zip(recs, keep) if k])


@pytest.mark.parametrize("shape", ["crlf_header_lf_last_line", "lf_header_crlf_last_line", "crlf_header_lf_lines", "blank_line_at_the_end", "no_sequence"])
def test_fasta_of_mixed_line_ends_gives_the_written_bytes_or_status_2(mk, codec, checker, matcher, shape):
    rnd = random.Random(13)
    s = seq(rnd, 150, True)
    odd = {"crlf_header_lf_last_line": b">odd one\r\n" + s[:60] + b"\r\n" + s[60:120] + b"\r\n" + s[120:] + b"\n",
           "lf_header_crlf_last_line": b">odd one\n" + s[:60] + b"\n" + s[60:] + b"\r\n",
           "crlf_header_lf_lines": b">odd one\r\n" + s[:60] + b"\n" + s[60:] + b"\n",
           "blank_line_at_the_end": b">odd one\n" + s + b"\n\n",
           "no_sequence": b">" + P + b"\n"}[shape]
    want = {"crlf_header_lf_last_line": odd[:-1] + b"\r\n", "lf_header_crlf_last_line": odd[:-2] + b"\n", "crlf_header_lf_lines": odd[:-1] + b"\r\n",
            "blank_line_at_the_end": odd[:-1], "no_sequence": None}[shape]  # (what the host writer makes of it)
    recs = [fasta_rec(b"a", seq(rnd, 100, True), 60), odd, fasta_rec(b"b", seq(rnd, 100, True), 60)]
    inv = shape == "no_sequence"  # (a record without sequence has no hit: it is kept under -v, with nothing else)
    r = matcher.extract_window_frames([{"text": b"".join(recs)}], codec, fmt=mk.MK_TEXT_FASTA, invert=inv)
    S = r["sources"][0]
    if r["status"] == 2:
        assert S["members"] == b"" and S["n_members"] == 0 and S["n_written"] == 0 and written_fasta(odd) is None
    else:
        assert r["status"] == 0 and want is not None
        check_frames(mk, checker, S, [want] if inv else [recs[0], want, recs[2]])
    if written_fasta(odd) is not None:  # what the header promises the device writes
        assert r["status"] == 0 and written_fasta(odd) == want


# ---- two sources, the other body kinds ----------------------------------------------------------------------------------------------
def _pair(n, seed):
    rnd = random.Random(seed)
    a, b = [], []
    for i in range(n):
        L = rnd.choice([40, 75, 100])
        a.append(b"@p%d/1\n" % i + seq(rnd, L, i % 4 == 0) + b"\n+p%d/1\n" % i + rand(rnd, L, b"IJ#5") + b"\n")
        b.append(b"@p%d/2\r\n" % i + seq(rnd, L + 3, i % 6 == 1) + b"\r\n+\r\n" + rand(rnd, L + 3, b"IJ#5") + b"\r\n")
    return a, b


def test_paired_sources_have_frames_of_their_own_and_the_info_is_their_sum(mk, codec, checker, matcher):
    a, b = _pair(2500, 21)
    src = [{"text": b"".join(a)}, {"text": b"".join(b)}]
    r = matcher.extract_window_frames(src, codec)
    n, kinds, ms = codec.zstd_records_info()
    same_answers(r, matcher.extract_window(src, logging=False))
    keep = [i % 4 == 0 or i % 6 == 1 for i in range(2500)]
    assert r["keep"] == keep
    for S, recs in zip(r["sources"], (a, b)):
        check_frames(mk, checker, S, [written_fastq(fastq_records(x)[0]) for x, k in zip(recs, keep) if k])
    assert r["sources"][0]["n_written"] != r["sources"][1]["n_written"]
    each = [S["n_members"] for S in r["sources"]]
    assert min(each) >= 2 and n == sum(each) and sum(kinds) == n  # (one block per frame)
    assert ms[0] == 0 and ms[1] > 0 and ms[2] > 0 and all(S["written_ms"] > 0 for S in r["sources"])


def _bgzf(data, block):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def test_bgzf_body_and_device_text_body(mk, codec, checker, matcher):
    import zstd_cases as zc
    text = mixed_fastq(2000, seed=31)
    w = [written_fastq(rec) for rec, k in zip(fastq_records(text), kept_of(2000)) if k]
    blob = _bgzf(text, 60000)
    mem, _, _ = mk.bgzf_members(blob)
    r = matcher.extract_window_frames([{"blob": blob, "members": mem}], codec)
    assert r["status"] == 0 and r["keep"] == kept_of(2000)
    check_frames(mk, checker, r["sources"][0], w)
    # a text that a decoder left on the device (here: another handle's unzstd), from byte 1000 on, behind a head from the host
    other = mk.Codec()
    assert other.unzstd(zc.compress(text))[:2] == (True, text)
    n = C.c_uint64(0)
    d_text = mk.load().mk_gzip_text_device(other._h, C.byref(n))
    assert d_text and n.value == len(text)
    r = matcher.extract_window_frames([{"head": text[:1000], "device_text": (d_text + 1000, len(text) - 1000)}], codec)
    assert r["status"] == 0 and r["keep"] == kept_of(2000)
    check_frames(mk, checker, r["sources"][0], w)
    other.close()


def test_the_frames_go_back_through_the_device_decoder(mk, codec, matcher):
    text = mixed_fastq(1500, seed=33)
    w = b"".join(written_fastq(rec) for rec, k in zip(fastq_records(text), kept_of(1500)) if k)
    r = matcher.extract_window_frames([{"text": text}], codec)
    S = r["sources"][0]
    assert S["n_members"] >= 1 and len(w) > 1000
    taken, back, blocks = codec.unzstd(S["members"])
    assert taken and back == w and blocks == S["n_members"]  # (one block per frame)


# ---- logging, text_below, capacities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fastq", "fasta", "paired"])
def test_with_logging_the_ids_are_the_header_lines_and_the_rows_mk_extract_windows(mk, codec, matcher, fmt):
    if fmt == "fastq":
        text = mixed_fastq(1500, seed=41)
        src, f = [{"text": text}], mk.MK_TEXT_FASTQ
        heads = [[wf.strip(rec[0])[1:] for rec in fastq_records(text)]]
    elif fmt == "paired":
        a, b = _pair(1200, 43)
        src, f = [{"text": b"".join(a)}, {"text": b"".join(b)}], mk.MK_TEXT_FASTQ
        heads = [[wf.strip(fastq_records(x)[0][0])[1:] for x in side] for side in (a, b)]
    else:
        rnd = random.Random(47)
        recs = [fasta_rec(b"chr%d some words" % i, seq(rnd, 200, i % 3 == 0), 60, b"\r\n" if i % 2 else b"\n") for i in range(900)]
        src, f = [{"text": b"".join(recs)}], mk.MK_TEXT_FASTA
        heads = [[wf.strip(x[1:x.find(b"\n")]) for x in recs]]
    r = matcher.extract_window_frames(src, codec, fmt=f, logging=True)
    same_answers(r, matcher.extract_window(src, fmt=f, logging=True))
    assert len(r["rows"]) > 100
    for S, h in zip(r["sources"], heads):
        kept = [x for x, k in zip(h, r["keep"]) if k]
        assert S["n_members"] >= 1 and S["ids"] == b"".join(kept) and S["id_end"] == np.cumsum([len(x) for x in kept]).tolist()
    rank = np.cumsum(r["keep"]) - 1  # every row's record is a kept one: its id is found by the record's rank among the kept
    for file, rec, _, _ in r["rows"][:50]:
        S = r["sources"][file]
        q = int(rank[rec])
        assert r["keep"][rec] and S["ids"][(S["id_end"][q - 1] if q else 0):S["id_end"][q]] == heads[file][rec]


def test_text_below(mk, codec, checker, matcher):
    text = mixed_fastq(1200, seed=51)
    recs = [written_fastq(rec) for rec, k in zip(fastq_records(text), kept_of(1200)) if k]
    w = b"".join(recs)
    r = matcher.extract_window_frames([{"text": text}], codec, text_below=len(w) + 1)  # just above the written size: the text
    S = r["sources"][0]
    assert S["as_text"] and S["members"] == w and S["n_members"] == 0 and S["n_written"] == len(w) and S["n_kept"] == 400
    r = matcher.extract_window_frames([{"text": text}], codec, text_below=len(w))  # "shorter than": not this one
    check_frames(mk, checker, r["sources"][0], recs)
    r = matcher.extract_window_frames([{"text": text}], codec, text_below=len(w) - 1)
    check_frames(mk, checker, r["sources"][0], recs)


def _raw_call(mk, matcher, codec, text, caps, logging, text_below=0, invert=False, kept_buffer=False, expect_status=0):
    """the entry point itself with guarded outputs -> (rc, the mk_window_members, the buffers)"""
    L = mk.load()
    arr, hold, bound = matcher._window_sources([{"text": text}])
    cap = bound // 8 + 2
    bufs = {"members": HostBuf(np.uint8, caps["members"]), "ids": HostBuf(np.uint8, caps["ids"]), "id_end": HostBuf(np.uint64, cap),
            "rec_start": HostBuf(np.uint64, cap + 1), "keep": HostBuf(np.uint8, cap), "tail": HostBuf(np.uint8, 64), "kept": HostBuf(np.uint8, 64)}
    arr[0].rec_start, arr[0].tail, arr[0].tail_cap = bufs["rec_start"].ptr, bufs["tail"].ptr, 64
    if kept_buffer:
        arr[0].kept, arr[0].kept_cap = bufs["kept"].ptr, 64
    Mm = (mk.WindowMembers * 1)()
    Mm[0].members, Mm[0].members_cap, Mm[0].ids, Mm[0].ids_cap = bufs["members"].ptr, caps["members"], bufs["ids"].ptr, caps["ids"]
    Mm[0].id_end, Mm[0].text_below = bufs["id_end"].ptr, text_below
    rows = np.zeros(1 << 16, dtype=mk.ROW_DTYPE)
    n_rec, status, n_rows, c2, k2 = C.c_uint64(), C.c_uint32(), C.c_uint64(), mk.Counters(), np.zeros(len(matcher.patterns), dtype=np.uint32)
    rc = L.mk_extract_window_frames(matcher._h, codec._h if codec else None, mk.MK_TEXT_FASTQ, 1, arr, Mm, int(logging), int(invert), cap, C.byref(n_rec),
                                    bufs["keep"].ptr, rows.ctypes.data, len(rows), C.byref(n_rows), C.byref(c2), k2.ctypes.data, C.byref(status))
    assert status.value == expect_status
    return rc, Mm[0], bufs


@pytest.mark.parametrize("text_below", [0, 1 << 30])
def test_capacity_exact_fit_one_short_and_guards(mk, codec, matcher, text_below):
    text = mixed_fastq(1500, seed=61)
    rc, Mm, bufs = _raw_call(mk, matcher, codec, text, {"members": 1 << 20, "ids": 1 << 16}, True, text_below)
    assert rc == mk.MK_OK and Mm.n_member_bytes > 1000 and Mm.n_id_bytes > 1000 and Mm.n_kept == 500 and bool(Mm.as_text) == bool(text_below)
    need = {"members": int(Mm.n_member_bytes), "ids": int(Mm.n_id_bytes)}
    want = {k: bufs[k].view(need[k]).tobytes() for k in need}
    id_end = bufs["id_end"].view(500).tolist()
    assert bufs["members"].untouched_from(need["members"]) and bufs["ids"].untouched_from(need["ids"]) and bufs["id_end"].untouched_from(500)
    rc, Mm, bufs = _raw_call(mk, matcher, codec, text, need, True, text_below)  # exact fit
    assert rc == mk.MK_OK and {k: bufs[k].view(need[k]).tobytes() for k in need} == want and bufs["id_end"].view(500).tolist() == id_end
    assert all(b.guard_intact() for b in bufs.values())
    for short in ("members", "ids", "both"):
        caps = {k: need[k] - (1 if short in (k, "both") else 0) for k in need}
        rc, Mm, bufs = _raw_call(mk, matcher, codec, text, caps, True, text_below)
        assert rc == mk.MK_E_CAPACITY, short
        err = mk.load().mk_last_error()
        if short != "ids":
            assert Mm.n_member_bytes == need["members"]
        if short != "members":
            assert Mm.n_id_bytes == need["ids"] and str(need["ids"]).encode() in err
        else:
            assert str(need["members"]).encode() in err
        for k in need:
            assert bufs[k].guard_intact() and bufs[k].untouched_from(caps[k]), (short, k)
        assert all(b.guard_intact() for b in bufs.values())
    rc, Mm, bufs = _raw_call(mk, matcher, codec, text, need, True, text_below)  # the handles afterwards
    assert rc == mk.MK_OK and {k: bufs[k].view(need[k]).tobytes() for k in need} == want


def test_refused_arguments(mk, codec, matcher):
    text = mixed_fastq(40, seed=71)
    caps = {"members": 1 << 16, "ids": 1 << 12}
    L = mk.load()
    rc, _, bufs = _raw_call(mk, matcher, codec, text, caps, True, invert=True)  # logging with invert
    assert rc == mk.MK_E_INVALID_ARG and b"invert" in L.mk_last_error() and all(b.untouched_from(0) for b in bufs.values())
    rc, _, bufs = _raw_call(mk, matcher, None, text, caps, False)  # no codec
    assert rc == mk.MK_E_INVALID_ARG and b"codec" in L.mk_last_error() and all(b.untouched_from(0) for b in bufs.values())
    rc, _, bufs = _raw_call(mk, matcher, codec, text, caps, False, kept_buffer=True)  # a kept buffer in a source
    assert rc == mk.MK_E_INVALID_ARG and b"kept" in L.mk_last_error() and all(b.untouched_from(0) for b in bufs.values())
    with pytest.raises(mk.MerkurioError) as e:
        matcher.extract_window_frames([{"text": text}], None)
    assert e.value.code == mk.MK_E_INVALID_ARG
    if mk.device_count() > 1:  # a codec on another device
        other = mk.Codec(1)
        rc, _, bufs = _raw_call(mk, matcher, other, text, caps, False)
        other.close()
        assert rc == mk.MK_E_INVALID_ARG and b"different devices" in L.mk_last_error()
    rc, Mm, _ = _raw_call(mk, matcher, codec, text, caps, False)  # the handles afterwards
    assert rc == mk.MK_OK and Mm.n_members == 1


def test_an_open_stream_on_the_codec_handle_is_refused(mk, matcher):
    import zstd_cases as zc
    text = mixed_fastq(40, seed=73)
    c = mk.Codec()
    zs = np.frombuffer(zc.compress(text * 50), dtype=np.uint8)  # (the caller's until the stream ends)
    taken = C.c_uint32(0)
    L = mk.load()
    assert L.mk_zstd_stream_begin(c._h, zs.ctypes.data, zs.size, 0, C.byref(taken)) == mk.MK_OK and taken.value == 1
    rc, _, bufs = _raw_call(mk, matcher, c, text, {"members": 1 << 16, "ids": 1 << 12}, False)
    assert rc == mk.MK_E_INVALID_ARG and b"open stream" in L.mk_last_error() and all(b.untouched_from(0) for b in bufs.values())
    assert L.mk_zstd_stream_end(c._h) == mk.MK_OK
    rc, Mm, _ = _raw_call(mk, matcher, c, text, {"members": 1 << 16, "ids": 1 << 12}, False)
    assert rc == mk.MK_OK and Mm.n_members == 1
    c.close()
