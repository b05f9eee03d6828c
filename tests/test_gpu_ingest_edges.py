"""The ingest kernels (merkurio_amd/csrc/ingest.hip: line table, record table, offset scans, gather, FASTA compaction) at the edges
of their shares -- a thread's 64 bytes, a wave's 4096, a block's 16 KiB, 16 / 256 / 4096 records, 1024 blocks and 1024 tiles per
round -- on the crafted texts of tests/ingest_cases.py, whose placement claims tests/test_ingest_cases_cpu.py proves from the texts.

What the device made of a text is read through the ABI alone: the whole record table is compared with the reference parser's, and
the gathered sequences are spelled back byte for byte from the log rows of a matcher over all 256 4-mers (a wrong, missing or
shifted byte changes a row); reads below four bases and the 4.2 M-record text are checked through the flags of the one 3-mer ACG
on reads that make it only across record boundaries.  Every FASTQ text runs through mk_extract_fastq_text and mk_extract_window,
FASTA through mk_extract_window; rows and counters must equal mk_extract_single on the parser's sequences and the kept text the
stored bytes of the kept records.  No expectation comes from the code under test."""
import time

import numpy as np
import pytest

import ingest_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def matchers(mk):
    """all 256 4-mers (rows spell the sequences); the 3-mer of the small reads; patterns across a '>' inside a sequence"""
    return {"k4": mk.Matcher(ic.kmers4()), "k3": mk.Matcher([ic.K3]), "gt": mk.Matcher([b"C>G", b"ACG", b"TAC>"])}


def _paths(mk, c):
    """the entry points a case runs through: name -> call(matcher, **kw)"""
    out = {}
    if c.fmt == "fastq":
        out["fastq_text"] = lambda m, **kw: ic.run_fastq_text(mk, m, c.text, **kw)
    out["window"] = lambda m, **kw: ic.run_window(mk, m, c.text, fmt=c.fmt, **kw)
    return out


def _stored(text, rec_start, keep):
    a = rec_start.tolist()
    return b"".join(text[a[i]:a[i + 1]] for i in np.flatnonzero(keep).tolist())


def _check_case(mk, matchers, c, rows_matcher="k4"):
    status, ref_start, seqs = ic.reference(c)
    assert status == 0
    m4, m3 = matchers[rows_matcher], matchers["k3"]
    n = len(seqs)
    keep_x, rows_x, counters_x = m4.extract_single(seqs, logging=True) if n else ([], [], None)
    flags3 = ic.flags_k3(seqs)
    for name, run in _paths(mk, c).items():
        r = run(m4, logging=True)
        assert r["status"] == 0 and r["n_rec"] == n, name
        assert np.array_equal(r["rec_start"], ref_start), name
        rows = r["rows"]
        if rows_matcher == "k4":
            assert ic.rebuild_sequences(rows["rec"], rows["pat"], rows["pos"], m4.patterns, n) == ic.spelled(seqs), name
        if n:
            assert ic.rows_list(rows) == rows_x and r["counters"] == counters_x and r["keep"].tolist() == keep_x, name
            assert r["counters"]["bases"] == sum(len(s) for s in seqs) and r["counters"]["records"] == n
        # the flags of the 3-mer: they see reads below four bases and any byte that went to a neighbour
        r = run(m3, logging=False)
        assert r["status"] == 0 and np.array_equal(r["rec_start"], ref_start) and np.array_equal(r["keep"], flags3), name
    for invert in (False, True):
        r = ic.run_window(mk, m3, c.text, fmt=c.fmt, logging=False, invert=invert, want=("kept", "tail"))
        assert r["status"] == 0 and np.array_equal(r["keep"], flags3 != invert) and r["tail"] == b"" and r["n_used"] == len(c.text)
        assert r["kept"].tobytes() == _stored(c.text, ref_start, flags3 != invert)


FQ_GENERAL = [n for n in ic.all_case_names("fq-") if not n.startswith("fq-refuse-")]
FA_GENERAL = [n for n in ic.all_case_names("fa-") if not n.startswith("fa-content-")]


@pytest.mark.parametrize("name", FQ_GENERAL)
def test_fastq_case(mk, matchers, name):
    """edges, dense and sparse blocks, text lengths, record counts, every read length, fixed lengths, all reads empty"""
    _check_case(mk, matchers, ic.case(name))


@pytest.mark.parametrize("name", FA_GENERAL)
def test_fasta_case(mk, matchers, name):
    """edges, closing entries at chosen text lengths, 8193 one-line records, the texts '>', '>a', '>a\\n'"""
    _check_case(mk, matchers, ic.case(name))


@pytest.mark.parametrize("en", ["lf", "crlf"])
def test_fasta_content(mk, matchers, en):
    """'>' inside a header and in the middle of a sequence line (sequence: patterns span it), a blank line inside a record, records
    without sequence"""
    c = ic.case(f"fa-content-{en}")
    seqs = ic.reference(c)[2]
    assert seqs == [b"ACGTAC>GATTACC", b"", b"ACGTAC>GA", b"", b"AC>GAC>G"]
    _check_case(mk, matchers, c, rows_matcher="gt")
    r = ic.run_window(mk, matchers["gt"], c.text, fmt="fasta")
    assert sorted(set(r["rows"]["pat"].tolist())) == [0, 1, 2] and r["keep"].tolist() == [True, False, True, False, True]


@pytest.mark.parametrize("en", ["lf", "crlf"])
def test_all_reads_empty(mk, matchers, en):
    """W.fixed stays 0, the sequences take 0 bytes and nothing is scanned: nothing kept, an empty kept text, everything under invert"""
    c = ic.case(f"fq-all-empty-{en}")
    n = len(ic.reference(c)[2])
    for m in matchers.values():
        for logging in (True, False):
            counters = m.extract_single([b""] * n, logging=logging)[2]  # (records are counted by the logging loop alone)
            assert counters["records"] == (n if logging else 0)
            for r in (ic.run_fastq_text(mk, m, c.text, logging=logging), ic.run_window(mk, m, c.text, logging=logging, want=("kept",))):
                assert r["status"] == 0 and r["n_rec"] == n and not r["keep"].any() and len(r["rows"]) == 0
                assert r["counters"] == counters and r["counters"]["bases"] == 0 and r["counters"]["extracted"] == 0
                assert r.get("kept") is None or len(r["kept"]) == 0
            r = ic.run_window(mk, m, c.text, logging=logging, invert=True, want=("kept",))
            assert r["status"] == 0 and r["keep"].all() and r["kept"].tobytes() == c.text and r["counters"]["extracted"] == n


@pytest.mark.parametrize("en", ["lf", "crlf"])
@pytest.mark.parametrize("place", ic.REFUSAL_PLACES)
@pytest.mark.parametrize("kind", ic.REFUSALS)
def test_refusal(mk, matchers, kind, place, en):
    """one spoilt record -- in a lane block of its own (255, 256), the last, across a block edge: status 1 and no output"""
    c = ic.case(f"fq-refuse-{kind}-{place}-{en}")
    assert ic.reference(c)[0] == 1
    for run in _paths(mk, c).values():
        r = run(matchers["k4"], logging=True)
        assert r["status"] == 1 and r["n_rec"] == 0 and len(r["keep"]) == 0 and len(r["rows"]) == 0
    good = ic.fq_refusal("none", place, c.eol)
    assert ic.run_fastq_text(mk, matchers["k3"], good, logging=False)["status"] == 0
    if kind == "at_alone":  # "@\r\n" is not '@' alone: a header with an empty id, which the device takes
        taken = c.text.replace(b"@\n", b"@\r\n")
        ref = ic.parse_fastq(taken)
        r = ic.run_fastq_text(mk, matchers["k3"], taken, logging=False)
        assert ref[0] == 0 and r["status"] == 0 and np.array_equal(r["rec_start"], ref[1]) and np.array_equal(r["keep"], ic.flags_k3(ref[2]))


@pytest.mark.parametrize("en", ["lf", "crlf"])
def test_window_cut_at_every_byte(mk, matchers, en):
    """three records, every prefix with more text to follow: the whole 4-line records are taken, the rest is the tail (the cut
    between '\\r' and '\\n' included), and the tail as the head of the remaining text gives the other records"""
    m = matchers["k4"]
    text = ic.fq_three_records(ic.EOLS[en])
    _, starts, seqs = ic.parse_fastq(text)
    first = [m.extract_single(seqs[:k], logging=True) if k else None for k in range(4)]
    rest = [m.extract_single(seqs[k:], logging=True) if k < 3 else None for k in range(4)]
    seen = set()
    for cut in range(len(text) + 1):
        status, ref_start, ref_seqs = ic.parse_fastq(text[:cut], ends_at_record=False)
        k = len(ref_seqs)
        seen.add(k)
        r = ic.run_window(mk, m, text[:cut], ends_at_record=False, want=("tail",))
        assert r["status"] == 0 and r["n_rec"] == k and r["n_used"] == int(ref_start[-1]) and r["tail"] == text[r["n_used"]:cut], cut
        assert np.array_equal(r["rec_start"], ref_start), cut
        if k:
            assert (r["keep"].tolist(), ic.rows_list(r["rows"]), r["counters"]) == first[k], cut
        r2 = ic.run_window(mk, m, text[cut:], head=r["tail"])
        assert r2["status"] == 0 and r2["n_rec"] == 3 - k, cut
        assert np.array_equal(r2["rec_start"], starts[k:] - starts[k]), cut
        if k < 3:
            assert (r2["keep"].tolist(), ic.rows_list(r2["rows"]), r2["counters"]) == rest[k], cut
    assert seen == {0, 1, 2, 3}


def test_more_than_1024_tiles_and_blocks(mk, matchers):
    """4 194 304 + 4097 records of the reads AC, G, ACG, CGA (about 50 MB, 3000 blocks of uneven newline counts): the second round
    of the block scan and of the tile scan, tile 1024 and the closing entry behind it.  Only a read of ACG holds the 3-mer; its
    neighbours make it across every kind of record boundary, so a shifted offset flips flags.  Text and expectation are numpy's.
    Measured on an MI355X: 0.023 s for the mk_extract_fastq_text call, 0.042 s for mk_extract_window with the kept text, under 1 s
    for the whole test; both times are printed (run with -s)."""
    text, rec_start, which = ic.big_small_reads()
    m = matchers["k3"]
    flags = which == 2
    n = len(which)
    t0 = time.perf_counter()
    r = ic.run_fastq_text(mk, m, text, logging=False)
    t1 = time.perf_counter()
    assert r["status"] == 0 and r["n_rec"] == n
    assert np.array_equal(r["rec_start"], rec_start) and np.array_equal(r["keep"], flags)
    assert r["counters"]["extracted"] == int(flags.sum())
    t2 = time.perf_counter()
    r = ic.run_window(mk, m, text, logging=False, want=("kept",))
    t3 = time.perf_counter()
    print(f"\n{n} records, {len(text)} bytes: mk_extract_fastq_text {t1 - t0:.3f} s, mk_extract_window with kept text {t3 - t2:.3f} s")
    assert r["status"] == 0 and np.array_equal(r["rec_start"], rec_start) and np.array_equal(r["keep"], flags)
    # the kept text: the stored bytes of the reads of ACG (offsets of 4.2 M selected lengths: 1025 tiles again)
    assert np.array_equal(r["kept"], text[np.repeat(flags, np.diff(rec_start).astype(np.int64))])
