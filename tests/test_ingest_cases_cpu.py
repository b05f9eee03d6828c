"""Every text of tests/ingest_cases.py before a kernel sees it: it places what its builder says it places (the claims are computed
from the text), it means under the reference parser what the GPU test expects (status 0, or 1 for the refusal cases), the reference
parsers agree with the oracle and the golden logs on the reference's own FASTQ / FASTA inputs and with _parse_fasta of
test_gpu_windows.py on the crafted FASTA texts, and the helper that rebuilds sequences from 4-mer log rows returns what a naive
search was given -- and not when one base differs."""
import os
import random

import numpy as np
import pytest

import ingest_cases as ic
import oracle_binding as ob


@pytest.mark.parametrize("name", ic.all_case_names())
def test_case_places_what_it_claims_and_means_what_is_expected(name):
    c = ic.case(name)
    status, rec_start, seqs = ic.reference(c)
    assert status == c.status
    if status:
        assert len(rec_start) == 0 and seqs == []
        return
    assert len(rec_start) == len(seqs) + 1 and int(rec_start[-1]) == len(c.text)
    marker = b"@" if c.fmt == "fastq" else b">"
    assert all(c.text[int(a):int(a) + 1] == marker for a in rec_start[:-1])
    missing = c.required - c.claims
    assert not missing, sorted(missing)
    assert len(c.text) <= 48 * ic.BLOCK


@pytest.mark.parametrize("en", ["lf", "crlf"])
def test_edge_texts_cover_every_combination(en):
    eol = ic.EOLS[en]
    whats = 12 if en == "crlf" else 8
    for edge in ic.EDGES:
        c = ic.case(f"fq-edges-{edge}-{en}")
        assert len(c.required) == whats * 4 and c.required <= c.claims
        assert len(c.text) > edge * (whats + 2)
    # a CRLF split between two blocks, for every line of a record and for both kinds of FASTA line
    if en == "crlf":
        claims = ic.case("fq-edges-16384-crlf").claims
        assert {(w + "_cr", 16384, -1) for w in ic.LINES} <= claims and {(w + "_nl", 16384, 0) for w in ic.LINES} <= claims
        claims = ic.case("fa-edges-crlf").claims
        assert {("hdr_cr", 16384, -1), ("hdr_nl", 16384, 0), ("seq_cr", 16384, -1), ("seq_nl", 16384, 0)} <= claims
    assert ic.fasta_required(eol) <= ic.case(f"fa-edges-{en}").claims


def test_length_count_and_shape_cases_are_what_their_names_say():
    for en, eol in ic.EOLS.items():
        for fmt, lengths in (("fq", ic.LENGTHS), ("fa", ic.FA_LENGTHS)):
            for n in lengths:
                for fe in (True, False):
                    c = ic.case(f"{fmt}-length-{n}-{'eol' if fe else 'noeol'}-{en}")
                    assert len(c.text) == n and c.text.endswith(eol) == fe and (fe or c.text[-1:] not in b"\r\n")
        assert {n % 64 for n in ic.LENGTHS} >= {0, 1, 63} and {16383, 16384, 16385, 32768} <= set(ic.LENGTHS)
        assert ic.length_phases(ic.case(f"fq-every-length-{en}").text) == {(L, p) for L in range(201) for p in range(4)}
        seqs = ic.reference(ic.case(f"fq-all-empty-{en}"))[2]
        assert len(seqs) >= 2000 and set(seqs) == {b""}
        # dense and sparse blocks: some thread has 36 newlines (LF) and somewhere two blocks in a row have none
        text = ic.case(f"fq-dense-sparse-{en}").text
        nl = np.frombuffer(text, dtype=np.uint8) == 10
        per_thread = np.add.reduceat(nl, np.arange(0, len(nl), 64))
        per_block = np.add.reduceat(nl, np.arange(0, len(nl), ic.BLOCK))
        assert per_thread.max() >= (36 if en == "lf" else 23)
        assert any(per_block[k] == per_block[k + 1] == 0 for k in range(len(per_block) - 1))
        assert len(ic.reference(ic.case(f"fa-counts-8193-{en}"))[2]) == 8193
    for n in ic.COUNTS:
        for kind in ("var", "fixed"):
            seqs = ic.reference(ic.case(f"fq-count-{n}-{kind}-lf"))[2]
            assert len(seqs) == n
            assert ({len(s) for s in seqs} == {37}) == (kind == "fixed")
    assert set(ic.COUNTS) == {1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8193}
    for L in ic.FIXED_LENGTHS:
        for en in ic.EOLS:
            text = ic.case(f"fq-fixed-{L}-{en}").text
            assert {ln for ln, _ in ic.length_phases(text)} == {L} and {p for _, p in ic.length_phases(text)} == {0, 1, 2, 3}
    assert any(ic.flags_k3(ic.reference(ic.case("fq-fixed-3-lf"))[2])) and not all(ic.flags_k3(ic.reference(ic.case("fq-fixed-3-lf"))[2]))


def test_refusals_spoil_the_record_they_name():
    for en, eol in ic.EOLS.items():
        good = ic.fq_refusal("none", "255", eol)
        assert ic.parse_fastq(good)[0] == 0
        for kind in ic.REFUSALS:
            for place in ic.REFUSAL_PLACES:
                text = ic.case(f"fq-refuse-{kind}-{place}-{en}").text
                assert ic.parse_fastq(text)[0] == 1
                # whole records in front of the spoilt one are fine; with it they are not
                cut = {"255": 255, "256": 256, "last": 299}.get(place)
                starts = ic.parse_fastq(good)[1]
                if cut is None:
                    cut = int(np.searchsorted(starts, ic.BLOCK, side="right")) - 1
                    assert starts[cut] < ic.BLOCK < starts[cut + 1]
                assert ic.parse_fastq(text[:int(starts[cut])])[0] == 0
                nxt = text.find(b"@r%d" % (cut + 1) + eol) if cut < 299 else len(text)
                assert ic.parse_fastq(text[:nxt])[0] == 1
    # what else the rule refuses or takes
    assert ic.parse_fastq(b"@a\nAC\n+\nII\n")[0] == 0 and ic.parse_fastq(b"@a\nAC\n+a\nII")[0] == 0
    assert ic.parse_fastq(b"@a\r\nAC\r\n+\r\nII\r\n")[2] == [b"AC"]
    assert ic.parse_fastq(b"@\r\nAC\r\n+\r\nII\r\n")[2] == [b"AC"]  # (an empty id: taken; "@\n" has no id at all)
    for bad in (b"@\nAC\n+\nII\n", b"@\nAC\r\n+\r\nII\r\n", b"@a\nAC\n\n+\nII\n", b"@a\nAC\n+\nII\n\n", b"@a\nAC\n+\nI\n", b">a\nAC\n", b"@a\nAC\n+\n"):
        assert ic.parse_fastq(bad)[0] == 1, bad


def test_window_cuts_of_the_reference_parser():
    for eol in (ic.LF, ic.CRLF):
        text = ic.fq_three_records(eol)
        status, starts, seqs = ic.parse_fastq(text)
        assert status == 0 and len(seqs) == 3
        for cut in range(len(text) + 1):
            st, rs, sq = ic.parse_fastq(text[:cut], ends_at_record=False)
            whole = sum(1 for z in starts[1:] if z <= cut)
            assert st == 0 and len(sq) == whole and sq == seqs[:whole] and int(rs[-1]) == int(starts[whole])
        st, rs, sq = ic.parse_fasta(b">a\nAC\n>b\nG", ends_at_record=False)
        assert (st, rs.tolist(), sq) == (0, [0, 6], [b"AC"])


def _parse_fasta_windows(text):
    """tests/test_gpu_windows.py::_parse_fasta, word for word (that module is GPU-marked as a whole and is not imported here)"""
    starts, ids, seqs = [], [], []
    pos = 0
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            starts.append(pos)
            ids.append(line[1:].rstrip(b"\r"))
            seqs.append(bytearray())
        elif seqs:
            seqs[-1] += line.replace(b"\r", b"")
        pos += len(line) + 1
    return starts, ids, [bytes(s) for s in seqs]


@pytest.mark.parametrize("name", ic.all_case_names("fa-"))
def test_fasta_parser_agrees_with_the_window_tests_parser(name):
    c = ic.case(name)
    status, rec_start, seqs = ic.reference(c)
    starts, _, seqs2 = _parse_fasta_windows(c.text)
    assert status == 0 and rec_start.tolist() == starts + [len(c.text)] and seqs == seqs2


def _log_rows(path):
    rows = []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln and not ln.startswith(b"#"):
            f, r, p, pos = ln.split(b"\t")
            rows.append((f, r, p, int(pos)))
    return rows


def _ids(text, rec_start, marker_len=1):
    return [text[int(a) + marker_len:].split(b"\n", 1)[0].rstrip(b"\r") for a in rec_start[:-1]]


def test_reference_parsers_agree_with_the_oracle_on_the_golden_inputs(golden):
    fx = os.path.join(golden, "fixtures")
    # FASTA: simple.fasta (-r -s ACG) and fixed-width.faa (DKAT across a line break): the oracle's loop on the parser's sequences
    # gives the rows of the reference's logs
    for name, kmers, rc in (("simple.fasta", [b"ACG"], True), ("fixed-width.faa", [b"DKAT"], False)):
        text = open(os.path.join(fx, "input", name), "rb").read()
        status, rec_start, seqs = ic.parse_fasta(text)
        assert status == 0 and int(rec_start[-1]) == len(text)
        _, patterns = ob.parse_pattern_list(kmers, reverse_complement=rc)
        om = ob.Matcher(patterns, ob.select_aho_corasick(False, False, False, patterns), 0, False)
        _, rows, _ = ob.extract_single(om, seqs, logging=True)
        ids = _ids(text, rec_start)
        got = [(name.encode(), ids[rec], patterns[pat], pos) for _, rec, pat, pos in rows]
        assert got == _log_rows(os.path.join(fx, "extract", name.rsplit(".", 1)[0] + ".log")) and got
    # paired FASTQ, -s CTT
    texts = [open(os.path.join(fx, f"input/paired-{k}.fastq"), "rb").read() for k in (1, 2)]
    parsed = [ic.parse_fastq(t) for t in texts]
    assert all(p[0] == 0 and int(p[1][-1]) == len(t) for p, t in zip(parsed, texts))
    _, patterns = ob.parse_pattern_list([b"CTT"])
    om = ob.Matcher(patterns, ob.select_aho_corasick(False, False, False, patterns), 0, False)
    _, rows, c = ob.extract_paired(om, parsed[0][2], parsed[1][2], logging=True)
    ids = [_ids(t, p[1]) for p, t in zip(parsed, texts)]
    got = [(b"paired-%d.fastq" % (f + 1), ids[f][rec], patterns[pat], pos) for f, rec, pat, pos in rows]
    assert got == _log_rows(os.path.join(fx, "extract/paired.log")) and got
    assert c["records"] == 4 and c["bases"] == 32


def test_rows_of_all_4mers_spell_the_sequences():
    rnd = random.Random(1)
    pats = ic.kmers4()
    assert len(pats) == 256 and len(set(pats)) == 256
    seqs = [bytes(rnd.choice(b"ACGT") for _ in range(L)) for L in (0, 1, 3, 4, 5, 8, 70, 200, 4, 0, 1000)]
    rec, pat, pos = ic.naive_rows(seqs, pats)
    assert ic.rebuild_sequences(rec, pat, pos, pats, len(seqs)) == ic.spelled(seqs)
    order = np.random.default_rng(0).permutation(len(rec))  # the order of the rows does not matter
    assert ic.rebuild_sequences(rec[order], pat[order], pos[order], pats, len(seqs)) == ic.spelled(seqs)
    # one base changed, anywhere: the rows spell another text
    for r, k in ((3, 0), (3, 3), (6, 69), (7, 100), (10, 999), (5, 4)):
        other = list(seqs)
        s = bytearray(other[r])
        s[k] = ord("A") if s[k] != ord("A") else ord("C")
        other[r] = bytes(s)
        rec2, pat2, pos2 = ic.naive_rows(other, pats)
        assert ic.rebuild_sequences(rec2, pat2, pos2, pats, len(seqs)) != ic.spelled(seqs)
    # rows that do not fit together are no sequence at all: one row dropped, one pattern swapped
    with pytest.raises(AssertionError):
        ic.rebuild_sequences(rec[:-3], pat[:-3], np.concatenate((pos[:-4], pos[-3:-2])), pats, len(seqs))
    swapped = pat.copy()
    swapped[len(pat) // 2] ^= 0x55
    with pytest.raises(AssertionError):
        ic.rebuild_sequences(rec, swapped, pos, pats, len(seqs))


def test_big_case_is_built_as_described():
    text, rec_start, which = ic.big_small_reads()
    n = ic.BIG_RECORDS
    assert n == 4_194_304 + 4097 and len(which) == n and len(rec_start) == n + 1 and int(rec_start[-1]) == len(text)
    assert 40e6 <= len(text) <= 56e6 and len(text) > 1024 * ic.BLOCK
    assert all(which[k] == 2 for k in (4_194_303, 4_194_304, 4_194_305, n - 1))
    # uneven newline counts per block; the first and the last 3000 records parse to the reads they were built from
    per_block = np.add.reduceat(text == 10, np.arange(0, len(text), ic.BLOCK))
    assert len(np.unique(per_block[:-1])) > 10
    for lo, hi in ((0, 3000), (n - 3000, n)):
        part = text[int(rec_start[lo]):int(rec_start[hi])].tobytes()
        status, rs, seqs = ic.parse_fastq(part)
        assert status == 0 and np.array_equal(rs + rec_start[lo], rec_start[lo:hi + 1])
        assert seqs == [ic.SMALL_READS[k] for k in which[lo:hi]]
    # ... and all of it to the record table (the parser's tables are numpy: no Python loop over 4 M records)
    status, s, e, _, end = ic.fastq_lines(text)
    assert status == 0 and end == len(text) and np.array_equal(s[:, 0].astype(np.uint64), rec_start[:-1])
    assert np.array_equal(e[:, 1] - s[:, 1], np.array([len(r) for r in ic.SMALL_READS])[which])
