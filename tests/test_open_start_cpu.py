"""mk_extract_window_open without a device: the start rule restated in Python (tests/open_start.py) names, on every crafted text of the
GPU tests, the start those tests expect, and the whole-file reference parser of tests/ingest_cases.py says whether that start begins a
record -- always on ordinary reads and on FASTA, not on the adversarial reads; the entry is declared, bound and exported and refuses
what only it refuses before it touches a handle or a device."""
import ctypes as C
import os
import random
import re

import pytest

import ingest_cases as ic
import open_start as osr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sweep_range(text, fmt, first_rec=2, n_rec=4):
    """every byte of the n_rec records (four, or five) first_rec .. first_rec + n_rec - 1, and the byte behind them"""
    rs = sorted(osr.record_starts(text, fmt))
    return range(rs[first_rec], rs[first_rec + n_rec] + 1)


@pytest.mark.parametrize("eol", [osr.LF, osr.CRLF])
@pytest.mark.parametrize("final_eol", [True, False])
@pytest.mark.parametrize("plus_id", [False, True])
def test_fastq_sweep_names_the_next_record_and_it_is_true(eol, final_eol, plus_id):
    text, seqs = osr.sweep_fastq(eol, final_eol, plus_id)
    assert 64 << 10 <= len(text) <= 100 << 10
    assert ic.parse_fastq(text, True)[2] == seqs
    true = sorted(osr.record_starts(text))
    cuts = osr.Cuts(text)
    rnd = random.Random(1)
    sweep = _sweep_range(text, "fastq")
    assert len(sweep) > 60
    for c in list(sweep) + [0, 1, len(text) - 1, len(text)] + [rnd.randrange(len(text)) for _ in range(40)]:
        named = osr.open_start(text[c:])
        assert (None if named is None else named[1]) == cuts.n_front(c)
        if named is None:  # only where fewer than two whole records follow the cut line
            assert sum(1 for t in true if t > c) < 3 + (not final_eol)
            continue
        # on these reads the named start is the first record start behind the cut -- behind, not at: line 0 is not taken
        assert c + named[1] == min(t for t in true if t > c)


@pytest.mark.parametrize("width", [0, 60, 80])
def test_fasta_sweep_names_the_next_header(width):
    text, seqs = osr.sweep_fasta(width)
    assert 64 << 10 <= len(text) <= 100 << 10
    assert ic.parse_fasta(text, True)[2] == seqs
    true = sorted(osr.record_starts(text, "fasta"))
    cuts = osr.Cuts(text, "fasta")
    sweep = _sweep_range(text, "fasta", 3, 5)
    assert {(c + cuts.n_front(c)) % 16 for c in range(0, len(text) - 2000)} == set(range(16))  # the start at every residue mod 16
    for c in list(sweep) + [0, len(text) - 1, len(text)]:
        named = osr.open_start(text[c:], "fasta")
        assert (None if named is None else named[1]) == cuts.n_front(c)
        later = [t for t in true if t > c]
        assert (named is None) == (not later) and (named is None or c + named[1] == later[0])


def test_edge_texts_put_the_start_where_their_names_say():
    for fmt in ("fastq", "fasta"):
        for at in osr.EDGE_BYTES:
            assert osr.open_start(osr.start_at_byte(at, fmt), fmt) == (1, at)
        for line in osr.EDGE_LINES:
            text = osr.start_at_line(line, fmt)
            assert osr.open_start(text, fmt) == (line, 3 * line)
    text = osr.one_shape_alone()
    start = osr.line_starts(text)
    assert osr.fq_shape(text, start, 1) and not osr.fq_shape(text, start, 5)
    assert osr.open_start(text) == (8, start[8])
    # line 0 is not taken, whatever it starts with
    body = osr.body_fastq()
    assert body[:1] == b"@" and osr.open_start(body) == (4, sorted(osr.record_starts(body))[1])
    fa = osr.body_fasta()
    assert fa[:1] == b">" and osr.open_start(fa, "fasta")[1] == sorted(osr.record_starts(fa, "fasta"))[1]


def test_status_2_texts_have_no_start():
    body = osr.body_fastq()
    start = osr.line_starts(body)
    # nine complete lines at the least: line 0 and two shapes behind it
    assert osr.open_start(b"III\n" + body[:start[8]]) == (1, 4)
    assert osr.open_start(b"III\n" + body[:start[8] - 1]) is None  # the ninth is not complete
    assert osr.open_start(body[:start[8]]) is None                 # eight complete lines
    assert osr.open_start(body[:start[12]]) == (4, start[4]) and osr.open_start(body[:start[12] - 1]) is None
    assert osr.open_start(b">x\n" + b"ACGT\n" * 1000 + b"ACG", "fasta") is None  # line 0 is the only header
    assert osr.open_start(b"ACGT\n" * 1000, "fasta") is None
    assert osr.open_start(b"") is None and osr.open_start(b"", "fasta") is None


def test_adversarial_reads_name_false_starts():
    text, seqs = osr.adversarial()
    assert ic.parse_fastq(text, True)[2] == seqs
    true = osr.record_starts(text)
    cuts = osr.Cuts(text)
    named = {c: cuts.n_front(c) for c in range(len(text) + 1)}
    false = [c for c, f in named.items() if f is not None and c + f not in true]
    right = [c for c, f in named.items() if f is not None and c + f in true]
    assert len(false) > len(right) > 50  # three lines of four lead to a false start
    for c in false[::7] + right[::7]:
        assert osr.open_start(text[c:])[1] == named[c]
    # a false start is the quality line of a record: three lines behind a true one
    start = osr.line_starts(text)
    assert all(start.index(c + named[c]) % 4 == 3 for c in false)


def test_the_entry_is_declared_bound_and_exported():
    from merkurio_amd import native
    header = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"\bint mk_extract_window_open\(", header) and "typedef struct mk_window_front" in header
    assert "mk_extract_window_open" in native.EXPORTS
    L = native.load()
    assert L.mk_extract_window_open.argtypes[:-1] == L.mk_extract_window.argtypes
    assert [f[0] for f in native.WindowFront._fields_] == ["front", "front_cap", "n_front"] and C.sizeof(native.WindowFront) == 24
    weak = open(os.path.join(ROOT, "merkurio_amd", "csrc", "cli", "device_abi_weak.hpp")).read()
    assert "mk_extract_window_open" in weak


def test_two_sources_or_a_head_are_refused_before_any_device_use():
    from merkurio_amd import native
    L = native.load()
    text = osr.body_fastq()
    buf = C.create_string_buffer(text, len(text))
    head = C.create_string_buffer(b"@h\n", 3)

    def call(n_sources, n_head, front=True):
        arr = (native.WindowSource * 2)()
        for S in arr:
            S.text, S.n_text = C.addressof(buf), len(text)
        arr[0].head, arr[0].n_head = (C.addressof(head) if n_head else None), n_head
        F = native.WindowFront()
        n_rec, n_rows, status = C.c_uint64(), C.c_uint64(), C.c_uint32()
        cnt = native.Counters()
        # (no matcher handle: a call that got past its own checks would answer "null argument")
        rc = L.mk_extract_window_open(None, None, 0, n_sources, arr, 0, 0, 0, C.byref(n_rec), None, None, 0, C.byref(n_rows), C.byref(cnt), None,
                                      C.byref(status), C.addressof(F) if front else None)
        return rc, L.mk_last_error().decode()

    rc, msg = call(2, 0)
    assert rc == native.MK_E_INVALID_ARG and "one source" in msg
    rc, msg = call(1, 3)
    assert rc == native.MK_E_INVALID_ARG and "no head" in msg
    rc, msg = call(1, 0, front=False)
    assert rc == native.MK_E_INVALID_ARG and "null argument" in msg
    rc, msg = call(1, 0)  # nothing of its own to refuse: the shared body's first check speaks
    assert rc == native.MK_E_INVALID_ARG and "null argument" in msg


def test_the_flag_parses_alongside_the_others():
    import subprocess
    from merkurio_amd import build
    exe = build.build_cli()
    h = subprocess.run([exe, "extract", "--help"], capture_output=True)
    assert h.returncode == 0 and b"--open-windows" in h.stdout + h.stderr
    # every other flag of `extract`, in groups whose members the parser lets stand together (-S excludes -o, -z and --zstd-output)
    groups = [[], ["-r", "-v", "--gpus", "2", "--window-mb", "1", "--batch-mb", "64", "--gzip-window", "1000000", "--bzip2-window", "1000000"],
              ["-r", "-z", "--z-members-from", "0", "--host-codec"], ["--host-ingest", "-a"], ["--zstd-output"],
              ["--device-zstd", "--zstd-stream", "--zstd-window", "1000", "--device-xz", "--xz-stream", "--xz-window", "1000", "--xz-spread", "9", "--xz-text-cap", "0"]]
    for flags in groups:
        p = subprocess.run([exe, "extract", "--open-windows", *flags, "-i", "/nonexistent/in.fastq", "-s", "ACGT", "-o", "/nonexistent/out"], capture_output=True)
        assert p.returncode != 2 and b"open-windows" not in p.stderr, p.stderr  # (2: the parser's own refusal)
    p = subprocess.run([exe, "extract", "--open-windows", "-S", "-i", "/nonexistent/in.fastq", "-s", "ACGT", "-j", "/nonexistent/x.json"], capture_output=True)
    assert p.returncode != 2 and b"open-windows" not in p.stderr, p.stderr
    p = subprocess.run([exe, "extract", "--open-windows=1", "-i", "x", "-s", "ACGT"], capture_output=True)
    assert p.returncode == 2  # the flag takes no value
