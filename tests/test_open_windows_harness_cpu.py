"""The seam and ordering logic of `merkurio extract --open-windows` (cli/extract_windows.cpp: the reader that does not wait for tails and
stays at most N + 2 windows ahead of the writer, device threads that live until the writer has ended, seams and re-runs sent to the
front of a device's queue, the tail hand-off from the writer to a chained reader, the rule that chains the rest of the file after 4
disproved windows in a row) WITHOUT a GPU: tests/helpers/open_windows_harness.cpp, built with ASan + UBSan, drives prepare + run over
a bgzip'ed FASTQ of 13 windows with stubs in the library's place that NAME the guesses -- all true, all false, a mix -- on 1, 2 and 3
handles, with windows finishing out of order; an error in a late window; a seam call that fails."""
import os
import random
import re
import struct
import subprocess
import zlib

import pytest

from cli_sources import reader_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _bgzf(data, block=20000):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out) + EOF_MEMBER


def _records(n, seed=3):
    """header lines begin "@r", quality lines "@F", sequences '+', the '+' line repeats the id: a quality line has the record shape"""
    rnd = random.Random(seed)
    recs = []
    for i in range(n):
        L = rnd.choice((100, 150, 151))
        recs.append((b"r%07d" % i, b"+" + bytes(rnd.choice(b"ACGT") for _ in range(L)), b"@" + b"F" * L))
    return recs


def _text(recs):
    return b"".join(b"@" + i + b"\n" + s + b"\n+" + i + b"\n" + q + b"\n" for i, s, q in recs)


def _expected(recs, name):
    kept = [r for r in recs if r[1][1:2] == b"A"]
    return b"".join(b"@" + i + b"\n" + s + b"\n+\n" + q + b"\n" for i, s, q in kept), b"".join(b"%s\t%s\tACGT\t0\n" % (name, i) for i, _, _ in kept)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("ow")
    cli_dir = os.path.join(ROOT, "merkurio_amd/csrc/cli")
    exe = str(d / "open_windows_harness")
    stages = [os.path.join(cli_dir, f + ".cpp") for f in ("extract_windows", "extract_sources", "extract_window_call", "extract_write")]
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-w", "-I", cli_dir, "-o", exe, os.path.join(ROOT, "tests/helpers/open_windows_harness.cpp"),
                    *stages, *reader_sources()], check=True)
    recs = _records(45000)  # 13.6 MB: 13 windows of 1 MiB
    (d / "in.fastq.gz").write_bytes(_bgzf(_text(recs)))
    return {"d": d, "exe": exe, "recs": recs}


def run(job, name, flags, handles=1, inp="in.fastq.gz", **env):
    d = job["d"]
    p = subprocess.run([job["exe"], str(d / name), str(handles), flags, str(d / inp)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MERKURIO_TIMING="1", **env))
    assert p.returncode in (0, 1), p.stdout[-2000:] + p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    m = re.search(r"extract --open-windows: (\d+) open windows, (\d+) seams, (\d+) re-runs", p.stderr)
    calls = [(f[1], int(f[3]), int(f[5])) for f in (ln.split() for ln in p.stdout.split("\n")) if f and f[0] == "#call"]
    out = open(d / (name + "_1.out"), "rb").read()
    log = open(d / (name + ".log"), "rb").read() if "l" in flags else b""
    return p.returncode, p.stdout, out, log, calls, tuple(int(x) for x in m.groups()) if m else None


def _log_rows(log):
    return b"".join(ln + b"\n" for ln in log.split(b"\n") if ln and not ln.startswith(b"#"))


def test_the_chain_without_the_flag_is_the_reference(job):
    rc, stdout, out, log, calls, row = run(job, "chain", "l")
    want, rows = _expected(job["recs"], b"in.fastq.gz")
    assert rc == 0 and row is None and out == want and _log_rows(log) == rows and "#records 45000" in stdout
    assert len(calls) >= 13 and all(k == "plain" for k, _, _ in calls) and all(h > 0 for _, h, _ in calls[1:])


@pytest.mark.parametrize("handles", [1, 2, 3])
@pytest.mark.parametrize("slow", [False, True])
def test_every_guess_true(job, handles, slow):
    rc, stdout, out, log, calls, row = run(job, "true_%d_%d" % (handles, slow), "ol", handles, OPEN_GUESS="true", **({"OPEN_SLOW": "1"} if slow else {}))
    want, rows = _expected(job["recs"], b"in.fastq.gz")
    assert rc == 0 and out == want and _log_rows(log) == rows and "#records 45000" in stdout
    n_open, seams, reruns = row
    assert n_open >= 12 and seams == n_open and reruns == 0
    assert sum(k == "open" for k, _, _ in calls) == n_open and sum(k == "seam" for k, _, _ in calls) == seams
    assert sum(k == "plain" for k, _, _ in calls) == 1  # window 0


@pytest.mark.parametrize("handles", [1, 3])
def test_every_guess_false_chains_the_file_after_four(job, handles):
    rc, stdout, out, log, calls, row = run(job, "false_%d" % handles, "ol", handles, OPEN_GUESS="false", OPEN_SLOW="1")
    want, rows = _expected(job["recs"], b"in.fastq.gz")
    assert rc == 0 and out == want and _log_rows(log) == rows and "#records 45000" in stdout
    n_open, seams, reruns = row
    # 4 disproved windows in a row switch the reader to the chain; it may have dealt out N + 1 more open windows by then
    assert 4 <= n_open <= 4 + handles + 1 and reruns == n_open and seams == n_open
    assert all(s != 0 for k, _, s in calls if k == "seam")  # every seam refused
    chained = [h for k, h, _ in calls if k == "plain" and h > 0]
    assert len(chained) >= 13 - 1 and len(chained) - reruns >= 13 - 1 - n_open > 0  # the re-runs, then the rest of the file


@pytest.mark.parametrize("handles", [1, 2])
def test_a_mix_of_true_and_false_guesses(job, handles):
    rc, stdout, out, log, calls, row = run(job, "mix_%d" % handles, "ol", handles, OPEN_GUESS="mix", OPEN_SLOW="1")
    want, rows = _expected(job["recs"], b"in.fastq.gz")
    assert rc == 0 and out == want and _log_rows(log) == rows and "#records 45000" in stdout
    n_open, seams, reruns = row
    # (the file's last window behind a false start is no whole records: the open call itself refuses it, no seam is sent)
    assert 0 < reruns < n_open and n_open - 1 <= seams <= n_open


def test_an_error_in_a_late_window_keeps_its_place(job):
    recs = list(job["recs"])
    i, s, q = recs[40000]
    recs[40000] = (i, s, q[:-7])  # a quality line seven bytes short
    (job["d"] / "bad.fastq.gz").write_bytes(_bgzf(_text(recs)))
    a = run(job, "bad_chain", "-", 1, "bad.fastq.gz")
    b = run(job, "bad_open", "o", 2, "bad.fastq.gz", OPEN_GUESS="true", OPEN_SLOW="1")
    err = lambda stdout: [ln for ln in stdout.split("\n") if ln.startswith("#error")]
    assert a[0] == 1 and b[0] == 1 and err(a[1]) == err(b[1]) and len(err(a[1])) == 1
    assert a[2] == b[2] and len(a[2]) > 1 << 20  # the same bytes in front of it


def test_a_seam_call_that_fails_ends_the_job(job):
    rc, stdout, out, log, calls, row = run(job, "fail", "o", 2, OPEN_GUESS="true", OPEN_FAIL_SEAM="3")
    assert rc == 1 and "#error" in stdout  # ... and every thread has ended: the harness returned
    want, _ = _expected(job["recs"], b"in.fastq.gz")
    assert want.startswith(out) and 0 < len(out) < len(want)
