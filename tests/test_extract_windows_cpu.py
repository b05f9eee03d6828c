"""The window pipeline of `merkurio extract` (cli/extract_windows.cpp with its sources, window call and writer) WITHOUT a GPU:
tests/helpers/extract_windows_harness.cpp drives WindowExtract::prepare + run over windows of 1 MiB with a stub in the library's place
that indexes a window with the host parser and keeps a record by a rule on its id alone (the byte sum of the id is divisible by 3; a
pair when either mate's is; -v flips it; one log row per kept record and source).  The expectation is computed here from the input
text: records split by the plain 4-line / header-line rule, the id rule applied, written the way the reference writes them.  Windows
the stub refuses reach the host parser's path, whose stub sees sequences only and keeps a record whose first base is 'A': the inputs
made here give exactly the records whose id hits such a sequence.  MERKURIO_TEST_SANITIZE=1 builds the harness with ASan + UBSan; the
program is run directly."""
import gzip
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cli_sources import reader_sources
from tag_windows import EOF, _bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FLAGS = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
          if os.environ.get("MERKURIO_TEST_SANITIZE") else ["-O1"])
MIB = 1 << 20
E_FILE2_SHORT = "Error during FASTQ record parsing of second file. Do the two input files contain the same number of records?"
E_FILE2_LONG = "The two input files have a different number of records. Please provide valid paired-end read files."


def hits(rid):
    return sum(rid.encode()) % 3 == 0


def fastq_records(rnd, total=0, lens=(50, 300), ident=lambda i: "r%d" % i, count=None):
    """-> [(id, sequence, quality)] of about `total` bytes of FASTQ, or `count` records; a record's sequence starts with 'A' exactly
    when its id hits"""
    recs, size, i = [], 0, 0
    while (size < total) if count is None else (i < count):
        rid, n = ident(i), rnd.randint(*lens)
        seq = ("A" if hits(rid) else rnd.choice("CGT")) + "".join(rnd.choices("ACGT", k=n - 1))
        recs.append((rid, seq, "".join(rnd.choices("FI5", k=n))))
        size += 2 * n + len(rid) + 6
        i += 1
    return recs


def fastq_text(recs, eol="\n", plus_id=False):
    return "".join("@%s%s%s%s+%s%s%s%s" % (rid, eol, seq, eol, rid if plus_id else "", eol, qual, eol) for rid, seq, qual in recs).encode()


def parse(text):
    """-> (is FASTQ, [(id, stored sequence, quality, header's line end)]): the plain 4-line rule (blank lines between records skipped),
    or the header-line rule of FASTA (the stored sequence keeps its inner line breaks, not its final line end)"""
    lines = text.decode().split("\n")
    out, k = [], 0
    if text[:1] == b">":
        for part in ("\n" + text.decode()).split("\n>")[1:]:
            head, _, body = part.partition("\n")
            out.append((head.rstrip("\r"), body.rstrip("\r\n"), None, "\r\n" if head.endswith("\r") else "\n"))
        return False, out
    while k + 3 < len(lines):
        if lines[k].strip("\r") == "":
            k += 1
            continue
        eol = "\r\n" if lines[k].endswith("\r") else "\n"
        out.append((lines[k].rstrip("\r")[1:], lines[k + 1].rstrip("\r"), lines[k + 3].rstrip("\r"), eol))
        k += 4
    return True, out


def expected(texts, names, invert=False):
    """-> ([the output of every input], the text log's rows) for one input or a pair"""
    parsed = [parse(t) for t in texts]
    n = min(len(p[1]) for p in parsed)
    outs, rows = [[] for _ in texts], []
    for r in range(n):
        if any(hits(p[1][r][0]) for p in parsed) == invert:
            continue
        for f, (fastq, recs) in enumerate(parsed):
            rid, seq, qual, eol = recs[r]
            outs[f].append(("@%s%s%s%s+%s%s%s" % (rid, eol, seq, eol, eol, qual, eol)) if fastq else ">%s%s%s%s" % (rid, eol, seq, eol))
            rows.append("%s\t%s\tACGT\t0\n" % (names[f], rid))
    return ["".join(o).encode() for o in outs], "".join(rows).encode()


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("xw")
    cli_dir = os.path.join(ROOT, "merkurio_amd/csrc/cli")
    exe = str(d / "extract_windows_harness")
    stages = [os.path.join(cli_dir, f + ".cpp") for f in ("extract_windows", "extract_sources", "extract_window_call", "extract_write")]
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-w", "-I", cli_dir, "-o", exe, os.path.join(ROOT, "tests/helpers/extract_windows_harness.cpp"),
                    *stages, *reader_sources()], check=True)
    rnd = random.Random(5)
    single = fastq_records(rnd, 5 * MIB)
    m1 = fastq_records(rnd, 3 * MIB, lens=(100, 150), ident=lambda i: "p%d/1" % i)
    m2 = fastq_records(rnd, count=len(m1), lens=(100, 150), ident=lambda i: "p%d/2 the second mate carries a longer header line" % i)
    return {"d": d, "exe": exe, "single": fastq_text(single), "single_recs": single, "m1": m1, "m2": m2}


def run(job, name, text, flags="-", handles=1, text2=None, ext=".fastq", raw=False):
    """runs the harness over the input(s) -> (exit status, stdout, [outputs], log)"""
    d = job["d"]
    ins = []
    for k, t in enumerate([text] if text2 is None else [text, text2]):
        p = d / ("%s_in%d%s" % (name, k + 1, ext))
        p.write_bytes(t)
        ins.append(str(p))
    p = subprocess.run([job["exe"], str(d / name), str(handles), flags, *ins], capture_output=True, text=True)
    assert p.returncode in (0, 1) and p.stderr == "", p.stdout + p.stderr
    outs = [open(d / ("%s_%d.out" % (name, k + 1)), "rb").read() for k in range(len(ins))]
    log = open(d / (name + ".log"), "rb").read() if "l" in flags else b""
    return p.returncode, p.stdout, outs, log, [os.path.basename(i) for i in ins]


def windows(stdout):
    """-> [(head bytes of input 1, of input 2, by_host)] per window the stub answered"""
    return [(int(f[3]), int(f[4]), int(f[6])) for f in (ln.split() for ln in stdout.split("\n")) if f and f[0] == "#window"]


@pytest.mark.parametrize("flags", ["-", "l", "vl"])
def test_a_plain_fastq_of_five_windows(job, flags):
    rc, stdout, outs, log, names = run(job, "plain_" + flags.strip("-"), job["single"], flags)
    want, rows = expected([job["single"]], names, invert="v" in flags)
    assert rc == 0 and "#error" not in stdout and "#records %d" % len(job["single_recs"]) in stdout, stdout
    w = windows(stdout)
    assert len(w) >= 5 and not any(h for _, _, h in w), w
    assert outs[0] == want[0] and len(want[0]) > MIB
    assert log == (rows if "l" in flags else b"")


@pytest.mark.parametrize("form", ["crlf", "plus_id"])
def test_fastq_that_is_not_stored_the_way_it_is_written(job, form):
    # (records of 20 to 60 bases: more of them in a window than the driver's first guess -- the call is made again)
    recs = fastq_records(random.Random(6), 3 * MIB, lens=(20, 60))
    text = fastq_text(recs, eol="\r\n" if form == "crlf" else "\n", plus_id=form == "plus_id")
    rc, stdout, outs, log, names = run(job, form, text, "l")
    want, rows = expected([text], names)
    assert rc == 0 and "#error" not in stdout, stdout
    assert outs[0] == want[0] and log == rows
    assert (b"\r\n+\r\n" in outs[0]) if form == "crlf" else (b"\n+\n" in outs[0] and b"\n+r" not in outs[0])


def test_wrapped_fasta_with_a_record_longer_than_three_windows(job):
    rnd = random.Random(7)
    parts = []
    for i in range(1200):
        rid = "c%d some description" % i
        n = 3 * MIB + MIB // 2 if i == 500 else rnd.randint(200, 2000)
        seq = ("A" if hits(rid) else rnd.choice("CGT")) + "".join(rnd.choices("ACGT", k=n - 1))
        parts.append(">%s\n%s\n" % (rid, "\n".join(seq[b:b + 60] for b in range(0, n, 60))))
    text = "".join(parts).encode()
    rc, stdout, outs, log, names = run(job, "fasta", text, "l", ext=".fasta")
    want, rows = expected([text], names)
    assert rc == 0 and "#error" not in stdout and "#records 1200" in stdout, stdout
    assert outs[0] == want[0] and log == rows and len(windows(stdout)) >= 2


def pair_texts(job, n1=None, n2=None):
    return fastq_text(job["m1"][:n1]), fastq_text(job["m2"][:n2])


def test_a_pair_whose_second_file_has_longer_ids_carries_leftovers(job):
    t1, t2 = pair_texts(job)
    rc, stdout, outs, log, names = run(job, "pair", t1, "l", text2=t2)
    want, rows = expected([t1, t2], names)
    assert rc == 0 and "#error" not in stdout, stdout
    assert outs == want and log == rows
    w = windows(stdout)
    assert len(w) >= 3 and any(h1 > 0 for h1, _, _ in w[1:]), w  # (file 1's windows hold more records than file 2's: its leftovers are carried)


@pytest.mark.parametrize("codec", ["gzip", "bgzf"])
def test_compressed_input_read_by_the_host_codec(job, codec):
    data = gzip.compress(job["single"], 1) if codec == "gzip" else _bgzf(job["single"]) + EOF
    rc, stdout, outs, log, names = run(job, codec, data, "cl", ext=".fastq.gz")
    want, rows = expected([job["single"]], names)
    assert rc == 0 and "#error" not in stdout, stdout
    assert outs[0] == want[0] and log == rows and len(windows(stdout)) >= 4


def test_a_blank_line_sends_its_window_alone_to_the_host_parser(job):
    text = job["single"]
    at = text.index(b"\n@r", MIB + MIB // 2) + 1  # (a record start in the middle of the second window)
    rc, stdout, outs, log, names = run(job, "blank", text[:at] + b"\n" + text[at:], "l")
    want, rows = expected([text], names)
    assert rc == 0 and "#error" not in stdout, stdout
    assert outs[0] == want[0] and log == rows
    assert [k for k, (_, _, h) in enumerate(windows(stdout)) if h] == [1], stdout


@pytest.mark.parametrize("short,message", [(1, E_FILE2_SHORT), (0, E_FILE2_LONG)])
def test_a_pair_with_one_record_missing_writes_the_common_part_then_fails(job, short, message):
    n = len(job["m1"])
    t1, t2 = pair_texts(job, n - 1 if short == 0 else n, n - 1 if short == 1 else n)
    rc, stdout, outs, _, names = run(job, "short%d" % short, t1, text2=t2)
    want, _ = expected([t1, t2], names)
    assert rc == 1 and "#error " + message in stdout, stdout
    assert outs == want


def test_blank_lines_at_the_end_of_the_second_file_are_no_error(job):
    t1, t2 = pair_texts(job)
    rc, stdout, outs, _, names = run(job, "blank_end", t1, text2=t2 + b"\n\n\n")
    want, _ = expected([t1, t2], names)
    assert rc == 0 and "#error" not in stdout, stdout
    assert outs == want


def test_garbage_behind_the_last_record_fails_after_what_is_in_front_of_it(job):
    rc, stdout, outs, _, names = run(job, "garbage", job["single"] + b"no record starts like this\n")
    want, _ = expected([job["single"]], names)
    assert rc == 1 and "#error Error during FASTQ/A record parsing." in stdout, stdout
    # (the windows in front of the one that holds the garbage -- at most the last 1 MiB and a record -- have been written)
    assert want[0].startswith(outs[0]) and outs[0].endswith(b"\n") and len(outs[0]) > len(want[0]) // 2


def test_one_two_and_three_handles_write_the_same_bytes(job):
    for n in (1, 2, 3):
        rc, stdout, outs, log, names = run(job, "handles%d" % n, job["single"], "l", handles=n)
        want, rows = expected([job["single"]], names)
        assert rc == 0 and "#error" not in stdout, stdout
        assert outs[0] == want[0] and log == rows
