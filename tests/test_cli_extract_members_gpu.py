"""`merkurio extract -z` on the window path: a window's kept records are packed in their written form, cut and deflated on its device
and come down as BGZF members (mk_extract_window_members).  Inputs of several windows (--window-mb 1) with '+id' lines, so that the
written form is not the stored one; every case runs -z on the new path (--z-members-from 0), -z --host-codec and plain output:
Python's gzip of -z is the plain output byte for byte, every member starts at a record start, and the MERKURIO_TIMING line says how
many windows left as members."""
import gzip
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from merkurio_amd import native as mk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
P = "ACGTTGCAAGGCTTAACGGAT"
CHUNK = 3000  # records (about a window) that share a share of kept records: 20 % and 80 % in turn


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build
    build.build_all()
    if mk.device_count() < 1:
        pytest.fail("no HIP device visible")


def _reads(seed, n, mate):
    rng = np.random.default_rng(seed)
    seqs = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, 150))
    hit = rng.random(n) < np.where((np.arange(n) // CHUNK) % 2 == 0, 0.2, 0.8)
    out = []
    for r in range(n):
        s = seqs[r].tobytes().decode()
        if hit[r]:
            k = (r * 7) % (150 - len(P))
            s = s[:k] + P + s[k + len(P):]
        name = "read%07d/%d extra words" % (r, mate)
        out.append("@%s\n%s\n+%s\n%s\n" % (name, s, name, "IIIIFFFF##" * 15))
    return "".join(out).encode()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("members_in")
    fq1, fq2 = _reads(1, 15000, 1), _reads(2, 15000, 2)  # 5.3 MB each
    assert len(fq1) > 5 << 20
    rng = np.random.default_rng(3)
    fa = []
    for r in range(3800):  # 3.3 MB, wrapped at 60 columns, records of less than 16 128 bytes
        L = int(rng.integers(300, 1400))
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L).tobytes().decode()
        if (r // 500) % 2 == 0 or r % 5 == 0:
            s = s[:100] + P + s[100 + len(P):]
        fa.append(">chr%d len=%d\n%s\n" % (r, L, "\n".join(s[k:k + 60] for k in range(0, L, 60))))
    fa = "".join(fa).encode()
    assert len(fa) > 3 << 20
    (d / "a_1.fastq").write_bytes(fq1)
    (d / "a_2.fastq").write_bytes(fq2)
    (d / "g.fasta").write_bytes(fa)
    (d / "b.fastq.gz").write_bytes(_bgzf(fq1, 60000) + mk.bgzf_eof())
    # a blank line in the middle of the file: the window that holds it is the host parser's
    k = fq1.index(b"\n@read0007000/") + 1
    (d / "blank.fastq").write_bytes(fq1[:k] + b"\n" + fq1[k:])
    return d


def _bgzf(data, block):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def run(args):
    p = subprocess.run([BIN] + args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))
    if p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    m = re.search(rb"extract -z: (\d+) windows as members, (\d+) as text", p.stderr)
    return (int(m.group(1)), int(m.group(2))) if m else None


def record_starts(text, fastq):
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1
    line_starts = np.concatenate([[0], nl[:-1] if len(nl) and nl[-1] == len(text) else nl])
    if fastq:
        return set(line_starts[::4].tolist())
    b = np.frombuffer(text, dtype=np.uint8)
    return set(int(x) for x in line_starts if b[x] == 62)


def check_z(blob, plain, fastq):
    mem, used, _ = mk.bgzf_members(blob)
    assert used == len(blob) and blob[-28:] == mk.bgzf_eof() and int(mem[-1]["isize"]) == 0
    assert gzip.decompress(blob) == plain
    starts = record_starts(plain, fastq)
    at = np.concatenate([[0], np.cumsum(mem["isize"][:-1])])[:-1]
    assert all(int(x) in starts for x in at), "a member starts inside a record"
    return mem["isize"][:-1].tolist()


def three_ways(tmp_path, base, ext, paired=False, extra=(), z_from="0", logs=False, new_path_only=()):
    """-> (windows as members, windows as text) of the new path; asserted: the three outputs agree.  new_path_only: flags of the new
    path's run alone (the other two are then the one-handle reference)"""
    out = {}
    for tag, fl in (("plain", []), ("members", ["-z", "--z-members-from", z_from, *new_path_only]), ("hostcodec", ["-z", "--host-codec"])):
        d = tmp_path / tag
        d.mkdir()
        lg = ["-l", str(d / "x.log"), "-j", str(d / "x.json")] if logs else []
        out[tag] = run(["extract", *base, "-s", P, "-r", "--window-mb", "1", *extra, *fl, *lg, "-o", str(d / "kept")])
    names = ["kept_1", "kept_2"] if paired else ["kept"]
    sizes = []
    for nm in names:
        plain = (tmp_path / "plain" / f"{nm}.{ext}").read_bytes()
        assert len(plain) > 500000
        sizes.append(check_z((tmp_path / "members" / f"{nm}.{ext}.gz").read_bytes(), plain, ext == "fastq"))
        check_z((tmp_path / "hostcodec" / f"{nm}.{ext}.gz").read_bytes(), plain, ext == "fastq")
    if logs:
        body = lambda p: open(p, "rb").read().split(b"\n", 4)[4]
        assert body(tmp_path / "members" / "x.log") == body(tmp_path / "plain" / "x.log")
        ja, jb = json.load(open(tmp_path / "members" / "x.json")), json.load(open(tmp_path / "plain" / "x.json"))
        for k in ("matching_records", "pattern_hit_counts", "summary_statistics", "paired_end_reads_statistics"):
            assert ja.get(k) == jb.get(k) and (k in ja) == (k in jb), k
        assert len(ja["matching_records"]) > 1000
    assert out["hostcodec"] == (0, 0)
    return out["members"], sizes


def test_single_fastq(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq")
    assert members >= 5 and text == 0


def test_single_fasta(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "g.fasta")], "fasta")
    assert members >= 3 and text == 0


def test_paired(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq"), "-2", str(inputs / "a_2.fastq")], "fastq", paired=True)
    assert members >= 5 and text == 0


def test_two_handles_on_one_device(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq", new_path_only=["--gpus", "2"])
    assert members >= 5 and text == 0


def test_logs_are_plain_outputs(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq"), "-2", str(inputs / "a_2.fastq")], "fastq", paired=True, logs=True)
    assert members >= 5 and text == 0


def test_invert(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq", extra=["-v"])
    assert members >= 5 and text == 0


def test_bgzipped_input(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "b.fastq.gz")], "fastq")
    assert members >= 5 and text == 0


def test_a_window_of_the_host_parser_keeps_its_place(inputs, tmp_path):
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "blank.fastq")], "fastq")
    assert members >= 4 and text == 0


def test_text_and_member_windows_in_turn(inputs, tmp_path):
    """windows of 20 % and of 80 % kept records: about 0.2 and 0.85 MB of written text a window"""
    (members, text), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq", z_from="500000")
    assert members >= 2 and text >= 2


def test_default_threshold_keeps_small_windows_on_the_gathering_path(inputs, tmp_path):
    """8 MiB: no window of this file reaches it -- the output is the gathering path's, cut by the rule on the whole kept text, as
    --host-codec's is"""
    d = tmp_path
    args = ["extract", "-i", str(inputs / "a_1.fastq"), "-s", P, "-r", "--window-mb", "1", "-z"]
    got = run(args + ["-o", str(d / "dev")])
    run(args + ["--host-codec", "-o", str(d / "host")])
    assert got is not None and got[0] == 0 and got[1] >= 5
    a, b = (d / "dev.fastq.gz").read_bytes(), (d / "host.fastq.gz").read_bytes()
    assert gzip.decompress(a) == gzip.decompress(b)
    assert mk.bgzf_members(a)[0]["isize"].tolist() == mk.bgzf_members(b)[0]["isize"].tolist()


@pytest.fixture(scope="module")
def line_end_inputs(tmp_path_factory):
    """the shapes whose written form is not the stored one, for the host writer to be the judge of: FASTQ records with CRLF, an LF
    header over CRLF lines, a CRLF header over LF lines, '+id' lines; FASTA records with CRLF and with LF; in both files the last
    record is kept and has no line end"""
    d = tmp_path_factory.mktemp("members_eol")
    rng = np.random.default_rng(7)
    fq = []
    for r in range(7000):  # 2.4 MB: three windows
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=150).tobytes().decode()
        if r % 2 == 0 or r == 6999:
            s = s[:40] + P + s[40 + len(P):]
        name = "read%05d shape %d" % (r, r % 4)
        h, b = [("\r\n", "\r\n"), ("\n", "\r\n"), ("\r\n", "\n"), ("\n", "\n")][r % 4]
        fq.append("@%s%s%s%s+%s%s%s%s" % (name, h, s, b, name if r % 3 else "", b, "IIIIFFFF##" * 15, b))
    fq = "".join(fq).encode()
    assert fq.endswith(b"#\n")
    (d / "eol.fastq").write_bytes(fq[:-1])
    fa = []
    for r in range(2600):  # 2.3 MB
        L = int(rng.integers(300, 1400))
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L).tobytes().decode()
        if r % 2 == 0 or r == 2599:
            s = s[:100] + P + s[100 + len(P):]
        e = "\r\n" if r % 3 == 0 else "\n"
        fa.append(">chr%d len=%d%s%s%s" % (r, L, e, e.join(s[k:k + 60] for k in range(0, L, 60)), e))
    fa = "".join(fa).encode()
    assert fa.endswith(b"\n") and not fa.endswith(b"\r\n")
    (d / "eol.fasta").write_bytes(fa[:-1])
    return d


@pytest.mark.parametrize("ext", ["fastq", "fasta"])
def test_line_end_shapes_are_written_as_the_host_writer_writes_them(line_end_inputs, tmp_path, ext):
    (members, text), _ = three_ways(tmp_path, ["-i", str(line_end_inputs / f"eol.{ext}")], ext)
    assert members >= 3 and text == 0
    plain = (tmp_path / "plain" / f"kept.{ext}").read_bytes()
    assert b"\r\n" in plain and plain.endswith(b"\n") and re.search(rb"[^\r]\n", plain)
