"""`merkurio extract --zstd-output` on the window path: a window's kept records are packed in their written form, cut and compressed on
its device and come down as zstd frames (mk_extract_window_frames).  Inputs of several windows (--window-mb 1) with '+id' lines, so that
the written form is not the stored one; every case runs --zstd-output on the new path (--z-members-from 0), --zstd-output --host-codec
(libzstd at the same cut rule: the checker) and plain output: the decoded .zst is the plain output byte for byte, every frame decodes
alone and starts at a record start, the logs are the plain run's, and the MERKURIO_TIMING rows say how many windows left as frames and
how many frames the window path made."""
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import zstd_out_cases as zo
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


def _bgzf(data, block):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("frames_in")
    fq1, fq2 = _reads(1, 15000, 1), _reads(2, 15000, 2)  # 5.3 MB each
    assert len(fq1) > 5 << 20
    rng = np.random.default_rng(3)
    fa = []
    for r in range(3800):  # 3.3 MB, wrapped at 60 columns, records of less than 16 384 bytes
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


def run(args):
    """-> (windows as frames, windows as text, frames from the window path, frames from the gathering path), None where a row is missing"""
    p = subprocess.run([BIN] + args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))
    if p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    w = re.search(rb"extract --zstd-output on the windows' devices: (\d+) windows as frames, (\d+) as text; written form ([0-9.]+) ms", p.stderr)
    f = re.search(rb"\[timing\] zstd output \(([^)]*)\): (\d+) frames written.*; (\d+) frames from the window path, (\d+) from the gathering path", p.stderr)
    if not f:
        return None
    assert int(f.group(2)) == int(f.group(3)) + int(f.group(4))
    return (int(w.group(1)) if w else 0, int(w.group(2)) if w else 0, int(f.group(3)), int(f.group(4)))


def record_starts(text, fastq):
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1
    line_starts = np.concatenate([[0], nl[:-1] if len(nl) and nl[-1] == len(text) else nl])
    if fastq:
        return set(line_starts[::4].tolist())
    b = np.frombuffer(text, dtype=np.uint8)
    return set(int(x) for x in line_starts if b[x] == 62)


def check_zst(blob, plain, fastq, own_format):
    """every frame decodes alone, together they are the plain output, every frame starts at a record start.  -> the frames' text sizes"""
    frames = zo.frames_by_libzstd(blob)
    assert b"".join(t for _, t in frames) == plain
    if own_format:
        for f, t in frames:
            assert zo.shape(f)["text"] == len(t) <= zo.TEXT_MAX - 1
    sizes = [len(t) for _, t in frames]
    starts = record_starts(plain, fastq)
    at = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    assert all(int(x) in starts for x in at), "a frame starts inside a record"
    return sizes


def three_ways(tmp_path, base, ext, paired=False, extra=(), z_from="0", logs=False, new_path_only=()):
    """-> run()'s tuple of the new path, the frames' text sizes per output; asserted: the three outputs agree"""
    out = {}
    for tag, fl in (("plain", []), ("frames", ["--zstd-output", "--z-members-from", z_from, *new_path_only]), ("hostcodec", ["--zstd-output", "--host-codec"])):
        d = tmp_path / tag
        d.mkdir()
        lg = ["-l", str(d / "x.log"), "-j", str(d / "x.json")] if logs else []
        out[tag] = run(["extract", *base, "-s", P, "-r", "--window-mb", "1", *extra, *fl, *lg, "-o", str(d / "kept")])
    names = ["kept_1", "kept_2"] if paired else ["kept"]
    sizes = []
    for nm in names:
        plain = (tmp_path / "plain" / f"{nm}.{ext}").read_bytes()
        assert len(plain) > 500000
        sizes.append(check_zst((tmp_path / "frames" / f"{nm}.{ext}.zst").read_bytes(), plain, ext == "fastq", True))
        check_zst((tmp_path / "hostcodec" / f"{nm}.{ext}.zst").read_bytes(), plain, ext == "fastq", False)
    if logs:
        body = lambda p: open(p, "rb").read().split(b"\n", 4)[4]
        assert body(tmp_path / "frames" / "x.log") == body(tmp_path / "plain" / "x.log")
        ja, jb = json.load(open(tmp_path / "frames" / "x.json")), json.load(open(tmp_path / "plain" / "x.json"))
        for k in ("matching_records", "pattern_hit_counts", "summary_statistics", "paired_end_reads_statistics"):
            assert ja.get(k) == jb.get(k) and (k in ja) == (k in jb), k
        assert len(ja["matching_records"]) > 1000
    assert out["plain"] is None and out["hostcodec"][:3] == (0, 0, 0)
    windows, text, from_windows, gathered = out["frames"]
    assert from_windows + gathered == sum(len(s) for s in sizes)
    return out["frames"], sizes


def test_single_fastq(inputs, tmp_path):
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq")
    assert windows >= 5 and text == 0 and from_windows >= windows and gathered == 0


def test_single_fasta(inputs, tmp_path):
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "g.fasta")], "fasta")
    assert windows >= 3 and text == 0 and from_windows >= windows and gathered == 0


def test_paired(inputs, tmp_path):
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq"), "-2", str(inputs / "a_2.fastq")], "fastq", paired=True)
    assert windows >= 5 and text == 0 and from_windows >= 2 * windows and gathered == 0


def test_two_handles_on_one_device(inputs, tmp_path):
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq", new_path_only=["--gpus", "2"])
    assert windows >= 5 and text == 0 and from_windows >= windows and gathered == 0


def test_logs_are_plain_outputs(inputs, tmp_path):
    (windows, text, from_windows, _), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq"), "-2", str(inputs / "a_2.fastq")], "fastq", paired=True, logs=True)
    assert windows >= 5 and text == 0 and from_windows >= 2 * windows


def test_invert(inputs, tmp_path):
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq", extra=["-v"])
    assert windows >= 5 and text == 0 and from_windows >= windows and gathered == 0


def test_bgzipped_input(inputs, tmp_path):
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "b.fastq.gz")], "fastq")
    assert windows >= 5 and text == 0 and from_windows >= windows and gathered == 0


def test_a_window_of_the_host_parser_keeps_its_place(inputs, tmp_path):
    """its kept records gather as text and leave as frames of the gathering path, between the windows' own"""
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "blank.fastq")], "fastq")
    assert windows >= 4 and text == 0 and from_windows >= windows and gathered >= 1


def test_text_and_frame_windows_in_turn(inputs, tmp_path):
    """windows of 20 % and of 80 % kept records: about 0.2 and 0.85 MB of written text a window"""
    (windows, text, from_windows, gathered), _ = three_ways(tmp_path, ["-i", str(inputs / "a_1.fastq")], "fastq", z_from="500000")
    assert windows >= 2 and text >= 2 and from_windows >= windows and gathered >= 2


def test_default_threshold_keeps_a_small_job_on_the_gathering_path(inputs, tmp_path):
    """8 MiB: no window of this file reaches it -- the frames are the gathering path's, cut by the rule on the whole kept text: the
    bytes of a threshold nothing reaches, and the frame sizes of --host-codec"""
    d = tmp_path
    args = ["extract", "-i", str(inputs / "a_1.fastq"), "-s", P, "-r", "--window-mb", "1", "--zstd-output"]
    got = run(args + ["-o", str(d / "dev")])
    huge = run(args + ["--z-members-from", str(1 << 40), "-o", str(d / "huge")])
    run(args + ["--host-codec", "-o", str(d / "host")])
    assert got[0] == 0 and got[1] >= 5 and got[2] == 0 and got[3] >= 2 and huge == got
    a, b, c = ((d / f"{n}.fastq.zst").read_bytes() for n in ("dev", "huge", "host"))
    assert a == b
    fa, fc = zo.frames_by_libzstd(a), zo.frames_by_libzstd(c)
    assert [t for _, t in fa] == [t for _, t in fc]


def test_an_empty_result_is_still_one_empty_frame(inputs, tmp_path):
    got = run(["extract", "-i", str(inputs / "a_1.fastq"), "-s", "ACGTTGCAACGTTGCAACGTTGCAACGTTGC", "--window-mb", "1", "--zstd-output", "--z-members-from", "0",
               "-o", str(tmp_path / "none")])
    blob = (tmp_path / "none.fastq.zst").read_bytes()
    assert len(blob) == 16 and [t for _, t in zo.frames_by_libzstd(blob)] == [b""] and zo.shape(blob)["block"] == 0
    assert got[2] == 0 and got[3] == 1  # (the empty frame is the writer's own)


def test_the_timing_rows_name_the_window_path(inputs, tmp_path):
    p = subprocess.run([BIN, "extract", "-i", str(inputs / "a_1.fastq"), "-s", P, "-r", "--window-mb", "1", "--zstd-output", "--z-members-from", "0", "-o",
                        str(tmp_path / "t")], capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()
    err = p.stderr.decode()
    rows = [l for l in err.splitlines() if l.startswith("[timing] zstd output")]
    assert len(rows) == 1 and "(device codec)" in rows[0], err[-2000:]
    n_frames = len(zo.frames_by_libzstd((tmp_path / "t.fastq.zst").read_bytes()))
    m = re.search(r"; (\d+) frames from the window path, (\d+) from the gathering path", rows[0])
    assert m and int(m.group(1)) == n_frames > 0 and int(m.group(2)) == 0 and f"{n_frames} frames written" in rows[0]
    k = re.search(r"blocks raw (\d+) rle (\d+) compressed (\d+),", rows[0])
    assert sum(map(int, k.groups())) == n_frames
    w = re.search(r"extract --zstd-output on the windows' devices: (\d+) windows as frames, 0 as text; written form ([0-9.]+) ms, cut \+ deflate ([0-9.]+) ms", err)
    assert w and int(w.group(1)) >= 5 and float(w.group(2)) > 0 and float(w.group(3)) > 0
