"""`merkurio extract --open-windows` against the same command without the flag: ONE bgzip'ed FASTQ / FASTA input (members of 20 000
bytes, --window-mb 1, five windows and more), kept records, text log and JSON log equal -- plain, -v, -S -j, CRLF, two and three
handles; reads made to fool the start rule (same output, re-runs reported); a FASTA record that spans three windows (no start in a
window: the chained re-run); a damaged member and a malformed record in a late window (same error, same bytes in front of it); and the
flag is inert with -z and with a pair."""
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


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build
    build.build_all()
    if mk.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")


def _bgzf(data, block=20000):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out) + mk.bgzf_eof()


def _seqs(seed, n, lens, first=b""):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.choice(lens))
        s = bytearray(first + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes())
        if rng.random() < 0.2 and L >= len(P):
            k = int(rng.integers(len(first), len(first) + L - len(P) + 1))
            s[k:k + len(P)] = P.encode()
        out.append(bytes(s))
    return out


def _fastq(seed=1, n=22000, eol=b"\n", adversarial=False):
    recs = []
    for i, s in enumerate(_seqs(seed, n, [100, 150, 151], b"+" if adversarial else b"")):
        rid = b"r%07d" % i
        q = (b"@" if adversarial else b"I") + b"F" * (len(s) - 1)
        recs.append(b"@" + rid + eol + s + eol + b"+" + (rid if adversarial else b"") + eol + q + eol)
    return b"".join(recs)


def _fasta(seed=2, n=9000):
    return b"".join(b">c%d\n" % i + b"".join(s[k:k + 60] + b"\n" for k in range(0, len(s), 60)) for i, s in enumerate(_seqs(seed, n, [300, 600, 901])))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("open_in")
    texts = {"a.fastq.gz": _fastq(), "crlf.fastq.gz": _fastq(3, eol=b"\r\n"), "adv.fastq.gz": _fastq(4, adversarial=True), "g.fasta.gz": _fasta()}
    # one record of 2.5 MB between small ones: with 1 MB windows it spans three of them
    rng = np.random.default_rng(9)
    big = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2_500_000)].tobytes()
    small = _fasta(5, 4000)
    cut = small.index(b">c2000\n")
    texts["big.fasta.gz"] = small[:cut] + b">big\n" + b"".join(big[k:k + 60] + b"\n" for k in range(0, len(big), 60)) + P.encode() + b"\n" + small[cut:]
    for name, text in texts.items():
        assert len(text) > 5 << 20 or name == "big.fasta.gz"
        (d / name).write_bytes(_bgzf(text))
    return d


def run(args, ok=True):
    p = subprocess.run([BIN] + args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))
    if ok and p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    m = re.search(rb"extract --open-windows: (\d+) open windows, (\d+) seams, (\d+) re-runs", p.stderr)
    errors = b"\n".join(ln for ln in p.stderr.split(b"\n") if ln and not ln.startswith(b"[timing]"))
    return p.returncode, errors, tuple(int(x) for x in m.groups()) if m else None


def both(tmp_path, base, extra=(), only_open=(), ok=True):
    """the command without and with --open-windows -> (the flag's timing row, the two runs' (code, stderr)); asserted: same files"""
    res = {}
    for tag, fl in (("chain", []), ("open", ["--open-windows", *only_open])):
        d = tmp_path / tag
        d.mkdir()
        res[tag] = run(["extract", *base, "-s", P, "-r", "--window-mb", "1", *extra, *fl, "-l", str(d / "x.log"), "-j", str(d / "x.json"),
                        *([] if "-S" in extra else ["-o", str(d / "kept")])], ok)  # (-S: the logs are the output)
    a, b = tmp_path / "chain", tmp_path / "open"
    names = sorted(f for f in os.listdir(a) if f.startswith("kept"))
    assert names == sorted(f for f in os.listdir(b) if f.startswith("kept"))
    for f in names:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    if ok:
        body = lambda p: open(p, "rb").read().split(b"\n", 4)[4]
        assert body(a / "x.log") == body(b / "x.log")
        ja, jb = json.load(open(a / "x.json")), json.load(open(b / "x.json"))
        for k in ("matching_records", "pattern_hit_counts", "summary_statistics"):
            assert ja.get(k) == jb.get(k) and (k in ja) == (k in jb), k
        assert len(ja["matching_records"]) > 500
    assert res["chain"][2] is None
    return res["open"][2], res


@pytest.mark.parametrize("name,extra", [(n, e) for n in ("a.fastq.gz", "g.fasta.gz") for e in ((), ("-v",), ("-S",))] + [("crlf.fastq.gz", ())])
def test_same_output_and_every_guess_holds(inputs, tmp_path, name, extra):
    (n_open, seams, reruns), _ = both(tmp_path, ["-i", str(inputs / name)], extra)
    assert n_open >= 4 and seams == n_open and reruns == 0
    if "-S" not in extra:
        assert os.path.getsize(tmp_path / "open" / ("kept.fasta" if "fasta" in name else "kept.fastq")) > 100000


@pytest.mark.parametrize("gpus", ["2", "3"])
def test_several_handles(inputs, tmp_path, gpus):
    (n_open, seams, reruns), _ = both(tmp_path, ["-i", str(inputs / "a.fastq.gz")], only_open=["--gpus", gpus])
    assert n_open >= 4 and reruns == 0


def test_reads_made_to_fool_the_rule_are_run_again(inputs, tmp_path):
    (n_open, seams, reruns), _ = both(tmp_path, ["-i", str(inputs / "adv.fastq.gz")])
    assert reruns >= 1 and n_open >= reruns


def test_a_record_that_spans_three_windows_takes_the_chained_way(inputs, tmp_path):
    (n_open, seams, reruns), _ = both(tmp_path, ["-i", str(inputs / "big.fasta.gz")])
    assert reruns >= 1
    assert b">big\n" in (tmp_path / "open" / "kept.fasta").read_bytes()


def _late_member(blob, frac=0.8):
    mem, _, _ = mk.bgzf_members(blob)
    return mem[int(len(mem) * frac)]


def test_a_damaged_member_in_a_late_window(inputs, tmp_path):
    blob = bytearray((inputs / "a.fastq.gz").read_bytes())
    e = _late_member(bytes(blob))
    blob[int(e["data_off"]) + int(e["data_len"]) // 2] ^= 0x55
    bad = tmp_path / "bad.fastq.gz"
    bad.write_bytes(bytes(blob))
    _, res = both(tmp_path, ["-i", str(bad)], ok=False)
    assert res["chain"][0] != 0 and res["open"][:2] == res["chain"][:2] and res["chain"][1]
    assert os.path.getsize(tmp_path / "open" / "kept.fastq") > 100000


def test_a_malformed_record_in_a_late_window(inputs, tmp_path):
    text = bytearray(_fastq())
    at = text.index(b"@r0018000\n")
    q = text.index(b"\n+\n", at) + 3
    del text[q:q + 7]  # the quality line of record 18 000 is seven bytes short
    bad = tmp_path / "bad.fastq.gz"
    bad.write_bytes(_bgzf(bytes(text)))
    _, res = both(tmp_path, ["-i", str(bad)], ok=False)
    assert res["chain"][0] != 0 and res["open"][:2] == res["chain"][:2] and res["chain"][1]
    assert os.path.getsize(tmp_path / "open" / "kept.fastq") > 100000


def test_the_flag_is_inert_with_z_and_with_a_pair(inputs, tmp_path):
    (tmp_path / "z").mkdir()
    timing, _ = both(tmp_path / "z", ["-i", str(inputs / "a.fastq.gz")], ["-z"])
    assert timing is None
    (tmp_path / "pair").mkdir()
    timing, _ = both(tmp_path / "pair", ["-i", str(inputs / "a.fastq.gz"), "-2", str(inputs / "crlf.fastq.gz")])
    assert timing is None
