"""The CLI's BGZF member table and run cutter (merkurio_amd/csrc/cli/bgzf_in.cpp: bgzf_walk, bgzf_run_end, bgzf_rebased) through
tests/helpers/bgzf_runs_harness.cpp, without a GPU or the library.  The files are written here, member by member, so every offset is known.

bgzf_run_end(m, m0, m_end, want): the first member not taken; at least one member is taken, then more while the text so far is less
than `want`; never past min(len(m), m_end); m0 == m_end takes nothing.  bgzf_rebased: data_off - file_lo, out_off - text_base.

The walker's verdicts are those of the reader before the member types were merged (WindowSource::open: `bgzf_members()` true -> BGZF,
false -> the serial gzip reader), read off its code:
  * FLG with FNAME set: it required `!(FLG & ~4)`, FLG exactly FEXTRA -> not BGZF, is_gzip();
  * a trailing partial member: `n - p < 18` (or `n - p < bsize`) at the last member start -> false for the whole file -> is_gzip();
  * an extra subfield in front of 'BC': it walked all subfields of the extra field and took BSIZE from 'BC' wherever it stood -> BGZF,
    data_off = member start + 12 + XLEN.
MERKURIO_TEST_SANITIZE=1 builds the harness with ASan + UBSan; the program is run directly."""
import os
import struct
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cli_sources import CLI_DIR, ROOT, reader_sources

_FLAGS = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
          if os.environ.get("MERKURIO_TEST_SANITIZE") else ["-O1"])
SIZES = [1, 300, 17, 0, 64, 255, 2, 300, 128, 5, 0]  # bytes of text per member: an empty member in the middle, the EOF marker last
ALL = 2 ** 64 - 1


def member(text, flg=4, front=b"", name=b""):
    """one gzip member with the BC subfield (behind `front`, other subfields) -> (bytes, offset of its DEFLATE stream, its length)"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    c = co.compress(text) + co.flush()
    xlen = len(front) + 6
    total = 12 + xlen + len(name) + len(c) + 8
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + front + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + name + c + struct.pack("<II", zlib.crc32(text), len(text)), 12 + xlen, len(c)


def build(texts, **kw):
    """-> (file bytes, [(data_off, out_off, data_len, isize, crc)])"""
    out, table, text_off = bytearray(), [], 0
    for t in texts:
        b, skip, clen = member(t, **kw)
        table.append((len(out) + skip, text_off, clen, len(t), zlib.crc32(t)))
        out += b
        text_off += len(t)
    return bytes(out), table


def fnv(b):
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & ALL
    return "%x" % h


def run_end(isizes, m0, m_end, want):
    end, m1, text = min(len(isizes), m_end), m0, 0
    while m1 < end and (m1 == m0 or text < want):
        text += isizes[m1]
        m1 += 1
    return m1


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_runs")
    exe = str(d / "bgzf_runs_harness")
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-w", "-I", CLI_DIR, "-o", exe, os.path.join(ROOT, "tests/helpers/bgzf_runs_harness.cpp"),
                    *reader_sources(without=("fastx", "sam_in", "bam_text", "bam_out"))], check=True)

    def harness(name, data, *queries):
        (d / name).write_bytes(data)
        p = subprocess.run([exe, str(d / name), *["%d:%d:%d" % q for q in queries]], capture_output=True, text=True, check=True)
        assert "#error" not in p.stdout, p.stdout
        return p.stdout.splitlines()
    return harness


def parse(lines):
    kind, n = lines[0].split()[1], int(lines[1].split()[1])
    table = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[2:2 + n]]
    rest = lines[2 + n:]
    text = rest.pop(0).split()[1:] if rest and rest[0].startswith("text") else None
    runs = []
    for ln in rest:
        if ln.startswith("run"):
            runs.append((tuple(int(x) for x in ln.split()[1:]), []))
        else:
            runs[-1][1].append(tuple(int(x) for x in ln.split()[1:]))
    return kind, table, text, runs


def test_runs_of_members_and_their_rebased_tables(job):
    texts = [bytes((7 * i + k) % 251 for k in range(n)) for i, n in enumerate(SIZES)]
    data, table = build(texts)
    n = len(SIZES)
    queries = []
    for k in (1, 2, 3, 5, 8):  # the sum of the first k ISIZEs exactly, one less, one more
        s = sum(SIZES[:k])
        queries += [(0, ALL, s), (0, ALL, s - 1), (0, ALL, s + 1)]
    queries += [(m0, ALL, 0) for m0 in (0, 3, n - 1)]                      # want 0: one member is still taken (an empty one too)
    queries += [(2, ALL, 1), (3, ALL, 1), (n - 2, ALL, 10 ** 9)]           # the empty member in the middle, the EOF marker at the end
    queries += [(n - 4, m_end, 10 ** 9) for m_end in (n - 2, n - 1, n, n + 5, ALL)]  # m_end in front of the last member, at it, past it
    queries += [(4, 6, 1), (4, 5, 10 ** 9)]
    queries += [(m, m, 100) for m in (0, 4, n)]                            # m0 == m_end: nothing is taken
    kind, got_table, text, runs = parse(job("t.gz", data, *queries))
    assert kind == "bgzf" and got_table == table
    assert text == [str(sum(SIZES)), fnv(b"".join(texts))]
    assert [r[0][:3] for r in runs] == queries
    for (m0, m_end, want, m1), rows in runs:
        assert m1 == run_end(SIZES, m0, m_end, want), (m0, m_end, want, m1)
        assert m1 <= min(n, m_end) and (m1 > m0 or m0 >= min(n, m_end))
        assert rows == [(a - table[m0][0], b - table[m0][1], c, d, e) for a, b, c, d, e in table[m0:m1]], (m0, m_end, want)
        assert not rows or rows[0][:2] == (0, 0)
    # the rule, spelled out for this file (1 + 300 + 17 = 318, then the empty member): exactly 318 and one less end behind three
    # members; one more takes the empty member and the next one
    ends = {q[0][:3]: q[0][3] for q in runs}
    assert ends[(0, ALL, 318)] == 3 and ends[(0, ALL, 317)] == 3 and ends[(0, ALL, 319)] == 5
    assert ends[(0, ALL, 0)] == 1 and ends[(3, ALL, 0)] == 4 and ends[(3, ALL, 1)] == 5 and ends[(2, ALL, 1)] == 3
    assert ends[(n - 2, ALL, 10 ** 9)] == n and ends[(n - 4, n - 2, 10 ** 9)] == n - 2 and ends[(n - 4, n + 5, 10 ** 9)] == n
    assert ends[(4, 4, 100)] == 4 and ends[(n, n, 100)] == n and ends[(4, 5, 10 ** 9)] == 5


def test_walker_verdicts(job):
    texts = [b"ACGT" * 20, b"\n", b"TTGA" * 75, b""]
    good, table = build(texts)
    # FLG with FNAME set (a valid gzip member, name included): not BGZF
    named, _ = build(texts, flg=4 | 8, name=b"reads.fq\0")
    assert zlib.decompress(named, 31) == texts[0]  # (zlib reads the first member: the file is sound gzip)
    kind, got, text, _ = parse(job("named.gz", named))
    assert kind == "gzip" and got == [] and text is None
    # a trailing partial member (ten bytes of a header; all but the last byte of a whole member): not BGZF
    first = table[1][0] - 18  # (the length of the first member: the second one's stream starts 18 bytes into it)
    for cut in (good + good[:10], good + good[:first - 1]):
        kind, got, text, _ = parse(job("partial.gz", cut))
        assert kind == "gzip" and got == [] and text is None
    # an extra subfield in front of BC: BGZF, the DEFLATE stream starts behind the whole extra field
    front = b"XY" + struct.pack("<H", 3) + b"abc"
    sub, sub_table = build(texts, front=front)
    assert [r[0] for r in sub_table][0] == 12 + 6 + len(front)
    kind, got, text, _ = parse(job("sub.gz", sub))
    assert kind == "bgzf" and got == sub_table and text == [str(sum(len(t) for t in texts)), fnv(b"".join(texts))]
    # and the plain file itself
    kind, got, text, _ = parse(job("good.gz", good))
    assert kind == "bgzf" and got == table
