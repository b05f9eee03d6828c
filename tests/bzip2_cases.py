"""The .bz2 files of test_bunzip2_cpu.py (bzip2_serial.hpp on the host) and test_gpu_bunzip2.py (the same code on a wave per block):
valid files that must be taken, damaged ones that must be handed back.  Python's bz2 (libbz2) writes and checks them.  A small
bit-level reader of a block's header finds the fields that the damaged files flip or patch."""
import bz2
import functools
import os
import random
import subprocess
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090


def fastq(n, seed=5):
    rng = random.Random(seed)
    return b"".join(b"@read%d lane=%d\n%s\n+\n%s\n" % (i, i % 8, bytes(rng.choices(b"ACGT", k=150)), bytes(rng.choices(b"FFFF:,#", k=150)))
                    for i in range(n))


def rle_text():
    """runs of 3, 4, 5, 258, 259, 260 and 1 000 equal bytes.  At level 1 a block closes at 99 981 symbols; 99 971 single bytes, then
    the run of 1 000 (coded 255 + 255 + 255 + 235, five symbols each): its second piece ends the first block exactly"""
    t = bytes(i % 251 for i in range(99971)) + b"A" * 1000
    for k, r in enumerate((3, 4, 5, 258, 259, 260, 1000, 4, 255, 256)):
        t += b"x" + bytes([66 + k]) * r
    return t + b"y" + b"Z" * 4  # (a run of exactly four ends the text: its count is 0)


@functools.lru_cache(maxsize=None)
def valid():
    """name -> (file, text)"""
    rng = random.Random(17)
    fq = fastq(1200)
    texts = {"empty": b"", "one": b"A", "all256": bytes(range(256)), "rle": rle_text(), "fastq": fq[:200000],
             "random": bytes(rng.getrandbits(8) for _ in range(120000)), "two-symbol": bytes(rng.choices(b"ab", k=50000)),
             "skew": bytes(rng.choices(b"a" * 300 + bytes(range(256)), k=90000))}
    out = {}
    for name, text in texts.items():
        for level in (1, 5, 9):
            out["%s-l%d" % (name, level)] = (bz2.compress(text, level), text)
    out["four-blocks-l1"] = (bz2.compress(fq[:350000], 1), fq[:350000])
    parts = [(fq[:90000], 1), (fq[90000:200000], 9), (b"", 5), (fq[200000:320000], 3)]
    out["two-streams"] = (b"".join(bz2.compress(t, l) for t, l in parts[:2]), b"".join(t for t, _ in parts[:2]))
    out["three-streams"] = (b"".join(bz2.compress(t, l) for t, l in (parts[0], parts[1], parts[3])), parts[0][0] + parts[1][0] + parts[3][0])
    out["streams-with-an-empty-one"] = (b"".join(bz2.compress(t, l) for t, l in parts), b"".join(t for t, _ in parts))
    with open(os.path.join(GOLDEN, "sample.fasta.bz2"), "rb") as f, open(os.path.join(GOLDEN, "sample.fasta.gz"), "rb") as g:
        out["golden-sample"] = (f.read(), zlib.decompress(g.read(), 31))
    return out


# ---- bits ----------------------------------------------------------------------------------------------------------------------------
def get_bits(b, at, k):
    v = 0
    for i in range(at, at + k):
        v = v << 1 | (b[i >> 3] >> (7 - (i & 7)) & 1)
    return v


def put_bits(b, at, k, v):
    """b: bytearray"""
    for j in range(k):
        i = at + j
        bit = v >> (k - 1 - j) & 1
        b[i >> 3] = (b[i >> 3] & ~(1 << (7 - (i & 7)))) | bit << (7 - (i & 7))


def flip(b, at):
    out = bytearray(b)
    out[at >> 3] ^= 1 << (7 - (at & 7))
    return bytes(out)


def find_magics(b):
    """[(bit, kind)] of every block (0) / end (1) magic, every bit offset tested"""
    v, out = 0, []
    for i in range(len(b) * 8):
        v = (v << 1 | (b[i >> 3] >> (7 - (i & 7)) & 1)) & ((1 << 48) - 1)
        if i >= 47 and v in (BLOCK_MAGIC, END_MAGIC):
            out.append((i - 47, int(v == END_MAGIC)))
    return out


def block_layout(b, magic_bit):
    """bit offsets of the fields of the block whose magic stands at magic_bit"""
    at = magic_bit + 48
    lay = {"crc": at, "randomised": at + 32, "orig_ptr": at + 33, "map": at + 57}
    at += 57
    used16 = get_bits(b, at, 16)
    at += 16
    n_in_use = 0
    for i in range(16):
        if used16 >> (15 - i) & 1:
            n_in_use += bin(get_bits(b, at, 16)).count("1")
            at += 16
    lay["n_groups"] = at
    n_groups, n_sel = get_bits(b, at, 3), get_bits(b, at + 3, 15)
    at += 18
    lay["selectors"] = at
    for _ in range(n_sel):
        while get_bits(b, at, 1):
            at += 1
        at += 1
    lay["lengths"] = at
    for _ in range(n_groups):
        at += 5
        for _ in range(n_in_use + 2):
            while get_bits(b, at, 1):
                at += 2
            at += 1
    lay["symbols"] = at
    return lay


@functools.lru_cache(maxsize=None)
def two_block_file():
    text = fastq(1200)[:150000]
    blob = bz2.compress(text, 1)
    magics = find_magics(blob)
    assert [k for _, k in magics] == [0, 0, 1]
    return blob, text, magics


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> file: every one must be handed back"""
    blob, text, magics = two_block_file()
    lay = block_layout(blob, magics[1][0])  # the second block, which starts at some bit of a byte
    out = {"flip-stream-header": flip(blob, 27), "flip-selectors": flip(blob, lay["selectors"] + 5), "flip-lengths": flip(blob, lay["lengths"] + 7),
           "flip-symbols": flip(blob, (lay["symbols"] + magics[2][0]) // 2), "flip-block-crc": flip(blob, lay["crc"] + 9),
           "flip-stream-crc": flip(blob, magics[2][0] + 48 + 3), "flip-first-block-symbols": flip(blob, (block_layout(blob, 32)["symbols"] + magics[1][0]) // 2),
           "trailing-bytes": blob + b"\n", "trailing-garbage": blob + b"BZh9garbage-behind-the-stream"}
    for k in range(1, 10):
        out["cut-%d0%%" % k] = blob[:len(blob) * k // 10]
    # hand-patched headers of a one-block file
    one_text = fastq(300)[:60000]
    one = bz2.compress(one_text, 9)
    l1 = block_layout(one, 32)
    nblock = rle1_symbols(one_text)
    for name, field, bits, value in (("randomised", "randomised", 1, 1), ("origptr-nblock", "orig_ptr", 24, nblock), ("ngroups-1", "n_groups", 3, 1),
                                     ("ngroups-7", "n_groups", 3, 7)):
        p = bytearray(one)
        put_bits(p, l1[field], bits, value)
        out["patched-" + name] = bytes(p)
    return out


def rle1_symbols(text):
    """how many symbols bzip2's first run-length step makes of text (runs of 4 .. 255 become four bytes and a count)"""
    n, i = 0, 0
    while i < len(text):
        j = i
        while j < len(text) and text[j] == text[i] and j - i < 255:
            j += 1
        n += j - i if j - i < 4 else 5
        i = j
    return n


def block_counter(work_dir):
    """count(file) -> blocks of a valid file as bzip2_serial.hpp counts them on the host: tests/helpers/bzip2_harness.cpp, built into
    work_dir without the sanitizers"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(work_dir), "bzip2_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(root, "tests/helpers/bzip2_harness.cpp")], check=True)

    def count(blob):
        src, dst = os.path.join(str(work_dir), "count-in.bz2"), os.path.join(str(work_dir), "count-out.bin")
        with open(src, "wb") as f:
            f.write(blob)
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, check=True)
        rep = dict(f.split("=") for f in p.stdout.split())
        assert rep["taken"] == "1", rep
        return int(rep["blocks"])
    return count


def libbz2_says(blob):
    """the text libbz2 makes of blob, or None where it refuses"""
    try:
        return bz2.decompress(blob)
    except (OSError, ValueError, EOFError):
        return None
