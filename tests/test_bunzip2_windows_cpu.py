"""merkurio_amd/csrc/codec/bzip2_chain.hpp -- what mk_bzip2_stream_* decides about a window of a .bz2 file: the walk over the upload's
magics, the cut, the carried state, stream ends and their folded CRCs, growing, text windows -- compiled for the host with
bz2_find_markers and the serial block decoder (tests/helpers/bzip2_windows_harness.cpp) and checked against Python's bz2 (libbz2).
No GPU.  MERKURIO_TEST_SANITIZE=1 builds the harness with ASan + UBSan; the program is run directly."""
import bz2
import os
import random
import subprocess

import pytest

import bzip2_cases as cases
import bzip2_craft as craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FLAGS = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
          if os.environ.get("MERKURIO_TEST_SANITIZE") else ["-O2"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bzip2_windows") / "bzip2_windows_harness")
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-Wall", "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(ROOT, "tests/helpers/bzip2_windows_harness.cpp")], check=True)
    return exe


def _call(args):
    p = subprocess.run(args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    return dict(f.split("=") for f in p.stdout.split() if "=" in f)


def run(harness, tmp_path, blob, window, text_cap=0, max_blocks=0):
    """-> (the report's fields, the text delivered)"""
    src, out = tmp_path / "in.bz2", tmp_path / "out.bin"
    src.write_bytes(blob)
    rep = _call([harness, "run", str(src), str(out), str(window), str(text_cap), str(max_blocks)])
    rep["sizes"] = [int(x) for x in rep["sizes"].split(",")] if rep.get("sizes") else []
    return rep, out.read_bytes()


def sweep(harness, tmp_path, blob, text, first, last, step):
    src, want = tmp_path / "in.bz2", tmp_path / "want.bin"
    src.write_bytes(blob), want.write_bytes(text)
    rep = _call([harness, "sweep", str(src), str(want), str(first), str(last), str(step)])
    assert int(rep["runs"]) == len(range(first, last + 1, step))
    return rep


def four_block_stream():
    """a level-1 stream of four blocks of pseudo-random text: block magics at odd bit phases"""
    text = random.Random(31).randbytes(330000)
    blob = bz2.compress(text, 1)
    magics = cases.find_magics(blob)
    assert [k for _, k in magics] == [0, 0, 0, 0, 1] and sum(1 for bit, _ in magics if bit & 7) >= 2
    return blob, text


def libbz2_prefix(blob):
    """what a BZ2Decompressor returns, fed byte by byte from the front and stream behind stream, before it raises (or the data ends).
    (Byte by byte: the call that raises returns nothing, so what its bytes produced is lost -- with one byte that is a block at most,
    and only a block whose own end raises.)"""
    out, data = [], blob
    while data:
        d = bz2.BZ2Decompressor()
        try:
            for at in range(len(data)):
                out.append(d.decompress(data[at:at + 1]))
                if d.eof:
                    break
        except (OSError, ValueError, EOFError):
            break
        if not d.eof:
            break
        data = d.unused_data
    return b"".join(out)


VALID = sorted(cases.valid()) + ["four-random-blocks"]


@pytest.mark.parametrize("name", VALID)
def test_every_window_size_gives_libbz2s_text(harness, tmp_path, name):
    """windows of every size from 15 bytes to the file's length + 1 (files of 2 KB and more: every 97th): the windows' texts behind
    each other are bz2.decompress's, the last state is 1, and every compressed byte was consumed"""
    blob, text = four_block_stream() if name == "four-random-blocks" else cases.valid()[name]
    assert bz2.decompress(blob) == text
    rep = sweep(harness, tmp_path, blob, text, 15, len(blob) + 1, 1 if len(blob) < 2048 else 97)
    assert rep["bad"] == "0", (name, rep)


def test_a_stream_of_blocks_over_several_windows_folds_its_crc(harness, tmp_path):
    blob, text = four_block_stream()
    rep, got = run(harness, tmp_path, blob, len(blob) // 4)
    assert rep["state"] == "1" and got == text and int(rep["windows"]) >= 3 and rep["blocks"] == "4" and rep["streams"] == "1", rep
    # ... and a wrong stream CRC is found after all the text, folded over the same windows
    bad = cases.flip(blob, cases.find_magics(blob)[-1][0] + 48 + 3)
    rep, got = run(harness, tmp_path, bad, len(blob) // 4)
    assert rep["state"] == "2" and got == text and rep["streams"] == "0" and int(rep["text"]) == len(text), rep


def test_an_end_magic_as_an_uploads_last_bits(harness, tmp_path):
    """the first window ends right behind the first stream's end magic, 1 .. 10 bytes further on (CRC and padding cut off, then "BZh" +
    level cut at each of its four bytes), and further still: the end magic is the cut unless all that decides it lies inside"""
    a, b = cases.fastq(400)[:50000], cases.fastq(400, seed=9)[:40000]
    first = bz2.compress(a, 1)
    blob = first + bz2.compress(b, 9)
    end_bit = cases.find_magics(first)[-1][0]
    end_byte = (end_bit + 48 + 7) // 8  # the first byte behind the end magic
    for extra in range(0, 24):
        rep, got = run(harness, tmp_path, blob, end_byte - 4 + extra)  # (the upload starts at byte 4, the first magic)
        assert rep["state"] == "1" and got == a + b and rep["streams"] == "2", (extra, rep)
        if extra < 4 + 4 + 6:  # CRC (4), "BZh" + level (4), the next magic (6) are not all inside: the first window stops at the end magic
            assert rep["sizes"][0] == len(a) and len(rep["sizes"]) >= 2, (extra, rep)


def test_an_empty_stream_first_in_the_middle_and_last(harness, tmp_path):
    empty = bz2.compress(b"")
    a, b = b"first stream\n" * 50, b"second stream\n" * 70
    za, zb = bz2.compress(a, 1), bz2.compress(b, 9)
    for blob, text, streams in ((empty + za + zb, a + b, 3), (za + empty + zb, a + b, 3), (za + zb + empty, a + b, 3), (empty * 3, b"", 3), (empty + za + empty * 2, a, 4)):
        assert bz2.decompress(blob) == text
        rep = sweep(harness, tmp_path, blob, text, 15, len(blob) + 1, 1)
        assert rep["bad"] == "0", rep
        rep, got = run(harness, tmp_path, blob, 20)
        assert rep["state"] == "1" and got == text and int(rep["streams"]) == streams, rep
    # a window of empty streams alone is a window of 0 bytes
    rep, got = run(harness, tmp_path, empty * 4 + za, 28)
    assert rep["state"] == "1" and got == a and 0 in rep["sizes"], rep


def _damaged():
    out = dict(cases.damaged())
    out.update((name, blob) for name, (blob, _, _) in craft.CASES.items() if name.startswith("bad-"))
    return out


def _opens(blob):
    """ "BZh1-9" in front: mk_bzip2_stream_begin opens a stream for it"""
    return blob[:3] == b"BZh" and 49 <= blob[3] <= 57


def test_a_damaged_stream_header_opens_no_stream(harness, tmp_path):
    """the damaged files without "BZh1-9" in front: nothing is opened (*taken = 0), nothing is delivered, the file is libbz2's"""
    names = sorted(n for n, blob in _damaged().items() if not _opens(blob))
    assert "flip-stream-header" in names
    for name in names:
        rep, got = run(harness, tmp_path, _damaged()[name], 64)
        assert rep["state"] == "2" and got == b"" and rep["windows"] == rep["text"] == rep["uploads"] == "0", (name, rep)


@pytest.mark.parametrize("name", sorted(n for n, blob in _damaged().items() if _opens(blob)))
def test_damaged_files_end_in_state_2_after_a_prefix_of_libbz2s_text(harness, tmp_path, name):
    """window sizes that put the damage into the first, a middle and the last window: the last state is 2, what was delivered is a prefix
    of what libbz2 writes before it refuses -- never more --, and stats.text_bytes is its length"""
    blob = _damaged()[name]
    limit = libbz2_prefix(blob)
    for window in sorted({len(blob) + 1, len(blob) // 2 + 1, len(blob) // 5 + 1, 4096, 64}):
        rep, got = run(harness, tmp_path, blob, window)
        assert rep["state"] == "2", (name, window, rep)
        assert limit.startswith(got), (name, window, len(got), len(limit))
        assert int(rep["text"]) == len(got) == sum(rep["sizes"]), (name, window, rep)


def test_late_damage_leaves_the_windows_in_front_of_it(harness, tmp_path):
    blob, text = four_block_stream()
    magics = cases.find_magics(blob)
    bad = cases.flip(blob, (magics[3][0] + magics[4][0]) // 2)  # inside the last block's symbols
    good_rep, _ = run(harness, tmp_path, blob, len(blob) // 4)
    rep, got = run(harness, tmp_path, bad, len(blob) // 4)
    assert rep["state"] == "2" and text.startswith(got) and libbz2_prefix(bad).startswith(got), rep
    assert len(got) >= sum(good_rep["sizes"][:2]) > 0, (rep, good_rep)  # the windows wholly in front of the damage stand


def test_a_block_magic_planted_inside_a_blocks_data(harness, tmp_path):
    """byte-aligned, where the compressor never leaves one: the table of magics has one too many, which shows when the block does not
    end on it.  State 2 or the exact text, never a wrong text"""
    planted = [n for n in craft.CASES if "magic-in-the" in n]
    assert planted
    for name in planted:
        blob = craft.CASES[name][0]
        text = craft.libbz2_says(blob)
        for window in (15, 40, len(blob) // 2 + 1, len(blob) + 1):
            rep, got = run(harness, tmp_path, blob, window)
            assert rep["state"] in ("1", "2"), rep
            assert got == text if rep["state"] == "1" else (text or b"").startswith(got), (name, window, rep)


def test_trailing_garbage_is_state_2_after_all_the_text(harness, tmp_path):
    blob, text = cases.valid()["four-blocks-l1"]
    for window in (len(blob) // 3, len(blob) + 64):
        rep, got = run(harness, tmp_path, blob + b"\x00\x01\x02\x03", window)
        assert rep["state"] == "2" and got == text and int(rep["text"]) == len(text), rep


def test_text_windows_and_short_decodes_do_not_change_the_text(harness, tmp_path):
    """a text cap below a block's text, and a stand-in that decodes two blocks per window ("no room for more"): several text windows per
    window, each of whole blocks; the rest of the blocks is the next window's"""
    blob, text = four_block_stream()
    whole, _ = run(harness, tmp_path, blob, len(blob) + 1)
    assert whole["sizes"] == [len(text)] and whole["uploads"] == "1"
    rep, got = run(harness, tmp_path, blob, len(blob) + 1, text_cap=100000)
    assert rep["state"] == "1" and got == text and len(rep["sizes"]) == 4 and rep["uploads"] == "1", rep  # (one block per text window: none fits beside another)
    rep, got = run(harness, tmp_path, blob, len(blob) + 1, text_cap=1)
    assert rep["state"] == "1" and got == text and len(rep["sizes"]) == 4, rep  # (at least one block, whatever the cap)
    rep, got = run(harness, tmp_path, blob, len(blob) + 1, max_blocks=2)
    assert rep["state"] == "1" and got == text and len(rep["sizes"]) == 2 and rep["uploads"] == "2", rep
    zeros = bz2.compress(bytes(600000) + random.Random(2).randbytes(200000), 1)
    rep, got = run(harness, tmp_path, zeros, len(zeros) + 1, text_cap=65536)
    assert rep["state"] == "1" and got == bz2.decompress(zeros) and len(rep["sizes"]) >= 3, rep


def test_a_window_smaller_than_a_block_grows(harness, tmp_path):
    blob, text = four_block_stream()
    rep, got = run(harness, tmp_path, blob, 1000)
    assert rep["state"] == "1" and got == text and int(rep["grown"]) > 0, rep
