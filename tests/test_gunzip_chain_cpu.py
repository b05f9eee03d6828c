"""merkurio_amd/csrc/codec/gzip_chain.hpp -- the host's part of the gzip proof (which guessed member start is real, which found block
start is dropped, where a window ends, when a file is handed back to zlib) -- compiled for the host into a stand-alone program
(tests/helpers/gzip_chain_harness.cpp) with -fsanitize=address,undefined.  The harness plays the device with the serial decoder of
gzip_segments.hpp and runs the round loop that gzip_host.cpp runs between its kernels.  No GPU.  The files, the modes (one shot over
all members, windows of 16 / 64 / 256 KiB), the chunk and the assertions are those of test_gpu_gunzip_members.py and
test_gpu_gunzip_windows.py; zlib is the checker.

The harness confirms a block start by decoding its whole block, the search kernel by 2 048 dry symbols: the two may keep different
starts.  No verdict and no text below depends on that -- a start is only ever USED once the piece in front of it has landed on it --
and no case is treated differently for it; piece counts are therefore not asserted here (the GPU tests assert the device's)."""
import os
import subprocess

import pytest

import deflate_craft as craft
import gunzip_members_cases as gm
import gunzip_windows_cases as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0,) + gw.WINDOWS  # 0 = one shot
# the files made of the ~2 MB member: one shot and the 256 KiB window (the smaller windows search every byte several times over,
# which takes the serial decoder under the sanitizers too long; every other file runs in all modes)
LARGE = ("fastq-one-member-2mb", "bit-flipped-in-window-3-of-8", "last-crc-wrong", "last-isize-wrong", "bytes-behind-the-last-member")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gzip_chain") / "gzip_chain_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe, os.path.join(ROOT, "tests/helpers/gzip_chain_harness.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def verdicts():
    return gw.verdicts()


def run(harness, tmp_path, blob, window):
    """-> (the report's fields as numbers, the text delivered)"""
    src, out = tmp_path / "in.gz", tmp_path / "out.bin"
    src.write_bytes(blob)
    p = subprocess.run([harness, str(src), str(window), str(craft.GUNZIP_CHUNK), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    return {k: int(v) for k, v in (f.split("=") for f in p.stdout.split())}, out.read_bytes()


def check(harness, tmp_path, verdicts, name, blob, expect, window):
    text, ok, members = verdicts[name]
    rep, got = run(harness, tmp_path, blob, window)
    print(name, window, expect, "->", rep, len(got), "of", len(text))
    if window == 0:  # test_gpu_gunzip_members.py's check: zlib's text and zlib's members, or not taken -- never another text
        if expect == "handed-back":
            assert not ok and not rep["taken"] and got == b"", name
        elif expect == "taken":
            assert rep["taken"], (name, "not taken", rep)
        if rep["taken"]:
            assert ok and got == text and rep["members"] == members, (name, rep)
        else:
            assert got == b"", name
        return rep, got
    # test_gpu_gunzip_windows.py's check
    assert rep["state"] in (1, 2), name
    assert got == text[:len(got)], (name, window)  # never another text; before a hand-back: zlib's prefix
    if rep["state"] == 1:
        assert ok and got == text and rep["members"] == members, (name, window, rep)
    if expect == "taken":
        assert rep["state"] == 1, (name, window, rep)
    elif expect == "handed-back":
        assert rep["state"] == 2 and not ok, (name, window, rep)
    return rep, got


@pytest.mark.parametrize("window", MODES)
def test_every_file_of_several_members(harness, tmp_path, verdicts, window):
    """every case of gunzip_members_cases.py: taken with zlib's text and zlib's number of members, handed back where zlib refuses, or
    either -- in one shot (a file with bytes behind its last member: not taken) and through windows"""
    assert len(gm.cases()) >= 40
    for name, blob, expect in gm.cases():
        check(harness, tmp_path, verdicts, name, blob, expect, window)
    for blob in (b"no gzip file\n" * 5, b""):
        rep, got = run(harness, tmp_path, blob, window)
        assert not rep["taken"] and rep["state"] == 2 and got == b""


@pytest.mark.parametrize("window", MODES)
def test_every_file_of_the_window_cases(harness, tmp_path, verdicts, window):
    """every file of gunzip_windows_cases.py: contexts across cuts, member boundaries and headers at window ends, false headers on both
    sides of a cut, hand-backs that deliver zlib's prefix, distances in front of a continued member"""
    for name, (blob, expect) in gw.files().items():
        if name in LARGE and window not in (0, 256 << 10):
            continue
        rep, got = check(harness, tmp_path, verdicts, name, blob, expect, window)
        if name == "fastq-one-member-2mb" and window == 256 << 10:
            assert rep["windows"] >= 6 and rep["members"] == 1, rep
        if name in ("far-matches", "sync-flush-every-3k", "names-copy-the-previous") and window == 16 << 10:
            assert rep["windows"] >= 4, (name, rep)
        # The three "match-reaches-..." files are the ones whose WINDOW COUNT depends on the confirm: their second block runs from
        # ~10 KB to ~21 KB of the stream, past the end of the first 16 KiB upload.  The kernel's 2 048 dry symbols confirm its start
        # inside that upload, so the device cuts there and resolves the match through the carry (the GPU test asserts windows >= 2);
        # the whole-block confirm cannot decode the block to its end inside the upload, finds no start, and the window grows until it
        # holds the file.  Verdict and text are the same either way and are asserted above; the carry is exercised here by the
        # files asserted to take four windows and more.
        if name == "many-windows-between-two-of-one-piece" and window == 64 << 10:
            assert rep["members"] == 3 and rep["windows"] >= 6, rep
        if name == "empty-members-among-long-ones" and window == 16 << 10:
            assert rep["members"] == 6, rep


def test_false_guesses_cost_rounds_not_the_file(harness, tmp_path, verdicts):
    """whole members planted in a stored block are guesses that the rounds drop: the decode is repeated, the file is taken"""
    name, blob, expect = [c for c in gm.cases() if c[0] == "false-guess-two-whole-members-apart"][0]
    rep, _ = check(harness, tmp_path, verdicts, name, blob, expect, 0)
    assert rep["taken"] and rep["repeated"] >= 1 and rep["members"] == 2, rep


def test_the_one_shot_calls_refuse_a_member_of_4_gib(harness):
    """the ISIZE rule on made-up lengths: one shot -- exact and below 4 GiB; a window -- modulo 2^32 with what the member had before"""
    def agrees(text, before, isize, whole):
        p = subprocess.run([harness, "--isize", str(text), str(before), str(isize), str(int(whole))], capture_output=True, text=True, check=True)
        assert not p.stderr
        return p.stdout.strip() == "agrees=1"
    assert agrees(1000, 0, 1000, True) and not agrees(1000, 0, 1001, True)
    assert agrees((1 << 32) - 1, 0, (1 << 32) - 1, True)
    assert not agrees(1 << 32, 0, 0, True) and not agrees((1 << 32) + 5, 0, 5, True)  # 4 GiB or more: refused, whatever ISIZE says
    assert agrees(1 << 32, 0, 0, False) and agrees((1 << 32) + 5, 0, 5, False)
    assert agrees(5, (1 << 33) - 2, 3, False) and not agrees(5, (1 << 33) - 2, 4, False)  # with the windows before
