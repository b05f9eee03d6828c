"""bzip2_serial.hpp and bzip2_stream.hpp on the host (tests/helpers/bzip2_harness.cpp under -fsanitize=address,undefined) on the
hand-made streams of tests/bzip2_craft.py: what libbz2's encoder never writes.  libbz2 is the judge (the craft module has checked
every case's prefix against it at import): an `ok-` case is taken with libbz2's text and the stated number of blocks, a `bad-` case
(libbz2 refuses it) and a `host-` case (libbz2 takes it; the decoder documents that it does not) are handed back with no text, the
cases that aim at one rule for that rule, and the sanitizers stay silent.  No GPU."""
import os
import subprocess

import pytest

import bzip2_craft as craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bzip2craft") / "bzip2_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe, os.path.join(ROOT, "tests/helpers/bzip2_harness.cpp")], check=True)
    return exe


def run(harness, tmp_path, blob):
    """-> (the report's fields, the text written)"""
    src, out = tmp_path / "in.bz2", tmp_path / "out.bin"
    src.write_bytes(blob)
    p = subprocess.run([harness, str(src), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    return dict(f.split("=") for f in p.stdout.split()), out.read_bytes()


def test_the_cases_per_prefix():
    n = craft.counts()
    print("hand-made bzip2 cases:", n)
    assert n["ok-"] + n["bad-"] + n["host-"] == len(craft.CASES) and all(n.values())
    host = [name for name in craft.CASES if name.startswith("host-")]
    assert all(any(w in name for w in ("randomised", "selectors-18003", "magic-in-the-symbols", "magic-in-the-selectors")) for name in host), host
    assert any("selectors-18003" in name for name in craft.CASES)


@pytest.mark.parametrize("name", sorted(craft.CASES))
def test_case(harness, tmp_path, name):
    blob, blocks, _ = craft.CASES[name]
    rep, got = run(harness, tmp_path, blob)
    if name.startswith("ok-"):
        text = craft.text_of(name)
        assert rep["taken"] == "1", (name, rep)
        assert got == text and int(rep["bytes"]) == len(text), name
        assert int(rep["blocks"]) == blocks and int(rep["unaligned"]) == craft.unaligned_blocks(blob), (name, rep)
    else:
        assert rep["taken"] == "0" and got == b"", (name, rep)
        if name in craft.WHY:
            why, status = craft.WHY[name]
            assert rep["why"] == why and (status is None or int(rep["status"]) == status), (name, rep)


def sweep(harness, tmp_path, files):
    for label, blob, text, blocks in files:
        rep, got = run(harness, tmp_path, blob)
        assert rep["taken"] == "1", (label, rep)
        assert got == text, label
        magics = craft.find_magics(blob)
        assert int(rep["blocks"]) == blocks == sum(1 for _, k in magics if k == 0), (label, rep)
        assert int(rep["streams"]) == sum(k for _, k in magics) and int(rep["unaligned"]) == craft.unaligned_blocks(blob), (label, rep)


def test_second_block_at_every_bit_phase(harness, tmp_path):
    sweep(harness, tmp_path, craft.sweep_spare_selectors())


def test_end_magic_and_crc_end_the_file_at_every_bit_phase(harness, tmp_path):
    sweep(harness, tmp_path, craft.sweep_end_magic())


def test_second_block_around_bytes_256_and_1024(harness, tmp_path):
    files = craft.sweep_window_seams()
    assert len(files) == 2 * 81
    sweep(harness, tmp_path, files)


def test_runs_and_counts_around_a_turn_of_64_and_short_texts(harness, tmp_path):
    sweep(harness, tmp_path, craft.sweep_expand())
