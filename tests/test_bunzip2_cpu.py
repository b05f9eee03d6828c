"""merkurio_amd/csrc/codec/bzip2_serial.hpp and bzip2_stream.hpp -- the bzip2 block decoder that the kernels of bzip2_inflate.hip run,
and the host's walk over the table of magics -- compiled for the host into a stand-alone program (tests/helpers/bzip2_harness.cpp) with
-fsanitize=address,undefined, and checked against Python's bz2 (libbz2, what the CLI's host path binds and what the reference reads
.bz2 with through needletail, src/cmd_extract.rs:281).  No GPU.  Every valid file must be taken with libbz2's text; every damaged one
must be handed back, and the sanitizers must stay silent on all of them."""
import os
import subprocess

import pytest

import bzip2_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bzip2") / "bzip2_harness")
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
    rep = dict(f.split("=") for f in p.stdout.split())
    return rep, out.read_bytes()


@pytest.mark.parametrize("name", sorted(cases.valid()))
def test_valid_files_are_taken_with_libbz2s_text(harness, tmp_path, name):
    blob, text = cases.valid()[name]
    assert cases.libbz2_says(blob) == text
    rep, got = run(harness, tmp_path, blob)
    assert rep["taken"] == "1", (name, rep)
    assert got == text and int(rep["bytes"]) == len(text), name
    magics = cases.find_magics(blob) if len(blob) < 60000 else None
    if magics is not None:
        assert int(rep["blocks"]) == sum(1 for _, k in magics if k == 0) and int(rep["streams"]) == sum(k for _, k in magics)
    if name.startswith("empty"):
        assert rep["blocks"] == "0" and rep["streams"] == "1"


def test_block_starts_at_any_bit_and_a_run_may_end_a_block(harness, tmp_path):
    """350 KB at level 1 are four blocks, at least one of which does not start on a byte; the run of 1 000 of the run-length corpus
    ends the first block of its level-1 file with a count byte"""
    rep, _ = run(harness, tmp_path, cases.valid()["four-blocks-l1"][0])
    assert rep["taken"] == "1" and int(rep["blocks"]) == 4 and int(rep["unaligned"]) >= 1, rep
    rep, _ = run(harness, tmp_path, cases.valid()["rle-l1"][0])
    assert rep["taken"] == "1" and int(rep["blocks"]) == 2 and int(rep["runend"]) >= 1, rep
    for name, streams in (("two-streams", 2), ("three-streams", 3), ("streams-with-an-empty-one", 4)):
        rep, _ = run(harness, tmp_path, cases.valid()[name][0])
        assert rep["taken"] == "1" and int(rep["streams"]) == streams, (name, rep)


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_files_are_handed_back(harness, tmp_path, name):
    rep, got = run(harness, tmp_path, cases.damaged()[name])
    assert rep["taken"] == "0" and got == b"", (name, rep)


def test_patched_headers_are_refused_for_what_was_patched(harness, tmp_path):
    """the bit-level patcher hits the field it means: the decoder names that refusal (codes of bzip2_serial.hpp)"""
    want = {"patched-randomised": -2, "patched-origptr-nblock": -3, "patched-ngroups-1": -4, "patched-ngroups-7": -4}
    for name, status in want.items():
        rep, _ = run(harness, tmp_path, cases.damaged()[name])
        assert rep["why"] == "block" and int(rep["status"]) == status, (name, rep)
    # and one symbol less than nblock is a valid origPtr as far as the header goes: the CRC is what refuses that file
    blob = bytearray(cases.damaged()["patched-origptr-nblock"])
    lay = cases.block_layout(bytes(blob), 32)
    cases.put_bits(blob, lay["orig_ptr"], 24, cases.get_bits(blob, lay["orig_ptr"], 24) - 1)
    rep, _ = run(harness, tmp_path, bytes(blob))
    assert rep["taken"] == "0" and rep["why"] == "block-crc", rep
