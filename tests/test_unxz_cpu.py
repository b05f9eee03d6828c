"""merkurio_amd/csrc/codec/lzma_serial.hpp, xz_plan.hpp and crc64.hpp -- the LZMA2 block decoder that the kernel of xz_inflate.hip runs,
the host's walk over an .xz file and the two CRCs -- compiled for the host into a stand-alone program (tests/helpers/xz_harness.cpp)
with -fsanitize=address,undefined, and checked against liblzma (the stdlib's lzma module).  No GPU.  Every valid file must be taken
with liblzma's text; every damaged one must be an error to liblzma and be handed back; the sanitizers must stay silent on all of
them; and the census the harness prints must have no empty cell: the crafted files reach every branch of the decoder."""
import ctypes as C
import os
import re

import pytest

import xz_cases as cases
import xz_craft as craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return cases.build_harness(tmp_path_factory.mktemp("xz"), sanitize=True)


@pytest.fixture(scope="module")
def reports(harness, tmp_path_factory):
    """the harness's report on every valid file, made once"""
    work = tmp_path_factory.mktemp("xz-valid")
    return {name: cases.run_harness(harness, work, blob) for name, (blob, _) in cases.valid().items()}


@pytest.mark.parametrize("name", sorted(cases.valid()))
def test_valid_files_are_taken_with_liblzmas_text(reports, name):
    blob, text = cases.valid()[name]
    assert cases.liblzma_says(blob) == text
    rep, got = reports[name]
    assert rep["taken"] == "1", (name, rep)
    assert got == text and int(rep["bytes"]) == len(text), name


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_files_are_an_error_to_liblzma_and_handed_back(harness, tmp_path, name):
    blob = cases.damaged()[name]
    assert cases.liblzma_says(blob) is None, name
    rep, got = cases.run_harness(harness, tmp_path, blob)
    assert rep["taken"] == "0" and int(rep["status"]) < 0 and got == b"", (name, rep)


# the refusal each crafted damage must be named with (codes of xz_plan.hpp and lzma_serial.hpp)
NAMED = {"flip-stream-header": -3, "flip-block-header": -10, "flip-check": -31, "flip-index": -7, "flip-footer": -4, "cut-stream-header": -1,
         "trailing-bytes": -4, "trailing-zeros-not-a-multiple-of-4": -11, "index-stored-size-off-by-one": -8, "index-text-size-off-by-one": -8,
         "backward-size-wrong": -5, "block-padding-not-zero": -11, "distance-one-past-the-text": -27, "shortrep-at-the-first-byte": -27,
         "distance-one-past-the-dictionary": -27, "chunk-states-one-byte-less": -25, "chunk-states-one-byte-more": -25, "final-code-not-zero": -29,
         "first-range-coder-byte-not-zero": -26, "control-byte-0x03": -20, "lc-plus-lp-5": -23, "first-chunk-without-dictionary-reset": -21,
         "first-lzma-chunk-without-props": -22, "end-of-payload-marker-mid-chunk": -28}


def test_damaged_files_are_refused_for_what_was_damaged(harness, tmp_path):
    for name, status in sorted(NAMED.items()):
        rep, _ = cases.run_harness(harness, tmp_path, cases.damaged()[name])
        assert int(rep["status"]) == status, (name, rep)


@pytest.mark.parametrize("name", sorted(cases.handed_back()))
def test_valid_files_of_other_kinds_are_handed_back_by_name(harness, tmp_path, name):
    blob, text, status = cases.handed_back()[name]
    assert cases.liblzma_says(blob) == text
    rep, got = cases.run_harness(harness, tmp_path, blob)
    assert rep["taken"] == "0" and int(rep["status"]) == status and got == b"", (name, rep)


def test_the_spread_rule(harness, tmp_path):
    """largest block's text x K <= the whole text, or the file is liblzma's"""
    blob, text = cases.blocks_of([3000, 1000])
    for spread, taken in ((1, "1"), (2, "0")):
        rep, _ = cases.run_harness(harness, tmp_path, blob, spread)
        assert rep["taken"] == taken and int(rep["status"]) == (0 if taken == "1" else cases.XZ_SPREAD), (spread, rep)
    for sizes, taken in (([2000, 2000], "1"), ([2001, 1999], "0")):  # K = 2 just admits, just refuses
        rep, _ = cases.run_harness(harness, tmp_path, cases.blocks_of(sizes)[0], 2)
        assert rep["taken"] == taken, (sizes, rep)
    rep, _ = cases.run_harness(harness, tmp_path, cases.valid()["preset-6"][0], 16)
    assert rep["taken"] == "0" and int(rep["status"]) == cases.XZ_SPREAD  # a single block
    rep, _ = cases.run_harness(harness, tmp_path, cases.valid()["empty"][0], 16)
    assert rep["taken"] == "1"


def test_every_cell_of_the_census_is_reached_by_a_valid_case(reports):
    total = {}
    for name, (rep, _) in reports.items():
        for key, value in rep.items():
            if re.match(r"(packet|len|slot|chunk|dist)\.", key):
                total[key] = total.get(key, 0) + int(value)
    print(sorted(total.items()))
    assert len(total) == 23
    assert not sorted(k for k, v in total.items() if v == 0)


def test_the_cases_are_what_their_names_say(reports):
    r = {name: rep for name, (rep, _) in reports.items()}
    assert int(r["3000-blocks"]["blocks"]) == 3000 and int(r["40-blocks"]["blocks"]) == 40 and int(r["empty"]["blocks"]) == 0
    assert int(r["two-streams-pad-8"]["streams"]) == 2 and int(r["mixed-checks"]["streams"]) == 5
    assert int(r["distances"]["slot.direct"]) >= 4 and int(r["distances"]["slot.tree"]) >= 10 and int(r["distances"]["slot.align"]) >= 3
    assert int(r["distances"]["dist.at-dict"]) >= 1 and int(r["dict-4k"]["dist.at-dict"]) == 2 and int(r["dict-4k"]["dist.at-start"]) == 1
    assert int(r["lengths"]["len.low"]) == 4 and int(r["lengths"]["len.mid"]) == 4 and int(r["lengths"]["len.high"]) == 6
    for k in ("rep0", "rep1", "rep2", "rep3", "shortrep"):
        assert int(r["reps"]["packet." + k]) >= 4, k
    assert int(r["stored-only"]["chunk.stored-reset"]) == 1 and int(r["stored-only"]["chunk.stored"]) == 1 and int(r["stored-only"]["packet.lit"]) == 0
    m = r["mixed-chunks"]
    assert [int(m["chunk." + k]) for k in ("all", "props", "state", "lzma", "stored", "stored-reset")] == [2, 3, 1, 1, 1, 1]
    assert int(r["mixed-chunks"]["lclp"]) == 4 and int(r["props-0-4-4"]["lclp"]) == 4 and int(r["props-0-0-0"]["lclp"]) == 0
    assert int(r["chunk-2MiB-zeros"]["bytes"]) == 2 << 20 and int(r["chunk-2MiB-zeros"]["chunk.all"]) == 1
    assert int(r["chunk-edges"]["chunk.lzma"]) >= 11


@pytest.mark.parametrize("pieces", [1, 2, 63, 64, 65])
def test_the_crc_fold_equals_the_bytewise_crc(harness, tmp_path, pieces):
    """pieces folded by the carry-less multiply-mod, as mk_xz_check_kernel folds a block's 64: CRC-64 and CRC-32, against the bytewise
    loop of the same header and against xz_craft's / zlib's"""
    import subprocess
    import zlib
    for n in (0, 1, 7, 8, 9, 1000):
        data = cases.rnd(n, n + 1)
        path = tmp_path / "d.bin"
        path.write_bytes(data)
        p = subprocess.run([harness, "--fold", str(path), str(pieces)], capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        rep = dict(f.split("=") for f in p.stdout.split())
        assert rep["fold64"] == rep["crc64"] == "%016x" % craft.crc64(data), (n, pieces, rep)
        assert rep["fold32"] == rep["crc32"] == "%08x" % zlib.crc32(data), (n, pieces, rep)


def test_the_entries_are_declared_bound_exported_and_refuse_null():
    from merkurio_amd import native as mk
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"int mk_xz_inflate_device\(mk_codec \*c, const uint8_t \*xz, uint64_t n, uint64_t \*text_bytes, uint32_t \*taken, uint64_t \*n_blocks\);", hdr)
    assert re.search(r"int mk_xz_info\(const mk_codec \*c, uint32_t \*blocks, uint32_t \*streams, uint32_t \*status, uint64_t \*largest_block_text, float ms\[4\]", hdr)
    L = mk.load()
    for name in ("mk_xz_inflate_device", "mk_xz_info", "mk_codec_set_xz_spread"):
        assert name in mk.EXPORTS and hasattr(L, name), name
    assert hasattr(mk.Codec, "unxz") and hasattr(mk.Codec, "unxz_info") and hasattr(mk.Codec, "set_xz_spread")
    n, taken, blocks = C.c_uint64(7), C.c_uint32(7), C.c_uint64(7)
    blob = (C.c_uint8 * 32)()
    assert L.mk_xz_inflate_device(None, blob, 32, C.byref(n), C.byref(taken), C.byref(blocks)) == mk.MK_E_INVALID_ARG
    assert L.mk_xz_info(None, None, None, None, None, None) == mk.MK_E_INVALID_ARG
