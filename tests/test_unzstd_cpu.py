"""merkurio_amd/csrc/codec/zstd_serial.hpp, zstd_plan.hpp and xxh64.hpp -- the Zstandard block decoder that the kernels of
zstd_inflate.hip run, the host's walk over frames and block headers, the scans and the checksum -- compiled for the host into a
stand-alone program (tests/helpers/zstd_harness.cpp) with -fsanitize=address,undefined, and checked against libzstd (the system's
libzstd.so.1, what the CLI's host path binds and what the reference reads .zst with through needletail, src/cmd_extract.rs:281).  No
GPU.  Every valid file must be taken with libzstd's text; every damaged one must be an error to libzstd and be handed back; the
sanitizers must stay silent on all of them; and the census the harness prints proves that the cases exercise what their names claim."""
import ctypes as C
import os
import re

import pytest

import zstd_cases as cases
import zstd_craft as craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return cases.build_harness(tmp_path_factory.mktemp("zstd"), sanitize=True)


@pytest.fixture(scope="module")
def reports(harness, tmp_path_factory):
    """the harness's report on every valid file, made once"""
    work = tmp_path_factory.mktemp("zstd-valid")
    return {name: cases.run_harness(harness, work, blob) for name, (blob, _) in cases.valid().items()}


@pytest.mark.parametrize("name", sorted(cases.valid()))
def test_valid_files_are_taken_with_libzstds_text(reports, name):
    blob, text = cases.valid()[name]
    assert cases.libzstd_says(blob) == text
    rep, got = reports[name]
    assert rep["taken"] == "1", (name, rep)
    assert got == text and int(rep["bytes"]) == len(text), name


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_files_are_an_error_to_libzstd_and_handed_back(harness, tmp_path, name):
    blob = cases.damaged()[name]
    assert cases.libzstd_says(blob) is None, name
    rep, got = cases.run_harness(harness, tmp_path, blob)
    assert rep["taken"] == "0" and got == b"", (name, rep)


def test_patched_files_are_refused_for_what_was_patched(harness, tmp_path):
    """the patches hit the field they mean: the decoder names that refusal (codes of zstd_serial.hpp)"""
    want = dict(cases.PATCHED_STATUS)
    want.update(craft.PATCHED_STATUS)
    want.update({"flip-content-size": -19, "flip-checksum": -20, "trailing-garbage": -21, "cut-in-checksum": -1})
    for name, status in sorted(want.items()):
        rep, _ = cases.run_harness(harness, tmp_path, cases.damaged()[name])
        assert int(rep["status"]) == status, (name, rep)


def test_the_checksum_is_xxh64_as_libzstd_computes_it(harness, tmp_path):
    """every valid file with a checksum is taken (above); one text-affecting bit flipped in a raw block: both refuse, this decoder for
    the checksum"""
    blob, _ = cases.valid()["raw-block"]
    at, size, typ = cases.first_block(blob)
    assert typ == 0
    bad = cases.flip(blob, (at + 3 + size // 2) * 8 + 1)
    assert cases.libzstd_says(bad) is None
    rep, _ = cases.run_harness(harness, tmp_path, bad)
    assert rep["taken"] == "0" and rep["why"] == "checksum", rep


# what at least one valid case must exercise: every key of the harness's census but these two, which are figures, not classes (both
# are asserted per case below)
NOT_REQUIRED = {"offset-at-window", "max-seq"}


def test_every_entry_of_the_census_is_hit_by_a_valid_case(reports):
    total = {}
    for name, (rep, _) in reports.items():
        for key, value in rep.items():
            if re.match(r"(block|lit|litfmt|streams|huf|mode|repeat|seqcount|fcs|rep|rep-at-block-start)\.|single-segment|skippable|empty-frames|checksums", key):
                total[key] = total.get(key, 0) + int(value)
    print(sorted(total.items()))
    assert len(total) >= 67
    missing = sorted(k for k, v in total.items() if v == 0 and k not in NOT_REQUIRED)
    assert not missing, missing


def test_the_cases_are_what_their_names_say(reports):
    r = {name: rep for name, (rep, _) in reports.items()}
    assert int(r["many-sequences"]["max-seq"]) >= 0x7F00 and int(r["many-sequences"]["seqcount.3"]) == 1
    assert int(r["crafted-127-sequences"]["seqcount.1"]) == 1 and int(r["crafted-128-sequences"]["seqcount.2"]) == 1
    assert int(r["long-match"]["max-ml"]) > 65538 and int(r["long-literals"]["max-ll"]) > 65535
    assert int(r["far-match"]["offset-at-window"]) >= 1
    assert int(r["chain-40"]["blocks"]) == 40 and int(r["chain-40"]["rounds"]) == 6
    # one stream below 256 LITERALS, four from there on (the FASTQ texts of these sizes have matches and stay below)
    for size, one, four in ((255, 1, 0), (256, 0, 1), (257, 0, 1)):
        rep = r["literals-%d" % size]
        assert (int(rep["streams.1"]), int(rep["streams.4"]), int(rep["seqcount.0"]), int(rep["lit.huffman"])) == (one, four, 1, 1), (size, rep)
    assert int(r["size-131072"]["blocks"]) == 1 and int(r["size-131073"]["blocks"]) == 2
    assert int(r["direct-weights"]["huf.direct"]) >= 1 and int(r["fastq-l3"]["huf.fse"]) >= 1
    assert int(r["raw-block"]["block.raw"]) >= 1 and int(r["crafted-rle-block"]["block.rle"]) == 1
    assert int(r["size-0"]["blocks"]) == 0 and int(r["size-0"]["empty-frames"]) == 1
    assert int(r["three-frames"]["frames"]) == 3 and int(r["skippable-around"]["skippable"]) == 3
    for t in ("ll", "of", "ml"):
        assert int(r["crafted-modes-rle-then-repeat"]["repeat.%s.of-rle" % t]) >= 1
        assert int(r["crafted-modes-predefined-then-repeat"]["repeat.%s.of-predefined" % t]) >= 1
        assert int(r["crafted-modes-fse-then-repeat"]["repeat.%s.of-fse" % t]) >= 1
    for v in (1, 2, 3):
        for z in ("ll", "ll0"):
            assert int(r["crafted-repeat-%d-%s-at-block-start" % (v, z)]["rep-at-block-start.%d.%s" % (v, z)]) == 1


def test_the_entries_are_declared_bound_exported_and_refuse_null():
    from merkurio_amd import native as mk
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"int mk_zstd_inflate_device\(mk_codec \*c, const uint8_t \*zs, uint64_t n, uint64_t \*text_bytes, uint32_t \*taken, uint64_t \*n_blocks\);", hdr)
    assert re.search(r"int mk_zstd_info\(const mk_codec \*c, uint32_t \*blocks, uint32_t \*frames, uint32_t \*rounds, float ms\[6\]\);", hdr)
    L = mk.load()
    for name in ("mk_zstd_inflate_device", "mk_zstd_info"):
        assert name in mk.EXPORTS and hasattr(L, name), name
    assert hasattr(mk.Codec, "unzstd") and hasattr(mk.Codec, "unzstd_info")
    n, taken, blocks = C.c_uint64(7), C.c_uint32(7), C.c_uint64(7)
    blob = (C.c_uint8 * 32)()
    assert L.mk_zstd_inflate_device(None, blob, 32, C.byref(n), C.byref(taken), C.byref(blocks)) == mk.MK_E_INVALID_ARG
    assert L.mk_zstd_info(None, None, None, None, None) == mk.MK_E_INVALID_ARG
