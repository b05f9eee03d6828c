"""merkurio_amd/csrc/codec/zstd_chain.hpp -- what the host decides about a window of mk_zstd_stream_*: the resumable walk, the carry
(tables as description bytes in a prelude, the three repeat offsets, the history, the running XXH64), the scans from a carried start --
compiled for the host into a stand-alone program (tests/helpers/zstd_windows_harness.cpp) with -fsanitize=address,undefined and run
with the serial decoder of zstd_serial.hpp.  No GPU.  Every valid file gives libzstd's text at one block per window, at windows of
1000 compressed bytes, at a text cap of one block, and with the first seam behind every block in turn; the census proves that the
seams cut everything a block can need of the blocks in front of it; every damaged file ends in state 2 behind a prefix of the text;
and zs_plan, now the resumable walk run once, yields the block table it yielded before the split."""
import ctypes as C
import json
import os
import re

import pytest

import zstd_cases as cases
import zstd_craft as craft
import zstd_windows_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return wc.build_harness(tmp_path_factory.mktemp("zstd-windows"), sanitize=True)


@pytest.fixture(scope="module")
def reports(harness, tmp_path_factory):
    """(name, setting) -> the harness's report and text, made once"""
    work = tmp_path_factory.mktemp("zstd-windows-valid")
    return {(name, s): wc.run_harness(harness, work, blob, *s) for name, (blob, _) in wc.all_valid().items() for s in wc.SETTINGS}


@pytest.mark.parametrize("name", sorted(wc.all_valid()))
def test_every_setting_gives_libzstds_text(reports, name):
    blob, text = wc.all_valid()[name]
    assert cases.libzstd_says(blob) == text
    for s in wc.SETTINGS:
        rep, got = reports[(name, s)]
        assert rep["state"] == "1" and got == text, (name, s, rep)
        if s[0] == "sweep":
            assert rep["same"] == "1" and int(rep["seams"]) == max(0, int(rep["blocks"]) - 1), (name, rep)
        else:
            assert int(rep["text"]) == len(text) and int(rep["consumed"]) == len(blob), (name, s, rep)
    one, _ = reports[(name, wc.SETTINGS[0])]
    if one["windows-blocks"] != "-":  # one block per window: no window has two
        assert max(int(b) for b in one["windows-blocks"].split(",")) <= 1, one


# what the seams must have cut at least once, summed over all files and settings
REQUIRED = ["seam.treeless", "seam.frame-end", "seam.skippable", "seam.two-frames", "seam.checksum-3-windows", "seam.history-below-window",
            "seam.history-at-window", "seam.match-below-window", "seam.match-at-window", "seam.rep-first.1", "seam.rep-first.2", "seam.rep-first.3"]
REQUIRED += ["seam.repeat.%s.of-%s" % (t, m) for t in ("ll", "of", "ml") for m in ("rle", "fse")]


def test_the_seams_cut_everything_a_block_needs(reports):
    total = {}
    for rep, _ in reports.values():
        for key, value in rep.items():
            if key.startswith("seam."):
                total[key] = total.get(key, 0) + int(value)
    print(sorted(total.items()))
    missing = [k for k in REQUIRED if total.get(k, 0) == 0]
    assert not missing, missing


def test_the_cases_are_what_their_names_say(reports):
    one = wc.SETTINGS[0]
    r = reports[("far-match", one)][0]  # a 1 KiB window: behind 1 KiB of text the history is the window
    assert int(r["seam.history-at-window"]) >= 1 and int(r["max-history"]) == 1024, r
    r = reports[("windows-fastq-wlog10-l19", one)][0]  # (pieces of 1500 bytes: behind the first block the history is the window already)
    assert int(r["seam.history-at-window"]) >= 3 and int(r["seam.match-at-window"]) >= 1 and int(r["seam.history-below-window"]) == 0, r
    r = reports[("windows-fastq-wlog17-l3", one)][0]
    assert int(r["seam.match-below-window"]) >= 1 and int(r["seam.checksum-3-windows"]) == 1 and int(r["windows"]) >= 3, r
    r = reports[("windows-skippable-between-frames", one)][0]
    assert int(r["seam.skippable"]) >= 1 and int(r["seam.frame-end"]) >= 1 and int(r["frames"]) == 2, r
    r = reports[("three-frames", wc.SETTINGS[2])][0]  # (frames of one block each under a cap of one block: a window per frame)
    assert int(r["frames"]) == 3, r
    r = reports[("three-frames", ("sweep",))][0]
    assert int(r["seam.two-frames"]) >= 1, r
    for t in ("ll", "of", "ml"):
        assert int(reports[("crafted-modes-rle-then-repeat", one)][0]["seam.repeat.%s.of-rle" % t]) >= 1
        assert int(reports[("crafted-modes-fse-then-repeat", one)][0]["seam.repeat.%s.of-fse" % t]) >= 1
    for v in (1, 2, 3):
        for z in ("ll", "ll0"):
            assert int(reports[("crafted-repeat-%d-%s-at-block-start" % (v, z), one)][0]["seam.rep-first.%d" % v]) == 1
    # every window behind the first copies out of the history and nothing waits for a round
    r = reports[("windows-matches-into-history-only", one)][0]
    assert int(r["windows"]) == 4 and int(r["rounds"]) == 0 and int(r["settled-bytes"]) >= 3 * 100000, r


def test_the_whole_file_in_one_window_is_the_one_shot_decoder(harness, tmp_path):
    """blocks, frames and rounds of a stream of one window are those of tests/helpers/zstd_harness.cpp"""
    old = cases.build_harness(tmp_path, sanitize=False)
    for name in ("chain-40", "fastq-l3-checksum", "three-frames", "windows-matches-into-history-only"):
        blob, text = wc.all_valid()[name]
        rep, got = wc.run_harness(harness, tmp_path, blob, "stream", wc.WHOLE, 0)
        ref, _ = cases.run_harness(old, tmp_path, blob)
        assert got == text and rep["windows"] == "1" and rep["max-history"] == "0", (name, rep)
        assert (rep["blocks"], rep["frames"], rep["rounds"]) == (ref["blocks"], ref["frames"], ref["rounds"]), (name, rep, ref)


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_files_end_in_state_2_behind_a_prefix(harness, tmp_path, name):
    blob = cases.damaged()[name]
    fq = cases.fastq(300)[:60000]  # (the text of the file the damaged ones were made from: zstd_cases.damaged)
    for s in (("stream", 1, 0), ("stream", 1000, 0), ("stream", wc.WHOLE, wc.BLOCK)):
        rep, got = wc.run_harness(harness, tmp_path, blob, *s)
        assert rep["state"] == "2", (name, s, rep)
        assert fq.startswith(got) or name.startswith("crafted-") and got == b"", (name, s, len(got))


def test_a_late_flipped_bit_hands_back_behind_the_windows_in_front_of_it(harness, tmp_path):
    blob, text = cases.valid()["fastq-l3-checksum"]
    rep, _ = wc.run_harness(harness, tmp_path, blob, "stream", 1, 0)
    assert int(rep["windows"]) >= 4
    bad = cases.flip(blob, (len(blob) - 40) * 8 + 3)  # (in the last block's sequences)
    assert cases.libzstd_says(bad) is None
    rep, got = wc.run_harness(harness, tmp_path, bad, "stream", 1, 0)
    assert rep["state"] == "2" and int(rep["windows"]) >= 3 and len(got) >= 3 * wc.BLOCK and text.startswith(got), rep
    # a wrong checksum: all blocks decode, the last window is not delivered
    bad = cases.flip(blob, len(blob) * 8 - 5)
    rep, got = wc.run_harness(harness, tmp_path, bad, "stream", 1, 0)
    assert rep["state"] == "2" and text.startswith(got) and len(got) < len(text), rep


@pytest.mark.parametrize("name", sorted(wc.all_valid()))
def test_the_walk_resumed_behind_every_block_is_the_walk(harness, tmp_path, name):
    rep, _ = wc.run_harness(harness, tmp_path, wc.all_valid()[name][0], "plan")
    assert rep["walked"] == "1" and rep["resumed"] == "1", (name, rep)


def test_zs_plan_yields_the_block_tables_it_yielded_before_the_split(harness, tmp_path):
    """tests/golden/zstd_plan_blocks.json: blocks, frames, literal bytes, sequences and an FNV-1a hash over the ZsBlock table that
    zs_plan made of every crafted file (whose bytes no compressor's version changes) before it became the resumable walk"""
    with open(os.path.join(ROOT, "tests", "golden", "zstd_plan_blocks.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(craft.valid())
    for name, want in sorted(golden.items()):
        rep, _ = wc.run_harness(harness, tmp_path, craft.valid()[name][0], "plan")
        assert {k: rep[k] for k in want} == want, (name, rep)


def test_the_entries_are_declared_bound_exported_and_refuse_null():
    from merkurio_amd import native as mk
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"int mk_zstd_stream_begin\(mk_codec \*c, const uint8_t \*zs, uint64_t n, uint64_t window_bytes, uint32_t \*taken\);", hdr)
    assert re.search(r"int mk_zstd_stream_next\(mk_codec \*c, uint64_t \*text_bytes, uint32_t \*state\);", hdr)
    L = mk.load()
    for name in ("mk_zstd_stream_begin", "mk_zstd_stream_next", "mk_zstd_stream_info", "mk_zstd_stream_end", "mk_codec_set_zstd_text_cap"):
        assert name in mk.EXPORTS and hasattr(L, name), name
    assert hasattr(mk.Codec, "unzstd_stream") and hasattr(mk.Codec, "unzstd_stream_info")
    assert C.sizeof(mk.ZstdStreamStats) == 8 * 8 + 6 * 4
    n, taken, state = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
    blob = (C.c_uint8 * 32)()
    assert L.mk_zstd_stream_begin(None, blob, 32, 0, C.byref(taken)) == mk.MK_E_INVALID_ARG
    assert L.mk_zstd_stream_next(None, C.byref(n), C.byref(state)) == mk.MK_E_INVALID_ARG
    assert L.mk_zstd_stream_info(None, None) == mk.MK_E_INVALID_ARG
    assert L.mk_zstd_stream_end(None) == mk.MK_E_INVALID_ARG
    assert L.mk_codec_set_zstd_text_cap(None, 0) == mk.MK_E_INVALID_ARG
