"""merkurio_amd/csrc/codec/xz_chain.hpp -- what the host decides about the windows of mk_xz_stream_*: the plan made when the stream
begins (greedy runs of whole blocks under a bound on the compressed span and a text cap), the generalised spread rule, the table
rebased to a window's own upload and text, the launch order, the per-window lc + lp -- compiled for the host into a stand-alone
program (tests/helpers/xz_windows_harness.cpp) with -fsanitize=address,undefined and run directly, nothing preloaded.  It decodes every
window from a copy of only that window's bytes with the serial decoder of lzma_serial.hpp.  No GPU.  Every valid file gives liblzma's
text at one block per window, at a text cap of three median blocks and in one window; the plan is the one windows_of() of
xz_windows_cases.py restates; damage in a block ends in state 2 behind exactly the windows in front of it; and xz_plan, now the
container walk plus the chunk-header walk, yields the block tables it yielded before the split."""
import ctypes as C
import os
import re

import pytest

import xz_cases as cases
import xz_windows_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return wc.build_harness(tmp_path_factory.mktemp("xz-windows"), sanitize=True)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("xz-windows-work")


@pytest.fixture(scope="module")
def old_harness(tmp_path_factory):
    return cases.build_harness(tmp_path_factory.mktemp("xz-one-shot"), sanitize=False)


def all_files():
    """the files of xz_windows_cases and every valid file of xz_cases (at spread 1 the rule passes each of them: the sum of the windows'
    largest blocks never exceeds the whole text)"""
    v = dict(cases.valid())
    v.update(wc.files())
    return v


def settings(rows):
    """one block per window; a text cap of three median blocks; no bound (one window)"""
    return ((1, wc.NO_CAP), (0, wc.median_cap(rows)), (0, wc.NO_CAP))


def counts(rep):
    return [int(x) for x in rep["window-blocks"].split(",")] if rep["window-blocks"] != "-" else []


@pytest.mark.parametrize("name", sorted(all_files()))
def test_every_setting_gives_liblzmas_text(harness, work, name):
    blob, text = all_files()[name]
    assert cases.liblzma_says(blob) == text
    plan, rows = wc.run_plan(harness, work, blob)
    assert plan["status"] == "0" and int(plan["blocks"]) == len(rows)
    for window, cap in settings(rows):
        rep, got = wc.run_stream(harness, work, blob, window, cap)
        want = wc.windows_of(rows, window, cap)
        assert rep["taken"] == "1" and rep["state"] == "1" and rep["status"] == "0" and got == text, (name, window, cap, rep["state"], rep["status"])
        assert counts(rep) == [n for _, n in want], (name, window, cap)
        assert int(rep["windows"]) == int(rep["planned"]) == len(want) and int(rep["blocks"]) == len(rows), (name, window, cap)
        assert int(rep["text"]) == len(text) and int(rep["consumed"]) == len(blob) and rep["streams"] == plan["streams"], (name, window, cap)
    one = counts(wc.run_stream(harness, work, blob, 1, wc.NO_CAP)[0])
    assert one == [1] * len(rows)
    whole = wc.run_stream(harness, work, blob, 0, wc.NO_CAP)[0]
    assert int(whole["windows"]) == (1 if rows else 0)


def test_the_cases_are_what_their_names_say(harness, work):
    f = wc.files()
    rep, _ = wc.run_stream(harness, work, f["lclp-0-then-4"][0], 1, wc.NO_CAP)
    assert rep["window-lclp"] == "0,0,0,4,4,4"  # (sized per window: the file's is 4)
    rep, _ = wc.run_stream(harness, work, f["lclp-0-then-4"][0], 0, wc.NO_CAP)
    assert rep["window-lclp"] == "4"
    rep, _ = wc.run_stream(harness, work, f["streams-without-blocks"][0], 1, wc.NO_CAP)
    assert rep["streams"] == "6" and rep["blocks"] == "5" and rep["windows"] == "5"
    rep, _ = wc.run_stream(harness, work, f["mixed-checks"][0], 0, wc.NO_CAP)
    assert rep["streams"] == "5" and rep["windows"] == "1"  # (one window across five streams of three check kinds)
    rep, _ = wc.run_stream(harness, work, f["empty"][0], 1, wc.NO_CAP)
    assert rep["state"] == "1" and rep["windows"] == "0" and rep["streams"] == "1"
    _, rows = wc.run_plan(harness, work, f["ascending-blocks"][0])
    assert [r[3] for r in rows] == [100, 200, 400, 800, 1600, 3200, 6400]
    _, rows = wc.run_plan(harness, work, f["far-block-second"][0])
    assert rows[1][3] > 2 * cases.RING and rows[1][2] > 0
    for short in (1, 2, 3):
        _, rows = wc.run_plan(harness, work, f["check-none-%d-short-of-a-dword" % short][0])
        assert [r[5] for r in rows] == [0, 0] and all((r[0] + r[1]) % 4 == 4 - short and r[4] == r[0] + r[1] + short for r in rows), rows
    _, rows = wc.run_plan(harness, work, f["chunk-2MiB-zeros-between"][0])
    assert [r[3] > 1 << 20 for r in rows] == [False, True, False]


@pytest.mark.parametrize("run", [1, 2, 3, 7])
def test_40_blocks_in_runs(harness, work, run):
    """window_bytes chosen for runs of `run` blocks: the exact span of blocks j .. j + run - 1, for every j, so that the greedy plan cuts
    runs of that length somewhere in the file whatever the blocks' sizes.  Every plan the harness makes is the restated one, its text is
    liblzma's, a window of exactly `run` blocks occurs, and between the plans for runs of 1, and likewise of 2, the harness cuts a seam behind
    every block"""
    blob, text = cases.valid()["40-blocks"]
    _, rows = wc.run_plan(harness, work, blob)
    seams, exact = set(), 0
    for j in range(0, 40 - run + 1) if run > 1 else [0]:
        window = 1 if run == 1 else rows[j + run - 1][4] + wc.check_bytes(rows[j + run - 1][5]) - rows[j][7]
        want = wc.windows_of(rows, window, 0)
        rep, got = wc.run_stream(harness, work, blob, window, wc.NO_CAP)
        assert rep["state"] == "1" and got == text and counts(rep) == [n for _, n in want], (run, j)
        at = 0
        for n in counts(rep):  # (the seams as the harness cut them)
            seams.add(at)
            at += n
        exact += run in counts(rep)
    assert exact >= 1
    if run <= 2:  # (not only the one-block-per-window plan puts a seam behind every block)
        assert seams == set(range(40))


def test_the_one_window_plan_is_taken_exactly_when_the_one_shot_call_takes_the_file(harness, old_harness, work):
    for sizes in ([3000, 1000], [2000, 2000], [2001, 1999]):
        blob = cases.blocks_of(sizes)[0]
        for spread in (1, 2):
            ref, _ = cases.run_harness(old_harness, work, blob, spread)
            rep, _ = wc.run_stream(harness, work, blob, 0, wc.NO_CAP, spread)
            assert rep["taken"] == ref["taken"] and rep["status"] == ref["status"], (sizes, spread, rep["status"], ref["status"])
            if ref["taken"] == "1":
                assert (rep["blocks"], rep["streams"], rep["text"]) == (ref["blocks"], ref["streams"], ref["bytes"])


def test_the_spread_rule_sums_the_windows_largest_blocks(harness, work):
    blob, text = cases.blocks_of([2000, 2000])
    # one block per window: 2 x (2000 + 2000) > 4000
    rep, got = wc.run_stream(harness, work, blob, 1, wc.NO_CAP, 2)
    assert rep["taken"] == "0" and int(rep["status"]) == cases.XZ_SPREAD and got == b"" and rep["windows"] == "0"
    # both blocks in one window: 2 x 2000 <= 4000
    rep, got = wc.run_stream(harness, work, blob, 0, wc.NO_CAP, 2)
    assert rep["taken"] == "1" and rep["state"] == "1" and got == text and rep["windows"] == "1"


def test_a_block_above_the_text_cap_is_refused_at_begin(harness, work):
    blob, _ = cases.blocks_of([1000, 3000, 1000])
    rep, got = wc.run_stream(harness, work, blob, 0, 2999)
    assert rep["taken"] == "0" and int(rep["status"]) == wc.XZ_BLOCK_OVER_CAP and got == b""
    rep, _ = wc.run_stream(harness, work, blob, 0, 3000)
    assert rep["taken"] == "1" and rep["state"] == "1" and rep["window-blocks"] == "1,1,1"
    # the code collides with none of xz_plan.hpp's or lzma_serial.hpp's
    used = set()
    for hdr in ("xz_plan.hpp", "lzma_serial.hpp"):
        src = open(os.path.join(ROOT, "merkurio_amd/csrc/codec", hdr)).read()
        used |= {int(x) for x in re.findall(r"k(?:Xz|Lz)\w+ = (-\d+)", src)}
    assert len(used) == 32 and wc.XZ_BLOCK_OVER_CAP not in used


# damage in the container: refused at begin, under the one-shot walk's code
CONTAINER = ("flip-stream-header", "flip-block-header", "flip-index", "flip-footer", "cut-stream-header", "cut-block-header", "cut-payload-early", "cut-payload-middle",
             "cut-payload-last", "cut-check", "cut-index", "cut-footer", "trailing-bytes", "trailing-zeros-not-a-multiple-of-4", "index-stored-size-off-by-one",
             "index-text-size-off-by-one", "backward-size-wrong", "block-padding-not-zero")


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_damaged_files(harness, old_harness, work, name):
    blob = cases.damaged()[name]
    assert cases.liblzma_says(blob) is None
    ref, _ = cases.run_harness(old_harness, work, blob)
    for window in (1, 0):
        rep, got = wc.run_stream(harness, work, blob, window, wc.NO_CAP)
        if name in CONTAINER:
            assert rep["taken"] == "0" and rep["status"] == ref["status"] and int(rep["status"]) >= -19 and got == b"", (name, rep["status"], ref["status"])
        else:  # damage inside a block: the stream opens and hands back
            assert rep["taken"] == "1" and rep["state"] == "2" and int(rep["status"]) <= -20, (name, rep["state"], rep["status"])
            if window == 0:
                assert rep["status"] == ref["status"] and got == b"", (name, rep["status"], ref["status"])


@pytest.mark.parametrize("block", [0, 17, 39])
@pytest.mark.parametrize("what", ["payload", "check"])
def test_a_damaged_block_hands_back_behind_the_windows_in_front_of_it(harness, work, block, what):
    blob, text = cases.valid()["40-blocks"]
    _, rows = wc.run_plan(harness, work, blob)
    r = rows[block]
    at = r[0] + r[1] // 2 if what == "payload" else r[4] + 3
    bad = cases.flip(blob, at * 8 + 2)
    assert cases.liblzma_says(bad) is None
    for window in (1, 8 * wc.mean_span(rows)):
        want = wc.windows_of(rows, window, 0)
        before = [(f, n) for f, n in want if f + n <= block]
        assert window == 1 or max(n for _, n in want) > 1
        rep, got = wc.run_stream(harness, work, bad, window, wc.NO_CAP)
        assert rep["taken"] == "1" and rep["state"] == "2" and -32 <= int(rep["status"]) <= -20, (block, what, window, rep["status"])
        if what == "check":
            assert int(rep["status"]) == -31
        delivered = sum(rows[k][3] for f, n in before for k in range(f, f + n))
        assert got == text[:delivered] and int(rep["windows"]) == len(before) and int(rep["text"]) == delivered, (block, what, window)
        assert int(rep["blocks"]) == sum(n for _, n in before)


def test_xz_plan_yields_the_block_tables_it_yielded_before_the_split(harness, work):
    """tests/golden/xz_plan_blocks.json: streams, the largest lc + lp, text, largest block and the XzBlock table that xz_plan made of
    every file of xz_cases.valid() before it became xz_walk + the chunk-header walk"""
    golden = wc.golden_tables()
    assert sorted(golden) == sorted(cases.valid())
    for name, want in sorted(golden.items()):
        rep, rows = wc.run_plan(harness, work, cases.valid()[name][0])
        assert rep["status"] == "0", name
        assert {k: int(rep[k]) for k in ("streams", "lclp", "text", "largest")} == {k: want[k] for k in ("streams", "lclp", "text", "largest")}, name
        assert [r[:7] for r in rows] == want["blocks"], name


def test_the_entries_are_declared_bound_exported_and_refuse_null():
    from merkurio_amd import native as mk
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"int mk_xz_stream_begin\(mk_codec \*c, const uint8_t \*xz, uint64_t n, uint64_t window_bytes, uint32_t \*taken\);", hdr)
    assert re.search(r"int mk_xz_stream_next\(mk_codec \*c, uint64_t \*text_bytes, uint32_t \*state\);", hdr)
    assert re.search(r"int mk_xz_stream_info\(const mk_codec \*c, mk_xz_stream_stats \*out\);", hdr)
    assert re.search(r"int mk_xz_stream_end\(mk_codec \*c\);", hdr)
    assert re.search(r"int mk_codec_set_xz_text_cap\(mk_codec \*c, uint64_t text_bytes\);", hdr)
    L = mk.load()
    for name in ("mk_xz_stream_begin", "mk_xz_stream_next", "mk_xz_stream_info", "mk_xz_stream_end", "mk_codec_set_xz_text_cap"):
        assert name in mk.EXPORTS and hasattr(L, name), name
    assert hasattr(mk.Codec, "unxz_stream") and hasattr(mk.Codec, "unxz_stream_info")
    assert C.sizeof(mk.XzStreamStats) == 8 * 8 + 4 + 4 + 4 * 4
    n, taken, state = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
    blob = (C.c_uint8 * 32)()
    assert L.mk_xz_stream_begin(None, blob, 32, 0, C.byref(taken)) == mk.MK_E_INVALID_ARG
    assert L.mk_xz_stream_next(None, C.byref(n), C.byref(state)) == mk.MK_E_INVALID_ARG
    assert L.mk_xz_stream_info(None, None) == mk.MK_E_INVALID_ARG
    assert L.mk_xz_stream_end(None) == mk.MK_E_INVALID_ARG
    assert L.mk_codec_set_xz_text_cap(None, 0) == mk.MK_E_INVALID_ARG
