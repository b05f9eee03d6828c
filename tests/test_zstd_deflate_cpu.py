"""merkurio_amd/csrc/codec/zstd_enc_serial.hpp -- the serial pieces of the zstd frame writer of zstd_deflate.hip -- compiled for the host
into a stand-alone program (tests/helpers/zstd_enc_harness.cpp, a naive greedy parser in front of them) with
-fsanitize=address,undefined.  Every frame it writes must decode with this project's decoder (zstd_serial.hpp, inside the harness) and,
alone, with libzstd; the block, literal and table kinds must be the ones each text is built to force.  mk_zstd_record_cuts (host code)
against the rule restated in Python.  No GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import zstd_cases as zc
import zstd_out_cases as zo
from merkurio_amd import native as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, M = zo.GRID, zo.TEXT_MAX


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("zstd-enc")), "zstd_enc_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g",
                    "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe, os.path.join(ROOT, "tests/helpers/zstd_enc_harness.cpp")], check=True)
    return exe


def run(exe, work, text):
    src, out = os.path.join(str(work), "in.bin"), os.path.join(str(work), "out.zst")
    with open(src, "wb") as f:
        f.write(text)
    p = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    rows = [dict(f.split("=") for f in line.split()) for line in p.stdout.splitlines()]
    with open(out, "rb") as f:
        return rows, f.read()


def texts():
    rng = random.Random(41)
    rnd = bytes(rng.getrandbits(8) for _ in range(6000))
    fq = zc.fastq(900)
    wide = bytes(rng.sample(range(127, 256), 129))  # 129 distinct bytes, all but one above 128
    few = b"A" * 10 + b"xy" + b"B" * 25 + b"C" * 40 + b"pqr" + b"D" * 70 + b"E" * 9  # five runs of five lengths: five sequences
    out = {"size-%d" % n: fq[:n] for n in (0, 1, 2, 3, 4, 63, 64, 65, 4095, 4096, 4097)}
    out.update({
        "one-byte": b"G" * 5000, "random": rnd, "two-symbols": b"aaababbbaa", "wide-literals": wide + b"Z" * 3000 + wide[:64],
        "literals-1023": zc.match_free_text(1023), "literals-1024": zc.match_free_text(1024), "literals-16383": zc.match_free_text(16383),
        "literals-16384": zc.match_free_text(16384), "short-matches": zc.short_matches_text(), "long-match": b"x" + b"G" * (M - 1),
        "long-literals": zo.match_free_bytes(66000) + fq[:3000] * 3, "far-offset": zo.far_offset_text(),
        "many-sequences": zc.short_matches_text()[:M - 1], "quads-32767": zo.quad_units(32767), "quads-127": zo.quad_units(127), "quads-128": zo.quad_units(128),
        "one-code-each": b"ab" + b"cd" * 20, "few-sequences": few, "fastq": fq[:300000],
    })
    return out


@pytest.fixture(scope="module")
def results(harness, tmp_path_factory):
    work = tmp_path_factory.mktemp("zstd-enc-run")
    return {name: run(harness, work, t) for name, t in texts().items()}


@pytest.mark.parametrize("name", sorted(texts()))
def test_every_frame_decodes_alone_with_both_decoders(results, name):
    text = texts()[name]
    rows, blob = results[name]
    assert all(r["self"] == "1" for r in rows), rows
    frames = zo.frames_by_libzstd(blob)
    assert b"".join(t for _, t in frames) == text and len(frames) == len(rows) == len(mk.zstd_record_cuts([len(text)])) - (1 if text else 0)
    for (frame, t), r in zip(frames, rows):
        s = zo.shape(frame)
        assert s["text"] == len(t) == int(r["n"]) and s["block"] == ("raw", "rle", "compressed").index(r["block"])
        assert len(frame) <= len(t) + 16, "a compressed block is never larger than the raw form"


def test_the_texts_force_what_their_names_say(results):
    r = {name: rows for name, (rows, _) in results.items()}
    assert [x["block"] for x in r["size-0"]] == ["raw"] and r["size-1"][0]["block"] == "rle" and r["size-4"][0]["block"] == "raw"
    assert r["one-byte"][0]["block"] == "rle" and r["random"][0]["block"] == "raw" and r["two-symbols"][0]["block"] == "raw"
    assert (r["wide-literals"][0]["block"], r["wide-literals"][0]["lit"]) == ("compressed", "raw")
    for n, streams in ((1023, "1"), (1024, "4"), (16383, "4"), (16384, "4")):
        row = r["literals-%d" % n][0]
        assert (row["lit"], row["streams"], row["nlit"], row["nseq"]) == ("huffman", streams, str(n), "0"), row
    assert (r["long-match"][0]["nseq"], r["long-match"][0]["ll"], r["long-match"][0]["of"], r["long-match"][0]["ml"]) == ("1", "rle", "rle", "rle")
    assert r["one-code-each"][0]["ll"] == r["one-code-each"][0]["of"] == r["one-code-each"][0]["ml"] == "rle"
    assert set(r["few-sequences"][0][t] for t in ("ll", "of", "ml")) <= {"predefined", "rle"} and "predefined" in r["few-sequences"][0].values()
    assert all(row[t] == "fse" for row in r["fastq"] for t in ("ll", "of", "ml")) and int(r["fastq"][0]["nseq"]) > 10000
    assert int(r["short-matches"][0]["nseq"]) > 20000


def test_the_size_formats_of_huffman_literals(results):
    for n, fmt in ((1023, 0), (1024, 2), (16383, 2), (16384, 3)):
        s = zo.shape(zo.frames_by_libzstd(results["literals-%d" % n][1])[0][0])
        assert (s["lit"], s["lit_format"], s["n_lit"]) == (2, fmt, n), (n, s)


def test_the_longest_codes(results):
    """match-length code 52, literal-length code 35, an offset beyond 2^16: the frames decode (above); here that the texts reach them"""
    s = zo.shape(zo.frames_by_libzstd(results["long-match"][1])[0][0])
    assert s["n_seq"] == 1 and s["n_lit"] == 2  # x, G, and one match of 114 686
    s = zo.shape(zo.frames_by_libzstd(results["long-literals"][1])[0][0])
    assert s["block"] == 2 and s["n_lit"] > 65536
    s = zo.shape(zo.frames_by_libzstd(results["far-offset"][1])[0][0])  # x y z 0, a run of zeros, xyz from 131 068 bytes back
    assert (s["block"], s["n_lit"], s["n_seq"], s["text"]) == (2, 4, 2, M - 1)


def test_the_three_forms_of_the_sequence_count(results):
    """one byte below 128, two bytes below 0x7F00, three from there on: one frame each (a record of 131 071 bytes is one frame)"""
    for name, lo, hi in (("quads-127", 127, 127), ("quads-128", 128, 128), ("quads-32767", 0x7F00, 32767), ("many-sequences", 0x7F00, M // 3)):
        rows, blob = results[name]
        frames = zo.frames_by_libzstd(blob)
        assert len(frames) == 1, name
        s = zo.shape(frames[0][0])
        assert lo <= s["n_seq"] <= hi and s["n_seq"] == int(rows[0]["nseq"]), (name, s)
    assert int(results["short-matches"][0][0]["nseq"]) < 0x7F00


# ---- mk_zstd_record_cuts ---------------------------------------------------------------------------------------------------------------
def ends_of(lengths):
    return np.cumsum(np.asarray(lengths, dtype=np.uint64))


@pytest.mark.parametrize("lengths", [
    [], [0, 0], [5], [M], [M + 1], [100, M, 100], [100, M + 1, 100], [G], [G - 1, 1, 50], [G, 50], [G + 1, 50], [G - 1, 2, G - 1, G + 1, 7],
    [G + zo.REACH - 1, 9], [G + zo.REACH, 9], [3 * G + 5], [331] * 2000,
], ids=lambda v: "x".join(map(str, v[:5])) or "empty")
def test_record_cuts_against_the_rule(lengths):
    e = ends_of(lengths)
    cuts = mk.zstd_record_cuts(e).tolist()
    assert cuts == zo.rule(e), lengths
    assert all(b - a <= M for a, b in zip(cuts, cuts[1:]))
    kept = set(e.tolist()) | {0}
    for a, c in zip(cuts, cuts[1:]):  # a cut is a record end, or lies on the grid inside a record that no frame could hold
        assert c in kept or c % G == 0, (lengths, c)


def test_record_cuts_edges():
    assert mk.zstd_record_cuts([]).tolist() == [0]
    assert mk.zstd_record_cuts([M]).tolist() == [0, G, M] and mk.zstd_record_cuts([M + 1]).tolist() == [0, G, M + 1]
    assert mk.zstd_record_cuts([G - 1, G + 5]).tolist() == [0, G + 5] and mk.zstd_record_cuts([G, G + 5]).tolist() == [0, G, G + 5]
    assert mk.zstd_record_cuts([G + 1, G + 5]).tolist() == [0, G + 1, G + 5]
    L_ = mk.load()
    e, out, n = np.array([G + 1, G + 5], dtype=np.uint64), np.zeros(2, dtype=np.uint64), C.c_uint64(0)
    assert L_.mk_zstd_record_cuts(e.ctypes.data, e.size, out.ctypes.data, 2, C.byref(n)) == mk.MK_E_CAPACITY and n.value == 3
    bad = np.array([9, 3], dtype=np.uint64)
    assert L_.mk_zstd_record_cuts(bad.ctypes.data, 2, out.ctypes.data, 2, C.byref(n)) == mk.MK_E_INVALID_ARG


def test_the_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"#define MK_ZSTD_CUT_GRID 114688u", hdr) and re.search(r"#define MK_ZSTD_FRAME_TEXT_MAX 131072u", hdr)
    L_ = mk.load()
    for name in ("mk_zstd_record_cuts", "mk_zstd_deflate_bound", "mk_zstd_deflate_records", "mk_zstd_deflate_info"):
        assert name in mk.EXPORTS and hasattr(L_, name) and name in hdr, name
    assert L_.mk_zstd_deflate_bound(0) == 32 and L_.mk_zstd_deflate_bound(3 * G + 1) == 3 * G + 1 + 16 * 5
    assert hasattr(mk.Codec, "zstd_records") and hasattr(mk.Codec, "zstd_record_cuts")
