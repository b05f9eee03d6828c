"""The .xz files of the xz window tests (mk_xz_stream_*): files() -> {name: (blob, text)} -- files of xz_cases.py whose blocks, streams
and checks a window plan can cut, and new ones made for what a window changes: streams without blocks, lc + lp that differs from
window to window, a launch order that differs from the file order, a far-reaching block that is not its window's first, a read-ahead
that ends where the upload ends, one huge chunk between small blocks.  Blocks are a few hundred bytes to a few KiB unless stated.
The plan itself is restated here in Python (windows_of) as the tests' oracle for what the harness and the library report."""
import functools
import json
import os
import subprocess

import xz_cases as cases
import xz_craft as craft

ROOT = cases.ROOT
NO_CAP = 0  # text cap 0: the harness plans without one, the library takes its default (far above these files)
XZ_BLOCK_OVER_CAP = -33  # xz_chain.hpp


def _crafted_block(build, kind, **kw):
    w = craft.Lzma2Writer()
    build(w)
    data, text = w.end()
    return (craft.block(data, text, kind, **kw), len(text)), text


def _stream_of(parts, kind):
    """parts: [(block, text)] -> (stream, text)"""
    return craft.stream([b for b, _ in parts], kind)[0], b"".join(t for _, t in parts)


def _real(text, kind, **kw):
    return cases.real_block(text, kind, **kw), text


def _short_of_a_dword(short):
    """two check-None blocks whose LZMA2 bytes end `short` bytes in front of a multiple of 4"""
    fq, parts, n = cases.fastq(40, 21 + short), [], 700
    while len(parts) < 2:
        n += 1
        if len(cases.raw(fq[:n])) % 4 == (4 - short) % 4:
            parts.append(_real(fq[:n], 0))
            n += 300
    return _stream_of(parts, 0)


@functools.lru_cache(maxsize=None)
def files():
    v = {name: cases.valid()[name] for name in ("40-blocks", "3000-blocks", "mixed-checks", "two-streams-pad-8", "empty")}
    v["fastq-blocks-mid-record"] = cases.blocks_of([1000, 777, 2048, 1, 4097, 333, 1500, 64, 2999, 1234, 800])
    fq = cases.fastq(120, 13)
    # ---- streams without blocks: in front, between two streams with blocks, at the end
    none4, none1 = craft.stream([], 4)[0], craft.stream([], 1)[0]
    a = _stream_of([_real(fq[:900], 4), _real(fq[900:2000], 4)], 4)
    b = _stream_of([_real(fq[2000:2500], 1), _real(fq[2500:4000], 1), _real(fq[4000:4100], 1)], 1)
    v["streams-without-blocks"] = (none4 + a[0] + none1 + none4 + b[0] + none1, a[1] + b[1])
    # ---- lc + lp = 0 in the first blocks, 4 in the later ones: the LDS is sized per window
    parts = [_crafted_block(cases._props(0, 0, 0), 4) for _ in range(3)] + [_crafted_block(cases._props(lc, lp, pb), 4) for lc, lp, pb in ((0, 4, 4), (4, 0, 0), (2, 2, 2))]
    v["lclp-0-then-4"] = _stream_of(parts, 4)
    # ---- ascending text sizes: the launch order (largest first) is the reverse of the file order
    v["ascending-blocks"] = cases.blocks_of([100, 200, 400, 800, 1600, 3200, 6400], seed=17)
    # ---- more than two rings of text with matches farther back than the ring, second in its window: text_off and in_off are not 0
    # behind the rebase, and the far reads go to device memory
    far = _crafted_block(cases._ring_edges, 4, sizes=True)
    assert len(far[1]) > 2 * cases.RING
    v["far-block-second"] = _stream_of([_real(fq[:333], 4), far, _real(fq[333:1000], 4)], 4)
    # ---- check None, the last block's LZMA2 bytes 1, 2, 3 bytes short of a dword: the upload ends where the block padding does
    for short in (1, 2, 3):
        v["check-none-%d-short-of-a-dword" % short] = _short_of_a_dword(short)
    # ---- one chunk of 2 MiB between small blocks
    v["chunk-2MiB-zeros-between"] = _stream_of([_real(fq[:500], 1), _crafted_block(cases._zeros_2m, 1, dict_size=4096), _real(fq[500:1300], 1)], 1)
    return v


def golden_tables():
    with open(os.path.join(ROOT, "tests", "golden", "xz_plan_blocks.json")) as f:
        return json.load(f)


# ---- the harness -----------------------------------------------------------------------------------------------------------------------

def build_harness(work_dir, sanitize):
    exe = os.path.join(str(work_dir), "xz_windows_harness")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-I", os.path.join(ROOT, "tests/helpers"), "-o", exe,
                    os.path.join(ROOT, "tests/helpers/xz_windows_harness.cpp")], check=True)
    return exe


def _run(exe, work_dir, blob, *args):
    src, out = os.path.join(str(work_dir), "in.xz"), os.path.join(str(work_dir), "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, args[0], src, out, *map(str, args[1:])], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        return p.stdout, f.read()


def run_stream(exe, work_dir, blob, window_bytes, text_cap, spread=1):
    """-> (the report's fields, the text of the windows delivered)"""
    stdout, text = _run(exe, work_dir, blob, "stream", window_bytes, text_cap, spread)
    return dict(f.split("=") for f in stdout.split()), text


def run_plan(exe, work_dir, blob):
    """-> (the fields of the first line, the rows: in_off in_bytes text_off text_bytes check_off check_kind dict_size head_off)"""
    lines = _run(exe, work_dir, blob, "plan")[0].split("\n")
    rep = dict(f.split("=") for f in lines[0].split())
    return rep, [[int(x) for x in ln.split()] for ln in lines[1:] if ln]


# ---- the plan, restated -------------------------------------------------------------------------------------------------------------------

def check_bytes(kind):
    return {0: 0, 1: 4, 4: 8}[kind]


def windows_of(rows, window_bytes, text_cap):
    """the greedy plan over rows of run_plan -> [(first, count)]: the longest run from the cursor with text <= cap and span <= window_bytes"""
    out, k = [], 0
    while k < len(rows):
        first, text = k, 0
        while k < len(rows):
            span = rows[k][4] + check_bytes(rows[k][5]) - rows[first][7]
            if k > first and ((text_cap and text + rows[k][3] > text_cap) or (window_bytes and span > window_bytes)):
                break
            text += rows[k][3]
            k += 1
        out.append((first, k - first))
    return out


def median_cap(rows):
    """the text of 3 median blocks -- and no less than the largest block's, because a block above the cap is refused when the stream begins
    (which has a test of its own)"""
    sizes = sorted(r[3] for r in rows)
    return max(3 * sizes[len(sizes) // 2], sizes[-1], 1) if sizes else 1


def mean_span(rows):
    return (rows[-1][4] + check_bytes(rows[-1][5]) - rows[0][7]) // len(rows)
