"""What test_unzstd_windows_cpu.py, test_gpu_unzstd_stream.py and test_cli_unzstd_windows_gpu.py share: the host harness of the zstd
window chain (tests/helpers/zstd_windows_harness.cpp: merkurio_amd/csrc/codec/zstd_chain.hpp with the serial decoder) and the files
whose seams cut what a block needs of the blocks in front of it.  The files are those of zstd_cases.py / zstd_craft.py and a few made
here with the same tools; libzstd is the checker."""
import functools
import os
import random
import struct
import subprocess

import zstd_cases as cases
import zstd_craft as craft

BLOCK = 128 << 10
WHOLE = 1 << 40  # a window no file here reaches


def build_harness(work_dir, sanitize):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(work_dir), "zstd_windows_harness")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(root, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(root, "tests/helpers/zstd_windows_harness.cpp")], check=True)
    return exe


def run_harness(exe, work_dir, blob, *args):
    """-> (the report's fields, the text written); args: ("stream", window_bytes, text_cap), ("sweep",) or ("plan",)"""
    src, out = os.path.join(str(work_dir), "in.zst"), os.path.join(str(work_dir), "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    if os.path.exists(out):
        os.remove(out)
    argv = [exe, args[0], src] + ([] if args[0] == "plan" else [out]) + [str(a) for a in args[1:]]
    p = subprocess.run(argv, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]  # (a sanitizer report ends the program with another status)
    assert not p.stderr, p.stderr[-2000:]
    rep = dict(f.split("=") for f in p.stdout.split())
    if args[0] == "plan":
        return rep, None
    with open(out, "rb") as f:
        return rep, f.read()


@functools.lru_cache(maxsize=None)
def flushed_fastq():
    """name -> (file, text): FASTQ in flushed pieces, so that blocks are short and many, at a 1 KiB and a 128 KiB window"""
    fq = cases.fastq(700, seed=11)
    out = {}
    for log in (10, 17):
        step = 1500 if log == 10 else 30000
        pieces = [fq[i:i + step] for i in range(0, 60000 if log == 10 else len(fq), step)]
        text = b"".join(pieces)
        for level in (3, 19):
            out["windows-fastq-wlog%d-l%d" % (log, level)] = (cases.compress(text, level, True, window_log=log, pieces=pieces), text)
    return out


@functools.lru_cache(maxsize=None)
def crafted():
    """what the corpora do not reach at a seam"""
    fq = cases.fastq(1300)
    a, b = cases.compress(fq[:50000], 3, True), cases.compress(fq[50000:90000], 19, False)
    skip = struct.pack("<II", 0x184D2A50, 5) + b"skip!"
    out = {"windows-skippable-between-frames": (a + skip + b + skip, fq[:90000])}
    # a history that holds everything a later window needs: every block of 128 KiB is the first one again, so each window behind the
    # first has matches into the history (and inside its own block) only
    rng = random.Random(41)
    unit = bytes(rng.getrandbits(8) for _ in range(BLOCK))
    out["windows-matches-into-history-only"] = (cases.compress(unit * 4, 3, True, window_log=18), unit * 4)
    return out


@functools.lru_cache(maxsize=None)
def seam_files():
    """name -> (file, text): the files of a few hundred KB at the most whose seams cut something"""
    v = cases.valid()
    names = ["fastq-l3-checksum", "fastq-l19", "fastq-l1", "three-frames", "skippable-around", "empty-frame-among", "flushed-records", "flushed-records-l19",
             "far-match", "size-131073", "long-match", "rle-literals", "crafted-rle-block", "crafted-repeat-across-a-raw-block", "golden-sample"]
    names += [n for n in v if n.startswith("crafted-modes-") or n.startswith("crafted-repeat-")]
    out = {n: v[n] for n in sorted(set(names))}
    out.update(flushed_fastq())
    out.update(crafted())
    return out


def all_valid():
    out = dict(cases.valid())
    out.update(flushed_fastq())
    out.update(crafted())
    return out


SETTINGS = (("stream", 1, 0), ("stream", 1000, 0), ("stream", WHOLE, BLOCK), ("sweep",))
