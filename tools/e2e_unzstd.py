#!/usr/bin/env python3
"""End-to-end timing of `merkurio extract` on .zst inputs: this build with --device-zstd (mk_zstd_inflate_device, a wave per block)
against another build's binary that inflates .zst with libzstd on one host thread at load (the parent commit's), on the same files,
in alternation.

  make   writes into --dir: big.fastq (--reads reads of 150 bp, 4 000 000 = 1.26 GB of text), big.l3.fastq.zst, big.l19.fastq.zst,
         small.l3.fastq.zst, small.l19.fastq.zst (--small-reads reads, 480 000 = 150 MB of text) -- one frame each with a content
         checksum, libzstd through ctypes at levels 3 and 19 -- and patterns.txt (a 25-mer planted in one read of a hundred)
  run    every configuration once per round, --runs rounds, medians with ranges; the phases of the [timing] row "zstd on the device"
         (mk_zstd_info) of the large files as medians, with the round count.  The plain big.fastq goes through both binaries the same
         way: the control row, which must not move.  Every run is a process of its own under a time limit; a run that fails ends the
         script there.

  sweep  the large files under --zstd-stream at every --windows value (compressed bytes per window, mk_zstd_stream_*) against the
         parent's binary, in alternation, medians of --runs; per window size the stream's summary row (windows, rounds, the six
         phases summed, peak device bytes) as medians.  Prints the table of profiles/e2e_unzstd_windows.txt.

Prints the table of profiles/e2e_unzstd.txt.  The device path becomes `extract`'s default for .zst only if its median is below the
parent's on both large-file rows by more than the two ranges overlap.  Example:
  tools/e2e_unzstd.py make --dir /tmp/zs
  tools/e2e_unzstd.py run --dir /tmp/zs --parent-bin /path/to/parent/merkurio --runs 5
"""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from e2e_bunzip2 import CHUNK, PATTERN, fastq_chunk  # noqa: E402  (the same reads as the bzip2 figures)
import zstd_cases as zc  # noqa: E402  (the ctypes binding of libzstd)

BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
RUN_LIMIT_S = 600


class Frame:
    """one zstd frame written piece by piece (ZSTD_compressStream2), with a content checksum"""

    def __init__(self, path, level):
        self.z = zc.lib()
        self.c = self.z.ZSTD_createCCtx()
        for param, value in ((zc.C_LEVEL, level), (zc.C_CHECKSUM, 1)):
            assert not self.z.ZSTD_isError(self.z.ZSTD_CCtx_setParameter(self.c, param, value))
        self.f = open(path, "wb")
        self.room = ctypes.create_string_buffer(self.z.ZSTD_compressBound(CHUNK * 320) + 1024)

    def write(self, blk, end=False):
        src = ctypes.create_string_buffer(blk, len(blk))
        ib = zc._Buf(ctypes.cast(src, ctypes.c_void_p), len(blk), 0)
        while True:
            ob = zc._Buf(ctypes.cast(self.room, ctypes.c_void_p), len(self.room), 0)
            r = self.z.ZSTD_compressStream2(self.c, ctypes.byref(ob), ctypes.byref(ib), zc.E_END if end else zc.E_CONTINUE)
            assert not self.z.ZSTD_isError(r)
            self.f.write(self.room.raw[:ob.pos])
            if ib.pos == ib.size and (not end or r == 0):
                break

    def close(self):
        self.write(b"", end=True)
        self.z.ZSTD_freeCCtx(self.c)
        self.f.close()


def make(a):
    import numpy as np
    os.makedirs(a.dir, exist_ok=True)
    with open(os.path.join(a.dir, "patterns.txt"), "wb") as f:
        f.write(PATTERN + b"\n")
    for name, reads, plain in (("small", a.small_reads, False), ("big", a.reads, True)):
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        frames = [Frame(os.path.join(a.dir, "%s.l%d.fastq.zst" % (name, level)), level) for level in (3, 19)]
        with open(os.path.join(a.dir, name + ".fastq") if plain else os.devnull, "wb") as fp:
            for first in range(0, reads, CHUNK):
                blk = fastq_chunk(first, min(CHUNK, reads - first), rng)
                fp.write(blk)
                for fr in frames:
                    fr.write(blk)
                if first % (10 * CHUNK) == 0:
                    print(f"# make {name}: {first} reads", flush=True)
        for fr in frames:
            fr.close()
        print(f"# {name}: {reads} reads written at levels 3 and 19 in {time.perf_counter() - t0:.0f} s", flush=True)


def run_once(binary, inp, patterns, out, extra):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(RUN_LIMIT_S), binary, "extract", "-i", inp, "-f", patterns, "-r", "-o", out, *extra], capture_output=True,
                       env=dict(os.environ, MERKURIO_TIMING="1"))
    dt = time.perf_counter() - t0
    err = p.stderr.decode(errors="replace")
    if p.returncode != 0:  # (nothing more is started on the device after a run that failed)
        raise SystemExit(f"{binary} {' '.join(extra)} -> {p.returncode}\n{err[-2000:]}")
    return dt, err


PHASES = re.compile(r"zstd on the device: (\d+) blocks, (\d+) frames, (\d+) rounds, upload ([\d.]+), tables \+ entropy decode ([\d.]+), scans ([\d.]+), "
                    r"execution ([\d.]+), cross-block rounds ([\d.]+), checksum ([\d.]+) ms")


def med(xs):
    return f"{statistics.median(xs):8.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def run(a):
    patterns = os.path.join(a.dir, "patterns.txt")
    out = os.path.join(a.dir, "out.fastq")
    inputs = ["small.l3.fastq.zst", "small.l19.fastq.zst", "big.l3.fastq.zst", "big.l19.fastq.zst", "big.fastq"]
    times = {(inp, who): [] for inp in inputs for who in ("this", "parent")}
    phases = {inp: [] for inp in inputs}
    for r in range(a.runs):
        for inp in inputs:
            path = os.path.join(a.dir, inp)
            for who, binary, extra in (("this", BIN, ["--device-zstd"] if inp.endswith(".zst") else []), ("parent", a.parent_bin, [])):
                dt, err = run_once(binary, path, patterns, out, extra)
                times[(inp, who)].append(dt)
                m = PHASES.search(err)
                if who == "this" and inp.endswith(".zst"):
                    if not m:
                        raise SystemExit(f"{inp}: the device did not take the file\n{err[-2000:]}")
                    phases[inp].append([float(x) for x in m.groups()])
            print(f"# round {r}: {inp} done", flush=True)
    print(f"extract, seconds per run, median [min .. max] of {a.runs}, alternating")
    print(f"{'input':24s} {'this build (--device-zstd)':>34s} {'parent (libzstd, one thread)':>34s}")
    for inp in inputs:
        print(f"{inp:24s} {med(times[(inp, 'this')]):>34s} {med(times[(inp, 'parent')]):>34s}")
    for inp in inputs:
        if phases[inp] and inp.startswith("big"):
            cols = list(zip(*phases[inp]))
            names = ("blocks", "frames", "rounds", "upload", "tables + entropy decode", "scans", "execution", "cross-block rounds", "checksum")
            print(f"{inp}: " + ", ".join(f"{n} {statistics.median(c):.1f}" for n, c in zip(names, cols)) + " (ms, medians)")


STREAM = re.compile(r"zstd input 0 on the device, window by window: (\d+) windows, (\d+) frames closed, (\d+) blocks, (\d+) rounds, largest history (\d+) bytes, "
                    r"handed back at -, [\d.]+ s \(upload ([\d.]+), tables \+ entropy decode ([\d.]+), walk \+ scans ([\d.]+), execution ([\d.]+), "
                    r"cross-block rounds ([\d.]+), checksum ([\d.]+) ms; peak (\d+) device bytes")


def sweep(a):
    patterns = os.path.join(a.dir, "patterns.txt")
    out = os.path.join(a.dir, "out.fastq")
    inputs = ["big.l3.fastq.zst", "big.l19.fastq.zst"]
    windows = [int(w) for w in a.windows.split(",")]
    times = {(inp, w): [] for inp in inputs for w in windows + ["parent"]}
    rows = {(inp, w): [] for inp in inputs for w in windows}
    for r in range(a.runs):
        for inp in inputs:
            path = os.path.join(a.dir, inp)
            for w in windows:  # (this build at one window size, then the parent: in alternation)
                dt, err = run_once(BIN, path, patterns, out, ["--zstd-stream", "--zstd-window", str(w)])
                m = STREAM.search(err)
                if not m:
                    raise SystemExit(f"{inp} at window {w}: the stream did not reach the file's end\n{err[-2000:]}")
                times[(inp, w)].append(dt)
                rows[(inp, w)].append([float(x) for x in m.groups()])
                times[(inp, "parent")].append(run_once(a.parent_bin, path, patterns, out, [])[0])
            print(f"# round {r}: {inp} done", flush=True)
    print(f"extract --zstd-stream, seconds per run, median [min .. max] of {a.runs}, alternating with the parent's binary")
    names = ("windows", "frames", "blocks", "rounds", "largest history", "upload", "tables + entropy decode", "walk + scans", "execution", "cross-block rounds",
             "checksum", "peak device bytes")
    for inp in inputs:
        print(f"{inp:24s} parent (libzstd, one thread) {med(times[(inp, 'parent')])}")
        for w in windows:
            print(f"{inp:24s} --zstd-window {w:<12d} {med(times[(inp, w)])}")
            print("    " + ", ".join(f"{n} {statistics.median(c):.1f}" for n, c in zip(names, zip(*rows[(inp, w)]))) + " (ms summed over the windows, medians)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("make")
    m.add_argument("--dir", required=True)
    m.add_argument("--reads", type=int, default=4000000)
    m.add_argument("--small-reads", type=int, default=480000)
    r = sub.add_parser("run")
    r.add_argument("--dir", required=True)
    r.add_argument("--parent-bin", required=True)
    r.add_argument("--runs", type=int, default=5)
    s = sub.add_parser("sweep")
    s.add_argument("--dir", required=True)
    s.add_argument("--parent-bin", required=True)
    s.add_argument("--runs", type=int, default=5)
    s.add_argument("--windows", default="16777216,67108864,268435456", help="compressed bytes per window, comma-separated")
    a = ap.parse_args()
    {"make": make, "run": run, "sweep": sweep}[a.cmd](a)
