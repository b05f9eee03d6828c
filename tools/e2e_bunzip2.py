#!/usr/bin/env python3
"""End-to-end timing of `merkurio extract` on .bz2 inputs: this build (mk_bzip2_inflate_device, a wave per block)
against another build's binary that inflates .bz2 with libbz2 at load (the parent commit's), on the same files, in alternation.

  make   writes into --dir: big.fastq (--reads reads of 150 bp, 4 000 000 = 1.26 GB of text), big.fastq.bz2, small.fastq.bz2
         (--small-reads reads, 480 000 = 150 MB of text) -- one stream each, Python's bz2 at level 9 -- and patterns.txt (a 25-mer
         planted in one read of a hundred)
  run    every configuration once per round, --runs rounds, medians with ranges; the phases of the [timing] row "bzip2 on the device"
         (mk_bzip2_info) as medians, and the share of the call that is its "text" phase (the chain walk on one lane plus the
         expansion).  The plain big.fastq goes through both binaries the same way: the control row, which must not move.

  sweep  --bzip2-window at 64, 128, 256, 512 MiB and 1 GiB (mk_bzip2_stream_*; a file at or below the window takes the one-shot
         call) beside the one-shot call alone (a window above any file), on big.fastq.bz2 and on that file --concat times behind
         itself (4: more than the largest window), every setting once per round, --runs rounds, medians with ranges; per setting the
         stream's own summary row.  Prints the table of profiles/e2e_bunzip2_windows.txt.

Prints the table of profiles/e2e_bunzip2.txt.  Example:
  tools/e2e_bunzip2.py make --dir /tmp/bz
  tools/e2e_bunzip2.py run --dir /tmp/bz --parent-bin /path/to/parent/merkurio --runs 5
  tools/e2e_bunzip2.py sweep --dir /tmp/bz --runs 5
"""
import argparse
import bz2
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
PATTERN = b"ACGTTGCAAGGCTTAACGGATCCAT"
CHUNK = 100000  # reads made at a time


def fastq_chunk(first, n, rng):
    """n records '@r%09d' of 150 bases and qualities as one bytes object; every hundredth read holds PATTERN"""
    ids = np.frombuffer(b"".join(b"@r%09d\n" % (first + i) for i in range(n)), dtype=np.uint8).reshape(n, 12)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 150))]
    pat = np.frombuffer(PATTERN, dtype=np.uint8)
    seq[(-first) % 100::100, 40:40 + len(pat)] = pat
    qual = np.frombuffer(b"FFFF:,#", dtype=np.uint8)[rng.integers(0, 7, size=(n, 150))]
    sep = np.tile(np.frombuffer(b"\n+\n", dtype=np.uint8), (n, 1))
    nl = np.full((n, 1), 10, dtype=np.uint8)
    return np.concatenate([ids, seq, sep, qual, nl], axis=1).tobytes()


def make(a):
    os.makedirs(a.dir, exist_ok=True)
    with open(os.path.join(a.dir, "patterns.txt"), "wb") as f:
        f.write(PATTERN + b"\n")
    for name, reads, plain in (("small", a.small_reads, False), ("big", a.reads, True)):
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        z = bz2.BZ2Compressor(9)
        text = 0
        with open(os.path.join(a.dir, name + ".fastq.bz2"), "wb") as fz, open(os.path.join(a.dir, name + ".fastq") if plain else os.devnull, "wb") as fp:
            for first in range(0, reads, CHUNK):
                blk = fastq_chunk(first, min(CHUNK, reads - first), rng)
                text += len(blk)
                fp.write(blk)
                fz.write(z.compress(blk))
                if first % (10 * CHUNK) == 0:
                    print(f"# make {name}: {first} reads", flush=True)
            fz.write(z.flush())
        print(f"# {name}.fastq.bz2: {reads} reads, {text} text bytes, {os.path.getsize(os.path.join(a.dir, name + '.fastq.bz2'))} compressed, "
              f"written in {time.perf_counter() - t0:.0f} s", flush=True)


def run_once(binary, inp, patterns, out, extra):
    t0 = time.perf_counter()
    p = subprocess.run([binary, "extract", "-i", inp, "-f", patterns, "-r", "-o", out, *extra], capture_output=True,
                       env=dict(os.environ, MERKURIO_TIMING="1"))
    dt = time.perf_counter() - t0
    err = p.stderr.decode(errors="replace")
    if p.returncode != 0:
        raise SystemExit(f"{binary} {' '.join(extra)} -> {p.returncode}\n{err[-2000:]}")
    return dt, err, os.path.getsize(out)


PHASES = re.compile(r"bzip2 on the device: (\d+) blocks, upload ([\d.]+), marker search ([\d.]+), block decode ([\d.]+), text ([\d.]+), CRC ([\d.]+) ms \(input 0: (\d+) text bytes, ([\d.]+) s\)")


def run(a):
    patterns = os.path.join(a.dir, "patterns.txt")
    for inp in ("small.fastq.bz2", "big.fastq.bz2", "big.fastq"):
        path = os.path.join(a.dir, inp)
        bz = inp.endswith(".bz2")
        configs = [("this build" + (" (device)" if bz else ""), BIN, [])]
        if bz and a.with_default:
            configs.append(("this build, libbz2", BIN, ["--host-codec"]))
        if a.parent_bin:
            configs.append(("parent build" + (" (libbz2)" if bz else ""), a.parent_bin, []))
        times = {name: [] for name, _, _ in configs}
        sizes, phases = set(), []
        with tempfile.TemporaryDirectory() as d:
            for r in range(a.runs):  # (in alternation: every configuration once per round)
                for name, binary, extra in configs:
                    dt, err, size = run_once(binary, path, patterns, os.path.join(d, "out.fastq"), extra)
                    times[name].append(dt)
                    sizes.add(size)
                    m = PHASES.search(err)
                    if m and "(device)" in name:
                        phases.append([float(x) for x in m.groups()])
                    if "(device)" in name and not m:
                        raise SystemExit("no 'bzip2 on the device' row: the file was not taken\n" + err[-2000:])
                    print(f"# {inp} round {r} {name}: {dt:.3f} s", flush=True)
        print(f"{inp}: {os.path.getsize(path)} bytes as stored, medians of {a.runs} in alternation; kept records of {sorted(sizes)} bytes"
              f" ({'EQUAL' if len(sizes) == 1 else 'DIFFER'})")
        for name, _, _ in configs:
            t = times[name]
            print(f"  {name:28s} median {statistics.median(t):8.3f} s   range {min(t):.3f} - {max(t):.3f} s")
        if phases:
            med = [statistics.median(col) for col in zip(*phases)]
            call_ms = med[7] * 1e3
            print(f"  mk_bzip2_inflate_device: {int(med[0])} blocks, {int(med[6])} text bytes, call {med[7]:.3f} s: upload {med[1]:.1f}, marker search {med[2]:.1f}, "
                  f"block decode {med[3]:.1f}, text (chain walk + expansion) {med[4]:.1f}, CRC {med[5]:.1f} ms")
            print(f"  share of the call: block decode {100 * med[3] / call_ms:.0f} %, chain walk + expansion {100 * med[4] / call_ms:.0f} %")
        sys.stdout.flush()
        if len(sizes) != 1:
            raise SystemExit(1)


STREAM = re.compile(r"bzip2 input 0 on the device, window by window: (\d+) windows, (\d+) streams closed, (\d+) blocks, (\d+) grown, handed back at (\S+).*?\((.*)\)")
SWEEP_MIB = (64, 128, 256, 512, 1024)


def sweep(a):
    patterns = os.path.join(a.dir, "patterns.txt")
    big = os.path.join(a.dir, "big.fastq.bz2")
    cat = os.path.join(a.dir, f"big_x{a.concat}.fastq.bz2")
    if not os.path.exists(cat):
        with open(cat, "wb") as out, open(big, "rb") as src:
            blob = src.read()
            for _ in range(a.concat):
                out.write(blob)
    for path in (big, cat):
        configs = [("one-shot", ["--bzip2-window", str(1 << 40)])] + [(f"{m} MiB", ["--bzip2-window", str(m << 20)]) for m in SWEEP_MIB]
        times, rows, sizes = {n: [] for n, _ in configs}, {}, set()
        with tempfile.TemporaryDirectory() as d:
            for r in range(a.runs):  # (in alternation: every setting once per round)
                for name, extra in configs:
                    dt, err, size = run_once(BIN, path, patterns, os.path.join(d, "out.fastq"), extra)
                    times[name].append(dt)
                    sizes.add(size)
                    m, one = STREAM.search(err), PHASES.search(err)
                    rows[name] = (f"{m.group(1)} windows, {m.group(3)} blocks, {m.group(4)} grown, handed back at {m.group(5)}; {m.group(6)}" if m
                                  else "one-shot call" if one else "NOT taken by the device")
                    print(f"# {os.path.basename(path)} round {r} {name}: {dt:.3f} s", flush=True)
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes as stored, medians of {a.runs} in alternation; kept records of {sorted(sizes)} bytes"
              f" ({'EQUAL' if len(sizes) == 1 else 'DIFFER'})")
        for name, _ in configs:
            t = times[name]
            print(f"  --bzip2-window {name:9s} median {statistics.median(t):8.3f} s   range {min(t):.3f} - {max(t):.3f} s   [{rows[name]}]")
        sys.stdout.flush()
        if len(sizes) != 1:
            raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("make")
    m.add_argument("--dir", required=True)
    m.add_argument("--reads", type=int, default=4000000)
    m.add_argument("--small-reads", type=int, default=480000)
    r = sub.add_parser("run")
    r.add_argument("--dir", required=True)
    r.add_argument("--runs", type=int, default=5)
    r.add_argument("--parent-bin", default=None)
    r.add_argument("--with-default", action="store_true", help="also this build with --host-codec (libbz2)")
    w = sub.add_parser("sweep")
    w.add_argument("--dir", required=True)
    w.add_argument("--runs", type=int, default=5)
    w.add_argument("--concat", type=int, default=4, help="copies of big.fastq.bz2 behind each other in the second file")
    a = ap.parse_args()
    {"make": make, "run": run, "sweep": sweep}[a.cmd](a)


if __name__ == "__main__":
    main()
