#!/usr/bin/env python3
"""Figures for the device's xz path (mk_xz_inflate_device, `extract --device-xz`).

  rates  the two rates the spread rule's K comes from, on FASTQ text written at preset 6 as ONE block (--mb MiB of text):
           r_wave  text bytes per second of one block decoding alone on the device (one wave; the decode kernel's own time, mk_xz_info)
           r_lzma  liblzma on one host thread over the same bytes (the stdlib's lzma module)
         and K = ceil(2 x r_lzma / r_wave): a file is taken only when its largest block's text x K <= its whole text.  The factor 2:
         boxes differ by that much, and a partly filled device finishes no sooner than its slowest wave.  Medians of --runs.  The
         default is one block of 24 MiB of text, what `xz -T -6` writes: about 10 s per device call.  The device calls run in this
         process with no time limit of their own: wrap the command in `timeout`
  make   writes into --dir: big.fastq (--reads reads of 150 bp, 4 000 000 = 1.26 GB of text) and small (--small-reads, 480 000 = 150 MB),
         each three ways through liblzma at preset 6 -- NAME.t4.fastq.xz (blocks of 24 MiB of text, what `xz -T4 -6` writes),
         NAME.1m.fastq.xz (blocks of 1 MiB, `xz --block-size=1MiB`), NAME.one.fastq.xz (a single block, `xz -6`) -- and patterns.txt
  run    `extract` end to end, this build with --device-xz against another build's binary (the parent commit's, liblzma on one host
         thread at load), in alternation, medians of --runs with ranges; the [timing] row says which path ran: the single-block files
         show the rule handing them back.  The plain big.fastq goes through both binaries as the control row.

  sweep  the big multi-block files under --xz-stream at every --caps value (text bytes per window, --xz-text-cap; 0 = the default)
         against the parent's binary with liblzma, in alternation, medians of --runs; per cap the stream's summary row (planned
         windows, windows, blocks, phases, peak device bytes).  --spread is passed as --xz-spread (0 = the default K, under which a
         file of 24 MiB blocks passes the rule only in windows of about 2.5 GiB of text).  Prints the table of
         profiles/e2e_unxz_windows.txt

Prints the table of profiles/e2e_unxz.txt.  Example:
  timeout -k 10 300 tools/e2e_unxz.py rates
  tools/e2e_unxz.py make --dir /tmp/xz && tools/e2e_unxz.py run --dir /tmp/xz --parent-bin /path/to/parent/merkurio --runs 5
"""
import argparse
import lzma
import math
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xz_craft as craft  # noqa: E402  (the container writer of the tests)

BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
RUN_LIMIT_S = 600


def raw6(text):
    return lzma.compress(text, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 6}])


def rates(a):
    import numpy as np
    from e2e_bunzip2 import fastq_chunk
    from merkurio_amd import native as mk
    rng = np.random.default_rng(7)
    text, reads = b"", 0
    while len(text) < a.mb << 20:
        text += fastq_chunk(reads, 20000, rng)
        reads += 20000
    text = text[:a.mb << 20]
    blob = craft.stream([(craft.block(raw6(text), text, 4, dict_size=8 << 20), len(text))], 4)[0]
    host, wave = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        got = lzma.decompress(blob)
        host.append(time.perf_counter() - t0)  # (the decompress alone; compared afterwards)
        assert got == text
    c = mk.Codec()
    c.set_xz_spread(1)
    try:
        for _ in range(a.runs + 1):  # (the first call allocates: not counted)
            taken, got, n_blocks = c.unxz(blob)
            assert taken and n_blocks == 1 and got == text, c.unxz_info()
            wave.append(c.unxz_info()[4][1] / 1e3)
    finally:
        c.close()
    r_lzma, r_wave = len(text) / statistics.median(host), len(text) / statistics.median(wave[1:])
    print(f"one block of {len(text)} text bytes ({len(blob)} stored), preset 6, medians of {a.runs}")
    print(f"r_wave  {r_wave / 1e6:9.2f} MB/s  (decode kernel, one wave: {min(wave[1:]):.3f} .. {max(wave[1:]):.3f} s)")
    print(f"r_lzma  {r_lzma / 1e6:9.2f} MB/s  (liblzma, one host thread: {min(host):.3f} .. {max(host):.3f} s)")
    print(f"K = ceil(2 x r_lzma / r_wave) = {math.ceil(2 * r_lzma / r_wave)}")


def make(a):
    import numpy as np
    from e2e_bunzip2 import CHUNK, PATTERN, fastq_chunk
    os.makedirs(a.dir, exist_ok=True)
    with open(os.path.join(a.dir, "patterns.txt"), "wb") as f:
        f.write(PATTERN + b"\n")
    for name, reads in (("small", a.small_reads), ("big", a.reads)):
        rng = np.random.default_rng(7)
        text = b"".join(fastq_chunk(first, min(CHUNK, reads - first), rng) for first in range(0, reads, CHUNK))
        if name == "big":
            with open(os.path.join(a.dir, "big.fastq"), "wb") as f:
                f.write(text)
        for tag, step in (("t4", 24 << 20), ("1m", 1 << 20), ("one", len(text))):
            t0 = time.perf_counter()
            parts = [text[k:k + step] for k in range(0, len(text), step)]
            blob = craft.stream([(craft.block(raw6(p), p, 4, dict_size=8 << 20, sizes=True), len(p)) for p in parts], 4)[0]
            with open(os.path.join(a.dir, f"{name}.{tag}.fastq.xz"), "wb") as f:
                f.write(blob)
            print(f"# {name}.{tag}: {len(parts)} blocks, {len(blob)} bytes in {time.perf_counter() - t0:.0f} s", flush=True)


def run_once(binary, inp, patterns, out, extra):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(RUN_LIMIT_S), binary, "extract", "-i", inp, "-f", patterns, "-r", "-o", out, *extra], capture_output=True,
                       env=dict(os.environ, MERKURIO_TIMING="1"))
    dt = time.perf_counter() - t0
    err = p.stderr.decode(errors="replace")
    if p.returncode != 0:  # (nothing more is started on the device after a run that failed)
        raise SystemExit(f"{binary} {' '.join(extra)} -> {p.returncode}\n{err[-2000:]}")
    return dt, err


def med(xs):
    return f"{statistics.median(xs):8.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def run(a):
    patterns, out = os.path.join(a.dir, "patterns.txt"), os.path.join(a.dir, "out.fastq")
    inputs = [f"{n}.{t}.fastq.xz" for n in ("small", "big") for t in ("t4", "1m", "one")] + ["big.fastq"]
    times = {(inp, who): [] for inp in inputs for who in ("this", "parent")}
    path_ran = {}
    for r in range(a.runs):
        for inp in inputs:
            for who, binary, extra in (("this", BIN, ["--device-xz"] + (["--xz-spread", str(a.spread)] if a.spread else []) if inp.endswith(".xz") else []),
                                       ("parent", a.parent_bin, [])):
                dt, err = run_once(binary, os.path.join(a.dir, inp), patterns, out, extra)
                times[(inp, who)].append(dt)
                if who == "this":
                    rows = [ln.strip() for ln in err.split("\n") if re.search(r"xz on the device: |xz input \d+: NOT taken", ln)]
                    path_ran[inp] = rows[0] if rows else "(plain input)"
            print(f"# round {r}: {inp} done", flush=True)
    print(f"extract, seconds per run, median [min .. max] of {a.runs}, alternating")
    print(f"{'input':24s} {'this build (--device-xz)':>34s} {'parent (liblzma, one thread)':>34s}")
    for inp in inputs:
        print(f"{inp:24s} {med(times[(inp, 'this')]):>34s} {med(times[(inp, 'parent')]):>34s}")
    for inp in inputs:
        print(f"{inp}: {path_ran[inp]}")


def sweep(a):
    patterns, out = os.path.join(a.dir, "patterns.txt"), os.path.join(a.dir, "out.fastq")
    inputs = ["big.t4.fastq.xz", "big.1m.fastq.xz"]
    caps = [int(c) for c in a.caps.split(",")]
    times = {(inp, c): [] for inp in inputs for c in caps + ["parent"]}
    summary = {}
    for r in range(a.runs):
        for inp in inputs:
            path = os.path.join(a.dir, inp)
            for c in caps:
                extra = ["--xz-stream", "--xz-window", "1", "--xz-text-cap", str(c)] + (["--xz-spread", str(a.spread)] if a.spread else [])
                dt, err = run_once(BIN, path, patterns, out, extra)
                times[(inp, c)].append(dt)
                rows = [ln.strip() for ln in err.split("\n") if "window by window" in ln]
                summary[(inp, c)] = rows[-1] if rows else "(no stream row)"
                dt, _ = run_once(a.parent_bin, path, patterns, out, [])
                times[(inp, "parent")].append(dt)
            print(f"# round {r}: {inp} done", flush=True)
    print(f"extract --xz-stream, seconds per run, median [min .. max] of {a.runs}, alternating with the parent's binary")
    for inp in inputs:
        print(f"{inp:24s} parent (liblzma, one thread) {med(times[(inp, 'parent')])}")
        for c in caps:
            print(f"{inp:24s} --xz-text-cap {c:<12d} {med(times[(inp, c)])}")
            print(f"    {summary[(inp, c)]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("rates")
    q.add_argument("--mb", type=int, default=24)
    q.add_argument("--runs", type=int, default=3)
    m = sub.add_parser("make")
    m.add_argument("--dir", required=True)
    m.add_argument("--reads", type=int, default=4000000)
    m.add_argument("--small-reads", type=int, default=480000)
    r = sub.add_parser("run")
    r.add_argument("--dir", required=True)
    r.add_argument("--parent-bin", required=True)
    r.add_argument("--runs", type=int, default=5)
    r.add_argument("--spread", type=int, default=0, help="--xz-spread for this build's runs; 0 = the default")
    w = sub.add_parser("sweep")
    w.add_argument("--dir", required=True)
    w.add_argument("--parent-bin", required=True)
    w.add_argument("--runs", type=int, default=5)
    w.add_argument("--caps", default="0,268435456,1073741824", help="--xz-text-cap values, comma separated; 0 = the default")
    w.add_argument("--spread", type=int, default=0, help="--xz-spread for this build's runs; 0 = the default")
    a = ap.parse_args()
    {"rates": rates, "make": make, "run": run, "sweep": sweep}[a.cmd](a)
