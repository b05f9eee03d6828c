#!/usr/bin/env python3
"""End-to-end timing of `merkurio extract` on a plain gzip input that is inflated on the device window by window.

  sweep   --gzip-window at 64, 128, 256, 512 MiB and 1 GiB (each streamed: the file must be larger, or the row says "one-shot"),
          medians of --runs runs taken in alternation, beside --host-codec and, with --parent-bin, the parent build's binary
  check   one file, streamed against --host-codec by the SHA-256 of the output; windows and peak device bytes from the timing rows
          (for a member of 6 GiB of text or more, and for a file of 20 GB or more)

Prints a table for profiles/e2e_gunzip_windows.txt.  Example:
  tools/e2e_gunzip_windows.py sweep --input reads.fastq.gz --patterns patterns.txt --runs 5 [--parent-bin /path/to/parent/merkurio]
  tools/e2e_gunzip_windows.py check --input huge.fastq.gz --patterns patterns.txt
"""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
MIB = 1 << 20


def run(binary, inp, patterns, out, extra):
    t0 = time.perf_counter()
    p = subprocess.run([binary, "extract", "-i", inp, "-f", patterns, "-r", "-o", out, *extra], capture_output=True,
                       env=dict(os.environ, MERKURIO_TIMING="1"))
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit(f"{binary} {' '.join(extra)} -> {p.returncode}\n{p.stderr.decode(errors='replace')[-2000:]}")
    return dt, p.stderr.decode(errors="replace")


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(16 * MIB), b""):
            h.update(blk)
    return h.hexdigest()


def summary_row(err):
    m = re.search(r"window by window: (\d+) windows, (\d+) members proved, (\d+) grown, (\d+) rounds repeated, handed back at ([^,]+),.*peak (\d+) device bytes", err)
    return m.groups() if m else None


def sweep(a):
    size = os.path.getsize(a.input)
    configs = [(f"window {w} MiB" + ("" if size > w * MIB else " (one-shot)"), BIN, ["--gzip-window", str(w * MIB)]) for w in (64, 128, 256, 512, 1024)]
    configs.append(("--host-codec", BIN, ["--host-codec"]))
    if a.parent_bin:
        configs.append(("parent build", a.parent_bin, []))
    times = {name: [] for name, _, _ in configs}
    with tempfile.TemporaryDirectory() as d:
        for r in range(a.runs):  # (in alternation: every configuration once per round)
            for name, binary, extra in configs:
                dt, _ = run(binary, a.input, a.patterns, os.path.join(d, "out.fastq"), extra)
                times[name].append(dt)
    print(f"# {a.input}: {size} compressed bytes, medians of {a.runs} in alternation")
    for name, _, _ in configs:
        t = times[name]
        print(f"{name:28s} median {statistics.median(t):8.3f} s   range {min(t):.3f} - {max(t):.3f} s")


def check(a):
    with tempfile.TemporaryDirectory() as d:
        o1, o2 = os.path.join(d, "dev.fastq"), os.path.join(d, "host.fastq")
        t1, err = run(BIN, a.input, a.patterns, o1, ["--gzip-window", str(a.window_mib * MIB)])
        t2, _ = run(BIN, a.input, a.patterns, o2, ["--host-codec"])
        s1, s2 = sha256(o1), sha256(o2)
    print(f"# {a.input}: {os.path.getsize(a.input)} compressed bytes, window {a.window_mib} MiB")
    print(f"streamed {t1:.3f} s, --host-codec {t2:.3f} s, outputs {'EQUAL' if s1 == s2 else 'DIFFER'} ({s1[:16]} / {s2[:16]})")
    row = summary_row(err)
    print("windows %s, members %s, grown %s, rounds repeated %s, handed back at %s, peak device bytes %s" % row if row else "no summary row: the file was not streamed")
    if s1 != s2:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("sweep", "check"):
        s = sub.add_parser(name)
        s.add_argument("--input", required=True)
        s.add_argument("--patterns", required=True)
    sub.choices["sweep"].add_argument("--runs", type=int, default=5)
    sub.choices["sweep"].add_argument("--parent-bin", default=None)
    sub.choices["check"].add_argument("--window-mib", type=int, default=256)
    a = ap.parse_args()
    (sweep if a.cmd == "sweep" else check)(a)


if __name__ == "__main__":
    main()
