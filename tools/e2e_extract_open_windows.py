#!/usr/bin/env python3
"""End-to-end wall time of `merkurio extract --open-windows` on a bgzip'ed FASTQ against the same command without the flag and, with
--parent BIN, against another build's binary (the parent commit's), on synthetic reads.
usage: tools/e2e_extract_open_windows.py [n_reads, default 20000000] [n_patterns, default 10000] [--reps R, default 5] [--parent BIN]
                                         [--gpus LIST, default 1,2] [--window-mb M, default: the CLI's own] [--step-timeout S, default 300]
                                         [--jobs J, default 16]
Rows: n_reads x 150 bp FASTQ bgzip'ed at zlib level 6 (members of 65 280 bytes of text, written by J processes), `extract -r`, with one
read in five kept and with every read kept, once per entry of --gpus (2 on a one-GPU machine: two handles on the one device).  Every
row runs its modes -- this build with the flag, this build without it, the parent binary -- in alternation, R times, and prints
medians with ranges.  For the runs with the flag it also prints the `[timing] extract --open-windows` row (open windows, seams,
re-runs: a clean file must show 0 re-runs) and, from the per-window rows, the sum of the window calls' times beside the wall time of
the run: a sum above the wall time means that calls overlapped.  The clean file WITHOUT the flag must lie inside the parent's own
range: both ranges are printed side by side.  Every run is one process under its own time limit; the script stops at the first run
that fails or runs out of time.  Results go to stdout: profiles/e2e_extract_open_windows.txt holds this script's output."""
import os, re, statistics, struct, subprocess, sys, time, zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opt(name, default, cast):
    if name in sys.argv:
        k = sys.argv.index(name)
        v = cast(sys.argv[k + 1])
        del sys.argv[k:k + 2]
        return v
    return default


reps = opt("--reps", 5, int)
parent = opt("--parent", None, str)
gpus = [int(x) for x in opt("--gpus", "1,2", str).split(",")]
window_mb = opt("--window-mb", None, str)
step_timeout = opt("--step-timeout", 300, int)
jobs = opt("--jobs", 16, int)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
npat = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
L = 150
MEMBER_TEXT = 65280
rng = np.random.default_rng(2)
tmp = os.environ.get("TMPDIR", "/tmp")
binp = os.environ.get("MERKURIO_BIN") or os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
km = os.path.join(tmp, "e2e_ow_kmers.txt")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
pats = ACGT[rng.integers(0, 4, size=(npat, 31))]
open(km, "wb").write(b"\n".join(p.tobytes() for p in pats) + b"\n")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def members_of(piece):
    """BGZF members (zlib level 6) of a piece of text whose length is a multiple of MEMBER_TEXT, or the file's last piece"""
    out = bytearray()
    for b in range(0, len(piece), MEMBER_TEXT):
        chunk = piece[b:b + MEMBER_TEXT]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def write_bgzipped_fastq(path, every):
    """n reads of 150 bases, one in `every` carries a k-mer, bgzip'ed at level 6"""
    t0 = time.time()
    piece_bytes = MEMBER_TEXT * 256
    carry = b""
    total = 0
    with open(path, "wb") as f, ProcessPoolExecutor(jobs) as pool:
        pending = []

        def drain(all_of_them):
            while pending and (all_of_them or len(pending) >= 2 * jobs):
                f.write(pending.pop(0).result())

        for lo in range(0, n, 1_000_000):
            m = min(1_000_000, n - lo)
            bases = ACGT[rng.integers(0, 4, size=(m, L))]
            idx = np.arange((-lo) % every, m, every)
            bases[idx, 7:38] = pats[(lo + idx) % npat]
            name = np.array([f"@r{i:010d}\n" for i in range(lo, lo + m)], dtype="S13")
            P = name.dtype.itemsize
            rec = np.empty((m, P + L + 3 + L + 1), dtype=np.uint8)
            rec[:, :P] = name.view(np.uint8).reshape(m, P)
            rec[:, P:P + L] = bases
            rec[:, P + L:P + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, P + L + 3:P + 2 * L + 3] = rng.integers(35, 74, size=(m, L), dtype=np.uint8)  # qualities: what keeps real FASTQ from compressing
            rec[:, -1] = 10
            text = carry + rec.tobytes()
            total += rec.size
            whole = len(text) // piece_bytes * piece_bytes
            for b in range(0, whole, piece_bytes):
                pending.append(pool.submit(members_of, text[b:b + piece_bytes]))
            carry = text[whole:]
            drain(False)
        if carry:
            pending.append(pool.submit(members_of, carry))
        drain(True)
        f.write(BGZF_EOF)
    print(f"generated {n} reads, one in {every} with a k-mer ({total / 1e6:.0f} MB of text, {os.path.getsize(path) / 1e6:.0f} MB bgzip'ed) in {time.time() - t0:.1f} s",
          flush=True)


def run(binary, args):
    """one run under its own time limit -> (seconds, stderr); a failure or a time-out ends the script"""
    t0 = time.time()
    try:
        p = subprocess.run([binary, "extract", "-f", km, "-r", *args], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, timeout=step_timeout,
                           env=dict(os.environ, MERKURIO_TIMING="1"))
    except subprocess.TimeoutExpired:
        sys.exit(f"TIMED OUT after {step_timeout} s: {binary} extract {' '.join(args)}")
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}): {binary} extract {' '.join(args)}\n{p.stderr.decode()[-2000:]}")
    return time.time() - t0, p.stderr


def row(label, src, g):
    out = os.path.join(tmp, "e2e_ow_out")
    common = ["-i", src, "--gpus", str(g)] + (["--window-mb", window_mb] if window_mb else [])
    modes = [("--open-windows", binp, ["--open-windows"], "open"), ("without the flag", binp, [], "chain")]
    if parent:
        modes.append(("parent build", parent, [], "parent"))
    times = {m[0]: [] for m in modes}
    summary, calls = [], []
    for rep in range(reps):
        for name, binary, flags, key in modes:
            secs, err = run(binary, [*common, *flags, "-o", out + "_" + key])
            times[name].append(secs)
            call_ms = sum(float(x) for x in re.findall(rb"window \d+: call ([0-9.]+) ms", err))
            if name == "--open-windows":
                m = re.search(rb"extract --open-windows: (\d+) open windows, (\d+) seams, (\d+) re-runs", err)
                summary.append(tuple(int(x) for x in m.groups()) if m else None)
            calls.append((name, secs, call_ms / 1e3, len(re.findall(rb"window \d+: call", err))))
    print(f"== {label}, --gpus {g}", flush=True)
    for name, ts in times.items():
        print(f"  {name}: median {statistics.median(ts):.2f} s [{min(ts):.2f}-{max(ts):.2f}] of {len(ts)}", flush=True)
    print(f"  open windows, seams, re-runs per run with the flag: {summary}", flush=True)
    for name in times:
        rows = [c for c in calls if c[0] == name]
        print(f"  {name}: window calls per run {rows[-1][3]}, sum of their times {statistics.median(c[2] for c in rows):.2f} s beside a wall time of "
              f"{statistics.median(c[1] for c in rows):.2f} s (medians)", flush=True)
    if parent:
        a, b = times["without the flag"], times["parent build"]
        inside = min(b) <= statistics.median(a) <= max(b)
        print(f"  without the flag [{min(a):.2f}-{max(a):.2f}] s against the parent's own range [{min(b):.2f}-{max(b):.2f}] s: median "
              f"{'inside' if inside else 'OUTSIDE'}", flush=True)
    outs = {key: out + "_" + key + ".fastq" for _, _, _, key in modes}
    sizes = {key: os.path.getsize(p) for key, p in outs.items() if os.path.exists(p)}
    print(f"  output bytes: {sizes}", flush=True)
    for p in outs.values():
        if os.path.exists(p):
            os.remove(p)


fq = os.path.join(tmp, "e2e_ow.fastq.gz")
for every, label in ((5, "20 % kept"), (1, "everything kept")):
    write_bgzipped_fastq(fq, every)
    for g in gpus:
        row(f"{n} x 150 bp FASTQ bgzip'ed at level 6, {label}", fq, g)
os.remove(fq)
