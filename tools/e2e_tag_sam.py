#!/usr/bin/env python3
"""End-to-end wall time of `merkurio tag` SAM -> SAM on the synthetic records of tools/e2e_tag.py written as plain SAM: the window
path (mk_tag_sam_window, the default) against --host-ingest (the host loop) in the same job, and the window path at several
--window-mb.  Shapes: -m with one record in `every` carrying a k-mer, everything kept, -S -j.
--bam: SAM -> BAM instead (mk_tag_sam_bam_window against the host loop; shapes: everything kept, -m, -m -j; sweep 64 / 128 / 240).
--odd: one kept record in the middle of the second 64 MiB window is one the device refuses (SAM -> SAM: an existing km value of 2 049
bytes; --bam: XF:f:1e-45): that window is the host loop's, the others stay on the device (tools/e2e_tag_window_turn.py times that
against the clean file)
usage: tools/e2e_tag_sam.py [n_records] [n_patterns] [every, default 5] [runs, default 5] [--sweep] [--bam] [--keep] [--odd]"""
import os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = [x for x in sys.argv[1:] if not x.startswith("--")]
n = int(argv[0]) if len(argv) > 0 else 8_000_000
npat = int(argv[1]) if len(argv) > 1 else 10_000
every = int(argv[2]) if len(argv) > 2 else 5
runs = int(argv[3]) if len(argv) > 3 else 5
L = 150
rng = np.random.default_rng(2)
tmp = os.environ.get("TMPDIR", "/tmp")
sam, km, out = os.path.join(tmp, "e2e_w.sam"), os.path.join(tmp, "e2e_w_kmers.txt"), os.path.join(tmp, "e2e_w_out")
t0 = time.time()
pats = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(npat, 31))]
open(km, "wb").write(b"\n".join(p.tobytes() for p in pats) + b"\n")
with open(sam, "wb") as f:
    f.write(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:2000000\n")
    for c0 in range(0, n, 1_000_000):  # a million records at a time: the whole table would be 3 GB of numpy
        m = min(1_000_000, n - c0)
        bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(m, L))]
        idx = np.arange(c0, c0 + m)
        sel = idx % every == 0
        bases[sel, 7:38] = pats[idx[sel] % npat]
        pre = np.array([f"r{i:010d}\t0\tchr1\t{i % 1000000 + 1:07d}\t60\t{L}M\t*\t0\t0\t" for i in range(c0, c0 + m)], dtype="S41")
        P = pre.dtype.itemsize
        rec = np.empty((m, P + L + 1 + L + 1 + 7), dtype=np.uint8)
        rec[:, :P] = pre.view(np.uint8).reshape(m, P)
        rec[:, P:P + L] = bases
        rec[:, P + L] = 9
        rec[:, P + L + 1:P + 2 * L + 1] = ord("I")
        rec[:, P + 2 * L + 1:-1] = np.frombuffer(b"\tNM:i:0", dtype=np.uint8)
        rec[:, -1] = ord("\n")
        odd_at = min(n - 1, int(1.5 * (64 << 20) / rec.shape[1])) // every * every if "--odd" in sys.argv else n
        if c0 <= odd_at < c0 + m:
            rec[:odd_at - c0].tofile(f)
            f.write(rec[odd_at - c0, :-1].tobytes() + (b"\tXF:f:1e-45" if "--bam" in sys.argv else b"\tkm:Z:" + b"A" * 2049) + b"\n")
            rec[odd_at - c0 + 1:].tofile(f)
            continue
        rec.tofile(f)
print(f"generated {n} records ({os.path.getsize(sam) / 1e6:.0f} MB SAM), one in {every} with a k-mer, {npat} 31-mers, in {time.time() - t0:.1f} s", flush=True)
binp = os.environ.get("MERKURIO_BIN") or os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
env = {k: v for k, v in os.environ.items() if k != "MERKURIO_TIMING"}


def timed(args, k):
    ts = []
    for _ in range(k):
        t0 = time.time()
        subprocess.run([binp, "tag", "-f", km, "-i", sam, *args], check=True, env=env, stderr=subprocess.DEVNULL)
        ts.append(time.time() - t0)
    return ts


def row(label, ts):
    print(f"{label:58s} median {statistics.median(ts):6.2f} s  range {min(ts):.2f} .. {max(ts):.2f}  ({len(ts)} runs)  "
          f"{n * L / statistics.median(ts) / 1e9:.3f} Gbases/s", flush=True)


shapes = (("-m", ["-o", out + ".sam", "-m"]), ("everything kept", ["-o", out + ".sam"]), ("-S -j", ["-S", "-j", out + ".json"]))
kind, sizes = "SAM -> SAM", (64, 128, 240, 512)
if "--bam" in sys.argv:
    shapes = (("everything kept", ["-o", out + ".bam"]), ("-m", ["-o", out + ".bam", "-m"]), ("-m -j", ["-o", out + ".bam", "-m", "-j", out + ".json"]))
    kind, sizes = "SAM -> BAM", (64, 128, 240)
timed(shapes[0][1], 1)  # (page cache, output file)
for name, args in shapes:
    row(f"{kind}, {name}, --host-ingest", timed(args + ["--host-ingest"], runs))
    row(f"{kind}, {name}, window path (default window)", timed(args, runs))
if "--sweep" in sys.argv:
    for name, args in shapes[:2]:
        for mb in sizes:
            row(f"{kind}, {name}, window path --window-mb {mb}", timed(args + ["--window-mb", str(mb)], 3))
# where a window's time goes: the phases summed over the windows of one run
for name, args in shapes[:2]:
    p = subprocess.run([binp, "tag", "-f", km, "-i", sam, *args], check=True, env=dict(env, MERKURIO_TIMING="1"), capture_output=True)
    for ln in p.stderr.decode().split("\n"):
        if "windows on the device" in ln:
            print(f"{name}: {ln}", flush=True)
for f in (sam, km, out + ".sam", out + ".bam", out + ".json"):
    if os.path.exists(f) and not (f in (sam, km) and "--keep" in sys.argv):  # (--keep: the input stays, for a kernel trace of one run)
        os.remove(f)
