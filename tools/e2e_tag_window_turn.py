#!/usr/bin/env python3
"""What one record the device refuses costs `merkurio tag` end to end: BAM -> SAM -m and SAM -> BAM -m on the synthetic records of
tools/e2e_tag_sam.py, a clean file beside the same file with ONE refusing kept record in the middle of the direction's second
default window (BAM -> SAM: XE:f:1e-05 in the second 240 MiB window of BAM text; SAM -> BAM: XF:f:1e-45 in the second 64 MiB window),
on this build and on another build of the CLI (MERKURIO_PARENT_BIN: the commit before the window turn) in the same job.  The four
(build, file) rows of a direction are timed in turn, round after round; medians with ranges, then each row's own window rows under
MERKURIO_TIMING=1 (which window was left to the host, how many ran where).
usage: tools/e2e_tag_window_turn.py [n_records, default 8 000 000] [n_patterns, default 10 000] [every, default 5] [runs, default 5]"""
import os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
n = int(argv[0]) if len(argv) > 0 else 8_000_000
npat = int(argv[1]) if len(argv) > 1 else 10_000
every = int(argv[2]) if len(argv) > 2 else 5
runs = int(argv[3]) if len(argv) > 3 else 5
L = 150
tmp = os.environ.get("TMPDIR", "/tmp")
this = os.environ.get("MERKURIO_BIN") or os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
parent = os.environ.get("MERKURIO_PARENT_BIN")
km = os.path.join(tmp, "e2e_t_kmers.txt")
LINE = 41 + L + 1 + L + 1 + 7  # bytes of a line
BAM_REC = 36 + 12 + 4 + (L + 1) // 2 + L + 4 + 4  # fixed fields, name, one CIGAR op, SEQ, QUAL, NM as one byte, an empty zz:Z:


def write_sam(path, odd_at, field):
    """the records of tools/e2e_tag_sam.py (the same seed: the same bytes every time); record odd_at (None: none) carries `field` too"""
    rng = np.random.default_rng(2)
    pats = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(npat, 31))]
    open(km, "wb").write(b"\n".join(p.tobytes() for p in pats) + b"\n")
    with open(path, "wb") as f:
        f.write(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:2000000\n")
        for c0 in range(0, n, 1_000_000):
            m = min(1_000_000, n - c0)
            bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(m, L))]
            idx = np.arange(c0, c0 + m)
            sel = idx % every == 0
            bases[sel, 7:38] = pats[idx[sel] % npat]
            pre = np.array([f"r{i:010d}\t0\tchr1\t{i % 1000000 + 1:07d}\t60\t{L}M\t*\t0\t0\t" for i in range(c0, c0 + m)], dtype="S41")
            P = pre.dtype.itemsize
            rec = np.empty((m, LINE), dtype=np.uint8)
            rec[:, :P] = pre.view(np.uint8).reshape(m, P)
            rec[:, P:P + L] = bases
            rec[:, P + L] = 9
            rec[:, P + L + 1:P + 2 * L + 1] = ord("I")
            rec[:, P + 2 * L + 1:-1] = np.frombuffer(b"\tNM:i:0", dtype=np.uint8)
            rec[:, -1] = ord("\n")
            if odd_at is not None and c0 <= odd_at < c0 + m:
                rec[:odd_at - c0].tofile(f)
                f.write(rec[odd_at - c0, :-1].tobytes() + field + b"\n")
                rec[odd_at - c0 + 1:].tofile(f)
            else:
                rec.tofile(f)


def kept(at):  # a record with a k-mer: -m keeps it
    return min(n - 1, at) // every * every


t0 = time.time()
clean_sam, odd_sam, clean_bam, odd_bam = (os.path.join(tmp, "e2e_t_" + x) for x in ("clean.sam", "odd.sam", "clean.bam", "odd.bam"))
out = os.path.join(tmp, "e2e_t_out")
odd_bam_at, odd_sam_at = kept(int(1.5 * (240 << 20) / BAM_REC)), kept(int(1.5 * (64 << 20) / LINE))
# (the input BAMs are written with another tag name, as in tools/e2e_tag.py: records that already carry `km` take the merge rule)
write_sam(odd_sam, odd_bam_at, b"\tXE:f:1e-05")
subprocess.run([this, "tag", "-f", km, "-i", odd_sam, "-o", odd_bam, "-t", "zz"], check=True)
write_sam(clean_sam, None, b"")
subprocess.run([this, "tag", "-f", km, "-i", clean_sam, "-o", clean_bam, "-t", "zz"], check=True)
write_sam(odd_sam, odd_sam_at, b"\tXF:f:1e-45")
print(f"{n} records of {L} bases, {npat} 31-mers, one record in {every} with a k-mer; odd record {odd_bam_at} (BAM) / {odd_sam_at} (SAM); "
      f"inputs made in {time.time() - t0:.0f} s", flush=True)
env = {k: v for k, v in os.environ.items() if k != "MERKURIO_TIMING"}
builds = [("this commit", this)] + ([("parent commit", parent)] if parent else [])
for kind, files, o in (("BAM -> SAM -m", (("clean", clean_bam), ("odd", odd_bam)), out + ".sam"),
                       ("SAM -> BAM -m", (("clean", clean_sam), ("odd", odd_sam)), out + ".bam")):
    rows = [(b, binp, fl, path) for b, binp in builds for fl, path in files]
    times = {r[:3:2]: [] for r in rows}
    for r in rows[:1]:  # (page cache, output file)
        subprocess.run([r[1], "tag", "-f", km, "-i", r[3], "-o", o, "-m"], check=True, env=env, stderr=subprocess.DEVNULL)
    for _ in range(runs):
        for b, binp, fl, path in rows:
            t0 = time.time()
            subprocess.run([binp, "tag", "-f", km, "-i", path, "-o", o, "-m"], check=True, env=env, stderr=subprocess.DEVNULL)
            times[(b, fl)].append(time.time() - t0)
    for b, binp, fl, path in rows:
        ts = times[(b, fl)]
        print(f"{kind}, {b:13s}, {fl:5s} file: median {statistics.median(ts):5.2f} s  range {min(ts):.2f} .. {max(ts):.2f}  ({len(ts)} runs)", flush=True)
    for b, binp, fl, path in rows:
        p = subprocess.run([binp, "tag", "-f", km, "-i", path, "-o", o, "-m"], check=True, env=dict(env, MERKURIO_TIMING="1"), capture_output=True)
        for ln in p.stderr.decode().split("\n"):
            if (" of " in ln and "windows on the device (" in ln) or "left to the host" in ln or "windows on the device (the rest" in ln:
                print(f"  {b}, {fl}: {ln}", flush=True)
for f in (clean_sam, odd_sam, clean_bam, odd_bam, km, out + ".sam", out + ".bam"):
    if os.path.exists(f):
        os.remove(f)
