#!/usr/bin/env python3
"""`merkurio extract` on a .fastq.gz of SEVERAL gzip members (mk_gzip_members_inflate_device) against zlib on the host (--host-codec),
and the one-member file as the guard of the kernels both paths share.  The FASTQ of tools/e2e_gz.py, compressed as (a) one member,
(b) 8 members, (c) members of ~256 KB of text.  Per shape: 5 runs of each binary and mode in alternation, medians of the wall time and
of the phases the [timing] line reports (mk_gzip_info).  --also BIN: another build's CLI (the parent commit's) in the same alternation.
usage: tools/gunzip_members_e2e.py [reads, default 4 000 000] [gzip level, default 6] [--also path/to/merkurio]"""
import os, re, statistics, subprocess, sys, time, zlib
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from bench import _fastq_binned

argv = sys.argv[1:]
also = argv.pop(argv.index("--also") + 1) if "--also" in argv else None
argv = [a for a in argv if a != "--also"]
n = int(argv[0]) if argv else 4_000_000
level = int(argv[1]) if len(argv) > 1 else 6
tmp = os.environ.get("TMPDIR", "/tmp")
bins = [("this build", os.path.join(ROOT, "merkurio_amd", "lib", "merkurio"))] + ([("other build", also)] if also else [])
REC = 13 + 150 + 3 + 150 + 1


def gz_member(text):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    return co.compress(text) + co.flush()


def main():
    rng = np.random.default_rng(9)
    pats = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(10000, 31))]
    km = os.path.join(tmp, "gzm_kmers.txt")
    open(km, "wb").write(b"\n".join(p.tobytes() for p in pats) + b"\n")
    raw = bytearray(_fastq_binned(n, seed=21))
    for i in range(0, n, 100):  # 1 % of the reads carry a k-mer
        raw[i * REC + 13 + 7:i * REC + 13 + 38] = pats[i % 10000].tobytes()
    raw = bytes(raw)
    per_c = max(1, (256 << 10) // REC)
    shapes = [("a: one member", n), ("b: 8 members", (n + 7) // 8), (f"c: members of {per_c * REC // 1024} KB of text", per_c)]
    files = []
    with Pool(min(16, os.cpu_count() or 4)) as pool:
        for label, per in shapes:
            t0 = time.time()
            parts = pool.map(gz_member, [raw[i * REC:min(n, i + per) * REC] for i in range(0, n, per)], chunksize=8)
            p = os.path.join(tmp, f"gzm_{label[0]}.fastq.gz")
            open(p, "wb").write(b"".join(parts))
            print(f"{label}: {n} reads, {len(raw) / 1e6:.0f} MB of FASTQ -> {len(parts)} members, {os.path.getsize(p) / 1e6:.0f} MB (gzip -{level}, {time.time() - t0:.0f} s)", flush=True)
            files.append((label, p, len(parts)))
    del raw
    out = os.path.join(tmp, "gzm_out")
    phase = re.compile(r"gzip input 0 on the device: (taken|NOT taken[^,]*), (?:(\d+) members proved, )?([\d.]+) s \((\d+) pieces; upload ([\d.]+), block search ([\d.]+), pieces ([\d.]+), resolution ([\d.]+), CRC ([\d.]+) ms\)")

    def run(binp, path, extra):
        t0 = time.time()
        r = subprocess.run([binp, "extract", "-i", path, "-f", km, "-o", out, *extra], env=dict(os.environ, MERKURIO_TIMING="1"), capture_output=True, text=True)
        dt = time.time() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        return dt, phase.search(r.stderr), os.path.getsize(out + ".fastq")

    for label, path, members in files:
        modes = [(f"{name}, device", b, []) for name, b in bins] + [("this build, --host-codec", bins[0][1], ["--host-codec"])]
        walls, phases, sizes, said = {m[0]: [] for m in modes}, {m[0]: [] for m in modes}, set(), {}
        for rep in range(5):
            for mode, b, extra in modes:
                dt, m, size = run(b, path, extra)
                walls[mode].append(dt), sizes.add(size)
                if m:
                    said[mode] = f"{m.group(1)}, {m.group(2) or '?'} members proved, {m.group(4)} pieces"
                    phases[mode].append([float(m.group(3)) * 1e3] + [float(m.group(k)) for k in range(5, 10)])
        assert len(sizes) == 1, sizes
        print(f"{label} ({members} members): output {sizes.pop()} bytes in every run")
        for mode, _, _ in modes:
            w = walls[mode]
            line = f"  {mode:28s} wall median {statistics.median(w):.2f} s (min {min(w):.2f}, max {max(w):.2f})"
            if phases[mode]:
                med = [statistics.median(c) for c in zip(*phases[mode])]
                lo, hi = min(p[0] for p in phases[mode]), max(p[0] for p in phases[mode])
                line += f"\n      {said[mode]}; gunzip call median {med[0]:.0f} ms (min {lo:.0f}, max {hi:.0f}): upload {med[1]:.1f}, block search {med[2]:.1f}, pieces {med[3]:.1f}, resolution {med[4]:.1f}, CRC {med[5]:.1f} ms"
            print(line, flush=True)
    for _, p, _ in files:
        os.remove(p)


if __name__ == "__main__":
    main()
