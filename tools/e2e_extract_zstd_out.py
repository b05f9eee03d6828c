#!/usr/bin/env python3
"""extract --zstd-output end to end: output size and speed, appended to profiles/e2e_extract_zstd_out.txt.

    tools/e2e_extract_zstd_out.py --sizes FASTQ [FASTA ...] -s PATTERN
        bytes written per input by --zstd-output (device), --zstd-output --host-codec (libzstd level 3 at the same cuts),
        libzstd level 1 at the same cuts (recompressed here from the frames' texts) and -z (BGZF)
    tools/e2e_extract_zstd_out.py --parent BIN FASTQ [FASTA ...] -s PATTERN
        wall seconds, medians of 5 with the two builds in alternation: this build's --zstd-output, -z and plain output against
        the parent build's --zstd-output (the yardstick: there the kept records are formatted by the host writer and compressed on
        the first device; here they leave their window's device as frames, mk_extract_window_frames), -z and plain output
    tools/e2e_extract_zstd_out.py --workloads [--reads N, default 8000000] [--parent BIN] [--sweep] [--fasta-mbp M, default 41.7]
        the same alternation on synthetic inputs made here: N x 150 bp FASTQ with 1 %, 20 % and 100 % of the reads kept, the 100 % input
        bgzip'ed (by this build's -z --host-codec), and a genome-like FASTA (24 records of M Mbp, every record kept).  Per row: this
        build's --zstd-output and plain output and, with --parent, the parent's two; medians of 5 with ranges, and the [timing] rows of
        the last --zstd-output run (frames from the window path / the gathering path, written-form kernels, cut + deflate, download).
        --sweep adds `--z-members-from` at 1, 8 and 64 MiB on the 1 % and 20 % inputs.  Every run is a process of its own under a
        time limit (--step-timeout, 300 s); the script stops at the first that fails.

Needs a GPU.  Nothing here is run by the tests."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
OUT = os.path.join(ROOT, "profiles", "e2e_extract_zstd_out.txt")


def written(binary, src, pattern, flags, work):
    out = os.path.join(work, "out" + os.path.splitext(src)[1])
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    t0 = time.perf_counter()
    subprocess.run([binary, "extract", "-i", src, "-s", pattern, *flags, "-o", out], check=True, capture_output=True)
    dt = time.perf_counter() - t0
    (path,) = [os.path.join(work, f) for f in os.listdir(work)]
    return path, os.path.getsize(path), dt


def level1_size(path):
    """the frames' texts compressed again by libzstd level 1, a frame each: the same cuts"""
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_findFrameCompressedSize.restype = z.ZSTD_decompress.restype = z.ZSTD_compress.restype = z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_findFrameCompressedSize.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    blob, at, total = open(path, "rb").read(), 0, 0
    text, room = ctypes.create_string_buffer(131072 + 8), ctypes.create_string_buffer(z.ZSTD_compressBound(131072))
    while at < len(blob):
        k = z.ZSTD_findFrameCompressedSize(blob[at:at + 131072 + 64], min(len(blob) - at, 131072 + 64))
        n = z.ZSTD_decompress(text, len(text), blob[at:at + k], k)
        total += z.ZSTD_compress(room, len(room), text.raw[:n], n, 1) + 4  # (+ the checksum the other rows carry)
        at += k
    return total


def timed(binary, args, limit):
    """one run under its own time limit -> (seconds, stderr); a failure or a time-out ends the script"""
    t0 = time.perf_counter()
    try:
        p = subprocess.run([binary, "extract", *args], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, timeout=limit, env=dict(os.environ, MERKURIO_TIMING="1"))
    except subprocess.TimeoutExpired:
        sys.exit("TIMED OUT after %d s: %s extract %s" % (limit, binary, " ".join(args)))
    if p.returncode != 0:
        sys.exit("FAILED (%d): %s extract %s\n%s" % (p.returncode, binary, " ".join(args), p.stderr.decode()[-2000:]))
    return time.perf_counter() - t0, p.stderr.decode()


def workloads(a, rows):
    """the synthetic rows: modes in alternation, medians of 5 with ranges"""
    import numpy as np
    rng = np.random.default_rng(2)
    work = tempfile.mkdtemp(prefix="e2e_zstd_", dir=os.environ.get("TMPDIR"))
    n, L, npat = a.reads, 150, 10000
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats = acgt[rng.integers(0, 4, size=(npat, 31))]
    km = os.path.join(work, "kmers.txt")
    open(km, "wb").write(b"\n".join(p.tobytes() for p in pats) + b"\n")

    def write_fastq(path, every):
        bases = acgt[rng.integers(0, 4, size=(n, L))]
        idx = np.arange(0, n, every)
        bases[idx, 7:38] = pats[idx % npat]
        name = np.array(["@r%010d\n" % i for i in range(n)], dtype="S13")
        rec = np.empty((n, 13 + L + 3 + L + 1), dtype=np.uint8)
        rec[:, :13] = name.view(np.uint8).reshape(n, 13)
        rec[:, 13:13 + L] = bases
        rec[:, 13 + L:16 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
        rec[:, 16 + L:16 + 2 * L] = rng.integers(35, 74, size=(n, L), dtype=np.uint8)
        rec[:, -1] = 10
        rec.tofile(path)

    def write_fasta(path):
        per = int(a.fasta_mbp * 1e6) // 60 * 60
        with open(path, "wb") as f:
            for r in range(24):
                sq = acgt[rng.integers(0, 4, size=per)]
                sq[1000:1031] = pats[r % npat]
                lines = np.empty((per // 60, 61), dtype=np.uint8)
                lines[:, :60] = sq.reshape(-1, 60)
                lines[:, 60] = 10
                f.write(b">chr%d\n" % (r + 1))
                lines.tofile(f)

    def row(label, src, modes=None):
        if modes is None:
            modes = [("--zstd-output", BIN, ["--zstd-output"]), ("plain output", BIN, [])]
            if a.parent:
                modes += [("--zstd-output, parent build", a.parent, ["--zstd-output"]), ("plain output, parent build", a.parent, [])]
        secs, timing = {m[0]: [] for m in modes}, ""
        for _ in range(5):
            for k, (name, binary, flags) in enumerate(modes):  # (in alternation; an output prefix per mode)
                dt, err = timed(binary, ["-f", km, "-i", src, "-o", os.path.join(work, "out%d" % k), *flags], a.step_timeout)
                secs[name].append(dt)
                if binary == BIN and "--zstd-output" in flags:
                    timing = "; ".join(ln[9:] for ln in err.splitlines() if "zstd output" in ln or "extract --zstd-output" in ln)
        rows.append("== " + label)
        for name, ts in secs.items():
            rows.append("  %s: median %.2f s [%.2f-%.2f] of %d" % (name, statistics.median(ts), min(ts), max(ts), len(ts)))
        rows.append("  last --zstd-output run: " + timing)
        for f in os.listdir(work):
            if f.startswith("out"):
                os.remove(os.path.join(work, f))

    fq, bz, fa = (os.path.join(work, x) for x in ("in.fastq", "in_bgzf.fastq.gz", "in.fasta"))
    for every, share in ((100, "1 %"), (5, "20 %"), (1, "100 %")):
        write_fastq(fq, every)
        row("%d x 150 bp FASTQ, %s kept" % (n, share), fq)
        if a.sweep and every != 1:
            row("%d x 150 bp FASTQ, %s kept, --z-members-from sweep" % (n, share), fq,
                [("--zstd-output --z-members-from %d MiB" % mib, BIN, ["--zstd-output", "--z-members-from", str(mib << 20)]) for mib in (1, 8, 64)])
    timed(BIN, ["-f", km, "-i", fq, "-z", "--host-codec", "-o", os.path.join(work, "in_bgzf")], 4 * a.step_timeout)  # (everything kept: the output is the input)
    os.remove(fq)
    row("%d x 150 bp FASTQ, bgzip'ed input, 100 %% kept" % n, bz)
    os.remove(bz)
    write_fasta(fa)
    row("genome-like FASTA, 24 x %.1f Mbp, every record kept" % a.fasta_mbp, fa)
    os.remove(fa), os.remove(km), os.rmdir(work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inputs", nargs="*")
    ap.add_argument("-s")
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--workloads", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--fasta-mbp", type=float, default=41.7)
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.inputs and not a.s:
        ap.error("inputs need -s PATTERN")
    rows = []
    if a.workloads:
        workloads(a, rows)
    with tempfile.TemporaryDirectory() as work:
        for src in a.inputs:
            if a.sizes:
                dev, n_dev, _ = written(BIN, src, a.s, ["--zstd-output"], work)
                l1 = level1_size(dev)
                _, n_l3, _ = written(BIN, src, a.s, ["--zstd-output", "--host-codec"], work)
                _, n_gz, _ = written(BIN, src, a.s, ["-z"], work)
                _, n_txt, _ = written(BIN, src, a.s, [], work)
                rows.append("sizes %s: text %d, --zstd-output %d, libzstd-1 %d, libzstd-3 %d, -z %d" % (os.path.basename(src), n_txt, n_dev, l1, n_l3, n_gz))
            if a.parent:
                runs = {"zstd": (BIN, ["--zstd-output"]), "z": (BIN, ["-z"]), "plain": (BIN, []), "parent-zstd": (a.parent, ["--zstd-output"]),
                        "parent-z": (a.parent, ["-z"]), "parent-plain": (a.parent, [])}
                secs = {k: [] for k in runs}
                for _ in range(5):
                    for k, (binary, flags) in runs.items():  # (in alternation)
                        secs[k].append(written(binary, src, a.s, flags, work)[2])
                rows.append("speed %s: " % os.path.basename(src) + ", ".join("%s %.3f s" % (k, statistics.median(v)) for k, v in secs.items()))
    with open(OUT, "a") as f:
        for r in rows:
            print(r)
            f.write(r + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
