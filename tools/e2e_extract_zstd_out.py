#!/usr/bin/env python3
"""extract --zstd-output end to end: output size and speed, appended to profiles/e2e_extract_zstd_out.txt.

    tools/e2e_extract_zstd_out.py --sizes FASTQ [FASTA ...] -s PATTERN
        bytes written per input by --zstd-output (device), --zstd-output --host-codec (libzstd level 3 at the same cuts),
        libzstd level 1 at the same cuts (recompressed here from the frames' texts) and -z (BGZF)
    tools/e2e_extract_zstd_out.py --parent BIN FASTQ [FASTA ...] -s PATTERN
        wall seconds, medians of 5 with the two builds in alternation: this build's --zstd-output, -z and plain output against
        the parent build's -z and plain output

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("-s", required=True)
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--parent")
    a = ap.parse_args()
    rows = []
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
                runs = {"zstd": (BIN, ["--zstd-output"]), "z": (BIN, ["-z"]), "plain": (BIN, []), "parent-z": (a.parent, ["-z"]), "parent-plain": (a.parent, [])}
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
