#!/usr/bin/env python3
"""End-to-end wall time and output size of `merkurio extract -z` (BGZF members that end at record ends) against `-z --host-codec`
(zlib level 6 on the host threads, same cuts) and plain output, on synthetic inputs.
usage: tools/e2e_extract_bgzf_out.py [n_reads, default 8000000] [n_patterns, default 10000] [--reps R, default 5] [--parent BIN]
                                     [--no-fasta] [--fasta-mbp M, default 41.7] [--step-timeout S, default 300] [--no-host-codec]
                                     [--no-sizes] [--sweep]
Rows: n_reads x 150 bp FASTQ with one read in five kept, the same with every read kept, and the genome FASTA row of DESIGN §8
(24 records of M Mbp, 60 columns, every record kept).  Every row runs its modes in alternation, R times, and prints medians with
ranges; --parent BIN adds -z and plain output written by another build's binary (the parent commit's) to the alternation: the
parent's -z is the yardstick of this build's -z (the kept records leave the device as members, mk_extract_window_members), and the
parent's plain output shows that plain output is no slower than before (margin: the parent's own range).  Further rows: the
everything-kept FASTQ bgzip'ed (--host-codec's own output of the row before is the input), and with --sweep `--z-members-from` at 0,
1, 8 and 64 MiB on FASTQ with 1 % and 20 % kept.  --no-host-codec / --no-sizes leave out the zlib runs and the zlib sizes (minutes
on the large rows).  Every run is one process under its own time limit; the
script stops at the first run that fails or runs out of time.  Also printed per row: the [timing] row of the last -z run (members,
cut / deflate / download in ms: the cut kernel beside the deflate launch), and the size of the -z output against zlib levels 1 and 6
on the same kept text.  Results go to stdout: profiles/e2e_extract_bgzf_out.txt is this script's output on one MI355X."""
import os, statistics, subprocess, sys, time, zlib
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
fasta_mbp = opt("--fasta-mbp", 41.7, float)
step_timeout = opt("--step-timeout", 300, int)
def flag(name):
    if name in sys.argv:
        sys.argv.remove(name)
        return True
    return False


no_fasta, no_host_codec, no_sizes, sweep = flag("--no-fasta"), flag("--no-host-codec"), flag("--no-sizes"), flag("--sweep")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
npat = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
L = 150
rng = np.random.default_rng(2)
tmp = os.environ.get("TMPDIR", "/tmp")
binp = os.environ.get("MERKURIO_BIN") or os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
km = os.path.join(tmp, "e2e_z_kmers.txt")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
pats = ACGT[rng.integers(0, 4, size=(npat, 31))]
open(km, "wb").write(b"\n".join(p.tobytes() for p in pats) + b"\n")


def write_fastq(path, every):
    """n reads of 150 bases, one in `every` carries a k-mer"""
    t0 = time.time()
    bases = ACGT[rng.integers(0, 4, size=(n, L))]
    idx = np.arange(0, n, every)
    bases[idx, 7:38] = pats[idx % npat]
    name = np.array([f"@r{i:010d}\n" for i in range(n)], dtype="S13")
    P = name.dtype.itemsize
    rec = np.empty((n, P + L + 3 + L + 1), dtype=np.uint8)
    rec[:, :P] = name.view(np.uint8).reshape(n, P)
    rec[:, P:P + L] = bases
    rec[:, P + L:P + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, P + L + 3:P + 2 * L + 3] = rng.integers(35, 74, size=(n, L), dtype=np.uint8)  # qualities: what keeps real FASTQ from compressing
    rec[:, -1] = 10
    rec.tofile(path)
    print(f"generated {n} reads, one in {every} with a k-mer ({os.path.getsize(path) / 1e6:.0f} MB) in {time.time() - t0:.1f} s", flush=True)


def write_fasta(path):
    t0 = time.time()
    per = int(fasta_mbp * 1e6) // 60 * 60
    with open(path, "wb") as f:
        for r in range(24):
            seq = ACGT[rng.integers(0, 4, size=per)]
            seq[1000:1031] = pats[r % npat]
            lines = np.empty((per // 60, 61), dtype=np.uint8)
            lines[:, :60] = seq.reshape(-1, 60)
            lines[:, 60] = 10
            f.write(b">chr%d\n" % (r + 1))
            lines.tofile(f)
    print(f"generated 24 records of {per / 1e6:.1f} Mbp ({os.path.getsize(path) / 1e6:.0f} MB) in {time.time() - t0:.1f} s", flush=True)


def run(binary, args):
    """one run under its own time limit -> (seconds, stderr); a failure or a time-out ends the script"""
    t0 = time.time()
    try:
        p = subprocess.run([binary, "extract", "-f", km, *args], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, timeout=step_timeout,
                           env=dict(os.environ, MERKURIO_TIMING="1"))
    except subprocess.TimeoutExpired:
        sys.exit(f"TIMED OUT after {step_timeout} s: {binary} extract {' '.join(args)}")
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}): {binary} extract {' '.join(args)}\n{p.stderr.decode()[-2000:]}")
    return time.time() - t0, p.stderr


def row(label, src, ext, modes=None, keep_zhost=None):
    out = os.path.join(tmp, "e2e_z_out")
    sized = modes is None and not no_sizes and not no_host_codec
    if modes is None:
        # (mode, binary, flags, output prefix: one per mode, so that no mode reads or overwrites another's file)
        modes = [("-z", binp, ["-z"], "z"), ("plain output", binp, [], "plain")]
        if not no_host_codec:
            modes.insert(1, ("-z --host-codec", binp, ["-z", "--host-codec"], "zhost"))
        if parent:
            modes += [("-z, parent build", parent, ["-z"], "zparent"), ("plain output, parent build", parent, [], "parent")]
    times = {m[0]: [] for m in modes}
    timing = b""
    windows = {}  # per mode of this build: how many windows left as members / as text, how many window calls were made
    for rep in range(reps):
        for name, binary, flags, key in modes:
            secs, err = run(binary, ["-i", src, "-o", out + "_" + key, *flags])
            times[name].append(secs)
            if binary == binp and "-z" in flags:
                w = [ln.split(b"extract -z: ")[1] for ln in err.split(b"\n") if b"extract -z: " in ln and b"windows as" in ln]
                rep_ = [ln.split(b"; ")[-1] for ln in err.split(b"\n") if b"calls repeated" in ln]
                windows[name] = (w[0].decode() if w else "?") + (", " + rep_[0].decode() if rep_ else "")
            if name == "-z":
                timing = b"\n  ".join(ln for ln in err.split(b"\n") if b"BGZF output" in ln or b"extract -z" in ln)
    print(f"== {label}", flush=True)
    for name, ts in times.items():
        print(f"  {name}: median {statistics.median(ts):.2f} s [{min(ts):.2f}-{max(ts):.2f}] of {len(ts)}" + (f"  ({windows[name]})" if name in windows else ""), flush=True)
    print("  " + timing.decode().strip(), flush=True)
    plain, z, zh = out + "_plain." + ext, out + "_z." + ext + ".gz", out + "_zhost." + ext + ".gz"
    if keep_zhost and os.path.exists(zh):
        os.replace(zh, keep_zhost)
    if not sized:
        for key in [m[3] for m in modes]:
            for p in (out + "_" + key + "." + ext, out + "_" + key + "." + ext + ".gz"):
                if os.path.exists(p):
                    os.remove(p)
        return
    sizes = {1: 0, 6: 0}
    with open(plain, "rb") as f:  # zlib on the kept text in pieces of 64 MB (a stream each: what a parallel gzip would write)
        while True:
            piece = f.read(64 << 20)
            if not piece:
                break
            for lv in sizes:
                sizes[lv] += len(zlib.compress(piece, lv))
    t = os.path.getsize(plain)
    print(f"  kept text {t / 1e6:.0f} MB; -z {os.path.getsize(z) / 1e6:.0f} MB (ratio {t / max(1, os.path.getsize(z)):.2f}), -z --host-codec "
          f"{os.path.getsize(zh) / 1e6:.0f} MB, zlib level 1 {sizes[1] / 1e6:.0f} MB, level 6 {sizes[6] / 1e6:.0f} MB", flush=True)
    for p in (plain, z, zh, out + "_parent." + ext, out + "_zparent." + ext + ".gz"):
        if os.path.exists(p):
            os.remove(p)


fq = os.path.join(tmp, "e2e_z.fastq")
write_fastq(fq, 5)
row(f"{n} x 150 bp FASTQ, 20 % kept", fq, "fastq")
write_fastq(fq, 1)
bz = os.path.join(tmp, "e2e_z_in.fastq.gz")
row(f"{n} x 150 bp FASTQ, everything kept", fq, "fastq", keep_zhost=bz)
if os.path.exists(bz):  # (the zlib-made members of the row above, which hold the input itself: everything was kept)
    row(f"{n} x 150 bp FASTQ, bgzip'ed input, everything kept", bz, "fastq")
    os.remove(bz)
if sweep:
    for every, share in ((100, "1 %"), (5, "20 %")):
        write_fastq(fq, every)
        row(f"{n} x 150 bp FASTQ, {share} kept, --z-members-from sweep", fq, "fastq",
            modes=[(f"-z --z-members-from {mib} MiB", binp, ["-z", "--z-members-from", str(mib << 20)], f"s{mib}") for mib in (0, 1, 8, 64)] +
                  ([("-z, parent build", parent, ["-z"], "zparent")] if parent else []))
os.remove(fq)
if not no_fasta:
    fa = os.path.join(tmp, "e2e_z.fasta")
    write_fasta(fa)
    row(f"genome FASTA, 24 x {fasta_mbp} Mbp, every record kept", fa, "fasta")
    os.remove(fa)
