"""What the tests of mk_extract_window_frames share (test_gpu_window_frames.py on the device, test_window_frames_cpu.py without one):
the written form restated as in test_gpu_window_members.py, inputs whose WRITTEN record ends lie where the cut rule of
mk_zstd_record_cuts changes its answer, and sparse keeps, where the end table the device hands the cut kernel repeats an end for every
record that is not kept."""
import random

import numpy as np

import zstd_out_cases as zo

P = b"ACGTTGCAAGGCTTAACGGAT"  # what a kept record holds (the other sequences are random: 4^-21 per place)
GRID, TEXT_MAX, REACH = zo.GRID, zo.TEXT_MAX, zo.REACH
# a record end at one of these, or one byte either side, is where a grid point's answer changes: the grid point itself, the last end
# that still snaps (x + REACH - 1), the first that does not (x + REACH), and the next grid point
EDGES = {"grid": GRID, "last_snap": GRID + REACH - 1, "first_raw": GRID + REACH, "two_grids": 2 * GRID}


def rand(rnd, n, alpha=b"ACGT"):
    return bytes(rnd.choices(alpha, k=n))


def seq(rnd, n, hit):
    s = bytearray(rand(rnd, n))
    if hit:
        k = rnd.randrange(0, n - len(P) + 1)
        s[k:k + len(P)] = P
    return bytes(s)


# ---- the written form, restated (include/merkurio_hip.h, THE WRITTEN FORM) ------------------------------------------------------------
def strip(line):
    return line[:-1] if line.endswith(b"\r") else line


def fastq_records(text):
    """the stored records of a FASTQ text: lists of four lines without '\\n' (a '\\r' in front of it is still there)"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [lines[k:k + 4] for k in range(0, len(lines), 4)]


def written_fastq(rec):
    eol = b"\r\n" if len(rec[0]) > 1 and rec[0].endswith(b"\r") else b"\n"
    return strip(rec[0]) + eol + strip(rec[1]) + eol + b"+" + eol + strip(rec[3]) + eol


def fasta_records(text):
    starts = [0] + [k + 1 for k in range(len(text) - 1) if text[k] == 10 and text[k + 1] == 62]
    return [text[a:b] for a, b in zip(starts, starts[1:] + [len(text)])]


def written_fasta(rec):
    """None: a record the device may refuse (its written form is not its bytes with the final line end fixed)"""
    h = rec.find(b"\n")
    if h < 0:
        return None
    eol = b"\r\n" if h > 1 and rec[h - 1:h] == b"\r" else b"\n"
    body = rec[:-2] if rec.endswith(b"\r\n") else rec[:-1] if rec.endswith(b"\n") else rec
    if len(body) <= h + 1 or body[-1:] in (b"\n", b"\r"):
        return None
    return body + eol


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def mixed_fastq(n, seed=3):
    """bare '+', '+id', CRLF, LF header with CRLF body lines, CRLF header with LF body lines; every third record holds P (kept_of),
    the last one among them, which has no line end"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        L = rnd.choice([21, 22, 36, 63, 64, 65, 100, 151, 250])
        rid = b"r%d/%d x" % (i, L) if i % 7 else b""  # (an empty id now and then: "@\r\n" is a header the index takes, "@\n" is not)
        s, q = seq(rnd, L, (n - 1 - i) % 3 == 0), rand(rnd, L, b"@+IJ#5ACGT>")
        shape = i % 5
        if not rid and shape not in (2, 4):
            rid = b"e"
        plus = b"+" + rid if shape == 1 else b"+"
        h_eol = b"\r\n" if shape in (2, 4) else b"\n"
        b_eol = b"\r\n" if shape in (2, 3) else b"\n"
        out.append(b"@" + rid + h_eol + s + b_eol + plus + b_eol + q + b_eol)
    return b"".join(out)[:-1]


def kept_of(n):
    return [(n - 1 - i) % 3 == 0 for i in range(n)]


def fasta_rec(rid, sq, width, eol=b"\n"):
    return b">" + rid + eol + b"".join(sq[k:k + width] + eol for k in range(0, len(sq), width))


def one_line_fasta(rnd, rid, stored, hit):
    """a single-line LF record of exactly `stored` bytes (header line + sequence line, line ends included): its written form is itself"""
    rec = b">" + rid + b"\n" + seq(rnd, stored - len(rid) - 3, hit) + b"\n"
    assert len(rec) == stored
    return rec


def edge_ends(edge, delta, seed=1):
    """written record ends of a text of a little more than two grid steps in which ONE record ends at EDGES[edge] + delta and none
    between the grid point in front of that place and it -- so that this end is the one the grid point's search finds"""
    rnd = random.Random(seed)
    target = EDGES[edge] + delta
    quiet_from = (target - 1) // GRID * GRID - 200 if edge in ("last_snap", "first_raw") else target - 40  # no end in [quiet_from, target)
    ends, at = [], 0
    while at + 3100 < quiet_from:
        at += rnd.choice([60, 200, 331, 1500, 3000])
        ends.append(at)
    ends.append(target)
    at = target
    while at < 2 * GRID + 30000:
        at += rnd.choice([60, 200, 331, 1500, 3000])
        ends.append(at)
    assert target - ([0] + [e for e in ends if e < target])[-1] >= 40 and all(b - a >= 40 for a, b in zip([0] + ends, ends))
    return ends


def edge_is_cut(edge, delta):
    """whether the end at EDGES[edge] + delta of edge_ends is a cut, by the rule's words: a grid point x takes the smallest end e >= x
    if e - x < REACH, else x itself.  An end one byte in front of a grid point is nobody's; the first end that does not snap is
    x + REACH"""
    if edge in ("grid", "two_grids"):
        return delta >= 0
    return EDGES[edge] + delta - GRID < REACH


def fasta_with_written_ends(ends, seed=1):
    """-> (text, keep, written forms of the kept records): kept single-line LF records that end, in the written text, at `ends`, with
    a record that is not kept behind every third of them (the device's end table repeats the end in front of it there)"""
    rnd = random.Random(seed)
    recs, keep, prev = [], [], 0
    for i, e in enumerate(ends):
        recs.append(one_line_fasta(rnd, b"k%d" % i, e - prev, True))
        keep.append(True)
        if i % 3 == 0:
            recs.append(one_line_fasta(rnd, b"d%d" % i, rnd.choice([40, 100, 333]), False))
            keep.append(False)
        prev = e
    written = [r for r, k in zip(recs, keep) if k]
    assert np.cumsum([len(w) for w in written]).tolist() == list(ends)
    return b"".join(recs), keep, written


SPARSE_REC = 313  # "@s%06d\n" + 150 bases + "\n+\n" + 150 qualities + "\n": the stored form is the written one


def sparse_fastq(n=3000, every=50, only=None, seed=17):
    """n records of 313 bytes; every `every`-th holds P -- only: None = all over the text, "first" / "last" = only those whose text
    lies in the first / the last GRID bytes.  -> (text, keep, the n records as rows of a uint8 array)"""
    rng = np.random.default_rng(seed)
    rec = np.empty((n, SPARSE_REC), dtype=np.uint8)
    i = np.arange(n)
    rec[:, 0] = ord("@")
    rec[:, 1] = ord("s")
    for d in range(6):
        rec[:, 2 + d] = 48 + i // 10 ** (5 - d) % 10
    rec[:, 8] = 10
    rec[:, 9:159] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, 150))
    rec[:, 159:162] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 162:312] = rng.choice(np.frombuffer(b"IJ#5F:,", dtype=np.uint8), size=(n, 150))
    rec[:, 312] = 10
    keep = i % every == every // 2
    if only == "first":
        keep &= (i + 1) * SPARSE_REC <= GRID
    elif only == "last":
        keep &= i * SPARSE_REC >= n * SPARSE_REC - GRID
    at = 9 + (i * 7) % (150 - len(P))
    for r in np.flatnonzero(keep):
        rec[r, at[r]:at[r] + len(P)] = np.frombuffer(P, dtype=np.uint8)
    return rec.tobytes(), keep.tolist(), rec
