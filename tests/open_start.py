"""The start rule of mk_extract_window_open (include/merkurio_hip.h) restated in plain Python, and the crafted texts its tests use.

A window may begin anywhere.  The call names the first record start it can find in the window's line table:
  FASTQ  the smallest line j >= 1 at which the record shape holds at j and at j + 4, all eight lines complete (ended by a '\\n')
  FASTA  the smallest line j >= 1 that begins with '>' (inside the text)
Line 0 is never taken.  open_start() is the rule, word for word; record_starts() asks the whole-file reference parser of
tests/ingest_cases.py where records begin."""
import random

import ingest_cases as ic

LF, CRLF = b"\n", b"\r\n"


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def line_starts(text):
    """start[k] = first byte of line k for k = 0 .. total_nl (the last one may be len(text): the empty piece behind a final '\\n')"""
    out = [0]
    pos = text.find(b"\n")
    while pos >= 0:
        out.append(pos + 1)
        pos = text.find(b"\n", pos + 1)
    return out


def fq_shape(text, start, j):
    """the record shape of mk_ingest_records_kernel at line j; lines j .. j + 3 must be complete (j + 4 < len(start))"""
    l0, l1, l2, l3, l4 = start[j:j + 5]
    e1, e3 = l2 - 1, l4 - 1
    if e1 > l1 and text[e1 - 1] == 13:
        e1 -= 1
    if e3 > l3 and text[e3 - 1] == 13:
        e3 -= 1
    return text[l0] == 64 and l1 - l0 >= 3 and l3 - l2 >= 2 and text[l2] == 43 and e3 - l3 == e1 - l1


def open_start(text, fmt="fastq", start=None):
    """-> (line, byte) of the start the rule names in `text`, or None"""
    start = line_starts(text) if start is None else start
    total_nl = len(start) - 1
    if fmt == "fasta":
        for j in range(1, total_nl + 1):
            if start[j] < len(text) and text[start[j]] == 62:
                return j, start[j]
        return None
    for j in range(1, total_nl - 8 + 1):
        if fq_shape(text, start, j) and fq_shape(text, start, j + 4):
            return j, start[j]
    return None


class Cuts:
    """open_start(text[c:]) for many c of one text without re-reading it: the lines of text[c:] behind its line 0 are lines of the
    text, and the shape at a line does not depend on where the window began.  (Checked against open_start on text[c:] by
    tests/test_open_start_cpu.py.)"""

    def __init__(self, text, fmt="fastq"):
        self.text, self.fmt = text, fmt
        self.start = line_starts(text)
        total_nl = len(self.start) - 1
        if fmt == "fasta":
            self.ok = [self.start[j] < len(text) and text[self.start[j]] == 62 for j in range(total_nl + 1)]
        else:
            shape = [j + 4 <= total_nl and fq_shape(text, self.start, j) for j in range(total_nl + 1)]
            self.ok = [j + 8 <= total_nl and shape[j] and shape[j + 4] for j in range(total_nl + 1)]
        # nxt[j] = the smallest line >= j at which the rule holds
        self.nxt = [None] * (total_nl + 2)
        for j in range(total_nl, -1, -1):
            self.nxt[j] = j if self.ok[j] else self.nxt[j + 1]

    def n_front(self, c):
        """bytes in front of the start named in text[c:], or None (status 2)"""
        import bisect
        j = bisect.bisect_right(self.start, c)  # the first line that begins behind byte c: line 1 of text[c:]
        j = self.nxt[j] if j < len(self.nxt) else None
        return None if j is None else self.start[j] - c


def record_starts(text, fmt="fastq"):
    """the true record starts of a whole file, by the reference parser"""
    status, rec_start, _ = (ic.parse_fasta if fmt == "fasta" else ic.parse_fastq)(text, True)
    assert status == 0
    return set(int(x) for x in rec_start[:-1])


# ---- texts ---------------------------------------------------------------------------------------------------------------------------
def _bases(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def kmers(seed=1, n=40, k=21):
    rnd = random.Random(seed)
    return [_bases(rnd, k) for _ in range(n)]


def fq_record(rid, seq, qual, eol=LF, plus_id=False):
    return b"@" + rid + eol + seq + eol + b"+" + (rid if plus_id else b"") + eol + qual + eol


def sweep_fastq(eol=LF, final_eol=True, plus_id=False, seed=3, n_rec=330, planted=None):
    """a few hundred reads of varying length, about 70 KiB; the first dozen are short, so that a sweep over three of them is a few
    hundred cuts.  Quality lines draw from an alphabet with '@' and '+' in it.  -> (text, [sequence])"""
    rnd = random.Random(seed)
    recs, seqs = [], []
    for i in range(n_rec):
        n = rnd.choice([1, 5, 9, 17, 30]) if i < 12 else rnd.choice([1, 31, 36, 75, 100, 150, 151, 250, 301])
        s = bytearray(_bases(rnd, n))
        if planted and n >= 31 and rnd.random() < 0.3:
            p = rnd.choice(planted)
            k = rnd.randrange(0, n - len(p) + 1)
            s[k:k + len(p)] = p
        q = bytes(rnd.choice(b"@+IJ#5F>") for _ in range(n))
        recs.append(fq_record(b"r%d/%d x" % (i, n), bytes(s), q, eol, plus_id))
        seqs.append(bytes(s))
    text = b"".join(recs)
    return (text if final_eol else text[:-len(eol)]), seqs


def sweep_fasta(width, eol=LF, seed=5, n_rec=420, planted=None):
    """records of 0 .. 900 bases wrapped at `width` columns (0: one line), about 80 KiB; the first few are short -> (text, [sequence])"""
    rnd = random.Random(seed * 1000 + width)
    out, seqs = [], []
    for i in range(n_rec):
        n = rnd.choice([0, 3, 61, 85]) if i < 8 else rnd.choice([0, 1, 59, 60, 61, 80, 160, 333, 900])
        s = bytearray(_bases(rnd, n))
        if planted and n >= 59 and rnd.random() < 0.3:
            p = rnd.choice(planted)
            k = rnd.randrange(0, n - len(p) + 1)
            s[k:k + len(p)] = p
        out.append(b">c%d n=%d" % (i, n) + eol)
        step = width if width else max(1, n)
        for k in range(0, n, step):
            out.append(bytes(s[k:k + step]) + eol)
        seqs.append(bytes(s))
    return b"".join(out), seqs


def body_fastq(seed=7, n_rec=40, eol=LF):
    rnd = random.Random(seed)
    out = []
    for i in range(n_rec):
        n = rnd.choice([4, 20, 36, 64])
        out.append(fq_record(b"b%d" % i, _bases(rnd, n), b"I" * n, eol))
    return b"".join(out)


def body_fasta(seed=8, n_rec=30):
    rnd = random.Random(seed)
    return b"".join(b">f%d\n" % i + _bases(rnd, rnd.choice([3, 60, 61])) + b"\n" for i in range(n_rec))


EDGE_BYTES = (63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385)
EDGE_LINES = (255, 256, 257, 4095, 4096, 4097)


def start_at_byte(at, fmt="fastq"):
    """line 0 is the rest of a cut line, `at` bytes with its line end: the first record starts at byte `at`, at line 1"""
    return b"A" * (at - 1) + b"\n" + (body_fasta() if fmt == "fasta" else body_fastq())


def start_at_line(line, fmt="fastq"):
    """`line` lines that start no record in front of the first one: the rule must name line `line`"""
    return b"AC\n" * line + (body_fasta() if fmt == "fasta" else body_fastq())


def one_shape_alone():
    """line 0; lines 1-4 have the record shape; lines 5-7 do not; records from line 8 on.  The shape at line 1 has none at line 5: the
    rule must pass it over and name line 8"""
    return b"IIII\n" + b"@lone\nACGT\n+\nIIII\n" + b"AC\n" * 3 + body_fastq()


def adversarial(n_rec=16, seed=9):
    """quality lines start with '@', sequences with '+', the '+' line repeats the id and so is as long as the header: the shape holds
    at every record's QUALITY line (quality, next header, next sequence, next '+' line), and again four lines on.  -> (text, [sequence])"""
    rnd = random.Random(seed)
    out, seqs = [], []
    for i in range(n_rec):
        n = rnd.choice([6, 9, 14])
        s = b"+" + _bases(rnd, n - 1)
        out.append(fq_record(b"a%02d" % i, s, b"@" + b"I" * (n - 1), LF, plus_id=True))
        seqs.append(s)
    return b"".join(out), seqs
