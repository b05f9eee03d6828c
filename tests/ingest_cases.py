"""Crafted FASTQ / FASTA texts for the ingest kernels (merkurio_amd/csrc/ingest.hip), the reference parsers that say what every
text means, and the helpers that make the device's record table and gathered sequences observable through the ABI.

The kernels cut a text into shares of 64 bytes (a thread), 4096 bytes (a wave) and 16 KiB (a block), records into groups of 16
(gather), 256 (record lanes) and 4096 (offset tiles), and loop over blocks and tiles 1024 at a time.  Every case here puts a chosen
byte at a chosen edge and says so: a builder returns its text together with the claims (what, edge, delta) that hold for it,
computed from the finished text by `fastq_claims` / `fasta_claims`, never from the builder's plan.  tests/test_ingest_cases_cpu.py
checks the claims and the texts without a device; tests/test_gpu_ingest_edges.py runs them.

Nothing here shares code with merkurio_amd/: the parsers restate the rule in the header comment of ingest.hip (4-line FASTQ, LF or
CRLF, '@' id / sequence / '+...' / quality of equal length, a header line of '@' alone -- "@\\n" -- refused) and the FASTA rule of
tests/test_gpu_windows.py::_parse_fasta (a line that starts with '>' is a header, every other line is sequence without its '\\n'
and '\\r' bytes)."""
import ctypes as C
import itertools
import random

import numpy as np

EDGES = (64, 4096, 16384, 32768)
DELTAS = (-2, -1, 0, 1)
BLOCK = 16384
LINES = ("hdr", "seq", "plus", "qual")
LF, CRLF = b"\n", b"\r\n"
EOLS = {"lf": LF, "crlf": CRLF}
SMALL_READS = (b"AC", b"G", b"ACG", b"CGA")  # only ACG holds the 3-mer; AC + G, ACG + ..., CGA + CG ... make it across records
K3 = b"ACG"
BIG_RECORDS = 4_194_304 + 4097  # 1024 offset tiles and one more round, then a tile and a record


# ---- reference parsers ---------------------------------------------------------------------------------------------------------
def fastq_lines(text, ends_at_record=True):
    """the 4-line records of `text` as arrays: (status, start[n, 4], end[n, 4], cr[n, 4], end_of_records).  start / end: a line
    without its line end; cr: the line end is CRLF (or a last line ends in a lone '\\r').  status 1: not plain 4-line FASTQ.
    ends_at_record=False: text may stop anywhere; only lines that end in '\\n' count and whole records of four of them."""
    b = np.frombuffer(text, dtype=np.uint8)
    n = len(b)
    nl = np.flatnonzero(b == 10).astype(np.int64)
    n_lines = len(nl) + (1 if ends_at_record and n and b[-1] != 10 else 0)
    none = np.zeros((0, 4), dtype=np.int64)
    if ends_at_record and n_lines % 4:
        return 1, none, none, none.astype(bool), 0
    n_rec = n_lines // 4
    start = np.concatenate(([0], nl + 1))
    end = np.concatenate((nl, [n]))
    end_of_records = n if ends_at_record else int(start[4 * n_rec])
    s = start[:4 * n_rec].reshape(n_rec, 4)
    e = end[:4 * n_rec].reshape(n_rec, 4)
    if n_rec == 0:
        return 0, none, none, none.astype(bool), end_of_records
    cr = (e > s) & (b[np.maximum(e, 1) - 1] == 13)
    e = e - cr
    # '@' and at least one more byte in front of the '\n': "@\n" is refused; "@\r\n" is taken, with an empty id (the device's written
    # form of such a record is pinned by tests/test_gpu_window_members.py::test_fastq_mixed_shapes)
    ok = (b[s[:, 0]] == ord("@")) & (e[:, 0] + cr[:, 0] - s[:, 0] >= 2)
    ok &= (e[:, 2] > s[:, 2]) & (b[np.minimum(s[:, 2], n - 1)] == ord("+"))
    ok &= (e[:, 3] - s[:, 3]) == (e[:, 1] - s[:, 1])
    if not ok.all():
        return 1, none, none, none.astype(bool), 0
    return 0, s, e, cr, end_of_records


def parse_fastq(text, ends_at_record=True):
    """-> (status, rec_start with the end entry (np.uint64), sequences)"""
    status, s, e, _, end = fastq_lines(text, ends_at_record)
    if status:
        return 1, np.zeros(0, dtype=np.uint64), []
    rec_start = np.concatenate((s[:, 0], [end])).astype(np.uint64)
    return 0, rec_start, [text[a:z] for a, z in zip(s[:, 1].tolist(), e[:, 1].tolist())]


def fasta_lines(text):
    """every line of `text`: (start, end without the line end, is CRLF, is header) as lists"""
    out = []
    pos = 0
    for line in text.split(b"\n"):
        cr = line.endswith(b"\r")
        out.append((pos, pos + len(line) - cr, cr, line.startswith(b">")))
        pos += len(line) + 1
    if out and out[-1][0] >= len(text):  # the empty piece behind a final '\n' is no line
        out.pop()
    return out


def parse_fasta(text, ends_at_record=True):
    """-> (status, rec_start with the end entry (np.uint64), sequences); status 1: the text does not start with a header.
    ends_at_record=False: the last record may go on in the next window and is left out; the end entry is its start."""
    if not text:
        return 0, np.zeros(1, dtype=np.uint64), []
    if text[:1] != b">":
        return 1, np.zeros(0, dtype=np.uint64), []
    starts, seqs = [], []
    pos = 0
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            starts.append(pos)
            seqs.append(bytearray())
        else:
            seqs[-1] += line.replace(b"\r", b"")
        pos += len(line) + 1
    end = len(text)
    if not ends_at_record:
        end = starts.pop()
        seqs.pop()
    return 0, np.array(starts + [end], dtype=np.uint64), [bytes(s) for s in seqs]


# ---- what a text places where -------------------------------------------------------------------------------------------------
def _claims_of(what, positions, out):
    p = np.asarray(positions, dtype=np.int64)
    for edge in EDGES:
        d = (p + 2) % edge - 2
        for delta in np.unique(d[d <= 1]).tolist():
            out.add((what, edge, int(delta)))


def fastq_claims(text):
    """{(what, edge, delta)}: what = 'hdr' | 'seq' | 'plus' | 'qual' (the first byte of that line of some record), that + '_nl' (its
    '\\n') or that + '_cr' (the '\\r' in front of it); the byte lies at a multiple of edge plus delta"""
    status, s, e, cr, _ = fastq_lines(text)
    assert status == 0
    out = set()
    for k, name in enumerate(LINES):
        _claims_of(name, s[:, k], out)
        nl = e[:, k] + cr[:, k]
        nl = nl[nl < len(text)]  # (a last line without its line end)
        _claims_of(name + "_nl", nl, out)
        _claims_of(name + "_cr", e[cr[:, k], k], out)
    return out


def fastq_required(edge, eol):
    whats = [w + t for w in LINES for t in (("", "_nl", "_cr") if eol == CRLF else ("", "_nl"))]
    return {(w, edge, d) for w in whats for d in DELTAS}


def fasta_claims(text):
    """as fastq_claims with what = 'gt' (a header's '>'), 'hdr_nl' / 'hdr_cr', 'seq' (first byte of a sequence line), 'seq_nl' /
    'seq_cr'; and ('hdr_crosses', 16384, 0): a header line lies in two blocks, ('hdr_covers', 16384, 0): in three or more (a whole
    block of header bytes)"""
    out = set()
    pos = {"gt": [], "hdr_nl": [], "hdr_cr": [], "seq": [], "seq_nl": [], "seq_cr": []}
    for a, z, cr, hdr in fasta_lines(text):
        kind = "hdr" if hdr else "seq"
        if z + cr > a:
            pos["gt" if hdr else "seq"].append(a)
        if cr:
            pos[kind + "_cr"].append(z)
        if z + cr < len(text):
            pos[kind + "_nl"].append(z + cr)
        if hdr and z > a:
            blocks = (z - 1) // BLOCK - a // BLOCK
            if blocks >= 1:
                out.add(("hdr_crosses", BLOCK, 0))
            if blocks >= 2:
                out.add(("hdr_covers", BLOCK, 0))
    for what, p in pos.items():
        if p:
            _claims_of(what, p, out)
    return out


def fasta_required(eol):
    edges = (64, 4096, 16384)
    req = {("gt", e, 0) for e in edges} | {("hdr_crosses", BLOCK, 0), ("hdr_covers", BLOCK, 0)}
    req |= {("seq_nl", e, d) for e in edges for d in (-1, 0)} | {("hdr_nl", e, d) for e in edges for d in (-1, 0)}
    if eol == CRLF:
        req |= {(w, e, -1) for w in ("hdr_cr", "seq_cr") for e in edges}
    return req


# ---- text builders -------------------------------------------------------------------------------------------------------------
def _bases(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


def _qual(rnd, n):
    """quality strings that start with '@', '+' or '>' and hold sequence letters: lines are counted, not guessed"""
    if not n:
        return b""
    return bytes([rnd.choice(b"@+>I")]) + bytes(rnd.choice(b"IJ#5ACGT@+") for _ in range(n - 1))


def fq_record(rid, seq, eol, qual=None, plus=b"+"):
    return b"@" + rid + eol + seq + eol + plus + eol + (b"I" * len(seq) if qual is None else qual) + eol


class _Text:
    """a text under construction; fill_to pads the id of one more record so that the text then has `target` bytes"""

    def __init__(self, rnd, eol, fasta=False):
        self.rnd, self.eol, self.fasta, self.parts, self.n, self.k = rnd, eol, fasta, [], 0, 0

    def add(self, piece):
        self.parts.append(piece)
        self.n += len(piece)

    def _filler(self, pad):
        rid = b"f%d." % self.k + b"x" * pad
        seq = bytes(b"ACGT"[(self.k * 7 + j * j + j // 3) % 4] for j in range(4 + self.k % 7))
        if self.fasta:
            return b">" + rid + self.eol + seq + self.eol
        return fq_record(rid, seq, self.eol, b"+" + b"J" * (len(seq) - 1))

    def fill_to(self, target):
        pad = target - self.n - len(self._filler(0))
        if pad < 0:  # no room for a record: the caller wants the next multiple
            return False
        self.add(self._filler(pad))
        self.k += 1
        assert self.n == target
        return True

    def bytes(self):
        return b"".join(self.parts)


def fq_edges(edge, eol, seed=1):
    """one short record per multiple of `edge`, each shifted one byte against the last, so that every line's first byte, '\\n' and
    '\\r' passes through offsets -2 .. +1 of a multiple; the room in between is the padded id of one more record (a header line of
    up to 32 KiB: whole blocks without a newline)"""
    rnd = random.Random(seed)
    t = _Text(rnd, eol)
    probe = fq_record(b"p", b"ACGT", eol)
    s, e, cr = (x[0] for x in fastq_lines(probe)[1:4])
    offs = set(s.tolist()) | set((e + cr).tolist()) | set(e[cr].tolist())
    shifts = sorted({d - o for o in offs for d in DELTAS}, reverse=True)
    mult = 0
    for sh in shifts:
        mult += 1
        while not t.fill_to(mult * edge + sh):
            mult += 1
        seq = _bases(rnd, 4)
        t.add(fq_record(b"p", seq, eol, _qual(rnd, 4)))
    t.fill_to(t.n + 40)
    return t.bytes()


def fq_dense_sparse(eol, seed=2):
    """runs of records of empty reads (7 bytes each with LF: about 36 newlines per thread) between reads of 20 000 and 40 000 bases,
    whose sequence and quality lines leave two or three blocks in a row without a newline"""
    rnd = random.Random(seed)
    empty = fq_record(b"a", b"", eol)
    parts = [empty * 3000, fq_record(b"long1", _bases(rnd, 20_000), eol), empty * 2500,
             fq_record(b"long2", _bases(rnd, 40_000), eol, b"@" * 40_000), empty * 100]
    parts += [fq_record(b"r%d" % i, _bases(rnd, 30 + i), eol) for i in range(5)]
    parts += [empty * 20]
    return b"".join(parts)


def fq_of_length(n, eol, final_eol, seed=3, fasta=False):
    """a text of exactly n bytes that ends with or without a line end (CRLF: without both bytes)"""
    rnd = random.Random(seed + n)
    t = _Text(rnd, eol, fasta)
    total = n if final_eol else n + len(eol)
    while total - t.n > 400:
        t.fill_to(t.n + rnd.randrange(60, 200))
    if not t.fill_to(total):  # (no room for a whole record: a shorter text before)
        raise ValueError("text too short")
    text = t.bytes()
    return text if final_eol else text[:-len(eol)]


def fq_counts(n_rec, eol, fixed, seed=4):
    """n_rec records: reads of lengths drawn from 0 .. 70 (the offsets path) or all of `fixed` bases (the fixed path)"""
    rnd = random.Random(seed * 100_003 + n_rec)
    out = []
    for i in range(n_rec):
        L = fixed if fixed else rnd.randrange(0, 71)
        out.append(fq_record(b"r%d" % i, _bases(rnd, L), eol, _qual(rnd, L), b"+r%d" % i if i % 5 == 0 else b"+"))
    return b"".join(out)


def fq_every_length(eol, seed=5):
    """every read length 0 .. 200 at every sequence start modulo 4 (the gather copies unaligned dwords)"""
    rnd = random.Random(seed)
    t = _Text(rnd, eol)
    for L in range(201):
        for phase in range(4):
            rid = b"L%d" % L
            while (t.n + 1 + len(rid) + len(eol)) % 4 != phase:
                rid += b"."
            seq = _bases(rnd, L)
            t.add(fq_record(rid, seq, eol, _qual(rnd, L)))
    return t.bytes()


def length_phases(text):
    status, s, e, _, _ = fastq_lines(text)
    assert status == 0
    return set(zip((e[:, 1] - s[:, 1]).tolist(), (s[:, 1] % 4).tolist()))


def fq_fixed_length(L, eol, n_rec=300, seed=6):
    """n_rec reads of L bases, ids of varying length; below four bases the reads are cuts of ACGACG..., so that the 3-mer flags
    depend on every byte"""
    rnd = random.Random(seed + L)
    out = []
    for i in range(n_rec):
        if L < 4:
            k = rnd.randrange(3)
            seq = (b"ACGACG")[k:k + L]
        else:
            seq = _bases(rnd, L)
        out.append(fq_record(b"i" * (1 + i % 5), seq, eol, _qual(rnd, L)))
    return b"".join(out)


def fq_all_empty(eol, n_rec=5000):
    return b"".join(fq_record(b"e%d" % (i % 10), b"", eol) for i in range(n_rec))


REFUSALS = ("short_quality", "no_plus", "no_at", "at_alone")
REFUSAL_PLACES = ("255", "256", "last", "block_edge")


def fq_refusal(kind, place, eol, seed=7):
    """300 good records (the record that lies across the first block edge among them), one of them spoilt"""
    rnd = random.Random(seed)
    recs = [(b"r%d" % i, _bases(rnd, rnd.randrange(40, 90))) for i in range(300)]
    texts = [fq_record(rid, seq, eol) for rid, seq in recs]
    ends = list(itertools.accumulate(len(t) for t in texts))
    k = {"255": 255, "256": 256, "last": 299}.get(place)
    if k is None:
        k = next(i for i, z in enumerate(ends) if z > BLOCK)
        assert ends[k] - len(texts[k]) < BLOCK < ends[k]
    rid, seq = recs[k]
    if kind == "none":  # (the good text the others are measured against)
        pass
    elif kind == "short_quality":
        texts[k] = fq_record(rid, seq, eol, b"I" * (len(seq) - 1))
    elif kind == "no_plus":
        texts[k] = fq_record(rid, seq, eol, plus=b"-")
    elif kind == "no_at":
        texts[k] = b"r" + texts[k][1:]
    else:  # the header line is '@' and nothing else (in a CRLF text too: "@\r\n" is a header with an empty id, which is taken)
        texts[k] = b"@\n" + fq_record(b"", seq, eol)[1 + len(eol):]
    return b"".join(texts)


def fq_three_records(eol):
    return fq_record(b"one", b"ACGTAC", eol) + fq_record(b"two", b"", eol) + fq_record(b"three 3", b"TTACGTA", eol, b"@+IIII>")


def big_small_reads(seed=8):
    """BIG_RECORDS records of the reads AC, G, ACG, CGA with ids of one or two bytes, in numpy alone: (text as a uint8 array,
    rec_start with the end entry, which read each record holds).  Reads of ACG lie either side of record 4 194 304 and at the end."""
    rng = np.random.default_rng(seed)
    n = BIG_RECORDS
    which = rng.integers(0, 4, n)
    which[[4_194_303, 4_194_304, 4_194_305, n - 1]] = 2
    L = np.array([len(r) for r in SMALL_READS], dtype=np.int64)[which]
    idlen = rng.integers(1, 3, n)
    rec_len = 1 + idlen + 1 + L + 1 + 2 + L + 1
    start = np.concatenate(([0], np.cumsum(rec_len)))
    text = np.full(int(start[-1]), ord("I"), dtype=np.uint8)
    a = start[:-1]
    text[a] = ord("@")
    text[a + 1] = ord("a")
    two = idlen == 2
    text[a[two] + 2] = ord("b")
    s0 = a + 1 + idlen + 1
    text[s0 - 1] = 10
    chars = np.zeros((4, 3), dtype=np.uint8)
    for k, r in enumerate(SMALL_READS):
        chars[k, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    for j in range(3):
        has = L > j
        text[s0[has] + j] = chars[which[has], j]
    text[s0 + L] = 10
    text[s0 + L + 1] = ord("+")
    text[s0 + L + 2] = 10
    text[start[1:] - 1] = 10
    return text, start.astype(np.uint64), which


# FASTA
def fa_edges(eol, seed=11):
    rnd = random.Random(seed)
    t = _Text(rnd, eol, fasta=True)
    E = len(eol)

    def at(multiple_of, not_multiple_of, back=0):
        """pad up to the next multiple of the one that is none of the other, less `back`"""
        m = (t.n // multiple_of + 1) * multiple_of
        while (not_multiple_of and m % not_multiple_of == 0) or not t.fill_to(m - back):
            m += multiple_of
        return m

    # '>' as the first byte of a thread, a wave, a block
    for mult, no in ((64, 4096), (4096, 16384), (16384, 0)):
        at(mult, no)
        t.add(b">first" + eol + _bases(rnd, 9) + eol)
    # a header line across a block edge, one of 20 000 bytes over a whole block
    at(BLOCK, 0, back=10)
    t.add(b">" + b"c" * 30 + eol + _bases(rnd, 70) + eol + _bases(rnd, 33) + eol)
    at(BLOCK, 0, back=100)
    t.add(b">" + b"w" * 20_000 + eol + _bases(rnd, 50) + eol)
    for mult, no in ((64, 4096), (4096, 16384), (16384, 0)):
        # the header's '\n' as the first byte of a share (CRLF: '\r' the last byte of the one before), then as the last byte of one
        for nl_delta in (0, -1):
            m = at(mult, no, back=40)
            head = b">h" + b"x" * (m + nl_delta - (E - 1) - t.n - 2)
            t.add(head + eol + _bases(rnd, 21) + eol)
        # ... and the same for a sequence line that follows another sequence line
        for nl_delta in (0, -1):
            m = at(mult, no, back=80)
            t.add(b">s" + eol + _bases(rnd, 17) + eol)
            t.add(_bases(rnd, m + nl_delta - (E - 1) - t.n) + eol + _bases(rnd, 5) + eol)
    t.fill_to(t.n + 50)
    return t.bytes()


def fa_content(eol):
    """'>' inside a header and in the middle of a sequence line (it is sequence), a blank line inside a record, records without
    sequence"""
    return eol.join([b">one > two >", b"ACGTAC>GATTA", b"CC", b">empty", b">blank inside", b"ACG", b"", b"TAC>GA", b">no sequence either",
                     b">last", b"AC>GAC>G", b""])


def fa_counts(n_rec, eol, seed=12):
    rnd = random.Random(seed)
    return b"".join(b">s%d" % i + eol + _bases(rnd, rnd.randrange(0, 71)) + eol for i in range(n_rec))


# ---- the registry: name -> case -------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, fmt, text, eol, status=0, required=frozenset(), note=None):
        self.name, self.fmt, self.text, self.eol, self.status, self.required, self.note = name, fmt, text, eol, status, set(required), note

    @property
    def claims(self):
        return fastq_claims(self.text) if self.fmt == "fastq" else fasta_claims(self.text)


LENGTHS = (2048, 2049, 2111, 16383, 16384, 16385, 32768)           # 0, 1 and 63 modulo 64; a block less one, one, one more; two
COUNTS = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8193)
FIXED_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 67, 128, 129)
FA_LENGTHS = (4096, 32768, 4097)                                   # a multiple of 64, of 16384, 1 modulo 64


def _builders():
    b = {}
    for en, eol in EOLS.items():
        for edge in EDGES:
            b[f"fq-edges-{edge}-{en}"] = lambda edge=edge, eol=eol: Case("", "fastq", fq_edges(edge, eol), eol, required=fastq_required(edge, eol))
        b[f"fq-dense-sparse-{en}"] = lambda eol=eol: Case("", "fastq", fq_dense_sparse(eol), eol)
        for n in LENGTHS:
            for fe in (True, False):
                b[f"fq-length-{n}-{'eol' if fe else 'noeol'}-{en}"] = lambda n=n, fe=fe, eol=eol: Case("", "fastq", fq_of_length(n, eol, fe), eol, note=(n, fe))
        b[f"fq-every-length-{en}"] = lambda eol=eol: Case("", "fastq", fq_every_length(eol), eol)
        b[f"fq-all-empty-{en}"] = lambda eol=eol: Case("", "fastq", fq_all_empty(eol), eol)
        for kind in REFUSALS:
            for place in REFUSAL_PLACES:
                b[f"fq-refuse-{kind}-{place}-{en}"] = lambda kind=kind, place=place, eol=eol: Case("", "fastq", fq_refusal(kind, place, eol), eol, status=1)
        b[f"fa-edges-{en}"] = lambda eol=eol: Case("", "fasta", fa_edges(eol), eol, required=fasta_required(eol))
        b[f"fa-content-{en}"] = lambda eol=eol: Case("", "fasta", fa_content(eol), eol)
        for n in FA_LENGTHS:
            for fe in (True, False):
                b[f"fa-length-{n}-{'eol' if fe else 'noeol'}-{en}"] = lambda n=n, fe=fe, eol=eol: Case("", "fasta", fq_of_length(n, eol, fe, fasta=True), eol, note=(n, fe))
        b[f"fa-counts-8193-{en}"] = lambda eol=eol: Case("", "fasta", fa_counts(8193, eol), eol)
    for n in COUNTS:  # (line ends are not what these are about: LF, and CRLF where a lane or a tile stands alone)
        for en in ("lf", "crlf") if n in (256, 4096, 4097) else ("lf",):
            b[f"fq-count-{n}-var-{en}"] = lambda n=n, eol=EOLS[en]: Case("", "fastq", fq_counts(n, eol, 0), eol, note=n)
            b[f"fq-count-{n}-fixed-{en}"] = lambda n=n, eol=EOLS[en]: Case("", "fastq", fq_counts(n, eol, 37), eol, note=n)
    for L in FIXED_LENGTHS:
        for en in ("lf", "crlf"):
            b[f"fq-fixed-{L}-{en}"] = lambda L=L, eol=EOLS[en]: Case("", "fastq", fq_fixed_length(L, eol), eol, note=L)
    for name, text in (("gt", b">"), ("gt-a", b">a"), ("gt-a-nl", b">a\n"), ("gt-a-crnl", b">a\r\n")):
        b[f"fa-tiny-{name}"] = lambda text=text: Case("", "fasta", text, LF)
    return b


_BUILDERS = _builders()
_CACHE = {}


def all_case_names(prefix=""):
    return [n for n in _BUILDERS if n.startswith(prefix)]


def case(name):
    if name not in _CACHE:
        c = _BUILDERS[name]()
        c.name = name
        _CACHE[name] = c
    return _CACHE[name]


def reference(c):
    """what the reference parser makes of a case (computed once per case)"""
    if not hasattr(c, "_ref"):
        c._ref = parse_fastq(c.text) if c.fmt == "fastq" else parse_fasta(c.text)
    return c._ref


# ---- observability: sequences from log rows, flags from numpy --------------------------------------------------------------------
def kmers4():
    return [bytes(p) for p in itertools.product(b"ACGT", repeat=4)]


def rebuild_sequences(rec, pat, pos, patterns, n_rec):
    """the log rows of a matcher over all 4-mers spell every sequence of four or more bases: -> one bytes per record (b"" where no
    row names the record).  Raises AssertionError if the rows of a record do not cover positions 0 .. max exactly once each."""
    rec, pat, pos = np.asarray(rec, dtype=np.int64), np.asarray(pat, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    assert len(rec) == 0 or (rec.min() >= 0 and rec.max() < n_rec)
    order = np.lexsort((pos, rec))
    rec, pat, pos = rec[order], pat[order], pos[order]
    count = np.bincount(rec, minlength=n_rec)
    first = np.concatenate(([0], np.cumsum(count)))
    assert np.array_equal(pos, np.arange(len(pos)) - first[rec]), "positions 0 .. L - 4 of a record, each once"
    table = np.array([list(p) for p in patterns], dtype=np.uint8)
    out = []
    for r in range(n_rec):
        a, z = int(first[r]), int(first[r + 1])
        if a == z:
            out.append(b"")
            continue
        grams = table[pat[a:z]]
        assert np.array_equal(grams[1:, :3], grams[:-1, 1:]), f"neighbouring 4-mers of record {r} disagree"
        out.append(grams[:, 0].tobytes() + grams[-1, 1:].tobytes())
    return out


def naive_rows(seqs, patterns):
    """(rec, pat, pos) of every occurrence, by Python's own search"""
    index = {p: k for k, p in enumerate(patterns)}
    rows = [(r, index[s[k:k + 4]], k) for r, s in enumerate(seqs) for k in range(len(s) - 3) if s[k:k + 4] in index]
    a = np.array(rows, dtype=np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def spelled(seqs):
    """what the 4-mer rows can say of these sequences: those of four bases and more"""
    return [s if len(s) >= 4 else b"" for s in seqs]


def flags_k3(seqs):
    return np.array([K3 in s for s in seqs], dtype=bool)


# ---- the two entry points, numpy arrays out --------------------------------------------------------------------------------------
def _rows_buffer(mk, n):
    return np.zeros(max(1, n), dtype=mk.ROW_DTYPE)


def rows_list(rows):
    return list(zip(rows["file"].tolist(), rows["rec"].tolist(), rows["pat"].tolist(), rows["pos"].tolist()))


def run_fastq_text(mk, m, text, logging=True, invert=False):
    """mk_extract_fastq_text -> dict(status, n_rec, rec_start, keep, rows, counters); text: bytes or a uint8 array"""
    L = mk.load()
    buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
    cap = int(np.count_nonzero(buf == 10)) // 4 + 2
    rec_start = np.zeros(cap + 1, dtype=np.uint64)
    keep = np.zeros(cap, dtype=np.uint8)
    rows = _rows_buffer(mk, 1 << 16)
    n_rec, n_rows, status = C.c_uint64(), C.c_uint64(), C.c_uint32()
    while True:
        cnt, counts = mk.Counters(), np.zeros(len(m.patterns), dtype=np.uint32)
        rc = L.mk_extract_fastq_text(m.handle, buf.ctypes.data if len(buf) else None, len(buf), int(logging), int(invert), cap, C.byref(n_rec),
                                     rec_start.ctypes.data, keep.ctypes.data, rows.ctypes.data, len(rows), C.byref(n_rows), C.byref(cnt),
                                     counts.ctypes.data, C.byref(status))
        if rc == mk.MK_E_CAPACITY and n_rows.value > len(rows):
            rows = _rows_buffer(mk, n_rows.value)
            continue
        mk._check(rc)
        break
    n = n_rec.value
    return {"status": status.value, "n_rec": n, "rec_start": rec_start[:n + 1].copy(), "keep": keep[:n].astype(bool),
            "rows": rows[:n_rows.value if logging else 0], "counters": cnt.as_dict(counts)}


def run_window(mk, m, text, fmt="fastq", logging=True, invert=False, head=b"", ends_at_record=True, want=()):
    """mk_extract_window on one source of plain text -> dict(status, n_rec, rec_start, keep, rows, counters, n_used, tail, kept);
    want: any of "tail", "kept" """
    L = mk.load()
    buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
    hb = np.frombuffer(head, dtype=np.uint8)
    total = len(buf) + len(hb)
    cap = int(np.count_nonzero(buf == 10)) + int(np.count_nonzero(hb == 10)) + 2
    arr = (mk.WindowSource * 1)()
    S = arr[0]
    S.head, S.n_head = (hb.ctypes.data if len(hb) else None), len(hb)
    S.text, S.n_text = (buf.ctypes.data if len(buf) else None), len(buf)
    S.ends_at_record = int(bool(ends_at_record))
    rec_start = np.zeros(cap + 1, dtype=np.uint64)
    S.rec_start = rec_start.ctypes.data
    tail = np.zeros(max(1, total if "tail" in want else 0), dtype=np.uint8)
    kept = np.zeros(max(1, total if "kept" in want else 0), dtype=np.uint8)
    if "tail" in want:
        S.tail, S.tail_cap = tail.ctypes.data, tail.size
    if "kept" in want:
        S.kept, S.kept_cap = kept.ctypes.data, kept.size
    keep = np.zeros(cap, dtype=np.uint8)
    rows = _rows_buffer(mk, 1 << 16)
    n_rec, n_rows, status = C.c_uint64(), C.c_uint64(), C.c_uint32()
    while True:
        cnt, counts = mk.Counters(), np.zeros(len(m.patterns), dtype=np.uint32)
        rc = L.mk_extract_window(m.handle, None, 1 if fmt == "fasta" else 0, 1, arr, int(logging), int(invert), cap, C.byref(n_rec), keep.ctypes.data,
                                 rows.ctypes.data, len(rows), C.byref(n_rows), C.byref(cnt), counts.ctypes.data, C.byref(status))
        if rc == mk.MK_E_CAPACITY and n_rows.value > len(rows):
            rows = _rows_buffer(mk, n_rows.value)
            continue
        mk._check(rc)
        break
    n = n_rec.value
    return {"status": status.value, "n_rec": n, "rec_start": rec_start[:n + 1].copy() if not status.value else rec_start[:0], "keep": keep[:n].astype(bool),
            "rows": rows[:n_rows.value if logging else 0], "counters": cnt.as_dict(counts), "n_used": int(S.n_used),
            "tail": tail[:S.n_tail].tobytes() if "tail" in want else None, "kept": kept[:S.n_kept_bytes] if "kept" in want else None}
