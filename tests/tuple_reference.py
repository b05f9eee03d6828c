"""A plain numpy reference of everything the record loops derive from the matcher's hits, for pattern sets of ONE length
k <= 32 over ACGT (case-sensitive).  TEST INFRASTRUCTURE ONLY; it uses neither the device nor the oracle library, and
test_tuple_reference_cpu.py pins it to the oracle before test_gpu_sets.py lets it judge the kernels of sets.hip.

The rules, restated from the reference (the lines are the ones sets.hip and DeviceLoop::join_mates cite):
  occurrences   every possibly-overlapping occurrence of every pattern inside a record, never across two records
  AC order      record, end, pattern id (src/cmd_extract.rs:332-351); with one length: record, position, pattern
  BNDMq order   record, pattern, position (src/cmd_extract.rs:365-384) -- the "set order" of sets.hip
  sets          the distinct patterns of a record, ascending (src/cmd_tag.rs:392-442,484-485), as a CSR
  counts        AC: += 1 per hit (src/cmd_extract.rs:353); BNDMq: += 1 per (record, pattern) with a hit (:380-383)
  pairs, AC     per pair all of mate 1, then all of mate 2, each in AC order (src/cmd_extract.rs:479-537); += 1 per hit
  pairs, BNDMq  per pair and pattern mate 1's positions, then mate 2's (:542-587); += 1 per (pair, pattern, mate) with a hit
  counters      records and bases of the batch, hits and records with a hit per file (:326-387, :471-475)
  keep          extract: hit != invert (:400-405, :600-606); tag: -m keeps records with a hit, -v without, else all
                (src/cmd_tag.rs:457-467)
Everything is arrays; there is no Python loop over tuples (only over the k bases of a pattern and over chunks of the text).
"""
import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i

CHUNK = 1 << 23  # text positions per pass: bounds the uint64 temporaries to a few hundred MB


def pattern_codes(patterns):
    """2-bit codes (uint64) of equal-length ACGT patterns, in list order"""
    k = len(patterns[0])
    assert 1 <= k <= 32 and all(len(p) == k for p in patterns), "one pattern length of at most 32"
    arr = np.frombuffer(b"".join(patterns), dtype=np.uint8).reshape(len(patterns), k)
    c = _CODE[arr]
    assert (c < 4).all(), "patterns over ACGT only"
    codes = np.zeros(len(patterns), dtype=np.uint64)
    for j in range(k):
        codes = (codes << np.uint64(2)) | c[:, j].astype(np.uint64)
    assert len(np.unique(codes)) == len(codes), "distinct patterns"
    return codes


def _windows(c, k):
    """c: the 2-bit codes of a text in the integer type of the result (2 * k bits must fit) -> the codes of text[i:i + k] for every i
    in [0, len - k]: windows of length 1, 2, 4, ... by doubling, k's binary digits put them together"""
    shift = c.dtype.type
    piece, have = c, 1
    out, out_len = None, 0
    while True:
        if k & have:
            if out is None:
                out, out_len = piece, have
            else:  # out covers [i, i + out_len), piece covers [j, j + have): append the piece at j = i + out_len
                m = min(len(out), len(piece) - out_len)
                out = (out[:m] << shift(2 * have)) | piece[out_len:out_len + m]
                out_len += have
        if 2 * have > k:
            break
        piece = (piece[:len(piece) - have] << shift(2 * have)) | piece[have:]
        have *= 2
    assert out_len == k
    return out[:len(c) - k + 1]


def window_codes(text, k):
    """codes[i] of text[i:i + k] for every i in [0, len - k], valid[i]: the window is ACGT throughout"""
    n = len(text) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    c = _CODE[text]
    bad = np.concatenate(([0], np.cumsum(c > 3, dtype=np.int64)))
    return _windows((c & 3).astype(np.uint64), k), bad[k:] == bad[:-k]


class Tuples:
    """(rec, pat, pos) arrays of one batch plus what the batch itself says (n_rec, bases)"""

    def __init__(self, rec, pat, pos, n_rec, n_bases, n_pat):
        self.rec, self.pat, self.pos = rec.astype(np.uint64), pat.astype(np.uint32), pos.astype(np.uint64)
        self.n_rec, self.n_bases, self.n_pat = int(n_rec), int(n_bases), int(n_pat)
        self._set_order = None

    def __len__(self):
        return len(self.rec)

    def take(self, order):
        return Tuples(self.rec[order], self.pat[order], self.pos[order], self.n_rec, self.n_bases, self.n_pat)

    # ---- emission orders
    def ac_order(self):
        return self.take(np.lexsort((self.pat, self.pos, self.rec)))  # (the last key is the primary one)

    def bndmq_order(self):
        if self._set_order is None:  # (record, pattern) as one key: rec * n_pat + pat fits 64 bits for every batch the ABI takes
            self._set_order = self.take(np.lexsort((self.pos, self.rec * np.uint64(self.n_pat) + self.pat)))
        return self._set_order

    def emission_order(self, ac):
        return self.ac_order() if ac else self.bndmq_order()

    # ---- the distinct patterns of every record
    def pattern_sets(self):
        """-> found_off uint64[n_rec + 1], found_pat uint32[found_off[n_rec]]"""
        s = self.bndmq_order()
        head = np.ones(len(s), dtype=bool)
        head[1:] = (s.rec[1:] != s.rec[:-1]) | (s.pat[1:] != s.pat[:-1])
        per_rec = np.bincount(s.rec[head].astype(np.int64), minlength=self.n_rec)
        found_off = np.zeros(self.n_rec + 1, dtype=np.uint64)
        np.cumsum(per_rec, out=found_off[1:])
        return found_off, s.pat[head]

    # ---- pattern_hit_counts
    def counts(self, ac):
        if ac:
            return np.bincount(self.pat, minlength=self.n_pat).astype(np.uint32)
        return np.bincount(self.pattern_sets()[1], minlength=self.n_pat).astype(np.uint32)

    # ---- flags, counters, keep
    def flags(self):
        return np.bincount(self.rec.astype(np.int64), minlength=self.n_rec) > 0

    def counters(self, keep=None):
        """what a call with logging on adds to the counters; keep: its keep flags (one record each)"""
        return {"records": self.n_rec, "bases": self.n_bases, "hits": (len(self), 0), "records_hit": (int(self.flags().sum()), 0),
                "extracted": 0 if keep is None else int(np.count_nonzero(keep))}

    def extract_keep(self, invert=False):
        return (self.flags() != bool(invert)).astype(np.uint8)

    def tag_keep(self, filter_matching=False, invert=False):
        has = self.flags()
        return (has if filter_matching else (~has if invert else np.ones(self.n_rec, dtype=bool))).astype(np.uint8)


def occurrences(data, off, patterns):
    """data: uint8[], off: uint64[n_rec + 1] (ascending), patterns: list of distinct ACGT strings of one length k <= 32
    -> Tuples in text order (record, position ascending)"""
    data = np.asarray(data, dtype=np.uint8)
    off = np.asarray(off).astype(np.int64)
    n_rec = len(off) - 1
    k = len(patterns[0])
    codes = pattern_codes(patterns)
    by_code = np.argsort(codes)
    sorted_codes = codes[by_code]
    lo, hi = int(off[0]), int(off[-1])
    # a table over the codes of the first q bases says where a pattern can start; the full code is compared only there
    q = min(k, 12)
    table = np.zeros(1 << (2 * q), dtype=bool)
    table[(codes >> np.uint64(2 * (k - q))).astype(np.int64)] = True
    g_all, p_all = [], []
    for a in range(lo, max(lo, hi - k + 1), CHUNK):
        b = min(hi, a + CHUNK + k - 1)  # windows that START in [a, a + CHUNK)
        c = _CODE[data[a:b]]
        at = np.flatnonzero(table[_windows((c & 3).astype(np.uint32), q)[:b - a - k + 1]])
        cols = c[at[:, None] + np.arange(k)]
        w = np.zeros(len(at), dtype=np.uint64)
        for j in range(k):
            w = (w << np.uint64(2)) | cols[:, j].astype(np.uint64)
        j = np.searchsorted(sorted_codes, w)
        j[j == len(sorted_codes)] = 0
        hit = (sorted_codes[j] == w) & (cols < 4).all(axis=1)  # (a letter outside ACGT matches no pattern)
        g_all.append(at[hit] + a)
        p_all.append(by_code[j[hit]])
    g = np.concatenate(g_all) if g_all else np.zeros(0, dtype=np.int64)
    pat = np.concatenate(p_all) if p_all else np.zeros(0, dtype=np.int64)
    # the record of a window's first byte: the last one that starts at or before it (empty records in front of it start there too)
    rec = np.searchsorted(off, g, side="right") - 1
    inside = g + k <= off[np.minimum(rec + 1, n_rec)]  # windows that cross a record boundary are no occurrences
    g, pat, rec = g[inside], pat[inside], rec[inside]
    return Tuples(rec, pat, g - off[rec], n_rec, hi - lo, len(patterns))


class Pairs:
    """the tuples of both mates of a paired batch as one list with a `file` field (0: mate 1, 1: mate 2)"""

    def __init__(self, t1, t2):
        assert t1.n_rec == t2.n_rec and t1.n_pat == t2.n_pat
        self.t1, self.t2 = t1, t2
        self.n_rec, self.n_pat = t1.n_rec, t1.n_pat
        self.file = np.concatenate((np.zeros(len(t1), dtype=np.uint32), np.ones(len(t2), dtype=np.uint32)))
        self.rec = np.concatenate((t1.rec, t2.rec))
        self.pat = np.concatenate((t1.pat, t2.pat))
        self.pos = np.concatenate((t1.pos, t2.pos))

    def __len__(self):
        return len(self.rec)

    def rows(self, ac):
        """(file, pair, pat, pos) arrays in pair order"""
        if ac:
            order = np.lexsort((self.pat, self.pos, self.file, self.rec))
        else:
            order = np.lexsort((self.pos, self.file, self.pat, self.rec))
        return self.file[order], self.rec[order], self.pat[order], self.pos[order]

    def counts(self, ac):
        if ac:
            return np.bincount(self.pat, minlength=self.n_pat).astype(np.uint32)
        order = np.lexsort((self.file, self.pat, self.rec))
        f, r, p = self.file[order], self.rec[order], self.pat[order]
        head = np.ones(len(r), dtype=bool)
        head[1:] = (r[1:] != r[:-1]) | (p[1:] != p[:-1]) | (f[1:] != f[:-1])
        return np.bincount(p[head], minlength=self.n_pat).astype(np.uint32)

    def keep(self, invert=False):
        return ((self.t1.flags() | self.t2.flags()) != bool(invert)).astype(np.uint8)

    def counters(self, keep=None):
        return {"records": 2 * self.n_rec, "bases": self.t1.n_bases + self.t2.n_bases, "hits": (len(self.t1), len(self.t2)),
                "records_hit": (int(self.t1.flags().sum()), int(self.t2.flags().sum())),
                "extracted": 0 if keep is None else 2 * int(np.count_nonzero(keep))}
