"""Every instantiation of the scan kernel (scan_variants.hip): the options that make launch_scan (scan_kernel.hip) choose it,
the two names it must report, and one small batch per variant whose answer the naive enumerator (naive.py) gives.

VARIANTS has a row per (S, QC, GF, plain, MC): sampling stride, q-gram mode (> 0 compiled in, 0 run-time q <= 16, -1 run-time q
in 17 .. 32), filter in global memory, plain stream loads, short-class mode (0 one class, 1 two classes with the short class's
stride and table kind at run time, 2 / 4 / 8 a byte-table short class with that stride compiled in).  The recipes follow
choose_geometry / plan_classes of matcher.cpp: a forced stride S gives the main class q = min(32, lmin - S + 1), so a row
fixes lmin, the shortest pattern of its main class:
  * q compiled in: lmin = q + S - 1;
  * run-time wide q: the smallest lmin there is, q = 17 and lmin = 16 + S (17 is a compiled-in q at no stride);
  * run-time narrow q: any lmin >= S would do (q = 1).  The rows take q = 8, or what 12 bases leave at the small strides:
    lmin = max(12, S + 7).  Below 12 bases two dozen random patterns turn up by accident in every few KB of random text
    and the filler could not be kept free of them; below q = 8 the few hundred q-grams of the set are most of the 4^q
    keys, every sample is a candidate and a near-miss no longer tells the filter from the verification.
This module knows nothing of merkurio_amd; tests/test_scan_variant_matrix_cpu.py holds the table against the sources and every
batch against the oracle before a kernel sees it.
"""
import functools
import random
from collections import namedtuple

import naive

CHUNK = 1024
TILE = 31 * CHUNK                     # tile_geometry.hpp: a short tile, the only kind a batch this small is cut into
STRIDES = (1, 2, 4, 8, 16)
LDS_FIXED = ((16, 16), (8, 24), (4, 28), (4, 18))  # (S, q) with q compiled in, filter in LDS
GF_FIXED = ((8, 14), (4, 18), (8, 24))             # ... filter in global memory
SHORT_BYTE_MAX_Q = 6                  # filter.hpp: kShortByteMaxQ, up to here the short class's table holds a byte per key
N_OFFSETS = 64                        # every pattern at every start offset 0 .. 63 of a record
TAIL_BYTES = CHUNK + 700              # the text behind the last tile: one whole chunk and a partial one
TEXT_MAX = 1 << 20

Variant = namedtuple("Variant", "S QC GF plain MC id lmin q options short_lengths stride2 q2 ci names")
Batch = namedtuple("Batch", "patterns records ci split planted near_miss cross borders long_rec tail_rec")
Expected = namedtuple("Expected", "flags tuples counts hits records_hit records bases")

# the rows whose matcher is case-insensitive: one per family
_CI = {(16, 16, False, False, 0), (8, -1, False, False, 0), (1, 0, False, True, 0), (4, 0, True, False, 0), (8, 24, False, False, 4),
       (2, 0, True, False, 1)}


def _row_id(S, QC, GF, plain, MC):
    q = f"q{QC}" if QC > 0 else ("narrow" if QC == 0 else "wide")
    end = "-plain" if plain else ("" if MC == 0 else ("-2class" if MC == 1 else f"-s2={MC}"))
    return f"S{S}-{q}-{'gf' if GF else 'lds'}{end}"


def _names(S, QC, GF, plain, MC):
    """(EMIT false, EMIT true), spelled as the MK_VARIANT* macros of scan_kernel.hip spell them"""
    end = ",plain>" if plain else (">" if MC == 0 else (",2-class>" if MC == 1 else f",s2={MC},2-class>"))
    return tuple(f"mk_scan_kernel<{S},{QC},{emit},{'true' if GF else 'false'}{end}" for emit in ("false", "true"))


def _short_class(S, QC, GF, MC):
    """(stride2, q2) of the short class: MC = 2 / 4 / 8 is a byte table (q2 <= 6) at that stride; MC = 1 is anything else -- next to
    a compiled-in main q a bit table, or a byte table at stride 1, next to a run-time q either kind at any stride"""
    if MC > 1:
        return MC, SHORT_BYTE_MAX_Q
    if QC > 0 and not GF:
        return (2, 8) if S >= 8 else (1, SHORT_BYTE_MAX_Q)
    return (2, 8) if QC == -1 else (4, SHORT_BYTE_MAX_Q)


def _variant(S, QC, GF, plain, MC):
    q = QC if QC > 0 else (17 if QC == -1 else max(12, S + 7) - S + 1)
    lmin = q + S - 1
    options = dict(force_stride=S)
    if GF:
        options["force_global_filter"] = 1
    short_lengths, s2, q2 = (), 0, 0
    if MC:
        s2, q2 = _short_class(S, QC, GF, MC)
        a = max(9, s2 + q2 - 1)  # the shortest pattern admits stride s2 with q-grams of q2 bases
        short_lengths = (a, a + 2)
        assert a + 2 < lmin
        options.update(length_classes=2, force_split_len=lmin, force_stride2=s2, force_q2=q2)
    key = (S, QC, GF, plain, MC)
    return Variant(S, QC, GF, plain, MC, _row_id(*key), lmin, q, options, short_lengths, s2, q2, key in _CI, _names(*key))


def _rows():
    out = []
    for gf, fixed in ((False, LDS_FIXED), (True, GF_FIXED)):          # one class
        out += [(S, q, gf, False, 0) for S, q in fixed]
        out += [(S, qc, gf, False, 0) for qc in (0, -1) for S in STRIDES]
    out += [(S, q, False, True, 0) for S, q in LDS_FIXED]            # plain loads: one class, filter in LDS
    out += [(S, qc, False, True, 0) for qc in (0, -1) for S in STRIDES]
    out += [(S, q, False, False, mc) for mc in (1, 2, 4, 8) for S, q in LDS_FIXED]  # two classes; no main class at stride 1
    out += [(S, qc, False, False, 1) for qc in (0, -1) for S in STRIDES[1:]]
    out += [(S, qc, True, False, 1) for qc in (0, -1) for S in STRIDES[1:]]   # ... next to a global filter: run-time q only
    return out


VARIANTS = [_variant(*r) for r in _rows()]
BY_ID = {v.id: v for v in VARIANTS}
assert len(VARIANTS) == 73 == len(BY_ID)


def main_lengths(v):
    return sorted({v.lmin, v.lmin + 1, v.lmin + v.S - 1, v.lmin + v.S, 2 * v.lmin})


# ---------------------------------------------------------------------------------------------------- patterns
class _Again(Exception):
    """this seed's random choices collide with the claims of the batch: the next seed"""


def _rand(rnd, n):
    return bytes(rnd.choices(b"ACGT", k=n))


def _patterns(v, rnd):
    """-> (patterns, roles).  roles: indices by what the batch uses them for"""
    lens = main_lengths(v)
    plain = {L: [_rand(rnd, L) for _ in range(4)] for L in lens}
    # two different patterns that overlap: the second begins with the first one's last five bases
    first = plain[lens[-2]][2]
    second = first[-5:] + _rand(rnd, lens[1] - 5)
    plain[lens[1]][1] = second
    # the suffix-nested triple: three tuples that end on one byte
    top = _rand(rnd, 2 * v.lmin)
    triple = [top, top[-(v.lmin + 1):], top[-v.lmin:]]
    runs = [b"A" * v.lmin, b"C" * (v.lmin + 1)]  # the patterns that overlap themselves at every shift
    shorts = {L: [_rand(rnd, L) for _ in range(2)] for L in v.short_lengths}
    host = plain[lens[-1]][3]  # the long pattern a short one is cut out of
    cut = [host[3:3 + v.short_lengths[0]]] if v.MC else []
    named = [("plain", p) for L in lens for p in plain[L]] + [("triple", p) for p in triple] + [("run", p) for p in runs]
    named += [("short", p) for L in v.short_lengths for p in shorts[L]] + [("cut", p) for p in cut]
    rnd.shuffle(named)  # (pattern ids of the two classes and of the lengths interleave)
    pats = [p for _, p in named]
    if len(set(pats)) != len(pats):
        raise _Again
    allowed = {(a, b) for a in triple for b in triple} | {(host, c) for c in cut}
    for a in pats:
        for b in pats:
            if a != b and b in a and (a, b) not in allowed:
                raise _Again
    if top.count(triple[1]) != 1 or top.count(triple[2]) != 1 or (cut and (cut[0] in top or host.count(cut[0]) != 1)):
        raise _Again
    idx = {p: i for i, p in enumerate(pats)}
    roles = {
        "triple": [idx[p] for p in triple], "runs": [idx[p] for p in runs], "overlap": (idx[first], idx[second]),
        "host": idx[host], "cut": [idx[p] for p in cut],
        # one pattern of each length, of either class, for the near-misses and the record ends
        "probe": [idx[plain[L][0]] for L in lens] + [idx[shorts[L][0]] for L in v.short_lengths],
        "tail": idx[plain[lens[0]][2]], "last": idx[plain[lens[2 if len(lens) > 2 else 0]][2]],
    }
    return pats, roles


# ---------------------------------------------------------------------------------------------------- records
class _Builder:
    def __init__(self, v, seed):
        self.v, self.rnd = v, random.Random(seed)
        self.patterns, self.roles = _patterns(v, self.rnd)
        self.folded = [p.lower() for p in self.patterns] if v.ci else self.patterns
        self.records, self.n_bytes = [], 0

    def occ(self, text):
        """[(pattern, start)] of every occurrence in text, sorted"""
        t = text.lower() if self.v.ci else text
        out = []
        for i, p in enumerate(self.folded):
            k = t.find(p)
            while k != -1:
                out.append((i, k))
                k = t.find(p, k + 1)
        return sorted(out)

    def implied(self, core, at=0):
        return sorted((i, at + k) for i, k in self.occ(core))

    def clean(self, n):
        """n random bases that hold no pattern (the bases in the middle of an accidental occurrence are redrawn)"""
        t = bytearray(self.rnd.choices(b"ACGT", k=n))
        dirty = True
        while dirty:
            dirty = False
            for p in self.patterns:
                k = t.find(p)
                while k != -1:
                    at = k + len(p) // 2
                    t[at] = self.rnd.choice([c for c in b"ACGT" if c != t[at]])
                    dirty = True
                    k = t.find(p, k + 1)
        return bytes(t)

    def around(self, pre, core, post, want=None):
        """filler + core + filler in which exactly the occurrences inside core occur (want: another claim, () = none at all)"""
        want = self.implied(core, pre) if want is None else sorted(want)
        for _ in range(60):
            rec = self.clean(pre) + core + self.clean(post)
            if self.occ(rec) == want:
                return rec
        raise _Again

    def add(self, rec):
        self.records.append(bytes(rec))
        self.n_bytes += len(rec)
        return len(self.records) - 1


def _near_misses(b, p):
    """p with base i replaced by the next base of ACGT, and by N, for every i"""
    out = []
    for i in range(len(p)):
        nxt = b"CGTA"[b"ACGT".index(p[i])]
        out.append(p[:i] + bytes([nxt]) + p[i + 1:])
        out.append(p[:i] + b"N" + p[i + 1:])
    return out


def _build(v, seed):
    b = _Builder(v, seed)
    P, roles, rnd = b.patterns, b.roles, b.rnd
    near_miss, cross = [], []
    misc = []  # built first, placed behind the first record, whose length brings the all-offsets records to a multiple of 64
    for pi in roles["probe"]:
        p = P[pi]
        # record ends: the record is the pattern, lacks a base at either end, has one more at either end; ends on the pattern
        misc += [("hit", p), ("none", b.around(0, p[:-1], 0, ())), ("none", b.around(0, p[1:], 0, ())), ("hit", b.around(0, p, 1)), ("hit", b.around(1, p, 0)),
                 ("hit", b.around(7 + len(p) % 5, p, 0)), ("none", b"")]
        # two records whose concatenation spells the pattern across the boundary
        h = len(p) // 2
        misc += [("cross", b.around(9, p[:h], 0, ()), b.around(0, p[h:], 11, ()), pi)]
        # near-misses: the filter passes on the q-grams that miss base i, the verification must refuse
        misc += [("none", b.around(5 + i % 7, nm, 6, ())) for i, nm in enumerate(_near_misses(b, p))]
        # lower case: an occurrence for a case-insensitive matcher alone; one lower-case base; a lower-case near-miss
        misc += [("any", b.clean(6) + p.lower() + b.clean(3)), ("any", b.clean(3) + p[:2] + p[2:3].lower() + p[3:] + b.clean(6)),
                 ("none", b.around(4, _near_misses(b, p)[len(p)].lower(), 5, ()))]
    # overlaps: a run pattern shifted by 1 .. S against itself, two different patterns over five shared bases, the triple
    for ri in roles["runs"]:
        run = P[ri][:1] * (len(P[ri]) + v.S)
        misc.append(("hit", b.around(5, run, 7, [(ri, 5 + k) for k in range(v.S + 1)])))
    first, second = (P[i] for i in roles["overlap"])
    misc.append(("hit", b.around(4, first + second[5:], 4)))
    misc.append(("hit", b.around(3, P[roles["triple"][0]], 2)))
    if roles["cut"]:
        misc.append(("hit", b.around(2, P[roles["host"]], 9)))
    n_misc = sum(len(m[1]) + (len(m[2]) if m[0] == "cross" else 0) for m in misc)
    near_miss.append(b.add(b.clean(64 + (-n_misc) % 64)))
    for m in misc:
        r = b.add(m[1])
        if m[0] == "cross":
            b.add(m[2])
            cross.append((r, r + 1, m[3]))
            near_miss += [r, r + 1]
        elif m[0] == "none":
            near_miss.append(r)
    assert b.n_bytes % 64 == 0
    # every pattern at every start offset 0 .. 63 of a record; every record a multiple of 64 bytes long, so the offsets in the
    # record are the residues modulo 64 in the batch
    planted = []
    for pi, p in enumerate(P):
        for o in range(N_OFFSETS):
            planted.append((b.add(b.around(o, p, -(o + len(p)) % 64)), pi, o))
    assert b.n_bytes % 64 == 0
    # the long record: 256 bytes before a tile border, two whole tiles, the text's tail.  A run pattern of L bases ends on every
    # byte from border - (L - 1) to border + 1 where 2 L of its base stand in [border - 2 L + 2, border + 2)
    pad = (-(b.n_bytes + 256)) % TILE
    if pad:
        near_miss.append(b.add(b.clean(pad)))
    start = b.n_bytes
    b0 = start + 256
    assert b0 % TILE == 0
    long_len = 256 + 2 * TILE + TAIL_BYTES
    text = bytearray(b.clean(long_len))
    want, borders = [], []
    for k, ri in enumerate((roles["runs"][0], roles["runs"][1], roles["runs"][0])):
        border, L = b0 + k * TILE, len(P[ri])
        a = border - 2 * L + 2 - start
        text[a:a + 2 * L] = P[ri][:1] * (2 * L)
        for g in (a - 1, a + 2 * L):  # the bases next to the run are not the run's
            if text[g] == P[ri][0]:
                text[g] = ord("G")
        want += [(ri, a + j) for j in range(L + 1)]
        borders.append((border, ri))
    tp, lp = P[roles["tail"]], P[roles["last"]]
    at = long_len - 350  # inside the partial chunk that ends the text
    text[at:at + len(tp)] = tp
    text[long_len - len(lp):] = lp  # the text's last byte is an occurrence's last
    want += b.implied(tp, at) + b.implied(lp, long_len - len(lp))
    if b.occ(bytes(text)) != sorted(want):
        raise _Again
    long_rec = b.add(text)
    assert b.n_bytes == b0 + 2 * TILE + TAIL_BYTES and b.n_bytes <= TEXT_MAX
    return Batch(P, b.records, v.ci, v.lmin if v.MC else 0, planted, near_miss, cross, borders, long_rec, (roles["tail"], roles["last"]))


@functools.lru_cache(maxsize=None)
def _batch(vid):
    v = BY_ID[vid]
    base = 7919 * VARIANTS.index(v)
    for attempt in range(16):
        try:
            return _build(v, base + attempt)
        except _Again:
            continue
    raise AssertionError(f"{vid}: no seed gives a batch that holds its claims")


def batch(row):
    """-> (patterns, records) of a row of VARIANTS (or its id)"""
    bt = details(row)
    return bt.patterns, bt.records


def details(row):
    """the Batch of a row: patterns, records and which record was built for what"""
    return _batch(row if isinstance(row, str) else row.id)


@functools.lru_cache(maxsize=None)
def _expected(vid):
    bt = _batch(vid)
    tuples, flags = [], []
    counts = [0] * len(bt.patterns)
    for r, rec in enumerate(bt.records):
        hits = naive.ac_order(bt.patterns, rec, bt.ci)
        flags.append(bool(hits))
        for p, pos in hits:
            tuples.append((r, p, pos))
            counts[p] += 1
    return Expected(flags, tuples, counts, len(tuples), sum(flags), len(bt.records), sum(len(r) for r in bt.records))


def expected(row):
    """flags, tuples in Aho-Corasick emission order, per-pattern counts and the summary counters: the naive enumerator's"""
    return _expected(row if isinstance(row, str) else row.id)


def record_starts(records):
    out = [0]
    for r in records:
        out.append(out[-1] + len(r))
    return out
