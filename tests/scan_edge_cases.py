"""Small scan batches in which the number of flagged records, and of tuples, inside chosen byte spans is exact by construction.

The patterns are 4-6-mers over ACG.  A record is filler, in which every third byte of the text is a T, so that no four
consecutive bytes are free of T and no pattern can occur, or filler with ONE pattern planted in it between two guard Ts (or
the record's ends).  No pattern of a set is a substring of another one, except in TUPLE_PATTERNS, whose first three are
suffixes of each other: planting the longest gives three tuples that end on the same byte, the next two, the shortest one.
What a case expects is written down while planting, never searched for; tests/test_scan_edge_cases_cpu.py holds every case
against the naive enumerator and the oracle before a kernel sees it.

The byte spans follow the scan's tile geometry as the kernels have it today (31 KiB tiles, tile i scanned by wave i of the
grid, the last KiB or more of a text dealt out chunk by chunk); the GPU tests assert that from the geometry of their own
launches and fail when it no longer holds.  This module knows nothing of merkurio_amd.
"""
import functools
import random
from collections import namedtuple

CHUNK = 1024
TILE = 31 * CHUNK         # tile_geometry.hpp: a short tile
MARGIN = 64               # hits keep this far from a tile's ends, so the wave that owns the tile is the one that finds them
FLAG_LIST_CAP = 2048      # scan_kernel.h: kFlagListCap
HIT_STAGE = 1024          # scan_kernel.h: kHitStage; a wave flushes when more than kHitStage - 64 tuples are staged
STAGE_EDGE = HIT_STAGE - 64
TEXT_MAX = 2 << 20

PATTERNS = [b"ACGA", b"CCAG", b"GACCA", b"CAGGC", b"AGCCGA", b"GGACAC"]
TUPLE_PATTERNS = [b"GACGCA", b"ACGCA", b"CGCA", b"CCAG"]
LONG_PATTERN = b"ACGGCAAGCCAGGACCGACAGCAAGGCCAGACGGACCAGC"  # 40 bytes, no T: next to the 4-mers it makes a second length class
WIDE_PATTERNS = [b"ACGGCAAGCCAGGACCGA", b"CAGCAAGGCCAGACGGACCA"]  # 18 and 20 bytes: q-grams longer than 16 bases

Span = namedtuple("Span", "start end F placement per_hit", defaults=(1,))
Case = namedtuple("Case", "name rec_len records patterns flags tuples offsets spans")


def _check_patterns(patterns, nested=0):
    for p in patterns:
        assert len(p) >= 4 and set(p) <= set(b"ACG"), p
    for i, p in enumerate(patterns):
        for j, q in enumerate(patterns):
            if i != j and not (i < nested and j < nested):
                assert q not in p, (p, q)
    for i in range(1, nested):
        assert patterns[i - 1].endswith(patterns[i]) and patterns[i - 1].count(patterns[i]) == 1


_check_patterns(PATTERNS)
_check_patterns(TUPLE_PATTERNS, nested=3)
_check_patterns(WIDE_PATTERNS)


def _pick(candidates, starts, F, placement, rnd):
    """F of the candidate records"""
    if F is None or F == len(candidates):
        return list(candidates)
    if F > len(candidates):
        raise ValueError(f"{F} hits asked of {len(candidates)} records")
    if placement == "mixed":
        return sorted(rnd.sample(candidates, F))
    if placement == "isolated":  # at most one hitting record in any 64 bytes, and then some
        out, last = [], None
        for r in candidates:
            if len(out) < F and (last is None or starts[r] - last >= 80):
                out.append(r)
                last = starts[r]
        if len(out) < F:
            raise ValueError(f"no room for {F} isolated hits")
        return out
    assert placement == "clustered"  # runs of 64 to 127 consecutive hitting records, two filler records between runs
    runs, left = [], F
    while left:
        n = left if left < 128 else 64 + rnd.randrange(0, 32)
        runs.append(n)
        left -= n
    gap = 2 if F + 2 * (len(runs) - 1) <= len(candidates) else 0
    out, at = [], 0
    for n in runs:
        out += candidates[at:at + n]
        at += n + gap
    assert len(out) == F
    return out


def make_case(name, rec_len, n_bytes, spans, seed, patterns=PATTERNS, extra=()):
    """rec_len: 8, 12 (any fixed length) or "ragged" (6 to 14 bytes); spans: Span(first byte, end byte, hitting records or None
    for all, placement, occurrences per hitting record).  A span's candidates are the records that lie in it entirely.
    extra: patterns that are part of the set and can occur nowhere (longer than a record)"""
    rnd = random.Random(seed)
    assert n_bytes <= TEXT_MAX
    text = bytearray(rnd.choices(b"ACG", k=n_bytes))
    text[2::3] = b"T" * len(range(2, n_bytes, 3))
    if rec_len == "ragged":
        offsets = [0]
        while offsets[-1] + 14 <= n_bytes:
            offsets.append(offsets[-1] + rnd.randint(6, 14))
    else:
        offsets = list(range(0, n_bytes + 1, rec_len))
        assert all(len(p) > rec_len for p in extra)
    n_rec = len(offsets) - 1
    del text[offsets[-1]:]
    nested = patterns is TUPLE_PATTERNS
    plants = []  # (record, pattern, offset in the record)
    taken = set()
    for sp in spans:
        cand = [r for r in range(n_rec) if offsets[r] >= sp.start and offsets[r + 1] <= sp.end]
        assert not taken.intersection(cand), "spans overlap"
        taken.update(cand)
        for r in _pick(cand, offsets, sp.F, sp.placement, rnd):
            n = offsets[r + 1] - offsets[r]
            if nested:
                p = patterns[3 - sp.per_hit] if sp.per_hit > 1 else patterns[rnd.choice((2, 3))]
            else:
                assert sp.per_hit == 1
                p = rnd.choice([q for q in patterns if len(q) <= n])
            plants.append((r, p, rnd.randrange(0, n - len(p) + 1)))
    for r, p, o in plants:  # the guards first: the record next door may begin or end with its own pattern
        a, b = offsets[r] + o, offsets[r] + o + len(p)
        if a > offsets[r]:
            text[a - 1] = ord("T")
        if b < offsets[r + 1]:
            text[b] = ord("T")
    for r, p, o in plants:
        text[offsets[r] + o:offsets[r] + o + len(p)] = p
    flags = [False] * n_rec
    tuples = []
    all_patterns = list(patterns) + list(extra)
    for r, p, o in plants:
        flags[r] = True
        for qi, q in enumerate(all_patterns):
            k = p.find(q)
            while k != -1:
                tuples.append((r, qi, o + k))
                k = p.find(q, k + 1)
    tuples.sort()  # (record, pattern, position): the order of a BNDMq matcher, which these small sets get
    text = bytes(text)
    records = [text[offsets[r]:offsets[r + 1]] for r in range(n_rec)]
    return Case(name, rec_len, records, all_patterns, flags, tuples, offsets, tuple(spans))


def span_counts(case):
    """per span: (flagged records, tuples) whose record lies in the span entirely"""
    per_rec = [0] * len(case.records)
    for r, _, _ in case.tuples:
        per_rec[r] += 1
    out = []
    for sp in case.spans:
        inside = [r for r in range(len(case.records)) if case.offsets[r] >= sp.start and case.offsets[r + 1] <= sp.end]
        out.append((sum(case.flags[r] for r in inside), sum(per_rec[r] for r in inside)))
    return out


def occurrence_starts(case):
    """text positions of the occurrences, ascending"""
    return sorted(case.offsets[r] + pos for r, _, pos in case.tuples)


# ---------------------------------------------------------------------------------------------------- the cases
# One tile: 31 KiB for the grid's first wave and one more KiB, which a text needs behind its last tile (the guarded tail); 16 bytes
# more, so that a text cut to whole records of any length used here is still that long.
ONE_TILE_BYTES = TILE + CHUNK + 16
ONE_TILE_SPAN = (MARGIN, TILE - MARGIN)
KINDS = {"fixed8": 8, "fixed12": 12, "ragged": "ragged"}
F_EDGES = [0, 1, FLAG_LIST_CAP - 1, FLAG_LIST_CAP, FLAG_LIST_CAP + 1, FLAG_LIST_CAP + 63, FLAG_LIST_CAP + 64, FLAG_LIST_CAP + 65, None]
F_SWEEP = list(range(FLAG_LIST_CAP - 64, FLAG_LIST_CAP + 65))

_REGISTRY = {}


def _register(name, fn):
    assert name not in _REGISTRY, name
    _REGISTRY[name] = functools.lru_cache(maxsize=None)(fn)
    return name


def case(name):
    return _REGISTRY[name]()


def all_case_names():
    return list(_REGISTRY)


def _one_tile(kind, F, placement, extra=()):
    name = f"one-tile-{kind}-{'all' if F is None else F}-{placement}" + ("-2class" if extra else "")
    span = Span(0, ONE_TILE_BYTES, None, placement) if F is None else Span(*ONE_TILE_SPAN, F, placement)
    seed = list(KINDS).index(kind) * 100003 + (F or 0) * 7 + len(placement)
    return _register(name, lambda: make_case(name, KINDS[kind], ONE_TILE_BYTES, [span], seed, extra=extra))


def _placements(kind, F):
    if F is None:
        return ["clustered"]
    if F <= 1:
        return ["isolated"]
    return ["clustered", "mixed"] if kind == "fixed8" else ["clustered"]


EDGE_CASES = {kind: [_one_tile(kind, F, pl) for F in F_EDGES for pl in _placements(kind, F)] for kind in KINDS}
EDGE_CASES_2CLASS = [_one_tile("fixed8", F, pl, extra=(LONG_PATTERN,)) for F in F_EDGES for pl in _placements("fixed8", F)]
SWEEP_CASES = [f"one-tile-fixed8-{F}-clustered" if f"one-tile-fixed8-{F}-clustered" in _REGISTRY else _one_tile("fixed8", F, "clustered")
               for F in F_SWEEP]

# The wide control: q-grams of more than 16 bases need patterns, and so records, too long for 2048 of them in one tile.
WIDE_REC_LEN = 20
WIDE_CASES = []
for _F in (0, 1, 700, None):
    def _wide(F=_F):
        span = Span(0, ONE_TILE_BYTES, None, "clustered") if F is None else Span(*ONE_TILE_SPAN, F, "mixed")
        return make_case(f"wide-{F}", WIDE_REC_LEN, ONE_TILE_BYTES, [span], 4242 + (F or 0), patterns=WIDE_PATTERNS)
    WIDE_CASES.append(_register(f"wide-{'all' if _F is None else _F}", _wide))

# Several waves: six tiles and a tail of records of 12 bytes (a tile is no multiple of 12: records straddle the tile borders).
#   tile 0: over capacity      tile 1: exactly 2048        tile 2: no hit at all
#   tiles 3 and 4: a few hits each, and the record that straddles their border holds a pattern that straddles it too
SEVERAL_BYTES = 6 * TILE + 5 * CHUNK + 8
SEVERAL_STRADDLE = 4 * TILE


def _several(kind):
    def build():
        spans = [Span(0 * TILE + MARGIN, 1 * TILE - MARGIN, FLAG_LIST_CAP + 150, "clustered"),
                 Span(1 * TILE + MARGIN, 2 * TILE - MARGIN, FLAG_LIST_CAP, "mixed"),
                 Span(2 * TILE + MARGIN, 3 * TILE - MARGIN, 0, "isolated"),
                 Span(3 * TILE + MARGIN, 4 * TILE - MARGIN, 70, "isolated"),
                 Span(4 * TILE + MARGIN, 5 * TILE - MARGIN, 130, "clustered"),
                 Span(5 * TILE + MARGIN, 6 * TILE - MARGIN, 1, "isolated")]
        c = make_case(f"several-{kind}", KINDS[kind], SEVERAL_BYTES, spans, 977)
        # the straddler, by hand: the record over byte 4 * TILE gets a 6-mer whose third byte is the first of tile 4
        # (or, where the record leaves no room for that, as near to it as the record allows: the 6-mer still straddles)
        r = max(i for i in range(len(c.records)) if c.offsets[i] < SEVERAL_STRADDLE)
        n = c.offsets[r + 1] - c.offsets[r]
        o = min(max(SEVERAL_STRADDLE - 2 - c.offsets[r], 0), n - 6)
        assert not c.flags[r] and c.offsets[r + 1] > SEVERAL_STRADDLE and c.offsets[r] + o < SEVERAL_STRADDLE < c.offsets[r] + o + 6, (r, o, n)
        p = PATTERNS[4]
        rec = bytearray(b"T" + c.records[r] + b"T")
        rec[o:o + 8] = b"T" + p + b"T"
        c.records[r] = bytes(rec[1:-1])
        c.flags[r] = True
        c.tuples.append((r, 4, o))
        c.tuples.sort()
        return c
    return _register(f"several-{kind}", build)


SEVERAL_CASES = {kind: _several(kind) for kind in ("fixed12", "ragged")}

# Tuple staging: one tile again, T tuples staged by its wave.  A wave's rounds are of whatever size its hit buffer happens to
# drain at, so the totals are swept: every T (one tuple per hitting record) from a round below the flush edge to two rounds above it, with one, two and three
# tuples per hitting record -- whatever the rounds' sizes, each count from kHitStage - 65 to - 63 is met before a round
# somewhere in the sweep, and totals that end exactly on a flush (an empty last one) are in it.
TUPLE_TOTALS = list(range(STAGE_EDGE - 66, STAGE_EDGE + 132))
TUPLE_CASES = []
for _T in TUPLE_TOTALS:
    for _t in (1, 2, 3) if _T % 3 == 0 else (1,):  # (several tuples per record: every third total)
        def _tuples(T=_T, t=_t):
            spans = [Span(MARGIN, TILE // 2, T // t, "clustered", t)]
            if T % t:
                spans.append(Span(TILE // 2 + MARGIN, TILE - MARGIN, 1, "isolated", T % t))
            return make_case(f"tuples-{T}-by-{t}", 8, ONE_TILE_BYTES, spans, 31 * T + t, patterns=TUPLE_PATTERNS)
        TUPLE_CASES.append(_register(f"tuples-{_T}-by-{_t}", _tuples))
TUPLE_CAP_CASE = _register("tuples-cap", lambda: make_case("tuples-cap", 8, ONE_TILE_BYTES, [Span(*ONE_TILE_SPAN, 700, "mixed", 3)], 5,
                                                            patterns=TUPLE_PATTERNS))

# Handle history (tests/test_gpu_handle_history.py)
BIG_BYTES = TEXT_MAX
SMALL_BYTES = 20 * CHUNK
HISTORY_CASES = {
    "big": _register("history-big", lambda: make_case("history-big", 8, BIG_BYTES, [Span(0, BIG_BYTES, 30000, "mixed")], 11)),
    "small": _register("history-small", lambda: make_case("history-small", 8, SMALL_BYTES, [Span(0, SMALL_BYTES, 300, "mixed")], 12)),
    "dense": _register("history-dense", lambda: make_case("history-dense", 12, 120000, [Span(0, 120000, None, "clustered")], 13)),
    "none": _register("history-none", lambda: make_case("history-none", 12, 120000, [Span(0, 120000, 0, "isolated")], 14)),
    "12pct": _register("history-12pct", lambda: make_case("history-12pct", 12, 120000, [Span(0, 120000, 1200, "mixed")], 15)),
    "tuples": _register("history-tuples", lambda: make_case("history-tuples", 8, 64000, [Span(0, 64000, 2500, "mixed", 3)], 16,
                                                           patterns=TUPLE_PATTERNS)),
    "ragged": _register("history-ragged", lambda: make_case("history-ragged", "ragged", 100000, [Span(0, 100000, 3000, "mixed")], 17)),
    "fixed8": _register("history-fixed8", lambda: make_case("history-fixed8", 8, 80000, [Span(0, 80000, 2000, "mixed")], 18)),
    "ragged-30k": _register("history-ragged-30k", lambda: make_case("history-ragged-30k", "ragged", 30 * CHUNK, [Span(0, 30 * CHUNK, 900, "mixed")], 19)),
    "ragged-300k": _register("history-ragged-300k", lambda: make_case("history-ragged-300k", "ragged", 300 * CHUNK, [Span(0, 300 * CHUNK, 9000, "mixed")], 20)),
    "order-1000": _register("history-order-1000", lambda: make_case("history-order-1000", 12, 12000, [Span(0, 12000, 400, "mixed", 3)], 21,
                                                                   patterns=TUPLE_PATTERNS)),
    "order-10": _register("history-order-10", lambda: make_case("history-order-10", 12, 120, [Span(0, 120, 4, "mixed", 2)], 22,
                                                               patterns=TUPLE_PATTERNS)),
}
