"""The kernels of sets.hip -- per-record pattern sets, BNDMq's pattern_hit_counts, log rows, the paired list -- at their tile
and grid edges, against tuple_reference.py (numpy; pinned to the oracle by test_tuple_reference_cpu.py).

The set kernels work on tiles of 4096 tuples (1024 lanes x 4 consecutive tuples, 256 per wave), two single-workgroup scans give
each of 1024 lanes ceil(tiles / 1024) tiles, the prefix maximum over found_off has the same three-pass shape over n_rec + 1
entries, the row / mark kernels loop from 524 288 tuples on and the count kernels from 262 144.  Every case here is a batch built
so that a named edge of that geometry is hit, and it ASSERTS that from the reference's tuples in set order before the device is
called: a later change to a generator cannot empty a case silently.  Batches are patterns planted in a random background; the
expected values always come from tuple_reference on the bytes that are sent, never from what was planted.  The C ABI is called
with numpy buffers (mk_tag_records, mk_extract_single, mk_extract_paired); every comparison is exact equality of integer arrays.
Run on the GPU box with `-m gpu`."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import tuple_reference as tr

pytestmark = pytest.mark.gpu

TILE, WAVE, LANE = 4096, 256, 4   # sets.hip: kSetsTile, tuples per wave, kSetsPer
SCAN_LANES = 1024                 # lanes of mk_sets_scan_kernel / mk_prefmax_scan_kernel
ROW_GRID = 2048 * 256             # threads of the row and mark kernels: a second loop iteration from here on
COUNT_GRID = 1024 * 256           # ... of the count kernels
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ALGOS = [True, False]
ALGO_IDS = ["ac", "bndmq"]


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


# ---------------------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def _patterns(k, n, seed=1):
    """n distinct random k-mers, sorted (the id of a pattern is its index)"""
    rng = np.random.default_rng(seed)
    arr = np.unique(ACGT[rng.integers(0, 4, size=(n + 16, k))], axis=0)
    assert len(arr) >= n
    return tuple(arr[i].tobytes() for i in range(n))


def _batch(patterns, plan_rec, plan_pat, n_rec, seed, fill=None):
    """A packed batch of n_rec records.  A record is `fill` random bases (default: fewer than k, which cannot hold an occurrence)
    followed by its planted patterns back to back, in random order: plan_rec[j] is the record of plant j, plan_pat[j] its pattern.
    -> (data uint8[], off uint64[n_rec + 1])"""
    k = len(patterns[0])
    rng = np.random.default_rng(seed)
    pat_arr = np.frombuffer(b"".join(patterns), dtype=np.uint8).reshape(len(patterns), k)
    plan_rec, plan_pat = np.asarray(plan_rec, dtype=np.int64), np.asarray(plan_pat, dtype=np.int64)
    n = len(plan_rec)
    cnt = np.bincount(plan_rec, minlength=n_rec) if n else np.zeros(n_rec, dtype=np.int64)
    fill = rng.integers(0, k, size=n_rec) if fill is None else np.asarray(fill, dtype=np.int64)
    off = np.zeros(n_rec + 1, dtype=np.uint64)
    np.cumsum(fill + k * cnt, out=off[1:])
    total = int(off[-1])
    data = np.zeros(total + 64, dtype=np.uint8)
    data[:total] = ACGT[rng.integers(0, 4, size=total, dtype=np.uint8)]
    if n:
        order = np.lexsort((rng.random(n), plan_rec))
        r = plan_rec[order]
        slot = np.arange(n) - np.searchsorted(r, r, side="left")
        start = off[:-1].astype(np.int64)[r] + fill[r] + k * slot
        which = plan_pat[order]
        for a in range(0, n, 1 << 20):  # (in pieces: the index array of a piece is k times its plants)
            data[(start[a:a + (1 << 20), None] + np.arange(k)).ravel()] = pat_arr[which[a:a + (1 << 20)]].ravel()
    return data, off


def _top_up(patterns, data, off, target, seed=3):
    """records of exactly one pattern each appended until the reference counts `target` tuples -> (data, off, tuples)"""
    k = len(patterns[0])
    t = tr.occurrences(data, off, patterns)
    missing = target - len(t)
    assert missing >= 0, f"the body already holds {len(t)} tuples, more than {target}"
    if missing:
        rng = np.random.default_rng(seed)
        pat_arr = np.frombuffer(b"".join(patterns), dtype=np.uint8).reshape(len(patterns), k)
        total = int(off[-1])
        more = pat_arr[rng.integers(0, len(patterns), size=missing)].ravel()
        data = np.concatenate((data[:total], more, np.zeros(64, dtype=np.uint8)))
        off = np.concatenate((off, np.uint64(total) + np.arange(1, missing + 1, dtype=np.uint64) * np.uint64(k)))
        t = tr.occurrences(data, off, patterns)
    assert len(t) == target
    return data, off, t


def _random_plan(n, n_rec, n_pat, seed, repeat=0.35):
    """n plants over n_rec records; a plant repeats its predecessor's pattern with probability `repeat` when both lie in one
    record: (record, pattern) runs of several tuples"""
    rng = np.random.default_rng(seed)
    rec = np.sort(rng.integers(0, n_rec, size=n))
    pat = rng.integers(0, n_pat, size=n)
    copy = np.zeros(n, dtype=bool)
    copy[1:] = (rec[1:] == rec[:-1]) & (rng.random(n - 1) < repeat) if n > 1 else False
    src = np.maximum.accumulate(np.where(copy, 0, np.arange(n)))
    return rec, pat[src]


def _set_order_plan(n, seed, run_across=(), record_ends_before=(), gap=0, n_pat=256):
    """A plan written down in set order: tuple i of the reference's set order is plant i.  Random records of a few patterns with
    runs; tuples s - 1 and s share record and pattern for s in run_across; a record ends at s - 1 and the next one starts (with a
    head) at s for s in record_ends_before, with `gap` hitless records in between.  -> (plan_rec, plan_pat, n_rec)"""
    rng = np.random.default_rng(seed)
    new_rec = rng.random(n) < 0.3
    head = new_rec | (rng.random(n) < 0.5)
    new_rec[1::40] = True           # (odd indices: never a seam) at most 40 heads per record
    for s in run_across:
        new_rec[s] = False
        head[s] = False
    gaps = np.zeros(n, dtype=np.int64)
    for s in record_ends_before:
        new_rec[s] = True
        gaps[s] = gap
    new_rec[0] = True
    head |= new_rec
    rec = np.cumsum(np.where(new_rec, 1 + gaps, 0)) - 1
    start = np.maximum.accumulate(np.where(new_rec, np.arange(n), 0))  # first tuple of the record
    heads_before = np.cumsum(head)
    rank = heads_before - heads_before[start]                          # heads of the record in front of this tuple's: ascending ids
    pat = rank + 50 * (rec % 5)
    assert pat.max() < n_pat
    return rec, pat, int(rec[-1]) + 1


class Expected:
    """the reference's answers for one batch, each derived once"""

    def __init__(self, t):
        self.t = t
        self.set_order = t.bndmq_order()
        self.found_off, self.found_pat = t.pattern_sets()
        s = self.set_order
        self.head = np.ones(len(s), dtype=bool)
        self.head[1:] = (s.rec[1:] != s.rec[:-1]) | (s.pat[1:] != s.pat[:-1])

    @functools.lru_cache(maxsize=None)
    def order(self, ac):
        return self.t.ac_order() if ac else self.set_order

    @functools.lru_cache(maxsize=None)
    def counts(self, ac):
        return np.bincount(self.t.pat if ac else self.found_pat, minlength=self.t.n_pat).astype(np.uint32)

    def same_run(self, i):
        s = self.set_order
        return bool(s.rec[i - 1] == s.rec[i] and s.pat[i - 1] == s.pat[i])

    def record_ends_before(self, i):
        return bool(self.set_order.rec[i - 1] != self.set_order.rec[i])

    def tiles(self):
        return (len(self.t) + TILE - 1) // TILE

    def off_tiles(self):
        return (self.t.n_rec + 1 + TILE - 1) // TILE


# ---------------------------------------------------------------------------- the ABI with numpy buffers
def _matcher(mk, patterns, ac):
    m = mk.Matcher(list(patterns), algo=mk.MK_ALGO_AC if ac else mk.MK_ALGO_BNDMQ)
    assert m.use_ac == ac
    return m


def _same_rows(mk, rows, n_rows, file, rec, pat, pos, what):
    assert n_rows == len(rec), (what, n_rows, len(rec))
    r = rows[:n_rows]
    for name, want in (("rec", rec), ("pat", pat), ("pos", pos), ("file", file)):
        if not np.array_equal(r[name], want.astype(r[name].dtype)):
            i = int(np.flatnonzero(r[name] != want.astype(r[name].dtype))[0])
            raise AssertionError(f"{what}: row {i} of {n_rows} differs in `{name}`: {r[i:i + 2]} against "
                                 f"{(int(file[i]), int(rec[i]), int(pat[i]), int(pos[i]))}")
    assert not r["_pad"].any(), what
    assert (rows[n_rows:]["pat"] == 0xEEEEEEEE).all(), f"{what}: rows written behind the last one"


def _new_rows(mk, n):
    rows = np.zeros(n + 4, dtype=mk.ROW_DTYPE)
    rows["pat"] = 0xEEEEEEEE
    return rows


def _check_tag(mk, m, data, off, e, ac, logging=True, filter_matching=False, invert=False, what=""):
    lib, t = mk.load(), e.t
    n_rec, n = t.n_rec, len(t)
    keep = np.full(n_rec + 4, 0xEE, dtype=np.uint8)
    rows = _new_rows(mk, n)
    n_rows, c = C.c_uint64(), mk.Counters()
    counts = np.zeros(t.n_pat, dtype=np.uint32)
    foff = np.full(n_rec + 1, 0xEEEEEEEE, dtype=np.uint64)
    fpat = np.full(len(e.found_pat) + 4, 0xEEEEEEEE, dtype=np.uint32)
    rc = lib.mk_tag_records(m.handle, data.ctypes.data, off.ctypes.data, n_rec, int(logging), int(filter_matching), int(invert),
                            keep.ctypes.data, rows.ctypes.data, n, C.byref(n_rows), C.byref(c), counts.ctypes.data,
                            foff.ctypes.data, fpat.ctypes.data, len(e.found_pat))
    assert rc == 0, (what, lib.mk_last_error())
    if not np.array_equal(foff, e.found_off):
        i = int(np.flatnonzero(foff != e.found_off)[0])
        raise AssertionError(f"{what}: found_off[{i}] of {n_rec + 1} is {foff[i:i + 3]}, the reference has {e.found_off[i:i + 3]}")
    if not np.array_equal(fpat[:len(e.found_pat)], e.found_pat):
        i = int(np.flatnonzero(fpat[:len(e.found_pat)] != e.found_pat)[0])
        raise AssertionError(f"{what}: found_pat[{i}] of {len(e.found_pat)} is {fpat[i:i + 3]}, the reference has {e.found_pat[i:i + 3]}")
    assert (fpat[len(e.found_pat):] == 0xEEEEEEEE).all(), f"{what}: found_pat written behind its end"
    want_keep = t.tag_keep(filter_matching, invert)
    assert np.array_equal(keep[:n_rec], want_keep) and (keep[n_rec:] == 0xEE).all(), what
    if logging:
        o = e.order(ac)
        _same_rows(mk, rows, n_rows.value, np.zeros(n, dtype=np.uint32), o.rec, o.pat, o.pos, f"{what} tag rows")
        assert np.array_equal(counts, e.counts(ac)), f"{what}: pattern_hit_counts differ at {np.flatnonzero(counts != e.counts(ac))[:5]}"
        assert c.as_dict(counts) == dict(t.counters(want_keep), pattern_hit_counts=e.counts(ac).tolist()), what
    else:
        assert n_rows.value == 0 and not counts.any() and c.nb_records_extracted == int(want_keep.sum()) and c.nb_hits_tot[0] == 0, what


def _check_single(mk, m, data, off, e, ac, invert=False, what=""):
    lib, t = mk.load(), e.t
    n_rec, n = t.n_rec, len(t)
    keep = np.full(n_rec + 4, 0xEE, dtype=np.uint8)
    rows = _new_rows(mk, n)
    n_rows, c = C.c_uint64(), mk.Counters()
    counts = np.zeros(t.n_pat, dtype=np.uint32)
    rc = lib.mk_extract_single(m.handle, data.ctypes.data, off.ctypes.data, n_rec, 1, int(invert), keep.ctypes.data, rows.ctypes.data, n,
                               C.byref(n_rows), C.byref(c), counts.ctypes.data)
    assert rc == 0, (what, lib.mk_last_error())
    o = e.order(ac)
    _same_rows(mk, rows, n_rows.value, np.zeros(n, dtype=np.uint32), o.rec, o.pat, o.pos, f"{what} extract rows")
    want_keep = t.extract_keep(invert)
    assert np.array_equal(keep[:n_rec], want_keep) and (keep[n_rec:] == 0xEE).all(), what
    assert np.array_equal(counts, e.counts(ac)), f"{what}: pattern_hit_counts differ at {np.flatnonzero(counts != e.counts(ac))[:5]}"
    assert c.as_dict(counts) == dict(t.counters(want_keep), pattern_hit_counts=e.counts(ac).tolist()), what


def _check_paired(mk, m, b1, b2, pairs, ac, invert=False, what=""):
    lib = mk.load()
    (d1, o1), (d2, o2) = b1, b2
    n_rec, n = pairs.n_rec, len(pairs)
    keep = np.full(n_rec + 4, 0xEE, dtype=np.uint8)
    rows = _new_rows(mk, n)
    n_rows, c = C.c_uint64(), mk.Counters()
    counts = np.zeros(pairs.n_pat, dtype=np.uint32)
    rc = lib.mk_extract_paired(m.handle, d1.ctypes.data, o1.ctypes.data, n_rec, d2.ctypes.data, o2.ctypes.data, n_rec, 1, int(invert),
                               keep.ctypes.data, rows.ctypes.data, n, C.byref(n_rows), C.byref(c), counts.ctypes.data)
    assert rc == 0, (what, lib.mk_last_error())
    f, rec, pat, pos = pairs.rows(ac)
    _same_rows(mk, rows, n_rows.value, f, rec, pat, pos, f"{what} paired rows")
    want_keep = pairs.keep(invert)
    assert np.array_equal(keep[:n_rec], want_keep) and (keep[n_rec:] == 0xEE).all(), what
    want_counts = pairs.counts(ac)
    assert np.array_equal(counts, want_counts), f"{what}: pattern_hit_counts differ at {np.flatnonzero(counts != want_counts)[:5]}"
    assert c.as_dict(counts) == dict(pairs.counters(want_keep), pattern_hit_counts=want_counts.tolist()), what


# ---------------------------------------------------------------------------- sizes
SIZES = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193]


@functools.lru_cache(maxsize=None)
def _sized(n, n_rec):
    """exactly n tuples in exactly n_rec records (n_rec None: whatever the body and its top-up come to)"""
    patterns = _patterns(20, 64)
    if n_rec is None:
        body = max(0, n - 3)
        recs = max(1, body // 2)
        rec, pat = _random_plan(body, recs, 64, seed=n)
        data, off = _batch(patterns, rec, pat, recs, seed=n + 1)
    else:
        top = min(2, n_rec - 1, n)  # records the top-up is expected to add
        recs = n_rec - top
        rec, pat = _random_plan(n - top, recs, 64, seed=n + 7 * n_rec)
        data, off = _batch(patterns, rec, pat, recs, seed=n + 7 * n_rec + 1)
    data, off, t = _top_up(patterns, data, off, n)
    assert len(t) == n and (n_rec is None or t.n_rec == n_rec)
    return patterns, data, off, Expected(t)


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_tuple_counts_around_lane_wave_and_tile(mk, n, ac):
    """n tuples exactly: the i < n guards of mk_sets_count_kernel / mk_sets_emit_kernel (is_head and the `last` test's i + 1 == n)
    with n one short of, at and one past a lane (4), a wave (256), a tile (4096) and two tiles"""
    patterns, data, off, e = _sized(n, None)
    assert len(e.t) == n and e.tiles() == (n + TILE - 1) // TILE
    assert n < 8 or (e.head.sum() < n and e.t.flags().sum() < len(e.found_pat))  # runs of several tuples, records of several patterns
    m = _matcher(mk, patterns, ac)
    _check_tag(mk, m, data, off, e, ac, what=f"n={n}")
    _check_single(mk, m, data, off, e, ac, what=f"n={n}")
    _check_tag(mk, m, data, off, e, ac, logging=False, filter_matching=True, what=f"n={n} quiet")


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n_rec,n", [(1, 1), (1, 4097), (4095, 1), (4095, 4096), (4095, 8193), (4096, 4095), (4096, 4096), (4096, 8192),
                                     (4097, 5), (4097, 4097), (4097, 8191)])
def test_record_counts_around_the_offset_tile(mk, n_rec, n, ac):
    """n_rec + 1 offsets one short of, at and past a tile of mk_prefmax_tile_kernel / mk_prefmax_apply_kernel (n_rec = 4095: one full
    tile; 4096: one entry in the second tile), crossed with tuple counts at the tile edges; n_rec = 1: all tuples in one record"""
    patterns, data, off, e = _sized(n, n_rec)
    assert e.t.n_rec == n_rec and len(e.t) == n and e.off_tiles() == (n_rec + 1 + TILE - 1) // TILE
    m = _matcher(mk, patterns, ac)
    _check_tag(mk, m, data, off, e, ac, what=f"n_rec={n_rec} n={n}")
    _check_single(mk, m, data, off, e, ac, invert=True, what=f"n_rec={n_rec} n={n}")


# ---------------------------------------------------------------------------- seams
N_SEAM = 3 * TILE + 77
LANE_SEAMS, WAVE_SEAMS = (8, 4 * 333, TILE + 4 * 5), (WAVE, 5 * WAVE, TILE + 3 * WAVE)
SEAMS = {
    # name: (run_across, record_ends_before)
    "runs-across-both-tile-seams": (LANE_SEAMS + WAVE_SEAMS + (TILE, 2 * TILE), ()),
    "records-end-at-both-tile-seams": (LANE_SEAMS + WAVE_SEAMS, (TILE, 2 * TILE)),
    "run-across-the-first-record-end-at-the-second": (LANE_SEAMS + WAVE_SEAMS + (TILE,), (2 * TILE,)),
    "record-end-at-the-first-run-across-the-second": (LANE_SEAMS + WAVE_SEAMS + (2 * TILE,), (TILE,)),
}


@functools.lru_cache(maxsize=None)
def _seam_batch(name, gap):
    run_across, ends = SEAMS[name]
    patterns = _patterns(20, 256)
    rec, pat, n_rec = _set_order_plan(N_SEAM - 2, seed=len(name) + gap, run_across=run_across, record_ends_before=ends, gap=gap)
    fill = None
    if gap:  # hitless records of every kind: empty, shorter than k, longer than k
        fill = np.random.default_rng(9).choice([0, 0, 5, 19, 33], size=n_rec)
        fill[rec] = np.minimum(fill[rec], 19)
    data, off = _batch(patterns, rec, pat, n_rec, seed=17, fill=fill)
    data, off, t = _top_up(patterns, data, off, N_SEAM)
    return patterns, data, off, Expected(t)


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("gap", [0, 3, 5000], ids=["adjacent", "3-hitless-between", "5000-hitless-between"])
@pytest.mark.parametrize("name", list(SEAMS))
def test_runs_and_record_ends_at_the_seams(mk, name, gap, ac):
    """is_head's hv[i - 1] read from the previous lane, wave and tile (a run across the seam must NOT start a head there), and the
    `last` test's hv[i + 1] read from the next tile (a record whose last tuple is tuple 4095 / 8191 stores its found_off from the
    last lane of a tile; the head at the start of the next tile takes its rank from tile_base alone).  With hitless records in
    between, the entries of found_off behind that store are filled by the prefix maximum."""
    run_across, ends = SEAMS[name]
    patterns, data, off, e = _seam_batch(name, gap)
    assert len(e.t) == N_SEAM and e.tiles() == 4
    for s in run_across:
        assert e.same_run(s), f"tuples {s - 1} and {s} do not share record and pattern"
    s_ord = e.set_order
    for s in ends:
        assert e.record_ends_before(s) and e.head[s], f"no record ends with tuple {s - 1}"
        assert int(s_ord.rec[s]) - int(s_ord.rec[s - 1]) == gap + 1, "the records at the seam are not `gap` hitless records apart"
    m = _matcher(mk, patterns, ac)
    _check_tag(mk, m, data, off, e, ac, what=name)
    _check_single(mk, m, data, off, e, ac, what=name)


# ---------------------------------------------------------------------------- tiles without heads, tiles of heads only
@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
def test_one_run_over_whole_tiles(mk, ac):
    """a homopolymer record of 21 000 bases and the matching k-mer: one head, then tiles whose count is 0 (mk_sets_count_kernel
    stores 0, the scan carries the base over them, mk_sets_emit_kernel stores nothing but the one found_off of the record's last
    tuple); ordinary records before and after it"""
    k = 20
    patterns = tuple(sorted(_patterns(k, 40) + (b"A" * k,)))
    rec, pat = _random_plan(100, 60, 41, seed=4)
    d1, o1 = _batch(patterns, rec, pat, 60, seed=5)
    d2, o2 = _batch(patterns, rec, pat, 60, seed=6)
    n1, n2 = int(o1[-1]), int(o2[-1])
    data = np.concatenate((d1[:n1], np.full(21_000, ord("A"), dtype=np.uint8), d2[:n2], np.zeros(64, dtype=np.uint8)))
    off = np.concatenate((o1, np.uint64(n1 + 21_000) + o2))
    e = Expected(tr.occurrences(data, off, patterns))
    per_tile = np.add.reduceat(e.head.astype(np.int64), np.arange(0, len(e.t), TILE))
    assert len(e.t) >= 21_000 - k + 1 + 150 and e.tiles() >= 6
    assert per_tile[0] > 50 and not per_tile[1:5].any() and per_tile[5] > 0, per_tile  # four whole tiles without a head
    assert int(e.found_off[61]) - int(e.found_off[60]) == 1  # the long record: one pattern
    m = _matcher(mk, patterns, ac)
    _check_tag(mk, m, data, off, e, ac, what="homopolymer")
    _check_single(mk, m, data, off, e, ac, what="homopolymer")


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
def test_every_tuple_is_a_head(mk, ac):
    """every tuple has a (record, pattern) of its own over more than three tiles: every lane of mk_sets_emit_kernel stores four
    patterns, the rank of a lane is four times its index plus the tile's base, and the total is n"""
    patterns = _patterns(20, 64)
    n = 3 * TILE + 1234
    rec = np.repeat(np.arange(n // 3 + 1), 3)[:n]
    pat = (np.arange(n) % 3) * 20 + (rec % 20)  # three distinct patterns per record
    data, off = _batch(patterns, rec, pat, int(rec[-1]) + 1, seed=8)
    e = Expected(tr.occurrences(data, off, patterns))
    assert len(e.t) == n and e.head.all() and len(e.found_pat) == n and e.tiles() == 4
    m = _matcher(mk, patterns, ac)
    _check_tag(mk, m, data, off, e, ac, what="all heads")
    _check_single(mk, m, data, off, e, ac, what="all heads")


# ---------------------------------------------------------------------------- hitless stretches: the prefix maximum
def _stretch_batch(last_has_hits):
    patterns = _patterns(20, 64)
    g = 9000  # more than two tiles of mk_prefmax_*
    hit_recs = [g, g + 1, 2 * g + 2, 2 * g + 7]
    n_rec = 3 * g + 8
    if last_has_hits:
        hit_recs.append(n_rec - 1)
    rec = np.repeat(hit_recs, 3)
    pat = np.tile([5, 9, 9], len(hit_recs)) + np.repeat(np.arange(len(hit_recs)), 3)
    fill = np.random.default_rng(12).choice([0, 0, 3, 19, 35], size=n_rec)  # hitless records: empty, short, longer than k
    fill[hit_recs] = 7
    data, off = _batch(patterns, rec, pat, n_rec, seed=13, fill=fill)
    return patterns, data, off, Expected(tr.occurrences(data, off, patterns)), hit_recs


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("last_has_hits", [False, True], ids=["hitless-last-record", "last-record-hit"])
def test_hitless_stretches_of_more_than_two_tiles(mk, last_has_hits, ac):
    """9000 hitless records in front of the first hit, between two hits and behind the last one: found_off is 0 up to the first
    hit, flat across the gaps (the tile_before carry of mk_prefmax_scan_kernel / mk_prefmax_apply_kernel over tiles whose own
    maximum is 0) and equal to the total through found_off[n_rec]"""
    patterns, data, off, e, hit_recs = _stretch_batch(last_has_hits)
    g = 9000
    assert sorted(set(e.t.rec.tolist())) == hit_recs and g > 2 * TILE and e.off_tiles() >= 7
    total = len(e.found_pat)
    assert total == 2 * len(hit_recs)
    assert not e.found_off[:g + 1].any() and (e.found_off[g + 2:2 * g + 3] == 4).all()
    if last_has_hits:
        assert (e.found_off[2 * g + 8:e.t.n_rec] == 8).all() and e.found_off[e.t.n_rec] == total == 10
    else:
        assert (e.found_off[2 * g + 8:] == total).all() and e.t.n_rec - (2 * g + 8) >= g
    m = _matcher(mk, patterns, ac)
    for fm, inv in ((False, False), (True, False), (False, True)):
        _check_tag(mk, m, data, off, e, ac, filter_matching=fm, invert=inv, what="stretches")
    _check_single(mk, m, data, off, e, ac, what="stretches")


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("kind", ["no-hit", "all-empty"])
def test_batches_without_a_hit(mk, kind, ac):
    """no tuple at all (launch_pattern_sets runs the prefix maximum alone, over zeros) in 9000 records, and 9000 empty sequences"""
    patterns = _patterns(20, 64)
    n_rec = 9000
    fill = np.zeros(n_rec, dtype=np.int64) if kind == "all-empty" else np.random.default_rng(2).choice([0, 10, 19, 40], size=n_rec)
    data, off = _batch(patterns, [], [], n_rec, seed=3, fill=fill)
    e = Expected(tr.occurrences(data, off, patterns))
    assert len(e.t) == 0 and not e.found_off.any() and (int(off[-1]) == 0) == (kind == "all-empty")
    m = _matcher(mk, patterns, ac)
    _check_tag(mk, m, data, off, e, ac, invert=True, what=kind)
    _check_single(mk, m, data, off, e, ac, invert=True, what=kind)


# ---------------------------------------------------------------------------- more than 1024 tiles: per = 2 in both scans
BIG_REC = 1025 * TILE + 1000  # 4 199 400 records


@functools.lru_cache(maxsize=None)
def _big():
    k = 16
    patterns = _patterns(k, 1000, seed=21)
    n_rec = BIG_REC
    cnt = np.ones(n_rec, dtype=np.int64)
    r = np.arange(n_rec)
    cnt[r % 64 == 5] = 2     # two patterns
    cnt[r % 256 == 9] = 9    # nine hits of ONE pattern: runs that cross seams
    for a, b in ((0, 8200), (100_000, 109_000), (2_000_000, 2_010_000), (n_rec - 9500, n_rec)):
        cnt[a:b] = 0         # hitless stretches of more than 8192 records, the last one up to the end of the batch
    rng = np.random.default_rng(22)
    rec = np.repeat(r, cnt)
    pat = rng.integers(0, 1000, size=len(rec))
    first = np.searchsorted(rec, rec, side="left")
    run = cnt[rec] == 9
    pat[run] = pat[first[run]]
    fill = np.where(cnt == 0, rng.integers(0, k, size=n_rec), 0)
    data, off = _batch(patterns, rec, pat, n_rec, seed=23, fill=fill)
    t0 = time.perf_counter()
    e = Expected(tr.occurrences(data, off, patterns))
    print(f"big batch: {int(off[-1])} bytes, {len(e.t)} tuples, reference in {time.perf_counter() - t0:.1f} s")
    return patterns, data, off, e


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
def test_more_than_1024_tiles(mk, ac):
    """4.2 M records holding more tuples than that: mk_sets_scan_kernel and mk_prefmax_scan_kernel give each lane per = 2 tiles and
    the trailing lanes an empty range (lo = hi = n_tiles); neither tile count is a multiple of 1024.  AC with logging: rows, the
    per-hit histogram and the sets after the second ordering.  BNDMq with logging: the counts come from the sets, and
    mk_count_u32_kernel loops (more than 262 144 entries); mk_rows_kernel loops in both (more than 524 288 tuples)."""
    patterns, data, off, e = _big()
    n = len(e.t)
    assert e.t.n_rec >= 4_198_400 and n >= 4_198_400 and len(patterns) == 1000
    for tiles in (e.tiles(), e.off_tiles()):
        assert tiles > SCAN_LANES and tiles % SCAN_LANES != 0 and (tiles + SCAN_LANES - 1) // SCAN_LANES == 2
        assert (SCAN_LANES - 1) * 2 >= tiles  # the last lane's range is empty
    assert len(e.found_pat) > COUNT_GRID and n > ROW_GRID
    hitless = np.flatnonzero(np.diff(e.found_off) == 0)
    stretch = np.diff(np.flatnonzero(np.diff(hitless) != 1))  # lengths of the inner stretches of consecutive hitless records
    assert (stretch > 8192).sum() >= 2 and not e.found_off[:8193].any() and (e.found_off[-9000:] == len(e.found_pat)).all()
    seams = np.arange(TILE, n, TILE)
    s = e.set_order
    crossing = (s.rec[seams - 1] == s.rec[seams]) & (s.pat[seams - 1] == s.pat[seams])
    assert crossing.sum() >= 8, "fewer than 8 runs of one (record, pattern) cross a tile seam"
    m = _matcher(mk, patterns, ac)
    t0 = time.perf_counter()
    _check_tag(mk, m, data, off, e, ac, what="more than 1024 tiles")
    print(f"{n} tuples in {e.t.n_rec} records, {'AC' if ac else 'BNDMq'}: mk_tag_records and its comparison took {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------------------- paired
def _pair_batches(n1, n2, n_rec, seed, n_pat=64, k=20):
    """two mates of n_rec records with n1 / n2 tuples; pair p draws its patterns from three ids (the same pattern in both mates is
    common, and several times in mate 1); a third of the pairs is hit in mate 1 only, a third in mate 2 only or not at all"""
    patterns = _patterns(k, n_pat)
    rng = np.random.default_rng(seed)

    def plan(n, allowed):
        rec = np.sort(rng.choice(allowed, size=n)) if n else np.zeros(0, dtype=np.int64)
        return rec, (rec * 3 + rng.integers(0, 3, size=n)) % n_pat

    r = np.arange(n_rec)
    a1 = r[r % 3 != 1] if n_rec >= 6 else r
    a2 = r[r % 3 != 2][::2] if n_rec >= 6 else r
    r1, p1 = plan(n1, a1)
    r2, p2 = plan(n2, a2)
    b1 = _batch(patterns, r1, p1, n_rec, seed=seed + 1)
    b2 = _batch(patterns, r2, p2, n_rec, seed=seed + 2)
    return patterns, b1, b2


def _pairs_exactly(patterns, b1, b2, target):
    """pairs of (one pattern, an empty mate) appended until both mates together hold `target` tuples"""
    t1, t2 = tr.occurrences(*b1, patterns), tr.occurrences(*b2, patterns)
    missing = target - len(t1) - len(t2)
    assert missing >= 0
    if missing:
        d1, o1, t1 = _top_up(patterns, *b1, len(t1) + missing)
        d2, o2 = b2
        o2 = np.concatenate((o2, np.full(missing, o2[-1], dtype=np.uint64)))
        b1, b2 = (d1, o1), (d2, o2)
        t2 = tr.occurrences(*b2, patterns)
    pairs = tr.Pairs(t1, t2)
    assert len(pairs) == target
    return b1, b2, pairs


def _assert_pair_kinds(pairs):
    """the pairs that tell the counting rules apart are in the batch"""
    n_pat = pairs.n_pat
    key1 = np.unique(pairs.t1.rec * np.uint64(n_pat) + pairs.t1.pat, return_counts=True)
    key2 = np.unique(pairs.t2.rec * np.uint64(n_pat) + pairs.t2.pat)
    both = np.isin(key1[0], key2)
    assert (both & (key1[1] >= 2)).any(), "no pair with one pattern in both mates and several times in mate 1"
    f1, f2 = pairs.t1.flags(), pairs.t2.flags()
    assert (f1 & ~f2).any() and (~f1 & f2).any() and (~f1 & ~f2).any() and (f1 & f2).any()
    c_ac, c_bq = pairs.counts(True), pairs.counts(False)
    assert (c_bq < c_ac).any() and c_bq.sum() > len(np.union1d(key1[0], key2))  # neither per hit nor per (pair, pattern)


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n1,n2", [(1, 0), (0, 1), (2731, 1364), (4096, 0), (0, 4096), (1300, 2796), (3000, 1097)],
                         ids=["1-mate1", "1-mate2", "4095", "4096-mate1-only", "4096-mate2-only", "4096", "4097"])
def test_paired_tuple_counts(mk, n1, n2, ac):
    """1, 4095, 4096 and 4097 tuples in both mates together (the leaf and tile edges of the ordering and of the row / count kernels
    behind DeviceLoop::join_mates), among them a mate without any hit: its n1 == 0 and n2 == 0 branches"""
    n = n1 + n2
    n_rec = 5 if n == 1 else 1500
    patterns, b1, b2 = _pair_batches(max(0, n1 - (2 if n1 > 2 else 0)), n2, n_rec, seed=n1 + 3 * n2)
    if n1 == 0:  # (a top-up would put tuples into mate 1)
        pairs = tr.Pairs(tr.occurrences(*b1, patterns), tr.occurrences(*b2, patterns))
    else:
        b1, b2, pairs = _pairs_exactly(patterns, b1, b2, n)
    assert len(pairs) == n and (len(pairs.t1) == 0) == (n1 == 0) and (len(pairs.t2) == 0) == (n2 == 0)
    if n1 > 1 and n2 > 1:
        _assert_pair_kinds(pairs)
    m = _matcher(mk, patterns, ac)
    for inv in (False, True):
        _check_paired(mk, m, b1, b2, pairs, ac, invert=inv, what=f"pairs {n1}+{n2}")


@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
def test_paired_grid_stride_and_buffer_growth(mk, ac):
    """more than 600 000 tuples, mate 1 several times mate 2's: mk_pair_mark_kernel (on mate 1's list), mk_rows_pair_kernel and
    mk_count_pair_heads_kernel run a second grid-stride iteration.  On a fresh matcher the scan buffer holds mate 1's list plus a
    quarter (ensure_device's room to grow) when mate 2 has been scanned: both lists do not fit and join_mates grows the buffer,
    keeping mate 2's tuples."""
    n_rec = 150_000
    patterns, b1, b2 = _pair_batches(545_000, 165_000, n_rec, seed=31)
    pairs = tr.Pairs(tr.occurrences(*b1, patterns), tr.occurrences(*b2, patterns))
    n1, n2 = len(pairs.t1), len(pairs.t2)
    assert n1 + n2 >= 600_000 and n1 > ROW_GRID and n1 > 3 * n2
    assert n1 > max(4096, n_rec // 8)                         # mate 1's scan sized the buffer for its own list
    assert (n1 + n2) * 16 > n1 * 16 + n1 * 16 // 4 + 4096     # ... and both lists exceed that with its room to grow
    _assert_pair_kinds(pairs)
    m = _matcher(mk, patterns, ac)
    _check_paired(mk, m, b1, b2, pairs, ac, what="600 k pairs, fresh matcher")
    _check_paired(mk, m, b2, b1, tr.Pairs(pairs.t2, pairs.t1), ac, invert=True, what="600 k pairs, mates exchanged")


# ---------------------------------------------------------------------------- state between calls
@pytest.mark.parametrize("ac", ALGOS, ids=ALGO_IDS)
def test_results_do_not_depend_on_the_previous_batch(mk, ac):
    """a large batch, then a small one on the same matcher, and the reverse: the scratch (tile counts, found_off, found_pat, rows,
    the pair buffer) still holds the large batch's values wherever the small one does not write"""
    patterns, data_l, off_l, e_l = _seam_batch("records-end-at-both-tile-seams", 5000)
    rec, pat = _random_plan(5, 7, 256, seed=1)
    data_s, off_s = _batch(patterns, rec, pat, 7, seed=2, fill=[0, 3, 0, 19, 0, 0, 2])
    e_s = Expected(tr.occurrences(data_s, off_s, patterns))
    data_0, off_0 = _batch(patterns, [], [], 3, seed=2, fill=[0, 3, 19])
    e_0 = Expected(tr.occurrences(data_0, off_0, patterns))
    assert len(e_l.t) > 3 * TILE and e_l.t.n_rec > 2 * TILE and len(e_s.t) == 5 and len(e_0.t) == 0
    m = _matcher(mk, patterns, ac)
    for data, off, e, what in ((data_s, off_s, e_s, "small first"), (data_l, off_l, e_l, "large"), (data_s, off_s, e_s, "small after large"),
                               (data_0, off_0, e_0, "hitless after small"), (data_l, off_l, e_l, "large again"),
                               (data_0, off_0, e_0, "hitless after large"), (data_s, off_s, e_s, "small last")):
        _check_tag(mk, m, data, off, e, ac, what=what)
        _check_single(mk, m, data, off, e, ac, what=what)
    # the same for the paired loop: 4097 tuples, then 5 in 7 pairs, then the reverse
    _, b1, b2 = _pair_batches(3000, 1097, 1500, seed=77, n_pat=256)
    big = tr.Pairs(tr.occurrences(*b1, patterns), tr.occurrences(*b2, patterns))
    s1, s2 = (data_s, off_s), _batch(patterns, [0, 0, 6], [int(pat[0]), 3, 3], 7, seed=5)
    small = tr.Pairs(e_s.t, tr.occurrences(*s2, patterns))
    assert len(big) > TILE and len(small) == 8
    for x1, x2, p, what in ((s1, s2, small, "small pairs first"), (b1, b2, big, "large pairs"), (s1, s2, small, "small pairs after large"),
                            (b1, b2, big, "large pairs again")):
        _check_paired(mk, m, x1, x2, p, ac, what=what)
