"""One scan wave at the capacity of its flag list (kFlagListCap = 2048 entries, scan_kernel.h) and of its tuple staging buffer
(kHitStage = 1024 tuples; a wave flushes when more than kHitStage - 64 = 960 are staged, scan_kernel_impl.hpp: drain_hits).

The batches come from tests/scan_edge_cases.py, where the flags and tuples are planted, and tests/test_scan_edge_cases_cpu.py
has held each against the naive enumerator and the oracle.  Which wave scans which bytes is read from the launch itself
(mk_matcher_scan_geometry): every test asserts that the hits it counts lie in the tiles of the wave it means, at least 64 bytes
from a tile's ends, and fails when a change of the geometry has moved them.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import guarded as G
import scan_edge_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------------- geometry
def tiles_of(g):
    T, S, n_long = g["long_tile_bytes"], g["short_tile_bytes"], g["n_long_tiles"]
    return [(i * T, i * T + T) for i in range(n_long)] + [(n_long * T + j * S, n_long * T + j * S + S) for j in range(g["n_short_tiles"])]


def occurrences_per_wave(g, case):
    """{wave: occurrences that begin in one of its tiles, 64 bytes or more from the tile's ends}, and the occurrences elsewhere
    (near a border or in the tail: the premise of a case says how many of those it allows)"""
    tiles = tiles_of(g)
    per_wave, elsewhere = {}, []
    for p in sc.occurrence_starts(case):
        t = next((i for i, (a, b) in enumerate(tiles) if a + sc.MARGIN <= p < b - sc.MARGIN), None)
        if t is None:
            elsewhere.append(p)
        else:
            w = t % g["n_waves"]
            per_wave[w] = per_wave.get(w, 0) + 1
    return per_wave, elsewhere


class Batch:
    """a case's text on the device"""

    def __init__(self, mk, torch, case):
        self.mk, self.torch, self.case = mk, torch, case
        data, off = mk.pack_records(case.records)
        self.n_rec, self.n_bytes = len(case.records), int(off[-1])
        self.d_seq = torch.zeros(self.n_bytes + 64, dtype=torch.uint8, device="cuda:0")
        self.d_seq[:self.n_bytes] = torch.from_numpy(data[:self.n_bytes].copy()).to("cuda:0")
        self.d_off = torch.from_numpy(off.astype(np.int64)).to("cuda:0")
        self.flagged = sum(case.flags)
        self.per_pattern = np.bincount([p for _, p, _ in case.tuples], minlength=len(case.patterns)).tolist()

    def scan(self, m, mode, density, records="offsets", hits=None, cap=0, counters=False):
        """one mk_scan_device -> (flags, *d_n_hits, counters or None).  records: "fixed" (mk_matcher_set_fixed_record_length, no
        offsets given), "offsets" (the record of a hit is guessed from the mean length, then searched for) or "index" (the
        coarse record index of ragged batches)"""
        mk, torch, lib = self.mk, self.torch, self.mk.load()
        fixed = self.case.rec_len if records == "fixed" else 0
        assert lib.mk_matcher_set_fixed_record_length(m.handle, fixed) == 0
        assert lib.mk_matcher_hint_record_lengths(m.handle, 0 if records == "index" else 1) == 0
        if density is not None:
            m.hint_hit_density(density)
        flags = G.DeviceBuf(torch, np.uint8, self.n_rec, pad_to=4)
        nh = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
        cnt = torch.zeros(len(self.case.patterns) + mk.MK_NUM_SUMMARY, dtype=torch.int64, device="cuda:0") if counters else None
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.mk_scan_device(m.handle, self.d_seq.data_ptr(), self.n_bytes, None if fixed else self.d_off.data_ptr(), self.n_rec, mode,
                                flags.ptr, hits.ptr if hits is not None else None, cap, nh.data_ptr(), cnt.data_ptr() if counters else None, st)
        assert rc == mk.MK_OK, (rc, lib.mk_last_error())
        torch.cuda.synchronize()
        assert flags.guard_intact(), "the guard behind d_rec_flags was written"
        assert lib.mk_matcher_check_device(m.handle, st) == mk.MK_OK
        return flags.view(self.n_rec).astype(bool).tolist(), int(nh.item()), (cnt.cpu().numpy().tolist() if counters else None)

    def check_flags(self, m, density, records, what):
        """MK_MODE_ANY, and the count mode: tuples with counters, where mk_count_flags_kernel sees every flag byte of the scan"""
        mk, c = self.mk, self.case
        f, nh, _ = self.scan(m, mk.MK_MODE_ANY, density, records)
        name = m.kernel_name
        assert f == c.flags and nh == 0, f"{what}: MK_MODE_ANY, {name}: {_diff(f, c.flags)}"
        f, nh, cnt = self.scan(m, mk.MK_MODE_ANY, density, records, counters=True)
        n_pat = len(c.patterns)
        assert f == c.flags, f"{what}: MK_MODE_ANY with counters, {m.kernel_name}: {_diff(f, c.flags)}"
        assert cnt[n_pat + mk.MK_SUM_RECORDS_HIT] == self.flagged, (what, m.kernel_name, cnt[n_pat:])
        hits = G.DeviceBuf(self.torch, mk.HIT_DTYPE, len(c.tuples) + 8)
        f, nh, cnt = self.scan(m, mk.MK_MODE_HITS, density, records, hits=hits, cap=len(c.tuples) + 8, counters=True)
        assert f == c.flags and nh == len(c.tuples), f"{what}: count mode, {m.kernel_name}: {nh} tuples, {_diff(f, c.flags)}"
        assert cnt[:n_pat] == self.per_pattern and cnt[n_pat + mk.MK_SUM_RECORDS_HIT] == self.flagged, (what, m.kernel_name, cnt)
        assert cnt[n_pat + mk.MK_SUM_HITS] == len(c.tuples) and hits.untouched_from(len(c.tuples))
        return name


def _diff(got, want):
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    return f"{len(bad)} flags differ, first records {bad[:5]}" if bad else "flags equal"


def assert_one_wave(m, case, F):
    """the premise of a one-tile case: every occurrence lies in the first wave's only tile (F is None: all but those near its end
    and in the tail do, and they alone are more than the list holds)"""
    g = m.scan_geometry()
    assert len(tiles_of(g)) == 1 and tiles_of(g)[0] == (0, sc.TILE) and g["n_waves"] == 16, g
    per_wave, elsewhere = occurrences_per_wave(g, case)
    if F is None:
        assert set(per_wave) == {0} and per_wave[0] > sc.FLAG_LIST_CAP + 65 and len(elsewhere) < 300, (per_wave, len(elsewhere))
    else:
        assert per_wave == ({0: F} if F else {}) and not elsewhere, (per_wave, elsewhere[:4])
        assert sum(case.flags) == F == len(case.tuples)


def _F(name):
    f = name.split("-")[3]
    return None if f == "all" else int(f)


# ---------------------------------------------------------------------------------------------------- the flag list of one wave
# (options, density hint, the kernel's name: its part behind the sampling stride / what it ends with)
FAMILIES = {
    "lds": (None, 0, ("false,false>",)),
    "global-filter-sparse": (dict(force_global_filter=True), 0, ("false,true>",)),
    "global-filter-dense": (dict(force_global_filter=True), 1000, ("false,true>",)),   # the lists are live at either density
    "plain-control": (None, 1000, ("false,false,plain>",)),                            # no list: every flag is a direct store
}
RECORDS = [("fixed8", "fixed"), ("fixed8", "offsets"), ("fixed12", "fixed"), ("fixed12", "offsets"), ("ragged", "index"), ("ragged", "offsets")]


@pytest.mark.parametrize("kind,records", RECORDS, ids=[f"{k}-{r}" for k, r in RECORDS])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_flag_list_of_one_wave_at_its_edges(mk, torch, family, kind, records):
    options, density, ends = FAMILIES[family]
    m = mk.Matcher(sc.PATTERNS, options=options)
    assert not m.use_ac and m.class_info()["split_len"] == 0
    for name in sc.EDGE_CASES[kind]:
        b = Batch(mk, torch, sc.case(name))
        kn = b.check_flags(m, density, records, name)
        assert_one_wave(m, b.case, _F(name))
        assert kn.endswith(ends) and kn.endswith("plain>") == (family == "plain-control"), kn
    m.close()


@pytest.mark.parametrize("family", ["lds", "global-filter-sparse"])
def test_flag_list_fill_swept_over_the_capacity(mk, torch, family):
    """every fill from 2048 - 64 to 2048 + 64 with the hits in runs, so that whole rounds of up to 64 arrive at the list's end"""
    options, density, ends = FAMILIES[family]
    m = mk.Matcher(sc.PATTERNS, options=options)
    for name in sc.SWEEP_CASES:
        c = sc.case(name)
        b = Batch(mk, torch, c)
        for records in ("fixed", "offsets"):
            f, nh, cnt = b.scan(m, mk.MK_MODE_ANY, density, records, counters=True)
            assert not m.kernel_name.endswith("plain>") and m.kernel_name.endswith(ends), m.kernel_name
            assert f == c.flags, f"{name}, {records}, {m.kernel_name}: {_diff(f, c.flags)}"
            assert cnt[len(c.patterns) + mk.MK_SUM_RECORDS_HIT] == _F(name), (name, cnt)
        assert_one_wave(m, c, _F(name))
    m.close()


@pytest.mark.parametrize("options", [None, dict(force_global_filter=True)], ids=["lds", "global-filter"])
def test_flag_list_with_two_length_classes(mk, torch, options):
    m = mk.Matcher(sc.PATTERNS + [sc.LONG_PATTERN], options=options)
    assert m.class_info()["split_len"] == 40 and m.class_info()["n_short"] == len(sc.PATTERNS)
    for name in sc.EDGE_CASES_2CLASS:
        b = Batch(mk, torch, sc.case(name))
        for records in ("fixed", "offsets"):
            kn = b.check_flags(m, 0, records, name)
            assert kn.endswith("2-class>"), kn
        assert_one_wave(m, b.case, _F(name))
    m.close()


@pytest.mark.parametrize("density", [0, 1000])
def test_wide_keys_control(mk, torch, density):
    """q-grams of more than 16 bases (64-bit keys): records long enough for such patterns cannot fill a list from one tile, so this
    is the control in which a wave's list only ever grows -- from none to every record of the tile hitting"""
    m = mk.Matcher(sc.WIDE_PATTERNS, options=dict(force_stride=1))
    assert m.filter_info()["q_gram"] > 16, m.filter_info()
    for name in sc.WIDE_CASES:
        b = Batch(mk, torch, sc.case(name))
        for records in ("fixed", "offsets"):
            kn = b.check_flags(m, density, records, name)
            assert "<1,-1," in kn and kn.endswith("plain>") == (density == 1000), kn
        g = m.scan_geometry()
        per_wave, elsewhere = occurrences_per_wave(g, b.case)
        assert set(per_wave) <= {0} and len(elsewhere) < 120 and tiles_of(g) == [(0, sc.TILE)]
    m.close()


# ---------------------------------------------------------------------------------------------------- several waves
@pytest.mark.parametrize("kind,records", [("fixed12", "fixed"), ("fixed12", "offsets"), ("ragged", "index"), ("ragged", "offsets")])
@pytest.mark.parametrize("family", ["lds", "global-filter-sparse", "global-filter-dense"])
def test_neighbouring_waves_over_at_and_under_capacity(mk, torch, family, kind, records):
    """wave 0 over capacity, wave 1 exactly at it, wave 2 without a hit (its count of 0 must be written all the same: the scatter
    kernel reads every wave's), a record and its occurrence across the border of waves 3 and 4"""
    options, density, ends = FAMILIES[family]
    m = mk.Matcher(sc.PATTERNS, options=options)
    c = sc.case(sc.SEVERAL_CASES[kind])
    b = Batch(mk, torch, c)
    # a launch before it that leaves every wave's list and count in use: stale counts would show in wave 2
    full = Batch(mk, torch, sc.case("one-tile-fixed8-all-clustered"))
    for _ in range(2):
        full.scan(m, mk.MK_MODE_ANY, density, "fixed")
        kn = b.check_flags(m, density, records, c.name)
        assert kn.endswith(ends), kn
    g = m.scan_geometry()
    tiles = tiles_of(g)
    assert tiles == [(i * sc.TILE, (i + 1) * sc.TILE) for i in range(6)] and g["n_waves"] >= 16, g
    per_wave, elsewhere = occurrences_per_wave(g, c)
    assert per_wave == {0: sc.FLAG_LIST_CAP + 150, 1: sc.FLAG_LIST_CAP, 3: 70, 4: 130, 5: 1}, per_wave
    assert elsewhere == [sc.SEVERAL_STRADDLE - 2] or (kind == "ragged" and len(elsewhere) == 1 and abs(elsewhere[0] - sc.SEVERAL_STRADDLE) < 6)
    r = next(r for r in range(len(c.records)) if c.offsets[r] < sc.SEVERAL_STRADDLE < c.offsets[r + 1])
    assert c.flags[r]
    m.close()


# ---------------------------------------------------------------------------------------------------- tuple staging
def _tuples(hits, n):
    h = hits.view(n)
    return list(zip(h["rec"].tolist(), h["pat"].tolist(), h["pos"].tolist()))


@pytest.mark.parametrize("density", [0, 1000], ids=["sparse", "dense"])
@pytest.mark.parametrize("options", [None, dict(force_global_filter=True)], ids=["lds", "global-filter"])
def test_tuple_staging_swept_over_the_flush_edge(mk, torch, options, density):
    """a wave stages T tuples, T from below kHitStage - 64 = 960 to two rounds above it, one to three tuples per hitting record
    (patterns that end on the same byte): the flags -- set from the staged tuples at a flush in the sparse flavour -- and the
    ordered tuples are the planted ones"""
    lib = mk.load()
    m = mk.Matcher(sc.TUPLE_PATTERNS, options=options)
    assert not m.use_ac
    st = torch.cuda.current_stream().cuda_stream
    names = set()
    for name in sc.TUPLE_CASES:
        c = sc.case(name)
        T = len(c.tuples)
        b = Batch(mk, torch, c)
        hits = G.DeviceBuf(torch, mk.HIT_DTYPE, T)
        f, nh, _ = b.scan(m, mk.MK_MODE_HITS, density, "fixed", hits=hits, cap=T)
        names.add(m.kernel_name)
        assert nh == T and f == c.flags, f"{name}, {m.kernel_name}: {nh} tuples, {_diff(f, c.flags)}"
        assert hits.guard_intact() and set(_tuples(hits, T)) == set(c.tuples), name
        assert lib.mk_order_hits_device(m.handle, hits.ptr, T, st) == mk.MK_OK, lib.mk_last_error()
        torch.cuda.synchronize()
        assert _tuples(hits, T) == c.tuples and hits.guard_intact(), name
        g = m.scan_geometry()
        per_wave, elsewhere = occurrences_per_wave(g, c)
        assert per_wave == {0: T} and not elsewhere and tiles_of(g) == [(0, sc.TILE)], (name, per_wave)
        fa, _, _ = b.scan(m, mk.MK_MODE_ANY, density, "fixed")  # the same occurrences as list entries, several per record
        assert fa == c.flags, f"{name}, {m.kernel_name}: {_diff(fa, c.flags)}"
    assert all(n.endswith("plain>") == (density == 1000 and options is None) for n in names), names
    m.close()


@pytest.mark.parametrize("density", [0, 1000], ids=["sparse", "dense"])
def test_hits_cap_exactly_the_tuples_and_one_less(mk, torch, density):
    """2100 tuples of one wave, two flushes and a rest: hits_cap = the tuple count fits; one less states the need, keeps the flags
    and the counters, stores that many distinct tuples of the batch and writes nothing behind them -- and mk_scan_batch refuses
    with MK_E_CAPACITY and the need in *n_hits"""
    lib = mk.load()
    m = mk.Matcher(sc.TUPLE_PATTERNS)
    c = sc.case(sc.TUPLE_CAP_CASE)
    b = Batch(mk, torch, c)
    T, n_pat = len(c.tuples), len(c.patterns)
    assert T == 2100
    st = torch.cuda.current_stream().cuda_stream
    for cap in (T, T - 1):
        hits = G.DeviceBuf(torch, mk.HIT_DTYPE, cap)
        f, nh, cnt = b.scan(m, mk.MK_MODE_HITS, density, "fixed", hits=hits, cap=cap, counters=True)
        assert nh == T and f == c.flags and hits.guard_intact(), (cap, nh, m.kernel_name)
        got = _tuples(hits, cap)
        assert len(set(got)) == cap and set(got) <= set(c.tuples)
        assert cnt[:n_pat] == np.bincount(hits.view(cap)["pat"], minlength=n_pat).tolist()
        assert cnt[n_pat:n_pat + 4] == [T, sum(c.flags), len(c.records), b.n_bytes], cnt[n_pat:]
        stored = hits.view(cap).copy()
        assert lib.mk_order_hits_device(m.handle, hits.ptr, cap, st) == mk.MK_OK, lib.mk_last_error()
        torch.cuda.synchronize()
        assert _tuples(hits, cap) == sorted(zip(stored["rec"].tolist(), stored["pat"].tolist(), stored["pos"].tolist())) and hits.guard_intact()
        if cap == T:
            assert _tuples(hits, cap) == c.tuples
    per_wave, elsewhere = occurrences_per_wave(m.scan_geometry(), c)
    assert per_wave == {0: T} and not elsewhere
    m.hint_hit_density(density)
    flags, got = m.scan(c.records, mk.MK_MODE_HITS, hits_cap=T)
    assert flags.tolist() == c.flags and list(zip(got["rec"].tolist(), got["pat"].tolist(), got["pos"].tolist())) == c.tuples
    data, off = mk.pack_records(c.records)
    fl, nh = G.HostBuf(np.uint8, len(c.records)), np.zeros(1, dtype=np.uint64)
    out = G.HostBuf(mk.HIT_DTYPE, T - 1)
    rc = lib.mk_scan_batch(m.handle, data.ctypes.data, off.ctypes.data, len(c.records), mk.MK_MODE_HITS, fl.ptr, out.ptr, T - 1, nh.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == mk.MK_E_CAPACITY and int(nh[0]) == T and str(T).encode() in lib.mk_last_error()
    assert out.guard_intact() and fl.guard_intact() and fl.view().astype(bool).tolist() == c.flags
    m.close()
