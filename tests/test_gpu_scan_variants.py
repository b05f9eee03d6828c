"""Every compiled variant of the scan kernel, launched by name and held against the naive enumerator.

scan_variants.hip instantiates mk_scan_kernel 146 times (73 combinations of stride, q-gram mode, filter memory, load flavour
and short-class mode, with and without tuples) and launch_scan picks one from the matcher's geometry.  The family tests next
door (test_gpu_structured_sets.py, test_gpu_classes.py, test_gpu_parity.py, test_gpu_scan_wave_capacity.py) stress a few of them
with large sets and assert a part of the kernel's name.  Here every row of tests/scan_variant_matrix.py is made to run -- the
name the handle reports must EQUAL the row's -- on a batch of a few hundred KB that puts every pattern at every offset 0 .. 63
of a record (every residue of the stride, every byte of a 16-byte load, every lane slot), at both ends of records, across
record and tile borders and into the text's tail, next to a near-miss at every base.  Flags, ordered tuples, per-pattern and
summary counters are the enumerator's (tests/test_scan_variant_matrix_cpu.py has held every batch against the oracle, and every
recipe against mk_plan_geometry); each mode is scanned twice on one handle.  Run on the GPU box with `-m gpu`.
"""
import numpy as np
import pytest

import guarded as G
import scan_variant_matrix as sm

pytestmark = pytest.mark.gpu

_NAMES_SEEN = set()


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


def _same(got, exp, what):
    """got == exp for long lists, with a failure message that names the first difference"""
    if got == exp:
        return
    k = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    raise AssertionError(f"{what}: {len(got)} items, the enumerator has {len(exp)}; first difference at {k}: "
                         f"{got[k:k + 3]} against {exp[k:k + 3]}")


class OnDevice:
    """a row's text and record offsets on the device; one mk_scan_device per call"""

    def __init__(self, mk, torch, records):
        self.mk, self.torch = mk, torch
        data, off = mk.pack_records(records)
        self.n_rec, self.n_bytes = len(records), int(off[-1])
        self.d_seq = torch.zeros(self.n_bytes + 64, dtype=torch.uint8, device="cuda:0")
        self.d_seq[:self.n_bytes] = torch.from_numpy(data[:self.n_bytes].copy()).to("cuda:0")
        self.d_off = torch.from_numpy(off.astype(np.int64)).to("cuda:0")

    def scan(self, m, mode, plain, n_pat, hits=None, cap=0):
        """-> (flags, *d_n_hits, counters, kernel name); the hint is set before every scan, as the plain rows need it"""
        mk, torch, lib = self.mk, self.torch, self.mk.load()
        assert lib.mk_matcher_set_fixed_record_length(m.handle, 0) == 0
        assert lib.mk_matcher_hint_record_lengths(m.handle, 0) == 0  # records of many lengths: the coarse record index
        m.hint_hit_density(1000 if plain else 0)
        flags = G.DeviceBuf(torch, np.uint8, self.n_rec, pad_to=4)
        nh = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
        cnt = torch.zeros(n_pat + mk.MK_NUM_SUMMARY, dtype=torch.int64, device="cuda:0")
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.mk_scan_device(m.handle, self.d_seq.data_ptr(), self.n_bytes, self.d_off.data_ptr(), self.n_rec, mode, flags.ptr,
                                hits.ptr if hits is not None else None, cap, nh.data_ptr(), cnt.data_ptr(), st)
        assert rc == mk.MK_OK, (rc, lib.mk_last_error())
        torch.cuda.synchronize()
        assert flags.guard_intact(), "the guard behind d_rec_flags was written"
        assert lib.mk_matcher_check_device(m.handle, st) == mk.MK_OK, lib.mk_last_error()
        return flags.view(self.n_rec).astype(bool).tolist(), int(nh.item()), cnt.cpu().numpy().tolist(), m.kernel_name


def _check_any(mk, dev, m, v, e, what):
    n_pat = len(e.counts)
    flags, nh, cnt, name = dev.scan(m, mk.MK_MODE_ANY, v.plain, n_pat)
    _NAMES_SEEN.add(name)
    assert name == v.names[0], f"{what}: MK_MODE_ANY ran {name}, the row is {v.names[0]}"
    _same(flags, e.flags, f"{what} flags of MK_MODE_ANY ({name})")
    assert nh == 0 and cnt[n_pat + mk.MK_SUM_RECORDS_HIT] == e.records_hit, (what, nh, cnt[n_pat:])


def _check_hits(mk, torch, dev, m, v, e, what):
    lib, n_pat, T = mk.load(), len(e.counts), e.hits
    hits = G.DeviceBuf(torch, mk.HIT_DTYPE, T + 16)
    flags, nh, cnt, name = dev.scan(m, mk.MK_MODE_HITS, v.plain, n_pat, hits=hits, cap=T + 16)  # one launch: no capacity retry
    _NAMES_SEEN.add(name)
    assert name == v.names[1], f"{what}: MK_MODE_HITS ran {name}, the row is {v.names[1]}"
    assert hits.guard_intact() and hits.untouched_from(max(nh, T)), f"{what}: d_hits written behind the tuples ({name})"
    st = torch.cuda.current_stream().cuda_stream
    n = min(nh, T + 16)
    assert lib.mk_order_hits_device(m.handle, hits.ptr, n, st) == mk.MK_OK, lib.mk_last_error()
    torch.cuda.synchronize()
    path = m.order_info()["path"]
    h = hits.view(n)
    got = list(zip(h["rec"].tolist(), h["pat"].tolist(), h["pos"].tolist()))
    _same(got, e.tuples, f"{what} tuples ({name}, order path {path})")
    assert nh == T and path in (1, 2, 3), (what, nh, T, path)
    _same(flags, e.flags, f"{what} flags of MK_MODE_HITS ({name})")
    _same(cnt[:n_pat], e.counts, f"{what} per-pattern counters ({name})")
    summary = [cnt[n_pat + k] for k in (mk.MK_SUM_HITS, mk.MK_SUM_RECORDS_HIT, mk.MK_SUM_RECORDS, mk.MK_SUM_BASES)]
    assert summary == [e.hits, e.records_hit, e.records, e.bases], f"{what}: summary counters {summary} ({name})"


@pytest.mark.parametrize("vid", [v.id for v in sm.VARIANTS])
def test_variant_runs_and_matches_the_enumerator(mk, torch, vid):
    v = sm.BY_ID[vid]
    patterns, records = sm.batch(v)
    e = sm.expected(v)
    m = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, case_insensitive=v.ci, options=v.options)
    # ---- the geometry the CPU test planned
    plan = mk.plan_geometry([len(p) for p in patterns], v.options)
    info, ci = m.filter_info(), m.class_info()
    assert m.use_ac and (info["q_gram"], info["stride"]) == (plan["q_gram"], plan["stride"]) == (v.q, v.S), (info, plan)
    assert m.filter_mode()["in_lds"] is (not v.GF) and bool(plan["in_lds"]) == (not v.GF)
    assert ci == {k: plan[k] for k in ("split_len", "n_short", "q_gram2", "stride2")}, (ci, plan)
    assert ci["split_len"] == (v.lmin if v.MC else 0) and (ci["stride2"], ci["q_gram2"]) == (v.stride2, v.q2), ci
    dev = OnDevice(mk, torch, records)
    assert dev.n_bytes == e.bases and dev.n_rec == e.records
    for turn in ("first", "second"):  # a variant must not depend on what an earlier launch on the handle left behind
        _check_any(mk, dev, m, v, e, f"{vid}, {turn} scan")
        if turn == "first":  # the borders the batch was built around are those of this launch
            g = m.scan_geometry()
            assert g["n_long_tiles"] == 0 and g["short_tile_bytes"] == sm.TILE and g["tile_run"] == 1, g
            assert g["tail_start"] == e.bases - sm.TAIL_BYTES == g["n_short_tiles"] * sm.TILE, g
        _check_hits(mk, torch, dev, m, v, e, f"{vid}, {turn} scan")
    m.close()


def test_every_compiled_variant_was_launched():
    """the names the tests above saw are all 146.  It needs the whole module: with a selection of rows (-k, a single test id,
    --lf) it fails, because the rows left out were not launched, and says so rather than pass on a subset"""
    table = {n for v in sm.VARIANTS for n in v.names}
    assert len(table) == 146
    unknown = _NAMES_SEEN - table
    assert not unknown, f"kernel names no row of the table has: {sorted(unknown)}"
    missing = sorted(table - _NAMES_SEEN)
    assert not missing, (f"{len(missing)} of the 146 compiled variants were not launched in this run, first {missing[:4]}: either rows "
                         f"failed before their launches (see above), or only a part of this module was selected -- this test is "
                         f"meaningful only when all 73 rows run with it")
