"""Every output of the C ABI (include/merkurio_hip.h) that comes with a capacity, called DIRECTLY through native.load() -- not
through the retrying wrappers of native.py -- with guarded buffers (guarded.py): ample, exact fit (cap == need), one short
(need - 1, 0 with a pointer, need // 2), the same handle after a refusal, and the callers' grow-and-call-again loop when several
outputs are too small at once.  What a call returns when it fits is compared with the CPU oracle, and the needs it states with
what the oracle's result says they are.  mk_scan_device is scanned with hits_cap below, at and above the number of tuples in
every kernel family the scan can pick.  A test id carries the name of the call it covers.  Run on the GPU box with `-m gpu`.
"""
import ctypes as C
import functools
import gzip
import random
import struct

import numpy as np
import pytest

import guarded as G
import oracle_binding as ob
import structured_sets as ss
import test_gpu_bam_window as bw
import test_gpu_codec as tc
import test_gpu_order as to
import test_gpu_sam_window as sw
import test_gpu_structured_sets as tss
import test_gpu_windows as tw

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


def _ptr(a):
    return a.ctypes.data if a.size else None


# ============================================================================ mk_scan_device under overflow
def _core(raw, locus, j, width=100, start=0):
    """the text of j consecutive k-mers of a tiled locus, from its k-mer `start` on: exactly j occurrences"""
    a = locus * width + start
    return raw[a] + b"".join(raw[a + i][-1:] for i in range(1, j))


def _batches(recs, width):
    """of a tiled set's records (structured_sets.tiled: locus window, the same with one base changed, random read, ...): a batch of
    equal lengths in which every read hits, and a ragged one with empty and short records"""
    n = 32 if width == 100 else 240
    windows, subs, rnd = recs[0:3 * n:3], recs[1:3 * n:3], recs[2:3 * n:3]
    assert len(windows) == n and len({len(r) for r in windows}) == 1
    ragged = [r[:len(r) - (i * 7) % 40] for i, r in enumerate(windows[:n // 2] + subs[:n // 2] + rnd[:n // 4])]
    ragged[3:3] = [b"", b"ACG"]
    return {"fixed": windows, "ragged": ragged + [b""]}


class _Truth:
    def __init__(self, patterns, use_ac, recs, ci=False):
        om = ob.Matcher(patterns, use_ac, 0, ci)
        assert om.rc == 0
        _, rows, self.counters, found = ob.tag_records(om, recs, logging=True)
        self.ordered = [(r, p, pos) for (_, r, p, pos) in rows]
        self.T = set(self.ordered)
        assert len(self.T) == len(self.ordered)
        self.flags = [bool(f) for f in found]
        self.H = len(self.ordered)


def _hits_tuples(h):
    return list(zip(h["rec"].tolist(), h["pat"].tolist(), h["pos"].tolist()))


def _scan_device_caps(mk, torch, m, patterns, recs, truth, fixed_len, density):
    """mk_scan_device of one batch at every hits_cap of the issue's list; returns the kernel name"""
    lib = mk.load()
    n_rec, n_pat, H = len(recs), len(patterns), truth.H
    data, off = mk.pack_records(recs)
    n_bytes = int(off[-1])
    d_seq = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda:0")
    d_seq[:n_bytes] = torch.from_numpy(data[:n_bytes].copy()).to("cuda:0")
    d_off = torch.from_numpy(off.astype(np.int64)).to("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    plen = np.array([len(p) for p in patterns], dtype=np.int64)
    ac = m.use_ac
    assert lib.mk_matcher_set_fixed_record_length(m.handle, fixed_len) == 0
    off_ptr = None if fixed_len else d_off.data_ptr()

    def scan(mode, hits_ptr, cap, counters):
        flags = G.DeviceBuf(torch, np.uint8, n_rec, pad_to=4)
        nh = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
        cnt = torch.zeros(n_pat + mk.MK_NUM_SUMMARY, dtype=torch.int64, device="cuda:0") if counters else None
        m.hint_hit_density(density)
        rc = lib.mk_scan_device(m.handle, d_seq.data_ptr(), n_bytes, off_ptr, n_rec, mode, flags.ptr, hits_ptr, cap, nh.data_ptr(),
                                cnt.data_ptr() if counters else None, st)
        assert rc == mk.MK_OK, (rc, lib.mk_last_error())
        torch.cuda.synchronize()
        assert flags.guard_intact(), "the guard behind d_rec_flags was written"
        return flags.view(n_rec).astype(bool).tolist(), int(nh.item()), (cnt.cpu().numpy() if counters else None)

    f_any, nh_any, _ = scan(mk.MK_MODE_ANY, None, 0, False)
    assert f_any == truth.flags and nh_any == 0
    name = None
    # the ample run: the summary entries every other capacity must repeat
    ample = G.DeviceBuf(torch, mk.HIT_DTYPE, 4 * H)
    f, nh, c0 = scan(mk.MK_MODE_HITS, ample.ptr, 4 * H, True)
    assert nh == H and f == truth.flags and set(_hits_tuples(ample.view(H))) == truth.T and ample.untouched_from(H)
    assert c0[:n_pat].tolist() == np.bincount(ample.view(H)["pat"], minlength=n_pat).tolist()
    summary = c0[n_pat:n_pat + 4].tolist()
    assert summary == [H, sum(truth.flags), n_rec, n_bytes], summary
    for cap in (None, 0, 1, 63, 64, 65, H // 2, H - 1, H, H + 1):
        null = cap is None
        cap = 0 if null else cap
        for counters in (True, False):
            hits = None if null else G.DeviceBuf(torch, mk.HIT_DTYPE, cap)  # a fresh one per scan: each is checked on its own
            f, nh, c = scan(mk.MK_MODE_HITS, None if null else hits.ptr, cap, counters)
            what = f"hits_cap {cap}{' (NULL)' if null else ''} of {H}, {m.kernel_name}"
            name = m.kernel_name
            assert nh == H, f"{what}: *d_n_hits = {nh}"
            assert f == f_any == truth.flags, f"{what}: flags"
            n = min(cap, H)
            if hits is not None:
                assert hits.untouched_from(cap), f"{what}: d_hits written at element {hits.first_touched_from(cap)}"
                stored = hits.view(n).copy()
                got = _hits_tuples(stored)
                assert len(set(got)) == n and set(got) <= truth.T, f"{what}: the stored tuples are not distinct members of the batch's"
                if cap >= H:
                    assert set(got) == truth.T
            if counters:
                hist = np.bincount(stored["pat"], minlength=n_pat).tolist() if hits is not None else [0] * n_pat
                assert c[:n_pat].tolist() == hist and sum(hist) == n, f"{what}: per-pattern counters are not the histogram of the stored tuples"
                assert c[n_pat:n_pat + 4].tolist() == summary, f"{what}: summary entries {c[n_pat:n_pat + 4].tolist()}, ample run {summary}"
        assert lib.mk_matcher_check_device(m.handle, st) == mk.MK_OK
        if hits is not None:
            assert lib.mk_order_hits_device(m.handle, hits.ptr, n, st) == mk.MK_OK, lib.mk_last_error()
            torch.cuda.synchronize()
            assert hits.untouched_from(cap), f"{what}: mk_order_hits_device wrote behind the tuples"
            assert np.array_equal(hits.view(n), to._expected(stored, ac, plen)), f"{what}: order of the stored prefix"
            if cap >= H:
                assert _hits_tuples(hits.view(n)) == truth.ordered, f"{what}: emission order"
    assert lib.mk_matcher_set_fixed_record_length(m.handle, 0) == 0
    return name


_ALGO = {"auto": 0, "ac": 1, "bndmq": 2}


@pytest.mark.parametrize("case", tss.TILED, ids=[c[0] for c in tss.TILED])
def test_mk_scan_device_overflow_in_every_kernel_family(mk, torch, case):
    name, k, n_loci, options, list_kw, algo, ci, family, gf = case
    width = 13 if algo == "bndmq" else 100
    raw, recs = tss._tiled(n_loci, width, k)
    patterns = mk.parse_pattern_list(kmer_seq=raw, **list_kw)
    m = mk.Matcher(patterns, algo=_ALGO[algo], case_insensitive=ci, options=options)
    names = {}
    for kind, batch in _batches(recs, width).items():
        if ci:
            batch = ss.mixed_case(batch)
        truth = _Truth(patterns, m.use_ac, batch, ci)
        assert 1000 <= truth.H <= 20000, truth.H
        if kind == "fixed":
            assert all(truth.flags)  # the "every read hits" shape
        else:
            assert not all(truth.flags) and len({len(r) for r in batch}) > 10
        for density in (0, 1000):
            names[(kind, density)] = _scan_device_caps(mk, torch, m, patterns, batch, truth, len(batch[0]) if kind == "fixed" else 0, density)
            assert family in names[(kind, density)], names
    tss._check_kernel(m, family, gf)
    if not gf:  # both load flavours ran
        for kind in ("fixed", "ragged"):
            assert names[(kind, 0)] != names[(kind, 1000)] and names[(kind, 1000)].endswith("plain>"), names


@pytest.mark.parametrize("case", [tss.CLASSES[0], tss.CLASSES[1], tss.CLASSES[8], tss.CLASSES[-1]], ids=lambda c: c[0])
def test_mk_scan_device_overflow_with_two_length_classes(mk, torch, case):
    name, forced, options, family = case
    raw, recs = tss._tiled_short(forced)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    m = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=options)
    assert m.class_info()["split_len"] == 31
    for kind, batch in _batches(recs, 100).items():
        truth = _Truth(patterns, True, batch)
        assert 1000 <= truth.H <= 40000, truth.H
        for density in (0, 1000):
            kn = _scan_device_caps(mk, torch, m, patterns, batch, truth, len(batch[0]) if kind == "fixed" else 0, density)
            assert family in kn and kn.endswith("2-class>"), kn
    tss._check_kernel(m, family, bool(options and options.get("force_global_filter")), two_class=True)


# ============================================================================ mk_scan_batch
@functools.lru_cache(maxsize=None)
def _exact_batch(H):
    """reads of a tiled set with exactly H occurrences: 100 per read and one shorter read"""
    raw, _ = tss._tiled(40, 100, 31)
    recs = [_core(raw, i % 40, 100) for i in range(H // 100)] + [_core(raw, 7, H % 100)]
    return raw, recs


@pytest.mark.parametrize("H", [4095, 4097], ids=["host-order", "device-order"])
def test_mk_scan_batch_hits_cap(mk, H):
    raw, recs = _exact_batch(H)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    truth = _Truth(patterns, True, recs)
    assert truth.H == H  # just below / just above kSortOnDevice (4096): the host / device ordering switch of mk_scan_batch
    m = mk.Matcher(patterns)
    lib = mk.load()
    data, off = mk.pack_records(recs)

    def call(cap, alloc):
        hits = G.HostBuf(mk.HIT_DTYPE, alloc)
        flags = G.HostBuf(np.uint8, len(recs))
        nh = C.c_uint64(12345)
        rc = lib.mk_scan_batch(m.handle, data.ctypes.data, off.ctypes.data, len(recs), mk.MK_MODE_HITS, flags.ptr, hits.ptr, cap, C.byref(nh))
        assert flags.guard_intact() and flags.view().astype(bool).tolist() == truth.flags, cap  # valid under overflow as well
        assert hits.untouched_from(cap), f"hits_cap {cap}: written at element {hits.first_touched_from(cap)}"
        return rc, nh.value, hits

    rc, n, hits = call(4 * H, 4 * H)
    assert rc == mk.MK_OK and n == H and _hits_tuples(hits.view(H)) == truth.ordered and hits.untouched_from(H)
    for cap in (H - 1, 0, H // 2, 1, 1023, 1024, 1025):  # batch_scan's device buffer starts at max(hits_cap, 1024)
        err0 = G.set_sentinel_error(mk)
        rc, n, _ = call(cap, H)
        assert rc == mk.MK_E_CAPACITY and n == H, (cap, rc, n)
        assert lib.mk_last_error() != err0 and str(H).encode() in lib.mk_last_error()
        rc, n, hits = call(H, H)  # exact fit, and the same handle after the refusal
        assert rc == mk.MK_OK and n == H and _hits_tuples(hits.view(H)) == truth.ordered, cap
    assert m.order_info()["path"] in (1, 2) if H >= 4096 else True


# ============================================================================ the driver loops on host batches
def _records_batch(kind, algo):
    """(raw patterns, records).  "few-huge" and "many-small": every scan of the batch -- of either half, for the paired loop --
    finds more tuples than the driver loops' first tuple buffer holds (_overflows), under either algorithm.  BNDMq gets 13
    patterns (the auto rule's bound): the middle k-mer of 13 loci."""
    raw, recs = tss._tiled(40, 100, 31)
    bndmq = algo == "bndmq"
    if bndmq:
        raw = [raw[l * 100 + 50] for l in range(13)]
    if kind == "small":
        return raw, _batches(recs, 100)["ragged"]
    if kind == "few-huge":  # few records with thousands of occurrences each
        if bndmq:
            return raw, [(raw[i] + b"N" + raw[i + 6] + b"N") * 1500 for i in range(6)] + [b"ACGTN" * 40]
        return raw, [b"".join(_core(raw, (i + j) % 40, 100) + b"N" for j in range(30)) for i in range(6)] + [b"ACGTN" * 40]
    rnd = random.Random(5)  # 20 000 records with two occurrences each (BNDMq: one), some without any
    n_loci = 13 if bndmq else 40
    tiled = tss._tiled(40, 100, 31)[0]
    return raw, [_core(tiled, rnd.randrange(n_loci), 2, start=50) if i % 10 else b"ACGT" * 8 for i in range(20000)]


def _overflows(kind, n_tuples, n_rec):
    """the batch is what its name says: the first scan of a fresh handle finds more tuples than the buffer it starts with
    (device_loop.hpp, scan_flags: max(4096, n_rec / 8)) and is repeated inside the call"""
    return kind == "small" or n_tuples > max(4096, n_rec // 8)


def _single_protocol(mk, m, recs, logging, invert, paired=False):
    lib = mk.load()
    n_pat = len(m.patterns)
    if paired:
        h = len(recs) // 2
        d1, o1 = mk.pack_records(recs[:h])
        d2, o2 = mk.pack_records(recs[h:2 * h])
        n = h
    else:
        d1, o1 = mk.pack_records(recs)
        n = len(recs)

    def invoke(caps, bufs):
        keep = G.HostBuf(np.uint8, n)
        c, counts, n_rows = mk.Counters(), np.zeros(n_pat, dtype=np.uint32), C.c_uint64(777)
        if paired:
            rc = lib.mk_extract_paired(m.handle, d1.ctypes.data, o1.ctypes.data, n, d2.ctypes.data, o2.ctypes.data, n, int(logging), int(invert),
                                       keep.ptr, bufs["rows"].ptr, caps["rows"], C.byref(n_rows), C.byref(c), counts.ctypes.data)
        else:
            rc = lib.mk_extract_single(m.handle, d1.ctypes.data, o1.ctypes.data, n, int(logging), int(invert), keep.ptr, bufs["rows"].ptr,
                                       caps["rows"], C.byref(n_rows), C.byref(c), counts.ctypes.data)
        assert keep.guard_intact()
        res = None
        if rc == mk.MK_OK:
            res = (keep.view().astype(bool).tolist(), G.rows_list(bufs["rows"].view(n_rows.value)), c.as_dict(counts))
        bufs["_partial"] = (keep.view().astype(bool).tolist(), G.rows_list(bufs["rows"].view(min(caps["rows"], n_rows.value))), c.as_dict(counts))
        return rc, {"rows": n_rows.value}, res
    return G.Protocol(mk, {"rows": [("rows", mk.ROW_DTYPE, 0)]}, invoke, {"rows": 0}, work_done=(("rows",), lambda R: R))


def _no_logging(mk, m, om, recs, paired):
    """logging == 0: keep and nb_records_extracted only; the rows buffer, with or without a capacity, stays untouched"""
    h = len(recs) // 2
    for invert in (False, True):
        exp = ob.extract_paired(om, recs[:h], recs[h:2 * h], logging=False, invert=invert) if paired else ob.extract_single(om, recs, logging=False, invert=invert)
        assert exp[1] == []
        p = _single_protocol(mk, m, recs, False, invert, paired=paired)
        for cap in (0, 4):
            o = p.call({"rows": cap}, alloc={"rows": 4})
            assert o.rc == mk.MK_OK and o.results == exp and o.needs["rows"] == 0 and o.bufs["rows"].untouched_from(0), (invert, cap)


@pytest.mark.parametrize("algo", ["ac", "bndmq"])
@pytest.mark.parametrize("kind", ["small", "few-huge", "many-small"])
def test_mk_extract_single_rows_cap(mk, kind, algo):
    raw, recs = _records_batch(kind, algo)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    om = ob.Matcher(patterns, algo == "ac", 0, False)
    for invert in (False, True):
        m = mk.Matcher(patterns, algo=_ALGO[algo])  # a fresh handle: its first call scans with scan_grow's first, too small buffer
        exp = ob.extract_single(om, recs, logging=True, invert=invert)
        assert _overflows(kind, len(exp[1]), len(recs))
        p = _single_protocol(mk, m, recs, True, invert)
        p.ample = {"rows": 4 * len(exp[1]) + 8}
        p.run(exp, {"rows": len(exp[1])})
    _no_logging(mk, mk.Matcher(patterns, algo=_ALGO[algo]), om, recs, paired=False)


@pytest.mark.parametrize("algo", ["ac", "bndmq"])
@pytest.mark.parametrize("kind", ["small", "few-huge", "many-small"])
def test_mk_extract_paired_rows_cap(mk, kind, algo):
    raw, recs = _records_batch(kind, algo)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    om = ob.Matcher(patterns, algo == "ac", 0, False)
    h = len(recs) // 2
    for invert in (False, True):
        m = mk.Matcher(patterns, algo=_ALGO[algo])  # a fresh handle: both mates' first scans outgrow its first tuple buffer
        exp = ob.extract_paired(om, recs[:h], recs[h:2 * h], logging=True, invert=invert)
        for mate in (0, 1):
            assert _overflows(kind, sum(r[0] == mate for r in exp[1]), h)
        p = _single_protocol(mk, m, recs, True, invert, paired=True)
        p.ample = {"rows": 4 * len(exp[1]) + 8}
        p.run(exp, {"rows": len(exp[1])})
    _no_logging(mk, mk.Matcher(patterns, algo=_ALGO[algo]), om, recs, paired=True)


@pytest.mark.parametrize("algo", ["ac", "bndmq"])
@pytest.mark.parametrize("logging", [1, 0])
@pytest.mark.parametrize("kind", ["small", "few-huge", "many-small"])
def test_mk_tag_records_rows_cap_and_found_cap(mk, kind, logging, algo):
    raw, recs = _records_batch(kind, algo)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    om = ob.Matcher(patterns, algo == "ac", 0, False)
    m = mk.Matcher(patterns, algo=_ALGO[algo])
    lib = mk.load()
    n, n_pat = len(recs), len(patterns)
    data, off = mk.pack_records(recs)
    keep_o, rows_o, c_o, found_o = ob.tag_records(om, recs, logging=bool(logging), filter_matching=True)
    sets_o = [sorted(set(f)) for f in found_o]
    exp = (keep_o, rows_o, c_o, sets_o)
    assert _overflows(kind, len(ob.tag_records(om, recs, logging=True)[1]), n)

    def invoke(caps, bufs):
        keep, foff = G.HostBuf(np.uint8, n), G.HostBuf(np.uint64, n + 1)
        c, counts, n_rows = mk.Counters(), np.zeros(n_pat, dtype=np.uint32), C.c_uint64(777)
        rows = bufs["rows"] if logging else None
        rc = lib.mk_tag_records(m.handle, data.ctypes.data, off.ctypes.data, n, logging, 1, 0, keep.ptr, rows.ptr if rows else None,
                                caps["rows"] if logging else 0, C.byref(n_rows), C.byref(c), counts.ctypes.data, foff.ptr, bufs["found"].ptr, caps["found"])
        assert keep.guard_intact() and foff.guard_intact()
        fo = foff.view().tolist()
        res = None
        if rc == mk.MK_OK:
            fp = bufs["found"].view(fo[n]).tolist()
            res = (keep.view().astype(bool).tolist(), G.rows_list(rows.view(n_rows.value)) if logging else [], c.as_dict(counts),
                   [fp[fo[i]:fo[i + 1]] for i in range(n)])
        needs = {"found": fo[n]}
        if logging:
            needs["rows"] = n_rows.value
        bufs["_partial"] = (keep.view().astype(bool).tolist(), G.rows_list(rows.view(min(caps["rows"], n_rows.value))) if logging else [], c.as_dict(counts))
        return rc, needs, res

    outputs = {"found": [("found", np.uint32, 0)]}
    needs = {"found": sum(map(len, sets_o))}  # distinct (record, pattern) pairs
    if logging:
        outputs["rows"] = [("rows", mk.ROW_DTYPE, 0)]
        needs["rows"] = len(rows_o)
    # the header: both needs are stated by one call (found_off[n_rec] and *n_rows)
    p = G.Protocol(mk, outputs, invoke, {k: 4 * v + 8 for k, v in needs.items()}, states_all=True, work_done=(("rows", "found"), lambda R: R[:3]))
    p.run(exp, needs)


def test_mk_tag_value_cap(mk):
    raw, _ = tss._tiled(40, 100, 31)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    m = mk.Matcher(patterns)
    lib = mk.load()
    for found, existing in (([5, 1, 700, 5], None), ([3], b"ZZZ,AAA"), (list(range(0, 300, 7)), b"TTTT," + patterns[14])):
        want = ob.tag_value(patterns, found, existing)
        N = len(want)
        assert N >= 2
        arr = np.asarray(found, dtype=np.uint32)

        def call(cap):
            out = G.HostBuf(np.uint8, N + 1)
            n = C.c_size_t(99)
            rc = lib.mk_tag_value(m.handle, arr.ctypes.data, len(found), existing, C.cast(out.ptr, C.c_char_p), cap, C.byref(n))
            assert out.untouched_from(cap), (cap, out.first_touched_from(cap))
            return rc, n.value, out

        rc, n, out = call(N + 1)  # the need excludes the NUL: len + 1 fits
        assert rc == mk.MK_OK and n == N and out.view().tobytes() == want + b"\0"
        for cap in (N, N - 1, 0, N // 2):  # cap == len must fail: no room for the NUL
            err0 = G.set_sentinel_error(mk)
            rc, n, out = call(cap)
            assert rc == mk.MK_E_CAPACITY and n == N, (cap, rc, n)
            assert lib.mk_last_error() != err0 and str(N + 1).encode() in lib.mk_last_error()
            rc, n, out = call(N + 1)
            assert rc == mk.MK_OK and n == N and out.view().tobytes() == want + b"\0"


# ============================================================================ text windows
def _fastq_window(seed=3, n=600):
    """(patterns, [(id, sequence, quality)]): every third read carries a pattern, some two"""
    rnd = random.Random(seed)
    patterns = sorted({tw._rand(rnd, 31) for _ in range(150)})
    recs = []
    for i in range(n):
        L = rnd.choice([36, 75, 150, 151])
        s = bytearray(tw._rand(rnd, L))
        for _ in range(0 if i % 3 else rnd.choice((1, 1, 2))):
            k = rnd.randrange(0, L - 31 + 1)
            s[k:k + 31] = rnd.choice(patterns)
        recs.append((b"r%d extra" % i, bytes(s), tw._rand(rnd, L, b"@+IJ#5ACGT>")))
    return patterns, recs


def _window_protocol(mk, m, codec, fmt, srcs, want, logging, invert):
    """mk_extract_window.  srcs: dicts as native.Matcher.extract_window takes them; want: per source the texts that come back.
    Capacities: rec, rows, and per source k tail<k> / kept<k> / all<k>."""
    lib = mk.load()
    n_pat, n_src = len(m.patterns), len(srcs)
    hold = []
    arr = (mk.WindowSource * n_src)()
    for k, sd in enumerate(srcs):
        S = arr[k]
        head = np.frombuffer(sd.get("head", b""), dtype=np.uint8)
        hold.append(head)
        S.head, S.n_head = _ptr(head), head.size
        if "members" in sd:
            mem, blob = sd["members"].copy(), np.frombuffer(sd["blob"], dtype=np.uint8)
            mem["out_off"] -= mem["out_off"][0]
            hold += [mem, blob]
            S.bgzf, S.n_bgzf, S.members, S.n_members = blob.ctypes.data, blob.size, mem.ctypes.data, len(mem)
        else:
            text = np.frombuffer(sd["text"], dtype=np.uint8)
            hold.append(text)
            S.text, S.n_text = _ptr(text), text.size
        S.ends_at_record = int(sd.get("ends_at_record", True))
    outputs = {"rec": [(f"rec_start{k}", np.uint64, 1) for k in range(n_src)] + [("keep", np.uint8, 0)]}
    if logging:
        outputs["rows"] = [("rows", mk.ROW_DTYPE, 0)]
    for k in range(n_src):
        for w in want:
            outputs[f"{w}{k}"] = [(f"{w}{k}", np.uint8, 0)]

    def invoke(caps, bufs):
        for k in range(n_src):
            S = arr[k]
            S.rec_start = bufs[f"rec_start{k}"].ptr
            if "tail" in want:
                S.tail, S.tail_cap = bufs[f"tail{k}"].ptr, caps[f"tail{k}"]
            if "kept" in want:
                S.kept, S.kept_cap = bufs[f"kept{k}"].ptr, caps[f"kept{k}"]
            if "all" in want:
                S.all, S.all_cap = bufs[f"all{k}"].ptr, caps[f"all{k}"]
        c, counts = mk.Counters(), np.zeros(n_pat, dtype=np.uint32)
        n_rec, n_rows, status = C.c_uint64(777), C.c_uint64(777), C.c_uint32(7)
        rows = bufs["rows"] if logging else None
        rc = lib.mk_extract_window(m.handle, codec._h if codec else None, fmt, n_src, arr, int(logging), int(invert), caps["rec"], C.byref(n_rec),
                                   bufs["keep"].ptr, rows.ptr if rows else None, caps["rows"] if logging else 0, C.byref(n_rows), C.byref(c),
                                   counts.ctypes.data, C.byref(status))
        assert status.value == 0
        needs = {"rec": n_rec.value}
        if logging:
            needs["rows"] = n_rows.value
        for k in range(n_src):
            S = arr[k]
            for w, v in (("tail", S.n_tail), ("kept", S.n_kept_bytes), ("all", S.n_window)):
                if w in want:
                    needs[f"{w}{k}"] = v
        res = None
        if rc == mk.MK_OK:
            n = n_rec.value
            res = {"keep": bufs["keep"].view(n).astype(bool).tolist(), "rows": G.rows_list(rows.view(n_rows.value)) if logging else [],
                   "counters": c.as_dict(counts)}
            for k in range(n_src):
                S = arr[k]
                res[f"rec_start{k}"] = bufs[f"rec_start{k}"].view(n + 1).tolist()
                res[f"n_used{k}"] = S.n_used
                for w, v in (("tail", S.n_tail), ("kept", S.n_kept_bytes), ("all", S.n_window)):
                    if w in want:
                        res[f"{w}{k}"] = bufs[f"{w}{k}"].view(v).tobytes()
        if n_rec.value <= caps["rec"]:  # (the rows: *n_rows is stated only when the texts fit; the protocol's rows_cap never exceeds the need)
            bufs["_partial"] = (bufs["keep"].view(n_rec.value).astype(bool).tolist(), G.rows_list(rows.view(caps["rows"])) if logging else [], c.as_dict(counts))
        return rc, needs, res
    done = (["rows"] if logging else []) + [f"kept{k}" for k in range(n_src) if "kept" in want]
    p = G.Protocol(mk, outputs, invoke, None, work_done=(done, lambda R: (R["keep"], R["rows"], R["counters"])))
    p.hold = (hold, arr)
    return p


def _window_expected(fmt_starts, texts, keep, rows, counters, want, n):
    """fmt_starts: per source the record starts in its window text (n + 1 entries, the last = n_used)"""
    exp = {"keep": keep, "rows": rows, "counters": counters}
    needs = {"rec": n, "rows": len(rows)}
    for k, (starts, text) in enumerate(zip(fmt_starts, texts)):
        exp[f"rec_start{k}"], exp[f"n_used{k}"] = starts, starts[n]
        vals = {"tail": text[starts[n]:], "kept": b"".join(text[starts[r]:starts[r + 1]] for r in range(n) if keep[r]), "all": text}
        for w in want:
            exp[f"{w}{k}"] = vals[w]
            needs[f"{w}{k}"] = len(vals[w])
    return exp, needs


def _fastq_starts(recs, eol=b"\n"):
    starts = [0]
    for rid, s, q in recs:
        starts.append(starts[-1] + len(tw._fastq([(rid, s, q)], eol)))
    return starts


def _run_window(mk, p, exp, needs, logging):
    if not logging:
        needs = {k: v for k, v in needs.items() if k != "rows"}
    p.ample = {k: 4 * v + 64 for k, v in needs.items()}
    return p.run(exp, needs)


@pytest.mark.parametrize("logging,invert", [(True, False), (False, True)])
def test_mk_extract_window_fastq_caps(mk, logging, invert):
    patterns, recs = _fastq_window()
    text = tw._fastq(recs) + b"@unfinished record\nACGTACGTAC"
    m = mk.Matcher(patterns)
    om = ob.Matcher(patterns, True, 0, False)
    k_o, r_o, c_o = ob.extract_single(om, [s for _, s, _ in recs], logging=logging, invert=invert)
    want = ("tail", "kept", "all")
    exp, needs = _window_expected([_fastq_starts(recs)], [text], k_o, r_o, c_o, want, len(recs))
    assert needs["tail0"] == 29
    p = _window_protocol(mk, m, None, mk.MK_TEXT_FASTQ, [{"text": text, "ends_at_record": False}], want, logging, invert)
    _run_window(mk, p, exp, needs, logging)


def test_mk_extract_window_fasta_caps(mk):
    patterns, recs = _fastq_window(seed=4, n=400)
    fa = [(rid, s) for rid, s, _ in recs]
    text = tw._fasta(fa, 60)
    starts, _, seqs = tw._parse_fasta(text)
    n = len(fa) - 1  # a window that may end anywhere: its last record cannot be known to be whole and stays behind as the tail
    m = mk.Matcher(patterns)
    om = ob.Matcher(patterns, True, 0, False)
    k_o, r_o, c_o = ob.extract_single(om, seqs[:n], logging=True, invert=False)
    want = ("tail", "kept")
    exp, needs = _window_expected([starts[:n + 1]], [text], k_o, r_o, c_o, want, n)
    p = _window_protocol(mk, m, None, mk.MK_TEXT_FASTA, [{"text": text, "ends_at_record": False}], want, True, False)
    _run_window(mk, p, exp, needs, True)


def test_mk_extract_window_paired_caps(mk):
    patterns, recs1 = _fastq_window(seed=5, n=300)
    _, recs2 = _fastq_window(seed=6, n=300)
    recs2 = [(rid, s if i % 2 else patterns[7] + s, None) for i, (rid, s, _) in enumerate(recs2)]
    recs2 = [(rid, s, b"I" * len(s)) for rid, s, _ in recs2]
    t1 = tw._fastq(recs1) + b"@half\nACGT\n+"
    t2 = tw._fastq(recs2) + b"@other half\nAC"
    m = mk.Matcher(patterns)
    om = ob.Matcher(patterns, True, 0, False)
    k_o, r_o, c_o = ob.extract_paired(om, [s for _, s, _ in recs1], [s for _, s, _ in recs2], logging=True, invert=False)
    want = ("tail", "kept")
    exp, needs = _window_expected([_fastq_starts(recs1), _fastq_starts(recs2)], [t1, t2], k_o, r_o, c_o, want, 300)
    p = _window_protocol(mk, m, None, mk.MK_TEXT_FASTQ, [{"text": t1, "ends_at_record": False}, {"text": t2, "ends_at_record": False}], want, True, False)
    _run_window(mk, p, exp, needs, True)


def test_mk_extract_window_bgzf_source_caps(mk):
    patterns, recs = _fastq_window(seed=8, n=500)
    body = tw._fastq(recs) + b"@cut here\nACGTAC"
    head = body[:100]
    blob = tw._bgzf(body[100:], 9000)
    members, used, _ = mk.bgzf_members(blob)
    assert used == len(blob) and len(members) >= 5
    m, codec = mk.Matcher(patterns), mk.Codec(0)
    om = ob.Matcher(patterns, True, 0, False)
    k_o, r_o, c_o = ob.extract_single(om, [s for _, s, _ in recs], logging=True, invert=False)
    want = ("tail", "kept")
    exp, needs = _window_expected([_fastq_starts(recs)], [body], k_o, r_o, c_o, want, len(recs))
    p = _window_protocol(mk, m, codec, mk.MK_TEXT_FASTQ, [{"head": head, "blob": blob, "members": members, "ends_at_record": False}], want, True, False)
    _run_window(mk, p, exp, needs, True)
    codec.close()


def test_mk_extract_fastq_text_caps(mk):
    patterns, recs = _fastq_window(seed=9, n=500)
    text = tw._fastq(recs)
    buf = np.frombuffer(text, dtype=np.uint8)
    m = mk.Matcher(patterns)
    om = ob.Matcher(patterns, True, 0, False)
    lib = mk.load()
    exp = ob.extract_single(om, [s for _, s, _ in recs], logging=True, invert=False)
    starts = _fastq_starts(recs)

    def invoke(caps, bufs):
        c, counts = mk.Counters(), np.zeros(len(patterns), dtype=np.uint32)
        n_rec, n_rows, status = C.c_uint64(777), C.c_uint64(777), C.c_uint32(7)
        rc = lib.mk_extract_fastq_text(m.handle, buf.ctypes.data, buf.size, 1, 0, caps["rec"], C.byref(n_rec), bufs["rec_start"].ptr, bufs["keep"].ptr,
                                       bufs["rows"].ptr, caps["rows"], C.byref(n_rows), C.byref(c), counts.ctypes.data, C.byref(status))
        assert status.value == 0
        res = None
        if rc == mk.MK_OK:
            n = n_rec.value
            res = (bufs["keep"].view(n).astype(bool).tolist(), G.rows_list(bufs["rows"].view(n_rows.value)), c.as_dict(counts),
                   bufs["rec_start"].view(n + 1).tolist())
        if n_rec.value <= caps["rec"]:
            bufs["_partial"] = (bufs["keep"].view(n_rec.value).astype(bool).tolist(), G.rows_list(bufs["rows"].view(caps["rows"])), c.as_dict(counts))
        return rc, {"rec": n_rec.value, "rows": n_rows.value}, res
    needs = {"rec": len(recs), "rows": len(exp[1])}
    p = G.Protocol(mk, {"rec": [("rec_start", np.uint64, 1), ("keep", np.uint8, 0)], "rows": [("rows", mk.ROW_DTYPE, 0)]}, invoke,
                   {k: 4 * v for k, v in needs.items()}, work_done=(("rows",), lambda R: R[:3]))
    p.run(exp + (starts,), needs)


@pytest.mark.parametrize("whole_text", [True, False], ids=["text_cap", "kept_cap"])
def test_mk_extract_fastq_bgzf_caps(mk, whole_text):
    patterns, recs = _fastq_window(seed=10, n=500)
    body = tw._fastq(recs) + b"@cut here\nACGTAC"
    head = body[:77]
    blob = tw._bgzf(body[77:], 7000)
    members, used, _ = mk.bgzf_members(blob)
    hb, bb = np.frombuffer(head, dtype=np.uint8), np.frombuffer(blob, dtype=np.uint8)
    m, codec = mk.Matcher(patterns), mk.Codec(0)
    om = ob.Matcher(patterns, True, 0, False)
    lib = mk.load()
    keep_o, rows_o, c_o = ob.extract_single(om, [s for _, s, _ in recs], logging=True, invert=False)
    starts = _fastq_starts(recs)
    kept_o = b"".join(body[starts[r]:starts[r + 1]] for r in range(len(recs)) if keep_o[r])
    texts = ("text",) if whole_text else ("tail", "kept")

    def invoke(caps, bufs):
        io = mk.WindowText()
        if whole_text:
            io.text, io.text_cap = bufs["text"].ptr, caps["text"]
        else:
            io.tail, io.tail_cap, io.kept, io.kept_cap = bufs["tail"].ptr, caps["tail"], bufs["kept"].ptr, caps["kept"]
        c, counts = mk.Counters(), np.zeros(len(patterns), dtype=np.uint32)
        n_rec, n_rows, status = C.c_uint64(777), C.c_uint64(777), C.c_uint32(7)
        rc = lib.mk_extract_fastq_bgzf(m.handle, codec._h, hb.ctypes.data, hb.size, bb.ctypes.data, bb.size, members.ctypes.data, len(members), 0, C.byref(io),
                                       1, 0, caps["rec"], C.byref(n_rec), bufs["rec_start"].ptr, bufs["keep"].ptr, bufs["rows"].ptr, caps["rows"],
                                       C.byref(n_rows), C.byref(c), counts.ctypes.data, C.byref(status))
        assert status.value == 0
        needs = {"rec": n_rec.value, "rows": n_rows.value}
        needs.update({"text": io.n_text} if whole_text else {"tail": io.n_tail, "kept": io.n_kept_bytes})
        res = None
        if rc == mk.MK_OK:
            n = n_rec.value
            res = {"keep": bufs["keep"].view(n).astype(bool).tolist(), "rows": G.rows_list(bufs["rows"].view(n_rows.value)), "counters": c.as_dict(counts),
                   "rec_start": bufs["rec_start"].view(n + 1).tolist(), "n_used": io.n_used, "n_text": io.n_text}
            res.update({t: bufs[t].view(needs[t]).tobytes() for t in texts})
        if n_rec.value <= caps["rec"]:
            bufs["_partial"] = (bufs["keep"].view(n_rec.value).astype(bool).tolist(), G.rows_list(bufs["rows"].view(caps["rows"])), c.as_dict(counts))
        return rc, needs, res
    exp = {"keep": keep_o, "rows": rows_o, "counters": c_o, "rec_start": starts, "n_used": starts[-1], "n_text": len(body)}
    exp.update({"text": body} if whole_text else {"tail": body[starts[-1]:], "kept": kept_o})
    needs = {"rec": len(recs), "rows": len(rows_o)}
    needs.update({"text": len(body)} if whole_text else {"tail": len(body) - starts[-1], "kept": len(kept_o)})  # len(text) - n_used
    outputs = {"rec": [("rec_start", np.uint64, 1), ("keep", np.uint8, 0)], "rows": [("rows", mk.ROW_DTYPE, 0)]}
    outputs.update({t: [(t, np.uint8, 0)] for t in texts})
    G.Protocol(mk, outputs, invoke, {k: 4 * v + 64 for k, v in needs.items()},
               work_done=(("rows", "kept"), lambda R: (R["keep"], R["rows"], R["counters"]))).run(exp, needs)
    codec.close()


# ============================================================================ tag windows
def _tag_window_protocol(mk, W, call, n_pat, logging, nothing_counted):
    """mk_tag_bam_window / mk_tag_sam_window: tail, out, rows + row_name, names.  W: the window struct with its inputs set."""
    outputs = {"tail": [("tail", np.uint8, 0)], "out": [("out", np.uint8, 0)]}
    if logging:
        outputs.update({"rows": [("rows", mk.ROW_DTYPE, 0), ("row_name", np.uint64, 0)], "names": [("names", np.uint8, 0)]})

    def invoke(caps, bufs):
        W.tail, W.tail_cap, W.out, W.out_cap = bufs["tail"].ptr, caps["tail"], bufs["out"].ptr, caps["out"]
        if logging:
            W.rows, W.rows_cap, W.row_name, W.names, W.names_cap = bufs["rows"].ptr, caps["rows"], bufs["row_name"].ptr, bufs["names"].ptr, caps["names"]
        c, counts, status = mk.Counters(), np.zeros(n_pat, dtype=np.uint32), C.c_uint32(7)
        c.nb_records_tot, c.nb_hits_tot[0] = 11, 13  # what the caller has counted so far
        counts[:] = 5
        rc = call(W, int(logging), c, counts, status)
        assert status.value == 0
        if rc != mk.MK_OK and nothing_counted:  # the counters are added when the window is done
            assert (c.nb_records_tot, c.nb_bases, c.nb_hits_tot[0], c.nb_records_hit[0], c.nb_records_extracted) == (11, 0, 13, 0, 0)
            assert (counts == 5).all()
        needs = {"tail": W.n_tail, "out": W.out_len}
        if logging:
            needs.update({"rows": W.n_rows, "names": W.n_names_bytes})
        res = None
        if rc == mk.MK_OK:
            c.nb_records_tot -= 11
            c.nb_hits_tot[0] -= 13
            counts -= 5
            res = {"n_rec": W.n_rec, "n_used": W.n_used, "n_kept": W.n_kept, "tail": bufs["tail"].view(W.n_tail).tobytes(),
                   "out": bufs["out"].view(W.out_len).tobytes(), "counters": c.as_dict(counts)}
            if logging:
                nb = bufs["names"].view(W.n_names_bytes).tobytes()
                rows, rn = bufs["rows"].view(W.n_rows), bufs["row_name"].view(W.n_rows).tolist()
                res["rows"] = [(nb[a:nb.index(b"\0", a)], int(r["rec"]), int(r["pat"]), int(r["pos"])) for a, r in zip(rn, rows)]
        return rc, needs, res
    return G.Protocol(mk, outputs, invoke, None)


def _tag_expected(keep, rows, c, logging):
    c = dict(c)
    c["extracted"] = sum(keep)  # (the device reports the records it wrote; the reference has no such counter in tag)
    if not logging:
        c = {**c, "records": 0, "bases": 0, "hits": (0, 0), "records_hit": (0, 0), "pattern_hit_counts": [0] * len(c["pattern_hit_counts"])}
    return c


@pytest.mark.parametrize("logging", [True, False])
def test_mk_tag_sam_window_caps(mk, logging):
    rnd = random.Random(12)
    pats = sw.patterns31(mk)
    text = b"".join(sw.sam_line(rnd, i, pats, hit=0.5) for i in range(800))
    body = text + b"unfinished\t0\tchr1"
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    lib = mk.load()
    keep, rows, c, out, n_rec = sw.expected(om, pats, text, b"km", logging, True, False)
    hb, tb = np.frombuffer(body[:50], dtype=np.uint8), np.frombuffer(body[50:], dtype=np.uint8)
    W = mk.SamWindow()
    W.head, W.n_head, W.text, W.n_text, W.last, W.filter_matching, W.invert = hb.ctypes.data, hb.size, tb.ctypes.data, tb.size, 0, 1, 0
    W.tag[0], W.tag[1] = b"km"
    p = _tag_window_protocol(mk, W, lambda W, lg, c, counts, st: lib.mk_tag_sam_window(m.handle, C.byref(W), lg, C.byref(c), counts.ctypes.data, C.byref(st)),
                             len(pats), logging, nothing_counted=True)
    exp = {"n_rec": n_rec, "n_used": len(text), "n_kept": sum(keep), "tail": body[len(text):], "out": out, "counters": _tag_expected(keep, rows, c, logging)}
    needs = {"tail": len(body) - len(text), "out": len(out)}
    if logging:
        exp["rows"] = rows
        hit_names = [nm for nm, k in zip([r[1] for r in sw.records_of(text)[0]], keep) if k]  # filter_matching: kept == has a hit
        needs.update({"rows": len(rows), "names": sum(len(nm) + 1 for nm in hit_names)})
    p.ample = {k: 4 * v + 64 for k, v in needs.items()}
    p.run(exp, needs)


@pytest.mark.parametrize("logging", [True, False])
def test_mk_tag_bam_window_caps(mk, logging):
    rnd = random.Random(13)
    pats = bw.patterns31(mk)
    recs = bw.make_records(rnd, 800, pats, hit=0.5)
    text = b"".join(recs)
    body = text + bw.bam_record(b"cut", b"ACGT" * 20)[:40]
    blob = bw._bgzf(body[64:], 20000)
    members, used, _ = mk.bgzf_members(blob)
    assert used == len(blob)
    members["out_off"] -= members["out_off"][0]
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    lib = mk.load()
    keep, rows, c, out = bw.expected(om, pats, recs, b"km", logging, True, False)
    hb, bb = np.frombuffer(body[:64], dtype=np.uint8), np.frombuffer(blob, dtype=np.uint8)
    W = mk.BamWindow()
    W.head, W.n_head, W.bgzf, W.n_bgzf, W.members, W.n_members = hb.ctypes.data, hb.size, bb.ctypes.data, bb.size, members.ctypes.data, len(members)
    W.last, W.filter_matching, W.invert, W.block_bytes = 0, 1, 0, 9000
    W.tag[0], W.tag[1] = b"km"
    p = _tag_window_protocol(mk, W, lambda W, lg, c, counts, st: lib.mk_tag_bam_window(m.handle, codec._h, C.byref(W), lg, C.byref(c), counts.ctypes.data, C.byref(st)),
                             len(pats), logging, nothing_counted=True)
    inner = p.invoke

    def invoke(caps, bufs):  # the members are this library's own parse: compared by what they inflate to
        rc, needs, res = inner(caps, bufs)
        if res is not None:
            res["out"] = gzip.decompress(res["out"] + mk.bgzf_eof()) if res["out"] else b""
            res["out_text_bytes"] = W.out_text_bytes
        return rc, needs, res
    p.invoke = invoke
    exp = {"n_rec": len(recs), "n_used": len(text), "n_kept": sum(keep), "tail": body[len(text):], "out": out, "out_text_bytes": len(out),
           "counters": _tag_expected(keep, rows, c, logging)}
    needs = {"tail": 40}
    assert len(out) > 3 * 9000  # several output members
    ample = {"tail": 4096, "out": 4 * mk.load().mk_bgzf_deflate_bound(len(out), 9000)}
    if logging:
        exp["rows"] = rows
        hit_names = [bw.decode(r)[0] for r, k in zip(recs, keep) if k]
        needs.update({"rows": len(rows), "names": sum(len(nm) + 1 for nm in hit_names)})
        ample.update({"rows": 4 * len(rows), "names": 4 * needs["names"]})
    p.ample = ample
    p.run(exp, needs)
    codec.close()


# ============================================================================ the codec
def _codec_text(n, seed=1):
    rng = random.Random(seed)
    return tc._fuzz_text(rng, n)


@pytest.mark.parametrize("pieces", [False, True], ids=["mk_bgzf_deflate", "mk_bgzf_deflate_pieces"])
def test_mk_bgzf_deflate_out_cap(mk, pieces):
    lib = mk.load()
    codec = mk.Codec(0)
    for n, block in ((200_000, 0), (70_000, 1000), (5, 0)):
        data = _codec_text(n, seed=n)
        src = np.frombuffer(data, dtype=np.uint8)
        bound = lib.mk_bgzf_deflate_bound(n, block)
        cuts = [0, n // 3, n // 3, n - 1, n]
        parts = [src[a:b].copy() for a, b in zip(cuts, cuts[1:])]
        ptrs = (C.c_void_p * len(parts))(*[_ptr(a) for a in parts])
        sizes = (C.c_uint64 * len(parts))(*[a.size for a in parts])

        def call(cap):
            out = G.HostBuf(np.uint8, bound)
            n_out = C.c_uint64(777)
            if pieces:
                rc = lib.mk_bgzf_deflate_pieces(codec._h, ptrs, sizes, len(parts), block, out.ptr, cap, C.byref(n_out))
            else:
                rc = lib.mk_bgzf_deflate(codec._h, src.ctypes.data, n, block, out.ptr, cap, C.byref(n_out))
            return rc, n_out.value, out

        rc, n_out, out = call(bound)  # exact fit
        assert rc == mk.MK_OK and 28 <= n_out <= bound
        assert out.untouched_from(n_out), "bytes beyond *out_len were written"
        R = out.view(n_out).tobytes()
        assert gzip.decompress(R + mk.bgzf_eof()) == data
        for cap in (bound - 1, 0, bound // 2, n_out):  # (below the bound the call refuses, even where the members would fit)
            if cap >= bound:
                continue
            err0 = G.set_sentinel_error(mk)
            rc, need, out = call(cap)
            assert rc == mk.MK_E_CAPACITY and need == bound, (cap, rc, need, bound)
            assert out.untouched_from(0) and lib.mk_last_error() != err0 and str(bound).encode() in lib.mk_last_error()
            rc, n2, out = call(bound)
            assert rc == mk.MK_OK and out.view(n2).tobytes() == R and out.untouched_from(n2)
    codec.close()


def test_mk_bgzf_inflate_span(mk, codec):
    """members with gaps between their out_off, a span that starts above 0: the call overwrites the span, nothing outside it"""
    lib = mk.load()
    data = _codec_text(300_000, seed=77)
    blob = tc.zlib_bgzf(data, 30_000)
    members, used, tb = mk.bgzf_members(blob)
    assert used == len(blob) and tb == len(data) and len(members) == 10
    mem = members.copy()
    mem["out_off"] = 5000 + members["out_off"] + 1500 * np.arange(len(mem), dtype=np.uint64)  # gaps of 1500 bytes
    mem = mem[[3, 0, 9, 1, 2, 8, 4, 7, 5, 6]].copy()  # (not in order of their output either)
    span_lo, span_hi = 5000, int((mem["out_off"] + mem["isize"]).max())
    src = np.frombuffer(blob, dtype=np.uint8)
    for cap in (span_hi, span_hi + 3000):
        out = G.HostBuf(np.uint8, span_hi + 3000)
        bad = C.c_uint64(7)
        rc = lib.mk_bgzf_inflate(codec._h, src.ctypes.data, src.size, mem.ctypes.data, len(mem), out.ptr, cap, C.byref(bad))
        assert rc == mk.MK_OK, (rc, lib.mk_last_error())
        b = out.view()
        assert np.array_equal(b[:span_lo], G.pattern(out.raw.size)[:span_lo]), "bytes below the span were written"
        assert out.untouched_from(span_hi), "bytes above the span were written"
        for k in range(len(mem)):
            a = int(mem["out_off"][k])
            src_off = int(mem["out_off"][k]) - 5000 - 1500 * int(np.where(members["data_off"] == mem["data_off"][k])[0][0])
            assert b[a:a + int(mem["isize"][k])].tobytes() == data[src_off:src_off + int(mem["isize"][k])], k
    # a member that would end one byte behind out_cap: refused, nothing written
    out = G.HostBuf(np.uint8, span_hi)
    err0 = G.set_sentinel_error(mk)
    rc = lib.mk_bgzf_inflate(codec._h, src.ctypes.data, src.size, mem.ctypes.data, len(mem), out.ptr, span_hi - 1, None)
    assert rc == mk.MK_E_INVALID_ARG and out.untouched_from(0) and lib.mk_last_error() != err0 and b"mk_bgzf_inflate" in lib.mk_last_error()


codec = tc.codec  # the seven inflate kernel variants of test_gpu_codec.py


def test_mk_gzip_text_read_around_the_end(mk):
    lib = mk.load()
    codec = mk.Codec(0)
    text = tc._fastq_text(4000)
    gz = gzip.compress(text, 6)
    src = np.frombuffer(gz, dtype=np.uint8)
    n, taken = C.c_uint64(0), C.c_uint32(0)
    assert lib.mk_gzip_inflate_device(codec._h, src.ctypes.data, src.size, C.byref(n), C.byref(taken)) == mk.MK_OK
    assert taken.value == 1 and n.value == len(text)
    N = len(text)
    for off, ln, ok in ((0, N, True), (N - 1, 1, True), (N - 100, 100, True), (N, 0, True), (17, 1000, True),
                        (N - 1, 2, False), (N, 1, False), (N + 1, 0, False), (0, N + 1, False), (N - 100, 101, False), (1 << 40, 4, False)):
        out = G.HostBuf(np.uint8, ln + 8)
        err0 = G.set_sentinel_error(mk)
        rc = lib.mk_gzip_text_read(codec._h, off, out.ptr, ln)
        if ok:
            assert rc == mk.MK_OK and out.view(ln).tobytes() == text[off:off + ln] and out.untouched_from(ln), (off, ln)
        else:  # a read beyond the text is refused and writes nothing
            assert rc == mk.MK_E_INVALID_ARG and out.untouched_from(0), (off, ln, rc)
            assert lib.mk_last_error() != err0 and str(off).encode() in lib.mk_last_error()
    codec.close()
