"""What a handle did before must not change what it answers.

mk_matcher carries state from call to call -- the hit density it last saw, the record shape, the bound of the last scan's record
numbers, per-wave flag lists and counts sized for the last grid, the coarse record index, the cached reference names -- and
mk_codec keeps a resident text, stream state, pass limits and a forced kernel.  Each sequence below runs on ONE long-lived handle;
after every step the step's result is compared with a fresh handle's and with the oracle's (zlib's / bz2's for the codec), all
three.  The scan batches are those of tests/scan_edge_cases.py (checked on the CPU by tests/test_scan_edge_cases_cpu.py)."""
import bz2
import gzip
import itertools
import random
import zlib

import numpy as np
import pytest

import guarded as G
import oracle_binding as ob
import scan_edge_cases as sc
import test_gpu_bam_sam_window as bs
import test_gpu_order as to
import test_gpu_sam_bam_window as sb
from tag_windows import patterns31
from test_gpu_scan_wave_capacity import Batch

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


_ORACLE = {}


def oracle(name):
    """(flags, tuples in emission order, per-pattern counts) of a case by the oracle's BNDMq loop"""
    if name not in _ORACLE:
        c = sc.case(name)
        om = ob.Matcher(c.patterns, False, 0, False)
        _, rows, counters, found = ob.tag_records(om, c.records, logging=True)
        _ORACLE[name] = ([bool(f) for f in found], [(r, p, pos) for (_, r, p, pos) in rows], counters["pattern_hit_counts"])
    return _ORACLE[name]


def answers(handle, call):
    return call(handle)


def same_as_fresh_and_oracle(mk, handle, make_fresh, call, want, what):
    """the helper of every sequence: the long-lived handle's answer, a fresh handle's, the oracle's -- all three compared"""
    got = answers(handle, call)
    fresh = make_fresh()
    ref = answers(fresh, call)
    fresh.close()
    assert ref == want, f"{what}: a fresh handle differs from the oracle"
    assert got == want, f"{what}: the handle's history changed its answer"
    assert got == ref
    return got


def scan_call(mk, torch, batch, mode, density=None, records="offsets"):
    """-> call(m) -> (flags, tuples in emission order or None, per-pattern counters or None)"""
    lib = mk.load()
    T = len(batch.case.tuples)

    def call(m):
        if mode == "any":
            f, nh, _ = batch.scan(m, mk.MK_MODE_ANY, density, records)
            assert nh == 0
            return f, None, None
        hits = G.DeviceBuf(torch, mk.HIT_DTYPE, T)
        f, nh, cnt = batch.scan(m, mk.MK_MODE_HITS, density, records, hits=hits, cap=T, counters=(mode == "count"))
        assert nh == T
        st = torch.cuda.current_stream().cuda_stream
        assert lib.mk_order_hits_device(m.handle, hits.ptr, T, st) == mk.MK_OK, lib.mk_last_error()
        torch.cuda.synchronize()
        assert hits.guard_intact()
        h = hits.view(T)
        return f, list(zip(h["rec"].tolist(), h["pat"].tolist(), h["pos"].tolist())), (cnt[:len(batch.case.patterns)] if cnt else None)
    return call


def want_of(name, mode):
    flags, tuples, counts = oracle(name)
    return (flags, None, None) if mode == "any" else (flags, tuples, list(counts) if mode == "count" else None)


# ---------------------------------------------------------------------------------------------------- grid shrink and growth
@pytest.mark.parametrize("options", [None, dict(force_global_filter=True)], ids=["lds", "global-filter"])
def test_grid_shrinks_and_grows(mk, torch, options):
    """2 MiB (many waves, every list partly filled), 20 KiB (one workgroup), 2 MiB again; the caller's flag buffer is 64 bytes longer
    than n_rec and full of 0xA5: a stale list entry of the large launch would set a byte beyond the small batch's records"""
    lib = mk.load()
    m = mk.Matcher(sc.PATTERNS, options=options)
    grids = []
    for step, key in enumerate(("big", "small", "big")):
        name = sc.HISTORY_CASES[key]
        b = Batch(mk, torch, sc.case(name))

        def call(h):
            h.hint_hit_density(0)
            assert lib.mk_matcher_set_fixed_record_length(h.handle, 8) == 0
            flags = torch.full((b.n_rec + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            nh = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            st = torch.cuda.current_stream().cuda_stream
            rc = lib.mk_scan_device(h.handle, b.d_seq.data_ptr(), b.n_bytes, None, b.n_rec, mk.MK_MODE_ANY, flags.data_ptr(), None, 0, nh.data_ptr(), None, st)
            assert rc == mk.MK_OK, lib.mk_last_error()
            torch.cuda.synchronize()
            assert lib.mk_matcher_check_device(h.handle, st) == mk.MK_OK
            assert not h.kernel_name.endswith("plain>")
            f = flags.cpu().numpy()
            behind = f[(b.n_rec + 3) // 4 * 4:]
            assert len(behind) >= 60 and (behind == 0xA5).all(), f"step {step}: bytes behind the flags of {b.n_rec} records were written"
            return f[:b.n_rec].astype(bool).tolist()
        same_as_fresh_and_oracle(mk, m, lambda: mk.Matcher(sc.PATTERNS, options=options), call, oracle(name)[0], f"step {step} ({key})")
        grids.append(m.launch_info()["grid_blocks"])
    assert grids[0] == grids[2] > grids[1] == 1, grids
    m.close()


# ---------------------------------------------------------------------------------------------------- mode order
def test_modes_in_every_order(mk, torch):
    """tuples, flags only, tuples with counters on the same text in each of the six orders, the first step of each once more at
    its end"""
    name = sc.HISTORY_CASES["tuples"]
    b = Batch(mk, torch, sc.case(name))
    m = mk.Matcher(sc.TUPLE_PATTERNS)
    for density in (0, 1000):
        for perm in itertools.permutations(("hits", "any", "count")):
            for mode in perm + (perm[0],):
                same_as_fresh_and_oracle(mk, m, lambda: mk.Matcher(sc.TUPLE_PATTERNS), scan_call(mk, torch, b, mode, density, "fixed"),
                                         want_of(name, mode), f"{perm}: {mode}, density {density}")
    m.close()


# ---------------------------------------------------------------------------------------------------- observed density
@pytest.mark.parametrize("mode", ["any", "hits"])
def test_density_observed_by_mk_scan_batch(mk, mode):
    """every record hits, none does, 12 % do, every record hits: mk_scan_batch sets the density for the next batch from what it
    saw, so the sequence crosses from the sparse flavour to the dense one and back; no hint is given anywhere"""
    m = mk.Matcher(sc.PATTERNS)
    names = []
    for key in ("dense", "none", "12pct", "dense"):
        name = sc.HISTORY_CASES[key]
        c = sc.case(name)

        def call(h):
            flags, hits = h.scan(c.records, mk.MK_MODE_ANY if mode == "any" else mk.MK_MODE_HITS, hits_cap=max(1, len(c.tuples)))  # (one scan: no retry)
            return flags.tolist(), (list(zip(hits["rec"].tolist(), hits["pat"].tolist(), hits["pos"].tolist())) if mode == "hits" else None), None
        same_as_fresh_and_oracle(mk, m, lambda: mk.Matcher(sc.PATTERNS), call, want_of(name, mode), f"{key}")
        names.append(m.kernel_name)
    flavours = {n.endswith("plain>") for n in names}
    assert flavours == {True, False}, f"the sequence never crossed the switch between the flavours: {names}"
    assert not names[0].endswith("plain>") and names[1].endswith("plain>") and not names[2].endswith("plain>"), names
    m.close()


# ---------------------------------------------------------------------------------------------------- record shapes
def test_record_shapes_in_turn(mk, torch):
    m = mk.Matcher(sc.PATTERNS)
    fresh = lambda: mk.Matcher(sc.PATTERNS)  # noqa: E731
    # host batches: mk_scan_batch reads the shape off the offsets -- equal lengths, ragged, equal lengths of another length
    for key in ("fixed8", "ragged", "12pct", "ragged", "fixed8"):
        name = sc.HISTORY_CASES[key]
        c = sc.case(name)
        for mode in ("any", "hits"):
            def call(h):
                flags, hits = h.scan(c.records, mk.MK_MODE_ANY if mode == "any" else mk.MK_MODE_HITS, hits_cap=max(1, len(c.tuples)))  # (one scan: no retry)
                return flags.tolist(), (list(zip(hits["rec"].tolist(), hits["pat"].tolist(), hits["pos"].tolist())) if mode == "hits" else None), None
            same_as_fresh_and_oracle(mk, m, fresh, call, want_of(name, mode), f"mk_scan_batch of {key}, {mode}")
    # device scans: a fixed length set, cleared, the ragged hint given and taken back
    b8, b12, br = (Batch(mk, torch, sc.case(sc.HISTORY_CASES[k])) for k in ("fixed8", "12pct", "ragged"))
    steps = [(b8, "fixed"), (b8, "offsets"), (br, "index"), (b12, "fixed"), (br, "offsets"), (b8, "index"), (b12, "offsets"), (br, "index"), (b8, "fixed")]
    for i, (b, records) in enumerate(steps):
        for mode in ("any", "count"):
            same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, b, mode, 0, records), want_of(b.case.name, mode),
                                     f"device step {i}: {b.case.name} as {records}, {mode}")
    # the coarse record index grows and shrinks
    for key in ("ragged-30k", "ragged-300k", "ragged-30k"):
        b = Batch(mk, torch, sc.case(sc.HISTORY_CASES[key]))
        for mode in ("any", "hits"):
            same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, b, mode, 0, "index"), want_of(b.case.name, mode), f"record index: {key}, {mode}")
    m.close()


# ---------------------------------------------------------------------------------------------------- the ordering bound
def test_ordering_bound_stale_in_both_directions(mk, torch):
    """mk_order_hits_device bins by the record count of the handle's last scan: tuples of a larger record range after a small scan,
    and of a small one after a large scan, must come out in order all the same"""
    m = mk.Matcher(sc.TUPLE_PATTERNS)
    fresh = lambda: mk.Matcher(sc.TUPLE_PATTERNS)  # noqa: E731
    b1000, b10 = (Batch(mk, torch, sc.case(sc.HISTORY_CASES[k])) for k in ("order-1000", "order-10"))
    assert b1000.n_rec == 1000 and b10.n_rec == 10
    rnd = np.random.default_rng(5)
    n = 20000
    far = np.zeros(n, dtype=mk.HIT_DTYPE)
    far["rec"] = rnd.integers(0, 10**6, n)
    far["rec"][:3] = (10**6 - 1, 0, 10**6 - 1)
    far["pat"] = rnd.integers(0, len(sc.TUPLE_PATTERNS), n)
    far["pos"] = rnd.integers(0, 140, n)
    far = rnd.permutation(np.unique(far))
    plen = np.array([len(p) for p in sc.TUPLE_PATTERNS], dtype=np.int64)
    want_far = to._expected(far, False, plen)
    near = np.array(sc.case(sc.HISTORY_CASES["order-10"]).tuples, dtype=np.int64)
    small = np.zeros(len(near), dtype=mk.HIT_DTYPE)
    small["rec"], small["pat"], small["pos"] = near[:, 0], near[:, 1], near[:, 2]
    small = small[::-1].copy()
    big = Batch(mk, torch, sc.case(sc.HISTORY_CASES["big"]))
    same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, b1000, "hits", 0, "fixed"), want_of(b1000.case.name, "hits"), "1000 records")
    same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, b10, "hits", 0, "fixed"), want_of(b10.case.name, "hits"), "10 records")
    assert np.array_equal(to._order_on_device(mk, m, far), want_far), "tuples of 10^6 records after a scan of 10"
    big.scan(m, mk.MK_MODE_ANY, 0, "fixed")
    assert np.array_equal(to._order_on_device(mk, m, small), to._expected(small, False, plen)), "tuples of 10 records after a scan of 262144"
    assert np.array_equal(to._order_on_device(mk, m, far), want_far)
    same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, b10, "hits", 0, "fixed"), want_of(b10.case.name, "hits"), "10 records again")
    m.close()


# ---------------------------------------------------------------------------------------------------- after a refusal
def test_after_a_refusal(mk, torch):
    lib = mk.load()
    m = mk.Matcher(sc.TUPLE_PATTERNS)
    fresh = lambda: mk.Matcher(sc.TUPLE_PATTERNS)  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    tup, other = sc.case(sc.HISTORY_CASES["tuples"]), Batch(mk, torch, sc.case(sc.HISTORY_CASES["order-1000"]))
    for density in (0, 1000):
        m.hint_hit_density(density)
        with pytest.raises(mk.MerkurioError) as e:  # MK_E_CAPACITY: a tuple scan with room for three
            m.scan(tup.records, mk.MK_MODE_HITS, hits_cap=3)
        assert e.value.code == mk.MK_E_CAPACITY
        assert lib.mk_matcher_check_device(m.handle, st) == mk.MK_OK
        for mode in ("any", "count"):
            same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, other, mode, None, "offsets"), want_of(other.case.name, mode),
                                     f"after MK_E_CAPACITY, {mode}")
        # MK_E_INVALID_ARG: the byte count does not fit the fixed record length
        assert lib.mk_matcher_set_fixed_record_length(m.handle, 7) == 0
        flags = torch.zeros(other.n_rec + 8, dtype=torch.uint8, device="cuda:0")
        nh = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        rc = lib.mk_scan_device(m.handle, other.d_seq.data_ptr(), other.n_bytes, None, other.n_rec, mk.MK_MODE_ANY, flags.data_ptr(), None, 0, nh.data_ptr(), None, st)
        assert rc == mk.MK_E_INVALID_ARG
        torch.cuda.synchronize()
        assert lib.mk_matcher_check_device(m.handle, st) == mk.MK_OK
        for mode in ("hits", "any"):
            same_as_fresh_and_oracle(mk, m, fresh, scan_call(mk, torch, other, mode, None, "fixed"), want_of(other.case.name, mode),
                                     f"after MK_E_INVALID_ARG, {mode}")
    m.close()


# ---------------------------------------------------------------------------------------------------- the reference-name cache
NAME_TABLES = [([b"chr1", b"chr2"], [b"chr2", b"chr1"]), ([b"chrA"], [b"chrB"])]


@pytest.mark.parametrize("tables", NAME_TABLES, ids=["swapped", "renamed"])
def test_reference_names_follow_the_call_sam_to_bam(mk, tables):
    """two name tables of the same count and the same total length: the second window must not be encoded with the first one's"""
    a, b = tables
    rnd = random.Random(8)
    pats = patterns31(mk)
    text = b"".join(sb.sam_line(rnd, i, pats, refs=a + b) for i in range(400))
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    seen = []
    for refs in (a, b, a, b, b, a):
        keep, rows, c, out, n_rec = sb.expected(om, pats, text, b"km", True, False, False, refs=refs)
        r = m.tag_sam_bam_window(codec, b"", text, last=True, refs=refs, logging=True)
        sb.check([r], keep, rows, c, out, n_rec, True)
        f = mk.Matcher(pats, device=0)
        r2 = f.tag_sam_bam_window(codec, b"", text, last=True, refs=refs, logging=True)
        f.close()
        assert sb.inflate(r["out"]) == sb.inflate(r2["out"]) == out
        seen.append(out)
    assert seen[0] != seen[1] and seen[0] == seen[2]  # the tables do encode the lines differently
    codec.close()
    m.close()


@pytest.mark.parametrize("tables", NAME_TABLES, ids=["swapped", "renamed"])
def test_reference_names_follow_the_call_bam_to_sam(mk, tables):
    a, b = tables
    rnd = random.Random(9)
    pats = patterns31(mk, 100)
    recs, existing = bs.make(rnd, pats, 300, lens=(0, 1, 31, 150))
    text, blob, members = bs.window(mk, recs)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    om = ob.Matcher(pats, True, 0, False)
    seen = []
    for refs in (a, b, a, b, b, a):
        keep, rows, c, out = bs.expected(om, pats, recs, refs, b"km", True, False, False, existing)
        r = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=refs, logging=True)
        bs.check(r, keep, rows, c, out, True)
        f = mk.Matcher(pats, device=0)
        r2 = f.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=refs, logging=True)
        f.close()
        assert r2["out"] == r["out"] == out
        seen.append(out)
    assert seen[0] != seen[1] and seen[0] == seen[2]
    codec.close()
    m.close()


# ---------------------------------------------------------------------------------------------------- the codec
def _fastq(n, seed):
    rnd = random.Random(seed)
    recs = [b"@r%d\n%s\n+\n%s\n" % (i, bytes(rnd.choice(b"ACGT") for _ in range(100)), bytes(rnd.choice(b"FFFF:,#") for _ in range(100))) for i in range(n)]
    return b"".join(recs), np.cumsum([len(r) for r in recs]).astype(np.uint64)


def test_codec_inflate_after_a_corrupt_member(mk):
    """good members, a member with one payload bit flipped (MK_E_CORRUPT), the good ones again -- under every forced inflate kernel"""
    text, _ = _fastq(1000, 1)
    assert 100 << 10 <= len(text) <= 300 << 10
    codec = mk.Codec(0)
    blob = codec.deflate(text)
    assert gzip.decompress(blob + mk.bgzf_eof()) == text
    members, used, _ = mk.bgzf_members(blob)
    assert used == len(blob) and len(members) >= 2
    bad = bytearray(blob)
    bad[int(members["data_off"][1]) + 200] ^= 0x10  # inside the second member's DEFLATE payload
    with pytest.raises((zlib.error, OSError, EOFError)):
        gzip.decompress(bytes(bad) + mk.bgzf_eof())
    for which in (1, 2, 3, 4, 5, 6, 0):
        codec.set_inflate_kernel(which)
        assert codec.inflate(blob) == text, which
        with pytest.raises(mk.MerkurioError) as e:
            codec.inflate(bytes(bad))
        assert e.value.code == mk.MK_E_CORRUPT, which
        assert codec.inflate(blob) == text, f"kernel {which}: after the corrupt member"
        fresh = mk.Codec(0)
        fresh.set_inflate_kernel(which)
        assert fresh.inflate(blob) == text
        fresh.close()
    codec.close()


def test_codec_calls_in_turn(mk):
    """gunzip, a gzip stream left after its first window, bunzip2, a bzip2 stream, deflate_records, the first gunzip again, with the pass
    limits, the gzip chunk and the bzip2 pass blocks set and restored in between; zlib / bz2 and a fresh codec say what is right"""
    text, rec_end = _fastq(1000, 2)
    text2, _ = _fastq(1200, 3)
    gz, gz2, bz = gzip.compress(text, 6), gzip.compress(text2, 6), bz2.compress(text2, 1)
    codec = mk.Codec(0)

    def gunzip_first():
        got = codec.gunzip(gz)
        f = mk.Codec(0)
        ref = f.gunzip(gz)
        f.close()
        assert got == ref == zlib.decompress(gz, 31), "gunzip"

    def deflate_records():
        got = codec.deflate_records(text, rec_end)
        f = mk.Codec(0)
        ref = f.deflate_records(text, rec_end)
        f.close()
        assert got == ref and gzip.decompress(got + mk.bgzf_eof()) == text, "deflate_records"

    for round_ in range(2):
        gunzip_first()
        it = codec.gunzip_stream(gz2, window=32768)
        first = next(it)
        it.close()  # mk_gzip_stream_end after the first window
        assert len(first) > 0 and text2.startswith(first) and len(first) < len(text2)
        codec.set_pass_limits(3, 65536)
        deflate_records()
        assert codec.inflate(codec.deflate(text)) == text
        codec.set_pass_limits(0, 0)
        taken, out, blocks = codec.bunzip2(bz)
        assert taken and out == bz2.decompress(bz) and blocks >= 2
        codec.set_bzip2_pass_blocks(1)
        taken, out, _ = codec.bunzip2(bz)
        assert taken and out == text2
        codec.set_bzip2_pass_blocks(0)
        assert b"".join(codec.bunzip2_stream(bz, window=40000)) == text2 and codec.stream_state == 1
        codec.set_gzip_chunk(16384)
        gunzip_first()
        codec.set_gzip_chunk(0)
        assert b"".join(codec.gunzip_stream(gz2, window=32768)) == text2 and codec.stream_state == 1
        deflate_records()
        gunzip_first()
    codec.close()
