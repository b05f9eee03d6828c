"""mk_xz_stream_* (Codec.unxz_stream): an .xz file decoded on the device window by window -- the plan made when the stream begins,
only the window's compressed span uploaded, the block table rebased to it, the launch's LDS sized by the window's lc + lp, the blocks
launched largest first, two text buffers.  The files are those of tests/xz_windows_cases.py (test_unxz_windows_cpu.py runs the same
chain on the host under the sanitizers); liblzma is the checker, and the host harness says how many windows, blocks and streams there
must be."""
import bz2
import ctypes as C
import gzip

import numpy as np
import pytest

import xz_cases as cases
import xz_windows_cases as wc
import zstd_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def codec(mk):
    c = mk.Codec()
    c.set_xz_spread(1)  # (every file is tried; the rule has tests of its own below)
    yield c
    c.close()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """xz_chain.hpp on the host, built once without the sanitizers: .stream(blob, window, cap, spread) and .plan(blob)"""
    work = tmp_path_factory.mktemp("xz-windows")
    exe = wc.build_harness(work, sanitize=False)

    class H:
        stream = staticmethod(lambda blob, window, cap, spread=1: wc.run_stream(exe, work, blob, window, cap, spread)[0])
        plan = staticmethod(lambda blob: wc.run_plan(exe, work, blob)[1])
    return H


def stream(codec, blob, window, cap):
    parts = list(codec.unxz_stream(blob, window, cap))
    return parts, codec.stream_state, codec.stream_stats


def settings(name, rows):
    """one block per window, a text cap of three median blocks, no bound; the 3000-block file: 64 blocks per window (its blocks have
    64 bytes of text each) and no bound -- never one block per window, which would be 3000 launches"""
    if name == "3000-blocks":
        return ((0, 64 * 64), (0, 0))
    return ((1, 0), (0, wc.median_cap(rows)), (0, 0))


COUNTS = (("windows", "windows"), ("planned_windows", "planned"), ("blocks", "blocks"), ("streams", "streams"), ("consumed_bytes", "consumed"), ("text_bytes", "text"),
          ("largest_block_text", "largest"))


@pytest.mark.parametrize("name", sorted(wc.files()))
def test_files_give_liblzmas_text_and_the_harness_counts(codec, harness, name):
    blob, text = wc.files()[name]
    assert cases.liblzma_says(blob) == text
    rows = harness.plan(blob)
    for window, cap in settings(name, rows):
        parts, state, stats = stream(codec, blob, window, cap)
        print(name, window, cap, stats)
        assert state == 1 and stats["status"] == 0 and b"".join(parts) == text, (name, window, cap, stats)
        assert len(parts) == stats["windows"] == stats["planned_windows"]
        rep = harness.stream(blob, window, cap)
        assert {k: stats[k] for k, _ in COUNTS} == {k: int(rep[h]) for k, h in COUNTS}, (name, window, cap, stats, rep)
        want = wc.windows_of(rows, window, cap)
        assert [len(p) for p in parts] == [sum(rows[k][3] for k in range(f, f + n)) for f, n in want]
        assert stats["peak_device_bytes"] > 0 or not rows
        if name == "3000-blocks":
            assert stats["windows"] == (47 if cap else 1) and codec.stream_windows[0]["blocks"] == (64 if cap else 3000)


def test_a_stream_and_the_one_shot_call_give_the_same_text(codec):
    for name in ("40-blocks", "mixed-checks", "streams-without-blocks", "far-block-second", "lclp-0-then-4", "ascending-blocks"):
        blob, text = wc.files()[name]
        taken, whole, n_blocks = codec.unxz(blob)
        info = codec.unxz_info()
        parts, state, stats = stream(codec, blob, 1, 0)
        assert taken is True and state == 1 and whole == b"".join(parts) == text and stats["blocks"] == n_blocks, (name, stats)
        parts, state, stats = stream(codec, blob, 0, 0)
        assert state == 1 and parts == [text] and (stats["blocks"], stats["streams"], stats["largest_block_text"]) == (info[0], info[1], info[3]), (name, stats, info)
        assert codec.unxz(blob)[:2] == (True, text)  # and the one-shot call after a stream


@pytest.mark.parametrize("block", [0, 17, 39])
@pytest.mark.parametrize("what", ["payload", "check"])
def test_a_damaged_block_hands_back_behind_the_windows_in_front_of_it(codec, harness, block, what):
    blob, text = cases.valid()["40-blocks"]
    rows = harness.plan(blob)
    r = rows[block]
    bad = cases.flip(blob, (r[0] + r[1] // 2 if what == "payload" else r[4] + 3) * 8 + 2)
    assert cases.liblzma_says(bad) is None
    for window in (1, 8 * wc.mean_span(rows)):
        before = [(f, n) for f, n in wc.windows_of(rows, window, 0) if f + n <= block]
        delivered = sum(rows[k][3] for f, n in before for k in range(f, f + n))
        parts, state, stats = stream(codec, bad, window, 0)
        rep = harness.stream(bad, window, 0)
        assert state == 2 and stats["status"] == int(rep["status"]) and -32 <= stats["status"] <= -20, (block, what, window, stats, rep)
        assert b"".join(parts) == text[:delivered] and len(parts) == stats["windows"] == len(before) and stats["text_bytes"] == delivered
    # the handle is none the worse for it
    assert b"".join(codec.unxz_stream(blob, 1)) == text and codec.stream_state == 1


def test_refusals_at_begin_leave_no_stream_open(mk, codec, harness):
    L, h = codec._L, codec._h
    n, state = C.c_uint64(0), C.c_uint32(0)
    good, text = wc.files()["fastq-blocks-mid-record"]

    def refused(blob, status, window=0, cap=0):
        assert list(codec.unxz_stream(blob, window, cap)) == [] and codec.stream_state == 2
        assert codec.stream_stats["status"] == status and codec.stream_stats["windows"] == 0, codec.stream_stats
        assert codec.unxz_stream_info()["status"] == status  # (without an open stream: the last one's figures)
        assert L.mk_xz_stream_next(h, C.byref(n), C.byref(state)) == mk.MK_E_INVALID_ARG  # no stream
        assert codec.unxz(good)[:2] == (True, text)  # a one-shot call works right after
    for name in ("flip-stream-header", "flip-index", "flip-footer", "trailing-bytes", "cut-payload-middle", "block-padding-not-zero"):
        blob = cases.damaged()[name]
        refused(blob, int(harness.stream(blob, 0, 0)["status"]))
    for name, (blob, _, status) in sorted(cases.handed_back().items()):
        refused(blob, status)
    for junk in (b"", b"\xfd7zXZ", b"not an xz file at all\n" * 9, gzip.compress(b"ACGT\n" * 99)):
        refused(junk, int(harness.stream(junk, 0, 0)["status"]))
    refused(cases.blocks_of([1000, 3000, 1000])[0], wc.XZ_BLOCK_OVER_CAP, 0, 2999)
    # the spread rule sums the windows' largest blocks
    two = cases.blocks_of([2000, 2000])
    codec.set_xz_spread(2)
    try:
        refused(two[0], cases.XZ_SPREAD, 1, 0)
        assert b"".join(codec.unxz_stream(two[0], 0, 0)) == two[1] and codec.stream_state == 1 and codec.stream_stats["windows"] == 1
        codec.set_xz_spread(0)  # the default, 107: a file of eleven blocks is liblzma's
        assert list(codec.unxz_stream(good, 0, 0)) == [] and codec.stream_state == 2 and codec.stream_stats["status"] == cases.XZ_SPREAD
    finally:
        codec.set_xz_spread(1)


def test_guards(mk, codec):
    blob, text = wc.files()["fastq-blocks-mid-record"]
    L, h = codec._L, codec._h
    src = np.frombuffer(blob, dtype=np.uint8)
    gz = np.frombuffer(gzip.compress(b"ACGT\n" * 4000), dtype=np.uint8)
    bz = np.frombuffer(bz2.compress(cases.fastq(400), 1), dtype=np.uint8)
    zs = np.frombuffer(zstd_cases.valid()["fastq-l3-checksum"][0], dtype=np.uint8)
    taken, n, state, blocks = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    INVALID = mk.MK_E_INVALID_ARG
    assert L.mk_xz_stream_next(h, C.byref(n), C.byref(state)) == INVALID  # no stream
    assert L.mk_xz_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_xz_inflate_device(h, src.ctypes.data, src.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert b"mk_xz_stream_end" in L.mk_last_error()
    assert L.mk_zstd_inflate_device(h, zs.ctypes.data, zs.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_bzip2_inflate_device(h, bz.ctypes.data, bz.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken)) == INVALID
    assert L.mk_gzip_members_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_stream_begin(h, gz.ctypes.data, gz.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_bzip2_stream_begin(h, bz.ctypes.data, bz.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_zstd_stream_begin(h, zs.ctypes.data, zs.size, 1, C.byref(taken)) == INVALID
    assert L.mk_xz_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == INVALID
    assert L.mk_xz_stream_next(h, C.byref(n), C.byref(state)) == 0 and state.value == 0 and n.value == 1000  # the stream is untouched by them
    assert L.mk_xz_stream_end(h) == 0
    # after _end they work again
    assert codec.unxz(blob)[:2] == (True, text)
    assert L.mk_gzip_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken)) == 0
    assert L.mk_bzip2_stream_begin(h, bz.ctypes.data, bz.size, 8192, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_xz_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == INVALID  # the reverse: a bzip2 stream open
    assert L.mk_bzip2_stream_end(h) == 0
    assert L.mk_zstd_stream_begin(h, zs.ctypes.data, zs.size, 1, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_zstd_stream_end(h) == 0
    # mk_gzip_text_release ends an xz stream as _end does
    assert L.mk_xz_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_gzip_text_release(h) == 0
    assert L.mk_xz_stream_next(h, C.byref(n), C.byref(state)) == INVALID
    assert b"".join(codec.unxz_stream(blob, 1)) == text and codec.stream_state == 1


def test_window_w_is_still_there_after_window_w_plus_1(codec):
    """read through the pointer of mk_gzip_text_device with a device-to-host copy of this test's own"""
    blob, text = wc.files()["fastq-blocks-mid-record"]
    L = codec._L
    src = np.frombuffer(blob, dtype=np.uint8)
    taken, n, state = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    assert L.mk_xz_stream_begin(codec._h, src.ctypes.data, src.size, 1, C.byref(taken)) == 0 and taken.value == 1
    with open("/proc/self/maps") as maps:  # (the HIP runtime the library itself runs on: the one this process has mapped)
        hip = C.CDLL(next(ln.split()[-1] for ln in maps if "libamdhip64" in ln))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def copy_out(ptr, size):
        out = np.empty(size, dtype=np.uint8)
        assert hip.hipMemcpy(out.ctypes.data, ptr, size, 2) == 0 and hip.hipDeviceSynchronize() == 0  # (2 = device to host)
        return out.tobytes()
    held, at, checked = [], 0, 0
    try:
        while True:
            assert L.mk_xz_stream_next(codec._h, C.byref(n), C.byref(state)) == 0
            if state.value != 0:
                break
            m = C.c_uint64(0)
            ptr = L.mk_gzip_text_device(codec._h, C.byref(m))
            assert m.value == n.value and copy_out(ptr, n.value) == text[at:at + n.value]
            if held:  # the window before this one, after this one was produced
                p_ptr, p_at, p_n = held[-1]
                assert p_ptr != ptr and copy_out(p_ptr, p_n) == text[p_at:p_at + p_n]
                checked += 1
            held.append((ptr, at, n.value))
            at += n.value
    finally:
        assert L.mk_xz_stream_end(codec._h) == 0
    assert state.value == 1 and at == len(text) and checked >= 9


def test_a_text_cap_below_the_buffers_of_the_stream_before_changes_nothing(codec):
    big, big_text = wc.files()["two-streams-pad-8"]
    assert list(codec.unxz_stream(big, 0, 0)) == [big_text]  # one window of 70 000 bytes
    blob, text = wc.files()["fastq-blocks-mid-record"]
    for cap in (4097, 5000, 1 << 20):
        parts = list(codec.unxz_stream(blob, 0, cap))
        assert b"".join(parts) == text and codec.stream_state == 1 and all(len(p) <= cap for p in parts), cap
    assert list(codec.unxz_stream(big, 0, 0)) == [big_text]
