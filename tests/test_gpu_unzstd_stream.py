"""mk_zstd_stream_* (Codec.unzstd_stream): a .zst file decoded on the device window by window -- the resumable walk, the carried
tables as a prelude in front of a window's compressed bytes, the history copied to the front of the next text buffer and read as
settled bytes by the execute step, the rounds over the window only, the checksum hashed window by window.  The files are the
seam-sensitive ones of tests/zstd_windows_cases.py (test_unzstd_windows_cpu.py runs the same chain on the host under the sanitizers);
libzstd is the checker, and the host harness says how many windows, frames, blocks and rounds there must be."""
import bz2
import ctypes as C

import numpy as np
import pytest

import zstd_cases as cases
import zstd_windows_cases as wc

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
    yield c
    c.close()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """report(file, window, cap) as zstd_chain.hpp makes it on the host, built once without the sanitizers"""
    work = tmp_path_factory.mktemp("zstd-windows")
    exe = wc.build_harness(work, sanitize=False)
    return lambda blob, window, cap: wc.run_harness(exe, work, blob, "stream", window, cap)[0]


def stream(codec, blob, window, cap):
    parts = list(codec.unzstd_stream(blob, window, cap))
    return parts, codec.stream_state, codec.stream_stats


# one block per window; a text cap of three blocks
SETTINGS = ((1, 0), (wc.WHOLE, 3 * wc.BLOCK))
COUNTS = (("windows", "windows"), ("frames", "frames"), ("blocks", "blocks"), ("consumed_bytes", "consumed"), ("text_bytes", "text"), ("rounds", "rounds"),
          ("max_history", "max-history"))


@pytest.mark.parametrize("name", sorted(wc.seam_files()))
def test_seam_files_give_libzstds_text_and_the_harness_counts(codec, harness, name):
    blob, text = wc.seam_files()[name]
    assert cases.libzstd_says(blob) == text
    for window, cap in SETTINGS:
        parts, state, stats = stream(codec, blob, window, cap)
        print(name, window, cap, stats)
        assert state == 1 and b"".join(parts) == text, (name, window, cap, stats)
        rep = harness(blob, window, cap)
        assert {k: stats[k] for k, _ in COUNTS} == {k: int(rep[h]) for k, h in COUNTS}, (name, window, cap, stats, rep)
        assert len(parts) == stats["windows"] and stats["peak_device_bytes"] > 0


def test_a_stream_and_the_one_shot_call_give_the_same_text(codec):
    for name in ("fastq-l3-checksum", "three-frames", "windows-fastq-wlog17-l19", "windows-matches-into-history-only"):
        blob, text = wc.seam_files()[name]
        taken, whole, n_blocks = codec.unzstd(blob)
        info = codec.unzstd_info()  # (of the one-shot call: a stream's begin clears them)
        parts, state, stats = stream(codec, blob, 1, 0)
        assert taken is True and state == 1 and whole == b"".join(parts) == text and stats["blocks"] == n_blocks, (name, stats)
        # and in one window the stream is the one-shot call: its blocks, frames and rounds
        parts, state, stats = stream(codec, blob, 0, 0)
        assert state == 1 and parts == [text] and (stats["blocks"], stats["frames"], stats["rounds"]) == info[:3], (name, stats, info)


def test_matches_into_the_history_are_read_as_bytes_and_wait_for_no_round(codec):
    """every 128 KiB block is the first one again under a 256 KiB frame window: at a block per window, every window behind the first
    has matches into its history only.  The execute step copies them as settled bytes, so no window runs a round of resolution --
    it would run one, as the whole file in one window does, if the settled bound were ignored"""
    blob, text = wc.seam_files()["windows-matches-into-history-only"]
    parts, state, stats = stream(codec, blob, 1, 0)
    assert state == 1 and b"".join(parts) == text and stats["windows"] == 4
    assert [w["rounds"] for w in codec.stream_windows[:4]] == [0, 0, 0, 0], codec.stream_windows
    assert stats["max_history"] >= wc.BLOCK
    parts, state, stats = stream(codec, blob, 0, 0)
    assert state == 1 and parts == [text] and stats["rounds"] >= 1, stats


def test_window_w_is_still_there_after_window_w_plus_1(codec):
    """read through the pointer of mk_gzip_text_device with a device-to-host copy of this test's own"""
    blob, text = wc.seam_files()["fastq-l3-checksum"]
    L = codec._L
    src = np.frombuffer(blob, dtype=np.uint8)
    taken, n, state = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    assert L.mk_zstd_stream_begin(codec._h, src.ctypes.data, src.size, 1, C.byref(taken)) == 0 and taken.value == 1
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
            assert L.mk_zstd_stream_next(codec._h, C.byref(n), C.byref(state)) == 0
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
        assert L.mk_zstd_stream_end(codec._h) == 0
    assert state.value == 1 and at == len(text) and checked >= 3


def test_damaged_files_are_handed_back_behind_a_prefix(codec):
    fq = cases.fastq(300)[:60000]
    for name, blob in sorted(cases.damaged().items()):
        parts, state, stats = stream(codec, blob, 1, 0)
        assert state == 2, (name, stats)
        assert fq.startswith(b"".join(parts)) or name.startswith("crafted-") and not parts, name
    blob, text = cases.valid()["fastq-l3-checksum"]
    bad = cases.flip(blob, (len(blob) - 40) * 8 + 3)
    parts, state, stats = stream(codec, bad, 1, 0)
    assert state == 2 and stats["windows"] >= 3 and text.startswith(b"".join(parts)) and len(b"".join(parts)) >= 3 * wc.BLOCK, stats
    # the handle is none the worse for it
    assert b"".join(codec.unzstd_stream(blob, 1)) == text and codec.stream_state == 1


def test_guards(mk, codec):
    blob, text = cases.valid()["fastq-l3-checksum"]
    L, h = codec._L, codec._h
    src = np.frombuffer(blob, dtype=np.uint8)
    gz = np.frombuffer(__import__("gzip").compress(b"ACGT\n" * 4000), dtype=np.uint8)
    bz = np.frombuffer(bz2.compress(cases.fastq(400), 1), dtype=np.uint8)
    taken, n, state, blocks = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    INVALID = mk.MK_E_INVALID_ARG
    assert L.mk_zstd_stream_next(h, C.byref(n), C.byref(state)) == INVALID  # no stream
    assert L.mk_zstd_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_zstd_inflate_device(h, src.ctypes.data, src.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_bzip2_inflate_device(h, bz.ctypes.data, bz.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken)) == INVALID
    assert L.mk_gzip_members_inflate_device(h, gz.ctypes.data, gz.size, C.byref(n), C.byref(taken), C.byref(blocks)) == INVALID
    assert L.mk_gzip_stream_begin(h, gz.ctypes.data, gz.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_bzip2_stream_begin(h, bz.ctypes.data, bz.size, 8192, C.byref(taken)) == INVALID
    assert L.mk_zstd_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == INVALID
    assert L.mk_zstd_stream_next(h, C.byref(n), C.byref(state)) == 0 and state.value == 0 and n.value == wc.BLOCK  # the stream is untouched by them
    assert L.mk_zstd_stream_end(h) == 0
    assert codec.unzstd(blob)[:2] == (True, text)  # after _end the one-shot call works
    # the reverse: a bzip2 stream open
    assert L.mk_bzip2_stream_begin(h, bz.ctypes.data, bz.size, 8192, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_zstd_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == INVALID
    assert L.mk_bzip2_stream_end(h) == 0
    # mk_gzip_text_release ends a zstd stream as _end does
    assert L.mk_zstd_stream_begin(h, src.ctypes.data, src.size, 1, C.byref(taken)) == 0 and taken.value == 1
    assert L.mk_gzip_text_release(h) == 0
    assert L.mk_zstd_stream_next(h, C.byref(n), C.byref(state)) == INVALID
    # no frame in front: not taken, and the handle lives on
    for junk in (b"", b"\x28\xb5", b"not a zstd file at all\n" * 9, bytes(gz), bytes(bz)):
        assert list(codec.unzstd_stream(junk, 4096)) == [] and codec.stream_state == 2 and codec.stream_stats is None
    assert b"".join(codec.unzstd_stream(blob, 8192)) == text and codec.stream_state == 1
