"""mk_extract_window_frames without a device: the entry point is declared, exported and bound with the members entry's argument
types; the inputs the device tests build for the cut rule's edges (window_frames_cases.py) are what they claim to be, by
mk_zstd_record_cuts (host code) and by the rule's restatement in Python; and the arguments the call refuses before it looks at a handle
or a device are refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import window_frames_cases as wf
import zstd_out_cases as zo
from merkurio_amd import native as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"\bint mk_extract_window_frames\(mk_matcher \*m, mk_codec \*codec,", hdr)
    L = mk.load()
    assert "mk_extract_window_frames" in mk.EXPORTS and hasattr(L, "mk_extract_window_frames")
    assert list(L.mk_extract_window_frames.argtypes) == list(L.mk_extract_window_members.argtypes) and len(L.mk_extract_window_frames.argtypes) == 17
    assert callable(getattr(mk.Matcher, "extract_window_frames", None))
    # the declaration's argument list is the members entry's, name for name but for the struct's
    args = {n: re.search(r"int %s\((.*?)\);" % n, hdr, re.S).group(1) for n in ("mk_extract_window_members", "mk_extract_window_frames")}
    norm = lambda s: re.sub(r"\s+", " ", s).replace("*frames", "*members")
    assert norm(args["mk_extract_window_frames"]) == norm(args["mk_extract_window_members"])


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("edge", list(wf.EDGES))
def test_the_edge_tables_and_the_rule(edge, delta):
    ends = wf.edge_ends(edge, delta)
    target = wf.EDGES[edge] + delta
    assert ends.count(target) == 1 and ends == sorted(set(ends)) and ends[-1] > 2 * zo.GRID
    cuts = mk.zstd_record_cuts(ends).tolist()
    assert cuts == zo.rule(ends)
    assert (target in cuts) == wf.edge_is_cut(edge, delta)
    if not wf.edge_is_cut(edge, delta) and edge in ("last_snap", "first_raw"):
        assert zo.GRID in cuts  # a raw cut on the grid, inside the record that ends at the target
    assert all(0 < b - a <= zo.TEXT_MAX for a, b in zip(cuts, cuts[1:]))
    # the same ends with every end repeated, as the device's table repeats them for records that are not kept: the same cuts
    assert mk.zstd_record_cuts(np.repeat(np.asarray(ends, dtype=np.uint64), 3)).tolist() == cuts


def test_the_inputs_have_the_written_ends_they_are_built_for():
    ends = wf.edge_ends("first_raw", 0)
    text, keep, written = wf.fasta_with_written_ends(ends)
    recs = wf.fasta_records(text)
    assert len(recs) == len(keep) and [wf.written_fasta(r) for r, k in zip(recs, keep) if k] == written
    assert all((wf.P in r) == k for r, k in zip(recs, keep))
    text, keep, rec = wf.sparse_fastq(3000, 50, "last")
    assert len(text) == 3000 * wf.SPARSE_REC and sum(keep) == 7 and all(i * wf.SPARSE_REC >= len(text) - zo.GRID for i in np.flatnonzero(keep))
    fq = wf.fastq_records(text)
    assert all(wf.written_fastq(r) == rec[i].tobytes() for i, r in enumerate(fq[:200]))
    assert [wf.P in r[1] for r in fq] == keep


def test_arguments_refused_before_a_handle_or_a_device_is_looked_at():
    """a codec is required; a source's `kept` buffer belongs to mk_extract_window; logging with invert names records that are not
    kept.  All three are decided from the arguments alone, so the handles here are blocks of zeroed memory that stand for a matcher
    and a codec: the call must not read them, and on a machine without a device it could do nothing with them anyway."""
    try:
        L = mk.load()
    except OSError as e:
        pytest.skip("the library does not load on this machine: %s" % e)
    fake_m, fake_c = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 16)
    text = np.frombuffer(wf.mixed_fastq(8), dtype=np.uint8)
    out = np.zeros(4096, dtype=np.uint8)

    def call(codec, logging, invert, kept):
        S = (mk.WindowSource * 1)()
        S[0].text, S[0].n_text, S[0].ends_at_record = text.ctypes.data, text.size, 1
        if kept:
            S[0].kept, S[0].kept_cap = out.ctypes.data, 64
        Mm = (mk.WindowMembers * 1)()
        id_end = np.zeros(64, dtype=np.uint64)
        Mm[0].members, Mm[0].members_cap, Mm[0].id_end = out.ctypes.data + 64, 1024, id_end.ctypes.data
        n_rec, status, n_rows, c2, counts = C.c_uint64(), C.c_uint32(), C.c_uint64(), mk.Counters(), np.zeros(4, dtype=np.uint32)
        keep = np.zeros(64, dtype=np.uint8)
        rc = L.mk_extract_window_frames(C.addressof(fake_m), codec, mk.MK_TEXT_FASTQ, 1, S, Mm, int(logging), int(invert), 64, C.byref(n_rec),
                                        keep.ctypes.data, None, 0, C.byref(n_rows), C.byref(c2), counts.ctypes.data, C.byref(status))
        return rc, L.mk_last_error()

    rc, err = call(None, False, False, False)
    assert rc == mk.MK_E_INVALID_ARG and b"mk_extract_window_frames" in err and b"codec" in err
    rc, err = call(C.addressof(fake_c), False, False, True)
    assert rc == mk.MK_E_INVALID_ARG and b"mk_extract_window_frames" in err and b"kept" in err
    rc, err = call(C.addressof(fake_c), True, True, False)
    assert rc == mk.MK_E_INVALID_ARG and b"mk_extract_window_frames" in err and b"invert" in err
    assert not out.any()
