"""mk_tag_sam_window (`tag` on a window of SAM text that stays on the device) is an addition to ABI v7: the header declares it, the
Python binding lists it, the built library exports it, and the version number has not moved.  No GPU needed."""
import ctypes as C
import os
import re

from merkurio_amd import native as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sam_window_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    assert re.search(r"\bint\s+mk_tag_sam_window\s*\(\s*mk_matcher\s*\*\s*m\s*,\s*mk_sam_window\s*\*\s*w\s*,", hdr)
    assert re.search(r"\}\s*mk_sam_window\s*;", hdr)
    assert "mk_tag_sam_window" in mk.EXPORTS
    L = mk.load()
    assert hasattr(L, "mk_tag_sam_window")
    assert L.mk_abi_version() == 7 and "#define MK_ABI_VERSION 7" in hdr


def test_sam_window_struct_layout_matches_the_header():
    """the ctypes mirror has the header's fields in the header's order (the C struct has no padding surprises: 8-byte fields, then
    three u32 + 4 tag bytes, then 8-byte fields, then 8 floats)"""
    hdr = open(os.path.join(ROOT, "include", "merkurio_hip.h")).read()
    body = re.search(r"typedef struct mk_sam_window \{(.*?)\} mk_sam_window;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = decl.split(",")
        names.append(re.search(r"(\w+)\s*(\[\d+\])?$", first.strip()).group(1))
        names += [re.search(r"(\w+)", x).group(1) for x in more]
    assert names == [f[0] for f in mk.SamWindow._fields_]
    assert C.sizeof(mk.SamWindow) == 4 * 8 + 16 + 9 * 8 + 8 * 8 + 8 * 4
    assert mk.SamWindow.tail.offset == 48 and mk.SamWindow.n_window.offset == 120


def test_a_null_window_is_refused_without_a_device():
    L = mk.load()
    st = C.c_uint32()
    assert L.mk_tag_sam_window(None, None, 0, None, None, C.byref(st)) == mk.MK_E_INVALID_ARG
