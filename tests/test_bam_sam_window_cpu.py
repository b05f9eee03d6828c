"""mk_tag_bam_sam_window without a GPU: the entry point is declared, listed, exported and refuses a NULL window; the ctypes struct
follows the header; and the number formatting the kernels use (merkurio_amd/csrc/bam_numbers.hpp), compiled for the host, gives
std::to_string's and snprintf("%g")'s bytes -- the host path's own calls (cli/bam_text.cpp: aux_to_text) -- for every value it takes, and
refuses exactly the floats "%g" writes in exponent notation (and inf / nan).

The float check is EXHAUSTIVE: every positive float of the 34 binades the rule can take and of two more on each side (3.2e8 values, on
all threads about 25 s on eight cores), every 64th one with its sign set as well.  Under MERKURIO_TEST_SANITIZE=1, where the same run takes several
minutes, it is the reduced set: every mantissa of the two edge binades on each side of the rule, per other binade every mantissa whose
scaled remainder is within 2 of one half, and 2^20 random ones."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "merkurio_hip.h")
SANITIZE = bool(os.environ.get("MERKURIO_TEST_SANITIZE"))
_FLAGS = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if SANITIZE else ["-O2"])


# ---- the ABI
def test_entry_is_declared_listed_and_exported():
    from merkurio_amd import native
    text = open(HEADER).read()
    assert re.search(r"#define MK_ABI_VERSION 7\b", text)
    assert re.search(r"int mk_tag_bam_sam_window\(mk_matcher \*m, mk_codec \*codec, mk_bam_sam_window \*w, int logging, mk_counters \*counters,\s*"
                     r"uint32_t \*pattern_hit_counts,\s*uint32_t \*status\);", text)
    assert "mk_tag_bam_sam_window" in native.EXPORTS
    L = native.load()
    assert hasattr(L, "mk_tag_bam_sam_window")
    assert L.mk_abi_version() == 7


def header_fields(name):
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        fn = re.search(r"\(\*(\w+)\)", decl)  # a function pointer
        if fn:
            out.append((fn.group(1), "void", True, 0))
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(.*)$", decl, re.S)
        ctype = m.group(2)
        for item in m.group(3).split(","):
            item = item.strip()
            ptr = item.startswith("*")
            nm = re.match(r"\*?\s*(\w+)", item).group(1)
            arr = re.search(r"\[(\d+)\]", item)
            out.append((nm, ctype, ptr, int(arr.group(1)) if arr else 0))
    return out


def test_ctypes_struct_follows_the_header():
    from merkurio_amd import native
    scalar = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "uint8_t": C.c_uint8, "float": C.c_float}
    want = header_fields("mk_bam_sam_window")
    got = native.BamSamWindow._fields_
    assert [f[0] for f in got] == [w[0] for w in want]
    for (name, ctype), (_, htype, ptr, arr) in zip([(f[0], f[1]) for f in got], want):
        if ptr:
            assert ctype is C.c_void_p, name
        elif arr:
            assert ctype._type_ is scalar[htype] and ctype._length_ == arr, name
        else:
            assert ctype is scalar[htype], name
    # what the issue lists, in its order
    assert [f[0] for f in got] == ["head", "n_head", "bgzf", "n_bgzf", "members", "n_members", "last", "filter_matching", "invert", "tag", "reserved",
                                   "ref_names", "ref_off", "n_refs", "tail", "tail_cap", "out", "out_cap", "rows", "rows_cap", "row_name", "names",
                                   "names_cap", "on_tail", "on_tail_ctx", "n_window", "n_used", "n_tail", "n_rec", "n_kept", "out_len", "n_rows",
                                   "n_names_bytes", "ms"]
    # the existing windows keep their layouts
    assert [f[0] for f in native.SamWindow._fields_] == [w[0] for w in header_fields("mk_sam_window")]
    assert [f[0] for f in native.BamWindow._fields_] == [w[0] for w in header_fields("mk_bam_window")]
    assert [f[0] for f in native.SamBamWindow._fields_] == [w[0] for w in header_fields("mk_sam_bam_window")]


def test_null_window_is_an_invalid_argument():
    from merkurio_amd import native
    L = native.load()
    c = native.Counters()
    status = C.c_uint32()
    # (the handles are checked before anything is done with them: no device needed)
    assert L.mk_tag_bam_sam_window(None, None, None, 0, C.byref(c), None, C.byref(status)) == native.MK_E_INVALID_ARG
    w = native.BamSamWindow()
    assert L.mk_tag_bam_sam_window(None, None, C.byref(w), 0, C.byref(c), None, C.byref(status)) == native.MK_E_INVALID_ARG


# ---- the numbers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bamnum") / "bam_numbers_harness")
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-Wall", "-pthread", "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(ROOT, "tests/helpers/bam_numbers_harness.cpp")], check=True)
    return exe


def run(harness, tmp_path, mode, lines):
    path = tmp_path / ("%s.txt" % mode)
    path.write_text("".join(s + "\n" for s in lines))
    r = subprocess.run([harness, mode, str(path)], capture_output=True, text=True, check=True)
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def test_integers_are_to_string(harness, tmp_path):
    vals = {0, 1, -1, -(1 << 31), (1 << 31) - 1, (1 << 31), (1 << 32) - 1, 1 << 32, -(1 << 63), (1 << 63) - 1, 255, 256, -128, -129, 65535, 65536, -32768,
            -32769, (1 << 28) - 1}
    for k in range(1, 19):  # every width's edges: 9 / 10 ... 10^18 - 1 / 10^18, both signs
        vals |= {10 ** k - 1, 10 ** k, 10 ** k + 1, -(10 ** k - 1), -(10 ** k), -(10 ** k + 1)}
    vals.add(((1 << 31) - 1) + 1)  # POS + 1 with POS = INT32_MAX, in 64 bits (the device refuses that record; the formatter is right anyway)
    vals = sorted(vals)
    rows = run(harness, tmp_path, "i", [str(v) for v in vals])
    assert [(v, r) for v, r in zip(vals, rows) if not (r[0] == r[1] == str(v))] == []


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def below(b):
    return b - 1  # the next float towards zero (positive, normal)


def test_named_floats(harness, tmp_path):
    inf = float("inf")
    small = bits(0.0001)  # the float next to 0.0001 (just above it)
    # the smallest float that still rounds to 0.0001: 9.999995e-05 is the halfway point, exact values above it round up
    lo = small
    while "%g" % struct.unpack("<f", struct.pack("<I", below(lo)))[0] == "0.0001":
        lo = below(lo)
    assert lo < small and "%g" % struct.unpack("<f", struct.pack("<I", below(lo)))[0] == "9.99999e-05"
    cases = [(bits(131072.5), "131072"), (bits(131073.5), "131074"),  # ties to even
             (bits(999999.5), None), (bits(999999.4375), "999999"), (small, "0.0001"), (lo, "0.0001"), (below(lo), None), (bits(9.99994e-05), None),
             (bits(-0.0), "-0"), (bits(0.0), "0"), (bits(1e6), None), (bits(inf), None), (bits(-inf), None), (0x7FC00000, None), (0xFFC00001, None),
             (1, None), (0x007FFFFF, None), (0x80000001, None),  # subnormals
             (0x00800000, None),  # the smallest normal
             (bits(1.0), "1"), (bits(-1.5), "-1.5"), (bits(0.1), "0.1"), (bits(100000.0), "100000"), (bits(123456.0), "123456"), (bits(-0.00012345), "-0.00012345"),
             (bits(3.14159274), "3.14159"), (bits(1e-5), None), (bits(524292.0), "524292"), (bits(0.5), "0.5"), (bits(1048575.0), None)]
    rows = run(harness, tmp_path, "f", ["%08x" % b for b, _ in cases])
    for (b, want), r in zip(cases, rows):
        libc = r[2]
        py = "%g" % struct.unpack("<f", struct.pack("<I", b))[0]
        assert libc.lstrip("-") == py.lstrip("-") or "n" in libc, (hex(b), libc, py)  # (the C library's %g is CPython's; nan's sign aside)
        if want is None:
            assert r[0] == "0", (hex(b), r)
            assert "e" in libc or "n" in libc, (hex(b), r)  # refused only where %g leaves fixed notation
        else:
            assert r[0] == "1" and r[1] == want == libc, (hex(b), r, want)


def test_every_float_of_the_rule_is_percent_g(harness):
    """exhaustive (see the module's docstring for what runs under the sanitizers)"""
    threads = min(16, os.cpu_count() or 1)
    r = subprocess.run([harness, "x", str(threads), "some" if SANITIZE else "all"], capture_output=True, text=True, check=True)
    m = re.match(r"checked (\d+) taken (\d+) bad (\d+)", r.stdout)
    assert m, r.stdout
    checked, taken, bad = map(int, m.groups())
    assert bad == 0, r.stdout
    if not SANITIZE:
        assert checked == 38 * (1 << 23) + 38 * (1 << 17)  # 38 binades, every 64th value twice
        # the taken ones: every float from the smallest that rounds to 0.0001 up to the largest below 999999.5, and their signed copies
        assert 283000000 < taken < 284000000
    else:
        assert checked > 8 * (1 << 23) and taken > 30 * (1 << 20)
