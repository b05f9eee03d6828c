"""mk_tag_sam_bam_window without a GPU: the entry point is declared, listed, exported and refuses a NULL window; the ctypes struct
follows the header; and the number parsing the kernels use (merkurio_amd/csrc/sam_numbers.hpp), compiled for the host, gives the C
library's strtof / strtoll values for every spelling it accepts and says "not converted" for everything outside its rule.  The
float check is against strtof itself, not Python's float (which rounds to double first)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "merkurio_hip.h")
_FLAGS = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
          if os.environ.get("MERKURIO_TEST_SANITIZE") else ["-O1"])


# ---- the ABI
def test_entry_is_declared_listed_and_exported():
    from merkurio_amd import native
    text = open(HEADER).read()
    assert re.search(r"#define MK_ABI_VERSION 7\b", text)
    assert re.search(r"int mk_tag_sam_bam_window\(mk_matcher \*m, mk_codec \*codec, mk_sam_bam_window \*w, int logging, mk_counters \*counters,\s*"
                     r"uint32_t \*pattern_hit_counts,\s*uint32_t \*status\);", text)
    assert "mk_tag_sam_bam_window" in native.EXPORTS
    L = native.load()
    assert hasattr(L, "mk_tag_sam_bam_window")
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
    want = header_fields("mk_sam_bam_window")
    got = native.SamBamWindow._fields_
    assert [f[0] for f in got] == [w[0] for w in want]
    for (name, ctype), (_, htype, ptr, arr) in zip([(f[0], f[1]) for f in got], want):
        if ptr:
            assert ctype is C.c_void_p, name
        elif arr:
            assert ctype._type_ is scalar[htype] and ctype._length_ == arr, name
        else:
            assert ctype is scalar[htype], name
    # the two existing windows keep their layouts
    assert [f[0] for f in native.SamWindow._fields_] == [w[0] for w in header_fields("mk_sam_window")]
    assert [f[0] for f in native.BamWindow._fields_] == [w[0] for w in header_fields("mk_bam_window")]


def test_null_window_is_an_invalid_argument():
    from merkurio_amd import native
    L = native.load()
    c = native.Counters()
    status = C.c_uint32()
    # (the handles are checked before anything is done with them: no device needed)
    assert L.mk_tag_sam_bam_window(None, None, None, 0, C.byref(c), None, C.byref(status)) == native.MK_E_INVALID_ARG
    w = native.SamBamWindow()
    assert L.mk_tag_sam_bam_window(None, None, C.byref(w), 0, C.byref(c), None, C.byref(status)) == native.MK_E_INVALID_ARG


# ---- the numbers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samnum") / "sam_numbers_harness")
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-Wall", "-I", os.path.join(ROOT, "merkurio_amd/csrc"), "-o", exe,
                    os.path.join(ROOT, "tests/helpers/sam_numbers_harness.cpp")], check=True)
    return exe


def run(harness, tmp_path, kind, spellings):
    path = tmp_path / ("%s.txt" % kind)
    with open(path, "wb") as f:
        for s in spellings:
            assert b"\n" not in s
            f.write(kind.encode() + b"\t" + s + b"\n")
    r = subprocess.run([harness, str(path)], capture_output=True, text=True, check=True)
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(spellings)
    return rows


def mantissas():
    """0, 1, 2^24 - 1, powers of two +- 1, odd mantissas next to float halfway points of their products, a dense random sample"""
    rng = random.Random(24)
    ms = {0, 1, 2, 3, 5, 7, 9, 10, 99, 100, 101, 123, 15, 125, 625, 3125, (1 << 24) - 1, (1 << 24) - 2, (1 << 23), (1 << 23) + 1, (1 << 23) - 1}
    for k in range(1, 24):
        ms |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    # m * 10^e has more than 24 significant bits for most odd m: its float lies next to a halfway point whenever the bits below the
    # 24th are 0111.. or 1000..; multiples of 5^k times odd numbers near 2^24 give many such products
    for k in range(1, 11):
        p = 5 ** k
        for j in range(1, 400, 2):
            for m in (j * p, ((1 << 24) // p - j) * p + rng.randrange(p)):
                if 0 <= m < (1 << 24):
                    ms.add(m)
    ms |= {rng.randrange(1 << 24) for _ in range(6000)}
    ms |= {rng.randrange(1 << 24) | 1 for _ in range(3000)}
    return sorted(ms)


def spell(rng, m, e):
    """several spellings of m * 10^e: point positions, leading and trailing zeros, e / E, signs"""
    digits = str(m)
    out = []
    out.append(b"%se%d" % (digits.encode(), e))
    out.append(b"%sE%+d" % (digits.encode(), e))
    # a point inside the digits: the exponent moves with it
    k = rng.randrange(1, len(digits) + 1)
    if k < len(digits) and e + (len(digits) - k) <= 1000:
        out.append(b"%s.%se%d" % (digits[:k].encode(), digits[k:].encode(), e + len(digits) - k))
    # no exponent at all where the power of ten can be written with zeros or a point
    if -10 <= e < 0:
        pad = digits.rjust(-e + 1, "0")
        out.append(b"%s.%s" % (pad[:e].encode(), pad[e:].encode()))
        out.append(b"-000%s.%s" % (pad[:e].encode(), pad[e:].encode()))
    if e == 0:
        out.append(digits.encode())
        out.append(b"+" + digits.encode())
        out.append(b"-00" + digits.encode())
    # trailing zeros in the fraction change m and e, not the value: only where the rule still holds for the new pair
    if m * 10 < (1 << 24) and e - 1 >= -10:
        out.append(b"%s.0e%d" % (digits.encode(), e))
    out.append(b"-" + out[0])
    return out


def test_floats_inside_the_rule_are_strtof(harness, tmp_path):
    rng = random.Random(1)
    ms = mantissas()
    spellings = []
    for e in range(-10, 11):
        for m in (ms if e in (-10, -5, -1, 0, 1, 7, 10) else ms[::7]):
            spellings += spell(rng, m, e)
    spellings += [b"0", b"-0", b"+0", b"0.0", b"-0.0", b"0e0", b"-0e-10", b"0.0123", b"1e-05", b"1.5", b"00000000000000000001.50", b"16777215",
                  b"1.6777215e7", b"16777215e10", b"16777215e-10", b"0.0000000001", b"1E+10"]
    rows = run(harness, tmp_path, "f", spellings)
    bad = [(s, r) for s, r in zip(spellings, rows) if not (r[0] == "1" and r[2] == "1" and r[1] == r[3])]
    assert not bad, bad[:10]
    assert len(spellings) > 200000


def test_floats_outside_the_rule_are_not_converted(harness, tmp_path):
    out = [b"16777216", b"1.6777216e7", b"167772160e-1", b"1e11", b"1e-11", b"0.00000000001", b"1.0e-11", b"10e11", b"inf", b"-inf", b"nan", b"NaN",
           b"infinity", b"0x1p3", b"0x10", b"", b"+", b"-", b".", b"1.5x", b"1.5 ", b" 1.5", b"1e", b"1e+", b"1.e5", b".5", b"5.", b"1..2", b"1e5.0",
           b"--1", b"1,5", b"99999999", b"123456789012345678901234567890", b"1e99999999999999999999", b"0.%s1" % (b"0" * 80), b"1e1000", b"1f", b"1.5f",
           # longer than the 63 bytes the host path hands strtof: what strtof sees there is not what is written
           b"0" * 70 + b"1.5", b"0" * 61 + b"1.5", b"1e" + b"0" * 70 + b"5", b"1." + b"0" * 62]
    ok = [b"0" * 60 + b"1.5", b"1e" + b"0" * 60 + b"5"]  # 63 bytes are still converted
    assert all(len(s) == 63 for s in ok) and all(r[0] == "1" and r[1] == r[3] for r in run(harness, tmp_path, "f", ok))
    rows = run(harness, tmp_path, "f", out)
    assert [(s, r[0]) for s, r in zip(out, rows) if r[0] != "0"] == []


def test_integers_are_strtoll_or_not_converted(harness, tmp_path):
    rng = random.Random(2)
    good = [b"0", b"-0", b"+0", b"1", b"-1", b"255", b"256", b"65535", b"65536", b"-128", b"-129", b"-32768", b"-32769", b"2147483647", b"2147483648",
            b"-2147483648", b"4294967295", b"4294967296", b"999999999999999999", b"-999999999999999999", b"+999999999999999999", b"000000000000000042"]
    for _ in range(20000):
        n = rng.randrange(1, 19)
        good.append(rng.choice([b"", b"-", b"+"]) + bytes(rng.choice(b"0123456789") for _ in range(n)))
    rows = run(harness, tmp_path, "i", good)
    bad = [(s, r) for s, r in zip(good, rows) if not (r[0] == "1" and r[2] == "1" and r[1] == r[3])]
    assert not bad, bad[:10]
    out = [b"", b"+", b"-", b" 1", b"1 ", b"1x", b"x", b"1.0", b"1e3", b"0x10", b"--1", b"+-1", b"1234567890123456789", b"-1234567890123456789",
           b"9223372036854775808", b"99999999999999999999999", b"1,2"]
    rows = run(harness, tmp_path, "i", out)
    assert [(s, r[0]) for s, r in zip(out, rows) if r[0] != "0"] == []


def test_cigar_lengths(harness, tmp_path):
    rng = random.Random(3)
    good = [b"0", b"1", b"9", b"10", b"150", b"999999999", b"268435455", b"268435456", b"000000001"]
    good += [bytes(rng.choice(b"0123456789") for _ in range(rng.randrange(1, 10))) for _ in range(5000)]
    rows = run(harness, tmp_path, "c", good)
    bad = [(s, r) for s, r in zip(good, rows) if not (r[0] == "1" and r[2] == "1" and r[1] == r[3])]
    assert not bad, bad[:10]
    out = [b"", b"1234567890", b"+1", b"-1", b" 1", b"1M", b"M"]
    rows = run(harness, tmp_path, "c", out)
    assert [(s, r[0]) for s, r in zip(out, rows) if r[0] != "0"] == []
