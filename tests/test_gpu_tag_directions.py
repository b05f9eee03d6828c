"""The four directions of `tag` on device windows (mk_tag_bam_window, mk_tag_sam_window, mk_tag_sam_bam_window, mk_tag_bam_sam_window)
on ONE input, taken as BAM records and as the SAM text of the same records (test_gpu_bam_sam_window.sam_line): an input side and an
output side may be combined freely, so all four find the same records, keep the same ones, log the same rows and count the same,
both text outputs are the same bytes, and both member outputs hold the same names and tag values.  What those answers ARE is the
business of the four directions' own files; here only that they agree.  The optional fields are Z strings only -- no number is
formatted or parsed, no integer type chosen -- and some records carry a field of the tag's name already."""
import random
import struct

import pytest

from tag_windows import _bgzf, bam_record, inflate, patterns31
from test_gpu_bam_sam_window import sam_line

pytestmark = pytest.mark.gpu
REFS = [b"chr1", b"chr2"]
FLAGS = [(False, False), (True, False), (True, True)]  # plain, -m, -m -v


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def handles(mk):
    pats = patterns31(mk, 40)
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    yield pats, m, codec
    codec.close()


def records(pats, lens, n, seed):
    """n records of the given lengths, a third with k-mers of the set planted (where they fit), a fifth with a km field already"""
    rnd = random.Random(seed)
    recs = []
    for i in range(n):
        L = rnd.choice(lens)
        s = bytearray(rnd.choice(b"ACGT") for _ in range(L))
        if rnd.random() < 0.35:
            for _ in range(rnd.choice((1, 2, 3))):
                p = rnd.choice(pats)
                if len(p) <= L:
                    at = rnd.randrange(L - len(p) + 1)
                    s[at:at + len(p)] = p
        aux = b"RGZ" + b"grp%d" % rnd.randrange(4) + b"\0" if rnd.random() < 0.5 else b""
        if rnd.random() < 0.2:
            aux += b"kmZ" + rnd.choice((b"TTTT", bytes(rnd.choice(pats)), b"AC,GT")) + b"\0" + b"XZZ" + b"behind\0"
        recs.append(bam_record(b"r%d.%d" % (i, rnd.randrange(1000)), bytes(s), aux=aux, cigar=((L << 4),), ref=i % 2, pos=rnd.randrange(10 ** 6)))
    return recs


def kept_names_and_tags(text):
    """[(name, [every Z field (tag, value)])] of the BAM records in text"""
    out, p = [], 0
    while p < len(text):
        size = struct.unpack_from("<i", text, p)[0]
        rec = text[p:p + 4 + size]
        p += 4 + size
        l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
        q = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        fields = []
        while q < len(rec):
            assert rec[q + 2] == ord("Z")
            e = rec.index(b"\0", q + 3)
            fields.append((rec[q:q + 2], rec[q + 3:e]))
            q = e + 1
        out.append((rec[36:36 + l_name - 1], fields))
    assert p == len(text)
    return out


def joined(res):
    """the windows of one direction as one answer: records re-numbered through the windows, counters summed"""
    assert all(r["status"] == 0 for r in res)
    rows, base = [], 0
    for r in res:
        rows += [(name, base + rec, pat, pos) for (name, rec, pat, pos) in r["rows"]]
        base += r["n_rec"]
    cs = [r["counters"] for r in res]
    counters = {k: [sum(x) for x in zip(*(c[k] for c in cs))] if isinstance(cs[0][k], (list, tuple)) else sum(c[k] for c in cs) for k in cs[0]}
    return dict(n_rec=base, n_kept=sum(r["n_kept"] for r in res), rows=rows, counters=counters, out=b"".join(r["out"] for r in res))


def run_all(mk, handles, recs, fm, inv, block=0xff00, bam_cut=None, sam_cut=None):
    """the records through the four directions -> their joined answers (bam_cut: members in the first of two windows; sam_cut: bytes)"""
    pats, m, codec = handles
    kw = dict(logging=True, filter_matching=fm, invert=inv)
    text = b"".join(recs)
    blob = _bgzf(text, block)
    members, used, tb = mk.bgzf_members(blob)
    assert used == len(blob) and tb == len(text)
    sam = b"".join(sam_line(r, REFS)[0] + b"\n" for r in recs)
    member_windows = [members] if bam_cut is None else [members[:bam_cut], members[bam_cut:]]
    text_windows = [sam] if sam_cut is None else [sam[:sam_cut], sam[sam_cut:]]

    def chain(call, windows):
        head, res = b"", []
        for i, win in enumerate(windows):
            res.append(call(head, win, i == len(windows) - 1))
            head = res[-1]["tail"]
        if len(windows) == 2:  # the first window ends inside a record / a line: the second starts with a head
            assert res[0]["tail"] and res[1]["tail"] == b""
        return joined(res)

    return dict(bam_bam=chain(lambda h, w, last: m.tag_bam_window(codec, h, blob, w, last, **kw), member_windows),
                bam_sam=chain(lambda h, w, last: m.tag_bam_sam_window(codec, h, blob, w, last, refs=REFS, **kw), member_windows),
                sam_sam=chain(lambda h, w, last: m.tag_sam_window(h, w, last, **kw), text_windows),
                sam_bam=chain(lambda h, w, last: m.tag_sam_bam_window(codec, h, w, last, refs=REFS, **kw), text_windows)), sam


def agree(res, n):
    first = res["bam_bam"]
    assert first["n_rec"] == n
    for name, r in res.items():
        for key in ("n_rec", "n_kept", "rows", "counters"):
            assert r[key] == first[key], (name, key)
    assert res["bam_sam"]["out"] == res["sam_sam"]["out"]
    assert res["bam_sam"]["out"].count(b"\n") == first["n_kept"]
    from_bam, from_sam = kept_names_and_tags(inflate(res["bam_bam"]["out"])), kept_names_and_tags(inflate(res["sam_bam"]["out"]))
    assert len(from_bam) == first["n_kept"] and from_bam == from_sam
    return first


SHAPES = {"one record": ((150,), 1), "one length": ((150,), 65), "ragged": ((1, 30, 31, 150), 65)}


@pytest.mark.parametrize("fm,inv", FLAGS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_window(mk, handles, shape, fm, inv):
    lens, n = SHAPES[shape]
    recs = records(handles[0], lens, n, seed=n + len(lens))
    res, _ = run_all(mk, handles, recs, fm, inv)
    agree(res, n)


@pytest.mark.parametrize("fm,inv", FLAGS)
def test_two_windows_with_a_head(mk, handles, fm, inv):
    recs = records(handles[0], (1, 30, 31, 150), 300, seed=9)
    sam_len = sum(len(sam_line(r, REFS)[0]) + 1 for r in recs)
    # members of 1000 bytes of text end inside records almost everywhere; 17 of them make the first window
    res, _ = run_all(mk, handles, recs, fm, inv, block=1000, bam_cut=17, sam_cut=sam_len // 2)
    first = agree(res, 300)
    assert first["rows"] and (first["n_kept"] < 300) == fm


@pytest.mark.parametrize("fm,inv", FLAGS)
def test_text_outputs_one_byte_short_then_exact(mk, handles, fm, inv):
    pats, m, codec = handles
    recs = records(pats, (1, 30, 31, 150), 300, seed=9)
    res, sam = run_all(mk, handles, recs, fm, inv)
    want = agree(res, 300)
    out, need = res["sam_sam"]["out"], len(res["sam_sam"]["out"])
    assert need > 0
    blob = _bgzf(b"".join(recs))
    members, _, _ = mk.bgzf_members(blob)

    def sam_sam(cap):  # (the wrapper has no out_cap: the helper all four share, with its struct filled as the wrapper fills it)
        w = mk.SamWindow()
        hold = m._window_common(w, b"", True, b"km", fm, inv) + m._window_text(w, sam)[0]
        r, rc, guard = m._tag_window(w, mk.load().mk_tag_sam_window, (m._h,), len(sam), True, True, cap, 16)
        del hold
        return dict(r, rc=rc, out_len=w.out_len, guard=guard)

    def bam_sam(cap):
        return m.tag_bam_sam_window(codec, b"", blob, members, True, refs=REFS, logging=True, filter_matching=fm, invert=inv, out_cap=cap, guard=16)

    for call in (sam_sam, bam_sam):
        short = call(need - 1)
        assert short["rc"] == mk.MK_E_CAPACITY and short["out_len"] == need and short["guard"] == b"\xa5" * 16 and short["out"] == b""
        fit = call(need)
        assert fit["rc"] == 0 and fit["status"] == 0 and fit["out_len"] == need and fit["out"] == out and fit["guard"] == b"\xa5" * 16
        assert fit["rows"] == want["rows"] and fit["n_kept"] == want["n_kept"]
