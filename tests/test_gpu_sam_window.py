"""`tag` on windows of SAM text that stay on the device (mk_tag_sam_window, an addition to ABI v7; kernels: sam.hip) against the
oracle's restatement of process_record (src/cmd_tag.rs:387-497) and the line rule of the CLI's host path (cli/sam_in.cpp: parse_sam_text,
SamFile::gather, SamFile::find_tag): lines split at '\\n' with one '\\r' stripped, '@' and empty lines skipped, SEQ = field 10
upper-cased for the matcher, a kept line leaves as line TAB tag ":Z:" value '\\n'.  Expected bytes are built here from the oracle's
answers; the inputs are valid, so no test but test_refusals accepts a refused window."""
import os
import random

import numpy as np
import pytest

import oracle_binding as ob
from tag_windows import existing_value, patterns31, records_of

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


def expected(ob_m, patterns, text, tag, logging, filter_matching, invert, last=True):
    """oracle: keep, rows [(name, rec, pat, pos)], counters, the kept lines with their tag appended, number of records"""
    recs, _ = records_of(text, last)
    keep, rows, c, found = ob.tag_records(ob_m, [r[2] for r in recs], logging=logging, filter_matching=filter_matching, invert=invert)
    out = bytearray()
    for (ln, _, _, aux), k, f in zip(recs, keep, found):
        if not k:
            continue
        ex = existing_value(aux, tag)
        out += ln + b"\t" + tag + b":Z:" + ob.tag_value(patterns, f, ex if ex else None) + b"\n"
    names = [(recs[rec][1], rec, pat, pos) for (_, rec, pat, pos) in rows]
    return keep, names, c, bytes(out), len(recs)


def sam_line(rnd, i, patterns, lens=(150,), hit=0.2, alpha=b"ACGT", aux_kinds=True, lower=0.0, eol=b"\n"):
    L = rnd.choice(lens)
    s = bytearray(rnd.choice(alpha) for _ in range(L))
    if patterns and rnd.random() < hit:
        for _ in range(rnd.choice((1, 1, 2, 3))):
            p = rnd.choice(patterns)
            if len(p) <= L:
                k = rnd.randrange(0, L - len(p) + 1)
                s[k:k + len(p)] = p
    if rnd.random() < lower:
        s = bytearray(bytes(s).lower())
    f = [b"read%d_%d" % (i, rnd.randrange(10 ** 6)), b"%d" % rnd.choice((0, 4, 99, 147)), b"chr1", b"%d" % rnd.randrange(1, 10 ** 6), b"60",
         (b"%dM" % L) if L else b"*", b"=", b"%d" % rnd.randrange(1, 10 ** 6), b"0", bytes(s) if L else b"*", (b"I" * L) if L else b"*"]
    if aux_kinds:
        pick = rnd.randrange(7)
        if pick >= 1:
            f.append(b"NM:i:%d" % rnd.randrange(9))
        if pick >= 2:
            f.append(b"AS:i:%d" % rnd.randrange(1000))
        if pick >= 3:
            f.append(b"RG:Z:grp%d" % rnd.randrange(4))
        if pick >= 4:
            f.append(b"ZB:B:s,1,-2,3")
        if pick >= 5:
            f += [b"XA:A:q", b"XH:H:0AFF", b"XF:f:1.5"]
        if pick >= 6:
            f = f[:10]  # (QUAL and everything behind it left out: SEQ is the last field)
    return b"\t".join(f) + eol


def run_windows(m, text, cuts, **kw):
    """text[cuts[i], cuts[i + 1]) as the bodies of consecutive windows, the tail of one carried as the head of the next"""
    head, res = b"", []
    for i in range(len(cuts) - 1):
        r = m.tag_sam_window(head, text[cuts[i]:cuts[i + 1]], last=(i == len(cuts) - 2), **kw)
        res.append(r)
        if r["status"]:
            break
        head = r["tail"]
    return res


def check_windows(res, keep, rows, c, out, n_rec, logging):
    assert all(x["status"] == 0 for x in res), [x["status"] for x in res]
    assert sum(x["n_rec"] for x in res) == n_rec and sum(x["n_kept"] for x in res) == sum(keep)
    assert b"".join(x["out"] for x in res) == out
    if logging:
        got_rows, base = [], 0
        for x in res:
            got_rows += [(nm, rec + base, pat, pos) for (nm, rec, pat, pos) in x["rows"]]
            base += x["n_rec"]
        assert got_rows == rows
        for k in ("records", "bases"):
            assert sum(x["counters"][k] for x in res) == c[k]
        assert sum(x["counters"]["hits"][0] for x in res) == c["hits"][0] and sum(x["counters"]["records_hit"][0] for x in res) == c["records_hit"][0]
        assert np.array_equal(np.sum([x["counters"]["pattern_hit_counts"] for x in res], axis=0), c["pattern_hit_counts"])


@pytest.mark.parametrize("filter_matching,invert", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("logging", [True, False])
def test_window_matches_oracle(mk, filter_matching, invert, logging):
    rnd = random.Random(11)
    pats = patterns31(mk)
    text = b"".join(sam_line(rnd, i, pats) for i in range(3000))
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", logging, filter_matching, invert)
    r = m.tag_sam_window(b"", text, last=True, logging=logging, filter_matching=filter_matching, invert=invert)
    assert r["status"] == 0 and r["n_rec"] == n_rec == 3000 and r["n_window"] == r["n_used"] == len(text) and r["tail"] == b""
    assert r["n_kept"] == sum(keep) and r["out"] == out
    if logging:
        assert r["rows"] == rows
        got = dict(r["counters"])
        assert got.pop("extracted") == sum(keep)  # (the device reports the records it wrote; the reference has no such counter in tag)
        want = dict(c)
        want.pop("extracted")
        assert got == want


def ragged_text(rnd, pats, n=1200):
    parts = []
    for i in range(n):
        parts.append(sam_line(rnd, i, pats, lens=(0, 1, 31, 150, 2500), hit=0.4, alpha=b"ACGTN", lower=0.3, eol=rnd.choice((b"\n", b"\r\n"))))
        if i % 97 == 5:
            parts.append(rnd.choice((b"\n", b"\r\n", b"@CO\ta comment in the middle\n", b"@CO\tanother\r\n")))
    return b"".join(parts)


def test_ragged_lines_and_window_cuts(mk):
    """SEQ lengths 0 ('*'), 1, 31, 150, 2 500; lower-case SEQ; CRLF mixed with LF; blank and @CO lines in the middle; a last line
    without a line end (last=True: a line, last=False: the tail); windows cut at arbitrary bytes with the tail carried as head"""
    rnd = random.Random(5)
    pats = patterns31(mk, 50)
    text = ragged_text(rnd, pats)[:-1]  # the last line has no '\n'
    assert not text.endswith(b"\n")
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"XK", True, False, False)
    one = m.tag_sam_window(b"", text, last=True, tag=b"XK")
    check_windows([one], keep, rows, c, out, n_rec, True)
    assert one["n_used"] == len(text) and one["tail"] == b""
    # the same text with more to follow: the unfinished line is the tail
    keep2, rows2, c2, out2, n_rec2 = expected(om, pats, text, b"XK", True, False, False, last=False)
    part = m.tag_sam_window(b"", text, last=False, tag=b"XK")
    check_windows([part], keep2, rows2, c2, out2, n_rec2, True)
    cut = text.rfind(b"\n") + 1
    assert n_rec2 == n_rec - 1 and part["n_used"] == cut and part["tail"] == text[cut:]
    for n_cuts in (1, 7, 60):
        cuts = [0] + sorted(rnd.randrange(1, len(text)) for _ in range(n_cuts)) + [len(text)]
        res = run_windows(m, text, cuts, tag=b"XK", logging=True)
        check_windows(res, keep, rows, c, out, n_rec, True)


def test_bndmq_counts_and_iupac_letters(mk):
    """fewer than 14 patterns: BNDMq's pattern_hit_counts (one per record and pattern) and its emission order; IUPAC letters"""
    rnd = random.Random(9)
    pats = mk.parse_pattern_list(kmer_seq=[b"ACGTACG", b"NNRYK", b"GATTACA", b"TTT"])
    text = b"".join(sam_line(rnd, i, pats, lens=(40, 41, 90), hit=0.5, alpha=b"ACGTNRYKMSWBDHV") for i in range(800))
    m = mk.Matcher(pats, device=0)
    assert not m.use_ac
    om = ob.Matcher(pats, False, 0, False)
    keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, True, False)
    r = m.tag_sam_window(b"", text, last=True, logging=True, filter_matching=True)
    assert r["status"] == 0 and r["out"] == out and r["rows"] == rows
    assert r["counters"]["pattern_hit_counts"] == c["pattern_hit_counts"] and r["counters"]["hits"] == c["hits"]


def test_existing_tag_values_are_merged(mk):
    """lines that already carry the tag (src/cmd_tag.rs:470-485): the values of test_gpu_bam_window's test of that name in text
    form, a second field of the same name (ignored), the tag as field 12 and as the last field, a field `kmX:` shorter than 5 bytes"""
    rnd = random.Random(8)
    pats = patterns31(mk, 30)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, True, 0, False)
    values = [b"", b"ZZZ", b"TTT,AAA,CCC", b"AAA,AAA,AAA", b",,", b"x,", b",x", pats[3], pats[5] + b"," + pats[1], b"a," + pats[0] + b",B,b,A", b"ACGT" * 100,
              b"0,00,000,0000", pats[2][:-1], pats[2] + b"A"]
    lines = []
    for i in range(600):
        s = bytearray(rnd.choice(b"ACGT") for _ in range(120))
        for _ in range(rnd.randrange(0, 4)):
            p = rnd.choice(pats[:8])
            k = rnd.randrange(0, 120 - 31)
            s[k:k + 31] = p
        f = [b"e%d" % i, b"0", b"chr1", b"100", b"60", b"120M", b"*", b"0", b"0", bytes(s), b"F" * 120]
        v = rnd.choice(values) if i % 3 else None
        mine = [] if v is None else [b"km:Z:" + v]
        if v is not None and i % 7 == 0:
            mine.append(b"km:Z:second,field")  # (only the first field of that name is looked at)
        short = [b"km:Z", b"km:", b"kmX:"][i % 3:i % 3 + 1] if i % 5 == 0 else []  # (shorter than 5 bytes: not a field of that name)
        where = i % 4
        if where == 0:    # the tag is field 12
            f += short[:0] + mine + [b"NM:i:2", b"AS:i:%d" % i] + short
        elif where == 1:  # ... the last field
            f += [b"NM:i:2"] + short + [b"AS:i:%d" % i] + mine
        elif where == 2:  # ... in the middle, behind a long field
            f += [b"NM:i:2", b"XL:Z:" + b"q" * 300] + short + mine + [b"AS:i:%d" % i]
        else:             # ... the only optional field
            f += mine if mine else short
        lines.append(b"\t".join(f) + b"\n")
    text = b"".join(lines)
    for fm in (False, True):
        keep, rows, c, out, n_rec = expected(om, pats, text, b"km", True, fm, False)
        r = m.tag_sam_window(b"", text, last=True, logging=True, filter_matching=fm)
        assert r["status"] == 0 and r["n_kept"] == sum(keep)
        if r["out"] != out:  # (which line differs, for the failure message)
            a, b = r["out"].split(b"\n"), out.split(b"\n")
            bad = [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:3]
            raise AssertionError(f"lines {bad}: {[(a[k][-90:], b[k][-90:]) for k in bad]}; {len(a)} / {len(b)} lines")
        assert r["rows"] == rows


def test_refusals(mk):
    rnd = random.Random(2)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    good = [sam_line(rnd, i, pats, hit=0.5) for i in range(50)]
    hit_seq = pats[0] + b"A" * 40

    def line(name, aux, n_fields=11):
        f = [name, b"0", b"chr1", b"100", b"60", b"71M", b"*", b"0", b"0", hit_seq, b"F" * len(hit_seq)][:n_fields]
        return b"\t".join(f + aux) + b"\n"

    def run(lines, **kw):
        return m.tag_sam_window(b"", b"".join(lines), last=True, **kw)

    assert run(good + [line(b"ok", [b"NM:i:1"])] + good)["status"] == 0
    # a record line with 9 fields: the host reader's "too few fields"
    r = run(good + [line(b"short", [], n_fields=9)] + good)
    assert r["status"] == 1 and r["out"] == b"" and r["counters"]["records"] == 0
    assert run(good + [line(b"ten", [], n_fields=10)])["status"] == 0  # (10 fields are enough)
    # a kept record with a field of the tag's name that is not a string (the reference bails) ...
    r = run(good + [line(b"old", [b"NM:i:1", b"km:i:5"])] + good)
    assert r["status"] == 4 and r["out"] == b""
    # ... but not when that record is dropped (-v drops records with a hit; a dropped record's fields are not looked at)
    assert run(good + [line(b"old", [b"km:i:5"])], invert=True)["status"] == 0
    # a value that is not plain ASCII, a value above 2 KiB
    assert run(good + [line(b"old", [b"km:Z:" + "AAA,é".encode()])])["status"] == 4
    assert run(good + [line(b"old", [b"km:Z:" + b"ACGT," * 500])])["status"] == 4
    assert run(good + [line(b"old", [b"km:Z:" + b"ACGT," * 400])])["status"] == 0
    # no output asked for: the checks still run, no text comes back
    r = run(good + [line(b"old", [b"km:i:5"])] + good, write=False)
    assert r["status"] == 4
    r = run(good, write=False)
    assert r["status"] == 0 and r["out"] == b"" and r["n_kept"] == 50 and r["counters"]["records"] == 50


def test_nothing_kept_and_empty_windows(mk):
    rnd = random.Random(4)
    pats = patterns31(mk, 20)
    m = mk.Matcher(pats, device=0)
    text = b"".join(sam_line(rnd, i, pats, hit=0.0) for i in range(300))
    r = m.tag_sam_window(b"", text, last=True, filter_matching=True)
    assert r["status"] == 0 and r["n_kept"] == 0 and r["out"] == b"" and r["n_rec"] == 300
    r = m.tag_sam_window(b"", b"", last=True)
    assert r["status"] == 0 and r["n_rec"] == 0 and r["n_window"] == 0
    r = m.tag_sam_window(b"", b"@HD\tVN:1.6\n\n\r\n", last=True)
    assert r["status"] == 0 and r["n_rec"] == 0 and r["n_used"] == 14 and r["out"] == b""
    r = m.tag_sam_window(b"", text[:100], last=False)  # not one line end: everything is the tail
    assert r["status"] == 0 and r["n_rec"] == 0 and r["n_used"] == 0 and r["tail"] == text[:100]


def _record_lines(path):
    return [ln for ln in open(path, "rb").read().split(b"\n") if ln and ln[:1] != b"@"]


def test_reference_fixtures(mk):
    """the reference's own tag fixtures: every record line of its outputs is the input line plus one km field"""
    fx = os.path.join(GOLDEN, "fixtures")
    text = open(os.path.join(fx, "input", "simple.sam"), "rb").read()
    pats = mk.parse_pattern_list(kmer_seq=[b"CTC"], reverse_complement=True)  # tag ... -s CTC -r
    m = mk.Matcher(pats, device=0)
    r = m.tag_sam_window(b"", text, last=True, filter_matching=True)
    assert r["status"] == 0 and r["out"].split(b"\n")[:-1] == _record_lines(os.path.join(fx, "tag", "simple.extracted.sam"))
    r = m.tag_sam_window(b"", text, last=True, invert=True)
    assert r["status"] == 0 and r["out"].split(b"\n")[:-1] == _record_lines(os.path.join(fx, "tag", "simple-inv.extracted.sam"))
    wf = os.path.join(GOLDEN, "example-workflow")
    text = open(os.path.join(wf, "output", "mutant_extracted.sorted.sam"), "rb").read()
    pats = mk.parse_pattern_list(kmer_file=os.path.join(wf, "significant_kmers.txt"), reverse_complement=True)
    m = mk.Matcher(pats, device=0)
    r = m.tag_sam_window(b"", text, last=True, logging=False)
    want = _record_lines(os.path.join(wf, "output", "mutant_extracted.sorted.tagged.sam"))
    assert r["status"] == 0 and len(want) == 48 and r["out"].split(b"\n")[:-1] == want


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_windows_against_the_oracle(mk, seed):
    """seeded differential test: line shapes (SEQ lengths 0 ... 3 000, lower case, IUPAC letters, every kind of optional field,
    existing values of the tag, CRLF, blank and '@' lines, a missing last line end), window cuts with the tail carried, filter flags,
    AC and BNDMq pattern sets -- every window must be taken and the lines must be the oracle's"""
    rnd = random.Random(3000 + seed)
    few = rnd.random() < 0.3
    if few:
        pats = mk.parse_pattern_list(kmer_seq=[bytes(rnd.choice(b"ACGT") for _ in range(rnd.choice((5, 9, 21)))) for _ in range(rnd.randrange(1, 9))])
    else:
        pats = patterns31(mk, rnd.choice((20, 300)), seed=seed)
    m = mk.Matcher(pats, device=0)
    om = ob.Matcher(pats, m.use_ac, 0, False)
    n = rnd.choice((1, 40, 700, 2500))
    lens = rnd.choice(((150,), (0, 1, 2, 33, 150, 151), (100, 3000), (75,)))
    alpha = rnd.choice((b"ACGT", b"ACGTN", b"ACGTNRYKM"))
    hit, lower, crlf = rnd.choice((0.0, 0.1, 0.9)), rnd.choice((0.0, 0.2)), rnd.choice((0.0, 0.0, 0.5, 1.0))
    tag = rnd.choice((b"km", b"XK"))
    carry = rnd.random() < 0.5
    parts = []
    for i in range(n):
        ln = sam_line(rnd, i, pats, lens=lens, hit=hit, alpha=alpha, lower=lower, eol=b"")
        if carry and rnd.random() < 0.3 and ln.count(b"\t") >= 10:  # some lines carry the tag already
            ln += b"\t" + tag + b":Z:" + rnd.choice((b"", b"AAA", b"T,A,T", pats[0], pats[-1] + b",zz", b",", b"b,a,,c"))
        parts.append(ln + (b"\r\n" if rnd.random() < crlf else b"\n"))
        if rnd.random() < 0.02:
            parts.append(rnd.choice((b"\n", b"@CO\tx\n", b"\r\n")))
    text = b"".join(parts)
    if rnd.random() < 0.5 and text.endswith(b"\n") and not text.endswith(b"\r\n"):
        text = text[:-1]
    fm, inv = rnd.choice(((False, False), (True, False), (False, True)))
    logging = rnd.random() < 0.7
    keep, rows, c, out, n_rec = expected(om, pats, text, tag, logging, fm, inv)
    n_cuts = rnd.choice((0, 1, 5, 40))
    cuts = [0] + sorted(rnd.randrange(0, len(text) + 1) for _ in range(n_cuts)) + [len(text)]
    res = run_windows(m, text, cuts, tag=tag, logging=logging, filter_matching=fm, invert=inv)
    assert len(res) == len(cuts) - 1
    check_windows(res, keep, rows, c, out, n_rec, logging)
