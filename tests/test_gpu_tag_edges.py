"""The kernels behind `tag` (merkurio_amd/csrc/sam.hip, bam.hip) at the edges of their own geometry -- a lane's 16 bytes and a step's
256 in the line kernels, 8 / 128 in the gathers, 4 / 64 in the BAM emit, the 64 lanes of a wave, the pieces of the BAM record chain --
on the crafted lines and records of tests/tag_edge_cases.py, whose placement claims tests/test_tag_edge_cases_cpu.py proves.

Every family runs through the entry points the way the existing tests call them and is compared with their restatements: `expected` of
test_gpu_sam_window.py, `encode` of test_gpu_sam_bam_window.py, the BAM -> BAM expectation of test_gpu_bam_window.py and `sam_line` of
test_gpu_bam_sam_window.py.  The matcher holds all 256 4-mers, so the log rows spell every gathered / un-nibbled sequence back byte for
byte, and every record of four bases or more is kept and named.  Every case but the refusals asserts status == 0; nothing is skipped."""
import pytest

import oracle_binding as ob
import tag_edge_cases as tc
import test_gpu_bam_sam_window as tbs
import test_gpu_bam_window as tbw
import test_gpu_sam_bam_window as tsb
import test_gpu_sam_window as tsw
from tag_windows import _bgzf, inflate, records_of

pytestmark = pytest.mark.gpu
TAG = b"km"


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


@pytest.fixture(scope="module")
def env(mk):
    """the matcher over all 4-mers, the oracle's, a codec"""
    pats = mk.parse_pattern_list(kmer_seq=tc.kmers4())
    m, codec = mk.Matcher(pats, device=0), mk.Codec(0)
    yield dict(mk=mk, pats=pats, m=m, om=ob.Matcher(pats, m.use_ac, 0, False), codec=codec)
    codec.close()


def counters_equal(got, want, n_kept):
    got, want = dict(got), dict(want)
    assert got.pop("extracted") == n_kept
    want.pop("extracted")
    assert got == want


def rows_spell(rows, pats, names, seqs):
    """the rows name their records by QNAME and spell the upper-cased sequences, with gaps exactly where a byte is no plain base"""
    assert all(nm == names[rec] for nm, rec, _, _ in rows)
    assert tc.spell_back(rows, pats, [len(s) for s in seqs]) == [tc.spelled(s) for s in seqs]


def check_sam(env, text, last=True, fm=False, bam_bits=None):
    """one window of SAM text through SAM -> SAM and SAM -> BAM (bam_bits: the refusal SAM -> BAM must answer with instead)"""
    m, om, pats, codec = env["m"], env["om"], env["pats"], env["codec"]
    recs, used = records_of(text, last)
    keep, rows, c, out, n_rec = tsw.expected(om, pats, text, TAG, True, fm, False, last)
    assert n_rec == len(recs)
    r = m.tag_sam_window(b"", text, last=last, filter_matching=fm)
    tsw.check_windows([r], keep, rows, c, out, n_rec, True)
    assert r["n_window"] == len(text) and r["n_used"] == used and r["tail"] == text[used:] and r["n_kept"] == sum(keep)
    counters_equal(r["counters"], c, sum(keep))
    rows_spell(r["rows"], pats, [x[1] for x in recs], [x[2] for x in recs])
    b = m.tag_sam_bam_window(codec, b"", text, last=last, refs=tsb.REFS, filter_matching=fm)
    if bam_bits is not None:
        assert b["status"] == bam_bits and b["out"] == b"" and b["n_kept"] == 0 and b["counters"]["records"] == 0
        return r
    keep2, rows2, c2, out2, n_rec2 = tsb.expected(om, pats, text, TAG, True, fm, False, last=last)
    tsb.check([b], keep2, rows2, c2, out2, n_rec2, True)
    assert b["n_used"] == used and b["tail"] == text[used:] and b["n_rec"] == n_rec and keep2 == keep
    counters_equal(b["counters"], c2, sum(keep))
    rows_spell(b["rows"], pats, [x[1] for x in recs], [x[2] for x in recs])
    return r


def check_sam_family(env, items, **kw):
    """the family as one window; once more without its last line end, as the whole text (last) and with more to follow"""
    text = tc.text_of(items)
    check_sam(env, text, **kw)
    cut = text[:-2] if text.endswith(b"\r\n") else text[:-1]
    r = check_sam(env, cut, last=True, **kw)
    assert r["tail"] == b""
    r = check_sam(env, cut, last=False, **kw)
    assert r["tail"] == cut[cut.rfind(b"\n") + 1:] != b""


def test_sam_tab_placement(env):
    check_sam_family(env, tc.sam_tab_family())


def test_sam_tab_placement_in_windows(env):
    """the same text cut into windows at every line start and one byte inside every fifth line, the tail carried as head"""
    items = tc.sam_tab_family()
    text = tc.text_of(items)
    cuts, at = [], 0
    for k, (ln, eol, _) in enumerate(items):
        cuts.append(at)
        if k % 5 == 0:
            cuts.append(at + 1)
        at += len(ln) + len(eol)
    cuts.append(len(text))
    m, om, pats, codec = env["m"], env["om"], env["pats"], env["codec"]
    keep, rows, c, out, n_rec = tsw.expected(om, pats, text, TAG, True, False, False)
    res = tsw.run_windows(m, text, cuts, logging=True)
    assert len(res) == len(cuts) - 1
    tsw.check_windows(res, keep, rows, c, out, n_rec, True)
    keep, rows, c, out, n_rec = tsb.expected(om, pats, text, TAG, True, False, False)
    res = tsb.run_windows(m, codec, text, cuts, refs=tsb.REFS)
    assert len(res) == len(cuts) - 1
    tsb.check(res, keep, rows, c, out, n_rec, True)


def test_sam_qname_longer_than_a_step(env):
    check_sam_family(env, tc.sam_long_qname_family(), bam_bits=2)


def test_sam_wanted_tabs_in_one_lane(env):
    items = tc.sam_lane_family()
    check_sam_family(env, items)
    check_sam(env, tc.text_of(items), fm=True)  # (SEQ '*' and 'A' have no 4-mer: mixed hits)


def test_sam_lines_only_sam_to_sam_takes(env):
    items, bits = tc.sam_odd_family()
    check_sam_family(env, items, bam_bits=bits)
    for kind, bit in (("ten", 1), ("many", 2), ("crowded", 2), ("end-tab", 2)):
        check_sam(env, tc.text_of([x for x in items if x[2]["kind"] == kind]), bam_bits=bit)
    short, bits = tc.sam_short_tag_family()
    check_sam_family(env, short, bam_bits=bits)


def test_sam_line_lengths(env):
    check_sam_family(env, tc.sam_length_family())


@pytest.mark.parametrize("group", [range(0, 4), range(4, 8), range(8, 12), range(12, 16)], ids=lambda g: "align%d-%d" % (g[0], g[-1]))
def test_sam_seq_lengths_and_alignments(env, group):
    check_sam(env, tc.text_of(tc.sam_seq_family(group)))


def test_sam_seq_case_and_confounders(env):
    items = tc.sam_case_family()
    check_sam_family(env, items)
    # SAM -> BAM: a confounder is nibble 15 ('N'), its neighbours a / z are 'A' and nibble 15
    b = env["m"].tag_sam_bam_window(env["codec"], b"", tc.text_of(items), last=True, refs=tsb.REFS)
    got, _ = tbw.split_records(inflate(b["out"]))
    assert b["status"] == 0 and len(got) == len(items)
    for rec, (_, _, d) in zip(got, items):
        if d["kind"] == "confounder":
            assert tbw.decode(rec)[1][d["at"] - 1:d["at"] + 2] == b"ANN"


def test_sam_existing_tag_field(env):
    items = tc.sam_existing_family()
    check_sam_family(env, items)
    check_sam(env, tc.text_of(items), fm=True)
    r = env["m"].tag_sam_window(b"", tc.text_of(items), last=True)
    lines = r["out"].split(b"\n")[:-1]
    assert len(lines) == len(items)
    for ln, (_, _, d) in zip(lines, items):  # the merged value holds the items of the first field of the name
        new = ln.split(b"\t")[-1]
        assert new.startswith(b"km:Z:") and all(v in new[5:].split(b",") for v in d["value"].split(b",") if d["value"])


def test_sam_refusals(env):
    m, codec = env["m"], env["codec"]
    for name, (text, status) in tc.sam_refusal_texts().items():
        r = m.tag_sam_window(b"", text, last=True)
        assert r["status"] == status and r["out"] == b"" and r["counters"]["records"] == 0, name
        b = m.tag_sam_bam_window(codec, b"", text, last=True, refs=tsb.REFS)
        assert b["status"] == status and b["out"] == b"" and b["counters"]["records"] == 0, name


def test_sam_record_counts_and_compaction(env):
    for name, (items, n) in tc.sam_count_texts().items():
        text = tc.text_of(items)
        for fm in (False, True):
            r = check_sam(env, text, fm=fm)
            assert r["n_rec"] == n, name


def test_sam_length_statistics(env):
    for name, (items, n, where) in tc.sam_stats_texts().items():
        r = check_sam(env, tc.text_of(items))
        assert r["n_rec"] == n, name


# ---- BAM ---------------------------------------------------------------------------------------------------------------------------
def check_bam(env, recs, existing=None, piece=0, fm=False, block=0xff00):
    """one window of BAM records through BAM -> BAM and BAM -> SAM"""
    mk, m, om, pats, codec = env["mk"], env["m"], env["om"], env["pats"], env["codec"]
    text, blob, members = tbs.window(mk, recs, block)
    dec = [tbw.decode(x) for x in recs]
    keep, rows, c, out = tbw.expected(om, pats, recs, TAG, True, fm, False, existing)
    r = m.tag_bam_window(codec, b"", blob, members, last=True, filter_matching=fm, piece_bytes=piece)
    assert r["status"] == 0 and r["n_rec"] == len(recs) and r["n_used"] == len(text) and r["tail"] == b""
    assert r["n_kept"] == sum(keep) and r["out_text_bytes"] == len(out) and inflate(r["out"]) == out
    assert r["rows"] == rows
    counters_equal(r["counters"], c, sum(keep))
    rows_spell(r["rows"], pats, [d[0] for d in dec], [d[1] for d in dec])
    keep2, rows2, c2, out2 = tbs.expected(om, pats, recs, tbs.REFS, TAG, True, fm, False, existing)
    s = m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=tbs.REFS, filter_matching=fm, piece_bytes=piece)
    assert s["n_rec"] == len(recs) and s["n_used"] == len(text) and s["tail"] == b""
    tbs.check(s, keep2, rows2, c2, out2)
    rows_spell(s["rows"], pats, [d[0] for d in dec], [d[1] for d in dec])


def test_bam_every_l_seq(env):
    recs = [r for r, _ in tc.bam_lseq_family()]
    check_bam(env, recs)
    check_bam(env, recs, fm=True, piece=256)


def test_bam_record_lengths(env):
    check_bam(env, [r for r, _ in tc.bam_length_family()])


def test_bam_length_statistics(env):
    """(not a wave-edge case: the BAM statistics are reduced over the pieces' lanes) the fixed-length and the offsets layout of the scan
    buffer in mk_bam_unpack_kernel, one record of another length first, last and in between"""
    for name, (recs, where) in tc.bam_stats_records().items():
        check_bam(env, recs)
        check_bam(env, recs, piece=256)  # (one lane a piece, at most 59 pieces: one wave sees them all, the odd record is one lane's alone)


@pytest.mark.parametrize("piece", [256, 4096])
def test_bam_record_starts_at_piece_edges(env, piece):
    recs, placed, total = tc.bam_piece_records(piece, 20, span3_at=8)
    check_bam(env, recs, piece=piece)


@pytest.mark.parametrize("count", [63, 64, 65, 129])
def test_bam_piece_counts(env, count):
    recs, total = tc.bam_piece_count_records(256, count)
    check_bam(env, recs, piece=256)


@pytest.mark.parametrize("piece", [256, 4096])
def test_bam_windows_that_end_inside_a_record(env, piece):
    """the members are cut so that the first window's text ends 1 ... 37 bytes into a record: those bytes are the tail, and the next
    window, given them as its head, continues the chain"""
    mk, m, om, pats, codec = env["mk"], env["m"], env["om"], env["pats"], env["codec"]
    recs, placed, total = tc.bam_piece_records(piece, 24)
    text = b"".join(recs)
    keep, rows, c, out = tbw.expected(om, pats, recs, TAG, True, False, False)
    keep2, rows2, c2, out2 = tbs.expected(om, pats, recs, tbs.REFS, TAG, True, False, False)
    starts = [0]
    for x in recs:
        starts.append(starts[-1] + len(x))
    for cut, k, d in tc.bam_cut_cases(recs, placed):
        first, second = _bgzf(text[:cut]), _bgzf(text[cut:])
        blob = first + second
        members, used, tb = mk.bgzf_members(blob)
        n1 = len(mk.bgzf_members(first)[0])
        assert used == len(blob) and tb == len(text)
        a = m.tag_bam_window(codec, b"", blob, members[:n1], last=False, piece_bytes=piece)
        assert a["status"] == 0 and a["n_rec"] == k and a["n_used"] == starts[k] and a["tail"] == text[starts[k]:cut] and len(a["tail"]) == d
        z = m.tag_bam_window(codec, a["tail"], blob, members[n1:], last=True, piece_bytes=piece)
        assert z["status"] == 0 and z["n_rec"] == len(recs) - k and z["tail"] == b"" and z["n_used"] == len(text) - starts[k]
        assert inflate(a["out"]) + inflate(z["out"]) == out
        assert a["rows"] + [(nm, rec + k, pat, pos) for nm, rec, pat, pos in z["rows"]] == rows
        assert a["counters"]["records"] + z["counters"]["records"] == len(recs)
        a = m.tag_bam_sam_window(codec, b"", blob, members[:n1], last=False, refs=tbs.REFS, piece_bytes=piece)
        assert a["status"] == 0 and a["rc"] == 0 and a["n_rec"] == k and a["tail"] == text[starts[k]:cut]
        z = m.tag_bam_sam_window(codec, a["tail"], blob, members[n1:], last=True, refs=tbs.REFS, piece_bytes=piece)
        assert z["status"] == 0 and z["rc"] == 0 and z["n_rec"] == len(recs) - k and z["tail"] == b""
        assert a["out"] + z["out"] == out2


@pytest.mark.parametrize("piece", [256, 4096])
def test_bam_window_that_ends_deep_inside_a_long_record(env, piece):
    """the unfinished record starts twelve pieces in front of the text's end: it is the tail, the window is taken, the next one goes on"""
    mk, m, om, pats, codec = env["mk"], env["m"], env["om"], env["pats"], env["codec"]
    recs, k, cut = tc.bam_long_tail_case(piece)
    text = b"".join(recs)
    start = sum(len(x) for x in recs[:k])
    keep, rows, c, out = tbw.expected(om, pats, recs, TAG, True, False, False)
    keep2, rows2, c2, out2 = tbs.expected(om, pats, recs, tbs.REFS, TAG, True, False, False)
    first = _bgzf(text[:cut])
    blob = first + _bgzf(text[cut:])
    members, used, tb = mk.bgzf_members(blob)
    n1 = len(mk.bgzf_members(first)[0])
    a = m.tag_bam_window(codec, b"", blob, members[:n1], last=False, piece_bytes=piece)
    assert a["status"] == 0 and a["n_rec"] == k and a["n_used"] == start and a["tail"] == text[start:cut]
    z = m.tag_bam_window(codec, a["tail"], blob, members[n1:], last=True, piece_bytes=piece)
    assert z["status"] == 0 and z["n_rec"] == len(recs) - k and z["tail"] == b""
    assert inflate(a["out"]) + inflate(z["out"]) == out
    assert a["rows"] + [(nm, rec + k, pat, pos) for nm, rec, pat, pos in z["rows"]] == rows
    a = m.tag_bam_sam_window(codec, b"", blob, members[:n1], last=False, refs=tbs.REFS, piece_bytes=piece)
    assert a["status"] == 0 and a["rc"] == 0 and a["n_rec"] == k and a["tail"] == text[start:cut]
    z = m.tag_bam_sam_window(codec, a["tail"], blob, members[n1:], last=True, refs=tbs.REFS, piece_bytes=piece)
    assert z["status"] == 0 and z["rc"] == 0 and a["out"] + z["out"] == out2


def test_bam_existing_tag_field(env):
    fam = tc.bam_existing_family()
    recs, existing = [r for r, _ in fam], [d["existing"] for _, d in fam]
    check_bam(env, recs, existing=existing)
    check_bam(env, recs, existing=existing, fm=True, piece=256)
    mk, m, codec = env["mk"], env["m"], env["codec"]
    text, blob, members = tbs.window(mk, recs[:5] + [tc.bam_over_record()] + recs[5:9])
    assert m.tag_bam_window(codec, b"", blob, members, last=True)["status"] == 4
    assert m.tag_bam_sam_window(codec, b"", blob, members, last=True, refs=tbs.REFS)["status"] == 4
