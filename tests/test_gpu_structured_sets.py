"""The scan on pattern sets with the structure of real k-mer lists (structured_sets.py) against the CPU oracle, bit-exact.

Every other GPU test draws its patterns uniformly at random: every sampled q-gram is then a key of its own, the exact table
(filter.hpp) is all but chain-free and a text sample verifies at most one entry.  The consecutive k-mers of a locus put up to
`stride` entries on one key; patterns that share a prefix put hundreds there.  That is where build_tables.hip sets overflow
flags under contention, where probe_chain walks beyond its second round, where probe_round finds several matching entries per
lane and bucket and drains the hit ring in the middle of a round, where the context kernels see entries of one key with
different masks, and where order_hits / sets / the tag kernels get a hundred tuples per record.  Every test asserts with
keys_per_entry(), at the geometry the matcher reports, that its set does stress the table, and from kernel_name that the
kernel variant it meant to run is the one that ran.  The cases here name kernel FAMILIES (a part of kernel_name) and between
them launch well under half of the compiled variants; every variant, by its exact name and on a batch with an occurrence at
every residue of the stride and a near-miss at every base, is test_gpu_scan_variants.py.  Run on the GPU box with `-m gpu`.
"""
import functools
import gzip
import random
import struct

import pytest

import naive
import oracle_binding as ob
import structured_sets as ss
import test_gpu_bam_window as bw
import test_gpu_sam_window as sw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X")
    return native


# ---------------------------------------------------------------------------- the oracle's answers, computed once per batch
class Expected:
    def __init__(self, patterns, use_ac, recs, ci=False):
        om = ob.Matcher(patterns, use_ac, 0, ci)
        assert om.rc == 0
        _, rows, self.counters, self.found = ob.tag_records(om, recs, logging=True)
        self.tuples = [(r, p, pos) for (_, r, p, pos) in rows]
        self.flags = [bool(f) for f in self.found]
        self.sets = [sorted(set(f)) for f in self.found]
        self.single = {lg: ob.extract_single(om, recs, logging=lg, invert=False) for lg in (True, False)}
        h = len(recs) // 2
        self.paired = ob.extract_paired(om, recs[:h], recs[h:2 * h], logging=True, invert=True)


_EXPECTED = {}


def _expected(key, patterns, use_ac, recs, ci=False):
    k = (key, bool(use_ac), ci)
    if k not in _EXPECTED:
        _EXPECTED[k] = (patterns, Expected(patterns, use_ac, recs, ci))
    assert _EXPECTED[k][0] == patterns
    return _EXPECTED[k][1]


def _same(got, exp, what):
    """got == exp for long lists, with a failure message that names the first difference (not a diff of 100 000 tuples)"""
    if got == exp:
        return
    k = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    raise AssertionError(f"{what}: {len(got)} items, the oracle has {len(exp)}; first difference at {k}: "
                         f"{got[k:k + 3]} against {exp[k:k + 3]}")


def _tuples(hits):
    return list(zip(hits["rec"].tolist(), hits["pat"].tolist(), hits["pos"].tolist()))


def _family(m, gf=False):
    """the kernel family of the main class's geometry (scan_kernel.hip: launch_scan)"""
    info = m.filter_info()
    S, q = info["stride"], info["q_gram"]
    fixed = ((8, 14), (4, 18), (8, 24)) if gf else ((16, 16), (8, 24), (4, 28), (4, 18))
    two = m.class_info()["split_len"] != 0
    qc = q if (S, q) in fixed and not (gf and two) else (0 if q <= 16 else -1)
    return f"<{S},{qc},"


def _check_kernel(m, family, gf=False, two_class=False):
    name = m.kernel_name
    assert family == _family(m, gf) and family in name, (family, _family(m, gf), name)
    assert name.split(",")[3].startswith("true" if gf else "false"), name
    assert name.endswith("2-class>") == two_class, name
    assert m.filter_mode()["in_lds"] is (not gf)


def _main_patterns(m, patterns):
    return [p for p in patterns if len(p) >= m.class_info()["split_len"]]


def _assert_tiled_precondition(m, patterns):
    """consecutive k-mers: a key carries `stride` entries; from stride 8 on that is more than a bucket holds"""
    info = m.filter_info()
    q, S = info["q_gram"], info["stride"]
    main = _main_patterns(m, patterns)
    assert ss.max_entries_on_a_key(main, q, S) >= min(S, len(main)), (q, S)
    if S >= 8:
        share = ss.overflowing_share(main, q, S)
        assert share >= 0.5, f"only {share:.2f} of the keys carry more than {ss.BUCKET_ENTRIES} entries at q = {q}, S = {S}"


def _check_against_oracle(mk, m, e, recs, what=""):
    """the shape of test_gpu_parity.test_scan_matches_oracle: tuples in emission order, flags of both modes, tag_records,
    extract_single with and without logging, extract_paired on the two halves"""
    flags, hits = m.scan(recs, mk.MK_MODE_HITS, hits_cap=len(e.tuples) + 16)
    path = m.order_info()["path"]
    _same(_tuples(hits), e.tuples, f"{what} tuples ({m.kernel_name}, order path {path})")
    _same(flags.tolist(), e.flags, f"{what} flags of MK_MODE_HITS")
    flags_any, _ = m.scan(recs, mk.MK_MODE_ANY)
    _same(flags_any.tolist(), e.flags, f"{what} flags of MK_MODE_ANY ({m.kernel_name})")
    keep, rows, c, found = m.tag_records(recs, logging=True)
    assert c == e.counters, what
    _same(found, e.sets, f"{what} found sets")
    _same([(r, p, pos) for (_, r, p, pos) in rows], e.tuples, f"{what} tag_records rows")
    for lg in (True, False):
        k1, r1, c1 = e.single[lg]
        k2, r2, c2 = m.extract_single(recs, logging=lg, invert=False)
        _same(k2, k1, f"{what} extract_single keep, logging={lg}")
        _same(r2, r1, f"{what} extract_single rows, logging={lg}")
        assert c2 == c1, (what, lg)
    h = len(recs) // 2
    k1, r1, c1 = e.paired
    k2, r2, c2 = m.extract_paired(recs[:h], recs[h:2 * h], logging=True, invert=True)
    _same(k2, k1, f"{what} extract_paired keep")
    _same(r2, r1, f"{what} extract_paired rows")
    assert c2 == c1, what
    return path


# ---------------------------------------------------------------------------- the sets
@functools.lru_cache(maxsize=None)
def _tiled(n_loci, width, k, **kw):
    return ss.tiled(n_loci, width, k, **kw)


@functools.lru_cache(maxsize=None)
def _tiled_short(forced):
    raw, recs = _tiled(12, 100, 31, n_reads=100, long_bytes=70_000)
    # (forced short-class strides of up to 8 need short patterns of 10 bases or more: a stride never exceeds the shortest)
    return ss.with_short(raw, recs, seed=9, n=3, lengths=(10, 12)) if forced else ss.with_short(raw, recs)


# (k, loci, matcher options, pattern-list options, algorithm, case-insensitive, kernel family, filter in global memory)
TILED = [
    ("k31", 31, 40, None, {}, "auto", False, "<16,16,", False),
    ("k21", 21, 40, None, {}, "auto", False, "<8,0,", False),
    ("k31-s1", 31, 40, dict(force_stride=1), {}, "auto", False, "<1,-1,", False),
    ("k31-s2", 31, 40, dict(force_stride=2), {}, "auto", False, "<2,-1,", False),
    ("k31-s4", 31, 40, dict(force_stride=4), {}, "auto", False, "<4,28,", False),
    ("k31-s8", 31, 40, dict(force_stride=8), {}, "auto", False, "<8,24,", False),
    ("k31-s16", 31, 40, dict(force_stride=16), {}, "auto", False, "<16,16,", False),
    ("k27-wide", 27, 40, dict(force_stride=8), {}, "auto", False, "<8,-1,", False),   # runtime q = 20
    ("k19-narrow", 19, 40, None, {}, "auto", False, "<8,0,", False),                  # runtime q = 12
    ("k21-ctx-8-14", 21, 40, dict(force_global_filter=True, force_stride=8), {}, "auto", False, "<8,14,", True),
    ("k21-ctx-4-18", 21, 40, dict(force_global_filter=True, force_stride=4), {}, "auto", False, "<4,18,", True),
    ("k31-ctx-8-24", 31, 40, dict(force_global_filter=True, force_stride=8), {}, "auto", False, "<8,24,", True),
    ("k21-gf-s2", 21, 40, dict(force_global_filter=True, force_stride=2), {}, "auto", False, "<2,-1,", True),  # runtime q = 20
    ("k31-tile-run", 31, 40, dict(tile_run=4), {}, "auto", False, "<16,16,", False),
    ("k31-ac", 31, 40, None, {}, "ac", False, "<16,16,", False),
    ("k31-bndmq", 31, 1, None, {}, "bndmq", False, "<16,16,", False),                 # 13 patterns: pattern-major emission
    ("k31-rc", 31, 40, None, dict(reverse_complement=True), "auto", False, "<8,24,", False),  # -r: 8 000 patterns
    ("k31-ci", 31, 40, None, {}, "auto", True, "<16,16,", False),
]


@pytest.mark.parametrize("case", TILED, ids=[c[0] for c in TILED])
def test_tiled_set_in_every_kernel_family(mk, case):
    name, k, n_loci, options, list_kw, algo, ci, family, gf = case
    raw, recs = _tiled(n_loci, 13 if algo == "bndmq" else 100, k)
    if ci:
        recs = ss.mixed_case(recs)
    patterns = mk.parse_pattern_list(kmer_seq=raw, **list_kw)
    rc, opats = ob.parse_pattern_list(raw, **list_kw)
    assert rc == 0 and patterns == opats
    m = mk.Matcher(patterns, algo={"auto": mk.MK_ALGO_AUTO, "ac": mk.MK_ALGO_AC, "bndmq": mk.MK_ALGO_BNDMQ}[algo],
                   case_insensitive=ci, options=options)
    assert m.use_ac == (algo != "bndmq") and (algo != "bndmq" or len(patterns) <= 13)
    _assert_tiled_precondition(m, patterns)
    e = _expected(("tiled", n_loci, k, tuple(sorted(list_kw)), ci), patterns, m.use_ac, recs, ci)
    assert len(e.tuples) > 10 * len(recs) or algo == "bndmq"  # a read of a locus matches dozens of patterns, not one
    assert max(len(s) for s in e.sets) >= (13 if algo == "bndmq" else 100)
    assert len(recs[-1]) > 4 * 31744  # the long record crosses several tile borders
    _check_against_oracle(mk, m, e, recs, name)
    _check_kernel(m, family, gf)


def test_tiled_set_in_both_load_flavours(mk):
    """the kernels for hit-dense text (plain stream loads, 16-byte loads at level 3) and for sparse hits walk the same chains"""
    raw, recs = _tiled(40, 100, 31)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    e = _expected(("tiled", 40, 31, (), False), patterns, True, recs)
    for options, family in ((None, "<16,16,"), (dict(force_stride=8), "<8,24,"), (dict(force_stride=2), "<2,-1,")):
        m = mk.Matcher(patterns, options=options)
        _assert_tiled_precondition(m, patterns)
        names = set()
        for density in (0, 1000):
            for mode in (mk.MK_MODE_HITS, mk.MK_MODE_ANY):
                m.hint_hit_density(density)  # mk_scan_batch replaces it with what the batch showed: set before each scan
                flags, hits = m.scan(recs, mode, hits_cap=len(e.tuples) + 16)  # one launch: no capacity retry
                names.add(m.kernel_name)
                assert family in m.kernel_name
                _same(flags.tolist(), e.flags, f"flags, density {density}, mode {mode}")
                if mode == mk.MK_MODE_HITS:
                    _same(_tuples(hits), e.tuples, f"tuples, density {density} ({m.kernel_name})")
        assert len(names) == 4 and sum(n.endswith("plain>") for n in names) == 2, names


# ---------------------------------------------------------------------------- two length classes
def _check_short_inside_long(patterns, recs, e, split_len):
    """a short pattern that is a substring of long ones: once per occurrence, at positions inside the long occurrences"""
    shorts = [i for i, p in enumerate(patterns) if len(p) < split_len]
    assert shorts
    per_pat = {i: 0 for i in shorts}
    long_spans = {}
    for r, p, pos in e.tuples:
        if p in per_pat:
            per_pat[p] += 1
        else:
            long_spans.setdefault(r, []).append((pos, pos + len(patterns[p])))
    for i in shorts:
        assert per_pat[i] == sum(len(naive.occurrences(patterns[i], r)) for r in recs), patterns[i]
    # the long record holds every locus once, so every short pattern lies at least once inside an occurrence of the pattern
    # it was cut from
    inside = {i: 0 for i in shorts}
    for r, p, pos in e.tuples:
        if p in inside and any(a <= pos and pos + len(patterns[p]) <= b for a, b in long_spans.get(r, ())):
            inside[p] += 1
    assert all(n >= 1 for n in inside.values()), inside


# (name, short-class options forced, matcher options, kernel family of the main class)
CLASSES = [("rule", False, None, "<16,16,"), ("rule-global-filter", False, dict(force_global_filter=True), "<16,0,")]
CLASSES += [(f"s2={s2}-q2={q2}", True, dict(length_classes=2, force_split_len=31, force_stride2=s2, force_q2=q2), "<16,16,")
            for s2 in (1, 2, 4, 8) for q2 in (0, 6, 8)]
CLASSES += [("s2=4-global-filter", True, dict(length_classes=2, force_split_len=31, force_stride2=4, force_global_filter=True, force_stride=8),
             "<8,-1,")]  # (two classes next to a global filter: the runtime-q kernels, q = 24)


@pytest.mark.parametrize("case", CLASSES, ids=[c[0] for c in CLASSES])
def test_short_patterns_cut_out_of_the_tiled_ones(mk, case):
    name, forced, options, family = case
    raw, recs = _tiled_short(forced)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    m = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=options)
    ci = m.class_info()
    n_short = sum(len(p) < 31 for p in patterns)
    assert ci["split_len"] == 31 and ci["n_short"] == n_short and 1 <= n_short <= 5, ci
    if forced:
        assert ci["stride2"] == options["force_stride2"], ci
    _assert_tiled_precondition(m, patterns)
    e = _expected(("short", forced), patterns, True, recs)
    _check_short_inside_long(patterns, recs, e, 31)
    _check_against_oracle(mk, m, e, recs, name)
    gf = bool(options and options.get("force_global_filter"))
    _check_kernel(m, family, gf, two_class=True)
    if "s2=" in m.kernel_name:  # the byte-table short class with its stride compiled in
        assert f"s2={ci['stride2']}," in m.kernel_name and ci["q_gram2"] <= 6, (m.kernel_name, ci)


# ---------------------------------------------------------------------------- shared prefixes, repeats, code collisions
N_GROUP = 400  # patterns per shared prefix (the issue's bound: 500), 160 planted occurrences of a prefix in the batch (bound: 200)
STRIDE_IDS = ["default", "s16", "s1"]
# (matcher options, the kernel family they must lead to) per set
PREFIX_STRIDES = [(None, "<16,16,"), (dict(force_stride=16), "<16,0,"), (dict(force_stride=1), "<1,-1,")]    # q = 16 (main class), 5, 20
REPEAT_STRIDES = [(None, "<16,16,"), (dict(force_stride=16), "<16,16,"), (dict(force_stride=1), "<1,-1,")]  # q = 16, 16, 31
COLLISION_STRIDES = {
    "dna": [(None, "<16,16,"), (dict(force_stride=16), "<16,16,"), (dict(force_stride=1), "<1,-1,")],
    # 12-mers admit no stride 16: the largest they do admit takes its place (q = 9 at the rule's stride 4, 5, 12)
    "protein": [(None, "<4,0,"), (dict(force_stride=8), "<8,0,"), (dict(force_stride=1), "<1,0,")],
}


def _forced_stride(m, options):
    if options:
        assert m.filter_info()["stride"] == options["force_stride"]


@pytest.mark.parametrize("options,family", PREFIX_STRIDES, ids=STRIDE_IDS)
def test_patterns_that_share_a_prefix(mk, options, family):
    raw, recs = ss.shared_prefix(N_GROUP)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    assert len(patterns) == 2 * N_GROUP
    m = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=options)
    _forced_stride(m, options)
    info = m.filter_info()
    most = ss.max_entries_on_a_key(_main_patterns(m, patterns), info["q_gram"], info["stride"])
    assert most >= N_GROUP, (most, info, m.class_info())  # the group with the 31-base prefix: all on its offset-0 key
    e = _expected(("prefix",), patterns, True, recs)
    assert sum(e.flags) >= 100
    _check_against_oracle(mk, m, e, recs, "prefix")
    # (by the rule the bare 20-base prefix is a short class of its own; a forced stride means one class)
    assert (m.class_info()["split_len"] != 0) == (options is None), m.class_info()
    _check_kernel(m, family, two_class=options is None)


@pytest.mark.parametrize("options,family", REPEAT_STRIDES, ids=STRIDE_IDS)
def test_repeats_and_microsatellites(mk, options, family):
    raw, recs = ss.repeats()
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    m = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=options)
    _forced_stride(m, options)
    info = m.filter_info()
    q, S = info["q_gram"], info["stride"]
    assert any(len(set(ss.pattern_keys(p, q, S))) == 1 for p in patterns)  # a homopolymer: all S entries on one key
    e = _expected(("repeats",), patterns, True, recs)
    assert len(e.tuples) >= len(recs[-1]) - 31  # the period-2 record: a tuple at nearly every position
    path = _check_against_oracle(mk, m, e, recs, "repeats")
    _check_kernel(m, family)
    # the default capacity: MK_E_CAPACITY, then the retry with the count the scan reported
    flags, hits = m.scan(recs, mk.MK_MODE_HITS)
    _same(_tuples(hits), e.tuples, f"repeats tuples after the capacity retry (order path {path} before, {m.order_info()['path']} now)")
    with pytest.raises(mk.MerkurioError) as err:
        m.scan(recs, mk.MK_MODE_HITS, hits_cap=len(e.tuples) - 1)
    assert err.value.code == mk.MK_E_CAPACITY


@pytest.mark.parametrize("kind,options,family", [(k, o, f) for k in ("dna", "protein") for o, f in COLLISION_STRIDES[k]],
                         ids=[f"{k}-{i}" for k in ("dna", "protein") for i in STRIDE_IDS])
def test_letters_that_share_a_code(mk, kind, options, family):
    """G / N, T / U, A / Y, C / R (and the 20 amino acids on 4 codes): patterns that differ only in such letters are one key
    and level 3 alone tells them apart"""
    raw, recs = ss.code_collisions(kind)
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    m = mk.Matcher(patterns, algo=mk.MK_ALGO_AC, options=options)
    _forced_stride(m, options)
    info = m.filter_info()
    q, S = info["q_gram"], info["stride"]
    spellings = {}
    for p in patterns:
        for o in range(S):
            spellings.setdefault(ss.pack_qgram(p, o, q), set()).add(p[o:o + q])
    assert sum(len(v) > 1 for v in spellings.values()) >= 20  # keys that several spellings of a q-gram share
    e = _expected(("collisions", kind), patterns, True, recs)
    assert sum(e.flags) >= 50 and not all(e.flags)
    _check_against_oracle(mk, m, e, recs, kind)
    _check_kernel(m, family)


# ---------------------------------------------------------------------------- a hundred tuples per record downstream
@functools.lru_cache(maxsize=None)
def _locus_reads():
    """reads of 200 bases that cover the 100 tiled 31-mers of their locus, the same with one base changed, random reads"""
    return ss.tiled(6, 100, 31, seed=7, n_reads=80, read_len=200, flank=60, long_bytes=0)


def _existing_values(rnd, raw, n):
    """every third record carries the tag already: a shuffled subset of 60 of the tiled k-mers (1 919 bytes: merged on the
    device with the hundred found patterns)"""
    return [b",".join(rnd.sample(raw, 60)) if i % 3 == 0 else None for i in range(n)]


FLAGS = [(False, False), (True, False), (False, True)]


@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "existing-tag"])
def test_bam_window_with_values_of_a_hundred_patterns(mk, carry):
    raw, seqs = _locus_reads()
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    rnd = random.Random(21)
    existing = _existing_values(rnd, raw, len(seqs)) if carry else [None] * len(seqs)
    recs = [bw.bam_record(b"read%d" % i, s, aux=b"NMC\x01" + (b"kmZ" + v + b"\0" if v else b"") + b"ASi" + struct.pack("<i", i))
            for i, (s, v) in enumerate(zip(seqs, existing))]
    blob = bw._bgzf(b"".join(recs))
    members, used, _ = mk.bgzf_members(blob)
    assert used == len(blob)
    m, codec = mk.Matcher(patterns, device=0), mk.Codec(0)
    _assert_tiled_precondition(m, patterns)
    om = ob.Matcher(patterns, True, 0, False)
    _, _, _, found = ob.tag_records(om, seqs, logging=False)
    assert sum(len(set(f)) >= 100 for f in found) >= 80
    assert max(len(ob.tag_value(patterns, f)) for f in found) > 3000  # values of several KB
    for fm, inv in FLAGS:
        for logging in (True, False):
            keep, rows, c, out = bw.expected(om, patterns, recs, b"km", logging, fm, inv, existing=existing)
            r = m.tag_bam_window(codec, b"", blob, members, last=True, logging=logging, filter_matching=fm, invert=inv)
            assert r["status"] == 0 and r["n_rec"] == len(recs) and r["n_kept"] == sum(keep), (fm, inv, logging, r["status"])
            got = gzip.decompress(r["out"] + mk.bgzf_eof()) if r["out"] else b""
            if got != out:  # (which record differs, for the failure message)
                a, _ = bw.split_records(got)
                b, _ = bw.split_records(out)
                bad = [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:3]
                raise AssertionError(f"{(fm, inv, logging)}: records {bad} of {len(a)} / {len(b)}: {[(a[k][-80:], b[k][-80:]) for k in bad]}")
            if logging:
                _same(r["rows"], rows, f"rows {(fm, inv)}")
                assert r["counters"]["pattern_hit_counts"] == c["pattern_hit_counts"] and r["counters"]["hits"] == c["hits"]
                assert r["counters"]["records_hit"] == c["records_hit"]
            _check_kernel(m, "<16,16,")  # the window's scan ran the tiled set's kernel family
    if carry:  # a value just above kBamMergeBytes (2 048): the window is handed back (status 4, no output), as test_refusals has it
        over = b",".join(raw[:64]) + b",A"
        assert len(over) == 2049
        recs[0] = bw.bam_record(b"over", seqs[0], aux=b"kmZ" + over + b"\0")
        blob = bw._bgzf(b"".join(recs))
        members, _, _ = mk.bgzf_members(blob)
        r = m.tag_bam_window(codec, b"", blob, members, last=True)
        assert r["status"] == 4 and r["out"] == b""
    codec.close()


@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "existing-tag"])
def test_sam_window_with_values_of_a_hundred_patterns(mk, carry):
    raw, seqs = _locus_reads()
    patterns = mk.parse_pattern_list(kmer_seq=raw)
    rnd = random.Random(22)
    existing = _existing_values(rnd, raw, len(seqs)) if carry else [None] * len(seqs)
    lines = []
    for i, (s, v) in enumerate(zip(seqs, existing)):
        # (the builder plants a "pattern" of the record's own length at offset 0: the line's SEQ is s)
        ln = sw.sam_line(rnd, i, [s], lens=(len(s),), hit=2.0, aux_kinds=False, eol=b"")
        assert ln.split(b"\t")[9] == s
        lines.append(ln + b"\tNM:i:1" + (b"\tkm:Z:" + v if v else b"") + b"\tAS:i:%d\n" % i)
    text = b"".join(lines)
    m = mk.Matcher(patterns, device=0)
    _assert_tiled_precondition(m, patterns)
    om = ob.Matcher(patterns, True, 0, False)
    _, _, _, found = ob.tag_records(om, seqs, logging=False)
    assert sum(len(set(f)) >= 100 for f in found) >= 80
    for fm, inv in FLAGS:
        for logging in (True, False):
            keep, rows, c, out, n_rec = sw.expected(om, patterns, text, b"km", logging, fm, inv)
            r = m.tag_sam_window(b"", text, last=True, logging=logging, filter_matching=fm, invert=inv)
            assert r["status"] == 0 and r["n_rec"] == n_rec == len(seqs) and r["n_kept"] == sum(keep), (fm, inv, logging, r["status"])
            if r["out"] != out:  # (which line differs, for the failure message)
                a, b = r["out"].split(b"\n"), out.split(b"\n")
                bad = [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:3]
                raise AssertionError(f"{(fm, inv, logging)}: lines {bad} of {len(a)} / {len(b)}: {[(a[k][-90:], b[k][-90:]) for k in bad]}")
            if logging:
                sw.check_windows([r], keep, rows, c, out, n_rec, True)
            _check_kernel(m, "<16,16,")  # the window's scan ran the tiled set's kernel family
    if carry:
        over = b",".join(raw[:64]) + b",A"
        assert len(over) == 2049
        line = b"\t".join(lines[0].split(b"\t")[:11]) + b"\tkm:Z:" + over + b"\n"
        r = m.tag_sam_window(b"", line + text, last=True)
        assert r["status"] == 4 and r["out"] == b""
