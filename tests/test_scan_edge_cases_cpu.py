"""Every batch of tests/scan_edge_cases.py, before a kernel sees it: the naive enumerator and the oracle's BNDMq loop give exactly
the flags and tuples that were planted, every span holds the number of flagged records it was asked for, and no text is longer
than 2 MiB.  Every case the GPU files use is registered there and checked here, none sampled."""
import pytest

import naive
import oracle_binding as ob
import scan_edge_cases as sc


def _asked(case):
    out = []
    for sp in case.spans:
        inside = sum(1 for r in range(len(case.records)) if case.offsets[r] >= sp.start and case.offsets[r + 1] <= sp.end)
        out.append(inside if sp.F is None else sp.F)
    return out


def test_registry_holds_what_the_gpu_files_use():
    names = set(sc.all_case_names())
    used = set(sc.SWEEP_CASES) | set(sc.EDGE_CASES_2CLASS) | set(sc.WIDE_CASES) | set(sc.TUPLE_CASES) | {sc.TUPLE_CAP_CASE}
    used |= {n for v in sc.EDGE_CASES.values() for n in v} | set(sc.SEVERAL_CASES.values()) | set(sc.HISTORY_CASES.values())
    assert used == names
    assert len(sc.SWEEP_CASES) == 129 and all(f"-{F}-" in n for F, n in zip(sc.F_SWEEP, sc.SWEEP_CASES))
    for kind in sc.KINDS:
        got = {n.split("-")[3] for n in sc.EDGE_CASES[kind]}
        assert got == {"0", "1", "2047", "2048", "2049", "2111", "2112", "2113", "all"}, got


@pytest.mark.parametrize("name", sc.all_case_names())
def test_case_is_what_it_says(name):
    c = sc.case(name)
    text_bytes = sum(len(r) for r in c.records)
    assert text_bytes <= sc.TEXT_MAX and text_bytes == c.offsets[-1]
    if c.rec_len == "ragged":
        assert {len(r) for r in c.records} == set(range(6, 15))
    else:
        assert {len(r) for r in c.records} == {c.rec_len} and c.rec_len in (8, 12, sc.WIDE_REC_LEN)
    # the naive enumerator, record by record
    tuples = [(r, p, pos) for r, rec in enumerate(c.records) for p, pos in naive.bndmq_order(c.patterns, rec)]
    assert tuples == c.tuples
    assert [bool(naive.ac_order(c.patterns, rec)) for rec in c.records] == c.flags
    # the oracle's loops
    om = ob.Matcher(c.patterns, False, 0, False)
    assert om.rc == 0
    _, rows, counters, found = ob.tag_records(om, c.records, logging=True)
    assert [(r, p, pos) for (_, r, p, pos) in rows] == c.tuples
    assert [bool(f) for f in found] == c.flags
    assert counters["records_hit"][0] == sum(c.flags) and counters["hits"][0] == len(c.tuples)
    # the spans hold what was asked for, and nothing is flagged outside them (the straddler of the several-wave cases apart)
    counts = sc.span_counts(c)
    assert [f for f, _ in counts] == _asked(c), (counts, _asked(c))
    by_hand = 1 if name.startswith("several-") else 0
    assert sum(f for f, _ in counts) + by_hand == sum(c.flags)
    for sp, (f, t) in zip(c.spans, counts):
        assert t == f * sp.per_hit


def test_tuple_cases_stage_the_totals_they_name():
    for name in sc.TUPLE_CASES:
        T = int(name.split("-")[1])
        assert len(sc.case(name).tuples) == T
    assert sc.TUPLE_TOTALS[0] <= sc.STAGE_EDGE - 65 and sc.TUPLE_TOTALS[-1] >= sc.STAGE_EDGE + 128


def test_placements():
    c = sc.case("one-tile-fixed8-2048-clustered")
    hit = [r for r, f in enumerate(c.flags) if f]
    runs, n = [], 1
    for a, b in zip(hit, hit[1:]):
        if b == a + 1:
            n += 1
        else:
            runs.append(n)
            n = 1
    runs.append(n)
    assert min(runs[:-1]) >= 64 and sum(runs) == 2048, runs
    c = sc.case("several-fixed12")
    starts = [c.offsets[r] for r, f in enumerate(c.flags) if f and 3 * sc.TILE + sc.MARGIN <= c.offsets[r] < 4 * sc.TILE - sc.MARGIN - 12]
    assert len(starts) == 70 and all(b - a >= 64 for a, b in zip(starts, starts[1:]))
    # the straddler: an occurrence that begins in tile 3 and ends in tile 4, in a record that does the same
    r = next(r for r in range(len(c.records)) if c.offsets[r] < sc.SEVERAL_STRADDLE < c.offsets[r + 1])
    pos = [c.offsets[rr] + p for rr, _, p in c.tuples if rr == r]
    assert c.flags[r] and pos == [sc.SEVERAL_STRADDLE - 2]
