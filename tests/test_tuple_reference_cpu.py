"""tuple_reference.py (numpy) against the C oracle and the naive enumerator, on small batches: the evidence that the numpy rules
are the reference's rules before test_gpu_sets.py uses them to judge the kernels of sets.hip on batches of millions of tuples.
Every output is compared: tuples in both emission orders, pattern sets, both kinds of pattern_hit_counts, keep flags, counters,
and the paired rows and counts in both pair orders.  No GPU."""
import random

import numpy as np
import pytest

import naive
import oracle_binding as ob
import tuple_reference as tr


def _patterns(rnd, n, k, extra=()):
    out = set(extra)
    while len(out) < n:
        out.add(bytes(rnd.choice(b"ACGT") for _ in range(k)))
    return sorted(out)


def _records(rnd, patterns, n, k, hit=0.5):
    """random records with planted patterns; among them empty ones, shorter than k, of exactly k, and a pattern planted several
    times and overlapping itself"""
    recs = []
    for i in range(n):
        kind = rnd.random()
        if kind < 0.08:
            recs.append(b"")
        elif kind < 0.16:
            recs.append(bytes(rnd.choice(b"ACGT") for _ in range(rnd.randrange(1, k))))
        elif kind < 0.24:
            recs.append(rnd.choice(patterns) if rnd.random() < 0.7 else bytes(rnd.choice(b"ACGT") for _ in range(k)))
        else:
            s = bytearray(rnd.choice(b"ACGTN" if rnd.random() < 0.1 else b"ACGT") for _ in range(rnd.randrange(k, 5 * k)))
            while rnd.random() < hit:
                p = rnd.choice(patterns)
                o = rnd.randrange(0, len(s) - k + 1)
                s[o:o + k] = p
            recs.append(bytes(s))
    return recs


def _homopolymer_batch(k):
    """a homopolymer pattern in homopolymer records: overlapping occurrences at every position"""
    patterns = sorted([b"A" * k, b"C" * k, b"AC" * (k // 2) + b"A" * (k % 2), b"G" * (k - 1) + b"T"])
    recs = [b"A" * (3 * k), b"", b"C" * k, b"C" * (k - 1), b"AC" * (2 * k), b"A" * k + b"C" * k + b"A" * (k + 2), b"G" * (2 * k) + b"T",
            b"a" * (2 * k), b"A" * (k - 1) + b"a" + b"A" * k]
    return patterns, recs


def _cases():
    rnd = random.Random(77)
    out = []
    for k, n_pat, n_rec in ((4, 12, 60), (5, 3, 40), (16, 40, 120), (21, 1, 50), (31, 60, 150), (32, 20, 60)):
        pats = _patterns(rnd, n_pat, k)
        out.append((f"random-k{k}", pats, _records(rnd, pats, n_rec, k)))
    for k in (3, 16, 31):
        pats, recs = _homopolymer_batch(k)
        out.append((f"homopolymer-k{k}", pats, recs))
    pats = _patterns(rnd, 5, 20)
    out.append(("all-empty", pats, [b""] * 7))
    out.append(("no-hit", pats, [b"ACGT" * 10] * 5 + [b""]))
    out.append(("one-record", pats, [pats[2] + pats[0] + pats[2]]))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def _pack(recs):
    data, off = ob.pack_records(recs)
    return data, off


def _rows_of(t):
    return list(zip([0] * len(t), t.rec.tolist(), t.pat.tolist(), t.pos.tolist()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_occurrences_are_the_naive_ones(case):
    _, patterns, recs = case
    t = tr.occurrences(*_pack(recs), patterns)
    want = sorted((r, p, pos) for r, s in enumerate(recs) for p, pat in enumerate(patterns) for pos in naive.occurrences(pat, s))
    assert sorted(zip(t.rec.tolist(), t.pat.tolist(), t.pos.tolist())) == want
    assert t.n_rec == len(recs) and t.n_bases == sum(len(s) for s in recs)
    # both orders, spelled by the naive enumerator
    ac = [(r, p, pos) for r, s in enumerate(recs) for p, pos in naive.ac_order(patterns, s)]
    bq = [(r, p, pos) for r, s in enumerate(recs) for p, pos in naive.bndmq_order(patterns, s)]
    a, b = t.ac_order(), t.bndmq_order()
    assert list(zip(a.rec.tolist(), a.pat.tolist(), a.pos.tolist())) == ac
    assert list(zip(b.rec.tolist(), b.pat.tolist(), b.pos.tolist())) == bq


@pytest.mark.parametrize("use_ac", [True, False], ids=["ac", "bndmq"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tag_records_against_the_oracle(case, use_ac):
    _, patterns, recs = case
    om = ob.Matcher(patterns, use_ac, 0, False)
    assert om.rc == 0
    t = tr.occurrences(*_pack(recs), patterns)
    found_off, found_pat = t.pattern_sets()
    for fm, inv in ((False, False), (True, False), (False, True)):
        keep, rows, c, found = ob.tag_records(om, recs, logging=True, filter_matching=fm, invert=inv)
        assert rows == _rows_of(t.emission_order(use_ac))
        sets = [sorted(set(f)) for f in found]
        assert [found_pat[int(found_off[i]):int(found_off[i + 1])].tolist() for i in range(len(recs))] == sets
        assert int(found_off[-1]) == len(found_pat) == sum(len(s) for s in sets)
        k = t.tag_keep(fm, inv)
        assert k.astype(bool).tolist() == keep
        assert dict(t.counters(k), pattern_hit_counts=t.counts(use_ac).tolist()) == c


@pytest.mark.parametrize("use_ac", [True, False], ids=["ac", "bndmq"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_extract_single_against_the_oracle(case, use_ac):
    _, patterns, recs = case
    om = ob.Matcher(patterns, use_ac, 0, False)
    t = tr.occurrences(*_pack(recs), patterns)
    for inv in (False, True):
        keep, rows, c = ob.extract_single(om, recs, logging=True, invert=inv)
        assert rows == _rows_of(t.emission_order(use_ac))
        k = t.extract_keep(inv)
        assert k.astype(bool).tolist() == keep
        assert dict(t.counters(k), pattern_hit_counts=t.counts(use_ac).tolist()) == c
        keep_quiet, _, _ = ob.extract_single(om, recs, logging=False, invert=inv)
        assert keep_quiet == keep


def _mates(case):
    """two batches of equal record count out of one case; the same pattern in both mates of some pairs, several times in mate 1"""
    _, patterns, recs = case
    h = len(recs) // 2
    r1, r2 = list(recs[:h]), list(recs[h:2 * h])
    k = len(patterns[0])
    if h >= 4:
        p = patterns[len(patterns) // 2]
        r1[0], r2[0] = p + b"N" + p + p, b"T" + p        # mate 1 three times, mate 2 once
        r1[1], r2[1] = b"", p + p                         # mate 2 only
        r1[2], r2[2] = p + patterns[0], b"ACGT"[:k - 1]   # mate 1 only
        r1[3], r2[3] = b"", b""                           # a hitless pair
    return patterns, r1, r2


@pytest.mark.parametrize("use_ac", [True, False], ids=["ac", "bndmq"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_extract_paired_against_the_oracle(case, use_ac):
    patterns, r1, r2 = _mates(case)
    om = ob.Matcher(patterns, use_ac, 0, False)
    pairs = tr.Pairs(tr.occurrences(*_pack(r1), patterns), tr.occurrences(*_pack(r2), patterns))
    for inv in (False, True):
        keep, rows, c = ob.extract_paired(om, r1, r2, logging=True, invert=inv)
        f, rec, pat, pos = pairs.rows(use_ac)
        assert list(zip(f.tolist(), rec.tolist(), pat.tolist(), pos.tolist())) == rows
        k = pairs.keep(inv)
        assert k.astype(bool).tolist() == keep
        assert dict(pairs.counters(k), pattern_hit_counts=pairs.counts(use_ac).tolist()) == c


def test_the_same_pattern_in_both_mates_counts_twice_for_bndmq():
    """the case that tells "per (pair, pattern, mate)" from "per (pair, pattern)" and from "per hit", spelled out"""
    p, q = b"ACGTTGCAAC", b"GGGTTTCCCA"
    r1, r2 = [p + b"T" + p + b"T" + p, q], [b"TT" + p, b"ACGT"]
    pairs = tr.Pairs(tr.occurrences(*_pack(r1), [p, q]), tr.occurrences(*_pack(r2), [p, q]))
    assert pairs.counts(ac=False).tolist() == [2, 1] and pairs.counts(ac=True).tolist() == [4, 1]
    om = ob.Matcher([p, q], False, 0, False)
    assert ob.extract_paired(om, r1, r2, logging=True)[2]["pattern_hit_counts"] == [2, 1]
    f, rec, pat, pos = pairs.rows(ac=False)
    assert list(zip(f.tolist(), rec.tolist(), pat.tolist(), pos.tolist())) == [(0, 0, 0, 0), (0, 0, 0, 11), (0, 0, 0, 22), (1, 0, 0, 2), (0, 1, 1, 0)]


def test_window_codes_at_every_length():
    rnd = np.random.default_rng(5)
    text = np.frombuffer(b"ACGTN", dtype=np.uint8)[rnd.choice(5, size=300, p=[0.24, 0.24, 0.24, 0.24, 0.04])]
    for k in range(1, 33):
        w, valid = tr.window_codes(text, k)
        assert len(w) == len(valid) == 300 - k + 1
        for i in (0, 1, 7, 100, 300 - k):
            s = text[i:i + k].tobytes()
            assert bool(valid[i]) == (b"N" not in s)
            if valid[i]:
                assert int(w[i]) == int(tr.pattern_codes([s])[0])
    assert len(tr.window_codes(text[:5], 6)[0]) == 0
