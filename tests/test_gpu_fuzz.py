"""Randomised differential test: many small random pattern sets / record batches through the
GPU path vs the oracle, covering the generic (runtime-q) kernel variants, every stride the
geometry rule can pick, odd pattern lengths, mixed alphabets, -I, -r/-c pattern lists, forced
BNDMq / Aho-Corasick emission orders, the global-filter mode, length classes (a few much shorter
patterns next to the set: split by the rule or forced, every short-class stride / table kind, r04)
and the FASTQ-text entry point (mk_extract_fastq_text == mk_extract_single on the same reads, r04).  A second test draws the
same options over STRUCTURED cases: patterns that are consecutive windows of a few "genomes" and records cut from the same
genomes, so that table keys carry many entries and a record holds many overlapping occurrences (structured_sets.py)."""
import os
import random

import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mk():
    from merkurio_amd import native
    native.load()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")
    return native


ALPHABETS = [b"ACGT", b"ACGTN", b"ACGTacgt", b"AC", b"ACDEFGHIKLMNPQRSTVWY", b"ACGTRYKMBVDHSWN"]


def _case(rnd):
    alpha = rnd.choice(ALPHABETS)
    n_pat = rnd.choice([1, 2, 5, 13, 14, 40, 300])
    base_len = rnd.choice([1, 2, 3, 4, 7, 8, 12, 15, 16, 17, 20, 21, 23, 24, 25, 28, 31, 32, 33, 40, 47, 48, 49, 64, 65, 90])
    mixed = rnd.random() < 0.3
    raw = []
    for _ in range(n_pat):
        L = max(1, base_len + (rnd.randrange(0, 9) if mixed else 0))
        raw.append(bytes(rnd.choice(alpha) for _ in range(L)))
    if base_len >= 15 and rnd.random() < 0.35:  # length classes: a few much shorter patterns next to the set
        for _ in range(rnd.choice([1, 1, 2, 5])):
            raw.append(bytes(rnd.choice(alpha) for _ in range(rnd.choice([1, 2, 3, 5, 8, 8, 9, 12, 14]))))
    recs = []
    for _ in range(rnd.choice([1, 20, 200])):
        n = rnd.choice([0, 1, base_len - 1 if base_len > 1 else 1, base_len, base_len + 1, 100, 151, 700])
        s = bytearray(rnd.choice(alpha) for _ in range(n))
        for _ in range(rnd.choice([0, 0, 1, 2])):
            p = rnd.choice(raw)
            if len(p) <= n:
                k = rnd.randrange(0, n - len(p) + 1)
                s[k:k + len(p)] = p
        recs.append(bytes(s))
    return raw, recs


# the list inside _case, which stays as it is: editing _case -- even to share this list -- risks the order of its draws, and
# its 32 x 60 cases are the record so far.  Keep the two lists equal.
_BASE_LENS = [1, 2, 3, 4, 7, 8, 12, 15, 16, 17, 20, 21, 23, 24, 25, 28, 31, 32, 33, 40, 47, 48, 49, 64, 65, 90]


def _structured_case(rnd):
    """patterns = runs of consecutive windows of one to four "genomes", records = windows of the same genomes (exact or with
    one letter changed) and random ones"""
    alpha = rnd.choice(ALPHABETS)
    genomes = [bytes(rnd.choice(alpha) for _ in range(rnd.randrange(200, 3001))) for _ in range(rnd.randrange(1, 5))]
    base_len = rnd.choice(_BASE_LENS)
    mixed = rnd.random() < 0.3
    raw = []
    for _ in range(rnd.choice([1, 2, 5])):
        g = rnd.choice(genomes)
        run = rnd.choice([1, 2, 13, 14, 40, 120])
        a = rnd.randrange(0, max(1, len(g) - base_len - 8 - run))
        for i in range(run):
            L = max(1, base_len + (rnd.randrange(0, 9) if mixed else 0))
            # never empty: a + i < 200 <= len(g).  A run longer than a short genome leaves (a = 0 then) ends at the genome's
            # end: its last windows are cut short there, on purpose -- patterns that are suffixes of one another
            raw.append(g[a + i:a + i + L])
    if base_len >= 15 and rnd.random() < 0.35:  # a few much shorter patterns cut from the same genomes
        for _ in range(rnd.choice([1, 1, 2, 5])):
            g = rnd.choice(genomes)
            L = rnd.choice([1, 2, 3, 5, 8, 8, 9, 12, 14])
            a = rnd.randrange(0, len(g) - L + 1)
            raw.append(g[a:a + L])
    recs = []
    for _ in range(rnd.choice([1, 20, 200])):
        n = rnd.choice([0, 1, base_len - 1 if base_len > 1 else 1, base_len, base_len + 1, 100, 151, 700])
        kind = rnd.randrange(3)
        if kind == 2:
            recs.append(bytes(rnd.choice(alpha) for _ in range(n)))
            continue
        g = rnd.choice(genomes)
        n = min(n, len(g))
        a = rnd.randrange(0, len(g) - n + 1)
        s = bytearray(g[a:a + n])
        if kind == 1 and n:
            s[rnd.randrange(n)] = rnd.choice(alpha)
        recs.append(bytes(s))
    return raw, recs


def _run_cases(mk, seed, case):
    rnd = random.Random(int(os.environ.get("MERKURIO_FUZZ_BASE", "1000")) + seed)
    for it in range(60):
        raw, recs = case(rnd)
        kw = dict(reverse_complement=rnd.random() < 0.3, canonical=False, lowercase=False, uppercase=rnd.random() < 0.1)
        if not kw["reverse_complement"] and rnd.random() < 0.2:
            kw["canonical"] = True
        ci = rnd.random() < 0.2
        rc, patterns = ob.parse_pattern_list(raw, **kw)
        assert rc == 0 and patterns == mk.parse_pattern_list(kmer_seq=raw, **kw)
        max_len = max(len(p) for p in patterns)
        choice = rnd.random()
        algo, q = mk.MK_ALGO_AUTO, 0
        if choice < 0.2:
            algo = mk.MK_ALGO_AC
        elif choice < 0.4 and max_len <= 64 and not ci:
            algo, q = mk.MK_ALGO_BNDMQ, rnd.choice([0, 1])
        options = dict(force_global_filter=True) if rnd.random() < 0.15 else None
        if rnd.random() < 0.3:  # length-class options; a set they cannot split is created by the rule instead
            options = dict(options or {}, length_classes=rnd.choice([1, 2, 2]), force_stride2=rnd.choice([0, 0, 1, 2, 4, 8]),
                           force_q2=rnd.choice([0, 0, 3, 6, 7, 8]))
        try:
            m = mk.Matcher(patterns, algo=algo, q=q, case_insensitive=ci, options=options)
        except mk.MerkurioError as e:
            if e.code != mk.MK_E_INVALID_ARG or not options or "length_classes" not in options:
                raise
            options = {k: v for k, v in options.items() if k == "force_global_filter"} or None
            m = mk.Matcher(patterns, algo=algo, q=q, case_insensitive=ci, options=options)
        use_ac = m.use_ac
        assert use_ac == (True if (ci or algo == mk.MK_ALGO_AC) else False if algo == mk.MK_ALGO_BNDMQ
                          else ob.select_aho_corasick(ci, False, False, patterns))
        om = ob.Matcher(patterns, use_ac, 0, ci)
        assert om.rc == 0
        logging, invert = rnd.random() < 0.8, rnd.random() < 0.3
        got = m.extract_single(recs, logging=logging, invert=invert)
        exp = ob.extract_single(om, recs, logging=logging, invert=invert)
        assert got == exp, (seed, it, patterns[:3], len(recs))
        if it % 3 == 0 and not any(b"\n" in r or b"\r" in r for r in recs):
            # the same reads as FASTQ text through the device's record index (ingest.hip)
            text = b"".join(b"@r%d x\n%s\n+\n%s\n" % (i, r, b"@" * len(r)) for i, r in enumerate(recs))
            status, rec_start, keep_t, rows_t, c_t = m.extract_fastq_text(text, logging=logging, invert=invert)
            assert status == 0 and (keep_t, rows_t, c_t) == exp and len(rec_start) == len(recs) + 1, (seed, it)
        if len(recs) >= 2:
            h = len(recs) // 2
            assert m.extract_paired(recs[:h], recs[h:2 * h], logging=True) == ob.extract_paired(om, recs[:h], recs[h:2 * h], logging=True)
        # tag: the keep/drop rule (-m / -v, src/cmd_tag.rs:457-467) with the same flags on both sides
        fm = rnd.random() < 0.5
        inv = (not fm) and rnd.random() < 0.5
        keep, rows, c, found = m.tag_records(recs, logging=logging, filter_matching=fm, invert=inv)
        keep_o, rows_o, c_o, found_o = ob.tag_records(om, recs, logging=logging, filter_matching=fm, invert=inv)
        assert keep == keep_o and rows == rows_o and c == c_o, (seed, it, fm, inv)
        assert found == [sorted(set(f)) for f in found_o]


# longer campaigns: MERKURIO_FUZZ_SEEDS=200 MERKURIO_FUZZ_BASE=5000 python -m pytest tests/test_gpu_fuzz.py -m gpu
@pytest.mark.parametrize("seed", range(int(os.environ.get("MERKURIO_FUZZ_SEEDS", "32"))))
def test_fuzz_vs_oracle(mk, seed):
    _run_cases(mk, seed, _case)


@pytest.mark.parametrize("seed", range(int(os.environ.get("MERKURIO_FUZZ_SEEDS", "16"))))
def test_fuzz_structured_vs_oracle(mk, seed):
    _run_cases(mk, seed, _structured_case)
