"""tests/scan_variant_matrix.py before a kernel sees it: its rows are exactly the instantiations of scan_variants.hip, its names
exactly what the MK_VARIANT* macros of scan_kernel.hip can spell for them, every recipe plans (mk_plan_geometry, host only) the
geometry its row stands for, and every batch holds what it claims -- by the naive enumerator, which the oracle must agree
with.  tests/test_gpu_scan_variants.py then runs every row."""
import os
import re

import pytest

import naive
import oracle_binding as ob
import scan_variant_matrix as sm
from merkurio_amd import native as mk

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "merkurio_amd", "csrc")
IDS = [v.id for v in sm.VARIANTS]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _key(v):
    return (v.S, v.QC, v.GF, v.plain, v.MC)


# ---------------------------------------------------------------------------------------------------- the table against the sources
def instantiations(src):
    """the (S, QC, GF, plain, MC) of the MK_INST* lines of scan_variants.hip, in file order"""
    out = []
    for kind, s, qc, third in re.findall(r"^\s*MK_INST(_PLAIN|_MC_GF|_MC|)\(\s*(-?\d+)\s*,\s*(-?\d+)\s*(?:,\s*(\w+)\s*)?\);", src, re.M):
        S, QC = int(s), int(qc)
        if kind == "":
            assert third in ("true", "false")
            out.append((S, QC, third == "true", False, 0))
        elif kind == "_PLAIN":
            assert third in ("true", "false")
            out.append((S, QC, third == "true", True, 0))
        elif kind == "_MC":
            out.append((S, QC, False, False, int(third)))
        else:
            assert third == ""
            out.append((S, QC, True, False, 1))
    return out


def test_rows_are_the_instantiations_of_scan_variants():
    src = _read("scan_variants.hip")
    inst = instantiations(src)
    # every line that instantiates is one the expression above reads
    assert len(inst) == len(re.findall(r"^\s*MK_INST\w*\(", src, re.M)), "an MK_INST* line of scan_variants.hip was not understood"
    assert len(set(inst)) == len(inst), "scan_variants.hip instantiates a variant twice"
    rows = [_key(v) for v in sm.VARIANTS]
    assert len(set(rows)) == len(rows) == 73
    missing, extra = set(inst) - set(rows), set(rows) - set(inst)
    assert not missing and not extra, f"instantiated without a row of VARIANTS: {sorted(missing)}; rows without an instantiation: {sorted(extra)}"
    assert len({v.id for v in sm.VARIANTS}) == 73


def macro_names(src):
    """every kernel name the MK_VARIANT* invocations of scan_kernel.hip can return: the macros' string pieces with the
    arguments of each invocation pasted in (a macro that invokes another one, MK_VARIANT_MCS, spells that one's names too)"""
    macros = {}
    for m in re.finditer(r"^#define (MK_VARIANT\w*)\(([^)]*)\)((?:.*\\\n)*.*)\n", src, re.M):
        macros[m.group(1)] = ([a.strip() for a in m.group(2).split(",")], m.group(3))
    assert set(macros) == {"MK_VARIANT", "MK_VARIANT_PLAIN", "MK_VARIANT_MC", "MK_VARIANT_MCS", "MK_VARIANT_MC_GF"}, sorted(macros)
    call = re.compile(r"\b(MK_VARIANT\w*)\(([^()]*)\)")

    def spell(name, args):
        params, body = macros[name]
        assert len(params) == len(args), (name, args)
        bind = dict(zip(params, args))
        out = set()
        for lit in re.findall(r'"mk_scan_kernel<"(?:\s*#\w+\s*"[^"]*")+', body):
            pieces = re.findall(r'"([^"]*)"|#(\w+)', lit)
            out.add("".join(text if not par else bind[par] for text, par in pieces))
        for inner, inner_args in call.findall(body):
            out |= spell(inner, [bind.get(a.strip(), a.strip()) for a in inner_args.split(",")])
        return out

    names = set()
    code = "\n".join(ln for ln in re.sub(r"\\\n", " ", src).split("\n") if not ln.startswith("#define"))
    for name, args in call.findall(code):
        names |= spell(name, [a.strip() for a in args.split(",")])
    return names


def test_names_are_what_the_dispatcher_can_spell():
    names = macro_names(_read("scan_kernel.hip"))
    table = {n for v in sm.VARIANTS for n in v.names}
    assert len(table) == 146
    assert names == table, f"only the dispatcher spells {sorted(names - table)}; only the table spells {sorted(table - names)}"
    for v in sm.VARIANTS:
        assert ",false," in v.names[0] and ",true," in v.names[1] and v.names[0].replace(",false,", ",true,", 1) == v.names[1]
        assert v.names[0].endswith("plain>") == v.plain and v.names[0].endswith("2-class>") == (v.MC != 0)
        assert (f"s2={v.MC}," in v.names[0]) == (v.MC > 1)


def test_short_class_table_bound_is_the_sources():
    m = re.search(r"constexpr uint32_t kShortByteMaxQ = (\d+);", _read("filter.hpp"))
    assert m and int(m.group(1)) == sm.SHORT_BYTE_MAX_Q


# ---------------------------------------------------------------------------------------------------- the recipes
@pytest.mark.parametrize("vid", IDS)
def test_recipe_plans_the_geometry_of_its_row(vid):
    v = sm.BY_ID[vid]
    patterns, _ = sm.batch(v)
    g = mk.plan_geometry([len(p) for p in patterns], v.options)
    fixed = sm.GF_FIXED if v.GF else sm.LDS_FIXED
    assert g["stride"] == v.S and g["q_gram"] == v.q and bool(g["in_lds"]) == (not v.GF), (g, v)
    # the q-gram mode the dispatcher derives from (S, q): compiled in, narrow or wide
    if v.QC > 0:
        assert (v.S, v.q) in fixed and v.q == v.QC
    else:
        assert ((v.S, v.q) not in fixed or (v.GF and v.MC)) and (v.q <= 16) == (v.QC == 0) and 1 <= v.q <= 32
    main = [len(p) for p in patterns if len(p) >= v.lmin]
    assert min(main) == v.lmin and sorted(set(main)) == sm.main_lengths(v) and v.q == min(32, v.lmin - v.S + 1)
    if not v.MC:
        assert g["split_len"] == 0 and g["n_short"] == 0 and len(main) == len(patterns)
        assert v.plain <= (not v.GF)  # only a one-class LDS-filter row has a plain-load twin
    else:
        shorts = [len(p) for p in patterns if len(p) < v.lmin]
        assert g["split_len"] == v.lmin and g["n_short"] == len(shorts) == 5 and sorted(set(shorts)) == list(v.short_lengths)
        assert g["stride2"] == v.stride2 and g["q_gram2"] == v.q2 and v.S >= 2
        byte_table = v.q2 <= sm.SHORT_BYTE_MAX_Q
        compiled = byte_table and v.stride2 in (2, 4, 8) and v.QC > 0 and not v.GF  # MK_VARIANT_MCS
        assert v.MC == (v.stride2 if compiled else 1), (v, g)
    assert 15 <= len(patterns) <= 32


# ---------------------------------------------------------------------------------------------------- the batches
def _nested_ok(v, patterns):
    """no pattern a substring of another one, but the suffix-nested triple and the short pattern cut out of a long one"""
    inside = [(a, b) for a in patterns for b in patterns if a != b and b in a]
    triple = [(a, b) for a, b in inside if a.endswith(b)]
    cut = [(a, b) for a, b in inside if not a.endswith(b)]
    tops = {a for a, _ in triple}
    assert len(triple) == 3 and len({a for a, b in triple} | {b for a, b in triple}) == 3, inside
    assert sorted(len(x) for x in {a for a, b in triple} | {b for a, b in triple}) == [v.lmin, v.lmin + 1, 2 * v.lmin] and tops
    assert len(cut) == (1 if v.MC else 0) and all(len(b) < v.lmin <= len(a) for a, b in cut), cut


@pytest.mark.parametrize("vid", IDS)
def test_batch_holds_what_it_claims(vid):
    v = sm.BY_ID[vid]
    bt, e = sm.details(v), sm.expected(v)
    patterns, records = sm.batch(v)
    assert patterns is bt.patterns and records is bt.records and (sm.batch(vid)[1] is records)  # deterministic, built once
    assert set(b"".join(patterns)) <= set(b"ACGT") and bt.ci == v.ci
    _nested_ok(v, patterns)
    starts = sm.record_starts(records)
    assert e.bases == starts[-1] <= sm.TEXT_MAX and e.records == len(records)
    per_rec = {}
    for r, p, pos in e.tuples:
        per_rec.setdefault(r, []).append((p, pos))
    # ---- the oracle agrees with the enumerator
    om = ob.Matcher(patterns, True, 0, v.ci)
    assert om.rc == 0
    _, rows, counters, found = ob.tag_records(om, records, logging=True)
    assert [(r, p, pos) for (_, r, p, pos) in rows] == e.tuples
    assert [bool(f) for f in found] == e.flags
    assert counters["pattern_hit_counts"] == e.counts and counters["hits"][0] == e.hits == len(e.tuples) == sum(e.counts)
    assert counters["records_hit"][0] == e.records_hit == sum(e.flags)
    assert counters["records"] == e.records and counters["bases"] == e.bases
    # ---- every pattern at every offset 0 .. 63 of a record, and at every residue modulo 64 of the batch
    assert sorted((p, o) for _, p, o in bt.planted) == [(p, o) for p in range(len(patterns)) for o in range(sm.N_OFFSETS)]
    residues = {}
    for r, p, o in bt.planted:
        assert (p, o) in per_rec[r] and records[r][o:o + len(patterns[p])] == patterns[p]
        # nothing but the planted pattern and the patterns inside it
        assert all(o <= pos and pos + len(patterns[q]) <= o + len(patterns[p]) for q, pos in per_rec[r]), (r, per_rec[r])
        residues.setdefault(p, set()).add((starts[r] + o) % 64)
    assert all(residues[p] == set(range(64)) for p in range(len(patterns)))
    assert all(c >= 64 for c in e.counts), e.counts
    for S in (v.S, 16):  # every residue of the sampling stride and every byte of a 16-byte load, in the text the kernel samples
        assert all({x % S for x in residues[p]} == set(range(S)) for p in range(len(patterns)))
    # ---- record ends: a record that is the pattern, one base short at either end, one base more at either end, empty
    probes = {}
    for r, rec in enumerate(records):
        for p, pat in enumerate(patterns):
            if rec == pat and r + 1 < len(records) and records[r + 1] == pat[:-1]:
                probes[p] = r
    assert sorted({len(patterns[p]) for p in probes}) == sorted(sm.main_lengths(v) + list(v.short_lengths))
    for p, r in probes.items():
        pat = patterns[p]
        assert per_rec[r] == [(p, 0)]
        assert records[r + 1] == pat[:-1] and records[r + 2] == pat[1:] and not e.flags[r + 1] and not e.flags[r + 2]
        assert len(records[r + 3]) == len(pat) + 1 == len(records[r + 4]) and per_rec[r + 3] == [(p, 0)] and per_rec[r + 4] == [(p, 1)]
        assert records[r + 5].endswith(pat) and len(records[r + 5]) > len(pat) + 6 and per_rec[r + 5] == [(p, len(records[r + 5]) - len(pat))]
        assert records[r + 6] == b"" and not e.flags[r + 6]
    # ---- the spelling across two records gives no tuple
    assert sorted(p for _, _, p in bt.cross) == sorted(probes)
    for r1, r2, p in bt.cross:
        assert r2 == r1 + 1 and patterns[p] in records[r1] + records[r2] and not e.flags[r1] and not e.flags[r2]
        assert records[r1] and records[r2]
    # ---- near-misses: for one pattern of each length every base replaced, by a base and by N; none gives a tuple
    assert not any(e.flags[r] for r in bt.near_miss)
    for p in probes:
        pat = patterns[p]
        for i in range(len(pat)):
            for repl in (b"CGTA"[b"ACGT".index(pat[i])], ord("N")):
                nm = pat[:i] + bytes([repl]) + pat[i + 1:]
                assert any(nm in records[r] for r in bt.near_miss), (pat, i, repl)
        # lower case: an occurrence only for a case-insensitive matcher
        low = [r for r, rec in enumerate(records) if pat.lower() in rec]
        assert len(low) == 1 and e.flags[low[0]] == v.ci
        mixed = pat[:2] + pat[2:3].lower() + pat[3:]
        assert any(mixed in rec and e.flags[r] == v.ci for r, rec in enumerate(records))
        assert any(rec != rec.upper() and r in bt.near_miss for r, rec in enumerate(records))
    # ---- overlaps: a pattern over itself at every shift 1 .. S, two patterns over shared bases, three that end on one byte
    runs = [p for p, pat in enumerate(patterns) if len(set(pat)) == 1]
    assert len(runs) == 2
    for p in runs:
        L = len(patterns[p])
        assert any([pos for q, pos in hits if q == p] == list(range(hits[0][1], hits[0][1] + v.S + 1)) and len(hits) == v.S + 1
                   for r, hits in per_rec.items() if r != bt.long_rec)
    assert any(len({p for p, _ in hits}) == 2 and len(hits) == 2 and abs(hits[0][1] - hits[1][1]) < len(patterns[hits[0][0]])
               and hits[0][1] + len(patterns[hits[0][0]]) != hits[1][1] + len(patterns[hits[1][0]]) for hits in per_rec.values())
    assert any(len(hits) == 3 and len({pos + len(patterns[p]) for p, pos in hits}) == 1 for hits in per_rec.values())
    if v.MC:  # a short pattern inside a long one: two tuples, the short one's span inside the long one's
        assert any(len(hits) == 2 and len(patterns[hits[0][0]]) < v.lmin <= len(patterns[hits[1][0]]) and
                   hits[1][1] < hits[0][1] and hits[0][1] + len(patterns[hits[0][0]]) < hits[1][1] + len(patterns[hits[1][0]])
                   for hits in per_rec.values())
    # ---- tile borders: the long record is the batch's last, the borders are those of the launch (31 KiB tiles, then the tail)
    assert bt.long_rec == len(records) - 1 and len(records[-1]) == 256 + 2 * sm.TILE + sm.TAIL_BYTES
    g = mk.scan_tile_geometry(e.bases, 16, 1)
    assert g["n_long_tiles"] == 0 and g["short_tile_bytes"] == sm.TILE and g["tail_start"] == e.bases - sm.TAIL_BYTES, g
    assert [b for b, _ in bt.borders] == [g["tail_start"] - 2 * sm.TILE, g["tail_start"] - sm.TILE, g["tail_start"]]
    ends = {}
    for p, pos in per_rec[bt.long_rec]:
        ends.setdefault(p, set()).add(starts[bt.long_rec] + pos + len(patterns[p]) - 1)
    for border, p in bt.borders:
        L = len(patterns[p])
        assert border % sm.TILE == 0 and p in runs and set(range(border - (L - 1), border + 2)) <= ends[p], (border, p)
    assert {p for _, p in bt.borders} == set(runs)
    tail_p, last_p = bt.tail_rec
    assert any(e.bases - 700 < x < e.bases - 1 for x in ends[tail_p]) and e.bases - 1 in ends[last_p]
    assert len(per_rec[bt.long_rec]) == sum(len(patterns[p]) + 1 for _, p in bt.borders) + 2
    # ---- the filler: a record nothing was planted in holds nothing
    assert sum(e.flags) < len(records) and e.hits >= 64 * len(patterns)


def test_enumerator_orders_the_nested_triple_longest_first():
    v = sm.VARIANTS[0]
    bt, e = sm.details(v), sm.expected(v)
    for r in range(len(bt.records)):
        hits = [(p, pos) for rr, p, pos in e.tuples if rr == r]
        if len(hits) == 3 and len({pos + len(bt.patterns[p]) for p, pos in hits}) == 1:
            assert [len(bt.patterns[p]) for p, _ in hits] == [2 * v.lmin, v.lmin + 1, v.lmin]
            assert hits == naive.ac_order(bt.patterns, bt.records[r], v.ci)
            return
    raise AssertionError("no record with the triple alone")
