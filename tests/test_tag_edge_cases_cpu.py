"""The crafted SAM lines and BAM records of tests/tag_edge_cases.py put their bytes where their builders say (proved here from the
bytes alone), and the references the GPU tests compare with accept every case that is meant to be taken: tag_windows.records_of /
existing_value, `encode` of test_gpu_sam_bam_window.py and `sam_line` of test_gpu_bam_sam_window.py.  No device."""
import itertools
import struct

import pytest

import tag_edge_cases as tc
from tag_windows import existing_value, records_of
from test_gpu_bam_sam_window import REFS as BAM_REFS
from test_gpu_bam_sam_window import sam_line as bam_to_sam
from test_gpu_bam_window import decode, split_records
from test_gpu_sam_bam_window import REFS as SAM_REFS
from test_gpu_sam_bam_window import encode


def nth_tab(line, which):
    """(independent of the builders) offset of the which-th tab, by walking the bytes"""
    seen = 0
    for k, c in enumerate(line):
        if c == 9:
            seen += 1
            if seen == which:
                return k
    return None


def encodes(items, tag=b"km"):
    """records_of takes the text, and every line encodes as BAM with a tag field appended"""
    recs, used = records_of(tc.text_of(items))
    assert used == len(tc.text_of(items)) and len(recs) == sum(1 for ln, _, _ in items if ln and ln[:1] != b"@")
    for ln, _, _, aux in recs:
        existing_value(aux, tag)
        encode(ln + b"\t" + tag + b":Z:ACGT", SAM_REFS)
    return recs


def test_tab_family_covers_every_lane_offset_and_step_edge():
    items = tc.sam_tab_family()
    seen = {w: set() for w in (1, 9, 10, 11)}
    for ln, eol, d in items:
        assert nth_tab(ln, d["tab"]) == d["off"] and eol == d["eol"]
        assert b"\r" not in ln and b"\n" not in ln and len(ln.split(b"\t")) == 12
        seen[d["tab"]].add((d["off"], eol))
    for w in (1, 9, 10, 11):
        for eol in (b"\n", b"\r\n"):
            offs = {o for o, e in seen[w] if e == eol}
            assert {o % tc.LANE for o in offs} == set(range(16)), w
            if w == 1:
                assert 254 in offs and max(offs) == 254  # QNAME inside the specification
                assert {15, 16} <= offs
            else:
                assert set(tc.STEP_EDGES) <= offs, w
                assert {o for o in offs if o < 255} == set(range(48, 64))  # byte 15 of lane 3, byte 0 of lane 4
    encodes(items)


def test_long_qname_family_carries_tab_1_across_steps():
    items = tc.sam_long_qname_family()
    offs = set()
    for ln, eol, d in items:
        assert nth_tab(ln, 1) == d["off"] == len(ln.split(b"\t")[0]) > 254
        offs.add(d["off"])
    assert set(tc.STEP_EDGES) <= offs and 300 in offs
    recs, _ = records_of(tc.text_of(items))
    assert len(recs) == len(items)


def test_lane_family_puts_tabs_9_10_11_into_one_lane():
    items = tc.sam_lane_family()
    together, straddle, kinds = set(), set(), set()
    for ln, eol, d in items:
        f = ln.split(b"\t")
        assert len(f) == d["fields"]
        kinds.add((d["kind"], d["fields"]))
        if d["kind"] == "star":
            assert f[9] == b"*" and f[10] == b"*"
        if d["kind"] == "one":
            assert len(f[9]) == 1 and len(f[10]) == 1 and f[9] != b"*" and f[10] != b"*"
        if d["kind"] == "empty-cigar":
            assert f[5] == b""
        if d["fields"] >= 12 and d["kind"] != "empty-cigar":
            t9, t10, t11 = nth_tab(ln, 9), nth_tab(ln, 10), nth_tab(ln, 11)
            assert t11 - t9 == 4
            (together if t9 // 16 == t11 // 16 else straddle).add(t9 % 16)
    assert together == set(range(0, 12)) and straddle == set(range(12, 16))  # every position of the three in a lane, and across two
    assert {("star", 11), ("star", 12), ("one", 11), ("one", 12), ("one-star-qual", 12), ("empty-cigar", 11), ("empty-cigar", 13)} <= kinds
    recs = encodes(items)
    assert {len(r[2]) for r in recs} == {0, 1, 10}  # '*' has no bases, 'A' has one


def test_odd_family_is_what_only_sam_to_sam_takes():
    items, bits = tc.sam_odd_family()
    assert bits == 3
    kinds = {}
    for ln, eol, d in items:
        f = ln.split(b"\t")
        assert len(f) == d["fields"] >= 10
        kinds.setdefault(d["kind"], []).append(ln)
        lanes = [sum(1 for c in ln[b:b + 16] if c == 9) for b in range(0, len(ln), 16)]
        if d["kind"] == "many":
            assert max(lanes) == 8  # (one-byte fields: every other byte is a tab)
        if d["kind"] == "crowded":
            assert max(lanes) > 11
            wanted = {nth_tab(ln, w) // 16 for w in (1, 9, 10, 11)}
            assert (wanted == {0} and lanes[0] > 11) == d["wanted_in_lane0"]
        if d["kind"] == "end-tab":
            assert ln.endswith(b"\t") and f[-1] == b""
    assert set(kinds) == {"ten", "many", "crowded", "end-tab"}
    crowded = [(ln, d) for ln, _, d in items if d["kind"] == "crowded"]
    assert any(d["wanted_in_lane0"] and ln.split(b"\t")[9] == b"*" for ln, d in crowded) and any(d["wanted_in_lane0"] and ln.split(b"\t")[9] == b"A" for ln, d in crowded)
    assert any(sum(1 for c in ln[b:b + 16] if c == 9) == 16 for ln, d in crowded for b in range(0, len(ln), 16))  # a lane of tabs alone
    assert any(existing_value(ln.split(b"\t")[11:], b"km") == b"TTTT,zz" for ln, d in crowded)
    # '\r' directly behind a tab: the CRLF form of the lines that end on a tab
    assert any(ln.endswith(b"\t") and eol == b"\r\n" for ln, eol, _ in items)
    recs, _ = records_of(tc.text_of(items))
    assert len(recs) == len(items)
    for ln, _, _, aux in recs:
        existing_value(aux, b"km")


def test_length_family_is_a_consecutive_run():
    items = tc.sam_length_family()
    lens = [len(ln) for ln, _, d in items if d["length"] is not None]
    assert all(len(ln) == d["length"] for ln, _, d in items if d["length"] is not None)
    assert lens == list(range(lens[0], lens[0] + len(lens))) and len(lens) >= 300
    assert {255, 256, 257, 511, 512, 513} <= set(lens) and {n % 16 for n in lens} == set(range(16))
    long = [ln for ln, _, d in items if d.get("long")]
    assert len(long) == 1 and len(long[0].split(b"\t")[9]) == len(long[0].split(b"\t")[10]) == 10000 and len(long[0]) > 16384
    encodes(items)


def test_seq_family_meets_every_length_at_every_alignment():
    met = set()
    for group in (range(0, 4), range(4, 8), range(8, 12), range(12, 16)):
        items = tc.sam_seq_family(group)
        for ln, _, d in items:
            f = ln.split(b"\t")
            start = nth_tab(ln, 9) + 1
            L = 0 if f[9] == b"*" else len(f[9])
            assert (L, start % 16) == (d["seq_len"], d["align"]) and d["align"] in group
            assert f[10] == b"*" or len(f[10]) == L
            met.add((L, start % 16))
        if group[0] == 0:
            encodes(items)
    assert met == {(L, a) for L in range(301) for a in range(16)}


def test_case_family_has_lower_case_and_confounders_everywhere_in_a_group():
    items = tc.sam_case_family()
    lower_at, conf = set(), {}
    for ln, _, d in items:
        seq = ln.split(b"\t")[9]
        if d["kind"] == "lower":
            assert [k for k, c in enumerate(seq) if 97 <= c <= 122] == [d["at"]]
            lower_at.add(d["at"] % 8)
        elif d["kind"] == "lower-all":
            assert seq == seq.lower() and seq.isalpha()
        else:
            k = d["at"]
            assert seq[k - 1:k + 2] == bytes([97, d["byte"], 122])
            in_group = k // 8 * 8 + 8 <= len(seq)  # the gather's full groups of eight; the rest goes byte by byte
            conf.setdefault(d["byte"], set()).add((k % 8, in_group))
    assert lower_at == set(range(8))
    assert set(conf) == set(tc.CONFOUNDERS) == {0x40, 0x5B, 0x60, 0x7B, 0xE1, 0xFA, 0xFF}
    for c, places in conf.items():
        assert {p for p, g in places if g} == set(range(8)) and any(not g for p, g in places), c
    recs = encodes(items)
    # the references leave every confounder as it is and map it to nibble 15
    for (ln, _, seq, _), (_, _, d) in zip(recs, items):
        if d["kind"] == "confounder":
            assert seq[d["at"] - 1:d["at"] + 2] == bytes([65, d["byte"], 90])
            rec = encode(ln + b"\tkm:Z:", SAM_REFS)
            name, text = decode(rec)
            assert text[d["at"] - 1:d["at"] + 2] == b"ANN"


def test_existing_family_places_the_field_behind_every_lane_offset():
    items = tc.sam_existing_family()
    offs, kinds = set(), set()
    for ln, eol, d in items:
        f = ln.split(b"\t")
        a = nth_tab(ln, 11) + 1
        kinds.add(d["kind"])
        if d["kind"] == "at":
            p = ln.index(b"\tkm:Z:")
            assert p - a == d["off"] and ln.count(b"\tkm:") == 1
            offs.add(d["off"])
        if d["kind"] == "field12":
            assert f[11].startswith(b"km:Z:")
        if d["kind"] == "last":
            assert f[-1] == b"km:Z:" + d["value"] and len(f[-1]) in (5, 6)
        if d["kind"] == "two":
            mine = [k for k, x in enumerate(f) if x.startswith(b"km:")]
            assert len(mine) == 2 and f[mine[0]][3:5] == b"Z:"
            p0, p1 = ln.index(b"\tkm:") + 1 - a, ln.rindex(b"\tkm:") + 1 - a
            assert p0 // 16 != p1 // 16 and (p0 // 256 != p1 // 256) == (d["gap"] == 300)
        if d["kind"] == "big":
            assert len(d["value"]) == tc.MERGE_MAX == 2048
        assert existing_value(f[11:], b"km") == d["value"]
    assert {o % 16 for o in offs} == set(range(16)) and {255, 256, 257} <= offs and 31 in offs
    assert kinds == {"at", "field12", "last", "two", "big"}
    encodes(items)
    short, bits = tc.sam_short_tag_family()
    assert bits == 2
    for ln, eol, d in short:
        assert existing_value(ln.split(b"\t")[11:], b"km") == d["value"]
    assert any(ln.endswith(b"\tkm:Z") for ln, _, _ in short)


def test_refusal_texts():
    texts = tc.sam_refusal_texts()
    assert set(texts) == {"value-2049", "i-first-40", "i-first-300", "nine-fields-last"}
    text, status = texts["value-2049"]
    assert status == 4 and max(len(f) for f in text.split(b"\n")[5].split(b"\t")) == 5 + 2049
    for gap in (40, 300):
        text, status = texts["i-first-%d" % gap]
        ln = text.split(b"\n")[3]
        assert status == 4 and ln.index(b"km:i:") < ln.index(b"km:Z:") and (ln.index(b"km:Z:") - ln.index(b"km:i:") > 256) == (gap == 300)
    text, status = texts["nine-fields-last"]
    lines = text.split(b"\n")[:-1]
    assert status == 1 and len(lines) % 4 == 0 and len(lines[-1].split(b"\t")) == 9 and all(len(x.split(b"\t")) >= 11 for x in lines[:-1])


def test_count_texts():
    texts = tc.sam_count_texts()
    counts = set()
    for name, (items, n) in texts.items():
        recs, _ = records_of(tc.text_of(items))
        assert len(recs) == n == sum(1 for _, _, d in items if d["rec"]), name
        flags = [d["rec"] for _, _, d in items]
        if "-first" in name:
            assert not flags[0] and flags[-1]
        if "-last" in name:
            assert flags[0] and not flags[-1]
        if "-run" in name:
            run = int(name.split("run")[1])
            runs = [len(list(g)) for k, g in itertools.groupby(flags) if not k]
            assert runs and all(r % run == 0 for r in runs) and flags[-1]
        counts.add(n)
        assert any(len(r[2]) < 4 for r in recs) or n == 1  # records without a 4-mer: dropped under filter_matching
    assert set(tc.RECORD_COUNTS) <= counts
    items, n = texts["one-among-40"]
    assert n == 1 and len(items) == 41
    assert {(ln[:1], eol) for ln, eol, d in items if not d["rec"]} == {(b"@", b"\n"), (b"", b"\n"), (b"", b"\r\n")}
    encodes(texts["n65-run4"][0])


def test_stats_texts():
    texts = tc.sam_stats_texts()
    bam = tc.bam_stats_records()
    assert set(texts) == set(bam)
    seen = set()
    for name, (items, n, where) in texts.items():
        recs, _ = records_of(tc.text_of(items))
        lens = [len(r[2]) for r in recs]
        assert n in (4, 64, 257) and len(lens) == n
        odd = [i for i, L in enumerate(lens) if L != 12]
        assert odd == ([] if where is None else [where]), name
        assert [struct.unpack_from("<i", r, 20)[0] for r in bam[name][0]] == lens and bam[name][1] == where
        if where is not None:
            seen.add((n, where, lens[where]))
    for n in (4, 64, 257):
        wave0 = (n - 1) // 4 * 4  # 64 lanes = 4 lines of 16 lanes: the line lane 0 of the last wave works on
        assert tc.last_wave_lane0(n) == wave0
        for where in {0, n - 1, wave0}:
            assert {L for (m, w, L) in seen if (m, w) == (n, where)} == {0, 5, 40}
    assert tc.last_wave_lane0(257) == 256 and tc.last_wave_lane0(64) == 60


# ---- BAM -----------------------------------------------------------------------------------------------------------------------
def bam_lines(recs):
    """the BAM -> SAM reference takes every record, and the records are a chain"""
    text = b"".join(recs)
    got, used = split_records(text)
    assert got == list(recs) and used == len(text)
    return [bam_to_sam(r, BAM_REFS) for r in recs]


def test_bam_lseq_family():
    fam = tc.bam_lseq_family()
    assert [d["l_seq"] for _, d in fam] == list(range(531))
    kinds, aligns = {}, set()
    for rec, d in fam:
        L = struct.unpack_from("<i", rec, 20)[0]
        assert L == d["l_seq"] and rec[12] == d["name_len"] + 1 and struct.unpack_from("<H", rec, 16)[0] == d["ops"]
        at = 36 + rec[12] + 4 * d["ops"]
        q = rec[at + (L + 1) // 2:at + (L + 1) // 2 + L]
        kind = 0 if L == 0 else 1 if q == b"\xff" * L else 2 if L > 1 and q[0] != 0xFF and q[1:] == b"\xff" * (L - 1) else 3 if any(x + 33 > 255 for x in q) else 0
        assert kind == d["kind"] or (L == 1 and d["kind"] == 2), (L, kind, d)
        kinds.setdefault(kind, set()).add(L)
        aligns.add((at % 8, L % 2))
    assert set(kinds) == {0, 1, 2, 3}
    for k in kinds:  # every kind of quality on both sides of the 128- and 256-base steps, odd and even
        assert {L % 2 for L in kinds[k]} == {0, 1} and any(L > 256 for L in kinds[k]) and any(0 < L < 128 for L in kinds[k])
    assert {d["name_len"] for _, d in fam} == set(range(1, 17)) and {d["ops"] for _, d in fam} == {0, 1, 2, 3}
    assert {a for a, _ in aligns} == set(range(8))
    lines = bam_lines([r for r, _ in fam])
    assert [len(s) for _, _, s in lines] == list(range(531))


def test_bam_length_family():
    fam = tc.bam_length_family()
    lens = [len(r) for r, _ in fam]
    assert lens == [d["length"] for _, d in fam] == list(range(lens[0], lens[0] + len(lens))) and len(lens) >= 130
    assert {n % 64 for n in lens} == set(range(64)) and all(4 + struct.unpack_from("<i", r, 0)[0] == len(r) for r, _ in fam)
    bam_lines([r for r, _ in fam])


@pytest.mark.parametrize("piece", [256, 4096])
def test_bam_piece_records_meet_the_pieces(piece):
    n_pieces = 20
    recs, placed, total = tc.bam_piece_records(piece, n_pieces, span3_at=8)
    starts = [0]
    for r in recs:
        starts.append(starts[-1] + len(r))
    assert total == starts[-1] == len(b"".join(recs))
    for j, delta, k in placed:
        assert starts[k] == j * piece + delta
    assert {d for _, d, _ in placed} == {-1, 0, 1}
    # one record holds three whole pieces: none of them has a record start
    empty = [j for j in range(n_pieces) if not any(j * piece <= s < (j + 1) * piece for s in starts[:-1])]
    assert len(empty) >= 3 and empty == list(range(empty[0], empty[0] + len(empty)))
    assert max(len(r) for r in recs) > 3 * piece
    bam_lines(recs)


@pytest.mark.parametrize("piece", [256, 4096])
def test_bam_cut_cases_end_inside_a_record_that_starts_before_a_piece(piece):
    recs, placed, total = tc.bam_piece_records(piece, 24)
    starts = [0]
    for r in recs:
        starts.append(starts[-1] + len(r))
    cuts = tc.bam_cut_cases(recs, placed)
    assert [d for _, _, d in cuts] == [1, 2, 3, 4, 35, 36, 37]
    for cut, k, d in cuts:
        assert cut == starts[k] + d and d < len(recs[k]) and 0 < k < len(recs)
        assert starts[k] % piece == piece - 1  # the record starts on a piece's last byte ...
        assert (starts[k] // piece < (cut - 1) // piece) == (d >= 2)  # ... and the text ends in the next piece from two bytes on


@pytest.mark.parametrize("piece", [256, 4096])
def test_bam_long_tail_case(piece):
    recs, k, cut = tc.bam_long_tail_case(piece)
    starts = [0]
    for r in recs:
        starts.append(starts[-1] + len(r))
    assert starts[k] < cut < starts[k + 1] and (cut - 1) // piece - starts[k] // piece >= 12 > 8  # (8: the record index's proof rounds)
    assert k + 1 < len(recs)
    bam_lines(recs)


def test_bam_piece_counts():
    for count in (63, 64, 65, 129):
        recs, total = tc.bam_piece_count_records(256, count)
        assert len(b"".join(recs)) == total and (total + 255) // 256 == count
        got, used = split_records(b"".join(recs))
        assert used == total and len(got) == len(recs)


def test_bam_existing_family():
    fam = tc.bam_existing_family()
    wheres = set()
    for rec, d in fam:
        line, name, seq = bam_to_sam(rec, BAM_REFS)
        f = line.split(b"\t")[11:]
        mine = [k for k, x in enumerate(f) if x[:3] == b"km:"]
        if d["existing"] is None:
            assert not mine
            continue
        assert f[mine[0]] == b"km:Z:" + d["existing"]
        where = "first" if mine[0] == 0 else "last" if mine[0] == len(f) - 1 else "middle"
        assert where == d["where"]
        wheres.add((where, f[mine[0] - 1][3:4] if mine[0] else None))
    assert {w for w, _ in wheres} == {"first", "middle", "last"}
    assert {t for w, t in wheres if w == "last"} >= {b"A", b"i", b"f", b"Z", b"H", b"B"}
    sizes = {len(x.split(b",")) - 1 for rec, d in fam for x in bam_to_sam(rec, BAM_REFS)[0].split(b"\t")[11:] if x[3:4] == b"B"}
    assert sizes == {0, 300}
    assert max(len(d["existing"] or b"") for _, d in fam) == 2048
    over = bam_to_sam(tc.bam_over_record(), BAM_REFS)[0].split(b"\t")[-1]
    assert over.startswith(b"km:Z:") and len(over) == 5 + 2049


def test_spelling():
    assert tc.spelled(b"ACGTNACGTA") == b"ACGT.ACGTA" and tc.spelled(b"ACG") == b"..." and tc.spelled(b"AC\xe1GTTTT") == b"...GTTTT"
    pats = tc.kmers4()
    rows = [(b"", 0, pats.index(b"ACGT"), 0), (b"", 0, pats.index(b"CGTT"), 1), (b"", 1, pats.index(b"TTTT"), 2)]
    assert tc.spell_back(rows, pats, [6, 6]) == [b"ACGTT.", b"..TTTT"]
    with pytest.raises(AssertionError):
        tc.spell_back(rows + [(b"", 0, pats.index(b"AAAA"), 2)], pats, [6, 6])
    assert tc.upper(b"az`{\xe1AZ") == b"AZ`{\xe1AZ"
