"""mk_bgzf_record_cuts (host code, no device): where the BGZF members of `extract -z` end -- at record ends wherever a record ends
within reach of a grid point.  The library against the numpy restatement of the rule in bgzf_cut_cases.py."""
import numpy as np
import pytest

import bgzf_cut_cases as cc
from merkurio_amd import native as mk

G, L = cc.G, cc.L


def test_constants_are_the_headers():
    assert (mk.BGZF_CUT_GRID, mk.BGZF_MEMBER_TEXT_MAX) == (G, L)


def test_no_records_and_an_empty_text_give_one_cut_and_no_member():
    assert mk.bgzf_record_cuts([]).tolist() == [0]
    assert mk.bgzf_record_cuts([0, 0]).tolist() == [0]


@pytest.mark.parametrize("name", sorted(cc.fixed_shapes()))
def test_fixed_shapes(name):
    e = cc.ends(cc.fixed_shapes()[name])
    cuts = mk.bgzf_record_cuts(e)
    assert cuts.tolist() == cc.rule(e).tolist()
    cc.check_properties(cuts, e)


def test_the_named_cuts():
    s = cc.fixed_shapes()
    cut = lambda name: mk.bgzf_record_cuts(cc.ends(s[name])).tolist()
    assert cut("one_byte") == [0, 1]
    assert cut("end_at_G") == [0, G, G + 500]
    assert cut("end_at_G_minus_1") == [0, G - 1 + 500, G - 1 + 1000]  # the end in front of the grid point is not looked at
    assert cut("end_at_G_plus_reach_minus_1") == [0, L - 1, L - 1 + 700]
    assert cut("end_at_G_plus_reach") == [0, G, L + 700]  # (no grid point behind G: the record end at L is no cut)
    assert cut("two_grid_points_one_record") == [0, G, 2 * G, 2 * G + 20150]
    assert cut("last_snap_is_T") == [0, -(-G // 331) * 331, 2 * G + 300]  # 2 G snaps to T: one cut, not two
    # the long record: raw cuts every G inside it, one cut at its end, record ends behind it
    lens = s["long_record_between_short"]
    e = cc.ends(lens)
    cuts = mk.bgzf_record_cuts(e)
    b, a = int(e[lens.index(200000) - 1]), int(e[lens.index(200000)])
    inside = [c for c in cuts.tolist() if b < c < a]
    assert (b, a) == (46000, 5 * G + 240) and inside == [k * G for k in range(1, 5)] and a in cuts.tolist()
    assert np.isin(cuts[cuts > a], e).all()


def test_records_that_are_not_kept_repeat_an_end():
    e = np.repeat(cc.ends(cc.fixed_shapes()["fastq_331_over_3G_100"]), 3)
    assert mk.bgzf_record_cuts(e).tolist() == cc.rule(np.unique(e)).tolist()


def test_random_length_mixes():
    for lens in cc.random_shapes(2000, seed=20261019):
        e = cc.ends(lens)
        cuts = mk.bgzf_record_cuts(e)
        assert cuts.tolist() == cc.rule(e).tolist()
        cc.check_properties(cuts, e)


def test_capacity_and_order_are_reported():
    import ctypes as C
    L_ = mk.load()
    e = cc.ends([G, 500])
    out, n = np.zeros(2, dtype=np.uint64), C.c_uint64(0)
    assert L_.mk_bgzf_record_cuts(e.ctypes.data, e.size, out.ctypes.data, 2, C.byref(n)) == mk.MK_E_CAPACITY and n.value == 3
    bad = np.array([10, 5], dtype=np.uint64)
    assert L_.mk_bgzf_record_cuts(bad.ctypes.data, 2, out.ctypes.data, 2, C.byref(n)) == mk.MK_E_INVALID_ARG
