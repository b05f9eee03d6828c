"""The cut rule of BGZF members that end at record ends (include/merkurio_hip.h), restated in numpy, and the record-length shapes
the tests of mk_bgzf_record_cuts (host) and of the device cut kernel (mk_bgzf_deflate_records) share."""
import numpy as np

G, L = 49152, 65280  # the grid step, the most text a member holds


def rule(rec_end):
    """0, the distinct snap(k * G) for k = 1 .. ceil(T / G) - 1 in increasing order, T"""
    e = np.asarray(rec_end, dtype=np.int64)
    T = int(e[-1]) if e.size else 0
    x = np.arange(1, -(-T // G), dtype=np.int64) * G
    first = e[np.searchsorted(e, x, side="left")] if x.size else x  # the smallest record end >= x
    snap = np.where(first < x + (L - G), first, x)
    return np.unique(np.concatenate([[0], snap, [T]])).astype(np.uint64)


def ends(lengths):
    return np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)


def fixed_shapes():
    """name -> record lengths"""
    fill = lambda total, rec=331: [rec] * (total // rec) + ([total % rec] if total % rec else [])
    return {
        "one_byte": [1],
        "fastq_331_over_3G_100": fill(3 * G + 100),
        "end_at_G": [G, 500],
        "end_at_G_minus_1": [G - 1, 500, 500],
        "end_at_G_plus_reach_minus_1": [1000, L - 1000 - 1, 700],  # the record that spans G ends at G + (L - G) - 1: it snaps
        "end_at_G_plus_reach": [1000, L - 1000, 700],              # ... at G + (L - G): a raw cut at G
        "long_record_between_short": fill(46000) + [200000] + fill(40000),  # raw cuts every G inside it, a snap at its end (5 G + 240)
        # a record end can be the snap of one grid point only (snap(x) < x + (L - G) <= x + G); what can coincide is the last grid
        # point's snap with T: the text ends inside the last grid point's reach, on the record that spans it
        "last_snap_is_T": fill(2 * G - 100) + [400],
        "two_grid_points_one_record": [100, 2 * G + 20000, 50],  # both grid points lie in one record: two raw cuts, then T
        "grid_multiple": fill(2 * G, 256),
        "65_grid_points": fill(65 * G + 77),  # one more grid point than a wave has lanes
    }


def random_shapes(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        kind = int(rng.integers(0, 4))
        k = int(rng.integers(1, 60))
        if kind == 0:
            lens = rng.integers(1, 700, size=k * 20)
        elif kind == 1:
            lens = rng.integers(1, 3 * G, size=k)
        elif kind == 2:  # short records with a few chromosome-sized ones between them
            lens = rng.integers(1, 400, size=k * 30)
            lens[rng.integers(0, lens.size, size=3)] = rng.integers(L - G - 3, 5 * G, size=3)
        else:  # ends on and around the grid points and the reach's edge
            at = np.sort(np.unique(np.concatenate([np.arange(1, k + 1) * G + d for d in rng.choice([-1, 0, 1, L - G - 1, L - G, L - G + 1], size=3)])))
            lens = np.diff(np.concatenate([[0], at]))
            lens = lens[lens > 0]
        yield lens.astype(np.uint64)


def check_properties(cuts, rec_end):
    """what the rule promises of any text"""
    cuts = np.asarray(cuts, dtype=np.int64)
    e = np.asarray(rec_end, dtype=np.int64)
    T = int(e[-1]) if e.size else 0
    assert cuts[0] == 0 and cuts[-1] == T
    gaps = np.diff(cuts)
    assert (gaps > 0).all() and (gaps <= L).all()
    raw = cuts[1:-1][~np.isin(cuts[1:-1], e)]
    if raw.size:  # every cut that is no record end lies inside a record longer than L - G
        r = np.searchsorted(e, raw, side="left")
        start = np.where(r > 0, e[np.maximum(r, 1) - 1], 0)
        assert (e[r] - start > L - G).all()
