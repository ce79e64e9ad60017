"""pll_amd_distance_from_counts -- the distance rule of pll_amd_pairwise_distances on one count table, host only --
against the rule of include/pll_amd.h restated in Python (rule() of tests/test_gpu_branch_lengths.py) over the
oracle's sumtable / derivatives on the expanded two-tip run Q (tests/distance_data.py).  No device.

Seeds: SEEDS below names the seed of every configuration.  test_seeds_are_well_conditioned holds each to the condition
the GPU file relies on: the yardstick run twice, once with every D(t) perturbed by up to 1e-12 relative, agrees with
itself in evals on at least 9 of 10 pairs and in the distance to `tolerance` on every pair."""
import ctypes as C
import math

import numpy as np
import pytest

import distance_data as DD
from distance_data import MAX_ITERS, MAX_LEN, MIN_LEN, TOL
from libpll_amd.pllapi import BRANCH_CONVERGED, BRANCH_MAX_ITERS, ERROR_PARAM_INVALID, PllError
from test_gpu_branch_lengths import lnl_tol, rule

# configuration -> seed (the GPU file's rate_cats = 1 configuration included)
SEEDS = {"dna-gtr-g4": 1, "dna-pinv": 2, "dna-matrix-per-category": 3, "aa-lg-g4": 4, "s5-3rates": 5, "dna-1rate": 6}
ALL_CONFIGS = dict(DD.CONFIGS, **{"dna-1rate": dict(states=4, rate_cats=1)})


def case_of(name):
    return DD.make_case(seed=SEEDS[name], **ALL_CONFIGS[name])


def pairs_of(case):
    return [(x, y) for x in range(case.tips) for y in range(x + 1, case.tips)]


def from_counts(amd, case, hm, masks, table, **kw):
    return amd.distance_from_counts(case.states, masks, table, hm["eigenvecs"], hm["inv_eigenvecs"], hm["eigenvals"],
                                    hm["freqs"], hm["rates"], hm["rate_weights"], hm["prop_invar"], **kw)


@pytest.mark.parametrize("name", list(DD.CONFIGS))
def test_equals_rule_over_oracle(amd, orc, name):
    case = case_of(name)
    codes, masks = DD.tip_codes(case, case.cmap(amd))
    hm = DD.host_model(amd, case)
    same = 0
    pairs = pairs_of(case)
    for x, y in pairs:
        table = DD.count_table(codes[x], codes[y], case.pw, len(masks))
        d, lnl, ev, st = from_counts(amd, case, hm, masks, table)
        q = DD.ExpandedRun(orc, amd, case, table, masks)
        t, ev_w, st_w = rule(q.D, DD.default_start(table, masks))
        assert abs(d - t) <= TOL, (x, y, d, t, ev, ev_w)
        assert abs(ev - ev_w) <= 1, (x, y, ev, ev_w)
        if ev == ev_w:
            assert st == st_w, (x, y, st, st_w)
            same += 1
        want = q.lnl(d)
        assert abs(lnl - want) <= lnl_tol(case.states) * abs(want), (x, y, lnl, want)
    assert 10 * same >= 9 * len(pairs), (same, len(pairs))


@pytest.mark.parametrize("name", list(ALL_CONFIGS))
def test_seeds_are_well_conditioned(amd, orc, name):
    case = case_of(name)
    codes, masks = DD.tip_codes(case, case.cmap(amd))
    same = 0
    pairs = pairs_of(case)
    for x, y in pairs:
        table = DD.count_table(codes[x], codes[y], case.pw, len(masks))
        start = DD.default_start(table, masks)
        t0, ev0, _ = rule(DD.ExpandedRun(orc, amd, case, table, masks).D, start)
        t1, ev1, _ = rule(DD.ExpandedRun(orc, amd, case, table, masks, perturb=1e-12, seed=x * 100 + y).D, start)
        assert abs(t0 - t1) <= TOL, (x, y, t0, t1)
        same += ev0 == ev1
    assert 10 * same >= 9 * len(pairs), (same, len(pairs))


def test_single_bin(amd, orc):
    case = case_of("dna-gtr-g4")
    hm = DD.host_model(amd, case)
    masks = np.arange(16, dtype=np.uint32)
    for a, b in [(1, 1), (1, 4), (5, 8), (15, 2)]:
        table = np.zeros(256, dtype=np.uint32)
        table[a * 16 + b] = 37
        d, lnl, ev, st = from_counts(amd, case, hm, masks, table)
        q = DD.ExpandedRun(orc, amd, case, table, masks)
        t, ev_w, st_w = rule(q.D, DD.default_start(table, masks))
        assert abs(d - t) <= TOL and ev == ev_w and st == st_w, (a, b, d, t, ev, ev_w, st, st_w)
        want = q.lnl(d)
        assert abs(lnl - want) <= 1e-12 * abs(want)
        if a & b:
            assert d <= MIN_LEN + TOL       # nothing speaks for a difference
        else:
            assert d > 5.0      # every column differs: the likelihood grows with t until a step falls below tolerance


@pytest.mark.parametrize("name", ["dna-gtr-g4", "dna-pinv", "aa-lg-g4"])
def test_identical_sequences(amd, orc, name):
    case = case_of(name)
    codes, masks = DD.tip_codes(case, case.cmap(amd))
    hm = DD.host_model(amd, case)
    x, y = case.duplicate
    table = DD.count_table(codes[x], codes[y], case.pw, len(masks))
    d, lnl, ev, st = from_counts(amd, case, hm, masks, table)
    q = DD.ExpandedRun(orc, amd, case, table, masks)
    t, ev_w, st_w = rule(q.D, 0.0)
    assert d <= MIN_LEN + TOL
    assert (ev, st) == (ev_w, st_w) and st == BRANCH_CONVERGED


def test_default_start(amd):
    case = case_of("dna-gtr-g4")
    codes, masks = DD.tip_codes(case, case.cmap(amd))
    hm = DD.host_model(amd, case)
    table = DD.count_table(codes[2], codes[5], case.pw, len(masks))
    start = DD.default_start(table, masks)
    assert 0.01 < start < 1.0
    a = from_counts(amd, case, hm, masks, table)
    b = from_counts(amd, case, hm, masks, table, start_length=start)
    assert a == b
    # one step from the default start is one step from that value, and the value is clamped by the rule's first line
    one = from_counts(amd, case, hm, masks, table, max_iters=1)
    assert one[2] == 1 and one[3] == BRANCH_MAX_ITERS and one == from_counts(amd, case, hm, masks, table, max_iters=1,
                                                                            start_length=start)
    lo = from_counts(amd, case, hm, masks, table, min_length=2 * start, max_iters=1)
    assert lo == from_counts(amd, case, hm, masks, table, min_length=2 * start, max_iters=1, start_length=2 * start)
    # an empty table starts at min_length and stays there
    d, lnl, ev, st = from_counts(amd, case, hm, masks, np.zeros(256, dtype=np.uint32))
    assert (d, lnl, ev, st) == (MIN_LEN, 0.0, 1, BRANCH_CONVERGED)


def test_parameter_errors(amd):
    case = case_of("dna-gtr-g4")
    codes, masks = DD.tip_codes(case, case.cmap(amd))
    hm = DD.host_model(amd, case)
    table = DD.count_table(codes[2], codes[5], case.pw, len(masks))
    for kw in [dict(min_length=0.0), dict(min_length=-1.0), dict(min_length=1.0, max_length=0.5),
               dict(max_length=math.inf), dict(min_length=math.nan), dict(tolerance=0.0), dict(tolerance=-1.0),
               dict(tolerance=math.nan), dict(max_iters=0), dict(start_length=math.inf),
               dict(start_length=-math.inf)]:
        amd.clear_error()
        with pytest.raises(PllError):
            from_counts(amd, case, hm, masks, table, **kw)
        assert amd.errno() == ERROR_PARAM_INVALID, kw
    bad = dict(hm, prop_invar=np.array([0.0, 1.0, 0.0, 0.0]))
    with pytest.raises(PllError):
        from_counts(amd, case, bad, masks, table)
    # NULL arrays and zero shapes, outputs untouched
    f = amd.lib.pll_amd_distance_from_counts
    R = case.rate_cats
    dp = C.POINTER(C.c_double)
    rows = [(dp * R)(*[a.ctypes.data_as(dp) for a in hm[k]])
            for k in ("eigenvecs", "inv_eigenvecs", "eigenvals", "freqs")]
    out = np.full(1, 7.0)
    good = [4, R, 16, masks.ctypes.data, table.ctypes.data] + [C.addressof(r) for r in rows] + \
           [hm["rates"].ctypes.data, hm["rate_weights"].ctypes.data, hm["prop_invar"].ctypes.data,
            MIN_LEN, MAX_LEN, TOL, MAX_ITERS, math.nan, out.ctypes.data, None, None, None]
    for i in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 17]:
        args = list(good)
        args[i] = 0 if i < 3 else None
        amd.clear_error()
        assert f(*args) == 0 and amd.errno() == ERROR_PARAM_INVALID, i
        assert out[0] == 7.0
    assert f(*good) == 1 and out[0] == from_counts(amd, case, hm, masks, table)[0]
