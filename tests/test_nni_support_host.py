"""Branch supports without a GPU.

* pll_amd_nni_support_counts (host only: no device, no partition) against the rule written out in Python
  (tests/support_data.py: counts_of): random tables, exact ties among the cs, delta exactly on the threshold (not
  counted), negative delta, a NaN column, a -inf column, one replicate.
* The yardstick of tests/test_gpu_nni_support.py on partitions of the genuine reference, for the small cases of
  tests/test_nni_host.py: its centres agree with the call sequence's log-likelihoods within the project's bars (1e-12;
  20 states 1e-11), and the inputs discriminate -- over the tested edges sh_count takes at least three distinct values,
  one edge has delta < 0 and count 0, one has a count above half the replicates.  The seeds: cases seed 3 (as in
  test_nni_host.py), replicate weights default_rng(WEIGHT_SEED), REPLICATES multinomial resamples.
"""
import math

import numpy as np
import pytest

import nni_data as N
import replicate_data as RD
import support_data as SD
from test_nni_host import SMALL, case_of

WEIGHT_SEED = 5
REPLICATES = 100


def check(amd, c, table, epsilon):
    want = SD.counts_of(c, table, epsilon)
    got = amd.nni_support_counts(c, table, epsilon)
    assert got == want, (got, want, c, epsilon)
    return got


def test_counts_random_tables(amd):
    rng = np.random.default_rng(1)
    seen = set()
    for count in (1, 2, 63, 64, 65, 130, 1000):
        for _ in range(20):
            c = -1000.0 + rng.normal(0, 3.0, 3)
            if rng.random() < 0.7:
                c[0] = c.max() + rng.uniform(0, 4.0)
            table = c[:, None] + rng.normal(0, 2.0, (3, count))
            for eps in (0.0, 0.1, 1.5):
                sh, lbp = check(amd, c, table, eps)
                seen.add((sh > 0, sh == count, lbp > 0))
    assert len(seen) >= 4, seen


def test_counts_ties(amd):
    # cs: exact ties between the two largest (gap 0), between the two smallest, among all three
    c = np.array([-100.0, -101.0, -103.0])
    cs = np.array([[0.5, 0.5, -1.0], [2.0, -0.25, -0.25], [0.75, 0.75, 0.75], [-1.0, 0.5, 0.5]]).T   # [3][4]
    table = c[:, None] + cs
    assert ((table - c[:, None]) == cs).all()   # (exactly representable: the ties are ties in the call too)
    for eps in (0.0, 0.5, 1.0, 1.5):
        sh, _ = check(amd, c, table, eps)
        # delta = 1: gaps 0, 2.25, 0, 0
        assert sh == (3 if eps < 1.0 else 0)


def test_counts_threshold_is_not_counted(amd):
    # delta = 2 exactly; replicate gaps 0.5, 1.5, 2.0: with epsilon 0.5 the second sits on the threshold
    c = np.array([-10.0, -12.0, -14.0])
    cs = np.array([[1.0, 0.5, -3.0], [1.0, -0.5, -3.0], [1.0, -1.0, -3.0]]).T
    table = c[:, None] + cs
    assert ((table - c[:, None]) == cs).all()
    assert check(amd, c, table, 0.5)[0] == 1
    assert check(amd, c, table, 0.0)[0] == 2      # gap 2.0 = delta: not counted
    assert check(amd, c, table, 0.25)[0] == 2
    assert check(amd, c, table, 1.5)[0] == 0      # gap 0.5 + 1.5 = delta: not counted


def test_counts_negative_delta(amd):
    rng = np.random.default_rng(2)
    c = np.array([-50.0, -49.0, -55.0])
    table = c[:, None] + rng.normal(0, 1.0, (3, 200))
    sh, lbp = check(amd, c, table, 0.0)
    assert sh == 0 and 0 < lbp < 200
    # gaps of exactly 0 do not help a negative delta either
    assert check(amd, c, np.repeat(c[:, None], 5, axis=1), 0.0) == (0, 0)


@pytest.mark.parametrize("bad", [math.nan, -math.inf], ids=["nan", "minus-inf"])
@pytest.mark.parametrize("row", [0, 1, 2])
def test_counts_bad_column(amd, bad, row):
    rng = np.random.default_rng(3)
    c = np.array([-20.0, -23.0, -24.0])
    table = c[:, None] + rng.normal(0, 0.5, (3, 64))
    table[row, ::2] = bad
    sh, lbp = check(amd, c, table, 0.0)
    if math.isnan(bad):
        assert sh <= 32 and lbp <= 32
    # the whole row, and a centre
    table[row, :] = bad
    sh, lbp = check(amd, c, table, 0.0)
    if math.isnan(bad):
        assert sh == 0 and lbp == 0
    c2 = c.copy()
    c2[row] = bad
    check(amd, c2, c[:, None] + rng.normal(0, 0.5, (3, 64)), 0.0)
    check(amd, c2, table, 0.0)


def test_counts_one_replicate_and_refusals(amd):
    c = np.array([-5.0, -9.0, -9.5])
    assert check(amd, c, c[:, None] + np.array([[0.0], [1.0], [0.5]]), 0.0) == (1, 1)
    assert check(amd, c, c[:, None] + np.array([[0.0], [4.5], [0.5]]), 0.0) == (0, 0)
    import ctypes as C
    out = np.full(2, 77, dtype=np.uint32)
    t = np.zeros((3, 4))
    for args in ((None, t.ctypes.data, 4, 0.0), (c.ctypes.data, None, 4, 0.0), (c.ctypes.data, t.ctypes.data, 0, 0.0),
                 (c.ctypes.data, t.ctypes.data, 4, -1.0), (c.ctypes.data, t.ctypes.data, 4, math.nan),
                 (c.ctypes.data, t.ctypes.data, 4, math.inf)):
        assert amd.lib.pll_amd_nni_support_counts(*args, out[:1].ctypes.data, out[1:].ctypes.data) == 0, args
        assert (out == 77).all()
    assert C.sizeof(C.c_uint) == 4


@pytest.mark.parametrize("name", list(SMALL))
def test_yardstick_on_the_reference(ref, name):
    case = case_of(name)
    r = N.build(ref, case)
    try:
        edges = N.nni_edges(case)
        terms = SD.persite_table(r, case, edges)
        own = RD.own_weights(r)
        assert (own == case.pw).all()
        c = SD.centres(terms, own)
        tol = 1e-11 if case.states == 20 else 1e-12
        worst = 0.0
        for i, edge in enumerate(edges):
            for k in range(3):
                want = N.sequence_lnl(r, case, edge, k)
                worst = max(worst, abs(c[i, k] - want) / abs(want))
                assert abs(c[i, k] - want) <= tol * abs(want), (i, k, c[i, k], want)
        weights = SD.bootstrap_weights(case, np.random.default_rng(WEIGHT_SEED), REPLICATES)
        table = SD.rell(terms, weights)
        stats = [SD.statistics(c[i], table[i], 0.0) for i in range(len(edges))]
        sh = [s[2] for s in stats]
        print("%s: centres within %.2e of the sequence; delta %s, sh_count %s, lbp_count %s"
              % (name, worst, ["%.3f" % s[0] for s in stats], sh, [s[3] for s in stats]))
        assert len(set(sh)) >= 3, sh
        assert any(s[0] < 0 and s[2] == 0 for s in stats)
        assert any(s[2] > REPLICATES // 2 for s in stats)
        assert all(0.0 <= s[1] <= 1.0 for s in stats)
    finally:
        r.destroy()
