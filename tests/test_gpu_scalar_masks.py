"""The 4-state whole-list kernel's scaling decisions as wave masks and its pair indices joined in scalar registers
(partials_fused.hpp: pllhip_fused_group_mask, pllhip_fused_pair_index), on the GPU.

Every case runs the fold / walk / eager partitions of tests/test_gpu_pair_fold.py next to the oracle and compares every
CLV and scale buffer bit for bit, and the lnL.  Two and a half tiles of sites at every rate-category count (40 at 4
categories: three tiles of 16, the last one ragged).

Mixed decisions inside a wave.  A balanced 16-taxon tree; pendant branches of 1e-100, so that a cherry whose tips differ
(A against C) is ~1e-100 in every entry and a cherry of two gaps or two equal characters is O(1):
  - a folded product (cherry, cherry) scales where at least one of its cherries mismatches (then ~1e-23 scaled, or
    ~1e-123 where both do),
  - its reader's own test fires where one of its two products had two mismatching cherries.
The columns repeat with period 4 -- per reader: nothing | cherry 0 | cherries 2, 3 | cherries 0, 1, 2 -- so the left
product scales at sites 1, 3 (mod 4), the right one at 2, 3, the reader at 2, 3; the second reader's columns are the
same pattern two sites on.  Every sub-step width (4, 8, 16, 32 sites) is a multiple of 4, so in every tile half the
sites scale and half do not, neighbours inside a sub-step differ, and so do the two sites either side of the boundary
between the sub-steps.  `_assert_mixed` checks exactly that on the ORACLE's scalers before anything is compared.
"""
import numpy as np
import pytest

from helpers import TREES, make_case
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_gpu_pair_fold import Trio, _cherries, _dry, _kids, _whole_list_kernel  # noqa: F401 (the environment fixture)

pytestmark = pytest.mark.gpu
ATTRS = ATTRIB_PATTERN_TIP
J = 2
SHORT = 1e-100
SITES = {1: 160, 2: 80, 4: 40, 8: 20}  # two and a half tiles of J * 64 / (2 * rate_cats) sites
# per reader and column (site % 4): which of its four cherries mismatch
MISMATCH = ((), (0,), (2, 3), (0, 1, 2))
CODES16 = b"ACGTMRWSYKVHDBN-"


def _levels(plan):
    """(cherries, products, readers) of the balanced 16-taxon plan: ops by parent CLV"""
    by_parent = {int(op["parent_clv_index"]): op for op in plan.ops}
    cherries = _cherries(plan)
    products = {p: op for p, op in by_parent.items() if p not in cherries and all(k in cherries for k in _kids(op))}
    readers = {p: op for p, op in by_parent.items() if all(k in products for k in _kids(op))}
    assert len(cherries) == 8 and len(products) == 4 and len(readers) == 2
    return cherries, products, readers


def mixed_case(rate_cats, scalers=True, sites=None):
    sites = SITES[rate_cats] if sites is None else sites
    case = make_case(4, "balanced", 16, sites, rate_cats=rate_cats, seed=7)
    plan = case["plan"] = TREES["balanced"](16, seed=7, use_scalers=scalers)
    cherries, products, readers = _levels(plan)
    seqs = [bytearray(b"-" * sites) for _ in range(plan.tips)]
    for r, reader in enumerate(sorted(readers)):
        four = [c for p in _kids(readers[reader]) for c in _kids(products[p])]
        for site in range(sites):
            column = (site + 2 * r) % 4
            for n, c in enumerate(four):
                a, b = _kids(cherries[c])
                if n in MISMATCH[column]:
                    seqs[a][site], seqs[b][site] = ord("A"), ord("C")
                elif (site // 4) % 2:          # equal characters instead of two gaps, every other group of four
                    seqs[a][site] = seqs[b][site] = b"GT"[n % 2]
    case["seqs"] = [bytes(s) for s in seqs]
    return case


def short_matrices(plan):
    """the cherries' pendant branches"""
    return sorted({int(op["child%d_matrix_index" % k]) for op in _cherries(plan).values() for k in (1, 2)})


def _assert_mixed(bits, sps, what):
    bits = np.asarray(bits).astype(np.int64)
    assert set(np.unique(bits)) <= {0, 1}, (what, np.unique(bits))
    ts = J * sps
    for t0 in range(0, len(bits), ts):
        tile = bits[t0:t0 + ts]
        k = int(tile.sum())
        assert 4 * k >= len(tile) and 4 * (len(tile) - k) >= len(tile), "%s: tile at site %d scales %d of %d" % (what, t0, k, len(tile))
        for s0 in range(0, len(tile), sps):
            sub = tile[s0:s0 + sps]
            assert (sub[1:] != sub[:-1]).any(), "%s: tile at %d, sub-step at %d: one decision for all" % (what, t0, s0)
        if len(tile) > sps:
            assert tile[sps - 1] != tile[sps], "%s: tile at %d: the same decision either side of the sub-step boundary" % (what, t0)


def assert_oracle_is_mixed(o, plan, rate_cats, per_rate=False):
    """the conditions of the module's docstring, at the folded products and at their readers, on the oracle's counts"""
    cherries, products, readers = _levels(plan)
    sps = 64 // (2 * rate_cats)

    def counts(op):
        c = np.asarray(o.scalers[int(op["parent_scaler_index"])]).astype(np.int64)
        if per_rate:
            c = c.reshape(-1, rate_cats)
            assert (c == c[:, :1]).all(), "the categories of a site decide alike here"
            c = c[:, 0]
        return c
    for c in cherries.values():
        assert not counts(c).any(), "a tip-tip op never scales"
    for p, op in products.items():
        _assert_mixed(counts(op), sps, "product %d" % p)
    for r, op in readers.items():
        own = counts(op) - sum(counts(products[p]) for p in _kids(op))
        _assert_mixed(own, sps, "reader %d" % r)


def _run_mixed(gpu, orc, rate_cats, attrs=ATTRS, scalers=True, defers=True):
    case = mixed_case(rate_cats, scalers)
    t = Trio(gpu, orc, case, attrs)
    mis = short_matrices(t.plan)
    # (without scale buffers nothing decides anything, and 1e-100 four times over would leave the doubles' range)
    t.matrices(mis, np.full(len(mis), SHORT if scalers else 1e-30))
    t.o.update_partials()
    if scalers:
        assert_oracle_is_mixed(t.o, t.plan, rate_cats, per_rate=bool(attrs & ATTRIB_RATE_SCALERS))
    t.update()
    if defers:
        d = _dry(gpu, t.plan, rate_cats=rate_cats)
        assert len(d["folded"]) == 4 and d["operands"] == [[3, 3], [3, 3]]
        assert t.folded() == 4 and t.fold.unstored_stats()["unstored_now"] == 4
        assert t.fold.deferred_stats()["deferred_now"] == 8
        assert t.walk.pair_fold_stats()["folded_now"] == 0 and t.walk.unstored_stats()["unstored_now"] == 4
        assert t.eager.unstored_stats()["unstored_now"] == 0
    else:
        assert t.folded() == 0 and t.fold.unstored_stats()["unstored_now"] == 0
        assert t.fold.deferred_stats()["deferred_now"] == 0
    t.lnl()
    t.read_everything()
    # once more through the kept plan
    t.update()
    t.lnl()
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_mixed_decisions_per_site(gpu, orc, rate_cats):
    _run_mixed(gpu, orc, rate_cats)


def test_mixed_decisions_per_rate_scalers(gpu, orc):
    """ATTRIB_RATE_SCALERS: groups of two lanes, no deferral"""
    _run_mixed(gpu, orc, 4, attrs=ATTRS | ATTRIB_RATE_SCALERS, defers=False)


def test_mixed_decisions_8_categories(gpu, orc):
    """groups of sixteen lanes, no deferral"""
    _run_mixed(gpu, orc, 8, defers=False)


@pytest.mark.parametrize("rate_cats", [1, 4])
def test_mixed_columns_without_scale_buffers(gpu, orc, rate_cats):
    _run_mixed(gpu, orc, rate_cats, scalers=False)


def _all_codes(case, constant_row):
    """every tip row drawn from all sixteen characters, a seed per row; one row constant"""
    codes = np.frombuffer(CODES16, dtype=np.uint8)
    seqs = []
    for i in range(case["plan"].tips):
        rng = np.random.default_rng(9000 + i)
        seqs.append(codes[rng.integers(0, 16, size=case["sites"])].tobytes())
    seqs[constant_row] = b"R" * case["sites"]
    case["seqs"] = seqs


@pytest.mark.parametrize("rate_cats", [1, 4])
def test_pair_indices_all_codes(gpu, orc, rate_cats):
    """4 categories: a sub-step's characters are two words of a row; 1 category: eight words from two lanes"""
    case = make_case(4, "balanced", 16, SITES[rate_cats], rate_cats=rate_cats, seed=7)
    case["plan"] = TREES["balanced"](16, seed=7, use_scalers=True)
    _all_codes(case, constant_row=_kids(sorted(_cherries(case["plan"]).items())[2][1])[1])
    assert len({bytes(s) for s in case["seqs"]}) == 16
    t = Trio(gpu, orc, case)
    t.update()
    assert t.folded() == 4 and t.fold.deferred_stats()["deferred_now"] == 8
    t.lnl()
    t.read_everything()
    t.destroy()


def test_pair_indices_more_rows_than_a_batch(gpu, orc):
    """70 tips at 4 categories: more tip rows than the 64 a wave's character registers hold -- the batch switch runs"""
    case = make_case(4, "random", 70, 40, rate_cats=4, seed=11)
    case["plan"] = TREES["random"](70, seed=11, use_scalers=True)
    _all_codes(case, constant_row=_kids(sorted(_cherries(case["plan"]).items())[0][1])[0])
    t = Trio(gpu, orc, case)
    d = _dry(gpu, t.plan)
    t.update()
    assert t.folded() == len(d["folded"]) > 0
    assert t.fold.deferred_stats()["deferred_now"] == len(_cherries(t.plan)) > 0
    assert t.fold.unstored_stats()["unstored_now"] >= t.folded()
    t.lnl()
    t.read_everything()
    t.destroy()
