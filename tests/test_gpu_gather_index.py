"""Index delivery of the 4-state whole-list kernel (DESIGN.md 2.0 "Tips", "Quad rows", 8.4h): the tile's character batch
lies in the wave's LDS, and every gathered factor's lane reads the table index of its site from there -- a quad row's
16-bit class, a pair row's byte, a single tip's nibble as the table's first or second character -- by ONE rule
(pllhip_fused_index, partials_fused.hpp; its host side: tests/test_host_gather_index.py).

Every case runs the default partition (quads on at one site per class) next to the quads-off twin, the per-level twin
and the oracle, as tests/test_gpu_quad_fold.py does: every CLV and every scale buffer bit for bit against all three, the
twins' edge lnL equal, the oracle's to 1e-12 relative (the result calls' tolerance).

Sites 1, 15, 16, 17, 33: less than a tile of every instance, one short of the 4-category tile, the tile, one more, two
tiles and one; 700: the four tips of every quad run through all 625 patterns over A, C, G, T and the gap plus 75 repeats,
shuffled -- class numbers beyond 255 (a dropped high byte shows) and neighbouring sites of a tile in different classes.
The shorter alignments are the first columns of the same.

Trees (the planner's answer for each is asserted from the statistics, so that a case cannot pass on another path):
  rooted 16   a balanced clade of 16 tips under one more op: its root reads two folded parents over two quads each --
              four wide gathers, the second to fourth from displaced tables
  rooted 8    the same of 8 tips: its root is a gathered-gathered op over two quads
  quad+tips   a quad read next to a slot whose value tip-inner ops made, the tips as child 1 (the table's first
              character: nibble, shift 4) or child 2 (shift 0)
  cherry+inner  a cherry read next to an inner node: a pair row's byte
  caterpillar 70  more than 64 tip operands: the batch switch refills the block in the middle of the list
"""
import numpy as np
import pytest

from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_gpu_pair_rows import Twins, _case, _cherries, _kids
from test_gpu_quad_rows import Quads

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP
SITES = (1, 15, 16, 17, 33, 700)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


# ---- the trees
def _rooted_balanced(n, tip_of=None):
    """a balanced clade over tips 0 .. n - 1 (tip_of: in another order), its root R joined with tip n; the root edge
    leads to tip n + 1 -- R is an op of the list with a reader, not an end of the root edge"""
    t = n + 2
    level = [i if tip_of is None else tip_of[i] for i in range(n)]
    joins, nxt = [], t
    while len(level) > 1:
        new = []
        for i in range(0, len(level), 2):
            joins.append((nxt, level[i], level[i + 1]))
            new.append(nxt)
            nxt += 1
        level = new
    joins.append((nxt, level[0], n))
    return W._assemble(t, joins, (nxt, n + 1), W.SplitMix64(5), "rooted-balanced")


def _side(tip, inner, child):
    return (tip, inner) if child == 1 else (inner, tip)


def _quad_and_tips(child):
    """the quad over tips 0 .. 3 read next to a slot: ((4, 5), 6), 7 -- a cherry, then two tip-inner steps --, and one more
    tip-inner op above the reader; the single tips as child `child`"""
    t = 10
    joins = [(t, 0, 1), (t + 1, 2, 3), (t + 2, t, t + 1), (t + 3, 4, 5), (t + 4, *_side(6, t + 3, child)),
             (t + 5, *_side(7, t + 4, child)), (t + 6, t + 2, t + 5), (t + 7, *_side(8, t + 6, child))]
    return W._assemble(t, joins, (t + 7, 9), W.SplitMix64(5), "quad-and-tips")


def _cherry_and_inner():
    """the cherry (0, 1) read next to an inner node, ((2, 3), 4), 5"""
    t = 8
    joins = [(t, 0, 1), (t + 1, 2, 3), (t + 2, t + 1, 4), (t + 3, t + 2, 5), (t + 4, t, t + 3), (t + 5, t + 4, 6)]
    return W._assemble(t, joins, (t + 5, 7), W.SplitMix64(5), "cherry-and-inner")


TREES = {
    "rooted16": lambda: _rooted_balanced(16),
    "rooted8": lambda: _rooted_balanced(8),
    "quad+tip1": lambda: _quad_and_tips(1),
    "quad+tip2": lambda: _quad_and_tips(2),
    "cherry+inner": _cherry_and_inner,
    "caterpillar70": lambda: W.caterpillar_tree(70, seed=7),
}
# tree: (quads taken = wide gathers of the list, quad products folded into their reader)
EXPECT = {"rooted16": (4, 2), "rooted8": (2, 0), "quad+tip1": (1, 0), "quad+tip2": (1, 0), "cherry+inner": (0, 0),
          "caterpillar70": (0, 0)}


# ---- the alignment
def _quad_tips(plan):
    """the four tips under every op over two cherries"""
    parent = {int(op["parent_clv_index"]): op for op in _cherries(plan)}
    return [_kids(parent[a]) + _kids(parent[b]) for a, b in (_kids(op) for op in plan.ops) if a in parent and b in parent]


def _columns(seed):
    """700 columns of four characters: every pattern over A, C, G, T, - once and 75 of them twice, shuffled"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([np.arange(625), rng.choice(625, 75, replace=False)])
    rng.shuffle(v)
    return [bytes(b"ACGT-"[(int(x) // 5 ** d) % 5] for x in v) for d in range(4)]


def _all_patterns(case, sites, tips_of_quads=None):
    seqs = [bytearray(s) for s in case["seqs"]]
    for q, tips in enumerate(_quad_tips(case["plan"]) if tips_of_quads is None else tips_of_quads):
        for tip, column in zip(tips, _columns(31 + q)):
            seqs[tip][:] = column[:sites]
    case["seqs"] = [bytes(s) for s in seqs]
    return case


def _new_case(tree, sites, rate_cats):
    plan = TREES[tree]()
    return _all_patterns(_case("random", plan.tips, sites, rate_cats, plan=plan), sites)


def test_the_700_columns():
    cols = _columns(31)
    patterns = list(zip(*cols))
    assert len(patterns) == 700 and len(set(patterns)) == 625
    assert all(a != b for a, b in zip(patterns, patterns[1:])), "neighbouring sites differ"


# ---- the cases
@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_trees(gpu, orc, monkeypatch, tree, rate_cats, sites):
    t = Quads(gpu, orc, monkeypatch, _new_case(tree, sites, rate_cats))
    t.update()
    taken, folded = EXPECT[tree]
    got = t.p.quad_list_stats()
    assert (got["taken"], got["wide_gathers"]) == (taken, taken), (tree, sites, got)
    assert t.p.quad_fold_stats()["live"] == folded, (tree, sites, t.p.quad_fold_stats())
    assert t.z.quad_list_stats()["wide_gathers"] == 0
    if sites == 700 and taken:
        assert t.p.quad_row_stats()["refused"] == 0, "625 classes: below the cap, and beyond a byte"
    t.check()
    t.p.update_partials(t.plan.ops)     # the kept plan replayed
    t.z.update_partials(t.plan.ops)
    t.check()
    t.destroy()


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats,attrs", [(8, PT), (4, PT | ATTRIB_RATE_SCALERS)])
@pytest.mark.parametrize("tree", ["caterpillar70", "rooted16"])
def test_instances_that_never_defer(gpu, orc, monkeypatch, tree, rate_cats, attrs, sites):
    """8 rate categories and per-rate scale buffers: eager tip-tip ops through pair rows, tip-inner ops through shifted
    tip rows -- the byte forms of the same rule, no wide one"""
    t = Twins(gpu, orc, monkeypatch, _new_case(tree, sites, rate_cats), attrs)
    t.update()
    assert t.p.quad_list_stats()["wide_gathers"] == 0 and t.p.pair_row_stats()["live"] >= 1
    t.check()
    t.destroy()


@pytest.mark.parametrize("sites", [33, 700])
def test_two_lists_in_turn(gpu, orc, monkeypatch, sites):
    """one partition, two lists: the second pairs the tips another way -- other pair rows, other quad rows, other
    classes -- and the first comes back after it"""
    first = _rooted_balanced(16)
    second = _rooted_balanced(16, tip_of=[(5 * i + 3) % 16 for i in range(16)])
    assert {tuple(x) for x in _quad_tips(first)}.isdisjoint({tuple(x) for x in _quad_tips(second)})
    case = _case("random", first.tips, sites, 4, plan=first)
    t = Quads(gpu, orc, monkeypatch, _all_patterns(case, sites))
    for plan in (first, second, first):
        t.update(plan.ops)
        got = t.p.quad_list_stats()
        assert (got["taken"], got["wide_gathers"]) == (4, 4), got
        t.check(ops=plan.ops, edge=plan.root_edge)
    # (the second list's rows were built beside the first's: other rows, not the same ones again)
    assert t.p.quad_row_stats()["built"] >= 8
    t.destroy()
