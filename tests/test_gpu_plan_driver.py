"""The 4-state list driver, live and dry: ONE (fused_plan.hip: pllhip_fused_plan_walk over pllhip_fused_plan_list).

pllhip_update_partials plans a list with the driver the device-less entry point pllhip_fused_plan_dry_edge plans it with,
so what the dry call says of a list -- which ops are deferred, whether the hinted edge is folded into the launch -- is
what the live call does.  The live side is read through the counters the library already has: pll_amd_deferred_stats
(ops deferred by the call; a CLV that is deferred is materialised, and counted, when it is read back) and
pll_amd_edge_fold_stats (lists launched with the epilogue).

8 balanced and 17 random tips, 1,000 sites, 4 categories, per-site scale buffers, PLLHIP_FUSED=2.  The dry entry point
plans one segment, so the live call is held to one too (PLLHIP_FUSED_SEGMENTS=1, as in test_gpu_edge_fold.py): a list
of two segments is never folded.  The second traversal is the one compared: it meets the first one's deferred cherries
(the dry call's old_deferred / old_scaler) and the hint the edge evaluation left.

The steps behind the plan -- parents left unstored, parents folded into their reader, the list planned once more -- are
held to pllhip_fused_plan_dry_folded by the last test, through pll_amd_unstored_stats and pll_amd_pair_fold_stats.
"""
import numpy as np
import pytest

from helpers import make_case, build_partition
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
from test_host_edge_fold_plan import _dry_edge
from test_host_pair_fold_plan import _call as _dry_folded

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_whole_list_launch(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    monkeypatch.delenv("PLLHIP_FUSED_WGS", raising=False)


def _inner_root(plan, cherry_end):
    """A traversal directed at an inner-inner edge neither end / one end of which is a cherry: (ops, edge, cherry parents)."""
    view = W.UnrootedView(plan)
    for a, b in sorted(view.edges()):
        if a < plan.tips:
            continue
        ops, edge = view.traversal((a, b))
        cherries = {int(op["parent_clv_index"]) for op in ops
                    if op["child1_clv_index"] < plan.tips and op["child2_clv_index"] < plan.tips}
        if len({a, b} & cherries) == (1 if cherry_end else 0):
            return ops, edge, cherries
    raise AssertionError("no such edge")


@pytest.mark.parametrize("shape,tips", [("balanced", 8), ("random", 17)])
@pytest.mark.parametrize("cherry_end", [False, True])
def test_live_call_does_what_the_dry_call_says(gpu, shape, tips, cherry_end):
    """cherry_end False: the hinted edge joins two stored CLVs, and is folded; True: one end is a cherry, which the
    evaluation materialises and the second traversal defers again -- no CLV in HBM, no fold."""
    case = make_case(4, shape, tips, 1000, rate_cats=4, seed=5)
    plan = case["plan"]
    p = build_partition(gpu, case, ATTRIB_PATTERN_TIP)
    p.set_deferral(True)
    p.set_edge_fold(True)
    ops, edge, cherries = _inner_root(plan, cherry_end)
    fi = [0] * 4
    # the first traversal defers every cherry and folds nothing (no hint yet); the evaluation materialises the
    # cherries it reads and leaves the hint
    p.update_partials(ops)
    lnl = p.compute_edge_loglikelihood(*edge, fi)
    st0, ef0 = p.deferred_stats(), p.edge_fold_stats()
    still = cherries - {edge[0], edge[2]}
    assert st0["deferred_now"] == len(still) and st0["materialised"] == len(cherries) - len(still) and ef0[0] == 0, (st0, ef0)
    nclv = plan.tips + plan.clv_buffers
    old, old_sc = np.zeros(nclv, dtype=np.uint8), np.full(nclv, -1, dtype=np.int32)
    for c in still:
        old[c], old_sc[c] = 1, c - plan.tips
    dry = _dry_edge(gpu, ops, plan, edge[:4], rate_cats=4, old=old, old_sc=old_sc)
    assert dry["rc"] == 0
    # the second one is planned again (the hint is new), with the driver the dry call has just run
    p.update_partials(ops)
    st1, ef1 = p.deferred_stats(), p.edge_fold_stats()
    print("%s %d: dry defers %r, folds %d (edge_out %r); live deferred %d ops, folded %d" %
          (shape, tips, dry["deferred"], dry["edge"][0], dry["edge"], st1["ops_deferred"] - st0["ops_deferred"], ef1[0] - ef0[0]))
    assert st1["ops_deferred"] - st0["ops_deferred"] == len(dry["deferred"])
    assert st1["deferred_now"] == len(dry["deferred"])
    assert ef1[0] - ef0[0] == dry["edge"][0], "the live call folds the edge exactly when the dry call does"
    # which ops: reading a CLV back materialises it exactly if it is deferred
    dry_deferred = {int(ops[i]["parent_clv_index"]) for i in dry["deferred"]}
    live_deferred = set()
    for op in ops:
        node = int(op["parent_clv_index"])
        before = p.deferred_stats()["materialised"]
        p.get_clv(node)
        if p.deferred_stats()["materialised"] > before:
            live_deferred.add(node)
    assert live_deferred == dry_deferred
    assert p.compute_edge_loglikelihood(*edge, fi) == lnl
    assert dry_deferred and dry["edge"][0] == (0 if cherry_end else 1), "the case is meant to defer, and to fold or not"
    p.destroy()


@pytest.mark.parametrize("shape,tips", [("random", 17), ("balanced", 16)])
def test_live_call_leaves_unstored_and_folds_what_the_dry_call_says(gpu, shape, tips):
    """ONE driver (fused_plan.hip: pllhip_fused_plan_walk) takes a list through plan, unstored, fold, plan once more and
    unstored again, for pllhip_update_partials and for pllhip_fused_plan_dry_folded alike: the parents the dry call
    says are deferred, left unstored and folded are the ones the live call does not have in HBM, each for that reason.
    40 sites (three tiles of 16 at 4 categories, the last ragged), per-site scale buffers, one full traversal."""
    case = make_case(4, shape, tips, 40, rate_cats=4, seed=5)
    plan = case["plan"]
    ops, fi = plan.ops, [0] * 4
    p = build_partition(gpu, case, ATTRIB_PATTERN_TIP)
    p.set_deferral(True)
    p.set_unstored_pairs(True)
    p.set_pair_fold(True)
    dry = _dry_folded(gpu, "pllhip_fused_plan_dry_folded", ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0, None,
                      None, True)
    assert dry["rc"] == 0
    print("%s %d: %d ops, dry defers %r, folds %r, leaves unstored %r" %
          (shape, tips, len(ops), dry["deferred"], dry["folded"], dry["unstored"]))
    assert dry["deferred"] and dry["folded"], "the case is meant to defer and to fold"
    assert dry["unstored"] or shape != "random", "the random tree is meant to leave walked parents unstored"
    p.update_partials(ops)
    assert p.deferred_stats()["ops_deferred"] == len(dry["deferred"])
    assert p.pair_fold_stats()["folded_now"] == len(dry["folded"])
    # (a folded parent is an unstored pair product as well)
    assert p.unstored_stats()["unstored_now"] == len(dry["unstored"]) + len(dry["folded"])
    # which CLVs: reading one back materialises it, and counts it, exactly if it was not in HBM
    live = {"deferred": set(), "unstored": set(), "folded": set()}
    for op in ops:
        node = int(op["parent_clv_index"])
        before = (p.deferred_stats()["materialised"], p.unstored_stats()["materialised"], p.pair_fold_stats()["materialised"])
        p.get_clv(node)
        after = (p.deferred_stats()["materialised"], p.unstored_stats()["materialised"], p.pair_fold_stats()["materialised"])
        rose = tuple(a - b for a, b in zip(after, before))
        assert rose in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 1)), (node, rose)
        if rose != (0, 0, 0):
            live["deferred" if rose[0] else "folded" if rose[2] else "unstored"].add(node)
    for what in live:
        assert live[what] == {int(ops[i]["parent_clv_index"]) for i in dry[what]}, what
    # the same bits as a partition that defers, leaves unstored and folds nothing
    q = build_partition(gpu, case, ATTRIB_PATTERN_TIP)
    q.set_deferral(False)
    q.set_unstored_pairs(False)
    q.set_pair_fold(False)
    q.update_partials(ops)
    assert p.compute_edge_loglikelihood(*plan.root_edge, fi) == q.compute_edge_loglikelihood(*plan.root_edge, fi)
    p.destroy()
    q.destroy()
