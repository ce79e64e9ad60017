"""The 4-state list driver, live and dry: ONE (fused_plan.hip: pllhip_fused_plan_list).

pllhip_update_partials plans a list with the driver the device-less entry point pllhip_fused_plan_dry_edge plans it with,
so what the dry call says of a list -- which ops are deferred, whether the hinted edge is folded into the launch -- is
what the live call does.  The live side is read through the counters the library already has: pll_amd_deferred_stats
(ops deferred by the call; a CLV that is deferred is materialised, and counted, when it is read back) and
pll_amd_edge_fold_stats (lists launched with the epilogue).

8 balanced and 17 random tips, 1,000 sites, 4 categories, per-site scale buffers, PLLHIP_FUSED=2.  The dry entry point
plans one segment, so the live call is held to one too (PLLHIP_FUSED_SEGMENTS=1, as in test_gpu_edge_fold.py): a list
of two segments is never folded.  The second traversal is the one compared: it meets the first one's deferred cherries
(the dry call's old_deferred / old_scaler) and the hint the edge evaluation left.
"""
import numpy as np
import pytest

from helpers import make_case, build_partition
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
from test_host_edge_fold_plan import _dry_edge

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
