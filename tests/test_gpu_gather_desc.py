"""Gather descriptors of the 4-state whole-list kernel on the device (DESIGN.md 2.0 "Memory queue", 8.4j): the plan is
128 bytes per op -- the record, then one descriptor of finished numbers per gathered factor (FusedGatherDesc,
partials_fused.hpp; its host side: tests/test_host_gather_desc.py) --, and the kernel reads the descriptors in place of
the record's character words.  tests/test_gpu_gather_index.py runs every form of a gather; the cases here are the ones
that depend on WHERE a record lies:

  headers + edge   two rooted clades of 16 tips joined at their roots: ops 0 and 1 of the walk both gather (the two header
                   records' look-ahead), and the root edge is inner-inner, so the evaluation's hint puts the edge
                   pseudo-op's record behind the last op -- planned, then replayed (the EDGE instance both times)
  segments         the same list without PLLHIP_FUSED_SEGMENTS=1: the two clades share no buffer and become two segments,
                   whose records begin at offsets counted in records of the new size
  batch refill     a 70-tip caterpillar: the batch of rows is refilled between two ops' descriptor reads
  table reuse      a replay after pll_update_prob_matrices on a matrix under a quad: the descriptors' table offsets stay,
                   the table behind them is rebuilt

Every case runs the default partition next to the quads-off twin, the per-level twin and the oracle: every CLV and
scale buffer bit for bit, the twins' edge lnL equal, the oracle's to 1e-12 relative.  Sites as in
tests/test_gpu_gather_index.py: 1, 15, 16, 17, 33 (around the 4-category tile of 16) and 700 (625 classes per quad).
"""
import ctypes as C

import numpy as np
import pytest

from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_gpu_gather_index import SITES, _all_patterns
from test_gpu_pair_rows import Twins, _case
from test_gpu_quad_rows import Quads
from test_gpu_table_reuse import Reuse

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _two_clades(n=16):
    """two balanced clades of n tips, each joined with one more tip (its root has a reader's shape: tip-inner); the root
    edge joins the two roots -- both ends stored CLVs, neither a cherry"""
    t = 2 * (n + 1)
    joins, nxt, roots = [], t, []
    for first in (0, n + 1):
        level = list(range(first, first + n))
        while len(level) > 1:
            new = []
            for i in range(0, len(level), 2):
                joins.append((nxt, level[i], level[i + 1]))
                new.append(nxt)
                nxt += 1
            level = new
        joins.append((nxt, level[0], first + n))
        roots.append(nxt)
        nxt += 1
    return W._assemble(t, joins, (roots[0], roots[1]), W.SplitMix64(5), "two-clades")


def _new_case(plan, sites, rate_cats):
    return _all_patterns(_case("random", plan.tips, sites, rate_cats, plan=plan), sites)


def _segments(gpu, plan):
    ops = np.ascontiguousarray(plan.ops)
    seg = (C.c_uint * len(ops))()
    f = gpu.lib.pllhip_fused_segments_dry
    f.restype = C.c_uint
    return f(C.c_uint(plan.tips), C.c_uint(plan.clv_buffers), C.c_uint(plan.scale_buffers), C.c_int(1),
             ops.ctypes.data_as(C.c_void_p), C.c_uint(len(ops)), C.c_uint(8), seg)


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_headers_and_edge_record(gpu, orc, monkeypatch, rate_cats, sites):
    t = Quads(gpu, orc, monkeypatch, _new_case(_two_clades(), sites, rate_cats))
    for x in (t.p, t.z):
        x.set_edge_fold(True)
    t.update()
    got = t.p.quad_list_stats()
    assert (got["taken"], got["wide_gathers"]) == (8, 8), got
    assert t.p.quad_fold_stats()["live"] == 4, "four walked ops: each clade's top op gathers four quads, its root one tip"
    assert t.p.edge_fold_stats()[0] == 0
    t.check()                           # (the evaluation leaves its hint)
    t.update()                          # planned again, with the pseudo-op's record behind the last op
    assert t.p.edge_fold_stats()[0] == 1
    # (terms nobody sums end the hint, and a CLV read ends the kept plan: the evaluation alone between the two launches)
    first = t.p.compute_edge_loglikelihood(*t.plan.root_edge, [0] * t.R)
    assert t.p.edge_fold_stats()[1] == 1, "served from the epilogue's terms"
    t.update()                          # the kept plan replayed: the EDGE instance reads that record again
    assert t.p.edge_fold_stats()[0] == 2
    assert t.p.compute_edge_loglikelihood(*t.plan.root_edge, [0] * t.R) == first
    assert t.p.edge_fold_stats()[1] == 2
    t.check()
    t.destroy()


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_segment_offsets(gpu, orc, monkeypatch, rate_cats, sites):
    monkeypatch.delenv("PLLHIP_FUSED_SEGMENTS")
    plan = _two_clades()
    assert _segments(gpu, plan) == 2, "the two clades share no buffer"
    t = Quads(gpu, orc, monkeypatch, _new_case(plan, sites, rate_cats))
    t.update()
    got = t.p.quad_list_stats()
    assert (got["taken"], got["wide_gathers"]) == (8, 8), got
    t.check()
    t.update()
    t.check()
    t.destroy()


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats,attrs", [(1, PT), (2, PT), (4, PT), (8, PT), (4, PT | ATTRIB_RATE_SCALERS)])
def test_batch_refill_between_descriptor_reads(gpu, orc, monkeypatch, rate_cats, attrs, sites):
    plan = W.caterpillar_tree(70, seed=7)
    t = Twins(gpu, orc, monkeypatch, _new_case(plan, sites, rate_cats), attrs)
    t.update()
    assert t.p.quad_list_stats()["wide_gathers"] == 0 and t.p.pair_row_stats()["live"] >= 1
    t.check()
    t.update()
    t.check()
    t.destroy()


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats,attrs", [(8, PT), (4, PT | ATTRIB_RATE_SCALERS)])
def test_byte_forms_in_the_instances_that_never_defer(gpu, orc, monkeypatch, rate_cats, attrs, sites):
    """eager tip-tip ops through pair rows and tip-inner ops through shifted tip rows: the first descriptor only"""
    t = Twins(gpu, orc, monkeypatch, _new_case(_two_clades(), sites, rate_cats), attrs)
    t.update()
    assert t.p.quad_list_stats()["wide_gathers"] == 0 and t.p.pair_row_stats()["live"] >= 1
    t.check()
    t.update()
    t.check()
    t.destroy()


@pytest.mark.parametrize("sites", SITES)
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_table_reuse_with_descriptors(gpu, orc, monkeypatch, rate_cats, sites):
    plan = _two_clades()
    t = Reuse(gpu, orc, monkeypatch, _new_case(plan, sites, rate_cats))
    t.update()
    t.check(lnl=False)                  # (an evaluation would hint an edge, and the list after it be planned anew)
    t.planned()                         # planned, then replayed with nothing written
    # the branch above tip 0: a tip matrix of the first quad -- its table is stale, the others are not
    mi = [int(op["child1_matrix_index"]) for op in plan.ops if int(op["child1_clv_index"]) == 0][0]
    # (an unchanged length is a write all the same: the kept plan is replayed, and exactly the rule's jobs run)
    t.lengths([mi], [t.length_of(mi)])
    want, everything = t.rule([mi]), t.rule(everything=True)
    assert 1 <= want["jobs_run"] < everything["jobs_run"] and want["jobs_skipped"] >= 1
    t.update()
    assert t.added() == want
    # a new length: the values must be those of the new matrix.  (No job count is asserted here: this tree has scale
    # buffers, and a plan whose quads stand on the host's matrix bounds may end with a new length -- pmatrix.hip; what is
    # compared is every CLV, every count and the lnL, below.)
    t.lengths([mi], [0.37])
    t.update()
    assert t.p.quad_list_stats()["wide_gathers"] == 8
    t.check()
    t.destroy()
