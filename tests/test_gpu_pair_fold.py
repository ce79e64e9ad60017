"""Folded pair products: an unstored gathered-gathered parent with exactly one reader, an inner-inner
op, is not walked by the 4-state whole-list launch at all -- its reader forms the product, and the scale bit, from the
two gathered factors at the top of its own op.

Every case runs three partitions of one process through the same calls -- `fold` (the default), `walk`
(pll_amd_set_pair_fold(p, 0): unstored parents are walked, as before) and `eager` (pll_amd_set_unstored_pairs(p, 0):
every walked op is stored) -- next to the oracle, and compares every CLV and scale buffer read back, bit for bit, and
the lnL.  40 sites: three tiles of 16 at 4 rate categories, the last one ragged.  The number of parents folded is
asserted through pll_amd_pair_fold_stats against the host rule (pllhip_fused_plan_dry_folded).

A folded reader at an even and at an odd position of the op loop, followed by an op of each kind, comes from five
small random trees; the combinations they cover are asserted from the host rule's walk (test_reader_positions*).

Not built: a reader whose other operand is a single gathered factor (a tip or a deferred cherry).  Such a product stays
walked and unstored; the hand-made tree below has one (Q) and checks that.
"""
import numpy as np
import pytest

from helpers import TREES, make_case, build_partition, oracle_run, bits_equal
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_host_pair_fold_plan import _call

pytestmark = pytest.mark.gpu
ATTRS = ATTRIB_PATTERN_TIP
SITES = 40


@pytest.fixture(autouse=True)
def _whole_list_kernel(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _kids(op):
    return [int(op["child1_clv_index"]), int(op["child2_clv_index"])]


def _cherries(plan):
    return {int(op["parent_clv_index"]): op for op in plan.ops if all(x < plan.tips for x in _kids(op))}


def _mismatch_columns(case, n=24):
    """the first n columns: the two tips of every cherry differ (A against C), no gaps"""
    seqs = [bytearray(s) for s in case["seqs"]]
    for op in _cherries(case["plan"]).values():
        a, b = _kids(op)
        seqs[a][:n] = b"A" * n
        seqs[b][:n] = b"C" * n
    case["seqs"] = [bytes(s) for s in seqs]


def _dry(gpu, plan, ops=None, rate_cats=4, edge=None):
    return _call(gpu, "pllhip_fused_plan_dry_folded", plan.ops if ops is None else ops, plan.tips, plan.clv_buffers,
                 plan.scale_buffers, rate_cats, 0, edge, None, True)


class Trio:
    """fold / walk / eager partitions and the oracle over one case"""

    def __init__(self, gpu, orc, case, attrs=ATTRS):
        self.case, self.plan, self.R = case, case["plan"], case["rate_cats"]
        self.fold = build_partition(gpu, case, attrs)
        self.walk = build_partition(gpu, case, attrs)
        self.walk.set_pair_fold(False)
        self.eager = build_partition(gpu, case, attrs)
        self.eager.set_unstored_pairs(False)
        self.parts = (self.fold, self.walk, self.eager)
        self.o = oracle_run(orc, gpu, self.fold, case, attrs)

    def update(self, ops=None):
        ops = self.plan.ops if ops is None else ops
        for p in self.parts:
            p.update_partials(ops)
        self.o.update_partials(ops)

    def matrices(self, indices, lengths):
        indices = np.asarray(indices, dtype=np.uint32)
        for p in self.parts:
            p.update_prob_matrices([0] * self.R, indices, np.asarray(lengths, dtype=np.float64))
        for mi in indices:
            self.o.pmat[int(mi)] = self.fold.get_pmatrix(int(mi))

    def lnl(self, edge=None):
        edge = self.plan.root_edge if edge is None else edge
        got = [p.compute_edge_loglikelihood(*edge, [0] * self.R) for p in self.parts]
        ref = self.o.edge_loglikelihood(*edge)
        assert got[0] == got[1] == got[2], got
        assert abs(got[0] - ref) <= 1e-12 * abs(ref), (got, ref)
        return got[0]

    def read_everything(self, ops=None):
        for op in (self.plan.ops if ops is None else ops):
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            for name, p in zip(("fold", "walk", "eager"), self.parts):
                assert bits_equal(p.get_clv(node), self.o.clv[node]), "%s: CLV %d differs from the oracle" % (name, node)
                if sc >= 0:
                    assert (p.get_scaler(sc) == self.o.scalers[sc]).all(), "%s: scaler %d" % (name, sc)

    def folded(self):
        return self.fold.pair_fold_stats()["folded_now"]

    def destroy(self):
        for p in self.parts:
            p.destroy()


def _case(shape, tips, seed, rate_cats, scalers, plan=None):
    case = make_case(4, shape, tips, SITES, rate_cats=rate_cats, seed=seed)
    case["plan"] = plan if plan is not None else TREES[shape](tips, seed=seed, use_scalers=scalers)
    _mismatch_columns(case)
    return case


def _hand_made(product_first, scalers=True):
    """10 tips: P = (cherry, cherry) read once, by R = (P, X) / (X, P); X = (tip 8, Q), Q = (cherry, cherry) -- Q's
    reader has a single gathered factor beside it, so Q stays walked.  Root edge: R -- tip 9."""
    joins = [(10, 0, 1), (11, 2, 3), (12, 4, 5), (13, 6, 7), (14, 10, 11), (15, 12, 13), (16, 8, 15),
             (17, 14, 16) if product_first else (17, 16, 14)]
    return W._assemble(10, joins, (17, 9), W.SplitMix64(5), "hand", scalers)


@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [False, True])
def test_balanced_16(gpu, orc, rate_cats, scalers):
    """Its walk is two readers of two products each: the first two ops of a tile, consecutive, and the last."""
    t = Trio(gpu, orc, _case("balanced", 16, 7, rate_cats, scalers))
    d = _dry(gpu, t.plan, rate_cats=rate_cats)
    assert len(d["folded"]) == 4 and d["operands"] == [[3, 3], [3, 3]]
    t.update()
    assert t.folded() == 4 and t.fold.unstored_stats()["unstored_now"] == 4
    assert t.walk.pair_fold_stats()["folded_now"] == 0 and t.walk.unstored_stats()["unstored_now"] == 4
    assert t.eager.unstored_stats()["unstored_now"] == 0
    first = t.lnl()
    t.read_everything()
    st = t.fold.pair_fold_stats()
    assert st["folded_now"] == 0 and st["materialised"] == 4, st
    # three replays through the kept plan, new matrices between the calls
    for step in range(3):
        t.matrices(t.plan.matrix_indices, np.asarray(t.plan.branch_lengths) * (1.3 + step) + 0.01)
        t.update()
        assert t.folded() == 4
        assert t.lnl() != first
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("product_first", [True, False])
@pytest.mark.parametrize("rate_cats,scalers", [(4, True), (4, False), (1, True), (2, True)])
def test_product_with_slot(gpu, orc, product_first, rate_cats, scalers):
    plan = _hand_made(product_first, scalers)
    t = Trio(gpu, orc, _case("random", 10, 3, rate_cats, scalers, plan=plan))
    d = _dry(gpu, plan, rate_cats=rate_cats)
    assert len(d["folded"]) == 1 and len(d["order"]) == 3
    assert sorted(d["operands"][-1]) == [0, 3] and d["operands"][-1].index(3) == (0 if product_first else 1)
    assert len(d["unstored"]) == 1, "Q: its reader has a tip beside it -- walked, unstored"
    t.update()
    assert t.folded() == 1 and t.fold.unstored_stats()["unstored_now"] == 2
    t.lnl()
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_scaling(gpu, orc, rate_cats):
    """Cherry branches of 1e-45 (tests/test_gpu_unstored_pairs.py): a product over two mismatching cherries falls below
    2^-256 and scales.  The reader's counts carry the bit; the counts the materialising launch writes are 0 or 1 and the
    eager partition's."""
    for plan in (W.balanced_tree(16, seed=7), _hand_made(True), _hand_made(False)):
        t = Trio(gpu, orc, _case("random", plan.tips, 3, rate_cats, True, plan=plan))
        cherry = _cherries(plan)
        mis = sorted({int(op["child%d_matrix_index" % k]) for op in cherry.values() for k in (1, 2)})
        t.matrices(mis, np.full(len(mis), 1e-45))
        t.update()
        d = _dry(gpu, plan, rate_cats=rate_cats)
        assert t.folded() == len(d["folded"]) > 0
        # a reader first: its counts include the folded products' bits
        scaled = 0
        for i in d["folded"]:
            parent = int(plan.ops[i]["parent_clv_index"])
            reader = next(op for op in plan.ops if parent in _kids(op))
            rsc = int(reader["parent_scaler_index"])
            got = t.fold.get_scaler(rsc)
            assert (got == t.o.scalers[rsc]).all() and (got == t.eager.get_scaler(rsc)).all()
            assert int(got[:24].min()) >= 1, "the reader inherits the product's scale bit in the mismatching columns"
        assert t.folded() == len(d["folded"]), "reading a reader's counts materialises nothing"
        for i in d["folded"]:
            sc = int(plan.ops[i]["parent_scaler_index"])
            got = t.fold.get_scaler(sc)
            assert got.max() <= 1 and (got == t.eager.get_scaler(sc)).all() and (got == t.o.scalers[sc]).all()
            scaled += int((got[:24] == 1).sum())
        assert scaled > 0, "no folded product scaled: the columns were meant to"
        t.lnl()
        t.read_everything()
        t.destroy()


@pytest.mark.parametrize("rate_cats,attrs", [(8, ATTRS), (4, ATTRS | ATTRIB_RATE_SCALERS)])
def test_instances_that_never_defer(gpu, orc, rate_cats, attrs):
    t = Trio(gpu, orc, _case("balanced", 16, 7, rate_cats, True), attrs)
    t.update()
    assert t.folded() == 0 and t.fold.pair_fold_stats()["ops_folded"] == 0
    t.lnl()
    t.read_everything()
    t.destroy()


def _walk_kind(types):
    """what the kernel runs a walked op as: 'F' a reader of folded products, else its kind 0 .. 3"""
    if 3 in types:
        return "F"
    gathered = [x in (1, 2) for x in types]
    if all(gathered):
        return 2 if types == [1, 1] else 3
    return 1 if any(gathered) else 0


# (tips, seed, cherries pinned): random trees whose walks, between them, have a folded reader at an even and at an odd
# position of the op loop followed by an op of every kind -- found by trying seeds against pllhip_fused_plan_dry_folded;
# a pinned cherry (its address handed out) is not deferred: a walked tip-tip op, kind 2
POSITION_CASES = [(24, 14, 0), (20, 25, 2), (16, 21, 0), (20, 16, 1), (12, 3, 0)]


def _position_case(gpu, tips, seed, npin):
    plan = W.random_tree(tips, seed=seed)
    pins = sorted(_cherries(plan))[:npin]
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[pins] = 1
    d = _call(gpu, "pllhip_fused_plan_dry_folded", plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0, None,
              pinned if npin else None, True)
    kinds = [_walk_kind(t) for t in d["operands"]]
    seen = {(p % 2, kinds[p + 1] if p + 1 < len(kinds) else "L") for p, k in enumerate(kinds) if k == "F"}
    return plan, pins, d, seen


def test_reader_positions_cover_every_following_kind(gpu):
    """the cases below, together: a folded reader at an even and at an odd loop position, followed by an inner-inner,
    a gathered-inner, a tip-tip and a gathered-gathered op, by another folded reader, and as the last op"""
    seen = set()
    for tips, seed, npin in POSITION_CASES:
        seen |= _position_case(gpu, tips, seed, npin)[3]
    assert seen == {(parity, k) for parity in (0, 1) for k in (0, 1, 2, 3, "F", "L")}, sorted(seen, key=str)


@pytest.mark.parametrize("tips,seed,npin", POSITION_CASES)
def test_reader_positions(gpu, orc, tips, seed, npin):
    plan, pins, d, seen = _position_case(gpu, tips, seed, npin)
    assert d["rc"] == 0 and len(d["folded"]) > 0 and seen
    t = Trio(gpu, orc, _case("random", tips, seed, 4, True, plan=plan))
    for p in t.parts:
        for clv in pins:
            assert p.dev_clv(clv)
    t.update()
    assert t.folded() == len(d["folded"])
    assert t.fold.deferred_stats()["deferred_now"] == len(_cherries(plan)) - npin
    t.lnl()
    t.read_everything()
    # the kept plan, with new matrices
    t.matrices(plan.matrix_indices, np.asarray(plan.branch_lengths) * 1.9 + 0.02)
    t.update()
    assert t.folded() == len(d["folded"])
    t.lnl()
    t.read_everything()
    t.destroy()


def test_random_96_more_rows_than_a_batch(gpu, orc):
    """96 tips: more tip rows than one batch of a wave's character registers holds (64 at 4 categories)."""
    t = Trio(gpu, orc, _case("random", 96, 5, 4, True))
    d = _dry(gpu, t.plan)
    assert len(d["folded"]) > 0
    t.update()
    assert t.folded() == len(d["folded"])
    t.lnl()
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("scalers", [False, True])
def test_edge_instance(gpu, orc, scalers):
    """evaluate, traverse, evaluate: the second traversal runs the EDGE instance over folded readers."""
    t = Trio(gpu, orc, _case("balanced", 32, 7, 4, scalers))
    t.update()
    a = t.lnl()
    t.matrices(t.plan.matrix_indices[:3], [0.21, 0.17, 0.33])
    t.update()
    assert t.folded() == len(_dry(gpu, t.plan, edge=t.plan.root_edge[:4])["folded"]) > 0
    b = t.lnl()
    assert a != b
    t.update()
    assert t.lnl() == b
    t.read_everything()
    t.destroy()


def test_partial_list_over_a_folded_parent(gpu, orc):
    """One pendant branch changes; the path to the root reads a parent an earlier call folded as the sibling."""
    t = Trio(gpu, orc, _case("balanced", 32, 7, 4, True))
    plan = t.plan
    t.update()
    d = _dry(gpu, plan)
    assert t.folded() == len(d["folded"]) > 0
    by_parent = {int(op["parent_clv_index"]): op for op in plan.ops}
    ends = (plan.root_edge[0], plan.root_edge[2])
    folded = plan.ops[d["folded"][0]]
    reader = next(op for op in plan.ops if int(folded["parent_clv_index"]) in _kids(op))
    side = 1 if int(reader["child1_clv_index"]) == int(folded["parent_clv_index"]) else 0  # the sibling's side
    node, matrix = _kids(reader)[side], int(reader["child%d_matrix_index" % (side + 1)])
    path = [reader]
    while node >= plan.tips:
        path.insert(0, by_parent[node])
        node, matrix = _kids(by_parent[node])[0], int(by_parent[node]["child1_matrix_index"])
    top = int(reader["parent_clv_index"])
    while top not in ends:
        up = next(op for op in plan.ops if top in _kids(op))
        path.append(up)
        top = int(up["parent_clv_index"])
    part = np.array(path, dtype=plan.ops.dtype)
    t.matrices([matrix], [0.377])
    t.update(part)
    got = t.lnl()
    t.update()
    assert t.lnl() == got
    t.read_everything()
    t.destroy()


def test_switch_between_calls(gpu, orc):
    t = Trio(gpu, orc, _case("balanced", 16, 7, 4, True))
    t.update()
    a = t.lnl()
    assert t.folded() == 4
    t.fold.set_pair_fold(False)
    t.update()
    assert t.folded() == 0 and t.fold.unstored_stats()["unstored_now"] == 4 and t.lnl() == a
    t.fold.set_pair_fold(True)
    t.update()
    assert t.folded() == 4 and t.lnl() == a
    t.fold.set_unstored_pairs(False)
    assert t.folded() == 0 and t.fold.unstored_stats()["unstored_now"] == 0
    t.update()
    assert t.folded() == 0 and t.lnl() == a
    t.read_everything()
    t.destroy()
