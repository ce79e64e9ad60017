"""The planner of the tree-scoring kernel (pllhip_tree_score_plan_dry: host logic, no device) on the trees of
tests/tree_score_data.py: the slots a plan uses are the Sethi-Ullman number of the edge, the walk never reads a slot
that does not hold the operand and never overwrites a live value, ops the edge does not depend on are dropped, and
the return codes say which route takes a list."""
from collections import Counter

import numpy as np
import pytest

import tree_score_data as T
from libpll_amd.pllapi import OPS_DTYPE, tree_score_plan

TREES = {
    "12": (dict(tips=12), 21, {2: 20, 3: 1}),
    "64": (dict(tips=64), 125, {3: 86, 4: 39}),
    "200": (dict(tips=200), 397, {4: 248, 5: 149}),
    "caterpillar-700": (dict(tips=700, seed=5, caterpillar=True), 1397, {1: 4, 2: 1393}),
}


def case_of(name, **kw):
    args = dict(states=4, seed=3, tip_queries=0, inner_queries=0, sites=8)
    args.update(TREES[name][0])
    args.update(kw)
    return T.make_case(**args)


def plan(amd, case, cand, max_slots=16, ops=None):
    ops = cand[0] if ops is None else ops
    return tree_score_plan(amd.lib, case.ntips, case.nclv, case.nscale, case.pattern_tip, ops, cand[3], cand[4],
                           cand[5], cand[6], max_slots)


def walk(case, cand, ops, order, slots, nslots):
    """run the plan as the kernel does; returns the set of kept positions"""
    written = {int(op["parent_clv_index"]) for op in ops}
    holds = [None] * nslots      # slot -> the CLV it holds
    live = [False] * nslots      # ... and whether that value has still to be read
    done = set()

    def take(clv, slot):
        if slot < 0:
            # a tip or an operand of an earlier call: never one the candidate writes
            assert clv not in written, (clv, slot)
            return
        assert holds[slot] == clv and live[slot], (clv, slot, holds[slot])
        live[slot] = False

    for pos, (l, r, par) in zip(order, slots):
        op = ops[pos]
        for child in (int(op["child1_clv_index"]), int(op["child2_clv_index"])):
            if child in written:
                assert child in done, "op %d runs before its operand %d" % (pos, child)
        take(int(op["child1_clv_index"]), l)
        take(int(op["child2_clv_index"]), r)
        assert 0 <= par < nslots
        assert not live[par], "op %d overwrites the live value of slot %d" % (pos, par)
        holds[par], live[par] = int(op["parent_clv_index"]), True
        done.add(int(op["parent_clv_index"]))
    # the edge's sides: written by the candidate -> live in exactly one slot; nothing else is left live
    left = {holds[s] for s in range(nslots) if live[s]}
    assert left == {c for c in (cand[3], cand[5]) if c in written}
    return {int(p) for p in order}


@pytest.mark.parametrize("pattern_tip", [True, False], ids=["pattern-tips", "tip-clvs"])
@pytest.mark.parametrize("name", list(TREES))
def test_slots_are_the_sethi_ullman_number(amd, name, pattern_tip):
    case = case_of(name, pattern_tip=pattern_tip)
    _, nedges, hist = TREES[name]
    assert len(case.edges) == nedges
    need = T.needs(case)
    lengths = np.full(len(case.edges), 0.1)
    seen, planned = Counter(), Counter()
    step = 1 if nedges < 500 else 7   # (the planner on every edge; the Python walk of every 7th on the long tree)
    for eid in range(nedges):
        want = T.slots_needed(case, eid, need)
        seen[want] += 1
        cand = T.full_candidate(case, eid, lengths)
        rc, order, slots, nslots = plan(amd, case, cand)
        planned[nslots] += 1
        assert rc == 0 and nslots == want, (eid, rc, nslots, want)
        assert len(order) == len(cand[0]) == len(set(order.tolist()))
        assert slots.max() == want - 1 if len(order) else True
        if eid % step == 0 or want != 2:
            walk(case, cand, cand[0], order, slots, nslots)
    assert dict(planned) == hist
    assert dict(seen) == hist


def test_slot_cap_sends_the_deeper_edges_to_the_general_route(amd):
    case = case_of("64")
    need = T.needs(case)
    lengths = np.full(len(case.edges), 0.1)
    taken = Counter()
    for eid in range(len(case.edges)):
        cand = T.full_candidate(case, eid, lengths)
        rc, order, slots, nslots = plan(amd, case, cand, max_slots=3)
        want = T.slots_needed(case, eid, need)
        assert nslots == want
        assert rc == (0 if want <= 3 else 1), (eid, rc, want)
        assert len(order) == len(cand[0])
        if rc == 1:
            assert order.tolist() == sorted(order.tolist()) and (slots == -1).all()
        taken[rc] += 1
    assert taken == {0: 86, 1: 39}


@pytest.mark.parametrize("name", ["12", "64"])
def test_path_candidates_and_dropped_ops(amd, name):
    case = case_of(name)
    rng = np.random.default_rng(5)
    nedges = len(case.edges)
    written_all = {op[0] for op in case.ops}
    inner_externals = 0
    for _ in range(25):
        eid, changed = (int(x) for x in rng.integers(0, nedges, 2))
        cand = T.path_candidate(case, eid, changed, 0.3)
        ops = cand[0]
        if changed == eid:
            assert len(ops) == 0
        # a stray op: a directed CLV the edge does not depend on, put last (it may read what the path writes)
        deps = set(T.depends(case, eid))
        stray_pos = next(i for i in range(len(case.ops)) if i not in deps)
        stray = np.zeros(1, dtype=OPS_DTYPE)
        stray[0] = case.ops[stray_pos]
        listed = np.concatenate([ops, stray])
        rc, order, slots, nslots = plan(amd, case, cand, ops=listed)
        assert rc == 0
        kept = walk(case, cand, listed, order, slots, nslots)
        assert kept == set(range(len(ops)))   # the stray op and nothing else is dropped
        # the operands the path reads from the partition: no slot
        on_path = {int(op["parent_clv_index"]) for op in ops}
        externals = 0
        for pos, (l, r, _) in zip(order, slots):
            for child, slot in ((int(listed[pos]["child1_clv_index"]), l), (int(listed[pos]["child2_clv_index"]), r)):
                assert (slot >= 0) == (child in on_path)
                externals += int(child not in on_path)
                inner_externals += int(child in written_all and child not in on_path)
        if len(ops):
            assert externals >= len(ops)   # a path reads the other subtree of each of its nodes from memory
            assert nslots == 1             # ... so one live value is all it ever holds
    assert inner_externals >= 10           # (directed CLVs of the partition among them, not only tips)


def test_return_codes(amd):
    case = case_of("12")
    lengths = np.full(len(case.edges), 0.1)
    eid = max(range(len(case.edges)), key=lambda e: len(T.depends(case, e)))
    cand = T.full_candidate(case, eid, lengths)
    ops = cand[0]
    assert len(ops) >= 4 and plan(amd, case, cand)[0] == 0
    # a parent CLV written twice; a parent scale buffer written twice
    bad = ops.copy()
    bad[1]["parent_clv_index"] = bad[0]["parent_clv_index"]
    assert plan(amd, case, cand, ops=bad)[0] == -1
    bad = ops.copy()
    bad[1]["parent_scaler_index"] = bad[0]["parent_scaler_index"]
    assert plan(amd, case, cand, ops=bad)[0] == -1
    # a read before its write in the same list: an op and the writer of its first child change places
    inner = next(i for i in range(len(ops)) if int(ops[i]["child1_clv_index"]) >= case.ntips)
    first = next(i for i in range(len(ops)) if ops[i]["parent_clv_index"] == ops[inner]["child1_clv_index"])
    assert first < inner
    bad = ops.copy()
    bad[[first, inner]] = bad[[inner, first]]
    assert plan(amd, case, cand, ops=bad)[0] == -1
    # an op that reads its own parent
    bad = ops.copy()
    bad[-1]["child1_clv_index"] = bad[-1]["parent_clv_index"]
    assert plan(amd, case, cand, ops=bad)[0] == -1
    # a tip parent; indices out of range
    bad = ops.copy()
    bad[0]["parent_clv_index"] = 2
    assert plan(amd, case, cand, ops=bad)[0] == -1
    for field, value in (("child1_clv_index", case.ntips + case.nclv), ("child2_scaler_index", case.nscale),
                         ("parent_scaler_index", -2)):
        bad = ops.copy()
        bad[0][field] = value
        assert plan(amd, case, cand, ops=bad)[0] == -1, field
    # a pattern tip as the edge's parent
    assert tree_score_plan(amd.lib, case.ntips, case.nclv, case.nscale, True, ops, 0, -1, cand[3], cand[4])[0] == -1
    # the planner keeps nothing from an invalid list: the good one still plans
    assert plan(amd, case, cand)[0] == 0
    # a child written by the list, read with a foreign scaler index: the general route
    odd = ops.copy()
    foreign = case.spare_sc
    assert foreign != odd[inner]["child1_scaler_index"]
    odd[inner]["child1_scaler_index"] = foreign
    rc, order, slots, _ = plan(amd, case, cand, ops=odd)
    assert rc == 1 and len(order) == len(ops)
    # ... read with no scaler at all: still the kernel's
    odd[inner]["child1_scaler_index"] = -1
    assert plan(amd, case, cand, ops=odd)[0] == 0


def _numpy_walk(ref, r, case, cand, order, slots):
    """the kernel's walk restated in numpy on the reference's own P-matrices: values and counts live in the plan's
    slots, every op takes the scaling rule of pll_update_partials, the edge term is pll_compute_edge_loglikelihood's"""
    ops, mi, bl, pc, ps, cc, cs, em = cand
    r.update_prob_matrices(cand.params, list(mi), bl)
    pm = {int(m): r.get_pmatrix(int(m)) for m in mi}                       # [R][4][4]
    nt = ref.map("nt")
    masks = [np.array([[(int(nt[ch]) >> s) & 1 for s in range(4)] for ch in seq], dtype=float) for seq in case.seqs]
    R = case.rate_cats
    held = {}

    def product(clv, m, slot):
        if slot >= 0:
            vals, cnt, owner = held[slot]
            assert owner == clv
            return np.einsum("kjs,nks->nkj", pm[m], vals), cnt, False
        assert clv < case.ntips
        return np.einsum("kjs,ns->nkj", pm[m], masks[clv]), 0, True

    for pos, (l, rr, par) in zip(order, slots):
        op = ops[pos]
        x, cx, tx = product(int(op["child1_clv_index"]), int(op["child1_matrix_index"]), l)
        y, cy, ty = product(int(op["child2_clv_index"]), int(op["child2_matrix_index"]), rr)
        p = x * y
        cnt = np.zeros(case.sites, dtype=np.int64)
        if op["parent_scaler_index"] >= 0 and not (tx and ty):
            small = (p < 2.0 ** -256).all(axis=(1, 2))
            p[small] *= 2.0 ** 256
            cnt = cx + cy + small.astype(np.int64)
        held[par] = (p, cnt, int(op["parent_clv_index"]))
    by_clv = {owner: (vals, cnt) for vals, cnt, owner in held.values()}
    u, cu = by_clv[pc]
    if cc in by_clv:
        v, cv = by_clv[cc]
        tb = np.einsum("kjs,nks->nkj", pm[em], v)
    else:
        tb, cv = np.einsum("kjs,ns->nkj", pm[em], masks[cc]), 0
    freqs = np.asarray(case.models[0][1])
    site = (u * freqs[None, None, :] * tb).sum(axis=2).sum(axis=1) / R
    counts = cu + cv
    pw = case.pw if case.pw is not None else np.ones(case.sites)
    return float((pw * (np.log(site) + counts * np.log(2.0 ** -256))).sum()), int(np.max(counts))


@pytest.mark.parametrize("kw,eids", [(dict(tips=12, sites=40), range(21)),
                                     (dict(tips=400, sites=6, seed=5, caterpillar=True), (0, 1, 300, 796))],
                         ids=["12-tips", "caterpillar-400"])
def test_walk_in_numpy_equals_the_reference_sequence(amd, ref, kw, eids):
    """the plan carried out with numbers: what the kernel is built to compute, against the three calls on the genuine
    reference -- slots, order, the scaling rule with counts travelling in the slots, the edge term"""
    case = T.make_case(states=4, tip_queries=0, inner_queries=0, **dict(dict(seed=3), **kw))
    r = T.build(ref, case)
    try:
        rng = np.random.default_rng(7)
        most = 0
        for eid in eids:
            cand = T.full_candidate(case, eid, T.fresh_lengths(case, rng))
            rc, order, slots, nslots = plan(amd, case, cand)
            assert rc == 0
            got, counts = _numpy_walk(ref, r, case, cand, order, slots)
            want = T.sequence_lnl(r, cand)
            assert abs(got - want) <= 1e-12 * abs(want), (eid, got, want)
            most = max(most, counts)
        if case.n >= 400:
            assert most > 0   # the scaling rule ran
    finally:
        r.destroy()
