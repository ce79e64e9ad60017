"""Data for the tree-scoring tests (tests/test_tree_score_host.py, tests/test_gpu_tree_score.py).

Trees from tests/insertion_data.py through tests/nni_data.py: every DIRECTED inner CLV has a buffer and a scale buffer
of its own, edge e uses matrix e, and `case.ops` computes all of them, children first.  A candidate is the tuple
`Partition.tree_loglikelihood` takes -- (ops, matrix_indices, lengths, parent, parent_scaler, child, child_scaler,
matrix) -- with the params indices attached; `sequence_lnl` is the definition of its value (include/pll_amd.h): the
three reference calls on the same partition, which overwrite what the candidate writes -- `restore` puts it back.
"""
import numpy as np

import nni_data as N
from libpll_amd.pllapi import OPS_DTYPE

make_case = N.make_case
build = N.build


class Candidate(tuple):
    """the tuple of Partition.tree_loglikelihood, plus .params"""
    params = None


def _candidate(case, ops, mi, bl, eid):
    a, b, _ = case.edges[eid]
    pc, ps = case.side(a, b)
    cc, cs = case.side(b, a)
    arr = np.zeros(len(ops), dtype=OPS_DTYPE)
    for i, op in enumerate(ops):
        arr[i] = op
    c = Candidate((arr, np.asarray(mi, dtype=np.uint32), np.asarray(bl, dtype=np.float64), pc, ps, cc, cs, eid))
    c.params = list(case.params)
    return c


def _writers(case):
    return {op[0]: i for i, op in enumerate(case.ops)}


def depends(case, eid):
    """positions in case.ops of the ops that the two sides of edge eid depend on, ascending"""
    a, b, _ = case.edges[eid]
    writer = _writers(case)
    todo = [case.side(a, b)[0], case.side(b, a)[0]]
    keep = set()
    while todo:
        c = todo.pop()
        if c in writer and writer[c] not in keep:
            keep.add(writer[c])
            op = case.ops[writer[c]]
            todo += [op[2], op[5]]
    return sorted(keep)


def full_candidate(case, eid, lengths):
    """the ops of case.ops that both sides of edge eid depend on, in case.ops order, with every edge's matrix listed"""
    assert len(lengths) == len(case.edges)
    return _candidate(case, [case.ops[i] for i in depends(case, eid)], range(len(case.edges)), lengths, eid)


def path_candidate(case, eid, changed_eid, t):
    """edge changed_eid gets length t and the tree is evaluated at edge eid: only the directed CLVs between the two,
    one matrix listed; everything else is read from the partition"""
    dirty = set()
    ops = []
    for i in depends(case, eid):
        op = case.ops[i]
        if changed_eid in (op[3], op[6]) or op[2] in dirty or op[5] in dirty:
            dirty.add(op[0])
            ops.append(op)
    return _candidate(case, ops, [changed_eid], [t], eid)


def sequence_lnl(p, cand):
    """the definition: pll_update_prob_matrices, pll_update_partials, pll_compute_edge_loglikelihood"""
    ops, mi, bl, pc, ps, cc, cs, m = cand
    if len(mi):
        p.update_prob_matrices(cand.params, list(mi), bl)
    if len(ops):
        p.update_partials(ops)
    return p.compute_edge_loglikelihood(pc, ps, cc, cs, m, cand.params)


def restore(p, case):
    """all matrices and all of case.ops again"""
    p.update_prob_matrices(case.params, list(range(len(case.lengths))), case.lengths)
    ops = np.zeros(len(case.ops), dtype=OPS_DTYPE)
    for i, op in enumerate(case.ops):
        ops[i] = op
    p.update_partials(ops)


def needs(case):
    """{directed CLV: the slots its value needs}: a tip 0; an op with operand needs a >= b: max(1, a + 1 if a == b
    else a)"""
    need = {}
    for op in case.ops:
        a, b = sorted((need.get(op[2], 0), need.get(op[5], 0)), reverse=True)
        need[op[0]] = max(1, a + 1 if a == b else a)
    return need


def slots_needed(case, eid, need=None):
    """the slots the edge needs: side needs x >= y: max(x, y + 1) if y > 0 else max(x, 1)"""
    need = need if need is not None else needs(case)
    a, b, _ = case.edges[eid]
    x, y = sorted((need.get(case.side(a, b)[0], 0), need.get(case.side(b, a)[0], 0)), reverse=True)
    return max(x, y + 1) if y > 0 else max(x, 1)


def fresh_lengths(case, rng):
    return rng.uniform(0.02, 0.6, len(case.edges))
