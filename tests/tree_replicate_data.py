"""Data for the tree-replicate tests (tests/test_tree_replicates_host.py, tests/test_gpu_tree_replicates.py).

pll_amd_tree_replicate_loglikelihood scores candidate trees (tests/tree_score_data.py) under every replicate of a set
(tests/replicate_data.py).  `sequence_persite` is what a candidate's per-site values mean: the sequence of
tree_score_data.sequence_lnl on the same partition, ending in the single call's per-site output under unit pattern
weights.  `ordered_sum` is the documented order of a replicate's sum (include/pll_amd.h) in numpy: rounded products,
spans of SPAN sites added one by one from +0, the spans' sums added one by one from +0.  `best_rule` is the documented
running maximum over the candidates.
"""
import numpy as np

import replicate_data as RD

SPAN = 2048   # REPL_SPAN of replicates.hpp
NONE = 0xffffffff   # nobody holds the replicate


def edge_of(cand):
    """(parent clv, parent scaler, child clv, child scaler, matrix) of a candidate"""
    return tuple(int(x) for x in cand[3:8])


def run_sequence(p, cand):
    """pll_update_prob_matrices and pll_update_partials of the candidate, on partition p"""
    ops, mi, bl = cand[0], cand[1], cand[2]
    if len(mi):
        p.update_prob_matrices(cand.params, list(mi), bl)
    if len(ops):
        p.update_partials(ops)


def sequence_persite(lib, p, case, cand):
    """[sites] the definition: the candidate's matrices and ops on p (which they overwrite), then the single call's
    per-site output at its edge with every pattern weight set to 1"""
    run_sequence(p, cand)
    return RD.unit_persite(lib, p, case, edge_of(cand))


def ordered_sum(persite, weights):
    """[replicates] sum_n (double)w_r[n] * persite[n] in the documented order"""
    s = np.asarray(persite, dtype=np.float64)
    w = np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1, len(s)).astype(np.float64)
    out = np.zeros(len(w))
    with np.errstate(invalid="ignore"):
        for r in range(len(w)):
            terms = w[r] * s
            spans = np.array([np.add.accumulate(np.concatenate(([0.0], terms[at:at + SPAN])))[-1]
                              for at in range(0, len(s), SPAN)])
            out[r] = np.add.accumulate(np.concatenate(([0.0], spans)))[-1]
    return out


def best_rule(lnl):
    """(best_index [replicates] uint32, best_lnl [replicates]) of a [candidates][replicates] table: in ascending
    candidate order, c takes over when nobody holds the replicate and its value is not NaN, or when its value is
    strictly greater than the held one"""
    lnl = np.asarray(lnl, dtype=np.float64)
    reps = lnl.shape[1]
    index = np.full(reps, NONE, dtype=np.uint32)
    value = np.full(reps, np.nan)
    for r in range(reps):
        for c in range(lnl.shape[0]):
            v = lnl[c, r]
            if (index[r] == NONE and not np.isnan(v)) or (index[r] != NONE and v > value[r]):
                index[r], value[r] = c, v
    return index, value
