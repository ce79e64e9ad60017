"""Real-valued tip CLVs and zero-likelihood sites (TEST DATA; tests/test_tip_values_host.py proves it on the CPU,
tests/test_gpu_tip_values.py and tests/test_gpu_zero_likelihood.py judge the product with it).

tip_values(kind, base, seed): `base` is a 0/1 array [tips][sites][R][S] (helpers.tip_clvs / helpers.index_tip_clvs);
the result has the same shape and real entries:
  error         the observed state(s) -- the entries that are 1 -- get 1 - e, the others e / (S - 1), with
                e = 10^U(-4, -0.5) per (tip, site): a sequencing-error model
  wide          every entry 10^U(-30, 0): the scaling rule fires from depth 1 on
  big           every entry 10^U(-3, 3): entries above 1
  sparse        10^U(-6, 0) with ZERO_FRACTION of the entries exactly 0 (every vector keeps one entry that is not), and
                one tip (number seed % tips) all zero at every 7th site: exactly those sites have likelihood zero --
                ceil(sites / 7) of them, between 3 and a third of the sites from 15 sites on
  per-category  `error` with an e of its own per (tip, site, category): what pll_set_tip_clv cannot say; it reaches a
                device through the mirror push (pll_amd_push_clv) and a reference partition through partition->clv[tip]
All but per-category hold the same vector in every category, as pll_set_tip_clv replicates it.

zero_cherries(case, seed, every): half of the tree's cherries (the first half in the op list's order: on a balanced tree
the other half keeps whole quads of untouched cherries) get two branches of length 0 and a second tip that copies its
sibling except at about 1 site in `every`, where it names another state: P = I on both sides and conflicting characters
make an all-zero CLV row there.  One inner branch gets length 0 as well.  zero_case builds the named cases of
ZERO_CASES; zero_cherries_directed does the same to a tests/insertion_data.py case.  agree compares values by class.
"""
import numpy as np

from exact_pruning import ExactRun
from helpers import (ALPHABET, build_partition, model_of, tip_clvs, index_tip_clvs, case_map, invariant_of, case_pinvs)
from oracle_api import OracleRun

KINDS = ("error", "wide", "big", "sparse", "per-category")
FINITE_KINDS = ("error", "wide", "big", "per-category")
ZERO_FRACTION = 0.25
ZERO_EVERY = 7
PLAIN = {4: b"ACGT", 20: b"ARNDCQEGHILKMFPSTWYV"}


def base_of(lib, case):
    """the case's own 0/1 tip CLVs [tips][sites][R][S]"""
    if case.get("tip_index") is not None:
        return index_tip_clvs(case)
    return tip_clvs(case, case_map(lib, case))


def _error(base, e):
    S = base.shape[-1]
    return np.where(base > 0, 1.0 - e, e / (S - 1))


def tip_values(kind, base, seed):
    base = np.asarray(base, dtype=np.float64)
    tips, sites, R, S = base.shape
    rng = np.random.default_rng(9000 + seed)
    if kind == "per-category":
        out = _error(base, 10.0 ** rng.uniform(-4.0, -0.5, size=(tips, sites, R, 1)))
        assert R == 1 or (out[:, :, 0] != out[:, :, 1]).any()
        return np.ascontiguousarray(out)
    if kind == "error":
        one = _error(base[:, :, 0], 10.0 ** rng.uniform(-4.0, -0.5, size=(tips, sites, 1)))
    elif kind == "wide":
        one = 10.0 ** rng.uniform(-30.0, 0.0, size=(tips, sites, S))
    elif kind == "big":
        one = 10.0 ** rng.uniform(-3.0, 3.0, size=(tips, sites, S))
        assert one.max() > 1.0
    elif kind == "sparse":
        one = 10.0 ** rng.uniform(-6.0, 0.0, size=(tips, sites, S))
        zero = rng.random((tips, sites, S)) < ZERO_FRACTION
        keep = rng.integers(0, S, size=(tips, sites))
        np.put_along_axis(zero, keep[:, :, None], False, axis=2)
        one[zero] = 0.0
        one[seed % tips, ::ZERO_EVERY, :] = 0.0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.repeat(one[:, :, None, :], R, axis=2))


def zero_sites(kind, sites):
    """the sites whose likelihood is zero by construction"""
    mask = np.zeros(sites, dtype=bool)
    if kind == "sparse":
        mask[::ZERO_EVERY] = True
    return mask


def per_category(values):
    return bool((values != values[:, :, :1, :]).any())


def apply(p, values):
    """upload `values` [tips][sites][R][S] as the tip CLVs of partition `p` (the product's or the reference's):
    pll_set_tip_clv, or -- values that differ between categories -- the mirror push / partition->clv[tip]"""
    values = np.asarray(values, dtype=np.float64)
    tips, sites, R, S = values.shape
    assert (tips, sites, R, S) == (p.s.tips, p.s.sites, p.s.rate_cats, p.s.states)
    if not per_category(values):
        for i in range(tips):
            p.set_tip_clv(i, values[i][:, 0, :].reshape(-1))
        return
    SP = p.s.states_padded
    for i in range(tips):
        padded = np.zeros((p.sites_total, R, SP))
        padded[:sites, :, :S] = values[i]
        if p.o.is_amd:
            p.put_clv(i, padded)
        else:
            np.ctypeslib.as_array(p.s.clv[i], shape=(padded.size,))[:] = padded.reshape(-1)


def build(lib, case, attrs, values, pinv=0.0):
    """a partition without pattern tips of `case` whose tips hold `values`"""
    from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
    assert not attrs & ATTRIB_PATTERN_TIP
    p = build_partition(lib, case, attrs, pinv=pinv)
    apply(p, values)
    return p


def oracle_of(orc, lib, p, case, attrs, values, invariant=None, pinv=0.0):
    inv = invariant if invariant is not None else (invariant_of(p) if max(case_pinvs(case, pinv)) > 0 else None)
    return OracleRun(orc, model_of(p, lib, case, pinv), case["plan"], attrs, tipclvs=np.array(values),
                     pattern_weights=case["pw"], invariant=inv)


def exact_of(lib, p, case, values):
    return ExactRun(model_of(p, lib, case), case["plan"], values, pattern_weights=case["pw"])


# ---- zero-length cherries

def cherries(plan):
    """(first tip, second tip) of every op that joins two tips"""
    return [(int(op["child1_clv_index"]), int(op["child2_clv_index"])) for op in plan.ops
            if int(op["child1_clv_index"]) < plan.tips and int(op["child2_clv_index"]) < plan.tips]


def set_branch(plan, matrix, length):
    """branch length of matrix slot `matrix` in the plan (a tree's slot is its child node's number)"""
    at = np.flatnonzero(np.asarray(plan.matrix_indices) == matrix)
    assert len(at) == 1
    plan.branch_lengths[at[0]] = float(length)


def zero_cherries(case, seed, every=8):
    """Changes `case` in place (its plan's branch lengths and its tip data); returns dict(cherries=[(a, b)...] with
    both branches at 0, conflicts={b: sites where b names another state than a}, inner=the inner matrix slot at 0)."""
    plan, sites, S = case["plan"], case["sites"], case["states"]
    rng = np.random.default_rng(11000 + seed)
    found = cherries(plan)
    chosen = found[:max(1, len(found) // 2)]
    assert chosen, "the tree has no cherry"
    idx = case.get("tip_index")
    plain = PLAIN.get(S, ALPHABET[:S])
    seqs = None if idx is not None else [bytearray(s) for s in case["seqs"]]
    conflicts = {}
    for a, b in chosen:
        set_branch(plan, a, 0.0)
        set_branch(plan, b, 0.0)
        at = np.flatnonzero(rng.random(sites) < 1.0 / every)
        if not len(at):
            at = rng.integers(0, sites, size=1)
        conflicts[b] = at
        if idx is not None:
            idx[b] = idx[a]
            for n in at:
                idx[b, n] = (max(int(idx[a, n]), 0) + 1 + int(rng.integers(0, S - 1))) % S
        else:
            seqs[b][:] = seqs[a]
            for n in at:
                other = [c for c in plain if c != seqs[a][n]]
                seqs[b][n] = other[int(rng.integers(0, len(other)))]
    if seqs is not None:
        case["seqs"] = [bytes(s) for s in seqs]
    # an inner branch: the first one in the op list's order (on a balanced tree it lies above a zero cherry, and the
    # quads of untouched cherries keep matrices with a positive bound)
    inner = [int(op["child%d_matrix_index" % k]) for op in plan.ops for k in (1, 2)
             if int(op["child%d_clv_index" % k]) >= plan.tips]
    inner = [m for m in inner if m != int(plan.root_edge[4])]
    slot = inner[0]
    set_branch(plan, slot, 0.0)
    return dict(cherries=chosen, conflicts=conflicts, inner=slot)


# name: (states, shape, tips, sites, 1 conflict in `every` sites, seed) -- 97 and 65 sites: a full tile and a ragged one
# of the 4-state and 20-state list kernels' tiles; seeds for which the oracle alone meets share_condition
ZERO_CASES = {"4-balanced16": (4, "balanced", 16, 97, 16, 1), "4-random23": (4, "random", 23, 97, 8, 1),
              "4-caterpillar12": (4, "caterpillar", 12, 97, 8, 1), "20-random11": (20, "random", 11, 65, 8, 1),
              "5-random12": (5, "random", 12, 37, 8, 1)}


def zero_case(lib, name, rate_cats=4):
    """(case, what zero_cherries did to it)"""
    from helpers import make_case, odd_state_case
    states, shape, tips, sites, every, seed = ZERO_CASES[name]
    if states in (4, 20):
        case = make_case(states, shape, tips, sites, rate_cats=rate_cats, seed=seed + sites)
        if states == 20:
            case["rates"], case["freqs"] = lib.aa_model("lg")
    else:
        case = odd_state_case(states, tips=tips, sites=sites, seed=seed + sites, shape=shape, rate_cats=rate_cats)
    return case, zero_cherries(case, seed, every)


def share_condition(per_site):
    """at least 3 sites are not finite, and at most a third of them; returns their mask"""
    bad = ~np.isfinite(per_site)
    assert 3 <= bad.sum() <= len(per_site) // 3, "%d of %d sites are not finite" % (bad.sum(), len(per_site))
    return bad


def zero_cherries_directed(case, seed, every=8):
    """zero_cherries for a tests/insertion_data.py case (character data), before its partition is built: the cherries
    among the tree's own tips; returns dict(cherries=[(a, b)...], inner=edge id)"""
    rng = np.random.default_rng(12000 + seed)
    n = case.n
    tip_edge = {b: e for e, (a, b, _) in enumerate(case.edges) if b < n}
    hang = {}
    for b, e in tip_edge.items():
        hang.setdefault(case.edges[e][0], []).append(b)
    found = [tuple(sorted(v)) for m, v in sorted(hang.items()) if len(v) == 2]
    chosen = found[:max(1, len(found) // 2)]
    assert chosen, "the tree has no cherry"
    plain = PLAIN.get(case.states, b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef"[:case.states])
    seqs = [bytearray(s) for s in case.seqs]

    def set_length(e, t):
        case.edges[e][2] = t
        case.lengths[e] = t
    for a, b in chosen:
        set_length(tip_edge[a], 0.0)
        set_length(tip_edge[b], 0.0)
        at = np.flatnonzero(rng.random(case.sites) < 1.0 / every)
        if not len(at):
            at = rng.integers(0, case.sites, size=1)
        seqs[b][:] = seqs[a]
        for s in at:
            other = [c for c in plain if c != seqs[a][s]]
            seqs[b][s] = other[int(rng.integers(0, len(other)))]
    case.seqs = [bytes(s) for s in seqs]
    inner = [e for e, (a, b, _) in enumerate(case.edges) if a >= n and b >= n]
    slot = inner[len(inner) // 2]
    set_length(slot, 0.0)
    return dict(cherries=chosen, inner=slot)


def agree(got, want, tol, what=""):
    """got against want, entry by entry, by class: NaN where want is NaN, the same infinity where want is infinite, and
    otherwise a finite number within tol relative (tol 0: equal); returns the largest relative difference"""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    nan, inf = np.isnan(w), np.isinf(w)
    assert (np.isnan(g) == nan).all(), "%s: NaN at %r, wanted at %r" % (what, np.argwhere(np.isnan(g))[:5].tolist(), np.argwhere(nan)[:5].tolist())
    assert (g[inf] == w[inf]).all(), "%s: %r where %r is wanted" % (what, g[inf][:5], w[inf][:5])
    fin = ~nan & ~inf
    assert np.isfinite(g[fin]).all(), what
    if not fin.any():
        return 0.0
    err = np.abs(g[fin] - w[fin])
    rel = float((err / np.maximum(np.abs(w[fin]), 1e-300)).max())
    assert (err <= tol * np.abs(w[fin])).all(), "%s: off by %.3g" % (what, rel)
    return rel
