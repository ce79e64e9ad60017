"""Data for the model-scoring tests (tests/test_gpu_model_score.py, tests/test_model_score_host.py).

Trees and alignments are those of tests/tree_score_data.py / tests/insertion_data.py.  A candidate model is the dict
`Partition.model_loglikelihood` takes: any of subst_params / frequencies (one entry per rate-matrix set, None = the
partition's), prop_invar (one number per set), category_rates, category_weights; a key that is missing means the
partition's value.  `sequence_lnl` is the definition of a candidate's value (include/pll_amd.h): the setters,
pll_update_eigen and the three calls of the tree on the same partition -- which is then left holding the candidate:
`restore` puts the case's own model, matrices and CLVs back.
"""
import numpy as np

import tree_score_data as T

BASE_ALPHA = 0.6   # (insertion_data.build)
GAMMA_BRACKET = (0.3, 1.0, 2.5, 5.0)


def base_model(lib, case):
    """the case's own model, every field spelled out"""
    R = case.rate_cats
    w = np.full(R, 1.0 / R) if case.cat_weights is None else np.array(case.cat_weights, dtype=np.float64)
    return dict(subst_params=[np.array(r, dtype=np.float64) for r, f in case.models],
                frequencies=[np.array(f, dtype=np.float64) for r, f in case.models],
                prop_invar=[float(v) for v in case.pinvs], category_rates=lib.compute_gamma_cats(BASE_ALPHA, R),
                category_weights=w)


def bracket_rates(lib, case, alpha):
    """the category rates of a Gamma shape.  At one category the mean rate is 1 whatever the shape: the bracket is a
    free rate there"""
    if case.rate_cats == 1:
        return np.array([0.4 + 0.5 * alpha])
    return lib.compute_gamma_cats(alpha, case.rate_cats)


def eight_models(lib, case, seed=5):
    """each field alone -- the exchangeabilities of ONE set only (the set of the last, fastest category: the slowest
    one's matrices are near the identity whatever its exchangeabilities; the other entries None), the frequencies of
    every set, the +I proportions flipped 0 <-> positive, unequal category weights, the category rates of three Gamma
    shapes -- and all of them together at a fourth shape"""
    rng = np.random.default_rng(seed)
    S, R, M = case.states, case.rate_cats, case.nmodels
    one = case.params[-1]
    subst = [None] * M
    subst[one] = rng.uniform(0.4, 3.5, S * (S - 1) // 2)
    freqs = [rng.dirichlet(np.ones(S) * 6) for _ in range(M)]
    flipped = [0.0 if v > 0 else 0.15 + 0.05 * i for i, v in enumerate(case.pinvs)]
    weights = rng.dirichlet(np.ones(R)) * 1.2
    models = [dict(subst_params=subst), dict(frequencies=freqs), dict(prop_invar=flipped),
              dict(category_weights=weights)]
    models += [dict(category_rates=bracket_rates(lib, case, a)) for a in GAMMA_BRACKET[:3]]
    models.append(dict(subst_params=[rng.uniform(0.4, 3.5, S * (S - 1) // 2) for _ in range(M)],
                       frequencies=[rng.dirichlet(np.ones(S) * 6) for _ in range(M)],
                       prop_invar=[0.05 + 0.1 * i for i in range(M)], category_weights=rng.dirichlet(np.ones(R)) * 0.9,
                       category_rates=bracket_rates(lib, case, GAMMA_BRACKET[3])))
    return models


def needs_invariant_sites(case):
    """the partition has no invariant index yet (insertion_data.build computes it with the first positive proportion)"""
    return max(case.pinvs) == 0


def apply_model(p, model):
    """the sequence's first three steps: really set the partition to the model"""
    sp, fr = model.get("subst_params"), model.get("frequencies")
    for i in range(p.s.rate_matrices):
        changed = False
        if sp is not None and sp[i] is not None:
            p.set_subst_params(i, sp[i])
            changed = True
        if fr is not None and fr[i] is not None:
            p.set_frequencies(i, fr[i])
            changed = True
        if changed:
            p.update_eigen(i)
    if model.get("prop_invar") is not None:
        for i, v in enumerate(model["prop_invar"]):
            p.update_invariant_sites_proportion(i, float(v))
    if model.get("category_rates") is not None:
        p.set_category_rates(model["category_rates"])
    if model.get("category_weights") is not None:
        p.set_category_weights(model["category_weights"])


def sequence_lnl(p, base, model, tree):
    """the definition, on a partition that holds `base`: the model's fields set, then the tree's three calls"""
    apply_model(p, base)
    apply_model(p, model)
    return T.sequence_lnl(p, tree)


def restore(p, case, base):
    apply_model(p, base)
    T.restore(p, case)


def inner_edge(case):
    """an edge with both sides inner where the tree has one (insertion_data.assert_discriminates picks the same)"""
    return max(range(len(case.edges)), key=lambda e: min(case.edges[e][0], case.edges[e][1]))


def assert_tells_apart(values, floor=1e-6):
    """every two of the values differ by more than `floor` relative: the floor of helpers.assert_discriminates"""
    v = [float(x) for x in values]
    for i in range(len(v)):
        for j in range(i):
            assert abs(v[i] - v[j]) > floor * abs(v[j]), "the fixture does not tell %d and %d apart: %r %r" % (
                j, i, v[j], v[i])


def model_state(p):
    """what the partition holds of its model on the host, as bytes"""
    s = p.s
    S, R, M = s.states, s.rate_cats, s.rate_matrices
    nsub = S * (S - 1) // 2
    arr = lambda ptr, n: np.ctypeslib.as_array(ptr, shape=(n,)).copy().tobytes()  # noqa: E731
    out = [arr(s.rates, R), arr(s.rate_weights, R), arr(s.prop_invar, M)]
    for i in range(M):
        out += [arr(s.frequencies[i], S), arr(s.subst_params[i], nsub), arr(s.eigenvals[i], S),
                arr(s.eigenvecs[i], S * S), arr(s.inv_eigenvecs[i], S * S)]
    return out
