"""pll_amd_simulate_columns without a device: the generator's known answers, the rule restated in NumPy byte for byte,
what a byte depends on, the distribution against exact site likelihoods, and the refusals."""
import numpy as np
import pytest

import simulate_data as SD
from exact_pruning import ExactRun
from libpll_amd.pllapi import ERROR_PARAM_INVALID, OPS_DTYPE, SIMULATE_NO_EDGE

SYMBOLS = {4: b"ACGT", 20: b"ARNDCQEGHILKMFPSTWYV", 7: b"abcdefg"}


# ---- the generator


KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(amd, counter, key, want):
    assert [int(x) for x in amd.philox4x32_10(counter, key)] == want
    assert [int(x[0]) for x in SD.philox(*[[c] for c in counter], *key)] == want   # (the yardstick's own generator)


# ---- the rule, byte for byte


@pytest.mark.parametrize("tree_name", list(SD.TREES))
@pytest.mark.parametrize("config", list(SD.CONFIGS))
def test_equals_the_restatement(amd, config, tree_name):
    case, tree = SD.case_of(config), SD.TREES[tree_name]()
    model = SD.host_model(amd, case, tree, SD.branch_lengths(tree))
    sym = SYMBOLS[case.states]
    kw = dict(seed=0x1234567 + len(tree_name), first_replicate=5, replicates=2, first_column=17, columns=150)
    got = SD.host_simulate(amd, model, tree, symbols=sym, **kw)
    want = SD.restate(model, tree.ops, tree.root, tree.edge, nodes=tree.nodes, symbols=sym, **kw)
    SD.same(got, want)
    if case.rate_cats > 1:
        assert len(np.unique(got["categories"])) == case.rate_cats
    assert got["invariant"].any() == bool(max(case.pinvs) > 0)


def test_columns_across_two_to_the_32(amd):
    """the carry into the counter's second word"""
    case, tree = SD.case_of("dna-g4-pinv"), SD.TREES["four-tips"]()
    model = SD.host_model(amd, case, tree, SD.branch_lengths(tree))
    kw = dict(seed=(0xfeedface << 32) | 0x0badcafe, first_replicate=0xfffffffe, replicates=3,
              first_column=2 ** 32 - 100, columns=300)
    got = SD.host_simulate(amd, model, tree, **kw)
    SD.same(got, SD.restate(model, tree.ops, tree.root, tree.edge, nodes=tree.nodes, **kw))
    # columns 2^32 - 1 and 2^32 are different columns, and neither is column 0 over again
    low = SD.host_simulate(amd, model, tree, seed=kw["seed"], first_replicate=0xfffffffe, replicates=3, first_column=0,
                           columns=300)
    assert got["out"][:, :, 100:].tobytes() != low["out"][:, :, :200].tobytes()


def test_zero_length_branch_and_pick_fallback(amd):
    case, tree = SD.case_of("dna-g4-pinv"), SD.TREES["balanced-16"]()
    lengths = SD.branch_lengths(tree)
    zero = tree.matrices[3]
    lengths[zero] = 0.0
    model = SD.host_model(amd, case, tree, lengths)
    model["pmatrices"][zero] = np.broadcast_to(np.eye(4), (4, 4, 4)).copy()   # exactly the identity
    # rows with a zero entry last: a state that is never entered, and frequencies whose sum stays below some u
    last = tree.matrices[5]
    pm = model["pmatrices"][last]
    pm[:, :, 2] += pm[:, :, 3]
    pm[:, :, 3] = 0.0
    pm *= 0.5                                      # rows sum to 0.5: half the draws find no c_j above u
    got = SD.host_simulate(amd, model, tree, seed=9, columns=2000)
    SD.same(got, SD.restate(model, tree.ops, tree.root, tree.edge, 9, 0, 1, 0, 2000, tree.nodes))
    steps = {s[2]: s for s in SD.walk_of(tree.ops, tree.root, tree.edge) if s[2] is not None}
    row = {n: j for j, n in enumerate(tree.nodes)}
    child, parent, _ = steps[zero]
    assert (got["out"][0, row[child]] == got["out"][0, row[parent]]).all()
    child, parent, _ = steps[last]
    below = got["out"][0, row[child]][got["invariant"][0] == 0]   # (an invariant column takes the root's state)
    assert not (below == 3).any() and (below == 2).mean() > 0.5   # the fallback is the last positive entry: 2


# ---- what a byte depends on


def test_bits_do_not_depend_on_the_request(amd):
    case, tree = SD.case_of("dna-matrix-per-category"), SD.TREES["balanced-16"]()
    model = SD.host_model(amd, case, tree, SD.branch_lengths(tree))
    whole = SD.host_simulate(amd, model, tree, seed=77, first_replicate=2, replicates=4, first_column=1000,
                             columns=400)
    part = SD.host_simulate(amd, model, tree, seed=77, first_replicate=3, replicates=2, first_column=1100,
                            columns=150)
    for key in ("categories", "invariant"):
        assert part[key].tobytes() == whole[key][1:3, 100:250].tobytes()
    assert part["out"].tobytes() == whole["out"][1:3, :, 100:250].tobytes()
    # a permuted and shortened node list
    order = np.random.default_rng(1).permutation(len(tree.nodes))[:11]
    sub = SD.host_simulate(amd, model, tree, nodes=[tree.nodes[j] for j in order], seed=77, first_replicate=2,
                           replicates=4, first_column=1000, columns=400)
    assert sub["out"].tobytes() == whole["out"][:, order].tobytes()
    # an inner node alone, no tip asked for; no optional output
    inner = [j for j, n in enumerate(tree.nodes) if n >= tree.tips][2]
    alone = SD.host_simulate(amd, model, tree, nodes=[tree.nodes[inner]], seed=77, first_replicate=2, replicates=4,
                             first_column=1000, columns=400, want=())
    assert set(alone) == {"out"} and alone["out"].tobytes() == whole["out"][:, [inner]].tobytes()
    # a repeated call; another seed is another alignment
    SD.same(whole, SD.host_simulate(amd, model, tree, seed=77, first_replicate=2, replicates=4, first_column=1000,
                                    columns=400))
    other = SD.host_simulate(amd, model, tree, seed=78, first_replicate=2, replicates=4, first_column=1000,
                             columns=400)
    assert (other["out"] != whole["out"]).mean() > 0.3


# ---- the distribution


BRANCHES = (0.1, 0.25, 0.05, 0.4, 0.15)
DIST_RATES = (0.137, 0.477, 1.0, 2.386)
DIST_SEEDS = (1, 2, 3, 0x123456789abcdef)
CHI2_BOUND = 414.5   # scipy.stats.chi2.isf(1e-9, 255), checked in the test


class _Plan:
    pass


def distribution_setup(amd):
    from distance_data import decompose
    rng = np.random.default_rng(12)
    exch, freqs = rng.uniform(0.5, 3.0, 6), rng.dirichlet(np.ones(4) * 6)
    lam, ev, iv = decompose(amd, 4, exch, freqs)
    ops = np.array([(4, -1, 0, 0, -1, 1, 1, -1), (5, -1, 2, 2, -1, 3, 3, -1)], dtype=OPS_DTYPE)
    emodel = dict(states=4, rate_cats=4, eigenvals=lam, eigenvecs=ev, inv_eigenvecs=iv, freqs=freqs,
                  rates=np.array(DIST_RATES), rate_weights=np.full(4, 0.25), pinv=0.15)
    # the 256 patterns as sites: tip t shows digit t of the pattern number in base 4
    pat = np.arange(256)
    digits = np.stack([(pat >> (2 * t)) & 3 for t in range(4)])
    tipclvs = np.zeros((4, 256, 4, 4))
    for t in range(4):
        tipclvs[t, pat, :, digits[t]] = 1.0
    invariant = np.where((digits == digits[0]).all(axis=0), digits[0], -1)

    def expected(scale):
        plan = _Plan()
        plan.matrix_indices, plan.branch_lengths, plan.ops = list(range(5)), [b * scale for b in BRANCHES], ops
        run = ExactRun(emodel, plan, tipclvs, invariant=invariant)
        _, per_site = run.edge_loglikelihood(5, 4, BRANCHES[4] * scale)
        p = np.exp(per_site).astype(np.float64)
        assert abs(p.sum() - 1.0) < 1e-12
        return run, p
    run, p_true = expected(1.0)
    _, p_long = expected(1.1)
    pm = {m: run.pmatrix(BRANCHES[m]).astype(np.float64) for m in range(5)}
    model = dict(states=4, pmatrices=pm, freqs=[freqs] * 4, weights=np.full(4, 0.25), pinv=np.full(4, 0.15))
    tree = SD.Tree(ops, 5, (4, 4), 4)
    return model, tree, p_true, p_long


def chi_square(out, p, columns):
    counts = np.bincount((out[0].astype(np.int64) << (2 * np.arange(4))[:, None]).sum(axis=0), minlength=256)
    e = columns * p
    assert e.min() >= 5
    return float(((counts - e) ** 2 / e).sum())


def test_the_distribution_is_the_site_likelihood(amd):
    """Pearson's chi-square of the 256 pattern counts of 2^18 columns against columns x exp(site lnL) of
    tests/exact_pruning.py, 255 degrees of freedom, bound chi2.isf(1e-9, 255) = 414.5.

    Measured with the NumPy restatement and with pll_amd_simulate_columns (the same bytes) on the committed seeds
    1, 2, 3, 0x123456789abcdef: chi-square 246.5, 272.5, 282.4, 283.9; the smallest expected count is 25.9.  Seed 1 against
    the likelihoods of branches 10 % longer: 751.4; seed 1 with the +I draw ignored: 6461.4."""
    from scipy.stats import chi2
    assert abs(chi2.isf(1e-9, 255) - CHI2_BOUND) < 0.05
    columns = 1 << 18
    model, tree, p_true, p_long = distribution_setup(amd)
    tips = [0, 1, 2, 3]
    first = None
    for seed in DIST_SEEDS:
        got = SD.host_simulate(amd, model, tree, nodes=tips, seed=seed, columns=columns, want=())
        x2 = chi_square(got["out"], p_true, columns)
        print("seed %#x: chi-square %.1f (smallest expected count %.1f)" % (seed, x2, columns * p_true.min()))
        assert x2 < CHI2_BOUND, (seed, x2)
        first = got if first is None else first
    # the test has power: slightly wrong likelihoods, and a simulator that forgets the invariant columns
    x2_long = chi_square(first["out"], p_long, columns)
    no_inv = dict(model, pinv=np.zeros(4))
    x2_inv = chi_square(SD.host_simulate(amd, no_inv, tree, nodes=tips, seed=DIST_SEEDS[0], columns=columns,
                                         want=())["out"], p_true, columns)
    print("10 %% longer branches: %.1f; +I ignored: %.1f" % (x2_long, x2_inv))
    assert x2_long > CHI2_BOUND and x2_inv > CHI2_BOUND


def test_the_restatement_has_that_distribution_too(amd):
    """the yardstick itself, on fewer columns (it is NumPy): the same bytes as the C, so the same statistic"""
    columns = 1 << 14
    model, tree, _, _ = distribution_setup(amd)
    got = SD.host_simulate(amd, model, tree, nodes=[0, 1, 2, 3], seed=1, columns=columns)
    SD.same(got, SD.restate(model, tree.ops, tree.root, tree.edge, 1, 0, 1, 0, columns, [0, 1, 2, 3]))


# ---- refusals


def test_refusals_leave_the_outputs_alone(amd):
    case, tree = SD.case_of("dna-g4-pinv"), SD.TREES["four-tips"]()
    model = SD.host_model(amd, case, tree, SD.branch_lengths(tree))
    base = dict(states=4, pmatrices=model["pmatrices"], frequencies=model["freqs"], rate_weights=model["weights"],
                prop_invar=model["pinv"], ops=tree.ops, root=tree.root, edge=tree.edge, seed=3, replicates=2,
                columns=10, nodes=tree.nodes, clv_count=tree.clv_count)

    def ops_with(i, **fields):
        ops = tree.ops.copy()
        for k, v in fields.items():
            ops[k][i] = v
        return ops
    swapped = tree.ops[::-1].copy()
    bad = {
        "no replicate": dict(replicates=0),
        "no column": dict(columns=0),
        "no node": dict(nodes=[]),
        "columns wrap": dict(first_column=2 ** 64 - 5),
        "root out of range": dict(root=tree.clv_count),
        "edge clv out of range": dict(edge=(tree.clv_count, tree.edge[1])),
        "edge matrix out of range": dict(edge=(tree.edge[0], max(model["pmatrices"]) + 1)),
        "child out of range": dict(ops=ops_with(0, child1_clv_index=tree.clv_count)),
        "matrix out of range": dict(ops=ops_with(0, child2_matrix_index=99)),
        "a parent without a state": dict(ops=swapped),
        "a node twice": dict(ops=ops_with(0, child2_clv_index=int(tree.ops["child1_clv_index"][0]))),
        "the edge's end again": dict(ops=ops_with(0, child1_clv_index=tree.edge[0])),
        "a requested node without a state": dict(nodes=[0, 1, tree.clv_count + 3], clv_count=tree.clv_count + 4),
        "a missing matrix": dict(pmatrices={m: (None if m == 1 else v) for m, v in model["pmatrices"].items()}),
        "no states": dict(states=0),
        "256 states": dict(states=256),
    }
    for name, change in bad.items():
        kw = dict(base, **change)
        raw = dict(out=np.full((2, max(len(kw["nodes"]), 1), 10), 0x5a, dtype=np.uint8),
                   categories=np.full((2, 10), 0x5a5a5a5a, dtype=np.uint32),
                   invariant=np.full((2, 10), 0x5a, dtype=np.uint8))
        amd.clear_error()
        assert not amd.simulate_columns(raw=raw, **kw), name
        assert amd.errno() == ERROR_PARAM_INVALID, (name, amd.errmsg())
        assert (raw["out"] == 0x5a).all() and (raw["categories"] == 0x5a5a5a5a).all() and \
            (raw["invariant"] == 0x5a).all(), name
    # NULL arrays
    for missing in ("out",):
        raw = dict(out=None, categories=np.full((2, 10), 7, dtype=np.uint32), invariant=None)
        amd.clear_error()
        assert not amd.simulate_columns(raw=raw, **base)
        assert amd.errno() == ERROR_PARAM_INVALID and (raw["categories"] == 7).all()
    amd.clear_error()
    assert not amd.lib.pll_amd_simulate_columns(4, 4, None, 0, None, None, None, None, 0, 1, 0, SIMULATE_NO_EDGE, 0, 1, 0,
                                                1, 0, 1, None, 1, None, None, None, None)
    assert amd.errno() == ERROR_PARAM_INVALID
    # nothing above left a trace
    good = amd.simulate_columns(**base)
    SD.same(good, SD.restate(model, tree.ops, tree.root, tree.edge, 3, 0, 2, 0, 10, tree.nodes))
