"""The default small-partition path: host mirrors kept current by the library itself, on every route.

A partition whose CLVs stay below PLL_AMD_AUTO_MIRROR_MB (default 64 MB) fills partition->clv[] / ->scale_buffer[] /
->pmatrix[] by itself.  tests/conftest.py switches that off for the suite; every test here takes the variable away
again before it creates a partition (it is read in pll_partition_create).  What only happens in this configuration:

  * pll_update_partials ends in pllhip_mirror_batch / k_mirror_copy: a job list built in host/hotpath.c, flushed every
    64 jobs, each flush launched in groups of 48 buffers, 16 bytes per lane and a word tail;
  * the device runs without deferred cherries, unstored pair products, pair folds and the edge fold, and the 20-state
    scaling certificate is resolved inside the mirror call;
  * pll_update_prob_matrices copies the range of matrices it was given, pll_set_tip_clv / pll_set_tip_states refresh
    the tip's mirror, pll_update_sumtable fills the caller's buffer; sharded partitions and partitions with site
    repeats copy buffer by buffer.

Every comparison reads the struct fields first and copies them (tests/default_mirror_data.py), and has two
expectations behind it: the oracle (counts bit for bit, CLVs by helpers.clv_ok with helpers.clvs_bitwise) and a twin
partition created with PLL_AMD_AUTO_MIRROR_MB=0 that is given the same calls and read through the pll_amd_sync_*
calls -- equal bytes, for every state count: the library promises the same bits with deferral on or off.
"""
import numpy as np
import pytest

import default_mirror_data as D
from default_mirror_data import assert_current, snapshot, written_by
from helpers import (make_case, odd_state_case, many_state_case, build_partition, oracle_run, bits_equal, rel_err,
                     clv_ok, clvs_bitwise, sumtable_err, random_sequence_case, repeat_columns, mixture, params_of)
from libpll_amd.pllapi import (ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_SITE_REPEATS, ATTRIB_AB_LEWIS,
                               ATTRIB_ARCH_AVX2)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("dna_path")]

POISON = 0x7FF453554D544142     # PLL_AMD_SUMTABLE_POISON (include/pll_amd.h)


def _pair(gpu, case, attrs, monkeypatch, build=build_partition):
    return D.pair(gpu, case, attrs, monkeypatch, build)


# ---- 1. flush and launch boundaries

_BOUNDARY = {}      # states -> (case, oracle after the full list): computed once, left unchanged


def _boundary_case(gpu, orc, p, states):
    if states not in _BOUNDARY:
        case = make_case(states, "random", 110, 37, seed=5)
        o = oracle_run(orc, gpu, p, case, ATTRIB_PATTERN_TIP)
        o.update_partials()
        _BOUNDARY[states] = (case, o)
    return _BOUNDARY[states]


@pytest.mark.parametrize("k", [23, 24, 25, 31, 32, 33, 47, 48, 49, 64, 108])
@pytest.mark.parametrize("states", [4, 20])
def test_flush_and_launch_boundaries(gpu, orc, monkeypatch, states, k):
    """The first k ops of a 108-op post-order list (a prefix is a valid list): two jobs per op, so k = 24 fills one
    k_mirror_copy launch of 48 buffers and 25 starts a second; 32 fills the 64 jobs of one flush in hotpath.c and 33
    starts a second; 48, 64 and 108 are the same boundaries further on.  Every parent and scale buffer of the prefix
    is current; no mirror exists for a CLV the prefix did not write.  (A prefix's CLVs are the full list's: every
    parent is written once, from operands earlier in the list -- one oracle run serves every k.)"""
    case = make_case(states, "random", 110, 37, seed=5)
    plan = case["plan"]
    assert len(plan.ops) == 108
    p, t = _pair(gpu, case, ATTRIB_PATTERN_TIP, monkeypatch)
    _, o = _boundary_case(gpu, orc, p, states)
    prefix, rest = plan.ops[:k], plan.ops[k:]
    p.update_partials(prefix)
    t.update_partials(prefix)
    assert not t.s.clv[int(prefix[0]["parent_clv_index"])], "the twin mirrors by itself"
    assert_current(p, t, o, prefix, states, "k = %d:" % k)
    # once more over poisoned mirrors (the same list gives the same values): a job dropped at a boundary is most often
    # a scale buffer, whose counts on a tree this shallow equal the zeros of a fresh mirror
    D.poison(p, *written_by(prefix))
    p.update_partials(prefix)
    t.update_partials(prefix)
    assert_current(p, t, o, prefix, states, "k = %d, over poisoned mirrors:" % k)
    for op in rest:
        assert not p.s.clv[int(op["parent_clv_index"])], "a mirror of CLV %d, which no op wrote" % int(op["parent_clv_index"])
        assert not p.s.scale_buffer[int(op["parent_scaler_index"])]
    for tip in range(plan.tips):
        assert not p.s.clv[tip]
    p.destroy()
    t.destroy()


# ---- 2. random op sequences

@pytest.mark.parametrize("seed", range(8))
def test_random_op_sequences_under_the_default(gpu, orc, monkeypatch, seed):
    """tests/test_gpu_api.py::test_random_op_sequences on mirroring partitions: 120 ops over ten CLV slots, each
    written many times, a quarter of the ops without a parent scale buffer (odd job counts), with and without pattern
    tips, per-site and per-rate scalers; in one call and in five random pieces.  After every call the mirrors of what
    that call named equal the oracle advanced by the same ops, and the twin."""
    monkeypatch.delenv("PLLHIP_AA_EXACT", raising=False)
    # (20 states: tip-inner mat-vecs in the reference's order, as in test_random_op_sequences and for its reason -- these
    # lists feed one CLV to both sides of an op again and again, which doubles any last-bit difference each time)
    monkeypatch.setenv("PLLHIP_AA_TI_MFMA", "0")
    case, attrs, ops, rng = random_sequence_case(seed)
    S = case["states"]
    assert (ops["parent_scaler_index"] < 0).sum() >= 10 and len(set(ops["parent_clv_index"].tolist())) <= 10
    cut = sorted(int(x) for x in rng.integers(1, len(ops), size=5))
    for pieces in ([(0, len(ops))], [(lo, hi) for lo, hi in zip([0] + cut, cut + [len(ops)]) if hi > lo]):
        p, t = _pair(gpu, case, attrs, monkeypatch)
        o = oracle_run(orc, gpu, p, case, attrs)
        for lo, hi in pieces:
            for x in (p, t, o):
                x.update_partials(ops[lo:hi])
            assert_current(p, t, o, ops[lo:hi], S, "seed %d, ops %d..%d:" % (seed, lo, hi))
        p.destroy()
        t.destroy()


# ---- 3. alignment and odd shapes

def _shape_case(states, rate_cats, sites):
    if states in (4, 20):
        return make_case(states, "random", 12, sites, rate_cats=rate_cats, seed=states + sites)
    if states > 32:
        return many_state_case(states, tips=12, sites=sites, seed=states + sites, rate_cats=rate_cats)
    return odd_state_case(states, tips=12, sites=sites, seed=states + sites, rate_cats=rate_cats)


@pytest.mark.parametrize("rate_scalers", [False, True], ids=["per-site", "per-rate"])
@pytest.mark.parametrize("states,rate_cats,sites", [(5, 1, 51), (7, 1, 51), (5, 3, 51), (13, 2, 51), (2, 4, 97),
                                                    (61, 2, 51), (4, 1, 51), (20, 1, 51)])
def test_alignment_and_odd_shapes(gpu, orc, monkeypatch, states, rate_cats, sites, rate_scalers):
    """k_mirror_copy moves 16 bytes per lane whatever the addresses: CLVs lie states x rate_cats x (sites + 64) doubles
    apart on the device, an odd number for (5, 1, 51), (7, 1, 51) and (5, 3, 51) -- every second CLV is 8-byte aligned
    only -- and per-site scale buffers 51 + 64 counts, so every second one is 4-byte aligned only.  The other shapes:
    word counts that are and are not multiples of four, the kernels of partials_gen_tile.hip, tips as CLVs."""
    stride = states * rate_cats * (sites + 64)
    assert (stride % 2 == 1) == ((states, rate_cats) in ((5, 1), (7, 1), (5, 3)))
    for pattern_tip in ((True, False) if states <= 32 else (False,)):
        attrs = (ATTRIB_PATTERN_TIP if pattern_tip else 0) | (ATTRIB_RATE_SCALERS if rate_scalers else 0)
        case = _shape_case(states, rate_cats, sites)
        plan = case["plan"]
        p, t = _pair(gpu, case, attrs, monkeypatch)
        o = oracle_run(orc, gpu, p, case, attrs)
        for x in (p, t, o):
            x.update_partials(plan.ops)
        assert_current(p, t, o, plan.ops, states, "%d states, pattern tips %r:" % (states, pattern_tip))
        D.poison(p, *written_by(plan.ops))            # (a tail word left out shows even where the count is zero)
        p.update_partials(plan.ops)
        t.update_partials(plan.ops)
        assert_current(p, t, o, plan.ops, states, "%d states, pattern tips %r, over poisoned mirrors:" % (states, pattern_tip))
        if not pattern_tip:
            for tip in range(plan.tips):
                assert bits_equal(D.clv_mirror(p, tip), o.clv[tip]), "mirror of tip %d" % tip
        p.destroy()
        t.destroy()


# ---- 4. mirrors of CLVs a call did not write

def _unchanged(p, first, addresses, skip_nodes, skip_scalers, what):
    """every mirror of `first` (a snapshot) but the skipped ones: the same pointer, the same bytes"""
    clvs, counts = first
    for node in clvs:
        if node not in skip_nodes:
            assert D.address(p.s.clv[node]) == addresses[0][node], "%s: CLV mirror %d moved" % (what, node)
            assert bits_equal(D.clv_mirror(p, node), clvs[node]), "%s: CLV mirror %d changed" % (what, node)
    for sc in counts:
        if sc not in skip_scalers:
            assert D.address(p.s.scale_buffer[sc]) == addresses[1][sc], "%s: scaler mirror %d moved" % (what, sc)
            assert (D.scaler_mirror(p, sc) == counts[sc]).all(), "%s: scaler mirror %d changed" % (what, sc)


def _addresses(p, nodes, scalers):
    return ({n: D.address(p.s.clv[n]) for n in nodes}, {s: D.address(p.s.scale_buffer[s]) for s in scalers})


@pytest.mark.parametrize("states", [4, 20])
def test_mirrors_a_call_did_not_write(gpu, orc, monkeypatch, states):
    """A partial traversal after three branch lengths changed: the rewritten parents equal a fresh oracle's with the
    new lengths, every other mirror keeps its pointer and its bytes.  Then the same with a root that moves: two
    re-rootings of tests/moving_root.py's walk, whose lists overwrite CLVs with values that point the other way."""
    import moving_root
    case = make_case(states, "random", 24, 97)
    plan, R = case["plan"], case["rate_cats"]
    attrs = ATTRIB_PATTERN_TIP
    p, t = _pair(gpu, case, attrs, monkeypatch)
    o = oracle_run(orc, gpu, p, case, attrs)
    for x in (p, t, o):
        x.update_partials(plan.ops)
    first = assert_current(p, t, o, plan.ops, states, "full traversal:")
    nodes, scalers = written_by(plan.ops)
    where = _addresses(p, nodes, scalers)
    changed = [3, int(plan.ops[2]["parent_clv_index"]), int(plan.ops[len(plan.ops) // 2]["child1_clv_index"])]
    lengths = np.random.default_rng(5).uniform(0.3, 0.9, 3)
    for x in (p, t):
        x.update_prob_matrices([0] * R, changed, lengths)
    D.set_lengths(plan, changed, lengths)
    sub = D.ops_above(plan, changed)
    assert 0 < len(sub) < len(plan.ops)
    for x in (p, t):
        x.update_partials(sub)
    fresh = oracle_run(orc, gpu, p, case, attrs)       # (the plan's new lengths)
    fresh.update_partials()
    # the untouched mirrors first: nothing below has been read through a sync call on p
    rewritten = written_by(sub)
    _unchanged(p, first, where, set(rewritten[0]), set(rewritten[1]), "partial traversal")
    assert_current(p, t, fresh, sub, states, "partial traversal:")
    assert any(not bits_equal(D.clv_mirror(p, n), first[0][n]) for n in rewritten[0]), "the new lengths changed nothing"
    p.destroy()
    t.destroy()

    # a moving root
    the_plan, view, moves = moving_root.walk("random", 24, 1)
    case = make_case(states, "random", 24, 97)
    case["plan"] = the_plan
    p, t = _pair(gpu, case, attrs, monkeypatch)
    o = oracle_run(orc, gpu, p, case, attrs)
    for x in (p, t, o):
        x.update_partials(moves[0]["ops"])
    assert_current(p, t, o, moves[0]["ops"], states, "move 0:")
    nodes, scalers = written_by(moves[0]["ops"])
    where = _addresses(p, nodes, scalers)
    done = 0
    for k, mv in enumerate(moves[1:], 1):
        if mv["changed"] is not None:
            for x in (p, t):
                x.update_prob_matrices([0] * R, [mv["changed"][0]], [mv["changed"][1]])
            o.pmat[mv["changed"][0]] = D.oracle_pmatrix(orc, o, mv["changed"][1])
        if not len(mv["ops"]):
            continue
        before = snapshot(p, nodes, scalers)
        for x in (p, t, o):
            x.update_partials(mv["ops"])
        rewritten = written_by(mv["ops"])
        assert len(rewritten[0]) < len(nodes)
        _unchanged(p, before, where, set(rewritten[0]), set(rewritten[1]), "move %d" % k)
        assert_current(p, t, o, mv["ops"], states, "move %d:" % k)
        done += 1
        if done == 2:
            break
    assert done == 2
    p.destroy()
    t.destroy()


# ---- 5. P-matrix mirrors

@pytest.mark.parametrize("kind", ["dna", "aa", "mixture"])
def test_pmatrix_mirrors(gpu, orc, monkeypatch, kind):
    """pll_update_prob_matrices copies ONE range, from the lowest to the highest index it was given: matrices 9, 2 and
    5 get new lengths on a partition whose matrices 0..11 were computed before.  The three show the new matrices, bit
    for bit the oracle's; 3, 4, 6, 7 and 8 -- inside the range, rewritten with what the device holds -- and 0, 1, 10
    and 11 still hold their earlier ones.  mixture: another rate matrix per category (helpers.mixture)."""
    states = 20 if kind == "aa" else 4
    case = make_case(states, "random", 8, 50, seed=3)
    if kind == "mixture":
        mixture(case, gpu, seed=2)
        assert len(set(params_of(case))) > 1
    pi = params_of(case)
    p, t = _pair(gpu, case, ATTRIB_PATTERN_TIP, monkeypatch)
    o = oracle_run(orc, gpu, p, case, ATTRIB_PATTERN_TIP)
    rng = np.random.default_rng(12)
    old = rng.uniform(0.02, 0.6, 12)
    for x in (p, t):
        x.update_prob_matrices(pi, np.arange(12), old)
    before = [D.pmatrix_mirror(p, m) for m in range(12)]
    for m in range(12):
        assert bits_equal(before[m], D.oracle_pmatrix(orc, o, old[m])), "matrix %d" % m
    named, new = [9, 2, 5], rng.uniform(0.7, 1.4, 3)
    for x in (p, t):
        x.update_prob_matrices(pi, named, new)
    after = [D.pmatrix_mirror(p, m) for m in range(12)]
    for m, length in zip(named, new):
        assert bits_equal(after[m], D.oracle_pmatrix(orc, o, length)), "matrix %d: the new length" % m
        assert not bits_equal(after[m], before[m])
    for m in range(12):
        if m not in named:
            assert bits_equal(after[m], before[m]), "matrix %d was not named" % m
        assert bits_equal(after[m], t.get_pmatrix(m)), "matrix %d: the twin's" % m
    p.destroy()
    t.destroy()


# ---- 6. tip writers and mirrors that a sync call allocated

@pytest.mark.parametrize("states", [4, 20])
def test_tip_writers_and_mirrors_of_the_sync_path(gpu, orc, monkeypatch, states):
    """Tips as CLVs.  Mirrors that pll_amd_sync_clv / pll_amd_sync_scaler allocated -- get_clv and get_scaler on a node
    before the first list writes it, pll_set_tip_clv on an inner index -- are not pinned memory of the device layer:
    the list's copy takes the per-buffer branch for them (hotpath.c) and they are as current as the others.
    pll_set_tip_clv on a tip after a traversal shows in the tip's mirror.  A mirror changed by hand and pushed
    (pll_amd_push_clv) is what the op above it reads.  Destroy frees both kinds of mirror: 50 more partitions."""
    case = make_case(states, "random", 10, 97, seed=6)
    plan, R = case["plan"], case["rate_cats"]
    sites = case["sites"]
    rng = np.random.default_rng(states)
    p, t = _pair(gpu, case, 0, monkeypatch)
    o = oracle_run(orc, gpu, p, case, 0)
    synced, set_by_hand = int(plan.ops[0]["parent_clv_index"]), int(plan.ops[1]["parent_clv_index"])
    synced_sc = int(plan.ops[0]["parent_scaler_index"])
    assert not p.s.clv[synced] and not p.s.scale_buffer[synced_sc]
    assert not p.get_clv(synced).any() and not p.get_scaler(synced_sc).any()       # allocated by the sync calls
    junk = rng.uniform(0.1, 1.0, (sites, states))
    for x in (p, t):
        x.set_tip_clv(set_by_hand, junk.reshape(-1))                                  # an inner index: allowed
    assert bits_equal(D.clv_mirror(p, set_by_hand), np.repeat(junk[:, None, :], R, axis=1))
    for x in (p, t, o):
        x.update_partials(plan.ops)
    assert_current(p, t, o, plan.ops, states, "full traversal:")
    # a tip gets a new vector
    tip = 2
    vec = rng.uniform(0.0, 1.0, (sites, states))
    for x in (p, t):
        x.set_tip_clv(tip, vec.reshape(-1))
    o.clv[tip] = np.repeat(vec[:, None, :], R, axis=1)
    assert bits_equal(D.clv_mirror(p, tip), o.clv[tip]), "the tip's mirror shows the new vector"
    assert bits_equal(D.clv_mirror(p, tip), t.get_clv(tip))
    sub = D.ops_above(plan, [tip])
    for x in (p, t, o):
        x.update_partials(sub)
    assert_current(p, t, o, sub, states, "above the new tip:")
    # mirrors changed by hand and pushed: one the sync path allocated, one the list's copy did
    pinned = next(int(op["parent_clv_index"]) for op in plan.ops[2:] if int(op["parent_clv_index"]) in plan.parent_of)
    for node in (synced, pinned):
        live = np.ctypeslib.as_array(p.s.clv[node], shape=(p.sites_total * p.span,))
        live[:] = live * rng.uniform(0.5, 1.5, live.size)
        values = live.copy()
        assert p.lib.pll_amd_push_clv(p.ptr, node) == 1, gpu.errmsg()
        t.put_clv(node, values)
        o.clv[node] = values.reshape(o.clv[node].shape)
        above = plan.ops[[node in (int(op["child1_clv_index"]), int(op["child2_clv_index"])) for op in plan.ops]]
        assert len(above) == 1
        for x in (p, t, o):
            x.update_partials(above)
        assert_current(p, t, o, above, states, "above the pushed CLV %d:" % node)
        assert bits_equal(D.clv_mirror(p, node).reshape(-1), values), "the pushed mirror itself is left alone"
    p.destroy()
    t.destroy()
    small = make_case(4, "balanced", 4, 20, seed=1)
    for k in range(50):
        attrs = ATTRIB_PATTERN_TIP if k % 2 else 0
        q = build_partition(gpu, small, attrs)
        node, sc = int(small["plan"].ops[0]["parent_clv_index"]), int(small["plan"].ops[0]["parent_scaler_index"])
        q.get_clv(node)                                     # a mirror of the sync path ...
        q.update_partials(small["plan"].ops)               # ... next to pinned ones
        assert q.s.clv[node] and q.s.scale_buffer[sc] and q.s.clv[int(small["plan"].ops[-1]["parent_clv_index"])]
        q.destroy()


# ---- 7. ascertainment bias

@pytest.mark.parametrize("states,pattern_tip", [(4, True), (4, False), (20, False)])
def test_ascertainment_bias_mirrors(gpu, ref, monkeypatch, states, pattern_tip):
    """Lewis correction: every CLV has sites + states rows and every scale buffer sites + states counts (x rate_cats
    per rate), and so have the mirrors -- equal to the genuine reference's own partition->clv[] / ->scale_buffer[],
    both read from the struct fields.  (20 states: tips as CLVs, pll_partition_create refuses pattern tips there.)"""
    from test_gpu_asc_bias import build
    monkeypatch.delenv(D.ENV, raising=False)
    case = make_case(states, "random", 9, 40, seed=states + 1)
    plan = case["plan"]
    attrs = ATTRIB_AB_LEWIS | (ATTRIB_PATTERN_TIP if pattern_tip else 0)
    g, r = build(gpu, case, attrs), build(ref, case, attrs | ATTRIB_ARCH_AVX2)
    g.update_partials(plan.ops)
    r.update_partials(plan.ops)
    nodes, scalers = written_by(plan.ops)
    if not pattern_tip:
        nodes = list(range(plan.tips)) + nodes
    clvs, counts = snapshot(g, nodes, scalers)
    want_clvs, want_counts = snapshot(r, nodes, scalers)
    assert g.sites_total == 40 + states
    for node in nodes:
        assert clvs[node].shape == (40 + states, case["rate_cats"], states)
        exact = clvs_bitwise(states) or node < plan.tips
        assert clv_ok(clvs[node], want_clvs[node], exact), "CLV mirror %d (with its extra sites)" % node
    for sc in scalers:
        assert counts[sc].shape == (40 + states,) and (counts[sc] == want_counts[sc]).all(), "scaler mirror %d" % sc
    g.destroy()
    r.destroy()


# ---- 8. sumtables

@pytest.mark.parametrize("states", [4, 20])
def test_sumtables_fill_the_callers_buffer(gpu, orc, monkeypatch, states):
    """On a mirroring partition pll_update_sumtable fills the caller's buffer instead of marking it with
    PLL_AMD_SUMTABLE_POISON: read without a sync call, one inner-inner and one tip-inner table against the oracle
    under the bound of tests/test_gpu_api.py::test_many_live_sumtables_and_caller_filled_tables (1e-10), and equal to
    the twin's synced table; the derivatives computed from it as there."""
    from test_gpu_api import _edges_for_sumtables
    case = make_case(states, "random", 10, 97, seed=7)
    plan, R = case["plan"], case["rate_cats"]
    p, t = _pair(gpu, case, ATTRIB_PATTERN_TIP, monkeypatch)
    o = oracle_run(orc, gpu, p, case, ATTRIB_PATTERN_TIP)
    for x in (p, t, o):
        x.update_partials(plan.ops)
    edges = _edges_for_sumtables(plan)
    inner, tip = next(e for e in edges if e[2] >= plan.tips), next(e for e in edges if e[2] < plan.tips)
    for (pc, ps, cc, cs) in (inner, tip):
        st, st_twin = p.alloc_sumtable(), t.alloc_sumtable()
        st[:] = 0.0
        p.update_sumtable(pc, cc, ps, cs, [0] * R, st)
        got = st.copy()                                       # the caller's buffer as it stands
        assert not (got.view(np.uint64) == POISON).any() and not np.isnan(got).any()
        want = o.sumtable(pc, cc, ps, cs)
        err = sumtable_err(got.reshape(want.shape), want)
        print("sumtable (%d, %d): %.3g" % (pc, cc, err))
        assert err < 1e-10
        t.update_sumtable(pc, cc, ps, cs, [0] * R, st_twin)
        assert bits_equal(got.reshape(want.shape), t.get_sumtable(st_twin)), "the twin's table"
        d = p.compute_likelihood_derivatives(ps, cs, 0.3, [0] * R, st)
        assert rel_err(d, o.derivatives(want, 0.3)) < 1e-10
    p.destroy()
    t.destroy()


# ---- 9. the scaling certificate

_AT_THRESHOLD = {}      # the branch lengths tests/test_gpu_cert.py's bisection arrives at, found once


def test_certificate_rerun_is_what_the_mirrors_show(gpu, orc, monkeypatch):
    """The fixture of tests/test_gpu_cert.py::test_certificate_trips_and_the_list_runs_again (just below the threshold,
    per-site scalers; 16 MB of CLVs, so the partition mirrors): the certificate is resolved inside the mirror call,
    before the copy -- when pll_update_partials returns, the counters show the re-run and every mirror holds the
    re-run's values, the oracle's bit for bit, counts included.  A copy taken before the re-run would show the matrix
    cores' values and, at the site at the threshold, the other count."""
    from test_gpu_cert import _place_at_threshold
    monkeypatch.setenv("PLLHIP_FUSED", "2")      # the whole-list kernel at this size
    monkeypatch.delenv("PLLHIP_AA_TI_MFMA", raising=False)
    monkeypatch.delenv("PLLHIP_AA_EXACT", raising=False)
    attrs = ATTRIB_PATTERN_TIP
    case = make_case(20, "caterpillar", 260, 96, seed=11)
    case["rates"], case["freqs"] = gpu.aa_model("lg")
    plan = case["plan"]
    if "lengths" not in _AT_THRESHOLD:
        with D.no_mirrors(monkeypatch):
            p0 = build_partition(gpu, case, attrs)
        o = oracle_run(orc, gpu, p0, case, attrs)
        p0.destroy()
        k, site, d = _place_at_threshold(orc, o, case, False, -1)
        assert abs(d) < 2.0 ** -36, "the bisection did not get within the narrow window: %g" % d
        _AT_THRESHOLD["lengths"] = plan.branch_lengths.copy()
    plan.branch_lengths[:] = _AT_THRESHOLD["lengths"]
    monkeypatch.delenv(D.ENV, raising=False)
    p = build_partition(gpu, case, attrs)
    o = oracle_run(orc, gpu, p, case, attrs)
    o.update_partials()
    before = p.scaling_certificate()
    p.update_partials(plan.ops)
    nodes, scalers = written_by(plan.ops)
    clvs, counts = snapshot(p, nodes, scalers)        # before anything else
    after = p.scaling_certificate()
    assert after["raised"] > before["raised"] and after["rerun"] > before["rerun"], (before, after)
    assert after["uncertified"] == 0
    for sc in scalers:
        assert (counts[sc] == o.scalers[sc]).all(), "scaler mirror %d differs from the reference's counts" % sc
    for node in nodes:
        assert bits_equal(clvs[node], o.clv[node]), "CLV mirror %d: not the re-run's values" % node
    p.destroy()


# ---- 10. deferral switched back on by the client

def test_deferral_switched_back_on(gpu, orc, monkeypatch):
    """pll_partition_create switches deferral off on a mirroring partition; a client may switch it on again
    (pll_amd_set_deferral, with unstored pairs and pair folds).  The mirror copy then has to give every deferred
    cherry its bytes first (PLLHIP_DEFERRED_FLUSH in pllhip_mirror_batch): a full traversal, a partial one and a
    second full one, mirrors against the oracle and the twin after each.  (Cherries are deferred by the whole-list
    kernel only: PLLHIP_FUSED=2 also where the dna_path fixture asks for the per-level launches.)"""
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    case = make_case(4, "balanced", 16, 97, seed=4)
    plan, R = case["plan"], case["rate_cats"]
    attrs = ATTRIB_PATTERN_TIP
    p, t = _pair(gpu, case, attrs, monkeypatch)
    assert p.deferred_stats()["ops_deferred"] == 0
    p.set_deferral(True)
    p.set_unstored_pairs(True)
    p.set_pair_fold(True)
    o = oracle_run(orc, gpu, p, case, attrs)
    for x in (p, t, o):
        x.update_partials(plan.ops)
    assert_current(p, t, o, plan.ops, 4, "full traversal:")
    st = p.deferred_stats()
    assert st["ops_deferred"] >= 8 and st["materialised"] >= 8 and st["deferred_now"] == 0, st
    rng = np.random.default_rng(10)
    changed = [1, int(plan.ops[9]["parent_clv_index"])]
    lengths = rng.uniform(0.3, 0.9, len(changed))
    for x in (p, t):
        x.update_prob_matrices([0] * R, changed, lengths)
    for mi, length in zip(changed, lengths):
        o.pmat[mi] = D.oracle_pmatrix(orc, o, length)
    sub = D.ops_above(plan, changed)
    assert 0 < len(sub) < len(plan.ops)
    for x in (p, t, o):
        x.update_partials(sub)
    assert_current(p, t, o, sub, 4, "partial traversal:")
    lengths = rng.uniform(0.02, 0.4, len(plan.matrix_indices))
    for x in (p, t):
        x.update_prob_matrices([0] * R, plan.matrix_indices, lengths)
    for mi, length in zip(plan.matrix_indices, lengths):
        o.pmat[int(mi)] = D.oracle_pmatrix(orc, o, length)
    for x in (p, t, o):
        x.update_partials(plan.ops)
    assert_current(p, t, o, plan.ops, 4, "second full traversal:")
    again = p.deferred_stats()
    assert again["ops_deferred"] > st["ops_deferred"] and again["materialised"] > st["materialised"], (st, again)
    p.destroy()
    t.destroy()


# ---- 11. site repeats and sharded partitions: the per-buffer branch

def _repeats_case(sites):
    case = make_case(4, "random", 12, sites, seed=9)
    repeat_columns(case, 9, 12)
    return case


def _per_buffer_branch(gpu, orc, monkeypatch, case, attrs, shards=None, classes=False):
    plan = case["plan"]
    p, t = _pair(gpu, case, attrs, monkeypatch)
    if shards is not None:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == shards == gpu.lib.pll_amd_shard_count(t.ptr)
    o = oracle_run(orc, gpu, p, case, attrs & ~ATTRIB_SITE_REPEATS)
    gpu.clear_error()
    for x in (p, t, o):
        x.update_partials(plan.ops)
    assert gpu.errno() == 0, gpu.errmsg()
    clvs, _ = assert_current(p, t, o, plan.ops, 4)
    for node in clvs:
        assert clvs[node].shape[0] == case["sites"], "one row per site"
    if classes:
        rows = [p.repeats_classes(int(op["parent_clv_index"])) for op in plan.ops]
        assert sum(1 for r in rows if 0 < r < case["sites"]) > len(plan.ops) // 2, "most nodes are stored by class"
    # a partial traversal behind it
    changed = [int(plan.ops[0]["parent_clv_index"])]
    for x in (p, t):
        x.update_prob_matrices([0] * case["rate_cats"], changed, [0.41])
    o.pmat[changed[0]] = D.oracle_pmatrix(orc, o, 0.41)
    sub = D.ops_above(plan, changed)
    for x in (p, t, o):
        x.update_partials(sub)
    assert gpu.errno() == 0, gpu.errmsg()
    assert_current(p, t, o, sub, 4, "partial traversal:")
    p.destroy()
    t.destroy()


def test_site_repeats(gpu, orc, monkeypatch):
    """PLL_ATTRIB_SITE_REPEATS: CLVs are stored by class on the device, the mirrors show one row per site."""
    _per_buffer_branch(gpu, orc, monkeypatch, _repeats_case(97), ATTRIB_PATTERN_TIP | ATTRIB_SITE_REPEATS, classes=True)


@pytest.mark.parametrize("sites,shards", [(97, 1), (321, 2)])
@pytest.mark.parametrize("repeats", [False, True], ids=["plain", "repeats"])
def test_device_list_on_one_device(gpu, orc, monkeypatch, sites, shards, repeats):
    """PLL_AMD_DEVICES=0,0: ranges are multiples of 256 sites, so 97 sites make a group of ONE range -- which is still a
    group: pll_amd_shard_count says 1, and the batched copy has to reach the range's own context -- and 321 sites two
    ranges (the smallest size that has two), whose mirrors are gathered buffer by buffer."""
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    attrs = ATTRIB_PATTERN_TIP | (ATTRIB_SITE_REPEATS if repeats else 0)
    _per_buffer_branch(gpu, orc, monkeypatch, _repeats_case(sites), attrs, shards=shards, classes=repeats and sites == 97)


def test_site_repeats_over_two_devices(gpu, orc, monkeypatch):
    """the site-repeats case on a partition created with a list of two distinct devices"""
    if gpu.device_count() < 2:
        pytest.skip("one device visible: a list of two distinct devices needs a second one "
                    "(test_device_list_on_one_device runs the same branches with PLL_AMD_DEVICES=0,0)")
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,1")
    _per_buffer_branch(gpu, orc, monkeypatch, _repeats_case(97), ATTRIB_PATTERN_TIP | ATTRIB_SITE_REPEATS)
    _per_buffer_branch(gpu, orc, monkeypatch, _repeats_case(321), ATTRIB_PATTERN_TIP | ATTRIB_SITE_REPEATS, shards=2)
