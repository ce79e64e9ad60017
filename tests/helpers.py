"""Shared builders for the parity tests: one description of a case, applied
identically to a pll-API library (product or reference) and to the oracle."""
import numpy as np

from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, OPS_DTYPE, SCALE_BUFFER_NONE
from oracle_api import OracleRun

TREES = {"balanced": W.balanced_tree, "caterpillar": W.caterpillar_tree, "random": W.random_tree}


def make_case(states=4, shape="balanced", tips=16, sites=200, rate_cats=4, seed=1, alpha=0.7,
              gap_frac=0.05, weights=True, branch=None, ambiguity=True):
    """A tree + alignment + model description (plain data)."""
    plan = TREES[shape](tips, seed=seed, branch=branch)
    rng = np.random.default_rng(seed)
    seqs = None
    if states in (4, 20):
        seqs = W.random_alignment(tips, sites, states, seed=seed + 100, gap_frac=gap_frac)
        if ambiguity:
            extra = b"RYKMSWBDHVN" if states == 4 else b"BZX"
            seqs = [bytearray(s) for s in seqs]
            for s in seqs:
                for pos in rng.integers(0, sites, size=max(1, sites // 25)):
                    s[pos] = extra[rng.integers(0, len(extra))]
            seqs = [bytes(s) for s in seqs]
    pw = rng.integers(1, 4, size=sites).astype(np.uint32) if weights else None
    if states == 4:
        rates, freqs = W.GTR_RATES, W.GTR_FREQS
    else:
        rates = rng.uniform(0.3, 4.0, states * (states - 1) // 2)
        freqs = rng.dirichlet(np.ones(states) * 8)
    return dict(states=states, plan=plan, seqs=seqs, sites=sites, rate_cats=rate_cats,
                alpha=alpha, pw=pw, rates=rates, freqs=freqs, seed=seed, tips=tips, cmap=None)


ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"


def odd_state_case(states, tips=9, sites=30, seed=3, shape="random", observed=None, **kw):
    """Data with 2..32 states (other than 4 and 20) over the alphabet A.. with a
    hand-made character map.  observed: tip characters name only the first `observed`
    states (more than 32 states: what 32-bit character masks can say; the gap is then
    those states)."""
    case = make_case(states, shape, tips, sites, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    n = observed or states
    alphabet = ALPHABET[:n]
    chars = np.frombuffer(alphabet, dtype=np.uint8)
    case["seqs"] = [chars[rng.integers(0, n, sites)].tobytes() for _ in range(tips)]
    cmap = np.zeros(256, dtype=np.uint32)
    for i, ch in enumerate(alphabet):
        cmap[ch] = 1 << i
    cmap[ord("-")] = (1 << n) - 1
    for s in range(0, tips, 3):
        b = bytearray(case["seqs"][s])
        b[s % sites] = ord("-")
        case["seqs"][s] = bytes(b)
    case["cmap"] = cmap
    return case


def many_state_case(states, tips=9, sites=30, seed=3, shape="random", **kw):
    """More than 32 states (61 = codons): the character maps of the API are 32-bit masks,
    so such data enters as tip CLVs; case["tip_index"][tip][site] = state, -1 = gap."""
    case = make_case(states, shape, tips, sites, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, states, size=(tips, sites))
    idx[rng.random((tips, sites)) < 0.03] = -1
    case["tip_index"] = idx
    return case


def constant_columns(case, every=3):
    """Make every `every`-th column one character in every tip, so that invariant[] is populated (tip characters or,
    for more than 32 states, tip state indices)."""
    if case.get("tip_index") is not None:
        case["tip_index"][:, ::every] = case["tip_index"][:1, ::every]
        return
    seqs = [bytearray(s) for s in case["seqs"]]
    for col in range(0, case["sites"], every):
        for s in seqs:
            s[col] = seqs[0][col]
    case["seqs"] = [bytes(s) for s in seqs]


def repeat_columns(case, seed, distinct):
    """Resample the alignment's columns from a pool of `distinct` of them, so that site repeats
    (PLL_ATTRIB_SITE_REPEATS) find few classes per node, like real data."""
    sites = case["sites"]
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, sites, size=distinct)
    pick = pool[rng.integers(0, len(pool), size=sites)]
    case["seqs"] = [bytes(np.frombuffer(s, dtype=np.uint8)[pick]) for s in case["seqs"]]


def index_tip_clvs(case):
    S, R = case["states"], case["rate_cats"]
    idx = case["tip_index"]
    out = (idx[:, :, None] == np.arange(S)[None, None, :]) | (idx[:, :, None] < 0)
    return np.repeat(out[:, :, None, :].astype(np.float64), R, axis=2)


def case_map(lib, case):
    if case["cmap"] is not None:
        return case["cmap"]
    return lib.map("nt" if case["states"] == 4 else "aa")


def params_of(case):
    """params_indices of a case: the mixture's (`mixture`), or one rate matrix for every category"""
    return list(case.get("params_indices") or [0] * case["rate_cats"])


def freqs_of(case):
    """freqs_indices of a case: its own where the mixture names them, its params_indices otherwise"""
    return list(case.get("freqs_indices") or params_of(case))


def case_pinvs(case, pinv=0.0):
    """+I proportion of every rate matrix: the mixture's `pinvs`, or `pinv` for the one matrix"""
    if case.get("models") is None:
        return [float(pinv)]
    assert not pinv, "a mixture case carries its own pinvs"
    return [float(v) for v in (case.get("pinvs") or [0.0] * len(case["models"]))]


def mixture(case, lib, seed, variant=0, pinv=False, params_indices=None):
    """Decorate a case (make_case / odd_state_case / many_state_case) with a model that no kernel gets right by
    accident: M = min(R, 3) rate matrices (2 at R = 1) of which the case's own is number 0, params_indices[k] =
    M - 1 - k % M (never 0 first, never the identity, shared where R > M), category weights that are unequal and sum
    to 1.3, and -- pinv -- distinct +I proportions, one of them 0.  variant 1: freqs_indices that differ from
    params_indices (odd k: the next matrix's; R = 1: matrix 0's).  params_indices: a list to use instead (deep trees
    of random data, where only the fastest category carries weight and ITS entry has to differ from 0 and from k)."""
    S, R = case["states"], case["rate_cats"]
    M = 2 if R == 1 else min(R, 3)
    rng = np.random.default_rng(7000 + seed)
    models = [(case["rates"], case["freqs"])]
    for _ in range(M - 1):
        models.append((rng.uniform(0.3, 4.0, S * (S - 1) // 2), rng.dirichlet(np.ones(S) * 6)))
    case["models"] = models
    case["params_indices"] = list(params_indices or [M - 1 - k % M for k in range(R)])
    assert len(case["params_indices"]) == R and max(case["params_indices"]) == M - 1
    if variant:
        case["freqs_indices"] = ([0] if R == 1 else
                                 [(i + k % 2) % M for k, i in enumerate(case["params_indices"])])
        assert case["freqs_indices"] != case["params_indices"]
    case["cat_weights"] = rng.dirichlet(np.ones(R)) * 1.3
    if pinv:
        case["pinvs"] = [0.0, 0.25] if M == 2 else [0.1, 0.0, 0.3]
    return case


def stale_freqs_defect(case, attrs, edge, plan):
    """Does the genuine reference give a wrong value here?  Its 4-state tip-inner edge kernel (pattern tips) fills a
    lookup table category by category and then, in its site loop, takes the invariant-site term of EVERY category from
    the frequencies pointer the table loop left behind -- the last category's (core_likelihood_avx.c:274 and
    :371).  With one frequency set, or without +I, that is the right pointer; in a mixture with +I it is not."""
    return (case["states"] == 4 and bool(attrs & ATTRIB_PATTERN_TIP) and min(edge[0], edge[2]) < plan.tips
            and len(set(freqs_of(case))) > 1 and max(case.get("pinvs") or [0.0]) > 0)


def undo_stale_freqs_defect(case, model, invariant, per_site):
    """The reference's per-site lnL of an edge under stale_freqs_defect, put right: at an invariant site its likelihood
    is off by sum_k w_k pinv_k (f_last[i] - f_k[i]) -- the last category's frequency of the site's state i in place of
    each category's own -- and nothing else.  model: model_of(the reference partition); for edges without scaling
    (site likelihood = exp(lnl / pattern weight): the caller asserts the counts are 0)."""
    fi, w = freqs_of(case), np.asarray(case["cat_weights"], dtype=np.float64)
    fr, pinvs = model["freqs"], model["pinvs"]
    pw = np.ones(len(per_site)) if case["pw"] is None else np.asarray(case["pw"], dtype=np.float64)
    out = np.array(per_site, dtype=np.float64)
    for n in np.flatnonzero(np.asarray(invariant) >= 0):
        i = int(invariant[n])
        delta = sum(w[k] * pinvs[fi[k]] * (fr[fi[-1]][i] - fr[fi[k]][i]) for k in range(len(fi)))
        out[n] = np.log(np.exp(per_site[n] / pw[n]) - delta) * pw[n]
    return out


def build_partition(lib, case, attrs, pinv=0.0):
    """Create + fill a partition on `lib`; returns it with P-matrices computed."""
    plan, S, R = case["plan"], case["states"], case["rate_cats"]
    if lib.is_amd:
        attrs &= ~0xF
    models = case.get("models") or [(case["rates"], case["freqs"])]
    p = lib.partition_create(plan.tips, plan.clv_buffers, S, case["sites"], len(models), plan.prob_matrices,
                             R, plan.scale_buffers, attrs)
    for i, (rates, freqs) in enumerate(models):
        p.set_frequencies(i, freqs)
        p.set_subst_params(i, rates)
    p.set_category_rates(lib.compute_gamma_cats(case["alpha"], R))
    if case.get("cat_weights") is not None:
        p.set_category_weights(case["cat_weights"])
    if case.get("tip_index") is not None:
        for i, clv in enumerate(index_tip_clvs(case)):
            p.set_tip_clv(i, clv[:, 0, :].reshape(-1))   # [sites][states]; the call replicates over rates
    else:
        cmap = case_map(lib, case)
        for i, s in enumerate(case["seqs"]):
            p.set_tip_states(i, cmap, s)
    if case["pw"] is not None:
        p.set_pattern_weights(case["pw"])
    for i, v in enumerate(case_pinvs(case, pinv)):
        if v > 0:
            p.update_invariant_sites_proportion(i, v)
    p.update_prob_matrices(params_of(case), plan.matrix_indices, plan.branch_lengths)
    return p


def model_of(part, lib, case, pinv=0.0):
    """Model arrays as the partition holds them on the host (eigen system from
    pll_update_eigen, category rates from pll_compute_gamma_cats).  A mixture case (`mixture`): eigen systems,
    frequencies and pinvs are lists with one entry per rate matrix, next to the two index lists and the weights."""
    S, R = case["states"], case["rate_cats"]
    if case.get("models") is not None:
        eig = [part.get_eigen(i) for i in range(len(case["models"]))]
        fr = [np.ctypeslib.as_array(part.s.frequencies[i], shape=(part.s.states_padded,)).copy()[:S]
              for i in range(len(case["models"]))]
        # (the case's own weights, not what the partition under test stored of them: the library does not touch them)
        w = np.full(R, 1.0 / R) if case.get("cat_weights") is None else np.array(case["cat_weights"], dtype=np.float64)
        return dict(states=S, rate_cats=R, rates=lib.compute_gamma_cats(case["alpha"], R), rate_weights=w,
                    eigenvals=[e[0] for e in eig], eigenvecs=[e[1] for e in eig], inv_eigenvecs=[e[2] for e in eig],
                    freqs=fr, pinvs=case_pinvs(case), params_indices=params_of(case), freqs_indices=freqs_of(case))
    vals, vecs, inv = part.get_eigen(0)
    fr = np.ctypeslib.as_array(part.s.frequencies[0], shape=(part.s.states_padded,)).copy()[:S]
    return dict(states=S, rate_cats=R, rates=lib.compute_gamma_cats(case["alpha"], R),
                rate_weights=np.full(R, 1.0 / R), eigenvals=vals, eigenvecs=vecs,
                inv_eigenvecs=inv, freqs=fr, pinv=pinv)


def encode_tips(part):
    """(tipcodes[tips][sites] uint8, tipmap) as the partition encoded them."""
    s = part.s
    codes = np.stack([np.ctypeslib.as_array(s.tipchars[i], shape=(s.sites,)).copy()
                      for i in range(s.tips)])
    tipmap = np.ctypeslib.as_array(s.tipmap, shape=(256,)).copy()
    return codes, tipmap


def tip_clvs(case, cmap):
    """0/1 tip CLVs [tips][sites][R][S] from the character map (pll.c:905-939)."""
    S, R = case["states"], case["rate_cats"]
    out = np.zeros((case["tips"], case["sites"], R, S))
    for i, seq in enumerate(case["seqs"]):
        masks = cmap[np.frombuffer(seq, dtype=np.uint8)]
        bits = (masks[:, None] >> np.arange(S)[None, :]) & 1
        out[i] = bits[:, None, :].astype(np.float64)
    return out


def invariant_of(part):
    s = part.s
    if not s.invariant:
        return None
    return np.ctypeslib.as_array(s.invariant, shape=(s.sites,)).copy()


def oracle_run(orc, lib, part, case, attrs, pinv=0.0, override=None):
    """override: entries of the model to replace (`model_variants`)"""
    model = model_of(part, lib, case, pinv)
    model.update(override or {})
    inv = invariant_of(part) if max(case_pinvs(case, pinv)) > 0 else None
    if attrs & ATTRIB_PATTERN_TIP:
        codes, tipmap = encode_tips(part)
        return OracleRun(orc, model, case["plan"], attrs, tipcodes=codes, tipmap=tipmap,
                         pattern_weights=case["pw"], invariant=inv)
    if case.get("tip_index") is not None:
        return OracleRun(orc, model, case["plan"], attrs, tipclvs=index_tip_clvs(case),
                         pattern_weights=case["pw"], invariant=inv)
    return OracleRun(orc, model, case["plan"], attrs, tipclvs=tip_clvs(case, case_map(lib, case)),
                     pattern_weights=case["pw"], invariant=inv)


def model_variants(model):
    """{name: entries to replace} -- the mistakes a kernel could make with a mixture's per-category inputs, as
    changes to the ORACLE's model (oracle_run(..., override=)): the mean weight for every category, 1 / R for every
    category, the identity for the indices (modulo the number of rate matrices), index 0 for every category, the
    first matrix's +I proportion for every matrix.  Only those that change the model at all."""
    R, M = model["rate_cats"], len(model["eigenvals"])
    pi, fi, w = list(model["params_indices"]), list(model["freqs_indices"]), np.asarray(model["rate_weights"])
    pinvs = list(model.get("pinvs") or [0.0] * M)
    out = {}
    if not np.allclose(w, w.mean(), rtol=1e-3):
        out["mean-weight"] = dict(rate_weights=np.full(R, w.mean()))
    if not np.allclose(w, 1.0 / R, rtol=1e-3):
        out["weights-1/R"] = dict(rate_weights=np.full(R, 1.0 / R))
    ident = [k % M for k in range(R)]
    for name, idx in (("identity", ident), ("all-zero", [0] * R)):
        if idx != pi or idx != fi:
            out["indices-" + name] = dict(params_indices=idx, freqs_indices=idx)
    if any(v != pinvs[0] for v in pinvs):
        out["pinvs[0]"] = dict(pinvs=[pinvs[0]] * M)
    return out


def assert_discriminates(orc, lib, part, case, attrs, edge=None, floor=1e-6):
    """On the oracle alone: every mistake of model_variants moves the edge lnL of this mixture case by more than
    `floor` relative -- nine orders of magnitude above the bounds the product is held to -- so a kernel that made it
    would fail.  The weights and indices variants must exist wherever the shape allows them (R > 1)."""
    edge = tuple(edge or case["plan"].root_edge)
    base = oracle_run(orc, lib, part, case, attrs)
    base.update_partials()
    want = base.edge_loglikelihood(*edge)
    variants = model_variants(base.m)
    need = {"weights-1/R", "indices-all-zero"}
    if case["rate_cats"] > 1:
        need |= {"mean-weight", "indices-identity"}
    if case.get("pinvs"):
        need.add("pinvs[0]")
        assert base.invariant is not None and (base.invariant >= 0).any(), "no invariant site in the fixture"
    assert need <= set(variants), "fixture is degenerate: %s" % sorted(need - set(variants))
    for name, change in variants.items():
        o = oracle_run(orc, lib, part, case, attrs, override=change)
        o.update_partials()
        got = o.edge_loglikelihood(*edge)
        assert abs(got - want) > floor * abs(want), "fixture does not tell %s apart: %r %r" % (name, got, want)
    return base


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def clvs_bitwise(states):
    """Does the configuration the environment selects promise every CLV bit for bit?  Not 20 states on the default
    path: PLLHIP_AA_TI_MFMA (default on) runs tip-inner mat-vecs of the whole-list kernel on the matrix cores."""
    import os
    return not (states == 20 and os.environ.get("PLLHIP_AA_TI_MFMA", "1") != "0" and
                os.environ.get("PLLHIP_AA_EXACT", "0") != "1")


def clv_err(a, b):
    """Largest difference of two CLVs [sites][rates][states], entry by entry, relative to the entry -- or to 1e-150 x
    the site's largest entry, if that is more.  The floor is for entries that were DENORMAL on the way (a block whose
    largest entry is kept above 2^-256 by the scaling can hold entries 200 orders of magnitude below it): they were
    rounded to a multiple of 2^-1074 there, so two summation orders that differ in the last bit of a normal number
    differ by 1e-12 relative in such an entry (seen: 6.4e-235 in a block with 2.4e-67 -- exactly 2^-1074 x 2^256
    apart).  Such entries weigh nothing in any likelihood."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if not a.size:
        return 0.0
    floor = 1e-150 * np.abs(b).reshape(b.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (b.ndim - 1))
    return float(np.max(np.abs(a - b) / np.maximum(np.maximum(np.abs(b), floor), 1e-300)))


def clv_ok(a, b, exact=True, tol=1e-12):
    """A CLV against the oracle's / the reference's: bit for bit, or -- 20 states on the default path, where the
    whole-list kernel runs the mat-vec of tip-inner ops on the matrix cores (round 6) -- to rounding, entry by entry
    (clv_err; ~6e-16 per op of depth measured on a 300-tip ladder: 1e-13 for the trees of the BASELINE configs, which
    tests/test_gpu_baseline_configs.py asks for, 1e-12 by default -- 400-tip ladders).
    (Scaler counts are compared bit for bit either way: the scaling certificate, tests/test_gpu_cert.py.)"""
    return bits_equal(a, b) if exact else clv_err(a, b) <= tol


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def sumtable_err(a, b):
    """max |a-b| relative to the largest entry of the same (site, rate) block:
    entries that are analytically zero (gap columns) carry only rounding noise."""
    scale = np.abs(b).max(axis=2, keepdims=True) + 1e-300
    return float(np.max(np.abs(a - b) / scale))


def derivative_magnitudes(model, sumtable, t, pattern_weights=None, invariant=None):
    """(sum_n w_n |L'/L|, sum_n w_n ((L'/L)^2 + |L''/L|)) from a sumtable [sites][R][S], in double: the size of the
    site terms that pll_compute_likelihood_derivatives adds up (d_f = sum_n w_n (-L'/L), dd_f = sum_n w_n ((L'/L)^2 -
    L''/L)).  The scale to judge a total by where its terms cancel: at a long branch (t = 50) every site's L'/L is
    what is left of the eigenvalues that are zero in exact arithmetic, and (L'/L)^2 and L''/L agree to the last
    bits -- a total near zero, against which rounding of the terms would look large."""
    S, R = model["states"], model["rate_cats"]
    if model.get("params_indices") is None:
        pinv = np.full(R, float(model.get("pinv", 0.0)))
        vals = np.repeat(np.asarray(model["eigenvals"])[None, :], R, axis=0)
        fr = np.repeat(np.asarray(model["freqs"])[None, :], R, axis=0)
    else:   # a mixture: category k has the eigenvalues, frequencies and pinv of rate matrix params_indices[k]
        pi = list(model["params_indices"])
        pinv = np.asarray(model.get("pinvs") or [0.0] * len(model["eigenvals"]), dtype=np.float64)[pi]
        vals = np.asarray(model["eigenvals"])[pi]
        fr = np.asarray(model["freqs"])[pi]
    x = vals * (np.asarray(model["rates"]) / (1.0 - pinv))[:, None]
    e = np.exp(x * t)
    st = np.asarray(sumtable, dtype=np.float64).reshape(-1, R, S)
    w = np.asarray(model["rate_weights"])
    lk = [(st * (e * x ** i)[None]).sum(axis=2) for i in range(3)]
    if pinv.max() > 0:
        inv = np.full(st.shape[0], -1) if invariant is None else np.asarray(invariant)
        inv_lk = np.where((inv >= 0)[:, None], fr[:, np.maximum(inv, 0)].T, 0.0) * pinv[None, :]
        lk = [lk[0] * (1 - pinv)[None, :] + inv_lk, lk[1] * (1 - pinv)[None, :], lk[2] * (1 - pinv)[None, :]]
    L0, L1, L2 = [(v * w[None, :]).sum(axis=1) for v in lk]
    pw = np.ones(st.shape[0]) if pattern_weights is None else np.asarray(pattern_weights, dtype=np.float64)
    d1, d2 = L1 / L0, L2 / L0
    return float((np.abs(d1) * pw).sum()), float(((d1 * d1 + np.abs(d2)) * pw).sum())


def deriv_errs(got, want, t, mags):
    """errors of (d_f, dd_f) against `want`: relative to the totals, and at t >= 50 relative to the magnitudes of
    their terms instead (`mags`, derivative_magnitudes or ExactRun.derivatives): there the totals are sums of terms
    that cancel to near zero"""
    out = []
    for g, w_, m in zip(got, want, mags):
        scale = float(m) if t >= 50 else abs(float(w_))
        out.append(abs(float(g) - float(w_)) / max(scale, 1e-300))
    return max(out)


def random_op_sequence(rng, tips, inner, scalers, matrices, length):
    """A valid-but-arbitrary op sequence over `inner` CLV slots: every op reads
    tips or slots written earlier and writes any slot other than its children.
    Produces every kind of dependency between neighbouring ops (read-after-write,
    write-after-read, write-after-write, shared scaler slots)."""
    ops = np.zeros(length, dtype=OPS_DTYPE)
    written = {}                      # inner CLV slot -> scaler slot that goes with it (or NONE)
    recent = []
    for i in range(length):
        pool = list(range(tips)) + sorted(written)

        def child():
            # mostly recent results, so that deep chains (and scaling events) build up
            if recent and rng.random() < 0.7:
                c = int(recent[rng.integers(0, len(recent))])
            else:
                c = int(pool[rng.integers(0, len(pool))])
            return c, (written[c] if c >= tips else SCALE_BUFFER_NONE)
        (a, sa), (b, sb) = child(), child()
        free = [s for s in range(tips, tips + inner) if s not in (a, b)]
        # bias towards a few slots so that reuse is frequent
        parent = int(free[min(int(rng.exponential(3.0)), len(free) - 1)])
        psc = int(rng.integers(0, scalers)) if rng.random() < 0.8 else SCALE_BUFFER_NONE
        # the reference adds child counts into the parent's buffer: a parent sharing its
        # scaler slot with one of its children would read what it is overwriting
        if psc in (sa, sb):
            psc = SCALE_BUFFER_NONE
        ops[i] = (parent, psc, a, int(rng.integers(0, matrices)), sa, b, int(rng.integers(0, matrices)), sb)
        # any other CLV that used this scaler slot loses it
        for k in list(written):
            if psc != SCALE_BUFFER_NONE and written[k] == psc:
                written[k] = SCALE_BUFFER_NONE
        written[parent] = psc
        recent = ([parent] + [r for r in recent if r != parent])[:3]
    return ops


def random_sequence_case(seed, states=None, rate_cats=4):
    """(case, attributes, ops, rng) for the random-op-sequence tests: 4- and 20-state
    data (or the state count given), with and without PATTERN_TIP, per-site and per-rate
    scalers."""
    rng = np.random.default_rng(1000 + seed)
    attrs = (ATTRIB_PATTERN_TIP if seed % 2 else 0) | (ATTRIB_RATE_SCALERS if seed % 4 >= 2 else 0)
    tips = 12
    sites = 97 + 64 * (seed % 4)
    if states is None:
        states = 4 if seed % 3 else 20
        case = make_case(states, "random", tips, sites, seed=seed + 50)
    elif states > 32:
        attrs &= ~ATTRIB_PATTERN_TIP
        case = many_state_case(states, tips=tips, sites=sites, seed=seed + 50, rate_cats=rate_cats)
    else:
        case = odd_state_case(states, tips=tips, sites=sites, seed=seed + 50, rate_cats=rate_cats)
    plan = case["plan"]
    ops = random_op_sequence(rng, tips, plan.clv_buffers, plan.scale_buffers, plan.prob_matrices - 1,
                             120)
    # every matrix slot gets its own branch length
    plan.matrix_indices = np.arange(plan.prob_matrices - 1, dtype=np.uint32)
    plan.branch_lengths = rng.uniform(0.01, 0.5, len(plan.matrix_indices))
    return case, attrs, ops, rng
