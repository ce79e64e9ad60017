"""The definition of pll_amd_site_posteriors (include/pll_amd.h), restated in numpy (TEST INFRASTRUCTURE).

`definition` runs on arrays read from a partition of either library (get_clv, get_scaler, get_pmatrix, the tip
characters and the model arrays of the partition struct).  It is ONE loop nest over categories i, states j and child
states k in the reference's order (core_likelihood.c:914-996, :348-403); numpy only carries the site axis along, so
every site sees exactly the scalar sequence of operations written here and no sum is reordered.

    termb[i][j] = sum_k P_i[j][k] clvc[i][k]                 (a pattern tip: the sum over its mask's set bits)
    x[i][j]     = ((clvp[i][j] * f_i[j] * termb[i][j]) * m_i) * (w_i * (1 - p_i))
    v[i]        = (w_i * p_i) * f_i[invariant[n]]
    terma       = sum_i (sum_j x[i][j] + v[i])

`asks` lists every edge of an insertion_data tree in both directions where the parent has a CLV.
"""
import types

import numpy as np

from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, OPS_DTYPE

SCALE_RATE_MAXDIFF = 4          # PLL_SCALE_RATE_MAXDIFF, pll.h
LOG_THRESHOLD = np.log(2.0 ** -256)   # log(PLL_SCALE_THRESHOLD)


def asks(case):
    """(parent clv, parent scaler, child clv, child scaler, matrix) for both directions of every edge; a pattern tip
    is never the parent"""
    out = []
    for e, (a, b, _) in enumerate(case.edges):
        for x, y in ((a, b), (b, a)):
            if case.pattern_tip and x < case.n:
                continue
            pc, ps = case.side(x, y)
            cc, cs = case.side(y, x)
            out.append((pc, ps, cc, cs, e))
    return out


def constant_columns(case, every=6):
    """every `every`-th column shows one unambiguous state in every tip (random columns never do, and +I would have
    nothing to act on); character data only; returns the columns"""
    alphabet = {4: b"ACGT", 20: b"ARNDCQEGHILKMFPSTWYV"}.get(case.states, b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef")
    cols = list(range(0, case.sites, every))
    seqs = [bytearray(s) for s in case.seqs]
    for col in cols:
        for s in seqs:
            s[col] = alphabet[(col // every) % case.states]
    case.seqs = [bytes(s) for s in seqs]
    return cols


def _model(p, fi):
    s = p.s
    R, S = s.rate_cats, s.states
    w = np.ctypeslib.as_array(s.rate_weights, shape=(R,)).copy()
    rates = np.ctypeslib.as_array(s.rates, shape=(R,)).copy()
    pinv = np.array([s.prop_invar[int(k)] for k in fi])
    freqs = [np.ctypeslib.as_array(s.frequencies[int(k)], shape=(s.states_padded,)).copy()[:S] for k in fi]
    inv = np.ctypeslib.as_array(s.invariant, shape=(s.sites,)).copy() if s.invariant else None
    return w, rates, pinv, freqs, inv


def definition(p, ask, freqs_indices):
    """dict: state_probs [sites][S], best_state, best_prob, rate_probs [sites][R + 1], site_rates, terma [sites] and
    persite_lnl [sites] (log(terma) + the scaler term, times the pattern weight)"""
    pc, ps, cc, cs, m = ask
    s = p.s
    S, R, sites = s.states, s.rate_cats, s.sites
    tip = bool(s.attributes & ATTRIB_PATTERN_TIP) and cc < s.tips
    w, rates, pinv, freqs, inv = _model(p, freqs_indices)
    clvp = p.get_clv(pc)[:sites]
    P = p.get_pmatrix(m)
    if tip:
        codes = np.ctypeslib.as_array(s.tipchars[cc], shape=(sites,)).copy().astype(np.uint32)
        mask = codes if S == 4 else np.ctypeslib.as_array(s.tipmap, shape=(256,)).copy()[codes]
    else:
        clvc = p.get_clv(cc)[:sites]

    # scaler counts: per rate brought to the site's smallest count, or one count per site
    rel = np.zeros((sites, R), dtype=np.int64)
    if s.attributes & ATTRIB_RATE_SCALERS:
        cnt = np.zeros((sites, R), dtype=np.int64)
        if ps >= 0:
            cnt += p.get_scaler(ps).reshape(-1, R)[:sites]
        if not tip and cs >= 0:
            cnt += p.get_scaler(cs).reshape(-1, R)[:sites]
        site_scalings = cnt.min(axis=1)
        rel = np.minimum(cnt - site_scalings[:, None], SCALE_RATE_MAXDIFF)
    else:
        site_scalings = np.zeros(sites, dtype=np.int64)
        if ps >= 0:
            site_scalings += p.get_scaler(ps)[:sites]
        if not tip and cs >= 0:
            site_scalings += p.get_scaler(cs)[:sites]

    x = np.zeros((R, S, sites))
    v = np.zeros((R, sites))
    with np.errstate(under="ignore"):
        for i in range(R):
            f = freqs[i]
            c = w[i] * (1.0 - pinv[i])
            m_i = np.ldexp(1.0, -256 * rel[:, i])
            for j in range(S):
                termb = np.zeros(sites)
                for k in range(S):
                    if tip:
                        termb = np.where((mask >> k) & 1 == 1, termb + P[i, j, k], termb)
                    else:
                        termb = termb + P[i, j, k] * clvc[:, i, k]
                t = clvp[:, i, j] * f[j] * termb
                t = np.where(rel[:, i] > 0, t * m_i, t)
                x[i, j] = t * c
            if pinv[i] > 0 and inv is not None:
                v[i] = np.where(inv >= 0, (w[i] * pinv[i]) * f[np.maximum(inv, 0)], 0.0)

        terma = np.zeros(sites)
        vsum = np.zeros(sites)
        rsum = np.zeros((R, sites))
        for i in range(R):
            for j in range(S):
                rsum[i] = rsum[i] + x[i, j]
            vsum = vsum + v[i]
            terma = terma + (rsum[i] + v[i])

        state_probs = np.zeros((sites, S))
        for j in range(S):
            acc = np.zeros(sites)
            for i in range(R):
                acc = acc + x[i, j]
            if inv is not None:
                acc = np.where(inv == j, acc + vsum, acc)
            state_probs[:, j] = acc / terma
        rate_probs = np.zeros((sites, R + 1))
        site_rates = np.zeros(sites)
        for i in range(R):
            rate_probs[:, i] = rsum[i] / terma
            r_i = rates[i] / (1.0 - pinv[i]) if pinv[i] > 0 else rates[i]
            site_rates = site_rates + rate_probs[:, i] * r_i
        rate_probs[:, R] = vsum / terma

    best_state = np.argmax(state_probs, axis=1)
    pw = np.ctypeslib.as_array(s.pattern_weights, shape=(sites,)).copy()
    persite = (np.log(terma) + site_scalings * LOG_THRESHOLD) * pw
    return dict(state_probs=state_probs, best_state=best_state.astype(np.uint8),
                best_prob=state_probs[np.arange(sites), best_state], rate_probs=rate_probs, site_rates=site_rates,
                terma=terma, persite_lnl=persite, rel=rel)


def exact_run(lib, p, case):
    """exact_pruning.ExactRun over an insertion_data case (one rate matrix, no scaling): every directed CLV in
    longdouble.  The P-matrices are the partition's own, raised to longdouble: the P-matrix of an edge is an INPUT of
    the definition ("whatever the partition holds under matrix_index"), so the exact value of the defined quantity is
    the one for that matrix.  ExactRun's own matrices -- longdouble exponentials over an eigensystem that is itself
    only double -- differ from the partition's by about 1e-16 absolute, which is 1e-13 relative in the off-diagonal
    entries of the slowest Gamma category on a short branch; a site's share of that category is a product of several
    such entries (measured with them: rate_probs off by up to 1.6e-12 relative, state_probs by 1.4e-13)."""
    from exact_pruning import ExactRun, LD

    class _Run(ExactRun):
        def __init__(self, pmats, *a, **kw):
            self._pmats = pmats
            super().__init__(*a, **kw)

        def pmatrix(self, t, order=0):
            assert order == 0
            return self._pmats[float(t)]
    from helpers import tip_clvs
    S, R = case.states, case.rate_cats
    vals, vecs, ivecs = p.get_eigen(0)
    fr = np.ctypeslib.as_array(p.s.frequencies[0], shape=(p.s.states_padded,)).copy()[:S]
    model = dict(states=S, rate_cats=R, rates=np.ctypeslib.as_array(p.s.rates, shape=(R,)).copy(),
                 rate_weights=np.ctypeslib.as_array(p.s.rate_weights, shape=(R,)).copy(), eigenvals=vals,
                 eigenvecs=vecs, inv_eigenvecs=ivecs, freqs=fr, pinv=case.pinv)
    cmap = case.cmap if case.cmap is not None else lib.map("nt" if S == 4 else "aa")
    tips = tip_clvs(dict(states=S, rate_cats=R, tips=case.ntips, sites=case.sites, seqs=case.seqs), cmap)
    plan = types.SimpleNamespace(matrix_indices=list(range(len(case.lengths))), branch_lengths=case.lengths)
    ops = np.zeros(len(case.ops), dtype=OPS_DTYPE)
    for i, op in enumerate(case.ops):
        ops[i] = op
    inv = np.ctypeslib.as_array(p.s.invariant, shape=(p.s.sites,)).copy() if (case.pinv > 0 and p.s.invariant) else None
    pmats = {float(t): p.get_pmatrix(m).astype(LD) for m, t in enumerate(case.lengths)}
    run = _Run(pmats, model, plan, tips, pattern_weights=case.pw, invariant=inv, ops=ops)
    run.invariant_index = np.full(case.sites, -1) if inv is None else inv
    return run


def exact_posteriors(run, ask):
    """(state_probs [sites][S], rate_probs [sites][R + 1]) in longdouble from an ExactRun: _edge_terms before its sum
    over the states"""
    LD = np.longdouble
    pc, _, cc, _, m = ask
    t = run.branch[m]
    pcv = np.einsum("kij,nkj->nki", run.pmatrix(t, 0), run.clv[cc])
    q = LD(1) - LD(run.pinv)
    x = run.clv[pc] * pcv * run.freqs[None, None, :] * (run.w * q)[None, :, None]    # [sites][R][S]
    v = run.inv_lk[:, None] * (run.w * LD(run.pinv))[None, :]                          # [sites][R]
    terma = x.sum(axis=(1, 2)) + v.sum(axis=1)
    sp = x.sum(axis=1)
    for n, j in enumerate(run.invariant_index):
        if j >= 0:
            sp[n, j] += v[n].sum()
    rp = np.concatenate([x.sum(axis=2), v.sum(axis=1)[:, None]], axis=1)
    return sp / terma[:, None], rp / terma[:, None]
