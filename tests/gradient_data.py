"""Helpers of the directed-list and branch-derivative tests (tests/test_directed_host.py,
tests/test_gpu_branch_derivatives.py, tests/test_gpu_tree_gradient.py).

* random trees as pll_utree_t: pll_amd_tree_from_joins over random valid join lists;
* the site loop of the reference's core_derivatives.c restated in numpy over a host sumtable: per site L, L', L'' and
  the sums of the absolute values of their terms, from which the closeness rule of the derivative tests is made.

The closeness rule.  d_f = sum_n w_n (-L'/L) and dd_f = sum_n w_n ((L'/L)^2 - L''/L); L, L', L'' are sums of terms
c_i, c_i mu_i, c_i mu_i^2 (c_i: weight x (1 - pinv) x table entry x exponential, or the invariant term with mu = 0;
mu_i: the eigenvalue times rate / (1 - pinv)).  A relative error eps in every c_i moves L by at most eps |L|_a with
|L|_a = sum |c_i|, and likewise L' and L''; to first order that moves

    d_f   by  eps E_f,  E_f = sum_n w_n (|L'|_a / |L| + |L'| |L|_a / L^2)
    dd_f  by  eps E_g,  E_g = sum_n w_n (2 |L'/L| (|L'|_a / |L| + |L'| |L|_a / L^2) + |L''|_a / |L| + |L''| |L|_a / L^2)

and a result passes if |got - want| <= K 2^-53 E with K = 1024 (4 states) or 8192 (more): a few hundred roundings per
site term on each side (two mat-vecs, the product, exp of a rounded argument).  K is reasoned, not measured.
"""
import ctypes as C

import numpy as np

from libpll_amd.pllapi import JOIN_DTYPE, JOIN_LAST_DTYPE, UNode

U = 2.0 ** -53


def K_of(states):
    return 1024.0 if states == 4 else 8192.0


# ---- trees


def random_joins(n, seed, caterpillar=False, low=0.05, high=0.4):
    """a random valid join list of n >= 3 tips: (joins [n - 3], last) as pll_amd_tree_from_joins takes them"""
    rng = np.random.default_rng(seed)
    joins = np.zeros(n - 3, dtype=JOIN_DTYPE)
    active = list(range(n))
    for s in range(n - 3):
        if caterpillar:
            a, b = (0, 1) if s == 0 else (n + s - 1, s + 1)
        else:
            a, b = (int(x) for x in rng.choice(active, 2, replace=False))
        active.remove(a)
        active.remove(b)
        active.append(n + s)
        joins[s] = (a, b, rng.uniform(low, high), rng.uniform(low, high))
    last = np.zeros(1, dtype=JOIN_LAST_DTYPE)
    last[0]["node"] = sorted(active)
    last[0]["length"] = rng.uniform(low, high, 3)
    return joins, last


def random_tree(lib, n, seed, caterpillar=False):
    """the pointer to a pll_utree_t (free it with lib.lib.pll_utree_destroy(tree, None))"""
    joins, last = random_joins(n, seed, caterpillar)
    return lib.tree_from_joins(joins, last, n)


def members(tree):
    """every ring member of the tree by slot: (node objects [3 (n - 2)], tips [n])"""
    t = tree.contents
    n = t.tip_count
    slots = []
    for i in range(n - 2):
        x = t.nodes[n + i].contents
        slots += [x, x.next.contents, x.next.contents.next.contents]
    return slots, [t.nodes[i].contents for i in range(n)]


def addr(node):
    return C.addressof(node)


def tree_bytes(tree):
    """every byte of the tree's structs: the tree itself, its node table and all its nodes"""
    t = tree.contents
    total = t.tip_count + t.inner_count
    slots, tips = members(tree)
    out = [C.string_at(C.addressof(t), C.sizeof(t)), C.string_at(t.nodes, total * C.sizeof(C.c_void_p))]
    out += [C.string_at(addr(x), C.sizeof(UNode)) for x in tips + slots]
    return b"".join(out)


# ---- the site loop of core_derivatives.c in numpy


def model_of(p, params):
    """what the site loop reads of the partition's model, per rate category: eigenvalues, rates, weights, +I
    proportions, frequencies; the invariant index per site (or None), the pattern weights"""
    S, R, sites = p.s.states, p.s.rate_cats, p.s.sites
    ev = np.array([p.get_eigen(params[k])[0] for k in range(R)])
    rates = np.array([p.s.rates[k] for k in range(R)])
    weights = np.array([p.s.rate_weights[k] for k in range(R)])
    pinv = np.array([p.s.prop_invar[params[k]] for k in range(R)])
    freqs = np.array([[p.s.frequencies[params[k]][j] for j in range(S)] for k in range(R)])
    inv = np.array([p.s.invariant[i] for i in range(sites)]) if p.s.invariant else None
    pw = np.array([p.s.pattern_weights[i] for i in range(sites)], dtype=np.float64)
    return dict(ev=ev, rates=rates, weights=weights, pinv=pinv, freqs=freqs, inv=inv, pw=pw)


def site_terms(table, m, t):
    """table [sites][R][S] (a host sumtable); m: model_of(); returns per site (L, L1, L2, aL, aL1, aL2)"""
    sites, R, S = table.shape
    ki = m["rates"] / (1.0 - m["pinv"])                       # [R]
    mu = m["ev"] * ki[:, None]                                # [R][S]
    scale = (m["weights"] * (1.0 - m["pinv"]))[:, None]       # [R][1]
    c = table * (np.exp(mu * t) * scale)[None, :, :]          # [sites][R][S]
    L = c.sum(axis=(1, 2))
    L1 = (c * mu).sum(axis=(1, 2))
    L2 = (c * mu * mu).sum(axis=(1, 2))
    aL = np.abs(c).sum(axis=(1, 2))
    aL1 = np.abs(c * mu).sum(axis=(1, 2))
    aL2 = (np.abs(c) * mu * mu).sum(axis=(1, 2))
    if m["inv"] is not None and (m["pinv"] > 0).any():
        for k in range(R):
            if m["pinv"][k] > 0:
                has = m["inv"] >= 0
                term = np.where(has, m["freqs"][k][np.where(has, m["inv"], 0)], 0.0) * m["pinv"][k] * m["weights"][k]
                L = L + term          # (mu = 0: nothing for L', L'')
                aL = aL + np.abs(term)
    return L, L1, L2, aL, aL1, aL2


def derivatives_numpy(table, m, t):
    """(d_f, dd_f) by the restated loop: a check of the restatement itself against the single call"""
    L, L1, L2, _, _, _ = site_terms(table, m, t)
    d1 = -L1 / L
    return float((m["pw"] * d1).sum()), float((m["pw"] * (d1 * d1 - L2 / L)).sum())


def error_scales(table, m, t):
    """(E_f, E_g) of the module docstring"""
    L, L1, L2, aL, aL1, aL2 = site_terms(table, m, t)
    with np.errstate(all="ignore"):
        first = aL1 / np.abs(L) + np.abs(L1) * aL / (L * L)
        E_f = float((m["pw"] * first).sum())
        E_g = float((m["pw"] * (2.0 * np.abs(L1 / L) * first + aL2 / np.abs(L) + np.abs(L2) * aL / (L * L))).sum())
    return E_f, E_g


def branch_yardstick(p, params, branch, sumtable, lengths, model=None):
    """the single calls on partition p for one branch at each of `lengths`, and the error scales from its host table:
    a list of ((d_f, dd_f), (E_f, E_g))"""
    pc, ps, cc, cs = (int(x) for x in branch)
    p.update_sumtable(pc, cc, ps, cs, params, sumtable)
    table = np.asarray(p.get_sumtable(sumtable), dtype=np.float64)[:p.s.sites]
    model = model or model_of(p, params)
    return [(p.compute_likelihood_derivatives(ps, cs, float(t), params, sumtable), error_scales(table, model, float(t)))
            for t in lengths]


def assert_close(got, want, E, states, what, record=None):
    """the closeness rule; record: a list that receives |delta| / (2^-53 E) of both values"""
    K = K_of(states)
    for name, g, w, e in (("d_f", got[0], want[0], E[0]), ("dd_f", got[1], want[1], E[1])):
        assert np.isfinite(g) and np.isfinite(w) and np.isfinite(e), (what, name, g, w, e)
        ratio = abs(g - w) / (U * e) if e > 0 else (0.0 if g == w else np.inf)
        if record is not None:
            record.append(ratio)
        assert ratio <= K, (what, name, g, w, ratio, K)
