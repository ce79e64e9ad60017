"""Felsenstein pruning in extended precision with no scaling at all (TEST INFRASTRUCTURE).

An independent check of what the oracle and the product compute: the oracle restates the reference operation by
operation in double precision and follows the same scaling rules, so it cannot tell whether those rules give back the
true likelihood.  This module computes the true value instead.  Every CLV, P-matrix and sum is in numpy's longdouble
(x87 80-bit: a 64-bit mantissa and an exponent down to 1e-4932), which holds a 700-tip caterpillar's CLVs without
rescaling them.

P-matrices come from the partition's own eigensystem (helpers.model_of), raised to longdouble:
P_k(t) = IV diag(exp(lambda r_k' t)) EV with r_k' = r_k / (1 - pinv), the orientation of the reference's
pll_core_update_pmatrix (P[j][k] = sum_m IV[j][m] e_m EV[m][k]).  The derivatives are those of -lnL with respect to
the branch length, the reference's convention (d_f = sum_n w_n (-L'/L), dd_f = sum_n w_n ((L'/L)^2 - L''/L)), from
the analytic dP/dt and d2P/dt2.
"""
import numpy as np

from libpll_amd.pllapi import OPS_DTYPE

LD = np.longdouble
# the 80-bit format (or better): a helper that silently fell back to double would judge nothing
assert np.finfo(LD).nmant >= 63, "numpy's longdouble is not the 80-bit format on this machine"


class ExactRun:
    """model: helpers.model_of(...) -- one rate matrix, or a mixture (per-matrix lists and params_indices /
    freqs_indices as oracle_api.OracleRun takes them: P-matrices and derivatives through params_indices, the
    frequencies and +I proportions of the lnL through freqs_indices); plan: the tree (ops, matrix indices,
    branch lengths); tipclvs: float64 [tips][sites][R][S] 0/1 tip vectors (helpers.tip_clvs / index_tip_clvs);
    invariant: int [sites] (-1 = variable) or None."""

    def __init__(self, model, plan, tipclvs, pattern_weights=None, invariant=None, ops=None):
        self.S, self.R = int(model["states"]), int(model["rate_cats"])
        R = self.R

        def ld(x):
            return np.asarray(x, dtype=np.float64).astype(LD)
        if model.get("params_indices") is None:
            self.pinv = float(model.get("pinv", 0.0))
            self.lam, self.ev, self.iv = ld(model["eigenvals"]), ld(model["eigenvecs"]), ld(model["inv_eigenvecs"])
            self.freqs = ld(model["freqs"])
            pi = fi = [0] * R
            lam, ev, iv, fr, pinvs = [self.lam], [self.ev], [self.iv], [self.freqs], [self.pinv]
        else:
            pi = [int(i) for i in model["params_indices"]]
            fi = [int(i) for i in (model.get("freqs_indices") or pi)]
            lam, ev, iv, fr = ([ld(a) for a in model[k]] for k in ("eigenvals", "eigenvecs", "inv_eigenvecs", "freqs"))
            pinvs = list(model.get("pinvs") or [0.0] * len(lam))
        # per category: [R][S], [R][S][S], [R][S][S]; frequencies and +I proportions for the lnL (freqs_indices) and
        # for the derivatives (params_indices)
        self._lam, self._ev, self._iv = (np.stack([a[i] for i in pi]) for a in (lam, ev, iv))
        self._fr, self._fr_d = np.stack([fr[i] for i in fi]), np.stack([fr[i] for i in pi])
        self._pv, self._pv_d = ld([pinvs[i] for i in fi]), ld([pinvs[i] for i in pi])
        self.w = np.asarray(model["rate_weights"], dtype=np.float64).astype(LD)
        self.rates = np.asarray(model["rates"], dtype=np.float64).astype(LD)
        self.sites = tipclvs.shape[1]
        self.pw = (np.ones(self.sites) if pattern_weights is None else np.asarray(pattern_weights)).astype(LD)
        inv = np.full(self.sites, -1) if invariant is None else np.asarray(invariant)
        if model.get("params_indices") is None:
            self.inv_lk = np.where(inv >= 0, self.freqs[np.maximum(inv, 0)], LD(0))
        self._inv = inv
        self.branch = {int(m): float(t) for m, t in zip(plan.matrix_indices, plan.branch_lengths)}
        self.clv = {i: np.asarray(c, dtype=np.float64).astype(LD) for i, c in enumerate(tipclvs)}
        for op in np.ascontiguousarray(plan.ops if ops is None else ops, dtype=OPS_DTYPE):
            a = self.propagate(self.clv[int(op["child1_clv_index"])], self.branch[int(op["child1_matrix_index"])])
            b = self.propagate(self.clv[int(op["child2_clv_index"])], self.branch[int(op["child2_matrix_index"])])
            self.clv[int(op["parent_clv_index"])] = a * b

    def _scaled_rates(self):
        return np.where(self._pv_d > 0, self.rates / (LD(1) - self._pv_d), self.rates)

    def pmatrix(self, t, order=0):
        """[R][S][S]: P(t) (order 0), dP/dt (1) or d2P/dt2 (2)"""
        r = self._scaled_rates()
        x = self._lam * r[:, None]                             # [R][S]: lambda_m r_k'
        d = np.exp(x * LD(t)) * x ** order
        return np.einsum("kjm,km,kmi->kji", self._iv, d, self._ev)

    def propagate(self, clv, t):
        """sum_j P(t)[i][j] clv[n][k][j]"""
        return np.einsum("kij,nkj->nki", self.pmatrix(t), clv)

    def _site_lk(self, terms, deriv=False):
        """terms [sites][R]: the categories' sums -> site likelihoods with the invariant part (deriv: with the
        frequencies and proportions the derivative calls take, params_indices)"""
        fr, p = (self._fr_d, self._pv_d) if deriv else (self._fr, self._pv)
        if (p > 0).any():
            inv_lk = np.where((self._inv >= 0)[:, None], fr[:, np.maximum(self._inv, 0)].T, LD(0))   # [sites][R]
            terms = terms * (LD(1) - p)[None, :] + inv_lk * p[None, :]
        return (terms * self.w[None, :]).sum(axis=1)

    def root_loglikelihood(self, node):
        """(sum, per-site [sites]) of pll_compute_root_loglikelihood at CLV `node`, in longdouble"""
        site = self._site_lk(np.einsum("nki,ki->nk", self.clv[node], self._fr))
        ps = np.log(site) * self.pw
        return ps.sum(), ps

    def _edge_terms(self, p, c, t, order, deriv=False):
        """sum_i pi_i p_i sum_j P^(order)(t)[i][j] c_j per (site, category)"""
        pc = np.einsum("kij,nkj->nki", self.pmatrix(t, order), self.clv[c])
        return np.einsum("nki,nki,ki->nk", self.clv[p], pc, self._fr_d if deriv else self._fr)

    def edge_loglikelihood(self, p, c, t):
        """(sum, per-site) over the edge p -- c of length t"""
        ps = np.log(self._site_lk(self._edge_terms(p, c, t, 0))) * self.pw
        return ps.sum(), ps

    def derivatives(self, p, c, t):
        """(d_f, dd_f, d_mag, dd_mag) of -lnL at branch length t: the two totals, and the size of what they add up,
        sum_n w_n |L'/L| and sum_n w_n ((L'/L)^2 + |L''/L|) (helpers.derivative_magnitudes)"""
        lk = self._site_lk(self._edge_terms(p, c, t, 0, True), True)
        # the invariant part does not depend on t
        qw = ((LD(1) - self._pv_d) * self.w)[None, :]
        d1 = (self._edge_terms(p, c, t, 1, True) * qw).sum(axis=1) / lk
        d2 = (self._edge_terms(p, c, t, 2, True) * qw).sum(axis=1) / lk
        return ((-d1 * self.pw).sum(), ((d1 * d1 - d2) * self.pw).sum(), (np.abs(d1) * self.pw).sum(),
                ((d1 * d1 + np.abs(d2)) * self.pw).sum())
