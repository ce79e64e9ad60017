"""A root that moves, on any route of pll_update_partials: the driver of tests/test_gpu_moving_root_routes.py and the
device-less planning of its 20-state lists (tests/test_moving_root_route_lists.py).

The walks are those of tests/unstored_state_data.py (walk_moves with replay_every = REPLAY_EVERY): move 0 is the full
traversal, every later move re-roots the tree at a drawn edge and recomputes only the CLVs that now point the wrong way
or lie above a changed branch, so nearly every list reads operands that earlier calls wrote.

RootWalk runs ONE product partition next to the oracle (helpers.oracle_run), which is given the same lists and the
partition's own P-matrices; optionally a second partition on another route runs the same calls.  Per move, in order:
the branch change, the list, the edge lnL with per-site values (LNL_RTOL, PERSITE_RTOL of
tests/test_gpu_result_calls.py); every 5th move the sumtable (< 1e-12) and the derivatives at TS (DERIV_RTOL); every
10th move and the last a fresh oracle's full traversal towards this root -- what exposes a stale CLV -- and every CLV
and scale buffer the move's list wrote, read back (counts bit for bit, CLVs by helpers.clv_ok with
helpers.clvs_bitwise: bit for bit except 20 states on the default path, 1e-12 there); every 7th move the replay -- one
branch under the list's last op gets a new length and the same list runs again, which is the kept plan of a partial
list with new matrices.  After the walk every CLV of move 0's list is read back.
"""
import os

import numpy as np

import unstored_state_data as U
from helpers import (build_partition, oracle_run, bits_equal, clv_ok, clv_err, clvs_bitwise, rel_err, sumtable_err,
                     derivative_magnitudes, deriv_errs, params_of, freqs_of)
from test_gpu_result_calls import DERIV_RTOL, PERSITE_RTOL, LNL_RTOL
from test_host_aa_list_plan import aa_dry

TS = (0.003, 0.13, 2.0)
REPLAY_EVERY, DERIV_EVERY, FRESH_EVERY = 7, 5, 10
KINDS = ("ops", "tip_tip_ahead", "tip_tip_in_list", "lookups", "inner_inner_matrix_cores", "tip_inner_matrix_cores",
         "tip_inner_vector_unit", "reloads")
# the lookup ops a 20-state list may hold: 64 MB of table sets of 4 x (23^2 + 64) rows of 4 x 20 doubles (a partition
# of this size adds nothing to the pool; pllhip_aa_lookup_budget) -- more than any list of these walks has ops
LOOKUP_BUDGET = (64 << 20) // (4 * (23 * 23 + 64) * 4 * 20 * 8)
MAX_SEGMENTS = 8


def walk(shape, tips, seed, scalers=True, branch=None):
    """(plan, view, moves) of one of U.WALKS, with the replays"""
    return U.walk_moves(shape, tips, seed, scalers=scalers, branch=branch, replay_every=REPLAY_EVERY)


def levels_of(ops):
    """dependency levels of a tree's list: an op lies one above the highest op of the list that wrote a child of it"""
    level = {}
    for op in ops:
        level[int(op["parent_clv_index"])] = 1 + max(level.get(int(op["child%d_clv_index" % k]), 0) for k in (1, 2))
    return max(level.values()) if level else 0


# ---- the 20-state lists without a device

def plan_lists(amd, plan, moves, pattern_tip=True, ti_mfma=1):
    """What pllhip_aa_list_plan_dry says of every list of a walk, in the order the library meets them: per move None
    (no op) or the dry call's result.  The bounds each list leaves on its CLVs are the next list's `incoming`.  A list
    of one op is not the whole-list kernel's: the per-level launches take it in the reference's order, where a value
    is marked only when an operand is (launch_levels) -- the dry call with ti_mfma = 0 states the same rule; its entry
    has planned = False.  (A replay plans nothing new: the same ops over operands with the same bounds.)"""
    incoming, out = None, []
    for mv in moves:
        ops = mv["ops"]
        if not len(ops):
            out.append(None)
            continue
        planned = len(ops) >= 2
        d = aa_dry(amd, ops, plan, lookups_max=LOOKUP_BUDGET, tt_inside=1, ti_mfma=ti_mfma if planned else 0,
                   max_segments=MAX_SEGMENTS, incoming=incoming, pattern_tip=1 if pattern_tip else 0)
        assert d["rc"] == 0 and d["too_wide"] == 0, (mv["root"], d["rc"], d["too_wide"])
        d["planned"] = planned
        incoming = d["bounds"]
        out.append(d)
    return out


def list_counts(dry, moves):
    """the conditions of the walks on the whole-list kernel, counted over the planned lists after move 0"""
    n = dict(planned=0, reloads=0, lookups=0, tip_tip=0, tip_inner_mfma=0, two_ops=0, kind1=0, kind2=0, kind0=0,
             largest_bound=0.0)
    for k, (d, mv) in enumerate(zip(dry, moves)):
        if d is None or not d["planned"]:
            continue
        n["largest_bound"] = max(n["largest_bound"], float(d["bounds"].max()))
        if k == 0:
            continue
        kinds = dict(zip(KINDS, d["kinds"]))
        n["planned"] += 1
        n["reloads"] += kinds["reloads"] > 0
        n["lookups"] += kinds["lookups"] > 0
        n["tip_tip"] += kinds["tip_tip_in_list"] > 0
        n["tip_inner_mfma"] += kinds["tip_inner_matrix_cores"] > 0
        n["two_ops"] += len(mv["ops"]) == 2
        n["kind%d" % d["cert_kind"]] += 1
    return n


def check_conditions(n, shape, pattern_tip, mfma):
    """The bars of the walks on the 20-state whole-list kernel; each lies below what the planner gives today (the
    table in tests/test_gpu_moving_root_routes.py).  A planner that moves a count below its bar asks for another seed,
    not for a lower bar."""
    assert n["two_ops"] >= 4, "two-op lists: %r" % n
    if not pattern_tip:
        assert n["reloads"] == n["planned"] > 0, "tip CLVs: every planned list reloads an operand: %r" % n
        return
    if shape == "random":
        assert n["reloads"] >= 45, "lists that reload operands of earlier calls: %r" % n
        assert n["lookups"] >= 10, "lists with a lookup op: %r" % n
        assert n["tip_tip"] >= 20, "lists with a tip-tip op: %r" % n
        if mfma:
            assert n["tip_inner_mfma"] >= 30, "lists with a tip-inner op on the matrix cores: %r" % n
    else:
        assert n["reloads"] >= 45 and n["tip_tip"] >= 30, "balanced: %r" % n


# ---- the walk on a device

class RootWalk:
    """case: make_case / odd_state_case / many_state_case data (its plan is replaced by the walk's); env: switches set
    through `monkeypatch` before the partition is created and left set; second: None or dict(attrs=, env=, lnl_rtol=)
    -- a partition that runs the same calls, created under `env` on top (put back afterwards: PLL_AMD_DEVICES), whose
    per-site lnL, sumtables, CLVs and counts equal the first one's bit for bit and whose lnL agrees to lnl_rtol (0: it
    and the derivatives are equal; otherwise the derivatives agree to DERIV_RTOL)."""

    def __init__(self, lib, orc, case, attrs, the_walk, monkeypatch=None, env=None, second=None):
        self.lib, self.orc, self.case, self.attrs = lib, orc, case, attrs
        self.plan, self.view, self.moves = the_walk
        case["plan"] = self.plan
        self.pi, self.fi = params_of(case), freqs_of(case)
        for name, value in (env or {}).items():
            monkeypatch.setenv(name, value)
        self.p = build_partition(lib, case, attrs)
        self.q, self.q_rtol = None, 0.0
        if second is not None:
            was = {name: os.environ.get(name) for name in second.get("env", {})}
            for name, value in second.get("env", {}).items():
                monkeypatch.setenv(name, value)
            self.q = build_partition(lib, case, second.get("attrs", attrs))
            for name, value in was.items():
                if value is None:
                    monkeypatch.delenv(name)
                else:
                    monkeypatch.setenv(name, value)
            self.q_rtol = float(second.get("lnl_rtol", 0.0))
        self.parts = [x for x in (self.p, self.q) if x is not None]
        self.o = oracle_run(orc, lib, self.p, case, attrs)
        self.exact = clvs_bitwise(case["states"])
        self.worst = dict(lnl=0.0, persite=0.0, sumtable=0.0, deriv=0.0, clv=0.0)

    # -- the calls, on the partitions and on the oracle
    def matrices(self, indices, lengths):
        indices = np.asarray(indices, dtype=np.uint32)
        for x in self.parts:
            x.update_prob_matrices(self.pi, indices, np.asarray(lengths, dtype=np.float64))
        for mi in indices:
            self.o.pmat[int(mi)] = self.p.get_pmatrix(int(mi))
            if self.q is not None:
                assert bits_equal(self.q.get_pmatrix(int(mi)), self.o.pmat[int(mi)])

    def update(self, ops):
        for x in self.parts:
            x.update_partials(ops)
        self.o.update_partials(ops)

    def lnl(self, edge, what):
        got = self.p.compute_edge_loglikelihood(*edge, self.fi, persite=True)
        ref = self.o.edge_loglikelihood(*edge, persite=True)
        e_lnl, e_site = abs(got[0] - ref[0]) / abs(ref[0]), rel_err(got[1], ref[1])
        self.worst["lnl"], self.worst["persite"] = max(self.worst["lnl"], e_lnl), max(self.worst["persite"], e_site)
        assert e_lnl <= LNL_RTOL, "%s: lnL %r, oracle %r" % (what, got[0], ref[0])
        assert e_site < PERSITE_RTOL, "%s: per-site lnL off by %.3g" % (what, e_site)
        if self.q is not None:
            b = self.q.compute_edge_loglikelihood(*edge, self.fi, persite=True)
            assert bits_equal(got[1], b[1]), "%s: per-site lnL of the second partition" % what
            assert abs(got[0] - b[0]) <= self.q_rtol * abs(got[0]), "%s: lnL %r, second partition %r" % (what, got[0], b[0])
        return got[0]

    def derivatives(self, edge, what):
        pc, ps, cc, cs = edge[:4]
        so = self.o.sumtable(pc, cc, ps, cs)
        first = None
        for x in self.parts:
            st = x.alloc_sumtable()
            x.update_sumtable(pc, cc, ps, cs, self.pi, st)
            table = x.get_sumtable(st)
            ds = [x.compute_likelihood_derivatives(ps, cs, t, self.pi, st) for t in TS]
            if first is None:
                first = (table, ds)
                e = sumtable_err(table, so)
                self.worst["sumtable"] = max(self.worst["sumtable"], e)
                assert e < 1e-12, "%s: sumtable off by %.3g" % (what, e)
                for t, d in zip(TS, ds):
                    want = self.o.derivatives(so, t)
                    mags = derivative_magnitudes(self.o.m, so, t, self.o.pw, self.o.invariant)
                    e = deriv_errs(d, want, t, mags)
                    self.worst["deriv"] = max(self.worst["deriv"], e)
                    assert e < DERIV_RTOL, "%s: derivatives at t = %g: %r, oracle %r" % (what, t, d, want)
            else:
                assert bits_equal(table, first[0]), "%s: sumtable of the second partition" % what
                for t, d, d0 in zip(TS, ds, first[1]):
                    # (lnl_rtol > 0: its totals are summed in another order -- shards --: the bar the totals themselves
                    # are held to)
                    mags = derivative_magnitudes(self.o.m, so, t, self.o.pw, self.o.invariant)
                    assert d == d0 or (self.q_rtol > 0 and deriv_errs(d, d0, t, mags) < DERIV_RTOL), \
                        "%s: derivatives of the second partition at t = %g: %r, %r" % (what, t, d, d0)

    def read_back(self, ops, what):
        for op in ops:
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            got = self.p.get_clv(node)
            self.worst["clv"] = max(self.worst["clv"], clv_err(got, self.o.clv[node]))
            assert clv_ok(got, self.o.clv[node], self.exact), "%s: CLV %d differs from the oracle's (%.3g)" % (
                what, node, clv_err(got, self.o.clv[node]))
            if sc >= 0:
                counts = self.p.get_scaler(sc)
                assert (counts == self.o.scalers[sc]).all(), "%s: scale buffer %d" % (what, sc)
            if self.q is not None:
                assert bits_equal(self.q.get_clv(node), got), "%s: CLV %d of the second partition" % (what, node)
                assert sc < 0 or (self.q.get_scaler(sc) == counts).all(), "%s: scale buffer %d of the second partition" % (what, sc)

    def fresh_traversal(self, mv, lnl, what):
        """a full traversal towards this root on an oracle of its own: a list that left a stale CLV shows"""
        fresh = oracle_run(self.orc, self.lib, self.p, self.case, self.attrs)
        fresh.pmat[:] = self.o.pmat
        full, full_edge = self.view.traversal(mv["root"])
        assert full_edge == mv["edge"]
        fresh.update_partials(full)
        ref = fresh.edge_loglikelihood(*mv["edge"])
        assert abs(lnl - ref) <= LNL_RTOL * abs(ref), "%s: lnL %r, a fresh traversal's %r" % (what, lnl, ref)

    # -- the walk
    def run(self, on_list=None):
        """on_list(k, move, replay): called after every list has been handed to the partitions, before anything
        reads a result.  Returns the walk's figures: the largest errors against the oracle and `scaled`, the moves
        with non-zero counts at both ends of the root edge (on the oracle)."""
        moves, last = self.moves, len(self.moves) - 1
        scaled = 0
        for k, mv in enumerate(moves):
            what = "move %d, root %r" % (k, mv["root"])
            if mv["changed"] is not None:
                self.matrices([mv["changed"][0]], [mv["changed"][1]])
            ops, edge = mv["ops"], mv["edge"]
            if len(ops):
                self.update(ops)
                if on_list:
                    on_list(k, mv, False)
            lnl = self.lnl(edge, what)
            # (a tip end has no counts)
            scaled += all(int(self.o.scalers[sc].max()) > 0 for sc in (edge[1], edge[3]) if sc >= 0) and edge[1] >= 0
            if k % DERIV_EVERY == 0:
                self.derivatives(edge, what)
            if k % FRESH_EVERY == 0 or k == last:
                self.fresh_traversal(mv, lnl, what)
                self.read_back(ops, what)
            if mv["replay"] is not None:
                assert len(ops) and k % REPLAY_EVERY == 0
                self.matrices([mv["replay"][0]], [mv["replay"][1]])
                self.update(ops)
                if on_list:
                    on_list(k, mv, True)
                again = self.lnl(edge, what + ", replayed")
                assert again != lnl, "%s: the replay's new branch length changed nothing" % what
                self.read_back(ops[-1:], what + ", replayed")
        self.read_back(moves[0]["ops"], "after the walk")
        return dict(self.worst, scaled=scaled)

    def destroy(self):
        for x in self.parts:
            x.destroy()
