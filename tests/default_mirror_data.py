"""Shared helpers of tests/test_gpu_default_mirrors.py: partitions that keep their host mirrors current by themselves
(PLL_AMD_AUTO_MIRROR_MB unset, the default), read the way an unmodified reference client reads them -- through the
struct fields, without a pll_amd_sync_* call -- and their twins: the same case with PLL_AMD_AUTO_MIRROR_MB=0, given the
same calls and read through get_clv / get_scaler / get_pmatrix.

Every reader here copies at once: get_clv and its like write into the very buffer the struct field points at, so a
comparison made after one of them would compare the sync call's copy, not the one the library made by itself.
"""
import contextlib
import ctypes as C

import numpy as np

from helpers import bits_equal, clv_ok, clvs_bitwise

ENV = "PLL_AMD_AUTO_MIRROR_MB"


@contextlib.contextmanager
def no_mirrors(monkeypatch):
    """partitions created inside are twins: PLL_AMD_AUTO_MIRROR_MB=0, read when a partition is created"""
    monkeypatch.setenv(ENV, "0")
    try:
        yield
    finally:
        monkeypatch.delenv(ENV, raising=False)


def pair(lib, case, attrs, monkeypatch, build):
    """(mirroring partition, twin) of one case; build(lib, case, attrs) creates a partition"""
    monkeypatch.delenv(ENV, raising=False)
    p = build(lib, case, attrs)
    with no_mirrors(monkeypatch):
        t = build(lib, case, attrs)
    return p, t


def address(pointer):
    """the address a struct field holds (None: NULL)"""
    return C.cast(pointer, C.c_void_p).value


def clv_mirror(p, node):
    """partition->clv[node] as it stands: [sites (+ states)][rate_cats][states], copied; no sync call"""
    assert p.s.clv[node], "partition->clv[%d] is NULL" % node
    n = p.sites_total * p.span
    return np.ctypeslib.as_array(p.s.clv[node], shape=(n,)).copy().reshape(p.sites_total, p.s.rate_cats,
                                                                          p.s.states_padded)[:, :, :p.s.states]


def scaler_mirror(p, sc):
    """partition->scale_buffer[sc] as it stands, copied; no sync call"""
    assert p.s.scale_buffer[sc], "partition->scale_buffer[%d] is NULL" % sc
    return np.ctypeslib.as_array(p.s.scale_buffer[sc], shape=(p.scaler_len,)).copy()


def pmatrix_mirror(p, m):
    """partition->pmatrix[m] as it stands: [rate_cats][states][states], copied; no sync call"""
    assert p.s.pmatrix[m], "partition->pmatrix[%d] is NULL" % m
    S, SP, R = p.s.states, p.s.states_padded, p.s.rate_cats
    return np.ctypeslib.as_array(p.s.pmatrix[m], shape=(R * S * SP,)).copy().reshape(R, S, SP)[:, :, :S]


def snapshot(p, nodes, scalers):
    """({node: CLV mirror}, {scale buffer: counts}) copied from the struct fields; a NULL pointer fails"""
    return ({int(n): clv_mirror(p, int(n)) for n in nodes},
            {int(s): scaler_mirror(p, int(s)) for s in scalers})


def poison(p, nodes, scalers):
    """Overwrite mirrors by hand with a pattern no result holds (all bits set: NaNs, counts of 2^32 - 1).  A fresh
    mirror is zeros and so are most scaler counts, so a copy that leaves out a buffer, a quad or a tail word can go
    unseen the first time; over poisoned mirrors it cannot."""
    for n in nodes:
        np.ctypeslib.as_array(p.s.clv[n], shape=(p.sites_total * p.span,)).view(np.uint64)[:] = 0xFFFFFFFFFFFFFFFF
    for s in scalers:
        np.ctypeslib.as_array(p.s.scale_buffer[s], shape=(p.scaler_len,))[:] = 0xFFFFFFFF


def written_by(ops):
    """(parent CLVs, parent scale buffers) a list names, each once, sorted"""
    nodes = sorted(set(int(x) for x in ops["parent_clv_index"]))
    scalers = sorted(set(int(x) for x in ops["parent_scaler_index"]) - {-1})
    return nodes, scalers


def assert_current(p, t, o, ops, states, what=""):
    """The mirrors of everything `ops` wrote on the mirroring partition p, read first and without a sync call, against
    the oracle o (counts bit for bit, CLVs by helpers.clv_ok with helpers.clvs_bitwise) and against the twin t (equal
    bytes).  Returns the snapshot."""
    nodes, scalers = written_by(ops)
    clvs, counts = snapshot(p, nodes, scalers)
    exact = clvs_bitwise(states)
    for node in nodes:
        assert clv_ok(clvs[node], o.clv[node], exact), "%s CLV mirror %d differs from the oracle" % (what, node)
        assert bits_equal(clvs[node], t.get_clv(node)), "%s CLV mirror %d differs from the twin's CLV" % (what, node)
    for sc in scalers:
        assert (counts[sc] == o.scalers[sc]).all(), "%s scaler mirror %d differs from the oracle" % (what, sc)
        assert (counts[sc] == t.get_scaler(sc)).all(), "%s scaler mirror %d differs from the twin's" % (what, sc)
    return clvs, counts


def ops_above(plan, changed):
    """the ops of plan.ops on the way from the nodes `changed` (the lower ends of branches) to the root edge, in list
    order -- what a client runs again after those branches got new lengths"""
    dirty = set()
    for node in changed:
        while node in plan.parent_of and plan.parent_of[node] != node:
            par = plan.parent_of[node]
            if par in dirty:
                break
            dirty.add(par)
            node = par
    parents = set(int(x) for x in plan.ops["parent_clv_index"])
    return plan.ops[[int(op["parent_clv_index"]) in (dirty & parents) for op in plan.ops]]


def set_lengths(plan, indices, lengths):
    """plan.branch_lengths of the matrices `indices` := lengths"""
    where = {int(mi): i for i, mi in enumerate(plan.matrix_indices)}
    for mi, t in zip(indices, lengths):
        plan.branch_lengths[where[int(mi)]] = float(t)


def oracle_pmatrix(orc, o, t):
    """the P-matrix of branch length t under the model of the OracleRun o: [rate_cats][states][states]"""
    return orc.pmatrix(o.S, o.R, o.m["rates"], float(t), o._ev, o._vc, o._iv, o._pinv)
