"""Shared data of tests/test_gpu_unstored_state.py, tests/test_unstored_state_lists.py and tests/moving_root.py (the
walks of tests/test_gpu_moving_root_routes.py): the trees and seeded walks of a root that moves, and the list builder that turns a new root edge into the op list a tree search would hand
pll_update_partials -- a partial traversal (the reference's pll_utree_traverse with a callback that stops at a node
whose CLV is valid and points the right way).

Nothing here needs a device.
"""
import numpy as np

from libpll_amd import workload as W
from libpll_amd.pllapi import OPS_DTYPE

# (tree, tips, seed) of the walks; every walk draws its root edges with numpy.random.default_rng(WALK_SEED) from
# sorted(view.edges()), tip edges included
WALKS = [("random", 17, 5), ("random", 20, 16), ("balanced", 16, 7), ("balanced", 32, 7)]
WALK_SEED = 1
MOVES = 60
TREES = {"balanced": W.balanced_tree, "random": W.random_tree}


def walk_plan(shape, tips, seed, scalers=True, branch=None):
    return TREES[shape](tips, seed=seed, use_scalers=scalers, branch=branch)


class Orientation:
    """Which way every inner CLV of an unrooted tree points, and what it was computed from.

    For each inner node: the neighbour its CLV currently points at (None: never computed) and the set of
    (branch, version) pairs beneath it when it was computed.  `move(root)` returns the post-order list of exactly the
    nodes that point the wrong way or lie above a changed branch, for the traversal directed at `root`, and the
    arguments of the edge lnL there; it records the list as run."""

    def __init__(self, view):
        self.view = view
        self.tips = view.tips
        self.version = {frozenset(e): 0 for e in view.edges()}
        self.toward = {x: None for x in view.adj if x >= self.tips}
        self.beneath = {x: None for x in self.toward}

    def change(self, edge):
        """the branch `edge` has a new length"""
        self.version[frozenset(edge)] += 1

    def truth(self, x, frm):
        """the (branch, version) pairs beneath x seen from neighbour frm"""
        out, stack = set(), [(x, frm)]
        while stack:
            y, f = stack.pop()
            for z in self.view.adj[y]:
                if z != f:
                    e = frozenset((y, z))
                    out.add((e, self.version[e]))
                    if z >= self.tips:
                        stack.append((z, y))
        return frozenset(out)

    def _op(self, x, frm):
        v = self.view
        c1, c2 = [y for y in v.adj[x] if y != frm]
        sc = lambda n: W._scaler_of(n, self.tips, v.use_scalers)  # noqa: E731
        return (x, sc(x), c1, v.matrix[frozenset((x, c1))], sc(c1), c2, v.matrix[frozenset((x, c2))], sc(c2))

    def move(self, root):
        a, b = root
        rows = []
        for top, away in ((a, b), (b, a)):
            stack = [(top, away, False)]
            while stack:
                x, frm, done = stack.pop()
                if x < self.tips:
                    continue
                if done:
                    rows.append(self._op(x, frm))
                    self.toward[x], self.beneath[x] = frm, self.truth(x, frm)
                    continue
                if self.toward[x] == frm and self.beneath[x] == self.truth(x, frm):
                    continue        # valid, and everything beneath it was when it was computed: not descended into
                stack.append((x, frm, True))
                for y in self.view.adj[x]:
                    if y != frm:
                        stack.append((y, x, False))
        ops = np.zeros(len(rows), dtype=OPS_DTYPE)
        for i, row in enumerate(rows):
            ops[i] = row
        if a < self.tips:
            a, b = b, a
        sc = lambda n: W._scaler_of(n, self.tips, self.view.use_scalers)  # noqa: E731
        return ops, (a, sc(a), b, sc(b), self.view.matrix[frozenset((a, b))])


def walk_moves(shape, tips, seed, scalers=True, change_branches=True, branch=None, replay_every=0):
    """The walk over one tree, as plain data: (plan, view, [move]) with move = dict(root, ops, edge, changed, replay)
    -- `changed` the (matrix index, new length) given to the previous root branch before the list, or None.  The first
    entry of the list is the full traversal at the plan's own root (move 0); MOVES drawn moves follow.

    replay_every = n > 0: every n-th move with a non-empty list (move 0 included) is followed by a replay -- the first
    branch its last op reads gets a new length and the SAME list is to be run once more.  `replay` is that (matrix
    index, new length), None elsewhere.  The tracker is told of the branch, so later lists recompute what lies above
    it (the list's own nodes among them, which the replay left current: that costs ops, not correctness).  The roots
    drawn and the lengths of `changed` are the same with and without replays."""
    plan = walk_plan(shape, tips, seed, scalers, branch)
    view = W.UnrootedView(plan, use_scalers=scalers)
    track = Orientation(view)
    edges = sorted(view.edges())
    rng = np.random.default_rng(WALK_SEED)
    lengths = np.random.default_rng(WALK_SEED + 1000)
    replay_lengths = np.random.default_rng(WALK_SEED + 2000)

    def replay_of(k, ops):
        if not replay_every or k % replay_every or not len(ops):
            return None
        top, kid = int(ops[-1]["parent_clv_index"]), int(ops[-1]["child1_clv_index"])
        track.change((top, kid))
        t = float(replay_lengths.uniform(0.01, 0.3)) if branch is None else float(branch) * float(replay_lengths.uniform(0.5, 2.0))
        return int(ops[-1]["child1_matrix_index"]), t

    root = tuple(view.root)
    ops, edge = track.move(root)
    moves = [dict(root=root, ops=ops, edge=edge, changed=None, replay=replay_of(0, ops))]
    for k in range(1, MOVES + 1):
        new = edges[int(rng.integers(len(edges)))]
        changed = None
        if change_branches and k % 3 == 0:
            track.change(root)
            t = float(lengths.uniform(0.01, 0.3)) if branch is None else float(branch) * float(lengths.uniform(0.5, 2.0))
            changed = (int(view.matrix[frozenset(root)]), t)
        root = new
        ops, edge = track.move(root)
        moves.append(dict(root=root, ops=ops, edge=edge, changed=changed, replay=replay_of(k, ops)))
    return plan, view, moves


def kinds_of(ops, tips):
    """(tip-tip ops, other ops) of a list"""
    tt = sum(1 for op in ops if int(op["child1_clv_index"]) < tips and int(op["child2_clv_index"]) < tips)
    return tt, len(ops) - tt
