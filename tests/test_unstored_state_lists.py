"""The list builder of tests/unstored_state_data.py (no device): the walks of tests/test_gpu_unstored_state.py run
with symbolic values.  A CLV's tag is what it was computed from -- its node, and for each child the child's tag and
the version of the branch to it -- so a stale or misdirected CLV anywhere beneath the root edge shows in the tags of
the root edge's two ends."""
import pytest

import unstored_state_data as U


def _full_tag(track, x, frm):
    """the tag a full traversal directed away from `frm` gives node x"""
    if x < track.tips:
        return x
    return (x, frozenset((_full_tag(track, y, x), track.version[frozenset((x, y))])
                         for y in track.view.adj[x] if y != frm))


def _run(store, versions, ops, tips):
    for op in ops:
        p = int(op["parent_clv_index"])
        kids = []
        for k in ("child1", "child2"):
            c = int(op[k + "_clv_index"])
            assert c < tips or c in store, "op %d reads CLV %d, which no list has written" % (p, c)
            kids.append((c if c < tips else store[c], versions[frozenset((p, c))]))
        store[p] = (p, frozenset(kids))


@pytest.mark.parametrize("change_branches", [False, True])
@pytest.mark.parametrize("shape,tips,seed", U.WALKS)
def test_partial_lists_leave_the_root_edge_current(shape, tips, seed, change_branches):
    plan = U.walk_plan(shape, tips, seed)
    view = U.W.UnrootedView(plan)
    track = U.Orientation(view)
    # the same draws as walk_moves, with the tracker in hand
    _, _, moves = U.walk_moves(shape, tips, seed, change_branches=change_branches)
    assert len(moves) == U.MOVES + 1 and len(moves[0]["ops"]) == tips - 2
    store, root = {}, None
    for k, mv in enumerate(moves):
        if mv["changed"] is not None:
            assert k % 3 == 0 and mv["changed"][0] == view.matrix[frozenset(root)]
            track.change(root)
        root = mv["root"]
        ops, edge = track.move(root)
        assert ops.tobytes() == mv["ops"].tobytes() and edge == mv["edge"]
        parents = [int(op["parent_clv_index"]) for op in ops]
        assert len(set(parents)) == len(parents)
        _run(store, track.version, ops, tips)
        a, b = root
        for x, frm in ((a, b), (b, a)):
            if x >= tips:
                assert store[x] == _full_tag(track, x, frm), "move %d: CLV %d is not what a full traversal gives" % (k, x)
        assert {edge[0], edge[2]} == {a, b} and edge[0] >= tips
        assert edge[4] == view.matrix[frozenset(root)]


# what the walks contain without branch changes: moves with two or more ops that are not tip-tip, moves with a tip-tip op
PINNED = {("random", 17, 5): (50, 28), ("random", 20, 16): (51, 24), ("balanced", 16, 7): (53, 36),
          ("balanced", 32, 7): (57, 35)}


@pytest.mark.parametrize("shape,tips,seed", U.WALKS)
def test_walks_have_lists_worth_planning(shape, tips, seed):
    """conditions 1 and 2 of the walks, with and without branch changes: at least two thirds of the moves have two or
    more ops that are not tip-tip, at least 20 contain a tip-tip op"""
    for change in (False, True):
        _, _, moves = U.walk_moves(shape, tips, seed, change_branches=change)
        kinds = [U.kinds_of(mv["ops"], tips) for mv in moves[1:]]
        two = sum(1 for tt, other in kinds if other >= 2)
        cherry = sum(1 for tt, other in kinds if tt >= 1)
        print("%s %d seed %d, branch changes %s: %d moves with >= 2 ops that are not tip-tip, %d with a tip-tip op"
              % (shape, tips, seed, change, two, cherry))
        assert two >= 40 and cherry >= 20, (two, cherry)
        # (a new length of the old root branch adds no op: the end that is re-oriented reads it anyway)
        assert (two, cherry) == PINNED[(shape, tips, seed)]
