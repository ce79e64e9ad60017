"""The walks of tests/test_gpu_moving_root_routes.py on the 20-state whole-list kernel, without a device: every list
goes through pllhip_aa_list_plan_dry (the three functions pllhip_aa_fused_update plans a new list with), each list's
outgoing bounds being the next one's incoming ones (moving_root.plan_lists).  A walk that stopped exercising the kernel
-- no operands of earlier calls, no lookups, nothing on inherited bounds -- shows here, on any machine.

Counted over the planned lists (two or more ops) after move 0; the bars are moving_root.check_conditions', the counts
they were set below are in the table of tests/test_gpu_moving_root_routes.py (and printed here).  No list is refused
(rc == 0) or too wide for every window (plan_lists asserts both).
"""
import pytest

import moving_root as M
import unstored_state_data as U

# (walk, pattern tips, scale buffers, tip-inner mat-vecs on the matrix cores): the configurations of rows a and b
CASES = [(U.WALKS[0], True, True, 1), (U.WALKS[1], True, True, 1), (U.WALKS[2], True, True, 1),
         (U.WALKS[0], True, True, 0), (U.WALKS[1], True, True, 0), (U.WALKS[2], True, True, 0),
         (U.WALKS[0], False, True, 1), (U.WALKS[0], True, False, 1), (U.WALKS[0], True, False, 0)]


def _counts(amd, walk_id, pattern_tip, scalers, ti_mfma):
    plan, _, moves = M.walk(*walk_id, scalers=scalers)
    dry = M.plan_lists(amd, plan, moves, pattern_tip=pattern_tip, ti_mfma=ti_mfma)
    return M.list_counts(dry, moves), dry, moves


@pytest.mark.parametrize("walk_id,pattern_tip,scalers,ti_mfma", CASES)
def test_walks_exercise_the_whole_list_kernel(amd, walk_id, pattern_tip, scalers, ti_mfma):
    n, dry, moves = _counts(amd, walk_id, pattern_tip, scalers, ti_mfma)
    print("%s %d seed %d, pattern tips %s, scale buffers %s, ti_mfma %d: %r" % (*walk_id, pattern_tip, scalers, ti_mfma, n))
    M.check_conditions(n, walk_id[0], pattern_tip, bool(ti_mfma))
    assert n["planned"] >= 45
    if not pattern_tip or not scalers:
        # no tip-inner op (tip CLVs), or no op that scales: nothing is ever tested under the certificate
        assert n["kind1"] == n["kind2"] == 0
        if not pattern_tip:
            assert n["largest_bound"] == 0.0 and n["lookups"] == n["tip_tip"] == 0
    elif ti_mfma:
        if walk_id[0] == "random":
            assert n["kind2"] >= 10, "lists that run on bounds inherited from earlier lists alone: %r" % n
        assert n["kind1"] >= 30 and 0 < n["largest_bound"] < 1e-12, n
    else:
        # in the reference's order nothing is ever marked
        assert n["kind1"] == n["kind2"] == 0 and n["largest_bound"] == 0.0


def test_one_op_lists_carry_bounds_on(amd):
    """a list of one op over a marked operand marks its parent (the per-level launches' rule): the bounds the next
    planned list meets are not those of a walk that forgot it"""
    plan, _, moves = M.walk(*U.WALKS[0])
    dry = M.plan_lists(amd, plan, moves)
    single = [d for d in dry if d is not None and not d["planned"]]
    assert single and any(d["cert_kind"] == 2 for d in single)
    assert all(d["list_ti_mfma"] == 0 and d["cert_kind"] in (0, 2) for d in single)


def test_replays_are_in_the_walks():
    for walk_id in U.WALKS[:3]:
        _, _, moves = M.walk(*walk_id)
        _, _, plain = U.walk_moves(*walk_id)
        assert [mv["root"] for mv in moves] == [mv["root"] for mv in plain]
        assert [mv["changed"] for mv in moves] == [mv["changed"] for mv in plain]
        assert all(mv["replay"] is None for mv in plain)
        replays = [k for k, mv in enumerate(moves) if mv["replay"] is not None]
        assert len(replays) >= 6 and all(k % M.REPLAY_EVERY == 0 for k in replays) and replays[0] == 0
        for k in replays:
            op, (matrix, length) = moves[k]["ops"][-1], moves[k]["replay"]
            assert matrix == int(op["child1_matrix_index"]) and length > 0
            assert int(op["parent_clv_index"]) in moves[k]["root"]
