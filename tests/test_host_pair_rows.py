"""Pair rows of the 4-state whole-list kernel, host side (no device): the byte, the index a lane takes from ONE row, and
the rows the encoder names per op (pllhip_fused_plan_dry_rows).

Byte n of the pair row of the ordered tip pair (a, b) is ((row_a[n] & 15) << 4) | (row_b[n] & 15): the pair-table index
that the kernel used to join from two tip rows on every tile (pllhip_fused_pair_index, tests/test_host_scalar_masks.py).
Every gathered factor now names one row and a shift: a cherry its pair row (shift 0, every bit of a byte counts), a
single tip its own row (low nibble, shift 4: a tip's factor table is indexed by the FIRST character).
"""
import ctypes as C

import numpy as np

from libpll_amd import workload as W

CH_LTIP, CH_SHIFT4, CH_NIBBLE = 1 << 16, 1 << 19, 1 << 20


def _fn(amd, name, argtypes, restype=C.c_uint):
    f = getattr(amd.lib, name)
    f.argtypes, f.restype = argtypes, restype
    return f


def test_byte_of_every_pair_of_raw_bytes(amd):
    """All 256 x 256 raw byte pairs: only the low nibbles count."""
    f = _fn(amd, "pllhip_pair_row_byte_dry", [C.c_uint, C.c_uint])
    for a in range(256):
        for b in range(256):
            assert f(a, b) == ((a & 15) << 4) | (b & 15), (a, b)


def test_one_row_gives_the_index_the_two_rows_gave(amd):
    """pllhip_fused_row_index on a pair row (built byte by byte with the function above), and on a single tip's row with
    shift 4 / 0, against pllhip_fused_pair_index on the tip rows -- every lane, both sub-steps, every kernel variant
    (sites per sub-step 4, 8, 16, 32).  Raw bytes with high nibbles set: a tip row's are masked, a pair row's count."""
    byte = _fn(amd, "pllhip_pair_row_byte_dry", [C.c_uint, C.c_uint])
    one = _fn(amd, "pllhip_fused_row_index_dry", [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint])
    two = _fn(amd, "pllhip_fused_pair_index_dry", [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint])
    rng = np.random.default_rng(5)
    M = 0x0f0f0f0f
    for sps in (4, 8, 16, 32):
        n = 2 * sps
        for rep in range(4):
            a = rng.integers(0, 256 if rep else 16, n).astype(np.uint8)
            b = rng.integers(0, 256 if rep else 16, n).astype(np.uint8)
            pair = np.array([byte(int(x), int(y)) for x, y in zip(a, b)], dtype=np.uint8)
            pa, pb, pp = (v.ctypes.data_as(C.c_void_p) for v in (a, b, pair))
            for j in range(2):
                for lane in range(64):
                    site = j * sps + lane // (64 // sps)
                    want = ((int(a[site]) & 15) << 4) | (int(b[site]) & 15)
                    assert two(pa, pb, M, M, sps, j, lane) == want
                    assert one(pp, 0, sps, j, lane) == want, (sps, j, lane)
                    assert one(pa, 1, sps, j, lane) == two(pa, pb, M, 0, sps, j, lane) == (int(a[site]) & 15) << 4
                    assert one(pb, 2, sps, j, lane) == two(pa, pb, 0, M, sps, j, lane) == int(b[site]) & 15
    assert one(None, 0, 8, 0, 0) == 0xffffffff and one(pp, 3, 8, 0, 0) == 0xffffffff
    assert one(pp, 0, 5, 0, 0) == 0xffffffff and one(pp, 0, 8, 2, 0) == 0xffffffff and one(pp, 0, 8, 0, 64) == 0xffffffff


def _rows(amd, plan, rate_cats=4, nslots=0):
    ops = np.ascontiguousarray(plan.ops)
    n = len(ops)
    nk, nb = C.c_uint(), C.c_uint()
    order, batch, gathers = (C.c_uint * n)(), (C.c_uint * n)(), (C.c_uint * (12 * n))()
    deferred, folded = (C.c_ubyte * n)(), (C.c_ubyte * n)()
    f = _fn(amd, "pllhip_fused_plan_dry_rows", [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_void_p, C.c_uint, C.c_uint] +
            [C.c_void_p] * 7, C.c_int)
    rc = f(plan.tips, plan.clv_buffers, plan.scale_buffers, 1, rate_cats, ops.ctypes.data_as(C.c_void_p), n, nslots,
           C.cast(C.byref(nk), C.c_void_p), C.cast(order, C.c_void_p), C.cast(deferred, C.c_void_p),
           C.cast(folded, C.c_void_p), C.cast(gathers, C.c_void_p), C.cast(batch, C.c_void_p), C.cast(C.byref(nb), C.c_void_p))
    assert rc == 0
    k = nk.value
    g = np.array(gathers, dtype=np.int64).reshape(n, 4, 3)[:k]
    return dict(order=list(order)[:k], deferred=[i for i in range(n) if deferred[i]], folded=[i for i in range(n) if folded[i]],
                gathers=g, batch=list(batch)[:k], nbatches=nb.value)


def _kids(op):
    return [int(op["child1_clv_index"]), int(op["child2_clv_index"])]


def _expected_factor(plan, d, clv):
    """the (first tip + 1, second tip + 1) a gathered child names: a tip itself, a deferred cherry its two tips in the
    order of the op's children"""
    if clv < plan.tips:
        return (clv + 1, 0)
    op = [plan.ops[i] for i in d["deferred"] if int(plan.ops[i]["parent_clv_index"]) == clv]
    assert len(op) == 1
    return tuple(k + 1 for k in _kids(op[0]))


def _check_rows(plan, d, lpr=1):
    """every walked op's gathers against the list itself; positions and batches against the one batching rule"""
    parent_op = {int(op["parent_clv_index"]): i for i, op in enumerate(plan.ops)}
    gathered = set(range(plan.tips)) | {int(plan.ops[i]["parent_clv_index"]) for i in d["deferred"]}
    q, batch, rpb = 0, 0, 64 // lpr
    for pos, i in enumerate(d["order"]):
        want = []
        for kid in _kids(plan.ops[i]):
            if kid in parent_op and parent_op[kid] in d["folded"]:
                want += [_expected_factor(plan, d, k) for k in _kids(plan.ops[parent_op[kid]])]
            elif kid in gathered:
                want.append(_expected_factor(plan, d, kid))
        if len(want) == 2 and want[0][1] == 0 and want[1][1] == 0 and all(k < plan.tips for k in _kids(plan.ops[i])):
            want = [(want[0][0], want[1][0])]     # an eager tip-tip op: the finished parent by its pair row
        g = d["gathers"][pos]
        got = [(int(x[0]), int(x[1])) for x in g if x[0] or x[1]]
        # (a reader of ONE folded product has the product "left": its factors first, whichever child it is)
        assert sorted(got) == sorted(want) and len(got) <= 4, (i, got, want)
        if q + len(got) > rpb:
            batch, q = batch + 1, 0
        assert d["batch"][pos] == batch
        for x in g:
            first, second, ch = int(x[0]), int(x[1]), int(x[2])
            if not first and not second:
                assert ch == 0
                continue
            assert ch & CH_LTIP and (ch & 0xff) == q * lpr and not ch & 0xff00
            assert bool(ch & CH_NIBBLE) == (not (first and second)), "a pair row's bytes count whole"
            assert bool(ch & CH_SHIFT4) == bool(first and not second), "a single tip is the table's first character"
            q += 1
    assert d["nbatches"] == batch + 1


def test_balanced_64_names_32_pair_rows(amd):
    plan = W.balanced_tree(64)
    d = _rows(amd, plan)
    assert len(d["order"]) == 14 and len(d["deferred"]) == 32 and len(d["folded"]) == 16
    four = [g for g in d["gathers"] if all(x[0] and x[1] for x in g)]
    assert len(four) == 8, "eight readers of two folded products: four pair rows each"
    named = [(int(x[0]), int(x[1])) for g in d["gathers"] for x in g if x[0] or x[1]]
    assert len(named) == 32 and len(set(named)) == 32 and all(a and b for a, b in named)
    assert sorted(t for ab in named for t in ab) == list(range(1, 65)), "every tip in exactly one pair row"
    assert d["nbatches"] == 1 and set(d["batch"]) == {0}
    assert all(int(x[2]) & (CH_SHIFT4 | CH_NIBBLE) == 0 for g in d["gathers"] for x in g)
    _check_rows(plan, d)


def test_caterpillar_names_a_pair_row_and_shifted_tip_rows(amd):
    plan = W.caterpillar_tree(12)
    d = _rows(amd, plan)
    assert len(d["deferred"]) == 1, "one cherry"
    named = [(int(x[0]), int(x[1]), int(x[2])) for g in d["gathers"] for x in g if x[0] or x[1]]
    pairs = [n for n in named if n[0] and n[1]]
    singles = [n for n in named if not (n[0] and n[1])]
    assert len(pairs) == 1 and not pairs[0][2] & (CH_SHIFT4 | CH_NIBBLE), "the cherry: shift 0"
    # (every op above the cherry adds one tip)
    assert len(singles) == len(plan.ops) - 1 and all(n[2] & CH_SHIFT4 and n[2] & CH_NIBBLE and not n[1] for n in singles), "tips: shift 4"
    _check_rows(plan, d)


RANDOM_160_SEED = 1   # (chosen so that the switch to the second batch lands on such a reader)


def test_random_160_second_batch_begins_at_a_reader_of_folded_products(amd):
    """More than 64 gathered rows at 4 categories (one lane per row, 64 rows per batch): a second batch, and the op that
    switches to it is a reader of folded products (three or four rows of its own)."""
    plan = W.random_tree(160, seed=RANDOM_160_SEED)
    d = _rows(amd, plan)
    nrows = sum(1 for g in d["gathers"] for x in g if x[0] or x[1])
    assert nrows > 64 and d["nbatches"] >= 2
    first = d["batch"].index(1)
    g = d["gathers"][first]
    assert sum(1 for x in g if x[0] or x[1]) >= 3, "a reader of folded products"
    parent_op = {int(op["parent_clv_index"]): i for i, op in enumerate(plan.ops)}
    assert any(parent_op.get(k) in d["folded"] for k in _kids(plan.ops[d["order"][first]]))
    _check_rows(plan, d)
    # 2 categories: two lanes per row, 32 rows per batch
    d2 = _rows(amd, plan, rate_cats=2)
    assert d2["nbatches"] > d["nbatches"]
    _check_rows(plan, d2, lpr=2)
