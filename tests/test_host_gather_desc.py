"""Gather descriptors of the 4-state whole-list kernel, host side (no device; DESIGN.md 2.0 "Memory queue", 8.4j):
pllhip_fused_gather_desc (partials_fused.hpp) through pllhip_fused_gather_desc_dry.

The kernel no longer decodes a record's character words: the encoder writes, per gathered factor, a descriptor of
finished numbers -- {table_off, form}: the byte offset of the factor's table, and in `form` the pick of the lane's
constant (8 the byte forms, 16 the wide one), the presence bit, the field's width, the total shift and the LDS offset
of the row.  Two things are checked here:

  - a descriptor IS its word: for every form, gather number, displacement, instance, row position, lane and sub-step
    the offset a lane reads and the index it forms through the descriptor are those of the index rule
    (pllhip_fused_index_dry), the index times the bytes of a table entry, and the table is the op's first table plus
    the tables of the gathers before it;
  - an encoded plan carries them: every descriptor of every record -- headers, ops, the record behind the last op --
    is the function of that record's character word, the gather's number and gather_off, for the lists the planner
    makes of a balanced 64-taxon tree, a 70-tip caterpillar (a second batch of rows) and a random 200-taxon tree, as
    they are and with their products over two cherries read as quads (one wide gather in place of two).
"""
import ctypes as C

import numpy as np
import pytest

from libpll_amd import workload as W
from test_host_gather_index import CH_WIDE, _rule
from test_host_pair_rows import CH_LTIP, CH_NIBBLE, CH_SHIFT4, _fn, _rows

CH_LOAD = 1 << 18
GD_PRESENT = 1 << 7
REC_WORDS = 13


def _entry(amd):
    return _fn(amd, "pllhip_fused_gather_desc_dry",
               [C.c_uint] * 7 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p], C.c_int)


def _desc(f, sps, ch, k, gather_off):
    d = (C.c_uint * 2)()
    assert f(sps, ch, k, gather_off, 0, 0, 0, C.cast(d, C.c_void_p), None, None, 0, 0, None) == 0, (sps, hex(ch), k)
    return d[0], d[1]


def _numbers(sps):
    w = 64 // sps
    ts = 2 * sps
    return w * 16, 256 * w * 16, (ts // 16 if ts >= 16 else 1)   # bytes of an entry, of a table; lanes per row


FORMS = {"wide": CH_LTIP | CH_WIDE, "pair": CH_LTIP, "first": CH_LTIP | CH_SHIFT4 | CH_NIBBLE, "second": CH_LTIP | CH_NIBBLE}


@pytest.mark.parametrize("sps", [4, 8, 16, 32])
def test_a_descriptor_is_its_word(amd, sps):
    # (pllhip_fused_index_dry is itself computed through the descriptor since the rule was re-expressed over it: the
    # comparison of out3 with it checks that the two entry points agree, not the rule.  What is independent here are the
    # asserts on table_off and on the form word's fields; the rule against data is tests/test_host_gather_index.py.)
    f = _entry(amd)
    _, rule = _rule(amd)
    entry, table, lpr = _numbers(sps)
    out3 = (C.c_uint * 3)()
    d2 = (C.c_uint * 2)()
    rng = np.random.default_rng(41 + sps)
    gather_off = 5 * table
    for name, bits in FORMS.items():
        if name == "wide" and sps == 4:
            continue
        for pos in (0, 1, 64 - (2 * lpr if name == "wide" else lpr)):
            for k in range(4):
                for units in range(4):
                    # (the top byte counts tables in a wide gather behind the first; in the first word it is the batch
                    # of CH_LOAD, and a byte form behind the first has none)
                    ch = bits | pos
                    if name == "wide" and k >= 1:
                        ch |= units << 24
                    elif k == 0:
                        ch |= CH_LOAD | units << 24
                    displaced = units if name == "wide" and k >= 1 else 0
                    tab, form = _desc(f, sps, ch, k, gather_off)
                    assert tab == gather_off + (k + displaced) * table, (name, k, units)
                    assert form & GD_PRESENT and (form & 31) == (16 if name == "wide" else 8)
                    assert (form >> 8) & 31 == {"wide": 16, "pair": 8}.get(name, 4)
                    assert form >> 20 == 16 * pos
                    assert 1 << ((form >> 16) & 31) == entry * (16 if name == "first" else 1)
                    for j in range(2):
                        for lane in range(64):
                            raw = int(rng.integers(0, 1 << 16))
                            want = rule(ch, sps, j, lane, raw)
                            assert f(sps, ch, k, gather_off, j, lane, raw, C.cast(d2, C.c_void_p), C.cast(out3, C.c_void_p),
                                     None, 0, 0, None) == 0
                            assert (d2[0], d2[1]) == (tab, form)
                            assert (out3[0], out3[1], out3[2]) == (want[0], want[1], want[2] * entry), (name, pos, k, j, lane)


def test_an_absent_factor_and_arguments_no_instance_has(amd):
    f = _entry(amd)
    d = (C.c_uint * 2)()
    p = C.cast(d, C.c_void_p)
    for ch in (0, CH_LOAD | 3 << 24, 5):
        assert f(8, ch, 0, 0, 0, 0, 0, p, None, None, 0, 0, None) == 0 and not d[1] & GD_PRESENT
    assert f(5, CH_LTIP, 0, 0, 0, 0, 0, p, None, None, 0, 0, None) == 1
    assert f(8, CH_LTIP, 4, 0, 0, 0, 0, p, None, None, 0, 0, None) == 1
    assert f(8, CH_LTIP, 0, 0, 2, 0, 0, p, None, None, 0, 0, None) == 1
    assert f(8, CH_LTIP, 0, 0, 0, 64, 0, p, None, None, 0, 0, None) == 1
    assert f(8, CH_LTIP, 0, 0, 0, 0, 0, None, None, None, 0, 0, None) == 1
    assert f(4, CH_LTIP | CH_WIDE, 0, 0, 0, 0, 0, p, None, None, 0, 0, None) == 1, "8 rate categories never defer: no wide form"
    assert f(8, CH_LTIP, 3, 0xffffffff - 3 * 32768 + 1, 0, 0, 0, p, None, None, 0, 0, None) == 1, "the table must fit 32 bits"
    assert f(8, CH_LTIP, 3, 0xffffffff - 3 * 32768, 0, 0, 0, p, None, None, 0, 0, None) == 0


def _encode(f, sps, forms, edge):
    forms = np.ascontiguousarray(forms, dtype=np.uint32)
    n = len(forms)
    recs = (C.c_uint * (REC_WORDS * (n + 3)))()
    rc = f(sps, 0, 0, 0, 0, 0, 0, None, None, forms.ctypes.data_as(C.c_void_p), n, int(edge), C.cast(recs, C.c_void_p))
    assert rc == 0
    return np.array(recs, dtype=np.int64).reshape(n + 3, REC_WORDS)


def _check_encoded(f, sps, forms, edge):
    """every descriptor of every record against the function of its word; the tables of an op follow each other"""
    _, table, _ = _numbers(sps)
    recs = _encode(f, sps, forms, edge)
    n = len(forms)
    assert not any(int(recs[0][5 + 2 * k + 1]) & GD_PRESENT for k in range(4)), "the first header looks ahead of op -1: nothing"
    tables = 0
    for i, r in enumerate(recs):
        gather_off = int(r[4])
        for k in range(4):
            ch = int(r[k])
            got = (int(r[5 + 2 * k]), int(r[5 + 2 * k + 1]))
            assert got == _desc(f, sps, ch, k, gather_off), (i, k)
            assert bool(got[1] & GD_PRESENT) == bool(ch & CH_LTIP)
        if 1 <= i <= n:
            # record i looks ahead to op i - 1: its gathers as the test handed them over, their tables one behind the other
            want = [int(x) for x in forms[i - 1]]
            at = gather_off
            for k in range(4):
                present = bool(int(r[5 + 2 * k + 1]) & GD_PRESENT)
                assert present == (want[k] != 0), (i, k)
                if not present:
                    continue
                assert int(r[5 + 2 * k]) == at and at == tables * table, (i, k)
                assert ((int(r[5 + 2 * k + 1]) & 31) == 16) == (want[k] > 256)
                units = want[k] - 256 if want[k] > 256 else 1
                at += units * table
                tables += units
            # (a quad's two factor tables, written for the pool's sake: behind the op's own)
            tables += 2 * sum(1 for x in want if x > 256)
    last = recs[n + 2]
    if edge:
        assert not last[:5].any() and not any(int(last[5 + 2 * k + 1]) & GD_PRESENT for k in range(4)), "the pseudo-op gathers nothing"
    else:
        assert (last == recs[n + 1]).all()
    return recs


def _forms_of(d):
    """what each walked op gathers, from the rows the planner names: both rows a pair row, one a single tip's"""
    out = np.zeros((len(d["order"]), 4), dtype=np.uint32)
    for pos, g in enumerate(d["gathers"]):
        for k, x in enumerate(g):
            first, second = int(x[0]), int(x[1])
            out[pos][k] = 3 if first and second else 1 if first else 2 if second else 0
    return out


def _with_quads(forms, units_of):
    """the products over two cherries read as quads: ONE wide gather per product side (gathers 0, 1 -> 0; 2, 3 -> 1), a
    reader of two products with both or neither"""
    out = forms.copy()
    nq = 0
    for pos, g in enumerate(forms):
        sides = [tuple(g[0:2]), tuple(g[2:4])]
        if sides[0] != (3, 3) or sides[1] not in ((3, 3), (0, 0)):
            continue
        q = [256 + units_of(nq)]
        if sides[1] == (3, 3):
            q.append(256 + units_of(nq + 1))
        nq += len(q)
        out[pos] = q + [0] * (4 - len(q))
    return out, nq


PLANS = {"balanced64": lambda: W.balanced_tree(64), "caterpillar70": lambda: W.caterpillar_tree(70),
         "random200": lambda: W.random_tree(200, seed=3)}


@pytest.mark.parametrize("name", sorted(PLANS))
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_encoded_plans_carry_the_descriptors_of_their_words(amd, name, rate_cats):
    f = _entry(amd)
    sps = 64 // (2 * rate_cats)
    d = _rows(amd, PLANS[name](), rate_cats=rate_cats)
    forms = _forms_of(d)
    for edge in (False, True):
        recs = _check_encoded(f, sps, forms, edge)
        # the words are the planner's own (pllhip_fused_plan_dry_rows), the batch switch apart
        for pos, g in enumerate(d["gathers"]):
            for k in range(4):
                assert int(recs[pos + 1][k]) & ~(CH_LOAD | 0xff000000) == int(g[k][2]), (pos, k)
        loads = [pos for pos in range(len(forms)) if int(recs[pos][0]) & CH_LOAD]
        assert [d["batch"][pos] for pos in loads] == list(range(1, d["nbatches"])), "one switch per batch, two ops ahead"
        assert all(int(recs[pos][0]) >> 24 == d["batch"][pos] for pos in loads)
    if name == "caterpillar70":
        assert d["nbatches"] >= 2, "the batch switch"
    quads, nq = _with_quads(forms, lambda i: 1 + i % 3)
    if name != "caterpillar70":
        assert nq > 0
    _check_encoded(f, sps, quads, True)


def test_the_flagship_walk(amd):
    """balanced 64 at 4 categories as the launch walks it with the quad fold: four ops over two folded quad products --
    four wide gathers each, tables of one to four units --, then two inner-inner ops; with the edge pseudo-op"""
    f = _entry(amd)
    forms = np.array([[257, 258, 260, 257], [260, 260, 260, 260], [257, 257, 257, 257], [259, 257, 258, 260], [0] * 4, [0] * 4],
                     dtype=np.uint32)
    recs = _check_encoded(f, 8, forms, True)
    # rows: a quad row is two lane positions at 4 categories; sixteen quads are 32 of the batch's 64
    assert [int(recs[pos + 1][k]) & 0xff for pos in range(4) for k in range(4)] == list(range(0, 32, 2))
    # the word's top byte: the units the gathers before it took beyond one each
    assert [int(recs[4][k]) >> 24 for k in range(1, 4)] == [2, 2, 3]
