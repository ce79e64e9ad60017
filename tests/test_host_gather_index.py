"""The index rule of the 4-state whole-list kernel, host side (no device; DESIGN.md 2.0 "Tips", "Quad rows"):
pllhip_fused_index (partials_fused.hpp) through pllhip_fused_index_dry.

A wave keeps its tile's character batch in LDS -- 64 lane positions of 16 bytes, 1 KB, as the tile's one load fetched
them -- and a lane takes the table index of its site with one read of that block: where, how wide, and what becomes of
the value read is one rule for every form of a gather.  Here the block is a numpy image; it is read at the offset and
width the rule returns, the rule forms the index of what was read, and the index must be

  - what the older dry entry points give for the same row (pllhip_fused_row_index_dry for the byte forms, the quad
    pick's pllhip_fused_quad_pick_dry for the wide one), and
  - the direct definition: the site's class, pllhip_pair_row_byte of its two characters, or the tip's code in its place,

for rate categories 1, 2, 4 and 8, both sub-steps, all 64 lanes, every form -- wide, a full byte, the low nibble with
shift 4 and with shift 0 -- and the row at the first lane position, in the middle and at the last one it fits.
"""
import ctypes as C

import numpy as np
import pytest

from test_host_pair_rows import CH_LTIP, CH_NIBBLE, CH_SHIFT4, _fn

CH_WIDE = 1 << 21
BATCH_BYTES = 1024


def _rule(amd):
    f = _fn(amd, "pllhip_fused_index_dry", [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p], C.c_int)
    out = (C.c_uint * 3)()

    def rule(ch, sps, j, lane, raw=0):
        assert f(ch, sps, j, lane, raw, C.cast(out, C.c_void_p)) == 0, (hex(ch), sps, j, lane)
        return out[0], out[1], out[2]
    return f, rule


def _read(image, offset, width):
    assert 0 <= offset and offset + width <= BATCH_BYTES and width in (1, 2)
    return int.from_bytes(image[offset:offset + width].tobytes(), "little")


def _index(rule, image, ch, sps, j, lane):
    offset, width, _ = rule(ch, sps, j, lane)
    return rule(ch, sps, j, lane, _read(image, offset, width))[2]


def _geometry(rate_cats):
    sps = 64 // (2 * rate_cats)
    ts = 2 * sps
    return sps, ts, (ts // 16 if ts >= 16 else 1)


@pytest.mark.parametrize("rate_cats", [1, 2, 4, 8])
def test_byte_forms(amd, rate_cats):
    """a cherry's pair row (every bit of the byte counts) and a single tip's row as the table's first and second
    character; raw bytes with high nibbles set, in a block whose other bytes are random"""
    sps, ts, lpr = _geometry(rate_cats)
    _, rule = _rule(amd)
    byte = _fn(amd, "pllhip_pair_row_byte_dry", [C.c_uint, C.c_uint])
    one = _fn(amd, "pllhip_fused_row_index_dry", [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint])
    rng = np.random.default_rng(11 + rate_cats)
    for pos in (0, 31, 64 - lpr):
        a = rng.integers(0, 256, ts).astype(np.uint8)
        b = rng.integers(0, 256, ts).astype(np.uint8)
        pair = np.array([byte(int(x), int(y)) for x, y in zip(a, b)], dtype=np.uint8)
        rows = {0: (pair, CH_LTIP), 1: (a, CH_LTIP | CH_SHIFT4 | CH_NIBBLE), 2: (b, CH_LTIP | CH_NIBBLE)}
        for kind, (row, bits) in rows.items():
            image = rng.integers(0, 256, BATCH_BYTES).astype(np.uint8)
            image[16 * pos:16 * pos + ts] = row
            words = np.zeros(max(ts, 16), dtype=np.uint8)
            words[:ts] = row
            for j in range(2):
                for lane in range(64):
                    site = j * sps + lane // (64 // sps)
                    got = _index(rule, image, bits | pos, sps, j, lane)
                    want = (pair[site], (int(a[site]) & 15) << 4, int(b[site]) & 15)[kind]
                    assert got == want, (rate_cats, pos, kind, j, lane)
                    assert got == one(words.ctypes.data_as(C.c_void_p), kind, sps, j, lane)


@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_wide_form(amd, rate_cats):
    """a quad row: 16-bit classes beyond 255, two planes (lanes per row) positions apart -- at the last position the second
    plane ends the block"""
    sps, ts, lpr = _geometry(rate_cats)
    _, rule = _rule(amd)
    pick = _fn(amd, "pllhip_fused_quad_pick_dry", [C.c_void_p, C.c_uint, C.c_uint, C.c_uint])
    where = _fn(amd, "pllhip_quad_row_offset_dry", [C.c_ulonglong, C.c_ulonglong], C.c_ulonglong)
    rng = np.random.default_rng(23 + rate_cats)
    last = 64 - 2 * lpr
    assert rate_cats != 4 or last == 62
    for pos in (0, 31, last):
        classes = rng.integers(0, 1024, ts).astype(np.uint16)
        classes[::3] |= 0x300
        lanes = np.zeros(2 * lpr * 16, dtype=np.uint8)
        for n in range(ts):
            off = int(where(n, lpr * 16))
            lanes[off:off + 2] = np.frombuffer(classes[n:n + 1].tobytes(), dtype=np.uint8)
        image = rng.integers(0, 256, BATCH_BYTES).astype(np.uint8)
        image[16 * pos:16 * pos + len(lanes)] = lanes
        for j in range(2):
            for lane in range(64):
                site = j * sps + lane // (64 // sps)
                offset, width, _ = rule(CH_LTIP | CH_WIDE | pos, sps, j, lane)
                assert width == 2 and offset % 2 == 0 and 16 * pos <= offset < 16 * (pos + 2 * lpr)
                got = _index(rule, image, CH_LTIP | CH_WIDE | pos, sps, j, lane)
                assert got == int(classes[site]), (rate_cats, pos, j, lane)
                assert got == pick(lanes.ctypes.data_as(C.c_void_p), sps, j, lane)
        if pos == last:
            assert max(rule(CH_LTIP | CH_WIDE | pos, sps, 1, lane)[0] for lane in range(64)) == BATCH_BYTES - 2


def test_a_displaced_gathers_top_byte_is_not_part_of_the_index(amd):
    """bits 24-31 of a later gather's word count tables, bit 18 asks for the next batch: neither moves the read"""
    _, rule = _rule(amd)
    for ch in (CH_LTIP | CH_WIDE | 5, CH_LTIP | 5, CH_LTIP | CH_NIBBLE | 5):
        for lane in (0, 9, 63):
            assert rule(ch | 7 << 24 | 1 << 18, 8, 1, lane, 0x2a5) == rule(ch, 8, 1, lane, 0x2a5)


def test_arguments_no_instance_has(amd):
    f, _ = _rule(amd)
    out = (C.c_uint * 3)()
    p = C.cast(out, C.c_void_p)
    assert f(CH_LTIP, 8, 0, 0, 0, p) == 0
    assert f(CH_LTIP, 5, 0, 0, 0, p) == 1 and f(CH_LTIP, 8, 2, 0, 0, p) == 1 and f(CH_LTIP, 8, 0, 64, 0, p) == 1
    assert f(CH_LTIP, 8, 0, 0, 0, None) == 1
    assert f(CH_LTIP | CH_WIDE, 4, 0, 0, 0, p) == 1, "8 rate categories never defer: no wide form"
    assert f(CH_LTIP | CH_WIDE | 63, 8, 1, 63, 0, p) == 1, "the second plane would lie beyond the block"
