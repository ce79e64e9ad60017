"""What the 4-state whole-list kernel does in scalar registers, run on the host (no device): the group mask of the
scaling rule (pllhip_fused_group_mask_dry), the count bit a lane takes for its entry of the tile
(pllhip_fused_entry_bit_dry) and the pair-table index formed from two tip rows' words (pllhip_fused_pair_index_dry) --
the kernel's own functions (partials_fused.hpp), each against a loop over lanes or bytes.
"""
import ctypes as C

import numpy as np
import pytest

ALL = (1 << 64) - 1
J = 2  # sub-steps per tile (PLLHIP_FUSED_J)


def _group_mask(amd, gw, mask):
    f = amd.lib.pllhip_fused_group_mask_dry
    f.restype = C.c_ulonglong
    f.argtypes = [C.c_uint, C.c_ulonglong]
    return int(f(gw, mask))


def _per_lane(gw, mask):
    """every lane of a group set exactly where all gw lanes of the group are set"""
    out = 0
    for lane in range(64):
        base = lane - lane % gw
        if all((mask >> l) & 1 for l in range(base, base + gw)):
            out |= 1 << lane
    return out


@pytest.mark.parametrize("gw", [2, 4, 8, 16])
def test_group_mask_deterministic(amd, gw):
    group = (1 << gw) - 1
    masks = [ALL, 0]
    masks += [group << (g * gw) for g in range(64 // gw)]         # each single group full
    masks += [ALL & ~(1 << lane) for lane in range(64)]           # each single lane missing
    for m in masks:
        got = _group_mask(amd, gw, m)
        assert got == _per_lane(gw, m), "gw %d mask %016x: %016x" % (gw, m, got)
    assert _group_mask(amd, gw, ALL) == ALL and _group_mask(amd, gw, 0) == 0
    for lane in range(64):
        base = lane - lane % gw
        assert _group_mask(amd, gw, ALL & ~(1 << lane)) == ALL & ~(group << base)


@pytest.mark.parametrize("gw", [2, 4, 8, 16])
def test_group_mask_random(amd, gw):
    rng = np.random.default_rng(1000 + gw)
    # dense masks (few lanes missing, so that whole groups survive) and uniform ones
    for density in (0.5, 0.8, 0.95, 0.99):
        for _ in range(750):
            bits = rng.random(64) < density
            m = int(sum(1 << i for i in range(64) if bits[i]))
            assert _group_mask(amd, gw, m) == _per_lane(gw, m), "gw %d mask %016x" % (gw, m)
    # the base bit the count extraction reads is the group's decision
    m = int(rng.integers(0, 1 << 63)) | (((1 << gw) - 1) << gw)
    got = _group_mask(amd, gw, m)
    assert (got >> gw) & 1 == 1


def test_group_mask_other_widths(amd):
    for gw in (0, 1, 3, 32, 64):
        assert _group_mask(amd, gw, ALL) == 0


@pytest.mark.parametrize("gw", [2, 4, 8, 16])
def test_entry_bit(amd, gw):
    """Entry t of a tile is group t % EPS of sub-step t / EPS: its count bit is that group's decision."""
    f = amd.lib.pllhip_fused_entry_bit_dry
    f.restype = C.c_uint
    f.argtypes = [C.c_uint, C.c_ulonglong, C.c_ulonglong, C.c_uint]
    rng = np.random.default_rng(2000 + gw)
    eps = 64 // gw
    for trial in range(200):
        below = [int(sum(1 << i for i in range(64) if rng.random() < 0.9)) for _ in range(J)]
        if trial == 0:
            below = [ALL, 0]
        elif trial == 1:
            below = [0, ALL]
        groups = [_group_mask(amd, gw, m) for m in below]
        for t in range(J * eps):
            want = (_per_lane(gw, below[t // eps]) >> ((t % eps) * gw)) & 1
            assert int(f(gw, groups[0], groups[1], t)) == want, (gw, trial, t)
    assert int(f(gw, 0, 0, J * eps)) == 0xffffffff and int(f(3, 0, 0, 0)) == 0xffffffff


def _pair_index(amd, row_a, row_b, lmask4, rmask4, sps, sub_step, lane):
    f = amd.lib.pllhip_fused_pair_index_dry
    f.restype = C.c_uint
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint]
    wa = np.ascontiguousarray(row_a, dtype=np.uint8).view("<u4")
    wb = np.ascontiguousarray(row_b, dtype=np.uint8).view("<u4")
    return int(f(wa.ctypes.data_as(C.c_void_p), wb.ctypes.data_as(C.c_void_p), lmask4, rmask4, sps, sub_step, lane))


@pytest.mark.parametrize("sps", [4, 8, 16, 32])
def test_pair_index(amd, sps):
    """Every lane, both sub-steps (the first and the last word of a row among them), all four mask combinations:
    (row_a[site] & lm) << 4 | (row_b[site] & rm), byte by byte."""
    rng = np.random.default_rng(sps)
    w = 64 // sps                    # lanes per site
    ts = J * sps                     # characters of a tile's row
    for trial in range(8):
        row_a = rng.integers(0, 16, ts, dtype=np.uint8)
        row_b = rng.integers(0, 16, ts, dtype=np.uint8)
        if trial == 0:               # the extremes: no byte may carry into its neighbour
            row_a[:], row_b[:] = 15, 15
        for lm, rm in ((15, 15), (15, 0), (0, 15), (0, 0)):
            for sub in range(J):
                for lane in range(64):
                    site = sub * sps + lane // w
                    want = ((int(row_a[site]) & lm) << 4) | (int(row_b[site]) & rm)
                    got = _pair_index(amd, row_a, row_b, lm * 0x01010101, rm * 0x01010101, sps, sub, lane)
                    assert got == want, (sps, trial, lm, rm, sub, lane, got, want)
    # sites in the first and in the last word of a row are among the above
    assert (0 * sps + 0 // w) // 4 == 0 and ((J - 1) * sps + 63 // w) // 4 == ts // 4 - 1


def test_pair_index_bad_arguments(amd):
    row = np.zeros(64, dtype=np.uint8)
    bad = 0xffffffff
    assert _pair_index(amd, row, row, 0, 0, 5, 0, 0) == bad
    assert _pair_index(amd, row, row, 0, 0, 8, J, 0) == bad
    assert _pair_index(amd, row, row, 0, 0, 8, 0, 64) == bad
