"""Table reuse of the 4-state whole-list launch, host side (no device; DESIGN.md 2.0 "Table reuse"): the write clock of
the P-matrices (pllhip_pmat_stamp_dry: what pllhip_update_pmatrices and pllhip_put_pmatrix do per matrix) and the
staleness rule a launch of the kept plan applies (pllhip_fused_stale_jobs through pllhip_table_reuse_dry).

A job is stale where a matrix it names was written after the plan's tables were last built, or where everything is (a
new plan).  A pair job names up to three matrices (lmat, rmat, pmat), a quad -- its record of kind 4 and that of kind 5
behind it -- up to seven: cherry a's two tip matrices, cherry b's, the matrices the two factors are read with, the
reader's; a side read from a kept table names no tip matrix.  The mask is the kernels' argument: bit i, job record i.
"""
import ctypes as C

import numpy as np
import pytest

from test_host_pair_rows import _fn

NONE, UNKNOWN = 0xFFFFFFFF, 0xFFFFFFFE
MASK_JOBS = 1024


class Rule:
    """a list of job records, a set of matrices with their clock, and the clock the tables were built at"""

    def __init__(self, amd, jobs, nmats):
        self.rule = _fn(amd, "pllhip_table_reuse_dry", [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_ulonglong,
                                                        C.c_int, C.c_void_p, C.c_void_p], C.c_int)
        self.stamp = _fn(amd, "pllhip_pmat_stamp_dry", [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint], C.c_int)
        self.kinds = np.array([k for k, _ in jobs], dtype=np.uint32)
        self.mats = np.full((len(jobs), 7), NONE, dtype=np.uint32)
        for i, (_, m) in enumerate(jobs):
            self.mats[i, :len(m)] = m
        self.written = np.zeros(nmats, dtype=np.uint64)
        self.clock = C.c_ulonglong(0)
        self.built = 0

    def write(self, m):
        assert self.stamp(self.written.ctypes.data, len(self.written), C.addressof(self.clock), m) == 0

    def launch(self, new_plan=False, build=True):
        """(the records that run, out4); build: the tables count as built at the clock as it is now"""
        mask = np.zeros(16, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint32)
        rc = self.rule(self.kinds.ctypes.data, self.mats.ctypes.data, len(self.kinds), self.written.ctypes.data,
                       len(self.written), self.built, 1 if new_plan else 0, mask.ctypes.data, out.ctypes.data)
        assert rc == 0
        if build:
            self.built = self.clock.value
        runs = [i for i in range(MASK_JOBS) if (int(mask[i >> 6]) >> (i & 63)) & 1]
        assert all(i < len(self.kinds) and self.kinds[i] != 5 for i in runs), "a bit past the list, or of a second record"
        return runs, [int(v) for v in out]


def _list():
    """every kind of job over 20 matrices, each position naming a matrix of its own; 18 only a walked op names, 19 none.
    Records: 0 a tip's factor, 1 a kept tip-tip table, 2 a reader over a new cherry, 3 a reader over a kept table,
    4 + 5 a quad over two new cherries, 6 + 7 a quad whose cherry a is read from a kept table, 8 another tip's factor
    with the matrix of record 0"""
    return [(0, [0]), (1, [1, 2]), (2, [3, 4, 5]), (3, [NONE, NONE, 6]), (4, [7, 8, 9, 10, 11, 12, 13]), (5, []),
            (4, [NONE, NONE, 14, 15, 16, 17, 5]), (5, []), (0, [0])]


def test_nothing_written_nothing_stale(amd):
    r = Rule(amd, _list(), 20)
    for m in range(20):
        r.write(m)
    runs, out = r.launch(new_plan=True)
    assert runs == [0, 1, 2, 3, 4, 6, 8] and out == [7, 0, 1, 1], "a new plan: every job, both launches; kind 5 is no job"
    for _ in range(3):
        assert r.launch() == ([], [0, 7, 0, 0])


def test_a_write_makes_the_jobs_that_name_the_matrix_stale(amd):
    """each of the seven positions of a quad, the three of a pair job, and the jobs that share a matrix"""
    jobs = _list()
    readers = {m: [i for i, (k, ms) in enumerate(jobs) if m in ms] for m in range(20)}
    assert readers[0] == [0, 8] and readers[5] == [2, 6] and readers[18] == readers[19] == []
    assert [readers[m] for m in range(7, 14)] == [[4]] * 7 and [readers[m] for m in (3, 4, 5)][:2] == [[2], [2]]
    r = Rule(amd, jobs, 20)
    r.launch(new_plan=True)
    for m in range(20):
        r.write(m)
        runs, out = r.launch()
        pair = any(jobs[i][0] < 4 for i in readers[m])
        quad = any(jobs[i][0] == 4 for i in readers[m])
        assert runs == readers[m], (m, runs)
        assert out == [len(readers[m]), 7 - len(readers[m]), int(pair), int(quad)], (m, out)
        assert r.launch() == ([], [0, 7, 0, 0]), "built: good until the next write"


def test_same_index_written_twice_and_writes_that_pile_up(amd):
    r = Rule(amd, _list(), 20)
    r.launch(new_plan=True)
    r.write(9)
    r.write(9)
    assert r.clock.value == 2 and r.written[9] == 2, "a write is a write"
    assert r.launch()[0] == [4]
    assert r.launch()[0] == []
    # (writes before a launch that builds nothing -- the rule asked without a launch -- stay stale; more pile up)
    r.write(1)
    assert r.launch(build=False)[0] == [1]
    r.write(6)
    r.write(1)
    assert r.launch()[0] == [1, 3]
    assert r.launch()[0] == []


def test_new_plan_makes_every_job_stale(amd):
    r = Rule(amd, _list(), 20)
    assert r.launch(new_plan=True)[0] == [0, 1, 2, 3, 4, 6, 8], "no matrix was ever written"
    assert r.launch()[0] == []
    r.write(18)
    assert r.launch()[0] == []
    runs, out = r.launch(new_plan=True)
    assert runs == [0, 1, 2, 3, 4, 6, 8] and out == [7, 0, 1, 1]
    # a matrix the clock does not cover: stale at every launch
    r.mats[3, 2] = UNKNOWN
    assert r.launch() == ([3], [1, 6, 1, 0])
    assert r.launch() == ([3], [1, 6, 1, 0])


def test_only_quads_or_only_pairs(amd):
    r = Rule(amd, [(4, [0, 1, 2, 3, 4, 5, 6]), (5, []), (2, [7, 8, 9])], 10)
    r.launch(new_plan=True)
    r.write(4)
    assert r.launch() == ([0], [1, 1, 0, 1])
    r.write(8)
    assert r.launch() == ([2], [1, 1, 1, 0])
    empty = Rule(amd, [], 4)
    assert empty.launch(new_plan=True) == ([], [0, 0, 0, 0])


@pytest.mark.parametrize("njobs", [MASK_JOBS, MASK_JOBS + 1, 3 * MASK_JOBS])
def test_more_jobs_than_the_mask_holds(amd, njobs):
    """up to 1,024 records the mask names each; beyond, the list runs all or nothing"""
    r = Rule(amd, [(0, [i % 50]) for i in range(njobs)], 50)
    runs, out = r.launch(new_plan=True)
    assert runs == list(range(MASK_JOBS)) and out == [njobs, 0, 1, 0]
    assert r.launch() == ([], [0, njobs, 0, 0])
    r.write(7)
    runs, out = r.launch()
    if njobs <= MASK_JOBS:
        assert runs == list(range(7, njobs, 50)) and out == [len(runs), njobs - len(runs), 1, 0]
    else:
        assert runs == list(range(MASK_JOBS)) and out == [njobs, 0, 1, 0], "all"
    assert r.launch() == ([], [0, njobs, 0, 0]), "or nothing"


def test_out_of_range_arguments_are_refused(amd):
    r = Rule(amd, _list(), 20)
    mask = np.zeros(16, dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint32)

    def rc(kinds=r.kinds, mats=r.mats, njobs=None, written=r.written, nmats=20, mask=mask, out=out):
        p = lambda a: None if a is None else a.ctypes.data
        return r.rule(p(kinds), p(mats), len(kinds) if njobs is None else njobs, p(written), nmats, 0, 0, p(mask), p(out))

    assert rc() == 0
    assert rc(out=None) == 1 and rc(mask=None) == 1 and rc(kinds=None, njobs=9) == 1 and rc(mats=None) == 1
    assert rc(written=None) == 1
    bad = r.mats.copy()
    bad[2, 1] = 20
    assert rc(mats=bad) == 1, "a matrix index past the clock's"
    kinds = r.kinds.copy()
    kinds[0] = 6
    assert rc(kinds=kinds) == 1
    kinds = r.kinds.copy()
    kinds[5] = 0
    assert rc(kinds=kinds) == 1, "a quad without its second record"
    kinds = r.kinds.copy()
    kinds[0] = 5
    assert rc(kinds=kinds) == 1, "a second record without its quad"
    assert rc(kinds=r.kinds[:5], mats=r.mats[:5]) == 1, "the list ends on a record of kind 4"
    clock = C.c_ulonglong(3)
    assert r.stamp(r.written.ctypes.data, 20, C.addressof(clock), 20) == 1 and clock.value == 3
    assert r.stamp(None, 20, C.addressof(clock), 0) == 1 and r.stamp(r.written.ctypes.data, 20, None, 0) == 1
    assert not r.written.any()
