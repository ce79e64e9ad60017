"""Host side of pll_amd_model_loglikelihood, without a device: the symbol, the candidate structure's layout, and the
eigen systems a candidate's sets get -- pll_amd_eigen_decompose, the routine behind pll_update_eigen, on the sets
tests/test_host.py pins against the reference's decomposition."""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal
from libpll_amd.pllapi import ModelCandidate, model_candidates


def test_library_exports_the_symbol(amd):
    assert hasattr(amd.lib, "pll_amd_model_loglikelihood")
    assert hasattr(amd.lib, "pllhip_model_loglikelihood")


def test_candidate_structure_is_five_pointers():
    assert C.sizeof(ModelCandidate) == 5 * C.sizeof(C.c_void_p)
    arr, keep = model_candidates([{}, dict(subst_params=[None, np.ones(6)], prop_invar=[0.0, 0.1])])
    assert not any(getattr(arr[0], name) for name, _ in ModelCandidate._fields_)
    assert arr[1].subst_params and arr[1].prop_invar and not arr[1].frequencies and not arr[1].category_rates
    ptrs = C.cast(arr[1].subst_params, C.POINTER(C.c_void_p))
    assert not ptrs[0] and ptrs[1] == keep[0][1].ctypes.data


def _decompose(amd, states, params, freqs):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    v, ev, inv = np.zeros(states), np.zeros((states, states)), np.zeros((states, states))
    ok = amd.lib.pll_amd_eigen_decompose(states, dp(np.ascontiguousarray(params, dtype=np.float64)),
                                         dp(np.ascontiguousarray(freqs, dtype=np.float64)), dp(v), dp(ev), dp(inv))
    return ok, v, ev, inv


@pytest.mark.parametrize("states", [4, 20])
def test_candidate_eigen_system_is_the_reference_decomposition(amd, ref, states):
    """the draws of tests/test_host.py::test_eigen_solver_bit_exact: a candidate that gives such a set gets the arrays
    the reference's pll_update_eigen leaves in a partition"""
    rng = np.random.default_rng(states)
    for trial in range(3):
        params = rng.uniform(0.2, 5.0, states * (states - 1) // 2)
        freqs = rng.dirichlet(np.ones(states) * 5)
        if states == 20 and trial == 0:
            params, freqs = ref.aa_model("lg")
        p = ref.partition_create(2, 1, states, 4, 1, 1, 4, 0, 0)
        p.set_subst_params(0, params)
        p.set_frequencies(0, freqs)
        p.update_eigen(0)
        v, ev, inv = p.get_eigen(0)
        p.destroy()
        ok, v2, ev2, inv2 = _decompose(amd, states, params, freqs)
        assert ok
        assert bits_equal(v, v2) and bits_equal(ev, ev2) and bits_equal(inv, inv2)


def test_all_zero_exchangeabilities_do_not_converge(amd):
    """finite and non-negative, so they pass the value checks: the call refuses the candidate by its decomposition"""
    ok, _, _, _ = _decompose(amd, 4, np.zeros(6), np.full(4, 0.25))
    assert not ok
    assert amd.errno() == 113
