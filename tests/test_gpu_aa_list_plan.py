"""The 20-state list, live and dry: ONE set of functions (fused_plan.hip: pllhip_aa_list_classify, _cert, _walk).

pllhip_aa_fused_update plans a new list with the functions the device-less pllhip_aa_list_plan_dry runs, so what the
dry call says of a list -- how many ops of each class, how many operands reloaded, whether anything tests under the
scaling certificate -- is what the live call does.  The live side is read through the counters the library already
has: pll_amd_list_kinds and pll_amd_scaling_certificate.

Balanced 16 x 40 sites (lookups over two cherries), caterpillar 12 x 40 (a tip-inner chain, a tip-inner lookup) and
random 40 x 33 (operands reloaded), character rows at the tips, per-site scale buffers, PLLHIP_FUSED=2.  A full
traversal, then a partial one of the last three ops on top: its operands carry the marks the first list left, which
the dry call gets as the first dry call's outgoing bounds.
"""
import pytest

from helpers import make_case, build_partition
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
from test_host_aa_list_plan import aa_dry

pytestmark = pytest.mark.gpu

KINDS = ("ops", "tip_tip_ahead", "tip_tip_in_list", "lookups", "inner_inner_matrix_cores", "tip_inner_matrix_cores",
         "tip_inner_vector_unit", "reloads")


@pytest.mark.parametrize("shape,tips,sites", [("balanced", 16, 40), ("caterpillar", 12, 40), ("random", 40, 33)])
@pytest.mark.parametrize("ti_mfma", ["0", "1"])
@pytest.mark.parametrize("segments", [None, "0"])
@pytest.mark.parametrize("lookup_mb", [None, "3"])
def test_live_list_is_what_the_dry_call_says(gpu, monkeypatch, shape, tips, sites, ti_mfma, segments, lookup_mb):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    monkeypatch.setenv("PLLHIP_AA_TI_MFMA", ti_mfma)
    for name, value in (("PLLHIP_FUSED_SEGMENTS", segments), ("PLLHIP_AA_LOOKUP_MB", lookup_mb), ("PLLHIP_AA_CHERRY", None),
                        ("PLLHIP_AA_TT_INSIDE", None), ("PLLHIP_AA_TT_PAIRS", None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    case = make_case(20, shape, tips, sites, seed=11)
    case["rates"], case["freqs"] = gpu.aa_model("lg")
    plan = case["plan"]
    p = build_partition(gpu, case, ATTRIB_PATTERN_TIP)
    # the switches as the library reads them: a table set is 4 x (codes^2 + 64) rows of 4 x 20 doubles; by default
    # 64 MB of them at these sizes (1/16 of the CLVs adds nothing); up to eight segments while the tiles are few
    table_set = 4 * (p.s.maxstates ** 2 + 64) * 4 * 20 * 8
    budget = ((64 if lookup_mb is None else int(lookup_mb)) << 20) // table_set
    max_segments = 8 if segments is None else 1
    incoming, lists = None, 0
    for ops in (plan.ops, plan.ops[-3:]):
        dry = aa_dry(gpu, ops, plan, lookups_max=budget, tt_inside=1, ti_mfma=int(ti_mfma), max_segments=max_segments,
                     incoming=incoming)
        assert dry["rc"] == 0
        p.update_partials(ops)
        live, cert = p.list_kinds(), p.scaling_certificate()
        print("%s %d, %d ops: dry %r cert_kind %d; live %r, certificate %r" %
              (shape, tips, len(ops), dry["kinds"], dry["cert_kind"], live, cert))
        assert [live[k] for k in KINDS] == dry["kinds"]
        lists += dry["cert_kind"] != 0
        assert cert["lists"] == lists and cert["uncertified"] == 0
        incoming = dry["bounds"]
        if len(ops) == len(plan.ops) and shape == "balanced":
            # (the case is meant to meet its budget: four ops over two cherries, 3 MB hold two table sets)
            assert dry["kinds"][3] == (4 if lookup_mb is None else 2) and budget == (44 if lookup_mb is None else 2)
    p.destroy()
