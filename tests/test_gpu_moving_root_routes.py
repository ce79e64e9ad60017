"""A root that moves, on every route pll_update_partials has (tests/moving_root.py: the driver and what it checks per
move; tests/unstored_state_data.py: the walks; tests/test_gpu_unstored_state.py, part D, is the same walk on the
4-state whole-list kernel with pattern tips).  60 moves after a full traversal; nearly every list reads operands that
earlier calls wrote -- kept plans, operands reloaded from HBM, scaler counts inherited from earlier launches, the
scaling certificate's bounds carried from list to list, the row maps of site repeats.

Each case asserts its route from the library's own counters:
  a, b  20 states, 4 categories, PLLHIP_FUSED=2 (partials_aa_fused.hip), 45 sites -- a workgroup tile of 32, a wave
        tile of 8, a sub-tile of 4 and one site.  On the matrix cores (aa_mode mfma, mfma-reference-order)
        pll_amd_list_kinds after every planned list equals `kinds` of pllhip_aa_list_plan_dry for that list, with the
        bounds carried from list to list (moving_root.plan_lists; tests/test_moving_root_route_lists.py asserts the
        same lists' conditions without a device), and pll_amd_scaling_certificate's `lists` equals the number of lists
        the dry calls give a certificate kind other than 0, one-op lists (per level) included.  aa_mode exact: the
        kernel's gate refuses the partition -- nothing is ever planned (list_kinds all zero) and every list takes at
        least as many profiled launches as it has dependency levels: the 20-state per-level route at 4 categories.
  c     20 states, 3 and 8 categories (chunked, partials_aa_mfma.hip): nothing planned, launches >= levels.
  d     4 states, PLLHIP_FUSED=0 (partials.hip): launches >= levels; a list with a tip-tip or tip-inner op has a
        launch of that kind.
  e     4 states, PLLHIP_FUSED=2 (partials_fused.hip): ONE launch per list of two or more ops, counted as inner-inner.
  f     5, 13, 61 states (partials_gen_tile.hip): launches >= levels.
  g     site repeats: most CLVs of the walk's lists are stored by class (pll_amd_repeats_classes); a plain partition
        runs the same calls, every result equal bit for bit.
  h     two shards of one device (pll_amd_shard_count == 2; a shard begins on a multiple of 256 sites, so 256 + 45
        sites) against the unsharded partition; list_kinds and the certificate as in (a) on both.
A whole-list launch is one profiled launch whatever the list: "launches >= levels" on at least 30 lists of two or more
levels is what a per-level route alone can give.

Measured on one MI355X (256 CUs); none of the seeds had to be replaced; the whole file takes 5.4 s.
a, b, h -- over the planned lists (two or more ops) after move 0: planned / with reloads / with lookups / with a tip-tip
op / with a tip-inner op on the matrix cores / of two ops; certificate kind 1 / 2 / 0; then the certificate's `lists`
at the end of the walk (one-op lists and replays included) and the largest CLV error against the oracle, mode mfma:
    random 17, seed 5, pattern tips    52 50 20 26 36 4    36 11  5    58   9.0e-16
      the same, per-rate buffers       52 50 20 26 36 4    36 11  5    58   9.0e-16
      the same, no scale buffers       52 50 20 26 36 4     0  0 52     0   9.0e-16
      the same, tip CLVs               52 52  0  0  0 4     0  0 52     0   0 (bit for bit)
      the same at 1e-40 (b)            52 50 20 26 36 4    36 11  5    58   6.3e-16   51 moves with counts at both ends
    random 20, seed 16                 53 53 12 24 39 8    39 12  2    66   9.7e-16
      the same, 301 sites (h)          53 53 12 24 39 8    39 12  2    66   1.1e-15   the two shards: 132
    balanced 16, seed 7                55 55  0 35 36 7    36  0 19    38   5.1e-16
  mfma-reference-order: the same lists with no tip-inner op on the matrix cores, certificate kind 0 throughout, `lists`
  0, every CLV bit for bit.  The largest bound the planner keeps: 4.4e-14 (random 20).  No certificate was raised.
Per level -- lists (replays included) of two or more levels, each in at least as many launches: 20 states exact 62 /
61 / 64 (random 17 / random 20 / balanced 16), 3 and 8 categories 62; 4 states 61; 5, 13 and 61 states 62.  4 states
on the whole-list kernel: 61 such lists, one launch each.  Every CLV bit for bit.
Site repeats: 322 of 322 CLVs written are stored by class, in 7 (4 states) and 6 (20 states) rows at the most.
Largest errors against the oracle over all cases: lnL 7.7e-16, per site 3.0e-16, sumtable 1.3e-15, derivatives 4.9e-12
(20 states with site repeats; 4 states 3.0e-13).
"""
import pytest

import moving_root as M
import unstored_state_data as U
from helpers import make_case, odd_state_case, many_state_case, repeat_columns
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_SITE_REPEATS

pytestmark = pytest.mark.gpu

PT, RS = ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
AA_SITES, DNA_SITES, GEN_SITES = 45, 40, 37
RANDOM17, RANDOM20, BALANCED16 = U.WALKS[:3]
PARTIALS = ("partials_ii", "partials_ti", "partials_tt")


def _case(gpu, states, walk_id, rate_cats=4, seed=None, sites=None):
    shape, tips, tree_seed = walk_id
    seed = tree_seed if seed is None else seed
    if states in (4, 20):
        case = make_case(states, shape, tips, sites or (AA_SITES if states == 20 else DNA_SITES), rate_cats=rate_cats, seed=seed)
        if states == 20:
            case["rates"], case["freqs"] = gpu.aa_model("lg")
    elif states > 32:
        case = many_state_case(states, tips=tips, sites=GEN_SITES, seed=seed, shape=shape, rate_cats=rate_cats)
    else:
        case = odd_state_case(states, tips=tips, sites=GEN_SITES, seed=seed, shape=shape, rate_cats=rate_cats)
    return case


def _report(name, figures, extra=""):
    print("%s: largest errors against the oracle: lnL %.2e, per site %.2e, sumtable %.2e, derivatives %.2e, CLV %.2e; "
          "%d moves with counts at both ends of the root edge%s"
          % (name, figures["lnl"], figures["persite"], figures["sumtable"], figures["deriv"], figures["clv"],
             figures["scaled"], extra))


# ---- route evidence

class Launches:
    """the profiled launches of every list (pll_amd_profile_read counts the launches of pll_update_partials under
    three kinds and nothing else under them)"""

    def __init__(self, p, tips, pattern_tip):
        self.p, self.tips, self.pattern_tip = p, tips, pattern_tip
        self.seen = []      # (ops, dependency levels, {kind: launches})
        p.profile_enable(True)
        p.profile_read()

    def __call__(self, k, mv, replay):
        prof = self.p.profile_read()
        self.seen.append((mv["ops"], M.levels_of(mv["ops"]), {name: prof[name][0] for name in PARTIALS}))

    def per_level(self):
        deep = 0
        for ops, levels, n in self.seen:
            assert sum(n.values()) >= levels, "a list of %d levels in %r launches" % (levels, n)
            deep += levels >= 2
            if self.pattern_tip:
                tt, other = U.kinds_of(ops, self.tips)
                ti = sum(1 for op in ops if (int(op["child1_clv_index"]) < self.tips) != (int(op["child2_clv_index"]) < self.tips))
                assert (n["partials_tt"] > 0) == (tt > 0) and (n["partials_ti"] > 0) == (ti > 0), (tt, ti, n)
        assert deep >= 30, "lists of two or more levels: %d" % deep
        return deep

    def whole_list(self):
        many = 0
        for ops, levels, n in self.seen:
            if len(ops) >= 2:
                assert n == dict(partials_ii=1, partials_ti=0, partials_tt=0), (len(ops), levels, n)
                many += levels >= 2
        assert many >= 30, "lists of two or more levels: %d" % many
        return many


class AaLists:
    """20 states on the whole-list kernel: what the library planned against the dry calls, list by list"""

    def __init__(self, gpu, w, pattern_tip, ti_mfma, certificate=True):
        self.p, self.certificate = w.p, certificate
        self.dry = M.plan_lists(gpu, w.plan, w.moves, pattern_tip=pattern_tip, ti_mfma=ti_mfma)
        self.counts = M.list_counts(self.dry, w.moves)
        self.last, self.cert_lists, self.checked = [0] * 8, 0, 0

    def __call__(self, k, mv, replay):
        d = self.dry[k]
        live = self.p.list_kinds()
        if d["planned"]:
            self.last = d["kinds"]
            self.checked += 1
        # (a list of one op goes per level: the kernel's last plan stands)
        assert [live[name] for name in M.KINDS] == self.last, "move %d%s: planned %r, the dry call %r" % (
            k, ", replayed" if replay else "", live, self.last)
        self.cert_lists += d["cert_kind"] != 0
        if self.certificate:
            assert self.p.scaling_certificate()["lists"] == self.cert_lists, (k, replay, self.p.scaling_certificate())

    def finish(self):
        cert = self.p.scaling_certificate()
        assert cert["uncertified"] == 0, cert
        # (a certificate that is raised runs its list again in the reference's order: the bounds the dry calls carry
        # would no longer be the library's)
        assert cert["raised"] == 0 and cert["rerun"] == 0, cert
        assert self.checked >= 45
        return cert


def _nothing_planned(p):
    assert not any(p.list_kinds().values()), "the 20-state whole-list kernel planned a list: %r" % p.list_kinds()


# ---- a, b: 20 states, 4 categories, the whole-list kernel forced

def _aa_walk(gpu, orc, monkeypatch, aa_mode, name, walk_id, attrs, scalers=True, branch=None, seed=None):
    w = M.RootWalk(gpu, orc, _case(gpu, 20, walk_id, seed=seed), attrs, M.walk(*walk_id, scalers=scalers, branch=branch),
                   monkeypatch, env={"PLLHIP_FUSED": "2"})
    pattern = bool(attrs & PT)
    if aa_mode == "exact":
        evidence = Launches(w.p, w.plan.tips, pattern)
        figures = w.run(evidence)
        _nothing_planned(w.p)
        extra = "; per level, %d lists of two or more levels" % evidence.per_level()
    else:
        evidence = AaLists(gpu, w, pattern, 1 if aa_mode == "mfma" else 0)
        M.check_conditions(evidence.counts, walk_id[0], pattern, aa_mode == "mfma")
        figures = w.run(evidence)
        extra = "; %r, certificate %r" % (evidence.counts, evidence.finish())
    assert w.p.scaling_certificate()["uncertified"] == 0
    w.destroy()
    _report("20 states, %s, %s" % (name, aa_mode), figures, extra)
    return figures


AA_WALKS = [pytest.param(RANDOM17, PT, True, id="random17"), pytest.param(RANDOM20, PT, True, id="random20"),
            pytest.param(BALANCED16, PT, True, id="balanced16"), pytest.param(RANDOM17, 0, True, id="random17-tip-clvs"),
            pytest.param(RANDOM17, PT | RS, True, id="random17-per-rate"),
            pytest.param(RANDOM17, PT, False, id="random17-no-scale-buffers")]


@pytest.mark.parametrize("walk_id,attrs,scalers", AA_WALKS)
def test_aa_whole_list(gpu, orc, monkeypatch, aa_mode, request, walk_id, attrs, scalers):
    _aa_walk(gpu, orc, monkeypatch, aa_mode, request.node.callspec.id, walk_id, attrs, scalers=scalers)


@pytest.mark.parametrize("mode", ["mfma", "exact"])
@pytest.mark.parametrize("attrs", [pytest.param(PT, id="per-site"), pytest.param(PT | RS, id="per-rate")])
def test_aa_whole_list_scaling(gpu, orc, monkeypatch, mode, attrs):
    """every branch at 1e-40: the counts at the root edge's ends are sums of counts left by earlier lists"""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "1" if mode == "exact" else "0")
    monkeypatch.setenv("PLLHIP_AA_TI_MFMA", "1")
    monkeypatch.setenv("PLLHIP_AA_CHERRY", "2")
    figures = _aa_walk(gpu, orc, monkeypatch, mode, "random17 at 1e-40, attributes %d" % attrs, RANDOM17, attrs, branch=1e-40)
    assert figures["scaled"] >= 10, "moves with non-zero counts at both ends of the root edge"


# ---- c: 20 states, 3 and 8 categories

@pytest.mark.parametrize("attrs", [pytest.param(PT, id="pattern-tips"), pytest.param(0, id="tip-clvs")])
@pytest.mark.parametrize("rate_cats", [3, 8])
def test_aa_chunked_categories(gpu, orc, monkeypatch, rate_cats, attrs):
    # (the matrix-core kernels, in the reference's order: every CLV bit for bit)
    env = {"PLLHIP_FUSED": "2", "PLLHIP_AA_EXACT": "0", "PLLHIP_AA_TI_MFMA": "0"}
    w = M.RootWalk(gpu, orc, _case(gpu, 20, RANDOM17, rate_cats=rate_cats), attrs, M.walk(*RANDOM17), monkeypatch, env=env)
    assert w.exact
    evidence = Launches(w.p, w.plan.tips, bool(attrs & PT))
    figures = w.run(evidence)
    _nothing_planned(w.p)
    deep = evidence.per_level()
    w.destroy()
    _report("20 states, %d categories, attributes %d" % (rate_cats, attrs), figures, "; %d lists of two or more levels" % deep)


# ---- d, e: 4 states

@pytest.mark.parametrize("attrs", [pytest.param(PT, id="pattern-tips"), pytest.param(0, id="tip-clvs")])
@pytest.mark.parametrize("rate_cats", [4, 3])
def test_dna_per_level(gpu, orc, monkeypatch, rate_cats, attrs):
    w = M.RootWalk(gpu, orc, _case(gpu, 4, RANDOM20, rate_cats=rate_cats), attrs, M.walk(*RANDOM20), monkeypatch,
                   env={"PLLHIP_FUSED": "0"})
    evidence = Launches(w.p, w.plan.tips, bool(attrs & PT))
    figures = w.run(evidence)
    deep = evidence.per_level()
    assert w.p.deferred_stats()["ops_deferred"] == 0
    w.destroy()
    _report("4 states per level, %d categories, attributes %d" % (rate_cats, attrs), figures, "; %d lists of two or more levels" % deep)


@pytest.mark.parametrize("rate_cats,attrs", [pytest.param(4, 0, id="tip-clvs"), pytest.param(8, PT, id="8-categories"),
                                             pytest.param(4, PT | RS, id="per-rate")])
def test_dna_whole_list(gpu, orc, monkeypatch, dna_path, rate_cats, attrs):
    """the cases part D of tests/test_gpu_unstored_state.py leaves out; dna_path `levels` is the same walk per level"""
    w = M.RootWalk(gpu, orc, _case(gpu, 4, RANDOM20, rate_cats=rate_cats), attrs, M.walk(*RANDOM20), monkeypatch)
    evidence = Launches(w.p, w.plan.tips, bool(attrs & PT))
    figures = w.run(evidence)
    deep = evidence.per_level() if dna_path == "levels" else evidence.whole_list()
    w.destroy()
    _report("4 states, %s, %d categories, attributes %d" % (dna_path, rate_cats, attrs), figures, "; %d lists of two or more levels" % deep)


# ---- f: generic states

@pytest.mark.parametrize("states,rate_cats,attrs", [
    pytest.param(5, 3, PT, id="5x3-pattern-tips"), pytest.param(5, 3, 0, id="5x3-tip-clvs"),
    pytest.param(13, 4, PT | RS, id="13x4-pattern-tips-per-rate"), pytest.param(13, 4, 0, id="13x4-tip-clvs"),
    pytest.param(61, 2, 0, id="61x2-tip-clvs")])
def test_generic_states(gpu, orc, monkeypatch, states, rate_cats, attrs):
    w = M.RootWalk(gpu, orc, _case(gpu, states, RANDOM17, rate_cats=rate_cats), attrs, M.walk(*RANDOM17), monkeypatch)
    evidence = Launches(w.p, w.plan.tips, bool(attrs & PT))
    figures = w.run(evidence)
    deep = evidence.per_level()
    w.destroy()
    _report("%d states, %d categories, attributes %d" % (states, rate_cats, attrs), figures, "; %d lists of two or more levels" % deep)


# ---- g: site repeats

@pytest.mark.parametrize("states", [4, 20])
def test_site_repeats(gpu, orc, monkeypatch, states):
    """columns from a pool of 8: the partition with site repeats next to the oracle, a plain one next to it"""
    case = _case(gpu, states, RANDOM17)
    repeat_columns(case, seed=states, distinct=8)
    env = {"PLLHIP_AA_EXACT": "0", "PLLHIP_AA_TI_MFMA": "0"}      # (as tests/test_gpu_repeats.py pins it)
    w = M.RootWalk(gpu, orc, case, PT | ATTRIB_SITE_REPEATS, M.walk(*RANDOM17), monkeypatch, env=env,
                   second=dict(attrs=PT, lnl_rtol=0.0))
    assert w.exact
    by_class = []

    def classes(k, mv, replay):
        by_class.extend(w.p.repeats_classes(int(op["parent_clv_index"])) for op in mv["ops"])
        assert all(w.q.repeats_classes(int(op["parent_clv_index"])) == 0 for op in mv["ops"])
    figures = w.run(classes)
    stored = sum(1 for c in by_class if c)
    assert all(c <= case["sites"] // 2 for c in by_class)
    assert stored >= len(by_class) // 2, "%d of %d CLVs written were stored by class" % (stored, len(by_class))
    w.destroy()
    _report("%d states, site repeats" % states, figures, "; %d of %d CLVs written stored by class, %d rows at the most"
            % (stored, len(by_class), max(by_class)))


# ---- h: two shards

def test_aa_two_shards(gpu, orc, monkeypatch):
    """the 20-tip walk, 20 states on the whole-list kernel: two shards of one device against the unsharded partition
    (per-site values bit for bit, lnL to 1e-12), the unsharded one against the oracle.  A shard begins on a multiple of
    256 sites (shard.hip): 256 + 45 sites, the second shard with the tails of the other cases."""
    env = {"PLLHIP_FUSED": "2", "PLLHIP_AA_EXACT": "0", "PLLHIP_AA_TI_MFMA": "1", "PLLHIP_AA_CHERRY": "2"}
    w = M.RootWalk(gpu, orc, _case(gpu, 20, RANDOM20, sites=256 + AA_SITES), PT, M.walk(*RANDOM20), monkeypatch, env=env,
                   second=dict(env={"PLL_AMD_DEVICES": "0,0"}, lnl_rtol=1e-12))
    assert gpu.lib.pll_amd_shard_count(w.p.ptr) == 1 and gpu.lib.pll_amd_shard_count(w.q.ptr) == 2
    evidence = AaLists(gpu, w, True, 1)
    both = AaLists(gpu, w, True, 1, certificate=False)
    both.p = w.q        # (pll_amd_list_kinds of a group: its first shard's)

    def on_list(k, mv, replay):
        evidence(k, mv, replay)
        both(k, mv, replay)
    figures = w.run(on_list)
    cert = evidence.finish()
    split = w.q.scaling_certificate()
    assert split["uncertified"] == 0 and split["lists"] == 2 * cert["lists"], (split, cert)
    w.destroy()
    _report("20 states, two shards", figures, "; certificate %r, of the two shards %r" % (cert, split))
