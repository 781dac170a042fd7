"""Tip pairs that a whole-tree launch of the plain 4-state walk kernel does not store (MBAMD_W4_NOSTORE, mbamd_walk4.h): the buffer
keeps a recipe -- its two compact tips, its scale mode, a snapshot of its two matrices -- and is recomputed by one launch of the
generic kernel before the first call that reads it (Walk4Unstored::ensureStored, mbamd_walk4_unstored.h).

  * CPU (`not gpu`): the host-emulation build of the same sources;
  * GPU (`gpu`): the product library on a MI355X.

The A/B partner is MBAMD_STORE_TIP_PAIRS=1: everything stored, as before.  Every case runs the same calls on two instances, with the
switch and without, and compares BITWISE whatever it reads; mbamdGetRecomputeCounts (buffers left unstored, buffers materialised,
materialising launches) says what happened, and is all zeros with the switch.

Which lists reach the plain kernel is test_walk4_plain.py's subject; the rules that stand in front of small trees are switched off
there and here in BOTH builds: MBAMD_NO_INLINE_PROGRAMS (a program of at most 96 entries travels in the kernel arguments), for lists
that are root-ward paths -- every whole-tree list of 4 or 5 taxa, every caterpillar -- MBAMD_NO_PATH4, and MBAMD_WALK_WAVES=1 where
the geometry rule would cut a list of 32 operations or more over several waves.  The partial updates below run on 33 taxa WITHOUT
MBAMD_NO_PATH4: their lists are the path kernels' (k_path4, k_path4_lnl), which read the unstored sibling.
"""
import ctypes as C
import os

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import data as mbdata
from mrbayes_amd import likelihood as lk
from mrbayes_amd import tree as mbtree
from mrbayes_amd.division import build_division, synthetic_division
from tests.hostemu import build_emu

SWITCH = "MBAMD_STORE_TIP_PAIRS"
NONE = bg.BEAGLE_OP_NONE
TO_WALK = {"MBAMD_NO_INLINE_PROGRAMS": "1"}
TO_WALK_NO_PATH = {"MBAMD_NO_INLINE_PROGRAMS": "1", "MBAMD_NO_PATH4": "1"}
ALWAYS, DYNAMIC = lk.MB_BEAGLE_SCALE_ALWAYS, lk.MB_BEAGLE_SCALE_DYNAMIC


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def balanced_tree(ntaxa):
    """taxon 1 (the calculation root) and two balanced halves of the others: (ntaxa - 1) / 2 tip pairs, more or less"""
    def sub(tips):
        if len(tips) == 1:
            return "%d:%.3f" % (tips[0], 0.02 + 0.01 * (tips[0] % 7))
        h = len(tips) // 2
        return "(%s,%s):%.3f" % (sub(tips[:h]), sub(tips[h:]), 0.03 + 0.01 * (len(tips) % 5))
    rest = list(range(2, ntaxa + 1))
    h = len(rest) // 2
    return mbtree.parse_newick("(1:0.05,%s,%s);" % (sub(rest[:h]), sub(rest[h:])), root_tip=0)


def make_tree(shape, ntaxa):
    if shape == "caterpillar":
        return mbtree.caterpillar_tree(ntaxa)
    if shape == "balanced":
        return balanced_tree(ntaxa)
    return mbtree.random_tree(ntaxa, 5, brlen=0.05)


_divisions = {}


def division(shape, ntaxa, ncat, npat, real_tip=None):
    """GTR (+G4 when ncat = 4), 5 % gaps everywhere; two tips carry ambiguity codes (0/1 tip partials: the engine keeps them as compact
    tips) in a fifth of their patterns.  real_tip: that tip is given as partials that are not 0/1 -- it cannot be a compact tip."""
    key = (shape, ntaxa, ncat, npat, real_tip)
    if key not in _divisions:
        st = mbdata.synthetic_states(ntaxa, npat, 4, 17 + ntaxa, 0.15, 0.05)
        rng = np.random.default_rng(3)
        tip_states, tip_partials = [], []
        for t in range(ntaxa):
            if t in (1, ntaxa - 1) or t == real_tip:
                gap = st[t] >= 4
                p = np.zeros((npat, 4))
                p[np.arange(npat), np.where(gap, 0, st[t])] = 1.0
                extra = (rng.random((npat, 4)) < 0.4) & (rng.random(npat) < 0.2)[:, None]
                p[extra] = 1.0
                p[gap] = 1.0
                if t == real_tip:
                    p = 0.25 + 0.5 * p
                tip_states.append(None)
                tip_partials.append(p)
            else:
                tip_states.append(np.ascontiguousarray(st[t], dtype=np.int32))
                tip_partials.append(None)
        _divisions[key] = build_division("gtr", make_tree(shape, ntaxa), np.ones(npat), tip_states, tip_partials,
                                         revmat=[0.10, 0.30, 0.05, 0.08, 0.40, 0.07], pi=[0.35, 0.25, 0.15, 0.25],
                                         alpha=0.7 if ncat > 1 else None, ncat=ncat)
    return _divisions[key]


def tip_pair_nodes(t):
    return [p for p in t.int_down_pass if t.left[p] < t.ntaxa and t.right[p] < t.ntaxa]


# ---- the A/B harness -------------------------------------------------------------------------------------------------------------
def run_ab(lib, monkeypatch, div, env, scenario, scaling=ALWAYS, **kw):
    """scenario(bd) -> (arrays, counter deltas); run without and with the switch.  Returns the counters of the build as shipped."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = []
    for store in (False, True):
        if store:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        bd = lk.BeagleDivision(div, lib, scaling=scaling, **kw)
        try:
            assert bd.inst.get_recompute_counts() == (0, 0, 0)
            out.append(scenario(bd))
        finally:
            bd.finalize()
    monkeypatch.delenv(SWITCH, raising=False)
    (a, ca), (b, cb) = out
    print("recompute counters (left unstored, materialised, launches): %s / with %s=1 %s" % (ca, SWITCH, cb))
    assert all(c == (0, 0, 0) for c in cb), cb
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), ("item", j)
    assert all(np.all(np.isfinite(x)) for x in a)
    return ca


def evaluation_state(bd, lnl):
    """what an evaluation leaves behind that needs no partials: lnL, site values, every exponent buffer, the cumulative buffer"""
    t = bd.div.tree
    out = [np.float64(lnl), bd.inst.get_site_log_likelihoods().copy()]
    out += [bd.inst.get_scale_exponents(bd.nodeScalerIndex[0][p]) for p in t.int_down_pass]
    out.append(bd.inst.get_scale_exponents(bd.siteScalerIndex[0]))
    return out


def whole_tree(bd, scheme, expected):
    """every evaluation of the scheme: the state first -- `expected` more buffers unstored, nothing materialised --, then get_partials
    of every interior node: each tip pair materialised by a launch of its own, in the call that reads it"""
    t = bd.div.tree
    arrays, counts = [], []
    left = made = 0
    for lnl, plain in scheme(bd):
        arrays += evaluation_state(bd, lnl)
        left += (expected or 0) if plain else 0
        c = bd.inst.get_recompute_counts()
        counts.append(c)
        if expected is not None and not stores_everything():
            assert c == (left, made, made), (c, left, made)
        for p in t.int_down_pass:
            arrays.append(bd.inst.get_partials(bd.condLikeIndex[0][p]))
        made += (expected or 0) if plain else 0
        c = bd.inst.get_recompute_counts()
        counts.append(c)
        if expected is not None and not stores_everything():
            assert c == (left, made, made), (c, left, made)
    return arrays, counts


def stores_everything():
    return SWITCH in os.environ


def scheme_always(bd):
    """rescaling everywhere, twice: a fresh cumulative buffer, then every node touched again into the other buffers"""
    yield bd.LogLike(0), True
    bd.AcceptMove(0)
    bd.upDateCl[0] = [True] * bd.nNodes
    bd.upDateTi[0] = [True] * bd.nNodes
    yield bd.LogLike(0), True


def scheme_nowhere(bd):
    yield bd.LogLike(0), True


def scheme_chosen(bd):
    """unscaled; the rescale-everything pass (exponents at every third node); then the evaluation that divides by the stored exponents
    (not plain: everything stored)"""
    yield bd.LogLike(0), True
    bd.AcceptMove(0)
    bd.FlipSiteScalerSpace(0)
    bd.ResetScalersPartition(0, 3)
    bd.inst.reset_scale_factors(bd.siteScalerIndex[0])
    bd.TouchAllTreeNodes(0)
    bd.TreeTiProbs_Beagle(0)
    bd.TreeCondLikes_Beagle_Rescale_All(0)
    rc, lnl = bd.TreeLikelihood_Beagle(0)
    assert rc == bg.BEAGLE_SUCCESS
    bd.ClearTouches(0)
    yield lnl, True
    bd.AcceptMove(0)
    bd.TouchAllTreeNodes(0)
    yield bd.LogLike(0), False


# name -> (tree shape, taxa, categories, patterns, scheme, scaling, environment of both builds)
WHOLE = {
    "caterpillar_5_k4": ("caterpillar", 5, 4, 130, scheme_always, ALWAYS, TO_WALK_NO_PATH),          # 3 operations: odd, one tip pair
    "caterpillar_12_k1": ("caterpillar", 12, 1, 64, scheme_always, ALWAYS, TO_WALK_NO_PATH),         # 10: even
    "caterpillar_13_k4": ("caterpillar", 13, 4, 130, scheme_nowhere, DYNAMIC, TO_WALK_NO_PATH),      # 11: odd
    "random_5_k1": ("random", 5, 1, 130, scheme_nowhere, DYNAMIC, TO_WALK_NO_PATH),
    "random_12_k4": ("random", 12, 4, 130, scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "random_13_k1": ("random", 13, 1, 130, scheme_chosen, DYNAMIC, TO_WALK_NO_PATH),
    "random_33_k4": ("random", 33, 4, 64, scheme_chosen, DYNAMIC, TO_WALK),
    "balanced_12_k4": ("balanced", 12, 4, 64, scheme_chosen, DYNAMIC, TO_WALK_NO_PATH),
    "balanced_13_k1": ("balanced", 13, 1, 130, scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "balanced_33_k4": ("balanced", 33, 4, 130, scheme_always, ALWAYS, TO_WALK),                      # 31 operations, 16 tip pairs
    "balanced_33_k1": ("balanced", 33, 1, 130, scheme_nowhere, DYNAMIC, TO_WALK),
    "random_100_k4": ("random", 100, 4, 130, scheme_always, ALWAYS, {"MBAMD_WALK_WAVES": "1"}),      # 98 operations: not inline
}


def check_whole_tree(lib, monkeypatch, name, npat=None, env=None):
    shape, ntaxa, ncat, p, scheme, scaling, e = WHOLE[name]
    div = division(shape, ntaxa, ncat, npat or p)
    pairs = len(tip_pair_nodes(div.tree))
    assert pairs >= 1
    if shape == "caterpillar":
        assert pairs == 1
    if shape == "balanced":
        assert pairs == {12: 4, 13: 4, 33: 16}[ntaxa]               # (33: two perfect halves of 16 tips, every tip in a pair)
    counts = run_ab(lib, monkeypatch, div, e if env is None else env, lambda bd: whole_tree(bd, scheme, pairs), scaling=scaling)
    assert counts[-1][0] >= pairs and counts[-1][1] == counts[-1][0] == counts[-1][2]


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_whole_tree_on_emulation(emu, monkeypatch, name):
    check_whole_tree(emu, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WHOLE))
def test_whole_tree(gpu, monkeypatch, name):
    check_whole_tree(gpu, monkeypatch, name)


@pytest.mark.gpu
def test_whole_tree_as_shipped(gpu, monkeypatch):
    """100 taxa x 40 000 patterns, G4: single-wave workgroups by the geometry rule, 98 operations through a device buffer -- no switch
    but MBAMD_STORE_TIP_PAIRS itself"""
    try:
        check_whole_tree(gpu, monkeypatch, "random_100_k4", npat=40000, env={})
    finally:
        _divisions.pop(("random", 100, 4, 40000, None), None)


# ---- the snapshot: matrices overwritten in place -----------------------------------------------------------------------------------
def overwrite(bd):
    """(a) evaluate, overwrite every matrix with other lengths (no partials update), read a tip pair: the matrices were copied behind
    the integration; (b) the partials list alone -- no integration follows --, every matrix set from the host, read a tip pair: the
    copy ran in front of the first overwrite"""
    t, inst = bd.div.tree, bd.inst
    pairs = tip_pair_nodes(t)
    arrays = [np.float64(bd.LogLike(0))]
    bd.AcceptMove(0)
    nodes = [p for p in t.all_down_pass]
    inst.update_transition_matrices(bd.cijkIndex[0], [bd.tiProbsIndex[0][p] for p in nodes], [3.1 * t.length[p] + 0.2 for p in nodes])
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in pairs]
    c1 = inst.get_recompute_counts()
    bd.FlipSiteScalerSpace(0)
    inst.reset_scale_factors(bd.siteScalerIndex[0])
    bd.TouchAllTreeNodes(0)
    bd.TreeTiProbs_Beagle(0)
    bd.TreeCondLikes_Beagle_Always_Rescale(0)
    bd.ClearTouches(0)
    junk = np.tile(np.full((4, 4), 0.25), (bd.div.ncat, 1, 1))
    for p in nodes:
        inst.set_transition_matrix(bd.tiProbsIndex[0][p], junk)
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in pairs]
    return arrays, [c1, inst.get_recompute_counts()]


def check_overwrite(lib, monkeypatch):
    div = division("balanced", 33, 4, 130)
    n = len(tip_pair_nodes(div.tree))
    counts = run_ab(lib, monkeypatch, div, TO_WALK, overwrite)
    assert counts == [(n, n, n), (2 * n, 2 * n, 2 * n)], counts


def test_overwritten_matrices_on_emulation(emu, monkeypatch):
    check_overwrite(emu, monkeypatch)


@pytest.mark.gpu
def test_overwritten_matrices(gpu, monkeypatch):
    check_overwrite(gpu, monkeypatch)


# ---- partial updates after a whole-tree evaluation ---------------------------------------------------------------------------------
def branch_move(bd, tips, factor, fused=True):
    """new lengths on the branches above `tips`, the lists of the paths above them, the log-likelihood; fused=False: something reads the
    top node between the list and the log-likelihood call, so the held path runs on its own (k_path4) instead of with it (k_path4_lnl)"""
    t = bd.div.tree
    old = [t.length[i] for i in tips]
    try:
        for i in tips:
            t.length[i] *= factor
            bd.TouchBranch(0, i)
        if fused:
            lnl = bd.LogLike(0)
            extra = []
        else:
            bd.FlipSiteScalerSpace(0)
            bd.inst.copy_scale_factors(bd.siteScalerIndex[0], bd.siteScalerScratchIndex)
            bd.TreeTiProbs_Beagle(0)
            bd.TreeCondLikes_Beagle_Always_Rescale(0)
            extra = [bd.inst.get_partials(bd.condLikeIndex[0][t.root_left])]
            rc, lnl = bd.TreeLikelihood_Beagle(0)
            assert rc == bg.BEAGLE_SUCCESS
            bd.ClearTouches(0)
    finally:
        for i, v in zip(tips, old):
            t.length[i] = v
    return [np.float64(lnl), bd.inst.get_site_log_likelihoods().copy(), bd.inst.get_scale_exponents(bd.siteScalerIndex[0])] + extra


def path_nodes(t, tip):
    out, p = [], t.anc[tip]
    while p != -1 and p >= t.ntaxa:
        out.append(p)
        if p == t.root_left:
            break
        p = t.anc[p]
    return out


def partial_updates(bd):
    """balanced 33 taxa, tips (2,3) (4,5) (6,7) (8,9) ... are tip pairs.  Returns arrays, counters and the list counters."""
    t, inst = bd.div.tree, bd.inst
    pairs = tip_pair_nodes(t)
    n = len(pairs)
    first = pairs[0]
    a = t.left[first]
    sib_pair = [q for q in pairs if q != first and t.anc[q] == t.anc[first]]
    assert sib_pair, "the first tip pair's sibling is a tip pair"
    far = [q for q in pairs if t.anc[q] != t.anc[first] and t.anc[t.anc[q]] == t.anc[t.anc[first]]]
    assert far
    b = t.left[far[0]]                           # (a tip of another tip pair under the same great-grandparent: the two paths join there)
    arrays, counts, lists = [np.float64(bd.LogLike(0))], [], []
    bd.AcceptMove(0)

    def note():
        counts.append(inst.get_recompute_counts())
        lists.append(inst.get_list_counts()[:4])
    note()                                       # (n, 0, 0)
    # a path that STARTS at a tip pair (stored: the path kernel stores everything) and whose next sibling is an unstored tip pair; fused
    arrays += branch_move(bd, [a], 2.5)
    note()                                       # one materialised
    bd.AcceptMove(0)
    # the same sibling again: nothing to materialise; the path on its own (k_path4)
    arrays += branch_move(bd, [a], 0.4, fused=False)
    note()
    bd.AcceptMove(0)
    # a forked path: the arms above a and b join; b's arm has an unstored sibling of its own
    arrays += branch_move(bd, [a, b], 1.7)
    note()
    # rejected: back to the buffers of the state before; then the whole tree into the other buffers, rejected too; then a path over a
    # sibling that neither launch has stored
    bd.ResetFlips(0)
    bd.TouchAllTreeNodes(0)
    arrays.append(np.float64(bd.LogLike(0)))
    note()                                       # n more left unstored (the other flip state)
    bd.ResetFlips(0)
    c = t.left[[q for q in pairs if q not in (first, sib_pair[0], far[0]) and t.anc[q] != t.anc[far[0]]][0]]
    arrays += branch_move(bd, [c], 3.0)
    note()
    bd.AcceptMove(0)
    # ... and every interior node of the state the chain is in
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
    note()
    return arrays, (counts, lists, n)


def check_partial_updates(lib, monkeypatch):
    div = division("balanced", 33, 4, 130)
    res = {}

    def scenario(bd):
        arrays, (counts, lists, n) = partial_updates(bd)
        res[stores_everything()] = (counts, lists, n)
        return arrays, counts
    run_ab(lib, monkeypatch, div, TO_WALK, scenario)
    counts, lists, n = res[False]
    print("partial updates: recompute counters %s, list counters (lists, paths, forked, fused) %s" % (counts, lists))
    assert res[True][1] == lists                                     # the same kernels in both builds
    assert counts[0] == (n, 0, 0)
    assert counts[1] == (n, 1, 1)                                    # the sibling of the path that starts at a tip pair
    assert counts[2] == (n, 1, 1)                                    # the same sibling again: nothing
    assert counts[3] == (n, 2, 2)                                    # the other arm's sibling
    assert counts[4] == (2 * n, 2, 2)
    assert counts[5] == (2 * n, 3, 3)
    assert counts[6][0] == 2 * n and counts[6][1] > 3 and counts[6][1] - 3 == counts[6][2] - 3
    # lists, paths, forked paths, paths fused with their log-likelihood
    assert lists[0] == (1, 0, 0, 0)
    assert lists[1] == (2, 1, 0, 1)                                  # k_path4_lnl
    assert lists[2] == (3, 2, 0, 1)                                  # k_path4
    assert lists[3] == (4, 3, 1, 2)                                  # forked
    assert lists[5] == (6, 4, 1, 3)


def test_partial_updates_on_emulation(emu, monkeypatch):
    check_partial_updates(emu, monkeypatch)


@pytest.mark.gpu
def test_partial_updates(gpu, monkeypatch):
    check_partial_updates(gpu, monkeypatch)


# ---- the other readers of partials --------------------------------------------------------------------------------------------------
def reader_edge(bd):
    """the edge log-likelihood with a tip pair as the child end"""
    t, inst = bd.div.tree, bd.inst
    x = tip_pair_nodes(t)[0]
    bd.LogLike(0)
    rc, lnl = inst.calculate_edge_log_likelihoods([bd.condLikeIndex[0][t.root_left]], [bd.condLikeIndex[0][x]], [bd.tiProbsIndex[0][x]],
                                                  [bd.cijkIndex[0]], [bd.cijkIndex[0]], [bd.siteScalerIndex[0]])
    assert rc == 0
    return [np.float64(lnl), inst.get_site_log_likelihoods().copy()], [inst.get_recompute_counts()]


def reader_gradient(bd):
    """pre-order partials (every sibling is read) and the gradient (every post-order buffer is read)"""
    t = bd.div.tree
    bd.LogLike(0)
    grad, sites = bd.BranchGradient(0, sites=True)
    nodes = list(t.all_down_pass)
    return [np.array([grad[n] for n in nodes])] + [sites[n] for n in nodes], [bd.inst.get_recompute_counts()]


def reader_derivatives(bd):
    t, inst = bd.div.tree, bd.inst
    x = tip_pair_nodes(t)[0]
    bd.LogLike(0)
    pcopy, m1, m2 = (bd.tiProbsScratchIndex[i] for i in (0, 1, 2))
    inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [0.07], first=[m1], second=[m2])
    rc, lnl, d1, d2 = inst.calculate_edge_derivatives([bd.condLikeIndex[0][t.root_left]], [bd.condLikeIndex[0][x]], [pcopy], [m1], [m2],
                                                      [bd.cijkIndex[0]], [bd.cijkIndex[0]], [bd.siteScalerIndex[0]])
    assert rc == 0
    s1, s2 = inst.get_site_derivatives()
    return [np.array([lnl, d1, d2]), inst.get_site_log_likelihoods().copy(), s1, s2], [inst.get_recompute_counts()]


def reader_final_pass(bd):
    t, inst = bd.div.tree, bd.inst
    bd.LogLike(0)
    bd.AcceptMove(0)
    cl, sc, ti = bd.condLikeIndex[0], bd.condLikeScratchIndex, bd.tiProbsIndex[0]
    ops = []
    for p in reversed(t.int_down_pass):
        ops.append([sc[p], -1, cl[p], ti[p], cl[t.root]] if p == t.root_left else [sc[p], sc[t.anc[p]], cl[p], ti[p], -1])
    inst.update_final_partials(np.asarray(ops, dtype=np.int32))
    out = []
    for p in t.int_down_pass:
        out += list(inst.get_scaled_partials(sc[p], bd.siteScalerIndex[0]))
    return out, [inst.get_recompute_counts()]


def reader_scaled(bd):
    t, inst = bd.div.tree, bd.inst
    bd.LogLike(0)
    out = []
    for x in tip_pair_nodes(t)[:3]:
        out += list(inst.get_scaled_partials(bd.condLikeIndex[0][x], bd.siteScalerIndex[0]))
    return out, [inst.get_recompute_counts()]


# name -> (scenario, BeagleDivision keywords, (materialised, launches) as a function of the number of tip pairs n)
READERS = {
    "edge": (reader_edge, {}, lambda n: (1, 1)),
    "gradient": (reader_gradient, {"pre_order": True}, lambda n: (n, 1)),            # the pre-order pass reads every sibling: one launch
    "derivatives": (reader_derivatives, {}, lambda n: (1, 1)),
    "final_pass": (reader_final_pass, {}, lambda n: (n, n)),                         # one operation, one launch each
    "scaled": (reader_scaled, {}, lambda n: (3, 3)),
}


def check_reader(lib, monkeypatch, name):
    scenario, kw, want = READERS[name]
    div = division("balanced", 33, 4, 130)
    n = len(tip_pair_nodes(div.tree))
    counts = run_ab(lib, monkeypatch, div, TO_WALK, scenario, **kw)
    assert counts == [(n,) + want(n)], (name, counts)


@pytest.mark.parametrize("name", sorted(READERS))
def test_reader_on_emulation(emu, monkeypatch, name):
    check_reader(emu, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(READERS))
def test_reader(gpu, monkeypatch, name):
    check_reader(gpu, monkeypatch, name)


# ---- not eligible: nothing is left unstored ----------------------------------------------------------------------------------------
def just_evaluate(bd):
    t = bd.div.tree
    lnl = bd.LogLike(0)
    c = bd.inst.get_recompute_counts()
    out = [np.float64(lnl), bd.inst.get_site_log_likelihoods().copy()]
    out += [bd.inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass if bd.div.nstates == 4]
    return out, [c, bd.inst.get_recompute_counts()]


def two_segments(bd):
    """the whole-tree list with its last operation issued twice: a buffer written twice ends the segment"""
    t, inst = bd.div.tree, bd.inst
    bd.TreeTiProbs_Beagle(0)
    ops = [bd._op(0, p) for p in t.int_down_pass]
    inst.update_partials(np.asarray(ops + [ops[-1]], dtype=np.int32), NONE)
    c = inst.get_recompute_counts()
    return [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass], [c, inst.get_recompute_counts()]


def real_tip_division():
    t = mbtree.caterpillar_tree(12)
    x = tip_pair_nodes(t)[0]
    return division("caterpillar", 12, 4, 130, real_tip=t.left[x])


# name -> (division, environment, scenario, BeagleDivision keywords)
NOT_ELIGIBLE = {
    "two_segments": (lambda: division("balanced", 33, 4, 130), TO_WALK, two_segments, {}),
    "two_waves": (lambda: division("random", 40, 4, 130), dict(TO_WALK, MBAMD_WALK_WAVES="2"), just_evaluate, {}),
    "no_plain_walk": (lambda: division("balanced", 33, 4, 130), dict(TO_WALK, MBAMD_NO_PLAIN_WALK="1"), just_evaluate, {}),
    "in_the_kernel_arguments": (lambda: division("balanced", 33, 4, 130), {}, just_evaluate, {}),
    "tip_given_as_partials": (real_tip_division, TO_WALK_NO_PATH, just_evaluate, {}),
    "twenty_states": (lambda: synthetic_division("wag", 12, 70, seed=11, tree_seed=5, p_gap=0.05), {}, just_evaluate, {}),
}


def check_not_eligible(lib, monkeypatch, name):
    make, env, scenario, kw = NOT_ELIGIBLE[name]
    counts = run_ab(lib, monkeypatch, make(), env, scenario, **kw)
    assert counts == [(0, 0, 0), (0, 0, 0)], (name, counts)


@pytest.mark.parametrize("name", sorted(NOT_ELIGIBLE))
def test_not_eligible_on_emulation(emu, monkeypatch, name):
    check_not_eligible(emu, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NOT_ELIGIBLE))
def test_not_eligible(gpu, monkeypatch, name):
    check_not_eligible(gpu, monkeypatch, name)


# ---- pattern shards: every child engine keeps its own recipes ------------------------------------------------------------------------
def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 130 patterns (children of 64 and 66): the counters are the sums over the children"""
    div = division("balanced", 33, 4, 130)
    n = len(tip_pair_nodes(div.tree))

    def scenario(bd):
        assert bd.inst.child_count() == 2
        return whole_tree(bd, scheme_always, None)
    counts = run_ab(lib, monkeypatch, div, dict(TO_WALK, MBAMD_SHARD="2"), scenario)
    assert counts == [(2 * n, 0, 0), (2 * n, 2 * n, 2 * n), (4 * n, 2 * n, 2 * n), (4 * n, 4 * n, 4 * n)], counts


def test_sharded_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- the export itself -----------------------------------------------------------------------------------------------------------
def check_counts_call(lib):
    bd = lk.BeagleDivision(division("caterpillar", 5, 1, 64), lib)
    try:
        assert lib.lib.mbamdGetRecomputeCounts(bd.inst.id, None) == bg.BEAGLE_ERROR_OUT_OF_RANGE
        assert lib.lib.mbamdGetRecomputeCounts(bd.inst.id + 1000, (C.c_long * 3)()) == bg.BEAGLE_ERROR_UNINITIALIZED_INSTANCE
    finally:
        bd.finalize()
    f64 = lk.BeagleDivision(division("balanced", 33, 4, 130), lib, double_precision=True)
    try:
        f64.LogLike(0)
        assert f64.inst.get_recompute_counts() == (0, 0, 0)
    finally:
        f64.finalize()


def test_counts_call_on_emulation(emu):
    check_counts_call(emu)


@pytest.mark.gpu
def test_counts_call(gpu):
    check_counts_call(gpu)
