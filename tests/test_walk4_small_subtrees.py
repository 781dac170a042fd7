"""Subtrees of up to four compact tips that a whole-tree launch of the plain 4-state walk kernel does not store (MBAMD_UNSTORED_TIPS,
MBAMD_W4_NOSTORE in mbamd_walk4.h): beside the tip pairs of test_walk4_tip_pairs.py, a subtree of three or four tips keeps a recipe that
stands alone -- its tips, its two or three operations with their scale modes, a snapshot of all its matrices -- and is recomputed by one
launch of the plain instantiation before the first call that reads it (Walk4Unstored::ensureStored, mbamd_walk4_unstored.h); its inner results land
nowhere.

  * CPU (`not gpu`): the host-emulation build of the same sources;
  * GPU (`gpu`): the product library on a MI355X.

The A/B partner is MBAMD_STORE_TIP_PAIRS=1: everything stored.  Every case runs the same calls on two instances, with the switch and
without, and compares BITWISE whatever it reads.  Two exports say what happened: mbamdGetRecomputeCounts counts tip pairs only (buffers
left unstored, buffers materialised, launches that materialised at least one), mbamdGetSubtreeRecomputeCounts the same for subtrees of
three and four tips; both read zeros with the switch.  What is expected of them is counted here on the tree, independently of the engine.

Small trees reach the plain device-buffer walk only with MBAMD_NO_INLINE_PROGRAMS (and MBAMD_NO_PATH4 for lists that are root-ward
paths), set in both runs, as in test_walk4_tip_pairs.py, whose helpers this module uses.  Shapes: 130 patterns (three blocks, the last
one partial), K = 4 and K = 1, rescaling always and dynamic.
"""
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import data as mbdata
from mrbayes_amd import likelihood as lk
from mrbayes_amd import tree as mbtree
from mrbayes_amd.division import build_division
from tests.hostemu import build_emu
from tests import test_walk4_tip_pairs as tp

SWITCH, TIPS = tp.SWITCH, "MBAMD_UNSTORED_TIPS"
NONE = bg.BEAGLE_OP_NONE
TO_WALK, TO_WALK_NO_PATH = tp.TO_WALK, tp.TO_WALK_NO_PATH
ALWAYS, DYNAMIC = tp.ALWAYS, tp.DYNAMIC
NPAT = 130


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
def newick(s):
    """taxon 1 is the calculation root; branch lengths by position"""
    out, n = [], 0
    for ch in s:
        if ch in ",)":
            n += 1
            out.append(":%.3f" % (0.02 + 0.013 * (n % 9)))
        out.append(ch)
    return mbtree.parse_newick("".join(out) + ";", root_tip=0)


TREES = {
    "four_balanced": lambda: newick("(1,((2,3),(4,5)),6)"),                 # the three shapes of four tips, each under a parent of five
    "four_right": lambda: newick("(1,(2,(3,(4,5))),6)"),
    "four_left": lambda: newick("(1,(((2,3),4),5),6)"),
    "top_balanced": lambda: newick("(1,(2,3),(4,5))"),                      # ... and as the top node, which the integration reads
    "pitchfork_5": lambda: newick("(1,((2,3),4),5)"),
    "ladder_12": lambda: mbtree.caterpillar_tree(12),
    "balanced_9": lambda: tp.balanced_tree(9),
    "balanced_17": lambda: tp.balanced_tree(17),
    "balanced_33": lambda: tp.balanced_tree(33),
    "random_33": lambda: mbtree.random_tree(33, 5, brlen=0.05),
    "random_100": lambda: mbtree.random_tree(100, 5, brlen=0.05),
    # a subtree of five tips over its parts of two, three and four, beside a pitchfork
    "boundary": lambda: newick("(1,((((2,3),4),5),6),((7,8),9))"),
    # pitchforks P1 P2 and balanced fours Q1 Q2: X = (P1, Q1), Y = (Q2, P2), top = (X, Y)
    "mixed_15": lambda: newick("(1,(((2,3),4),((5,6),(7,8))),(((9,10),(11,12)),((13,14),15)))"),
    "two_pitchforks": lambda: newick("(1,((2,3),4),((5,6),7))"),
}
_divisions = {}


def division(name, ncat, npat=NPAT, real_tip=None):
    """as test_walk4_tip_pairs.division, over the trees above"""
    key = (name, ncat, npat, real_tip)
    if key not in _divisions:
        tree = TREES[name]()
        ntaxa = tree.ntaxa
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
        _divisions[key] = build_division("gtr", tree, np.ones(npat), tip_states, tip_partials,
                                         revmat=[0.10, 0.30, 0.05, 0.08, 0.40, 0.07], pi=[0.35, 0.25, 0.15, 0.25],
                                         alpha=0.7 if ncat > 1 else None, ncat=ncat)
    return _divisions[key]


def subtree_tips(t, real=()):
    """{interior node: tips below it, if they are all compact tips; else 0}"""
    n = {}
    for p in t.int_down_pass:
        k = [(0 if c in real else 1) if c < t.ntaxa else n[c] for c in (t.left[p], t.right[p])]
        n[p] = k[0] + k[1] if k[0] and k[1] else 0
    return n


def flagged(t, T=4, real=()):
    """(tip-pair nodes, nodes of three ... T tips) in post-order"""
    n = subtree_tips(t, real)
    return [p for p in t.int_down_pass if n[p] == 2], [p for p in t.int_down_pass if 3 <= n[p] <= T]


# ---- the A/B harness -------------------------------------------------------------------------------------------------------------
def counts_of(inst):
    return inst.get_recompute_counts(), inst.get_subtree_recompute_counts()


def run_ab(lib, monkeypatch, div, env, scenario, scaling=ALWAYS, T=None, **kw):
    """scenario(bd) -> (arrays, [(tip-pair triple, subtree triple), ...]); run without and with the switch.  Returns the counters of the
    build as shipped (T = None) or at MBAMD_UNSTORED_TIPS = T."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if T is not None:
        monkeypatch.setenv(TIPS, str(T))
    out = []
    for store in (False, True):
        if store:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        bd = lk.BeagleDivision(div, lib, scaling=scaling, **kw)
        try:
            assert counts_of(bd.inst) == ((0, 0, 0), (0, 0, 0))
            out.append(scenario(bd))
        finally:
            bd.finalize()
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(TIPS, raising=False)
    (a, ca), (b, cb) = out
    print("counters (tip pairs, subtrees) x (left unstored, materialised, launches): %s / with %s=1 %s" % (ca, SWITCH, cb))
    assert all(c == ((0, 0, 0), (0, 0, 0)) for c in cb), cb
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), ("item", j)
    assert all(np.all(np.isfinite(x)) for x in a)
    return ca


# ---- whole-tree evaluations, every interior node read in post-order and in pre-order --------------------------------------------------
def whole_tree(bd, scheme, order, T):
    """every evaluation of the scheme: the state first, then get_partials of every interior node -- post-order, or pre-order (a parent
    before its children: materialising it must leave the parts inside it unstored).  Every flagged node is materialised by a launch
    of its own, in the call that reads it; the top node, if flagged, by the integration."""
    t = bd.div.tree
    pairs, subs = flagged(t, T)
    arrays, counts = [], []
    left = [0, 0]
    made = [0, 0]
    check = not tp.stores_everything()
    nodes = list(t.int_down_pass) if order == "post" else list(reversed(t.int_down_pass))
    for lnl, plain in scheme(bd):
        arrays += tp.evaluation_state(bd, lnl)
        if plain:
            left[0] += len(pairs)
            left[1] += len(subs)
            if t.root_left in subs:
                made[1] += 1
            assert t.root_left not in pairs
        c = counts_of(bd.inst)
        counts.append(c)
        if check:
            assert c == ((left[0], made[0], made[0]), (left[1], made[1], made[1])), (c, left, made)
        for p in nodes:
            arrays.append(bd.inst.get_partials(bd.condLikeIndex[0][p]))
            if plain:
                made[0] += p in pairs
                made[1] += p in subs and p != t.root_left
            c = counts_of(bd.inst)
            if check:                            # (after every read: only the node named was made)
                assert c == ((left[0], made[0], made[0]), (left[1], made[1], made[1])), (p, c, left, made)
        counts.append(c)
    return arrays, counts


# name -> (tree, categories, scheme, scaling, environment of both builds)
WHOLE = {
    "four_balanced_k4": ("four_balanced", 4, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "four_balanced_k1": ("four_balanced", 1, tp.scheme_nowhere, DYNAMIC, TO_WALK_NO_PATH),
    "four_right_k4": ("four_right", 4, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "four_right_k1": ("four_right", 1, tp.scheme_chosen, DYNAMIC, TO_WALK_NO_PATH),
    "four_left_k4": ("four_left", 4, tp.scheme_chosen, DYNAMIC, TO_WALK_NO_PATH),
    "four_left_k1": ("four_left", 1, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "top_balanced_k4": ("top_balanced", 4, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "pitchfork_5_k4": ("pitchfork_5", 4, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "pitchfork_5_k1": ("pitchfork_5", 1, tp.scheme_nowhere, DYNAMIC, TO_WALK_NO_PATH),
    "ladder_12_k4": ("ladder_12", 4, tp.scheme_chosen, DYNAMIC, TO_WALK_NO_PATH),
    "ladder_12_k1": ("ladder_12", 1, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "balanced_9_k4": ("balanced_9", 4, tp.scheme_always, ALWAYS, TO_WALK_NO_PATH),
    "balanced_9_k1": ("balanced_9", 1, tp.scheme_chosen, DYNAMIC, TO_WALK_NO_PATH),
    "balanced_17_k4": ("balanced_17", 4, tp.scheme_chosen, DYNAMIC, TO_WALK),
    "balanced_17_k1": ("balanced_17", 1, tp.scheme_always, ALWAYS, TO_WALK),
    "balanced_33_k4": ("balanced_33", 4, tp.scheme_always, ALWAYS, TO_WALK),
    "balanced_33_k1": ("balanced_33", 1, tp.scheme_nowhere, DYNAMIC, TO_WALK),
    "random_33_k4": ("random_33", 4, tp.scheme_chosen, DYNAMIC, TO_WALK),
    "random_33_k1": ("random_33", 1, tp.scheme_always, ALWAYS, TO_WALK),
    "mixed_15_k4": ("mixed_15", 4, tp.scheme_always, ALWAYS, TO_WALK),
}


def check_whole_tree(lib, monkeypatch, name, order):
    tree, ncat, scheme, scaling, env = WHOLE[name]
    div = division(tree, ncat)
    pairs, subs = flagged(div.tree)
    assert pairs and subs
    counts = run_ab(lib, monkeypatch, div, env, lambda bd: whole_tree(bd, scheme, order, 4), scaling=scaling)
    assert counts[-1][1][0] >= len(subs) and counts[-1][1][0] == counts[-1][1][1] == counts[-1][1][2]


@pytest.mark.parametrize("order", ["post", "pre"])
@pytest.mark.parametrize("name", sorted(WHOLE))
def test_whole_tree_on_emulation(emu, monkeypatch, name, order):
    check_whole_tree(emu, monkeypatch, name, order)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["post", "pre"])
@pytest.mark.parametrize("name", sorted(WHOLE))
def test_whole_tree(gpu, monkeypatch, name, order):
    check_whole_tree(gpu, monkeypatch, name, order)


@pytest.mark.gpu
def test_whole_tree_as_shipped(gpu, monkeypatch):
    """100 taxa x 40 000 patterns, G4: single-wave workgroups by the geometry rule, 98 operations through a device buffer -- no switch
    but MBAMD_STORE_TIP_PAIRS itself.  lnL, site values, exponents and all partials."""
    div = division("random_100", 4, npat=40000)
    try:
        pairs, subs = flagged(div.tree)
        assert pairs and subs
        run_ab(gpu, monkeypatch, div, {}, lambda bd: whole_tree(bd, tp.scheme_always, "post", 4))
    finally:
        _divisions.pop(("random_100", 4, 40000, None), None)


# ---- the boundary: five tips are stored, their parts of two, three and four are not ------------------------------------------------------
def check_boundary(lib, monkeypatch, T, ncat, scaling):
    div = division("boundary", ncat)
    t = div.tree
    n = subtree_tips(t)
    assert sorted(n.values()) == [2, 2, 3, 3, 4, 5, 8]
    pairs, subs = flagged(t, T)
    assert len(pairs) == 2 and len(subs) == {2: 0, 3: 2, 4: 3}[T]
    scheme = tp.scheme_always if scaling == ALWAYS else tp.scheme_nowhere
    evals = 2 if scaling == ALWAYS else 1
    counts = run_ab(lib, monkeypatch, div, TO_WALK_NO_PATH, lambda bd: whole_tree(bd, scheme, "post", T), scaling=scaling, T=T)
    assert counts[0] == ((2, 0, 0), (len(subs), 0, 0))
    assert counts[-1] == ((2 * evals,) * 3, (len(subs) * evals,) * 3)
    if T == 2:
        assert all(c[1] == (0, 0, 0) for c in counts)


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("ncat,scaling", [(4, ALWAYS), (1, DYNAMIC)])
def test_boundary_on_emulation(emu, monkeypatch, T, ncat, scaling):
    check_boundary(emu, monkeypatch, T, ncat, scaling)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("ncat,scaling", [(4, ALWAYS), (1, DYNAMIC)])
def test_boundary(gpu, monkeypatch, T, ncat, scaling):
    check_boundary(gpu, monkeypatch, T, ncat, scaling)


def check_clamped(lib, monkeypatch):
    """anything else is clamped to 2 ... 4"""
    for value, T in (("1", 2), ("0", 2), ("-3", 2), ("5", 4), ("99", 4)):
        div = division("boundary", 4)
        counts = run_ab(lib, monkeypatch, div, TO_WALK_NO_PATH, lambda bd: whole_tree(bd, tp.scheme_nowhere, "post", T), scaling=DYNAMIC, T=value)
        assert counts[0] == ((2, 0, 0), ({2: 0, 4: 3}[T], 0, 0))


def test_clamped_on_emulation(emu, monkeypatch):
    check_clamped(emu, monkeypatch)


@pytest.mark.gpu
def test_clamped(gpu, monkeypatch):
    check_clamped(gpu, monkeypatch)


# ---- exclusions ---------------------------------------------------------------------------------------------------------------------
def evaluate_and_read(bd):
    t = bd.div.tree
    lnl = bd.LogLike(0)
    c = counts_of(bd.inst)
    out = [np.float64(lnl), bd.inst.get_site_log_likelihoods().copy()]
    out += [bd.inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
    return out, [c, counts_of(bd.inst)]


def check_real_tip(lib, monkeypatch):
    """a tip given as real partials inside a would-be pitchfork: that pitchfork (and the tip pair in it) is stored.  Its sibling
    pitchfork is stored too, and both exports read zero: a child that is real partials is read from HBM, which the plain instantiation
    cannot do, so the whole list runs on the generic kernel, where nothing is flagged (the rule of test_walk4_tip_pairs'
    tip_given_as_partials).  Counted on the tree, with that tip set aside, the sibling alone would qualify."""
    t = TREES["two_pitchforks"]()
    real = 2                                                         # taxon 3, in the tip pair (2,3)
    assert t.anc[real] >= t.ntaxa and t.left[t.anc[real]] < t.ntaxa and t.right[t.anc[real]] < t.ntaxa
    div = division("two_pitchforks", 4, real_tip=real)
    pairs, subs = flagged(div.tree, 4, real=(real,))
    assert len(pairs) == 1 and len(subs) == 1

    def scenario(bd):
        arrays, counts = evaluate_and_read(bd)
        assert bd.inst.get_walk_counts()[0] == 0                     # (not on the plain instantiation)
        return arrays, counts
    counts = run_ab(lib, monkeypatch, div, TO_WALK_NO_PATH, scenario)
    assert counts == [((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 0))], counts


def same_buffer_twice(bd):
    """pitchfork_5's list with the pitchfork's operation reading the tip pair as BOTH children (the general kind): stored, and so is
    its parent; the tip pair is not"""
    t, inst = bd.div.tree, bd.inst
    bd.UpDateCijk(0)
    bd.TreeTiProbs_Beagle(0)
    ops = [bd._op(0, p) for p in t.int_down_pass]
    fork = [i for i, p in enumerate(t.int_down_pass) if subtree_tips(t)[p] == 3][0]
    pair = ops[fork][3] if ops[fork][3] >= t.ntaxa else ops[fork][5]
    ops[fork][3] = ops[fork][5] = pair
    inst.update_partials(np.asarray(ops, dtype=np.int32), NONE)
    c = counts_of(inst)
    return [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass], [c, counts_of(inst)]


def check_same_buffer_twice(lib, monkeypatch):
    counts = run_ab(lib, monkeypatch, division("pitchfork_5", 4), TO_WALK_NO_PATH, same_buffer_twice)
    assert counts == [((1, 0, 0), (0, 0, 0)), ((1, 1, 1), (0, 0, 0))], counts


def swapped_children(bd):
    """four_balanced's list with the second tip pair computed FIRST: the four's operation reads (forwarded, slot) in the original launch
    and in the materialising one"""
    t, inst = bd.div.tree, bd.inst
    bd.UpDateCijk(0)
    bd.TreeTiProbs_Beagle(0)
    ops = [bd._op(0, p) for p in t.int_down_pass]
    assert [subtree_tips(t)[p] for p in t.int_down_pass[:3]] == [2, 2, 4]
    ops[0], ops[1] = ops[1], ops[0]
    inst.update_partials(np.asarray(ops, dtype=np.int32), NONE)
    c = counts_of(inst)
    return [inst.get_partials(bd.condLikeIndex[0][p]) for p in reversed(t.int_down_pass)], [c, counts_of(inst)]


def check_swapped_children(lib, monkeypatch):
    counts = run_ab(lib, monkeypatch, division("four_balanced", 4), TO_WALK_NO_PATH, swapped_children)
    assert counts == [((2, 0, 0), (1, 0, 0)), ((2, 2, 2), (1, 1, 1))], counts


def inner_scaled_alone(bd):
    """the whole-tree list with exponents recorded at the INNER nodes of the flagged subtrees only: a recipe must rescale an inner
    result as the original launch did -- its parent does not rescale, so a dropped scale mode changes the parent's bits (where the
    parent rescales too, the power of two cancels exactly and nothing could show it)"""
    t, inst = bd.div.tree, bd.inst
    n = subtree_tips(t)
    bd.UpDateCijk(0)
    bd.TreeTiProbs_Beagle(0)
    ops, inner = [], []
    for p in t.int_down_pass:
        op = bd._op(0, p)
        if 2 <= n[p] <= 3 and t.anc[p] >= t.ntaxa and 3 <= n[t.anc[p]] <= 4:
            op[1] = bd.nodeScalerIndex[0][p]
            inner.append(p)
        ops.append(op)
    assert inner
    inst.update_partials(np.asarray(ops, dtype=np.int32), NONE)
    c = counts_of(inst)
    out = [inst.get_partials(bd.condLikeIndex[0][p]) for p in reversed(t.int_down_pass)]
    out += [inst.get_scale_exponents(bd.nodeScalerIndex[0][p]) for p in inner]
    assert any(np.any(x != 0) for x in out[-len(inner):])            # (there is something to drop)
    return out, [c, counts_of(inst)]


def check_inner_scaled_alone(lib, monkeypatch, tree, ncat):
    div = division(tree, ncat)
    pairs, subs = flagged(div.tree)
    counts = run_ab(lib, monkeypatch, div, TO_WALK_NO_PATH, inner_scaled_alone, scaling=DYNAMIC)
    assert counts == [((len(pairs), 0, 0), (len(subs), 0, 0)), ((len(pairs),) * 3, (len(subs),) * 3)], counts


INNER_SCALED = [("pitchfork_5", 4), ("four_balanced", 1), ("four_right", 4), ("four_left", 1), ("mixed_15", 4)]


@pytest.mark.parametrize("tree,ncat", INNER_SCALED)
def test_inner_scaled_alone_on_emulation(emu, monkeypatch, tree, ncat):
    check_inner_scaled_alone(emu, monkeypatch, tree, ncat)


@pytest.mark.gpu
@pytest.mark.parametrize("tree,ncat", INNER_SCALED)
def test_inner_scaled_alone(gpu, monkeypatch, tree, ncat):
    check_inner_scaled_alone(gpu, monkeypatch, tree, ncat)


def test_real_tip_on_emulation(emu, monkeypatch):
    check_real_tip(emu, monkeypatch)


def test_same_buffer_twice_on_emulation(emu, monkeypatch):
    check_same_buffer_twice(emu, monkeypatch)


def test_swapped_children_on_emulation(emu, monkeypatch):
    check_swapped_children(emu, monkeypatch)


@pytest.mark.gpu
def test_real_tip(gpu, monkeypatch):
    check_real_tip(gpu, monkeypatch)


@pytest.mark.gpu
def test_same_buffer_twice(gpu, monkeypatch):
    check_same_buffer_twice(gpu, monkeypatch)


@pytest.mark.gpu
def test_swapped_children(gpu, monkeypatch):
    check_swapped_children(gpu, monkeypatch)


def both_exports(scenario):
    def run(bd):
        arrays, _ = scenario(bd)
        return arrays, [counts_of(bd.inst)]
    return run


def two_segments(bd):
    """the whole-tree list with its last operation issued twice: a buffer written twice ends the segment (the eigen-system is set
    first: the matrices are real ones)"""
    bd.UpDateCijk(0)
    return tp.two_segments(bd)


def check_not_eligible(lib, monkeypatch, name):
    """the cases of test_walk4_tip_pairs.NOT_ELIGIBLE that flag nothing at all: both exports read zero"""
    make, env, scenario, kw = tp.NOT_ELIGIBLE[name]
    if name == "two_segments":
        scenario = two_segments
    counts = run_ab(lib, monkeypatch, make(), env, both_exports(scenario), **kw)
    assert counts == [((0, 0, 0), (0, 0, 0))], (name, counts)


NOT_ELIGIBLE = ["two_segments", "two_waves", "no_plain_walk", "in_the_kernel_arguments", "twenty_states"]


@pytest.mark.parametrize("name", NOT_ELIGIBLE)
def test_not_eligible_on_emulation(emu, monkeypatch, name):
    check_not_eligible(emu, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NOT_ELIGIBLE)
def test_not_eligible(gpu, monkeypatch, name):
    check_not_eligible(gpu, monkeypatch, name)


def check_counts_call(lib):
    bd = lk.BeagleDivision(division("pitchfork_5", 1), lib)
    try:
        assert lib.lib.mbamdGetSubtreeRecomputeCounts(bd.inst.id, None) == bg.BEAGLE_ERROR_OUT_OF_RANGE
        assert lib.lib.mbamdGetSubtreeRecomputeCounts(bd.inst.id + 1000, (C.c_long * 3)()) == bg.BEAGLE_ERROR_UNINITIALIZED_INSTANCE
    finally:
        bd.finalize()
    f64 = lk.BeagleDivision(division("mixed_15", 4), lib, double_precision=True)
    try:
        f64.LogLike(0)
        assert counts_of(f64.inst) == ((0, 0, 0), (0, 0, 0))
    finally:
        f64.finalize()


def test_counts_call_on_emulation(emu, monkeypatch):
    monkeypatch.setenv("MBAMD_NO_INLINE_PROGRAMS", "1")
    check_counts_call(emu)


@pytest.mark.gpu
def test_counts_call(gpu, monkeypatch):
    monkeypatch.setenv("MBAMD_NO_INLINE_PROGRAMS", "1")
    check_counts_call(gpu)


# ---- readers on mixed_15: pitchforks P1 P2, balanced fours Q1 Q2 --------------------------------------------------------------------------
def parts(t):
    """(P1, Q1, Q2, P2) of mixed_15: the nodes of three and four tips in post-order"""
    n = subtree_tips(t)
    big = [p for p in t.int_down_pass if n[p] in (3, 4)]
    assert [n[p] for p in big] == [3, 4, 4, 3]
    return big


def overwrite(bd):
    """test_walk4_tip_pairs.overwrite, reading every flagged node: (a) matrices overwritten behind an evaluation, (b) behind a list
    that no integration followed"""
    t, inst = bd.div.tree, bd.inst
    pairs, subs = flagged(t)
    read = subs + pairs                          # (a subtree before the tip pairs inside it)
    arrays = [np.float64(bd.LogLike(0))]
    bd.AcceptMove(0)
    nodes = [p for p in t.all_down_pass]
    inst.update_transition_matrices(bd.cijkIndex[0], [bd.tiProbsIndex[0][p] for p in nodes], [3.1 * t.length[p] + 0.2 for p in nodes])
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in read]
    c1 = counts_of(inst)
    bd.FlipSiteScalerSpace(0)
    inst.reset_scale_factors(bd.siteScalerIndex[0])
    bd.TouchAllTreeNodes(0)
    bd.TreeTiProbs_Beagle(0)
    bd.TreeCondLikes_Beagle_Always_Rescale(0)
    bd.ClearTouches(0)
    junk = np.tile(np.full((4, 4), 0.25), (bd.div.ncat, 1, 1))
    for p in nodes:
        inst.set_transition_matrix(bd.tiProbsIndex[0][p], junk)
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in read]
    return arrays, [c1, counts_of(inst)]


def check_overwrite(lib, monkeypatch):
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), TO_WALK, overwrite)
    assert counts == [((6, 6, 6), (4, 4, 4)), ((12, 12, 12), (8, 8, 8))], counts


def tip_overwritten(bd):
    """a tip of Q1 gets new states, a tip of Q2 partials in its place: the recipes that name it -- its tip pair AND the four -- are made
    first, in one launch; the others stay"""
    t, inst = bd.div.tree, bd.inst
    P1, Q1, Q2, P2 = parts(t)
    arrays = [np.float64(bd.LogLike(0))]
    counts = [counts_of(inst)]

    def a_tip(p):
        while p >= t.ntaxa:
            p = t.left[p]
        return p
    x = a_tip(Q1)
    inst.set_tip_states(x, np.zeros(NPAT, dtype=np.int32))
    counts.append(counts_of(inst))
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in (Q1, t.anc[x])]
    y = a_tip(Q2)
    inst.set_tip_partials(y, np.full((NPAT, 4), 0.3))
    counts.append(counts_of(inst))
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in (t.anc[y], Q2)]
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
    counts.append(counts_of(inst))
    return arrays, counts


def check_tip_overwritten(lib, monkeypatch):
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), TO_WALK, tip_overwritten)
    assert counts[0] == ((6, 0, 0), (4, 0, 0))
    assert counts[1] == ((6, 1, 1), (4, 1, 1))
    assert counts[2] == ((6, 2, 2), (4, 2, 2))
    assert counts[3] == ((6, 6, 6), (4, 4, 4))


def inner_overwritten(bd):
    """the buffer of a tip pair INSIDE an unstored four is overwritten by a list of its own (one operation: a path, stored); then the
    four is read: its recipe makes the tip pair's old result again on the way, which must land nowhere -- the buffer keeps what the
    list wrote"""
    t, inst = bd.div.tree, bd.inst
    P1, Q1, Q2, P2 = parts(t)
    arrays = [np.float64(bd.LogLike(0))]
    counts = [counts_of(inst)]
    a, b = t.left[Q1], t.right[Q1]
    assert subtree_tips(t)[a] == 2 and subtree_tips(t)[b] == 2
    op = bd._op(0, b)
    op[0] = bd.condLikeIndex[0][a]               # (a's buffer := the operation of b)
    inst.update_partials(np.asarray([op], dtype=np.int32), NONE)
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in (Q1, a, b)]
    counts.append(counts_of(inst))
    return arrays, counts


def check_inner_overwritten(lib, monkeypatch):
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), TO_WALK, inner_overwritten)
    assert counts == [((6, 0, 0), (4, 0, 0)), ((6, 1, 1), (4, 1, 1))], counts


def partial_updates(bd):
    """branch moves behind a whole-tree evaluation (the lists are the path kernels')"""
    t, inst = bd.div.tree, bd.inst
    P1, Q1, Q2, P2 = parts(t)
    arrays, counts, lists = [np.float64(bd.LogLike(0))], [], []
    bd.AcceptMove(0)

    def note():
        counts.append(counts_of(inst))
        lists.append(inst.get_list_counts()[:4])

    def tip_of(p, right=False):
        while p >= t.ntaxa:
            p = t.right[p] if right else t.left[p]
        return p
    note()                                       # ((6, 0, 0), (4, 0, 0))
    # the path above a tip of P1: its siblings are a tip, Q1 (four tips, unstored) and the other half; fused with its log-likelihood
    arrays += tp.branch_move(bd, [tip_of(P1)], 2.5)
    note()                                       # Q1 made
    bd.AcceptMove(0)
    # the path above a tip of Q2: its siblings are a tip, a tip pair and P2 (three tips), both made by one launch; on its own (k_path4)
    arrays += tp.branch_move(bd, [tip_of(Q2)], 0.4, fused=False)
    note()
    bd.AcceptMove(0)
    # a forked path: the arms above a tip of Q1 (its sibling tip pair is still unstored) and a tip of P2 join at the top
    arrays += tp.branch_move(bd, [tip_of(Q1), tip_of(P2)], 1.7)
    note()
    # rejected: back to the buffers of the state before; the whole tree into the other buffers (six tip pairs and four subtrees more
    # are left unstored there), rejected too; then the path above the other tip pair of Q1: its one unstored sibling is the tip pair
    # (5,6) of the FIRST evaluation, whose recipe the second left alone (P1 was written by the first move, the halves are stored).
    # Siblings of three and four tips across a reject and restore: restored_moves, below
    bd.ResetFlips(0)
    bd.TouchAllTreeNodes(0)
    arrays.append(np.float64(bd.LogLike(0)))
    note()
    bd.ResetFlips(0)
    arrays += tp.branch_move(bd, [tip_of(Q1, right=True)], 3.0)
    note()
    bd.AcceptMove(0)
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
    note()
    return arrays, (counts, lists)


def check_partial_updates(lib, monkeypatch):
    res = {}

    def scenario(bd):
        arrays, (counts, lists) = partial_updates(bd)
        res[tp.stores_everything()] = lists
        return arrays, counts
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), TO_WALK, scenario)
    print("partial updates: list counters (lists, paths, forked, fused) %s" % (res[False],))
    assert res[True] == res[False]                                   # the same kernels in both builds
    assert counts[0] == ((6, 0, 0), (4, 0, 0))
    assert counts[1] == ((6, 0, 0), (4, 1, 1))                       # Q1, the sibling of four tips
    assert counts[2] == ((6, 1, 1), (4, 2, 2))                       # a tip pair and P2 in ONE launch
    assert counts[3] == ((6, 2, 2), (4, 2, 2))                       # the tip pair beside the arm inside Q1
    assert counts[4] == ((12, 2, 2), (8, 2, 2))                      # the other flip state: a whole-tree launch reads tips alone
    assert counts[5] == ((12, 3, 3), (8, 2, 2))                      # the tip pair (5,6) of the first evaluation
    assert counts[6] == ((12, 4, 4), (8, 2, 2))                      # of all current buffers only (13,14) was still unstored
    lists = res[False]
    assert lists[1] == (2, 1, 0, 1)                                  # k_path4_lnl
    assert lists[2] == (3, 2, 0, 1)                                  # k_path4
    assert lists[3] == (4, 3, 1, 2)                                  # forked


def restored_moves(bd):
    """the two evaluations first -- the whole tree into either set of buffers, the second rejected --, so that every move below finds
    the siblings of its path as the FIRST evaluation left them, and the second evaluation's recipes beside them in the other buffers:
    a path whose sibling is P2 (three tips) fused with its log-likelihood (k_path4_lnl), rejected; a path whose sibling is Q1 (four
    tips) on its own (k_path4); then the other flip state's recipes are read, and every current buffer"""
    t, inst = bd.div.tree, bd.inst
    P1, Q1, Q2, P2 = parts(t)
    arrays, counts, lists = [np.float64(bd.LogLike(0))], [], []
    bd.AcceptMove(0)

    def note():
        counts.append(counts_of(inst))
        lists.append(inst.get_list_counts()[:4])

    def tip_of(p):
        while p >= t.ntaxa:
            p = t.left[p]
        return p
    bd.TouchAllTreeNodes(0)
    arrays.append(np.float64(bd.LogLike(0)))
    note()                                       # ((12, 0, 0), (8, 0, 0)): nothing of either state is stored
    bd.ResetFlips(0)
    # the path above a tip of Q2: its siblings are a tip, the other tip pair of Q2, P2 (three tips, unstored) and the other half
    arrays += tp.branch_move(bd, [tip_of(Q2)], 0.4)
    note()                                       # the tip pair and P2 in ONE launch
    bd.ResetFlips(0)
    # the path above a tip of P1: its siblings are two tips, Q1 (four tips, unstored) and the other half
    arrays += tp.branch_move(bd, [tip_of(P1)], 2.5, fused=False)
    note()                                       # Q1 alone
    bd.AcceptMove(0)
    # the second evaluation's Q1 and P2, in the buffers that are the scratch ones now: nothing above touched them
    arrays += [inst.get_partials(bd.condLikeScratchIndex[p]) for p in (Q1, P2)]
    note()
    arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
    note()                                       # still unstored: (5,6) (7,8) (9,10) (13,14) and Q2
    return arrays, (counts, lists)


def check_restored_moves(lib, monkeypatch):
    res = {}

    def scenario(bd):
        arrays, (counts, lists) = restored_moves(bd)
        res[tp.stores_everything()] = lists
        return arrays, counts
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), TO_WALK, scenario)
    print("restored moves: list counters (lists, paths, forked, fused) %s" % (res[False],))
    assert res[True] == res[False]                                   # the same kernels in both builds
    assert counts[0] == ((12, 0, 0), (8, 0, 0))
    assert counts[1] == ((12, 1, 1), (8, 1, 1))                      # P2, the sibling of three tips, with the tip pair (11,12)
    assert counts[2] == ((12, 1, 1), (8, 2, 2))                      # Q1, the sibling of four tips
    assert counts[3] == ((12, 1, 1), (8, 4, 4))                      # the other flip state's recipes
    assert counts[4] == ((12, 5, 5), (8, 5, 5))
    lists = res[False]
    assert lists[0] == (2, 0, 0, 0)
    assert lists[1] == (3, 1, 0, 1)                                  # k_path4_lnl
    assert lists[2] == (4, 2, 0, 1)                                  # k_path4
    assert lists[3] == lists[4] == lists[2]


def reader_edge(bd):
    """the edge log-likelihood and the branch-length derivatives with an unstored four, then an unstored pitchfork, as the child end"""
    t, inst = bd.div.tree, bd.inst
    P1, Q1, Q2, P2 = parts(t)
    bd.LogLike(0)
    rc, lnl = inst.calculate_edge_log_likelihoods([bd.condLikeIndex[0][t.root_left]], [bd.condLikeIndex[0][Q1]], [bd.tiProbsIndex[0][Q1]],
                                                  [bd.cijkIndex[0]], [bd.cijkIndex[0]], [bd.siteScalerIndex[0]])
    assert rc == 0
    out = [np.float64(lnl), inst.get_site_log_likelihoods().copy()]
    c = [counts_of(inst)]
    pcopy, m1, m2 = (bd.tiProbsScratchIndex[i] for i in (0, 1, 2))
    inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [0.07], first=[m1], second=[m2])
    rc, lnl, d1, d2 = inst.calculate_edge_derivatives([bd.condLikeIndex[0][t.root_left]], [bd.condLikeIndex[0][P2]], [pcopy], [m1], [m2],
                                                      [bd.cijkIndex[0]], [bd.cijkIndex[0]], [bd.siteScalerIndex[0]])
    assert rc == 0
    s1, s2 = inst.get_site_derivatives()
    return out + [np.array([lnl, d1, d2]), inst.get_site_log_likelihoods().copy(), s1, s2], c + [counts_of(inst)]


def reader_cross_products(bd):
    bd.LogLike(0)
    return [bd.RateMatrixCrossProducts(0)], [counts_of(bd.inst)]


def reader_scaled(bd):
    t, inst = bd.div.tree, bd.inst
    bd.LogLike(0)
    out = []
    for x in parts(t)[:2]:
        out += list(inst.get_scaled_partials(bd.condLikeIndex[0][x], bd.siteScalerIndex[0]))
    return out, [counts_of(inst)]


def with_both(reader):
    def run(bd):
        arrays, _ = reader(bd)
        return arrays, [counts_of(bd.inst)]
    return run


# name -> (scenario, BeagleDivision keywords, the counters at the end)
READERS = {
    "edge": (reader_edge, {}, [((6, 0, 0), (4, 1, 1)), ((6, 0, 0), (4, 2, 2))]),
    "gradient": (with_both(tp.reader_gradient), {"pre_order": True}, [((6, 6, 1), (4, 4, 1))]),       # every sibling is read: one launch
    "cross_products": (reader_cross_products, {"pre_order": True}, [((6, 6, 1), (4, 4, 1))]),
    "final_pass": (with_both(tp.reader_final_pass), {}, [((6, 6, 6), (4, 4, 4))]),                    # one operation, one launch each
    "scaled": (reader_scaled, {}, [((6, 0, 0), (4, 2, 2))]),
}


def check_reader(lib, monkeypatch, name):
    scenario, kw, want = READERS[name]
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), TO_WALK, scenario, **kw)
    assert counts == want, (name, counts)


def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 130 patterns: the counters are the sums over the children"""
    def scenario(bd):
        assert bd.inst.child_count() == 2
        t = bd.div.tree
        arrays = tp.evaluation_state(bd, bd.LogLike(0))
        c = [counts_of(bd.inst)]
        arrays += [bd.inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
        return arrays, c + [counts_of(bd.inst)]
    counts = run_ab(lib, monkeypatch, division("mixed_15", 4), dict(TO_WALK, MBAMD_SHARD="2"), scenario)
    assert counts == [((12, 0, 0), (8, 0, 0)), ((12, 12, 12), (8, 8, 8))], counts


CHECKS = {"inner_overwritten": check_inner_overwritten, "overwritten_matrices": check_overwrite, "tip_overwritten": check_tip_overwritten, "partial_updates": check_partial_updates,
          "restored_moves": check_restored_moves,
          "sharded": check_sharded}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_scenario_on_emulation(emu, monkeypatch, name):
    CHECKS[name](emu, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CHECKS))
def test_scenario(gpu, monkeypatch, name):
    CHECKS[name](gpu, monkeypatch)


@pytest.mark.parametrize("name", sorted(READERS))
def test_reader_on_emulation(emu, monkeypatch, name):
    check_reader(emu, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(READERS))
def test_reader(gpu, monkeypatch, name):
    check_reader(gpu, monkeypatch, name)
