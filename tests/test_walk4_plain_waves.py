"""Whole-tree 4-state lists on SEVERAL plain waves per pattern block (k_walk4_t<Walk4Args, true, true>, mbamd_walk4.h;
Walk4Builder::placePlainWaves, mbamd_walk4_host.h): the list is cut into phases, every wave runs the plain loop on its part, the workgroup
meets between the phases and a value that crosses waves travels through an LDS slot of the workgroup's pool -- a result left unstored
(MBAMD_W4_NOSTORE) included.

  * CPU (`not gpu`): the host-emulation build of the same sources (the waves of a workgroup are fibers that meet at the barriers);
  * GPU (`gpu`): the product library on a MI355X.

Everything is BITWISE, through the C ABI.  Every case runs the same calls three times -- W waves forced (MBAMD_WALK_WAVES=W), one wave
(MBAMD_WALK_WAVES=1: the plain loop as it was) and MBAMD_NO_PLAIN_WALK=1 at W waves (the generic kernel: barrier entries, values that
cross waves through HBM) -- and compares whatever it reads: lnL, site values, every exponent buffer, the cumulative buffer and the
partials of every interior node (which materialises every buffer the launch left unstored).  mbamdGetPlainWaveCounts says which W ran.

The rules that stand in front of small lists are switched off in ALL runs: MBAMD_NO_INLINE_PROGRAMS, MBAMD_NO_PATH4 where the list is a
path, MBAMD_WALK_SMALL_PHASE=1 (lists of fewer than 32 operations run on one wave otherwise) and MBAMD_WALK_PLAIN_MIN_OPS=1 (as shipped
a list runs the plain loop on several waves from 32 operations per wave).  Shapes: 65 patterns (two blocks, the second of one lane) and
130 (three, the last of two); K = 1 and 4; W = 2, 3, 4.
"""
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import data as mbdata
from mrbayes_amd import likelihood as lk
from mrbayes_amd import tree as mbtree
from mrbayes_amd.division import build_division
from tests.hostemu import build_emu
from tests import test_walk4_tip_pairs as tp
from tests import test_walk4_small_subtrees as ss

NONE = bg.BEAGLE_OP_NONE
ALWAYS, DYNAMIC = tp.ALWAYS, tp.DYNAMIC
SMALL = {"MBAMD_NO_INLINE_PROGRAMS": "1", "MBAMD_WALK_SMALL_PHASE": "1", "MBAMD_WALK_PLAIN_MIN_OPS": "1"}
SMALL_NO_PATH = dict(SMALL, MBAMD_NO_PATH4="1")
WAVES, GENERIC = "MBAMD_WALK_WAVES", "MBAMD_NO_PLAIN_WALK"


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def mirrored(s):
    """the mirror image of a newick string's tree below the calculation root: the children of every node in the other order"""
    def parse(i):
        if s[i] != "(":
            j = i
            while s[j] not in ",)":
                j += 1
            return s[i:j], j
        kids, i = [], i + 1
        while True:
            k, i = parse(i)
            kids.append(k)
            if s[i] == ")":
                return kids, i + 1
            i += 1

    def write(n, top=False):
        if isinstance(n, str):
            return n
        kids = [n[0]] + n[:0:-1] if top else n[::-1]              # (taxon 1 stays the calculation root)
        return "(" + ",".join(write(k) for k in kids) + ")"
    return write(parse(0)[0], top=True)


def balanced(first, count):
    if count == 1:
        return str(first)
    h = count // 2
    return "(%s,%s)" % (balanced(first, h), balanced(first + h, count - h))


NEWICK = {
    "balanced_8": "(1,%s,10)" % balanced(2, 8),                   # 8 operations: even
    "balanced_16": "(1,%s,18)" % balanced(2, 16),                 # 16
    "balanced_7": "(1,%s,9)" % balanced(2, 7),                    # 7: odd counts per wave
    # a tip pair A and a subtree of four tips B under R: the cut takes R into the second phase, A and B run on different waves, and one of
    # them reaches R through its slot from the other wave -- unstored, as the other is
    "crossing": "(1,((2,3),((4,5),(6,7))),8)",
    # the same twice, under a second-phase operation each, beside a third subtree
    "crossing_2": "(1,(((2,3),((4,5),(6,7))),(((8,9),(10,11)),(12,13))),((14,15),(16,(17,18))))",
}
TREES = {name: (lambda s=s: ss.newick(s)) for name, s in NEWICK.items()}
TREES.update({name + "_mirror": (lambda s=s: ss.newick(mirrored(s))) for name, s in NEWICK.items() if name != "balanced_7"})
TREES["ladder_9"] = lambda: mbtree.caterpillar_tree(9)            # cannot be cut: falls back to the generic kernel
TREES["random_33"] = lambda: mbtree.random_tree(33, 5, brlen=0.05)
TREES["mixed_15"] = lambda: ss.newick("(1,(((2,3),4),((5,6),(7,8))),(((9,10),(11,12)),((13,14),15)))")   # pitchforks and fours, as test_walk4_small_subtrees'
TREES["random_100"] = lambda: mbtree.random_tree(100, 5, brlen=0.05)
_divisions = {}


def division(name, ncat, npat):
    """GTR (+G4 when ncat = 4) over a tree of the table above, 5 % gaps; two tips carry ambiguity codes as 0/1 tip partials (kept as
    compact tips) -- the data of test_walk4_small_subtrees.division, in a table and a cache of this module's own"""
    key = (name, ncat, npat)
    if key not in _divisions:
        tree = TREES[name]()
        ntaxa = tree.ntaxa
        st = mbdata.synthetic_states(ntaxa, npat, 4, 17 + ntaxa, 0.15, 0.05)
        rng = np.random.default_rng(3)
        tip_states, tip_partials = [], []
        for t in range(ntaxa):
            if t in (1, ntaxa - 1):
                gap = st[t] >= 4
                p = np.zeros((npat, 4))
                p[np.arange(npat), np.where(gap, 0, st[t])] = 1.0
                extra = (rng.random((npat, 4)) < 0.4) & (rng.random(npat) < 0.2)[:, None]
                p[extra] = 1.0
                p[gap] = 1.0
                tip_states.append(None)
                tip_partials.append(p)
            else:
                tip_states.append(np.ascontiguousarray(st[t], dtype=np.int32))
                tip_partials.append(None)
        _divisions[key] = build_division("gtr", tree, np.ones(npat), tip_states, tip_partials,
                                         revmat=[0.10, 0.30, 0.05, 0.08, 0.40, 0.07], pi=[0.35, 0.25, 0.15, 0.25],
                                         alpha=0.7 if ncat > 1 else None, ncat=ncat)
    return _divisions[key]


# ---- the harness: the same scenario at W waves, at one wave and on the generic kernel ------------------------------------------------
def run_three(lib, monkeypatch, div, W, scenario, scaling=ALWAYS, env=SMALL_NO_PATH, extra=None, **kw):
    """scenario(bd) -> arrays.  Returns (walk counts, plain launches by W) of the run at W waves."""
    for k, v in dict(env, **(extra or {})).items():
        monkeypatch.setenv(k, v)
    runs = []
    for waves, generic in ((W, False), (1, False), (W, True)):
        monkeypatch.setenv(WAVES, str(waves))
        if generic:
            monkeypatch.setenv(GENERIC, "1")
        else:
            monkeypatch.delenv(GENERIC, raising=False)
        bd = lk.BeagleDivision(div, lib, scaling=scaling, **kw)
        try:
            assert bd.inst.get_plain_wave_counts() == (0,) * 8
            arrays = scenario(bd)
            runs.append((arrays, bd.inst.get_walk_counts(), bd.inst.get_plain_wave_counts()))
        finally:
            bd.finalize()
    monkeypatch.delenv(GENERIC, raising=False)
    monkeypatch.delenv(WAVES, raising=False)
    (a, wa, pa), (b, wb, pb), (c, wc, pc) = runs
    print("W = %d: walk counts %s, plain launches by W %s / one wave %s %s / generic %s %s" % (W, wa, pa, wb, pb, wc, pc))
    assert len(a) == len(b) == len(c)
    for j, (x, y, z) in enumerate(zip(a, b, c)):
        assert np.array_equal(x, y), ("W waves against one wave: item", j)
        assert np.array_equal(x, z), ("W waves against the generic kernel: item", j)
    assert all(np.all(np.isfinite(x)) for x in a)
    assert sum(pb[1:]) == 0 and pb[0] == wb[0]                       # one wave: every plain launch is of one wave
    assert wc[0] == 0 and sum(pc) == 0                               # the generic kernel: none
    assert sum(pa) == wa[0]
    return wa, pa


def everything(bd, scheme):
    """every evaluation of the scheme: lnL, site values, exponents, the cumulative buffer, then every interior node's partials"""
    t = bd.div.tree
    arrays, plain = [], 0
    for lnl, is_plain in scheme(bd):
        arrays += tp.evaluation_state(bd, lnl)
        arrays += [bd.inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
        plain += is_plain
    bd.plain_evaluations = plain
    return arrays


SCHEMES = [(tp.scheme_always, ALWAYS, 2), (tp.scheme_chosen, DYNAMIC, 2), (tp.scheme_nowhere, DYNAMIC, 1)]
STORE = [{"MBAMD_UNSTORED_TIPS": "4"}, {"MBAMD_UNSTORED_TIPS": "2"}, {"MBAMD_STORE_TIP_PAIRS": "1"}]
# every tree at W = 2, 3, 4; the scale mode (everywhere / unscaled, then every third node / nowhere), what is left unstored (subtrees
# of up to four tips / tip pairs / nothing), K and the pattern count rotate so that every value of each meets every W and every tree
# meets two values of each
# (the trees of up to nine operations have no cut into three: W = 2 only)
CASES = []
TWO_ONLY = {"balanced_7", "balanced_8", "balanced_8_mirror", "crossing", "crossing_mirror"}
for i, name in enumerate(sorted(set(TREES) - {"random_100"})):            # (random_100: test_as_shipped alone)
    for W in ((2,) if name in TWO_ONLY else (2, 3, 4)):
        j = i + W
        CASES.append((name, W, j % 3, (i + 2 * W) % 3, (1, 4)[(i + W // 2) % 2], (65, 130)[(i + W) % 2]))


def check_whole_tree(lib, monkeypatch, name, W, scheme, store, ncat, npat):
    make, scaling, plain = SCHEMES[scheme]
    div = division(name, ncat, npat)
    wa, pa = run_three(lib, monkeypatch, div, W, lambda bd: everything(bd, make), scaling=scaling, extra=STORE[store])
    # every plain evaluation ran W waves on the plain loop -- but a ladder, which cannot be cut: the generic kernel
    if name == "ladder_9":
        assert sum(pa) == 0 and wa[0] == 0 and wa[1] >= plain, (name, W, wa, pa)
    else:
        assert pa[W - 1] == plain and sum(pa) == plain, (name, W, pa)


@pytest.mark.parametrize("name,W,scheme,store,ncat,npat", CASES)
def test_whole_tree_on_emulation(emu, monkeypatch, name, W, scheme, store, ncat, npat):
    check_whole_tree(emu, monkeypatch, name, W, scheme, store, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,scheme,store,ncat,npat", CASES)
def test_whole_tree(gpu, monkeypatch, name, W, scheme, store, ncat, npat):
    check_whole_tree(gpu, monkeypatch, name, W, scheme, store, ncat, npat)


# ---- what is left unstored crosses waves, and is left unstored all the same --------------------------------------------------------
def check_unstored_counts(lib, monkeypatch, name, W):
    """the recompute counters of a launch on W waves are those of one wave: the same buffers left unstored, each made when it is read"""
    div = division(name, 4, 130)
    pairs, subs = ss.flagged(div.tree)
    assert pairs and subs
    for k, v in SMALL_NO_PATH.items():
        monkeypatch.setenv(k, v)
    seen = []
    for waves in (W, 1):
        monkeypatch.setenv(WAVES, str(waves))
        bd = lk.BeagleDivision(div, lib)
        try:
            arrays, counts = ss.whole_tree(bd, tp.scheme_always, "pre", 4)
            seen.append((arrays, counts, bd.inst.get_plain_wave_counts()))
        finally:
            bd.finalize()
    monkeypatch.delenv(WAVES, raising=False)
    (a, ca, pa), (b, cb, pb) = seen
    assert ca == cb and ca[-1][0][0] == 2 * len(pairs) and ca[-1][1][0] == 2 * len(subs)
    assert pa[W - 1] == 2 and pb[0] == 2
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


UNSTORED = [("crossing", 2), ("crossing_mirror", 2), ("crossing_2", 2), ("crossing_2", 3), ("crossing_2_mirror", 4), ("mixed_15", 2)]


@pytest.mark.parametrize("name,W", UNSTORED)
def test_unstored_counts_on_emulation(emu, monkeypatch, name, W):
    check_unstored_counts(emu, monkeypatch, name, W)


@pytest.mark.gpu
@pytest.mark.parametrize("name,W", UNSTORED)
def test_unstored_counts(gpu, monkeypatch, name, W):
    check_unstored_counts(gpu, monkeypatch, name, W)


# ---- readers behind such a launch: mixed_15 at two and three waves -------------------------------------------------------------------
def scenario_arrays(scenario):
    def run(bd):
        return scenario(bd)[0]
    return run


# a root-ward path over an unstored sibling, reject and restore; matrices overwritten before the read (the snapshot kernel read a
# program of several waves and its side table)
READERS = {"partial_updates": ss.partial_updates, "restored_moves": ss.restored_moves, "overwritten_matrices": ss.overwrite}


def check_reader(lib, monkeypatch, name, W):
    wa, pa = run_three(lib, monkeypatch, division("mixed_15", 4, 130), W, scenario_arrays(READERS[name]), env=SMALL)
    assert pa[W - 1] == 2 and sum(pa) == 2, pa                      # (each scenario evaluates the whole tree twice)


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("name", sorted(READERS))
def test_reader_on_emulation(emu, monkeypatch, name, W):
    check_reader(emu, monkeypatch, name, W)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("name", sorted(READERS))
def test_reader(gpu, monkeypatch, name, W):
    check_reader(gpu, monkeypatch, name, W)


# ---- one buffer as both children ---------------------------------------------------------------------------------------------------
def same_buffer_twice(bd):
    """balanced_16's list with the operations above the two halves of four reading ONE half as both children (the general kind; at two
    waves the cut is right there)"""
    t, inst = bd.div.tree, bd.inst
    n = ss.subtree_tips(t)
    bd.UpDateCijk(0)
    bd.TreeTiProbs_Beagle(0)
    ops = [bd._op(0, p) for p in t.int_down_pass]
    twice = 0
    for op, p in zip(ops, t.int_down_pass):
        if n[p] == 8:
            op[5] = op[3]
            op[6] = op[4]
            twice += 1
    assert twice >= 2
    inst.update_partials(np.asarray(ops, dtype=np.int32), NONE)
    return [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]


def check_same_buffer_twice(lib, monkeypatch, W):
    wa, pa = run_three(lib, monkeypatch, division("balanced_16", 4, 130), W, same_buffer_twice)
    assert pa[W - 1] == 1 and sum(pa) == 1, pa                      # (what is no longer read is a root of its own: a forest, cut over W waves)


@pytest.mark.parametrize("W", [2, 3])
def test_same_buffer_twice_on_emulation(emu, monkeypatch, W):
    check_same_buffer_twice(emu, monkeypatch, W)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 3])
def test_same_buffer_twice(gpu, monkeypatch, W):
    check_same_buffer_twice(gpu, monkeypatch, W)


# ---- fallback ------------------------------------------------------------------------------------------------------------------------
def check_fallback(lib, monkeypatch):
    """a pool of three slots does not hold the random tree's live values: evictions, so the generic kernel at two waves (three slots
    each) -- and the counts say so; the same list with the slots of the geometry rule runs the plain loop on two waves"""
    div = division("random_33", 4, 130)
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv(WAVES, "2")
    out = []
    for slots in ("3", None):
        if slots:
            monkeypatch.setenv("MBAMD_MAX_LDS_SLOTS", slots)
        else:
            monkeypatch.delenv("MBAMD_MAX_LDS_SLOTS", raising=False)
        bd = lk.BeagleDivision(div, lib)
        try:
            arrays = everything(bd, tp.scheme_always)
            out.append((arrays, bd.inst.get_walk_counts(), bd.inst.get_plain_wave_counts()))
        finally:
            bd.finalize()
    monkeypatch.delenv(WAVES, raising=False)
    (a, wa, pa), (b, wb, pb) = out
    print("three slots: %s %s; the rule's: %s %s" % (wa, pa, wb, pb))
    assert wa == (0, 2) and sum(pa) == 0
    assert wb == (2, 0) and pb[1] == 2
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_fallback_on_emulation(emu, monkeypatch):
    check_fallback(emu, monkeypatch)


@pytest.mark.gpu
def test_fallback(gpu, monkeypatch):
    check_fallback(gpu, monkeypatch)


def check_as_shipped(lib, monkeypatch, W):
    """nothing set but the wave count: 100 taxa are 98 operations -- 49 and 32 per wave run the plain loop on two and three waves, 24
    per wave do not (MBAMD_WALK_PLAIN_MIN_OPS)"""
    monkeypatch.setenv(WAVES, str(W))
    bd = lk.BeagleDivision(division("random_100", 4, 130), lib)
    try:
        bd.LogLike(0)
        want = (0,) * (W - 1) + (1,) + (0,) * (8 - W) if W < 4 else (0,) * 8
        assert bd.inst.get_plain_wave_counts() == want
        assert bd.inst.get_walk_counts() == ((1, 0) if W < 4 else (0, 1))
    finally:
        bd.finalize()


@pytest.mark.parametrize("W", [2, 3, 4])
def test_as_shipped_on_emulation(emu, monkeypatch, W):
    check_as_shipped(emu, monkeypatch, W)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 3, 4])
def test_as_shipped(gpu, monkeypatch, W):
    check_as_shipped(gpu, monkeypatch, W)


def check_counts_call(lib):
    import ctypes as C
    bd = lk.BeagleDivision(division("crossing", 1, 65), lib)
    try:
        assert lib.lib.mbamdGetPlainWaveCounts(bd.inst.id, None) == bg.BEAGLE_ERROR_OUT_OF_RANGE
        assert lib.lib.mbamdGetPlainWaveCounts(bd.inst.id + 1000, (C.c_long * 8)()) == bg.BEAGLE_ERROR_UNINITIALIZED_INSTANCE
    finally:
        bd.finalize()


def test_counts_call_on_emulation(emu):
    check_counts_call(emu)


@pytest.mark.gpu
def test_counts_call(gpu):
    check_counts_call(gpu)
