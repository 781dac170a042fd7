"""The plain instantiation of the 4-state tree-walk kernel (k_walk4_t<Walk4Args, true>, mbamd_walk4.h): whole-tree lists -- one wave,
every entry an operation, no prefetch, wait, barrier or stored exponent -- run on a copy of the kernel with that code compiled out.

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on fibers);
  * GPU (`gpu`): the product library on a MI355X.

The A/B partner is MBAMD_NO_PLAIN_WALK=1: the same lists on the generic kernel.  Every case builds the same division twice, with the
switch and without, and compares BITWISE after every evaluation: the log-likelihood, the per-site values, every interior partials
buffer, every node's exponent buffer and the cumulative buffer; mbamdGetWalkCounts says which kernel ran, evaluation by evaluation.

Which lists reach k_walk4_t<Walk4Args> at all is not this file's subject, and two rules of the engine stand in front of the small
trees here: a list that is a root-ward path (or two that join) runs on k_path4 -- every whole-tree list of 4 or 5 taxa is one -- and a
program of at most 96 entries travels in the kernel arguments (k_walk4_t<Walk4ArgsInline>, never plain: 33 taxa are 34 entries).  The
cases below therefore set MBAMD_NO_PATH4 / MBAMD_NO_INLINE_PROGRAMS where noted -- in BOTH builds, so that the plain switch is the only
difference.  A third rule is the launch geometry: with few pattern blocks a list of 32 operations or more is cut over several waves
(barriers: generic), so the 100-taxon case at 130 patterns sets MBAMD_WALK_WAVES=1; on the GPU the same tree at 40 000 patterns -- 2 500
single-wave workgroups by the geometry rule itself -- runs with nothing set but the A/B switch.
"""
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import data as mbdata
from mrbayes_amd import likelihood as lk
from mrbayes_amd import tree as mbtree
from mrbayes_amd.division import build_division
from tests.engine_checks import REL_FP64
from tests.hostemu import build_emu

NPAT = 130                   # three pattern blocks, the last with two live lanes; walk4_grid launches 8 K workgroups: 5 K leave at once
TO_WALK = {"MBAMD_NO_INLINE_PROGRAMS": "1"}                          # 33 taxa: the program through a device buffer
TO_WALK_TINY = {"MBAMD_NO_INLINE_PROGRAMS": "1", "MBAMD_NO_PATH4": "1"}   # 4 / 5 taxa: ... and not on the path kernel
SWITCH = "MBAMD_NO_PLAIN_WALK"


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


_divisions = {}


def balanced_tree(ntaxa):
    """taxon 1 (the calculation root) and two perfectly balanced halves of the others: the tree that needs the most live results
    for its size -- 32 tips keep four results alive besides the one in registers, so three LDS slots must evict"""
    def sub(tips):
        if len(tips) == 1:
            return "%d:%.3f" % (tips[0], 0.02 + 0.01 * (tips[0] % 7))
        h = len(tips) // 2
        return "(%s,%s):%.3f" % (sub(tips[:h]), sub(tips[h:]), 0.03 + 0.01 * (len(tips) % 5))
    rest = list(range(2, ntaxa + 1))
    h = len(rest) // 2
    return mbtree.parse_newick("(1:0.05,%s,%s);" % (sub(rest[:h]), sub(rest[h:])), root_tip=0)


def division(ntaxa, ncat, NPAT=NPAT):
    """GTR (+G4 when ncat = 4) on a random tree, NPAT patterns, 5 % gaps everywhere; two tips carry IUPAC-style ambiguity codes
    (0/1 tip partials: two or three compatible states) in a fifth of their patterns.  Built once per shape, never changed by a test
    that does not put it back."""
    key = (ntaxa, ncat, NPAT)
    if key not in _divisions:
        st = mbdata.synthetic_states(ntaxa, NPAT, 4, 17 + ntaxa, 0.15, 0.05)
        tr = balanced_tree(ntaxa) if ntaxa == 33 else mbtree.random_tree(ntaxa, 5, brlen=0.05)
        rng = np.random.default_rng(3)
        tip_states, tip_partials = [], []
        for t in range(ntaxa):
            if t in (1, ntaxa - 1):
                gap = st[t] >= 4
                p = np.zeros((NPAT, 4))
                p[np.arange(NPAT), np.where(gap, 0, st[t])] = 1.0
                extra = (rng.random((NPAT, 4)) < 0.4) & (rng.random(NPAT) < 0.2)[:, None]      # further compatible states
                p[extra] = 1.0
                p[gap] = 1.0
                tip_states.append(None)
                tip_partials.append(p)
            else:
                tip_states.append(np.ascontiguousarray(st[t], dtype=np.int32))
                tip_partials.append(None)
        _divisions[key] = build_division("gtr", tr, np.ones(NPAT), tip_states, tip_partials, revmat=[0.10, 0.30, 0.05, 0.08, 0.40, 0.07],
                                         pi=[0.35, 0.25, 0.15, 0.25], alpha=0.7 if ncat > 1 else None, ncat=ncat)
    return _divisions[key]


def snapshot(bd, lnl):
    """everything an evaluation leaves behind, in a fixed order"""
    t = bd.div.tree
    out = [np.float64(lnl), bd.inst.get_site_log_likelihoods().copy()]
    for p in t.int_down_pass:
        out.append(bd.inst.get_partials(bd.condLikeIndex[0][p]))
        out.append(bd.inst.get_scale_exponents(bd.nodeScalerIndex[0][p]))
    out.append(bd.inst.get_scale_exponents(bd.siteScalerIndex[0]))
    return out


# ---- the evaluation sequences: each yields (what the evaluation left, its log-likelihood) per evaluation -------------------------
def seq_always(bd):
    """MB_BEAGLE_SCALE_ALWAYS twice: a fresh cumulative buffer (reset: the kernel stores its sums), then every node touched without
    the everything-changed flag (the cumulative buffer is copied, the old exponents removed, the kernel ADDS its sums)."""
    yield bd.LogLike(0)
    bd.AcceptMove(0)
    bd.upDateCl[0] = [True] * bd.nNodes
    bd.upDateTi[0] = [True] * bd.nNodes
    yield bd.LogLike(0)


def seq_unscaled(bd):
    """the dynamic scheme's first evaluation: no operation names an exponent buffer, no cumulative buffer"""
    yield bd.LogLike(0)


def seq_dynamic(bd):
    """the dynamic scheme: unscaled; the rescale-everything pass (SCALE_WRITE at every third node, a cumulative buffer: plain); then
    the evaluation that divides by the stored exponents (SCALE_READ entries: generic), on the same instance"""
    yield bd.LogLike(0)
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
    yield lnl
    bd.AcceptMove(0)
    bd.TouchAllTreeNodes(0)
    yield bd.LogLike(0)


def seq_partial(bd):
    """a whole-tree evaluation, then a branch move: the list of the path above a deep tip reads children of the earlier launch"""
    t = bd.div.tree
    yield bd.LogLike(0)
    bd.AcceptMove(0)
    deep = max(range(t.ntaxa), key=lambda i: _depth(t, i))
    old = t.length[deep]
    t.length[deep] = old * 2.5
    try:
        bd.TouchBranch(0, deep)
        yield bd.LogLike(0)
    finally:
        t.length[deep] = old


def _depth(t, i):
    d = 0
    while t.anc[i] != -1:
        i = t.anc[i]
        d += 1
    return d


P, G = (1, 0), (0, 1)        # one launch of the plain / of the generic kernel
# name -> (taxa, categories, sequence, scaling, environment of both builds, walk launches per evaluation as shipped)
CASES = {
    # ---- lists that must run plain
    "always_k4_33": (33, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, TO_WALK, [P, P]),
    "always_k1_33": (33, 1, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, TO_WALK, [P, P]),
    "always_k4_4": (4, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, TO_WALK_TINY, [P, P]),          # 2 operations
    "always_k4_5": (5, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, TO_WALK_TINY, [P, P]),          # 3: odd, the peeled entry
    "always_k1_5": (5, 1, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, TO_WALK_TINY, [P, P]),
    "always_k4_100": (100, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, {"MBAMD_WALK_WAVES": "1"}, [P, P]),   # 98 operations: not inline
    "unscaled_k4_33": (33, 4, seq_unscaled, lk.MB_BEAGLE_SCALE_DYNAMIC, TO_WALK, [P]),
    "unscaled_k1_5": (5, 1, seq_unscaled, lk.MB_BEAGLE_SCALE_DYNAMIC, TO_WALK_TINY, [P]),
    # ---- lists that must not, and must still be right
    "dynamic_k4_33": (33, 4, seq_dynamic, lk.MB_BEAGLE_SCALE_DYNAMIC, TO_WALK, [P, P, G]),
    "slots3_k4_33": (33, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, dict(TO_WALK, MBAMD_MAX_LDS_SLOTS="3"), [G, G]),      # evictions: prefetch entries
    "waves2_k4_40": (40, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, dict(TO_WALK, MBAMD_WALK_WAVES="2"), [G, G]),         # barrier and padding
    "partial_k4_33": (33, 4, seq_partial, lk.MB_BEAGLE_SCALE_ALWAYS, dict(TO_WALK, MBAMD_NO_PATH4="1"), [P, G]),         # external children
}
ORACLE = {"always_k4_33", "always_k1_33", "always_k4_5", "always_k4_100"}        # (at least) one plain case per K against the oracle


def run_case(lib, monkeypatch, oracle, name, npat=NPAT):
    ntaxa, ncat, seq, scaling, env, shipped = CASES[name]
    div = division(ntaxa, ncat, npat)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    runs, counts = [], []
    for off in (False, True):
        if off:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        bd = lk.BeagleDivision(div, lib, scaling=scaling)
        try:
            snaps, deltas = [], []
            before = bd.inst.get_walk_counts()
            for i, lnl in enumerate(seq(bd)):
                after = bd.inst.get_walk_counts()
                deltas.append((after[0] - before[0], after[1] - before[1]))
                before = after
                snaps.append(snapshot(bd, lnl))
                if not off and oracle is not None and name in ORACLE:
                    want = oracle.tree_loglike(div, use_shortcuts=False)
                    print("%s evaluation %d: engine %.10f oracle %.10f" % (name, i, lnl, want))
                    assert abs(lnl - want) <= REL_FP64 * abs(want), (name, i, lnl, want)
        finally:
            bd.finalize()
        runs.append(snaps)
        counts.append(deltas)
    monkeypatch.delenv(SWITCH, raising=False)
    print("%s: walk launches (plain, generic) per evaluation %s / with %s=1 %s" % (name, counts[0], SWITCH, counts[1]))
    assert counts[0] == shipped, (name, counts[0], shipped)
    assert counts[1] == [(0, a + b) for a, b in shipped], (name, counts[1])
    assert len(runs[0]) == len(runs[1]) == len(shipped)
    for i, (x, y) in enumerate(zip(runs[0], runs[1])):
        assert len(x) == len(y)
        for j, (a, b) in enumerate(zip(x, y)):
            assert np.array_equal(a, b), (name, "evaluation", i, "item", j)
        assert np.isfinite(x[0]) and np.all(np.isfinite(x[1]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_walk_on_emulation(emu, oracle, monkeypatch, name):
    run_case(emu, monkeypatch, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_walk(gpu, oracle, monkeypatch, name):
    run_case(gpu, monkeypatch, oracle, name)


@pytest.mark.gpu
def test_plain_walk_as_shipped(gpu, monkeypatch):
    """100 taxa x 40 000 patterns, G4: 625 pattern blocks x 4 categories are single-wave workgroups by the geometry rule, 98 operations
    do not travel in the kernel arguments -- no switch but MBAMD_NO_PLAIN_WALK itself."""
    monkeypatch.setitem(CASES, "shipped", (100, 4, seq_always, lk.MB_BEAGLE_SCALE_ALWAYS, {}, [P, P]))
    try:
        run_case(gpu, monkeypatch, None, "shipped", npat=40000)
    finally:
        _divisions.pop((100, 4, 40000), None)


# ---- the export itself -------------------------------------------------------------------------------------------------------
def check_walk_counts_call(lib):
    div = division(5, 1)
    bd = lk.BeagleDivision(div, lib)
    try:
        assert bd.inst.get_walk_counts() == (0, 0)
        assert lib.lib.mbamdGetWalkCounts(bd.inst.id, None) == bg.BEAGLE_ERROR_OUT_OF_RANGE
        assert lib.lib.mbamdGetWalkCounts(bd.inst.id + 1000, (C.c_long * 2)()) == bg.BEAGLE_ERROR_UNINITIALIZED_INSTANCE
    finally:
        bd.finalize()
    f64 = lk.BeagleDivision(division(33, 4), lib, double_precision=True)
    try:
        f64.LogLike(0)
        assert f64.inst.get_walk_counts() == (0, 0)
        assert f64.inst.get_list_counts() == (0,) * 6
    finally:
        f64.finalize()


def test_walk_counts_call_on_emulation(emu):
    check_walk_counts_call(emu)


@pytest.mark.gpu
def test_walk_counts_call(gpu):
    check_walk_counts_call(gpu)
