"""The per-kind loop bodies of the plain 4-state tree-walk kernel (k_walk4_t<Walk4Args, true>, mbamd_walk4.h): the host gives every
operation of a plain plan a kind number for its pair of child kinds (MBAMD_W4_KIND_*: a child is a compact tip, the forwarded result
or an LDS slot), the kernel dispatches on it once per entry and runs a body that tests neither TIP nor FWD; pairs without a body of
their own run the general one.

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on fibers);
  * GPU (`gpu`): the product library on a MI355X.

The A/B partner is MBAMD_NO_PLAIN_WALK=1: the same lists on the generic kernel, which reads the TIP / FWD flags and nothing of the kind
number.  Every case builds the same division twice, with the switch and without, and compares BITWISE after every evaluation: the
log-likelihood, the per-site values, the partials of every interior node, every node's exponent buffer and the cumulative buffer;
mbamdGetWalkCounts says that the plain kernel ran.  Both builds set MBAMD_NO_INLINE_PROGRAMS, MBAMD_NO_PATH4 and MBAMD_WALK_WAVES=1 --
the smallest lists that reach the plain kernel through a device buffer (tests/test_walk4_plain.py has the reasons).  130 patterns are
two full pattern blocks and one of 2 lanes; K = 4 and K = 1.

Which tree yields which kinds (child 1 = left, child 2 = right; taxon 1 is the calculation root; the scheduler forwards the result an
operation's parent consumes next and keeps the others in LDS slots):
  ladder_tip_first   (2, (3, (4, ... (N-1, N))))      one (tip, tip), then (tip, fwd) all the way up
  ladder_tip_last    ((((N, N-1), ...), 3), 2)        one (tip, tip), then (fwd, tip)
      9 taxa = 7 operations (odd: the last one is the peeled entry), 10 taxa = 8 (even): each kind is once the peeled entry or the
      last of the loop, once inside it
  balanced / balanced_mirror, 8 and 16 taxa            cherries (tip, tip) with KEEP (the first of two siblings) and without (the
      second: forwarded); a half of three tips is (tip, fwd) in one tree and (fwd, tip) in its mirror image; the joins of two interior
      children: one sibling waits in a slot, the other is forwarded -- (slot, fwd) in both trees and (fwd, slot) in the unmirrored one
      (the scheduler chooses which subtree goes first), at 16 taxa with KEEP (an inner join) and without (the join below the root)
  random 33 taxa                                       a mix in no particular order
  same_child_twice   balanced 16, one join's operation rewritten to name its first child's buffer as both children: (fwd, fwd) has no
      body of its own -- the general body
Scale modes: rescaling everywhere (twice: a fresh cumulative buffer, then sums added), nowhere, and at every third node.  NOSTORE: the
tip pairs are flagged as shipped, and unflagged in the cases that set MBAMD_STORE_TIP_PAIRS=1 in both builds.

That every body is reached by this module was shown on scratch emulation builds with one fault put into each body in turn (the first
factor's first component + 1): failing cases of the 21 -- (tip, tip) 21, (tip, fwd) 12 (ladder_tip_first, balanced, random),
(fwd, tip) 12 (ladder_tip_last, balanced_mirror, random), (slot, fwd) 13 (both balanced trees, random), (fwd, slot) 8 (balanced,
random), the general body 2 (same_child_twice, and nothing else: every other operation here has a body of its own).  No such build
is kept (profiles/walk4_kinds.txt).
"""
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import data as mbdata
from mrbayes_amd import likelihood as lk
from mrbayes_amd import tree as mbtree
from mrbayes_amd.division import build_division
from tests.hostemu import build_emu

NPAT = 130
TO_PLAIN = {"MBAMD_NO_INLINE_PROGRAMS": "1", "MBAMD_NO_PATH4": "1", "MBAMD_WALK_WAVES": "1"}
STORED = dict(TO_PLAIN, MBAMD_STORE_TIP_PAIRS="1")
SWITCH = "MBAMD_NO_PLAIN_WALK"
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


# ---- trees ---------------------------------------------------------------------------------------------------------------------
def _tip(i):
    return "%d:%.3f" % (i, 0.02 + 0.01 * (i % 7))


def ladder(ntaxa, tip_first):
    def join(tip, sub, i):
        sub = "%s:%.3f" % (sub, 0.03 + 0.01 * (i % 5))
        return "(%s,%s)" % ((tip, sub) if tip_first else (sub, tip))
    s = "(%s,%s)" % ((_tip(ntaxa - 1), _tip(ntaxa)) if tip_first else (_tip(ntaxa), _tip(ntaxa - 1)))
    for i in range(ntaxa - 2, 2, -1):
        s = join(_tip(i), s, i)
    return "(1:0.05,%s);" % join(_tip(2), s, 2)[1:-1]


def balanced(ntaxa, mirror):
    def pair(a, b):
        return "%s,%s" % ((b, a) if mirror else (a, b))

    def sub(tips):
        if len(tips) == 1:
            return _tip(tips[0])
        h = len(tips) // 2
        return "(%s):%.3f" % (pair(sub(tips[:h]), sub(tips[h:])), 0.03 + 0.01 * (len(tips) % 5))
    rest = list(range(2, ntaxa + 1))
    h = len(rest) // 2
    return "(1:0.05,%s);" % pair(sub(rest[:h]), sub(rest[h:]))


def make_tree(shape, ntaxa):
    if shape == "ladder_tip_first":
        return mbtree.parse_newick(ladder(ntaxa, True), root_tip=0)
    if shape == "ladder_tip_last":
        return mbtree.parse_newick(ladder(ntaxa, False), root_tip=0)
    if shape == "balanced":
        return mbtree.parse_newick(balanced(ntaxa, False), root_tip=0)
    if shape == "balanced_mirror":
        return mbtree.parse_newick(balanced(ntaxa, True), root_tip=0)
    return mbtree.random_tree(ntaxa, 5, brlen=0.05)


_divisions = {}


def division(shape, ntaxa, ncat):
    """GTR (+G4 when ncat = 4), NPAT patterns, 5 % gaps everywhere; two tips carry ambiguity codes (0/1 tip partials: compact tips with
    two or three compatible states) in a fifth of their patterns.  Built once per shape and never changed."""
    key = (shape, ntaxa, ncat)
    if key not in _divisions:
        st = mbdata.synthetic_states(ntaxa, NPAT, 4, 17 + ntaxa, 0.15, 0.05)
        rng = np.random.default_rng(3)
        tip_states, tip_partials = [], []
        for t in range(ntaxa):
            if t in (1, ntaxa - 1):
                gap = st[t] >= 4
                p = np.zeros((NPAT, 4))
                p[np.arange(NPAT), np.where(gap, 0, st[t])] = 1.0
                extra = (rng.random((NPAT, 4)) < 0.4) & (rng.random(NPAT) < 0.2)[:, None]
                p[extra] = 1.0
                p[gap] = 1.0
                tip_states.append(None)
                tip_partials.append(p)
            else:
                tip_states.append(np.ascontiguousarray(st[t], dtype=np.int32))
                tip_partials.append(None)
        _divisions[key] = build_division("gtr", make_tree(shape, ntaxa), np.ones(NPAT), tip_states, tip_partials,
                                         revmat=[0.10, 0.30, 0.05, 0.08, 0.40, 0.07], pi=[0.35, 0.25, 0.15, 0.25],
                                         alpha=0.7 if ncat > 1 else None, ncat=ncat)
    return _divisions[key]


# ---- what an evaluation leaves behind, and the evaluation sequences --------------------------------------------------------------
def snapshot(bd, lnl):
    t = bd.div.tree
    out = [np.float64(lnl), bd.inst.get_site_log_likelihoods().copy()]
    for p in t.int_down_pass:
        out.append(bd.inst.get_partials(bd.condLikeIndex[0][p]))
        out.append(bd.inst.get_scale_exponents(bd.nodeScalerIndex[0][p]))
    out.append(bd.inst.get_scale_exponents(bd.siteScalerIndex[0]))
    return out


def seq_always(bd):
    """rescaling everywhere, twice: a fresh cumulative buffer (the kernel stores its sums), then every node touched again into the
    other buffers (the kernel adds its sums)"""
    yield bd.LogLike(0)
    bd.AcceptMove(0)
    bd.upDateCl[0] = [True] * bd.nNodes
    bd.upDateTi[0] = [True] * bd.nNodes
    yield bd.LogLike(0)


def seq_unscaled(bd):
    """the dynamic scheme's first evaluation: no operation names an exponent buffer, no cumulative buffer"""
    yield bd.LogLike(0)


def seq_chosen(bd):
    """unscaled, then the rescale-everything pass: SCALE_WRITE at every third node, the others unscaled, a cumulative buffer"""
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


def same_child_twice(seq):
    """the sequence `seq` on a division whose last join of two interior children names its FIRST child's buffer as both children
    (the second child's matrix stays): both are the forwarded result, a pair without a body of its own"""
    def run(bd):
        t = bd.div.tree
        node = [p for p in t.int_down_pass if t.left[p] >= t.ntaxa and t.right[p] >= t.ntaxa][-1]
        plain_op = bd._op

        def op(chain, p):
            o = plain_op(chain, p)
            if p == node:
                o[5] = o[3]
            return o
        bd._op = op
        yield from seq(bd)
    return run


# name -> (tree shape, taxa, categories, sequence, scaling, environment of both builds)
CASES = {}
for _shape in ("ladder_tip_first", "ladder_tip_last"):
    CASES[_shape + "_9_k4_always"] = (_shape, 9, 4, seq_always, ALWAYS, TO_PLAIN)
    CASES[_shape + "_10_k4_always"] = (_shape, 10, 4, seq_always, ALWAYS, TO_PLAIN)
    CASES[_shape + "_9_k1_chosen"] = (_shape, 9, 1, seq_chosen, DYNAMIC, TO_PLAIN)
    CASES[_shape + "_10_k1_unscaled_stored"] = (_shape, 10, 1, seq_unscaled, DYNAMIC, STORED)
for _shape in ("balanced", "balanced_mirror"):
    CASES[_shape + "_8_k4_always"] = (_shape, 8, 4, seq_always, ALWAYS, TO_PLAIN)
    CASES[_shape + "_16_k4_always"] = (_shape, 16, 4, seq_always, ALWAYS, TO_PLAIN)
    CASES[_shape + "_8_k1_unscaled"] = (_shape, 8, 1, seq_unscaled, DYNAMIC, TO_PLAIN)
    CASES[_shape + "_16_k1_chosen_stored"] = (_shape, 16, 1, seq_chosen, DYNAMIC, STORED)
CASES["random_33_k4_always"] = ("random", 33, 4, seq_always, ALWAYS, TO_PLAIN)
CASES["random_33_k1_chosen"] = ("random", 33, 1, seq_chosen, DYNAMIC, TO_PLAIN)
CASES["random_33_k4_always_stored"] = ("random", 33, 4, seq_always, ALWAYS, STORED)
CASES["same_child_twice_16_k4_always"] = ("balanced", 16, 4, same_child_twice(seq_always), ALWAYS, TO_PLAIN)
CASES["same_child_twice_16_k1_chosen"] = ("balanced_mirror", 16, 1, same_child_twice(seq_chosen), DYNAMIC, TO_PLAIN)


def run_case(lib, monkeypatch, name):
    shape, ntaxa, ncat, seq, scaling, env = CASES[name]
    div = division(shape, ntaxa, ncat)
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
            for lnl in seq(bd):
                after = bd.inst.get_walk_counts()
                deltas.append((after[0] - before[0], after[1] - before[1]))
                snaps.append(snapshot(bd, lnl))
                before = bd.inst.get_walk_counts()        # (reading an unstored tip pair back is a launch of the generic kernel)
        finally:
            bd.finalize()
        runs.append(snaps)
        counts.append(deltas)
    monkeypatch.delenv(SWITCH, raising=False)
    print("%s: walk launches (plain, generic) per evaluation %s / with %s=1 %s" % (name, counts[0], SWITCH, counts[1]))
    assert counts[0] == [(1, 0)] * len(counts[0]), (name, counts[0])           # the plain kernel ran, and nothing else
    assert counts[1] == [(0, 1)] * len(counts[1]), (name, counts[1])
    assert len(runs[0]) == len(runs[1]) >= 1
    for i, (x, y) in enumerate(zip(runs[0], runs[1])):
        assert len(x) == len(y)
        for j, (a, b) in enumerate(zip(x, y)):
            assert np.array_equal(a, b), (name, "evaluation", i, "item", j)
        assert np.isfinite(x[0]) and np.all(np.isfinite(x[1]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_walk4_kinds_on_emulation(emu, monkeypatch, name):
    run_case(emu, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_walk4_kinds(gpu, monkeypatch, name):
    run_case(gpu, monkeypatch, name)
