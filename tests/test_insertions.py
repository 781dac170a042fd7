"""Regraft and placement scores: the log-likelihood with a subtree attached at every listed point
(mbamdCalculateInsertionLogLikelihoods; csrc/mbamd_insertions.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference and the bound B -- derived from the operation counts, not tuned -- are in tests/insertion_reference.py:
    |log R_c - ref| <= B = (7 (S + 8) (1 + 2 h) + 7 (S + 8) + 16) u,        the weighted sums: sum_c weight_c B.
test_reference_against_whole_trees checks the reference itself against float64 pruning of the enlarged trees.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.insertion_reference import Candidate, bound, enlarged_site_likelihoods, lnl_bound, log_ratios, transition, tree_state
from tests.preorder_reference import reference as gradient_reference
from tests.preorder_reference import tip_vector, unit_roundoff
from tests.pruning_reference import NTAXA
from tests.test_derivatives import expected_layout

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
NONE = bg.BEAGLE_OP_NONE
SPARE = 40
TIP = 2                      # the tip whose own buffer serves as the compact-tip subtree
PENDANT = (0.07, 0.31)       # the two pendant branch lengths


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def random_subtree(div, seed=3):
    """partials [K][P][S] in (0.05, 1) that single precision holds exactly"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 1.0, size=(div.ncat, div.npatterns, div.nstates)).astype(np.float32).astype(np.float64)


def tip_subtree(div, tip=TIP):
    return np.broadcast_to(tip_vector(div, tip), (div.ncat, div.npatterns, div.nstates))


def split_nodes(t):
    """a tip branch, an interior branch and the top branch"""
    top = t.root_left
    tip = next(n for n in t.all_down_pass if t.left[n] < 0 and n != TIP)
    interior = next(n for n in t.all_down_pass if t.left[n] >= 0 and n != top)
    return [tip, interior, top]


# ---- 1. the reference, no engine code -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("states,ncat,npat", [(4, 4, 70), (20, 2, 70)])
def test_reference_against_whole_trees(states, ncat, npat):
    """log R_c of the formula against lnL_c(enlarged tree) - lnL_c(tree), both float64 pruning from scratch: every branch at the
    child end and three branches split at 0.3 of their length, a tip subtree and a random-partials subtree.  Both sides are double
    with |lnL| ~ 1e3: rounding stays near 1e-12 |lnL|, a wrong formula is off by O(1); asserted at 1e-9 (|lnL| + 1)."""
    st = tree_state(states, ncat, npat)
    div, t = st["div"], st["div"].tree
    L0 = enlarged_site_likelihoods(div, st["lengths"])
    assert np.allclose(L0, st["L"], rtol=1e-12, atol=0.0)
    lnl0 = float((div.weights * np.log(L0)).sum())
    worst, count = 0.0, 0
    for sub, tl in ((tip_subtree(div), PENDANT[0]), (random_subtree(div), PENDANT[1])):
        pendant = transition(div, tl)
        for node, split in [(n, 0.0) for n in t.all_down_pass] + [(n, 0.3) for n in split_nodes(t)]:
            cand = Candidate(node, split, sub, pendant)
            L1 = enlarged_site_likelihoods(div, st["lengths"], cand)
            lnl1 = float((div.weights * np.log(L1)).sum())
            ref = log_ratios(st, cand)
            assert np.all(np.abs(ref - (np.log(L1) - np.log(L0))) <= 1e-9 * (np.abs(np.log(L1)) + 1.0))
            worst = max(worst, abs(float((div.weights * ref).sum()) - (lnl1 - lnl0)) / (1e-9 * (abs(lnl1) + 1.0)))
            count += 1
    print("%d states x %d x %d: %d candidates, worst difference / (1e-9 (|lnL| + 1)) = %.3g" % (states, ncat, npat, count, worst))
    assert count == 2 * (2 * t.ntaxa - 3 + 3) and worst <= 1.0, worst


# ---- the engine side ------------------------------------------------------------------------------------------------------------
Item = collections.namedtuple("Item", "cand pre post post_matrix sub sub_matrix scale")


class Harness:
    """a division on an instance with spare buffers, after LogLike and the pre-order pass"""

    def __init__(self, lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
        self.st = tree_state(states, ncat, npat, ntaxa)
        self.div = div = self.st["div"]
        self.double_precision = double_precision
        self.u = unit_roundoff(div, gradient_reference(states, ncat, npat, ntaxa), double_precision)
        self.B = bound(div, self.st["h"], self.u)
        self.bd = bd = lk.BeagleDivision(div, lib, scaling=scaling, double_precision=double_precision, pre_order=True, spare=SPARE)
        self.inst = bd.inst
        self._buffer, self._matrix = bd.spareBufferIndex, bd.spareMatrixIndex
        if ntaxa == NTAXA:
            name = self.inst.details.implName.decode()
            assert expected_layout(states, ncat, double_precision) in name, name
        self.lnl = bd.LogLike(0)
        bd.AcceptMove(0)
        bd._PreOrderPass(0, "test_insertions")
        self.w = bd.cijkIndex[0]
        self.nodes = list(div.tree.all_down_pass)

    def finalize(self):
        self.bd.finalize()

    def buffer(self):
        self._buffer += 1
        assert self._buffer <= self.bd.spareBufferIndex + SPARE
        return self._buffer - 1

    def partials(self, values):
        idx = self.buffer()
        self.inst.set_partials(idx, values)
        return idx

    def matrix(self, values):
        self._matrix += 1
        assert self._matrix <= self.bd.spareMatrixIndex + SPARE
        self.inst.set_transition_matrix(self._matrix - 1, values)
        return self._matrix - 1

    def point(self, node, split):
        """(pre, post, postMatrix) of the point: off the child end, one pre-order operation into a scratch buffer"""
        bd, t = self.bd, self.div.tree
        if split == 0.0:
            return bd.preOrderIndex[node], bd.condLikeIndex[0][node], NONE
        tl = self.st["lengths"][node]
        upper, lower = self.matrix(transition(self.div, (1.0 - split) * tl)), self.matrix(transition(self.div, split * tl))
        dst = self.buffer()
        if node == t.root_left:
            op = [dst, NONE, NONE, bd.preOrderStartIndex, upper, NONE, NONE]
        else:
            p = t.anc[node]
            sib = t.right[p] if t.left[p] == node else t.left[p]
            op = [dst, NONE, NONE, bd.preOrderIndex[p], upper, bd.condLikeIndex[0][sib], bd.tiProbsIndex[0][sib]]
        self.inst.update_pre_partials(np.asarray([op], dtype=np.int32))
        return dst, bd.condLikeIndex[0][node], lower

    def subtrees(self):
        """[(reference column, buffer)]: the compact tip of the tree's own tip TIP, a partials subtree; and the two pendant matrices"""
        subs = [(tip_subtree(self.div), self.bd.condLikeIndex[0][TIP]), (random_subtree(self.div), None)]
        subs[1] = (subs[1][0], self.partials(subs[1][0]))
        mats = [(transition(self.div, tl), None) for tl in PENDANT]
        return subs, [(m, self.matrix(m)) for m, _ in mats]

    def item(self, node, split, sub, mat, scale=NONE, shift=0, where=None):
        pre, post, pm = where if where is not None else self.point(node, split)
        return Item(Candidate(node, split, sub[0], mat[0], shift), pre, post, pm, sub[1], mat[1], scale)

    def call(self, items, sites=True, inst=None):
        return (inst or self.inst).calculate_insertion_log_likelihoods(
            [i.pre for i in items], [i.post for i in items], [i.post_matrix for i in items], [i.sub for i in items],
            [i.sub_matrix for i in items], [i.scale for i in items], [self.w] * len(items), sites=sites)

    def reference(self, items):
        return np.stack([log_ratios(self.st, i.cand) for i in items])

    def check(self, items, label):
        """error / bound of the site values and of the sums of one call over `items`; asserts both <= 1"""
        w = self.div.weights
        rc, per, sums = self.call(items)
        ref = self.reference(items)
        assert rc == 0 and per.shape == ref.shape and np.all(np.isfinite(ref))
        e_site = float(np.abs(per - ref).max()) / self.B
        e_sum = float(np.abs(sums - (w[None, :] * ref).sum(1)).max()) / (self.B * float(w.sum()))
        print("%s: %d entries, error / bound: site values %.3f, sums %.3f" % (label, len(items), e_site, e_sum))
        assert e_site <= 1.0 and e_sum <= 1.0, (e_site, e_sum)
        return per, sums

    def mixed_list(self):
        """tip and interior post, a compact-tip and a partials subtree, postMatrix given and NONE, two subtree matrices -- in stretches
        that share a subtree and alternating"""
        t = self.div.tree
        (tip_sub, par_sub), (m1, m2) = self.subtrees()
        items = [self.item(n, 0.0, tip_sub, m1) for n in self.nodes] + [self.item(n, 0.0, par_sub, m2) for n in self.nodes]
        for i, n in enumerate(split_nodes(t)):
            where = self.point(n, 0.3)
            items.append(self.item(n, 0.3, tip_sub, m2 if i & 1 else m1, where=where))
            items.append(self.item(n, 0.3, par_sub, m1 if i & 1 else m2, where=where))
        for n in self.nodes[:4]:
            items += [self.item(n, 0.0, par_sub, m1), self.item(n, 0.0, tip_sub, m2)]
        assert any(t.left[i.cand.node] < 0 for i in items) and any(t.left[i.cand.node] >= 0 for i in items)
        return items


def label_of(states, ncat, npat, double_precision=False, ntaxa=NTAXA):
    return "%d states x %d x %d, %d taxa%s" % (states, ncat, npat, ntaxa, " fp64" if double_precision else "")


# ---- 2. per case, against the derived bound ---------------------------------------------------------------------------------------
def check_case(lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA):
    hs = Harness(lib, states, ncat, npat, double_precision, ntaxa)
    try:
        items = hs.mixed_list()
        before = hs.inst.get_insertion_launches()
        hs.check(items, label_of(states, ncat, npat, double_precision, ntaxa))
        after = hs.inst.get_insertion_launches()
        core = not double_precision and 16 <= states <= 64
        assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if core else (1, 0)), (before, after)
        # the binding of the division: the child end of every branch, one subtree
        score = hs.bd.InsertionLogLikelihoods(0, items[0].sub, items[0].sub_matrix)
        ref = (hs.div.weights[None, :] * hs.reference(items[:len(hs.nodes)])).sum(1)
        assert list(score) == hs.nodes
        assert max(abs(score[n] - ref[i]) for i, n in enumerate(hs.nodes)) <= hs.B * float(hs.div.weights.sum())
    finally:
        hs.finalize()


#        states, categories, patterns                     what it reaches
CASES = [(4, 4, 130),             # two full 64-pattern blocks plus 2 patterns
         (4, 9, 70),              # a second batch of categories
         (3, 2, 70),              # the plain kernel, a small state count
         (12, 2, 70),             # the plain kernel, the MFMA level layout
         (12, 6, 70),             # the plain kernel, the generic level layout
         (16, 2, 70),             # the matrix-core threshold
         (20, 4, 70),             # one tile, tree-walk tiles, a tail of 6 patterns
         (33, 1, 70),             # the second tile row and column hold one state
         (61, 1, 40),             # 2 x 2 tiles, no posteriors, a partial block
         (61, 2, 70)]             # 2 x 2 tiles with posteriors
CASES_F64 = [(4, 4, 130), (20, 2, 70)]


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_insertions_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_insertions_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_insertions(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_insertions_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


# ---- 3. an entry stands alone, bit for bit ----------------------------------------------------------------------------------------
def standalone_list(hs):
    """subtrees s1, s1, s2, s1 and two pendant matrices, over eleven entries: more than one run of the kernel"""
    (s1, s2), (m1, m2) = hs.subtrees()
    pattern = [(s1, m1), (s1, m1), (s2, m1), (s1, m2)]
    where = hs.point(split_nodes(hs.div.tree)[1], 0.3)
    items = [hs.item(n, 0.0, *pattern[i % 4]) for i, n in enumerate(hs.nodes[:10])]
    items.insert(5, hs.item(split_nodes(hs.div.tree)[1], 0.3, s2, m2, where=where))
    return items


def check_standalone(lib, monkeypatch, states, ncat, npat, double_precision=False):
    monkeypatch.delenv("MBAMD_POSTERIOR_NODES", raising=False)
    hs = Harness(lib, states, ncat, npat, double_precision)
    try:
        items = standalone_list(hs)
        rc, per, sums = hs.call(items)
        assert rc == 0 and np.all(np.isfinite(per))
        rc, rper, rsums = hs.call(items[::-1])
        assert rc == 0 and np.array_equal(rper[::-1], per) and np.array_equal(rsums[::-1], sums)
        for i, it in enumerate(items):
            rc, one, osum = hs.call([it])
            assert rc == 0 and np.array_equal(one[0], per[i]) and osum[0] == sums[i], i
        rc, none, nsums = hs.call(items, sites=False)
        assert rc == 0 and none is None and np.array_equal(nsums, sums)
    finally:
        hs.finalize()
    for cap in (1, 3):
        monkeypatch.setenv("MBAMD_POSTERIOR_NODES", str(cap))
        try:
            capped = Harness(lib, states, ncat, npat, double_precision)
            try:
                before = sum(capped.inst.get_insertion_launches())
                rc, cper, csums = capped.call(standalone_list(capped))
                assert sum(capped.inst.get_insertion_launches()) - before == (len(items) + cap - 1) // cap
                assert rc == 0 and np.array_equal(cper, per) and np.array_equal(csums, sums), cap
            finally:
                capped.finalize()
        finally:
            monkeypatch.delenv("MBAMD_POSTERIOR_NODES")


STANDALONE = [(4, 4, 70), (12, 2, 70), (20, 4, 70)]


@pytest.mark.parametrize("states,ncat,npat", STANDALONE)
def test_an_entry_stands_alone_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_standalone(emu, monkeypatch, states, ncat, npat)


def test_an_entry_stands_alone_double_precision_on_emulation(emu, monkeypatch):
    check_standalone(emu, monkeypatch, 4, 4, 70, double_precision=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", STANDALONE)
def test_an_entry_stands_alone(gpu, monkeypatch, states, ncat, npat):
    check_standalone(gpu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
def test_an_entry_stands_alone_double_precision(gpu, monkeypatch):
    check_standalone(gpu, monkeypatch, 4, 4, 70, double_precision=True)


# ---- 4. the matrix-core kernel against the plain one ------------------------------------------------------------------------------
MFMA_CASES = [(20, 4, 70), (33, 1, 70), (61, 2, 70)]


def check_mfma_against_generic(lib, monkeypatch, states, ncat, npat):
    """MBAMD_INSERT_GENERIC=1 sends 16 ... 64 states to the plain kernel: each result within B of the reference and within 2 B of the
    other; the launch counters tell which kernel ran"""
    results = []
    for generic in (False, True):
        monkeypatch.delenv("MBAMD_INSERT_GENERIC", raising=False)
        if generic:
            monkeypatch.setenv("MBAMD_INSERT_GENERIC", "1")
        try:
            hs = Harness(lib, states, ncat, npat)
            try:
                results.append(hs.check(hs.mixed_list(), label_of(states, ncat, npat) + (", plain kernel" if generic else ", matrix cores")))
                assert hs.inst.get_insertion_launches() == ((1, 0) if generic else (0, 1))
                B, W = hs.B, float(hs.div.weights.sum())
            finally:
                hs.finalize()
        finally:
            monkeypatch.delenv("MBAMD_INSERT_GENERIC", raising=False)
    (pm, sm), (pg, sg) = results
    e_site, e_sum = float(np.abs(pm - pg).max()) / (2.0 * B), float(np.abs(sm - sg).max()) / (2.0 * B * W)
    print("one against the other (2 B): site values %.3f, sums %.3f" % (e_site, e_sum))
    assert e_site <= 1.0 and e_sum <= 1.0


@pytest.mark.parametrize("states,ncat,npat", MFMA_CASES)
def test_mfma_against_generic_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_mfma_against_generic(emu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", MFMA_CASES)
def test_mfma_against_generic(gpu, monkeypatch, states, ncat, npat):
    check_mfma_against_generic(gpu, monkeypatch, states, ncat, npat)


# ---- 5. the engine against itself -----------------------------------------------------------------------------------------------
def check_against_enlarged_trees(lib, states, ncat, npat):
    """For a tip branch, an interior branch and the top branch: the enlarged tree built with ordinary beagleUpdatePartials operations
    on the same instance (a new node over the branch's node, across the identity, and the subtree, across the pendant matrix; then
    the path to the top); its root log-likelihood minus the tree's against outSumLogRatios, within the two bounds added"""
    hs = Harness(lib, states, ncat, npat, scaling=lk.MB_BEAGLE_SCALE_DYNAMIC)
    try:
        bd, inst, t, div = hs.bd, hs.inst, hs.div.tree, hs.div
        top = t.root_left
        (_, par_sub), (m1, _) = hs.subtrees()
        identity = hs.matrix(np.broadcast_to(np.eye(states), (ncat, states, states)))
        nodes = split_nodes(t)
        rc, _, sums = hs.call([hs.item(n, 0.0, par_sub, m1) for n in nodes], sites=False)
        assert rc == 0
        cl, ti = bd.condLikeIndex[0], bd.tiProbsIndex[0]
        slack = hs.B * float(div.weights.sum()) + 2.0 * lnl_bound(div, hs.st["h"], hs.u)
        for i, n in enumerate(nodes):
            cur, node = hs.buffer(), n
            ops = [[cur, NONE, NONE, par_sub[1], m1[1], cl[n], identity]]
            while node != top:
                p = t.anc[node]
                sib = t.right[p] if t.left[p] == node else t.left[p]
                dst = hs.buffer()
                ops.append([dst, NONE, NONE, cur, ti[node], cl[sib], ti[sib]])
                cur, node = dst, p
            inst.update_partials(np.asarray(ops, dtype=np.int32), NONE)
            rc, lnl1 = inst.calculate_edge_log_likelihoods([cur], [cl[t.root]], [ti[top]], [hs.w], [hs.w], [bd.siteScalerIndex[0]])
            assert rc == 0
            print("%s, branch of node %d: lnL %.6f -> %.6f, difference - sum of log ratios = %.3g (slack %.3g)" %
                  (label_of(states, ncat, npat), n, hs.lnl, lnl1, (lnl1 - hs.lnl) - sums[i], slack))
            assert abs((lnl1 - hs.lnl) - sums[i]) <= slack
    finally:
        hs.finalize()


SELF_CASES = [(4, 4, 70), (20, 2, 70)]


@pytest.mark.parametrize("states,ncat,npat", SELF_CASES)
def test_against_enlarged_trees_on_emulation(emu, states, ncat, npat):
    check_against_enlarged_trees(emu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", SELF_CASES)
def test_against_enlarged_trees(gpu, states, ncat, npat):
    check_against_enlarged_trees(gpu, states, ncat, npat)


# ---- 6. scale and range -----------------------------------------------------------------------------------------------------------
def check_tiny_subtree(lib, states, ncat, npat, double_precision=False):
    """a partials subtree whose columns lie near 2^-140 (2^-1000 in double precision), no scale buffer: the exponent is carried
    exactly, the bound is the same.  Eight-bit mantissas: single precision holds them exactly even as subnormals."""
    shift = -1000 if double_precision else -140
    hs = Harness(lib, states, ncat, npat, double_precision)
    try:
        rng = np.random.default_rng(5)
        mant = rng.integers(128, 256, size=(ncat, npat, states)).astype(np.float64) / 256.0
        _, (m1, m2) = hs.subtrees()
        sub = (mant, hs.partials(np.ldexp(mant, shift)))
        items = [hs.item(n, 0.0, sub, m1, shift=shift) for n in hs.nodes] + [hs.item(split_nodes(hs.div.tree)[1], 0.3, sub, m2, shift=shift)]
        per, _ = hs.check(items, label_of(states, ncat, npat, double_precision) + ", subtree at 2^%d" % shift)
        assert float(per.max()) < 0.5 * shift * np.log(2.0)
    finally:
        hs.finalize()


def check_scaled_clade(lib, states, ncat, npat, double_precision=False):
    """a clade of the tree under MB_BEAGLE_SCALE_ALWAYS as the subtree: its rescaled buffer, and its node scalers accumulated into a
    spare cumulative buffer passed as subtreeScaleIndices"""
    hs = Harness(lib, states, ncat, npat, double_precision)
    try:
        bd, t = hs.bd, hs.div.tree
        v = next(n for n in t.int_down_pass[::-1] if n != t.root_left and t.left[t.left[n]] + t.left[t.right[n]] > -2)
        clade, stack = [], [v]
        while stack:
            n = stack.pop()
            if t.left[n] >= 0:
                clade.append(n)
                stack += [t.left[n], t.right[n]]
        assert len(clade) >= 2
        cum = bd.spareScalerIndex
        hs.inst.reset_scale_factors(cum)
        hs.inst.accumulate_scale_factors([bd.nodeScalerIndex[0][n] for n in clade], cum)
        assert np.any(hs.inst.get_scale_exponents(cum) != 0)
        _, (m1, m2) = hs.subtrees()
        sub = (hs.st["post"][v], bd.condLikeIndex[0][v])
        items = [hs.item(n, 0.0, sub, m1, scale=cum) for n in hs.nodes] + [hs.item(split_nodes(t)[0], 0.3, sub, m2, scale=cum)]
        hs.check(items, label_of(states, ncat, npat, double_precision) + ", a rescaled clade of %d interior nodes" % len(clade))
    finally:
        hs.finalize()


def check_impossible(lib, states, ncat, npat, double_precision=False):
    """a subtree column that is zero on the one state the point allows (a tip with an observed state, the identity as the pendant
    matrix): -infinity there and in the sum, rc 0, and the neighbours untouched"""
    hs = Harness(lib, states, ncat, npat, double_precision)
    try:
        div = hs.div
        tip = split_nodes(div.tree)[0]
        st = np.asarray(div.tip_states[tip])
        c0 = int(np.nonzero(st < states)[0][3])
        values = random_subtree(div, seed=7)
        values[:, c0, st[c0]] = 0.0
        sub = (values, hs.partials(values))
        eye = np.broadcast_to(np.eye(states), (ncat, states, states)).copy()
        identity = (eye, hs.matrix(eye))
        _, (m1, _) = hs.subtrees()
        items = [hs.item(hs.nodes[-1], 0.0, sub, m1), hs.item(tip, 0.0, sub, identity), hs.item(tip, 0.0, sub, m1)]
        rc, per, sums = hs.call(items)
        ref = hs.reference(items)
        assert rc == 0 and per[1, c0] == -np.inf and ref[1, c0] == -np.inf and sums[1] == -np.inf
        keep = np.ones(per.shape, dtype=bool)
        keep[1, c0] = False
        assert np.all(np.isfinite(per[keep])) and float(np.abs(per[keep] - ref[keep]).max()) <= hs.B
        assert np.all(np.abs(sums[[0, 2]] - (div.weights[None, :] * ref[[0, 2]]).sum(1)) <= hs.B * float(div.weights.sum()))
    finally:
        hs.finalize()


def test_tiny_subtree_on_emulation(emu):
    check_tiny_subtree(emu, 4, 4, 70)
    check_tiny_subtree(emu, 20, 2, 70)
    check_tiny_subtree(emu, 12, 2, 70)
    check_tiny_subtree(emu, 4, 4, 70, double_precision=True)


def test_scaled_clade_on_emulation(emu):
    check_scaled_clade(emu, 4, 4, 70)
    check_scaled_clade(emu, 20, 2, 70)
    check_scaled_clade(emu, 12, 2, 70)
    check_scaled_clade(emu, 4, 4, 70, double_precision=True)


def test_deep_tree_on_emulation(emu):
    check_case(emu, 4, 4, 70, ntaxa=60)


def test_impossible_attachment_on_emulation(emu):
    check_impossible(emu, 4, 4, 70)
    check_impossible(emu, 20, 2, 70)
    check_impossible(emu, 4, 4, 70, double_precision=True)


@pytest.mark.gpu
def test_tiny_subtree(gpu):
    check_tiny_subtree(gpu, 4, 4, 70)
    check_tiny_subtree(gpu, 20, 2, 70)
    check_tiny_subtree(gpu, 12, 2, 70)
    check_tiny_subtree(gpu, 4, 4, 70, double_precision=True)


@pytest.mark.gpu
def test_scaled_clade(gpu):
    check_scaled_clade(gpu, 4, 4, 70)
    check_scaled_clade(gpu, 20, 2, 70)
    check_scaled_clade(gpu, 12, 2, 70)
    check_scaled_clade(gpu, 4, 4, 70, double_precision=True)


@pytest.mark.gpu
def test_deep_tree(gpu):
    check_case(gpu, 4, 4, 70, ntaxa=60)


@pytest.mark.gpu
def test_impossible_attachment(gpu):
    check_impossible(gpu, 4, 4, 70)
    check_impossible(gpu, 20, 2, 70)
    check_impossible(gpu, 4, 4, 70, double_precision=True)


# ---- 7. pattern shards ------------------------------------------------------------------------------------------------------------
def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 4 states x 4 categories x 130 patterns: two children, the site values those of the unsharded instance bit
    for bit, the sums within the bound"""
    results = []
    for shards in (None, "2"):
        monkeypatch.delenv("MBAMD_SHARD", raising=False)
        if shards:
            monkeypatch.setenv("MBAMD_SHARD", shards)
        try:
            hs = Harness(lib, 4, 4, 130)
            try:
                per, sums = hs.check(hs.mixed_list(), label_of(4, 4, 130) + (", %s shards" % shards if shards else ""))
                results.append((hs.inst.child_count(), per, sums))
                B, W = hs.B, float(hs.div.weights.sum())
            finally:
                hs.finalize()
        finally:
            monkeypatch.delenv("MBAMD_SHARD", raising=False)
    (n0, p0, s0), (n2, p2, s2) = results
    assert n0 == 1 and n2 == 2
    assert np.array_equal(p0, p2) and np.all(np.abs(s0 - s2) <= B * W)


def test_sharded_insertions_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_insertions(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5


def check_argument_errors(lib, double_precision=False):
    """Every bad call returns its code and leaves the output arrays as they were; returns (status, message) of each, in order: the
    two engines run one body, so they answer alike -- check_engines_agree."""
    seen = []
    st = tree_state(4, 2, 130)
    div, t = st["div"], st["div"].tree
    nodes = list(t.all_down_pass)
    n = len(nodes)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True, spare=4)
    try:
        inst = bd.inst

        def raw(lists, count=None, outputs=(True, True)):
            arrays = [None if v is None else np.asarray(v, dtype=np.int32) for v in lists]
            per, sums = np.full((n, 130), SENTINEL), np.full(n, SENTINEL)
            rc = inst.lib.mbamdCalculateInsertionLogLikelihoods(
                inst.id, *[None if a is None else a.ctypes.data_as(_ip) for a in arrays], n if count is None else count,
                per.ctypes.data_as(_dp) if outputs[0] else None, sums.ctypes.data_as(_dp) if outputs[1] else None)
            return rc, per, sums

        def refused(code, lists, count=None):
            rc, per, sums = raw(lists, count)
            assert rc == code, (rc, code, lib.last_error())
            assert lib.last_error() and np.all(per == SENTINEL) and np.all(sums == SENTINEL)
            seen.append((rc, lib.last_error()))

        def lists(**change):
            base = dict(pres=[bd.preOrderIndex[x] for x in nodes], posts=[bd.condLikeIndex[0][x] for x in nodes], pms=[NONE] * n,
                        subs=[bd.condLikeIndex[0][TIP]] * n, sms=[bd.tiProbsIndex[0][TIP]] * n, scales=[NONE] * n, weights=[bd.cijkIndex[0]] * n)
            base.update(change)
            return [base[key] for key in ("pres", "posts", "pms", "subs", "sms", "scales", "weights")]

        # more than one category and no log-likelihood call yet
        refused(bg.BEAGLE_ERROR_GENERAL, lists())
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd._PreOrderPass(0, "test_insertions")
        rc, per, sums = raw(lists())
        assert rc == 0 and np.all(np.isfinite(per)) and np.all(np.isfinite(sums)) and not np.any(per == SENTINEL)
        unwritten, nmat, nscale = bd.spareBufferIndex + 1, bd.spareMatrixIndex + 4, bd.spareScalerIndex + 4
        # another weights index; an unflagged pre-order buffer; unreadable post and subtree buffers
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(weights=[bd.cijkScratchIndex] * n))
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(pres=[bd.preOrderStartIndex] * n))
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(pres=[bd.condLikeIndex[0][t.root_left]] * n))
        for bad in (unwritten, -1, 10 ** 6):
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(posts=[bad] * n))
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(subs=[bad] * n))
        # a matrix or scale index out of range; a subtree matrix of BEAGLE_OP_NONE
        for bad in (nmat, -2):
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(pms=[NONE] * (n - 1) + [bad]))
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(sms=[bd.tiProbsIndex[0][TIP]] * (n - 1) + [bad]))
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(scales=[NONE] * (n - 1) + [bad - nmat + nscale if bad > 0 else bad]))
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(sms=[NONE] * n))
        # NULL index arrays with count > 0; count < 0
        for missing in range(7):
            broken = lists()
            broken[missing] = None
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, broken)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, lists(), count=-1)
        # count == 0 succeeds (NULL arrays too) and writes nothing; both outputs NULL succeed after the checks
        for empty in (lists(), [None] * 7):
            rc, per, sums = raw(empty, count=0)
            assert rc == 0 and np.all(per == SENTINEL) and np.all(sums == SENTINEL)
        assert raw(lists(), outputs=(False, False))[0] == 0
        assert raw(lists(posts=[unwritten] * n), outputs=(False, False))[0] == bg.BEAGLE_ERROR_OUT_OF_RANGE
        rc, per, sums = raw(lists(), outputs=(True, False))
        rc2, per2, sums2 = raw(lists(), outputs=(False, True))
        assert rc == 0 and rc2 == 0 and np.all(sums == SENTINEL) and np.all(per2 == SENTINEL) and np.all(np.isfinite(per)) and np.all(np.isfinite(sums2))
        # the latest log-likelihood call had two subsets
        top = t.root_left
        one = dict(parents=[bd.condLikeIndex[0][top]], children=[bd.condLikeIndex[0][t.root]], probs=[bd.tiProbsIndex[0][top]],
                   weights=[bd.cijkIndex[0]], freqs=[bd.cijkIndex[0]], cums=[bd.siteScalerIndex[0]])
        inst.calculate_edge_log_likelihoods(**{key: value * 2 for key, value in one.items()})
        refused(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, lists())
        inst.calculate_edge_log_likelihoods(**one)
        assert raw(lists())[0] == 0
    finally:
        bd.finalize()
    # a multi-partition instance does not serve it
    N, S, K, P = NTAXA, 4, 2, 130
    flags = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
    inst = bg.BeagleInstance(lib, N, 3 * N, N, S, P, 2, 4 * N, K, N, preference_flags=flags)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.asarray(div.tip_states[tip]).astype(np.int32))
        inst.set_pattern_weights(div.weights)
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
        assert inst.child_count() == 2
        with pytest.raises(bg.BeagleError) as err:
            inst.calculate_insertion_log_likelihoods([N + 1], [0], [NONE], [1], [0], [NONE], [0])
        assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION and lib.last_error()
        seen.append((err.value.code, lib.last_error()))
    finally:
        inst.finalize()
    return seen


def check_engines_agree(lib):
    single, double = check_argument_errors(lib), check_argument_errors(lib, double_precision=True)
    assert len(single) == len(double) and len(single) >= 25
    for i, (s, d) in enumerate(zip(single, double)):
        assert s == d, (i, s, d)


def test_argument_errors_on_emulation(emu):
    check_engines_agree(emu)


@pytest.mark.gpu
def test_argument_errors(gpu):
    check_engines_agree(gpu)
