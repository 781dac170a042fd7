"""The pre-order pass and the gradient of the log-likelihood in all branch lengths (beagleUpdatePrePartials,
beagleSetDifferentialMatrix, beagleCalculateEdgeDerivatives; csrc/mbamd_preorder.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference (tests/preorder_reference.py) is numpy float64 from the `Division` alone: post-order pruning as in
tests/pruning_reference.py, the pre-order recursion un-normalised,
    pre_top[k,c,j] = sum_i P_top,k[i,j] pi_i tip_root[c,i]
    tmp[k,c,i]     = pre_parent[k,c,i] sum_j P_sib,k[i,j] post_sib[k,c,j],      pre_n[k,c,j] = sum_i P_n,k[i,j] tmp[k,c,i]
and Q = U diag(lambda) U^-1, D_k = r_k Q.  Per branch (node n) and pattern c
    N_c = sum_k w_k sum_l pre_n[k,c,l] sum_j D_k[l,j] post_n[k,c,j],   A_c the same with |D_k|,   L_c = sum_k w_k sum_l pre_n[k,c,l] post_n[k,c,l]
    d_c = N_c / L_c.
test_reference_against_finite_differences checks this reference itself against central differences of the float64 log-likelihood.

Tolerance, derived and not tuned: everything in both passes is a sum of non-negative terms; an operation is two S-term inner products,
a product and an exact rescaling and adds at most 2 (S + 8) u relative error to every component it produces; chains add.  With h the
number of operations on the longest post-order root-to-tip chain plus the same for the pre-order list,
    |d_c - d_c,ref| <= b_c = (S + 8) (1 + 2 h) u (A_c + |N_c|) / L_c
the weighted sums get sum_c weight_c b_c and the sums of squares sum_c weight_c (2 |d_c| b_c + b_c^2).  u = 2^-24 on the
single-precision engine; u = 2^-53 kappa on the double-precision engine, kappa the cancellation inside the spectral sums of the
matrices (tests/pruning_reference.py), the largest over the branches of the tree.
"""
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.preorder_reference import CASES, CASES_F64, bounds, division, gradient_indices, post_order, reference, unit_roundoff
from tests.pruning_reference import NTAXA, U32
from tests.test_derivatives import expected_layout

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


# ---- the reference ------------------------------------------------------------------------------------------------------------
def log_likelihood(div, lengths):
    t = div.tree
    cl, mats = post_order(div, lengths)
    top = t.root_left
    L = np.einsum("k,i,kci,kij,kcj->c", div.category_weights(0), np.asarray(div.pi, dtype=np.float64), cl[top], mats[top], cl[t.root])
    return float((div.weights * np.log(L)).sum())


def test_reference_against_finite_differences():
    """The reference itself (no engine code): sum_c weight_c d_c of every branch against the central difference of the float64
    log-likelihood.  Step 1e-4 t (at least 1e-7): the truncation error is O(step^2 f''') ~ 1e-8 relative, the rounding error
    2^-53 |lnL| / step -- with |lnL| ~ 1e3 and the shortest branches ~ 1e-2 that is ~ 1e-7 absolute; asserted at 2e-6 relative to
    |g| + 1."""
    worst = 0.0
    for ntaxa in (NTAXA, 60):
        div = division(4, 4, 70, ntaxa)
        ref = reference(4, 4, 70, ntaxa)
        for n in ref["nodes"]:
            g = float((div.weights * ref[n]["d"]).sum())
            t0 = ref["lengths"][n]
            step = max(1e-4 * t0, 1e-7)
            up, down = dict(ref["lengths"]), dict(ref["lengths"])
            up[n], down[n] = t0 + step, t0 - step
            fd = (log_likelihood(div, up) - log_likelihood(div, down)) / (2.0 * step)
            worst = max(worst, abs(fd - g) / (abs(g) + 1.0))
    print("reference against central differences: worst relative difference %.2e" % worst)
    assert worst <= 2e-6, worst


# ---- the per-case check -------------------------------------------------------------------------------------------------------
def check_case(lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    div = division(states, ncat, npat, ntaxa)
    ref = reference(states, ncat, npat, ntaxa)
    t, S, w = div.tree, div.nstates, div.weights
    u = unit_roundoff(div, ref, double_precision)
    b = bounds(div, ref, u)
    bd = lk.BeagleDivision(div, lib, scaling=scaling, double_precision=double_precision, pre_order=True)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(states, ncat, double_precision) in name, name
        bd.LogLike(0)
        bd.AcceptMove(0)
        grad = bd.BranchGradient(0)
        assert sorted(grad) == sorted(ref["nodes"]) and len(grad) == 2 * t.ntaxa - 3
        ix = gradient_indices(bd)
        rc, per, sums, sq = inst.calculate_edge_gradient(sites=True, **ix)
        assert rc == 0 and per.shape == (len(ref["nodes"]), npat)
        rc, none, sums0, sq0 = inst.calculate_edge_gradient(sites=False, **ix)
        assert rc == 0 and none is None
        assert np.array_equal(sums, sums0) and np.array_equal(sq, sq0)
        worst = [0.0, 0.0, 0.0]
        for i, n in enumerate(ref["nodes"]):
            d, bn = ref[n]["d"], b[n]
            assert grad[n] == sums[i]
            worst[0] = max(worst[0], float((np.abs(per[i] - d) / bn).max()))
            worst[1] = max(worst[1], abs(sums[i] - float((w * d).sum())) / float((w * bn).sum()))
            worst[2] = max(worst[2], abs(sq[i] - float((w * d * d).sum())) / float((w * (2.0 * np.abs(d) * bn + bn * bn)).sum()))
        print("%d states x %d x %d, %d taxa%s: error / bound over %d branches: sites %.3f, sums %.3f, squared sums %.3f (min L %.1e, min column %.1e)" %
              (states, ncat, npat, t.ntaxa, " fp64" if double_precision else "", len(ref["nodes"]), worst[0], worst[1], worst[2],
               ref["min_L"], ref["min_column"]))
        assert max(worst) <= 1.0, worst
        # the root branch once more through the one-branch call: P' of the branch into a spare matrix buffer
        top = t.root_left
        pcopy, m1 = bd.tiProbsScratchIndex[0], bd.tiProbsScratchIndex[1]
        inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [ref["lengths"][top]], first=[m1])
        rc, lnl, d1, _ = inst.calculate_edge_derivatives(parents=[bd.condLikeIndex[0][top]], children=[bd.condLikeIndex[0][t.root]],
                                                         probs=[bd.tiProbsIndex[0][top]], first=[m1], second=None, weights=[bd.cijkIndex[0]],
                                                         freqs=[bd.cijkIndex[0]], cums=[bd.siteScalerIndex[0]])
        assert rc == 0
        i = ref["nodes"].index(top)
        b1 = float((w * (S + 8) * u * ref["root_scale1"]).sum())
        assert abs(sums[i] - d1) <= float((w * b[top]).sum()) + b1, (sums[i], d1)
        return worst
    finally:
        bd.finalize()


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_gradient_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_gradient_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


def test_gradient_deep_tree_on_emulation(emu):
    """60 taxa: L down to ~1e-55 and un-normalised pre-order columns down to ~1e-107 in the float64 reference, far below fp32's range
    -- passes only if both the normalisation and the recombination of the categories in q are right"""
    ref = reference(4, 4, 70, 60)
    assert ref["min_L"] < 1e-45 and ref["min_column"] < 1e-45 and ref["min_column"] > 1e-300
    check_case(emu, 4, 4, 70, ntaxa=60)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_gradient(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_gradient_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
def test_gradient_deep_tree(gpu):
    check_case(gpu, 4, 4, 70, ntaxa=60)


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def _raises(lib, code, call, *args, **kwargs):
    with pytest.raises(bg.BeagleError) as err:
        call(*args, **kwargs)
    assert err.value.code == code, (err.value.code, code)
    assert lib.last_error()
    return err.value.code, lib.last_error()


def check_argument_errors(lib, double_precision=False):
    """Every bad call is refused with the expected status; returns (status, message) of each, in order: the two engines run one
    body per call (mbamd_preorder.h, mbamd_crossproducts.h), so they answer alike -- check_engines_agree."""
    seen = []

    def raises(code, call, *args, **kwargs):
        seen.append(_raises(lib, code, call, *args, **kwargs))

    div = division(4, 2, 130)
    t = div.tree
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    try:
        inst = bd.inst
        # more than one category and no log-likelihood call yet
        raises(bg.BEAGLE_ERROR_GENERAL, inst.calculate_edge_gradient, **gradient_indices(bd))
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchGradient(0)
        ix = gradient_indices(bd)                                                       # (the evaluation flipped index tables)
        ops = bd.PreOrderOperations(0)
        # a scale index in a pre-order list
        for field in (1, 2):
            bad = ops.copy()
            bad[3, field] = bd.nodeScalerIndex[0][t.root_left]
            raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst.update_pre_partials, bad)
            assert "self-normalised" in lib.last_error()
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst.update_pre_partials, ops, bd.siteScalerIndex[0])
        # a weights index different from the remembered one
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.calculate_edge_gradient, **dict(ix, weights=[bd.cijkScratchIndex] * len(ix["posts"])))
        # a pre index that no pre-order operation wrote; one that beagleUpdatePartials has overwritten since
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.calculate_edge_gradient, **dict(ix, pres=[bd.preOrderStartIndex] * len(ix["posts"])))
        victim = bd.preOrderIndex[t.root_left]
        inst.update_partials(np.array([[victim, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, bd.condLikeIndex[0][0], bd.tiProbsIndex[0][0],
                                        bd.condLikeIndex[0][1], bd.tiProbsIndex[0][1]]], dtype=np.int32), bg.BEAGLE_OP_NONE)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.calculate_edge_gradient, **ix)
        inst.update_pre_partials(ops)                                                   # (all of them pre-order buffers again)
        assert inst.calculate_edge_gradient(sites=False, **ix)[0] == 0
        # a destination holding compact tip states; out-of-range buffer and matrix indices
        for row, field, value in ((1, 0, bd.condLikeIndex[0][0]), (1, 0, 10 ** 6), (1, 3, -2), (1, 5, 10 ** 6), (1, 4, 10 ** 6), (1, 6, -3)):
            bad = ops.copy()
            bad[row, field] = value
            raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.update_pre_partials, bad)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.calculate_edge_gradient, **dict(ix, dmats=[10 ** 6] * len(ix["posts"])))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.calculate_edge_gradient, **dict(ix, posts=[10 ** 6] * len(ix["posts"])))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.set_differential_matrix, 10 ** 6, np.zeros((div.ncat, 4, 4)))
    finally:
        bd.finalize()
    # a multi-partition instance serves none of the three
    N, S, K, P = NTAXA, 4, 2, 130
    flags = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
    inst = bg.BeagleInstance(lib, N, 3 * N, N, S, P, 2, 4 * N, K, N, preference_flags=flags)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.asarray(div.tip_states[tip]).astype(np.int32))
        inst.set_pattern_weights(div.weights)
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
        assert inst.child_count() == 2
        one = np.array([[N + 1, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, N, 0, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE]], dtype=np.int32)
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst.update_pre_partials, one)
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst.set_differential_matrix, 0, np.zeros((K, S, S)))
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst.calculate_edge_gradient, [0], [N + 1], [0], [0])
    finally:
        inst.finalize()
    return seen


def check_engines_agree(lib):
    single, double = check_argument_errors(lib), check_argument_errors(lib, double_precision=True)
    assert len(single) == len(double)
    for i, (s, d) in enumerate(zip(single, double)):
        assert s == d, (i, s, d)


def test_argument_errors_on_emulation(emu):
    check_engines_agree(emu)


@pytest.mark.gpu
def test_argument_errors(gpu):
    check_engines_agree(gpu)


# ---- pattern shards -----------------------------------------------------------------------------------------------------------
def _gradient_call(lib, div):
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, pre_order=True)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchGradient(0)
        rc, per, sums, sq = bd.inst.calculate_edge_gradient(sites=True, **gradient_indices(bd))
        assert rc == 0
        return bd.inst.child_count(), per, sums, sq
    finally:
        bd.finalize()


def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 4 states x 4 categories x 130 patterns: the children's sums added, their per-site values concatenated"""
    div, ref = division(4, 4, 130), reference(4, 4, 130)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    n0, per0, sums0, sq0 = _gradient_call(lib, div)
    monkeypatch.setenv("MBAMD_SHARD", "2")
    try:
        n2, per2, sums2, sq2 = _gradient_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n0 == 1 and n2 == 2
    b, w = bounds(div, ref, U32), div.weights
    for i, n in enumerate(ref["nodes"]):
        d = ref[n]["d"]
        assert np.all(np.abs(per2[i] - per0[i]) <= b[n])
        assert np.all(np.abs(per2[i] - d) <= b[n])
        assert abs(sums2[i] - sums0[i]) <= float((w * b[n]).sum())
        assert abs(sums2[i] - float((w * d).sum())) <= float((w * b[n]).sum())
        assert abs(sq2[i] - sq0[i]) <= float((w * (2.0 * np.abs(d) * b[n] + b[n] * b[n])).sum())


def test_sharded_gradient_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_gradient(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- launch grouping ----------------------------------------------------------------------------------------------------------
def dependency_groups(ops):
    """the rule of beagle.h, written down independently: a new launch where an operation reads or writes a buffer the current launch
    writes, or writes a buffer the current launch reads"""
    groups, reads, writes = 0, set(), set()
    for op in ops:
        dst, used = int(op[0]), {int(op[3])} | ({int(op[5])} if op[5] != bg.BEAGLE_OP_NONE else set())
        if groups == 0 or used & writes or dst in writes or dst in reads:
            groups += 1
            reads, writes = set(), set()
        reads |= used
        writes.add(dst)
    return groups


def check_launch_grouping(lib, double_precision=False):
    """mbamdGetKernelTiming counts launches (both engines count the pre-order launches): one whole-tree list is one launch per
    dependency group, not one per operation"""
    div = division(4, 4, 130)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchGradient(0)
        ops = bd.PreOrderOperations(0)
        groups = dependency_groups(ops)
        assert 1 < groups < len(ops) == 2 * NTAXA - 3
        bd.inst.get_kernel_timing(reset=True)
        bd.inst.update_pre_partials(ops)
        _, launches = bd.inst.get_kernel_timing(reset=True)
        assert launches == groups, (launches, groups, len(ops))
    finally:
        bd.finalize()


def check_gradient_launches(lib, monkeypatch, double_precision=False):
    """one gradient call over every branch at 4 states x 4 categories x 130 patterns is one chunk on one engine: the read-out
    launch and the launch that adds its block sums"""
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    bd = lk.BeagleDivision(division(4, 4, 130), lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchGradient(0)
        assert bd.inst.child_count() == 1
        bd.inst.get_kernel_timing(reset=True)
        assert bd.inst.calculate_edge_gradient(sites=False, **gradient_indices(bd))[0] == 0
        _, launches = bd.inst.get_kernel_timing(reset=True)
        assert launches == 2, launches
    finally:
        bd.finalize()


def test_gradient_launches_on_emulation(emu, monkeypatch):
    check_gradient_launches(emu, monkeypatch)
    check_gradient_launches(emu, monkeypatch, double_precision=True)


@pytest.mark.gpu
def test_gradient_launches(gpu, monkeypatch):
    check_gradient_launches(gpu, monkeypatch)
    check_gradient_launches(gpu, monkeypatch, double_precision=True)


def test_launch_grouping_on_emulation(emu):
    check_launch_grouping(emu)
    check_launch_grouping(emu, double_precision=True)


@pytest.mark.gpu
def test_launch_grouping(gpu):
    check_launch_grouping(gpu)
    check_launch_grouping(gpu, double_precision=True)
