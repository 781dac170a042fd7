"""First and second derivative of the log-likelihood in all branch lengths from one read of the buffers
(mbamdCalculateEdgeSecondDerivatives; csrc/mbamd_preorder.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference is numpy float64 from the `Division` alone, that of tests/test_preorder_gradient.py (post-order pruning, the pre-order
recursion un-normalised, N_c, A_c, L_c and d_c = N_c / L_c per branch) with, per branch (node n) and pattern c,
    M_c  = sum_k w_k sum_l pre_n[k,c,l] sum_j (r_k^2 Q^2)[l,j] post_n[k,c,j],      A2_c the same with |r_k^2 Q^2|
    d2_c = M_c / L_c - d_c^2.
test_reference_against_finite_differences checks it against central differences of the reference's own analytic gradient.

Tolerance, derived and not tuned.  With b1_c = (S + 8) (1 + 2 h) u (A_c + |N_c|) / L_c the gradient's bound (the module docstring of
tests/test_preorder_gradient.py: every component of either buffer is a sum of non-negative terms carrying at most (S + 8) 2 h u
relative error, the read-out is one more S-term inner product, a product and a ratio), the ratio M_c / L_c is the same expression with
D2 in the place of D1 and carries (S + 8) (1 + 2 h) u (A2_c + |M_c|) / L_c; the square of d1 carries 2 |d1_c| b1_c + b1_c^2; the
posterior weights, the subtraction and the sums in double are inside the eight of (S + 8):
    |d2_c - d2_c,ref| <= b2_c = (S + 8) (1 + 2 h) u (A2_c + |M_c|) / L_c + 2 |d1_c| b1_c + b1_c^2
The matrix-core kernel (16 ... 64 states, single precision) forms row l of D post as an fp32 accumulation over the S post-order
states -- the zero rows and zero reduction indices of its tiles add exact zeros --, whose error is at most S u sum_j |D[l,j]| post[j]
(the standard bound of a recursive sum of S products; the term the 64 K u of tests/test_cross_products.py stands for there, with
the reduction length S of this kernel in the place of 64 K).  Weighted with pre and divided by L it adds
    S u A_c / L_c to b1_c       and       S u A2_c / L_c to the first term of b2_c,
and b2_c takes the enlarged b1_c in its other two terms.  The sums get sum_c weight_c b_c.  u = 2^-24 on the single-precision
engine; u = 2^-53 kappa on the double-precision engine (unit_roundoff of tests/preorder_reference.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.preorder_reference import bounds as gradient_bounds
from tests.preorder_reference import division, post_order, pre_order, rate_matrix, tip_vector, unit_roundoff
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA, U32, branch_length, spectral
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
def second_matrices(div):
    """D2_k = r_k^2 Q^2, [K][S][S]"""
    Q = rate_matrix(div)
    r = np.asarray(div.cat_rates, dtype=np.float64)
    return (r * r)[:, None, None] * (Q @ Q)[None, :, :]


@functools.lru_cache(maxsize=None)
def reference(states, ncat, npat, ntaxa=NTAXA):
    """the gradient's reference, and per node n: d2 [P], M, A2; plus the root branch's scale of the one-branch call's d2"""
    div = division(states, ncat, npat, ntaxa)
    g = gradient_reference(states, ncat, npat, ntaxa)
    t = div.tree
    post, mats = post_order(div, g["lengths"])
    pre = pre_order(div, post, mats)
    w, pi = div.category_weights(0), np.asarray(div.pi, dtype=np.float64)
    D2 = second_matrices(div)
    res = {"nodes": list(g["nodes"]), "lengths": g["lengths"], "h": g["h"], "g": g}
    for n in res["nodes"]:
        M = np.einsum("k,kcl,klj,kcj->c", w, pre[n], D2, post[n])
        A2 = np.einsum("k,kcl,klj,kcj->c", w, pre[n], np.abs(D2), post[n])
        L = g[n]["L"]
        res[n] = dict(d2=M / L - g[n]["d"] ** 2, M=M, A2=A2)
    # the root branch as the one-branch call sees it (tests/test_derivatives.py): parent = the top node, child = the root tip
    top = t.root_left
    m1, m2 = spectral(div, g["lengths"][top], 1)[0], spectral(div, g["lengths"][top], 2)[0]
    L0 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], mats[top], post[t.root])
    R1 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], m1, post[t.root])
    R2 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], m2, post[t.root])
    B1 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], np.abs(m1), post[t.root])
    B2 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], np.abs(m2), post[t.root])
    res["root"] = dict(d1=R1 / L0, scale1=(B1 + np.abs(R1)) / L0, scale2=(B2 + np.abs(R2)) / L0)
    return res


def gradient_sum(div, lengths, n):
    """sum_c weight_c d_c of branch n at the branch lengths `lengths`, analytically (the reference's gradient)"""
    post, mats = post_order(div, lengths)
    pre = pre_order(div, post, mats)
    w = div.category_weights(0)
    D = np.asarray(div.cat_rates, dtype=np.float64)[:, None, None] * rate_matrix(div)[None, :, :]
    N = np.einsum("k,kcl,klj,kcj->c", w, pre[n], D, post[n])
    L = np.einsum("k,kcl,kcl->c", w, pre[n], post[n])
    return float((div.weights * N / L).sum())


def test_reference_against_finite_differences():
    """The reference itself (no engine code): sum_c weight_c d2_c of every branch against the central difference of the reference's
    own analytic gradient in that branch's length.  Step 1e-4 t (at least 1e-7): the truncation error is O(step^2 g''') ~ 1e-8
    relative; the rounding error of a gradient sum is ~ 2^-53 times the sum of its terms' magnitudes, ~ 1e-16 x 1e3 x a few, divided
    by the step -- with the shortest branches ~ 1e-2 that is ~ 1e-7 absolute, as in
    test_preorder_gradient.test_reference_against_finite_differences; asserted at 2e-6 relative to |value| + 1, as there."""
    worst = 0.0
    for ntaxa in (NTAXA, 60):
        div = division(4, 4, 70, ntaxa)
        ref = reference(4, 4, 70, ntaxa)
        for n in ref["nodes"]:
            value = float((div.weights * ref[n]["d2"]).sum())
            t0 = ref["lengths"][n]
            step = max(1e-4 * t0, 1e-7)
            up, down = dict(ref["lengths"]), dict(ref["lengths"])
            up[n], down[n] = t0 + step, t0 - step
            fd = (gradient_sum(div, up, n) - gradient_sum(div, down, n)) / (2.0 * step)
            worst = max(worst, abs(fd - value) / (abs(value) + 1.0))
    print("second-derivative reference against central differences of the gradient: worst relative difference %.2e" % worst)
    assert worst <= 2e-6, worst


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def matrix_core(states, double_precision):
    return 16 <= states <= 64 and not double_precision


def bounds(div, ref, u, mfma):
    """{node: (b1 [P], b2 [P])}; mfma: with the matrix core's S-term fp32 accumulation"""
    S, g = div.nstates, ref["g"]
    f = (S + 8) * (1 + 2 * ref["h"]) * u
    b1 = gradient_bounds(div, g, u)
    out = {}
    for n in ref["nodes"]:
        L = g[n]["L"]
        bn = b1[n] + (S * u * g[n]["A"] / L if mfma else 0.0)
        first = f * (ref[n]["A2"] + np.abs(ref[n]["M"])) / L + (S * u * ref[n]["A2"] / L if mfma else 0.0)
        out[n] = (bn, first + 2.0 * np.abs(g[n]["d"]) * bn + bn * bn)
    return out


# ---- the per-case check -------------------------------------------------------------------------------------------------------
def curvature_indices(bd):
    nodes = list(bd.div.tree.all_down_pass)
    return dict(posts=[bd.condLikeIndex[0][n] for n in nodes], pres=[bd.preOrderIndex[n] for n in nodes],
                dmats1=[bd.diffMatrixIndex] * len(nodes), dmats2=[bd.diffMatrix2Index] * len(nodes), weights=[bd.cijkIndex[0]] * len(nodes))


def gradient_of(ix):
    return dict(posts=ix["posts"], pres=ix["pres"], dmats=ix["dmats1"], weights=ix["weights"])


def new_division(lib, div, double_precision=False, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    return lk.BeagleDivision(div, lib, scaling=scaling, double_precision=double_precision, second_order=True)


def check_case(lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    div = division(states, ncat, npat, ntaxa)
    ref = reference(states, ncat, npat, ntaxa)
    g = ref["g"]
    t, S, w = div.tree, div.nstates, div.weights
    u = unit_roundoff(div, g, double_precision)
    mfma = matrix_core(states, double_precision)
    b = bounds(div, ref, u, mfma)
    nodes = ref["nodes"]
    bd = new_division(lib, div, double_precision, scaling)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(states, ncat, double_precision) in name, name
        bd.LogLike(0)
        bd.AcceptMove(0)
        before = inst.get_second_derivative_launches()
        curv = bd.BranchCurvature(0)
        assert sorted(curv) == sorted(nodes) and len(curv) == 2 * t.ntaxa - 3
        ix = curvature_indices(bd)
        rc, per1, per2, sums1, sums2 = inst.calculate_edge_second_derivatives(sites=True, **ix)
        assert rc == 0 and per1.shape == per2.shape == (len(nodes), npat)
        # 3. the same sums without the per-site values
        rc, none1, none2, sums1n, sums2n = inst.calculate_edge_second_derivatives(sites=False, **ix)
        assert rc == 0 and none1 is None and none2 is None
        assert np.array_equal(sums1, sums1n) and np.array_equal(sums2, sums2n)
        # 2. which kernel ran: three calls, one chunk each
        after = inst.get_second_derivative_launches()
        assert (after[0] - before[0], after[1] - before[1]) == ((0, 3) if mfma else (3, 0)), (before, after)
        # 1. d1 is the gradient call's
        rc, gper, gsums, _ = inst.calculate_edge_gradient(sites=True, **gradient_of(ix))
        assert rc == 0
        worst = [0.0, 0.0, 0.0, 0.0]
        for i, n in enumerate(nodes):
            b1, b2 = b[n]
            assert curv[n] == (sums1[i], sums2[i])
            if mfma:
                assert np.all(np.abs(per1[i] - gper[i]) <= b1) and abs(sums1[i] - gsums[i]) <= float((w * b1).sum())
            worst[0] = max(worst[0], float((np.abs(per1[i] - g[n]["d"]) / b1).max()))
            worst[1] = max(worst[1], abs(sums1[i] - float((w * g[n]["d"]).sum())) / float((w * b1).sum()))
            worst[2] = max(worst[2], float((np.abs(per2[i] - ref[n]["d2"]) / b2).max()))
            worst[3] = max(worst[3], abs(sums2[i] - float((w * ref[n]["d2"]).sum())) / float((w * b2).sum()))
        if not mfma:
            assert np.array_equal(per1, gper) and np.array_equal(sums1, gsums)
        print("%d states x %d x %d, %d taxa%s, %s kernel: error / bound over %d branches: d1 sites %.3f, sums %.3f; d2 sites %.3f, sums %.3f" %
              (states, ncat, npat, t.ntaxa, " fp64" if double_precision else "", "matrix-core" if mfma else "plain", len(nodes),
               worst[0], worst[1], worst[2], worst[3]))
        assert max(worst) <= 1.0, worst
        # 4. the root branch once more through the one-branch call: P' and P'' of the branch into spare matrix buffers
        top = t.root_left
        pcopy, m1, m2 = bd.tiProbsScratchIndex[0], bd.tiProbsScratchIndex[1], bd.tiProbsScratchIndex[2]
        inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [ref["lengths"][top]], first=[m1], second=[m2])
        rc, lnl, e1, e2 = inst.calculate_edge_derivatives(parents=[bd.condLikeIndex[0][top]], children=[bd.condLikeIndex[0][t.root]],
                                                          probs=[bd.tiProbsIndex[0][top]], first=[m1], second=[m2], weights=[bd.cijkIndex[0]],
                                                          freqs=[bd.cijkIndex[0]], cums=[bd.siteScalerIndex[0]])
        assert rc == 0
        # (that call's own bound, formed like b2: both ends of the branch carry the post-order chain's error)
        f = (S + 8) * (1 + 2 * ref["h"]) * u
        r1 = f * ref["root"]["scale1"]
        r2 = f * ref["root"]["scale2"] + 2.0 * np.abs(ref["root"]["d1"]) * r1 + r1 * r1
        i = nodes.index(top)
        assert abs(sums2[i] - e2) <= float((w * b[top][1]).sum()) + float((w * r2).sum()), (sums2[i], e2)
        assert abs(sums1[i] - e1) <= float((w * b[top][0]).sum()) + float((w * r1).sum()), (sums1[i], e1)
        return worst
    finally:
        bd.finalize()


#        states, categories, patterns                     what it reaches
CASES = [(4, 4, 130),             # two full 64-pattern blocks plus 2 patterns
         (4, 9, 70),              # a second batch of eight categories
         (3, 2, 70),              # a small state count
         (12, 2, 70),             # level layouts, plain kernel
         (12, 6, 70),             # level layouts, plain kernel
         (16, 2, 70),             # first matrix-core count
         (20, 4, 70),             # the tree-walk arena
         (33, 2, 70),             # first two-row-tile count
         (61, 1, 40),             # one category, no posteriors
         (64, 2, 70),             # full tiles
         (24, 2, 70)]             # one row tile on the level layouts (an odd one out of the tree-walk counts)
CASES_F64 = [(4, 4, 130), (20, 2, 70)]


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_second_derivatives_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_second_derivatives_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


def test_second_derivatives_deep_tree_on_emulation(emu):
    """60 taxa: L down to ~1e-55 in the float64 reference, far below fp32's range"""
    assert gradient_reference(4, 4, 70, 60)["min_L"] < 1e-45
    check_case(emu, 4, 4, 70, ntaxa=60)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_second_derivatives(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_second_derivatives_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
def test_second_derivatives_deep_tree(gpu):
    check_case(gpu, 4, 4, 70, ntaxa=60)


# ---- the matrix-core kernel against the plain one ---------------------------------------------------------------------------------
def _curvature_call(lib, div):
    """(children, per-site d1, per-site d2, sums of d1, sums of d2, read-out launches (plain, matrix core) of the call) on a fresh instance"""
    bd = new_division(lib, div)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchCurvature(0)
        before = bd.inst.get_second_derivative_launches()
        bd.inst.get_kernel_timing(reset=True)
        rc, per1, per2, sums1, sums2 = bd.inst.calculate_edge_second_derivatives(sites=True, **curvature_indices(bd))
        _, launches = bd.inst.get_kernel_timing(reset=True)
        after = bd.inst.get_second_derivative_launches()
        assert rc == 0
        # (per child and chunk: the read-out launch and k_gradient_sums)
        assert launches == 2 * bd.inst.child_count(), launches
        return bd.inst.child_count(), per1, per2, sums1, sums2, (after[0] - before[0], after[1] - before[1])
    finally:
        bd.finalize()


MFMA_CASES = [(16, 2, 70), (20, 4, 70), (24, 2, 70), (33, 2, 70), (61, 1, 40), (64, 2, 70)]


def check_mfma_against_generic(lib, monkeypatch, states, ncat, npat):
    """MBAMD_CURV_GENERIC=1 sends 16 ... 64 states to the plain kernel: each result within b of the reference and within 2 b of the
    other.  Either kernel is one read-out launch and one of k_gradient_sums per chunk (mbamdGetKernelTiming counts both), so the
    read-out launches are counted per kernel (mbamdGetSecondDerivativeLaunches): that count tells them apart."""
    div, ref = division(states, ncat, npat), reference(states, ncat, npat)
    g, w = ref["g"], div.weights
    bm, bp = bounds(div, ref, U32, True), bounds(div, ref, U32, False)
    monkeypatch.delenv("MBAMD_CURV_GENERIC", raising=False)
    _, m1, m2, ms1, ms2, lm = _curvature_call(lib, div)
    monkeypatch.setenv("MBAMD_CURV_GENERIC", "1")
    try:
        _, p1, p2, ps1, ps2, lp = _curvature_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_CURV_GENERIC")
    assert lm == (0, 1) and lp == (1, 0), (lm, lp)
    worst = [0.0, 0.0, 0.0]
    for i, n in enumerate(ref["nodes"]):
        d1, d2 = g[n]["d"], ref[n]["d2"]
        for q, (core, plain, r) in enumerate(((m1[i], p1[i], d1), (m2[i], p2[i], d2))):
            worst[0] = max(worst[0], float((np.abs(core - r) / bm[n][q]).max()))
            worst[1] = max(worst[1], float((np.abs(plain - r) / bp[n][q]).max()))
            worst[2] = max(worst[2], float((np.abs(core - plain) / (2.0 * bm[n][q])).max()))
        for q, (core, plain, r) in enumerate(((ms1[i], ps1[i], float((w * d1).sum())), (ms2[i], ps2[i], float((w * d2).sum())))):
            worst[0] = max(worst[0], abs(core - r) / float((w * bm[n][q]).sum()))
            worst[1] = max(worst[1], abs(plain - r) / float((w * bp[n][q]).sum()))
            worst[2] = max(worst[2], abs(core - plain) / (2.0 * float((w * bm[n][q]).sum())))
    print("%d states x %d x %d: error / bound: matrix core %.3f, plain %.3f, one against the other (2 b) %.3f; read-out launches %s and %s" %
          (states, ncat, npat, worst[0], worst[1], worst[2], lm, lp))
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("states,ncat,npat", MFMA_CASES)
def test_mfma_against_generic_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_mfma_against_generic(emu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", MFMA_CASES)
def test_mfma_against_generic(gpu, monkeypatch, states, ncat, npat):
    check_mfma_against_generic(gpu, monkeypatch, states, ncat, npat)


# ---- pattern shards -----------------------------------------------------------------------------------------------------------
SHARD_CASES = [(4, 4, 130), (20, 4, 70)]


def check_sharded(lib, monkeypatch, states, ncat, npat):
    """MBAMD_SHARD=2: the children's sums added, their per-site values concatenated"""
    div, ref = division(states, ncat, npat), reference(states, ncat, npat)
    g, w = ref["g"], div.weights
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    monkeypatch.delenv("MBAMD_CURV_GENERIC", raising=False)
    n0, a1, a2, as1, as2, _ = _curvature_call(lib, div)
    monkeypatch.setenv("MBAMD_SHARD", "2")
    try:
        n2, s1, s2, ss1, ss2, _ = _curvature_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n0 == 1 and n2 == 2
    b = bounds(div, ref, U32, matrix_core(states, False))
    for i, n in enumerate(ref["nodes"]):
        for q, (one, two, sum1, sum2, r) in enumerate(((a1[i], s1[i], as1[i], ss1[i], g[n]["d"]), (a2[i], s2[i], as2[i], ss2[i], ref[n]["d2"]))):
            bq = b[n][q]
            assert np.all(np.abs(two - one) <= bq) and np.all(np.abs(two - r) <= bq)
            assert abs(sum2 - sum1) <= float((w * bq).sum()) and abs(sum2 - float((w * r).sum())) <= float((w * bq).sum())


@pytest.mark.parametrize("states,ncat,npat", SHARD_CASES)
def test_sharded_second_derivatives_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_sharded(emu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", SHARD_CASES)
def test_sharded_second_derivatives(gpu, monkeypatch, states, ncat, npat):
    check_sharded(gpu, monkeypatch, states, ncat, npat)


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, double_precision=False):
    """Every bad call is refused with the expected status and writes nothing to its outputs; returns (status, message) of each, in
    order: the two engines run one body (mbamd_preorder.h), so they answer alike -- check_engines_agree."""
    seen = []
    div = division(4, 2, 130)
    t = div.tree
    bd = new_division(lib, div, double_precision)
    try:
        inst = bd.inst

        def raises(code, inst_, ix):
            """the call through the C ABI with sentinel-filled outputs"""
            arrays = [np.asarray(ix[k], dtype=np.int32) for k in ("posts", "pres", "dmats1", "dmats2", "weights")]
            n = len(arrays[0])
            outs = [np.full(max(n, 1) * 130, -7.5), np.full(max(n, 1) * 130, -7.5), np.full(max(n, 1), -7.5), np.full(max(n, 1), -7.5)]
            rc = inst_.lib.mbamdCalculateEdgeSecondDerivatives(inst_.id, *[a.ctypes.data_as(_ip) for a in arrays], n,
                                                             *[o.ctypes.data_as(_dp) for o in outs])
            assert rc == code, (rc, code)
            assert lib.last_error()
            assert all(np.all(o == -7.5) for o in outs)
            seen.append((rc, lib.last_error()))

        # more than one category and no log-likelihood call yet
        raises(bg.BEAGLE_ERROR_GENERAL, inst, curvature_indices(bd))
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchCurvature(0)
        ix = curvature_indices(bd)                                                      # (the evaluation flipped index tables)
        n = len(ix["posts"])
        # a weights index different from the remembered one
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, dict(ix, weights=[bd.cijkScratchIndex] * n))
        # a pre index that no pre-order operation wrote; one that beagleUpdatePartials has overwritten since
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, dict(ix, pres=[bd.preOrderStartIndex] * n))
        victim = bd.preOrderIndex[t.root_left]
        inst.update_partials(np.array([[victim, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, bd.condLikeIndex[0][0], bd.tiProbsIndex[0][0],
                                        bd.condLikeIndex[0][1], bd.tiProbsIndex[0][1]]], dtype=np.int32), bg.BEAGLE_OP_NONE)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix)
        inst.update_pre_partials(bd.PreOrderOperations(0))                              # (all of them pre-order buffers again)
        assert inst.calculate_edge_second_derivatives(sites=False, **ix)[0] == 0
        # out-of-range matrix and buffer indices
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, dict(ix, dmats1=[10 ** 6] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, dict(ix, dmats2=[10 ** 6] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, dict(ix, dmats2=[-1] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, dict(ix, posts=[10 ** 6] * n))
        # NULL index arrays; a negative count
        outs = [np.full(n * 130, -7.5), np.full(n * 130, -7.5), np.full(n, -7.5), np.full(n, -7.5)]
        good = [np.asarray(ix[k], dtype=np.int32) for k in ("posts", "pres", "dmats1", "dmats2", "weights")]
        for missing in range(5):
            ptrs = [None if j == missing else a.ctypes.data_as(_ip) for j, a in enumerate(good)]
            rc = inst.lib.mbamdCalculateEdgeSecondDerivatives(inst.id, *ptrs, n, *[o.ctypes.data_as(_dp) for o in outs])
            assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE and all(np.all(o == -7.5) for o in outs)
            seen.append((rc, lib.last_error()))
        rc = inst.lib.mbamdCalculateEdgeSecondDerivatives(inst.id, *[a.ctypes.data_as(_ip) for a in good], -1, *[o.ctypes.data_as(_dp) for o in outs])
        assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE
        seen.append((rc, lib.last_error()))
        # no edges: success, nothing written (NULL arrays allowed); every output NULL: success
        rc = inst.lib.mbamdCalculateEdgeSecondDerivatives(inst.id, None, None, None, None, None, 0, *[o.ctypes.data_as(_dp) for o in outs])
        assert rc == 0 and all(np.all(o == -7.5) for o in outs)
        rc = inst.lib.mbamdCalculateEdgeSecondDerivatives(inst.id, *[a.ctypes.data_as(_ip) for a in good], n, None, None, None, None)
        assert rc == 0
        # only the second per-site array and the first sums
        rc = inst.lib.mbamdCalculateEdgeSecondDerivatives(inst.id, *[a.ctypes.data_as(_ip) for a in good], n, None, outs[1].ctypes.data_as(_dp),
                                                         outs[2].ctypes.data_as(_dp), None)
        full = inst.calculate_edge_second_derivatives(sites=True, **ix)
        assert rc == 0 and np.array_equal(outs[1].reshape(n, 130), full[2]) and np.array_equal(outs[2], full[3])
        assert np.all(outs[0] == -7.5) and np.all(outs[3] == -7.5)
    finally:
        bd.finalize()
    # a multi-partition instance does not serve the call
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
            inst.calculate_edge_second_derivatives([0], [N + 1], [0], [1], [0])
        assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION
        seen.append((err.value.code, lib.last_error()))
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


def test_second_order_needs_its_flag(emu):
    """a division built without second_order keeps the buffer numbering of before and refuses BranchCurvature"""
    div = division(4, 2, 130)
    plain = lk.BeagleDivision(div, emu, pre_order=True)
    second = lk.BeagleDivision(div, emu, second_order=True)
    try:
        assert plain.numDiffMatrices + 1 == second.numDiffMatrices and plain.diffMatrixIndex == second.diffMatrixIndex
        assert second.diffMatrix2Index == second.diffMatrixIndex + 1 and plain.preOrderIndex == second.preOrderIndex
        with pytest.raises(ValueError):
            plain.BranchCurvature(0)
    finally:
        plain.finalize()
        second.finalize()
