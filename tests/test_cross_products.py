"""The cross-product matrix of the gradient in the rate matrix (beagleCalculateCrossProductDerivative; csrc/mbamd_crossproducts.h,
DESIGN 4.4.3).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference is numpy float64 from the `Division` alone: post-order pruning and the un-normalised pre-order recursion of
tests/test_preorder_gradient.py, then, from the definition,
    den_e,k(c) = sum_l pre_e[k,c,l] post_e[k,c,l],        q_k(c) = w_k L_k(c) / sum_k' w_k' L_k'(c),   L_k(c) = den_e,k(c) at any node
    X[i,j]     = sum_e t_e sum_c weight_c sum_k q_k(c) r_k pre_e[k,c,i] post_e[k,c,j] / den_e,k(c).
test_reference_against_finite_differences checks this reference itself against central differences of the float64 log-likelihood
under Q -> Q + eps M for two matrices M that commute with Q.

Tolerance, derived and not tuned.  Every term of X[i,j] is non-negative, so the error is relative per entry.  With h as in
tests/test_preorder_gradient.py (the operations on the longest post-order chain plus those on the longest pre-order chain), every
component of a post-order or pre-order buffer carries at most (S + 8) (1 + 2 h) u relative error (an operation: two S-term inner
products, a product, an exact rescaling; chains add).  A term of X is  weight q r t pre_i post_j / den:
  * pre_i and post_j: (S + 8) (1 + 2 h) u each;
  * den, an S-term sum of products of such components: no more than its terms carry, 2 (S + 8) (1 + 2 h) u, its own S roundings
    being part of the (S + 8) the operations were charged with;
  * q, a ratio of two sums of the same kind taken at another branch: numerator and denominator share the factor whose error they
    carry, what remains is bounded by the error of den once more -- counted with den above;
together at most 4 (S + 8) (1 + 2 h) u.  The matrix core adds up to 64 K products in fp32 before the sum goes to double (the flush
rule of k_cross_products_mfma): 64 K u.  The coefficient's rounding to fp32, its product with pre_i, the product with post_j, the
conversions of t r and of q and the double-precision sums: 8 u covers them.
    |X[i,j] - X_ref[i,j]| <= b_ij = (4 (S + 8) (1 + 2 h) + 64 K + 8) u X_ref[i,j]
u = 2^-24 on the single-precision engine; u = 2^-53 kappa on the double-precision engine (unit_roundoff of
tests/test_preorder_gradient.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.preorder_reference import bound_factor
from tests.preorder_reference import bounds as gradient_bounds
from tests.preorder_reference import division, gradient_indices, post_order, rate_matrix, tip_vector, unit_roundoff
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA, U32, branch_length
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
@functools.lru_cache(maxsize=None)
def reference(states, ncat, npat, ntaxa=NTAXA):
    """per node n of all_down_pass the S x S matrix M_n = sum_c weight_c sum_k q_k(c) r_k pre_n[k,c,:] post_n[k,c,:]^T / den_n,k(c),
    so that X = sum_e t_e M_e; plus the nodes, their lengths and h"""
    div = division(states, ncat, npat, ntaxa)
    g = gradient_reference(states, ncat, npat, ntaxa)
    t = div.tree
    lengths = g["lengths"]
    post, mats = post_order(div, lengths)
    w, pi, r = div.category_weights(0), np.asarray(div.pi, dtype=np.float64), np.asarray(div.cat_rates, dtype=np.float64)
    top = t.root_left
    pre = {top: np.einsum("kij,ci->kcj", mats[top], pi[None, :] * tip_vector(div, t.root))}
    for p in reversed(t.int_down_pass):
        for n, sib in ((t.left[p], t.right[p]), (t.right[p], t.left[p])):
            tmp = pre[p] * np.einsum("kij,kcj->kci", mats[sib], post[sib])
            pre[n] = np.einsum("kij,kci->kcj", mats[n], tmp)
    Lk = np.einsum("kcl,kcl->kc", pre[top], post[top])
    q = w[:, None] * Lk
    q = q / q.sum(axis=0)[None, :]
    res = {"nodes": list(g["nodes"]), "lengths": lengths, "h": g["h"]}
    for n in res["nodes"]:
        den = np.einsum("kcl,kcl->kc", pre[n], post[n])
        coef = div.weights[None, :] * q * r[:, None] / den
        res[n] = np.einsum("kc,kci,kcj->ij", coef, pre[n], post[n])
    return res


def x_ref(ref, nodes, lengths):
    return sum(t * ref[n] for n, t in zip(nodes, lengths))


def log_likelihood(div, lengths, lam):
    """the float64 log-likelihood with the eigenvalues `lam` on the division's eigenvectors"""
    t, K = div.tree, div.ncat
    es = div.eigen[0]
    U, Ui = np.asarray(es.evec, dtype=np.float64), np.asarray(es.ivec, dtype=np.float64)
    mats = {n: np.stack([(U * np.exp(lam * r * lengths[n])[None, :]) @ Ui for r in div.cat_rates]) for n in t.all_down_pass}
    cl = {tip: np.broadcast_to(tip_vector(div, tip), (K, div.npatterns, div.nstates)) for tip in range(t.ntaxa)}
    for p in t.int_down_pass:
        out = np.ones((K, div.npatterns, div.nstates))
        for c in (t.left[p], t.right[p]):
            out = out * np.einsum("kij,kcj->kci", mats[c], cl[c])
        cl[p] = out
    top = t.root_left
    L = np.einsum("k,i,kci,kij,kcj->c", div.category_weights(0), np.asarray(div.pi, dtype=np.float64), cl[top], mats[top], cl[t.root])
    return float((div.weights * np.log(L)).sum())


def test_reference_against_finite_differences():
    """The reference itself (no engine code).  For M = Q and M = Q Q -- both commute with Q, and Q Q is not symmetric, so a
    transposed X fails -- the central difference of the float64 log-likelihood under Q + eps M (the same eigenvectors, eigenvalues
    lambda + eps lambda and lambda + eps lambda^2) against sum_ij X_ref[i,j] M[i,j].  Step 1e-5: the truncation error is
    O(step^2 f''') ~ 1e-10 f''', the rounding error 2^-53 |lnL| / step ~ 1e-8 with |lnL| ~ 1e3; asserted at 2e-6 relative to
    |value| + 1, as test_preorder_gradient.test_reference_against_finite_differences is."""
    worst = 0.0
    for ntaxa in (NTAXA, 60):
        div = division(4, 4, 70, ntaxa)
        ref = reference(4, 4, 70, ntaxa)
        X = x_ref(ref, ref["nodes"], [ref["lengths"][n] for n in ref["nodes"]])
        Q = rate_matrix(div)
        lam = np.asarray(div.eigen[0].eval, dtype=np.float64)
        assert not np.allclose(Q @ Q, (Q @ Q).T)
        for M, dlam in ((Q, lam), (Q @ Q, lam * lam)):
            eps = 1e-5
            fd = (log_likelihood(div, ref["lengths"], lam + eps * dlam) - log_likelihood(div, ref["lengths"], lam - eps * dlam)) / (2.0 * eps)
            value = float((X * M).sum())
            assert abs(float((X.T * M).sum()) - value) > 1e-3 * abs(value) or M is Q
            worst = max(worst, abs(fd - value) / (abs(value) + 1.0))
    print("cross-product reference against central differences: worst relative difference %.2e" % worst)
    assert worst <= 2e-6, worst


# ---- the per-case check -------------------------------------------------------------------------------------------------------
def cross_indices(bd, nodes):
    return dict(posts=[bd.condLikeIndex[0][n] for n in nodes], pres=[bd.preOrderIndex[n] for n in nodes], rates=[0] * len(nodes),
                weights=[bd.cijkIndex[0]] * len(nodes))


def check_case(lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    div = division(states, ncat, npat, ntaxa)
    ref = reference(states, ncat, npat, ntaxa)
    gref = gradient_reference(states, ncat, npat, ntaxa)
    t, w = div.tree, div.weights
    u = unit_roundoff(div, gref, double_precision)
    f = bound_factor(div, ref, u)
    nodes = ref["nodes"]
    lengths = [ref["lengths"][n] for n in nodes]
    bd = lk.BeagleDivision(div, lib, scaling=scaling, double_precision=double_precision, pre_order=True)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(states, ncat, double_precision) in name, name
        bd.LogLike(0)
        bd.AcceptMove(0)
        # 1. all branches at their lengths
        X = bd.RateMatrixCrossProducts(0)
        Xr = x_ref(ref, nodes, lengths)
        assert X.shape == (states, states) and len(nodes) == 2 * t.ntaxa - 3
        assert [branch_length(t, n) for n in nodes] == lengths
        worst = [float((np.abs(X - Xr) / (f * Xr)).max())]
        rc, X1 = inst.calculate_cross_products(edge_lengths=lengths, **cross_indices(bd, nodes))
        assert rc == 0 and np.array_equal(X1, X)
        # 2. a strict subset, reversed, other lengths: overwritten, not accumulated
        sub = nodes[::2][::-1]
        tsub = [0.5 * ref["lengths"][n] + 0.01 for n in sub]
        rc, X2 = inst.calculate_cross_products(edge_lengths=tsub, **cross_indices(bd, sub))
        X2r = x_ref(ref, sub, tsub)
        assert rc == 0
        worst.append(float((np.abs(X2 - X2r) / (f * X2r)).max()))
        # 3. the identity with the branch-length gradient of the same instance: sum_ij Q_ij X_ij = sum_e t_e g_e
        grad = bd.BranchGradient(0)
        rc, X3 = inst.calculate_cross_products(edge_lengths=lengths, **cross_indices(bd, nodes))
        assert rc == 0 and np.array_equal(X3, X)
        Q = rate_matrix(div)
        gb = gradient_bounds(div, gref, u)
        lhs, rhs = float((Q * X).sum()), sum(tl * grad[n] for n, tl in zip(nodes, lengths))
        slack = float((np.abs(Q) * f * Xr).sum()) + sum(tl * float((w * gb[n]).sum()) for n, tl in zip(nodes, lengths))
        worst.append(abs(lhs - rhs) / slack)
        # 4. no edges: zeros
        rc, X0 = inst.calculate_cross_products([], [], [], [], [])
        assert rc == 0 and X0.shape == (states, states) and not X0.any()
        print("%d states x %d x %d, %d taxa%s: error / bound: all %d branches %.3f, %d branches %.3f, identity %.3f (sum Q X = %.6g)" %
              (states, ncat, npat, t.ntaxa, " fp64" if double_precision else "", len(nodes), worst[0], len(sub), worst[1], worst[2], lhs))
        assert max(worst) <= 1.0, worst
        return worst
    finally:
        bd.finalize()


#        states, categories, patterns                     what it reaches
CASES = [(4, 4, 130),             # two full 64-pattern blocks plus 2 patterns
         (4, 9, 70),              # a second batch of eight categories
         (3, 2, 70),              # the plain kernel, a small state count
         (12, 2, 70),             # the plain kernel, the MFMA level layout
         (12, 6, 70),             # the plain kernel, the generic level layout
         (16, 2, 70),             # the matrix-core threshold
         (20, 4, 70),             # one tile, tree-walk tiles, a tail of 6 patterns
         (33, 1, 70),             # the second tile row and column hold one state
         (61, 1, 40),             # 2 x 2 tiles, one category: no posteriors; a partial block
         (61, 2, 70)]
CASES_F64 = [(4, 4, 130), (20, 2, 70)]


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_cross_products_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_cross_products_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


def test_cross_products_deep_tree_on_emulation(emu):
    """60 taxa: likelihoods down to ~1e-55 in the float64 reference, far below fp32's range"""
    assert gradient_reference(4, 4, 70, 60)["min_L"] < 1e-45
    check_case(emu, 4, 4, 70, ntaxa=60)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_cross_products(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_cross_products_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
def test_cross_products_deep_tree(gpu):
    check_case(gpu, 4, 4, 70, ntaxa=60)


# ---- the matrix-core kernel against the plain one ---------------------------------------------------------------------------------
def _cross_call(lib, div):
    """(children, X, launches of the call) on a fresh instance"""
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, pre_order=True)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        X = bd.RateMatrixCrossProducts(0)
        nodes = list(div.tree.all_down_pass)
        bd.inst.get_kernel_timing(reset=True)
        rc, X1 = bd.inst.calculate_cross_products(edge_lengths=[branch_length(div.tree, n) for n in nodes], **cross_indices(bd, nodes))
        _, launches = bd.inst.get_kernel_timing(reset=True)
        assert rc == 0 and np.array_equal(X, X1)
        return bd.inst.child_count(), X, launches
    finally:
        bd.finalize()


MFMA_CASES = [(20, 4, 70), (33, 1, 70), (61, 2, 70)]


def check_mfma_against_generic(lib, monkeypatch, states, ncat, npat):
    """MBAMD_XPROD_GENERIC=1 sends 16 ... 64 states to the plain kernel: each result within b of the reference and within 2 b of the
    other; the launch count (mbamdGetKernelTiming) tells the kernels apart -- the matrix-core kernel is one launch, the plain one
    a launch per 256 entries of the matrix, and k_cross_product_sums one more"""
    div, ref = division(states, ncat, npat), reference(states, ncat, npat)
    nodes = ref["nodes"]
    Xr = x_ref(ref, nodes, [ref["lengths"][n] for n in nodes])
    b = bound_factor(div, ref, U32) * Xr
    monkeypatch.delenv("MBAMD_XPROD_GENERIC", raising=False)
    _, Xm, lm = _cross_call(lib, div)
    monkeypatch.setenv("MBAMD_XPROD_GENERIC", "1")
    try:
        _, Xg, lg = _cross_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_XPROD_GENERIC")
    print("%d states x %d x %d: error / bound: matrix core %.3f, plain %.3f, one against the other (2 b) %.3f; launches %d and %d" %
          (states, ncat, npat, float((np.abs(Xm - Xr) / b).max()), float((np.abs(Xg - Xr) / b).max()),
           float((np.abs(Xm - Xg) / (2.0 * b)).max()), lm, lg))
    assert np.all(np.abs(Xm - Xr) <= b) and np.all(np.abs(Xg - Xr) <= b) and np.all(np.abs(Xm - Xg) <= 2.0 * b)
    assert lm == 2 and lg == (states * states + 255) // 256 + 1 and lg != lm, (lm, lg)


@pytest.mark.parametrize("states,ncat,npat", MFMA_CASES)
def test_mfma_against_generic_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_mfma_against_generic(emu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", MFMA_CASES)
def test_mfma_against_generic(gpu, monkeypatch, states, ncat, npat):
    check_mfma_against_generic(gpu, monkeypatch, states, ncat, npat)


# ---- pattern shards -----------------------------------------------------------------------------------------------------------
def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 4 states x 4 categories x 130 patterns: the children's matrices added"""
    div, ref = division(4, 4, 130), reference(4, 4, 130)
    nodes = ref["nodes"]
    Xr = x_ref(ref, nodes, [ref["lengths"][n] for n in nodes])
    b = bound_factor(div, ref, U32) * Xr
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    n0, X0, _ = _cross_call(lib, div)
    monkeypatch.setenv("MBAMD_SHARD", "2")
    try:
        n2, X2, _ = _cross_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n0 == 1 and n2 == 2
    assert np.all(np.abs(X2 - X0) <= b) and np.all(np.abs(X2 - Xr) <= b) and np.all(np.abs(X0 - Xr) <= b)


def test_sharded_cross_products_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_cross_products(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


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
    nodes = list(t.all_down_pass)
    lengths = [branch_length(t, n) for n in nodes]
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    try:
        inst = bd.inst
        cross = inst.calculate_cross_products
        # more than one category and no log-likelihood call yet
        raises(bg.BEAGLE_ERROR_GENERAL, cross, edge_lengths=lengths, **cross_indices(bd, nodes))
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.RateMatrixCrossProducts(0)
        ix = cross_indices(bd, nodes)                                                   # (the evaluation flipped index tables)
        n = len(nodes)
        assert cross(edge_lengths=lengths, **ix)[0] == 0
        # a buffer for the sums of squares
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, cross, edge_lengths=lengths, squared=True, **ix)
        # a weights index different from the remembered one
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **dict(ix, weights=[bd.cijkScratchIndex] * n))
        # a pre index that no pre-order operation wrote; one that beagleUpdatePartials has overwritten since
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **dict(ix, pres=[bd.preOrderStartIndex] * n))
        ops = bd.PreOrderOperations(0)
        victim = bd.preOrderIndex[t.root_left]
        inst.update_partials(np.array([[victim, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, bd.condLikeIndex[0][0], bd.tiProbsIndex[0][0],
                                        bd.condLikeIndex[0][1], bd.tiProbsIndex[0][1]]], dtype=np.int32), bg.BEAGLE_OP_NONE)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **ix)
        inst.update_pre_partials(ops)                                                   # (all of them pre-order buffers again)
        assert cross(edge_lengths=lengths, **ix)[0] == 0
        # an invalid post buffer, an unknown rates index
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **dict(ix, posts=[10 ** 6] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **dict(ix, posts=[-1] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **dict(ix, rates=[7] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths, **dict(ix, rates=[-1] * n))
        # an edge length that is negative or not finite
        for bad in (-1e-3, float("nan"), float("inf")):
            raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, cross, edge_lengths=lengths[:-1] + [bad], **ix)
        # null arrays
        arrays = [np.asarray(ix[key], dtype=np.int32) for key in ("posts", "pres", "rates", "weights")] + [np.asarray(lengths, dtype=np.float64)]
        out = np.empty((4, 4))
        for missing in range(6):
            ptrs = [a.ctypes.data_as(_dp if a.dtype == np.float64 else _ip) for a in arrays] + [out.ctypes.data_as(_dp)]
            ptrs[missing] = None
            rc = inst.lib.beagleCalculateCrossProductDerivative(inst.id, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], n, ptrs[5], None)
            assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE and lib.last_error(), (missing, rc)
            seen.append((rc, lib.last_error()))
        # the latest log-likelihood call had two subsets
        top = t.root_left
        one = dict(parents=[bd.condLikeIndex[0][top]], children=[bd.condLikeIndex[0][t.root]], probs=[bd.tiProbsIndex[0][top]],
                   weights=[bd.cijkIndex[0]], freqs=[bd.cijkIndex[0]], cums=[bd.siteScalerIndex[0]])
        inst.calculate_edge_log_likelihoods(**{key: value * 2 for key, value in one.items()})
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, cross, edge_lengths=lengths, **ix)
        inst.calculate_edge_log_likelihoods(**one)
        assert cross(edge_lengths=lengths, **ix)[0] == 0
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
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst.calculate_cross_products, [0], [N + 1], [0], [0], [0.1])
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
