"""The gradient in the site model: category rates, category weights and the direct term of the root frequencies
(mbamdCalculateSiteModelDerivatives; csrc/mbamd_site_model.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference (tests/site_model_reference.py) is numpy float64 from the `Division` alone; test_reference_against_finite_differences
checks it against central differences of the float64 log-likelihood in every r_k (P rebuilt from the eigen-system), every w_k and
every pi_i at fixed Q.

Tolerance, derived and not tuned.  Every output is a sum over patterns and categories of terms  weight q_k x / den_k  with x a sum
of products of one pre-order (or parent) component, one matrix entry and one post-order (or child) component.  This is the
structure of the cross-product matrix (tests/test_cross_products.py), contracted with D, and the argument is that one: with h the
operations on the longest post-order chain plus those on the longest pre-order chain, a component of either buffer carries at most
(S + 8) (1 + 2 h) u relative error; den, a sum of products of such components, 2 (S + 8) (1 + 2 h) u; q, a ratio of sums of the same
kind at another branch, is counted with den: 4 (S + 8) (1 + 2 h) u together.  Where the cross products add up to 64 K products in an
fp32 accumulator (64 K u), this call runs an S-term FMA chain over a row of D in the engine's precision: S u, relative to the sum of
the ABSOLUTE terms -- D has both signs, so the bound is on A (the same sum with |D|), not on the value.  D's own rounding to the
engine's precision, the product with the pre-order component, the conversions and the division, and the double-precision sums: 8 u.
    |G[e][k] - G_ref[e][k]| <= f A_ref[e][k],        f = (4 (S + 8) (1 + 2 h) + S + 8) u = site_factor
    |R[k] - R_ref[k]|       <= f sum_e t_e A_ref[e][k]
    |C[k] - C_ref[k]|       <= f C_ref[k],           |F[i] - F_ref[i]| <= f F_ref[i]          (sums of non-negative terms)
The constant differs from tests/preorder_reference.bound_factor in S u where that has 64 K u -- there is no matrix-core accumulator
here -- and is the smaller of the two at every shape below.  u = 2^-24 on the single-precision engine, 2^-53 kappa on the
double-precision engine (unit_roundoff).
"""
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.preorder_reference import CASES, CASES_F64, bounds, division, gradient_indices, rate_matrix, tip_vector, unit_roundoff
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA, U32
from tests.site_model_reference import reference, site_factor
from tests.test_derivatives import expected_layout

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
NONE = bg.BEAGLE_OP_NONE


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
def log_likelihood(div, lengths, rates, w, pi):
    """the float64 log-likelihood with the category rates, category weights (as given, not normalised) and root frequencies as
    arguments; the transition matrices from the division's eigen-system, which stays what it is: Q is fixed"""
    t, K = div.tree, div.ncat
    es = div.eigen[0]
    U, Ui, lam = (np.asarray(x, dtype=np.float64) for x in (es.evec, es.ivec, es.eval))
    mats = {n: np.stack([(U * np.exp(lam * r * lengths[n])[None, :]) @ Ui for r in rates]) for n in t.all_down_pass}
    cl = {tip: np.broadcast_to(tip_vector(div, tip), (K, div.npatterns, div.nstates)) for tip in range(t.ntaxa)}
    for p in t.int_down_pass:
        out = np.ones((K, div.npatterns, div.nstates))
        for c in (t.left[p], t.right[p]):
            out = out * np.einsum("kij,kcj->kci", mats[c], cl[c])
        cl[p] = out
    top = t.root_left
    L = np.einsum("k,i,kci,kij,kcj->c", w, pi, cl[top], mats[top], cl[t.root])
    return float((div.weights * np.log(L)).sum())


@pytest.mark.parametrize("states,ncat,npat,ntaxa", [(4, 4, 70, NTAXA), (4, 4, 70, 60), (20, 4, 70, NTAXA)])
def test_reference_against_finite_differences(states, ncat, npat, ntaxa):
    """The reference itself (no engine code): R_ref[k], C_ref[k] / w_k and F_ref[i] against central differences of the float64
    log-likelihood in r_k, w_k and pi_i.  Step and tolerance as test_preorder_gradient.test_reference_against_finite_differences:
    1e-4 of the parameter (at least 1e-7), 2e-6 relative to |g| + 1."""
    div, ref = division(states, ncat, npat, ntaxa), reference(states, ncat, npat, ntaxa)
    r0, w0, pi0 = np.asarray(div.cat_rates, dtype=np.float64), div.category_weights(0), np.asarray(div.pi, dtype=np.float64)
    worst = 0.0
    for which, x0, grad in ((0, r0, ref["R"]), (1, w0, ref["C"] / w0), (2, pi0, ref["F"])):
        for i in range(len(x0)):
            step = max(1e-4 * x0[i], 1e-7)
            side = []
            for sign in (1.0, -1.0):
                args = [r0.copy(), w0.copy(), pi0.copy()]
                args[which][i] += sign * step
                side.append(log_likelihood(div, ref["lengths"], *args))
            fd = (side[0] - side[1]) / (2.0 * step)
            worst = max(worst, abs(fd - grad[i]) / (abs(grad[i]) + 1.0))
    print("site-model reference against central differences (%d states, %d taxa): worst relative difference %.2e" % (states, div.tree.ntaxa, worst))
    assert worst <= 2e-6, worst


# ---- engine against reference -------------------------------------------------------------------------------------------------
def prepared(div, lib, double_precision=False):
    """a BeagleDivision after LogLike, AcceptMove and BranchGradient: the pre-order buffers are there, q is that of the edge call"""
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchGradient(0)
    except Exception:
        bd.finalize()
        raise
    return bd


def set_unit_matrix(bd):
    d = bd.div
    bd.inst.set_differential_matrix(bd.diffMatrixIndex, np.broadcast_to(rate_matrix(d), (d.ncat, d.nstates, d.nstates)))


def ratios(out, ref, f):
    """error / bound of the four outputs (rc, G, R, C, F) of one call against the reference"""
    _, G, R, Cn, F = out
    return [float((np.abs(G - ref["G"]) / (f * ref["A"])).max()), float((np.abs(R - ref["R"]) / (f * ref["RA"])).max()),
            float((np.abs(Cn - ref["C"]) / (f * ref["C"])).max()), float((np.abs(F - ref["F"]) / (f * ref["F"])).max())]


def check_case(lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA):
    div = division(states, ncat, npat, ntaxa)
    ref = reference(states, ncat, npat, ntaxa)
    f = site_factor(div, ref, unit_roundoff(div, gradient_reference(states, ncat, npat, ntaxa), double_precision))
    bd = prepared(div, lib, double_precision)
    try:
        assert expected_layout(states, ncat, double_precision) in bd.inst.details.implName.decode()
        set_unit_matrix(bd)
        out = bd.inst.calculate_site_model_derivatives(edge_lengths=ref["t"], **gradient_indices(bd))
        assert out[0] == 0 and out[1].shape == (len(ref["nodes"]), ncat)
        worst = ratios(out, ref, f)
        print("%d states x %d x %d, %d taxa%s: error / bound: per edge and category %.3f, rates %.3f, counts %.3f, root frequencies %.3f" %
              ((states, ncat, npat, div.tree.ntaxa, " fp64" if double_precision else "") + tuple(worst)))
        assert max(worst) <= 1.0, worst
        # the front end: the same call with the tree's own lengths
        rates, counts, root = bd.SiteModelGradient(0)
        assert np.array_equal(rates, out[2]) and np.array_equal(counts, out[3]) and np.array_equal(root, out[4])
    finally:
        bd.finalize()


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_site_model_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_site_model_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


def test_site_model_deep_tree_on_emulation(emu):
    check_case(emu, 4, 4, 70, ntaxa=60)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_site_model(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_site_model_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
def test_site_model_deep_tree(gpu):
    check_case(gpu, 4, 4, 70, ntaxa=60)


# ---- identities on the engine's own outputs -----------------------------------------------------------------------------------
def check_identities(lib, states, ncat, npat, double_precision=False):
    div = division(states, ncat, npat)
    gref = gradient_reference(states, ncat, npat)
    ref, rref = reference(states, ncat, npat), reference(states, ncat, npat, unit=False)
    u = unit_roundoff(div, gref, double_precision)
    f, w, pi = site_factor(div, ref, u), div.weights, np.asarray(div.pi, dtype=np.float64)
    t = div.tree
    bd = prepared(div, lib, double_precision)
    try:
        inst, ix = bd.inst, gradient_indices(bd)
        # D_k = r_k Q (BranchGradient left it): the categories of an edge add up to the branch-length gradient
        _, _, sums, _ = inst.calculate_edge_gradient(sites=False, **ix)
        _, G, _, Cn, F = inst.calculate_site_model_derivatives(rates=False, **ix)
        b = bounds(div, gref, u)
        for e, n in enumerate(ref["nodes"]):
            assert abs(G[e].sum() - sums[e]) <= float((w * b[n]).sum()) + f * float(rref["A"][e].sum()), (n, G[e].sum(), sums[e])
        # the counts and the root term, weighted with pi, add up to the number of sites
        assert abs(Cn.sum() - w.sum()) <= f * float(ref["C"].sum()), (Cn.sum(), w.sum())
        assert abs(float(pi @ F) - w.sum()) <= f * float(pi @ ref["F"]), (float(pi @ F), w.sum())
        # a root call as the latest log-likelihood call: its buffer is the top node's partials times the root branch's factor,
        # made by one operation (the top node through an identity matrix, the root tip through the root branch's matrix)
        top, S = t.root_left, div.nstates
        x, eye = bd.condLikeScratchIndex[top], bd.tiProbsScratchIndex[0]
        inst.set_transition_matrix(eye, np.broadcast_to(np.eye(S), (div.ncat, S, S)))
        inst.update_partials(np.array([[x, NONE, NONE, bd.condLikeIndex[0][top], eye, bd.condLikeIndex[0][t.root], bd.tiProbsIndex[0][top]]],
                                      dtype=np.int32), NONE)
        rc, _ = inst.calculate_root_log_likelihoods([x], [bd.cijkIndex[0]], [bd.cijkIndex[0]], [bd.siteScalerIndex[0]])
        assert rc == 0
        _, _, _, Cr, Fr = inst.calculate_site_model_derivatives(edges=False, rates=False, **ix)
        assert np.all(np.abs(Fr - F) <= 2.0 * f * ref["F"]), (Fr, F)
        assert np.all(np.abs(Fr - ref["F"]) <= f * ref["F"]) and np.all(np.abs(Cr - ref["C"]) <= f * ref["C"])
    finally:
        bd.finalize()


IDENTITY_CASES = [(4, 4, 130, False), (20, 4, 70, False), (12, 6, 70, False), (61, 1, 40, False), (4, 4, 130, True)]


@pytest.mark.parametrize("states,ncat,npat,double_precision", IDENTITY_CASES)
def test_identities_on_emulation(emu, states, ncat, npat, double_precision):
    check_identities(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", IDENTITY_CASES)
def test_identities(gpu, states, ncat, npat, double_precision):
    check_identities(gpu, states, ncat, npat, double_precision)


# ---- determinism --------------------------------------------------------------------------------------------------------------
def _all_outputs(lib, div, lengths, double_precision=False, variations=False):
    bd = prepared(div, lib, double_precision)
    try:
        set_unit_matrix(bd)
        ix = gradient_indices(bd)
        call = bd.inst.calculate_site_model_derivatives
        full = call(edge_lengths=lengths, **ix)
        if variations:
            again = call(edge_lengths=lengths, **ix)
            for a, b in zip(full[1:], again[1:]):
                assert np.array_equal(a, b)
            names = ("edges", "rates", "counts", "root")
            for i, name in enumerate(names):
                alone = call(edge_lengths=lengths, **dict(ix, **{n: n == name for n in names}))
                assert np.array_equal(alone[1 + i], full[1 + i]), name
                assert all(alone[1 + j] is None for j in range(4) if j != i)
                without = call(edge_lengths=lengths, **dict(ix, **{n: n != name for n in names}))
                for j in range(4):
                    assert (without[1 + j] is None) if j == i else np.array_equal(without[1 + j], full[1 + j]), (name, j)
            # no edges: the edge outputs are zeros, the two others what they were
            none = call([], [], [], [], edge_lengths=[])
            assert none[1].shape == (0, div.ncat) and np.array_equal(none[2], np.zeros(div.ncat))
            assert np.array_equal(none[3], full[3]) and np.array_equal(none[4], full[4])
        return bd.inst.child_count(), full
    finally:
        bd.finalize()


def check_determinism(lib, monkeypatch, states, ncat, npat, double_precision=False):
    """every output bit for bit the same with and without each other output, called twice, and with the 13 edges in three chunks
    (MBAMD_POSTERIOR_NODES=5, the cap of chunked_readout: boundaries inside the list)"""
    div, ref = division(states, ncat, npat), reference(states, ncat, npat)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    monkeypatch.delenv("MBAMD_POSTERIOR_NODES", raising=False)
    _, whole = _all_outputs(lib, div, ref["t"], double_precision, variations=True)
    monkeypatch.setenv("MBAMD_POSTERIOR_NODES", "5")
    try:
        bd = prepared(div, lib, double_precision)
        try:
            set_unit_matrix(bd)
            bd.inst.get_kernel_timing(reset=True)
            cut = bd.inst.calculate_site_model_derivatives(edge_lengths=ref["t"], **gradient_indices(bd))
            _, launches = bd.inst.get_kernel_timing(reset=True)
        finally:
            bd.finalize()
    finally:
        monkeypatch.delenv("MBAMD_POSTERIOR_NODES")
    assert len(ref["nodes"]) == 13 and launches == 3 * 2 + 3, launches
    for a, b in zip(whole[1:], cut[1:]):
        assert np.array_equal(a, b)


DETERMINISM_CASES = [(4, 4, 130, False), (20, 4, 70, False), (4, 4, 130, True)]


@pytest.mark.parametrize("states,ncat,npat,double_precision", DETERMINISM_CASES)
def test_determinism_on_emulation(emu, monkeypatch, states, ncat, npat, double_precision):
    check_determinism(emu, monkeypatch, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", DETERMINISM_CASES)
def test_determinism(gpu, monkeypatch, states, ncat, npat, double_precision):
    check_determinism(gpu, monkeypatch, states, ncat, npat, double_precision)


# ---- pattern shards -----------------------------------------------------------------------------------------------------------
def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 4 states x 4 categories x 130 patterns: the children's sums added in child order"""
    div, ref = division(4, 4, 130), reference(4, 4, 130)
    f = site_factor(div, ref, U32)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    n0, one = _all_outputs(lib, div, ref["t"])
    monkeypatch.setenv("MBAMD_SHARD", "2")
    try:
        n2, two = _all_outputs(lib, div, ref["t"])
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n0 == 1 and n2 == 2
    assert max(ratios(two, ref, f)) <= 1.0 and max(ratios(one, ref, f)) <= 1.0
    for a, b, bound in zip(one[1:], two[1:], (ref["A"], ref["RA"], ref["C"], ref["F"])):
        assert np.all(np.abs(a - b) <= 2.0 * f * bound)


def test_sharded_site_model_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_site_model(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- argument errors ----------------------------------------------------------------------------------------------------------
POISON = -7.25


def raw_call(lib, inst, posts, pres, dmats, weights, lengths, count, want=(True, True, True, True)):
    """the C entry itself on poisoned output arrays: (status, message, the arrays were left as they were).  An index array or
    `lengths` may be None (NULL)."""
    K, S = inst.category_count, inst.state_count
    ints = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (posts, pres, dmats, weights)]
    t = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.float64)
    outs = [np.full(n, POISON) if on else None for n, on in zip((max(count, 1) * K, K, K, S), want)]
    rc = lib.lib.mbamdCalculateSiteModelDerivatives(inst.id, *[None if a is None else a.ctypes.data_as(_ip) for a in ints],
                                                    None if t is None else t.ctypes.data_as(_dp), count,
                                                    *[None if o is None else o.ctypes.data_as(_dp) for o in outs])
    return rc, lib.last_error() if rc else "", all(o is None or np.all(o == POISON) for o in outs)


def check_argument_errors(lib, double_precision=False):
    """Every bad call is refused with the expected status and a message, and writes nothing; returns (status, message) of each, in
    order: the two engines run one body (mbamd_site_model.h), so they answer alike -- check_engines_agree."""
    seen = []

    def refused(code, inst, *args, **kwargs):
        rc, message, untouched = raw_call(lib, inst, *args, **kwargs)
        assert rc == code, (rc, code, message)
        assert message and untouched, (message, untouched)
        seen.append((rc, message))

    div = division(4, 2, 130)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    try:
        inst = bd.inst
        ix = gradient_indices(bd)
        n = len(ix["posts"])
        t = [0.1] * n
        # more than one category and no log-likelihood call yet
        refused(bg.BEAGLE_ERROR_GENERAL, inst, ix["posts"], ix["pres"], ix["dmats"], ix["weights"], t, n)
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.BranchGradient(0)
        ix = gradient_indices(bd)                                                       # (the evaluation flipped index tables)
        good = (ix["posts"], ix["pres"], ix["dmats"], ix["weights"])
        assert raw_call(lib, inst, *good, t, n)[0] == 0
        # a weights index different from the remembered one; a pre index no pre-order operation wrote; matrix and buffer indices
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix["posts"], ix["pres"], ix["dmats"], [bd.cijkScratchIndex] * n, t, n)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix["posts"], [bd.preOrderStartIndex] * n, ix["dmats"], ix["weights"], t, n)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix["posts"], [10 ** 6] * n, ix["dmats"], ix["weights"], t, n)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix["posts"], ix["pres"], [10 ** 6] * n, ix["weights"], t, n)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix["posts"], ix["pres"], ix["dmats"][:-1] + [-1], ix["weights"], t, n)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, [10 ** 6] * n, ix["pres"], ix["dmats"], ix["weights"], t, n)
        # a bad index is found whichever outputs are asked for
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, ix["posts"], ix["pres"], [10 ** 6] * n, ix["weights"], t, n, want=(False, False, True, True))
        # NULL index arrays, a negative count
        for missing in range(4):
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, *[None if i == missing else a for i, a in enumerate(good)], t, n)
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, *good, t, -1)
        # the edge lengths: NULL with the rates asked for, negative, not finite
        refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, *good, None, n)
        assert raw_call(lib, inst, *good, None, n, want=(True, False, True, True))[0] == 0
        for bad in (-0.1, float("nan"), float("inf")):
            refused(bg.BEAGLE_ERROR_OUT_OF_RANGE, inst, *good, t[:3] + [bad] + t[4:], n)
        # every output NULL
        rc, message, _ = raw_call(lib, inst, *good, t, n, want=(False, False, False, False))
        assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE and message
        seen.append((rc, message))
        # no edges is legal, with NULL index arrays too
        rc, _, untouched = raw_call(lib, inst, None, None, None, None, None, 0, want=(True, False, True, True))
        assert rc == 0 and not untouched
        # a latest log-likelihood call with two subsets (the root branch's operands twice)
        top, root = div.tree.root_left, div.tree.root
        two = [[bd.condLikeIndex[0][top]] * 2, [bd.condLikeIndex[0][root]] * 2, [bd.tiProbsIndex[0][top]] * 2, [bd.cijkIndex[0]] * 2,
               [bd.cijkIndex[0]] * 2, [bd.siteScalerIndex[0]] * 2]
        assert inst.calculate_edge_log_likelihoods(*two)[0] == 0
        refused(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst, *good, t, n)
        refused(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst, None, None, None, None, None, 0, want=(False, False, False, True))
    finally:
        bd.finalize()
    N, S, P = NTAXA, 4, 130
    flags = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
    # one category: the root term needs a log-likelihood call, the others do not
    inst = bg.BeagleInstance(lib, N, 3 * N, N, S, P, 2, 4 * N, 1, N, preference_flags=flags)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.asarray(div.tip_states[tip]).astype(np.int32))
        inst.set_pattern_weights(div.weights)
        rng = np.random.default_rng(3)
        inst.set_partials(N, rng.uniform(0.1, 1.0, size=(1, P, S)))
        m = rng.uniform(0.1, 1.0, size=(1, S, S))
        inst.set_transition_matrix(0, m / m.sum(axis=2, keepdims=True))
        inst.update_pre_partials(np.array([[N + 1, NONE, NONE, N, 0, NONE, NONE]], dtype=np.int32))
        inst.set_differential_matrix(1, rate_matrix(div)[None, :, :])
        refused(bg.BEAGLE_ERROR_GENERAL, inst, [0], [N + 1], [1], [0], [0.1], 1)
        rc, out, r, c, f = inst.calculate_site_model_derivatives([0], [N + 1], [1], [0], [0.1], root=False)
        assert rc == 0 and f is None and out.shape == (1, 1) and c[0] == div.weights.sum() and r[0] == 0.1 * out[0, 0]
    finally:
        inst.finalize()
    # a multi-partition instance is not served
    inst = bg.BeagleInstance(lib, N, 3 * N, N, S, P, 2, 4 * N, 2, N, preference_flags=flags)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.asarray(div.tip_states[tip]).astype(np.int32))
        inst.set_pattern_weights(div.weights)
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
        assert inst.child_count() == 2
        refused(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, inst, [0], [N + 1], [0], [0], [0.1], 1)
        assert "multi-partition" in seen[-1][1]
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


# ---- launches -----------------------------------------------------------------------------------------------------------------
def check_launches(lib, monkeypatch, double_precision=False):
    """one call over every branch at 4 states x 4 categories x 130 patterns is one chunk on one engine: the edge
    read-out and the launch that adds its block sums, the counts, the root term, and ONE launch that adds the block sums of both;
    q is BranchGradient's (the same log-likelihood call): no launch"""
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    monkeypatch.delenv("MBAMD_POSTERIOR_NODES", raising=False)
    div, ref = division(4, 4, 130), reference(4, 4, 130)
    bd = prepared(div, lib, double_precision)
    try:
        assert bd.inst.child_count() == 1
        ix = gradient_indices(bd)
        for kwargs, expected in ((dict(), 5), (dict(counts=False, root=False), 2), (dict(edges=False, rates=False), 3),
                                 (dict(edges=False, rates=False, root=False), 2)):
            bd.inst.get_kernel_timing(reset=True)
            assert bd.inst.calculate_site_model_derivatives(edge_lengths=ref["t"], **dict(ix, **kwargs))[0] == 0
            _, launches = bd.inst.get_kernel_timing(reset=True)
            assert launches == expected, (kwargs, launches, expected)
    finally:
        bd.finalize()


def test_launches_on_emulation(emu, monkeypatch):
    check_launches(emu, monkeypatch)
    check_launches(emu, monkeypatch, double_precision=True)


@pytest.mark.gpu
def test_launches(gpu, monkeypatch):
    check_launches(gpu, monkeypatch)
    check_launches(gpu, monkeypatch, double_precision=True)
