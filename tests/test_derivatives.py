"""First and second derivative of the edge log-likelihood in the branch length (beagleUpdateTransitionMatrices /
beagleCalculateEdgeLogLikelihoods[ByPartition] with derivative arguments, beagleGetSiteDerivatives; csrc/mbamd_derivatives.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference is numpy float64 from the `Division` alone: Felsenstein pruning of the whole tree to the two ends of the root
branch (no scaling at these sizes), P / P' / P'' from the eigen-system and the category rates, then
    L_c = sum_k w_k sum_i pi_i parent[k,c,i] sum_j P_k[i,j] child[k,c,j],   D1_c, D2_c the same with P', P'',
    d1_c = D1_c / L_c,   d2_c = D2_c / L_c - d1_c^2.

Tolerances are the forward-error bound of an n-term inner product, from the reference's own quantities: with A1_c the sum of the
absolute values of D1_c's addends (A2_c likewise),
    |d1 - d1_ref| <= (S + 8) u (A1_c + |D1_c|) / L_c
    |d2 - d2_ref| <= (S + 8) u [(A2_c + |D2_c|) / L_c + 2 |d1_c| (A1_c + |D1_c|) / L_c]
u = 2^-24 (single precision); u = 2^-53 kappa on the double-precision engine, kappa the cancellation inside the spectral sum of
the matrices (computed below from the eigen-system).  The weighted sums get sum_c weight_c times the per-site bounds.
(The matrices P, P', P'' themselves are held to a tighter bound, in double roundoffs, by tests/test_matrix_bounds.py.)
"""
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.pruning_reference import NTAXA, U32, U64, branch_length, interior_edge, kappa, make_division, reference, spectral

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


def expected_layout(states, ncat, double_precision):
    if double_precision:
        return "double-precision"
    if states == 4:
        return "4-state tree-walk kernels"
    if states in (2, 3, 5, 6, 7, 8, 9, 10, 16, 20, 40, 60, 61, 62, 63):
        return "general-state tree-walk kernels"
    if states >= 5 and ((states <= 32 and ncat <= 4) or ncat <= 2):
        return "general-state MFMA"
    return "general-state vector kernels"


def edge_indices(bd):
    t = bd.div.tree
    p = t.root_left
    return dict(parents=[bd.condLikeIndex[0][p]], children=[bd.condLikeIndex[0][t.root]],
                probs=[bd.tiProbsIndex[0][p]], weights=[bd.cijkIndex[0]], freqs=[bd.cijkIndex[0]], cums=[bd.siteScalerIndex[0]])


def interior_edge_indices(bd):
    """The same likelihood over the branch above interior_edge's v: the parent end is a new buffer, (u's factor) x (the root tip's
    factor), with its own node exponents; the cumulative buffer is every node's exponents except the top node's, plus the new ones."""
    t, inst = bd.div.tree, bd.inst
    top = t.root_left
    v, u = interior_edge(t)
    x, sx, cum = bd.condLikeScratchIndex[top], bd.nodeScalerScratchIndex[top], bd.siteScalerScratchIndex
    inst.update_partials(np.array([[x, sx, bg.BEAGLE_OP_NONE, bd.condLikeIndex[0][u], bd.tiProbsIndex[0][u],
                                    bd.condLikeIndex[0][t.root], bd.tiProbsIndex[0][top]]], dtype=np.int32), bg.BEAGLE_OP_NONE)
    inst.reset_scale_factors(cum)
    inst.accumulate_scale_factors([bd.nodeScalerIndex[0][p] for p in t.int_down_pass if p != top] + [sx], cum)
    return dict(parents=[x], children=[bd.condLikeIndex[0][v]], probs=[bd.tiProbsIndex[0][v]], weights=[bd.cijkIndex[0]],
                freqs=[bd.cijkIndex[0]], cums=[cum])


# ---- the per-case check -----------------------------------------------------------------------------------------------------
def check_case(lib, states, ncat, npat, double_precision=False, interior_child=False, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    div = make_division(states, ncat, npat)
    t = div.tree
    ref = reference(states, ncat, npat, interior=interior_child)
    S, tl = div.nstates, ref["t"]
    u = U64 * kappa(div, tl) if double_precision else U32
    um = U64 if double_precision else U32                   # the matrices: the bound is on the spectral terms themselves
    bd = lk.BeagleDivision(div, lib, scaling=scaling, double_precision=double_precision)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(states, ncat, double_precision) in name, name
        full = bd.LogLike(0)
        bd.AcceptMove(0)
        assert np.any(inst.get_scale_exponents(bd.siteScalerIndex[0]) != 0)     # SCALE_ALWAYS: the exponents are not all zero
        ix = interior_edge_indices(bd) if interior_child else edge_indices(bd)
        pcopy, m1, m2 = (bd.tiProbsScratchIndex[i] for i in (0, 1, 2))
        # -- matrices: P bit-equal to the call without derivative lists, P' and P'' against the spectral sums
        inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [tl], first=[m1], second=[m2])
        assert np.array_equal(inst.get_transition_matrix(pcopy), inst.get_transition_matrix(ix["probs"][0]))
        for order, buf in ((1, m1), (2, m2)):
            want, mag = spectral(div, tl, order)
            got = inst.get_transition_matrix(buf)
            ratio = float((np.abs(got - want) / ((S + 8) * um * mag)).max())
            print("%d states x %d: d%dP/dt%d worst error / bound %.3f" % (states, ncat, order, order, ratio))
            assert ratio <= 1.0, (states, ncat, order, ratio)
        assert (inst.get_transition_matrix(m1) < 0).any()                       # (not clamped)
        # -- the plain call, then the derivative call on the same arguments
        rc, plain = inst.calculate_edge_log_likelihoods(**ix)
        assert rc == 0
        if not interior_child:
            assert plain == full
        else:                                               # (the same tree seen from another branch: fp32 rounding apart)
            assert abs(plain - full) <= 1e-5 * abs(full), (plain, full)
        plain_sites = inst.get_site_log_likelihoods()
        rc, lnl, d1, d2 = inst.calculate_edge_derivatives(first=[m1], second=[m2], **ix)
        assert rc == 0
        sites = inst.get_site_log_likelihoods()
        s1, s2 = inst.get_site_derivatives()
        assert abs(lnl - plain) <= 1e-10 * abs(plain), (lnl, plain)
        assert np.all(np.abs(sites - plain_sites) <= 1e-10 * np.abs(plain_sites))
        b1, b2 = (S + 8) * u * ref["scale1"], (S + 8) * u * ref["scale2"]
        r1, r2 = float((np.abs(s1 - ref["d1"]) / b1).max()), float((np.abs(s2 - ref["d2"]) / b2).max())
        w = div.weights
        R1 = abs(d1 - float((w * ref["d1"]).sum())) / float((w * b1).sum())
        R2 = abs(d2 - float((w * ref["d2"]).sum())) / float((w * b2).sum())
        print("%d states x %d x %d%s%s: lnL %.9f d1 %.9f d2 %.9f; error / bound: sites %.3f %.3f, sums %.3f %.3f" %
              (states, ncat, npat, " fp64" if double_precision else "", " interior child" if interior_child else "", lnl, d1, d2, r1, r2, R1, R2))
        assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
        assert R1 <= 1.0 and R2 <= 1.0, (R1, R2)
        # -- the first derivative alone
        rc, lnl_f, d1_f, none = inst.calculate_edge_derivatives(first=[m1], second=None, **ix)
        assert rc == 0 and none is None
        assert abs(lnl_f - plain) <= 1e-10 * abs(plain)
        assert abs(d1_f - float((w * ref["d1"]).sum())) <= float((w * b1).sum())
        f1, _ = inst.get_site_derivatives()
        assert np.all(np.abs(f1 - ref["d1"]) <= b1)
        # -- a plain call afterwards: no derivatives to read any more
        inst.calculate_edge_log_likelihoods(**ix)
        out = np.empty(npat)
        assert inst.lib.beagleGetSiteDerivatives(inst.id, out.ctypes.data_as(_dp), None) == bg.BEAGLE_ERROR_GENERAL
    finally:
        bd.finalize()


#        states, categories, patterns                     what it reaches
CASES = [(4, 4, 130),             # two full 64-pattern blocks plus 2 patterns
         (4, 9, 70),              # the second batch of eight categories
         (20, 4, 70),             # two 32-pattern tiles plus 6 patterns
         (61, 1, 40),             # one eigen part
         (12, 2, 70),             # the MFMA level layout
         (12, 6, 70),             # the generic level layout
         (3, 2, 70)]              # a small state count (the engine puts 2-10 states except 4 on the tree-walk tiles)
CASES_F64 = [(4, 4, 130), (20, 2, 70)]


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_derivatives_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


def test_derivatives_interior_child_on_emulation(emu):
    check_case(emu, 4, 4, 130, interior_child=True)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_derivatives_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_derivatives(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
def test_derivatives_interior_child(gpu):
    check_case(gpu, 4, 4, 130, interior_child=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_derivatives_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def _raw_edge(inst, ix, first, second, want1, want2, count=1):
    arr = lambda v: np.ascontiguousarray(list(v) * count, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(_ip)
    keep = [arr(ix[k]) for k in ("parents", "children", "probs", "weights", "freqs", "cums")]
    f = None if first is None else arr(first)
    s = None if second is None else arr(second)
    out, o1, o2 = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    return inst.lib.beagleCalculateEdgeLogLikelihoods(inst.id, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(f), ptr(s), ptr(keep[3]),
                                                      ptr(keep[4]), ptr(keep[5]), count, C.byref(out),
                                                      C.byref(o1) if want1 else None, C.byref(o2) if want2 else None)


def check_argument_errors(lib, double_precision=False):
    div = make_division(4, 2, 130)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision)
    try:
        inst = bd.inst
        bd.LogLike(0)
        ix = edge_indices(bd)
        pcopy, m1, m2 = (bd.tiProbsScratchIndex[i] for i in (0, 1, 2))
        tl = branch_length(div.tree, div.tree.root_left)
        inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [tl], first=[m1], second=[m2])
        assert _raw_edge(inst, ix, [m1], [m2], True, True) == 0
        assert _raw_edge(inst, ix, [m1], None, True, False) == 0                                   # the first derivative alone
        assert _raw_edge(inst, ix, None, [m2], False, True) == bg.BEAGLE_ERROR_OUT_OF_RANGE        # a second without a first
        assert _raw_edge(inst, ix, [m1], [m2], True, False) == bg.BEAGLE_ERROR_OUT_OF_RANGE        # an index without its output
        assert _raw_edge(inst, ix, [m1], None, True, True) == bg.BEAGLE_ERROR_OUT_OF_RANGE         # an output without its index
        assert _raw_edge(inst, ix, None, None, True, False) == bg.BEAGLE_ERROR_OUT_OF_RANGE
        assert _raw_edge(inst, ix, [m1], [m2], True, True, count=2) == bg.BEAGLE_ERROR_NO_IMPLEMENTATION
        assert "one subset" in lib.last_error()
        # a derivative index equal to another output of the same matrices call
        with pytest.raises(bg.BeagleError) as err:
            inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [tl], first=[pcopy])
        assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE
        with pytest.raises(bg.BeagleError) as err:
            inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [tl], first=[m1], second=[m1])
        assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE
        # no derivative call was the last one: nothing to read
        inst.calculate_edge_log_likelihoods(**ix)
        with pytest.raises(bg.BeagleError) as err:
            inst.get_site_derivatives()
        assert err.value.code == bg.BEAGLE_ERROR_GENERAL
    finally:
        bd.finalize()


def test_argument_errors_on_emulation(emu):
    check_argument_errors(emu)
    check_argument_errors(emu, double_precision=True)


@pytest.mark.gpu
def test_argument_errors(gpu):
    check_argument_errors(gpu)
    check_argument_errors(gpu, double_precision=True)


# ---- pattern shards -------------------------------------------------------------------------------------------------------------
def _derivative_call(lib, div):
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS)
    try:
        inst = bd.inst
        bd.LogLike(0)
        ix = edge_indices(bd)
        pcopy, m1, m2 = (bd.tiProbsScratchIndex[i] for i in (0, 1, 2))
        inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [branch_length(div.tree, div.tree.root_left)], first=[m1], second=[m2])
        rc, lnl, d1, d2 = inst.calculate_edge_derivatives(first=[m1], second=[m2], **ix)
        assert rc == 0
        return inst.child_count(), (lnl, d1, d2), (inst.get_site_log_likelihoods(),) + inst.get_site_derivatives()
    finally:
        bd.finalize()


def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=3 at 4 states x 2 categories x 130 patterns: the children's sums added, their site arrays concatenated"""
    div = make_division(4, 2, 130)
    ref = reference(4, 2, 130)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    n0, sums0, sites0 = _derivative_call(lib, div)
    monkeypatch.setenv("MBAMD_SHARD", "3")
    try:
        n3, sums3, sites3 = _derivative_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n0 == 1 and n3 == 3
    for a, b in zip(sites0, sites3):
        assert np.array_equal(a, b)
    w = div.weights
    scales = (abs(sums0[0]), float((w * ref["scale1"]).sum()), float((w * ref["scale2"]).sum()))
    for a, b, scale in zip(sums0, sums3, scales):
        assert abs(a - b) <= 1e-12 * scale, (a, b, scale)


def test_sharded_derivatives_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_derivatives(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- partitions ---------------------------------------------------------------------------------------------------------------
def check_partitions(lib, double_precision=False):
    """A two-partition instance (70 + 60 patterns, their own models, trees and cumulative buffers) through the ByPartition form:
    every partition against the reference on its range."""
    keys = [(4, 2, 70, 11, 5), (4, 2, 60, 13, 7)]
    divs = [make_division(*k) for k in keys]
    refs = [reference(*k) for k in keys]
    S, K, N = 4, 2, NTAXA
    Pa, Pb = divs[0].npatterns, divs[1].npatterns
    nInt, nNodes = N - 2, 2 * N - 2
    u = U64 * max(kappa(d, r["t"]) for d, r in zip(divs, refs)) if double_precision else U32
    inst = bg.BeagleInstance(lib, N, N + nInt, N, S, Pa + Pb, 2, 2 * nNodes + 4, K, nInt + 2,
                             preference_flags=bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.concatenate([divs[0].tip_states[tip], divs[1].tip_states[tip]]).astype(np.int32))
        inst.set_pattern_weights(np.concatenate([divs[0].weights, divs[1].weights]))
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(Pa, dtype=np.int32), np.ones(Pb, dtype=np.int32)]))
        assert inst.child_count() == 2
        ops, eig_idx, rate_idx, prob_idx, lengths, first, second = [], [], [], [], [], [], []
        for d, dv in enumerate(divs):
            es = dv.eigen[0]
            inst.set_eigen_decomposition(d, es.evec, es.ivec, es.eval)
            inst.set_state_frequencies(d, dv.pi)
            inst.set_category_weights(d, dv.category_weights(0))
            inst.set_category_rates_with_index(d, dv.cat_rates)
            tr = dv.tree
            for p in tr.all_down_pass:
                if p == tr.root:
                    continue
                eig_idx.append(d); rate_idx.append(d); prob_idx.append(d * nNodes + p)
                lengths.append(branch_length(tr, p))
            for p in tr.int_down_pass:
                l, r = tr.left[p], tr.right[p]
                ops.append([p, p - N, -1, l, d * nNodes + l, r, d * nNodes + r, d, nInt + d])
        inst.update_transition_matrices_with_multiple_models(eig_idx, rate_idx, prob_idx, lengths)
        # the root branches once more, with their derivative matrices (probabilities into a spare buffer)
        spare = 2 * nNodes
        roots = [dv.tree.root_left for dv in divs]
        inst.update_transition_matrices_with_multiple_models([0, 1], [0, 1], [spare + 3, spare + 3], [refs[0]["t"], refs[1]["t"]],
                                                             first=[spare, spare + 1], second=None)
        inst.update_transition_matrices_with_multiple_models([0], [0], [spare + 3], [refs[0]["t"]], first=None, second=[spare + 2])
        for d in range(2):
            inst.reset_scale_factors_by_partition(nInt + d, d)
        mixed = [x for pair in zip(ops[:nInt], ops[nInt:]) for x in pair]
        inst.update_partials_by_partition(np.array(mixed, dtype=np.int32))
        parents, children = roots, [dv.tree.root for dv in divs]
        probs = [d * nNodes + roots[d] for d in range(2)]
        rc, by_plain, _ = inst.calculate_edge_log_likelihoods_by_partition(parents, children, probs, [0, 1], [0, 1], [nInt, nInt + 1], [0, 1], 1)
        assert rc == 0
        # first derivatives of both partitions in one call
        rc, lnl, d1, none = inst.calculate_edge_derivatives_by_partition(parents, children, probs, [spare, spare + 1], None, [0, 1], [0, 1],
                                                                         [nInt, nInt + 1], [0, 1])
        assert rc == 0 and none is None
        s1, _ = inst.get_site_derivatives()
        sites = inst.get_site_log_likelihoods()
        rng = [slice(0, Pa), slice(Pa, Pa + Pb)]
        for d in range(2):
            w, r = divs[d].weights, refs[d]
            b1 = (S + 8) * u * r["scale1"]
            assert abs(lnl[0][d] - by_plain[d]) <= 1e-10 * abs(by_plain[d])
            assert abs(d1[0][d] - float((w * r["d1"]).sum())) <= float((w * b1).sum()), d
            assert np.all(np.abs(s1[rng[d]] - r["d1"]) <= b1), d
            assert abs(float((sites[rng[d]] * w).sum()) - by_plain[d]) <= 1e-9 * abs(by_plain[d])
        assert abs(d1[1] - (d1[0][0] + d1[0][1])) <= 1e-12 * (abs(d1[0][0]) + abs(d1[0][1]))
        assert abs(lnl[1] - (lnl[0][0] + lnl[0][1])) <= 1e-12 * abs(lnl[1])
        # both derivatives of partition 0 alone
        rc, lnl0, d10, d20 = inst.calculate_edge_derivatives_by_partition([parents[0]], [children[0]], [probs[0]], [spare], [spare + 2], [0], [0],
                                                                          [nInt], [0])
        assert rc == 0
        w, r = divs[0].weights, refs[0]
        b1, b2 = (S + 8) * u * r["scale1"], (S + 8) * u * r["scale2"]
        assert abs(d10[0][0] - float((w * r["d1"]).sum())) <= float((w * b1).sum())
        assert abs(d20[0][0] - float((w * r["d2"]).sum())) <= float((w * b2).sum())
        assert d20[1] == d20[0][0] and d10[1] == d10[0][0] and lnl0[1] == lnl0[0][0]
        _, s2 = inst.get_site_derivatives()
        assert np.all(np.abs(s2[rng[0]] - r["d2"]) <= b2)
    finally:
        inst.finalize()


def test_partitioned_derivatives_on_emulation(emu):
    check_partitions(emu)
    check_partitions(emu, double_precision=True)


@pytest.mark.gpu
def test_partitioned_derivatives(gpu):
    check_partitions(gpu)
    check_partitions(gpu, double_precision=True)


# ---- a held root-ward path ------------------------------------------------------------------------------------------------------
def _depth(t, i):
    d = 0
    while t.anc[i] != -1:
        i = t.anc[i]
        d += 1
    return d


def check_held_path(lib):
    """A branch-length change on the four-state instance leaves a root-ward path held for the log-likelihood call: a derivative
    call runs it first (never the fused launch) and gives the plain sequence's lnL; the evaluation after it is bit-equal to a
    twin's that never saw a derivative call."""
    div = make_division.__wrapped__(4, 4, 130)             # (a division of its own: the branch lengths change; both engines read it)
    t = div.tree
    ref_t = branch_length(t, t.root_left)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS)
    twin = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS)
    try:
        assert bd.LogLike(0) == twin.LogLike(0)
        bd.AcceptMove(0); twin.AcceptMove(0)
        deep = sorted((i for i in range(t.ntaxa) if i != t.root), key=lambda i: _depth(t, i))
        b, b2 = deep[-1], deep[0]
        old = t.length[b]
        t.length[b] = old * 1.7
        bd.TouchBranch(0, b); twin.TouchBranch(0, b)
        want = twin.LogLike(0)
        twin.AcceptMove(0)
        # the same evaluation call by call (LaunchBEAGLELogLikeForDivision, SCALE_ALWAYS), the likelihood call with derivatives
        inst = bd.inst
        before = inst.get_list_counts()
        bd.FlipSiteScalerSpace(0)
        inst.copy_scale_factors(bd.siteScalerIndex[0], bd.siteScalerScratchIndex)
        bd.TreeTiProbs_Beagle(0)
        spare = [bd.tiProbsScratchIndex[i] for i in range(t.ntaxa) if i != b][:3]
        inst.update_transition_matrices(bd.cijkIndex[0], [spare[0]], [ref_t], first=[spare[1]], second=[spare[2]])
        bd.TreeCondLikes_Beagle_Always_Rescale(0)
        ix = edge_indices(bd)
        rc, lnl, d1, d2 = inst.calculate_edge_derivatives(first=[spare[1]], second=[spare[2]], **ix)
        after = inst.get_list_counts()
        bd.ClearTouches(0)
        bd.AcceptMove(0)
        assert rc == 0
        assert after[1] - before[1] == 1, (before, after)    # the list was a root-ward path ...
        assert after[3] == before[3], (before, after)        # ... and did not run fused with a log-likelihood
        assert abs(lnl - want) <= 1e-10 * abs(want), (lnl, want)
        assert np.isfinite(d1) and np.isfinite(d2)
        t.length[b2] = t.length[b2] * 0.6
        bd.TouchBranch(0, b2); twin.TouchBranch(0, b2)
        assert bd.LogLike(0) == twin.LogLike(0)
        assert np.array_equal(bd.inst.get_site_log_likelihoods(), twin.inst.get_site_log_likelihoods())
    finally:
        bd.finalize()
        twin.finalize()


def test_derivatives_after_a_held_path_on_emulation(emu):
    check_held_path(emu)


@pytest.mark.gpu
def test_derivatives_after_a_held_path(gpu):
    check_held_path(gpu)
