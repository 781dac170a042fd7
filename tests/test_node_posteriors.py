"""Node-state and category posteriors from the pre-order buffers (mbamdCalculateNodePosteriors, mbamdGetCategoryPosteriors;
csrc/mbamd_posteriors.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference is numpy float64 from the `Division` alone, that of tests/test_preorder_gradient.py (post-order pruning) and
tests/test_edge_second_derivatives.py (the pre-order recursion, un-normalised).  Per node n, with w the category weights and
j = pre[n] * post[n] [K][P][S]:
    den = j.sum(2),     q = w den / (w den).sum(0),     p = (q j / den).sum(0)
q [K][P] is the same at every node (it is taken at the top interior node).

Tolerance, derived and not tuned, on the premises of the module docstring of tests/test_preorder_gradient.py: every component of
either buffer is a sum of non-negative terms carrying at most (S + 8) 2 h' u relative error over its chain of h' operations, so j,
den, the ratio j / den and q (itself such a ratio) carry at most f = (S + 8) (1 + 2 h) u each, to first order:
    |p - p_ref| <= b = 4 f p_ref        per component,        |q - q_ref| <= 2 f q_ref
the sums get sum_c weight_c b_c(a).  u = 2^-24 on the single-precision engine; u = 2^-53 kappa on the double-precision engine
(unit_roundoff of tests/preorder_reference.py).  Where p_ref is exactly 0 (a state a compact tip excludes) the engine's value
must be exactly 0.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.preorder_reference import CASES, CASES_F64, division, post_order, pre_order, unit_roundoff
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA
from tests.test_derivatives import expected_layout

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
SENTINEL = -7.5


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
    """the gradient's reference (nodes, lengths, h, L), and p [P][S] per node n; q [K][P]"""
    div = division(states, ncat, npat, ntaxa)
    g = gradient_reference(states, ncat, npat, ntaxa)
    post, mats = post_order(div, g["lengths"])
    pre = pre_order(div, post, mats)
    w = div.category_weights(0)
    res = {"nodes": list(g["nodes"]), "lengths": g["lengths"], "h": g["h"], "g": g}
    for n in res["nodes"]:
        j = pre[n] * post[n]
        den = j.sum(2)
        q = w[:, None] * den / (w[:, None] * den).sum(0)
        p = (q[:, :, None] * j / den[:, :, None]).sum(0)
        # the reference itself: the category sum is the gradient reference's L, and the posteriors of a pattern add up to one
        assert np.all(np.abs((w[:, None] * den).sum(0) - g[n]["L"]) <= 1e-10 * g[n]["L"])
        assert float(np.abs(p.sum(1) - 1.0).max()) <= 1e-14
        res[n] = p
        if n == div.tree.root_left:
            res["q"] = q
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def rel_error(div, ref, u):
    """f of the module docstring"""
    return (div.nstates + 8) * (1 + 2 * ref["h"]) * u


def node_indices(bd):
    nodes = list(bd.div.tree.all_down_pass)
    return dict(posts=[bd.condLikeIndex[0][n] for n in nodes], pres=[bd.preOrderIndex[n] for n in nodes], weights=[bd.cijkIndex[0]] * len(nodes))


def new_division(lib, div, double_precision=False, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    return lk.BeagleDivision(div, lib, scaling=scaling, double_precision=double_precision, pre_order=True)


def observed(div, n):
    """patterns at which tip n shows a state / misses one; (None, None) for an interior node"""
    if n >= div.tree.ntaxa:
        return None, None
    st = np.asarray(div.tip_states[n])
    return st < div.nstates, st >= div.nstates


def worst_ratio(got, want, bound):
    """max |got - want| / bound where want > 0; where want is exactly 0, got must be"""
    zero = want == 0.0
    assert np.all(got[zero] == 0.0)
    return float((np.abs(got - want)[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


# ---- 1. values, 2. best states, 3. tips -------------------------------------------------------------------------------------------
def check_case(lib, states, ncat, npat, double_precision=False, ntaxa=NTAXA, scaling=lk.MB_BEAGLE_SCALE_ALWAYS):
    div = division(states, ncat, npat, ntaxa)
    ref = reference(states, ncat, npat, ntaxa)
    t, S, w = div.tree, div.nstates, div.weights
    f = rel_error(div, ref, unit_roundoff(div, ref["g"], double_precision))
    nodes = ref["nodes"]
    bd = new_division(lib, div, double_precision, scaling)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(states, ncat, double_precision) in name, name
        if ncat > 1:
            bd.LogLike(0)
            bd.AcceptMove(0)
        else:
            # one category: q = 1, nothing is asked of a log-likelihood call -- the buffers are computed, no likelihood is
            bd.UpDateCijk(0)
            bd.TreeTiProbs_Beagle(0)
            bd.TreeCondLikes_Beagle_Always_Rescale(0)
            bd.ClearTouches(0)
            bd.AcceptMove(0)
        sums_only = bd.NodePosteriors(0)
        wrapped = bd.NodePosteriors(0, sites=True, best=True)
        ix = node_indices(bd)
        rc, per, states_, values, sums = inst.calculate_node_posteriors(sites=True, best=True, **ix)
        assert rc == 0 and per.shape == (len(nodes), npat, S) and states_.shape == values.shape == (len(nodes), npat) and sums.shape == (len(nodes), S)
        rc, none, none_s, none_v, sums0 = inst.calculate_node_posteriors(sites=False, best=False, **ix)
        assert rc == 0 and none is None and none_s is None and none_v is None
        rc, _, only_s, only_v, sums1 = inst.calculate_node_posteriors(sites=False, best=True, **ix)
        # the sums do not depend on the per-pattern outputs asked for; best states without the per-site values are the same
        assert np.array_equal(sums, sums0) and np.array_equal(sums, sums1)
        assert np.array_equal(only_s, states_) and np.array_equal(only_v, values)
        assert sorted(sums_only) == sorted(nodes) and len(nodes) == 2 * t.ntaxa - 3
        worst = dict(sites=0.0, sums=0.0, total=0.0, best=0.0, missing=0.0)
        left_out = pairs = 0
        tips_seen = missing_seen = 0
        for i, n in enumerate(nodes):
            p = ref[n]
            b = 4.0 * f * p
            # NodePosteriors is the raw call
            assert np.array_equal(sums_only[n], sums[i]) and np.array_equal(wrapped[0][n], sums[i]) and np.array_equal(wrapped[1][n], per[i])
            assert np.array_equal(wrapped[2][n][0], states_[i]) and np.array_equal(wrapped[2][n][1], values[i])
            # 1. values
            worst["sites"] = max(worst["sites"], worst_ratio(per[i], p, b))
            worst["sums"] = max(worst["sums"], worst_ratio(sums[i], (w[:, None] * p).sum(0), (w[:, None] * b).sum(0)))
            worst["total"] = max(worst["total"], float((np.abs(per[i].sum(1) - 1.0) / b.sum(1)).max()))
            order = np.sort(p, axis=1)
            first, second = order[:, -1], order[:, -2]
            worst["best"] = max(worst["best"], float((np.abs(values[i] - first) / (4.0 * f * first)).max()))
            # 2. best states: where the reference separates the two best states by more than twice their bounds
            clear = first - second > 2.0 * 4.0 * f * (first + second)
            want = np.argmax(p, axis=1)
            assert np.array_equal(states_[i][clear], want[clear]), (n, np.flatnonzero(clear & (states_[i] != want)))
            pairs += npat
            left_out += int((~clear).sum())
            agree = states_[i] == want
            assert np.array_equal(values[i][agree], per[i][np.arange(npat)[agree], want[agree]])
            # (the best state is the FIRST that attains the maximum of the engine's own values)
            assert np.array_equal(states_[i], np.argmax(per[i], axis=1)) and np.array_equal(values[i], per[i].max(1))
            # 3. tips
            seen, missing = observed(div, n)
            if seen is not None:
                st = np.asarray(div.tip_states[n])
                indicator = np.zeros((npat, S))
                indicator[np.arange(npat)[seen], st[seen]] = 1.0
                assert np.array_equal(per[i][seen], indicator[seen])
                tips_seen += int(seen.sum())
                if missing.any():
                    worst["missing"] = max(worst["missing"], worst_ratio(per[i][missing], p[missing], b[missing]))
                    missing_seen += int(missing.sum())
        share = left_out / pairs
        print("%d states x %d x %d, %d taxa%s: error / bound over %d nodes: sites %.3f, sums %.3f, sum over states %.3f, best %.3f, "
              "missing tips %.3f; best states not compared %.2e of %d" %
              (states, ncat, npat, t.ntaxa, " fp64" if double_precision else "", len(nodes), worst["sites"], worst["sums"], worst["total"],
               worst["best"], worst["missing"], share, pairs))
        assert tips_seen > 0 and missing_seen > 0
        assert max(worst.values()) <= 1.0, worst
        assert share <= 0.01, share
        return worst
    finally:
        bd.finalize()


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_posteriors_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_posteriors_double_precision_on_emulation(emu, states, ncat, npat):
    check_case(emu, states, ncat, npat, double_precision=True)


def test_posteriors_deep_tree_on_emulation(emu):
    """60 taxa: un-normalised pre-order columns down to ~1e-107 in the float64 reference -- passes only if the scale cancels"""
    assert gradient_reference(4, 4, 70, 60)["min_column"] < 1e-45
    check_case(emu, 4, 4, 70, ntaxa=60)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_posteriors(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_posteriors_double_precision(gpu, states, ncat, npat):
    check_case(gpu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
def test_posteriors_deep_tree(gpu):
    check_case(gpu, 4, 4, 70, ntaxa=60)


# ---- 4. category posteriors -------------------------------------------------------------------------------------------------------
def check_category_posteriors(lib, states, ncat, npat, double_precision=False):
    div, ref = division(states, ncat, npat), reference(states, ncat, npat)
    f = rel_error(div, ref, unit_roundoff(div, ref["g"], double_precision))
    bd = new_division(lib, div, double_precision)
    try:
        if ncat == 1:
            # (no log-likelihood call: nothing is asked of one)
            q = bd.CategoryPosteriors(0)
            assert q.shape == (1, npat) and np.all(q == 1.0)
            return
        bd.LogLike(0)
        bd.AcceptMove(0)
        q = bd.CategoryPosteriors(0)
        assert q.shape == (ncat, npat) and np.array_equal(q, bd.inst.get_category_posteriors(bd.cijkIndex[0]))
        qr = ref["q"]
        r = np.asarray(div.cat_rates, dtype=np.float64)
        rate, rate_ref = (q * r[:, None]).sum(0), (qr * r[:, None]).sum(0)
        worst = (float((np.abs(q - qr) / (2.0 * f * qr)).max()), float((np.abs(q.sum(0) - 1.0) / (2.0 * f)).max()),
                 float((np.abs(rate - rate_ref) / (2.0 * f * rate_ref)).max()))
        print("%d states x %d x %d%s: category posteriors, error / bound: q %.3f, rows %.3f, site rates %.3f" %
              (states, ncat, npat, " fp64" if double_precision else "", worst[0], worst[1], worst[2]))
        assert max(worst) <= 1.0, worst
        # the same after the gradient call has computed them, and after a second evaluation
        bd.BranchGradient(0)
        assert np.array_equal(q, bd.CategoryPosteriors(0))
        bd.TouchAllTreeNodes(0)
        bd.LogLike(0)
        bd.AcceptMove(0)
        assert np.array_equal(q, bd.CategoryPosteriors(0))
    finally:
        bd.finalize()


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_category_posteriors_on_emulation(emu, states, ncat, npat):
    check_category_posteriors(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_category_posteriors_double_precision_on_emulation(emu, states, ncat, npat):
    check_category_posteriors(emu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_category_posteriors(gpu, states, ncat, npat):
    check_category_posteriors(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_category_posteriors_double_precision(gpu, states, ncat, npat):
    check_category_posteriors(gpu, states, ncat, npat, double_precision=True)


# ---- 5. chunks, 6. shards -----------------------------------------------------------------------------------------------------------
def _posterior_call(lib, div):
    """(children, launches of the call, posteriors, best states, best posteriors, sums) on a fresh instance"""
    bd = new_division(lib, div)
    try:
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.NodePosteriors(0)
        bd.inst.get_kernel_timing(reset=True)
        rc, per, states, values, sums = bd.inst.calculate_node_posteriors(sites=True, best=True, **node_indices(bd))
        _, launches = bd.inst.get_kernel_timing(reset=True)
        assert rc == 0
        return bd.inst.child_count(), launches, per, states, values, sums
    finally:
        bd.finalize()


CHUNK_CASES = [(4, 4, 130), (20, 4, 70)]


def check_chunked(lib, monkeypatch, states, ncat, npat):
    """MBAMD_POSTERIOR_NODES=5: the 13 nodes in three launches (and three of k_gradient_sums), every output bit for bit the same"""
    div = division(states, ncat, npat)
    monkeypatch.delenv("MBAMD_POSTERIOR_NODES", raising=False)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    _, launches1, per1, states1, values1, sums1 = _posterior_call(lib, div)
    monkeypatch.setenv("MBAMD_POSTERIOR_NODES", "5")
    try:
        _, launches3, per3, states3, values3, sums3 = _posterior_call(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_POSTERIOR_NODES")
    assert len(div.tree.all_down_pass) == 13 and launches1 == 2 and launches3 == 6, (launches1, launches3)
    assert np.array_equal(per1, per3) and np.array_equal(states1, states3) and np.array_equal(values1, values3) and np.array_equal(sums1, sums3)


@pytest.mark.parametrize("states,ncat,npat", CHUNK_CASES)
def test_chunked_posteriors_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_chunked(emu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CHUNK_CASES)
def test_chunked_posteriors(gpu, monkeypatch, states, ncat, npat):
    check_chunked(gpu, monkeypatch, states, ncat, npat)


def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 at 4 states x 4 categories x 130 patterns: the children's sums added, their per-pattern values concatenated"""
    div, ref = division(4, 4, 130), reference(4, 4, 130)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    monkeypatch.delenv("MBAMD_POSTERIOR_NODES", raising=False)
    n1, _, per1, states1, values1, sums1 = _posterior_call(lib, div)
    monkeypatch.setenv("MBAMD_SHARD", "2")
    try:
        n2, _, per2, states2, values2, sums2 = _posterior_call(lib, div)
        bd = new_division(lib, div)
        try:
            bd.LogLike(0)
            q2 = bd.CategoryPosteriors(0)
        finally:
            bd.finalize()
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n1 == 1 and n2 == 2
    f, w = rel_error(div, ref, 2.0 ** -24), div.weights
    assert np.all(np.abs(q2 - ref["q"]) <= 2.0 * f * ref["q"])
    for i, n in enumerate(ref["nodes"]):
        p = ref[n]
        b = 4.0 * f * p
        assert np.all(np.abs(per2[i] - per1[i]) <= b) and np.all(np.abs(per2[i] - p) <= b)
        first = p.max(1)
        assert np.all(np.abs(values2[i] - values1[i]) <= 4.0 * f * first) and np.all(np.abs(values2[i] - first) <= 4.0 * f * first)
        assert np.array_equal(states2[i], np.argmax(per2[i], axis=1))
        bs = (w[:, None] * b).sum(0)
        assert np.all(np.abs(sums2[i] - sums1[i]) <= bs) and np.all(np.abs(sums2[i] - (w[:, None] * p).sum(0)) <= bs)


def test_sharded_posteriors_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_posteriors(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, double_precision=False):
    """Every bad call is refused with the expected status and writes nothing to its outputs; returns (status, message) of each, in
    order: the two engines run one body (mbamd_posteriors.h), so they answer alike -- check_engines_agree."""
    seen = []
    div = division(4, 2, 130)
    t, P, S, K = div.tree, 130, 4, 2
    bd = new_division(lib, div, double_precision)
    try:
        inst = bd.inst

        def outputs(n):
            n = max(n, 1)
            return [np.full(n * P * S, SENTINEL), np.full(n * P, int(SENTINEL), dtype=np.int32), np.full(n * P, SENTINEL), np.full(n * S, SENTINEL)]

        def untouched(outs):
            return all(np.all(o == (int(SENTINEL) if o.dtype == np.int32 else SENTINEL)) for o in outs)

        def call(arrays, n, outs):
            return inst.lib.mbamdCalculateNodePosteriors(inst.id, *[None if a is None else a.ctypes.data_as(_ip) for a in arrays], n,
                                                         None if outs[0] is None else outs[0].ctypes.data_as(_dp),
                                                         None if outs[1] is None else outs[1].ctypes.data_as(_ip),
                                                         None if outs[2] is None else outs[2].ctypes.data_as(_dp),
                                                         None if outs[3] is None else outs[3].ctypes.data_as(_dp))

        def raises(code, ix):
            """the call through the C ABI with sentinel-filled outputs"""
            arrays = [np.asarray(ix[k], dtype=np.int32) for k in ("posts", "pres", "weights")]
            outs = outputs(len(arrays[0]))
            rc = call(arrays, len(arrays[0]), outs)
            assert rc == code, (rc, code, lib.last_error())
            assert lib.last_error() and untouched(outs)
            seen.append((rc, lib.last_error()))

        def raises_q(code, index, out=True):
            q = np.full(K * P, SENTINEL)
            rc = inst.lib.mbamdGetCategoryPosteriors(inst.id, index, q.ctypes.data_as(_dp) if out else None)
            assert rc == code, (rc, code, lib.last_error())
            assert lib.last_error() and np.all(q == SENTINEL)
            seen.append((rc, lib.last_error()))

        # more than one category and no log-likelihood call yet
        raises(bg.BEAGLE_ERROR_GENERAL, node_indices(bd))
        raises_q(bg.BEAGLE_ERROR_GENERAL, bd.cijkIndex[0])
        bd.LogLike(0)
        bd.AcceptMove(0)
        bd.NodePosteriors(0)
        ix = node_indices(bd)                                                           # (the evaluation flipped index tables)
        n = len(ix["posts"])
        # a weights index different from the remembered one
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, weights=[bd.cijkScratchIndex] * n))
        raises_q(bg.BEAGLE_ERROR_OUT_OF_RANGE, bd.cijkScratchIndex)
        raises_q(bg.BEAGLE_ERROR_OUT_OF_RANGE, bd.cijkIndex[0], out=False)
        # a pre index that no pre-order operation wrote; one that beagleUpdatePartials has overwritten since
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, pres=[bd.preOrderStartIndex] * n))
        victim = bd.preOrderIndex[t.root_left]
        inst.update_partials(np.array([[victim, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, bd.condLikeIndex[0][0], bd.tiProbsIndex[0][0],
                                        bd.condLikeIndex[0][1], bd.tiProbsIndex[0][1]]], dtype=np.int32), bg.BEAGLE_OP_NONE)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, ix)
        inst.update_pre_partials(bd.PreOrderOperations(0))                              # (all of them pre-order buffers again)
        assert inst.calculate_node_posteriors(sites=False, **ix)[0] == 0
        # a post-order buffer nothing has written (the other half of an interior node's pair); indices out of range
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, posts=[bd.condLikeScratchIndex[t.root_left]] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, posts=[10 ** 6] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, posts=[-1] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, pres=[10 ** 6] * n))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, pres=[-1] * n))
        # NULL index arrays; a negative count; no room for the sums
        good = [np.asarray(ix[k], dtype=np.int32) for k in ("posts", "pres", "weights")]
        for missing in range(3):
            outs = outputs(n)
            rc = call([None if j == missing else a for j, a in enumerate(good)], n, outs)
            assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE and untouched(outs)
            seen.append((rc, lib.last_error()))
        outs = outputs(n)
        rc = call(good, -1, outs)
        assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE and untouched(outs)
        seen.append((rc, lib.last_error()))
        rc = call(good, n, outs[:3] + [None])
        assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE and untouched(outs)
        seen.append((rc, lib.last_error()))
        # no nodes: success, nothing written (NULL arrays allowed)
        rc = call([None, None, None], 0, outs)
        assert rc == 0 and untouched(outs)
        # only the best states and the sums
        rc = call(good, n, [None, outs[1], None, outs[3]])
        full = inst.calculate_node_posteriors(sites=True, best=True, **ix)
        assert rc == 0 and np.array_equal(outs[1].reshape(n, P), full[2]) and np.array_equal(outs[3].reshape(n, S), full[4])
        assert np.all(outs[0] == SENTINEL) and np.all(outs[2] == SENTINEL)
        # the latest log-likelihood call had several subsets
        top = t.root_left
        two = lambda v: [v, v]
        inst.calculate_edge_log_likelihoods(two(bd.condLikeIndex[0][top]), two(bd.condLikeIndex[0][t.root]), two(bd.tiProbsIndex[0][top]),
                                            two(bd.cijkIndex[0]), two(bd.cijkIndex[0]), two(bd.siteScalerIndex[0]))
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, ix)
        raises_q(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, bd.cijkIndex[0])
    finally:
        bd.finalize()
    # a multi-partition instance serves neither call
    N = NTAXA
    flags = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
    inst = bg.BeagleInstance(lib, N, 3 * N, N, S, P, 2, 4 * N, K, N, preference_flags=flags)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.asarray(div.tip_states[tip]).astype(np.int32))
        inst.set_pattern_weights(div.weights)
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
        assert inst.child_count() == 2
        for refused in (lambda: inst.calculate_node_posteriors([0], [N + 1], [0]), lambda: inst.get_category_posteriors(0)):
            with pytest.raises(bg.BeagleError) as err:
                refused()
            assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION
            seen.append((err.value.code, lib.last_error()))
    finally:
        inst.finalize()
    return seen


def check_engines_agree(lib):
    single, double = check_argument_errors(lib), check_argument_errors(lib, double_precision=True)
    assert len(single) == len(double) == 21
    for i, (s, d) in enumerate(zip(single, double)):
        assert s == d, (i, s, d)


def test_argument_errors_on_emulation(emu):
    check_engines_agree(emu)


@pytest.mark.gpu
def test_argument_errors(gpu):
    check_engines_agree(gpu)
