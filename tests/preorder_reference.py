"""What the tests of the calls on the pre-order buffers share (tests/test_preorder_gradient.py, test_cross_products.py,
test_edge_second_derivatives.py, test_node_posteriors.py, test_preorder_exponent_range.py, and the tree part of test_complex_eigen.py): the divisions and cases, the
numpy float64 reference of both passes and of the gradient, and its a-priori bounds.  No engine code and no tests.

The reference is numpy float64 from the `Division` alone: post-order pruning as in tests/pruning_reference.py, the pre-order
recursion un-normalised,
    pre_top[k,c,j] = sum_i P_top,k[i,j] pi_i tip_root[c,i]
    tmp[k,c,i]     = pre_parent[k,c,i] sum_j P_sib,k[i,j] post_sib[k,c,j],      pre_n[k,c,j] = sum_i P_n,k[i,j] tmp[k,c,i]
and Q = U diag(lambda) U^-1, D_k = r_k Q.  Per branch (node n) and pattern c
    N_c = sum_k w_k sum_l pre_n[k,c,l] sum_j D_k[l,j] post_n[k,c,j],   A_c the same with |D_k|,   L_c = sum_k w_k sum_l pre_n[k,c,l] post_n[k,c,l]
    d_c = N_c / L_c.
pre_operation, pre_order_given, lnl_posteriors, edge_terms and mixed are the same formulas on columns and matrices AS GIVEN -- what an
engine holds, read back -- for tests/test_preorder_exponent_range.py, which measures the readers and not the post-order pass.
The bounds (`bounds`, `unit_roundoff`, `bound_factor`) are derived in the module docstrings of tests/test_preorder_gradient.py and
tests/test_cross_products.py.
"""
import functools

import numpy as np

from mrbayes_amd.division import synthetic_division
from tests.pruning_reference import NTAXA, U32, U64, branch_length, kappa, make_division, spectral

#        states, categories, patterns                     what it reaches
CASES = [(4, 4, 130),             # two full 64-pattern blocks plus 2 patterns
         (4, 9, 70),              # a second batch of eight categories
         (20, 4, 70),             # two 32-pattern tiles plus 6 patterns
         (61, 1, 40),             # one category: no posteriors
         (12, 2, 70),             # the MFMA level layout
         (12, 6, 70),             # the generic level layout
         (3, 2, 70)]              # a small state count
CASES_F64 = [(4, 4, 130), (20, 2, 70)]


@functools.lru_cache(maxsize=None)
def division(states, ncat, npat, ntaxa=NTAXA):
    if ntaxa == NTAXA:
        return make_division(states, ncat, npat)
    kind = {4: "gtr", 20: "wag"}.get(states, "gen%d" % states)
    div = synthetic_division(kind, ntaxa, npat, seed=11, tree_seed=5, alpha=0.7, ncat=ncat, p_gap=0.05)
    div.weights = 1.0 + (np.arange(npat) % 3).astype(np.float64)
    return div


def tip_vector(div, tip):
    S, P = div.nstates, div.npatterns
    st = np.asarray(div.tip_states[tip])
    one = np.ones((P, S))
    ok = st < S
    one[ok] = 0.0
    one[np.arange(P)[ok], st[ok]] = 1.0
    return one


def post_order(div, lengths):
    """post-order partials [K][P][S] of every node, and P [K][S][S] of every branch, at the branch lengths `lengths`"""
    t, K = div.tree, div.ncat
    mats = {n: spectral(div, lengths[n], 0)[0] for n in t.all_down_pass}
    cl = {tip: np.broadcast_to(tip_vector(div, tip), (K, div.npatterns, div.nstates)) for tip in range(t.ntaxa)}
    for p in t.int_down_pass:
        out = np.ones((K, div.npatterns, div.nstates))
        for c in (t.left[p], t.right[p]):
            out = out * np.einsum("kij,kcj->kci", mats[c], cl[c])
        cl[p] = out
    return cl, mats


def pre_operation(parent, m_own, sib=None, m_sib=None):
    """one pre-order operation, un-normalised, on columns [K][P][S] and matrices [K][S][S] as given:
    tmp[k,c,i] = parent[k,c,i] sum_j m_sib[k,i,j] sib[k,c,j] (no sibling: the factor 1), out[k,c,j] = sum_i m_own[k,i,j] tmp[k,c,i]"""
    tmp = parent if sib is None else parent * np.einsum("kij,kcj->kci", m_sib, sib)
    return np.einsum("kij,kci->kcj", m_own, tmp)


def pre_order_given(t, pre_top, post, mats):
    """the recursion below the top interior node from columns and matrices AS GIVEN (a `Division`'s own float64 ones, or what an
    engine holds, read back): {node: un-normalised pre-order partials [K][P][S]}"""
    pre = {t.root_left: pre_top}
    for p in reversed(t.int_down_pass):
        for n, sib in ((t.left[p], t.right[p]), (t.right[p], t.left[p])):
            pre[n] = pre_operation(pre[p], mats[n], post[sib], mats[sib])
    return pre


def pre_order(div, post, mats):
    """un-normalised pre-order partials [K][P][S] of every node below the root tip"""
    t = div.tree
    pi = np.asarray(div.pi, dtype=np.float64)
    top = t.root_left
    return pre_order_given(t, np.einsum("kij,ci->kcj", mats[top], pi[None, :] * tip_vector(div, t.root)), post, mats)


def lnl_posteriors(w, pi, parent, matrix=None, child=None):
    """q [K][P] of a log-likelihood call on operands as given (child None: a root call), and its per-category sums
    l_k(c) = w_k sum_i pi_i parent[k,c,i] sum_j matrix[k,i,j] child[k,c,j]; a pattern without likelihood: q = 0"""
    f = parent if child is None else parent * np.einsum("kij,kcj->kci", matrix, child)
    l = w[:, None] * np.einsum("i,kci->kc", pi, f)
    L = l.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(L > 0, l / L, 0.0), l


def edge_terms(pre, post, D):
    """per category and pattern [K][P], from columns and a (differential) matrix as given:
    N = sum_l pre[l] sum_j D[l,j] post[j], A the same with |D|, den = sum_l pre[l] post[l]"""
    N = np.einsum("kcl,klj,kcj->kc", pre, D, post)
    A = np.einsum("kcl,klj,kcj->kc", pre, np.abs(D), post)
    return N, A, np.einsum("kcl,kcl->kc", pre, post)


def mixed(q, num, den):
    """sum_k q_k num_k / den_k over the categories with a denominator [P] -- the read-outs' form (include/libhmsbeagle/beagle.h): a
    category whose den is zero carries nothing.  With q_k = w_k den_k / sum w den (one tree, seen from any branch) this is
    (sum_k w_k num_k) / (sum_k w_k den_k), the N_c / L_c of the module docstring."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, q * num / den, 0.0).sum(0)


def rate_matrix(div):
    es = div.eigen[0]
    U, Ui, lam = (np.asarray(x, dtype=np.float64) for x in (es.evec, es.ivec, es.eval))
    return (U * lam[None, :]) @ Ui


def depth_of(t, n):
    """pre-order operations from the start vector down to pre(n)"""
    d = 1
    while n != t.root_left:
        n = t.anc[n]
        d += 1
    return d


@functools.lru_cache(maxsize=None)
def reference(states, ncat, npat, ntaxa=NTAXA):
    """per node n of all_down_pass: d [P], N, A, L; plus h, the smallest L and the smallest un-normalised pre-order column maximum"""
    div = division(states, ncat, npat, ntaxa)
    t = div.tree
    lengths = {n: branch_length(t, n) for n in t.all_down_pass}
    post, mats = post_order(div, lengths)
    w, pi = div.category_weights(0), np.asarray(div.pi, dtype=np.float64)
    D = np.asarray(div.cat_rates, dtype=np.float64)[:, None, None] * rate_matrix(div)[None, :, :]
    top = t.root_left
    pre = pre_order(div, post, mats)
    res = {"nodes": list(t.all_down_pass), "lengths": lengths}
    dmax = max(depth_of(t, n) for n in range(t.ntaxa) if n != t.root)
    res["h"] = (dmax - 1) + dmax
    res["min_column"] = min(float(v.max(axis=2).min()) for v in pre.values())
    for n in t.all_down_pass:
        N = np.einsum("k,kcl,klj,kcj->c", w, pre[n], D, post[n])
        A = np.einsum("k,kcl,klj,kcj->c", w, pre[n], np.abs(D), post[n])
        L = np.einsum("k,kcl,kcl->c", w, pre[n], post[n])
        res[n] = dict(d=N / L, N=N, A=A, L=L)
    res["min_L"] = min(float(res[n]["L"].min()) for n in t.all_down_pass)
    # the root branch as tests/test_derivatives.py sees it: parent = the top node, child = the root tip, P' from the eigen-system
    m1 = spectral(div, lengths[top], 1)[0]
    L0 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], mats[top], post[t.root])
    D1 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], m1, post[t.root])
    A1 = np.einsum("k,i,kci,kij,kcj->c", w, pi, post[top], np.abs(m1), post[t.root])
    res["root_scale1"] = (A1 + np.abs(D1)) / L0
    return res


def gradient_indices(bd):
    nodes = list(bd.div.tree.all_down_pass)
    return dict(posts=[bd.condLikeIndex[0][n] for n in nodes], pres=[bd.preOrderIndex[n] for n in nodes],
                dmats=[bd.diffMatrixIndex] * len(nodes), weights=[bd.cijkIndex[0]] * len(nodes))


def unit_roundoff(div, ref, double_precision):
    if not double_precision:
        return U32
    return U64 * max(kappa(div, tl) for tl in set(ref["lengths"].values()))


def bounds(div, ref, u):
    S = div.nstates
    return {n: (S + 8) * (1 + 2 * ref["h"]) * u * (ref[n]["A"] + np.abs(ref[n]["N"])) / ref[n]["L"] for n in ref["nodes"]}


def bound_factor(div, ref, u):
    """of the cross-product matrix (tests/test_cross_products.py)"""
    return (4 * (div.nstates + 8) * (1 + 2 * ref["h"]) + 64 * div.ncat + 8) * u
