"""The numpy float64 reference of the insertion log-likelihoods (mbamdCalculateInsertionLogLikelihoods; csrc/mbamd_insertions.h,
DESIGN 4.4.12) and its a-priori bound.  No engine code and no tests (tests/test_insertions.py holds those).

From the `Division` alone: post-order pruning and the un-normalised pre-order recursion of tests/preorder_reference.py, the
posterior category probabilities q_k(c) = w_k L_k(c) / sum_k' w_k' L_k'(c) with L_k(c) = sum_l pre_top[k,c,l] post_top[k,c,l],
and then the call's formula.  A candidate (`Candidate`) is a point on the branch above `node`, a fraction `split` of the branch
length above the node (0: the child end), a subtree column `sub` [K][P][S] and a pendant matrix `pendant` [K][S][S]:
    a      = pre(node)                                        (child end)
             the pre-order operation of the node with the UPPER part of its branch as its own matrix (elsewhere)
    b[m]   = post(node)[m]        or        sum_j P(lower part)[m,j] post(node)[j]
    s[m]   = sum_j pendant[m,j] sub[j]
    R_c    = sum_k q_k(c) (sum_m a b s) / (sum_m a b),        log R_c + shift ln 2
`shift`: the subtree's columns are sub 2^shift (a subtree far below the range of float64 products is given by its mantissas).
enlarged_site_likelihoods prunes the tree WITH the subtree hung there from scratch: what log R_c must be the difference of.

The bound, derived and not tuned.  Every term of R_c is non-negative, so the error of R_c is relative and that of log R_c
absolute.  With h as in tests/test_preorder_gradient.py (the operations on the longest post-order chain plus those on the longest
pre-order chain) every component of a post-order or pre-order buffer of the tree carries at most e = (S + 8) (1 + 2 h) u (an
operation: two S-term inner products, a product, an exact rescaling; chains add; tests/test_cross_products.py).  An S-term
inner product with a matrix stored in the engine's precision adds (S + 8) u whatever the order of its additions -- the matrix
core's fp32 partial sums, two states per instruction, are such an order, so the matrix-core kernel is covered by the same count.
  * a: e; off the child end one more pre-order operation, 2 (S + 8) u;
  * b: e, and (S + 8) u for the product with the lower part of the branch;
  * s: the subtree is a post-order buffer of the tree (its chain is no longer than the tree's: e) or partials set from float64
    values the engine's precision holds exactly (nothing), then the pendant product, (S + 8) u; its power of two is exact;
  * num_k / den_k: the terms a_m b_m of numerator and denominator are perturbed by at most e_a + e_b each, the ratio by twice
    that; s enters the numerator only: 2 (e_a + e_b) + e_s;
  * q, a ratio of sums of products of two components taken at another branch: 2 e;
  * the products a b and (a b) s, the conversion of q, the division, the double-precision sums over states and categories
    (S K 2^-53) and the logarithm: 16 u covers them.
    |log R_c - ref| <= B = (7 (S + 8) (1 + 2 h) + 7 (S + 8) + 16) u
and the weighted sums get sum_c weight_c B.  u = 2^-24 on the single-precision engine, 2^-53 kappa on the double-precision
engine (unit_roundoff of tests/preorder_reference.py).  lnl_bound is the same count for a root log-likelihood of a tree two
operations deeper (the enlarged tree of test 5): every site likelihood a sum of products of components, (S + 8) (1 + 2 (h + 2)) u.
"""
import collections
import functools

import numpy as np

from tests.preorder_reference import division, post_order, pre_operation, pre_order, tip_vector
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA, branch_length, spectral

LN2 = float(np.log(2.0))

Candidate = collections.namedtuple("Candidate", "node split sub pendant shift", defaults=(0,))


def transition(div, t):
    """P_k(t) [K][S][S]; t == 0: the identity"""
    if t == 0.0:
        return np.broadcast_to(np.eye(div.nstates), (div.ncat, div.nstates, div.nstates)).copy()
    return spectral(div, t, 0)[0]


@functools.lru_cache(maxsize=None)
def tree_state(states, ncat, npat, ntaxa=NTAXA):
    """what every candidate of a division shares: lengths, post, mats, pre, q, the site likelihoods L and h"""
    div = division(states, ncat, npat, ntaxa)
    t = div.tree
    lengths = {n: branch_length(t, n) for n in t.all_down_pass}
    post, mats = post_order(div, lengths)
    pre = pre_order(div, post, mats)
    w = div.category_weights(0)
    top = t.root_left
    Lk = w[:, None] * np.einsum("kcl,kcl->kc", pre[top], post[top])
    L = Lk.sum(0)
    return dict(div=div, lengths=lengths, post=post, mats=mats, pre=pre, q=Lk / L[None, :], L=L, h=gradient_reference(states, ncat, npat, ntaxa)["h"])


def point_vectors(st, node, split):
    """(a, b) [K][P][S] at the point `split` of the way up the branch above `node`"""
    div = st["div"]
    t = div.tree
    post, pre, mats = st["post"], st["pre"], st["mats"]
    if split == 0.0:
        return pre[node], post[node]
    tl = st["lengths"][node]
    lower, upper = transition(div, split * tl), transition(div, (1.0 - split) * tl)
    if node == t.root_left:
        pi = np.asarray(div.pi, dtype=np.float64)
        a = np.einsum("kij,ci->kcj", upper, pi[None, :] * tip_vector(div, t.root))
    else:
        p = t.anc[node]
        sib = t.right[p] if t.left[p] == node else t.left[p]
        a = pre_operation(pre[p], upper, post[sib], mats[sib])
    return a, np.einsum("kij,kcj->kci", lower, post[node])


def log_ratios(st, cand):
    """log R_c [P] of a candidate, from the formula"""
    a, b = point_vectors(st, cand.node, cand.split)
    s = np.einsum("kij,kcj->kci", cand.pendant, cand.sub)
    den = np.einsum("kcm,kcm->kc", a, b)
    num = np.einsum("kcm,kcm,kcm->kc", a, b, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where(den > 0, st["q"] * num / den, 0.0).sum(0)
        return np.log(R) + cand.shift * LN2


def enlarged_site_likelihoods(div, lengths, cand=None):
    """L_c [P] of the tree by pruning from scratch, rooted at the root tip; `cand`: with its subtree hung on its branch"""
    t, K = div.tree, div.ncat
    w, pi = div.category_weights(0), np.asarray(div.pi, dtype=np.float64)

    def column(n):
        if t.left[n] < 0:
            return np.broadcast_to(tip_vector(div, n), (K, div.npatterns, div.nstates))
        return message(t.left[n]) * message(t.right[n])

    def message(n):
        """what the branch above n brings to its upper end"""
        if cand is not None and cand.node == n:
            x = np.einsum("kij,kcj->kci", transition(div, cand.split * lengths[n]), column(n)) * np.einsum("kij,kcj->kci", cand.pendant, cand.sub)
            return np.einsum("kij,kcj->kci", transition(div, (1.0 - cand.split) * lengths[n]), x)
        return np.einsum("kij,kcj->kci", transition(div, lengths[n]), column(n))

    return np.einsum("k,i,ci,kci->c", w, pi, tip_vector(div, t.root), message(t.root_left))


def bound(div, h, u):
    """B: of log R_c of every candidate"""
    S = div.nstates
    return (7 * (S + 8) * (1 + 2 * h) + 7 * (S + 8) + 16) * u


def lnl_bound(div, h, u):
    """of a root log-likelihood of the tree, or of the tree with one subtree of the same depth hung on it"""
    return (div.nstates + 8) * (1 + 2 * (h + 2)) * u * float(div.weights.sum())
