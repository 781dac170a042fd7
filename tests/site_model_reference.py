"""The numpy float64 reference of the gradient in the site model (mbamdCalculateSiteModelDerivatives), built from
tests/preorder_reference.py: post-order pruning, the un-normalised pre-order recursion, q of the log-likelihood call over the root
branch, and per edge e (node n), category k and pattern c
    N_k, A_k, den_k = edge_terms(pre_n, post_n, D)            (A: the same sum with |D|)
    G_ref[e,k] = sum_c weight_c q_k(c) N_k(c) / den_k(c),     A_ref[e,k] the same with A_k
    R_ref[k]   = sum_e t_e G_ref[e,k]
    C_ref[k]   = sum_c weight_c q_k(c)
    F_ref[i]   = sum_c weight_c sum_k q_k(c) parent[k,c,i] f_k(c,i) / sum_l pi_l parent[k,c,l] f_k(c,l)
with parent = the top interior node's post-order partials and f_k = P_top,k tip_root.  D_k = Q (`unit`, the form whose R_ref is
d lnL / d r_k) or D_k = r_k Q (the branch-length gradient's matrix).  No engine code and no tests.
"""
import functools

import numpy as np

from tests.preorder_reference import bound_factor, division, edge_terms, lnl_posteriors, post_order, pre_order, rate_matrix
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA


def site_model_terms(div, lengths, nodes, D):
    """G [edges][K], A [edges][K], C [K], F [S] of the division at the branch lengths `lengths` with the differential matrices D [K][S][S]"""
    t = div.tree
    post, mats = post_order(div, lengths)
    pre = pre_order(div, post, mats)
    w, pi = div.category_weights(0), np.asarray(div.pi, dtype=np.float64)
    top = t.root_left
    q, _ = lnl_posteriors(w, pi, post[top], mats[top], post[t.root])
    G, A = np.zeros((len(nodes), div.ncat)), np.zeros((len(nodes), div.ncat))
    for e, n in enumerate(nodes):
        N, Aabs, den = edge_terms(pre[n], post[n], D)
        G[e] = (div.weights[None, :] * q * N / den).sum(axis=1)
        A[e] = (div.weights[None, :] * q * Aabs / den).sum(axis=1)
    C = (div.weights[None, :] * q).sum(axis=1)
    term = post[top] * np.einsum("kij,kcj->kci", mats[top], post[t.root])            # parent[k,c,i] f_k(c,i)
    F = np.einsum("c,kc,kci->i", div.weights, q / np.einsum("i,kci->kc", pi, term), term)
    return G, A, C, F


@functools.lru_cache(maxsize=None)
def reference(states, ncat, npat, ntaxa=NTAXA, unit=True):
    """G_ref, A_ref [edges][K], R_ref [K], C_ref [K], F_ref [S]; nodes, lengths and h as tests/preorder_reference.reference"""
    div = division(states, ncat, npat, ntaxa)
    g = gradient_reference(states, ncat, npat, ntaxa)
    nodes, lengths = list(g["nodes"]), g["lengths"]
    Q = rate_matrix(div)
    r = np.ones(div.ncat) if unit else np.asarray(div.cat_rates, dtype=np.float64)
    G, A, C, F = site_model_terms(div, lengths, nodes, r[:, None, None] * Q[None, :, :])
    t = np.array([lengths[n] for n in nodes])
    return dict(nodes=nodes, lengths=lengths, t=t, h=g["h"], G=G, A=A, R=t @ G, RA=t @ A, C=C, F=F)


def site_factor(div, ref, u):
    """the relative bound of every output on its sum of absolute terms (derived in tests/test_site_model_gradient.py): bound_factor's
    4 (S + 8) (1 + 2 h) + 8, with the S roundings of the FMA chain over D's row in the place of the 64 K products of the matrix core"""
    return bound_factor(div, ref, u) - (64 * div.ncat - div.nstates) * u
