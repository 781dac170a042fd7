"""An independent reference for the engine tests: Felsenstein pruning in numpy float64 from a `Division` alone (no engine code),
with the quantities the tests' error bounds are made of.  Used by test_derivatives.py and engine_checks.py."""
import functools

import numpy as np

from mrbayes_amd import likelihood as lk
from mrbayes_amd.division import synthetic_division

NTAXA = 8
U32 = 2.0 ** -24
U64 = 2.0 ** -53


# ---- cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_division(states, ncat, npat, seed=11, tree_seed=5):
    kind = {4: "gtr", 20: "wag"}.get(states, "gen%d" % states)
    div = synthetic_division(kind, NTAXA, npat, seed=seed, tree_seed=tree_seed, alpha=0.7, ncat=ncat, p_gap=0.05)
    div.weights = 1.0 + (np.arange(npat) % 3).astype(np.float64)         # pattern weights that are not all one
    return div


def branch_length(t, node):
    return min(max(t.length[node], lk.BRLENS_MIN), lk.BRLENS_MAX)


def spectral(div, t, order):
    """(matrices [K][S][S], sums of the absolute spectral terms [K][S][S]) of d^order P / dt^order at branch length t"""
    es = div.eigen[0]
    U, Ui, lam = np.asarray(es.evec, dtype=np.float64), np.asarray(es.ivec, dtype=np.float64), np.asarray(es.eval, dtype=np.float64)
    mats, mags = [], []
    for r in div.cat_rates:
        e = (lam * r) ** order * np.exp(lam * r * t)
        terms = U[:, :, None] * e[None, :, None] * Ui[None, :, :]       # [i][s][j]
        mats.append(terms.sum(axis=1))
        mags.append(np.abs(terms).sum(axis=1))
    return np.stack(mats), np.stack(mags)


def kappa(div, t):
    """the cancellation inside the spectral sum: max over entries above 1e-6 of the largest of sum_s |terms| / |entry|"""
    worst = 1.0
    for order in (0, 1, 2):
        m, mag = spectral(div, t, order)
        for k in range(m.shape[0]):
            keep = np.abs(m[k]) > 1e-6 * np.abs(m[k]).max()
            worst = max(worst, float((mag[k][keep] / np.abs(m[k][keep])).max()))
    return worst


@functools.lru_cache(maxsize=None)
def reference(states, ncat, npat, seed=11, tree_seed=5, interior=False):
    """Pruning in float64 -> per-site L, D1, D2, A1, A2 over the root branch, whose child end is the root tip (interior: over
    the branch below the top interior node instead, see interior_edge: both ends are interior partials)."""
    div = make_division(states, ncat, npat, seed, tree_seed)
    t, S, K, P = div.tree, div.nstates, div.ncat, div.npatterns
    cl = {}
    for tip in range(t.ntaxa):
        st = np.asarray(div.tip_states[tip])
        one = np.zeros((P, S))
        ok = st < S
        one[np.arange(P)[ok], st[ok]] = 1.0
        one[~ok] = 1.0
        cl[tip] = np.broadcast_to(one, (K, P, S))
    for p in t.int_down_pass:
        out = np.ones((K, P, S))
        for c in (t.left[p], t.right[p]):
            m, _ = spectral(div, branch_length(t, c), 0)
            out = out * np.einsum("kij,kcj->kci", m, cl[c])
        cl[p] = out
    parent, child, tl = cl[t.root_left], cl[t.root], branch_length(t, t.root_left)
    if interior:
        v, u = interior_edge(t)
        parent = np.einsum("kij,kcj->kci", spectral(div, branch_length(t, u), 0)[0], cl[u]) * np.einsum("kij,kcj->kci", spectral(div, tl, 0)[0], cl[t.root])
        child, tl = cl[v], branch_length(t, v)
    w = div.category_weights(0)
    pi = np.asarray(div.pi, dtype=np.float64)
    res = {"t": tl}
    for order, name in ((0, "L"), (1, "D1"), (2, "D2")):
        m, _ = spectral(div, tl, order)
        res[name] = np.einsum("k,i,kci,kij,kcj->c", w, pi, parent, m, child)
        res["A" + name] = np.einsum("k,i,kci,kij,kcj->c", w, pi, parent, np.abs(m), child)
    L = res["L"]
    res["d1"] = res["D1"] / L
    res["d2"] = res["D2"] / L - res["d1"] ** 2
    res["scale1"] = (res["AD1"] + np.abs(res["D1"])) / L
    res["scale2"] = (res["AD2"] + np.abs(res["D2"])) / L + 2.0 * np.abs(res["d1"]) * res["scale1"]
    return res


def interior_edge(t):
    """(v, u): an interior child v of the top interior node and its sibling u.  The branch above v has interior partials at both
    ends once the top node's other two neighbours -- u and the root tip -- are combined into a buffer of their own."""
    l, r = t.left[t.root_left], t.right[t.root_left]
    return (l, r) if l >= t.ntaxa else (r, l)
