"""The numpy float64 reference of mbamdSampleAncestralStates (include/libhmsbeagle/mbamd_reports.h) for
tests/test_ancestral_sampling.py.  No engine code and no tests.

It follows the header to the letter -- the same `mix`, the same streams, the same selection rule -- on what the ENGINE holds:
`get_partials` of every listed buffer, `get_transition_matrix` of every listed matrix, `get_category_posteriors`, and the
frequencies and tip states of the `Division`.  To avoid cascades every slot is judged given the engine's category and the engine's
state at its parent slot.

Margins.  Beside every draw the reference returns its margin: the distance of u from the nearest cumulative boundary
(v_0 + ... + v_j) / T.  A draw whose margin exceeds eps must match the engine's exactly; one inside eps is excused.  eps is derived:
  * an edge weight is ONE rounded product of two stored values, which the reference forms in float64 from the same two values:
    every weight, hence every partial sum and T (sums of non-negative terms), is off by at most u relative, a normalised boundary
    -- a ratio of two such sums -- by at most 2 u to first order; the engine's own double sums and x = u T add a few 2^-53.
    eps = 4 u leaves a factor two;
  * the top's weight carries the S-term FMA chain of f beside its two products: at most (S + 2) u relative per weight, a boundary
    moves by at most 2 (S + 2) u; eps = 2 (S + 4) u;
  * u = 2^-24 on the single-precision engine, 2^-53 on the double-precision one;
  * the category draw uses the engine's own doubles q_k(c), in the same order: no allowance at all (eps = 0).
"""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)


def mix(x):
    x = np.asarray(x, dtype=np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def uniform(seed, stream, c):
    """u(seed, stream, c) of the header for an array of pattern indices c"""
    with np.errstate(over="ignore"):
        head = mix(np.array([(int(seed) + 0x9E3779B97F4A7C15 * (int(stream) + 1)) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
        x = mix(head + G * (np.asarray(c, dtype=np.uint64) + np.uint64(1)))
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def pick(v, u):
    """the selection rule, row by row: v [n][m] weights, u [n] -> (index [n], -1 where the sum is not positive; margin [n])"""
    v = np.asarray(v, dtype=np.float64)
    run = np.cumsum(v, axis=1)                          # (sequential: the ascending running sum)
    T = run[:, -1]
    ok = T > 0.0
    x = u * T
    hit = (x[:, None] < run) & (v > 0.0)
    first = np.argmax(hit, axis=1)
    last = v.shape[1] - 1 - np.argmax((v > 0.0)[:, ::-1], axis=1)
    index = np.where(hit.any(axis=1), first, last)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.abs(u[:, None] - run / T[:, None]).min(axis=1)
    return np.where(ok, index, -1), np.where(ok, margin, np.inf)


def tip_weights(codes, S):
    """[P][S] indicator of a compact tip (a code >= S: missing, the vector of ones)"""
    codes = np.asarray(codes)
    P = len(codes)
    out = np.ones((P, S))
    seen = codes < S
    out[seen] = 0.0
    out[np.arange(P)[seen], codes[seen]] = 1.0
    return out


def judge(held, seed, states, cats, u_engine):
    """held: what the engine holds --
         q [K][P] or None (one category), freqs [S], top [K][P][S], lnl_child: [K][P][S] partials, tip codes [P] or None (a root
         call), lnl_matrix [K][S][S] or None, edges: a list of (parent slot, [K][P][S] partials or tip codes [P], matrix [K][S][S])
       states [slots][P], cats [P] (or None with one category): the engine's draw; u_engine: its unit roundoff.
    -> a list over the draws (category, top, edge 0, ...) of dict(want [P], margin [P], eps, weights [P][n], forced [P])
       want: the reference's draw given the engine's category and parent state (-1: none); forced: a tip with one compatible state."""
    top = np.asarray(held["top"])
    K, P, S = top.shape
    c = np.arange(P)
    out = []
    if held["q"] is not None:
        v = np.asarray(held["q"]).T
        want, margin = pick(v, uniform(seed, 0, c))
        out.append(dict(name="category", want=want, margin=margin, eps=0.0, weights=v, forced=np.zeros(P, dtype=bool)))
        k = np.asarray(cats)
    else:
        out.append(None)
        k = np.zeros(P, dtype=np.int64)
    live = k >= 0
    kk = np.where(live, k, 0)
    # the top
    f = np.ones((P, S))
    if held["lnl_child"] is not None:
        child = np.asarray(held["lnl_child"])
        col = tip_weights(child, S) if child.ndim == 1 else child[kk, c]
        f = np.einsum("cij,cj->ci", np.asarray(held["lnl_matrix"])[kk], col)
    v = np.asarray(held["freqs"])[None, :] * top[kk, c] * f
    v[~live] = 0.0
    want, margin = pick(v, uniform(seed, 1, c))
    out.append(dict(name="top", want=want, margin=margin, eps=2.0 * (S + 4) * u_engine, weights=v, forced=np.zeros(P, dtype=bool)))
    for i, (slot, post, matrix) in enumerate(held["edges"]):
        a = np.asarray(states[slot])
        has = live & (a >= 0)
        row = np.asarray(matrix)[kk, np.where(has, a, 0)]              # [P][S]: P_k[a, .]
        post = np.asarray(post)
        forced = np.zeros(P, dtype=bool)
        if post.ndim == 1:
            v = row * tip_weights(post, S)
            forced = has & (post < S)
        else:
            v = row * post[kk, c]
        v[~has] = 0.0
        want, margin = pick(v, uniform(seed, 2 + i, c))
        # one compatible state is that state, without arithmetic
        want = np.where(forced, np.where(post < S, post, 0) if post.ndim == 1 else want, want)
        margin = np.where(forced, np.inf, margin)
        out.append(dict(name="edge %d" % i, want=want, margin=margin, eps=4.0 * u_engine, weights=v, forced=forced))
    return out


def change_counts(states, parents, weights):
    """outChangeCounts recomputed from the returned states"""
    states = np.asarray(states)
    out = np.zeros(len(parents))
    for i, slot in enumerate(parents):
        a, b = states[slot], states[i + 1]
        out[i] = float((np.asarray(weights)[(a >= 0) & (b >= 0) & (a != b)]).sum())
    return out
