"""The reference of tests/test_autocorrelated_rates.py: the site-order HMM over the rate categories of
mbamdCalculateAutocorrelatedLogLikelihood, written from include/libhmsbeagle/mbamd_reports.h alone, in np.longdouble.  No engine
code and no tests.

    H = sum over all paths k_0 .. k_{n-1} of  w_{k_0} L_{k_0}(c_0) prod_{s>=1} T^(j_s)[k_{s-1}, k_s] L_{k_s}(c_s)
    ln H = sum_s l(c_s) + ln(u^T A_1 .. A_{n-1} 1),   u = q(c_0),   A_s = T^(j_s) diag(q(c_s) / w)

`forward_backward` is the sequential algorithm with per-site normalisation, on the q and l that the engine itself returns;
`brute_force` enumerates the K^n paths from category likelihoods; `perfectly_correlated` is the closed form at T = identity, in log
space.  `bounds` is the a-priori rounding bound of the engine's arithmetic, derived in the docstring of the test module.
"""
import itertools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def power(T, j):
    """T^(j) by the header's rule: left-to-right binary exponentiation (square, then times T where the bit is set)"""
    T = np.asarray(T, dtype=LD)
    out = T.copy()
    for bit in bin(int(j))[3:]:
        out = out @ out
        if bit == "1":
            out = out @ T
    return out


def site_jumps(n, jumps):
    return np.ones(n, dtype=np.int64) if jumps is None else np.asarray(jumps, dtype=np.int64)


def forward_backward(q, l, w, patterns, T, jumps=None):
    """(ln H, the correction ln(u^T A_1 .. 1), gamma [K][n]) in longdouble, from q [K][P], l [P], w [K], the sites' patterns, T [K][K]
    and the jumps (None: ones; jumps[0] is not read)"""
    q, l, w = np.asarray(q, dtype=LD), np.asarray(l, dtype=LD), np.asarray(w, dtype=LD)
    patterns = np.asarray(patterns)
    K, n = q.shape[0], len(patterns)
    j = site_jumps(n, jumps)
    powers = {int(v): power(T, int(v)) for v in set(j[1:].tolist())}
    d = q[:, patterns] / w[:, None]                                                    # [K][n]
    alpha = np.zeros((n, K), dtype=LD)
    log_c = LD(0.0)
    a = q[:, patterns[0]].copy()
    dead = False
    for s in range(n):
        if s > 0:
            a = (a @ powers[int(j[s])]) * d[:, s]
        c = a.sum()
        if not c > 0:
            dead = True
            break
        a = a / c
        log_c += np.log(c)
        alpha[s] = a
    if dead:
        return -math.inf, -math.inf, np.zeros((K, n))
    beta = np.zeros((n, K), dtype=LD)
    b = np.ones(K, dtype=LD)
    for s in range(n - 1, -1, -1):
        beta[s] = b
        if s > 0:
            b = powers[int(j[s])] @ (d[:, s] * b)
            b = b / b.max()
    g = alpha * beta
    g = g / g.sum(1, keepdims=True)
    lsum = LD(0.0)
    for v in l[patterns]:
        lsum += v
    return lsum + log_c, log_c, g.T.copy()


def brute_force(Lk, w, patterns, T, jumps=None):
    """ln H over all K^n paths, in longdouble, from the category likelihoods Lk [K][P]"""
    Lk, w = np.asarray(Lk, dtype=LD), np.asarray(w, dtype=LD)
    K, n = Lk.shape[0], len(patterns)
    j = site_jumps(n, jumps)
    powers = [None] + [power(T, int(j[s])) for s in range(1, n)]
    H = LD(0.0)
    for path in itertools.product(range(K), repeat=n):
        term = w[path[0]] * Lk[path[0], patterns[0]]
        for s in range(1, n):
            term = term * powers[s][path[s - 1], path[s]] * Lk[path[s], patterns[s]]
        H += term
    return np.log(H)


def perfectly_correlated(q, l, w, patterns):
    """ln sum_k w_k prod_s L_k(c_s) with L_k = q_k L / w_k, in log space (longdouble); and gamma [K], the same at every site"""
    q, l, w = np.asarray(q, dtype=LD), np.asarray(l, dtype=LD), np.asarray(w, dtype=LD)
    with np.errstate(divide="ignore"):
        logs = np.log(w) + (np.log(q[:, patterns]) + l[None, patterns] - np.log(w)[:, None]).sum(1)
    top = logs.max()
    total = top + np.log(np.exp(logs - top).sum())
    return total, np.exp(logs - total)


def levels(n, R):
    out = 0
    while True:
        n = (n + R - 1) // R
        out += 1
        if n <= 1:
            return out


def bounds(n, K, R, jumps, l_sites, correction, lnH):
    """(bound of |ln H - ref|, relative bound of a gamma component) -- the docstring of tests/test_autocorrelated_rates.py"""
    j = site_jumps(n, jumps)
    c_pow = float(K * (j[1:] - 1).sum())
    chunks, lv = (n + R - 1) // R, levels(n, R)
    product = (K * (n + chunks) + 2 * n + c_pow + K * K) * U
    last = (4.0 * (abs(float(correction)) + math.log(2.0 * K * K)) + abs(float(lnH)) + float(np.abs(l_sites).sum())) * U
    lsum = min(n - 1, (R - 1) * lv) * U * float(np.abs(l_sites).sum())
    gamma = 2.0 * (K * (n + 2 * chunks + R * (lv + 1)) + 2 * n + c_pow + 1) * U + (K + 1) * U
    return product + last + lsum, gamma
