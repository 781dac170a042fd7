"""High-precision restatement of mbamdUpdateTransitionMatricesFromRateMatrix, for tests/test_rate_exponential.py: the same series,

    exp(Q tau) = ( sum_{n <= N} e^-y y^n / n!  R^n )^(2^s),   R = I + Q / mu,  mu = max_i sum_{j != i} q_ij,  y = mu tau / 2^s <= 1

in np.longdouble (operation_reference.LONGDOUBLE_QUALIFIES: unit roundoff 2^-64 on x86) with N_REF = 30 terms instead of the
engine's 25: at y <= 1 and s <= 20 the terms left out are below 2^20 / 31! = 2^-92.6.  Like the engine it uses the off-diagonals of Q
only; the row sums, mu, the argument mu r t and everything after are formed in the wide type from the very doubles the engine is
given.  Every quantity is non-negative, so the reference's own error is componentwise relative: the count of roundings of the engine
(test_rate_exponential.py derives c(N, S)) at N_REF and 2^-64.  test_reference_against_mpmath pins it against mpmath.expm.

Also here: the rate matrices of the test cases, the numbers the engine's host side derives (the squaring count decides the bound),
and the edge lengths that make mu r t hit a given value.
"""
import functools

import numpy as np

from tests.operation_reference import LD, LONGDOUBLE_QUALIFIES

N_DEVICE = 25                         # MBAMD_RATE_EXP_TERMS (mbamd_rate_exponential_table.h)
N_REF = 30
MAX_ARGUMENT = 2.0 ** 20              # mu r t at most: 20 squarings


# ---- what the engine's host side derives, in its order of operations (rate_exp_matrix, rate_exp_args) --------------------------------
def row_sums(Q):
    """sum_{j != i} q_ij in double, j ascending"""
    S = Q.shape[0]
    out = np.zeros(S)
    for i in range(S):
        s = 0.0
        for j in range(S):
            if j != i:
                s = s + float(Q[i, j])
        out[i] = s
    return out


def mu_of(Q):
    return float(row_sums(Q).max())


def argument(mu, r, t):
    """x = mu (r t) as the engine forms it"""
    return float(np.float64(mu) * (np.float64(r) * np.float64(t)))


def reduce_argument(x):
    """(s, y): the smallest s with x / 2^s <= 1, and y = x / 2^s"""
    s = 0
    if x > 1.0:
        f, e = np.frexp(x)
        s = int(e) - 1 if f == 0.5 else int(e)
    return s, float(np.ldexp(x, -s))


def edge_length_for(mu, r, target, over=False):
    """The largest t with mu (r t) <= target (over: the smallest t with mu (r t) > target), by stepping through the doubles"""
    if target == 0.0 and not over:
        return 0.0
    t = target / (mu * r)
    for _ in range(64):
        if argument(mu, r, t) <= target:
            break
        t = float(np.nextafter(t, 0.0))
    for _ in range(64):
        up = float(np.nextafter(t, np.inf))
        if argument(mu, r, up) > target:
            break
        t = up
    assert argument(mu, r, t) <= target < argument(mu, r, float(np.nextafter(t, np.inf))), (mu, r, target)
    return float(np.nextafter(t, np.inf)) if over else t


# ---- rate matrices -------------------------------------------------------------------------------------------------------------------
def _finish(Q):
    Q = np.array(Q, dtype=np.float64)
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -row_sums(Q))
    return np.ascontiguousarray(Q)


def dense_q(rng, S):
    """Dense, non-reversible; every rate a multiple of 2^-10 and the largest row sum a power of two, so that the row sums, mu and
    mu r t (r, t powers of two) are exact: the arguments 1 and 2^20 are hit exactly."""
    Q = rng.integers(1, 1024, size=(S, S)).astype(np.float64)
    np.fill_diagonal(Q, 0.0)
    i = int(np.argmax(Q.sum(axis=1)))
    total = Q[i].sum()
    j = (i + 1) % S
    Q[i, j] += 2.0 ** np.ceil(np.log2(total)) - total
    Q = _finish(Q / 1024.0)
    m = mu_of(Q)
    assert np.frexp(m)[0] == 0.5, m
    return Q


def sparse_q(rng, S):
    """Non-reversible with 30 % of the rates zero (every state keeps one way out); the rates over four orders of magnitude"""
    Q = rng.random((S, S)) * np.exp2(rng.integers(-12, 2, size=(S, S)).astype(np.float64))
    Q[rng.random((S, S)) < 0.3] = 0.0
    for i in range(S):
        Q[i, (i + 1) % S] = max(Q[i, (i + 1) % S], 0.01)
    return _finish(Q)


def cycle_q(S, rate=0.7):
    """The one-way cycle i -> i + 1 (mod S): a circulant, eigenvalues rate (w^k - 1), nearly all complex"""
    return _finish(rate * np.roll(np.eye(S), 1, axis=1))


def chain_q(S):
    """The one-way chain 0 -> 1 -> ... -> S - 1 at rate 1, the last state absorbing: ONE Jordan block for the eigenvalue -1.
    P_ij(t) = e^-t t^(j-i) / (j-i)! for i <= j < S - 1; at S = 3: P_00 = e^-t, P_01 = t e^-t, P_02 = 1 - e^-t - t e^-t."""
    Q = np.zeros((S, S))
    for i in range(S - 1):
        Q[i, i + 1] = 1.0
    return _finish(Q)


def reversible_q(rng, S):
    """(Q, pi): Q_ij = r_ij pi_j, one expected substitution per unit time (as matrix_reference.reversible_system, 'ordinary')"""
    pi = rng.random(S) + 0.2
    pi = pi / pi.sum()
    r = np.triu(rng.random((S, S)) + 0.1, 1)
    r = r + r.T
    q = r * pi[None, :]
    np.fill_diagonal(q, 0.0)
    q = q / (pi * q.sum(axis=1)).sum()
    return _finish(q), pi


KINDS = ("dense", "sparse", "cycle", "chain")


def rate_matrix(kind, S, seed=61):
    rng = np.random.default_rng(seed + 100 * S + KINDS.index(kind))
    return {"dense": lambda: dense_q(rng, S), "sparse": lambda: sparse_q(rng, S), "cycle": lambda: cycle_q(S), "chain": lambda: chain_q(S)}[kind]()


# ---- the reference -------------------------------------------------------------------------------------------------------------------
class RateExponentialReference:
    """P, P', P'' of one rate matrix in the wide type; the powers of R are formed once"""

    def __init__(self, Q, terms=N_REF):
        assert LONGDOUBLE_QUALIFIES
        Q = np.asarray(Q, dtype=np.float64)
        S = self.S = Q.shape[0]
        off = Q.astype(LD)
        off[np.arange(S), np.arange(S)] = LD(0)
        sums = off.sum(axis=1)
        self.mu = sums.max()
        self.Q = off.copy()
        self.Q[np.arange(S), np.arange(S)] = -sums
        self.absQ = np.abs(self.Q.astype(np.float64))
        eye = np.eye(S, dtype=LD)
        if self.mu > 0:
            R = off / self.mu
            R[np.arange(S), np.arange(S)] = (self.mu - sums) / self.mu
        else:
            R = eye.copy()
        self.powers = [eye, R]
        for _ in range(2, terms + 1):
            self.powers.append(self.powers[-1] @ R)

    def transition(self, tau):
        """exp(Q tau), tau in the wide type"""
        x = self.mu * tau
        s = 0
        while x > 1:
            x = x / 2
            s += 1
        w = np.exp(-x)
        T = w * self.powers[0]
        for n in range(1, len(self.powers)):
            w = w * x / n
            T = T + w * self.powers[n]
        for _ in range(s):
            T = T @ T
        return T

    def matrices(self, rates, t):
        """(P, P', P'') [K][S][S] each, in the wide type, at the edge length t"""
        out = [np.empty((len(rates), self.S, self.S), dtype=LD) for _ in range(3)]
        for k, r in enumerate(rates):
            r = LD(float(r))
            P = self.transition(r * LD(float(t)))
            D1 = r * (self.Q @ P)
            out[0][k], out[1][k], out[2][k] = P, D1, r * (self.Q @ D1)
        return out


@functools.lru_cache(maxsize=None)
def reference_for(kind, S):
    return RateExponentialReference(rate_matrix(kind, S))
