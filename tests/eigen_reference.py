"""High-precision restatement of what the device eigen-solver is given and what must come out, for tests/test_eigen_bounds.py.
It shares nothing with k_eigen_reversible: no Jacobi iteration, no rotation.

    symmetrised(q, pi, mode)        B = D Q D^-1, d = sqrt(pi), in the wide type -- symmetrised entry by entry as the kernel defines it,
                                    B_ij = (d_i q_ij / d_j + d_j q_ji / d_i) / 2, B_ii = -sum_(j != i) q_ij (the given diagonal is not
                                    read).  mode 1: q holds exchangeabilities r_ij; Q_ij = r_ij pi_j, scaled to one expected
                                    substitution per unit time, -sum_i pi_i Q_ii = 1 (mode 0 takes the rates as they are, as the
                                    kernel does)
    cases(rng, S)                   six kinds of rate matrix as (name, exchangeabilities, pi); rate_matrix() makes the mode-0 input
    transition(B, pi, rates, t, o)  X[k] = D^-1 (r_k B)^o exp(B r_k t) D from numpy.linalg.eigh of B rounded to double, the spectral
                                    sum in the wide type (matrix_reference.MatrixReference); clamped at zero for o = 0 as the kernels do
    mpmath_transition(...)          the same by mpmath.expm, for test_reference_against_mpmath (tests/test_eigen_bounds.py)

The wide type is np.longdouble where its unit roundoff is at most 2^-60 (operation_reference.LONGDOUBLE_QUALIFIES), else mpmath at 200
bits in numpy object arrays.  eigh's own error -- a backward error of a few n 2^-53 |B| -- is too much on the hard kinds by itself
(system_of says where, and refines the pairs on the wide B); the mpmath comparison holds transition() to 2^-45 sqrt(pi_j / pi_i), far
inside every bound of the test module (whose smallest term is 1e-10 |B|).
"""
import mpmath
import numpy as np

from tests import matrix_reference as mr
from tests.operation_reference import LD, LONGDOUBLE_QUALIFIES

KINDS = ("ordinary", "equal rates", "near-equal", "skewed", "sparse", "wide rates")
PREC = 200


def wide(a):
    """a float64 array in the wide type, exactly"""
    a = np.asarray(a, dtype=np.float64)
    if LONGDOUBLE_QUALIFIES:
        return a.astype(LD)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mpmath.mpf(float(a[idx]))
    return out


def narrow(a):
    """a wide array rounded to float64"""
    if LONGDOUBLE_QUALIFIES:
        return np.asarray(a).astype(np.float64)
    a = np.asarray(a, dtype=object)
    return np.array([float(v) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)


def wsqrt(a):
    if LONGDOUBLE_QUALIFIES:
        return np.sqrt(a)
    return np.frompyfunc(mpmath.sqrt, 1, 1)(a)


def fro(a):
    """Frobenius norm of a wide array, as a float"""
    with mpmath.workprec(PREC):
        return float(wsqrt((a * a).sum()))


def symmetrised(q, pi, mode):
    with mpmath.workprec(PREC):
        q, pi = wide(q), wide(pi)
        S = len(pi)
        off = ~np.eye(S, dtype=bool)
        if mode == 1:
            q = np.where(off, q * pi[None, :], q * 0)
            q = q / (pi * q.sum(axis=1)).sum()
        q = np.where(off, q, q * 0)
        d = wsqrt(pi)
        b = d[:, None] * q / d[None, :]
        b = (b + b.T) / 2
        b[np.arange(S), np.arange(S)] = -q.sum(axis=1)
        return b


def rate_matrix(exch, pi):
    """Q_ij = r_ij pi_j with rows summing to zero, one expected substitution per unit time, in float64: the mode-0 input"""
    q = np.asarray(exch, dtype=np.float64) * np.asarray(pi)[None, :]
    np.fill_diagonal(q, 0.0)
    np.fill_diagonal(q, -q.sum(axis=1))
    return q / -(pi * np.diag(q)).sum()


def one_case(rng, S, kind):
    """(exchangeabilities: symmetric, zero diagonal; frequencies: positive, summing to one to rounding)"""
    assert kind in KINDS, kind
    pi = rng.random(S) + 0.2
    r = rng.random((S, S)) + 0.1
    if kind == "equal rates":
        pi, r = np.ones(S), np.ones((S, S))
    elif kind == "near-equal":
        pi, r = 1.0 + 1e-9 * rng.random(S), 1.0 + 1e-9 * rng.random((S, S))
    elif kind == "skewed":
        small = rng.choice(S, size=max(1, S // 3), replace=False)
        pi[small] = 10.0 ** -rng.uniform(6.0, 10.0, size=len(small))
    elif kind == "sparse":
        r = np.where(rng.random((S, S)) < 0.85, 0.0, r)
    elif kind == "wide rates":
        r = r * 10.0 ** rng.uniform(-8.0, 2.0, size=(S, S))
    r = np.triu(r, 1)
    if kind == "sparse":                                    # the ring i <-> i + 1 keeps Q irreducible
        for i in range(S):
            a, b = min(i, (i + 1) % S), max(i, (i + 1) % S)
            if a != b and r[a, b] == 0.0:
                r[a, b] = rng.random() + 0.1
    return r + r.T, pi / pi.sum()


def cases(rng, S):
    for kind in KINDS:
        r, pi = one_case(rng, S, kind)
        yield kind, r, pi


def system_of(B, pi):
    """(U, U^-1, lambda) in float64 from numpy.linalg.eigh of B rounded to double, refined on the wide B.  eigh alone is not enough
    on the hard kinds: its eigenvalues are off by a few u |B|, which a long branch multiplies by r t (1 240 at the longest), and its
    vectors by u |B| / gap, 1e-12 where a slow mode lies 1e-3 from the stationary one and has not decayed.  Three steps of the
    refinement of Ogita and Aishima (Japan J. Indust. Appl. Math. 35, 2018: with R = I - V^T V and T = V^T B V, lambda_i = T_ii /
    (1 - R_ii), V <- V (I + E), E_ij = (T_ij + lambda_j R_ij) / (lambda_j - lambda_i) across a gap and R_ij / 2 inside a cluster)
    square the error each where the correction is small against the gap; eigenvalues closer than 2^-20 |B| count as a cluster (the
    step does not converge across a gap its own correction exceeds), whose basis is only re-orthogonalised: eigh's mixing inside a
    cluster, u |B| / gap, meets a difference of the factors f of at most r t gap, u |B| r t e^(lambda r t) in all -- nothing unless
    two modes slower than 1e-3 lie within 1e-6 of each other, which no kind here makes."""
    b = narrow(B)
    lam, v = np.linalg.eigh(0.5 * (b + b.T))
    with mpmath.workprec(PREC):
        vw, eye = wide(v), wide(np.eye(len(lam)))
        delta = 2.0 ** -20 * fro(B)
        for _ in range(3):
            R = eye - vw.T.dot(vw)
            T = vw.T.dot(B.dot(vw))
            lw = np.diagonal(T) / (1 - np.diagonal(R))
            gap = lw[None, :] - lw[:, None]
            apart = narrow(abs(gap)) > delta
            E = np.where(apart, (T + lw[None, :] * R) / np.where(apart, gap, eye * 0 + 1), R / 2)
            vw = vw + vw.dot(E)
        lam, v = narrow((vw * B.dot(vw)).sum(axis=0) / (vw * vw).sum(axis=0)), narrow(vw)
    d = np.sqrt(np.asarray(pi, dtype=np.float64))
    return np.ascontiguousarray(v / d[:, None]), np.ascontiguousarray(v.T * d[None, :]), np.ascontiguousarray(lam)


def transition(B, pi, rates, t, order):
    """X [K][S][S] in the wide type"""
    return mr.MatrixReference(*system_of(B, pi)).matrices(np.asarray(rates, dtype=np.float64), t, order)[0]


def mpmath_transition(B, pi, r, t, order, digits=40):
    """D^-1 (r B)^order exp(B r t) D as an mpmath matrix, clamped at zero for order 0"""
    with mpmath.workdps(digits):
        S = len(pi)
        to_mpf = mr.to_mpf if LONGDOUBLE_QUALIFIES else (lambda x: x)
        Bm = mpmath.matrix(S, S)
        for i in range(S):
            for j in range(S):
                Bm[i, j] = to_mpf(B[i, j])
        rm = mpmath.mpf(float(r))
        E = mpmath.expm(Bm * (rm * mpmath.mpf(float(t))))
        for _ in range(order):
            E = (Bm * rm) * E
        d = [mpmath.sqrt(mpmath.mpf(float(p))) for p in pi]
        X = mpmath.matrix(S, S)
        for i in range(S):
            for j in range(S):
                X[i, j] = E[i, j] * d[j] / d[i]
                if order == 0 and X[i, j] < 0:
                    X[i, j] = mpmath.mpf(0)
        return X
