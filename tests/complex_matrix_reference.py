"""High-precision restatement of the transition-matrix kernels on a COMPLEX instance (BEAGLE_FLAG_EIGEN_COMPLEX), for
tests/test_complex_eigen.py: tests/matrix_reference.py with eigenvalues a_s + i b_s.

V, V^-1 are the real block form (include/libhmsbeagle/beagle.h): b_s == 0 is a real eigenvalue; b_p != 0 opens the adjacent pair
(p, p + 1) with a_(p+1) = a_p, b_(p+1) = -b_p.  With mu_s = r_k (a_s + i b_s) and z_s = mu_s^o exp(mu_s t),

    X[k] = V B V^-1,    B = [Re z_s] at a real s,   [[Re z_p, Im z_p], [-Im z_p, Re z_p]] at a pair           (clamped at zero for o = 0)

from the very doubles the engine is given.  Written as a sum over ONE index, with partner(p) = p + 1, partner(p + 1) = p:

    X[k,i,j] = sum_s (V[i,s] Re z_s - V[i,partner(s)] Im z_s) V^-1[s,j]            (z_(p+1) = conj z_p)

Together with X comes what the rounding bound of test_complex_eigen.py is made of: real indices contribute to W as in
matrix_reference.py, a pair contributes

    n_p |z_p| (|V[i,p]| + |V[i,p+1]|) (|V^-1[p,j]| + |V^-1[p+1,j]|),     n_p = S + c_o + 4 + 2 |x_p| + 2 |y_p|,   c = (7, 13, 17)

with x = a r t, y = b r t, |z_p| = |mu_p|^o e^(x_p); `mag` is the same sum without the counts.

Precision: np.longdouble where its unit roundoff is at most 2^-60 (operation_reference.LONGDOUBLE_QUALIFIES).  Both arguments are formed
exactly (fractions.Fraction) and split into the nearest double and the remainder, as matrix_reference._exact_argument does for x:
    exp(x) = exp(hi) (1 + lo);    cos(y) = cos(hi) - sin(hi) lo,   sin(y) = sin(hi) + cos(hi) lo,     |lo| <= 2^-53 |y|
The angle matters as much as the exponent: an error d in y moves Re z and Im z by |z| d ABSOLUTELY, and the product of three doubles
rounded to 64 bits would be off by 2 * 2^-64 |y| -- 2^-53 |z| at |y| = 1 000.  The neglected lo^2 / 2 is below 2^-80.  cosl / sinl reduce
a 64-bit argument properly.  The rest is a handful of longdouble roundings per term and numpy's pairwise sum: (S + 8) 2^-64 of `mag`.
test_reference_against_mpmath (test_complex_eigen.py) holds X to 2^-58 of mag against the same sum at 50 digits, and that sum to
mpmath.expm of the matrix the system defines.  Where longdouble is no wider than double everything is mpmath at 200 bits (slow: the
test module keeps a reduced list of shapes then).
"""
import fractions

import mpmath
import numpy as np

from tests.operation_reference import LD, LONGDOUBLE_QUALIFIES

# the count of roundings in Re z and Im z beyond 2 |x| + 2 |y|, by derivative order (derived in test_complex_eigen.py)
C_ORDER = (7, 13, 17)


def pairs_of(b):
    """partner [S] (int) of the imaginary parts b: p + 1, p, or s itself; raises on an unpaired value"""
    b = np.asarray(b, dtype=np.float64)
    partner = np.arange(len(b))
    s = 0
    while s < len(b):
        if b[s] != 0.0:
            assert s + 1 < len(b) and b[s + 1] == -b[s], "an unpaired imaginary part"
            partner[s], partner[s + 1] = s + 1, s
            s += 1
        s += 1
    return partner


def _exact_argument(lam, r, t):
    """lam r t exactly, as (nearest double, remainder as a double)"""
    x = fractions.Fraction(float(lam)) * fractions.Fraction(float(r)) * fractions.Fraction(float(t))
    hi = float(x)
    return hi, float(x - fractions.Fraction(hi))


class ComplexMatrixReference:
    """The spectral sums of one complex eigen-system (V, V^-1, a, b); V^-1 may come in the wide type (test_reference_against_mpmath
    gives the inverse of V to 64 bits, so that the system defines ONE matrix to compare an exponential with)."""

    def __init__(self, V, Vi, a, b):
        self.V, self.a, self.b = (np.asarray(x, dtype=np.float64) for x in (V, a, b))
        self.Vi_wide = np.asarray(Vi, dtype=LD) if LONGDOUBLE_QUALIFIES else np.asarray(Vi, dtype=np.float64)
        self.Vi = np.asarray(Vi, dtype=np.float64)
        self.S = len(self.a)
        self.partner = pairs_of(self.b)
        self.first = np.flatnonzero(self.partner > np.arange(self.S))            # the first index of every pair
        self.real = np.flatnonzero(self.partner == np.arange(self.S))
        self.absV, self.absVi = np.abs(self.V), np.abs(self.Vi)
        # |V[i,p]| + |V[i,p+1]| and |V^-1[p,j]| + |V^-1[p+1,j]| per pair
        self.pairV = self.absV[:, self.first] + self.absV[:, self.first + 1]
        self.pairVi = self.absVi[self.first, :] + self.absVi[self.first + 1, :]
        if LONGDOUBLE_QUALIFIES:
            # [i][j][s]: s last, the axis numpy sums pairwise
            VL = self.V.astype(LD)
            self.A = np.ascontiguousarray(VL[:, None, :] * self.Vi_wide.T[None, :, :])
            self.Ap = np.ascontiguousarray(VL[:, self.partner][:, None, :] * self.Vi_wide.T[None, :, :])

    def factors(self, r, t, order):
        """(Re z_s, Im z_s in the wide type, |z_s|, |x_s|, |y_s| as float64)"""
        S = self.S
        xh, xl, yh, yl = np.empty(S), np.empty(S), np.empty(S), np.empty(S)
        for s in range(S):
            xh[s], xl[s] = _exact_argument(self.a[s], r, t)
            yh[s], yl[s] = _exact_argument(self.b[s], r, t)
        if LONGDOUBLE_QUALIFIES:
            e = np.exp(xh.astype(LD)) * (LD(1) + xl.astype(LD))
            c0, s0 = np.cos(yh.astype(LD)), np.sin(yh.astype(LD))
            re, im = e * (c0 - s0 * yl.astype(LD)), e * (s0 + c0 * yl.astype(LD))
            mr, mi = self.a.astype(LD) * LD(r), self.b.astype(LD) * LD(r)
            for _ in range(order):
                re, im = mr * re - mi * im, mr * im + mi * re
            mod = np.exp(xh) * np.hypot(self.a * r, self.b * r) ** order
            return re, im, mod, np.abs(xh), np.abs(yh)
        re, im, mod = np.empty(S, dtype=object), np.empty(S, dtype=object), np.empty(S)
        with mpmath.workprec(200):
            for s in range(S):
                mu = mpmath.mpc(mpmath.mpf(float(self.a[s])), mpmath.mpf(float(self.b[s]))) * mpmath.mpf(float(r))
                z = mu ** order * mpmath.exp(mu * mpmath.mpf(float(t)))
                re[s], im[s], mod[s] = z.real, z.imag, float(abs(z))
        return re, im, mod, np.abs(xh), np.abs(yh)

    def matrices(self, rates, t, order):
        """(X [K][S][S] in the wide type, W [K][S][S] float64, mag [K][S][S] float64); X clamped at zero for order 0"""
        S, K = self.S, len(rates)
        X = np.empty((K, S, S), dtype=LD if LONGDOUBLE_QUALIFIES else object)
        W, mag = np.empty((K, S, S)), np.empty((K, S, S))
        for k, r in enumerate(rates):
            re, im, mod, ax, ay = self.factors(r, t, order)
            if LONGDOUBLE_QUALIFIES:
                X[k] = (self.A * re[None, None, :]).sum(axis=-1) - (self.Ap * im[None, None, :]).sum(axis=-1)
            else:
                with mpmath.workprec(200):
                    for i in range(S):
                        for j in range(S):
                            X[k, i, j] = mpmath.fsum((mpmath.mpf(self.V[i, s]) * re[s] - mpmath.mpf(self.V[i, self.partner[s]]) * im[s]) *
                                                     mpmath.mpf(self.Vi[s, j]) for s in range(S))
            # (the magnitudes in float64: a relative 2^-53 S of a bound is nothing)
            rl, fp = self.real, self.first
            n_real = S + 2 * order + 5 + 2.0 * ax[rl]
            n_pair = S + C_ORDER[order] + 4 + 2.0 * ax[fp] + 2.0 * ay[fp]
            mag[k] = self.absV[:, rl] @ (mod[rl][:, None] * self.absVi[rl, :]) + self.pairV @ (mod[fp][:, None] * self.pairVi)
            W[k] = self.absV[:, rl] @ ((mod[rl] * n_real)[:, None] * self.absVi[rl, :]) + self.pairV @ ((mod[fp] * n_pair)[:, None] * self.pairVi)
        if order == 0:
            X = np.where(X < 0, X * 0, X)
        return X, W, mag

    def defined_matrix(self):
        """V D V^-1 in the wide type: the rate matrix the doubles define"""
        assert LONGDOUBLE_QUALIFIES
        D = np.diag(self.a.astype(LD))
        for p in self.first:
            D[p, p + 1], D[p + 1, p] = LD(self.b[p]), -LD(self.b[p])
        return self.V.astype(LD) @ D @ self.Vi_wide


# ---- the same sum at 50 digits, and the matrix exponential it must equal ---------------------------------------------------------------
def _mp(v):
    return v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v))


def mpmath_entry(V, Vi, a, b, r, t, order, i, j, digits=50):
    """One entry of X and of mag by mpmath at `digits` digits, from the doubles (Vi: doubles, or an mpmath matrix): (value, clamped for order 0; mag)"""
    partner = pairs_of(b)
    with mpmath.workdps(digits):
        terms, mags = [], []
        for s in range(len(a)):
            mu = mpmath.mpc(mpmath.mpf(float(a[s])), mpmath.mpf(float(b[s]))) * mpmath.mpf(float(r))
            z = mu ** order * mpmath.exp(mu * mpmath.mpf(float(t)))
            vi = _mp(Vi[s, j])
            terms.append((mpmath.mpf(float(V[i, s])) * z.real - mpmath.mpf(float(V[i, partner[s]])) * z.imag) * vi)
            if partner[s] >= s:
                p = partner[s]
                vij = abs(vi) + (abs(_mp(Vi[p, j])) if p != s else 0)
                mags.append(abs(z) * (abs(mpmath.mpf(float(V[i, s]))) + (abs(mpmath.mpf(float(V[i, p]))) if p != s else 0)) * vij)
        v = mpmath.fsum(terms)
        if order == 0 and v < 0:
            v = mpmath.mpf(0)
        return v, float(mpmath.fsum(mags))


def mp_inverse(V, digits=50):
    """V^-1 of a float64 matrix as an mpmath matrix at `digits` digits"""
    with mpmath.workdps(digits):
        return mpmath.matrix(np.asarray(V, dtype=np.float64).tolist()) ** -1


def mp_block_matrix(V, Vi_mp, a, b, digits=50):
    """V D Vi_mp (mpmath matrix): with Vi_mp = V^-1 the one matrix whose exponential the spectral sum is"""
    S = len(a)
    partner = pairs_of(b)
    with mpmath.workdps(digits):
        D = mpmath.zeros(S)
        for s in range(S):
            D[s, s] = mpmath.mpf(float(a[s]))
            if partner[s] > s:
                D[s, s + 1], D[s + 1, s] = mpmath.mpf(float(b[s])), -mpmath.mpf(float(b[s]))
        return mpmath.matrix(np.asarray(V, dtype=np.float64).tolist()) * D * Vi_mp


def to_wide(m):
    """an mpmath matrix rounded to the wide type (longdouble: nearest double plus the remainder)"""
    out = np.empty((m.rows, m.cols), dtype=LD if LONGDOUBLE_QUALIFIES else np.float64)
    for i in range(m.rows):
        for j in range(m.cols):
            hi = float(m[i, j])
            out[i, j] = LD(hi) + LD(float(m[i, j] - mpmath.mpf(hi))) if LONGDOUBLE_QUALIFIES else hi
    return out
