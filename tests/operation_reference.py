"""High-precision restatement of the engine's arithmetic operations, for tests/test_operation_bounds.py and its neighbours.

One partials operation, the root / edge integration and a pruning pass over explicit transition matrices (no eigen-system), as plain
numpy einsum in np.longdouble where its unit roundoff is at most 2^-60 (x86: 2^-64), and EXACTLY, in fractions.Fraction, where it is
not.  Every input is a float64 array holding values already rounded to the engine's storage type, so what a caller compares is the
engine's arithmetic alone; every term of every sum here is non-negative, so the reference's own relative error is a few units of its
roundoff whatever the order of summation.

    ref = Reference()               # longdouble where it qualifies, Fractions otherwise
    ref = Reference(exact=True)     # Fractions (slow: small shapes)
"""
import fractions
import math

import numpy as np

LD = np.longdouble
LONGDOUBLE_QUALIFIES = bool(np.finfo(LD).eps <= 2.0 ** -60)
LN2 = 0.69314718055994530942        # the engine's constant (the double nearest ln 2)


def dense_tip(states, nstates, ncat):
    """Compact states as the 0/1 partials the engine treats them as (a code >= nstates is missing: all ones), float64 [K][P][S]"""
    P = len(states)
    d = np.zeros((ncat, P, nstates))
    for c, s in enumerate(states):
        if s < 0 or s >= nstates:
            d[:, c, :] = 1.0
        else:
            d[:, c, s] = 1.0
    return d


class Reference:
    def __init__(self, exact=None):
        self.exact = (not LONGDOUBLE_QUALIFIES) if exact is None else bool(exact)
        if not self.exact:
            assert np.finfo(LD).eps <= 2.0 ** -60

    # ---- number types ---------------------------------------------------------------------------------------------------------
    def widen(self, a):
        """float64 (or float32) values, exactly, in the reference's type"""
        a = np.asarray(a, dtype=np.float64)
        if not self.exact:
            return a.astype(LD)
        out = np.empty(a.shape, dtype=object)
        flat = out.reshape(-1)
        for n, v in enumerate(a.reshape(-1)):
            flat[n] = fractions.Fraction(float(v))
        return out

    def einsum(self, spec, *ops):
        if not self.exact:
            return np.einsum(spec, *ops)
        # (numpy's einsum takes no object arrays: the same sum of products through broadcasting)
        ins, out = spec.split("->")
        ins = ins.split(",")
        letters = sorted(set("".join(ins)))
        prod = None
        for sub, op in zip(ins, ops):
            t = op.transpose([sub.index(l) for l in letters if l in sub]).reshape([op.shape[sub.index(l)] if l in sub else 1 for l in letters])
            prod = t if prod is None else prod * t
        res = prod.sum(axis=tuple(n for n, l in enumerate(letters) if l not in out))
        kept = [l for l in letters if l in out]
        return res.transpose([kept.index(l) for l in out])

    def to_float(self, a):
        return np.asarray(a).astype(np.float64)

    def scaled(self, values, exponents):
        """values x 2^exponents (integers, broadcast against the values), exactly"""
        e = np.broadcast_to(np.asarray(exponents), np.shape(values))
        if not self.exact:
            return np.ldexp(self.widen(values), e.astype(np.int32))
        out = self.widen(values)
        flat, ef = out.reshape(-1), e.reshape(-1)
        for n in range(flat.size):
            flat[n] = flat[n] * fractions.Fraction(2) ** int(ef[n])
        return flat.reshape(np.shape(values))

    def log(self, a):
        """ln of positive reference values, float64 or better"""
        if not self.exact:
            return np.log(a)
        # ln x = ln f + log1p((x - f) / f), f the double nearest x: the correction is formed from the exact remainder
        out = np.empty(np.shape(a), dtype=LD)
        flat = out.reshape(-1)
        for n, x in enumerate(np.asarray(a, dtype=object).reshape(-1)):
            f = float(x)
            flat[n] = LD(math.log(f)) + LD(math.log1p(float((x - fractions.Fraction(f)) / fractions.Fraction(f))))
        return out

    # ---- comparisons ----------------------------------------------------------------------------------------------------------
    def rel_error(self, got, want):
        """|got - want| / want per element as float64; 0 where both are zero, inf where only the reference is"""
        g = self.widen(got)
        d = np.abs(g - want)
        out = np.zeros(np.shape(want))
        nz = np.asarray(want != 0, dtype=bool)
        if nz.any():
            out[nz] = self.to_float(d[nz] / want[nz])
        out[~nz & np.asarray(g != 0, dtype=bool)] = np.inf
        return out

    def exponents(self, col_max, bound, lo, hi):
        """The exponent a rescale stores for a column whose maximum is col_max: frexp's (the maximum / 2^e in [0.5, 1)), clamped to
        [lo, hi]; 0 for a dead column.  Also: which columns' maxima lie within `bound` (relative) of a power of two -- there a
        kernel within its error bound may land on the other side."""
        m, e = np.frexp(self.to_float(col_max))
        live = m > 0
        e = np.where(live, np.clip(e, lo, hi), 0).astype(np.int64)
        near = live & ((m <= 0.5 * (1.0 + bound)) | (m >= 1.0 - bound))
        return e, near

    # ---- the operations -------------------------------------------------------------------------------------------------------
    def contract(self, m, v):
        """sum_j m[k][i][j] v[k][c][j] -> [k][c][i]"""
        return self.einsum("kij,kcj->kci", m, v)

    def operation(self, m1, v1, m2, v2):
        """One partials operation: (m1 . v1) * (m2 . v2), [K][P][S]"""
        return self.contract(m1, v1) * self.contract(m2, v2)

    def factors(self, m1, v1, m2, v2):
        """The two factors of every element of one operation, (m1 . v1, m2 . v2): what an absolute error per rounding of one
        factor is multiplied by in the product (tests/test_exponent_range.py)"""
        return self.contract(m1, v1), self.contract(m2, v2)

    def root(self, weights, freqs, partials):
        """L_c = sum_k w_k sum_i pi_i partials[k][c][i]"""
        return self.einsum("k,i,kci->c", weights, freqs, partials)

    def edge(self, weights, freqs, parent, m, child):
        """L_c = sum_k w_k sum_i pi_i parent[k][c][i] sum_j m[k][i][j] child[k][c][j]"""
        return self.einsum("k,i,kci->c", weights, freqs, parent * self.contract(m, child))

    def prune(self, ops, sources, matrices):
        """A list of operations (destination, child 1, child 2; a child's matrix has the child's index) over `sources` (index -> wide
        [K][P][S]); returns index -> wide partials, the sources included."""
        have = dict(sources)
        for dst, a, b in ops:
            have[dst] = self.operation(matrices[a], have[a], matrices[b], have[b])
        return have
