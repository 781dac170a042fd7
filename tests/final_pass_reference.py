"""High-precision restatement of the final ("up") pass and of the scaled read-out, for tests/test_final_pass_bounds.py.

The recurrences of mrbayes_amd/csrc/mbamd_reports.h on tests/operation_reference.py's number types (np.longdouble where its roundoff
is at most 2^-60, exact Fractions otherwise); all arrays are [K][P][S], matrices [K][S][S]:

    top(down, factor)      final(top)[a] = down[a] factor[a]              factor = P_top . tip_root, or None on a rooted tree
    step(anc, down, m)     u[a] = anc[a] / sum_i m[a][i] down[i]          (0 where that sum is 0)
                           final[a] = (sum_i u[i] m[a][i]) down[a]        -- m[a][i] in the SECOND sum too, as the reference program has it

Every term is non-negative, so the reference's own relative error is a few units of its roundoff whatever the order of summation.

read_out(...) is the integer model of mbamdGetScaledPartials: no arithmetic beyond exact powers of two.
"""
import numpy as np

from tests.operation_reference import LN2

SMALLEST_NORMAL = 2.0 ** -126
SUBNORMAL_STEP = 2.0 ** -149


def top(ref, down, factor=None):
    return down if factor is None else down * factor


def step(ref, anc, down, m):
    s = ref.einsum("kai,kci->kca", m, down)
    live = np.asarray(s != 0, dtype=bool)
    u = anc * 0
    u[live] = anc[live] / s[live]
    return ref.einsum("kci,kai->kca", u, m) * down


def whole_tree(ref, tree, down, matrices, root_factor):
    """final partials of every interior node of `tree` (mrbayes_amd.tree.Tree): node -> wide [K][P][S]; `down` and `matrices` by node"""
    out = {tree.root_left: top(ref, down[tree.root_left], root_factor)}
    for p in reversed(tree.int_down_pass):
        if p != tree.root_left:
            out[p] = step(ref, out[tree.anc[p]], down[p], matrices[p])
    return out


def read_out(raw, exponents):
    """What the scaled read-out owes for the buffer `raw` (float32 values, [K][P][S]) with the integer exponents [K][P]:
        emax_c = the largest exponent over the categories with any non-zero value at pattern c (0 where there is none)
        out    = raw 2^(e_kc - emax_c), EXACTLY, as float64 (24 bits and an exponent far inside double's range)
        ln     = float32(emax LN2)
    and `rounded`: out rounded to nearest-even on float32's subnormal grid where it lies below 2^-126 (the same value elsewhere)."""
    raw = np.asarray(raw, dtype=np.float64)
    e = np.asarray(exponents, dtype=np.int64)
    live = (raw != 0).any(axis=2)                                          # [K][P]
    emax = np.where(live.any(axis=0), np.where(live, e, np.iinfo(np.int64).min).max(axis=0), 0)
    shift = (e - emax[None, :]).astype(np.int32)
    out = np.ldexp(raw, shift[:, :, None])
    assert np.all((out != 0) == (raw != 0)), "the model itself underflowed"
    rounded = np.where(out < SMALLEST_NORMAL, np.rint(out / SUBNORMAL_STEP) * SUBNORMAL_STEP, out)
    ln = (emax.astype(np.float64) * LN2).astype(np.float32)
    return out, rounded, ln, emax, shift


def integer_exponent(ln):
    """the integer e behind a read-out's ln = float32(e LN2); asserted, not assumed"""
    ln = np.asarray(ln)
    assert ln.dtype == np.float32
    e = np.rint(ln.astype(np.float64) / LN2).astype(np.int64)
    assert np.array_equal(ln, (e.astype(np.float64) * LN2).astype(np.float32)), "lnScale is not float32(e ln 2) of an integer e"
    return e
