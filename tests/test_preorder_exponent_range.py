"""The calls that read post-order buffers AFTER a log-likelihood call, on post-order operands anywhere in the exponent range:
beagleUpdatePrePartials, beagleCalculateEdgeDerivatives, mbamdCalculateEdgeSecondDerivatives, beagleCalculateCrossProductDerivative,
mbamdCalculateNodePosteriors, mbamdGetCategoryPosteriors and the one-branch derivative call (csrc/mbamd_preorder.h,
mbamd_crossproducts.h, mbamd_posteriors.h, mbamd_derivatives.h).  A dynamically rescaling client (MrBayes' MB_BEAGLE_SCALE_DYNAMIC)
submits unscaled lists until a likelihood underflows: after a successful call its post-order buffers hold columns anywhere between 1
and 2^-149.  tests/test_exponent_range.py holds the post-order kernels to bounds there; every other test of the calls above runs on
rescaled operands.

  * CPU (`not gpu`): the host-emulation build of the same sources;
  * GPU (`gpu`): the product library on a MI355X.

What is measured.  An unscaled column at 2^-146 holds three bits: that loss is the post-order pass's and test_exponent_range's to
bound.  This module measures what the READERS add, so its reference is numpy float64 (80-bit long double for the double-precision
engine, whose columns at 2^-1070 times anything leave float64's range) computed from what the engine holds -- post-order buffers,
transition and differential matrices and the start vector read back (floats widen exactly), category weights, frequencies, rates and
pattern weights as set -- through the entry points of tests/preorder_reference.py that take columns and matrices as given: the
un-normalised pre-order recursion and, per edge (post, pre), category k and pattern c,
    den_k = sum_l pre[l] post[l],     N_k = sum_l pre[l] sum_j D1_k[l,j] post[j],     A_k the same with |D1_k|     (M_k, A2_k: with D2_k)
    q_k   = l_k / sum_k' l_k',  l_k = w_k sum_i pi_i parent[i] sum_j P_k[i,j] child[j] of the latest log-likelihood call's operands
    d     = sum_k q_k N_k / den_k,     d2 = sum_k q_k M_k / den_k - d^2,     p(a) = sum_k q_k pre[a] post[a] / den_k
    X[i,j] = sum_e t_e sum_c weight_c sum_k q_k r_k pre_e[i] post_e[j] / den_e,k
over the categories with den_k > 0 (include/libhmsbeagle/beagle.h: the others carry nothing).  On one tree q_k = w_k den_k / L_c at
every branch and these are N_c / L_c and the rest of the neighbouring modules; on the single operations of tier A the buffers belong
to no tree and only this form says what the calls return.

Bounds: the neighbouring modules' with the post-order chain taken out -- operands as stored are exact.  u = 2^-24; on the
double-precision engine u = 2^-53 kappa, unit_roundoff of tests/preorder_reference.py.  One pre-order operation adds at most
2 (S + 8) u to every component (tests/test_preorder_gradient.py); h = the operations on the pre-order chain from the start vector to
the edge's pre-order buffer; f = (S + 8) (1 + 2 h) u.
    a pre-order buffer       |got 2^e - want| <= 2 (S + 8) h u want per component, e one integer per column; every live column's
                             maximum lies in [0.5, 1), a dead column is zero
    gradient                 b1 = f sum_k q_k (A_k + |N_k|) / den_k;  sums: sum_c weight_c b1;  squares: sum_c weight_c (2 |d| b1 + b1^2)
    second derivatives       b2 = f sum_k q_k (A2_k + |M_k|) / den_k + 2 |d| b1 + b1^2; the matrix-core kernel (16 ... 64 states,
                             single precision) adds S u sum_k q_k A_k / den_k to b1 and the same with A2 to b2's first term
                             (tests/test_edge_second_derivatives.py)
    cross products           (4 (S + 8) (1 + 2 h) + 64 K + 8) u X_e per edge (tests/test_cross_products.py)
    node posteriors          4 f p per component, the best value 4 f (its reference), the best state where the reference separates
                             the two best by more than twice their bounds (tests/test_node_posteriors.py)
    one-branch derivatives   (S + 8) u (A1 + |D1|) / L and (S + 8) u [(A2 + |D2|) / L + 2 |d1| (A1 + |D1|) / L]
                             (tests/test_derivatives.py: its operands were always the call's own), lnL_c within
                             site_bound((2 S + K + 6) u) of tests/test_operation_bounds.py
    q                        k_category_posteriors takes the power of two out of the parent's and the child's column, forms
                             l_k from an S-step FMA chain, one product with the parent -- S + 1 roundings of positive terms in the
                             engine's precision --, the frequency, the sum over the states and the weight in double, puts the
                             powers of two back exactly and divides: |q - q_ref| <= 2 (S + 4) u q_ref on the single-precision
                             engine; the double-precision engine's sum over the S states is in the same precision as its products,
                             S more roundings: 2 (2 S + 4) u q_ref.  A pattern without likelihood: q = 0.
There is no absolute 2^-150 term and no exempted site: with the column's power of two taken out before the first product no kernel
of the family needed an allowance.  Every output of a call that returns 0 must be finite.

Tier A, single operations.  The post-order buffer T is test_exponent_range's tiny_columns (columns at 2^-104 ... 2^-146, elements up
to six binades below; the double-precision engine: 2^-1000 ... 2^-1070) with one pattern zero throughout.  R is a pre-order buffer
made by one operation from a start vector the client set, Z by one more with T as the SIBLING (checked).  Every read-out call runs over
the two edges (T, R) and (T, Z); the one-branch call takes the tiny buffer as parent and as child against an ordinary one (all patterns
alive: rc 0; with the dead pattern: BEAGLE_ERROR_FLOATING_POINT and the live sites to their bounds) -- and its operands are then
those q is made of.  The dead pattern's categories are skipped: zeros in every per-site output, nothing in any sum.

Tier B, a whole dynamically scaled evaluation: BeagleDivision(MB_BEAGLE_SCALE_DYNAMIC) at a taxon count where the float64 reference of
tests/preorder_reference.py puts the smallest site likelihood in [2^-146, 2^-127]; LogLike, AcceptMove, then every call of the family
over the whole tree.  Asserted from the engine: no rescale happened, the cumulative exponents are all zero, the root's smallest
live column maximum lies below 2^-126.  4 states x 4 x 70 at 50 taxa (1.2e-44), 20 states x 4 x 70 at 28 (1.9e-41; 29 and 30 taxa lie
below 2^-146), 61 states x 1 x 33 at 21 (1.7e-44): with 61 states the frequency and the root branch stand between the root's column
and the site likelihood, five decimal orders, and at 40 patterns no taxon count has the likelihood in the window AND a subnormal
root column (20 taxa: 4.0e-42 with the smallest column at 1.5e-36; 21: 4.2e-38; 22: the likelihood at 6.8e-48).  With four
categories a site's slowest or fastest category may underflow altogether where the site does not: a dead column, skipped by every
call and by the reference alike -- the bits it held are the post-order pass's loss, not a reader's.

Every check prints its worst error / bound (pytest -s shows them); a case collects what it missed and fails at its end.
"""
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests.hostemu import build_emu
from tests.operation_reference import LONGDOUBLE_QUALIFIES
from tests.preorder_reference import (depth_of, division, edge_terms, lnl_posteriors, mixed, pre_operation, pre_order_given, tip_vector,
                                      unit_roundoff)
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import U32
from tests.test_exponent_range import COLUMN_EXPONENTS, DEAD_PATTERN, switched, tiny_columns
from tests.test_operation_bounds import expected_layout, preference, random_matrices, site_bound, stored, vector

NONE = bg.BEAGLE_OP_NONE
SHIFT64 = 1000                                          # the double-precision engine's columns: 2^-1000 times columns at 2^-0 ... 2^-70
EXPONENTS64 = (0, 10, 20, 30, 40, 50, 60, 70)


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def wide(a, dbl):
    """values as stored, exactly, in the reference's type"""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.longdouble) if dbl else a


def narrow(a):
    return np.asarray(a).astype(np.float64)


def matrix_core(S, dbl, generic=False):
    return 16 <= S <= 64 and not dbl and not generic


class Case:
    """what a case prints and what it missed"""
    def __init__(self, label):
        self.label, self.missed = label, []

    def ratio(self, what, got, want, bound):
        """max |got - want| / bound; where the reference is exactly zero (with a zero bound) the engine's value must be"""
        got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want), np.asarray(bound)
        if not np.isfinite(got).all():
            self.missed.append("%s: %d values are not finite" % (what, int((~np.isfinite(got)).sum())))
            return float("inf")
        free = narrow(bound) > 0
        if np.any(got[~free] != narrow(want)[~free]):
            self.missed.append("%s: a value whose reference and bound are zero is not" % what)
        r = float(narrow(np.abs(got[free] - want[free]) / bound[free]).max()) if free.any() else 0.0
        if not r <= 1.0:
            self.missed.append("%s: error / bound %.3f" % (what, r))
        return r

    def check(self, what, ok, detail=""):
        if not ok:
            self.missed.append("%s %s" % (what, detail))

    def say(self, what, **ratios):
        print("%s %-30s error / bound: %s" % (self.label, what, ", ".join("%s %.3f" % (k.replace("_", " "), v) for k, v in ratios.items())))

    def done(self):
        assert not self.missed, (self.label, self.missed)


# ---- the checks both tiers share ---------------------------------------------------------------------------------------------------
def check_pre_buffer(case, what, got, want, h, S, u):
    """a pre-order buffer as read back against the un-normalised reference, up to one power of two per column"""
    gmax, wcol = got.max(axis=2), want.max(axis=2)
    live = narrow(wcol > 0).astype(bool)
    case.check(what, np.isfinite(got).all(), "holds values that are not finite")
    case.check(what, not got[~live].any(), "a dead column is not zero")
    case.check(what, bool(np.all((gmax[live] >= 0.5) & (gmax[live] < 1.0))), "a live column's maximum lies outside [0.5, 1)")
    e = np.zeros(gmax.shape, dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        e[live] = np.rint(narrow(np.log2(wcol[live] / np.where(gmax[live] > 0, gmax[live], 1.0)))).astype(np.int32)
    scaled = np.ldexp(want, -e[:, :, None])
    return case.ratio(what, got, scaled, 2 * (S + 8) * h * u * scaled)


def check_readouts(case, inst, edges, q, D1, D2, idx, pw, rates, lengths, S, K, u, dbl, generic=False):
    """every read-out call over `edges` = [(post index, pre index, post as stored, un-normalised reference pre, h)] against the
    reference; idx = (D1's matrix index, D2's, the weights index)"""
    mfma = matrix_core(S, dbl, generic)
    n, P = len(edges), len(pw)
    posts, pres = [e[0] for e in edges], [e[1] for e in edges]
    ref = []
    for _, _, post, pre, h in edges:
        f = (S + 8) * (1 + 2 * h) * u
        N, A, den = edge_terms(pre, post, D1)
        M, A2, _ = edge_terms(pre, post, D2)
        d = mixed(q, N, den)
        b1 = f * mixed(q, A + np.abs(N), den)
        b1m = b1 + (S * u * mixed(q, A, den) if mfma else 0)
        d2 = mixed(q, M, den) - d * d
        b2 = f * mixed(q, A2 + np.abs(M), den) + (S * u * mixed(q, A2, den) if mfma else 0) + 2 * np.abs(d) * b1m + b1m * b1m
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(den > 0, q / den, 0)                         # [K][P]
        p = np.einsum("kc,kca,kca->ca", coef, pre, post)
        X = np.einsum("c,kc,k,kci,kcj->ij", wide(pw, dbl), coef, wide(rates, dbl), pre, post)
        ref.append(dict(d=d, b1=b1, b1m=b1m, d2=d2, b2=b2, p=p, X=X, f=f, fx=(4 * (S + 8) * (1 + 2 * h) + 64 * K + 8) * u))
    wsum = lambda v: (pw * v).sum()
    # -- the gradient
    rc, per, sums, sq = inst.calculate_edge_gradient(posts, pres, [idx[0]] * n, [idx[2]] * n, sites=True)
    case.check("gradient", rc == 0, "rc %d" % rc)
    r = [max(case.ratio("gradient sites", per[i], ref[i]["d"], ref[i]["b1"]) for i in range(n)),
         max(case.ratio("gradient sums", sums[i], wsum(ref[i]["d"]), wsum(ref[i]["b1"])) for i in range(n)),
         max(case.ratio("gradient squared sums", sq[i], wsum(ref[i]["d"] ** 2), wsum(2 * np.abs(ref[i]["d"]) * ref[i]["b1"] + ref[i]["b1"] ** 2))
             for i in range(n))]
    case.say("gradient, %d edges" % n, sites=r[0], sums=r[1], squared_sums=r[2])
    # -- first and second derivatives from one read
    before = inst.get_second_derivative_launches()
    rc, per1, per2, sums1, sums2 = inst.calculate_edge_second_derivatives(posts, pres, [idx[0]] * n, [idx[1]] * n, [idx[2]] * n, sites=True)
    after = inst.get_second_derivative_launches()
    case.check("second derivatives", rc == 0, "rc %d" % rc)
    case.check("second derivatives", (after[0] - before[0], after[1] - before[1]) == ((0, 1) if mfma else (1, 0)), "kernel: %s -> %s" % (before, after))
    r = [max(case.ratio("d1 sites", per1[i], ref[i]["d"], ref[i]["b1m"]) for i in range(n)),
         max(case.ratio("d1 sums", sums1[i], wsum(ref[i]["d"]), wsum(ref[i]["b1m"])) for i in range(n)),
         max(case.ratio("d2 sites", per2[i], ref[i]["d2"], ref[i]["b2"]) for i in range(n)),
         max(case.ratio("d2 sums", sums2[i], wsum(ref[i]["d2"]), wsum(ref[i]["b2"])) for i in range(n))]
    case.say("second derivatives, %s kernel" % ("matrix-core" if mfma else "plain"), d1_sites=r[0], d1_sums=r[1], d2_sites=r[2], d2_sums=r[3])
    # -- cross products, all edges in one call
    rc, X = inst.calculate_cross_products(posts, pres, [0] * n, [idx[2]] * n, lengths)
    case.check("cross products", rc == 0, "rc %d" % rc)
    Xr = sum(t * ref[i]["X"] for i, t in enumerate(lengths))
    Xb = sum(t * ref[i]["fx"] * ref[i]["X"] for i, t in enumerate(lengths))
    case.say("cross products, %d edges" % n, entries=case.ratio("cross products", X, Xr, Xb))
    # -- node posteriors with sites and best states
    rc, pp, states, values, psums = inst.calculate_node_posteriors(posts, pres, [idx[2]] * n, sites=True, best=True)
    case.check("node posteriors", rc == 0, "rc %d" % rc)
    r, open_states = [0.0, 0.0, 0.0], 0
    for i in range(n):
        p, f4 = ref[i]["p"], 4 * ref[i]["f"]
        r[0] = max(r[0], case.ratio("posterior sites", pp[i], p, f4 * p))
        r[1] = max(r[1], case.ratio("posterior sums", psums[i], np.einsum("c,ca->a", wide(pw, dbl), p), f4 * np.einsum("c,ca->a", wide(pw, dbl), p)))
        order = np.sort(narrow(p), axis=1)
        first, second = order[:, -1], order[:, -2]
        r[2] = max(r[2], case.ratio("best values", values[i], first, f4 * first))
        clear = first - second > 2.0 * narrow(f4) * (first + second)
        open_states += int((~clear).sum())
        case.check("best states", np.array_equal(states[i][clear], np.argmax(narrow(p), axis=1)[clear]), "differ where the reference is clear")
        case.check("best states", np.array_equal(states[i], np.argmax(pp[i], axis=1)) and np.array_equal(values[i], pp[i].max(1)),
                   "are not the first maximum of the engine's own values")
    case.say("node posteriors", sites=r[0], sums=r[1], best=r[2])
    case.check("best states", open_states <= 0.02 * n * P + 2, "%d of %d not compared" % (open_states, n * P))
    return dict(per=per, per1=per1, per2=per2, pp=pp, values=values, states=states)


def check_branch(case, what, inst, call, W, F, parent, child, mats, pw, which, S, K, u, dbl, expect_rc=0):
    """the one-branch derivative call `call()` against its operands as stored (mats = P, P', P''); returns the reference's q"""
    rc, lnl, d1, d2 = call()
    site = inst.get_site_log_likelihoods()
    s1, s2 = inst.get_site_derivatives()
    case.check(what, rc == expect_rc, "rc %d, expected %d" % (rc, expect_rc))
    fwd = parent * np.einsum("kij,kcj->kci", mats[0], child)
    L = np.einsum("k,i,kci->c", W, F, fwd)
    term = lambda m: np.einsum("k,i,kci->c", W, F, parent * np.einsum("kij,kcj->kci", m, child))
    D1, A1, D2, A2 = term(mats[1]), term(np.abs(mats[1])), term(mats[2]), term(np.abs(mats[2]))
    Lw, ok = L[which], which
    r1, r2 = D1[ok] / Lw, D2[ok] / Lw - (D1[ok] / Lw) ** 2
    b1 = (S + 8) * u * (A1[ok] + np.abs(D1[ok])) / Lw
    b2 = (S + 8) * u * ((A2[ok] + np.abs(D2[ok])) / Lw + 2 * np.abs(r1) * (A1[ok] + np.abs(D1[ok])) / Lw)
    lnL = np.log(Lw)
    bl = site_bound((2 * S + K + 6) * u, narrow(lnL))
    r = [case.ratio(what + " lnL sites", site[ok], lnL, bl), case.ratio(what + " d1 sites", s1[ok], r1, b1), case.ratio(what + " d2 sites", s2[ok], r2, b2)]
    if expect_rc == 0:
        w = pw[ok]
        r += [case.ratio(what + " lnL sum", lnl, (w * lnL).sum(), (w * bl).sum()), case.ratio(what + " d1 sum", d1, (w * r1).sum(), (w * b1).sum()),
              case.ratio(what + " d2 sum", d2, (w * r2).sum(), (w * b2).sum())]
        case.say(what, lnL_sites=r[0], d1_sites=r[1], d2_sites=r[2], lnL_sum=r[3], d1_sum=r[4], d2_sum=r[5])
    else:
        case.say(what + " (live sites)", lnL_sites=r[0], d1_sites=r[1], d2_sites=r[2])
    return lnl_posteriors(W, F, parent, mats[0], child)[0]


def check_q(case, what, inst, q_ref, S, K, u, dbl, weights_index=0):
    q = inst.get_category_posteriors(weights_index)
    if K == 1:
        case.check(what, bool(np.all(q == 1.0)), "one category: q is not 1")
        return
    f = 2 * ((2 * S + 4) if dbl else (S + 4)) * u
    case.say(what, q=case.ratio(what, q, q_ref, f * q_ref))


# ---- tier A: single operations -----------------------------------------------------------------------------------------------------
# partials buffers: 1 the start vector; 2 = R; 3 = T, tiny with a dead pattern; 4 = Z; 5 = T with every pattern alive; 6 an ordinary
# post-order buffer.  Matrices: 0, 1, 2 transition matrices; 3, 4 differential matrices D1, D2; 5, 6 the one-branch call's P', P''.
START, R, T, Z, TL, O = 1, 2, 3, 4, 5, 6


def signed_matrices(rng, S, K, dbl):
    m = rng.random((K, S, S)) - 0.5
    return stored(m - m.mean(axis=2, keepdims=True), dbl)


def tiny_buffer(rng, S, K, P, dbl):
    if not dbl:
        a, m_of = tiny_columns(rng, S, K, P)
        assert set(np.unique(m_of).tolist()) == set(COLUMN_EXPONENTS)
        return a
    a, m_of = tiny_columns(rng, S, K, P, EXPONENTS64)
    assert set(np.unique(m_of).tolist()) == set(EXPONENTS64)
    return stored(a * 2.0 ** -SHIFT64, True)


def unit(S, K, P, dbl):
    return unit_roundoff(division(S, K, P), gradient_reference(S, K, P), True) if dbl else U32


def check_single_operations(lib, S, K, P, dbl=False, layout=None, generic=False):
    assert not dbl or LONGDOUBLE_QUALIFIES, "the double-precision tier needs a long double wider than float64 as its reference"
    rng = np.random.default_rng(29 + 1000 * S + 10 * K + (1 if dbl else 0))
    u = unit(S, K, P, dbl)
    case = Case("%2d states x %d x %d %s%s" % (S, K, P, "fp64" if dbl else "fp32", " plain second-derivative kernel" if generic else ""))
    inst = bg.BeagleInstance(lib, 1, 8, 1, S, P, 1, 8, K, 2, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        assert (layout or expected_layout(S, K, dbl)) in name, name
        tm = [random_matrices(rng, S, K, dbl) for _ in range(3)]
        dm = [signed_matrices(rng, S, K, dbl) for _ in range(4)]
        for n in range(3):
            inst.set_transition_matrix(n, tm[n])
        for n in range(4):
            inst.set_differential_matrix(3 + n, dm[n])
        for n, m in enumerate(tm + dm):
            assert np.array_equal(inst.get_transition_matrix(n), m), "matrix round trip (%d)" % n
        w, f = vector(rng, K, dbl), vector(rng, S, dbl)
        pw, rates = 1.0 + (np.arange(P) % 3).astype(np.float64), rng.random(K) + 0.5
        inst.set_category_weights(0, w)
        inst.set_state_frequencies(0, f)
        inst.set_pattern_weights(pw)
        inst.set_category_rates(rates)
        alive = tiny_buffer(rng, S, K, P, dbl)
        tiny = alive.copy()
        tiny[:, DEAD_PATTERN, :] = 0.0
        start = stored(rng.random((K, P, S)) * 0.9 + 0.05, dbl)
        other = stored(rng.random((K, P, S)) * 0.9 + 0.05, dbl)
        for n, a in ((START, start), (T, tiny), (TL, alive), (O, other)):
            inst.set_partials(n, a)
            assert np.array_equal(inst.get_partials(n), a), "partials round trip (buffer %d)" % n
        top = 2.0 ** -(SHIFT64 if dbl else 104)
        assert 0 < alive.max(axis=2).min() < top * 2.0 ** -41 and alive.max() < top
        W, F, M, D = wide(w, dbl), wide(f, dbl), [wide(m, dbl) for m in tm], [wide(m, dbl) for m in dm]
        Tw, Aw, Ow = wide(tiny, dbl), wide(alive, dbl), wide(other, dbl)
        # -- the pre-order operations: R from the start vector, Z from R with the tiny buffer as the sibling
        inst.update_pre_partials(np.array([[R, NONE, NONE, START, 0, NONE, NONE]], dtype=np.int32))
        inst.update_pre_partials(np.array([[Z, NONE, NONE, R, 1, T, 2]], dtype=np.int32))
        got_r, got_z = inst.get_partials(R), inst.get_partials(Z)
        pre_r = pre_operation(wide(start, dbl), M[0])
        pre_z = pre_operation(pre_r, M[1], Tw, M[2])
        case.say("pre-order operations", no_sibling=check_pre_buffer(case, "R", got_r, pre_r, 1, S, u),
                 tiny_sibling=check_pre_buffer(case, "Z on R as stored", got_z, pre_operation(wide(got_r, dbl), M[1], Tw, M[2]), 1, S, u),
                 tiny_sibling_chain=check_pre_buffer(case, "Z", got_z, pre_z, 2, S, u))
        # -- the one-branch derivative call, the tiny buffer as parent and as child; its operands are q's
        everyone, live = np.ones(P, dtype=bool), np.arange(P) != DEAD_PATTERN
        branch = lambda p, c: (lambda: inst.calculate_edge_derivatives([p], [c], [0], [5], [6], [0], [0], [NONE]))
        mats = (M[0], D[2], D[3])
        q_ref = check_branch(case, "one branch, tiny parent", inst, branch(TL, O), W, F, Aw, Ow, mats, pw, everyone, S, K, u, dbl)
        check_q(case, "q, tiny parent", inst, q_ref, S, K, u, dbl)
        q_ref = check_branch(case, "one branch, tiny child", inst, branch(O, TL), W, F, Ow, Aw, mats, pw, everyone, S, K, u, dbl)
        check_q(case, "q, tiny child", inst, q_ref, S, K, u, dbl)
        rc, _ = inst.calculate_root_log_likelihoods([TL], [0], [0], [NONE])
        case.check("root call", rc == 0, "rc %d" % rc)
        check_q(case, "q, tiny root", inst, lnl_posteriors(W, F, Aw)[0], S, K, u, dbl)
        q_ref = check_branch(case, "one branch, dead pattern", inst, branch(O, T), W, F, Ow, Tw, mats, pw, live, S, K, u, dbl,
                             expect_rc=bg.BEAGLE_ERROR_FLOATING_POINT)
        check_q(case, "q, dead pattern", inst, q_ref, S, K, u, dbl)
        case.check("q", not narrow(q_ref)[:, DEAD_PATTERN].any(), "the reference's q of the dead pattern")
        if K == 1:
            q_ref = np.ones((1, P))
        # -- every read-out call with the tiny buffer as post: against R (one operation) and against Z (two)
        out = check_readouts(case, inst, [(T, R, Tw, pre_r, 1), (T, Z, Tw, pre_z, 2)], q_ref, D[0], D[1], (3, 4, 0), pw, rates, [0.3, 0.7],
                             S, K, u, dbl, generic)
        dead = [out[k][:, DEAD_PATTERN] for k in ("per", "per1", "per2", "pp", "values")]
        case.check("dead pattern", not any(a.any() for a in dead) and not out["states"][:, DEAD_PATTERN].any(), "is not zero in every per-site output")
        print("%s SINGLE OPERATIONS %s; %s" % (case.label, "missed: %s" % case.missed if case.missed else "all within their bounds", name.split(": ", 1)[-1]))
        case.done()
    finally:
        inst.finalize()


#               switches                 shape        double   layout
SINGLE_CASES = [((), (4, 4, 70), False, None),                              # four states: registers, no LDS
                ((), (20, 4, 70), False, None),                             # tree-walk tiles, matrix-core second-derivative and cross-product kernels
                ((), (61, 1, 40), False, None),                             # two row tiles, one category
                ((), (12, 4, 70), False, "general-state MFMA"),             # the level layouts
                ((), (33, 4, 70), False, "general-state vector kernels"),
                (("MBAMD_CURV_GENERIC",), (20, 4, 70), False, None),        # the plain second-derivative kernel beyond four states
                ((), (4, 2, 70), True, None), ((), (20, 2, 70), True, None)]
SINGLE_IDS = ["%s%dx%dx%d%s" % ("".join(s[6:] + "-" for s in c[0]), *c[1], "-fp64" if c[2] else "") for c in SINGLE_CASES]


def run_single(lib, monkeypatch, switches, shape, dbl, layout):
    with switched(monkeypatch, switches):
        check_single_operations(lib, *shape, dbl=dbl, layout=layout, generic="MBAMD_CURV_GENERIC" in switches)


@pytest.mark.parametrize("switches,shape,dbl,layout", SINGLE_CASES, ids=SINGLE_IDS)
def test_single_operations_on_emulation(emu, monkeypatch, switches, shape, dbl, layout):
    run_single(emu, monkeypatch, switches, shape, dbl, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("switches,shape,dbl,layout", SINGLE_CASES, ids=SINGLE_IDS)
def test_single_operations(gpu, monkeypatch, switches, shape, dbl, layout):
    run_single(gpu, monkeypatch, switches, shape, dbl, layout)


# ---- tier B: a whole dynamically scaled evaluation ---------------------------------------------------------------------------------
def check_dynamic_division(lib, states, ncat, npat, ntaxa):
    div = division(states, ncat, npat, ntaxa)
    gref = gradient_reference(states, ncat, npat, ntaxa)
    t, S, K, P, u = div.tree, div.nstates, div.ncat, div.npatterns, U32
    case = Case("%2d states x %d x %d, %d taxa, dynamic scaling" % (S, K, P, ntaxa))
    # (the float64 reference from the `Division`: only to say which regime the taxon count puts the evaluation in)
    assert 2.0 ** -146 <= gref["min_L"] <= 2.0 ** -127, gref["min_L"]
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_DYNAMIC, pre_order=True, second_order=True)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name, name
        bd.LogLike(0)
        bd.AcceptMove(0)
        top, nodes = t.root_left, list(t.all_down_pass)
        # the regime, from the engine: the first, unscaled pass succeeded, no exponent anywhere, subnormal root columns
        assert not bd.rescaleBeagleAll and bd.successCount[0] == 1
        assert not inst.get_scale_exponents(bd.siteScalerIndex[0]).any()
        # (with several categories one of them may have underflowed altogether where the site has not -- the float64 reference puts
        #  such columns at 1e-60 and below: a dead column, which every call skips; no site is dead in all its categories)
        root_columns = inst.get_partials(bd.condLikeIndex[0][top]).max(axis=2)
        gone = root_columns == 0
        assert not gone.all(axis=0).any(), np.flatnonzero(gone.all(axis=0)).tolist()
        root_columns = root_columns[~gone]
        assert root_columns.min() < 2.0 ** -126, float(root_columns.min())
        bd.BranchCurvature(0)                            # the start vector, the pre-order list of the whole tree, D1 and D2
        # what the engine holds
        post = {n: (np.ascontiguousarray(np.broadcast_to(tip_vector(div, n), (K, P, S))) if n < t.ntaxa else inst.get_partials(bd.condLikeIndex[0][n]))
                for n in nodes + [t.root]}
        mats = {n: inst.get_transition_matrix(bd.tiProbsIndex[0][n]) for n in nodes}
        D1, D2 = inst.get_transition_matrix(bd.diffMatrixIndex), inst.get_transition_matrix(bd.diffMatrix2Index)
        assert all(np.isfinite(a).all() for a in post.values())
        w, pi, pw = div.category_weights(0), np.asarray(div.pi, dtype=np.float64), np.asarray(div.weights, dtype=np.float64)
        rates = np.asarray(div.cat_rates, dtype=np.float64)
        pre = pre_order_given(t, pre_operation(inst.get_partials(bd.preOrderStartIndex), mats[top]), post, mats)
        depth = {n: depth_of(t, n) for n in nodes}
        case.say("pre-order buffers, %d nodes" % len(nodes),
                 buffers=max(check_pre_buffer(case, "pre-order buffer of node %d" % n, inst.get_partials(bd.preOrderIndex[n]), pre[n], depth[n], S, u)
                             for n in nodes))
        q_ref, _ = lnl_posteriors(w, pi, post[top], mats[top], post[t.root])
        check_q(case, "q", inst, q_ref, S, K, u, False, bd.cijkIndex[0])
        if K == 1:
            q_ref = np.ones((1, P))
        lengths = [min(max(t.length[n], lk.BRLENS_MIN), lk.BRLENS_MAX) for n in nodes]
        edges = [(bd.condLikeIndex[0][n], bd.preOrderIndex[n], post[n], pre[n], depth[n]) for n in nodes]
        check_readouts(case, inst, edges, q_ref, D1, D2, (bd.diffMatrixIndex, bd.diffMatrix2Index, bd.cijkIndex[0]), pw, rates, lengths, S, K, u, False)
        # the root branch through the one-branch call: P' and P'' of the branch into spare matrix buffers
        pcopy, m1, m2 = bd.tiProbsScratchIndex[0], bd.tiProbsScratchIndex[1], bd.tiProbsScratchIndex[2]
        inst.update_transition_matrices(bd.cijkIndex[0], [pcopy], [lengths[nodes.index(top)]], first=[m1], second=[m2])
        call = lambda: inst.calculate_edge_derivatives([bd.condLikeIndex[0][top]], [bd.condLikeIndex[0][t.root]], [bd.tiProbsIndex[0][top]], [m1], [m2],
                                                       [bd.cijkIndex[0]], [bd.cijkIndex[0]], [bd.siteScalerIndex[0]])
        check_branch(case, "one branch, the root's", inst, call, w, pi, post[top], post[t.root],
                     (mats[top], inst.get_transition_matrix(m1), inst.get_transition_matrix(m2)), pw, np.ones(P, dtype=bool), S, K, u, False)
        print("%s DYNAMIC DIVISION %s; smallest site likelihood %.1e, root columns 2^%.1f ... 2^%.1f, %d dead; %s" %
              (case.label, "missed: %s" % case.missed if case.missed else "all within their bounds", gref["min_L"],
               np.log2(root_columns.min()), np.log2(root_columns.max()), int(gone.sum()), name.split(": ", 1)[-1]))
        case.done()
    finally:
        bd.finalize()


#                 states, categories, patterns, taxa: the smallest site likelihood of the float64 reference in [2^-146, 2^-127]
DYNAMIC_CASES = [(4, 4, 70, 50), (20, 4, 70, 28), (61, 1, 33, 21)]


@pytest.mark.parametrize("states,ncat,npat,ntaxa", DYNAMIC_CASES)
def test_dynamic_division_on_emulation(emu, states, ncat, npat, ntaxa):
    check_dynamic_division(emu, states, ncat, npat, ntaxa)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,ntaxa", DYNAMIC_CASES)
def test_dynamic_division(gpu, states, ncat, npat, ntaxa):
    check_dynamic_division(gpu, states, ncat, npat, ntaxa)
