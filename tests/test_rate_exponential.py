"""mbamdUpdateTransitionMatricesFromRateMatrix: P = exp(Q r t), P' = r Q P, P'' = r Q P' of ANY rate matrix, on the device, by
uniformization with scaling and squaring (mbamd_rate_exponential.h; the contract: beagle.h), both engines.

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

  k_rate_exp_s4            4 states (a thread per entry and category)          k_rate_powers_small / _mfma<1..4>: R^1 ... R^N, once a call
  k_rate_exp_small         2, 3, 5 ... 8 states
  k_rate_exp_mfma<1..4>    9 ... 64 states (the fp64 matrix cores, operands in LDS)

The reference is tests/rate_exponential_reference.py: the same series in np.longdouble with N_REF = 30 terms, from the very doubles the
engine is given.

A. THE BOUND, from the kernels' own operation order.  u = 2^-53, N = 25, x = mu (r t) as the host rounds it, s the squaring count,
y = x / 2^s <= 1 (exact), T = sum_n w_n R^n, P = T^(2^s).  Every term of every sum is non-negative, so the relative errors of the
terms bound the relative error of the sum, componentwise and whatever the order.  Roundings that term n of T[i][j] takes part in:
    2 n              the n factors of R along a path: R_ij = q_ij / mu is rounded once, R_ii = (mu - sum_i) / mu twice
    (n - 1) (S + 3)  R^n = R^(n-1) R, n - 1 chains of fused multiply-adds, 4 ceil(S / 4) <= S + 3 links on the matrix cores (S elsewhere)
    2 n + 2          w_n = (w_(n-1) y) / n, and w_0 = e^-y from libm, within one unit in the last place = 2 u
    N - n + 1        the series: fma(w_n, R^n, T) and the N - n additions behind it
together (n - 1) (S + 3) + 3 n + N + 3 <= (N - 1) (S + 3) + 4 N + 3 at n = N.  (The CPU trial of the issue, 0.01 - 0.07 of
2^s (N + S + 4) u, is the typical case; the worst case has an entry made of the LAST term alone -- P_0j of a one-way chain at a short
edge -- and that term carries all N - 1 products.)  The row sums the host forms carry (S - 2) u each, relative to sum_i <= mu: R_ii is
off by at most S u absolutely, a shift of Q's diagonal by S u mu, which moves exp componentwise by the factor e^(+- S u mu tau):
S u y <= S u relative in T.  So T is within c_T u, c_T = (N - 1) (S + 3) + 4 N + 3 + S.  A squaring doubles a relative error and adds
its own chain: d' = 2 d + (S + 3) u, after s squarings 2^s c_T u + (2^s - 1) (S + 3) u.  Hence
    c(N, S) = c_T + S + 3 = N (S + 7) + S + 3                                              (1 % for the higher-order terms)
The terms left out of the series sum to at most tail(N, y) = y^(N+1) / (N+1)! per entry (Lagrange's remainder times e^-y; they
commute with T, and rows of T sum to at most one: 2^s tail(N, y) reaches P, absolutely).  The argument: x carries two roundings, so the
engine's exp is that of tau (1 + 2 u): |dP| <= 2 u tau (|Q| P)[i][j].  With the reference's own error (the same count at N_REF, 2^-64)

    E_P = 1.01 2^s c(N, S) u P + 2^s tail(N, y) + 2.02 u tau |Q| P + 2^s c(N_REF, S) 2^-64 P + 2^s tail(N_REF, y) + S 2^-1074
    double precision   |got - P| <= E_P;        single precision   |got - P| <= E_P + 2^-24 |P| + 2^-150     (ONE rounding of the double)

P' = r (Q P) is formed from the double P in LDS: the chain of S + 3 links, the product with r, and the S - 2 roundings of Q's diagonal,

    E_P' = r |Q| E_P + 1.01 (2 S + 5) u r |Q| P,        E_P'' = r |Q| E_P' + 1.01 (2 S + 5) u r |Q| (r |Q| P)        (+ S 2^-1074 each)

plus the rounding of the stored type.  At s = 20 and 64 states E_P is 2^20 1842 u = 2^-22.2 of P: the cap 2^20 keeps the double
result within a few single-precision roundings.

B. EXACT PROPERTIES: no entry of P negative; an absorbing state's row the unit vector; the entries below a one-way chain's diagonal
zero; t = 0 and r = 0.0 give P = I, P' = r Q rounded once; r = 0.0 gives P' = P'' = 0.   C. rows of P sum to one within the row's E_P.
D. AGREEMENT with the eigen paths: a reversible Q against mbamdSetRateMatrices + beagleUpdateTransitionMatrices on the same
(single-precision: the device solver's) instance, the one-way cycle against a complex instance fed numpy's eigen-system; the margin is
E_P plus the eigen path's own bound (tests/test_matrix_bounds.py, tests/test_complex_eigen.py) on the system that path holds.
E. EVERY STORED COPY: matrices made by the call, read back and set into a second instance: partials and lnL bit for bit.
F. END TO END: a 6-tip tree under the defective 3-state chain against long-double pruning.   G. LISTS of 1, 3 and 70 entries; a queued
update of a result.   H. pattern shards.   I. REFUSALS: status, and every matrix as it was; a Q of all zeros; the host side alone
under the host sanitizers.

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import ctypes as C
import functools
import math

import mpmath
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd import model as mbmodel
from tests import complex_matrix_reference as cr
from tests import matrix_reference as mr
from tests import rate_exponential_reference as rx
from tests.hostemu import build_emu
from tests.operation_reference import LD, LONGDOUBLE_QUALIFIES, Reference, dense_tip
from tests.test_matrix_products import NCAT, NTAXA, tree_division
from tests.test_operation_bounds import (_check_sites, expected_layout, operation_bound, preference, random_tree, root_bound, stored,
                                         vector)

NONE = bg.BEAGLE_OP_NONE
U64 = 2.0 ** -53
REF = Reference()
_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
pytestmark = pytest.mark.skipif(not LONGDOUBLE_QUALIFIES, reason="the reference needs a long double wider than double")


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def tag(S, K, double_precision):
    return "%2d states x %d %s" % (S, K, "fp64" if double_precision else "fp32")


def rates_of(K):
    """one rate exactly 0.0 among four; the largest a power of two, so that it can make mu r t hit a value exactly"""
    return np.array([0.5]) if K == 1 else np.array([0.0, 0.3, 1.1, 2.0])


# ---- A. the bound --------------------------------------------------------------------------------------------------------------------
def c_count(N, S):
    return N * (S + 7) + S + 3


def tail(N, y):
    return y ** (N + 1) / math.factorial(N + 1)


def rounding_stored(X, double_precision):
    return 0.0 if double_precision else 2.0 ** -24 * np.abs(mr.to_float(X)) + 2.0 ** -150


def bounds(ref, mu, rate, t, P, double_precision):
    """(E_P, E_P', E_P'') [S][S] of one category, the rounding of the stored type not yet in them; and s"""
    S = ref.S
    s, y = rx.reduce_argument(rx.argument(mu, rate, t))
    Pf = mr.to_float(P)
    QP = ref.absQ @ Pf
    grow = 2.0 ** s
    e0 = (1.01 * grow * c_count(rx.N_DEVICE, S) * U64 * Pf + grow * tail(rx.N_DEVICE, y) + 2.02 * U64 * rate * t * QP +
          grow * c_count(rx.N_REF, S) * 2.0 ** -64 * Pf + grow * tail(rx.N_REF, y) + S * 2.0 ** -1074)
    e1 = rate * (ref.absQ @ e0) + 1.01 * (2 * S + 5) * U64 * rate * QP + S * 2.0 ** -1074
    e2 = rate * (ref.absQ @ e1) + 1.01 * (2 * S + 5) * U64 * rate * (ref.absQ @ (rate * QP)) + S * 2.0 ** -1074
    return (e0, e1, e2), s


def arguments_of(mu, pivot):
    """(what, t): edge lengths that make mu pivot t hit 0, 2^-30, just under 1, exactly 1 (or the double below), just over 1, 37, 2^20"""
    below_one = float(np.nextafter(1.0, 0.0))
    return [("0", 0.0), ("2^-30", rx.edge_length_for(mu, pivot, 2.0 ** -30)), ("under 1", rx.edge_length_for(mu, pivot, below_one)),
            ("1", rx.edge_length_for(mu, pivot, 1.0)), ("over 1", rx.edge_length_for(mu, pivot, 1.0, over=True)),
            ("37", rx.edge_length_for(mu, pivot, 37.0)), ("2^20", rx.edge_length_for(mu, pivot, rx.MAX_ARGUMENT))]


@functools.lru_cache(maxsize=None)
def case_reference(kind, S, K):
    """(Q, rates, mu, [(what, t, (P, P', P''))]): computed once, shared by both engines on the emulation and on the device"""
    Q, rates = rx.rate_matrix(kind, S), rates_of(K)
    ref, mu = rx.reference_for(kind, S), rx.mu_of(Q)
    out = [(what, t, ref.matrices(rates, t)) for what, t in arguments_of(mu, float(rates.max()))]
    for a in out:
        for m in a[2]:
            m.setflags(write=False)
    return Q, rates, mu, out


def check_element_wise(lib, S, K, double_precision):
    dbl = double_precision
    worst, squarings = [0.0, 0.0, 0.0], set()
    for kind in rx.KINDS:
        Q, rates, mu, cases = case_reference(kind, S, K)
        ref = rx.reference_for(kind, S)
        n = len(cases)
        inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 3 * n, K, 1, preference_flags=preference(dbl))
        try:
            name = inst.details.implName.decode()
            assert expected_layout(S, K, dbl) in name, name
            inst.set_category_rates(rates)
            inst.update_transition_matrices_from_rate_matrix(Q, list(range(n)), [t for _, t, _ in cases], first=list(range(n, 2 * n)),
                                                             second=list(range(2 * n, 3 * n)))
            pivot = int(np.argmax(rates))
            s_pivot = {what: rx.reduce_argument(rx.argument(mu, rates[pivot], t))[0] for what, t, _ in cases}
            assert [s_pivot[w] for w in ("0", "2^-30", "under 1", "over 1", "37", "2^20")] == [0, 0, 0, 1, 6, 20], s_pivot
            if kind in ("dense", "chain"):               # (exact arithmetic: the values themselves are hit)
                assert [rx.argument(mu, rates[pivot], t) for w, t, _ in cases if w in ("1", "2^20")] == [1.0, rx.MAX_ARGUMENT]
            Qhat = np.array(ref.Q.astype(np.float64))
            np.fill_diagonal(Qhat, -rx.row_sums(Q))
            for u, (what, t, wide) in enumerate(cases):
                got = [inst.get_transition_matrix(u + o * n) for o in range(3)]
                for k in range(K):
                    E, s = bounds(ref, mu, rates[k], t, wide[0][k], dbl)
                    squarings.add(s)
                    for o in range(3):
                        bound = E[o] + rounding_stored(wide[o][k], dbl)
                        ratio = float((mr.error(got[o][k], wide[o][k]) / bound).max())
                        worst[o] = max(worst[o], ratio)
                        assert ratio <= 1.0, (tag(S, K, dbl), kind, "mu r t " + what, "category %d" % k, "order %d" % o, "s = %d" % s, ratio)
                    # C. the row sums, added in the wide type
                    row = np.abs(got[0][k].astype(LD).sum(axis=1) - LD(1)).astype(np.float64)
                    assert (row <= (E[0] + rounding_stored(wide[0][k], dbl)).sum(axis=1)).all(), (kind, what, k, row)
                    # B. the exact properties
                    assert (got[0][k] >= 0).all(), (kind, what, k, "a negative entry")
                    if t == 0.0 or rates[k] == 0.0:
                        assert np.array_equal(got[0][k], np.eye(S)), (kind, what, k, "P = I")
                        assert np.array_equal(got[1][k], stored(rates[k] * Qhat, dbl)), (kind, what, k, "P' = r Q rounded once")
                    if rates[k] == 0.0:
                        assert not got[1][k].any() and not got[2][k].any(), (kind, what, k, "zero derivatives")
                    if kind == "chain":
                        assert np.array_equal(got[0][k][S - 1], np.eye(S)[S - 1]), (what, k, "the absorbing state's row")
                        assert not np.tril(got[0][k], -1).any(), (what, k, "below the chain's diagonal")
                for o in range(3):
                    assert np.array_equal(stored(got[o], dbl), got[o])
        finally:
            inst.finalize()
    print("%s ELEMENT-WISE worst error / bound P %.3f, P' %.3f, P'' %.3f over %d rate matrices x 7 arguments; squarings met %s; %s" %
          (tag(S, K, dbl), worst[0], worst[1], worst[2], len(rx.KINDS), sorted(squarings), name.split(": ", 1)[-1]))
    return worst


#         every size class, the first MFMA size, a tile edge with one live column, the codon sizes
STATES = (2, 3, 4, 5, 8, 9, 16, 17, 20, 61, 64)
ELEMENT_CASES = [pytest.param(S, K, dbl, id="%s-%dx%d" % ("fp64" if dbl else "fp32", S, K)) for dbl in (False, True) for S in STATES for K in (1, 4)]


@pytest.mark.parametrize("S,K,double_precision", ELEMENT_CASES)
def test_element_wise_on_emulation(emu, S, K, double_precision):
    check_element_wise(emu, S, K, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision", ELEMENT_CASES)
def test_element_wise(gpu, S, K, double_precision):
    check_element_wise(gpu, S, K, double_precision)


# ---- the reference against mpmath ------------------------------------------------------------------------------------------------------
def test_reference_against_mpmath():
    """The long-double reference against mpmath.expm at 60 digits, S <= 5, the defective chain among them and its closed form at three
    states: within the reference's own term 2^s c(N_REF, S) 2^-64 P + 2^s tail(N_REF, y).  No engine."""
    worst = 0.0
    with mpmath.workdps(60):
        for kind, S in (("chain", 3), ("chain", 5), ("dense", 4), ("sparse", 5), ("cycle", 5), ("dense", 2)):
            Q = rx.rate_matrix(kind, S)
            ref = rx.reference_for(kind, S)
            mu = rx.mu_of(Q)
            A = mpmath.matrix(S, S)
            for i in range(S):
                for j in range(S):
                    if i != j:
                        A[i, j] = mpmath.mpf(float(Q[i, j]))
            for i in range(S):
                A[i, i] = -mpmath.fsum(A[i, j] for j in range(S) if j != i)
            for r, t in ((0.5, 1e-9), (1.0, 0.3), (2.0, 0.77), (1.1, 40.0 / mu), (2.0, rx.edge_length_for(mu, 2.0, rx.MAX_ARGUMENT))):
                P, D1, D2 = (m[0] for m in ref.matrices([r], t))
                tau = mpmath.mpf(r) * mpmath.mpf(t)
                s, y = rx.reduce_argument(rx.argument(mu, r, t))
                if s <= 12:
                    want = mpmath.expm(A * tau, method="taylor")
                else:                                    # (expm's own scaling works at the working precision: square by hand)
                    want = mpmath.expm(A * (tau / 2 ** s), method="taylor")
                    for _ in range(s):
                        want = want * want
                d1 = mpmath.mpf(r) * (A * want)
                d2 = mpmath.mpf(r) * (A * d1)
                own = 2.0 ** s * (c_count(rx.N_REF, S) * 2.0 ** -64 + tail(rx.N_REF, 1.0))
                absA = np.abs(ref.Q.astype(np.float64))
                Pf = P.astype(np.float64)
                scale = [Pf + own, r * absA @ (Pf + own), r * absA @ (r * absA @ (Pf + own))]
                for o, (have, exact) in enumerate(((P, want), (D1, d1), (D2, d2))):
                    for i in range(S):
                        for j in range(S):
                            err = float(abs(mr.to_mpf(have[i, j]) - exact[i, j]))
                            limit = own * scale[o][i, j] * (1 if o == 0 else 2 * S + 5) + 2.0 ** -1074
                            worst = max(worst, err / limit)
                            assert err <= limit, (kind, S, r, t, o, i, j, err, limit)
                if kind == "chain" and S == 3:
                    e = mpmath.exp(-tau)
                    closed = (e, tau * e, 1 - e - tau * e)
                    for j in range(3):
                        assert abs(want[0, j] - closed[j]) <= mpmath.mpf(10) ** -45 * 2 ** s, (r, t, j)
                        assert float(abs(mr.to_mpf(P[0, j]) - closed[j])) <= own * (float(closed[j]) + own) + 2.0 ** -1074, (r, t, j)
    print("REFERENCE long double against mpmath.expm: worst difference / its own term %.3f" % worst)


# ---- D. agreement with the eigen paths -------------------------------------------------------------------------------------------------
LENGTHS = (0.0, 1e-3, 0.1, 2.5, 40.0)


def check_against_device_eigen_system(lib, S, K):
    """a reversible Q: this call against mbamdSetRateMatrices + beagleUpdateTransitionMatrices (the single-precision engine's)"""
    rng = np.random.default_rng(67 + S)
    Q, pi = rx.reversible_q(rng, S)
    rates = mr.category_rates(rng, K)
    ref = rx.RateExponentialReference(Q)
    mu, n = rx.mu_of(Q), len(LENGTHS)
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 2 * n, K, 1, preference_flags=preference(False))
    try:
        inst.set_category_rates(rates)
        inst.set_rate_matrices(0, Q[None], pi)
        inst.update_transition_matrices(0, list(range(n)), LENGTHS)
        inst.update_transition_matrices_from_rate_matrix(Q, list(range(n, 2 * n)), LENGTHS)
        held = mr.MatrixReference(*inst.get_eigen_decomposition(0))
        worst = 0.0
        for u, t in enumerate(LENGTHS):
            eig, own = inst.get_transition_matrix(u), inst.get_transition_matrix(n + u)
            X, W, _ = held.matrices(rates, t, 0)
            P = ref.matrices(rates, t)[0]
            for k in range(K):
                margin = (bounds(ref, mu, rates[k], t, P[k], False)[0][0] + rounding_stored(P[k], False) +
                          1.01 * U64 * W[k] + 2.0 ** -1000 + rounding_stored(X[k], False))
                ratio = float((np.abs(own[k] - eig[k]) / margin).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (S, K, t, k, ratio)
        print("%s AGAINST THE DEVICE EIGEN-SYSTEM of a reversible Q: worst difference / margin %.3f" % (tag(S, K, False), worst))
    finally:
        inst.finalize()


def check_against_complex_eigen_system(lib, S, K, double_precision):
    """the one-way cycle: this call against a complex instance fed numpy's eigen-system of the same Q"""
    dbl = double_precision
    Q = rx.cycle_q(S, rate=1.0)
    es = mbmodel.eigen_general(Q)
    rates = mr.category_rates(np.random.default_rng(71 + S), K)
    ref = rx.RateExponentialReference(Q)
    held = cr.ComplexMatrixReference(es.evec, es.ivec, es.eval, es.imag)
    mu, n = rx.mu_of(Q), len(LENGTHS)
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 2 * n, K, 1, preference_flags=preference(dbl), requirement_flags=bg.BEAGLE_FLAG_EIGEN_COMPLEX)
    try:
        assert inst.details.flags & bg.BEAGLE_FLAG_EIGEN_COMPLEX
        inst.set_category_rates(rates)
        inst.set_eigen_decomposition(0, es.evec, es.ivec, np.concatenate([es.eval, es.imag]))
        inst.update_transition_matrices(0, list(range(n)), LENGTHS)
        inst.update_transition_matrices_from_rate_matrix(Q, list(range(n, 2 * n)), LENGTHS)
        worst = 0.0
        for u, t in enumerate(LENGTHS):
            eig, own = inst.get_transition_matrix(u), inst.get_transition_matrix(n + u)
            X, W, _ = held.matrices(rates, t, 0)
            P = ref.matrices(rates, t)[0]
            for k in range(K):
                margin = (bounds(ref, mu, rates[k], t, P[k], dbl)[0][0] + rounding_stored(P[k], dbl) +
                          1.01 * U64 * W[k] + 2.0 ** -1000 + rounding_stored(X[k], dbl))
                ratio = float((np.abs(own[k] - eig[k]) / margin).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (S, K, dbl, t, k, ratio)
        print("%s AGAINST THE COMPLEX EIGEN-SYSTEM of the one-way cycle: worst difference / margin %.3f" % (tag(S, K, dbl), worst))
    finally:
        inst.finalize()


@pytest.mark.parametrize("S", [4, 5, 20, 61])
def test_against_device_eigen_system_on_emulation(emu, S):
    check_against_device_eigen_system(emu, S, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 5, 20, 61])
def test_against_device_eigen_system(gpu, S):
    check_against_device_eigen_system(gpu, S, 4)


COMPLEX_CASES = [pytest.param(S, dbl, id="%s-%d" % ("fp64" if dbl else "fp32", S)) for dbl in (False, True) for S in (4, 5, 20)]


@pytest.mark.parametrize("S,double_precision", COMPLEX_CASES)
def test_against_complex_eigen_system_on_emulation(emu, S, double_precision):
    check_against_complex_eigen_system(emu, S, 4, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,double_precision", COMPLEX_CASES)
def test_against_complex_eigen_system(gpu, S, double_precision):
    check_against_complex_eigen_system(gpu, S, 4, double_precision)


# ---- E. every stored copy --------------------------------------------------------------------------------------------------------------
class RateMatrixDivision(lk.BeagleDivision):
    """A division whose transition matrices come from the new call (`made`: the values read back are kept in `values`) or are those
    values given to beagleSetTransitionMatrix (`set`)."""

    def __init__(self, div, lib, mode, q, values=None, **kw):
        self.mode, self.q, self.values = mode, q, ({} if values is None else values)
        super().__init__(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, **kw)

    def TreeTiProbs_Beagle(self, chain):
        super().TreeTiProbs_Beagle(chain)
        t, inst = self.div.tree, self.inst
        nodes = [p for p in t.all_down_pass if self.upDateTi[chain][p]]
        own = [self.tiProbsIndex[chain][p] for p in nodes]
        if self.mode == "made":
            inst.update_transition_matrices_from_rate_matrix(self.q, own, [min(max(t.length[p], lk.BRLENS_MIN), lk.BRLENS_MAX) for p in nodes])
            for p, m in zip(nodes, own):
                self.values[p] = inst.get_transition_matrix(m)
        else:
            for p, m in zip(nodes, own):
                inst.set_transition_matrix(m, self.values[p])


def results_of(bd):
    t, inst = bd.div.tree, bd.inst
    out = [np.float64(bd.LogLike(0)), inst.get_site_log_likelihoods().copy()]
    bd.AcceptMove(0)
    return out + [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]


def check_copies(lib, monkeypatch, S, double_precision, switches, layout):
    div = tree_division(S)
    q = rx.rate_matrix("sparse", S)
    runs = {}
    for k in switches:
        monkeypatch.setenv(k, "1")
    try:
        made = RateMatrixDivision(div, lib, "made", q, double_precision=double_precision)
        try:
            name = made.inst.details.implName.decode()
            assert layout in name, name
            runs["made"] = results_of(made)
        finally:
            made.finalize()
        twin = RateMatrixDivision(div, lib, "set", q, values=made.values, double_precision=double_precision)
        try:
            runs["set"] = results_of(twin)
        finally:
            twin.finalize()
    finally:
        for k in switches:
            monkeypatch.delenv(k, raising=False)
    assert len(made.values) == 2 * NTAXA - 3 and all(np.isfinite(x).all() for x in runs["made"]) and len(runs["made"]) == len(runs["set"])
    for n, (x, y) in enumerate(zip(runs["made"], runs["set"])):
        assert np.array_equal(x, y), (tag(S, NCAT, double_precision), "item %d" % n, np.argwhere(np.asarray(x) != np.asarray(y))[:4].tolist())
    print("%s COPIES: lnL %.6f, %d arrays bit-identical on device-made and host-set matrices; %s" %
          (tag(S, NCAT, double_precision), runs["made"][0], len(runs["made"]), name.split(": ", 1)[-1]))


#              four states on the walk, 20 states on k_walkg, 5 states on the level kernels (the MFMA A-operand image); both engines
COPY_CASES = [pytest.param(4, False, (), "4-state tree-walk kernels", id="fp32-4"),
              pytest.param(20, False, (), "general-state tree-walk kernels", id="fp32-20"),
              pytest.param(5, False, ("MBAMD_NO_WALKG",), "general-state MFMA", id="fp32-5-levels"),
              pytest.param(4, True, (), "double-precision", id="fp64-4"), pytest.param(20, True, (), "double-precision", id="fp64-20"),
              pytest.param(5, True, (), "double-precision", id="fp64-5")]


@pytest.mark.parametrize("S,double_precision,switches,layout", COPY_CASES)
def test_copies_on_emulation(emu, monkeypatch, S, double_precision, switches, layout):
    check_copies(emu, monkeypatch, S, double_precision, switches, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("S,double_precision,switches,layout", COPY_CASES)
def test_copies(gpu, monkeypatch, S, double_precision, switches, layout):
    check_copies(gpu, monkeypatch, S, double_precision, switches, layout)


# ---- F. end to end ---------------------------------------------------------------------------------------------------------------------
def check_tree(lib, double_precision, seed=73):
    """Six tips under the defective three-state chain, two categories, 70 patterns: every site's log-likelihood against pruning with
    the long-double P.  m operations, each within B_op of its exact value on its operands, two matrices per operation each within
    e_P (relative: the largest E_P / P over the non-zero entries, the stored rounding in it) -- relative errors of non-negative terms
    add along the tree: B = ((1 + B_op) (1 + e_P)^2)^m (1 + B_root) - 1."""
    dbl = double_precision
    S, K, P, ntips = 3, 2, 70, 6
    rng = np.random.default_rng(seed)
    Q = rx.chain_q(S)
    ref, mu = rx.reference_for("chain", S), rx.mu_of(Q)
    rates = np.array([0.4, 1.7])
    ops = random_tree(rng, ntips)
    nint, nodes = len(ops), ntips + len(ops)
    root = ops[-1][0]
    lengths = (0.05 + 1.5 * rng.random(nodes - 1)).tolist()
    states = [rng.integers(0, S, size=P).astype(np.int32) for _ in range(ntips)]
    w, f = vector(rng, K, dbl), vector(rng, S, dbl)
    pw = 1.0 + (np.arange(P) % 3)
    wide, e_p = [], 0.0
    for t in lengths:
        X = ref.matrices(rates, t)[0]
        wide.append(X)
        for k in range(K):
            E = bounds(ref, mu, rates[k], t, X[k], dbl)[0][0] + rounding_stored(X[k], dbl)
            live = mr.to_float(X[k]) > 0
            e_p = max(e_p, float((E[live] / mr.to_float(X[k])[live]).max()))
    wide.append(wide[0])                                     # (the root has no branch)
    B = ((1.0 + operation_bound(S, dbl)) * (1.0 + e_p) ** 2) ** nint * (1.0 + root_bound(S, K, dbl)) - 1.0
    inst = bg.BeagleInstance(lib, ntips, nint, ntips, S, P, 1, nodes, K, nint + 1, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        inst.set_category_rates(rates)
        inst.update_transition_matrices_from_rate_matrix(Q, list(range(nodes - 1)), lengths)
        for n in range(ntips):
            inst.set_tip_states(n, states[n])
        inst.set_category_weights(0, w)
        inst.set_state_frequencies(0, f)
        inst.set_pattern_weights(pw)
        inst.reset_scale_factors(nint)
        inst.update_partials(np.array([[d, d - ntips, NONE, a, a, b, b] for d, a, b in ops], dtype=np.int32), nint)
        rc, lnl = inst.calculate_root_log_likelihoods([root], [0], [0], [nint])
        sources = {n: REF.widen(dense_tip(states[n], S, K)) for n in range(ntips)}
        L = REF.root(REF.widen(w), REF.widen(f), REF.prune(ops, sources, wide)[root])
        assert (REF.to_float(L) > 0).all()
        worst = _check_sites(inst, "6 tips, defective chain", rc, lnl, L, B, pw, tag(S, K, dbl))
        print("%s TREE under the defective chain: lnL %.9f, e_P %.3g, worst site error / bound %.3f; %s" % (tag(S, K, dbl), lnl, e_p, worst, name.split(": ", 1)[-1]))
    finally:
        inst.finalize()


@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
def test_tree_on_emulation(emu, double_precision):
    check_tree(emu, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
def test_tree(gpu, double_precision):
    check_tree(gpu, double_precision)


# ---- G. lists --------------------------------------------------------------------------------------------------------------------------
def check_lists(lib, S, K, double_precision):
    """Calls of 1, 3 and 70 entries, the last with both derivative lists: every entry bit for bit what a call of its own gives (the
    table's entries and arguments are found where they lie), the 70 within the bound; either derivative list alone; a result that
    a queued beagleUpdateTransitionMatrices still names."""
    dbl = double_precision
    rng = np.random.default_rng(79 + S)
    Q = rx.rate_matrix("sparse", S)
    ref, mu = rx.reference_for("sparse", S), rx.mu_of(Q)
    rates = rates_of(K)
    big = 70
    lengths = np.concatenate([[0.0], np.exp(rng.uniform(np.log(1e-4), np.log(300.0 / mu), size=big - 1))])
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 3 * big + 12, K, 1, preference_flags=preference(dbl))
    try:
        inst.set_category_rates(rates)
        inst.set_eigen_decomposition(0, *mr.reversible_system(rng, S, "ordinary"))
        inst.update_transition_matrices_from_rate_matrix(Q, np.arange(big), lengths, first=big + np.arange(big), second=2 * big + np.arange(big))
        got = [[inst.get_transition_matrix(o * big + u) for u in range(big)] for o in range(3)]
        worst = 0.0
        for u in range(big):
            wide = ref.matrices(rates, lengths[u])
            for k in range(K):
                E, _ = bounds(ref, mu, rates[k], lengths[u], wide[0][k], dbl)
                for o in range(3):
                    ratio = float((mr.error(got[o][u][k], wide[o][k]) / (E[o] + rounding_stored(wide[o][k], dbl))).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (tag(S, K, dbl), "entry %d" % u, k, o, ratio)
        a, b, c = 3 * big, 3 * big + 4, 3 * big + 8
        for u in (0, 1, 37, big - 1):                    # one entry a call
            inst.update_transition_matrices_from_rate_matrix(Q, [a], [lengths[u]], first=[b], second=[c])
            for o, m in enumerate((a, b, c)):
                assert np.array_equal(inst.get_transition_matrix(m), got[o][u]), ("one entry", u, o)
        pick = [5, 69, 20]                               # three entries; either derivative list alone
        inst.update_transition_matrices_from_rate_matrix(Q, [a, a + 1, a + 2], lengths[pick])
        inst.update_transition_matrices_from_rate_matrix(Q, [a + 3, b, b + 1], lengths[pick], first=[b + 2, b + 3, c])
        inst.update_transition_matrices_from_rate_matrix(Q, [c + 1, c + 2, c + 3], lengths[pick], second=[a + 3, b, b + 1])
        for n, u in enumerate(pick):
            assert np.array_equal(inst.get_transition_matrix(a + n), got[0][u]), ("three entries", u)
            assert np.array_equal(inst.get_transition_matrix((b + 2, b + 3, c)[n]), got[1][u]), ("first alone", u)
            assert np.array_equal(inst.get_transition_matrix((c + 1, c + 2, c + 3)[n]), got[0][u]), ("second alone: P", u)
            assert np.array_equal(inst.get_transition_matrix((a + 3, b, b + 1)[n]), got[2][u]), ("second alone", u)
        # a queued update of the result runs first: this call's matrix stays
        inst.update_transition_matrices(0, [a], [0.2])
        inst.update_transition_matrices_from_rate_matrix(Q, [a], [lengths[37]])
        assert np.array_equal(inst.get_transition_matrix(a), got[0][37]), "queued update of the result"
        print("%s LISTS of 1, 3 and %d entries: worst error / bound %.3f; single calls bit-identical" % (tag(S, K, dbl), big, worst))
    finally:
        inst.finalize()


LIST_CASES = [pytest.param(4, 4, False, id="fp32-4"), pytest.param(5, 4, False, id="fp32-5"), pytest.param(20, 4, False, id="fp32-20"),
              pytest.param(4, 4, True, id="fp64-4"), pytest.param(5, 1, True, id="fp64-5"), pytest.param(20, 4, True, id="fp64-20")]


@pytest.mark.parametrize("S,K,double_precision", LIST_CASES)
def test_lists_on_emulation(emu, S, K, double_precision):
    check_lists(emu, S, K, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision", LIST_CASES)
def test_lists(gpu, S, K, double_precision):
    check_lists(gpu, S, K, double_precision)


# ---- H. pattern shards -----------------------------------------------------------------------------------------------------------------
def check_shards(lib, monkeypatch, S):
    """MBAMD_SHARD=2 at 130 patterns (two children, each with its own matrix buffers): the matrices read back and the per-site lnL of
    the tree -- computed by each child from ITS matrices -- bit-equal with the plain instance's"""
    div = tree_division(S)
    q = rx.rate_matrix("dense", S)
    seen = {}
    for shards in (None, "2"):
        monkeypatch.delenv("MBAMD_SHARD", raising=False)
        if shards:
            monkeypatch.setenv("MBAMD_SHARD", shards)
        try:
            bd = RateMatrixDivision(div, lib, "made", q)
        finally:
            monkeypatch.delenv("MBAMD_SHARD", raising=False)
        try:
            assert bd.inst.child_count() == (2 if shards else 1)
            lnl = bd.LogLike(0)
            seen[shards] = (lnl, bd.inst.get_site_log_likelihoods().copy(), dict(bd.values))
        finally:
            bd.finalize()
    assert np.isfinite(seen[None][0]) and np.array_equal(seen[None][1], seen["2"][1])
    for p, m in seen[None][2].items():
        assert np.array_equal(m, seen["2"][2][p]), p
    print("%s SHARDS: per-site lnL of 2 children bit-equal with the plain instance's (lnL %.6f)" % (tag(S, NCAT, False), seen[None][0]))


@pytest.mark.parametrize("S", [4, 20])
def test_shards_on_emulation(emu, monkeypatch, S):
    check_shards(emu, monkeypatch, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 20])
def test_shards(gpu, monkeypatch, S):
    check_shards(gpu, monkeypatch, S)


# ---- I. refusals -----------------------------------------------------------------------------------------------------------------------
def ints(*v):
    return (C.c_int * len(v))(*v)


def dbls(v):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    return (C.c_double * len(v))(*v.tolist())


def check_refusals(lib, S):
    """Every refusal on a single- and a double-precision instance: its status, and every matrix buffer bit for bit as it was -- the
    bad value stands LAST, behind entries that would have written.  Then a two-partition instance."""
    K, M = 2, 8
    call = lib.lib.mbamdUpdateTransitionMatricesFromRateMatrix
    rng = np.random.default_rng(83 + S)
    given = [stored(rng.standard_normal((K, S, S)), False) for _ in range(M)]
    Q = rx.rate_matrix("sparse", S)
    mu = rx.mu_of(Q)
    rates = np.array([0.25, 2.0])
    good_q, good_t = dbls(Q), dbls([0.1, 0.2])
    p, d1, d2 = ints(0, 1), ints(2, 3), ints(4, 5)
    null_i, null_d = C.cast(None, _ip), C.cast(None, _dp)

    def with_entry(i, j, v):
        bad = Q.copy()
        bad[i, j] = v
        return dbls(bad)
    over = float(np.nextafter(rx.edge_length_for(mu, 2.0, rx.MAX_ARGUMENT), np.inf))
    assert rx.argument(mu, 2.0, over) > rx.MAX_ARGUMENT
    off_diagonal = Q.copy()
    off_diagonal[S - 1, S - 1] += 1e-6
    refused = {
        "a negative off-diagonal": lambda i: call(i, with_entry(S - 1, 0, -1e-3), p, d1, d2, good_t, 2),
        "a NaN entry": lambda i: call(i, with_entry(S - 1, S - 2, np.nan), p, d1, d2, good_t, 2),
        "an infinite entry": lambda i: call(i, with_entry(0, 1, np.inf), p, d1, d2, good_t, 2),
        "a diagonal off by 1e-6": lambda i: call(i, dbls(off_diagonal), p, d1, d2, good_t, 2),
        "a negative t": lambda i: call(i, good_q, p, d1, d2, dbls([0.1, -1e-9]), 2),
        "an infinite t": lambda i: call(i, good_q, p, d1, d2, dbls([0.1, np.inf]), 2),
        "a NaN t": lambda i: call(i, good_q, p, d1, d2, dbls([0.1, np.nan]), 2),
        "mu r t just above 2^20": lambda i: call(i, good_q, p, d1, d2, dbls([0.1, over]), 2),
        "an index twice in one list": lambda i: call(i, good_q, ints(0, 0), d1, d2, good_t, 2),
        "an index twice among the lists": lambda i: call(i, good_q, p, d1, ints(4, 1), good_t, 2),
        "an index too large": lambda i: call(i, good_q, ints(0, M), d1, d2, good_t, 2),
        "a negative index": lambda i: call(i, good_q, p, ints(2, -1), d2, good_t, 2),
        "a second-derivative index too large": lambda i: call(i, good_q, p, d1, ints(4, M + 3), good_t, 2),
        "rateMatrix NULL": lambda i: call(i, null_d, p, d1, d2, good_t, 2),
        "probabilityIndices NULL": lambda i: call(i, good_q, null_i, d1, d2, good_t, 2),
        "edgeLengths NULL": lambda i: call(i, good_q, p, d1, d2, null_d, 2),
        "a negative count": lambda i: call(i, good_q, p, d1, d2, good_t, -1),
    }
    pair = [bg.BeagleInstance(lib, 2, 3, 2, S, 130, 1, M, K, 1, preference_flags=preference(dbl)) for dbl in (False, True)]
    try:
        assert "double-precision" not in pair[0].details.implName.decode() and "double-precision" in pair[1].details.implName.decode()
        for inst in pair:
            inst.set_category_rates(rates)
            for n in range(M):
                inst.set_transition_matrix(n, given[n])
        for what, refuse in refused.items():
            texts = []
            for inst in pair:
                rc = refuse(inst.id)
                assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE, (what, rc, lib.last_error())
                texts.append(lib.last_error())
                for n in range(M):
                    assert np.array_equal(inst.get_transition_matrix(n), given[n]), (what, "matrix %d changed" % n)
            assert texts[0] == texts[1] and "mbamdUpdateTransitionMatricesFromRateMatrix" in texts[0], (what, texts)
        for inst in pair:
            assert call(inst.id, null_d, null_i, null_i, null_i, null_d, 0) == bg.BEAGLE_SUCCESS, "count 0"
            # (the largest admitted argument is accepted)
            assert call(inst.id, good_q, ints(6), null_i, null_i, dbls([rx.edge_length_for(mu, 2.0, rx.MAX_ARGUMENT)]), 1) == bg.BEAGLE_SUCCESS
            assert not np.array_equal(inst.get_transition_matrix(6), given[6])
            # a Q of all zeros: identities and zero derivatives
            assert call(inst.id, dbls(np.zeros((S, S))), ints(5), ints(6), ints(7), dbls([3.0]), 1) == bg.BEAGLE_SUCCESS
            assert np.array_equal(inst.get_transition_matrix(5), np.tile(np.eye(S), (K, 1, 1))), "a Q of all zeros"
            assert not inst.get_transition_matrix(6).any() and not inst.get_transition_matrix(7).any(), "a Q of all zeros: derivatives"
            inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
            assert inst.child_count() == 2
            for n in range(M):
                inst.set_transition_matrix(n, given[n])
            rc = call(inst.id, good_q, p, d1, d2, good_t, 2)
            assert rc == bg.BEAGLE_ERROR_NO_IMPLEMENTATION, ("a multi-partition instance", rc)
            for n in range(M):
                assert np.array_equal(inst.get_transition_matrix(n), given[n]), ("a multi-partition instance", "matrix %d changed" % n)
        print("%d states REFUSALS: %d refused calls, the same text on both engines, no matrix changed; a two-partition instance refused" % (S, len(refused)))
    finally:
        for inst in pair:
            inst.finalize()


def test_host_side_under_sanitizers(tmp_path):
    """What the call checks and the table it sends are plain C++ (mbamd_rate_exponential_table.h): tools/rate_exponential_host_check.cpp
    gives them every refusal and a valid list as a stand-alone program built with the address and undefined-behaviour sanitizers.
    No engine, no device."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rate_exponential_host_check")
    subprocess.check_call([build_emu.host_compiler(), "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "mrbayes_amd", "csrc"), os.path.join(root, "tools", "rate_exponential_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and "ok: 0 wrong answers" in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])


@pytest.mark.parametrize("S", [4, 5, 20])
def test_refusals_on_emulation(emu, S):
    check_refusals(emu, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 5, 20])
def test_refusals(gpu, S):
    check_refusals(gpu, S)
