"""The device eigen-solver (k_eigen_reversible, launched by Instance::setRateMatrices behind mbamdSetRateMatrices[From]) against bounds
derived from its code: the decomposition itself in double, read back through mbamdGetEigenDecomposition, and the single-precision
transition matrices made from it against exp(Q t).

  * CPU (`not gpu`): the host-emulation build of the same sources.  Its mbd_jacobi_rotation (tests/hostemu/mbamd_dev_base.h) is the
    textbook formula in exact divisions;
  * GPU (`gpu`): the product library on a MI355X, whose mbd_jacobi_rotation (csrc/device/mbamd_dev_base.h) forms the angle from the
    hardware's approximate fp64 reciprocal and square root and Newton-refines the normalisation only.  A GPU ratio above 1 with the
    emulation inside the bound points there.

The reference is tests/eigen_reference.py: B = D Q D^-1 in the wide type from the very doubles the solver is given, numpy.linalg.eigh
and the spectral sum of tests/matrix_reference.py for exp(Q t); test_reference_against_mpmath holds it to 2^-45 sqrt(pi_j / pi_i).

NOTATION.  S states, n = S rounded up to even (an odd S gets a dummy index), u = 2^-53, |.| the Frobenius norm, |.|_2 the spectral one.
The kernel keeps A (n x n, starts as B or V0^T B V0) and V (starts as I or V0); a STEP applies n / 2 disjoint rotations J: A <- J^T A J,
V <- V J; a sweep is n - 1 steps; the launch passes a cap of 30 sweeps.  w = the number of warm calls since the last cold start behind a
buffer (Instance::eigenWarm: a warm call stores w + 1, the call that finds 64 starts cold again, so w <= 64).  L = diag(lambda).

OMEGA, the loss of orthogonality:  |V^T V - I| <= omega(w) = (1 + w) omega_1,   omega_1 = 1.01 * 30 (n - 1) (6 sqrt(2) + 10) u sqrt(n).
  One step.  V' = V J + dV and, with G = V^T V:  G' - I = J^T (G - I) J + (J^T J - I) + dV^T V J + (V J)^T dV + dV^T dV.
  * the normalisation of (c, s), nu = 10 u.  w = fl(1 + t t) is off by 2 u relative (the square, the sum).  The device takes
    c0 = rsq(w) and two Newton steps c <- c (1.5 - 0.5 w c c): a relative error e of c becomes 1.5 e^2, so ANY c0 within 2^-20 (the
    ISA documents v_rsq_f64 far tighter) leaves 1.5 (1.5 2^-40)^2 < 2^-78 of algorithmic error after two -- THIS IS THE ASSUMPTION the
    bound rests on: the angle t may be as rough as the hardware makes it, c and s = t c are normalised against the same w.  The last
    step rounds three times where it matters (0.5 w c c twice, an absolute u of 0.5; 1.5 - h once; the product once): c = (1 + 3 u) /
    sqrt(w), c^2 w = 1 + 6 u; s = fl(t c) adds u to s, 2 u to s^2; w against 1 + t^2 another 2 u:  |c^2 + s^2 - 1| <= 10 u.  (The
    emulation: sqrt, division -- c^2 w = 1 + 4 u, 8 u in all.)  J^T J = (c^2 + s^2) I on each pair exactly (its off-diagonal c s - s c
    is zero in exact arithmetic of the stored c, s), so |J^T J - I| <= nu sqrt(n) and |J^T X J| <= (1 + nu) |X|;
  * the column update V[k,p] = c v0 - s v1, V[k,q] = s v0 + c v1: two products and a sum, THREE roundings, |dV[k,p]| <= 3 u (|c v0| +
    |s v1|) (contraction to a fused multiply-add only removes one).  Over a pair of columns (|c| a + |s| b)^2 + (|s| a + |c| b)^2 <=
    2 (a^2 + b^2): |dV| <= 3 sqrt(2) u |V| = 3 sqrt(2) u sqrt(n) to first order, and the two cross terms are 2 |dV| |V J|_2.
  So |G - I| grows by at most (6 sqrt(2) + 10) u sqrt(n) per step, there are at most 30 (n - 1) steps per call, and a warm call starts
  from the V its source left (the dummy row and column of an odd S are loaded as the identity: exact): (1 + w) calls.  1 % for the
  second-order terms.  The assertion holds the Frobenius norm to omega, hence every entry.

RHO, the residual:  |B V - V L| <= rho, and |B Q - Q L| <= rho for the orthogonal Q nearest to V (|V - Q|_2 <= |G - I|_2 <= omega: the
polar factor), which is what the eigenvalue and the matrix assertions use.
  rho = 1.01 ((1e-10 + 3 omega) |L| + u |B| (S + 8 + [mode 1] 1040 + [warm] 2 n sqrt(n) + 30 (n - 1) (12 + 6 sqrt(2) sqrt(n))))
  * the stopping criterion.  The loop ends when the off-diagonal sum of squares o4 <= 1e-20 d4, the diagonal's: |off(A)| <= 1e-10 |L|,
    lambda being A's diagonal (both sums of at most n^2 non-negative terms: a relative n^2 u, inside the 1 %).  This term dominates
    by four orders of magnitude: what the assertion catches is a system that left the loop at the sweep cap, unconverged;
  * A against V^T B V, the invariant the rotations keep up to rounding -- a non-orthogonal J is no error here, A' = J^T A J and
    V' = V J keep A = V^T B V whatever J is:
      - forming B: two square roots, a product, a division, the sum (and, mode 1, two more products) on every off-diagonal entry, at
        most 9 u |b_ij|; the diagonal is minus a running sum of S - 1 terms, each with up to two roundings of its own: (S + 2) u
        |b_ii|.  (S + 8) u |B| covers both.  Mode 1 scales every entry by 1 / tot, tot a sum of positive terms that thread 0 adds
        one after the other over up to 1 024 partial sums, each a short sum itself: 1 040 u relative at most;
      - the warm transform V0^T (B V0): two sums of n terms, n u sum |a| |v| each, and | |A| |V| | <= |A| sqrt(n): 2 n sqrt(n) u |B|;
      - a step: every entry of A passes two 2 x 2 combinations, three roundings each, 6 u (|c| + |s|)^2 <= 12 u of its block's
        magnitudes: 12 u |A|; and the step's dV moves V^T B V by 2 |dV| |B|_2 <= 6 sqrt(2) u sqrt(n) |B|.  At most 30 (n - 1) steps;
  * from A = V^T B V + E to the residual: V^T (B V - V L) = off(A) - E + (I - G) L, and |V^-1|_2 <= 1 / (1 - omega): omega |L| once;
    from V to Q: (B Q - Q L) - (B V - V L) = B (Q - V) - (Q - V) L, 2 omega |B| = 2 omega |L| (B is symmetric: |B| is the norm of
    its eigenvalues, and |L| is that to within rho).  3 omega |L| in all.

PART A asserts, on every decomposition: everything finite; the two above; U[i,s] pi_i = U^-1[s,i] to 4.04 u (U = fl(V / d_i), U^-1 =
fl(V d_i), d_i = fl(sqrt(pi_i)): one division, one product, the root twice -- 4 u); the sorted lambda against numpy's eigvalsh(B) within
rho + 64 u |B| (Hoffman-Wielandt: sqrt(sum (mu_i - lambda_i)^2) <= |B Q - Q L|; 64 u |B| for eigvalsh's own backward error and
B's rounding to double); exactly one |lambda| <= rho, every other one below -rho.

PART B, the single-precision matrices against X = D^-1 (r B)^o exp(B r t) D of the TRUE B, tau = r_k t, E_b = rho + 2 omega sqrt(n) |B|:
    |got - X| <= 2^-24 |X| + 2^-150 + 1.01 u (W + 4 mag)
                 + sqrt(pi_j / pi_i) (tau E_b e^(tau E_b) + 2 omega sqrt(n) (1 + omega sqrt(n)) e^(tau rho))                    o = 0
                 + sqrt(pi_j / pi_i) r_k (E_b (1 + tau |B|) e^(tau E_b) + 2 omega sqrt(n) (1 + omega sqrt(n)) (|B| + rho) e^(tau rho))   o = 1
  * the first three terms are test_matrix_bounds.py's: the kernels' arithmetic on the doubles [U | U^-1 | lambda] they read, which
    here are the ones the accessor returned (W and mag from THAT system); 4 u mag more because U and U^-1 are D^-1 V and V^T D only
    to the 4 u of part A, and the reference knows D exactly;
  * the last term.  got's exact counterpart is D^-1 M D, M = V f(L) V^T, f(x) = (r x)^o e^(x tau).  Split V = Q + R, Q orthogonal,
    |R|_2 <= omega (taken as omega sqrt(n) here, the entry-wise reading: larger, never smaller).  Q f(L) Q^T = f(B + E) with
    E = Q L Q^T - B, |E| = |B Q - Q L| <= rho (taken as E_b = rho + 2 omega sqrt(n) |B|, the price of the move from V to Q counted
    once more: larger).  For symmetric B without a positive eigenvalue |e^(B s)|_2 <= 1 and |e^((B + E) s)|_2 <= e^(s |E|), so from
    e^((B+E) tau) - e^(B tau) = int_0^tau e^(B (tau - s)) E e^((B + E) s) ds:  |e^((B+E) tau) - e^(B tau)|_2 <= tau |E| e^(tau |E|).
    The remainder R f Q^T + Q f R^T + R f R^T is at most (2 |R| + |R|^2) max |f(lambda)|, and no computed lambda exceeds rho:
    max e^(lambda tau) <= e^(rho tau).  Order 1: r (B + E) e^((B+E) tau) - r B e^(B tau) = r E e^((B+E) tau) + r B (e^((B+E) tau) -
    e^(B tau)), one more factor |B|, and max |r lambda e^(lambda tau)| <= r (|B| + rho) e^(rho tau).  An element (i, j) of D^-1 (.) D
    is the element of (.) times d_j / d_i.
  Order 1 is asked at t = 0, where it returns Q itself: the sharpest single look at U L U^-1.

Parts C (warm starts in chains of 70 calls over three buffers, mixed warm and cold jobs, a far move, in place, refusals) and D (the
256-thread launch at more than 32 states, the device-copy branch of 128 systems in one call) run the same assertions.  Each check
prints the worst error / bound it met and the measured |B V - V L| / |B| (pytest -s shows them).
"""
import math

import mpmath
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from tests import eigen_reference as er
from tests import matrix_reference as mr
from tests.operation_reference import LD, LONGDOUBLE_QUALIFIES
from tests.test_matrix_bounds import emu, gpu                      # noqa: F401  (the fixtures)
from tests.test_operation_bounds import expected_layout, preference

U64 = 2.0 ** -53
SWEEP_CAP = 30


def even(S):
    return (S + 1) & ~1


def omega_of(S, w):
    n = even(S)
    return (1 + w) * 1.01 * SWEEP_CAP * (n - 1) * (6.0 * math.sqrt(2.0) + 10.0) * U64 * math.sqrt(n)


def rho_of(S, norm_b, norm_lam, mode, warm, w):
    n = even(S)
    roundings = S + 8 + (1040 if mode == 1 else 0) + (2.0 * n * math.sqrt(n) if warm else 0.0) + \
        SWEEP_CAP * (n - 1) * (12.0 + 6.0 * math.sqrt(2.0) * math.sqrt(n))
    return 1.01 * ((1e-10 + 3.0 * omega_of(S, w)) * norm_lam + U64 * norm_b * roundings)


class Worst:
    """the worst error / bound of one test, and the largest measured residual / |B|"""

    def __init__(self, label):
        self.label, self.ratio, self.residual = label, {}, 0.0

    def hold(self, what, value, bound, context):
        r = value / bound
        self.ratio[what] = max(self.ratio.get(what, 0.0), r)
        assert r <= 1.0, (self.label, what, context, "error %.3e" % value, "bound %.3e" % bound, "ratio %.3f" % r)

    def report(self):
        print("%s worst error / bound: %s; largest |BV - VL| / |B| %.2e" %
              (self.label, ", ".join("%s %.3g" % kv for kv in self.ratio.items()), self.residual))


def check_decomposition(worst, B, pi, system, mode, warm, w, context):
    """part A's assertions on one decomposition (U, U^-1, lambda, V) of the wide matrix B; returns (rho, omega, |B|)"""
    U, Ui, lam, V = system
    S = len(pi)
    for a, name in zip(system, ("U", "U^-1", "lambda", "V")):
        assert np.isfinite(a).all(), (worst.label, context, name, "not finite")
    with mpmath.workprec(er.PREC):
        norm_b, norm_lam = er.fro(B), float(np.sqrt((lam * lam).sum()))
        omega, rho = omega_of(S, w), rho_of(S, norm_b, norm_lam, mode, warm, w)
        Vw, lw = er.wide(V), er.wide(lam)
        residual = er.fro(B.dot(Vw) - Vw * lw[None, :])
        gram = Vw.T.dot(Vw) - er.wide(np.eye(S))
        worst.residual = max(worst.residual, residual / norm_b)
        worst.hold("residual", residual, rho, context)
        worst.hold("orthogonality", er.fro(gram), omega, context)
        pair = er.narrow(abs(er.wide(U) * er.wide(pi)[:, None] - er.wide(Ui).T))
        room = 4.04 * U64 * np.abs(Ui.T)
        assert ((pair <= room) | (pair == 0)).all(), (worst.label, context, "U pi against U^-1", float((pair / np.maximum(room, 1e-300)).max()))
        worst.ratio["U pi = U^-1"] = max(worst.ratio.get("U pi = U^-1", 0.0), float((pair / np.maximum(room, 1e-300)).max()))
    b = er.narrow(B)
    mu = np.linalg.eigvalsh(0.5 * (b + b.T))
    worst.hold("eigenvalues", float(np.abs(np.sort(lam) - mu).max()), rho + 64.0 * U64 * norm_b, context)
    stationary = np.abs(lam) <= rho
    assert stationary.sum() == 1 and (lam[~stationary] < -rho).all(), (worst.label, context, "one zero eigenvalue, the rest negative", np.sort(lam)[-3:], rho)
    return rho, omega, norm_b


def matrix_ratio(got, B, pi, system, rates, t, order, rho, omega, norm_b):
    """max over the elements of |got - X| / part B's bound"""
    S, n = len(pi), even(len(pi))
    X = er.transition(B, pi, rates, t, order)
    _, W, mag = mr.MatrixReference(*system[:3]).matrices(np.asarray(rates, dtype=np.float64), t, order)
    g = np.sqrt(pi[None, :] / pi[:, None])
    r = np.asarray(rates, dtype=np.float64)
    tau = r * t
    rem = 2.0 * omega * math.sqrt(n) * (1.0 + omega * math.sqrt(n))
    eb = rho + 2.0 * omega * math.sqrt(n) * norm_b
    if order == 0:
        spectral = tau * eb * np.exp(tau * eb) + rem * np.exp(tau * rho)
    else:
        spectral = r * (eb * (1.0 + tau * norm_b) * np.exp(tau * eb) + rem * (norm_b + rho) * np.exp(tau * rho))
    bound = 2.0 ** -24 * np.abs(mr.to_float(X)) + 2.0 ** -150 + 1.01 * U64 * (W + 4.0 * mag) + g[None, :, :] * spectral[:, None, None]
    return float((mr.error(got, X) / bound).max())


def make(lib, S, eigen_buffers, matrices=2, K=1):
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, eigen_buffers, matrices, K, 1, preference_flags=preference(False))
    name = inst.details.implName.decode()
    assert expected_layout(S, K, False) in name, name
    return inst, name.split(": ", 1)[-1]


def given(r, pi, mode):
    """what the solver is handed: the exchangeabilities (mode 1) or the rate matrix made from them in double (mode 0)"""
    return r if mode == 1 else er.rate_matrix(r, pi)


# ---- A. the decomposition in double, cold starts -------------------------------------------------------------------------------------
def check_cold(lib, S, seed=41):
    rng = np.random.default_rng(seed + S)
    jobs = [(kind, r, pi, 0) for kind, r, pi in er.cases(rng, S)]
    jobs += [(kind + ", exchangeabilities", r * 3.7, pi, 1) for kind, r, pi, _ in jobs if kind in ("ordinary", "skewed")]
    inst, name = make(lib, S, len(jobs))
    worst = Worst("%2d states COLD" % S)
    try:
        for e, (kind, r, pi, mode) in enumerate(jobs):
            q = given(r, pi, mode)
            inst.set_rate_matrices(e, q[None], pi, exchangeabilities=(mode == 1))
        for e, (kind, r, pi, mode) in enumerate(jobs):
            check_decomposition(worst, er.symmetrised(given(r, pi, mode), pi, mode), pi, inst.get_eigen_decomposition(e, basis=True), mode, False, 0, kind)
        worst.report()
    finally:
        inst.finalize()
    return worst


#              both sides of the dummy index (2 | 3, 4 | 5), of the 256- and the 1 024-thread launch (32 | 33) and of the LDS maximum (63 | 64)
COLD_STATES = [2, 3, 4, 5, 20, 31, 32, 33, 61, 63, 64]
MATRIX_STATES = [2, 4, 20, 33, 61, 64]
CHAIN_STATES = [4, 20, 61]
if not LONGDOUBLE_QUALIFIES:          # (the mpmath reference: the small shapes)
    COLD_STATES, MATRIX_STATES, CHAIN_STATES = [2, 3, 4, 5], [2, 4], [4]


@pytest.mark.parametrize("S", COLD_STATES)
def test_cold_on_emulation(emu, S):
    check_cold(emu, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", COLD_STATES)
def test_cold(gpu, S):
    check_cold(gpu, S)


def check_accessor(lib, S=5):
    """after beagleSetEigenDecomposition the accessor returns the doubles it was given bit for bit and has no basis to return; the index
    is checked; a double-precision instance has no such call"""
    rng = np.random.default_rng(43)
    inst, _ = make(lib, S, 2)
    try:
        U, Ui, lam = rng.standard_normal((S, S)), rng.standard_normal((S, S)), -rng.random(S)
        inst.set_eigen_decomposition(1, U, Ui, lam)                           # (before any device solve: no bookkeeping yet)
        for a, b in zip(inst.get_eigen_decomposition(1), (U, Ui, lam)):
            assert np.array_equal(a, b)
        with pytest.raises(bg.BeagleError) as err:
            inst.get_eigen_decomposition(1, basis=True)
        assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE
        r, pi = er.one_case(rng, S, "ordinary")
        inst.set_rate_matrices(1, er.rate_matrix(r, pi)[None], pi)
        assert len(inst.get_eigen_decomposition(1, basis=True)) == 4
        inst.set_eigen_decomposition(1, U, Ui, lam)                           # (after one: the basis no longer belongs to the buffer)
        for a, b in zip(inst.get_eigen_decomposition(1), (U, Ui, lam)):
            assert np.array_equal(a, b)
        for index, basis in ((1, True), (0, True), (2, False), (-1, False)):
            with pytest.raises(bg.BeagleError) as err:
                inst.get_eigen_decomposition(index, basis=basis)
            assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE, (index, basis)
        single = inst.get_eigen_decomposition(1)
        # a handle of two partition children: every child is given the same systems, the first one answers
        parts = bg.BeagleInstance(lib, 2, 3, 2, S, 130, 2, 2, 1, 1, preference_flags=preference(False))
        try:
            parts.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
            parts.set_eigen_decomposition(0, U, Ui, lam)
            parts.set_eigen_decomposition(1, U, Ui, lam)
            for a, b in zip(parts.get_eigen_decomposition(0), (U, Ui, lam)):
                assert np.array_equal(a, b)
            with pytest.raises(bg.BeagleError) as err:
                parts.get_eigen_decomposition(0, basis=True)
            assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE
            parts.set_rate_matrices(1, er.rate_matrix(r, pi)[None], pi)
            worst = Worst("%2d states PARTITION CHILDREN" % S)
            check_decomposition(worst, er.symmetrised(er.rate_matrix(r, pi), pi, 0), pi, parts.get_eigen_decomposition(1, basis=True), 0, False, 0, "children")
            for a, b in zip(parts.get_eigen_decomposition(0), (U, Ui, lam)):
                assert np.array_equal(a, b)
        finally:
            parts.finalize()
        assert all(np.array_equal(a, b) for a, b in zip(single, inst.get_eigen_decomposition(1)))
    finally:
        inst.finalize()
    dbl = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 2, 1, 1, preference_flags=preference(True))
    try:
        with pytest.raises(bg.BeagleError) as err:
            dbl.get_eigen_decomposition(0)
        assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION
    finally:
        dbl.finalize()


def test_accessor_on_emulation(emu):
    check_accessor(emu)


@pytest.mark.gpu
def test_accessor(gpu):
    check_accessor(gpu)


# ---- B. transition matrices through the solver against exp(Q t) ----------------------------------------------------------------------
def check_matrices(lib, S, K=4, seed=45):
    rng = np.random.default_rng(seed + S)
    jobs = list(er.cases(rng, S))
    rates = mr.category_rates(rng, K)
    L = len(mr.LENGTHS)
    inst, name = make(lib, S, len(jobs), L + 2, K)
    worst = Worst("%2d states x %d MATRICES" % (S, K))
    try:
        inst.set_category_rates(rates)
        for e, (kind, r, pi) in enumerate(jobs):
            inst.set_rate_matrices(e, er.rate_matrix(r, pi)[None], pi)
        for e, (kind, r, pi) in enumerate(jobs):
            B = er.symmetrised(er.rate_matrix(r, pi), pi, 0)
            system = inst.get_eigen_decomposition(e, basis=True)
            rho, omega, norm_b = check_decomposition(worst, B, pi, system, 0, False, 0, kind)
            inst.update_transition_matrices(e, list(range(L)), mr.LENGTHS)
            inst.update_transition_matrices(e, [L], [0.0], first=[L + 1])
            for l, t in enumerate(mr.LENGTHS):
                worst.hold("P", matrix_ratio(inst.get_transition_matrix(l), B, pi, system, rates, t, 0, rho, omega, norm_b), 1.0, (kind, "t = %g" % t))
            worst.hold("P'(0) = Q", matrix_ratio(inst.get_transition_matrix(L + 1), B, pi, system, rates, 0.0, 1, rho, omega, norm_b), 1.0, kind)
        worst.report()
        print("   ", name)
    finally:
        inst.finalize()
    return worst


@pytest.mark.parametrize("S", MATRIX_STATES)
def test_matrices_on_emulation(emu, S):
    check_matrices(emu, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", MATRIX_STATES)
def test_matrices(gpu, S):
    check_matrices(gpu, S)


# ---- C. warm starts ------------------------------------------------------------------------------------------------------------------
def perturbed(rng, r):
    """the next state of a chain, as engine_checks.check_device_eigen_warm_start moves it"""
    r = r * np.exp(0.05 * (rng.random(r.shape) - 0.5))
    return 0.5 * (r + r.T)


def after(w_source):
    """Instance::setRateMatrices' bookkeeping: (the job starts warm, the count it stores) from the source's count"""
    warm = 0 <= w_source < 64
    return warm, (w_source + 1 if warm else 0)


CHAIN_STEPS = (0, 1, 8, 16, 24, 32, 40, 48, 56, 63, 64, 65, 69)
MIXED_STEP = 20            # one of the three source buffers is overwritten by beagleSetEigenDecomposition before this call


def check_chain(lib, S, kind, seed=47):
    """70 calls of three systems each (one shared frequency vector per call, as the ABI has it), target and source ranges alternating
    between eigen buffers 0-2 and 3-5 as FlipCijkSpace does"""
    rng = np.random.default_rng(seed + S + 100 * er.KINDS.index(kind))
    r0, pi = er.one_case(rng, S, kind)
    rs = [r0, perturbed(rng, r0), perturbed(rng, r0)]
    inst, name = make(lib, S, 6, 2, 1)
    worst = Worst("%2d states CHAIN from %s" % (S, kind))
    try:
        inst.set_category_rates([1.0])
        cur = 0
        inst.set_rate_matrices(cur, np.stack([er.rate_matrix(r, pi) for r in rs]), pi)
        w = {e: 0 for e in range(3)}
        w.update({e: -1 for e in range(3, 6)})
        restarts = 0
        for step in range(70):
            rs = [perturbed(rng, r) for r in rs]
            qs = [er.rate_matrix(r, pi) for r in rs]
            if step == MIXED_STEP:
                junk = np.eye(S)
                inst.set_eigen_decomposition(cur + 1, junk, junk, np.zeros(S))
                w[cur + 1] = -1
            new = 3 - cur
            inst.set_rate_matrices_from(new, np.stack(qs), pi, cur)
            started = [after(w[cur + e]) for e in range(3)]
            for e in range(3):
                w[new + e] = started[e][1]
            if step == MIXED_STEP:
                assert [s[0] for s in started] == [True, False, True]
            if step == 64:                                  # the 64-call restart (system 1 started anew at the mixed call)
                assert [s[0] for s in started] == [False, True, False]
            restarts += sum(1 for s in started if not s[0])
            cur = new
            if step in CHAIN_STEPS or step == MIXED_STEP:
                for e in range(3):
                    B = er.symmetrised(qs[e], pi, 0)
                    system = inst.get_eigen_decomposition(cur + e, basis=True)
                    context = ("step %d" % step, "system %d" % e, "warm" if started[e][0] else "cold")
                    rho, omega, norm_b = check_decomposition(worst, B, pi, system, 0, started[e][0], w[cur + e], context)
                    if e == 0:
                        inst.update_transition_matrices(cur, [0], [0.37])
                        worst.hold("P", matrix_ratio(inst.get_transition_matrix(0), B, pi, system, [1.0], 0.37, 0, rho, omega, norm_b), 1.0, context)
        assert restarts == 3, restarts                      # the mixed call's cold job and the 64-call restart of the other two
        worst.report()
    finally:
        inst.finalize()
    return worst


CHAIN_CASES = [(S, kind) for S in CHAIN_STATES for kind in ("equal rates", "skewed", "wide rates")]


@pytest.mark.parametrize("S,kind", CHAIN_CASES)
def test_chain_on_emulation(emu, S, kind):
    check_chain(emu, S, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("S,kind", CHAIN_CASES)
def test_chain(gpu, S, kind):
    check_chain(gpu, S, kind)


def snapshot(inst, indices):
    return [inst.get_eigen_decomposition(e, basis=True) for e in indices]


def check_warm_edges(lib, S, seed=49):
    """a far move, in place, the refused shifted overlap, the refused non-positive frequency"""
    rng = np.random.default_rng(seed + S)
    (ra, pia), (rb, pib), (rc, pic) = (er.one_case(rng, S, kind) for kind in ("ordinary", "wide rates", "skewed"))
    inst, name = make(lib, S, 3)
    worst = Worst("%2d states WARM EDGES" % S)
    try:
        qa, qb, qc = er.rate_matrix(ra, pia), er.rate_matrix(rb, pib), er.rate_matrix(rc, pic)
        inst.set_rate_matrices(0, qa[None], pia)
        # a far move: the basis of an unrelated matrix of the same size (another kind, other frequencies)
        inst.set_rate_matrices_from(1, qb[None], pib, 0)
        check_decomposition(worst, er.symmetrised(qb, pib, 0), pib, inst.get_eigen_decomposition(1, basis=True), 0, True, 1, "far move")
        # in place: the source is the target
        inst.set_rate_matrices_from(1, qc[None], pic, 1)
        check_decomposition(worst, er.symmetrised(qc, pic, 0), pic, inst.get_eigen_decomposition(1, basis=True), 0, True, 2, "in place")
        inst.set_rate_matrices_from(2, qa[None], pia, 1)
        check_decomposition(worst, er.symmetrised(qa, pia, 0), pia, inst.get_eigen_decomposition(2, basis=True), 0, True, 3, "far move back")
        # a shifted overlap: refused, nothing written
        before = snapshot(inst, range(3))
        with pytest.raises(bg.BeagleError) as err:
            inst.set_rate_matrices_from(1, np.stack([qb, qb]), pib, 0)
        assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE and "overlaps" in lib.last_error(), lib.last_error()
        with pytest.raises(bg.BeagleError) as err:
            inst.set_rate_matrices_from(0, np.stack([qb, qb]), pib, 1)
        assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE
        # a frequency that is not positive: refused (no symmetric form), nothing written
        for bad in (0.0, -0.1, float("nan")):
            pin = pib.copy()
            pin[S - 1] = bad
            with pytest.raises(bg.BeagleError) as err:
                inst.set_rate_matrices(0, qb[None], pin)
            assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION, bad
        for old, now in zip(before, snapshot(inst, range(3))):
            for a, b in zip(old, now):
                assert np.array_equal(a, b)
        worst.report()
    finally:
        inst.finalize()
    return worst


@pytest.mark.parametrize("S", CHAIN_STATES)
def test_warm_edges_on_emulation(emu, S):
    check_warm_edges(emu, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", CHAIN_STATES)
def test_warm_edges(gpu, S):
    check_warm_edges(gpu, S)


# ---- D. launch shapes ----------------------------------------------------------------------------------------------------------------
def check_launch_256(lib, monkeypatch, S, seed=51):
    """MBAMD_EIGEN_256: the 256-thread launch beyond 32 states, cold and one warm step, beside the default launch on the same input"""
    rng = np.random.default_rng(seed + S)
    jobs = [(kind, r, pi, perturbed(rng, r)) for kind, r, pi in er.cases(rng, S)]
    default, _ = make(lib, S, 2 * len(jobs))
    monkeypatch.setenv("MBAMD_EIGEN_256", "1")
    try:
        narrow, _ = make(lib, S, 2 * len(jobs))
    finally:
        monkeypatch.delenv("MBAMD_EIGEN_256", raising=False)
    worst = Worst("%2d states 256 THREADS" % S)
    same = []
    try:
        for e, (kind, r, pi, r2) in enumerate(jobs):
            for inst in (default, narrow):
                inst.set_rate_matrices(2 * e, er.rate_matrix(r, pi)[None], pi)
                inst.set_rate_matrices_from(2 * e + 1, er.rate_matrix(r2, pi)[None], pi, 2 * e)
        for e, (kind, r, pi, r2) in enumerate(jobs):
            for index, rr, warm in ((2 * e, r, False), (2 * e + 1, r2, True)):
                B = er.symmetrised(er.rate_matrix(rr, pi), pi, 0)
                context = (kind, "warm" if warm else "cold")
                a = default.get_eigen_decomposition(index, basis=True)
                b = narrow.get_eigen_decomposition(index, basis=True)
                rho, _, _ = check_decomposition(worst, B, pi, b, 0, warm, int(warm), context)
                check_decomposition(Worst(worst.label + " (default launch)"), B, pi, a, 0, warm, int(warm), context)
                worst.hold("eigenvalues against the default launch", float(np.abs(np.sort(a[2]) - np.sort(b[2])).max()), 2.0 * rho, context)
                same.append(all(np.array_equal(x, y) for x, y in zip(a, b)))
        worst.report()
        print("    bit-identical to the default launch: %d of %d systems (not asserted: the convergence sums are reduced in another order)" % (sum(same), len(same)))
    finally:
        default.finalize()
        narrow.finalize()
    return worst


LAUNCH_STATES = [33, 61, 64] if LONGDOUBLE_QUALIFIES else [33]


@pytest.mark.parametrize("S", LAUNCH_STATES)
def test_launch_256_on_emulation(emu, monkeypatch, S):
    check_launch_256(emu, monkeypatch, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", LAUNCH_STATES)
def test_launch_256(gpu, monkeypatch, S):
    check_launch_256(gpu, monkeypatch, S)


COPY_COUNT, COPY_STATES = 128, 64      # 128 x 64 x 64 doubles = 4 MiB, + 64 frequencies + 64 > half the 8 MiB staging ring


def check_device_copy(lib, kinds, seed=53):
    """The branch of Instance::setRateMatrices that takes the rate matrices through a device copy instead of the staging ring: the
    smallest call that is over half the ring, 128 systems of 64 states at once on an instance of 128 eigen buffers; systems 0, 63 and
    127 against part A (every system of a call shares one frequency vector: the kinds that differ in the exchangeabilities)."""
    S = COPY_STATES
    assert (COPY_COUNT * S * S + S) * 8 + 64 > (8 << 20) // 2 >= ((COPY_COUNT - 1) * S * S + S) * 8 + 64
    rng = np.random.default_rng(seed)
    pi = er.one_case(rng, S, "ordinary")[1]
    made = {kind: er.one_case(rng, S, kind)[0] for kind in kinds}
    rs = [made[kinds[e % len(kinds)]] if e % 7 else perturbed(rng, made[kinds[e % len(kinds)]]) for e in range(COPY_COUNT)]
    qs = np.stack([er.rate_matrix(r, pi) for r in rs])
    inst, name = make(lib, S, COPY_COUNT)
    worst = Worst("%d x %d states DEVICE COPY" % (COPY_COUNT, S))
    try:
        inst.set_rate_matrices(0, qs, pi)
        for e in (0, 63, 127):
            check_decomposition(worst, er.symmetrised(qs[e], pi, 0), pi, inst.get_eigen_decomposition(e, basis=True), 0, False, 0, "system %d" % e)
        worst.report()
    finally:
        inst.finalize()
    return worst


def test_device_copy_on_emulation(emu):
    """(the emulation runs a workgroup's 1 024 threads one barrier interval at a time: equal rates only, which converge in the fewest
    sweeps -- the count stays at the branch's threshold)"""
    check_device_copy(emu, ("equal rates",))


@pytest.mark.gpu
def test_device_copy(gpu):
    check_device_copy(gpu, ("ordinary", "equal rates", "near-equal", "sparse", "wide rates"))


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_reference_against_mpmath():
    """transition() -- numpy.linalg.eigh of B in double, the spectral sum in the wide type -- against mpmath.expm at 40 digits on the
    wide B itself, every kind, up to 20 states: exp(Q t) within 2^-45 sqrt(pi_j / pi_i); r Q exp(Q r t), whose entries are of the size of
    r |B| (5e7 where one of two frequencies is 1e-8), within 2^-45 max(1, r |B|) sqrt(pi_j / pi_i).  No engine."""
    rng = np.random.default_rng(55)
    worst = 0.0
    points = [(1.0, 0.0), (1.3e-6, 1e-8), (0.7, 0.1), (1.0, 2.5), (12.4, 100.0)]
    for S in (2, 3, 5, 20):
        for kind, r, pi in er.cases(rng, S):
            B = er.symmetrised(er.rate_matrix(r, pi), pi, 0)
            g = np.sqrt(pi[None, :] / pi[:, None])
            for rate, t in (points if S < 20 else [points[0], points[int(rng.integers(1, len(points)))]]):
                for order in ((0, 1) if t == 0.0 or S < 20 else (0,)):
                    X = er.transition(B, pi, [rate], t, order)[0]
                    want = er.mpmath_transition(B, pi, rate, t, order)
                    with mpmath.workdps(40):
                        diff = np.array([[float(abs(mr.to_mpf(X[i, j]) - want[i, j])) for j in range(S)] for i in range(S)])
                    scale = 1.0 if order == 0 else max(1.0, rate * er.fro(B))        # (order 1 carries the factor r B)
                    ratio = float((diff / (2.0 ** -45 * scale * g)).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (S, kind, rate, t, order, ratio)
    print("REFERENCE eigh + wide spectral sum against mpmath.expm: worst difference / (2^-45 sqrt(pi_j / pi_i)) %.3g" % worst)
