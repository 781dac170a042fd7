"""The transition-matrix kernels against an a-priori rounding bound: P, dP/dt and d2P/dt2 from an eigen-system, branch lengths and
category rates (beagleUpdateTransitionMatrices[WithMultipleModels]) element by element, both engines, every kernel that forms them:

  single precision   k_transition_matrices_s4_inline / k_transition_matrices_s4     4 states (jobs in the arguments / staged)
                     k_transition_matrices_ev with its own exponentials            2 ... 8 states except 4
                     k_transition_matrices_mfma<1..4>                              9 ... 64 states
  double precision   k64_exponentials + k64_matrices                               below 16 states
                     k64_exponentials + k64_matrices_mfma<1..4>                    16 ... 64 states
each at derivative orders 0, 1 and 2 -- and the second copies these kernels write for the partials kernels (part C).
(Above 64 states Instance::launchMatrices would run k_eigen_exponentials + k_transition_matrices_ev and Engine64::launchMatrices
k64_matrices again, but beagleCreateInstance refuses more than 64 states: no call reaches those branches, and
test_more_than_64_states_is_refused holds the refusal instead of a bound at 65 and 80 states.)

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference is tests/matrix_reference.py: X[k,i,j] = sum_s U[i,s] (lambda_s r_k)^o exp(lambda_s r_k t) U^-1[s,j] in np.longdouble
(mpmath where longdouble is no wider than double) from the doubles U, U^-1, lambda that beagleSetEigenDecomposition is given; clamped
at zero for o = 0 only.  The eigen-systems are made here (numpy.linalg.eigh of a symmetrised random reversible rate matrix): the bound
concerns the kernels' arithmetic, not the decomposition.

THE BOUND.  All kernels compute in double, u = 2^-53; x_s = lambda_s r_k t.  The computed term s of the sum carries
  * two roundings in the exponent's argument, fl(fl(lambda_s t) r_k): a relative 2 u of x_s, which the exponential turns into a
    relative 2 |x_s| u of itself;
  * the exponential, 2 u: HIP documents 1 ulp for the double-precision exp (HIP programming guide, math API, "exp: 1 ULP"), and one
    ulp is at most 2 u relative; the emulation calls the host's libm, whose exp is within 1 ulp as well (glibc documents 1 ulp);
  * 2 o u for the factor (lambda_s r_k)^o: deriv_exponential forms lr = fl(lambda r) and e lr (two roundings) or e fl(lr lr) (lr
    squared carries 2 u + 1 u, the product one more: four);
  * two products, U[i,s] e_s and its product with U^-1[s,j] (the latter fused into the addition where the compiler or the matrix
    core does so), and the additions: a term takes part in at most S - 1 roundings of a sum of S terms in ANY order.  On the fp64
    matrix cores (k_transition_matrices_mfma, k64_matrices_mfma: v_mfma_f64_16x16x4_f64) the first product is rounded in the vector
    ALU and every one of the ceil(S / 4) 4 fused steps of the chain rounds once -- at most S + 3 roundings after the product, the
    padded steps adding an exact zero: S of them act on a real term.
That is (2 |x_s| + 2 + 2 o + 2 + S - 1) u = (S + 2 o + 3 + 2 |x_s|) u per term to first order; the bound keeps a constant of 5
(two units of slack) and 1 % for the higher-order terms:

    E[k,i,j] = 1.01 u sum_s (S + 2 o + 5 + 2 |x_s|) |U[i,s]| |(lambda_s r_k)^o e^(x_s)| |U^-1[s,j]|  +  2^-1000

(2^-1000: exp underflows on the longest branches -- gradually from x = -708, to zero below -745 -- and a subnormal exponential is
off by up to 2^-1075 absolutely, times |U| |U^-1|).  The assertion:
    double precision   |got - X| <= E
    single precision   |got - X| <= 2^-24 |X| + 2^-150 + E      one rounding of the double sum to float (half a unit of a normal
                                                                float, half the spacing 2^-149 of the subnormal ones)
The clamp of order 0 moves the computed value and the reference towards each other or not at all.  Wherever the sum does not cancel,
E is a few units of 2^-53 and the single-precision bound half a float ulp: the kernels must round a correct double ONCE.

What the library tells and what it does not.  implName names the layout of the partials kernels (asserted in every case); WHICH matrix
kernel runs follows from the state count alone (Instance::launchMatrices, Engine64::launchMatrices) and from the job count at four
states, and the library reports neither that nor the number of matrix launches: mbamdGetKernelTiming counts partials launches only
(single precision: timed partials launches; double precision: walks, levels, pre-order launches).  So part B asserts the RESULTS of
the queue's rules -- a wrong flush gives a wrong matrix -- and not launch counts; the launch counts of the double-precision engine are
asserted where operations run (part C's lists).

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import mpmath
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from tests import matrix_reference as mr
from tests.engine_checks import F64_GENERAL_SWITCHES
from tests.hostemu import build_emu
from tests.operation_reference import LONGDOUBLE_QUALIFIES
from tests.test_operation_bounds import (F64_LEVELS, F64_WALK, column_scaled, element_scaled, expected_layout, f64_launches, preference,
                                         stored)

NONE = bg.BEAGLE_OP_NONE
U64 = 2.0 ** -53


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
    return "%2d states x %2d %s" % (S, K, "fp64" if double_precision else "fp32")


def bound_ratio(got, X, W, double_precision):
    """max over the elements of |got - X| / bound"""
    bound = 1.01 * U64 * W + 2.0 ** -1000
    if not double_precision:
        bound = bound + 2.0 ** -24 * np.abs(mr.to_float(X)) + 2.0 ** -150
    return float((mr.error(got, X) / bound).max())


def systems_of(rng, S):
    return [mr.reversible_system(rng, S, kind) for kind in mr.KINDS]


class Held:
    """the worst error / bound per derivative order of one check"""

    def __init__(self, label):
        self.label, self.worst = label, [0.0, 0.0, 0.0]

    def check(self, inst, index, ref, rates, t, order, double_precision, what):
        got = inst.get_transition_matrix(index)
        X, W, _ = ref.matrices(rates, t, order)
        ratio = bound_ratio(got, X, W, double_precision)
        self.worst[order] = max(self.worst[order], ratio)
        assert ratio <= 1.0, (self.label, what, "order %d" % order, "t = %g" % t, ratio)
        return got

    def report(self, what, name):
        print("%s %s worst error / bound: P %.3f, P' %.3f, P'' %.3f; %s" % ((self.label, what) + tuple(self.worst) + (name.split(": ", 1)[-1],)))


# ---- A. element-wise: every state count at which the padding or the kernel changes ---------------------------------------------------
# matrices 0-5: P of the six lengths, 6-11: P', 12-17: P'', 18-23: P by the call without derivative lists
def check_matrices(lib, S, K, double_precision, seed=21):
    """P, P' and P'' of six branch lengths in ONE call per eigen-system (three kinds of system), every matrix against the bound"""
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    systems = systems_of(rng, S)
    rates = mr.category_rates(rng, K)
    L = len(mr.LENGTHS)
    held = Held(tag(S, K, dbl))
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, len(systems), 4 * L, K, 1, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        inst.set_category_rates(rates)
        for n, (U, Ui, lam) in enumerate(systems):
            inst.set_eigen_decomposition(n, U, Ui, lam)
        for n, (kind, system) in enumerate(zip(mr.KINDS, systems)):
            ref = mr.MatrixReference(*system)
            idx = [list(range(o * L, (o + 1) * L)) for o in range(4)]
            inst.update_transition_matrices(n, idx[0], mr.LENGTHS, first=idx[1], second=idx[2])
            got = [[held.check(inst, idx[o][l], ref, rates, t, o, dbl, kind) for l, t in enumerate(mr.LENGTHS)] for o in range(3)]
            inst.update_transition_matrices(n, idx[3], mr.LENGTHS)
            for l in range(L):
                assert np.array_equal(inst.get_transition_matrix(idx[3][l]), got[0][l]), (kind, "P with and without derivative lists", l)
            assert all((g >= 0).all() for g in got[0]), kind                       # order 0 is clamped ...
            assert any((g < 0).any() for g in got[1]), kind                        # ... the derivatives are not
            if (rates == 0.0).any():                                              # the rate 0.0: P' = P'' = 0 exactly
                k0 = int(np.argmax(rates == 0.0))
                assert all((g[k0] == 0).all() for o in (1, 2) for g in got[o]), kind
        held.report("MATRICES", name)
    finally:
        inst.finalize()
    return held.worst


#   states: categories     single precision -- k_transition_matrices_ev up to 8 states (4: the four-state kernel), _mfma<1..4> at both
#                          edges of every 16-row wave (15 | 16 | 17, 31 | 32 | 33, 48 | 49, 63 | 64) and past the 8-step operand chunk
#                          (33 and more)
SHAPES_F32 = {2: (4,), 3: (1, 5), 4: (1, 4, 16), 5: (2,), 8: (4, 9), 9: (1,), 15: (2,), 16: (4, 16), 17: (5,), 20: (4,), 31: (2,), 32: (1, 9),
              33: (4,), 48: (2,), 49: (5,), 61: (1, 4), 63: (2,), 64: (1, 4)}
#                          double precision -- k64_matrices below 16, k64_matrices_mfma<1..4> from 16 on
SHAPES_F64 = {4: (1, 4, 16), 15: (2,), 16: (4, 9), 17: (5,), 20: (4,), 33: (2,), 49: (1,), 61: (4,), 64: (2, 5)}
if not LONGDOUBLE_QUALIFIES:          # (the mpmath reference: one small shape per kernel)
    SHAPES_F32 = {4: (4,), 5: (2,), 17: (2,)}
    SHAPES_F64 = {4: (4,), 17: (2,)}
MATRIX_CASES = [pytest.param(S, K, False, id="fp32-%dx%d" % (S, K)) for S, Ks in SHAPES_F32.items() for K in Ks] + \
               [pytest.param(S, K, True, id="fp64-%dx%d" % (S, K)) for S, Ks in SHAPES_F64.items() for K in Ks]


@pytest.mark.parametrize("S,K,double_precision", MATRIX_CASES)
def test_matrices_on_emulation(emu, S, K, double_precision):
    check_matrices(emu, S, K, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision", MATRIX_CASES)
def test_matrices(gpu, S, K, double_precision):
    check_matrices(gpu, S, K, double_precision)


def check_refused(lib, S, double_precision):
    with pytest.raises(bg.BeagleError) as err:
        bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 4, 2, 1, preference_flags=preference(double_precision))
    assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION and "more than 64 states" in lib.last_error(), (err.value.code, lib.last_error())


@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("S", [65, 80])
def test_more_than_64_states_is_refused_on_emulation(emu, S, double_precision):
    check_refused(emu, S, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("S", [65, 80])
def test_more_than_64_states_is_refused(gpu, S, double_precision):
    check_refused(gpu, S, double_precision)


# ---- B. launch geometry and the queue ------------------------------------------------------------------------------------------------
def spread_lengths(rng, count):
    """`count` branch lengths: the six of part A first, then log-uniform over 1e-8 ... 100"""
    more = np.exp(rng.uniform(np.log(1e-8), np.log(100.0), size=max(count - len(mr.LENGTHS), 0)))
    return np.concatenate([np.array(mr.LENGTHS), more])[:count]


def check_four_state_jobs(lib, count, K, seed=23):
    """Four states, single precision: `count` branches in ONE call, P, P' and P'' of each -- `count` jobs per launch, one launch per
    order.  Instance::launchMatrices takes k_transition_matrices_s4_inline (jobs in the kernel arguments, one block of 64 threads) for
    count <= 8 and count K <= 64, else k_transition_matrices_s4 from staged jobs, 256 (job, category) pairs per block.  (Which of
    the two ran is not told by the library: the cases sit on both sides of both conditions.)"""
    S = 4
    rng = np.random.default_rng(seed + 100 * count + K)
    system = mr.reversible_system(rng, S, mr.KINDS[count % 3])
    rates = mr.category_rates(rng, K)
    lengths = spread_lengths(rng, count)
    held = Held(tag(S, K, False))
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, 3 * count, K, 1, preference_flags=preference(False))
    try:
        name = inst.details.implName.decode()
        assert "4-state tree-walk kernels" in name, name
        inline = count <= 8 and count * K <= 64
        blocks = 1 if inline else (count * K + 255) // 256
        inst.set_category_rates(rates)
        inst.set_eigen_decomposition(0, *system)
        ref = mr.MatrixReference(*system)
        idx = [list(range(o * count, (o + 1) * count)) for o in range(3)]
        inst.update_transition_matrices(0, idx[0], lengths, first=idx[1], second=idx[2])
        for o in range(3):
            for l, t in enumerate(lengths):
                held.check(inst, idx[o][l], ref, rates, t, o, False, "job %d of %d" % (l, count))
        held.report("%d JOBS (%s, %d block%s)" % (count, "inline" if inline else "staged", blocks, "" if blocks == 1 else "s"), name)
    finally:
        inst.finalize()
    return held.worst


#                  jobs, categories
FOUR_STATE_JOBS = [(1, 4), (8, 4),          # inline: 4 and 32 threads
                   (9, 4),                  # staged: more jobs than the arguments hold
                   (4, 16),                 # inline: 64 threads, the whole block
                   (8, 9),                  # staged: 72 (job, category) pairs
                   (70, 4)]                 # staged: 280 pairs, a second block of k_transition_matrices_s4


@pytest.mark.parametrize("count,K", FOUR_STATE_JOBS)
def test_four_state_jobs_on_emulation(emu, count, K):
    check_four_state_jobs(emu, count, K)


@pytest.mark.gpu
@pytest.mark.parametrize("count,K", FOUR_STATE_JOBS)
def test_four_state_jobs(gpu, count, K):
    check_four_state_jobs(gpu, count, K)


def check_queue(lib, S, K, double_precision, seed=25):
    """The matrix queue (Instance::updateMatrices / flushMatrices, Engine64::updateMatrices / flushMatrices): what several calls leave
    in the matrix buffers, every matrix against the bound of part A.
      two systems   updates from two eigen-systems by successive calls: nothing flushes between them (at four states in single
                    precision every call launches at once), the jobs of both systems share a launch per order -- each matrix must
                    come from its own system;
      clash         an output index queued twice with different lengths: the queue flushes before the second call's jobs, the second
                    length wins; a derivative index of the second call that equals a pending probability index of the first holds
                    the derivative;
      rate sets     beagleUpdateTransitionMatricesWithMultipleModels over two eigen-systems x two category-rate vectors: a change of
                    rate vector flushes (a launch carries one vector) -- each matrix must follow its own vector."""
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    sysA, sysB = mr.reversible_system(rng, S, "ordinary"), mr.reversible_system(rng, S, "skewed")
    refs = [mr.MatrixReference(*sysA), mr.MatrixReference(*sysB)]
    rates = [mr.category_rates(rng, K), mr.category_rates(rng, K)]
    held = Held(tag(S, K, dbl))
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 2, 12, K, 1, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        inst.set_eigen_decomposition(0, *sysA)
        inst.set_eigen_decomposition(1, *sysB)
        inst.set_category_rates(rates[0])
        inst.set_category_rates_with_index(1, rates[1])

        def expect(index, system, rate_set, t, order, what):
            return held.check(inst, index, refs[system], rates[rate_set], t, order, dbl, what)

        # -- two systems in one queue
        inst.update_transition_matrices(0, [0, 1], [0.1, 2.5], first=[2, 3], second=[4, 5])
        inst.update_transition_matrices(1, [6, 7], [0.1, 1e-3], first=[8, 9], second=[10, 11])
        for o in range(3):
            expect(2 * o, 0, 0, 0.1, o, "two systems")
            expect(2 * o + 1, 0, 0, 2.5, o, "two systems")
            expect(6 + 2 * o, 1, 0, 0.1, o, "two systems")
            expect(7 + 2 * o, 1, 0, 1e-3, o, "two systems")
        assert not np.array_equal(inst.get_transition_matrix(0), inst.get_transition_matrix(6))     # (the same length, two systems)
        # -- clash: matrices 0 and 1 are pending when the second call names them again
        inst.update_transition_matrices(0, [0, 1], [0.3, 0.7])
        inst.update_transition_matrices(1, [0, 2], [0.05, 1.5], first=[1, 3])
        expect(0, 1, 0, 0.05, 0, "clash")
        expect(1, 1, 0, 0.05, 1, "clash")
        expect(2, 1, 0, 1.5, 0, "clash")
        expect(3, 1, 0, 1.5, 1, "clash")
        # -- rate sets: (system, rate vector) of matrices 0 ... 3 = (0, 0), (0, 1), (1, 0), (1, 1); their derivatives in 4 ... 11
        which = [(0, 0), (0, 1), (1, 0), (1, 1)]
        lengths = [0.2, 0.4, 0.6, 0.8]
        inst.update_transition_matrices_with_multiple_models([w[0] for w in which], [w[1] for w in which], [0, 1, 2, 3], lengths,
                                                             first=[4, 5, 6, 7], second=[8, 9, 10, 11])
        for n, (system, rate_set) in enumerate(which):
            for o in range(3):
                expect(4 * o + n, system, rate_set, lengths[n], o, "rate sets")
        held.report("QUEUE", name)
    finally:
        inst.finalize()
    return held.worst


QUEUE_CASES = [pytest.param(20, 4, False, id="fp32-20x4"), pytest.param(61, 2, False, id="fp32-61x2"), pytest.param(4, 4, False, id="fp32-4x4"),
               pytest.param(20, 4, True, id="fp64-20x4"), pytest.param(4, 4, True, id="fp64-4x4")]
if not LONGDOUBLE_QUALIFIES:          # (the mpmath reference: 61 states would take a minute)
    QUEUE_CASES = [c for c in QUEUE_CASES if c.values[0] != 61]


@pytest.mark.parametrize("S,K,double_precision", QUEUE_CASES)
def test_queue_on_emulation(emu, S, K, double_precision):
    check_queue(emu, S, K, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision", QUEUE_CASES)
def test_queue(gpu, S, K, double_precision):
    check_queue(gpu, S, K, double_precision)


# ---- C. the copies the partials kernels read ----------------------------------------------------------------------------------------
# beagleGetTransitionMatrix reads the transposed matrices (double precision: M) only.  The kernels also write what the partials kernels
# really read: the MFMA A-operand image, the tree walk's tables (whose missing-data rows k_wg_init_tables wrote when the instance was
# made), the double-precision engine's MT.  Instance 1 has its matrices from the kernels; instance 2 gets the values read back from
# instance 1 through beagleSetTransitionMatrix, which fills every copy on the host.  The same operation in both must give the same
# bits: a difference is a device-written copy that disagrees with the matrix read back.
# buffers: 0, 1 compact tips; 2 a tip given as partials; 3 = A; 4 = B; 5, 6 results.  Matrices 0, 1.  Scale buffers 0, 1, cumulative 2.
CHILD_KINDS = (("states,states", 0, 1), ("states,partials", 0, 4), ("partials,states", 3, 1), ("partials,partials", 3, 4),
               ("one buffer twice", 4, 4), ("tip partials,partials", 2, 3))


def check_copies(lib, monkeypatch, S, K, double_precision, switches, layout, chained_launches=None, seed=27):
    dbl, P = double_precision, 70                        # (two 32-pattern tiles and a remainder)
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    system = mr.reversible_system(rng, S, "ordinary")
    rates = mr.category_rates(rng, K)
    for k, v in switches:
        monkeypatch.setenv(k, v)
    try:
        pair = [bg.BeagleInstance(lib, 3, 8, 2, S, P, 1, 2, K, 3, preference_flags=preference(dbl)) for _ in (0, 1)]
    finally:
        for k, _ in switches:
            monkeypatch.delenv(k, raising=False)
    try:
        name = pair[0].details.implName.decode()
        assert layout in name and layout in pair[1].details.implName.decode(), name
        made, twin = pair
        made.set_category_rates(rates)
        made.set_eigen_decomposition(0, *system)
        # (matrix 1 at length 0: the identity to rounding -- about half of its off-diagonal sums come out negative, a few 1e-17,
        #  and are clamped.  A copy that kept the unclamped value shows where a compact state selects that column, and against
        #  buffer B, whose elements lie 40 binades apart)
        made.update_transition_matrices(0, [0, 1], [0.1, 0.0])
        for n in (0, 1):
            m = made.get_transition_matrix(n)
            assert (m > 0).any() and np.array_equal(stored(m, dbl), m)
            twin.set_transition_matrix(n, m)
            assert np.array_equal(twin.get_transition_matrix(n), m), "set / get round trip"
        st = [rng.integers(0, S + 1, size=P).astype(np.int32) for _ in (0, 1)]
        st[0][0], st[1][0], st[0][1], st[1][1] = S, 0, S - 1, S          # (the missing code in both tips, at every shape)
        tp = stored(rng.random((P, S)) * 0.9 + 0.05, dbl)
        pa, pb = column_scaled(rng, S, K, P, dbl), element_scaled(rng, S, K, P, dbl)
        for inst in pair:
            for n in (0, 1):
                inst.set_tip_states(n, st[n])
            inst.set_tip_partials(2, tp)
            inst.set_partials(3, pa)
            inst.set_partials(4, pb)

        def both(call):
            a, b = call(made), call(twin)
            return a, b

        for kind, c1, c2 in CHILD_KINDS:
            def unscaled(inst):
                inst.update_partials(np.array([[5, NONE, NONE, c1, 0, c2, 1]], dtype=np.int32), NONE)
                return inst.get_partials(5)

            def scaled(inst):
                inst.reset_scale_factors(2)
                inst.update_partials(np.array([[6, 0, NONE, c1, 0, c2, 1]], dtype=np.int32), 2)
                return inst.get_partials(6), inst.get_scale_exponents(0), inst.get_scale_exponents(2)
            a, b = both(unscaled)
            assert np.isfinite(a).all() and (a > 0).any(), kind
            assert np.array_equal(a, b), (kind, "unscaled", np.argwhere(a != b)[:4].tolist())
            a, b = both(scaled)
            assert np.any(a[1] != 0), kind
            for x, y, what in zip(a, b, ("partials", "exponents", "cumulative exponents")):
                assert np.array_equal(x, y), (kind, "SCALE_WRITE", what, np.argwhere(x != y)[:4].tolist())
        if chained_launches is not None:
            # two chained operations as ONE list: the smallest list the double-precision four-state walk takes (Engine64::tryWalk4)
            def chained(inst):
                f64_launches(inst)
                inst.reset_scale_factors(2)
                inst.update_partials(np.array([[5, 0, NONE, 3, 0, 0, 1], [6, 1, NONE, 5, 0, 4, 1]], dtype=np.int32), 2)
                n = f64_launches(inst)
                return n, inst.get_partials(5), inst.get_partials(6), inst.get_scale_exponents(0), inst.get_scale_exponents(1)
            a, b = both(chained)
            assert a[0] == chained_launches and b[0] == chained_launches, (a[0], b[0], chained_launches)
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y), "chained list"
        print("%s %d patterns COPIES: %d operations bit-identical on kernel-written and host-written matrices; %s%s" %
              (tag(S, K, dbl), P, 2 * len(CHILD_KINDS) + (2 if chained_launches is not None else 0), name.split(": ", 1)[-1],
               "" if not switches else " [" + ",".join(k[6:] for k, _ in switches) + "]"))
    finally:
        for inst in pair:
            inst.finalize()


F64_PLAIN = tuple((name, "1") for name in F64_GENERAL_SWITCHES)
#              states, categories, fp64, switches, layout, launches of the chained list (None: no such list)
COPY_CASES = [pytest.param(4, 4, False, (), "4-state tree-walk kernels", None, id="fp32-walk4"),
              pytest.param(20, 4, False, (), "general-state tree-walk kernels", None, id="fp32-walkg-20"),
              pytest.param(61, 2, False, (), "general-state tree-walk kernels", None, id="fp32-walkg-61"),
              pytest.param(12, 2, False, (), "general-state MFMA", None, id="fp32-mfma-12x2"),
              pytest.param(40, 1, False, (("MBAMD_NO_WALKG", "1"),), "general-state MFMA", None, id="fp32-mfma-40x1"),
              pytest.param(12, 6, False, (), "general-state vector kernels", None, id="fp32-vector-12x6"),
              pytest.param(33, 3, False, (), "general-state vector kernels", None, id="fp32-vector-33x3"),      # (two tiles: rows of 64)
              pytest.param(4, 4, True, F64_WALK, "double-precision", 1, id="fp64-4-walk"),
              pytest.param(4, 4, True, F64_LEVELS, "double-precision", 2, id="fp64-4-levels"),
              pytest.param(20, 4, True, (), "double-precision", None, id="fp64-20"),
              pytest.param(20, 4, True, F64_PLAIN, "double-precision", None, id="fp64-20-plain"),
              pytest.param(61, 2, True, (), "double-precision", None, id="fp64-61"),
              pytest.param(61, 2, True, F64_PLAIN, "double-precision", None, id="fp64-61-plain")]


@pytest.mark.parametrize("S,K,double_precision,switches,layout,chained_launches", COPY_CASES)
def test_copies_on_emulation(emu, monkeypatch, S, K, double_precision, switches, layout, chained_launches):
    check_copies(emu, monkeypatch, S, K, double_precision, switches, layout, chained_launches)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision,switches,layout,chained_launches", COPY_CASES)
def test_copies(gpu, monkeypatch, S, K, double_precision, switches, layout, chained_launches):
    check_copies(gpu, monkeypatch, S, K, double_precision, switches, layout, chained_launches)


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_reference_against_mpmath():
    """The longdouble reference against mpmath at 50 digits, at every state count of part A and every kind of eigen-system: the
    entries of smallest and largest magnitude and a few random ones agree to 2^-58 of the sum of the term magnitudes.  No engine.
    (Where longdouble is no wider than double the reference is mpmath at 200 bits itself, on the reduced list of state counts.)"""
    rng = np.random.default_rng(31)
    worst = 0.0
    #          rate, length: a short branch, an ordinary one, every term decayed (x down to -1200 lambda: the exact argument matters)
    points = [(1.3e-6, 1e-8), (0.7, 0.1), (12.4, 100.0), (1.0, 2.5), (0.0, 0.1)]
    for S in sorted(set(SHAPES_F32) | set(SHAPES_F64)):
        for kind in mr.KINDS:
            U, Ui, lam = mr.reversible_system(rng, S, kind)
            ref = mr.MatrixReference(U, Ui, lam)
            r, t = points[int(rng.integers(len(points)))] if S > 33 else (None, None)
            for rate, length in (points if S <= 33 else [(r, t)]):
                for order in (0, 1, 2):
                    X, _, mag = ref.matrices(np.array([rate]), length, order)
                    a = np.abs(mr.to_float(X[0])).reshape(-1)
                    by_size = np.argsort(a)
                    picks = set(by_size[:3].tolist() + by_size[-2:].tolist() + rng.integers(0, S * S, size=3).tolist())
                    for e in picks:
                        i, j = divmod(int(e), S)
                        want, m = mr.mpmath_entry(U, Ui, lam, rate, length, order, i, j)
                        with mpmath.workdps(50):
                            diff = float(abs(mr.to_mpf(X[0, i, j]) - want))
                        assert abs(m - mag[0, i, j]) <= 1e-12 * m
                        if m > 0:
                            worst = max(worst, diff / m)
                        assert diff <= 2.0 ** -58 * m, (S, kind, rate, length, order, i, j, diff, m)
    print("REFERENCE longdouble against mpmath: worst difference / term magnitudes 2^%.1f" % (np.log2(worst) if worst > 0 else -np.inf))
