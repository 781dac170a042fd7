"""Transition matrices made out of transition matrices on the device: beagleConvolveTransitionMatrices,
beagleTransposeTransitionMatrices and beagleSetTransitionMatrices (mbamd_matrix_products.h; the contract: beagle.h), both engines.

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

  single and double precision   k_matrix_products_s4          4 states (a thread per entry and category)
                                k_matrix_products_lds         2, 3, 5 ... 8 states
                                k_matrix_products_mfma<1..4>  9 ... 64 states (the fp64 matrix cores)
                                k_matrix_transpose, k_matrix_scatter

A. THE BOUND of a product.  The operands are read back with beagleGetTransitionMatrix -- exactly the stored values, float or double --
and X[k,i,j] = sum_l A[k,i,l] B[k,l,j] is formed in np.longdouble (mpmath where longdouble is no wider than double: the
LONGDOUBLE_QUALIFIES convention).  With W[k,i,j] = sum_l |A[k,i,l]| |B[k,l,j]| and u = 2^-53:

    double precision   |got - X| <= 1.01 (S + 5) u W + S 2^-1074
    single precision   |got - X| <= 1.01 (S + 5) u W + S 2^-1074 + 2^-24 |X| + 2^-150

The kernels form products and sums in double.  A term takes part in at most one rounding of its product and in S - 1 additions,
whatever their order: (1 + S - 1) u = S u of its magnitude to first order.  On the fp64 matrix cores (k_matrix_products_mfma) the
product is fused into the addition and the chain has 4 ceil(S / 4) <= S + 3 roundings, the padded steps adding an exact zero.  The
constant S + 5 keeps two units of slack over S + 3, as tests/test_matrix_bounds.py does, and 1 % covers the higher-order terms.  The
absolute term covers products in the subnormal range, each off by up to 2^-1075 (and exact zeros of underflow).  Single precision
adds the ONE rounding of the double sum to float: half a unit of a normal float, half the spacing 2^-149 of the subnormal ones.
(The reference's own error: a product of two doubles rounded to 64 bits and S - 1 additions, (S + 1) 2^-64 W at most -- 2^-11 of
the bound.)

B. EVERY STORED COPY.  beagleGetTransitionMatrix reads one copy of a matrix buffer; the partials kernels read others (the MFMA
A-operand image, the tree walk's tables with their bf16 pieces from 40 states on, the double-precision engine's padded transpose).
On a small tree half the branches get a convolved matrix (two half-length segments), the other half a matrix transposed twice; a
second instance gets the values read back from the first through beagleSetTransitionMatrix, a third through ONE
beagleSetTransitionMatrices call.  Everything computed from the matrices is compared bit for bit.

C. CHAPMAN-KOLMOGOROV.  lnL with every branch's matrix made as P(t/3) P(2t/3) against lnL with P(t), at the project's parity tolerances.

D. LISTS: dependent chains, interleaved entries, more entries than one launch takes, one result written twice, an operand whose update
is still queued, an unstored-subtree recipe whose matrix is overwritten.   E. ROLES: pattern shards, a two-partition instance.
F. ARGUMENT ERRORS: every refusal, both engines with the same status and text, all matrices unchanged afterwards.

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd.division import synthetic_division
from tests import matrix_reference as mr
from tests.engine_checks import REL_FP64
from tests.hostemu import build_emu
from tests.operation_reference import LD, LONGDOUBLE_QUALIFIES
from tests.test_operation_bounds import expected_layout, preference, stored
from tests.test_walk4_tip_pairs import TO_WALK, division as walk4_division, tip_pair_nodes

NONE = bg.BEAGLE_OP_NONE
U64 = 2.0 ** -53
LIST_MAX = 16384                      # MBAMD_MATRIX_LIST_MAX (mbamd_matrix_products.h): entries of one launch
_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


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


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def product_reference(A, B):
    """(X [K][S][S] in the wide type, W [K][S][S] float64) from the stored values A, B (float64 arrays)"""
    W = np.einsum("kil,klj->kij", np.abs(A), np.abs(B))
    if LONGDOUBLE_QUALIFIES:
        # [k][i][j][l]: l last, the axis numpy sums pairwise
        X = (A.astype(LD)[:, :, None, :] * np.swapaxes(B.astype(LD), 1, 2)[:, None, :, :]).sum(axis=-1)
        return X, W
    K, S = A.shape[0], A.shape[1]
    X = np.empty((K, S, S), dtype=object)
    with mpmath.workprec(200):
        for k in range(K):
            for i in range(S):
                for j in range(S):
                    X[k, i, j] = mpmath.fsum(mpmath.mpf(float(A[k, i, l])) * mpmath.mpf(float(B[k, l, j])) for l in range(S))
    return X, W


def product_ratio(got, A, B, double_precision):
    """max over the elements of |got - X| / bound"""
    S = A.shape[1]
    X, W = product_reference(A, B)
    bound = 1.01 * (S + 5) * U64 * W + S * 2.0 ** -1074
    if not double_precision:
        bound = bound + 2.0 ** -24 * np.abs(mr.to_float(X)) + 2.0 ** -150
    return float((mr.error(got, X) / bound).max())


def test_reference_against_mpmath():
    """The longdouble reference against mpmath at 200 bits on one shape with signed operands: within (S + 1) 2^-64 W.  No engine."""
    if not LONGDOUBLE_QUALIFIES:
        return                        # (the reference is mpmath itself)
    rng = np.random.default_rng(5)
    S, K = 17, 2
    A, B = rng.standard_normal((K, S, S)), rng.standard_normal((K, S, S)) * np.exp2(rng.integers(-30, 30, size=(K, S, S)))
    X, W = product_reference(A, B)
    worst = 0.0
    with mpmath.workprec(200):
        for k in range(K):
            for i in range(S):
                for j in range(S):
                    want = mpmath.fsum(mpmath.mpf(float(A[k, i, l])) * mpmath.mpf(float(B[k, l, j])) for l in range(S))
                    worst = max(worst, float(abs(mr.to_mpf(X[k, i, j]) - want)) / W[k, i, j])
    print("REFERENCE longdouble against mpmath: worst difference / W 2^%.1f" % np.log2(worst))
    assert worst <= (S + 1) * 2.0 ** -64


# ---- A. element-wise -----------------------------------------------------------------------------------------------------------------
# matrices 0, 1: P of a short and a long branch; 2, 3: P'; 4, 5: P''; 6: random signed; 7: random signed, tiny (its square is subnormal
# in the stored type); 8 ...: results
SHORT, LONG = 1e-3, 2.5
PAIRS = [(0, 1), (1, 0), (0, 0), (2, 1), (3, 0), (4, 5), (5, 2), (6, 1), (0, 6), (6, 7), (6, 6), (7, 7), (3, 6)]


def check_products(lib, S, K, double_precision, seed=41):
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    system = mr.reversible_system(rng, S, "ordinary")
    rates = mr.category_rates(rng, K)
    first = 8
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, first + len(PAIRS) + 4, K, 1, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        inst.set_category_rates(rates)
        inst.set_eigen_decomposition(0, *system)
        inst.update_transition_matrices(0, [0, 1], [SHORT, LONG], first=[2, 3], second=[4, 5])
        signed = stored(rng.standard_normal((K, S, S)) * np.exp2(rng.integers(-8, 9, size=(K, S, S)).astype(np.float64)), dbl)
        tiny = stored(rng.standard_normal((K, S, S)) * 2.0 ** (-530 if dbl else -70), dbl)
        inst.set_transition_matrix(6, signed)
        inst.set_transition_matrix(7, tiny)
        operands = [inst.get_transition_matrix(n) for n in range(first)]
        assert all(np.array_equal(stored(m, dbl), m) for m in operands)
        assert (operands[2] < 0).any() and (operands[4] < 0).any() and np.array_equal(operands[6], signed)
        results = list(range(first, first + len(PAIRS)))
        inst.convolve_transition_matrices([a for a, _ in PAIRS], [b for _, b in PAIRS], results)
        worst = 0.0
        for (a, b), r in zip(PAIRS, results):
            got = inst.get_transition_matrix(r)
            ratio = product_ratio(got, operands[a], operands[b], dbl)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag(S, K, dbl), "matrix %d x matrix %d" % (a, b), ratio)
            assert np.array_equal(stored(got, dbl), got)
        sub = inst.get_transition_matrix(results[PAIRS.index((7, 7))])
        assert (sub != 0).any() and np.abs(sub).max() < (2.0 ** -1022 if dbl else 2.0 ** -126), "the subnormal product"
        for n in range(first):                             # the operands are what they were
            assert np.array_equal(inst.get_transition_matrix(n), operands[n]), n
        # -- the transpose: into another buffer, in place, and of a product
        t0 = first + len(PAIRS)
        inst.transpose_transition_matrices([0, 6, results[3]], [t0, t0 + 1, t0 + 2])
        for src, dst in ((0, t0), (6, t0 + 1)):
            assert np.array_equal(inst.get_transition_matrix(dst), operands[src].transpose(0, 2, 1)), ("transpose", src)
        assert np.array_equal(inst.get_transition_matrix(t0 + 2), inst.get_transition_matrix(results[3]).transpose(0, 2, 1))
        inst.transpose_transition_matrices([6, 3], [6, 3])
        assert np.array_equal(inst.get_transition_matrix(6), signed.transpose(0, 2, 1)), "transpose in place"
        assert np.array_equal(inst.get_transition_matrix(3), operands[3].transpose(0, 2, 1)), "transpose in place"
        inst.transpose_transition_matrices([6], [6])
        assert np.array_equal(inst.get_transition_matrix(6), signed), "transposed twice"
        # -- the batch set: the same bits as single sets; of an index named twice the later matrix stays
        batch = np.stack([signed, tiny, operands[2], operands[5]])
        inst.set_transition_matrices([t0, t0 + 1, t0 + 3, t0 + 1], batch)
        for dst, m in ((t0, signed), (t0 + 1, operands[5]), (t0 + 3, operands[2])):
            inst.set_transition_matrix(0, m)
            assert np.array_equal(inst.get_transition_matrix(dst), inst.get_transition_matrix(0)), ("batch set", dst)
        print("%s PRODUCTS worst error / bound over %d products: %.3f; %s" % (tag(S, K, dbl), len(PAIRS), worst, name.split(": ", 1)[-1]))
    finally:
        inst.finalize()
    return worst


#         the state counts at which a kernel or its padding changes
STATES = (2, 3, 4, 5, 8, 9, 16, 17, 20, 32, 33, 40, 48, 49, 61, 64)
if not LONGDOUBLE_QUALIFIES:          # (the mpmath reference: one small shape per kernel)
    STATES = (4, 5, 17)
PRODUCT_CASES = [pytest.param(S, K, dbl, id="%s-%dx%d" % ("fp64" if dbl else "fp32", S, K)) for dbl in (False, True) for S in STATES for K in (1, 3)]


@pytest.mark.parametrize("S,K,double_precision", PRODUCT_CASES)
def test_products_on_emulation(emu, S, K, double_precision):
    check_products(emu, S, K, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision", PRODUCT_CASES)
def test_products(gpu, S, K, double_precision):
    check_products(gpu, S, K, double_precision)


# ---- B, C. on a tree -----------------------------------------------------------------------------------------------------------------
NTAXA, NPAT, NCAT = 7, 130, 2         # 130 patterns: two 64-pattern blocks and a ragged tail


def tree_division(S):
    """7 taxa, 130 patterns, 2 categories, a tenth of the tip states missing"""
    kind = {4: "gtr", 20: "wag"}.get(S, "gen%d" % S)
    return synthetic_division(kind, NTAXA, NPAT, seed=19, tree_seed=6, alpha=0.6, ncat=NCAT, p_gap=0.1)


class ProductDivision(lk.BeagleDivision):
    """A division whose transition matrices pass through the new calls (two chains' worth of matrix buffers: the second chain's and
    the scratch set are the temporaries).  mode:
         made    every other branch P(t/2) P(t/2) by beagleConvolveTransitionMatrices, the others transposed twice (alternately
                 through a temporary and in place); the values read back are kept in `values`
         set     `values` through beagleSetTransitionMatrix, one call per branch
         batch   `values` through ONE beagleSetTransitionMatrices call
         thirds  every branch P(t/3) P(2t/3)
         plain   nothing: P(t) of beagleUpdateTransitionMatrices"""

    def __init__(self, div, lib, mode, values=None, **kw):
        self.mode, self.values = mode, ({} if values is None else values)
        super().__init__(div, lib, nchains=2, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, **kw)

    def TreeTiProbs_Beagle(self, chain):
        super().TreeTiProbs_Beagle(chain)
        t, inst = self.div.tree, self.inst
        nodes = [p for p in t.all_down_pass if self.upDateTi[chain][p]]
        own = [self.tiProbsIndex[chain][p] for p in nodes]
        tmp1, tmp2 = [self.tiProbsIndex[1][p] for p in nodes], [self.tiProbsScratchIndex[p] for p in nodes]
        length = [min(max(t.length[p], lk.BRLENS_MIN), lk.BRLENS_MAX) for p in nodes]
        cijk = self.cijkIndex[chain]
        if self.mode == "made":
            conv = list(range(0, len(nodes), 2))
            inst.update_transition_matrices(cijk, [tmp1[i] for i in conv], [0.5 * length[i] for i in conv])
            inst.update_transition_matrices(cijk, [tmp2[i] for i in conv], [0.5 * length[i] for i in conv])
            inst.convolve_transition_matrices([tmp1[i] for i in conv], [tmp2[i] for i in conv], [own[i] for i in conv])
            through = list(range(1, len(nodes), 4))
            inst.transpose_transition_matrices([own[i] for i in through], [tmp1[i] for i in through])
            inst.transpose_transition_matrices([tmp1[i] for i in through], [own[i] for i in through])
            in_place = list(range(3, len(nodes), 4))
            inst.transpose_transition_matrices([own[i] for i in in_place] * 2, [own[i] for i in in_place] * 2)
            for p, m in zip(nodes, own):
                self.values[p] = inst.get_transition_matrix(m)
        elif self.mode == "set":
            for p, m in zip(nodes, own):
                inst.set_transition_matrix(m, self.values[p])
        elif self.mode == "batch":
            inst.set_transition_matrices(own, np.stack([self.values[p] for p in nodes]))
        elif self.mode == "thirds":
            inst.update_transition_matrices(cijk, tmp1, [x / 3.0 for x in length])
            inst.update_transition_matrices(cijk, tmp2, [2.0 * x / 3.0 for x in length])
            inst.convolve_transition_matrices(tmp1, tmp2, own)


def everything(bd):
    """what an evaluation, the pre-order pass and both gradients leave behind, in a fixed order"""
    t, inst = bd.div.tree, bd.inst
    out = [np.float64(bd.LogLike(0)), inst.get_site_log_likelihoods().copy()]
    bd.AcceptMove(0)
    out += [inst.get_partials(bd.condLikeIndex[0][p]) for p in t.int_down_pass]
    grad, per = bd.BranchGradient(0, sites=True)
    nodes = list(t.all_down_pass)
    out += [np.array([grad[n] for n in nodes]), np.stack([per[n] for n in nodes])]
    out += [inst.get_partials(bd.preOrderIndex[n]) for n in nodes]
    out.append(bd.RateMatrixCrossProducts(0))
    return out


def check_copies(lib, S, double_precision):
    div = tree_division(S)
    made = ProductDivision(div, lib, "made", double_precision=double_precision, pre_order=True)
    try:
        name = made.inst.details.implName.decode()
        assert expected_layout(S, NCAT, double_precision) in name, name
        want = everything(made)
    finally:
        made.finalize()
    assert len(made.values) == 2 * NTAXA - 3 and all(np.isfinite(x).all() for x in want)
    for mode in ("set", "batch"):
        twin = ProductDivision(div, lib, mode, values=made.values, double_precision=double_precision, pre_order=True)
        try:
            got = everything(twin)
        finally:
            twin.finalize()
        assert len(got) == len(want)
        for n, (x, y) in enumerate(zip(want, got)):
            assert np.array_equal(x, y), (tag(S, NCAT, double_precision), mode, "item %d of %d" % (n, len(want)), np.argwhere(np.asarray(x) != np.asarray(y))[:4].tolist())
    print("%s %d patterns COPIES: lnL %.6f, %d arrays bit-identical on device-made, host-set and batch-set matrices; %s" %
          (tag(S, NCAT, double_precision), NPAT, want[0], len(want), name.split(": ", 1)[-1]))


#              one case per layout: the 4-state arenas, the MFMA A-operand image (12 states), the walk tables in fp32 mode (5, 20 states)
#              and with their bf16 pieces (40, 61 states), the double-precision engine below and on the matrix cores
COPY_CASES = [pytest.param(4, False, id="fp32-4"), pytest.param(5, False, id="fp32-5"), pytest.param(12, False, id="fp32-12"),
              pytest.param(20, False, id="fp32-20"), pytest.param(40, False, id="fp32-40"), pytest.param(61, False, id="fp32-61"),
              pytest.param(4, True, id="fp64-4"), pytest.param(20, True, id="fp64-20")]


@pytest.mark.parametrize("S,double_precision", COPY_CASES)
def test_copies_on_emulation(emu, S, double_precision):
    check_copies(emu, S, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,double_precision", COPY_CASES)
def test_copies(gpu, S, double_precision):
    check_copies(gpu, S, double_precision)


def check_chapman_kolmogorov(lib, S, double_precision):
    """relative 1e-11 on the double-precision engine (README: its parity with the fp64 reference), REL_FP64 on the single one"""
    div = tree_division(S)
    lnl = {}
    for mode in ("plain", "thirds"):
        bd = ProductDivision(div, lib, mode, double_precision=double_precision)
        try:
            lnl[mode] = bd.LogLike(0)
        finally:
            bd.finalize()
    rel = abs(lnl["thirds"] - lnl["plain"]) / abs(lnl["plain"])
    tol = 1e-11 if double_precision else REL_FP64
    print("%s CHAPMAN-KOLMOGOROV lnL %.10f with P(t), %.10f with P(t/3) P(2t/3): relative %.2e (tolerance %.0e)" %
          (tag(S, NCAT, double_precision), lnl["plain"], lnl["thirds"], rel, tol))
    assert np.isfinite(lnl["plain"]) and rel <= tol, (lnl, rel)


@pytest.mark.parametrize("S,double_precision", COPY_CASES)
def test_chapman_kolmogorov_on_emulation(emu, S, double_precision):
    check_chapman_kolmogorov(emu, S, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,double_precision", COPY_CASES)
def test_chapman_kolmogorov(gpu, S, double_precision):
    check_chapman_kolmogorov(gpu, S, double_precision)


# ---- D. lists ------------------------------------------------------------------------------------------------------------------------
def list_instance(lib, S, K, double_precision, nmat, seed=43):
    """matrices 0 ... 5: P at six lengths"""
    rng = np.random.default_rng(seed + S)
    inst = bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, nmat, K, 1, preference_flags=preference(double_precision))
    inst.set_category_rates(mr.category_rates(rng, K))
    inst.set_eigen_decomposition(0, *mr.reversible_system(rng, S, "ordinary"))
    inst.update_transition_matrices(0, list(range(6)), [0.01, 0.2, 0.05, 1.5, 0.3, 0.7])
    return inst


def one_by_one(inst, entries):
    for a, b, r in entries:
        inst.convolve_transition_matrices([a], [b], [r])
        inst.get_transition_matrix(r)                      # (a read in between: every entry a call and a launch of its own)


def check_lists(lib, S, K, double_precision):
    dbl = double_precision
    inst = list_instance(lib, S, K, dbl, 40)
    try:
        P = [inst.get_transition_matrix(n) for n in range(6)]
        # -- five dependent entries through two temporaries (10, 11): ((((P0 P1) P2) P3) P4) P5 -> 12; the same one by one -> 22
        chain = [(0, 1, 10), (10, 2, 11), (11, 3, 10), (10, 4, 11), (11, 5, 12)]
        inst.convolve_transition_matrices(*zip(*chain))
        one_by_one(inst, [(0, 1, 20), (20, 2, 21), (21, 3, 20), (20, 4, 21), (21, 5, 22)])
        got = inst.get_transition_matrix(12)
        assert np.array_equal(got, inst.get_transition_matrix(22)), "dependent chain"
        want = P[0]
        for n in range(1, 6):
            want = np.einsum("kil,klj->kij", want, P[n])
        assert np.allclose(got, want, rtol=(1e-12 if dbl else 1e-5), atol=0), "dependent chain against float64"
        # -- the chain interleaved with independent entries (results 13 ... 16)
        free = [(3, 4, 13), (5, 0, 14), (2, 2, 15), (1, 5, 16)]
        mixed = [chain[0], free[0], chain[1], free[1], chain[2], free[2], chain[3], free[3], chain[4]]
        for r in (10, 11, 12):
            inst.set_transition_matrix(r, np.zeros_like(P[0]))
        inst.convolve_transition_matrices(*zip(*mixed))
        one_by_one(inst, [(a, b, r + 10) for a, b, r in free])
        assert np.array_equal(inst.get_transition_matrix(12), inst.get_transition_matrix(22)), "interleaved chain"
        for _, _, r in free:
            assert np.array_equal(inst.get_transition_matrix(r), inst.get_transition_matrix(r + 10)), ("interleaved", r)
        # -- one result written twice: the later entry wins; and read in between
        inst.convolve_transition_matrices([0, 1, 17, 3], [1, 0, 2, 4], [17, 17, 18, 17])
        one_by_one(inst, [(1, 0, 27), (27, 2, 28), (3, 4, 27)])
        assert np.array_equal(inst.get_transition_matrix(17), inst.get_transition_matrix(27)), "written twice"
        assert np.array_equal(inst.get_transition_matrix(18), inst.get_transition_matrix(28)), "read between two writes"
        # -- transposes in list order: 6 <- P0^T, 7 <- (P0^T)^T, then 6 in place
        inst.transpose_transition_matrices([0, 6, 6], [6, 7, 6])
        assert np.array_equal(inst.get_transition_matrix(7), P[0]) and np.array_equal(inst.get_transition_matrix(6), P[0])
        # -- an operand whose update is still queued (the double-precision engine queues beagleUpdateTransitionMatrices; at four
        #    states the single-precision one launches at once, elsewhere it queues too)
        inst.update_transition_matrices(0, [8], [0.4])
        before = inst.get_transition_matrix(8)
        inst.update_transition_matrices(0, [8], [0.9])
        inst.convolve_transition_matrices([8, 1], [1, 8], [30, 31])
        after = inst.get_transition_matrix(8)
        assert not np.array_equal(before, after)
        one_by_one(inst, [(8, 1, 32), (1, 8, 33)])
        assert np.array_equal(inst.get_transition_matrix(30), inst.get_transition_matrix(32)), "queued update of the first operand"
        assert np.array_equal(inst.get_transition_matrix(31), inst.get_transition_matrix(33)), "queued update of the second operand"
        # -- a result that a queued update still names: the update runs first, the product stays
        inst.update_transition_matrices(0, [34], [0.2])
        inst.convolve_transition_matrices([0], [1], [34])
        one_by_one(inst, [(0, 1, 35)])
        assert np.array_equal(inst.get_transition_matrix(34), inst.get_transition_matrix(35)), "queued update of the result"
        print("%s LISTS: chain of 5, interleaved, written twice, queued updates: bit-identical to one call per entry" % tag(S, K, dbl))
    finally:
        inst.finalize()


LIST_CASES = [pytest.param(4, 2, False, id="fp32-4"), pytest.param(5, 2, False, id="fp32-5"), pytest.param(20, 2, False, id="fp32-20"),
              pytest.param(4, 2, True, id="fp64-4"), pytest.param(20, 2, True, id="fp64-20")]


@pytest.mark.parametrize("S,K,double_precision", LIST_CASES)
def test_lists_on_emulation(emu, S, K, double_precision):
    check_lists(emu, S, K, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision", LIST_CASES)
def test_lists(gpu, S, K, double_precision):
    check_lists(gpu, S, K, double_precision)


def check_long_list(lib, double_precision):
    """LIST_MAX + 9 independent entries at four states, one category: the second launch begins at entry LIST_MAX of the staged table.
    Entry u is P0 P1 (u even) or P1 P0 (u odd) into buffer 8 + u; then as many transposes in place."""
    n = LIST_MAX + 9
    inst = list_instance(lib, 4, 1, double_precision, 8 + n)
    try:
        u = np.arange(n)
        inst.convolve_transition_matrices(u % 2, 1 - u % 2, 8 + u)
        inst.convolve_transition_matrices([0, 1], [1, 0], [6, 7])
        want = [inst.get_transition_matrix(6), inst.get_transition_matrix(7)]
        assert not np.array_equal(want[0], want[1])
        look = sorted(set(list(range(0, n, 997)) + [LIST_MAX - 2, LIST_MAX - 1, LIST_MAX, LIST_MAX + 1, n - 2, n - 1]))
        for v in look:
            assert np.array_equal(inst.get_transition_matrix(8 + v), want[v % 2]), ("entry", v)
        inst.transpose_transition_matrices(8 + u, 8 + u)
        for v in look:
            assert np.array_equal(inst.get_transition_matrix(8 + v), want[v % 2].transpose(0, 2, 1)), ("transposed entry", v)
        print("%s LONG LIST: %d entries, %d looked at" % (tag(4, 1, double_precision), n, len(look)))
    finally:
        inst.finalize()


@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
def test_long_list_on_emulation(emu, double_precision):
    check_long_list(emu, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
def test_long_list(gpu, double_precision):
    check_long_list(gpu, double_precision)


def check_recipe(lib, monkeypatch):
    """Four states, single precision: a whole-tree list leaves its tip pairs unstored, as recipes that hold a snapshot of their
    matrices (tests/test_walk4_tip_pairs.py).  The list alone, then EVERY matrix of the tree overwritten, then the tip pairs read:
    the old result bit for bit, whether beagleSetTransitionMatrix overwrote the matrices (as ever) or beagleConvolveTransitionMatrices."""
    for k, v in TO_WALK.items():
        monkeypatch.setenv(k, v)
    div = walk4_division("balanced", 33, 4, NPAT)          # (the shape of test_overwritten_matrices there)
    t = div.tree
    pairs = tip_pair_nodes(t)
    runs = {}
    for how in ("set", "convolve"):
        bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS)
        try:
            inst = bd.inst
            lnl = bd.LogLike(0)
            bd.AcceptMove(0)
            arrays = [np.float64(lnl)] + [inst.get_partials(bd.condLikeIndex[0][p]) for p in pairs]
            c0 = inst.get_recompute_counts()
            bd.FlipSiteScalerSpace(0)
            inst.reset_scale_factors(bd.siteScalerIndex[0])
            bd.TouchAllTreeNodes(0)
            bd.TreeTiProbs_Beagle(0)
            bd.TreeCondLikes_Beagle_Always_Rescale(0)
            bd.ClearTouches(0)
            nodes = list(t.all_down_pass)
            own = [bd.tiProbsIndex[0][p] for p in nodes]
            old = [bd.tiProbsScratchIndex[p] for p in nodes]              # (the first evaluation's matrices)
            if how == "set":
                junk = np.tile(np.full((4, 4), 0.25), (div.ncat, 1, 1))
                for m in own:
                    inst.set_transition_matrix(m, junk)
            else:
                inst.convolve_transition_matrices(old, old[1:] + old[:1], own)
                assert not np.array_equal(inst.get_transition_matrix(own[0]), inst.get_transition_matrix(old[0]))
            arrays += [inst.get_partials(bd.condLikeIndex[0][p]) for p in pairs]
            c1 = inst.get_recompute_counts()
            runs[how] = (arrays, c0, c1)
        finally:
            bd.finalize()
    (a, a0, a1), (b, b0, b1) = runs["set"], runs["convolve"]
    n = len(pairs)
    # (left unstored, materialised, launches): both evaluations left every tip pair unstored, and the reads materialised them
    assert a0 == b0 == (n, n, n) and a1 == b1 == (2 * n, 2 * n, 2 * n), (a0, b0, a1, b1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for p in range(n):                                     # the second evaluation's tip pairs: the first one's, from the snapshot
        assert np.array_equal(b[1 + n + p], b[1 + p]), ("tip pair", p)
    print("RECIPE: %d unstored tip pairs read back bit for bit after every matrix was overwritten by a convolution" % n)


def test_recipe_on_emulation(emu, monkeypatch):
    check_recipe(emu, monkeypatch)


@pytest.mark.gpu
def test_recipe(gpu, monkeypatch):
    check_recipe(gpu, monkeypatch)


# ---- E. roles ------------------------------------------------------------------------------------------------------------------------
def check_shards(lib, monkeypatch, S):
    """MBAMD_SHARD=3 at 130 patterns (children of 64, 64 and 2 patterns, each with its own matrices): per-site lnL of the tree with
    device-made matrices, bit-equal with the plain instance's"""
    div = tree_division(S)
    sites = {}
    for shards in (None, "3"):
        monkeypatch.delenv("MBAMD_SHARD", raising=False)
        if shards:
            monkeypatch.setenv("MBAMD_SHARD", shards)
        try:
            bd = ProductDivision(div, lib, "made")
        finally:
            monkeypatch.delenv("MBAMD_SHARD", raising=False)
        try:
            assert bd.inst.child_count() == (3 if shards else 1)
            lnl = bd.LogLike(0)
            sites[shards] = (lnl, bd.inst.get_site_log_likelihoods().copy(), dict(bd.values))
        finally:
            bd.finalize()
    assert np.isfinite(sites[None][0])
    assert np.array_equal(sites[None][1], sites["3"][1])
    for p, m in sites[None][2].items():
        assert np.array_equal(m, sites["3"][2][p]), p
    print("%s SHARDS: per-site lnL of 3 children bit-equal with the plain instance's (lnL %.6f)" % (tag(S, NCAT, False), sites[None][0]))


@pytest.mark.parametrize("S", [4, 20])
def test_shards_on_emulation(emu, monkeypatch, S):
    check_shards(emu, monkeypatch, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 20])
def test_shards(gpu, monkeypatch, S):
    check_shards(gpu, monkeypatch, S)


def check_partitions(lib, S, double_precision):
    """One model and tree over 130 patterns, as a plain instance and as a two-partition instance (70 + 60 patterns) through the
    ByPartition calls; every branch's matrix is P(t/2) P(t/2), convolved on the device.  Per-site lnL bit-equal."""
    div = tree_division(S)
    t, N, K = div.tree, NTAXA, NCAT
    nInt, nNodes = N - 2, 2 * N - 2
    es = div.eigen[0]
    nodes = list(t.all_down_pass)
    half = [0.5 * t.length[p] for p in nodes]
    sites = []
    for partitioned in (False, True):
        inst = bg.BeagleInstance(lib, N, N + nInt, N, S, NPAT, 2, 3 * nNodes, K, nInt + 2, preference_flags=preference(double_precision))
        try:
            for tip in range(N):
                inst.set_tip_states(tip, div.tip_states[tip])
            inst.set_pattern_weights(div.weights)
            if partitioned:
                inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
                assert inst.child_count() == 2
            for d in range(2):
                inst.set_eigen_decomposition(d, es.evec, es.ivec, es.eval)
                inst.set_state_frequencies(d, div.pi)
                inst.set_category_weights(d, div.category_weights(0))
            inst.set_category_rates(div.cat_rates)
            inst.update_transition_matrices(0, [nNodes + p for p in nodes], half)
            inst.update_transition_matrices(0, [2 * nNodes + p for p in nodes], half)
            inst.convolve_transition_matrices([nNodes + p for p in nodes], [2 * nNodes + p for p in nodes], nodes)
            top = t.root_left
            if partitioned:
                ops = [[p, p - N, NONE, t.left[p], t.left[p], t.right[p], t.right[p], d, nInt + d] for p in t.int_down_pass for d in range(2)]
                for d in range(2):
                    inst.reset_scale_factors_by_partition(nInt + d, d)
                inst.update_partials_by_partition(np.array(ops, dtype=np.int32))
                rc, _, lnl = inst.calculate_edge_log_likelihoods_by_partition([top, top], [t.root, t.root], [top, top], [0, 1], [0, 1],
                                                                              [nInt, nInt + 1], [0, 1], 1)
            else:
                ops = [[p, p - N, NONE, t.left[p], t.left[p], t.right[p], t.right[p]] for p in t.int_down_pass]
                inst.reset_scale_factors(nInt)
                inst.update_partials(np.array(ops, dtype=np.int32), nInt)
                rc, lnl = inst.calculate_edge_log_likelihoods([top], [t.root], [top], [0], [0], [nInt])
            assert rc == 0 and np.isfinite(lnl)
            sites.append(inst.get_site_log_likelihoods().copy())
        finally:
            inst.finalize()
    assert np.array_equal(sites[0], sites[1]), np.argwhere(sites[0] != sites[1])[:4].tolist()
    print("%s PARTITIONS: per-site lnL of 70 + 60 patterns bit-equal with the plain instance's" % tag(S, K, double_precision))


PARTITION_CASES = [pytest.param(4, False, id="fp32-4"), pytest.param(20, False, id="fp32-20"), pytest.param(4, True, id="fp64-4")]


@pytest.mark.parametrize("S,double_precision", PARTITION_CASES)
def test_partitions_on_emulation(emu, S, double_precision):
    check_partitions(emu, S, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("S,double_precision", PARTITION_CASES)
def test_partitions(gpu, S, double_precision):
    check_partitions(gpu, S, double_precision)


# ---- F. argument errors --------------------------------------------------------------------------------------------------------------
def ints(*v):
    return (C.c_int * len(v))(*v)


def check_refusals(lib, S):
    """Every refusal of the three calls on a single- and a double-precision instance of the same dimensions: BEAGLE_ERROR_OUT_OF_RANGE,
    the same text on both engines, and every matrix as it was -- the bad entry stands LAST, behind entries that would have written."""
    K, M = 2, 6
    L = lib.lib
    rng = np.random.default_rng(47 + S)
    given = [stored(rng.standard_normal((K, S, S)), False) for _ in range(M)]
    mats = (C.c_double * (2 * K * S * S))(*([1.5] * (2 * K * S * S)))
    ok, bad_hi, bad_lo = ints(0, 1), ints(2, M), ints(2, -1)
    null_i, null_d = C.cast(None, _ip), C.cast(None, _dp)
    calls = {
        "convolve: first NULL": lambda i: L.beagleConvolveTransitionMatrices(i, null_i, ok, ints(2, 3), 2),
        "convolve: second NULL": lambda i: L.beagleConvolveTransitionMatrices(i, ok, null_i, ints(2, 3), 2),
        "convolve: result NULL": lambda i: L.beagleConvolveTransitionMatrices(i, ok, ok, null_i, 2),
        "convolve: negative count": lambda i: L.beagleConvolveTransitionMatrices(i, ok, ok, ints(2, 3), -1),
        "convolve: first too large": lambda i: L.beagleConvolveTransitionMatrices(i, bad_hi, ok, ints(4, 5), 2),
        "convolve: first negative": lambda i: L.beagleConvolveTransitionMatrices(i, bad_lo, ok, ints(4, 5), 2),
        "convolve: second too large": lambda i: L.beagleConvolveTransitionMatrices(i, ok, bad_hi, ints(4, 5), 2),
        "convolve: second negative": lambda i: L.beagleConvolveTransitionMatrices(i, ok, bad_lo, ints(4, 5), 2),
        "convolve: result too large": lambda i: L.beagleConvolveTransitionMatrices(i, ok, ok, bad_hi, 2),
        "convolve: result negative": lambda i: L.beagleConvolveTransitionMatrices(i, ok, ok, bad_lo, 2),
        "convolve: result is first": lambda i: L.beagleConvolveTransitionMatrices(i, ints(0, 3), ints(1, 1), ints(2, 3), 2),
        "convolve: result is second": lambda i: L.beagleConvolveTransitionMatrices(i, ints(0, 1), ints(1, 3), ints(2, 3), 2),
        "transpose: input NULL": lambda i: L.beagleTransposeTransitionMatrices(i, null_i, ok, 2),
        "transpose: result NULL": lambda i: L.beagleTransposeTransitionMatrices(i, ok, null_i, 2),
        "transpose: negative count": lambda i: L.beagleTransposeTransitionMatrices(i, ok, ok, -3),
        "transpose: input too large": lambda i: L.beagleTransposeTransitionMatrices(i, bad_hi, ints(4, 5), 2),
        "transpose: input negative": lambda i: L.beagleTransposeTransitionMatrices(i, bad_lo, ints(4, 5), 2),
        "transpose: result too large": lambda i: L.beagleTransposeTransitionMatrices(i, ok, bad_hi, 2),
        "transpose: result negative": lambda i: L.beagleTransposeTransitionMatrices(i, ok, bad_lo, 2),
        "set: indices NULL": lambda i: L.beagleSetTransitionMatrices(i, null_i, mats, null_d, 2),
        "set: matrices NULL": lambda i: L.beagleSetTransitionMatrices(i, ok, null_d, null_d, 2),
        "set: negative count": lambda i: L.beagleSetTransitionMatrices(i, ok, mats, null_d, -1),
        "set: index too large": lambda i: L.beagleSetTransitionMatrices(i, bad_hi, mats, null_d, 2),
        "set: index negative": lambda i: L.beagleSetTransitionMatrices(i, bad_lo, mats, null_d, 2),
    }
    nothing = {
        "convolve: count 0": lambda i: L.beagleConvolveTransitionMatrices(i, null_i, null_i, null_i, 0),
        "transpose: count 0": lambda i: L.beagleTransposeTransitionMatrices(i, null_i, null_i, 0),
        "set: count 0": lambda i: L.beagleSetTransitionMatrices(i, null_i, null_d, null_d, 0),
    }
    pair = [bg.BeagleInstance(lib, 2, 3, 2, S, 5, 1, M, K, 1, preference_flags=preference(dbl)) for dbl in (False, True)]
    try:
        assert "double-precision" not in pair[0].details.implName.decode() and "double-precision" in pair[1].details.implName.decode()
        for inst in pair:
            for n in range(M):
                inst.set_transition_matrix(n, given[n])
        for what, call in list(calls.items()) + list(nothing.items()):
            texts = []
            for inst in pair:
                rc = call(inst.id)
                if what in nothing:
                    assert rc == bg.BEAGLE_SUCCESS, (what, rc, lib.last_error())
                else:
                    assert rc == bg.BEAGLE_ERROR_OUT_OF_RANGE, (what, rc)
                    texts.append(lib.last_error())
                for n in range(M):
                    assert np.array_equal(inst.get_transition_matrix(n), given[n]), (what, "matrix %d changed" % n)
            if texts:
                assert texts[0] == texts[1] and what.split(":")[0] in texts[0].lower(), (what, texts)
        print("%d states REFUSALS: %d refused calls, the same text on both engines, no matrix changed; %d empty calls accepted" % (S, len(calls), len(nothing)))
    finally:
        for inst in pair:
            inst.finalize()


@pytest.mark.parametrize("S", [4, 5, 20])
def test_refusals_on_emulation(emu, S):
    check_refusals(emu, S)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 5, 20])
def test_refusals(gpu, S):
    check_refusals(gpu, S)
