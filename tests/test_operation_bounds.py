"""The engines' arithmetic operations against a-priori rounding bounds: one partials operation element by element, the root and edge
integration per site, a small tree per site -- single and double precision, transition matrices set directly (no eigen-system).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference is tests/operation_reference.py: numpy einsum in np.longdouble (unit roundoff 2^-64 <= 2^-60 on x86; exact Fractions
where longdouble is no wider than double).  Every input is rounded to the engine's storage type -- float32 for the single-precision
engine (matrices, partials, category weights, frequencies), float64 for the double-precision one -- BEFORE it goes to the engine and
to the reference, and the set / get calls are asserted to round-trip it bit for bit: the bounds concern arithmetic only.

Every term of every sum is non-negative, so these relative bounds hold for any order of summation.  u = 2^-24 / 2^-53:
  one operation, per element     B_op   = (2 S + 4) u      two dot products of S terms and one product (the bf16-piece contraction
                                                           of 40 and 60-63 states drops three cross terms of at most u each and
                                                           accumulates per block of 16 states: inside this bound for S >= 40)
  root integration, per site     B_root = (S + K + 4) u_e
  edge integration, per site     B_edge = (2 S + K + 6) u_e
  a site's log-likelihood        |got - ln L| <= B (1 + B) + 4 * 2^-53 |ln L|    (the log, the e ln 2 term and their addition)
  a tree of m operations         B = (1 + B_op)^m (1 + B_root) - 1               (m B_op + B_root with its higher-order terms)
u_e is the roundoff of the arithmetic the integration kernel really uses (integration_roundoff below).

Operand ranges: buffer A's (category, pattern) columns are spread over 2^-100 ... 2^0 (single) / 2^-900 ... 2^0 (double) -- clear of
the double-precision engine's exponent clamp at -1000; buffer B's ELEMENTS are spread over the 40 binades 2^-10 ... 2^30, so that
every unscaled result stays a normal float32 (>= 2^-104.4 * 2^-14.4), with one pattern all zero and one pattern zero in category 0
only.  The single-precision engine's range below that -- columns at 2^-104 ... 2^-146, subnormal results, where the bounds carry an
absolute term and the bf16-piece contraction runs its range-safe instantiation ("Operand range") -- is
tests/test_exponent_range.py's, which uses the helpers of this module.

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import math

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from tests.engine_checks import F64_GENERAL_SWITCHES
from tests.hostemu import build_emu
from tests.operation_reference import LN2, LONGDOUBLE_QUALIFIES, Reference, dense_tip

NONE = bg.BEAGLE_OP_NONE
REF = Reference()
DEAD_PATTERN, DEAD_CATEGORY_PATTERN = 3, 5          # buffer B: all zero in every category / in category 0 only


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


# ---- what the bounds are made of ---------------------------------------------------------------------------------------------------
def roundoff(double_precision):
    return 2.0 ** -53 if double_precision else 2.0 ** -24


def storage(double_precision):
    return np.float64 if double_precision else np.float32


def stored(a, double_precision):
    """`a` rounded to the engine's storage type, as the float64 array both the engine and the reference take"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(storage(double_precision)).astype(np.float64))


def operation_bound(S, double_precision):
    return (2 * S + 4) * roundoff(double_precision)


def integration_roundoff(double_precision, edge):
    """The double-precision engine integrates in double throughout (k64_integrate, k64_integrate_wide).  The single-precision
    engine's kernels (k_integrate_lnl, k_integrate_lnl_wide, k_integrate_lnl_s4, k_integrate_lnl_wg_wide) widen every partial to
    double before the frequency, the category weight and the sums -- the ROOT form is double arithmetic on float data -- but in
    the EDGE form the child's matrix-vector product is a float fma chain and its product with the parent a float multiplication:
    float arithmetic bounds it."""
    return 2.0 ** -24 if (edge and not double_precision) else 2.0 ** -53


def root_bound(S, K, double_precision):
    return (S + K + 4) * integration_roundoff(double_precision, edge=False)


def edge_bound(S, K, double_precision):
    return (2 * S + K + 6) * integration_roundoff(double_precision, edge=True)


def site_bound(B, lnl):
    """on |got - ln L| of a site whose likelihood carries the relative bound B"""
    return B * (1.0 + B) + 4.0 * 2.0 ** -53 * np.abs(REF.to_float(lnl))


def expected_layout(S, K, double_precision, force_generic=False, no_walkg=False, no_mfma=False):
    """the engine's implName for this shape (Instance::implName, Engine64::implName): as far as the library tells which kernels run"""
    if double_precision:
        return "double-precision"
    if S == 4 and not force_generic:
        return "4-state tree-walk kernels"
    compiled = (2 <= S <= 10 and S != 4) or S in (16, 20, 40) or 60 <= S <= 63
    if compiled and not force_generic and not no_walkg:
        return "general-state tree-walk kernels"
    tiles = (S + 31) // 32
    if 5 <= S <= 64 and ((tiles == 1 and K <= 4) or (tiles == 2 and K <= 2)) and not no_mfma:
        return "general-state MFMA"
    return "general-state vector kernels"


def preference(double_precision):
    return bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def random_matrices(rng, S, K, double_precision, factor=1.0):
    m = rng.random((K, S, S)) + 0.05
    return stored(m / m.sum(axis=2, keepdims=True) * factor, double_precision)


def column_scaled(rng, S, K, P, double_precision):
    """buffer A: every (category, pattern) column times its own power of two, the exponents spread evenly over the range"""
    lo = -900 if double_precision else -100
    ex = rng.permutation(np.linspace(lo, 0, K * P).round()).reshape(K, P, 1)
    return stored((rng.random((K, P, S)) * 0.9 + 0.05) * np.exp2(ex), double_precision)


def element_scaled(rng, S, K, P, double_precision, dead=True):
    """buffer B: every element times its own power of two over 40 binades; with `dead`, one pattern all zero and one pattern zero
    in category 0 only"""
    b = (rng.random((K, P, S)) * 0.9 + 0.05) * np.exp2(rng.integers(-10, 31, size=(K, P, S)).astype(np.float64))
    if dead:
        b[:, DEAD_PATTERN, :] = 0.0
        b[0, DEAD_CATEGORY_PATTERN, :] = 0.0
    return stored(b, double_precision)


def vector(rng, n, double_precision):
    """non-uniform category weights / state frequencies, summing to one before the rounding to the storage type"""
    v = rng.random(n) + 0.1
    return stored(v / v.sum(), double_precision)


def tag(S, K, P, double_precision):
    return "%2d states x %2d x %3d %s" % (S, K, P, "fp64" if double_precision else "fp32")


# ---- A. one operation, element-wise --------------------------------------------------------------------------------------------------
# buffers: 0, 1 compact tips; 2 a tip given as partials; 3 = A; 4 = B; 5, 6, 7 results.  Matrices 0, 1.  Scale buffer 0, cumulative 1.
def check_operation(lib, S, K, P, double_precision, layout=None, seed=1):
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    B_op = operation_bound(S, dbl)
    inst = bg.BeagleInstance(lib, 3, 10, 2, S, P, 1, 4, K, 4, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        # (implName tells the layout -- which family of kernels serves the instance.  For ONE operation nothing tells more: the
        #  double-precision engine counts a launch per level whichever kernel of launchLevel runs, and the instantiation of the
        #  single-precision level kernels is not reported either: not asserted.  Lists are another matter: check_chained_operations
        #  and check_tree assert the walk, the levels and the chain kernel through the launch and list counts)
        assert (layout or expected_layout(S, K, dbl)) in name, name
        per_category = (not dbl) and "tree-walk" in name          # the arena layouts: an exponent per (pattern, category)
        ti = [random_matrices(rng, S, K, dbl), random_matrices(rng, S, K, dbl)]
        for n in (0, 1):
            inst.set_transition_matrix(n, ti[n])
            assert np.array_equal(inst.get_transition_matrix(n), ti[n]), "matrix round trip"
        # (the missing code S included.  The reference takes a missing state as the vector of ones -- the sum of the matrix row --;
        #  kernels that take it as the factor 1 instead are, on rows that sum to one before the rounding to the storage type, within
        #  u / 2 of that sum: less than the S - 1 roundings the bound allows the dot product it replaces)
        st = [rng.integers(0, S + 1, size=P).astype(np.int32) for _ in (0, 1)]
        # (never both tips missing at one pattern: the rows sum to one, the result would be 1 to rounding -- a column maximum AT a
        #  power of two, whose exponent no bound decides)
        st[1] = np.where((st[0] == S) & (st[1] == S), np.arange(P) % S, st[1]).astype(np.int32)
        st[0][0], st[1][0], st[0][1], st[1][1] = S, 0, S - 1, S               # (at every shape: each tip missing somewhere)
        for n in (0, 1):
            inst.set_tip_states(n, st[n])
        tp = stored(rng.random((P, S)) * 0.9 + 0.05, dbl)
        pa, pb = column_scaled(rng, S, K, P, dbl), element_scaled(rng, S, K, P, dbl)
        inst.set_tip_partials(2, tp)
        inst.set_partials(3, pa)
        inst.set_partials(4, pb)
        tp_dense = np.ascontiguousarray(np.broadcast_to(tp, (K, P, S)))
        for idx, a in ((2, tp_dense), (3, pa), (4, pb)):
            assert np.array_equal(inst.get_partials(idx), a), "partials round trip"
        src = {0: dense_tip(st[0], S, K), 1: dense_tip(st[1], S, K), 2: tp_dense, 3: pa, 4: pb}
        wide = {k: REF.widen(v) for k, v in src.items()}
        wm = [REF.widen(m) for m in ti]
        lo, hi = (-1000, 1 << 30) if dbl else (-126, 126)          # f64_new_exponent / scale_exponent (mbamd_kernels.h)
        worst, skipped, columns = 0.0, 0, 0
        for kind, c1, c2 in (("states,states", 0, 1), ("states,partials", 0, 4), ("partials,states", 3, 1), ("partials,partials", 3, 4),
                             ("one buffer twice", 4, 4), ("tip partials,partials", 2, 3)):
            want = REF.operation(wm[0], wide[c1], wm[1], wide[c2])
            # -- no scaling
            inst.update_partials(np.array([[5, NONE, NONE, c1, 0, c2, 1]], dtype=np.int32), NONE)
            got = inst.get_partials(5)
            assert np.isfinite(got).all(), kind
            r0 = float(REF.rel_error(got, want).max()) / B_op             # (inf where the reference is 0 and the engine is not)
            # -- SCALE_WRITE into scale buffer 0 with cumulative buffer 1
            inst.reset_scale_factors(1)
            inst.update_partials(np.array([[6, 0, NONE, c1, 0, c2, 1]], dtype=np.int32), 1)
            got2 = inst.get_partials(6)
            e = inst.get_scale_exponents(0)                                # [K][P]
            assert np.isfinite(got2).all(), kind
            col_max = want.max(axis=2) if per_category else np.broadcast_to(want.max(axis=(0, 2)), (K, P))
            e_ref, near = REF.exponents(col_max, B_op, lo, hi)
            skipped += int(near.sum())
            columns += near.size
            assert np.array_equal(e[~near], e_ref[~near]), (kind, np.argwhere((e != e_ref) & ~near)[:4].tolist())
            dead = REF.to_float(col_max) == 0
            assert np.all(e[dead] == 0) and np.all(got2[REF.to_float(want) == 0] == 0), kind
            r1 = float(REF.rel_error(REF.scaled(got2, e[:, :, None]), want).max()) / B_op
            assert np.array_equal(inst.get_scale_exponents(1), e), kind
            # BEAGLE's per-pattern factor: e ln 2, of the largest of a pattern's category exponents on the single-precision
            # engine (beagleGetScaleFactors), of the one per-pattern exponent on the double-precision engine
            lnsc = e.max(axis=0).astype(np.float64) * LN2
            assert np.array_equal(inst.get_scale_factors(0), lnsc) and np.array_equal(inst.get_scale_factors(1), lnsc), kind
            # -- SCALE_READ: the bits of the write pass
            inst.update_partials(np.array([[7, NONE, 0, c1, 0, c2, 1]], dtype=np.int32), NONE)
            assert np.array_equal(inst.get_partials(7), got2), kind
            print("%s %-22s worst error / bound: unscaled %.3f, scaled %.3f" % (tag(S, K, P, dbl), kind, r0, r1))
            assert r0 <= 1.0 and r1 <= 1.0, (kind, r0, r1)
            worst = max(worst, r0, r1)
        print("%s OPERATION worst error / bound %.3f; %d of %d columns within the bound of a power of two; %s" %
              (tag(S, K, P, dbl), worst, skipped, columns, name.split(": ", 1)[-1]))
        assert skipped <= 0.01 * columns, (skipped, columns)
    finally:
        inst.finalize()
    return worst


#             states, categories, patterns
OP_SHAPES = [(4, 4, 130), (4, 1, 64), (4, 3, 65), (4, 8, 70), (4, 9, 70), (4, 16, 33),                    # four states; (4, 1, 64): a full block
             (2, 4, 70), (2, 1, 33), (3, 4, 40), (5, 2, 70), (8, 4, 70), (9, 3, 40), (15, 2, 40),         # small state counts
             # matrix-core tile counts 1 ... 4 and both sides of the fp64 fuse boundary ceil(S / 16) K = 8; the fp64 two-tip kernels
             # without LDS at (32, 4), (64, 1) and (33 ... 64, 2)
             (16, 1, 70), (16, 4, 40), (16, 8, 33), (17, 2, 40), (20, 4, 70), (20, 5, 33), (32, 4, 40), (33, 2, 40), (33, 3, 33),
             (40, 1, 70), (48, 2, 33), (49, 1, 40), (49, 2, 33), (60, 1, 45), (61, 1, 33), (61, 3, 40), (62, 2, 33), (64, 1, 31), (64, 2, 70)]
PRECISIONS = [pytest.param(False, id="fp32"), pytest.param(True, id="fp64")]


@pytest.mark.parametrize("double_precision", PRECISIONS)
@pytest.mark.parametrize("S,K,P", OP_SHAPES)
def test_operation_on_emulation(emu, S, K, P, double_precision):
    check_operation(emu, S, K, P, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", PRECISIONS)
@pytest.mark.parametrize("S,K,P", OP_SHAPES)
def test_operation(gpu, S, K, P, double_precision):
    check_operation(gpu, S, K, P, double_precision)


# ---- A, continued: the kernels behind the A/B switches meet the same bound -----------------------------------------------------------
#                    switches                     shape        fp64   layout the switch must give (None: the default one)
SWITCH_CASES = [(("MBAMD_FORCE_GENERIC",), (4, 4, 130), False, "general-state vector kernels"),
                (("MBAMD_NO_MFMA",), (15, 2, 40), False, "general-state vector kernels"),        # (by default: the MFMA level kernels)
                (("MBAMD_NO_MFMA",), (33, 2, 40), False, "general-state vector kernels"),
                (("MBAMD_NO_WALKG",), (20, 4, 70), False, "general-state MFMA"),                 # (by default: the tree-walk layout)
                (("MBAMD_NO_WALKG",), (61, 1, 33), False, "general-state MFMA"),
                # one wave per (operation, 32 patterns): implName does not tell it from the kernel per factor tile
                (("MBAMD_MFMA_WHOLE",), (17, 2, 40), False, "general-state MFMA"),
                (("MBAMD_MFMA_WHOLE",), (33, 2, 40), False, "general-state MFMA"),
                # the plain one-wave level kernels of the double-precision engine: MBAMD_F64_MFMA_NO_LDS and MBAMD_F64_NO_TIPS_KERNEL change
                # the kernel of a single operation (the other three concern lists and matrix calls); the library counts one launch per
                # level whichever kernel of launchLevel runs, so WHICH instantiation ran is not told and not asserted.
                # (MBAMD_F64_NO_WALK / MBAMD_F64_WALK_ALWAYS change nothing for a list of ONE operation -- Engine64::tryWalk4 takes lists
                #  of two and more: check_chained_operations below and part C carry them, with the launch counts)
                (F64_GENERAL_SWITCHES, (20, 4, 70), True, None),
                (F64_GENERAL_SWITCHES, (33, 2, 40), True, None),
                (F64_GENERAL_SWITCHES, (61, 3, 40), True, None)]
SWITCH_IDS = ["%s-%dx%d" % ("+".join(s[6:] for s in c[0]) if len(c[0]) == 1 else "F64_GENERAL", c[1][0], c[1][1]) for c in SWITCH_CASES]


def check_operation_under_switches(lib, monkeypatch, switches, shape, double_precision, layout):
    for name in switches:
        monkeypatch.setenv(name, "1")
    try:
        check_operation(lib, *shape, double_precision, layout=layout)      # (an instance reads the switches when it is created)
    finally:
        for name in switches:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("switches,shape,double_precision,layout", SWITCH_CASES, ids=SWITCH_IDS)
def test_operation_under_switches_on_emulation(emu, monkeypatch, switches, shape, double_precision, layout):
    check_operation_under_switches(emu, monkeypatch, switches, shape, double_precision, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("switches,shape,double_precision,layout", SWITCH_CASES, ids=SWITCH_IDS)
def test_operation_under_switches(gpu, monkeypatch, switches, shape, double_precision, layout):
    check_operation_under_switches(gpu, monkeypatch, switches, shape, double_precision, layout)


# ---- A, continued: two chained operations in ONE list, double precision at four states -- the smallest list Engine64::tryWalk4 takes ----
# buffers: 0 compact tip; 2 = A; 3 = B; 4, 5 results.  Scale buffers 0, 1, cumulative 2.
def f64_launches(inst):
    """partials launches of the double-precision engine since the last reset: one per tree walk, per dependency level of a list on
    the level kernels, per list on the chain kernel (Engine64::kernelTiming; the call runs what is queued first)"""
    return inst.get_kernel_timing(reset=True)[1]


def check_chained_operations(lib, monkeypatch, K, P, switches, launches, seed=7):
    S, dbl = 4, True
    rng = np.random.default_rng(seed + 10 * K)
    B_op = operation_bound(S, dbl)
    for k, v in switches:
        monkeypatch.setenv(k, v)
    try:
        inst = bg.BeagleInstance(lib, 2, 6, 2, S, P, 1, 4, K, 4, preference_flags=preference(dbl))
    finally:
        for k, _ in switches:
            monkeypatch.delenv(k, raising=False)
    try:
        ti = [random_matrices(rng, S, K, dbl), random_matrices(rng, S, K, dbl)]
        for n in (0, 1):
            inst.set_transition_matrix(n, ti[n])
        st = rng.integers(0, S + 1, size=P).astype(np.int32)
        inst.set_tip_states(0, st)
        pa, pb = column_scaled(rng, S, K, P, dbl), element_scaled(rng, S, K, P, dbl)
        inst.set_partials(2, pa)
        inst.set_partials(3, pb)
        wm = [REF.widen(m) for m in ti]
        f64_launches(inst)
        inst.reset_scale_factors(2)
        inst.update_partials(np.array([[4, 0, NONE, 2, 0, 0, 1], [5, 1, NONE, 4, 0, 3, 1]], dtype=np.int32), 2)
        got = f64_launches(inst)
        assert got == launches, (switches, got, launches)              # the walk: one launch; the levels: one per operation
        e = [inst.get_scale_exponents(n) for n in (0, 1)]
        assert np.array_equal(inst.get_scale_exponents(2), e[0] + e[1])
        r = []
        # the first operation against its operands; the second against the first one's result AS STORED (read back) and buffer B
        g4, g5 = inst.get_partials(4), inst.get_partials(5)
        for g, ex, want in ((g4, e[0], REF.operation(wm[0], REF.widen(pa), wm[1], REF.widen(dense_tip(st, S, K)))),
                            (g5, e[1], REF.operation(wm[0], REF.widen(g4), wm[1], REF.widen(pb)))):
            e_ref, near = REF.exponents(np.broadcast_to(want.max(axis=(0, 2)), (K, P)), B_op, -1000, 1 << 30)
            assert not near.any() and np.array_equal(ex, e_ref)
            assert np.all(g[REF.to_float(want) == 0] == 0)
            r.append(float(REF.rel_error(REF.scaled(g, ex[:, :, None]), want).max()) / B_op)
        print("%s CHAINED %s: %d launch(es); worst error / bound %.3f, %.3f" % (tag(S, K, P, dbl), ",".join(k[6:] for k, _ in switches) or "default",
                                                                                got, r[0], r[1]))
        assert max(r) <= 1.0, r
    finally:
        inst.finalize()


F64_WALK = (("MBAMD_F64_WALK_ALWAYS", "1"), ("MBAMD_F64_WALK_SLOTS", "2"))      # (children fall out of LDS: the memory path runs too)
F64_LEVELS = (("MBAMD_F64_NO_WALK", "1"),)
CHAINED_CASES = [pytest.param((), 1, id="default"), pytest.param(F64_WALK, 1, id="walk"), pytest.param(F64_LEVELS, 2, id="levels")]


@pytest.mark.parametrize("switches,launches", CHAINED_CASES)
@pytest.mark.parametrize("K,P", [(4, 130), (3, 65)])
def test_chained_operations_double_precision_on_emulation(emu, monkeypatch, K, P, switches, launches):
    check_chained_operations(emu, monkeypatch, K, P, switches, launches)


@pytest.mark.gpu
@pytest.mark.parametrize("switches,launches", CHAINED_CASES)
@pytest.mark.parametrize("K,P", [(4, 130), (3, 65)])
def test_chained_operations_double_precision(gpu, monkeypatch, K, P, switches, launches):
    check_chained_operations(gpu, monkeypatch, K, P, switches, launches)


# ---- B. root and edge integration ----------------------------------------------------------------------------------------------------
# buffers: 0 compact tip; 2 = A; 3 = B (no dead columns: a dead site has no logarithm); 4 = C, column-scaled at 2^-30; 5, 6 results.
def _check_sites(inst, what, rc, lnl, L, B, pw, label):
    """the per-site values of the call just made (beagleGetSiteLogLikelihoods follows the last call: every case here has its own
    reference) and the returned sum.

    The sum is held to two bounds.  (a) P x (the largest site bound): not a derived bound -- it ignores the pattern weights (up to 3
    here) and the rounding of the summation itself; it is kept as a check because the errors of the sites do not line up, and it
    holds with the device's order of summation (a 64-lane halving tree per block, the blocks added on the host; worst ratio 0.67 at
    these shapes -- a serial sum over a block's 64 lanes gives up to 1.34).  A legitimate change of the summation order can turn it
    red without anything being wrong.  (b) the derived one: sum_c w_c bound_c for the sites' own errors, plus the products w_c lnL_c
    (half a unit each), the six halving steps of a block and the nblocks - 1 additions on the host, each at most 2^-53 of the sum of
    the magnitudes: (6.5 + nblocks) 2^-53 sum_c w_c |ln L_c|."""
    assert rc == 0, (what, rc)
    want = REF.log(L)
    site = inst.get_site_log_likelihoods()
    bound = site_bound(B, want)
    ratio = float((np.abs(REF.to_float(REF.widen(site) - want)) / bound).max())
    ref_sum = (REF.widen(pw) * want).sum()
    sum_ratio = float(abs(REF.widen(lnl) - ref_sum)) / (len(pw) * float(bound.max()))
    nblocks = (len(pw) + 63) // 64
    derived = float((pw * bound).sum()) + (6.5 + nblocks) * 2.0 ** -53 * float((pw * np.abs(REF.to_float(want))).sum())
    derived_ratio = float(abs(REF.widen(lnl) - ref_sum)) / derived
    print("%s %-28s worst site error / bound %.3f, sum error / bound %.4f (derived bound: %.4f)" % (label, what, ratio, sum_ratio, derived_ratio))
    assert ratio <= 1.0, (what, ratio)
    assert sum_ratio <= 1.0 and derived_ratio <= 1.0, (what, lnl, float(ref_sum), sum_ratio, derived_ratio)
    return ratio


def check_integration(lib, S, K, P, double_precision, seed=3):
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    label = tag(S, K, P, dbl)
    inst = bg.BeagleInstance(lib, 2, 10, 2, S, P, 3, 4, K, 6, preference_flags=preference(dbl))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        ti = [random_matrices(rng, S, K, dbl), random_matrices(rng, S, K, dbl)]
        for n in (0, 1):
            inst.set_transition_matrix(n, ti[n])
        st = rng.integers(0, S + 1, size=P).astype(np.int32)
        inst.set_tip_states(0, st)
        pa, pb = column_scaled(rng, S, K, P, dbl), element_scaled(rng, S, K, P, dbl, dead=False)
        pc = stored((rng.random((K, P, S)) * 0.9 + 0.05) * 2.0 ** -30, dbl)
        for idx, a in ((2, pa), (3, pb), (4, pc)):
            inst.set_partials(idx, a)
        w = [vector(rng, K, dbl) for _ in range(3)]
        f = [vector(rng, S, dbl) for _ in range(3)]
        for q in range(3):
            inst.set_category_weights(q, w[q])
            inst.set_state_frequencies(q, f[q])
        pw = 1.0 + (np.arange(P) % 3)
        inst.set_pattern_weights(pw)
        W, F = [REF.widen(x) for x in w], [REF.widen(x) for x in f]
        wm = [REF.widen(m) for m in ti]
        Br, Be = root_bound(S, K, dbl), edge_bound(S, K, dbl)
        worst = 0.0
        # -- root on a buffer set directly, no cumulative buffer (A: the columns hundreds of binades apart)
        rc, lnl = inst.calculate_root_log_likelihoods([2], [0], [0], [NONE])
        worst = max(worst, _check_sites(inst, "root, buffer set directly", rc, lnl, REF.root(W[0], F[0], REF.widen(pa)), Br, pw, label))
        # -- root on the result of a SCALE_WRITE operation with its cumulative buffer: the reference integrates the partials and the
        #    exponents the operation left (read back), so that the bound is the integration's alone
        def scaled_operation(dst, scale, cum, c1, c2):
            inst.reset_scale_factors(cum)
            inst.update_partials(np.array([[dst, scale, NONE, c1, 0, c2, 1]], dtype=np.int32), cum)
            e = inst.get_scale_exponents(cum)
            assert np.array_equal(e, inst.get_scale_exponents(scale)) and np.any(e != 0)
            return REF.scaled(inst.get_partials(dst), e[:, :, None])
        r5 = scaled_operation(5, 0, 1, 2, 3)
        rc, lnl = inst.calculate_root_log_likelihoods([5], [1], [1], [1])
        worst = max(worst, _check_sites(inst, "root, scaled operation", rc, lnl, REF.root(W[1], F[1], r5), Br, pw, label))
        # -- edge: the child as compact states, then as partials
        rc, lnl = inst.calculate_edge_log_likelihoods([3], [0], [0], [0], [0], [NONE])
        L = REF.edge(W[0], F[0], REF.widen(pb), wm[0], REF.widen(dense_tip(st, S, K)))
        worst = max(worst, _check_sites(inst, "edge, child compact states", rc, lnl, L, Be, pw, label))
        rc, lnl = inst.calculate_edge_log_likelihoods([3], [2], [1], [2], [2], [NONE])
        L = REF.edge(W[2], F[2], REF.widen(pb), wm[1], REF.widen(pa))
        worst = max(worst, _check_sites(inst, "edge, child partials", rc, lnl, L, Be, pw, label))
        # -- root over three subsets in one call (the codon models' call): their own weights, frequencies and cumulative buffers, the
        #    third without one
        r5 = scaled_operation(5, 0, 1, 4, 3)
        r6 = scaled_operation(6, 2, 3, 3, 4)
        rc, lnl = inst.calculate_root_log_likelihoods([5, 6, 3], [0, 1, 2], [0, 1, 2], [1, 3, NONE])
        L = REF.root(W[0], F[0], r5) + REF.root(W[1], F[1], r6) + REF.root(W[2], F[2], REF.widen(pb))
        worst = max(worst, _check_sites(inst, "root, three subsets", rc, lnl, L, Br, pw, label))
        print("%s INTEGRATION worst error / bound %.3f; %s" % (label, worst, name.split(": ", 1)[-1]))
    finally:
        inst.finalize()
    return worst


# (16 states and more: the fp64 engine's wide integration kernel; K = 1 and K = 9; a full block; odd pattern counts)
INTEGRATION_SHAPES = [(4, 4, 130), (4, 1, 64), (4, 9, 70), (4, 16, 33), (2, 4, 70), (5, 2, 70), (9, 3, 40), (16, 1, 70), (20, 4, 70), (33, 3, 33),
                      (40, 1, 70), (61, 3, 40), (64, 2, 70)]


@pytest.mark.parametrize("double_precision", PRECISIONS)
@pytest.mark.parametrize("S,K,P", INTEGRATION_SHAPES)
def test_integration_on_emulation(emu, S, K, P, double_precision):
    check_integration(emu, S, K, P, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", PRECISIONS)
@pytest.mark.parametrize("S,K,P", INTEGRATION_SHAPES)
def test_integration(gpu, S, K, P, double_precision):
    check_integration(gpu, S, K, P, double_precision)


# ---- C. a small tree with explicit matrices, per site --------------------------------------------------------------------------------
NTIPS = 12


def random_tree(rng, ntips):
    """A random binary topology (check_double_precision_walk_categories's way: join two roots until one is left): operations
    (destination, child 1, child 2), interior nodes ntips, ntips + 1, ... in the order they can be computed."""
    roots = rng.permutation(ntips).tolist()
    ops, nxt = [], ntips
    while len(roots) > 1:
        i, j = sorted(rng.choice(len(roots), size=2, replace=False).tolist())
        ops.append((nxt, roots[i], roots[j]))
        del roots[j]
        roots[i] = nxt
        nxt += 1
    return ops


def f64_chain_kernel_serves(S, K):
    """Engine64::chainKernelServes and the instantiations of launchChains: a root-ward path as ONE launch of k64_partials_chain"""
    tiles = (S + 15) // 16
    lds = 2 * K * ((((S + 3) // 4) + 3) & ~3) * tiles * 64 * 8                     # f64_frag_lds_bytes
    return 16 < S <= 64 and 1 <= K <= 4 and tiles * K <= 8 and lds <= 65536 and (tiles == 2 or (tiles in (3, 4) and K == 1))


def check_tree(lib, S, K, P, double_precision, monkeypatch=None, switches=(), seed=5):
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    label = tag(S, K, P, dbl) + ("" if not switches else " [" + ",".join(k[6:] for k, _ in switches) + "]")
    ops = random_tree(rng, NTIPS)
    nint, nodes = len(ops), NTIPS + len(ops)
    root = ops[-1][0]
    parent = {c: d for d, a, b in ops for c in (a, b)}

    def path_from(n):
        out = []
        while n in parent:
            n = parent[n]
            out.append(n)
        return out
    tip = max(range(NTIPS), key=lambda n: len(path_from(n)))
    path = path_from(tip)
    assert len(path) >= 3, path
    mats = [random_matrices(rng, S, K, dbl, factor=1e-3) for _ in range(nodes)]      # (times 1e-3: the exponents are not zero)
    new_matrix = random_matrices(rng, S, K, dbl, factor=1e-3)
    # (no missing code here: the general-state and double-precision kernels take a missing state as the factor 1, the 4-state
    #  single-precision kernels as the sum of the matrix row -- one and the same to rounding while rows sum to one, as in A and B,
    #  and a factor 1000 apart on these matrices)
    states = [rng.integers(0, S, size=P).astype(np.int32) for _ in range(NTIPS)]
    w, f = vector(rng, K, dbl), vector(rng, S, dbl)
    pw = 1.0 + (np.arange(P) % 3)
    rows = lambda which: np.array([[d, d - NTIPS, NONE, a, a, b, b] for d, a, b in ops if which is None or d in which], dtype=np.int32)
    # m operations below the root, each within B_op of its exact value on the operands it was given: relative errors of non-negative
    # terms add along the tree; the higher-order terms are kept
    B = (1.0 + operation_bound(S, dbl)) ** nint * (1.0 + root_bound(S, K, dbl)) - 1.0
    sources = {n: REF.widen(dense_tip(states[n], S, K)) for n in range(NTIPS)}
    W, F = REF.widen(w), REF.widen(f)
    for k, v in switches:
        monkeypatch.setenv(k, v)
    try:
        inst = bg.BeagleInstance(lib, NTIPS, nint, NTIPS, S, P, 1, nodes, K, nint + 1, preference_flags=preference(dbl))
    finally:
        for k, _ in switches:
            monkeypatch.delenv(k, raising=False)
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        for n in range(nodes - 1):                               # (the root has no branch)
            inst.set_transition_matrix(n, mats[n])
        for n in range(NTIPS):
            inst.set_tip_states(n, states[n])
        inst.set_category_weights(0, w)
        inst.set_state_frequencies(0, f)
        inst.set_pattern_weights(pw)
        # -- the whole tree as one list
        before = inst.get_list_counts()
        if dbl:
            f64_launches(inst)
        inst.reset_scale_factors(nint)
        inst.update_partials(rows(None), nint)
        launched = f64_launches(inst) if dbl else None
        rc, lnl = inst.calculate_root_log_likelihoods([root], [0], [0], [nint])
        wm = [REF.widen(m) for m in mats]
        L = REF.root(W, F, REF.prune(ops, sources, wm)[root])
        worst = _check_sites(inst, "tree of %d operations" % nint, rc, lnl, L, B, pw, label)
        assert np.any(inst.get_scale_exponents(nint) != 0)
        middle = inst.get_list_counts()
        # -- one tip's matrix replaced: only the root-ward path is submitted again
        inst.set_transition_matrix(tip, new_matrix)
        inst.remove_scale_factors([d - NTIPS for d in path], nint)
        inst.update_partials(rows(set(path)), nint)
        launched2 = f64_launches(inst) if dbl else None
        rc, lnl2 = inst.calculate_root_log_likelihoods([root], [0], [0], [nint])
        wm[tip] = REF.widen(new_matrix)
        L2 = REF.root(W, F, REF.prune(ops, sources, wm)[root])
        worst = max(worst, _check_sites(inst, "path of %d operations again" % len(path), rc, lnl2, L2, B, pw, label))
        assert lnl2 != lnl
        after = inst.get_list_counts()
        # (lists, paths, forked paths, fused paths, walks, walked operations) -- counted by the single-precision engine's tree-walk
        # layouts only
        print("%s TREE worst error / bound %.3f; list counts %s -> %s -> %s; %s" % (label, worst, before, middle, after, name.split(": ", 1)[-1]))
        if dbl:
            # the double-precision engine counts its partials launches (f64_launches): k64_walk4 is one launch per list -- every
            # four-state list of 2 ... 64 operations unless MBAMD_F64_NO_WALK is set --, the level kernels one per dependency level,
            # k64_partials_chain one for a root-ward path where it has an instantiation ((20, 4), (33, 1), (40, 1) here; none for
            # four tiles x two categories: (61, 2) stays on the levels, like every state count below 17)
            depth = {n: 0 for n in range(NTIPS)}
            for d, a, b in ops:
                depth[d] = 1 + max(depth[a], depth[b])
            print("%s TREE launches: %d for the tree (%d levels), %d for the path (%d operations)" % (label, launched, depth[root], launched2, len(path)))
            if S == 4 and ("MBAMD_F64_NO_WALK", "1") not in switches:
                assert launched == 1 and launched2 == 1, (launched, launched2)
            else:
                assert launched == depth[root] and depth[root] > 1, (launched, depth[root])
                assert launched2 == (1 if f64_chain_kernel_serves(S, K) else len(path)), (launched2, len(path))
        if "tree-walk" in name:
            assert middle[4] - before[4] == 1 and middle[5] - before[5] == nint, (before, middle)   # the whole tree: one walk (k_walk4_t / k_walkg)
            # the second list: a root-ward path (k_path4; k_pathg exists for 20 and 60-63 states), elsewhere a second walk
            if S == 4 or S == 20 or 60 <= S <= 63:
                assert after[1] - middle[1] == 1 and after[4] == middle[4], (middle, after)
            else:
                assert after[1] == middle[1] and after[4] - middle[4] == 1, (middle, after)
    finally:
        inst.finalize()
    return worst


TREE_SHAPES = [(4, 4, 130), (4, 3, 70), (2, 4, 70), (8, 2, 70), (20, 4, 70), (33, 1, 40), (40, 1, 40), (61, 2, 40)]


@pytest.mark.parametrize("double_precision", PRECISIONS)
@pytest.mark.parametrize("S,K,P", TREE_SHAPES)
def test_tree_on_emulation(emu, S, K, P, double_precision):
    check_tree(emu, S, K, P, double_precision)


@pytest.mark.parametrize("switches", [F64_WALK, F64_LEVELS], ids=["walk", "levels"])
@pytest.mark.parametrize("S,K,P", [s for s in TREE_SHAPES if s[0] == 4])
def test_tree_four_states_double_precision_on_emulation(emu, monkeypatch, S, K, P, switches):
    check_tree(emu, S, K, P, True, monkeypatch, switches)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", PRECISIONS)
@pytest.mark.parametrize("S,K,P", TREE_SHAPES)
def test_tree(gpu, S, K, P, double_precision):
    check_tree(gpu, S, K, P, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("switches", [F64_WALK, F64_LEVELS], ids=["walk", "levels"])
@pytest.mark.parametrize("S,K,P", [s for s in TREE_SHAPES if s[0] == 4])
def test_tree_four_states_double_precision(gpu, monkeypatch, S, K, P, switches):
    check_tree(gpu, S, K, P, True, monkeypatch, switches)


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
def test_reference_types_agree():
    """np.longdouble serves where its roundoff is at most 2^-60; elsewhere -- and here, on a small shape -- exact Fractions: both give
    the same operation, likelihoods, logarithms and exponents."""
    rng = np.random.default_rng(9)
    S, K, P = 5, 2, 7
    exact, fast = Reference(exact=True), Reference(exact=False) if LONGDOUBLE_QUALIFIES else Reference(exact=True)
    assert REF.exact == (not LONGDOUBLE_QUALIFIES)
    m = [random_matrices(rng, S, K, True) for _ in (0, 1)]
    a, b = column_scaled(rng, S, K, P, True), element_scaled(rng, S, K, P, True)
    w, f = vector(rng, K, True), vector(rng, S, True)
    out = []
    for r in (exact, fast):
        want = r.operation(r.widen(m[0]), r.widen(a), r.widen(m[1]), r.widen(b))
        L = r.edge(r.widen(w), r.widen(f), r.widen(a), r.widen(m[0]), r.widen(b + 1.0))
        got = r.to_float(want) * (1.0 + 2.0 ** -50)
        out.append((r.to_float(want), r.to_float(L), r.to_float(r.log(L)), r.exponents(want.max(axis=2), 2.0 ** -40, -1000, 1000)[0],
                    r.rel_error(got, want), r.to_float(r.scaled(b, np.full(b.shape, -7)))))
    (w0, L0, l0, e0, r0, s0), (w1, L1, l1, e1, r1, s1) = out
    assert np.array_equal(w0, w1) and np.array_equal(L0, L1) and np.array_equal(e0, e1) and np.array_equal(s0, s1)
    assert np.all(np.abs(l0 - l1) <= 2.0 ** -52 * np.abs(l0))
    assert np.all(w0[:, DEAD_PATTERN, :] == 0) and np.all(r0[:, DEAD_PATTERN, :] == 0)
    live = w0 != 0
    assert np.all(np.abs(r0[live] - 2.0 ** -50) <= 2.0 ** -52) and np.all(np.abs(r0 - r1) <= 2.0 ** -60)   # (to_float rounds: 2^-53)
    assert math.isinf(float(exact.rel_error(np.ones(1), exact.widen(np.zeros(1)))[0]))
