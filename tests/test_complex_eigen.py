"""Complex eigen-systems (BEAGLE_FLAG_EIGEN_COMPLEX, include/libhmsbeagle/beagle.h): the matrices of non-reversible rate
models, from the CX form of every transition-matrix kernel (tests/test_matrix_bounds.py lists them) up through the tree.

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

A. every matrix element by element against an a-priori bound; B. the copies the partials kernels read; C. through the tree (log-
likelihoods, the gradient in the branch lengths, the cross products, shards, partitions); D. arguments.

THE BOUND of part A.  The reference is tests/complex_matrix_reference.py: X = V B V^-1 in np.longdouble from the doubles the engine is
given.  Real indices carry the terms of test_matrix_bounds.py unchanged -- complex_factor (mbamd_kernels.h) takes deriv_exponential for
them.  For a pair (p, p + 1), with u = 2^-53, x = a r t, y = b r t, mu = r (a + i b), z = mu^o e^(mu t), |z| = |mu|^o e^x, it differs in
four places.
 1. THE ANGLE.  fl(fl(b t) r) is off by a relative 2 u of y; an error d in the angle ROTATES e^(i y): both Re z and Im z move by |z| d,
    that is by up to 2 |y| u |z| each -- an absolute error, whatever |Re z| or |Im z| are.  So every product of a pair is weighted with
    the modulus |z|, and the count gains 2 |y| next to the exponent's 2 |x| (which is relative to e^x, a factor of both parts).
 2. SIN AND COS.  The HIP math documentation is not part of the ROCm installation this was written against; ASSUMED: at most 2 ulp for
    the double-precision sin, cos and sincos (the figure CUDA documents for them; the OpenCL profile OCML is built for allows 4 ulp
    single, and its double routines are held to the same 2 here).  2 ulp of a value of at most 1 is at most 4 u absolute; the host's
    libm, which the emulation calls, documents 1 ulp.  With the exponential's 2 u and the product e * cos: 2 + 4 + 1 = 7 roundings in
    each of Re e^(mu t), Im e^(mu t), in units of u |e^(mu t)|, beyond 2 |x| + 2 |y|:  c_0 = 7.
 3. mu^o IS A COMPLEX PRODUCT.  The errors of exp and of the angle are common to both parts (a factor and a rotation) and pass through
    a complex product unchanged relative to |z|; the 4 + 1 of sin / cos / product are independent in the two parts and gain the
    factor (|Re| + |Im|) / |.| <= sqrt 2.  o = 1: mu = (fl(a r), fl(b r)), one rounding each; z = (mr Re - mi Im, mr Im + mi Re): per
    part 2 (the roundings of mu and of the products, on |mr Re| + |mi Im| <= |mu| |e|) + 1 (the sum) + 5 sqrt 2 + 2 (exp) = 12.1:
    c_1 = 13.  o = 2: q = mu^2 = (mr^2 - mi^2, 2 mr mi) carries 4 u |mu|^2 per part (3 per square or product and the subtraction);
    z = q e: 4 sqrt 2 (q's error on |Re| + |Im|) + 5 sqrt 2 + 1 (products) + 1 (sum) + 2 (exp) = 16.7:  c_2 = 17.
 4. FOUR PRODUCTS.  An entry takes V[i,p] Re z V^-1[p,j], V[i,p+1] Im z V^-1[p,j] and the two with p + 1: each at most
    |z| |V[i,.]| |V^-1[.,j]|.  The kernels combine the two factors of an index first, a[s] = V[i,s] C[s] + V[i,partner(s)] G[s] -- its
    products and one more rounding from the addition -- so the sum over s still has S terms: 2 (the two products of a term) + 1 (the
    combination) + S - 1 (the sum, or the matrix cores' chain as in test_matrix_bounds.py).
    So per product of a pair (2 |x| + 2 |y| + c_o) + 2 + 1 + S - 1 = S + c_o + 2 + 2 |x| + 2 |y|; with that module's two units of slack
        n_p = S + c_o + 4 + 2 |x_p| + 2 |y_p|,        c = (7, 13, 17)
    and  W[k,i,j] = sum over real s of (S + 2 o + 5 + 2 |x_s|) |V[i,s]| |(a_s r)^o e^(x_s)| |V^-1[s,j]|
                  + sum over pairs of n_p |z_p| (|V[i,p]| + |V[i,p+1]|) (|V^-1[p,j]| + |V^-1[p+1,j]|)
        E = 1.01 u W + 2^-1000
    double precision   |got - X| <= E;       single precision   |got - X| <= 2^-24 |X| + 2^-150 + E        (as test_matrix_bounds.py)

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import functools

import mpmath
import numpy as np
import pytest
import scipy.linalg

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd import model as mbmodel
from mrbayes_amd.division import synthetic_division
from tests import complex_matrix_reference as cr
from tests import matrix_reference as mr
from tests.engine_checks import ABS_F64, REL_F64, REL_FP64, engine_lnl
from tests.hostemu import build_emu
from tests.operation_reference import LONGDOUBLE_QUALIFIES
from tests.preorder_reference import bound_factor
from tests.pruning_reference import NTAXA, U32, U64, branch_length
from tests.test_matrix_bounds import CHILD_KINDS, COPY_CASES, Held, bound_ratio, tag
from tests.test_operation_bounds import column_scaled, element_scaled, expected_layout, f64_launches, preference, stored

NONE = bg.BEAGLE_OP_NONE
COMPLEX = bg.BEAGLE_FLAG_EIGEN_COMPLEX


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


# ---- eigen-systems: (name, V, V^-1, a, b, Q or None) -----------------------------------------------------------------------------------
def rate_matrix_system(S):
    """eigen_general of the `nrev` rate matrix: at least one conjugate pair and -- the eigenvalue 0 -- at least one real eigenvalue"""
    q, _ = mbmodel.nonreversible_q(S)
    es = mbmodel.eigen_general(q)
    assert (es.imag != 0).any() and (es.imag == 0).any(), es.imag
    return "rate matrix", es.evec, es.ivec, es.eval, es.imag, q


def cycle_system(S):
    """Q = C - I of the directed S-cycle: eigenvalues w^k - 1, nearly all complex, |b| up to 1; P oscillates in t"""
    q = np.roll(np.eye(S), 1, axis=1) - np.eye(S)
    es = mbmodel.eigen_general(q)
    assert (es.imag != 0).sum() >= S - 2
    return "cycle", es.evec, es.ivec, es.eval, es.imag, q


def placed_pairs(S):
    """(0, 1) and (S-2, S-1), and where S allows (3, 4), (15, 16), (31, 32): the boundaries of a 4-step MFMA, of a 16-row wave and of
    the 8-step operand chunk; reals in between"""
    pairs = [(0, 1)]
    for p in (3, 15, 31, S - 2):
        if p > pairs[-1][1] and p + 1 <= S - 1 and all(p + 1 < q or p > q + 1 for q, _ in pairs[1:]):
            pairs.append((p, p + 1))
    pairs = sorted(set(pairs))
    return [pq for i, pq in enumerate(pairs) if i == 0 or pq[0] > pairs[i - 1][1]]


def placed_system(rng, S):
    """V a random orthogonal matrix times diag(0.5 ... 2), V^-1 by mpmath and rounded; D with its pairs where placed_pairs puts them"""
    V = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((S, S)))[0] * np.linspace(0.5, 2.0, S)[None, :])
    Vi = np.ascontiguousarray(cr.to_wide(cr.mp_inverse(V)).astype(np.float64))
    a, b = -3.0 * rng.random(S), np.zeros(S)
    for p, q in placed_pairs(S):
        a[q] = a[p]
        b[p] = (0.2 + 1.8 * rng.random()) * (1.0 if rng.random() < 0.5 else -1.0)
        b[q] = -b[p]
    return "placed", V, Vi, a, b, None


def all_real_system(rng, S):
    U, Ui, lam = mr.reversible_system(rng, S, "ordinary")
    return "all real", U, Ui, lam, np.zeros(S), None


def systems_of(rng, S):
    return [rate_matrix_system(S), cycle_system(S), placed_system(rng, S), all_real_system(rng, S)]


def test_placed_pairs():
    assert placed_pairs(3) == [(0, 1)] and placed_pairs(4) == [(0, 1), (2, 3)] and placed_pairs(5) == [(0, 1), (3, 4)]
    assert placed_pairs(17) == [(0, 1), (3, 4), (15, 16)] and placed_pairs(33) == [(0, 1), (3, 4), (15, 16), (31, 32)]
    assert placed_pairs(61) == [(0, 1), (3, 4), (15, 16), (31, 32), (59, 60)] and placed_pairs(16) == [(0, 1), (3, 4), (14, 15)]


def complex_instance(lib, *dims, double_precision=False, **kw):
    inst = bg.BeagleInstance(lib, *dims, preference_flags=preference(double_precision), requirement_flags=COMPLEX, **kw)
    assert inst.details.flags & COMPLEX and not inst.details.flags & bg.BEAGLE_FLAG_EIGEN_REAL, hex(inst.details.flags)
    return inst


# ---- A. element-wise -----------------------------------------------------------------------------------------------------------------
EXTRA_LENGTHS = (0.3, 0.7, 1.5)          # nine jobs per order: more than the four-state inline kernel's arguments hold


def check_matrices(lib, S, K, double_precision, jobs=6, seed=41):
    """P, P' and P'' of `jobs` branch lengths in ONE call per eigen-system (four systems), every matrix against the bound"""
    dbl = double_precision
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    systems = systems_of(rng, S)
    rates = mr.category_rates(rng, K)
    lengths = (mr.LENGTHS + EXTRA_LENGTHS)[:jobs]
    L = len(lengths)
    assert L == jobs and lengths[0] == 0.0
    held = Held(tag(S, K, dbl))
    inst = complex_instance(lib, 2, 3, 2, S, 5, len(systems), 4 * L, K, 1, double_precision=dbl)
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, dbl) in name, name
        inst.set_category_rates(rates)
        for n, (_, V, Vi, a, b, _) in enumerate(systems):
            inst.set_eigen_decomposition(n, V, Vi, np.concatenate([a, b]))
        for n, (kind, V, Vi, a, b, Q) in enumerate(systems):
            ref = cr.ComplexMatrixReference(V, Vi, a, b)
            idx = [list(range(o * L, (o + 1) * L)) for o in range(4)]
            inst.update_transition_matrices(n, idx[0], lengths, first=idx[1], second=idx[2])
            got = [[held.check(inst, idx[o][l], ref, rates, t, o, dbl, kind) for l, t in enumerate(lengths)] for o in range(3)]
            inst.update_transition_matrices(n, idx[3], lengths)
            for l in range(L):
                assert np.array_equal(inst.get_transition_matrix(idx[3][l]), got[0][l]), (kind, "P with and without derivative lists", l)
            assert all((g >= 0).all() for g in got[0]), kind                       # order 0 is clamped ...
            assert any((g < 0).any() for g in got[1]), kind                        # ... the derivatives are not
            if (rates == 0.0).any():                                              # the rate 0.0: P' = P'' = 0 exactly
                k0 = int(np.argmax(rates == 0.0))
                assert all((g[k0] == 0).all() for o in (1, 2) for g in got[o]), kind
            if LONGDOUBLE_QUALIFIES:
                # P' at t = 0 is r_k Q, Q = V D V^-1 as the doubles define it (formed apart from the spectral sums, in the wide type);
                # where the system came from a rate matrix, that matrix too, the decomposition's own residual added to the bound
                Qd = ref.defined_matrix()
                _, W, _ = ref.matrices(rates, 0.0, 1)
                X0 = np.asarray(rates, dtype=Qd.dtype)[:, None, None] * Qd[None, :, :]
                assert bound_ratio(got[1][0], X0, W, dbl) <= 1.0, (kind, "P'(0) = r Q")
                if Q is not None:
                    resid = np.abs(Qd - Q.astype(Qd.dtype)).astype(np.float64)
                    XQ = np.asarray(rates, dtype=Qd.dtype)[:, None, None] * Q.astype(Qd.dtype)[None, :, :]
                    assert bound_ratio(got[1][0], XQ, W + rates[:, None, None] * resid[None, :, :] / (1.01 * U64), dbl) <= 1.0, (kind, "P'(0) = r Q, the rate matrix")
        held.report("COMPLEX MATRICES, %d jobs" % jobs, name)
    finally:
        inst.finalize()
    return held.worst


#   states: categories   single precision -- 3, 5, 8: k_transition_matrices_ev; 4: the four-state kernels, at most 8 jobs (inline) and more
#                        (staged); 16 ... 64: k_transition_matrices_mfma<1..4>, 17 and 33 past a wave's 16 rows, 33 and more past the chunk
SHAPES_F32 = {3: (1,), 4: (1, 4), 5: (2,), 8: (4,), 16: (4,), 17: (5,), 33: (4,), 61: (1, 4), 64: (2,)}
#                        double precision -- k64_matrices below 16, k64_matrices_mfma<1..4> from 16 on
SHAPES_F64 = {4: (4,), 15: (2,), 16: (4,), 33: (2,), 61: (4,)}
if not LONGDOUBLE_QUALIFIES:          # (the mpmath reference: one small shape per kernel)
    SHAPES_F32 = {4: (4,), 5: (2,), 17: (2,)}
    SHAPES_F64 = {4: (4,), 17: (2,)}
MATRIX_CASES = [pytest.param(S, K, False, jobs, id="fp32-%dx%d%s" % (S, K, "-staged" if jobs > 8 else ""))
                for S, Ks in SHAPES_F32.items() for K in Ks for jobs in ((6, 9) if S == 4 else (6,))] + \
               [pytest.param(S, K, True, 6, id="fp64-%dx%d" % (S, K)) for S, Ks in SHAPES_F64.items() for K in Ks]


@pytest.mark.parametrize("S,K,double_precision,jobs", MATRIX_CASES)
def test_matrices_on_emulation(emu, S, K, double_precision, jobs):
    check_matrices(emu, S, K, double_precision, jobs)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision,jobs", MATRIX_CASES)
def test_matrices(gpu, S, K, double_precision, jobs):
    check_matrices(gpu, S, K, double_precision, jobs)


# ---- B. the copies the partials kernels read ----------------------------------------------------------------------------------------
# Part C of test_matrix_bounds.py with a COMPLEX `made` instance, whose matrices come from the CX kernels, and a REAL `twin`, which gets
# the values read back through beagleSetTransitionMatrix: the same operation in both must give the same bits.  A difference is a
# device-written table, packed image, bf16 piece or fp64 MT that disagrees with the matrix.
def check_copies(lib, monkeypatch, S, K, double_precision, switches, layout, chained_launches=None, seed=47):
    dbl, P = double_precision, 70
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    _, V, Vi, a, b, _ = rate_matrix_system(S)
    rates = mr.category_rates(rng, K)
    for k, v in switches:
        monkeypatch.setenv(k, v)
    try:
        made = complex_instance(lib, 3, 8, 2, S, P, 1, 2, K, 3, double_precision=dbl)
        twin = bg.BeagleInstance(lib, 3, 8, 2, S, P, 1, 2, K, 3, preference_flags=preference(dbl))
    finally:
        for k, _ in switches:
            monkeypatch.delenv(k, raising=False)
    pair = [made, twin]
    try:
        name = made.details.implName.decode()
        assert layout in name and layout in twin.details.implName.decode(), name
        assert twin.details.flags & bg.BEAGLE_FLAG_EIGEN_REAL and not twin.details.flags & COMPLEX
        made.set_category_rates(rates)
        made.set_eigen_decomposition(0, V, Vi, np.concatenate([a, b]))
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
            return call(made), call(twin)

        for kind, c1, c2 in CHILD_KINDS:
            def unscaled(inst):
                inst.update_partials(np.array([[5, NONE, NONE, c1, 0, c2, 1]], dtype=np.int32), NONE)
                return inst.get_partials(5)

            def scaled(inst):
                inst.reset_scale_factors(2)
                inst.update_partials(np.array([[6, 0, NONE, c1, 0, c2, 1]], dtype=np.int32), 2)
                return inst.get_partials(6), inst.get_scale_exponents(0), inst.get_scale_exponents(2)
            x, y = both(unscaled)
            assert np.isfinite(x).all() and (x > 0).any(), kind
            assert np.array_equal(x, y), (kind, "unscaled", np.argwhere(x != y)[:4].tolist())
            x, y = both(scaled)
            assert np.any(x[1] != 0), kind
            for p, q, what in zip(x, y, ("partials", "exponents", "cumulative exponents")):
                assert np.array_equal(p, q), (kind, "SCALE_WRITE", what, np.argwhere(p != q)[:4].tolist())
        if chained_launches is not None:
            def chained(inst):
                f64_launches(inst)
                inst.reset_scale_factors(2)
                inst.update_partials(np.array([[5, 0, NONE, 3, 0, 0, 1], [6, 1, NONE, 5, 0, 4, 1]], dtype=np.int32), 2)
                n = f64_launches(inst)
                return n, inst.get_partials(5), inst.get_partials(6), inst.get_scale_exponents(0), inst.get_scale_exponents(1)
            x, y = both(chained)
            assert x[0] == chained_launches and y[0] == chained_launches, (x[0], y[0], chained_launches)
            for p, q in zip(x[1:], y[1:]):
                assert np.array_equal(p, q), "chained list"
        print("%s %d patterns COMPLEX COPIES: %d operations bit-identical on CX-kernel-written and host-written matrices; %s" %
              (tag(S, K, dbl), P, 2 * len(CHILD_KINDS) + (2 if chained_launches is not None else 0), name.split(": ", 1)[-1]))
    finally:
        for inst in pair:
            inst.finalize()


@pytest.mark.parametrize("S,K,double_precision,switches,layout,chained_launches", COPY_CASES)
def test_copies_on_emulation(emu, monkeypatch, S, K, double_precision, switches, layout, chained_launches):
    check_copies(emu, monkeypatch, S, K, double_precision, switches, layout, chained_launches)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,double_precision,switches,layout,chained_launches", COPY_CASES)
def test_copies(gpu, monkeypatch, S, K, double_precision, switches, layout, chained_launches):
    check_copies(gpu, monkeypatch, S, K, double_precision, switches, layout, chained_launches)


# ---- C. through the tree ------------------------------------------------------------------------------------------------------------
# float64 pruning written here; its matrices are exp(Q r t) by scipy.linalg.expm (double precision: by mpmath at 30 digits, rounded),
# never from the decomposition.
@functools.lru_cache(maxsize=None)
def division(states, ncat, npat):
    div = synthetic_division("nrev%d" % states, NTAXA, npat, seed=11, tree_seed=5, alpha=0.7, ncat=ncat, p_gap=0.05)
    div.weights = 1.0 + (np.arange(npat) % 3).astype(np.float64)
    assert div.complex_eigen and (div.eigen[0].imag != 0).any()
    return div


@functools.lru_cache(maxsize=None)
def _expm(states, tau, wide):
    q = mbmodel.nonreversible_q(states)[0]
    if not wide:
        return scipy.linalg.expm(q * tau)
    with mpmath.workdps(30):
        return np.array(mpmath.expm(mpmath.matrix(q.tolist()) * mpmath.mpf(tau)).tolist(), dtype=np.float64)


def matrices_of(div, lengths, wide=False):
    return {n: np.stack([_expm(div.nstates, float(r) * float(lengths[n]), wide) for r in div.cat_rates]) for n in div.tree.all_down_pass}


def tip_vector(div, tip):
    S, P = div.nstates, div.npatterns
    st = np.asarray(div.tip_states[tip])
    one = np.ones((P, S))
    ok = st < S
    one[ok] = 0.0
    one[np.arange(P)[ok], st[ok]] = 1.0
    return one


def post_order(div, mats):
    t, K = div.tree, div.ncat
    cl = {tip: np.broadcast_to(tip_vector(div, tip), (K, div.npatterns, div.nstates)) for tip in range(t.ntaxa)}
    for p in t.int_down_pass:
        out = np.ones((K, div.npatterns, div.nstates))
        for c in (t.left[p], t.right[p]):
            out = out * np.einsum("kij,kcj->kci", mats[c], cl[c])
        cl[p] = out
    return cl


def site_likelihoods(div, lengths, wide=False):
    t = div.tree
    mats = matrices_of(div, lengths, wide)
    cl = post_order(div, mats)
    top = t.root_left
    return np.einsum("k,i,kci,kij,kcj->c", div.category_weights(0), np.asarray(div.pi, dtype=np.float64), cl[top], mats[top], cl[t.root])


def log_likelihood(div, lengths):
    return float((div.weights * np.log(site_likelihoods(div, lengths))).sum())


def lengths_of(div):
    return {n: branch_length(div.tree, n) for n in div.tree.all_down_pass}


def kappa_max(div):
    """the cancellation inside the spectral sums of the division's matrices, as tests/pruning_reference.kappa takes it for real systems"""
    es = div.eigen[0]
    ref = cr.ComplexMatrixReference(es.evec, es.ivec, es.eval, es.imag)
    worst = 1.0
    for tl in sorted(set(lengths_of(div).values())):
        for order in (0, 1, 2):
            X, _, mag = ref.matrices(np.asarray(div.cat_rates, dtype=np.float64), tl, order)
            m = np.abs(mr.to_float(X))
            for k in range(m.shape[0]):
                keep = m[k] > 1e-6 * m[k].max()
                worst = max(worst, float((mag[k][keep] / m[k][keep]).max()))
    return worst


@functools.lru_cache(maxsize=None)
def gradient_reference(states, ncat, npat):
    """tests/preorder_reference.reference for the non-reversible division, its matrices from expm: per node d, N, A, L and the
    S x S matrix M_n of tests/test_cross_products.reference"""
    div = division(states, ncat, npat)
    t = div.tree
    lengths = lengths_of(div)
    mats = matrices_of(div, lengths)
    post = post_order(div, mats)
    w, pi, r = div.category_weights(0), np.asarray(div.pi, dtype=np.float64), np.asarray(div.cat_rates, dtype=np.float64)
    Q = div.rate_matrices[0]
    D = r[:, None, None] * Q[None, :, :]
    top = t.root_left
    # a non-reversible model cannot turn the root branch round: the process starts at the top interior node with pi, the root tip
    # is its third child.  `pre` of the top node is what reaches it from outside its two subtrees; the ROOT BRANCH is read at the
    # root tip: (pre, post) = (P_top^T (pi post_top), tip_root), stored under `top` below
    pre = {top: pi[None, None, :] * np.einsum("kij,cj->kci", mats[top], tip_vector(div, t.root))}
    for p in reversed(t.int_down_pass):
        for n, sib in ((t.left[p], t.right[p]), (t.right[p], t.left[p])):
            pre[n] = np.einsum("kij,kci->kcj", mats[n], pre[p] * np.einsum("kij,kcj->kci", mats[sib], post[sib]))
    Lk = np.einsum("kcl,kcl->kc", pre[top], post[top])
    pre[top] = np.einsum("kij,kci->kcj", mats[top], pi[None, None, :] * post[top])
    post = dict(post)
    post[top] = np.broadcast_to(tip_vector(div, t.root), pre[top].shape)

    def depth_of(n):
        d = 1
        while n != top:
            n, d = t.anc[n], d + 1
        return d
    dmax = max(depth_of(n) for n in range(t.ntaxa) if n != t.root)
    res = {"nodes": list(t.all_down_pass), "lengths": lengths, "h": (dmax - 1) + dmax}
    qk = w[:, None] * Lk
    qk = qk / qk.sum(axis=0)[None, :]
    for n in t.all_down_pass:
        N = np.einsum("k,kcl,klj,kcj->c", w, pre[n], D, post[n])
        A = np.einsum("k,kcl,klj,kcj->c", w, pre[n], np.abs(D), post[n])
        L = np.einsum("k,kcl,kcl->c", w, pre[n], post[n])
        den = np.einsum("kcl,kcl->kc", pre[n], post[n])
        M = np.einsum("kc,kci,kcj->ij", div.weights[None, :] * qk * r[:, None] / den, pre[n], post[n])
        res[n] = dict(d=N / L, N=N, A=A, L=L, M=M)
    return res


def check_tree(lib, states, ncat, npat, double_precision):
    """lnL and per-site lnL against the pruning reference; at 4 and 20 states the gradient in the branch lengths against central
    differences of the reference's log-likelihood, and sum_ij X[i,j] Q[i,j] = sum_e t_e d lnL / dt_e on the cross products"""
    dbl = double_precision
    div = division(states, ncat, npat)
    t, S, w = div.tree, div.nstates, div.weights
    lengths = lengths_of(div)
    Lref = site_likelihoods(div, lengths, wide=dbl)
    ref_sum = float(np.dot(w, np.log(Lref)))
    gradients = states in (4, 20)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=dbl, pre_order=gradients)
    try:
        assert bd.inst.details.flags & COMPLEX, hex(bd.inst.details.flags)
        lnl = bd.LogLike(0)
        site = bd.inst.get_site_log_likelihoods().copy()
        bd.AcceptMove(0)
        # the project's own tolerances for this precision (tests/engine_checks.py): the sum within REL_FP64 (single) or ABS_F64 +
        # REL_F64 |ref| (double); every site |L / L_ref - 1| <= (2 ntaxa - 2) (S + 8) u kappa -- check_double_precision_general_paths'
        # bound, u = 2^-53 with the cancellation of the spectral sums; single precision: u = 2^-24, matrices rounded once from double
        u = U64 * kappa_max(div) if dbl else U32
        worst_site = float(np.abs(np.exp(site - np.log(Lref)) - 1.0).max())
        site_bound = (2 * t.ntaxa - 2) * (S + 8) * u
        print("nrev%d x %d x %d%s: lnL %.9f (reference %.9f), worst site error / bound %.3g" %
              (states, ncat, npat, " fp64" if dbl else "", lnl, ref_sum, worst_site / site_bound))
        if dbl:
            assert abs(lnl - ref_sum) <= ABS_F64 + REL_F64 * abs(ref_sum), (lnl, ref_sum)
        else:
            assert abs(lnl - ref_sum) / abs(ref_sum) < REL_FP64, (lnl, ref_sum)
        assert worst_site <= site_bound, (worst_site, site_bound)
        if not gradients:
            return
        # the gradient against central differences of the reference: the step and the tolerance of
        # tests/test_preorder_gradient.test_reference_against_finite_differences (2e-6 relative to |g| + 1)
        grad = bd.BranchGradient(0)
        g = gradient_reference(states, ncat, npat)
        nodes = g["nodes"]
        assert sorted(grad) == sorted(nodes) and len(grad) == 2 * t.ntaxa - 3
        worst = 0.0
        for n in nodes:
            t0 = lengths[n]
            step = max(1e-4 * t0, 1e-7)
            up, down = dict(lengths), dict(lengths)
            up[n], down[n] = t0 + step, t0 - step
            fd = (log_likelihood(div, up) - log_likelihood(div, down)) / (2.0 * step)
            worst = max(worst, abs(fd - grad[n]) / (abs(grad[n]) + 1.0))
        print("nrev%d%s: BranchGradient against central differences: worst relative difference %.2e" % (states, " fp64" if dbl else "", worst))
        assert worst <= 2e-6, worst
        # the identity, with the slack tests/test_cross_products.check_case gives it
        X = bd.RateMatrixCrossProducts(0)
        tl = [lengths[n] for n in nodes]
        f = bound_factor(div, g, u)
        Xr = sum(x * g[n]["M"] for n, x in zip(nodes, tl))
        gb = {n: (S + 8) * (1 + 2 * g["h"]) * u * (g[n]["A"] + np.abs(g[n]["N"])) / g[n]["L"] for n in nodes}
        Q = div.rate_matrices[0]
        lhs, rhs = float((Q * X).sum()), sum(x * grad[n] for n, x in zip(nodes, tl))
        slack = float((np.abs(Q) * f * np.abs(Xr)).sum()) + sum(x * float((w * gb[n]).sum()) for n, x in zip(nodes, tl))
        print("nrev%d%s: sum Q X = %.9g, sum t g = %.9g, difference / slack %.3f" % (states, " fp64" if dbl else "", lhs, rhs, abs(lhs - rhs) / slack))
        assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)
    finally:
        bd.finalize()


TREE_CASES = [pytest.param(4, 4, 130, False, id="fp32-nrev4"), pytest.param(20, 4, 70, False, id="fp32-nrev20"),
              pytest.param(61, 2, 70, False, id="fp32-nrev61"), pytest.param(4, 4, 130, True, id="fp64-nrev4"),
              pytest.param(20, 4, 70, True, id="fp64-nrev20")]


@pytest.mark.parametrize("states,ncat,npat,double_precision", TREE_CASES)
def test_tree_on_emulation(emu, states, ncat, npat, double_precision):
    check_tree(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", TREE_CASES)
def test_tree(gpu, states, ncat, npat, double_precision):
    check_tree(gpu, states, ncat, npat, double_precision)


def check_sharded(lib, monkeypatch):
    """a complex instance under MBAMD_SHARD=2: two children (the flag travels with the dimensions), per-site lnL bit-equal"""
    div = division(4, 4, 130)
    got = []
    for shards in (None, "2"):
        monkeypatch.delenv("MBAMD_SHARD", raising=False)
        if shards:
            monkeypatch.setenv("MBAMD_SHARD", shards)
        try:
            bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS)
        finally:
            monkeypatch.delenv("MBAMD_SHARD", raising=False)
        try:
            assert bd.inst.details.flags & COMPLEX and bd.inst.child_count() == (2 if shards else 1)
            bd.LogLike(0)
            got.append(bd.inst.get_site_log_likelihoods().copy())
        finally:
            bd.finalize()
    assert np.isfinite(got[0]).all() and np.array_equal(got[0], got[1])


def test_sharded_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


def check_two_partitions(lib):
    """beagleSetPatternPartitions on a complex instance: the child engines are complex too -- per-partition sums equal to two single
    instances (engine_checks.check_multi_partition_instance's layout and tolerance)"""
    divs = [division(4, 4, 130), synthetic_division("nrev4", NTAXA, 70, seed=23, tree_seed=9, alpha=0.4, ncat=4, p_gap=0.05)]
    S, K, N = 4, 4, NTAXA
    want = [engine_lnl(lib, d) for d in divs]
    Pa, Pb = divs[0].npatterns, divs[1].npatterns
    nInt, nNodes = N - 2, 2 * N - 2
    inst = complex_instance(lib, N, N + nInt, N, S, Pa + Pb, 2, 2 * nNodes, K, nInt + 2)
    try:
        for t in range(N):
            inst.set_tip_states(t, np.concatenate([divs[0].tip_states[t], divs[1].tip_states[t]]).astype(np.int32))
        inst.set_pattern_weights(np.concatenate([divs[0].weights, divs[1].weights]))
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(Pa, dtype=np.int32), np.ones(Pb, dtype=np.int32)]))
        assert inst.child_count() == 2
        ops, eig_idx, rate_idx, prob_idx, lengths = [], [], [], [], []
        for d, dv in enumerate(divs):
            es = dv.eigen[0]
            inst.set_eigen_decomposition(d, es.evec, es.ivec, es.values)
            inst.set_state_frequencies(d, dv.pi)
            inst.set_category_weights(d, dv.category_weights(0))
            inst.set_category_rates_with_index(d, dv.cat_rates)
            tr = dv.tree
            for p in tr.all_down_pass:
                if p == tr.root:
                    continue
                eig_idx.append(d); rate_idx.append(d); prob_idx.append(d * nNodes + p)
                lengths.append(branch_length(tr, p))
            for p in tr.int_down_pass:
                l, r = tr.left[p], tr.right[p]
                ops.append([p, p - N, -1, l, d * nNodes + l, r, d * nNodes + r, d, nInt + d])
        inst.update_transition_matrices_with_multiple_models(eig_idx, rate_idx, prob_idx, lengths)
        for d in range(2):
            inst.reset_scale_factors_by_partition(nInt + d, d)
        inst.update_partials_by_partition(np.array([x for pair in zip(ops[:nInt], ops[nInt:]) for x in pair], dtype=np.int32))
        parents = [divs[d].tree.root_left for d in range(2)]
        rc, by, total = inst.calculate_edge_log_likelihoods_by_partition(parents, [divs[d].tree.root for d in range(2)],
                                                                         [d * nNodes + parents[d] for d in range(2)], [0, 1], [0, 1],
                                                                         [nInt, nInt + 1], [0, 1], 1)
        assert rc == 0
        for d in range(2):
            assert abs(by[d] - want[d]) <= 1e-10 * abs(want[d]), (d, by[d], want[d])
        assert abs(total - sum(want)) <= 1e-10 * abs(total)
    finally:
        inst.finalize()


def test_two_partitions_on_emulation(emu):
    check_two_partitions(emu)


@pytest.mark.gpu
def test_two_partitions(gpu):
    check_two_partitions(gpu)


# ---- D. arguments -------------------------------------------------------------------------------------------------------------------
def _raises(lib, code, call, *args, **kwargs):
    with pytest.raises(bg.BeagleError) as err:
        call(*args, **kwargs)
    assert err.value.code == code, (err.value.code, code)
    assert lib.last_error()


def check_arguments(lib, double_precision):
    dbl = double_precision
    S, K = 5, 2
    dims = (2, 3, 2, S, 5, 2, 6, K, 1)
    rng = np.random.default_rng(53)
    # both eigen flags required
    _raises(lib, bg.BEAGLE_ERROR_NO_IMPLEMENTATION, bg.BeagleInstance, lib, *dims, preference_flags=preference(dbl),
            requirement_flags=COMPLEX | bg.BEAGLE_FLAG_EIGEN_REAL)
    _, V, Vi, a, b, _ = rate_matrix_system(S)
    p = int(np.flatnonzero(b != 0)[0])
    rates = np.array([0.7, 1.9])
    # the preference flag alone makes a complex instance; with EIGEN_REAL required it does not
    for pref_only in (True, False):
        inst = bg.BeagleInstance(lib, *dims, preference_flags=preference(dbl) | COMPLEX, requirement_flags=0 if pref_only else bg.BEAGLE_FLAG_EIGEN_REAL)
        try:
            assert bool(inst.details.flags & COMPLEX) == pref_only and bool(inst.details.flags & bg.BEAGLE_FLAG_EIGEN_REAL) != pref_only
        finally:
            inst.finalize()
    inst = bg.BeagleInstance(lib, *dims, preference_flags=preference(dbl) | COMPLEX)
    try:
        inst.set_category_rates(rates)
        inst.set_eigen_decomposition(0, V, Vi, np.concatenate([a, b]))
        inst.update_transition_matrices(0, [0], [0.3])
        X, W, _ = cr.ComplexMatrixReference(V, Vi, a, b).matrices(rates, 0.3, 0)
        assert bound_ratio(inst.get_transition_matrix(0), X, W, dbl) <= 1.0, "the preference flag: the imaginary parts are read"
        bad = b.copy()
        bad[p + 1] = 0.0                               # an unpaired imaginary part
        _raises(lib, bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.set_eigen_decomposition, 0, V, Vi, np.concatenate([a, bad]))
        bad = np.zeros(S)
        bad[S - 1] = 0.5                               # ... at the last index
        _raises(lib, bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.set_eigen_decomposition, 0, V, Vi, np.concatenate([a, bad]))
        bad = b.copy()
        bad[p + 1] = -np.nextafter(b[p], 2.0 * b[p])   # ... a conjugate that is not exact
        _raises(lib, bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.set_eigen_decomposition, 0, V, Vi, np.concatenate([a, bad]))
        bad = a.copy()
        bad[p + 1] = np.nextafter(a[p], 0.0)           # a pair with unequal real parts
        _raises(lib, bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.set_eigen_decomposition, 0, V, Vi, np.concatenate([bad, b]))
        for where in (0, S - 1, S + p, 2 * S - 1):     # a non-finite value
            for value in (np.nan, np.inf):
                bad = np.concatenate([a, b])
                bad[where] = value
                _raises(lib, bg.BEAGLE_ERROR_OUT_OF_RANGE, inst.set_eigen_decomposition, 0, V, Vi, bad)
        # (the refused calls left the system as it was)
        inst.update_transition_matrices(0, [1], [0.3])
        assert np.array_equal(inst.get_transition_matrix(1), inst.get_transition_matrix(0))
        if not dbl:
            # mbamdSetRateMatrices over an index that held a complex system: the reversible solver's system with zero imaginary parts
            # -- matrices within the REAL bound of tests/test_matrix_bounds.py, from the eigen-system numpy gives for the same matrix
            # (the device's Jacobi iteration and numpy's eigh differ by a few units of 2^-53, far inside the bound's half float ulp)
            U, Ui, lam = mr.reversible_system(rng, S, "ordinary")
            qrev = (U * lam[None, :]) @ Ui
            pi = Ui[np.argmax(lam)] / Ui[np.argmax(lam)].sum()          # (the left eigenvector of the eigenvalue 0)
            inst.set_rate_matrices(0, qrev[None, :, :], pi)
            inst.update_transition_matrices(0, [2], [0.3], first=[3])
            for o, m in ((0, 2), (1, 3)):
                X, W, _ = mr.MatrixReference(U, Ui, lam).matrices(rates, 0.3, o)
                assert bound_ratio(inst.get_transition_matrix(m), X, W, False) <= 1.0, ("after mbamdSetRateMatrices", o)
    finally:
        inst.finalize()
    # an instance created without the flag behaves as today: S eigenvalues, EIGEN_REAL
    inst = bg.BeagleInstance(lib, *dims, preference_flags=preference(dbl))
    try:
        assert inst.details.flags & bg.BEAGLE_FLAG_EIGEN_REAL and not inst.details.flags & COMPLEX
        U, Ui, lam = mr.reversible_system(rng, S, "ordinary")
        inst.set_category_rates(rates)
        # (what lies behind the S eigenvalues is not read: NaN there changes nothing)
        inst.set_eigen_decomposition(0, U, Ui, lam)
        inst.update_transition_matrices(0, [0], [0.3])
        X, W, _ = mr.MatrixReference(U, Ui, lam).matrices(rates, 0.3, 0)
        assert bound_ratio(inst.get_transition_matrix(0), X, W, dbl) <= 1.0
        with pytest.raises(ValueError):
            inst.set_eigen_decomposition(0, U, Ui, np.concatenate([lam, np.zeros(S)]))
    finally:
        inst.finalize()


@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
def test_arguments_on_emulation(emu, double_precision):
    check_arguments(emu, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("double_precision", [False, True], ids=["fp32", "fp64"])
def test_arguments(gpu, double_precision):
    check_arguments(gpu, double_precision)


# ---- the python layer -----------------------------------------------------------------------------------------------------------------
def test_eigen_general_and_nrev_division():
    """eigen_general: the block form reproduces Q, pairs are adjacent; transition_matrices with imaginary parts equals expm; the `nrev`
    rate matrix has pi as its stationary distribution, one expected substitution per unit time and is not reversible"""
    for S in (3, 4, 5, 20, 61):
        q, pi = mbmodel.nonreversible_q(S)
        assert np.allclose(q.sum(axis=1), 0.0, atol=1e-13) and np.allclose(pi @ q, 0.0, atol=1e-13) and (pi > 0).all()
        assert abs(-(pi * np.diag(q)).sum() - 1.0) <= 1e-13
        flow = pi[:, None] * q
        assert not np.allclose(flow, flow.T)
        es = mbmodel.eigen_general(q)
        cr.pairs_of(es.imag)
        assert np.abs(es.evec @ mbmodel.eigen_blocks(es, es.eval + 1j * es.imag) @ es.ivec - q).max() <= 1e-12
        P = mbmodel.transition_matrices(es, 0.3, [0.5, 2.0])
        for k, r in enumerate((0.5, 2.0)):
            assert np.abs(P[k] - scipy.linalg.expm(q * 0.3 * r)).max() <= 1e-12
    rev = mbmodel.EigenSystem(*mr.reversible_system(np.random.default_rng(3), 4, "ordinary"))
    assert rev.imag is None and rev.values is rev.eval


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_reference_against_mpmath():
    """The longdouble reference against mpmath at 50 digits, as test_matrix_bounds.test_reference_against_mpmath: the entries of
    smallest and largest magnitude and a few random ones agree to 2^-58 of the sum of the term magnitudes, at every state count of
    part A and every kind of system.  And the spectral sum itself against mpmath.expm, for the systems that come from a rate
    matrix: with V^-1 the inverse of V to 64 bits the doubles define ONE matrix Q' = V D V^-1 (formed in mpmath), and the reference
    must give (r Q')^o expm(Q' r t) -- up to 8 states at three points, at 15 ... 17 states at one (mpmath's expm takes seconds beyond)."""
    rng = np.random.default_rng(59)
    worst = worst_expm = 0.0
    points = [(1.3e-6, 1e-8), (0.7, 0.1), (12.4, 100.0), (1.0, 2.5), (0.0, 0.1)]
    for S in sorted(set(SHAPES_F32) | set(SHAPES_F64)):
        for kind, V, Vi, a, b, Q in systems_of(rng, S):
            ref = cr.ComplexMatrixReference(V, Vi, a, b)
            r, t = points[int(rng.integers(len(points)))] if S > 33 else (None, None)
            for rate, length in (points if S <= 33 else [(r, t)]):
                for order in (0, 1, 2):
                    X, _, mag = ref.matrices(np.array([rate]), length, order)
                    m0 = np.abs(mr.to_float(X[0])).reshape(-1)
                    by_size = np.argsort(m0)
                    picks = set(by_size[:3].tolist() + by_size[-2:].tolist() + rng.integers(0, S * S, size=3).tolist())
                    for e in picks:
                        i, j = divmod(int(e), S)
                        want, m = cr.mpmath_entry(V, Vi, a, b, rate, length, order, i, j)
                        with mpmath.workdps(50):
                            diff = float(abs(mr.to_mpf(X[0, i, j]) - want))
                        assert abs(m - mag[0, i, j]) <= 1e-12 * m
                        if m > 0:
                            worst = max(worst, diff / m)
                        assert diff <= 2.0 ** -58 * m, (S, kind, rate, length, order, i, j, diff, m)
            if Q is None or S > 17 or not LONGDOUBLE_QUALIFIES:
                continue
            Vi_mp = cr.mp_inverse(V)
            ref = cr.ComplexMatrixReference(V, cr.to_wide(Vi_mp), a, b)
            with mpmath.workdps(50):
                Qp = cr.mp_block_matrix(V, Vi_mp, a, b)
                assert max(abs(Qp[i, j] - mpmath.mpf(float(Q[i, j]))) for i in range(S) for j in range(S)) <= 1e-11
            for rate, length in ([(0.7, 0.1), (1.0, 2.5), (12.4, 1.0)] if S <= 8 else [(1.0, 2.5)]):
                with mpmath.workdps(50):
                    E = mpmath.expm(Qp * mpmath.mpf(rate) * mpmath.mpf(length))
                    by_order = [E, Qp * mpmath.mpf(rate) * E, Qp * Qp * mpmath.mpf(rate) ** 2 * E]
                for order in (0, 1, 2):
                    X, _, mag = ref.matrices(np.array([rate]), length, order)
                    for i in range(S):
                        for j in range(S):
                            with mpmath.workdps(50):
                                want = by_order[order][i, j]
                                want = mpmath.mpf(0) if order == 0 and want < 0 else want
                                diff = float(abs(mr.to_mpf(X[0, i, j]) - want))
                            worst_expm = max(worst_expm, diff / mag[0, i, j])
                            assert diff <= 2.0 ** -58 * mag[0, i, j], (S, kind, "expm", rate, length, order, i, j, diff, mag[0, i, j])
    print("COMPLEX REFERENCE longdouble against mpmath: worst difference / term magnitudes 2^%.1f (spectral sum), 2^%.1f (expm)" %
          (np.log2(worst) if worst > 0 else -np.inf, np.log2(worst_expm) if worst_expm > 0 else -np.inf))
