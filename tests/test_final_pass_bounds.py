"""The final ("up") pass and the scaled read-out of the single-precision engine (mbamdUpdateFinalPartials, mbamdGetScaledPartials;
csrc/mbamd_reports.h, Instance::finalPass / getScaledPartials, the shard gather of mbamd_engine.cpp) against a-priori bounds.

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X -- there the double division, frexp / ldexp, ldexpf and the float conversions are the
    device libraries', not the host's libm.

The reference is tests/final_pass_reference.py on tests/operation_reference.py: np.longdouble (unit roundoff 2^-64 on x86; exact
Fractions where longdouble is no wider than double).  Every input is rounded to float32 BEFORE it goes to the engine and to the
reference, and set / get are asserted to round-trip it bit for bit: the bounds concern arithmetic only.  The double-precision engine
refuses both calls (asserted by check_handle_roles); nothing here concerns it.

Every term of every sum is non-negative, so these relative bounds hold for any order of summation.  u = 2^-53 (k_final_pass widens
every float to double and rounds ONCE, on the store):

  A. one step, per element
     top node      U[a] = down[a] f[a],  f[a] = sum_j P[a][j] tip[j]: the products of two floats are exact in double, S - 1 additions,
                   one product, an exact power of two, one rounding to float:        B_top  = (S + 2) u + 2^-24
                   held on the TRUE value got 2^e, e the integer behind the read-out's lnScale.
     a step below  s[a] = sum_i P[a][i] d[i] (exact products, S - 1 additions), the quotient (1), the products u[i] P[a][i] (1 each) and
                   S - 1 additions, the product with d[a] (1), one rounding to float:  B_step = (2 S + 5) u + 2^-24
                   held on the stored buffer against the recurrence evaluated on the ancestor's final partials AS STORED (read back).
     (S u and (2 S + 1) u to first order; the two and four spare units cover the higher-order terms.)  The float rounding dominates, so the
     worst error / bound sits just under 1: one float operation too many about doubles the error.
     Where the value owed lies below 2^-126 in the scale it is delivered in, the bound cannot hold (float32 has fewer bits there): the
     correctly rounded subnormal -- |got - want| <= 2^-150 + bound want; twice 2^-150 for the top node, whose stored subnormal the
     read-out shifts and rounds again -- or zero is accepted; `hold` counts both.  One pattern per buffer has state 0 about 128 binades
     below the rest of its column, so that every step meets such values.

  B. a whole tree through the real calls, per element and per site.  Recursively, with B_op = (2 S + 4) 2^-24 per down-pass operation
     (tests/test_operation_bounds.py) and beta(tip) = 0:
         beta(p)    = (1 + beta(left)) (1 + beta(right)) (1 + B_op) - 1                        down partials of p
         gamma(top) = (1 + beta(top)) (1 + B_top) - 1                                            (the root tip and its matrix are data)
         gamma(p)   = (1 + gamma(anc)) (1 + beta(p)) (1 + B_step) / (1 - beta(p)) - 1            s carries beta(p) and DIVIDES
     held on got 2^emax.  Loose (1e-5 ... 1e-4): this part is for the exponent bookkeeping, where an error is a factor of two or more.
     The reference itself is checked on its own data: sum_k w_k sum_a pi_a final_k[a] is the site likelihood at EVERY interior node if
     pi_a P[a][i] = pi_i P[i][a]; the matrices are the engine's floats, so per step the identity is off by at most
         tau(p) - tau(anc) = sum_k w_k sum_a sum_i |pi_a P[a][i] - pi_i P[i][a]| u[i] d[a]      (evaluated by the reference, absolute)
     -- a few 2^-24 of the likelihood with P[a][i] in the second sum, and tens of percent with P[i][a] unless pi is uniform.
     The engine's read-out is held to the same invariant against beagleGetSiteLogLikelihoods:
         |ln sum_k w_k sum_a pi_a (got 2^emax) - lnL_c| <= 1.01 (gamma(p) + tau(p) / L_c) + the site bound of test_operation_bounds.py
     with B = (1 + B_op)^m (1 + B_edge) - 1 over the m operations of the tree (|ln(1 + x)| <= 1.01 |x| below 0.01).

  C. the read-out, exactly: out = raw 2^(e_k - emax) is a power-of-two scaling -- bit for bit where the exact result is >= 2^-126, the
     nearest-even subnormal or zero below --, emax the largest exponent over the categories with any non-zero value (0 without one),
     lnScale = float32(emax ln 2); the exponents are the cumulative buffer's plus, for final partials, the pass's own.

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import functools

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd.division import synthetic_division
from tests import final_pass_reference as fp
from tests.hostemu import build_emu
from tests.operation_reference import Reference, dense_tip
from tests.test_operation_bounds import edge_bound, expected_layout, operation_bound, site_bound

NONE = bg.BEAGLE_OP_NONE
REF = Reference()
U = 2.0 ** -53
F32_MAX_BINADE = 2.0 ** 127
# B_op, the down pass's bound, is claimed for normal floats (the bf16 pieces of 40 and 60-63 states need their operands
# above about 2^-110): a down-pass value that is at least this in the scale it is stored in is the product of two sums that are at
# least this as well, and a term of such a sum that underflows is off by 2^-150 -- 2^-42 of the sum
NORMAL_MARGIN = 2.0 ** -108


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def top_bound(S):
    return (S + 2) * U + 2.0 ** -24


def step_bound(S):
    return (2 * S + 5) * U + 2.0 ** -24


def f32(a):
    """`a` rounded to float32, as the float64 array both the engine and the reference take"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64))


def as_f32(a):
    """a float64 array read from the engine, which holds float32 values: the same values as float32 (asserted)"""
    b = np.asarray(a).astype(np.float32)
    assert np.array_equal(b.astype(np.float64), a)
    return b


class Tally:
    """what `hold` and `exact_read_out` met: the worst error / bound; of the values owed below 2^-126 whose nearest float32 is not zero,
    how many came as subnormals and how many as zeros"""

    def __init__(self):
        self.worst, self.subnormal, self.flushed = 0.0, 0, 0

    def __str__(self):
        return "worst error / bound %.3f; below 2^-126: %d kept as subnormals, %d zero" % (self.worst, self.subnormal, self.flushed)


def hold(got, emax, want, bound, what, tally, columns=None, roundings=1):
    """The engine's float32 values `got` [K][P][S], delivered in the scale 2^-emax[c], against the reference's TRUE values `want`:
    |got 2^emax - want| <= bound want where want 2^-emax >= 2^-126, the rounded subnormal or zero below, zero where want is zero.
    `columns` [K][P]: the columns held to it (all of them by default); the others must be finite, and zero where want is zero.
    `roundings`: how many roundings to float32's subnormal grid lie between the double result and `got` (2^-150 each)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and np.isfinite(got).all() and np.all(got >= 0), what
    e3 = np.broadcast_to(np.asarray(emax, dtype=np.int64)[None, :, None], got.shape)
    true = REF.scaled(got, e3)
    zero = np.asarray(want == 0, dtype=bool)
    assert np.all(got[zero] == 0), (what, "non-zero where the reference is zero", np.argwhere(zero & (got != 0))[:4].tolist())
    err = np.abs(true - want)
    w_out = np.ldexp(REF.to_float(want), (-e3).astype(np.int32))            # (classification and the subnormal allowance only)
    held = np.ones(got.shape, dtype=bool) if columns is None else np.broadcast_to(np.asarray(columns, dtype=bool)[:, :, None], got.shape)
    normal = held & ~zero & (w_out >= fp.SMALLEST_NORMAL)
    ratio = 0.0
    if normal.any():
        rel = REF.to_float(err[normal] / want[normal]) / bound
        ratio = float(rel.max())
        assert ratio <= 1.0, (what, "worst error / bound %.4f" % ratio, np.argwhere(normal)[int(rel.argmax())].tolist())
    sub = held & ~zero & ~normal
    if sub.any():
        err_out = np.ldexp(REF.to_float(err[sub]), (-e3[sub]).astype(np.int32))
        kept = got[sub] != 0
        assert np.all(~kept | (err_out <= roundings * 2.0 ** -150 + bound * w_out[sub])), (what, "a subnormal result is not the rounded one")
        tally.subnormal += int(kept.sum())
        tally.flushed += int((~kept & (w_out[sub] > 2.0 ** -150)).sum())
    tally.worst = max(tally.worst, ratio)
    return ratio


def exact_read_out(got, ln, raw, exponents, what, tally):
    """a read-out (got, ln) against the integer model of `raw` with `exponents`; returns the model's emax and shifts"""
    out, rounded, ln_model, emax, shift = fp.read_out(raw, exponents)
    assert got.dtype == np.float32 and ln.dtype == np.float32
    assert np.array_equal(ln, ln_model), (what, np.argwhere(ln != ln_model)[:4].tolist())
    sub = (out != 0) & (out < fp.SMALLEST_NORMAL)
    exact = out.astype(np.float32)
    assert np.array_equal(got[~sub], exact[~sub]), (what, np.argwhere(~sub & (got != exact))[:4].tolist())
    kept = got[sub] != 0
    assert np.array_equal(got[sub][kept], rounded.astype(np.float32)[sub][kept]), (what, "a subnormal result is not the rounded one")
    tally.subnormal += int(kept.sum())
    tally.flushed += int((~kept & (rounded[sub] != 0)).sum())
    return emax, shift


def column_exponents(raw, scaled, emax, owed=None):
    """The exponent of every (category, pattern) column of a final-pass buffer, from the buffer and its read-out WITHOUT a cumulative
    buffer: scaled = raw 2^(e_kc - emax_c) at the column's largest element (asserted to be an exact power of two apart); 0 for a dead
    column, whose exponent no read-out shows.  `owed` = (exponents, near): frexp's of the reference's column maxima and which of
    them lie within the bound of a power of two -- asserted where they decide, and taken where the read-out shifted the column's
    largest element out of the normal range (categories more than a hundred binades apart), which then must not be `near`."""
    idx = raw.argmax(axis=2)[:, :, None]
    r = np.take_along_axis(np.asarray(raw, dtype=np.float64), idx, 2)[:, :, 0]
    s = np.take_along_axis(np.asarray(scaled, dtype=np.float64), idx, 2)[:, :, 0]
    live = r > 0
    shown = live & (s >= fp.SMALLEST_NORMAL)
    m, sh = np.frexp(np.where(shown, s / np.where(shown, r, 1.0), 1.0))
    assert np.all(m == 0.5)
    e = np.where(shown, np.asarray(emax)[None, :] + sh - 1, 0).astype(np.int64)
    if owed is None:
        assert np.array_equal(shown, live), "a column's largest element left the normal range in the read-out: choose closer categories"
        return e
    want, near = owed
    assert np.array_equal(e[shown & ~near], want[shown & ~near]) and not near[live & ~shown].any() and np.all(want[~live] == 0)
    return np.where(shown, e, want)


# ---- A. one step, element by element -------------------------------------------------------------------------------------------------
# buffers: 0 compact root tip; 2, 3, 4 down partials of top, a, b; 5 a root tip given as partials; 6, 7, 8 final partials.  Matrices 0, 1, 2.
ZERO_TOP, ZERO_TOP_CAT0, ZERO_TIP = 21, 23, 25            # top's down buffer: all zero / zero in category 0; the partials tip: all zero
ZERO_ALL, ZERO_CAT0, ZERO_STATE0, ZERO_BUT_ONE = 3, 5, 7, 9       # down buffer of a; of b ten patterns further
TINY_TOP, TINY_STEP = 29, 27                              # state 0 about 128 binades below the rest of its column: a result below 2^-126


def matrices_of_kind(rng, S, K, kind):
    """`dense`: positive.  `sparse`: about 70 % zeros, the diagonal positive.  `identity`: sparse, and the LAST step's last category
    the identity.  Rows sum to one before the rounding to float32."""
    out = []
    for n in range(3):
        m = rng.random((K, S, S)) + 0.05
        if kind != "dense":
            m = m * ((rng.random((K, S, S)) < 0.3) | np.eye(S, dtype=bool)[None, :, :])
        m = m / m.sum(axis=2, keepdims=True)
        if kind == "identity" and n == 2:
            m[K - 1] = np.eye(S)
        out.append(f32(m))
    return out


def spread_partials(rng, S, K, P):
    """columns over 2^-90 ... 2^0, the elements of a column over another 12 binades: the smallest about 2^-107, a normal float"""
    ex = rng.permutation(np.linspace(-90, 0, K * P).round()).reshape(K, P, 1)
    el = rng.integers(-12, 1, size=(K, P, S)).astype(np.float64)
    return (rng.random((K, P, S)) * 0.9 + 0.05) * np.exp2(ex + el)


def check_steps(lib, S, K, P, seed=1):
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    label = "%2d states x %d x %3d" % (S, K, P)
    Bt, Bs = top_bound(S), step_bound(S)
    inst = bg.BeagleInstance(lib, 2, 12, 2, S, P, 1, 4, K, 4)
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name, name
        st = rng.permutation(np.arange(P) % (S + 1)).astype(np.int32)         # every code 0 ... S: the missing one included
        inst.set_tip_states(0, st)
        down = [spread_partials(rng, S, K, P) for _ in range(3)]
        down[0][:, ZERO_TOP, :] = 0.0
        down[0][0, ZERO_TOP_CAT0, :] = 0.0
        keep = int(rng.integers(0, S))
        for n, shift in ((1, 0), (2, 10)):
            down[n][:, ZERO_ALL + shift, :] = 0.0
            down[n][0, ZERO_CAT0 + shift, :] = 0.0
            down[n][:, ZERO_STATE0 + shift, 0] = 0.0
            down[n][:, ZERO_BUT_ONE + shift, np.arange(S) != keep] = 0.0
        for n, c in ((0, TINY_TOP), (1, TINY_STEP), (2, TINY_STEP + 10)):
            down[n][:, c, :] = (rng.random((K, S)) * 0.9 + 0.05) * 2.0 ** 8
            down[n][:, c, 0] = (rng.random(K) * 0.5 + 0.5) * 2.0 ** -120
        down = [f32(d) for d in down]
        amb = rng.random((K, P, S)) * 0.9 + 0.05
        amb[:, ZERO_TIP, :] = 0.0
        amb = f32(amb)
        for n in range(3):
            inst.set_partials(2 + n, down[n])
        inst.set_partials(5, amb)
        for idx, a in ((2, down[0]), (3, down[1]), (4, down[2]), (5, amb)):
            assert np.array_equal(inst.get_partials(idx), a), "partials round trip"
        wd = [REF.widen(d) for d in down]
        tips = {"compact root tip": (0, REF.widen(dense_tip(st, S, K))), "partials root tip": (5, REF.widen(amb)), "rooted": (-1, None)}
        tally = {"top": Tally(), "step": Tally(), "read-out": Tally()}
        for kind in ("dense", "sparse", "identity"):
            ti = matrices_of_kind(rng, S, K, kind)
            for n in range(3):
                inst.set_transition_matrix(n, ti[n])
                assert np.array_equal(inst.get_transition_matrix(n), ti[n]), "matrix round trip"
            wm = [REF.widen(m) for m in ti]
            for form, (root_tip, tip) in tips.items():
                what = "%s, %s matrices, %s" % (label, kind, form)
                inst.update_final_partials(np.array([[6, -1, 2, 0, root_tip], [7, 6, 3, 1, -1], [8, 7, 4, 2, -1]], dtype=np.int32))
                # -- the top node: true values through the read-out, the raw buffer normalised
                want = fp.top(REF, wd[0], None if tip is None else REF.contract(wm[0], tip))
                assert float(REF.to_float(want.max())) < F32_MAX_BINADE
                got, ln = inst.get_scaled_partials(6)
                emax = fp.integer_exponent(ln)
                # (a value below 2^-126 is rounded to the subnormal grid when it is stored and again when the read-out shifts it)
                r_top = hold(got, emax, want, Bt, what + ": top", tally["top"], roundings=2)
                raw = [as_f32(inst.get_partials(6 + n)) for n in range(3)]
                assert all(np.isfinite(r).all() for r in raw), what
                col = raw[0].max(axis=2)
                dead = np.asarray(want.max(axis=2) == 0, dtype=bool)
                assert dead[:, ZERO_TOP].all() and dead[0, ZERO_TOP_CAT0] and not dead[1:, ZERO_TOP_CAT0].any()
                # (the closed upper end is deliberate: a double just below 1, 1 - 2^-30 say, rounds to 1.0f)
                assert np.all((col[~dead] >= 0.5) & (col[~dead] <= 1.0)), (what, col[~dead].min(), col[~dead].max())
                assert np.all(raw[0][dead] == 0) and np.all(emax[dead.all(axis=0)] == 0), what
                # [K][P]: the pass's own exponents (with a sparse matrix the tiny state can be a column's only live one)
                e_col = column_exponents(raw[0], got, emax, REF.exponents(want.max(axis=2), Bt, -(1 << 20), 1 << 20))
                exact_read_out(got, ln, raw[0], e_col, what + ": top read-out", tally["read-out"])
                # -- the steps below: the stored buffer against the recurrence on the ancestor's STORED final partials
                r_step = []
                for n in (1, 2):
                    want = fp.step(REF, REF.widen(raw[n - 1]), wd[n], wm[n])
                    assert float(REF.to_float(REF.scaled(REF.to_float(want), e_col[:, :, None]).max())) < F32_MAX_BINADE
                    r_step.append(hold(raw[n], np.zeros(P, dtype=np.int64), want, Bs, what + ": step %d" % n, tally["step"]))
                    # they inherit the top node's exponents: the read-out is the integer model of the raw buffer with THOSE
                    got_n, ln_n = inst.get_scaled_partials(6 + n)
                    exact_read_out(got_n, ln_n, raw[n], e_col, what + ": read-out of step %d" % n, tally["read-out"])
                print("%s worst error / bound: top %.3f, steps %.3f %.3f" % (what, r_top, r_step[0], r_step[1]))
        assert all(tally[x].subnormal + tally[x].flushed > 0 for x in tally), label              # TINY_TOP, TINY_STEP
        print("%s STEPS top: %s; steps: %s; read-outs: %s; %s" % (label, tally["top"], tally["step"], tally["read-out"], name.split(": ", 1)[-1]))
    finally:
        inst.finalize()
    return tally


#               states, categories, patterns: the 4-state arena, the tree-walk arena (2 ... 10, 20, 61 states), the general tile-major buffer
#               (33, 64 states); a partial last block of 64 patterns everywhere; 64 states = MBAMD_REP_MAXS
STEP_SHAPES = [(4, 1, 65), (4, 4, 130), (2, 2, 129), (7, 3, 70), (20, 4, 70), (33, 1, 70), (33, 2, 70), (61, 2, 40), (64, 1, 66)]


@pytest.mark.parametrize("S,K,P", STEP_SHAPES)
def test_steps_on_emulation(emu, S, K, P):
    check_steps(emu, S, K, P)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,P", STEP_SHAPES)
def test_steps(gpu, S, K, P):
    check_steps(gpu, S, K, P)


# ---- B. a whole tree through the real calls ------------------------------------------------------------------------------------------
#             kind, taxa, patterns
TREE_CASES = [("gtr", 40, 130), ("wag", 16, 70), ("gen33", 12, 70), ("m3", 12, 40)]
SCHEMES = [pytest.param(lk.MB_BEAGLE_SCALE_ALWAYS, id="always"), pytest.param(lk.MB_BEAGLE_SCALE_DYNAMIC, id="dynamic")]


@functools.lru_cache(maxsize=None)
def tree_division(kind, ntaxa, npat):
    return synthetic_division(kind, ntaxa, npat, seed=11, tree_seed=5, p_gap=0.05)


def final_operations(bd, part, nodes=None):
    """the final pass from root_left over the interior nodes in pre-order (`nodes`: only those), into the scratch buffers"""
    t = bd.div.tree
    cl, sc, ti = bd.condLikeIndex[0], bd.condLikeScratchIndex, bd.tiProbsIndex[0]
    ops = []
    for p in reversed(t.int_down_pass):
        if nodes is not None and p not in nodes:
            continue
        if p == t.root_left:
            ops.append([sc[p] + part, -1, cl[p] + part, ti[p] + part, cl[t.root]])
        else:
            ops.append([sc[p] + part, sc[t.anc[p]] + part, cl[p] + part, ti[p] + part, -1])
    return np.asarray(ops, dtype=np.int32)


def cumulative_index(bd, part):
    scaled = bd.scaling == lk.MB_BEAGLE_SCALE_ALWAYS or bd.rescaleBeagleAll
    return bd.siteScalerIndex[0] + part if scaled else NONE


def read_tree(bd, cums):
    """{(node, part): (values, lnScale)} of every interior node, read with the parts' cumulative buffers `cums`"""
    t = bd.div.tree
    return {(p, j): bd.inst.get_scaled_partials(bd.condLikeScratchIndex[p] + j, cums[j]) for p in t.int_down_pass for j in range(bd.step)}


def same_read_outs(a, b, keys=None):
    return all(np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) for k in (keys if keys is not None else a))


@functools.lru_cache(maxsize=None)
def tree_reference(kind, ntaxa, npat, matrix_bytes):
    """The reference's down pass, final pass, site likelihoods and invariant defect for one case on the matrices the engine holds
    (`matrix_bytes`: their float64 bytes, [part][node of all_down_pass][K][S][S]); checked here on its own data."""
    div = tree_division(kind, ntaxa, npat)
    t, S, K, parts = div.tree, div.nstates, div.ncat, div.n_cijk_parts
    mats = np.frombuffer(matrix_bytes, dtype=np.float64).reshape(parts, len(t.all_down_pass), K, S, S)
    F = REF.widen(f32(div.pi))
    src = {n: REF.widen(dense_tip(div.tip_states[n], S, K)) for n in range(t.ntaxa)}
    ops = [(p, t.left[p], t.right[p]) for p in t.int_down_pass]
    top = t.root_left
    out = dict(final=[], W=[], unscaled=[], per_pattern=[], L=0, tau={p: 0 for p in t.int_down_pass}, invariant={p: 0 for p in t.int_down_pass}, F=F)
    for j in range(parts):
        W = REF.widen(f32(div.category_weights(j)))
        wm = {n: REF.widen(mats[j][i]) for i, n in enumerate(t.all_down_pass)}
        down = REF.prune(ops, src, wm)
        final = fp.whole_tree(REF, t, down, wm, REF.contract(wm[top], src[t.root]))
        out["L"] = out["L"] + REF.edge(W, F, down[top], wm[top], src[t.root])
        tau = {top: 0}
        for p in reversed(t.int_down_pass):
            out["invariant"][p] = out["invariant"][p] + REF.einsum("k,a,kca->c", W, F, final[p])
            if p == top:
                continue
            # the step's departure from detailed balance, evaluated as the docstring writes it
            s = REF.einsum("kai,kci->kca", wm[p], down[p])
            live = np.asarray(s != 0, dtype=bool)
            u = final[t.anc[p]] * 0
            u[live] = final[t.anc[p]][live] / s[live]
            defect = np.abs(F[None, :, None] * wm[p] - (F[None, :, None] * wm[p]).transpose(0, 2, 1))
            tau[p] = tau[t.anc[p]] + REF.einsum("k,kai,kci,kca->c", W, defect, u, down[p])
            out["tau"][p] = out["tau"][p] + tau[p]
        out["final"].append(final)
        # the smallest non-zero element of every (category, pattern) column over the nodes' down partials: as it is, and relative to
        # the largest element of its pattern at that node
        d64 = np.stack([REF.to_float(down[p]) for p in t.int_down_pass])                                 # [node][K][P][S]
        least = np.where(d64 != 0, d64, np.inf).min(axis=3)
        out["unscaled"].append(least.min(axis=0) >= NORMAL_MARGIN)
        out["per_pattern"].append((least / d64.max(axis=(1, 3))[:, None, :]).min(axis=0) >= NORMAL_MARGIN)
        out["W"].append(W)
    worst = 0.0
    for p in t.int_down_pass:
        slack = out["tau"][p] + 2.0 ** -55 * out["L"]
        off = np.abs(out["invariant"][p] - out["L"])
        assert np.all(off <= slack), (kind, p, float(REF.to_float((off / out["L"]).max())))
        worst = max(worst, float(REF.to_float((slack / out["L"]).max())))
    assert 0 < worst < 1e-5, worst              # (what the identity is held to: a few 2^-24 per step below the top)
    out["invariant_slack"] = worst
    return out


def tree_bounds(t, S):
    B_op, beta = operation_bound(S, False), {n: 0.0 for n in range(t.ntaxa)}
    for p in t.int_down_pass:
        beta[p] = (1 + beta[t.left[p]]) * (1 + beta[t.right[p]]) * (1 + B_op) - 1
    gamma = {t.root_left: (1 + beta[t.root_left]) * (1 + top_bound(S)) - 1}
    for p in reversed(t.int_down_pass):
        if p != t.root_left:
            gamma[p] = (1 + gamma[t.anc[p]]) * (1 + beta[p]) * (1 + step_bound(S)) / (1 - beta[p]) - 1
    return beta, gamma


def rejected_move(t):
    """A tip whose branch a move changes and two interior nodes r, a = anc(r) OFF the tip's root-ward path, a below the top node: the
    shortest such path"""
    best = None
    for tip in range(t.ntaxa):
        if tip == t.root:
            continue
        path, n = [], t.anc[tip]
        while n != t.root:
            path.append(n)
            n = t.anc[n]
        for r in t.int_down_pass:
            a = t.anc[r]
            if r not in path and a not in path and a != t.root and (best is None or len(path) < len(best[1])):
                best = (tip, path, r, a)
    assert best is not None
    return best


def check_tree(lib, kind, ntaxa, npat, scaling):
    div = tree_division(kind, ntaxa, npat)
    t, S, K, P, parts = div.tree, div.nstates, div.ncat, div.npatterns, div.n_cijk_parts
    label = "%s %d taxa x %d patterns, %s" % (kind, ntaxa, npat, "always" if scaling == lk.MB_BEAGLE_SCALE_ALWAYS else "dynamic")
    top = t.root_left
    bd = lk.BeagleDivision(div, lib, scaling=scaling)
    try:
        inst = bd.inst
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name, name

        def verify(what):
            """the whole pass on the chain's current state, every node read and held to the reference on the matrices the engine holds"""
            site = inst.get_site_log_likelihoods()
            for j in range(parts):
                inst.update_final_partials(final_operations(bd, j))
            cums = [cumulative_index(bd, j) for j in range(parts)]
            first = read_tree(bd, cums)
            assert np.array_equal(inst.get_site_log_likelihoods(), site)
            mats = np.stack([np.stack([inst.get_transition_matrix(bd.tiProbsIndex[0][n] + j) for n in t.all_down_pass]) for j in range(parts)])
            ref = tree_reference(kind, ntaxa, npat, mats.tobytes())
            # The columns whose down pass stays in float32's normal range, in the scale the engine stores it in: unscaled under the
            # dynamic scheme while no likelihood underflows -- the slow categories of a variable site leave the range there, rightly:
            # they carry nothing --, with one exponent per pattern on the general layout, per (pattern, category) on the arena layouts.
            # The others are held to nothing but being finite: B_op is not claimed there.  A site is held to the invariant where all
            # its columns are.
            if cums[0] == NONE:
                columns = ref["unscaled"]
            elif "tree-walk" in name:
                columns = [np.ones((K, P), dtype=bool)] * parts
            else:
                assert scaling == lk.MB_BEAGLE_SCALE_ALWAYS
                columns = ref["per_pattern"]
            sites = np.all([c.all(axis=0) for c in columns], axis=0)
            ncol = sum(int(c.sum()) for c in columns)
            assert ncol >= 0.5 * parts * K * P and sites.sum() >= 10, (ncol, int(sites.sum()))
            gamma = tree_bounds(t, S)[1]
            tally, L = Tally(), ref["L"]
            B_tree = (1 + operation_bound(S, False)) ** (len(t.int_down_pass) * parts) * (1 + edge_bound(S, K * parts, False)) - 1
            ln_ref = REF.log(L)
            assert np.all(np.abs(REF.to_float(REF.widen(site) - ln_ref)) <= site_bound(B_tree, ln_ref)), label
            worst_site = 0.0
            for p in reversed(t.int_down_pass):
                engine = 0
                for j in range(parts):
                    got, ln = first[(p, j)]
                    emax = fp.integer_exponent(ln)
                    hold(got, emax, ref["final"][j][p], gamma[p], "%s: node %d part %d" % (label, p, j), tally, columns[j])
                    engine = engine + REF.einsum("k,a,kca->c", ref["W"][j], ref["F"], REF.scaled(got, np.broadcast_to(emax[None, :, None], got.shape)))
                allowed = 1.01 * (gamma[p] + REF.to_float(ref["tau"][p] / L)) + site_bound(B_tree, ln_ref)
                ratio = float((np.abs(REF.to_float(REF.log(engine) - REF.widen(site))) / allowed)[sites].max())
                assert ratio <= 1.0, (label, p, ratio)
                worst_site = max(worst_site, ratio)
            print("%s%s TREE %d of %d columns, %d of %d sites; elements: %s (bounds %.1e ... %.1e); site invariant error / bound %.3f (the reference's own: within %.1e); %s; %s" %
                  (label, what, ncol, parts * K * P, int(sites.sum()), P, tally, gamma[top], max(gamma.values()), worst_site, ref["invariant_slack"],
                   "cumulative buffer" if cums[0] != NONE else "unscaled", name.split(": ", 1)[-1]))
            return first, cums

        lnl = bd.LogLike(0)
        bd.AcceptMove(0)
        first, cums = verify("")
        # -- a move is proposed and rejected: the evaluation overwrote the scratch buffers of the tip's root-ward path, the flips are
        #    undone, and a second pass from the same top node, into the same buffers, re-makes that path only
        tip, path, r, a = rejected_move(t)
        old = t.length[tip]
        try:
            t.length[tip] = 2.0 * old
            bd.TouchBranch(0, tip)
            assert bd.LogLike(0) != lnl
        finally:
            t.length[tip] = old
        bd.ResetFlips(0)
        sc = bd.condLikeScratchIndex
        for j in range(parts):
            # before the new pass: what the evaluation overwrote is refused as an ancestor, what it left is still served
            if len(path) > 1:
                with pytest.raises(bg.BeagleError, match="does not hold final partials"):
                    inst.update_final_partials(np.array([[sc[path[0]] + j, sc[path[1]] + j, bd.condLikeIndex[0][path[0]] + j,
                                                          bd.tiProbsIndex[0][path[0]] + j, -1]], dtype=np.int32))
            inst.update_final_partials(final_operations(bd, j, nodes={r}))
            inst.update_final_partials(final_operations(bd, j, nodes=set(path)))
            # after it: a node the new pass did not re-make no longer holds final partials
            with pytest.raises(bg.BeagleError, match="does not hold final partials"):
                inst.update_final_partials(final_operations(bd, j, nodes={r}))
        again = read_tree(bd, cums)
        assert same_read_outs(first, again, [(p, j) for p in path for j in range(parts)]), label
        for j in range(parts):
            inst.update_final_partials(final_operations(bd, j))
        assert same_read_outs(first, read_tree(bd, cums)), label
        # -- the same move accepted: new matrices, new down partials along the path, other buffers; the whole pass again
        try:
            t.length[tip] = 2.0 * old
            bd.TouchBranch(0, tip)
            assert bd.LogLike(0) != lnl
            bd.AcceptMove(0)
            assert not same_read_outs(first, verify(" after an accepted move")[0])
        finally:
            t.length[tip] = old
    finally:
        bd.finalize()


@pytest.mark.parametrize("scaling", SCHEMES)
@pytest.mark.parametrize("kind,ntaxa,npat", TREE_CASES)
def test_tree_on_emulation(emu, kind, ntaxa, npat, scaling):
    check_tree(emu, kind, ntaxa, npat, scaling)


@pytest.mark.gpu
@pytest.mark.parametrize("scaling", SCHEMES)
@pytest.mark.parametrize("kind,ntaxa,npat", TREE_CASES)
def test_tree(gpu, kind, ntaxa, npat, scaling):
    check_tree(gpu, kind, ntaxa, npat, scaling)


def check_sharded_tree(lib, monkeypatch):
    """MBAMD_SHARD=3 at 130 patterns (children of 64, 64 and 2): every node's read-out, gathered from the children's pattern ranges,
    is the unsharded one bit for bit"""
    div = tree_division(*TREE_CASES[0])

    def run():
        bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS)
        try:
            bd.LogLike(0)
            bd.AcceptMove(0)
            bd.inst.update_final_partials(final_operations(bd, 0))
            return bd.inst.child_count(), read_tree(bd, [cumulative_index(bd, 0)])
        finally:
            bd.finalize()
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    n1, plain = run()
    monkeypatch.setenv("MBAMD_SHARD", "3")
    try:
        n3, sharded = run()
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    assert n1 == 1 and n3 == 3
    assert len(plain) == div.tree.n_int_nodes and same_read_outs(plain, sharded)


def test_sharded_tree_on_emulation(emu, monkeypatch):
    check_sharded_tree(emu, monkeypatch)


@pytest.mark.gpu
def test_sharded_tree(gpu, monkeypatch):
    check_sharded_tree(gpu, monkeypatch)


# ---- C. the read-out, exactly ----------------------------------------------------------------------------------------------------------
# buffers: 0 compact root tip; 2 = A, 3 = B, 4 = C, 5 = D operands; 6, 7, 8 the chained results; 9, 10 final partials.  Matrices 0, 1.
# Scale buffers 0, 1, 2, cumulative 3.
DEAD_PATTERN, DEAD_CATEGORY_PATTERN, SUBNORMAL_PATTERNS = 3, 5, (7, 9)


def check_read_out(lib, S, K, P, seed=11):
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    label = "%2d states x %d x %3d" % (S, K, P)
    inst = bg.BeagleInstance(lib, 2, 12, 2, S, P, 1, 4, K, 6)
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name, name
        per_category = "tree-walk" in name                  # the arena layouts: an exponent per (pattern, category); else per pattern
        ti = []
        for n in (0, 1):
            m = rng.random((K, S, S)) + 0.05
            ti.append(f32(m / m.sum(axis=2, keepdims=True)))
            inst.set_transition_matrix(n, ti[n])
            assert np.array_equal(inst.get_transition_matrix(n), ti[n]), "matrix round trip"
        st = rng.permutation(np.arange(P) % (S + 1)).astype(np.int32)
        inst.set_tip_states(0, st)
        # A, C, D: every (category, pattern) column at its own power of two over 100 binades; four patterns by design --
        #   the dead category's operands at the top of the range, the live ones 40 binades down in each of the three operations;
        #   category 0 at the top and the others 45 (48) binades down in each: shifts of about -135 (-144)
        ex = rng.integers(-100, 1, size=(3, K, P))
        ex[:, 0, DEAD_CATEGORY_PATTERN], ex[:, 1:, DEAD_CATEGORY_PATTERN] = 0, -40
        for c, depth in zip(SUBNORMAL_PATTERNS, (-45, -48)):
            ex[:, 0, c], ex[:, 1:, c] = 0, depth
        a, c, d = [(rng.random((K, P, S)) * 0.9 + 0.05) * np.exp2(ex[n].astype(np.float64))[:, :, None] for n in range(3)]
        d[0, DEAD_CATEGORY_PATTERN, :] = 0.0
        d[:, DEAD_PATTERN, :] = 0.0
        b = (rng.random((K, P, S)) * 0.9 + 0.05) * np.exp2(rng.integers(-4, 5, size=(K, P, S)).astype(np.float64))
        operands = [f32(x) for x in (a, b, c, d)]
        for n, x in enumerate(operands):
            inst.set_partials(2 + n, x)
            assert np.array_equal(inst.get_partials(2 + n), x), "partials round trip"
        inst.reset_scale_factors(3)
        inst.update_partials(np.array([[6, 0, NONE, 2, 0, 3, 1], [7, 1, NONE, 6, 0, 4, 1], [8, 2, NONE, 7, 0, 5, 1]], dtype=np.int32), 3)
        e = inst.get_scale_exponents(3).astype(np.int64)
        assert np.array_equal(e, sum(inst.get_scale_exponents(n).astype(np.int64) for n in range(3)))
        raw = as_f32(inst.get_partials(8))
        live = (raw != 0).any(axis=2)
        # what the inputs were chosen to produce
        assert not live[:, DEAD_PATTERN].any() and not live[0, DEAD_CATEGORY_PATTERN] and live[1:, DEAD_CATEGORY_PATTERN].all()
        tally = Tally()
        got, ln = inst.get_scaled_partials(8, 3)
        emax, shift = exact_read_out(got, ln, raw, e, label + ": the cumulative buffer", tally)
        assert ln[DEAD_PATTERN] == 0 and np.all(got[:, DEAD_PATTERN, :] == 0)
        if per_category:
            assert e[0, DEAD_CATEGORY_PATTERN] > e[1:, DEAD_CATEGORY_PATTERN].max() + 100 and emax[DEAD_CATEGORY_PATTERN] == e[1:, DEAD_CATEGORY_PATTERN].max()
            assert tally.subnormal + tally.flushed >= S and shift[live].min() <= -130, (tally.subnormal, tally.flushed, shift[live].min())
        else:
            assert np.all(e == e[0][None, :]) and np.all(shift[live] == 0)           # one exponent per pattern: nothing to shift
        # the same buffer as the top of a final pass (compact root tip) with one step below it: the pass's own exponents are ADDED
        inst.update_final_partials(np.array([[9, -1, 8, 0, 0], [10, 9, 7, 1, -1]], dtype=np.int32))
        raw9 = as_f32(inst.get_partials(9))
        got9, ln9 = inst.get_scaled_partials(9)
        top = fp.top(REF, REF.widen(raw), REF.contract(REF.widen(ti[0]), REF.widen(dense_tip(st, S, K))))
        own = column_exponents(raw9, got9, fp.integer_exponent(ln9), REF.exponents(top.max(axis=2), top_bound(S), -(1 << 20), 1 << 20))
        assert np.any(own != 0) and np.any(own.max(axis=0) != own.min(axis=0)) if K > 1 else np.any(own != 0)
        for buf in (9, 10):
            got, ln = inst.get_scaled_partials(buf, 3)
            exact_read_out(got, ln, as_f32(inst.get_partials(buf)), e + own, label + ": final partials %d with the cumulative buffer" % buf, tally)
        print("%s READ-OUT exact; smallest shift %d; %s; %s" % (label, shift[live].min(), tally, name.split(": ", 1)[-1]))
    finally:
        inst.finalize()
    return tally


READ_OUT_SHAPES = [(4, 3, 130), (20, 2, 70), (33, 2, 70), (61, 2, 40)]


@pytest.mark.parametrize("S,K,P", READ_OUT_SHAPES)
def test_read_out_on_emulation(emu, S, K, P):
    check_read_out(emu, S, K, P)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,P", READ_OUT_SHAPES)
def test_read_out(gpu, S, K, P):
    check_read_out(gpu, S, K, P)


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
def test_reference_types_agree():
    """the recurrences in exact Fractions and in longdouble on a small shape, zero sums included; the read-out model on values whose
    rounding is known"""
    rng = np.random.default_rng(9)
    S, K, P = 5, 2, 6
    m = matrices_of_kind(rng, S, K, "sparse")[0]
    anc, d = f32(rng.random((K, P, S))), f32(spread_partials(rng, S, K, P))
    d[:, 1, :] = 0.0
    d[:, 2, 1:] = 0.0
    out = []
    for r in (Reference(exact=True), REF):
        w = fp.step(r, r.widen(anc), r.widen(d), r.widen(m))
        out.append(r.to_float(w))
    assert np.all(out[0][:, 1, :] == 0) and np.any(out[0][:, 2, 0] != 0) and np.all(out[0][:, 2, 1:] == 0)
    assert np.all(np.abs(out[0] - out[1]) <= 2.0 ** -50 * out[0])
    raw = np.array([[[1.0, 0.75]], [[0.0, 0.0]], [[1.0 + 2.0 ** -23, 0.5]]], dtype=np.float32)          # [3][1][2]
    o, rounded, ln, emax, shift = fp.read_out(raw, np.array([[0], [200], [-149]]))
    assert emax[0] == 0 and ln[0] == 0 and list(shift[:, 0]) == [0, 200, -149]                          # (the dead category's 200 is ignored)
    assert o[2, 0, 0] == (1.0 + 2.0 ** -23) * 2.0 ** -149 and rounded[2, 0, 0] == 2.0 ** -149 and rounded[2, 0, 1] == 0.0      # ties to even
    assert np.array_equal(fp.integer_exponent(np.array([-7 * 0.69314718055994530942], dtype=np.float32)), [-7])
