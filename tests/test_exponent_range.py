"""The single-precision engine's operations over the WHOLE float32 exponent range: operand columns at 2^-104 ... 2^-146, results down
into the subnormal zone -- where unscaled lists of a dynamically rescaling client live (MrBayes submits unscaled lists until a
likelihood underflows).  tests/test_operation_bounds.py, whose helpers and reference (tests/operation_reference.py) this module uses,
holds the same kernels to the same relative bounds for columns at 2^-100 and above.

  * CPU (`not gpu`): the host-emulation build of the same sources;
  * GPU (`gpu`): the product library on a MI355X -- which also tells whether anything on the device flushes subnormals.

The bound.  u = 2^-24.  A dot product of S fused steps carries one rounding per step; a rounding is at most u |value| where the value
is a normal float and at most 2^-150 (half the spacing of the subnormals) where it is not; sums of subnormals are exact.  With f1, f2
the reference's two factors of an element, F1 = f1 (1 + d1) + e1 and F2 = f2 (1 + d2) + e2 with |d| within the relative bound and
|e| <= S 2^-150, and the product rounds once more:
  one operation, per element     |got - want| <= B_op want + (S (f1 + f2) + 1) 2^-150,   B_op = (2 S + 4) u
(the relative part is test_operation_bounds's; the products e d, e1 e2 are far inside its slack).  The range-safe form of the
bf16-piece contraction (40 and 60-63 states: wg_contract_bf16<RS>) works on the values times 2^24: whatever the matrix core drops
or flushes there is below 2^-126 in the scaled domain, 2^-150 in the result's -- the same term.
  edge integration, per site     the child's matrix-vector product is a float fma chain (S roundings), its product with the parent a
                                 float multiplication, everything after is double arithmetic on widened floats with weights and
                                 frequencies that sum to one: (S max_i parent_i + 1) 2^-150 on the site's likelihood L_c, beside
                                 site_bound(B_edge) on its logarithm.  Checked in the likelihood's domain, |L' - L_c| <= (e^b - 1) L_c
                                 + allowance, because a site whose allowance reaches its likelihood (a child column at 2^-146 under
                                 61 states: every product below 2^-150) legitimately comes out as 0 -- and then, and only then, a
                                 call without a dead pattern returns BEAGLE_ERROR_FLOATING_POINT too
  root integration, per site     floats widen to double exactly: site_bound(B_root) alone
  a stored exponent              a rescale stores frexp's exponent of the column maximum, clamped to [-126, 126]: decided wherever
                                 the maximum's own error interval (the bound above, at the column's largest allowance) lies inside
                                 one binade.  Columns whose maximum is within B_op of a power of two are `near`
                                 (Reference.exponents: at most 1 % of the columns, by the choice of seeds); columns whose ABSOLUTE
                                 allowance reaches a power of two -- factors far below 2^-126 times large ones -- are counted apart
                                 and printed: no arithmetic decides their exponent.
  a chain of operations          every operation against the bound above on its operands AS STORED (read back); the root's per-site
                                 log-likelihood against site_bound((1 + B_op)^m (1 + B_root) - 1) plus the absolute allowances of
                                 the operations carried up the tree through the reference's own factors (first order and the
                                 product of two), over L_c.

Operands: buffer A's (category, pattern) columns sit at 2^-m, m in {104, 112, 118, 122, 126, 130, 138, 146}, elements up to six
binades below their column; m and the spread are drawn per column, the largest element of a column keeps the column's binade.
Buffer B: (i) elements 2^10 ... 2^30 -- results stay normal, the handling of the small operand is isolated; (ii) elements
0.05 ... 0.95 -- results land in the subnormal zone.  One pattern of B is zero throughout.  Matrices: random_matrices as they stand
(entries of at least 2^-10; smaller ones are out of scope, DESIGN.md "Operand range").

Where the module departs from a plain reading of its brief, and why.  (a) A pure caterpillar's whole-tree list is itself a
root-ward path and never reaches the walk kernel: the ladder of twelve tips stands on three cherries.  (b) One factor on all matrices
gives eleven operations 11.4 binades each: the columns cannot pass 2^-100 in the first half of the ladder AND end at 2^-126 or above;
ending there puts the last operand near 2^-113, where the plain bf16 split still passes.  The ladder therefore runs to 2^-124 (every
root column normal) and to 2^-132 (last operand near 2^-120, root columns subnormal), the ranges asserted from the read-back.  (c)
Stored exponents: beside Reference.exponents' `near` columns, columns whose absolute allowance reaches a power of two are exempt from
equality, and held to the range of exponents their allowance admits; only columns of A at 2^-130 and below, and the products of a
buffer with itself, may be among them (asserted).  (d) "The same call without the dead pattern returns 0" holds wherever no site can
underflow altogether; at (61, 1, 40) with the tiny buffer as the child, five sites at 2^-146 do -- every product lies below 2^-150 --
and that call returns BEAGLE_ERROR_FLOATING_POINT as the header says it must for an infinite sum: the test asserts the error exactly
where a site came out as 0, and that only sites whose allowance reaches their likelihood did.

Each check prints the worst error / bound it met (pytest -s shows them).
"""
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd.division import synthetic_division
from tests.hostemu import build_emu
from tests.operation_reference import Reference, dense_tip
from tests.test_operation_bounds import (edge_bound, expected_layout, operation_bound, preference, random_matrices, root_bound,
                                         site_bound, stored, vector)

NONE = bg.BEAGLE_OP_NONE
REF = Reference()
TINY = 2.0 ** -150                                   # the largest error of one rounding to a subnormal float
COLUMN_EXPONENTS = (104, 112, 118, 122, 126, 130, 138, 146)
DEAD_PATTERN = 3
LO, HI = -126, 126                                   # scale_exponent's clamp (mbamd_kernels.h)


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def tag(S, K, P):
    return "%2d states x %2d x %3d fp32" % (S, K, P)


class switched:
    """environment switches an instance reads when it is created"""
    def __init__(self, monkeypatch, names):
        self.mp, self.names = monkeypatch, names

    def __enter__(self):
        for n in self.names:
            self.mp.setenv(n, "1")

    def __exit__(self, *exc):
        for n in self.names:
            self.mp.delenv(n, raising=False)


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def tiny_columns(rng, S, K, P, exponents=COLUMN_EXPONENTS):
    """buffer A: column (k, c) at 2^-m, its elements up to `spread` binades below, m and spread drawn per column (every m occurs);
    returns the values as stored and m [K][P]"""
    m = rng.permutation(np.resize(np.array(exponents), K * P)).reshape(K, P, 1)
    spread = rng.integers(0, 7, size=(K, P, 1))
    shift = rng.integers(0, 7, size=(K, P, S)) % (spread + 1)
    np.put_along_axis(shift, rng.integers(0, S, size=(K, P, 1)), 0, axis=2)
    a = (rng.random((K, P, S)) * 0.5 + 0.5) * np.exp2(-(m + shift).astype(np.float64))
    return stored(a, False), m[:, :, 0]


def ordinary(rng, S, K, P, large, dead=True):
    """buffer B: (large) every element times its own power of two, 2^10 ... 2^30; (not large) elements 0.05 ... 0.95"""
    b = rng.random((K, P, S)) * 0.9 + 0.05
    if large:
        b = b * np.exp2(rng.integers(10, 31, size=(K, P, S)).astype(np.float64))
    if dead:
        b[:, DEAD_PATTERN, :] = 0.0
    return stored(b, False)


def allowance(S, want, f1, f2):
    """the bound of one operation, per element (reference type)"""
    return operation_bound(S, False) * want + (S * (f1 + f2) + 1) * REF.widen(TINY)


def ratio(got, want, tol):
    return float(REF.to_float(np.abs(REF.widen(got) - want) / tol).max())


def clamped_exponent(x):
    """what a rescale stores for the column maximum x (float64 array): 0 for a dead column"""
    m, e = np.frexp(x)
    return np.where(m > 0, np.clip(e, LO, HI), 0).astype(np.int64)


def exponent_range(col_max, col_tol):
    """the smallest and the largest exponent a rescale may store for a column whose maximum lies within col_tol of col_max, and
    whether the column may come out dead (all zero: exponent 0)"""
    low = REF.to_float(col_max - col_tol)
    may_die = low <= 0
    a = np.where(may_die, LO, clamped_exponent(np.maximum(low, 2.0 ** -149)))
    b = clamped_exponent(REF.to_float(col_max + col_tol))
    return a, b, may_die


def undecided(col_max, col_tol):
    """columns whose maximum may, within its allowance, have another stored exponent"""
    lo, hi, may_die = exponent_range(col_max, col_tol)
    return (lo != hi) | (may_die & (REF.to_float(col_max) > 0))


# ---- 1. one operation across the range ---------------------------------------------------------------------------------------------
# buffers: 0 compact tip; 2 a tip given as partials; 3 = A; 4 = B; 5, 6, 7 results; 8 = A', columns at 2^-50 ... 2^-60.  Matrices 0, 1.
# Scale buffer 0, cumulative 1.  ("A twice" is what the brief asks for, and it is vacuous for the arithmetic: both factors are at most
# 2^-104, every product lies below the subnormals, and the absolute term admits the zeros that come out -- it checks finiteness, zeros
# and the exponents of dead columns.  "A' twice" is the same pair where it says something: products at 2^-100 ... 2^-132, small
# results of operands that are not small.)
HALF_EXPONENTS = (50, 52, 54, 56, 58, 60)
def check_range_operation(lib, S, K, P, large, layout, seed=1):
    rng = np.random.default_rng(seed + 1000 * S + 10 * K + (1 if large else 0))
    B_op = operation_bound(S, False)
    inst = bg.BeagleInstance(lib, 3, 10, 2, S, P, 1, 4, K, 4, preference_flags=preference(False))
    try:
        name = inst.details.implName.decode()
        assert layout in name, name
        per_category = "tree-walk" in name
        pieces = per_category and S >= 40            # the bf16-piece contraction: client-set partials take its range-safe form
        ti = [random_matrices(rng, S, K, False), random_matrices(rng, S, K, False)]
        for n in (0, 1):
            inst.set_transition_matrix(n, ti[n])
            assert np.array_equal(inst.get_transition_matrix(n), ti[n]), "matrix round trip"
        st = rng.integers(0, S + 1, size=P).astype(np.int32)
        st[0], st[1] = S, S - 1
        inst.set_tip_states(0, st)
        tp = stored(rng.random((P, S)) * 0.9 + 0.05, False)
        pa, m_of = tiny_columns(rng, S, K, P)
        pb = ordinary(rng, S, K, P, large)
        ph, _ = tiny_columns(rng, S, K, P, HALF_EXPONENTS)
        assert set(np.unique(m_of).tolist()) == set(COLUMN_EXPONENTS)
        inst.set_tip_partials(2, tp)
        inst.set_partials(3, pa)
        inst.set_partials(4, pb)
        inst.set_partials(8, ph)
        tp_dense = np.ascontiguousarray(np.broadcast_to(tp, (K, P, S)))
        for idx, a in ((2, tp_dense), (3, pa), (4, pb), (8, ph)):
            assert np.array_equal(inst.get_partials(idx), a), "partials round trip (buffer %d)" % idx
        wide = {0: REF.widen(dense_tip(st, S, K)), 2: REF.widen(tp_dense), 3: REF.widen(pa), 4: REF.widen(pb), 8: REF.widen(ph)}
        wm = [REF.widen(m) for m in ti]
        worst, skipped, open_columns, columns = 0.0, 0, 0, 0
        before = inst.get_range_safe_counts()
        for kind, c1, c2 in (("partials A,partials B", 3, 4), ("states,partials A", 0, 3), ("A twice", 3, 3), ("tip partials,partials A", 2, 3),
                             ("A' twice", 8, 8)):
            f1, f2 = REF.factors(wm[0], wide[c1], wm[1], wide[c2])
            want = f1 * f2
            tol = allowance(S, want, f1, f2)
            zero = REF.to_float(want) == 0
            # -- no scaling
            inst.update_partials(np.array([[5, NONE, NONE, c1, 0, c2, 1]], dtype=np.int32), NONE)
            got = inst.get_partials(5)
            assert np.isfinite(got).all(), kind
            assert np.all(got[zero] == 0), kind
            r0 = ratio(got, want, tol)
            # -- SCALE_WRITE into scale buffer 0 with cumulative buffer 1
            inst.reset_scale_factors(1)
            inst.update_partials(np.array([[6, 0, NONE, c1, 0, c2, 1]], dtype=np.int32), 1)
            got2 = inst.get_partials(6)
            e = inst.get_scale_exponents(0)
            assert np.isfinite(got2).all(), kind
            assert np.all(got2[zero] == 0), kind
            r1 = ratio(REF.scaled(got2, e[:, :, None]), want, tol)
            print("%s %-24s B %s: worst error / bound: unscaled %.3f, scaled %.3f" % (tag(S, K, P), kind, "2^10..2^30" if large else "0.05..0.95", r0, r1))
            assert r0 <= 1.0 and r1 <= 1.0, (kind, r0, r1)
            if per_category:
                col_max, col_tol = want.max(axis=2), tol.max(axis=2)
            else:
                col_max, col_tol = np.broadcast_to(want.max(axis=(0, 2)), (K, P)), np.broadcast_to(tol.max(axis=(0, 2)), (K, P))
            e_ref, near = REF.exponents(col_max, B_op, LO, HI)
            unknown = undecided(col_max, col_tol) & ~near
            # the ceiling on that exemption: an absolute allowance reaches a power of two only where a factor is subnormal -- a
            # column of A at 2^-130 and below (in the layouts with one exponent per pattern: in every category) -- or where the
            # product itself lies below the normal floats: the two pairs of a buffer with itself
            m_col = m_of if per_category else np.broadcast_to(m_of.min(axis=0), (K, P))
            assert not (unknown & (m_col < 130)).any() or c1 == c2, (kind, np.argwhere(unknown & (m_col < 130))[:4].tolist())
            skipped += int(near.sum())
            open_columns += int(unknown.sum())
            columns += near.size
            ok = near | unknown
            assert np.array_equal(e[~ok], e_ref[~ok]), (kind, np.argwhere((e != e_ref) & ~ok)[:4].tolist())
            e_lo, e_hi, may_die = exponent_range(col_max, col_tol)         # (an undecided column: between its two ends' exponents)
            assert np.all(near | ((e >= e_lo) & (e <= e_hi)) | (may_die & (e == 0))), kind
            assert np.all(e[REF.to_float(col_max) == 0] == 0), kind
            # -- SCALE_READ: the bits of the write pass
            inst.update_partials(np.array([[7, NONE, 0, c1, 0, c2, 1]], dtype=np.int32), NONE)
            assert np.array_equal(inst.get_partials(7), got2), kind
            worst = max(worst, r0, r1)
        after = inst.get_range_safe_counts()
        if pieces:                                   # every one of the fifteen lists read a buffer the client set
            assert after[0] - before[0] == 15 and after[1] == before[1], (before, after)
        else:
            assert after == before == (0, 0), (before, after)
        print("%s RANGE OPERATION worst error / bound %.3f; %d of %d columns near a power of two, %d more undecided by their absolute allowance; %s" %
              (tag(S, K, P), worst, skipped, columns, open_columns, name.split(": ", 1)[-1]))
        assert skipped <= 0.01 * columns, (skipped, columns)
    finally:
        inst.finalize()
    return worst


#               switches                  shape        layout
RANGE_CASES = [((), (4, 2, 70), None), ((), (8, 2, 40), None), ((), (15, 2, 40), None), ((), (20, 2, 40), None), ((), (33, 2, 40), None),
               ((), (40, 1, 40), None), ((), (61, 1, 33), None), ((), (63, 1, 33), None),
               (("MBAMD_FORCE_GENERIC",), (4, 2, 70), "general-state vector kernels"),
               (("MBAMD_NO_MFMA",), (33, 2, 40), "general-state vector kernels"),
               (("MBAMD_NO_WALKG",), (61, 1, 33), "general-state MFMA")]
RANGE_IDS = ["%s%dx%dx%d" % ("".join(s[6:] + "-" for s in c[0]), *c[1]) for c in RANGE_CASES]
REGIMES = [pytest.param(True, id="B-large"), pytest.param(False, id="B-unit")]


def run_range_operation(lib, monkeypatch, switches, shape, large, layout):
    S, K, P = shape
    with switched(monkeypatch, switches):
        check_range_operation(lib, S, K, P, large, layout or expected_layout(S, K, False))


@pytest.mark.parametrize("large", REGIMES)
@pytest.mark.parametrize("switches,shape,layout", RANGE_CASES, ids=RANGE_IDS)
def test_range_operation_on_emulation(emu, monkeypatch, switches, shape, layout, large):
    run_range_operation(emu, monkeypatch, switches, shape, large, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("large", REGIMES)
@pytest.mark.parametrize("switches,shape,layout", RANGE_CASES, ids=RANGE_IDS)
def test_range_operation(gpu, monkeypatch, switches, shape, layout, large):
    run_range_operation(gpu, monkeypatch, switches, shape, large, layout)


# ---- 2. unscaled chains, each step held on its own ---------------------------------------------------------------------------------
# Twelve compact tips.  A pure caterpillar's list IS a root-ward path (Instance::recognisePath) and would never reach the walk kernel,
# so the ladder stands on three cherries (three results waiting: not the path kernels' shape), and the list of a changed matrix at
# tip 6 is the pure path of its six upper rungs.
NTIPS = 12
LADDER = [(12, 0, 1), (13, 2, 3), (14, 4, 5), (15, 12, 13), (16, 15, 14)] + [(17 + i, 16 + i, 6 + i) for i in range(6)]
CHANGED_TIP = 6


def carried(S, ops, sources, wm):
    """the reference's partials of every node and the absolute allowance its elements have gathered on the way up"""
    have = dict(sources)
    slack = {n: 0 for n in sources}
    for d, a, b in ops:
        f1, f2 = REF.factors(wm[a], have[a], wm[b], have[b])
        e1 = REF.contract(wm[a], slack[a]) if a in slack and not np.isscalar(slack[a]) else 0
        e2 = REF.contract(wm[b], slack[b]) if b in slack and not np.isscalar(slack[b]) else 0
        have[d] = f1 * f2
        slack[d] = (S * (f1 + f2) + 1) * REF.widen(TINY) + f2 * e1 + f1 * e2 + e1 * e2
    return have, slack


def check_range_chain(lib, S, K, P, depth, seed=11):
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    label = tag(S, K, P) + " to 2^-%d" % depth
    ops, nint, nodes = LADDER, len(LADDER), NTIPS + len(LADDER)
    root = ops[-1][0]
    B_op = operation_bound(S, False)
    base = [random_matrices(rng, S, K, False) for _ in range(nodes)]
    new_base = random_matrices(rng, S, K, False)
    states = [rng.integers(0, S, size=P).astype(np.int32) for _ in range(NTIPS)]
    w, f = vector(rng, K, False), vector(rng, S, False)
    W, F = REF.widen(w), REF.widen(f)
    sources = {n: REF.widen(dense_tip(states[n], S, K)) for n in range(NTIPS)}
    # ONE factor on all matrices: every node's value carries it once per matrix below it, the root 2 m times.  Chosen so that the
    # root's smallest column maximum comes out at 2^-depth.  Eleven operations of equal weight between 2^0 and 2^-126 are 11.4
    # binades each: the columns cannot pass 2^-100 before the last rungs AND end normal, and the last operand then sits near 2^-113,
    # where the plain bf16 split still keeps most of its bits.  So two depths: 124 -- every root column a normal float --, and 132 --
    # the last operand near 2^-120, the root's columns subnormal, which the absolute term of the bound is there for.  Both ranges
    # are asserted from the read-back.
    unit = REF.to_float(REF.prune(ops, sources, [REF.widen(m) for m in base])[root].max(axis=2)).min()
    factor = float(2.0 ** ((-float(depth) - np.log2(unit)) / (2 * nint)))
    mats = [stored(m * factor, False) for m in base]
    new_matrix = stored(new_base * factor, False)
    rows = lambda which: np.array([[d, NONE, NONE, a, a, b, b] for d, a, b in ops if which is None or d in which], dtype=np.int32)
    path = [d for d, a, b in ops if d >= 17]
    B = (1.0 + B_op) ** nint * (1.0 + root_bound(S, K, False)) - 1.0
    inst = bg.BeagleInstance(lib, NTIPS, nint, NTIPS, S, P, 1, nodes, K, nint + 1, preference_flags=preference(False))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name and "tree-walk" in name, name
        for n in range(nodes - 1):
            inst.set_transition_matrix(n, mats[n])
        for n in range(NTIPS):
            inst.set_tip_states(n, states[n])
        inst.set_category_weights(0, w)
        inst.set_state_frequencies(0, f)
        inst.set_pattern_weights(np.ones(P))
        wm = [REF.widen(m) for m in mats]
        worst = 0.0

        def held(what, which):
            """the root's per-site values, then every operation of `which` on its operands as stored"""
            rc, lnl = inst.calculate_root_log_likelihoods([root], [0], [0], [NONE])
            assert rc == 0, (what, rc)
            site = inst.get_site_log_likelihoods()
            counts = inst.get_list_counts()
            have, slack = carried(S, ops, sources, wm)
            L = REF.root(W, F, have[root])
            lnL = REF.log(L)
            bound = site_bound(B, lnL) + REF.to_float(REF.root(W, F, slack[root]) / L)
            rs = float((np.abs(REF.to_float(REF.widen(site) - lnL)) / bound).max())
            got = {d: inst.get_partials(d) for d, a, b in ops}
            assert all(np.isfinite(g).all() for g in got.values())
            seen = dict(sources)
            seen.update({d: REF.widen(g) for d, g in got.items()})
            low, rmax = 0, 0.0
            for d, a, b in ops:
                if d not in which:
                    continue
                f1, f2 = REF.factors(wm[a], seen[a], wm[b], seen[b])
                r = ratio(got[d], f1 * f2, allowance(S, f1 * f2, f1, f2))
                rmax = max(rmax, r)
                below = [float(np.mean(got[c].max(axis=2) < 2.0 ** -100)) for c in (a, b) if c >= NTIPS]
                low += int(any(x >= 0.1 for x in below))
                last = below
                assert r <= 1.0, (what, d, r)
            top = got[root].max(axis=2)
            print("%s %-22s worst step error / bound %.3f, worst site error / bound %.3f; root columns 2^%.1f ... 2^%.1f; %d operations read a tenth of their operand's columns below 2^-100" %
                  (label, what, rmax, rs, np.log2(top.min()), np.log2(top.max()), low))
            assert rs <= 1.0, (what, rs)
            # (from the read-back: the root's columns are normal floats, the last operation's operand lies below 2^-100 in at least
            #  half its columns and at least two operations read an operand with a tenth of its columns there; at the greater depth
            #  the root's columns are subnormal in at least half the columns and dead in none)
            assert low >= 2 and last[0] >= 0.5, (what, low, last)
            if depth < 126:
                assert top.min() >= 2.0 ** -126, (what, float(top.min()))
            else:
                assert 0 < top.min() < 2.0 ** -126 and np.mean(top < 2.0 ** -126) >= 0.5, (what, float(top.min()), float(top.max()))
            return max(rmax, rs), counts

        before = inst.get_list_counts()
        safe0 = inst.get_range_safe_counts()
        inst.update_partials(rows(None), NONE)
        r, middle = held("ladder of %d" % nint, set(d for d, a, b in ops))
        worst = max(worst, r)
        inst.set_transition_matrix(CHANGED_TIP, new_matrix)
        wm[CHANGED_TIP] = REF.widen(new_matrix)
        inst.update_partials(rows(set(path)), NONE)
        r, after = held("path of %d again" % len(path), set(path))
        worst = max(worst, r)
        # a third list, the shape of a topology move: the matrices of tips 0 and 2 change -- arm 12, arm 13, their join 15, the stem
        # up to the root (cherry 14 stays): a FORKED path (k_path4 / k_pathg<..., FORK>), whose upper rungs read the small columns
        forked = [d for d, a, b in ops if d != 14]
        for n in (0, 2):
            fresh = stored(random_matrices(rng, S, K, False) * factor, False)
            inst.set_transition_matrix(n, fresh)
            wm[n] = REF.widen(fresh)
        inst.update_partials(rows(set(forked)), NONE)
        r, last_counts = held("forked path of %d" % len(forked), set(forked))
        worst = max(worst, r)
        safe1 = inst.get_range_safe_counts()
        print("%s RANGE CHAIN worst error / bound %.3f; list counts %s -> %s -> %s -> %s; %s" % (label, worst, before, middle, after, last_counts, name.split(": ", 1)[-1]))
        assert middle[4] - before[4] == 1 and middle[5] - before[5] == nint, (before, middle)       # the ladder: one walk
        if S == 4 or S == 20 or 60 <= S <= 63:                                                      # the path: k_path4 / k_pathg
            assert after[1] - middle[1] == 1 and after[4] == middle[4], (middle, after)
        else:
            assert after[1] == middle[1] and after[4] - middle[4] == 1, (middle, after)
        if S == 4 or S == 20 or 60 <= S <= 63:                                                      # the forked path
            assert last_counts[1] - after[1] == 1 and last_counts[2] - after[2] == 1 and last_counts[4] == after[4], (after, last_counts)
        else:
            assert last_counts[1] == after[1] and last_counts[4] - after[4] == 1, (after, last_counts)
        # (unscaled results are of unknown magnitude to the host: all three lists of the bf16-piece state counts ran range-safe)
        assert (safe1[0] - safe0[0], safe1[1] - safe0[1]) == ((3, 0) if S >= 40 else (0, 0)), (safe0, safe1)
    finally:
        inst.finalize()
    return worst


CHAIN_SHAPES = [(4, 2, 70), (20, 2, 40), (40, 1, 40), (61, 1, 33)]
CHAIN_DEPTHS = [124, 132]


@pytest.mark.parametrize("depth", CHAIN_DEPTHS)
@pytest.mark.parametrize("S,K,P", CHAIN_SHAPES)
def test_range_chain_on_emulation(emu, S, K, P, depth):
    check_range_chain(emu, S, K, P, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", CHAIN_DEPTHS)
@pytest.mark.parametrize("S,K,P", CHAIN_SHAPES)
def test_range_chain(gpu, S, K, P, depth):
    check_range_chain(gpu, S, K, P, depth)


# ---- 3. integration across the range -----------------------------------------------------------------------------------------------
# buffers: 2 = the tiny buffer; 3 = an ordinary one (0.05 ... 0.95).  Matrix 0.
def check_range_integration(lib, S, K, P, seed=3):
    rng = np.random.default_rng(seed + 1000 * S + 10 * K)
    label = tag(S, K, P)
    inst = bg.BeagleInstance(lib, 2, 10, 2, S, P, 1, 4, K, 6, preference_flags=preference(False))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name, name
        m = random_matrices(rng, S, K, False)
        inst.set_transition_matrix(0, m)
        pt, m_of = tiny_columns(rng, S, K, P)
        assert set(np.unique(m_of).tolist()) == set(COLUMN_EXPONENTS)
        po = ordinary(rng, S, K, P, large=False, dead=False)
        dead = pt.copy()
        dead[:, DEAD_PATTERN, :] = 0.0
        inst.set_partials(3, po)
        w, f = vector(rng, K, False), vector(rng, S, False)
        inst.set_category_weights(0, w)
        inst.set_state_frequencies(0, f)
        inst.set_pattern_weights(np.ones(P))
        W, F, M, O = REF.widen(w), REF.widen(f), REF.widen(m), REF.widen(po)
        Br, Be = root_bound(S, K, False), edge_bound(S, K, False)
        tiny = REF.widen(TINY)
        forms = (("root", lambda: inst.calculate_root_log_likelihoods([2], [0], [0], [NONE]),
                  lambda T: (REF.root(W, F, T), Br, 0 * tiny)),
                 ("edge, tiny child", lambda: inst.calculate_edge_log_likelihoods([3], [2], [0], [0], [0], [NONE]),
                  lambda T: (REF.edge(W, F, O, M, T), Be, (S * O.max(axis=(0, 2)) + 1) * tiny)),
                 ("edge, tiny parent", lambda: inst.calculate_edge_log_likelihoods([2], [3], [0], [0], [0], [NONE]),
                  lambda T: (REF.edge(W, F, T, M, O), Be, (S * T.max(axis=(0, 2)) + 1) * tiny)))
        alive = np.arange(P) != DEAD_PATTERN
        worst = 0.0
        for what, call, reference in forms:
            for values, which, code in ((dead, alive, bg.BEAGLE_ERROR_FLOATING_POINT), (pt, np.ones(P, dtype=bool), 0)):
                inst.set_partials(2, values)
                assert np.array_equal(inst.get_partials(2), values), "partials round trip"
                rc, lnl = call()
                site = inst.get_site_log_likelihoods()
                L, B, slack = reference(REF.widen(values))
                L, slack = L[which], (slack[which] if np.ndim(slack) else slack)
                # in the likelihood's domain, where an absolute allowance belongs: |ln L' - ln L| <= b is |L' - L| <= (e^b - 1) L to
                # first order in the direction that matters; a site whose allowance reaches its likelihood may come out as 0
                relative = np.expm1(site_bound(B, REF.log(L)))
                tol = relative * L + slack
                got = np.exp(REF.widen(site[which]))                       # (exp(-inf) = 0)
                assert not np.isnan(site[which]).any(), what
                r = float(REF.to_float(np.abs(got - L) / tol).max())
                may_vanish = REF.to_float(L * (1 - relative) - slack) <= 0
                print("%s %-18s %s: worst site error / bound %.3f; %d sites may underflow to zero, %d did" %
                      (label, what, "one pattern all zero" if code else "every pattern alive ", r, int(may_vanish.sum()), int(np.isinf(site[which]).sum())))
                assert r <= 1.0, (what, code, r)
                # beagle.h: BEAGLE_ERROR_FLOATING_POINT when the sum is NaN or infinite -- with a dead pattern always; without one
                # only where a site's likelihood underflowed altogether, which the bound above allows nowhere else
                vanished = bool(np.isinf(site).any())
                assert rc == (bg.BEAGLE_ERROR_FLOATING_POINT if vanished else 0), (what, rc, vanished)
                assert vanished if code else (not vanished or may_vanish.any()), (what, rc)
                worst = max(worst, r)
        print("%s RANGE INTEGRATION worst error / bound %.3f; %s" % (label, worst, name.split(": ", 1)[-1]))
    finally:
        inst.finalize()
    return worst


INTEGRATION_SHAPES = [(4, 4, 70), (20, 4, 70), (33, 2, 40), (61, 1, 40)]


@pytest.mark.parametrize("S,K,P", INTEGRATION_SHAPES)
def test_range_integration_on_emulation(emu, S, K, P):
    check_range_integration(emu, S, K, P)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,P", INTEGRATION_SHAPES)
def test_range_integration(gpu, S, K, P):
    check_range_integration(gpu, S, K, P)


# ---- 4. dynamic against always rescaling, through BeagleDivision -------------------------------------------------------------------
# MrBayes' dynamic rescaling submits the whole tree as ONE unscaled list and rescales only after a floating-point error.  A division
# whose first unscaled pass just succeeds has the partials of its upper nodes where the plain bf16 split loses bits.  Both
# evaluations are within their tree bound of the true value, so they are within the sum of the two of each other: m operations and
# the edge integration each; the unscaled evaluation also carries the absolute allowances of its operations up the tree (`carried`,
# on the matrices the engine read back), the rescaling one needs none -- its columns are normalised after every operation.
def check_range_division(lib, kind, ntaxa, P, brlen):
    div = synthetic_division(kind, ntaxa, P, seed=5, tree_seed=6, brlen=brlen)
    S, K, t = div.nstates, div.ncat, div.tree
    label = "%-3s %2d states, %d taxa x %d patterns, branch length %g" % (kind, S, ntaxa, P, brlen)
    m = len(t.int_down_pass)
    B = (1.0 + operation_bound(S, False)) ** m * (1.0 + edge_bound(S, K, False)) - 1.0
    out = {}
    for how, scaling in (("dynamic", lk.MB_BEAGLE_SCALE_DYNAMIC), ("always", lk.MB_BEAGLE_SCALE_ALWAYS)):
        bd = lk.BeagleDivision(div, lib, scaling=scaling)
        try:
            lnl = bd.LogLike(0)
            site = bd.inst.get_site_log_likelihoods()
            counts = bd.inst.get_range_safe_counts()
            if how == "dynamic":
                assert not bd.rescaleBeagleAll and bd.successCount[0] == 1          # the first, unscaled pass succeeded
                top = [bd.inst.get_partials(bd.condLikeIndex[0][t.root_left] + j) for j in range(bd.step)]
                cols = np.concatenate([g.max(axis=2).ravel() for g in top])
                window = float(np.mean((cols < 2.0 ** -100) & (cols >= 2.0 ** -125)))
                assert window >= 0.25, window
                # the allowance the unscaled operations gather, on the matrices as the engine holds them
                F = REF.widen(stored(div.pi, False))
                L, slack = 0, 0
                for j in range(bd.step):
                    wm = {n: REF.widen(bd.inst.get_transition_matrix(bd.tiProbsIndex[0][n] + j)) for n in range(t.n_nodes) if n != t.root}
                    sources = {n: REF.widen(dense_tip(div.tip_states[n], S, K)) for n in range(ntaxa)}
                    have, gathered = carried(S, [(p, t.left[p], t.right[p]) for p in t.int_down_pass], sources, wm)
                    W = REF.widen(stored(div.category_weights(j), False))
                    parent, edge = have[t.root_left], REF.contract(wm[t.root_left], sources[t.root])
                    L = L + REF.einsum("k,i,kci->c", W, F, parent * edge)
                    slack = slack + REF.einsum("k,i,kci->c", W, F, gathered[t.root_left] * edge) + W.sum() * (S * parent.max(axis=(0, 2)) + 1) * REF.widen(TINY)
                extra = REF.to_float(slack / L)
                ref_error = float((np.abs(REF.to_float(REF.widen(site) - REF.log(L))) / (site_bound(B, site) + extra)).max())
                assert counts == ((1, 0) if S >= 40 else (0, 0)), counts         # (the unscaled list of a codon model ran range-safe)
            else:
                assert counts == ((0, 1) if S >= 40 else (0, 0)), counts         # (every list of an always-rescaling client: the plain code)
            out[how] = (lnl, site)
        finally:
            bd.finalize()
    (lnl_d, site_d), (lnl_a, site_a) = out["dynamic"], out["always"]
    bound = site_bound(B, site_d) + site_bound(B, site_a) + extra
    r = float((np.abs(site_d - site_a) / bound).max())
    print("%s RANGE DIVISION dynamic against always: worst site difference / bound %.3f (dynamic against the reference: %.3f); lnL %.6f / %.6f; "
          "%.0f %% of the top node's columns in 2^-125 ... 2^-100, smallest 2^%.1f" % (label, r, ref_error, lnl_d, lnl_a, 100 * window, np.log2(cols[cols > 0].min())))
    assert r <= 1.0 and ref_error <= 1.0, (r, ref_error)
    return r


# (taxa and branch lengths: the first unscaled pass succeeds and at least a quarter of the top node's columns lie in 2^-125 ... 2^-100
#  -- asserted from the read-back.  With the plain bf16 split in the unscaled list the codon case is at 3.2 times its bound, and at
#  6.1 times the unscaled evaluation's own bound against the reference; with the range-safe one at 0.012 and 0.021.)
DIVISION_CASES = [("m3", 23, 40, 0.8), ("gtr", 60, 70, 0.5)]


@pytest.mark.parametrize("kind,ntaxa,P,brlen", DIVISION_CASES)
def test_range_division_on_emulation(emu, kind, ntaxa, P, brlen):
    check_range_division(emu, kind, ntaxa, P, brlen)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ntaxa,P,brlen", DIVISION_CASES)
def test_range_division(gpu, kind, ntaxa, P, brlen):
    check_range_division(gpu, kind, ntaxa, P, brlen)


# ---- 5. which instantiation a list runs: the host's choice ---------------------------------------------------------------------------
# buffers: 0, 1 compact tips; 2 ... 6 results; scale buffers 0, 1.  (plain: every partials operand last written by a SCALE_WRITE
# operation of this layout, or a compact tip; range-safe: anything else -- Instance::flushWalkG)
def check_choice(lib, S, K, P):
    rng = np.random.default_rng(17 + S)
    inst = bg.BeagleInstance(lib, 2, 8, 2, S, P, 1, 2, K, 3, preference_flags=preference(False))
    try:
        assert "tree-walk" in inst.details.implName.decode()
        for n in (0, 1):
            inst.set_transition_matrix(n, random_matrices(rng, S, K, False))
            inst.set_tip_states(n, rng.integers(0, S, size=P).astype(np.int32))
        seen = [inst.get_range_safe_counts()]

        def step(what, row, expect):
            inst.update_partials(np.array([row], dtype=np.int32), NONE)
            inst.get_partials(row[0])
            seen.append(inst.get_range_safe_counts())
            got = (seen[-1][0] - seen[-2][0], seen[-1][1] - seen[-2][1])
            assert got == (expect if S >= 40 else (0, 0)), (what, got, expect)
        step("two compact tips, rescaled", [2, 0, NONE, 0, 0, 1, 1], (0, 1))
        step("a rescaled buffer and a tip, rescaled", [3, 1, NONE, 2, 0, 1, 1], (0, 1))
        step("rescaled buffers, result left unscaled", [4, NONE, NONE, 2, 0, 3, 1], (0, 1))
        step("an unscaled result", [5, NONE, NONE, 4, 0, 1, 1], (1, 0))
        step("a result written with another node's exponents", [6, NONE, 0, 2, 0, 1, 1], (0, 1))
        step("... read", [5, NONE, NONE, 6, 0, 1, 1], (1, 0))
        inst.set_partials(2, ordinary(rng, S, K, P, large=False, dead=False))
        step("a buffer the client has set since", [5, NONE, NONE, 2, 0, 1, 1], (1, 0))
        step("both kinds in one list", [5, NONE, NONE, 3, 0, 2, 1], (1, 0))
        # a list that is refused changes nothing: buffer 5 holds an unscaled result, and a SCALE_WRITE operation on it with a matrix
        # index past the end never runs -- whoever reads buffer 5 next still takes the range-safe form
        refused(inst, [5, 1, NONE, 0, 0, 1, 7], 5)
        assert inst.get_range_safe_counts() == seen[-1]
        step("the destination of a refused rescaling list", [6, NONE, NONE, 5, 0, 1, 1], (1, 0))
        # indices out of range, destination and children, far and near: refused before anything is read or written with them
        # (the instance has 8 + 2 buffers: 10 is one past the end)
        for row in ([1000000, NONE, NONE, 0, 0, 1, 1], [-5, NONE, NONE, 0, 0, 1, 1], [10, NONE, NONE, 0, 0, 1, 1],
                    [5, NONE, NONE, 1000000, 0, 1, 1], [5, NONE, NONE, 0, 0, -7, 1], [5, 0, NONE, 0, 0, 10, 1]):
            refused(inst, row, 3)
        assert inst.get_range_safe_counts() == seen[-1]
        step("a valid list after the refused ones", [4, NONE, NONE, 3, 0, 1, 1], (0, 1))
    finally:
        inst.finalize()


def refused(inst, row, readable):
    """the operation is refused with BEAGLE_ERROR_OUT_OF_RANGE -- when it is submitted or, where lists are queued, by the call that
    flushes the queue"""
    with pytest.raises(bg.BeagleError) as err:
        inst.update_partials(np.array([row], dtype=np.int32), NONE)
        inst.get_partials(readable)
    assert err.value.code == bg.BEAGLE_ERROR_OUT_OF_RANGE, err.value


@pytest.mark.parametrize("S,K,P", [(40, 1, 40), (61, 1, 33), (20, 2, 40)])
def test_choice_of_instantiation_on_emulation(emu, S, K, P):
    check_choice(emu, S, K, P)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,P", [(40, 1, 40), (61, 1, 33), (20, 2, 40)])
def test_choice_of_instantiation(gpu, S, K, P):
    check_choice(gpu, S, K, P)


# ---- 6. the top of the range -------------------------------------------------------------------------------------------------------
# The range-safe form multiplies a row value by 2^24 before the split and the finished factor comes out times 2^24: operands and
# factors must stay below 2^103 ("Operand range": a limit of lists that read partials of unknown magnitude at 40 and 60-63
# states; the plain form and the other state counts reach 2^127).  Columns at 2^60 ... 2^100 against ordinary ones: the relative
# bound alone decides (the absolute term is there and means nothing), finite results, exponents as the reference's.
def check_top_of_range(lib, S, K, P):
    rng = np.random.default_rng(23 + S)
    B_op = operation_bound(S, False)
    inst = bg.BeagleInstance(lib, 2, 8, 2, S, P, 1, 2, K, 3, preference_flags=preference(False))
    try:
        name = inst.details.implName.decode()
        assert expected_layout(S, K, False) in name, name
        ti = [random_matrices(rng, S, K, False), random_matrices(rng, S, K, False)]
        for n in (0, 1):
            inst.set_transition_matrix(n, ti[n])
        st = rng.integers(0, S, size=P).astype(np.int32)
        inst.set_tip_states(0, st)
        big, m_of = tiny_columns(rng, S, K, P, (-60, -80, -90, -96, -100))
        assert float(big.max()) < 2.0 ** 101 and float(big.max()) >= 2.0 ** 99
        po = ordinary(rng, S, K, P, large=False, dead=False)
        inst.set_partials(2, big)
        inst.set_partials(3, po)
        wide = {0: REF.widen(dense_tip(st, S, K)), 2: REF.widen(big), 3: REF.widen(po)}
        wm = [REF.widen(m) for m in ti]
        worst = 0.0
        for kind, c1, c2 in (("large partials,partials", 2, 3), ("states,large partials", 0, 2)):
            f1, f2 = REF.factors(wm[0], wide[c1], wm[1], wide[c2])
            want = f1 * f2
            inst.update_partials(np.array([[4, NONE, NONE, c1, 0, c2, 1]], dtype=np.int32), NONE)
            got = inst.get_partials(4)
            assert np.isfinite(got).all(), kind
            r0 = ratio(got, want, allowance(S, want, f1, f2))
            inst.reset_scale_factors(1)
            inst.update_partials(np.array([[5, 0, NONE, c1, 0, c2, 1]], dtype=np.int32), 1)
            got2, e = inst.get_partials(5), inst.get_scale_exponents(0)
            assert np.isfinite(got2).all(), kind
            r1 = ratio(REF.scaled(got2, e[:, :, None]), want, allowance(S, want, f1, f2))
            e_ref, near = REF.exponents(want.max(axis=2), B_op, LO, HI)
            assert near.sum() <= 0.01 * near.size and np.array_equal(e[~near], e_ref[~near]), kind
            print("%s %-26s worst error / bound: unscaled %.3f, scaled %.3f" % (tag(S, K, P), kind, r0, r1))
            assert r0 <= 1.0 and r1 <= 1.0, (kind, r0, r1)
            worst = max(worst, r0, r1)
        print("%s TOP OF RANGE worst error / bound %.3f; %s" % (tag(S, K, P), worst, name.split(": ", 1)[-1]))
    finally:
        inst.finalize()


TOP_SHAPES = [(20, 1, 40), (40, 1, 40), (61, 1, 33)]


@pytest.mark.parametrize("S,K,P", TOP_SHAPES)
def test_top_of_range_on_emulation(emu, S, K, P):
    check_top_of_range(emu, S, K, P)


@pytest.mark.gpu
@pytest.mark.parametrize("S,K,P", TOP_SHAPES)
def test_top_of_range(gpu, S, K, P):
    check_top_of_range(gpu, S, K, P)
