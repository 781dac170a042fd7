"""Autocorrelated rates: the site-order HMM over the rate categories on the device (mbamdCalculateAutocorrelatedLogLikelihood;
csrc/mbamd_autocorrelated.h, include/libhmsbeagle/mbamd_reports.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

The reference (tests/autocorrelated_reference.py) is a sequential forward-backward pass in np.longdouble with per-site
normalisation on the engine's OWN q and l (mbamdGetCategoryPosteriors, beagleGetSiteLogLikelihoods) -- which isolates the new code
--, T^(j) by the header's exponentiation rule in longdouble; the brute-force test alone starts from the reference pruning.

The bound, derived from the code and not tuned (u = 2^-53, first order; R = HMM_CHUNK).  Every number is non-negative, so nothing
cancels: a product of two matrices whose entries carry the relative errors e1 and e2 carries e1 + e2 + K u (an FMA chain of K
terms), however the factors are bracketed, and the scalings by powers of two are exact.
  * a site's factor A_s = T^(j_s) diag(q / w): the division, u; the scaling of the column, u; T^(j) itself c_pow(j) u with
    c_pow(j) = K (j - 1) -- hmm_power multiplies floor(log2 j) + popcount(j) - 1 times, but a SQUARING doubles the relative error
    of its operand before it adds K u, so e(2m) = 2 e(m) + K u, e(2m + 1) = e(2m) + K u, e(1) = 0, whence e(j) = (j - 1) K u: the
    error of a power grows with j, not with log j (the 2 K ceil(log2 j) that counts the multiplications alone is no bound);
  * the multiplications: n - ceil(n / R) in the leaf pass, fewer than ceil(n / R) above it, K u each;
  * the end: the K^2 entries of the last product are added (K^2 u), ln, the exponent times ln 2 and the two additions round
    relative to their values: (4 (|correction| + ln(2 K^2)) + |ln H| + sum |l|) u;
  * sum_s l(c_s), added in the tree's order: a site's value passes through at most min(n - 1, (R - 1) levels) additions, each
    rounding relative to a partial sum that is at most sum |l|.
    |ln H - ref| <= [K (n + ceil(n/R)) + 2 n + sum_s c_pow(j_s) + K^2] u + (4 (|corr| + ln 2K^2) + |ln H| + sum |l|) u
                    + min(n - 1, (R - 1) levels) u sum |l|
alpha_s beta_s is such a product of all n factors (the chunk's own sites are walked again, the vectors pass through at most R
vector-matrix steps per level), gamma a ratio of it and a sum of K of them:
    |gamma - ref| <= { 2 [K (n + 2 ceil(n/R) + R (levels + 1)) + 2 n + sum_s c_pow(j_s) + 1] + K + 1 } u ref     per component,
and a gamma whose reference is exactly 0 must be exactly 0.  Every test prints its worst error / bound.

Measured on the MI355X (profiles/autocorrelated_rates.txt), worst error / bound over all cases of both engines: ln H 0.101,
gamma 0.0092, the brute-force enumeration 0.0033 of its tolerance; on the host emulation 0.0998, 0.0098 and the same.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests import autocorrelated_reference as ar
from tests.hostemu import build_emu
from tests.preorder_reference import division, post_order, unit_roundoff
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
SENTINEL = -7.5
R = 64                     # HMM_CHUNK, mrbayes_amd/csrc/mbamd_autocorrelated.h:33

#        states, categories, patterns, double precision
CASES = [(4, 4, 130, False), (4, 16, 70, False), (4, 5, 70, False), (20, 8, 70, False), (20, 2, 70, False), (61, 2, 64, False),
         (4, 4, 130, True), (20, 2, 70, True)]
SMALL = [(4, 4, 130, False), (4, 4, 130, True)]


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def test_chunk_length_is_the_headers():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrbayes_amd", "csrc", "mbamd_autocorrelated.h")).read()
    assert int(re.search(r"constexpr int HMM_CHUNK = (\d+);", src).group(1)) == R


class Held:
    """a division after LogLike, with what the engine holds of that call: q [K][P], l [P]; w the category weights"""

    def __init__(self, lib, states, ncat, npat, double_precision=False, read=True):
        self.div = division(states, ncat, npat)
        self.bd = lk.BeagleDivision(self.div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision)
        self.lnl = self.bd.LogLike(0)
        self.bd.AcceptMove(0)
        self.inst, self.K, self.P = self.bd.inst, ncat, npat
        self.w = np.asarray(self.div.category_weights(0), dtype=np.float64)
        self.widx = self.bd.cijkIndex[0]
        if read:
            self.q = self.inst.get_category_posteriors(self.widx)
            self.l = self.inst.get_site_log_likelihoods()

    def call(self, patterns, T, jumps=None, posteriors=True):
        return self.inst.autocorrelated_log_likelihood(self.widx, patterns, T, jumps=jumps, posteriors=posteriors)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bd.finalize()


def sites(n, P, seed=3):
    """n sites drawn with repetition from the patterns"""
    return np.random.default_rng(seed).integers(0, P, size=n).astype(np.int32)


def row_stochastic(K, seed=5):
    T = np.random.default_rng(seed).random((K, K)) + 0.05
    return T / T.sum(1, keepdims=True)


def doubly_stochastic(K, rho=0.6):
    return rho * np.eye(K) + (1.0 - rho) / K * np.ones((K, K))


def banded(K):
    """zero entries: a category moves to itself or to a neighbour"""
    T = np.eye(K) + np.eye(K, k=1) * 0.5 + np.eye(K, k=-1) * 0.25
    return T / T.sum(1, keepdims=True)


def against_reference(h, patterns, T, jumps=None, what=""):
    """one call with posteriors against forward_backward on the engine's own q and l; returns (error / bound of ln H, of gamma)"""
    K, n = h.K, len(patterns)
    rc, lnH, gamma = h.call(patterns, T, jumps)
    assert rc == 0 and gamma.shape == (K, n)
    want, corr, g = ar.forward_backward(h.q, h.l, h.w, patterns, T, jumps)
    b, bg_rel = ar.bounds(n, K, R, jumps, h.l[patterns], corr, want)
    ratio = abs(float(lnH - want)) / b
    zero = g == 0.0
    assert np.all(gamma[zero] == 0.0)
    gratio = float((np.abs(gamma - g)[~zero] / (bg_rel * g[~zero])).max())
    col = float(np.abs(gamma.sum(0) - 1.0).max())
    print("%s n=%d K=%d: ln H %.12g, error / bound %.3g (bound %.3g); gamma %.3g; column sums off by %.3g" % (what, n, K, lnH, ratio, b, gratio, col))
    assert ratio <= 1.0 and gratio <= 1.0
    assert col <= K * 2.0 ** -52
    return ratio, gratio


# ---- 1. brute force -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def category_likelihoods(states, ncat, npat):
    """L_k(c) [K][P] over the root branch from the reference pruning (numpy float64, from the Division alone), and h"""
    div = division(states, ncat, npat)
    g = gradient_reference(states, ncat, npat)
    post, mats = post_order(div, g["lengths"])
    t = div.tree
    pi = np.asarray(div.pi, dtype=np.float64)
    return np.einsum("i,kci,kij,kcj->kc", pi, post[t.root_left], mats[t.root_left], post[t.root]), g


def check_brute_force(lib, states, ncat, npat, double_precision, n):
    """H over all K^n paths from the reference pruning's L_k(c): the formula itself.  The engine's L_k = q_k L / w_k carries the
    relative error 2 f (q) + f (L) of tests/test_node_posteriors.py per site: n 3 f, plus the bound of the module docstring."""
    Lk, g = category_likelihoods(states, ncat, npat)
    with Held(lib, states, ncat, npat, double_precision) as h:
        f = (h.div.nstates + 8) * (1 + 2 * g["h"]) * unit_roundoff(h.div, g, double_precision)
        for T, jumps in ((row_stochastic(ncat), None), (banded(ncat), [9, 1, 2, 5, 1, 3][:n]), (doubly_stochastic(ncat), None)):
            patterns = sites(n, npat, seed=7)
            rc, lnH, _ = h.call(patterns, T, jumps, posteriors=False)
            want = float(ar.brute_force(Lk, h.w, patterns, T, jumps))
            own = ar.forward_backward(h.q, h.l, h.w, patterns, T, jumps)
            tol = n * 3.0 * f + ar.bounds(n, ncat, R, jumps, h.l[patterns], own[1], own[0])[0]
            print("brute force %d states K=%d n=%d%s: ln H %.12g, all paths %.12g, error / tolerance %.3g" %
                  (states, ncat, n, " fp64" if double_precision else "", lnH, want, abs(lnH - want) / tol))
            assert rc == 0 and abs(lnH - want) <= tol


BRUTE = [(4, 4, 130, False, 6), (20, 2, 70, False, 6), (4, 4, 130, True, 5), (4, 1, 70, False, 4)]


@pytest.mark.parametrize("states,ncat,npat,double_precision,n", BRUTE)
def test_brute_force_on_emulation(emu, states, ncat, npat, double_precision, n):
    check_brute_force(emu, states, ncat, npat, double_precision, n)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision,n", BRUTE)
def test_brute_force(gpu, states, ncat, npat, double_precision, n):
    check_brute_force(gpu, states, ncat, npat, double_precision, n)


# ---- 2. independence, 3. perfect correlation, 4. general T ----------------------------------------------------------------------
def check_identities(lib, states, ncat, npat, double_precision):
    with Held(lib, states, ncat, npat, double_precision) as h:
        K, P, n = ncat, npat, 2 * R + 9
        patterns = sites(n, P)
        tag = "%d states%s" % (states, " fp64" if double_precision else "")
        # 2. every row of T equal to w / sum w: independent sites
        T = np.tile(h.w / h.w.sum(), (K, 1))
        rc, lnH, gamma = h.call(patterns, T)
        lsum = float(np.sum(h.l[patterns].astype(np.longdouble)))
        b, brel = ar.bounds(n, K, R, None, h.l[patterns], 0.0, lsum)
        print("%s independence: |ln H - sum l| / bound %.3g, gamma against q %.3g" %
              (tag, abs(lnH - lsum) / b, float((np.abs(gamma - h.q[:, patterns]) / (brel * h.q[:, patterns])).max())))
        assert rc == 0 and abs(lnH - lsum) <= b
        assert np.all(np.abs(gamma - h.q[:, patterns]) <= brel * h.q[:, patterns])
        # ... and with every site listed once per unit of (integer) pattern weight: the log-likelihood call's own sum, within ITS
        # bound -- P + 2 roundings relative to sum_c weight_c |l_c| at most, in whatever order the device adds -- plus ours
        weights = np.asarray(h.div.weights)
        assert np.array_equal(weights, np.round(weights))
        every = np.repeat(np.arange(P, dtype=np.int32), weights.astype(int))
        rc, lnH, _ = h.call(every, T, posteriors=False)
        b = ar.bounds(len(every), K, R, None, h.l[every], 0.0, h.lnl)[0] + (P + 2) * 2.0 ** -53 * float((weights * np.abs(h.l)).sum())
        print("%s independence, every site: ln H %.12g, the log-likelihood call %.12g, difference / bound %.3g" % (tag, lnH, h.lnl, abs(lnH - h.lnl) / b))
        assert rc == 0 and abs(lnH - h.lnl) <= b
        # 3. T = identity: one category for the whole sequence
        short = patterns[:R + 3]
        rc, lnH, gamma = h.call(short, np.eye(K))
        want, g = ar.perfectly_correlated(h.q, h.l, h.w, short)
        own = ar.forward_backward(h.q, h.l, h.w, short, np.eye(K))
        b, brel = ar.bounds(len(short), K, R, None, h.l[short], own[1], want)
        print("%s perfect correlation: |ln H - closed form| / bound %.3g, gamma %.3g" %
              (tag, abs(lnH - float(want)) / b, float((np.abs(gamma - g[:, None]) / (brel * g[:, None])).max())))
        assert rc == 0 and abs(lnH - float(want)) <= b
        assert np.all(np.abs(gamma - g[:, None]) <= brel * g[:, None])               # gamma_s(k) does not depend on s
        # 4. general T
        for name, T in (("random", row_stochastic(K)), ("doubly stochastic", doubly_stochastic(K)), ("banded", banded(K))):
            against_reference(h, patterns, T, what="%s %s" % (tag, name))


@pytest.mark.parametrize("states,ncat,npat,double_precision", CASES)
def test_identities_and_general_on_emulation(emu, states, ncat, npat, double_precision):
    check_identities(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", CASES)
def test_identities_and_general(gpu, states, ncat, npat, double_precision):
    check_identities(gpu, states, ncat, npat, double_precision)


# ---- 5. chunk boundaries, 6. jumps --------------------------------------------------------------------------------------------------
BOUNDARIES = [1, 2, R - 1, R, R + 1, 2 * R + 1, R * R - 1, R * R, R * R + 1, R * R + R + 1]


def check_boundaries(lib, states, ncat, npat, double_precision):
    """the smallest sizes that reach one, two and three levels and every ragged tail"""
    with Held(lib, states, ncat, npat, double_precision) as h:
        T = row_stochastic(ncat, seed=9)
        for n in BOUNDARIES:
            against_reference(h, sites(n, npat, seed=n), T, what="boundaries")


@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_chunk_boundaries_on_emulation(emu, states, ncat, npat, double_precision):
    check_boundaries(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_chunk_boundaries(gpu, states, ncat, npat, double_precision):
    check_boundaries(gpu, states, ncat, npat, double_precision)


def check_jumps(lib, states, ncat, npat, double_precision):
    with Held(lib, states, ncat, npat, double_precision) as h:
        n = 2 * R + 1
        patterns, T = sites(n, npat), row_stochastic(ncat, seed=2)
        bits = lambda r: (r[0], r[1], r[2].tobytes())
        plain = bits(h.call(patterns, T))
        assert bits(h.call(patterns, T, np.ones(n, dtype=np.int32))) == plain                # NULL is all ones
        mix = np.resize(np.array([1, 2, 3, 10, 11, 99, 100, 1000000], dtype=np.int32), n)
        against_reference(h, patterns, T, mix, what="jumps, a mix")
        own = np.arange(1, n + 1, dtype=np.int32)                                             # every site its own jump
        against_reference(h, patterns, T, own, what="jumps, all distinct")
        against_reference(h, patterns, banded(ncat), own, what="jumps, all distinct, banded")
        first = bits(h.call(patterns, T, mix))
        for j0 in (0, -5, 7):                                                                  # siteJumps[0] is ignored
            other = mix.copy()
            other[0] = j0
            assert bits(h.call(patterns, T, other)) == first
        assert first != plain


@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_jumps_on_emulation(emu, states, ncat, npat, double_precision):
    check_jumps(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_jumps(gpu, states, ncat, npat, double_precision):
    check_jumps(gpu, states, ncat, npat, double_precision)


# ---- 7. no underflow ------------------------------------------------------------------------------------------------------------------
def check_no_underflow(lib, states, ncat, npat, double_precision):
    """n = 20 000 sites that alternate between the pattern whose q peaks on the first category and the one whose q peaks on the
    last, under T = identity plus epsilon: the product u^T A_1 .. 1, unscaled, would be below 10^-400 (asserted on the reference)"""
    with Held(lib, states, ncat, npat, double_precision) as h:
        n, K = 20000, ncat
        a, b = int(np.argmax(h.q[0])), int(np.argmax(h.q[K - 1]))
        patterns = np.resize(np.array([a, b], dtype=np.int32), n)
        eps = 1e-3
        T = (1.0 - eps) * np.eye(K) + eps / K * np.ones((K, K))
        want, corr, _ = ar.forward_backward(h.q, h.l, h.w, patterns, T)
        assert float(corr) < -400.0 * math.log(10.0), float(corr)
        ratio, _ = against_reference(h, patterns, T, what="no underflow (correction %.6g)" % float(corr))
        rc, lnH, _ = h.call(patterns, T, posteriors=False)
        assert rc == 0 and math.isfinite(lnH)


@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_no_underflow_on_emulation(emu, states, ncat, npat, double_precision):
    check_no_underflow(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_no_underflow(gpu, states, ncat, npat, double_precision):
    check_no_underflow(gpu, states, ncat, npat, double_precision)


# ---- 8. determinism -------------------------------------------------------------------------------------------------------------------
def check_determinism(lib, double_precision):
    states, ncat, npat = 4, 4, 130
    n = R * R + 5
    levels = ar.levels(n, R)
    patterns, T, T2 = sites(n, npat), row_stochastic(ncat), doubly_stochastic(ncat)
    with Held(lib, states, ncat, npat, double_precision, read=False) as h:
        h.inst.get_kernel_timing(reset=True)
        rc, lnH, gamma = h.call(patterns, T)
        # cold: k_category_posteriors, one k_hmm_products per level, one k_hmm_vectors per level above the leaves, k_hmm_posteriors
        assert h.inst.get_kernel_timing(reset=True)[1] == 1 + levels + (levels - 1) + 1
        rc2, lnH2, gamma2 = h.call(patterns, T)
        assert h.inst.get_kernel_timing(reset=True)[1] == 2 * levels
        assert (rc, lnH) == (rc2, lnH2) and gamma.tobytes() == gamma2.tobytes()
        # without the posteriors: the same ln H, the reduction alone
        rc3, lnH3, none = h.call(patterns, T, posteriors=False)
        assert none is None and lnH3 == lnH and h.inst.get_kernel_timing(reset=True)[1] == levels
        # another T after the same log-likelihood call (the correlation move): q is kept, no k_category_posteriors launch
        rc4, lnH4, _ = h.call(patterns, T2, posteriors=False)
        assert rc4 == 0 and lnH4 != lnH and h.inst.get_kernel_timing(reset=True)[1] == levels
        # a new log-likelihood call: q is computed again
        h.inst.calculate_edge_log_likelihoods(*edge_call(h.bd))
        h.inst.get_kernel_timing(reset=True)
        rc5, lnH5, _ = h.call(patterns, T, posteriors=False)
        assert rc5 == 0 and abs(lnH5 - lnH) <= 1e-5 * abs(lnH) and h.inst.get_kernel_timing(reset=True)[1] == 1 + levels
    return lnH, gamma


def edge_call(bd):
    """the operands of the division's log-likelihood call, as index lists"""
    t = bd.div.tree
    top = t.root_left
    return ([bd.condLikeIndex[0][top]], [bd.condLikeIndex[0][t.root]], [bd.tiProbsIndex[0][top]], [bd.cijkIndex[0]], [bd.cijkIndex[0]],
            [bd.siteScalerIndex[0]])


def check_sharded(lib, monkeypatch):
    """MBAMD_SHARD=2 (two engines, each with its part of the patterns): the bits of the plain instance"""
    states, ncat, npat = 4, 4, 130
    n = 2 * R + 1
    patterns, T = sites(n, npat), row_stochastic(ncat)
    jumps = np.resize(np.array([1, 3, 2], dtype=np.int32), n)
    out = []
    for shard in (None, "2"):
        monkeypatch.delenv("MBAMD_SHARD", raising=False)
        if shard:
            monkeypatch.setenv("MBAMD_SHARD", shard)
        try:
            with Held(lib, states, ncat, npat, read=False) as h:
                rc, lnH, gamma = h.call(patterns, T, jumps)
                out.append((h.inst.child_count(), rc, lnH, gamma.tobytes()))
        finally:
            monkeypatch.delenv("MBAMD_SHARD", raising=False)
    assert (out[0][0], out[1][0]) == (1, 2)
    assert out[0][1:] == out[1][1:]


def test_determinism_on_emulation(emu):
    check_determinism(emu, False)
    check_determinism(emu, True)


def test_sharded_on_emulation(emu, monkeypatch):
    check_sharded(emu, monkeypatch)


@pytest.mark.gpu
def test_determinism(gpu):
    check_determinism(gpu, False)
    check_determinism(gpu, True)


@pytest.mark.gpu
def test_sharded(gpu, monkeypatch):
    check_sharded(gpu, monkeypatch)


# ---- 9. an underflowed pattern ----------------------------------------------------------------------------------------------------------
def check_underflowed_pattern(lib, states, ncat, npat, double_precision):
    """A pattern whose top column is zero in every category (forced by hand, as tests/test_ancestral_sampling.py does): L = 0, all
    its q are zero.  A call that lists it writes -inf and zeros and returns BEAGLE_ERROR_FLOATING_POINT; one that does not is served."""
    with Held(lib, states, ncat, npat, double_precision, read=False) as h:
        bd, dead = h.bd, 5
        top = bd.condLikeIndex[0][h.div.tree.root_left]
        partials = h.inst.get_partials(top)
        partials[:, dead, :] = 0.0
        h.inst.set_partials(top, partials)
        rc, lnl = bd.TreeLikelihood_Beagle(0)
        assert not np.isfinite(lnl)
        h.q, h.l = h.inst.get_category_posteriors(h.widx), h.inst.get_site_log_likelihoods()
        assert np.all(h.q[:, dead] == 0.0)
        T = row_stochastic(ncat)
        patterns = sites(R + 7, npat)
        patterns[patterns == dead] = dead + 1
        against_reference(h, patterns, T, what="beside an underflowed pattern")
        patterns[R + 1] = dead
        rc, lnH, gamma = h.call(patterns, T)
        assert rc == bg.BEAGLE_ERROR_FLOATING_POINT and lnH == -math.inf and np.all(gamma == 0.0)
        rc, lnH, _ = h.call(patterns, T, posteriors=False)
        assert rc == bg.BEAGLE_ERROR_FLOATING_POINT and lnH == -math.inf


@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_underflowed_pattern_on_emulation(emu, states, ncat, npat, double_precision):
    check_underflowed_pattern(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", SMALL)
def test_underflowed_pattern(gpu, states, ncat, npat, double_precision):
    check_underflowed_pattern(gpu, states, ncat, npat, double_precision)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, ncat, double_precision=False):
    """Every bad call is refused with the expected status and writes nothing to its outputs; returns (status, message) of each, in
    order: the two engines run one body (mbamd_autocorrelated.h), so they answer alike."""
    seen = []
    P, n = 130, 70
    div = division(4, ncat, P)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision)
    good_T = doubly_stochastic(ncat)
    try:
        inst = bd.inst

        def call(widx, patterns, T, jumps=None, count=None, null_out=False):
            c = None if patterns is None else np.asarray(patterns, dtype=np.int32)
            j = None if jumps is None else np.asarray(jumps, dtype=np.int32)
            t = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
            outs = [np.full(1, SENTINEL), np.full(ncat * n, SENTINEL)]
            rc = inst.lib.mbamdCalculateAutocorrelatedLogLikelihood(inst.id, widx, None if c is None else c.ctypes.data_as(_ip),
                                                                    None if j is None else j.ctypes.data_as(_ip), n if count is None else count,
                                                                    None if t is None else t.ctypes.data_as(_dp),
                                                                    None if null_out else outs[0].ctypes.data_as(_dp), outs[1].ctypes.data_as(_dp))
            return rc, outs

        def raises(code, *args, **kw):
            rc, outs = call(*args, **kw)
            assert rc == code, (rc, code, lib.last_error())
            assert lib.last_error() and all(np.all(o == SENTINEL) for o in outs)
            seen.append((rc, lib.last_error()))

        patterns = sites(n, P)
        # no log-likelihood call yet (what beagleGetSiteLogLikelihoods refuses with, too): with one category as well
        raises(bg.BEAGLE_ERROR_GENERAL, bd.cijkIndex[0], patterns, good_T)
        with pytest.raises(bg.BeagleError) as err:
            inst.get_site_log_likelihoods()
        assert err.value.code == bg.BEAGLE_ERROR_GENERAL
        bd.LogLike(0)
        bd.AcceptMove(0)
        w = bd.cijkIndex[0]
        rc, outs = call(w, patterns, good_T)
        assert rc == 0 and np.isfinite(outs[0][0]) and np.all(outs[1] >= 0.0)
        # a weights index that is not the call's
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, bd.cijkScratchIndex, patterns, good_T)
        # siteCount < 1; NULL arrays
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, good_T, count=0)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, good_T, count=-3)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, None, good_T)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, None)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, good_T, null_out=True)
        # a pattern index outside [0, patternCount)
        for bad in (-1, P):
            other = patterns.copy()
            other[n - 1] = bad
            raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, other, good_T)
        # a jump < 1 behind site 0
        for bad in (0, -2):
            jumps = np.ones(n, dtype=np.int32)
            jumps[1] = bad
            raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, good_T, jumps=jumps)
        # an entry of T that is negative or not finite (one category: T is read to be checked, and for nothing else)
        for bad in (-1e-9, math.nan, math.inf):
            T = good_T.copy()
            T[ncat - 1, 0] = bad
            raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, T)
        # the latest log-likelihood call had several subsets
        two = lambda v: v + v
        inst.calculate_edge_log_likelihoods(*[two(v) for v in edge_call(bd)])
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, w, patterns, good_T)
        # a weight that is not positive: the emission of such a category is not in q
        zero = np.asarray(div.category_weights(0), dtype=np.float64).copy()
        zero[0] = 0.0
        inst.set_category_weights(w, zero)
        inst.calculate_edge_log_likelihoods(*edge_call(bd))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, w, patterns, good_T)
    finally:
        bd.finalize()
    # a multi-partition instance does not serve the call
    N = NTAXA
    flags = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
    inst = bg.BeagleInstance(lib, N, 3 * N, N, 4, P, 2, 4 * N, ncat, N, preference_flags=flags)
    try:
        for tip in range(N):
            inst.set_tip_states(tip, np.asarray(div.tip_states[tip]).astype(np.int32))
        inst.set_pattern_weights(div.weights)
        inst.set_pattern_partitions(2, np.concatenate([np.zeros(70, dtype=np.int32), np.ones(60, dtype=np.int32)]))
        assert inst.child_count() == 2
        with pytest.raises(bg.BeagleError) as err:
            inst.autocorrelated_log_likelihood(0, [0, 1], good_T)
        assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION
        seen.append((err.value.code, lib.last_error()))
    finally:
        inst.finalize()
    return seen


def check_engines_agree(lib):
    for ncat in (2, 1):
        single, double = check_refusals(lib, ncat), check_refusals(lib, ncat, double_precision=True)
        assert len(single) == len(double) == 17
        for i, (s, d) in enumerate(zip(single, double)):
            assert s[0] == d[0], (i, s, d)


def test_refusals_on_emulation(emu):
    check_engines_agree(emu)


@pytest.mark.gpu
def test_refusals(gpu):
    check_engines_agree(gpu)


# ---- 11. one category -------------------------------------------------------------------------------------------------------------------
def check_one_category(lib, states, npat, double_precision):
    """K = 1: ln H = sum_s l(c_s), gamma = 1, whatever T holds"""
    with Held(lib, states, 1, npat, double_precision) as h:
        for n in (1, R + 2, R * R + 3):
            patterns = sites(n, npat, seed=n)
            jumps = np.resize(np.array([1, 4], dtype=np.int32), n)
            rc, lnH, gamma = h.call(patterns, [[0.25]], jumps)
            lsum = float(np.sum(h.l[patterns].astype(np.longdouble)))
            b = ar.bounds(n, 1, R, None, h.l[patterns], 0.0, lsum)[0]
            print("one category, %d states n=%d: |ln H - sum l| / bound %.3g" % (states, n, abs(lnH - lsum) / b))
            assert rc == 0 and abs(lnH - lsum) <= b and np.all(gamma == 1.0) and gamma.shape == (1, n)
            assert h.call(patterns, [[3.0]], None, posteriors=False)[1] == lnH


ONE = [(61, 40, False), (4, 70, False), (4, 70, True)]


@pytest.mark.parametrize("states,npat,double_precision", ONE)
def test_one_category_on_emulation(emu, states, npat, double_precision):
    check_one_category(emu, states, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,npat,double_precision", ONE)
def test_one_category(gpu, states, npat, double_precision):
    check_one_category(gpu, states, npat, double_precision)
