"""One draw of all ancestral states from their joint posterior (mbamdSampleAncestralStates; csrc/mbamd_ancestral_sampling.h,
include/libhmsbeagle/mbamd_reports.h).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on the host);
  * GPU (`gpu`): the product library on a MI355X.

1. Draw for draw against the numpy float64 reference of tests/ancestral_sampling_reference.py, which follows the header to the
   letter on what the engine holds; the allowance eps around a cumulative boundary is derived in that module's docstring (4 u on an
   edge, 2 (S + 4) u at the top, nothing for the category).  A draw whose margin exceeds eps matches exactly; at most 1 % of a
   case's draws may lie inside eps -- the seed is fixed here, and the share is asserted from the reference's margins alone.
2. The draws ARE from the joint posterior: over the seeds 1 .. R the frequency of every state at every node and pattern lies within
   6 sqrt(p (1 - p) / R) + 1 / R of the marginal posterior p that NodePosteriors(sites=True) returns on the same instance, and on
   one interior branch the frequency of every (parent state, child state) pair within the same bound of the pair posterior formed
   in numpy from tests/preorder_reference.py.  R = 4000: a pair of posterior 0.005 has 20 expected hits.
3. Structure: a depth-first list (more launches, other streams) is as right as the breadth-first one; calls repeat bit for bit and
   change with the seed; pattern shards and pattern ranges return the unsharded arrays bit for bit; count == 0; an underflowed
   pattern is -1 throughout.  (Streams are tied to edge positions, so one tree cannot be listed in two orders with the same draw.)
4. Every refusal of the header, on both engines alike, with the outputs untouched.
"""
import ctypes as C

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from tests import ancestral_sampling_reference as ar
from tests.hostemu import build_emu
from tests.preorder_reference import division, post_order, pre_order
from tests.preorder_reference import reference as gradient_reference
from tests.pruning_reference import NTAXA, interior_edge
from tests.test_derivatives import expected_layout

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
SENTINEL = -7

#        states, categories, patterns                     what it reaches
CASES = [(4, 4, 130),             # two full 64-pattern blocks plus 2 patterns, bitplane tips
         (4, 9, 70),              # a second batch of eight categories
         (20, 4, 70),             # tree-walk tiles
         (61, 1, 40),             # one category: no q
         (12, 6, 70)]             # the level kernels' layout
CASES_F64 = [(4, 4, 130), (20, 2, 70)]
SEED = 1
R = 4000


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def new_division(lib, div, double_precision=False):
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision, pre_order=True)
    bd.LogLike(0)
    bd.AcceptMove(0)
    return bd


def depth_first_edges(bd):
    """the edges of AncestralSamplingEdges in depth-first order: a child right behind its parent's subtree start"""
    t = bd.div.tree
    top = t.root_left
    nodes, parents = [top, t.root], [0]

    def walk(p, slot):
        for n in (t.left[p], t.right[p]):
            nodes.append(n)
            parents.append(slot)
            if t.left[n] >= 0:
                walk(n, len(nodes) - 1)
    walk(top, 0)
    return nodes, parents, [bd.condLikeIndex[0][n] for n in nodes[1:]], [bd.tiProbsIndex[0][n if n != t.root else top] for n in nodes[1:]]


def launches_of(parents):
    """the greedy cut of the header: consecutive edges whose parent slots all lie before the launch's first slot"""
    groups, first = 0, None
    for i, slot in enumerate(parents):
        if first is None or slot > first:
            groups, first = groups + 1, i
    return groups


def held_by(bd, edges):
    """what the engine holds, as ancestral_sampling_reference.judge takes it"""
    div, inst, t = bd.div, bd.inst, bd.div.tree
    nodes, parents, posts, mats = edges
    operand = lambda n, idx: np.asarray(div.tip_states[n]) if n < t.ntaxa else inst.get_partials(idx)
    return dict(q=inst.get_category_posteriors(bd.cijkIndex[0]) if div.ncat > 1 else None, freqs=np.asarray(div.pi, dtype=np.float64),
                top=inst.get_partials(bd.condLikeIndex[0][t.root_left]), lnl_child=np.asarray(div.tip_states[t.root]),
                lnl_matrix=inst.get_transition_matrix(bd.tiProbsIndex[0][t.root_left]),
                edges=[(parents[i], operand(n, posts[i]), inst.get_transition_matrix(mats[i])) for i, n in enumerate(nodes[1:])])


def draw(bd, edges, seed, **kw):
    _, parents, posts, mats = edges
    rc, states, cats, counts = bd.inst.sample_ancestral_states(parents, posts, mats, bd.cijkIndex[0], seed, categories=True, changes=True, **kw)
    assert rc == 0
    return states, cats, counts


# ---- 1. draw for draw ---------------------------------------------------------------------------------------------------------------
def check_draws(lib, states, ncat, npat, double_precision=False, depth_first=False):
    div = division(states, ncat, npat)
    bd = new_division(lib, div, double_precision)
    try:
        name = bd.inst.details.implName.decode()
        assert expected_layout(states, ncat, double_precision) in name, name
        t, S = div.tree, div.nstates
        edges = depth_first_edges(bd) if depth_first else bd.AncestralSamplingEdges(0)
        nodes, parents = edges[0], edges[1]
        assert len(nodes) == 2 * t.ntaxa - 2 and sorted(nodes) == sorted(list(t.all_down_pass) + [t.root])
        got, cats, counts = draw(bd, edges, SEED)
        assert got.shape == (len(nodes), npat) and cats.shape == (npat,) and counts.shape == (len(parents),)
        # the wrapper is the raw call on the breadth-first list
        if not depth_first:
            by_node, cats_w, changes_w = bd.SampleAncestralStates(0, seed=SEED, categories=True, changes=True)
            assert all(np.array_equal(by_node[n], got[i]) for i, n in enumerate(nodes)) and np.array_equal(cats_w, cats)
            assert [changes_w[n] for n in nodes[1:]] == list(counts)
        assert np.all((cats >= 0) & (cats < ncat))
        if ncat == 1:
            assert np.all(cats == 0)
        judged = ar.judge(held_by(bd, edges), SEED, got, cats, 2.0 ** -53 if double_precision else 2.0 ** -24)
        excused = total = forced = missing = 0
        for j, r in enumerate(judged):
            if r is None:
                continue
            mine = cats if j == 0 else got[j - 1]
            clear = r["margin"] > r["eps"]
            print("%s: %d of %d draws inside eps = %.3g, smallest margin outside %.3g" %
                  (r["name"], int((~clear).sum()), npat, r["eps"], float(r["margin"][clear].min())))
            assert np.array_equal(mine[clear], r["want"][clear]), (r["name"], np.flatnonzero(clear & (mine != r["want"])))
            excused += int((~clear).sum())
            total += npat
            # a tip with one compatible state is that state; no state of reference weight 0 is ever returned
            assert np.array_equal(mine[r["forced"]], r["want"][r["forced"]])
            there = mine >= 0
            assert np.all(r["weights"][np.arange(npat)[there], mine[there]] > 0.0), r["name"]
            forced += int(r["forced"].sum())
            if j >= 2 and nodes[j - 1] < t.ntaxa:
                missing += int((np.asarray(div.tip_states[nodes[j - 1]]) >= S).sum())
        print("%d states x %d x %d%s%s: %d of %d draws inside eps" %
              (states, ncat, npat, " fp64" if double_precision else "", " depth-first" if depth_first else "", excused, total))
        assert excused <= 0.01 * total, (excused, total)
        assert forced > 0 and missing > 0
        # the sampled substitutions are those of the returned states (pattern weights are exact in double)
        want = ar.change_counts(got, parents, div.weights)
        assert np.all(np.abs(counts - want) <= 1e-12 * np.abs(want)), (counts, want)
        assert want.sum() > 0
    finally:
        bd.finalize()


@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_draws_on_emulation(emu, states, ncat, npat):
    check_draws(emu, states, ncat, npat)


@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_draws_double_precision_on_emulation(emu, states, ncat, npat):
    check_draws(emu, states, ncat, npat, double_precision=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES)
def test_draws(gpu, states, ncat, npat):
    check_draws(gpu, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", CASES_F64)
def test_draws_double_precision(gpu, states, ncat, npat):
    check_draws(gpu, states, ncat, npat, double_precision=True)


# ---- 2. the joint posterior -----------------------------------------------------------------------------------------------------------
def pair_posterior(div, v):
    """[P][S][S]: the posterior of (state at v's parent, state at v) from tests/preorder_reference.py, in float64"""
    t = div.tree
    g = gradient_reference(div.nstates, div.ncat, div.npatterns)
    post, mats = post_order(div, g["lengths"])
    pre = pre_order(div, post, mats)
    p = t.anc[v]
    sib = t.right[p] if t.left[p] == v else t.left[p]
    tmp = pre[p] * np.einsum("kij,kcj->kci", mats[sib], post[sib])
    joint = np.einsum("k,kca,kab,kcb->cab", div.category_weights(0), tmp, mats[v], post[v])
    return joint / joint.sum(axis=(1, 2), keepdims=True)


def check_joint(lib):
    div = division(4, 4, 130)
    t, S, P = div.tree, 4, 130
    bd = new_division(lib, div)
    try:
        edges = bd.AncestralSamplingEdges(0)
        nodes, parents, posts, mats = edges
        v, _ = interior_edge(t)
        slot_v = nodes.index(v)
        assert parents[slot_v - 1] == 0 and t.anc[v] == t.root_left
        hits = np.zeros((len(nodes), P, S))
        pairs = np.zeros((P, S, S))
        cols = np.arange(P)
        for seed in range(1, R + 1):
            rc, states, _, _ = bd.inst.sample_ancestral_states(parents, posts, mats, bd.cijkIndex[0], seed)
            assert states.min() >= 0
            for s in range(len(nodes)):
                hits[s, cols, states[s]] += 1.0
            pairs[cols, states[0], states[slot_v]] += 1.0
        _, marginal = bd.NodePosteriors(0, sites=True)
        bound = lambda p: 6.0 * np.sqrt(p * (1.0 - p) / R) + 1.0 / R
        worst = 0.0
        for s, n in enumerate(nodes):
            if n == t.root:
                # the root tip is not a node of NodePosteriors: its observed states are returned as they are
                st = np.asarray(div.tip_states[n])
                assert np.all(hits[s][cols[st < S], st[st < S]] == R)
                continue
            p = np.clip(marginal[n], 0.0, 1.0)
            worst = max(worst, float((np.abs(hits[s] / R - p) / bound(p)).max()))
        pp = pair_posterior(div, v)
        worst_pair = float((np.abs(pairs / R - pp) / bound(pp)).max())
        interesting = pp[pp * R >= 20.0]
        print("R = %d: |frequency - posterior| / bound, worst over %d nodes x %d patterns x %d states %.3f; over the %d x %d x %d pairs of the "
              "branch above node %d %.3f (%d pairs with at least 20 expected hits, the smallest of posterior %.4f)" %
              (R, len(nodes) - 1, P, S, worst, P, S, S, v, worst_pair, interesting.size, float(interesting.min())))
        assert interesting.size > P
        assert worst <= 1.0 and worst_pair <= 1.0, (worst, worst_pair)
    finally:
        bd.finalize()


def test_joint_posterior_on_emulation(emu):
    check_joint(emu)


@pytest.mark.gpu
def test_joint_posterior(gpu):
    check_joint(gpu)


# ---- 3. structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("states,ncat,npat,double_precision", [(4, 4, 130, False), (20, 4, 70, False), (20, 2, 70, True)])
def test_depth_first_draws_on_emulation(emu, states, ncat, npat, double_precision):
    check_draws(emu, states, ncat, npat, double_precision, depth_first=True)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", [(4, 4, 130, False), (20, 4, 70, False), (20, 2, 70, True)])
def test_depth_first_draws(gpu, states, ncat, npat, double_precision):
    check_draws(gpu, states, ncat, npat, double_precision, depth_first=True)


def check_launches_and_seeds(lib, double_precision=False):
    """one launch for the top, one per group of the greedy cut, one for the sums; the same call twice is the same arrays, another seed
    is not"""
    div = division(4, 4, 130)
    bd = new_division(lib, div, double_precision)
    try:
        seen = {}
        for name, edges in (("breadth", bd.AncestralSamplingEdges(0)), ("depth", depth_first_edges(bd))):
            first = draw(bd, edges, SEED)
            bd.inst.get_kernel_timing(reset=True)
            again = draw(bd, edges, SEED)
            _, launches = bd.inst.get_kernel_timing(reset=True)
            other = draw(bd, edges, SEED + 1)
            assert all(np.array_equal(x, y) for x, y in zip(first, again))
            assert not np.array_equal(first[0], other[0]) and not np.array_equal(first[1], other[1])
            assert launches == 2 + launches_of(edges[1]), (name, launches, launches_of(edges[1]))
            seen[name] = (launches, first, edges[0])
        assert seen["breadth"][0] < seen["depth"][0]
        # slot 0, the root tip's edge and the category do not depend on the order of the list (streams 0, 1 and 2)
        assert np.array_equal(seen["breadth"][1][1], seen["depth"][1][1])
        assert np.array_equal(seen["breadth"][1][0][:2], seen["depth"][1][0][:2])
        # count == 0: the top alone
        rc, top, cats, counts = bd.inst.sample_ancestral_states([], [], [], bd.cijkIndex[0], SEED, categories=True, changes=True)
        assert rc == 0 and top.shape == (1, 130) and counts.shape == (0,)
        assert np.array_equal(top[0], seen["breadth"][1][0][0]) and np.array_equal(cats, seen["breadth"][1][1])
    finally:
        bd.finalize()


def test_launches_and_seeds_on_emulation(emu):
    check_launches_and_seeds(emu)
    check_launches_and_seeds(emu, double_precision=True)


@pytest.mark.gpu
def test_launches_and_seeds(gpu):
    check_launches_and_seeds(gpu)
    check_launches_and_seeds(gpu, double_precision=True)


def check_launch_cap(lib):
    """32768 + 5 edges that all hang from slot 0 (the root tip, again and again): the cut has nothing to cut, so the cap of 32768
    edges per launch does -- two launches of edges; the edges on either side of the cap, and the last, are drawn as the header says"""
    div = division(4, 9, 70)
    bd = new_division(lib, div)
    try:
        t, S, P, count = div.tree, 4, 70, 32768 + 5
        top = t.root_left
        parents, posts, mats = [0] * count, [bd.condLikeIndex[0][t.root]] * count, [bd.tiProbsIndex[0][top]] * count
        bd.inst.sample_ancestral_states(parents, posts, mats, bd.cijkIndex[0], SEED)
        bd.inst.get_kernel_timing(reset=True)
        rc, got, cats, counts = bd.inst.sample_ancestral_states(parents, posts, mats, bd.cijkIndex[0], SEED, categories=True, changes=True)
        _, launches = bd.inst.get_kernel_timing(reset=True)
        assert rc == 0 and launches == 2 + 2 and got.shape == (count + 1, P) and got.min() >= 0
        codes = np.asarray(div.tip_states[t.root])
        seen = codes < S
        assert np.all(got[1:, seen] == codes[seen][None, :]) and (~seen).any()
        matrix, c = bd.inst.get_transition_matrix(bd.tiProbsIndex[0][top]), np.arange(P)
        for i in (0, 32767, 32768, count - 1):
            want, margin = ar.pick(matrix[cats, got[0]] * ar.tip_weights(codes, S), ar.uniform(SEED, 2 + i, c))
            clear = ~seen & (margin > 4.0 * 2.0 ** -24)
            assert clear.any() and np.array_equal(got[i + 1][clear], want[clear]), i
        assert np.array_equal(counts, (div.weights[None, :] * (got[1:] != got[0][None, :])).sum(1))
    finally:
        bd.finalize()


def test_launch_cap_on_emulation(emu):
    check_launch_cap(emu)


@pytest.mark.gpu
def test_launch_cap(gpu):
    check_launch_cap(gpu)


def _one_draw(lib, div):
    bd = new_division(lib, div)
    try:
        return (bd.inst.child_count(),) + draw(bd, bd.AncestralSamplingEdges(0), SEED)
    finally:
        bd.finalize()


def check_sharded_and_ranges(lib, monkeypatch, states, ncat, npat):
    """MBAMD_SHARD=2 (two engines, each with its part of the patterns) and MBAMD_SAMPLE_PATTERNS=64 (one engine, one 64-pattern
    range after another): the arrays of the plain instance bit for bit, the change counts to the last bit"""
    div = division(states, ncat, npat)
    monkeypatch.delenv("MBAMD_SHARD", raising=False)
    monkeypatch.delenv("MBAMD_SAMPLE_PATTERNS", raising=False)
    n1, states1, cats1, counts1 = _one_draw(lib, div)
    monkeypatch.setenv("MBAMD_SHARD", "2")
    try:
        n2, states2, cats2, counts2 = _one_draw(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_SHARD")
    monkeypatch.setenv("MBAMD_SAMPLE_PATTERNS", "64")
    try:
        n3, states3, cats3, counts3 = _one_draw(lib, div)
    finally:
        monkeypatch.delenv("MBAMD_SAMPLE_PATTERNS")
    assert (n1, n2, n3) == (1, 2, 1)
    assert np.array_equal(states1, states2) and np.array_equal(cats1, cats2) and np.array_equal(counts1, counts2)
    assert np.array_equal(states1, states3) and np.array_equal(cats1, cats3) and np.array_equal(counts1, counts3)


@pytest.mark.parametrize("states,ncat,npat", [(4, 4, 130), (20, 4, 70)])
def test_sharded_and_ranges_on_emulation(emu, monkeypatch, states, ncat, npat):
    check_sharded_and_ranges(emu, monkeypatch, states, ncat, npat)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat", [(4, 4, 130), (20, 4, 70)])
def test_sharded_and_ranges(gpu, monkeypatch, states, ncat, npat):
    check_sharded_and_ranges(gpu, monkeypatch, states, ncat, npat)


def check_underflow(lib, states, ncat, npat, double_precision=False):
    """A pattern whose top column is zero in every category (forced by hand): q is all zero there, nothing can be drawn, every slot
    of the pattern is -1 and no change is counted; the other patterns keep their draw."""
    div = division(states, ncat, npat)
    bd = new_division(lib, div, double_precision)
    try:
        t, dead = div.tree, 5
        edges = bd.AncestralSamplingEdges(0)
        before = draw(bd, edges, SEED)
        top = bd.condLikeIndex[0][t.root_left]
        partials = bd.inst.get_partials(top)
        partials[:, dead, :] = 0.0
        bd.inst.set_partials(top, partials)
        rc, lnl = bd.TreeLikelihood_Beagle(0)
        assert not np.isfinite(lnl)
        if ncat > 1:
            q = bd.inst.get_category_posteriors(bd.cijkIndex[0])
            assert np.all(q[:, dead] == 0.0)
        got, cats, counts = draw(bd, edges, SEED)
        assert np.all(got[:, dead] == -1) and (ncat == 1 or cats[dead] == -1)
        alive = np.arange(npat) != dead
        assert np.array_equal(cats[alive], before[1][alive])
        assert got[:, alive].min() >= 0
        assert np.array_equal(counts, ar.change_counts(got, edges[1], div.weights))
    finally:
        bd.finalize()


UNDERFLOW_CASES = [(4, 4, 130, False), (61, 1, 40, False), (20, 2, 70, True)]


@pytest.mark.parametrize("states,ncat,npat,double_precision", UNDERFLOW_CASES)
def test_underflow_on_emulation(emu, states, ncat, npat, double_precision):
    check_underflow(emu, states, ncat, npat, double_precision)


@pytest.mark.gpu
@pytest.mark.parametrize("states,ncat,npat,double_precision", UNDERFLOW_CASES)
def test_underflow(gpu, states, ncat, npat, double_precision):
    check_underflow(gpu, states, ncat, npat, double_precision)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, ncat, double_precision=False):
    """Every bad call is refused with the expected status and writes nothing to its outputs; returns (status, message) of each, in
    order: the two engines run one body (mbamd_ancestral_sampling.h), so they answer alike."""
    seen = []
    div = division(4, ncat, 130)
    t, P = div.tree, 130
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision)
    try:
        inst = bd.inst

        def call(ix, n, null_states=False, seed=SEED):
            arrays = [None if ix[k] is None else np.asarray(ix[k], dtype=np.int32) for k in ("parents", "posts", "mats")]
            rows = max(n, 0) + 1
            outs = [np.full(rows * P, SENTINEL, dtype=np.int32), np.full(P, SENTINEL, dtype=np.int32), np.full(rows, float(SENTINEL))]
            rc = inst.lib.mbamdSampleAncestralStates(inst.id, *[None if a is None else a.ctypes.data_as(_ip) for a in arrays], n, ix["weights"], seed,
                                                     None if null_states else outs[0].ctypes.data_as(_ip), outs[1].ctypes.data_as(_ip),
                                                     outs[2].ctypes.data_as(_dp))
            return rc, outs

        def raises(code, ix, n=None, **kw):
            rc, outs = call(ix, len(ix["parents"]) if n is None else n, **kw)
            assert rc == code, (rc, code, lib.last_error())
            assert lib.last_error() and all(np.all(o == SENTINEL) for o in outs)
            seen.append((rc, lib.last_error()))

        def indices():
            _, parents, posts, mats = bd.AncestralSamplingEdges(0)
            return dict(parents=parents, posts=posts, mats=mats, weights=bd.cijkIndex[0])

        # no log-likelihood call yet: with one category too
        raises(bg.BEAGLE_ERROR_GENERAL, indices())
        raises(bg.BEAGLE_ERROR_GENERAL, dict(parents=[], posts=[], mats=[], weights=bd.cijkIndex[0]))
        bd.LogLike(0)
        bd.AcceptMove(0)
        ix = indices()                                                                  # (the evaluation flipped index tables)
        n = len(ix["parents"])
        rc, outs = call(ix, n)
        assert rc == 0 and outs[0].min() >= 0 and outs[1].min() >= 0 and outs[2][:n].min() >= 0.0 and outs[2][n] == SENTINEL
        # a weights index different from the remembered one
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, weights=bd.cijkScratchIndex))
        # a parent slot that is not an earlier slot
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, parents=[1] + ix["parents"][1:]))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, parents=ix["parents"][:-1] + [n]))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, parents=ix["parents"][:-1] + [-1]))
        # a post-order buffer nothing has written (the other half of an interior node's pair); indices out of range
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, posts=ix["posts"][:-1] + [bd.condLikeScratchIndex[t.root_left]]))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, posts=ix["posts"][:-1] + [10 ** 6]))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, posts=[-1] + ix["posts"][1:]))
        # a matrix index out of range
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, mats=ix["mats"][:-1] + [10 ** 6]))
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, mats=[-1] + ix["mats"][1:]))
        # NULL index arrays with count > 0; a negative count; no room for the states
        for missing in ("parents", "posts", "mats"):
            raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, dict(ix, **{missing: None}), n=n)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, ix, n=-1)
        raises(bg.BEAGLE_ERROR_OUT_OF_RANGE, ix, null_states=True)
        # no edges: NULL arrays allowed, the top alone
        rc, outs0 = call(dict(parents=None, posts=None, mats=None, weights=ix["weights"]), 0)
        assert rc == 0 and np.array_equal(outs0[0], outs[0][:P]) and np.array_equal(outs0[1], outs[1]) and outs0[2][0] == SENTINEL
        # the latest log-likelihood call had several subsets
        top = t.root_left
        two = lambda v: [v, v]
        inst.calculate_edge_log_likelihoods(two(bd.condLikeIndex[0][top]), two(bd.condLikeIndex[0][t.root]), two(bd.tiProbsIndex[0][top]),
                                            two(bd.cijkIndex[0]), two(bd.cijkIndex[0]), two(bd.siteScalerIndex[0]))
        raises(bg.BEAGLE_ERROR_NO_IMPLEMENTATION, ix)
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
            inst.sample_ancestral_states([0], [0], [0], 0, SEED)
        assert err.value.code == bg.BEAGLE_ERROR_NO_IMPLEMENTATION
        seen.append((err.value.code, lib.last_error()))
    finally:
        inst.finalize()
    return seen


def check_engines_agree(lib):
    for ncat in (2, 1):
        single, double = check_refusals(lib, ncat), check_refusals(lib, ncat, double_precision=True)
        assert len(single) == len(double) == 18
        for i, (s, d) in enumerate(zip(single, double)):
            assert s == d, (i, s, d)


def test_refusals_on_emulation(emu):
    check_engines_agree(emu)


@pytest.mark.gpu
def test_refusals(gpu):
    check_engines_agree(gpu)
