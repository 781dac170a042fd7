"""Wall time of ONE mbamdCalculateInsertionLogLikelihoods call over all 2N-3 branches of a tree -- one partials subtree, one pendant
matrix, no per-site values -- ALTERNATING call by call with ONE beagleCalculateEdgeDerivatives call over the same
branches, which reads the same two buffers per branch.  usage: insertion_time.py [case] [repeats]   (MBAMD_LIBRARY selects the
library; MBAMD_INSERT_GENERIC=1 the plain kernel at 16 ... 64 states)
A case is a name under tests/golden or kind:taxa:patterns:categories, a synthetic division, as in tools/gradient_time.py: bench_c4
is DNA at 1000 taxa x 50 000 patterns x 4 categories, wag:200:10000:4 the 20-state shape.

First line: the child end of every branch (postMatrix = BEAGLE_OP_NONE).  Beyond four states a second line: a point 0.3 of the way up
every branch -- the pre-order vectors at the points written by one beagleUpdatePrePartials call into scratch buffers (timed on its
own), the lower parts of the branches as postMatrix.

The bytes a call must move: the two partials buffers of every branch, 4 S bytes per (pattern, category) each (the subtree's one
buffer is read once per run of entries and is not counted); printed divided by the call's time, for both calls."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, likelihood as lk
from tests.engine_checks import division_from_golden
case = sys.argv[1] if len(sys.argv) > 1 else "bench_c4"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
lib = bg.BeagleLibrary()
if ":" in case:
    from mrbayes_amd.division import synthetic_division
    kind, ntaxa, npat, ncat = case.split(":")
    div = synthetic_division(kind, int(ntaxa), int(npat), seed=11, tree_seed=5, alpha=0.7, ncat=int(ncat))
else:
    div = division_from_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"), case)
t = div.tree
nodes = list(t.all_down_pass)
n = len(nodes)
split = div.nstates != 4
bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, pre_order=True, spare=2 * n + 2 if split else 2)
try:
    inst = bd.inst
    lnl = bd.LogLike(0)
    bd.AcceptMove(0)
    grad = bd.BranchGradient(0)                  # (sets the start vector and D, runs the pre-order pass; warms the gradient call up)
    rng = np.random.default_rng(3)
    subtree = bd.spareBufferIndex
    inst.set_partials(subtree, rng.uniform(0.05, 1.0, size=(div.ncat, div.npatterns, div.nstates)))
    pendant = bd.tiProbsIndex[0][nodes[0]]
    gx = dict(posts=[bd.condLikeIndex[0][v] for v in nodes], pres=[bd.preOrderIndex[v] for v in nodes], dmats=[bd.diffMatrixIndex] * n,
              weights=[bd.cijkIndex[0]] * n)
    cell = 4.0 * div.nstates * div.npatterns * div.ncat
    moved = 2 * n * cell

    def timed(ix, what):
        rc, _, expect = inst.calculate_insertion_log_likelihoods(sites=False, **ix)          # (the warm-up)
        before = inst.get_insertion_launches()
        first_ms, ins_ms = [], []
        for i in range(repeats):
            t0 = time.perf_counter()
            rc, _, sums, _ = inst.calculate_edge_gradient(sites=False, **gx)
            t1 = time.perf_counter()
            rc2, _, scores = inst.calculate_insertion_log_likelihoods(sites=False, **ix)
            t2 = time.perf_counter()
            first_ms.append((t1 - t0) * 1e3)
            ins_ms.append((t2 - t1) * 1e3)
        after = inst.get_insertion_launches()
        assert rc == 0 and rc2 == 0 and np.array_equal(scores, expect) and all(grad[v] == sums[i] for i, v in enumerate(nodes))
        first, ins = float(np.median(first_ms)), float(np.median(ins_ms))
        print("%s (%s): insertion scores of %d branches, %s (%s): %.3f ms a call (%.3f ... %.3f; %.2f GB to move: %.2f TB/s) against the "
              "first-derivative call alternating with it %.3f ms (%.3f ... %.3f; %.2f TB/s): %.2f x; best score %.3f at node %d, worst %.3f" %
              (case, inst.details.implName.decode(), n, what, "matrix core" if after[1] > before[1] else "plain kernel", ins, min(ins_ms),
               max(ins_ms), moved / 1e9, moved / ins / 1e9, first, min(first_ms), max(first_ms), moved / first / 1e9, ins / first,
               float(scores.max()), nodes[int(scores.argmax())], float(scores.min())))

    ix = dict(pres=gx["pres"], posts=gx["posts"], post_matrices=[bg.BEAGLE_OP_NONE] * n, subtrees=[subtree] * n, subtree_matrices=[pendant] * n,
              subtree_scales=[bg.BEAGLE_OP_NONE] * n, weights=gx["weights"])
    timed(ix, "child end")
    if split:
        lengths = [min(max(t.length[v], lk.BRLENS_MIN), lk.BRLENS_MAX) for v in nodes]
        upper = [bd.spareMatrixIndex + i for i in range(n)]
        lower = [bd.spareMatrixIndex + n + i for i in range(n)]
        inst.update_transition_matrices(bd.cijkIndex[0], np.asarray(upper, dtype=np.int32), [0.7 * tl for tl in lengths])
        inst.update_transition_matrices(bd.cijkIndex[0], np.asarray(lower, dtype=np.int32), [0.3 * tl for tl in lengths])
        scratch = [bd.spareBufferIndex + 1 + i for i in range(n)]
        ops = []
        for i, v in enumerate(nodes):
            if v == t.root_left:
                ops.append([scratch[i], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, bd.preOrderStartIndex, upper[i], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE])
            else:
                p = t.anc[v]
                sib = t.right[p] if t.left[p] == v else t.left[p]
                ops.append([scratch[i], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, bd.preOrderIndex[p], upper[i], bd.condLikeIndex[0][sib], bd.tiProbsIndex[0][sib]])
        ops = np.asarray(ops, dtype=np.int32)
        pre_ms = []
        for i in range(max(3, repeats // 4)):
            inst.synchronize()
            t0 = time.perf_counter()
            inst.update_pre_partials(ops)
            inst.synchronize()
            pre_ms.append((time.perf_counter() - t0) * 1e3)
        print("%s: the pre-order vectors at 0.3 of every branch, one beagleUpdatePrePartials call of %d operations: %.3f ms" % (case, n, float(np.median(pre_ms))))
        timed(dict(ix, pres=scratch, post_matrices=lower), "0.3 of the way up every branch (postMatrix)")
finally:
    bd.finalize()
