"""Wall time of one whole branch-length gradient -- the pre-order list of the tree plus ONE beagleCalculateEdgeDerivatives call over
all 2N-3 branches without per-site values -- at a BASELINE shape, next to the full-tree evaluation of the same run and a byte model
(DESIGN 4.4.2).  usage: gradient_time.py [case] [repeats]   (MBAMD_LIBRARY selects the library)
A case is a name under tests/golden or kind:taxa:patterns:categories, a synthetic division (gen61:100:5000:3 is the shape of the codon
workload with its three classes as rate categories: the golden codon case keeps them as three eigen-systems, which the gradient calls
do not serve).

The byte model: a pre-order operation reads two partials buffers and writes one, the derivative call reads two per branch, a
buffer is 4 S bytes per (pattern, category); divided by 8 TB/s.

A second line times ONE beagleCalculateCrossProductDerivative call over the same branches (the gradient in the rate matrix, DESIGN
4.4.3; MBAMD_XPROD_GENERIC=1 selects the plain kernel) next to the same byte model -- two partials buffers per branch -- and, from 16
states, the matrix-core flop model 2 (32 TILES)^2 x patterns x categories x branches at 157.3 TFLOP/s.

A third line times ONE mbamdCalculateEdgeSecondDerivatives call over the same branches, no per-site values (first and second
derivative of every branch; MBAMD_CURV_GENERIC=1 selects the plain kernel), ALTERNATING with the first-derivative call
of the first line: medians and the spread (min ... max) of both, the same byte model -- the curvature call reads the same two
buffers per branch -- and, from 16 states, the matrix-core flop model 2 matrices x 2 x 32 TILES x S x patterns x categories x
branches at 157.3 TFLOP/s.

A fourth line times ONE mbamdCalculateNodePosteriors call over the same (post-order, pre-order) pairs (the posterior of every state at
every node) without per-pattern outputs, ALTERNATING with the first-derivative call, against the same byte model: the
call reads the same two buffers per node and has no matrix; then with best states only, alternating with the first-derivative call
that returns its per-site values (count x patterns results cross the host link in both).

A fifth line times ONE mbamdCalculateSiteModelDerivatives call over the same branches with a unit-rate differential matrix (the
gradient in category rates, category weights and root frequencies) -- all outputs but the per-edge values, and the
rates alone --, ALTERNATING with the first-derivative call, against the same byte model: the edge part reads the same two buffers."""
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
bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, second_order=True)
try:
    inst, t = bd.inst, div.tree
    lnl = bd.LogLike(0)
    bd.AcceptMove(0)
    evals = [lk.record_evaluation(bd), lk.record_evaluation(bd)]
    for i in range(10):
        evals[i & 1].run()
    inst.synchronize()
    t0 = time.perf_counter()
    for i in range(repeats):
        evals[i & 1].run()
    inst.synchronize()
    eval_ms = (time.perf_counter() - t0) / repeats * 1e3
    grad = bd.BranchGradient(0)                  # (sets the start vector and D; warms both calls up)
    ops = bd.PreOrderOperations(0)
    nodes = list(t.all_down_pass)
    ix = dict(posts=[bd.condLikeIndex[0][n] for n in nodes], pres=[bd.preOrderIndex[n] for n in nodes],
              dmats=[bd.diffMatrixIndex] * len(nodes), weights=[bd.cijkIndex[0]] * len(nodes))
    pre_ms, read_ms = [], []
    for i in range(repeats):
        inst.synchronize()
        t0 = time.perf_counter()
        inst.update_pre_partials(ops)
        inst.synchronize()
        t1 = time.perf_counter()
        rc, _, sums, _ = inst.calculate_edge_gradient(sites=False, **ix)
        t2 = time.perf_counter()
        pre_ms.append((t1 - t0) * 1e3)
        read_ms.append((t2 - t1) * 1e3)
    assert rc == 0 and all(grad[n] == sums[i] for i, n in enumerate(nodes))
    inst.get_kernel_timing(reset=True)
    inst.update_pre_partials(ops)
    _, launches = inst.get_kernel_timing(reset=True)
    cell = 4.0 * div.nstates * div.npatterns * div.ncat
    model_pre, model_read = 3 * len(ops) * cell / 8e12 * 1e3, 2 * len(nodes) * cell / 8e12 * 1e3
    pre, read = float(np.median(pre_ms)), float(np.median(read_ms))
    print("%s (%s): lnL %.3f; full-tree evaluation %.3f ms; gradient of %d branches: pre-order pass %.3f ms in %d launches (byte model %.3f ms: %.0f %%), "
          "read-out %.3f ms (byte model %.3f ms: %.0f %%), together %.3f ms = %.1f evaluations; |gradient| max %.3f" %
          (case, inst.details.implName.decode(), lnl, eval_ms, len(nodes), pre, launches, model_pre, 100.0 * model_pre / pre, read, model_read,
           100.0 * model_read / read, pre + read, (pre + read) / eval_ms, max(abs(v) for v in grad.values())))
    lengths = [min(max(t.length[n], lk.BRLENS_MIN), lk.BRLENS_MAX) for n in nodes]
    cx = dict(posts=ix["posts"], pres=ix["pres"], rates=[0] * len(nodes), weights=ix["weights"], edge_lengths=lengths)
    rc, X = inst.calculate_cross_products(**cx)                  # (warm-up)
    inst.get_kernel_timing(reset=True)
    cross_ms = []
    for i in range(repeats):
        t0 = time.perf_counter()
        rc, X1 = inst.calculate_cross_products(**cx)
        cross_ms.append((time.perf_counter() - t0) * 1e3)
    _, launches = inst.get_kernel_timing(reset=True)
    assert rc == 0 and np.array_equal(X, X1)
    es = div.eigen[0]
    Q = (np.asarray(es.evec, dtype=np.float64) * np.asarray(es.eval, dtype=np.float64)[None, :]) @ np.asarray(es.ivec, dtype=np.float64)
    lhs, rhs = float((Q * X).sum()), sum(tl * grad[n] for n, tl in zip(nodes, lengths))
    cross = float(np.median(cross_ms))
    S = div.nstates
    tiles = 0 if S < 16 or S > 64 else (1 if S <= 32 else 2)
    flops = 2.0 * (32 * tiles) ** 2 * div.npatterns * div.ncat * len(nodes)
    model_flop = flops / 157.3e12 * 1e3
    print("%s: cross products of %d branches (%s): %.3f ms in %d launches a call (byte model %.3f ms: %.0f %%%s); sum Q X = %.6f against sum t g = %.6f" %
          (case, len(nodes), "plain kernel" if os.environ.get("MBAMD_XPROD_GENERIC") and tiles else "matrix core" if tiles else "plain kernel",
           cross, launches // repeats, model_read, 100.0 * model_read / cross,
           "; flop model %.3f ms: %.0f %%" % (model_flop, 100.0 * model_flop / cross) if tiles else "", lhs, rhs))
    curv = bd.BranchCurvature(0)                 # (sets D1 and D2; the warm-up)
    sx = dict(posts=ix["posts"], pres=ix["pres"], dmats1=ix["dmats"], dmats2=[bd.diffMatrix2Index] * len(nodes), weights=ix["weights"])
    before = inst.get_second_derivative_launches()
    first_ms, second_ms = [], []
    for i in range(repeats):
        t0 = time.perf_counter()
        rc, _, sums, _ = inst.calculate_edge_gradient(sites=False, **ix)
        t1 = time.perf_counter()
        rc2, _, _, s1, s2 = inst.calculate_edge_second_derivatives(sites=False, **sx)
        t2 = time.perf_counter()
        first_ms.append((t1 - t0) * 1e3)
        second_ms.append((t2 - t1) * 1e3)
    after = inst.get_second_derivative_launches()
    assert rc == 0 and rc2 == 0 and all(curv[n] == (s1[i], s2[i]) for i, n in enumerate(nodes))
    core = after[1] > before[1]
    assert core or all(grad[n] == s1[i] for i, n in enumerate(nodes))
    first, second = float(np.median(first_ms)), float(np.median(second_ms))
    flops = 2.0 * 2.0 * (32 * tiles) * S * div.npatterns * div.ncat * len(nodes)
    model_flop = flops / 157.3e12 * 1e3
    print("%s: first and second derivatives of %d branches (%s): %.3f ms a call (%.3f ... %.3f; byte model %.3f ms: %.0f %%%s) against "
          "the first-derivative call alternating with it %.3f ms (%.3f ... %.3f; %.0f %%); sum of d2 over the branches %.6g" %
          (case, len(nodes), "matrix core" if core else "plain kernel", second, min(second_ms), max(second_ms), model_read,
           100.0 * model_read / second, "; flop model %.3f ms: %.0f %%" % (model_flop, 100.0 * model_flop / second) if core else "",
           first, min(first_ms), max(first_ms), 100.0 * model_read / first, sum(v[1] for v in curv.values())))
    px = dict(posts=ix["posts"], pres=ix["pres"], weights=ix["weights"])
    rc, _, _, _, expect = inst.calculate_node_posteriors(sites=False, **px)            # (the warm-up)
    rc, _, _, _, _ = inst.calculate_node_posteriors(sites=False, best=True, **px)
    # (two loops: best states and their posteriors are count x patterns values that cross the host link, so their yardstick is the
    #  first-derivative call WITH its per-site values, which are as many doubles)
    first_ms, sums_ms, first2_ms, best_ms = [], [], [], []
    for i in range(repeats):
        t0 = time.perf_counter()
        rc, _, sums, _ = inst.calculate_edge_gradient(sites=False, **ix)
        t1 = time.perf_counter()
        rc2, _, _, _, psums = inst.calculate_node_posteriors(sites=False, **px)
        t2 = time.perf_counter()
        first_ms.append((t1 - t0) * 1e3)
        sums_ms.append((t2 - t1) * 1e3)
    assert rc == 0 and rc2 == 0 and np.array_equal(psums, expect)
    for i in range(repeats):
        t0 = time.perf_counter()
        rc, per, sums, _ = inst.calculate_edge_gradient(sites=True, **ix)
        t1 = time.perf_counter()
        rc2, _, states, _, psums = inst.calculate_node_posteriors(sites=False, best=True, **px)
        t2 = time.perf_counter()
        first2_ms.append((t1 - t0) * 1e3)
        best_ms.append((t2 - t1) * 1e3)
    assert rc == 0 and rc2 == 0 and np.array_equal(psums, expect)
    first, psum, first2, pbest = (float(np.median(v)) for v in (first_ms, sums_ms, first2_ms, best_ms))
    out_mib = len(nodes) * div.npatterns * 12.0 / 2 ** 20
    print("%s: node posteriors of %d nodes: sums only %.3f ms a call (%.3f ... %.3f; byte model %.3f ms: %.0f %%) against the "
          "first-derivative call alternating with it %.3f ms (%.3f ... %.3f; %.0f %%); with best states (%.1f MiB to the host) %.3f ms "
          "(%.3f ... %.3f) against the first-derivative call WITH its per-site values (%.1f MiB) alternating with it %.3f ms (%.3f ... %.3f); "
          "largest |sum over states - sum of weights| %.3g" %
          (case, len(nodes), psum, min(sums_ms), max(sums_ms), model_read, 100.0 * model_read / psum, first, min(first_ms), max(first_ms),
           100.0 * model_read / first, out_mib, pbest, min(best_ms), max(best_ms), out_mib * 2.0 / 3.0, first2, min(first2_ms), max(first2_ms),
           float(np.abs(psums.sum(1) - float(np.asarray(div.weights, dtype=np.float64).sum())).max())))
    inst.set_differential_matrix(bd.diffMatrix2Index, np.broadcast_to(Q, (div.ncat, S, S)))           # (unit rate: D_k = Q)
    mx = dict(posts=ix["posts"], pres=ix["pres"], dmats=[bd.diffMatrix2Index] * len(nodes), weights=ix["weights"], edge_lengths=lengths)
    rc, _, expect, _, _ = inst.calculate_site_model_derivatives(edges=False, **mx)                    # (the warm-up)
    inst.get_kernel_timing(reset=True)
    first_ms, model_ms, rates_ms = [], [], []
    for i in range(repeats):
        t0 = time.perf_counter()
        rc, _, sums, _ = inst.calculate_edge_gradient(sites=False, **ix)
        t1 = time.perf_counter()
        rc2, _, rates, counts, root = inst.calculate_site_model_derivatives(edges=False, **mx)
        t2 = time.perf_counter()
        rc3, _, rates1, _, _ = inst.calculate_site_model_derivatives(edges=False, counts=False, root=False, **mx)
        t3 = time.perf_counter()
        first_ms.append((t1 - t0) * 1e3)
        model_ms.append((t2 - t1) * 1e3)
        rates_ms.append((t3 - t2) * 1e3)
    _, launches = inst.get_kernel_timing(reset=True)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and np.array_equal(rates, expect) and np.array_equal(rates1, expect)
    first, model, rates_only = (float(np.median(v)) for v in (first_ms, model_ms, rates_ms))
    print("%s: site-model derivatives of %d branches x %d categories (rates, counts, root frequencies): %.3f ms a call (%.3f ... %.3f; byte "
          "model %.3f ms: %.0f %%), the rates alone %.3f ms (%.3f ... %.3f), against the first-derivative call alternating with them %.3f ms "
          "(%.3f ... %.3f): %.2f x and %.2f x; %d launches a round of the three; sum of the counts %.6f, sum pi F %.6f against %.6f sites" %
          (case, len(nodes), div.ncat, model, min(model_ms), max(model_ms), model_read, 100.0 * model_read / model, rates_only, min(rates_ms),
           max(rates_ms), first, min(first_ms), max(first_ms), model / first, rates_only / first, launches // repeats, float(counts.sum()),
           float(np.asarray(div.pi, dtype=np.float64) @ root), float(np.asarray(div.weights, dtype=np.float64).sum())))
finally:
    bd.finalize()
