"""Wall time of one whole branch-length gradient -- the pre-order list of the tree plus ONE beagleCalculateEdgeDerivatives call over
all 2N-3 branches without per-site values -- at a BASELINE shape, next to the full-tree evaluation of the same run and a byte model
(DESIGN 4.4.2).  usage: gradient_time.py [case] [repeats]   (MBAMD_LIBRARY selects the library)

The byte model: a pre-order operation reads two partials buffers and writes one, the derivative call reads two per branch, a
buffer is 4 S bytes per (pattern, category); divided by 8 TB/s."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, likelihood as lk
from tests.engine_checks import division_from_golden
case = sys.argv[1] if len(sys.argv) > 1 else "bench_c4"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
lib = bg.BeagleLibrary()
div = division_from_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"), case)
bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, pre_order=True)
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
finally:
    bd.finalize()
