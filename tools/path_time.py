"""Device time of the partial updates of branch moves (k_path4_lnl: the root-ward path and the log-likelihood in one launch) at a BASELINE
shape, through the python twin of src/mbbeagle.c.  usage: path_time.py [case] [moves] [branches]   (MBAMD_LIBRARY selects the library)
`branches` (default 1) = branches touched per move: 2 gives the lists of topology moves, two root-ward paths that join."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, likelihood as lk
from tests.engine_checks import division_from_golden
case = sys.argv[1] if len(sys.argv) > 1 else "bench_c2"
moves = int(sys.argv[2]) if len(sys.argv) > 2 else 300
branches = int(sys.argv[3]) if len(sys.argv) > 3 else 1
lib = bg.BeagleLibrary()
div = division_from_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"), case)
t = div.tree
bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_DYNAMIC)
try:
    bd.LogLike(0)
    bd.AcceptMove(0)
    bd.inst.kernel_timing(True)
    rng = np.random.default_rng(5)
    nodes = [i for i in range(len(t.anc)) if t.anc[i] != -1 and i != t.root]
    ops = 0
    t0 = time.perf_counter()
    for rep in range(moves):
        for b in ([int(rng.choice(nodes))] if branches == 1 else [int(x) for x in rng.choice(nodes, branches, replace=False)]):
            t.length[b] *= 1.1 if rep % 2 else 0.9
            bd.TouchBranch(0, b)
        bd.LogLike(0)
        bd.AcceptMove(0)
    wall = (time.perf_counter() - t0) / moves
    kms, kn = bd.inst.get_kernel_timing()
    sms, sn = bd.inst.get_step_timing()
    print("%s: %d moves of %d branch(es): partials launches %d, %.2f us each; all kernels of an evaluation %.2f us; wall per move %.1f us; lists %s" %
          (case, moves, branches, kn, kms / max(kn, 1) * 1e3, sms / max(sn, 1) * 1e3, wall * 1e6, bd.inst.get_list_counts()))
finally:
    bd.finalize()
