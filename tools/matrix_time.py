"""Wall time of beagleUpdateTransitionMatrices on a real and on a complex instance (BEAGLE_FLAG_EIGEN_COMPLEX) at the
branch counts of the workloads: 4 states x 4 categories x 1998 branches, 20 x 4 x 398, 61 x 1 x 198 x 3 eigen-systems; both precisions.
usage: matrix_time.py [repeats]   (MBAMD_LIBRARY selects the library)

Both instances get the same seeded reversible eigen-system (the complex one with zero imaginary parts), so both form the same matrices:
the ratio is what the complex form of the kernels costs by itself -- the factor pair, the partner column's second load, one more
multiply-add per operand -- without the trigonometry, which zero imaginary parts skip.  A third column times the complex instance on
the `nrev` rate matrix of the same size (mrbayes_amd.model.nonreversible_q), whose eigenvalues are nearly all conjugate pairs: that one
includes sincos.  Warmed, the instances alternating, each timed window ending in a device synchronise; the median of `repeats`."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, model as mbmodel
from tests import matrix_reference as mr

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
lib = bg.BeagleLibrary()
#            states, categories, branches, eigen-systems
WORKLOADS = [(4, 4, 1998, 1), (20, 4, 398, 1), (61, 1, 198, 3)]
for double_precision in (False, True):
    pref = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
    for S, K, B, E in WORKLOADS:
        rng = np.random.default_rng(1000 * S + K)
        U, Ui, lam = mr.reversible_system(rng, S, "ordinary")
        es = mbmodel.eigen_general(mbmodel.nonreversible_q(S)[0])
        rates = mbmodel.discrete_gamma(0.7, K)
        lengths = np.exp(rng.uniform(np.log(1e-3), np.log(1.0), size=B))
        idx = [list(range(e * B, (e + 1) * B)) for e in range(E)]
        made = []
        for flags, system in ((0, (U, Ui, lam)), (bg.BEAGLE_FLAG_EIGEN_COMPLEX, (U, Ui, np.concatenate([lam, np.zeros(S)]))),
                              (bg.BEAGLE_FLAG_EIGEN_COMPLEX, (es.evec, es.ivec, es.values))):
            inst = bg.BeagleInstance(lib, 2, 3, 2, S, 64, E, E * B, K, 1, preference_flags=pref, requirement_flags=flags)
            inst.set_category_rates(rates)
            for e in range(E):
                inst.set_eigen_decomposition(e, *system)
            made.append(inst)
        try:
            def run(inst):
                for e in range(E):
                    inst.update_transition_matrices(e, idx[e], lengths)
                inst.synchronize()
            for _ in range(5):
                for inst in made:
                    run(inst)
            ms = [[], [], []]
            for _ in range(repeats):
                for n, inst in enumerate(made):
                    t0 = time.perf_counter()
                    run(inst)
                    ms[n].append((time.perf_counter() - t0) * 1e3)
            real, cplx, nrev = (float(np.median(m)) for m in ms)
            same = all(np.array_equal(made[0].get_transition_matrix(m), made[1].get_transition_matrix(m)) for m in (0, B // 2, E * B - 1))
            print("%2d states x %d categories x %4d branches x %d systems, %s: real %.4f ms, complex (the same system) %.4f ms, ratio %.3f; "
                  "complex (nrev system, %d pairs) %.4f ms, ratio %.3f; real and complex matrices %s" %
                  (S, K, B, E, "fp64" if double_precision else "fp32", real, cplx, cplx / real, int((es.imag > 0).sum()), nrev, nrev / real,
                   "bit-equal" if same else "differ in the last bits"))
        finally:
            for inst in made:
                inst.finalize()
