"""Wall time of beagleUpdateTransitionMatrices on a real and on a complex instance (BEAGLE_FLAG_EIGEN_COMPLEX) at the
branch counts of the workloads: 4 states x 4 categories x 1998 branches, 20 x 4 x 398, 61 x 1 x 198 x 3 eigen-systems; both precisions.
usage: matrix_time.py [repeats]             (MBAMD_LIBRARY selects the library)
       matrix_time.py convolve [runs]      beagleConvolveTransitionMatrices instead: see the end of this text

Both instances get the same seeded reversible eigen-system (the complex one with zero imaginary parts), so both form the same matrices:
the ratio is what the complex form of the kernels costs by itself -- the factor pair, the partner column's second load, one more
multiply-add per operand -- without the trigonometry, which zero imaginary parts skip.  A third column times the complex instance on
the `nrev` rate matrix of the same size (mrbayes_amd.model.nonreversible_q), whose eigenvalues are nearly all conjugate pairs: that one
includes sincos.  Warmed, the instances alternating, each timed window ending in a device synchronise; the median of `repeats`.

convolve: 200 results at 61 states x 4 categories and at 4 states x 4, both precisions, by three routes on ONE instance --
    convolve   one beagleConvolveTransitionMatrices call of 200 entries
    update     one beagleUpdateTransitionMatrices call of the same 200 result buffers (what an eigen-system costs for as many matrices)
    host       the route there was before: per result beagleGetTransitionMatrix twice, a host matmul, beagleSetTransitionMatrix
each timed window ending in a device synchronise.  A run is the mean of 10 windows (2 on the host route); `runs` alternating runs
(default 5) after a warm-up; the range over the runs is printed."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, model as mbmodel
from tests import matrix_reference as mr


def complex_cost(repeats):
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


def convolve_cost(runs):
    lib = bg.BeagleLibrary()
    N = 200
    for S, K in ((61, 4), (4, 4)):
        for double_precision in (False, True):
            pref = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
            rng = np.random.default_rng(1000 * S + K)
            rates = mbmodel.discrete_gamma(0.7, K)
            lengths = np.exp(rng.uniform(np.log(1e-3), np.log(1.0), size=N))
            A, B, R = (np.arange(n * N, (n + 1) * N, dtype=np.int32) for n in range(3))      # (as arrays: no list conversion in a timed call)
            inst = bg.BeagleInstance(lib, 2, 3, 2, S, 64, 1, 3 * N, K, 1, preference_flags=pref)
            try:
                inst.set_category_rates(rates)
                inst.set_eigen_decomposition(0, *mr.reversible_system(rng, S, "ordinary"))
                inst.update_transition_matrices(0, A, 0.5 * lengths)
                inst.update_transition_matrices(0, B, 0.5 * lengths)

                def convolve():
                    inst.convolve_transition_matrices(A, B, R)
                    inst.synchronize()

                def update():
                    inst.update_transition_matrices(0, R, lengths)
                    inst.synchronize()

                def host():
                    for a, b, r in zip(A, B, R):
                        inst.set_transition_matrix(r, np.matmul(inst.get_transition_matrix(a), inst.get_transition_matrix(b)))
                    inst.synchronize()
                routes = (("convolve", convolve, 10), ("update", update, 10), ("host", host, 2))
                for _, call, _ in routes:
                    for _ in range(3):
                        call()
                ms = {name: [] for name, _, _ in routes}
                for _ in range(runs):
                    for name, call, inner in routes:
                        t0 = time.perf_counter()
                        for _ in range(inner):
                            call()
                        ms[name].append((time.perf_counter() - t0) * 1e3 / inner)
                print("%2d states x %d categories x %d results, %s: %s (ms per call, range of %d alternating runs)" %
                      (S, K, N, "fp64" if double_precision else "fp32",
                       ", ".join("%s %.4f ... %.4f" % (name, min(v), max(v)) for name, v in ms.items()), runs))
            finally:
                inst.finalize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "convolve":
        convolve_cost(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        complex_cost(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
