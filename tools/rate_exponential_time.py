"""Wall time of mbamdUpdateTransitionMatricesFromRateMatrix beside beagleConvolveTransitionMatrices of the same counts:
61 states x 4 categories x 198 branches and 4 states x 4 categories x 1998 branches, both precisions, on ONE instance per shape.
usage: rate_exponential_time.py [repeats]             (MBAMD_LIBRARY selects the library)

Q is the `nrev` rate matrix of the size (mrbayes_amd.model.nonreversible_q), the rates a discrete gamma (0.7), the edge lengths
log-uniform in 1e-3 ... 1 (the draw of tools/matrix_time.py).  Routes, each timed window ending in a device synchronise:
    rate matrix   one call, P only                    rate matrix + P' + P''   one call with both derivative lists
    rate matrix, 64 t   the same call with every edge 64 times as long: up to six squarings more per matrix (the difference of the
                  two times over the difference of the mean squaring counts is what one squaring of every matrix costs, to set
                  against the convolve call's one product of every matrix)
    powers only   a call of ONE branch at t = 0: the powers launch and a one-workgroup launch (what every call pays first)
    convolve      one beagleConvolveTransitionMatrices call of as many entries (ONE product per matrix)
After a warm-up the routes alternate; the median of `repeats` windows and their range are printed, with the mean squaring count."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, model as mbmodel
from tests import matrix_reference as mr
from tests import rate_exponential_reference as rx


def main(repeats):
    lib = bg.BeagleLibrary()
    for S, K, B in ((61, 4, 198), (4, 4, 1998)):
        for double_precision in (False, True):
            pref = bg.BEAGLE_FLAG_PRECISION_DOUBLE if double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE
            rng = np.random.default_rng(1000 * S + K)
            Q = np.array(mbmodel.nonreversible_q(S)[0], dtype=np.float64)
            np.fill_diagonal(Q, 0.0)
            np.fill_diagonal(Q, -rx.row_sums(Q))
            mu = rx.mu_of(Q)
            rates = mbmodel.discrete_gamma(0.7, K)
            lengths = np.exp(rng.uniform(np.log(1e-3), np.log(1.0), size=B))
            squarings = [rx.reduce_argument(rx.argument(mu, r, t))[0] for t in lengths for r in rates]
            P, D1, D2, A = (np.arange(n * B, (n + 1) * B, dtype=np.int32) for n in range(4))
            inst = bg.BeagleInstance(lib, 2, 3, 2, S, 64, 1, 4 * B, K, 1, preference_flags=pref)
            try:
                inst.set_category_rates(rates)
                inst.set_eigen_decomposition(0, *mr.reversible_system(rng, S, "ordinary"))
                inst.update_transition_matrices(0, A, 0.5 * lengths)
                inst.update_transition_matrices(0, D1, 0.5 * lengths)

                def plain():
                    inst.update_transition_matrices_from_rate_matrix(Q, P, lengths)
                    inst.synchronize()

                def derivatives():
                    inst.update_transition_matrices_from_rate_matrix(Q, P, lengths, first=D1, second=D2)
                    inst.synchronize()

                def longer():
                    inst.update_transition_matrices_from_rate_matrix(Q, P, 64.0 * lengths)
                    inst.synchronize()

                def powers():
                    inst.update_transition_matrices_from_rate_matrix(Q, P[:1], [0.0])
                    inst.synchronize()

                def convolve():
                    inst.convolve_transition_matrices(A, A, D2)
                    inst.synchronize()
                routes = (("rate matrix", plain), ("rate matrix, 64 t", longer), ("rate matrix + P' + P''", derivatives), ("powers only", powers),
                          ("convolve", convolve))
                for _, call in routes:
                    for _ in range(5):
                        call()
                ms = {name: [] for name, _ in routes}
                for _ in range(repeats):
                    for name, call in routes:
                        t0 = time.perf_counter()
                        call()
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                more = [rx.reduce_argument(rx.argument(mu, r, 64.0 * t))[0] for t in lengths for r in rates]
                print("%2d states x %d categories x %4d branches, %s, mu %.3f, mean squarings %.2f (max %d; at 64 t: %.2f, max %d): %s (ms per call: median, range of %d)" %
                      (S, K, B, "fp64" if double_precision else "fp32", mu, float(np.mean(squarings)), max(squarings), float(np.mean(more)), max(more),
                       "; ".join("%s %.4f (%.4f ... %.4f)" % (name, float(np.median(v)), min(v), max(v)) for name, v in ms.items()), repeats))
            finally:
                inst.finalize()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
