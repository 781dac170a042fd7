"""mbamdCalculateAutocorrelatedLogLikelihood (the site-order HMM over the rate categories) next to what a host
implementation must pay before its first addition: the read-back of q (mbamdGetCategoryPosteriors) and of the site log-likelihoods
(beagleGetSiteLogLikelihoods).  usage: autocorrelated_time.py [case ...] [repeats=N] [out=<file>]   (MBAMD_LIBRARY selects the
library).  A case is a name under tests/golden or kind:taxa:patterns:categories, a synthetic division; the default is the
benchmark's shape (bench_c4: DNA, 1000 taxa x 50 000 patterns, four rate categories) and the codon shape gen61:100:5000:3.  Every
pattern is one site, in a shuffled order, so n = the pattern count.  Both engines are measured.

Per case and engine, wall times of the synchronous calls (medians, min ... max):
    cold   one call right after a log-likelihood call (q is computed first: k_category_posteriors)
    warm   a second call with another T after the same log-likelihood call (the correlation move)
    ... with the posteriors (gamma [K][n] comes back), the launches of each, and on the single-precision engine the device time of
    the reduction's kernels (mbamdKernelTiming: events around them)
    read-back, cold / warm: mbamdGetCategoryPosteriors + beagleGetSiteLogLikelihoods after a log-likelihood call / again
The device calls are measured BEFORE the first read-back: once a client has read the site log-likelihoods the single-precision
engine writes them to pinned host memory, and the calls measured last ("sites on the host") read them from there."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, likelihood as lk
from tests.engine_checks import division_from_golden

args = [a for a in sys.argv[1:] if "=" not in a]
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
cases = args or ["bench_c4", "gen61:100:5000:3"]
repeats = int(opts.get("repeats", 20))
out = open(opts["out"], "a") if "out" in opts else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def spread(v):
    return "%.3f ms (%.3f ... %.3f)" % (float(np.median(v)), min(v), max(v))


lib = bg.BeagleLibrary()
for case in cases:
    if ":" in case:
        from mrbayes_amd.division import synthetic_division
        kind, ntaxa, npat, ncat = case.split(":")
        div = synthetic_division(kind, int(ntaxa), int(npat), seed=11, tree_seed=5, alpha=0.7, ncat=int(ncat))
    else:
        div = division_from_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"), case)
    K, P, t = div.ncat, div.npatterns, div.tree
    patterns = np.random.default_rng(1).permutation(P).astype(np.int32)
    Ts = [rho * np.eye(K) + (1.0 - rho) / K * np.ones((K, K)) for rho in (0.3, 0.6)]
    for double_precision in (False, True):
        bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, double_precision=double_precision)
        try:
            inst = bd.inst
            lnl = bd.LogLike(0)
            bd.AcceptMove(0)
            top = t.root_left
            edge = ([bd.condLikeIndex[0][top]], [bd.condLikeIndex[0][t.root]], [bd.tiProbsIndex[0][top]], [bd.cijkIndex[0]], [bd.cijkIndex[0]],
                    [bd.siteScalerIndex[0]])
            w = bd.cijkIndex[0]

            def again():
                inst.calculate_edge_log_likelihoods(*edge)
                inst.synchronize()

            def timed(f):
                t0 = time.perf_counter()
                f()
                return (time.perf_counter() - t0) * 1e3

            def device_calls(label):
                rc, lnH, _ = inst.autocorrelated_log_likelihood(w, patterns, Ts[0])                                  # (the warm-up)
                inst.autocorrelated_log_likelihood(w, patterns, Ts[0], posteriors=True)
                cold, warm, cold_g, warm_g = [], [], [], []
                for i in range(repeats):
                    again()
                    cold.append(timed(lambda: inst.autocorrelated_log_likelihood(w, patterns, Ts[0])))
                    warm.append(timed(lambda: inst.autocorrelated_log_likelihood(w, patterns, Ts[1])))
                    again()
                    cold_g.append(timed(lambda: inst.autocorrelated_log_likelihood(w, patterns, Ts[0], posteriors=True)))
                    warm_g.append(timed(lambda: inst.autocorrelated_log_likelihood(w, patterns, Ts[1], posteriors=True)))
                inst.kernel_timing(True)
                inst.get_kernel_timing(reset=True)
                for i in range(repeats):
                    inst.autocorrelated_log_likelihood(w, patterns, Ts[i & 1])
                ms, launches = inst.get_kernel_timing(reset=True)
                for i in range(repeats):
                    inst.autocorrelated_log_likelihood(w, patterns, Ts[i & 1], posteriors=True)
                ms_g, launches_g = inst.get_kernel_timing(reset=True)
                inst.kernel_timing(False)
                say("  %s: ln H %.6f (rho 0.3); cold %s, warm %s; with posteriors cold %s, warm %s" % (label, lnH, spread(cold), spread(warm), spread(cold_g), spread(warm_g)))
                say("  %s: warm call %d launches, device %.4f ms a call; with posteriors %d launches, device %.4f ms a call%s" %
                    (label, launches // repeats, ms / repeats, launches_g // repeats, ms_g / repeats,
                     " (no device timing on this engine)" if double_precision else ""))
                return float(np.median(warm))

            say("%s (%s): lnL %.3f; %d taxa x %d patterns x %d categories x %d states; n = %d sites" %
                (case, inst.details.implName.decode(), lnl, t.ntaxa, P, K, div.nstates, P))
            warm = device_calls("sites on the device")
            back_cold, back_warm = [], []
            for i in range(repeats + 1):
                again()
                a = timed(lambda: (inst.get_category_posteriors(w), inst.get_site_log_likelihoods()))
                b = timed(lambda: (inst.get_category_posteriors(w), inst.get_site_log_likelihoods()))
                if i:                                                                                                  # (the first: the warm-up)
                    back_cold.append(a)
                    back_warm.append(b)
            say("  read-back of q and the site log-likelihoods (%.2f MB): cold %s, warm %s; the warm call is %.2f x the cold read-back" %
                ((K + 1) * P * 8 / 1e6, spread(back_cold), spread(back_warm), warm / float(np.median(back_cold))))
            if not double_precision:
                device_calls("sites on the host")
        finally:
            bd.finalize()
