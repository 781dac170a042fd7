"""ONE mbamdSampleAncestralStates call over the whole tree (a draw of all ancestral states from their joint posterior)
next to the route that existed before it for ancestral states: the pre-order pass plus ONE mbamdCalculateNodePosteriors call with
best states only, on the same instance.  usage: ancestral_sampling_time.py [case ...] [repeats=N]
(MBAMD_LIBRARY selects the library).  A case is a name under tests/golden or kind:taxa:patterns:categories, a synthetic division;
the default is the benchmark's shape (bench_c4: DNA, 1000 taxa x 50 000 patterns, four rate categories) and the codon shape
gen61:100:5000:3.  The lines go to standard output and, with out=<file>, to that file.

Times are wall times of the synchronous calls (medians, min ... max); for the sampling call also the device time of its kernels and
its launches (mbamdKernelTiming: events around the call's launches).  The byte model is that of DESIGN 4.4.7, a buffer being
4 S bytes per (pattern, category), divided by 8 TB/s: a pre-order operation reads two buffers and writes one, the posteriors read
two per node, the sampling call ONE CATEGORY of one buffer per interior edge (1 / K of it) -- a sector-granular read moves more
where the drawn categories of neighbouring patterns differ, which is reported as the upper model (every category touched)."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from mrbayes_amd import beagle as bg, likelihood as lk
from tests.engine_checks import division_from_golden

args = [a for a in sys.argv[1:] if "=" not in a]
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
cases = args or ["bench_c4", "gen61:100:5000:3"]
repeats = int(opts.get("repeats", 10))
out = open(opts["out"], "a") if "out" in opts else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


lib = bg.BeagleLibrary()
for case in cases:
    if ":" in case:
        from mrbayes_amd.division import synthetic_division
        kind, ntaxa, npat, ncat = case.split(":")
        div = synthetic_division(kind, int(ntaxa), int(npat), seed=11, tree_seed=5, alpha=0.7, ncat=int(ncat))
    else:
        div = division_from_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"), case)
    bd = lk.BeagleDivision(div, lib, scaling=lk.MB_BEAGLE_SCALE_ALWAYS, pre_order=True)
    try:
        inst, t = bd.inst, div.tree
        lnl = bd.LogLike(0)
        bd.AcceptMove(0)
        nodes, parents, posts, mats = bd.AncestralSamplingEdges(0)
        sx = dict(parent_slots=parents, posts=posts, matrices=mats, weights_index=bd.cijkIndex[0])
        rc, states, _, counts = inst.sample_ancestral_states(seed=1, changes=True, **sx)          # (the warm-up)
        assert rc == 0 and states.min() >= 0
        inst.kernel_timing(True)
        inst.get_kernel_timing(reset=True)
        wall = []
        for i in range(repeats):
            t0 = time.perf_counter()
            inst.sample_ancestral_states(seed=2 + i, changes=True, **sx)
            wall.append((time.perf_counter() - t0) * 1e3)
        dev_ms, launches = inst.get_kernel_timing(reset=True)
        inst.kernel_timing(False)
        bd.NodePosteriors(0)                                                                     # (start vector; the warm-up)
        ops = bd.PreOrderOperations(0)
        down = list(t.all_down_pass)
        px = dict(posts=[bd.condLikeIndex[0][n] for n in down], pres=[bd.preOrderIndex[n] for n in down], weights=[bd.cijkIndex[0]] * len(down))
        inst.calculate_node_posteriors(sites=False, best=True, **px)
        pre_ms, sums_ms, best_ms = [], [], []
        inst.get_kernel_timing(reset=True)
        for i in range(repeats):
            inst.synchronize()
            t0 = time.perf_counter()
            inst.update_pre_partials(ops)
            inst.synchronize()
            t1 = time.perf_counter()
            inst.calculate_node_posteriors(sites=False, best=False, **px)
            t2 = time.perf_counter()
            inst.calculate_node_posteriors(sites=False, best=True, **px)
            t3 = time.perf_counter()
            pre_ms.append((t1 - t0) * 1e3)
            sums_ms.append((t2 - t1) * 1e3)
            best_ms.append((t3 - t2) * 1e3)
        _, old_launches = inst.get_kernel_timing(reset=True)
        S, K, P = div.nstates, div.ncat, div.npatterns
        cell = 4.0 * S * P * K
        interior = sum(1 for n in nodes[1:] if n >= t.ntaxa)
        model_old = (3 * len(ops) + 2 * len(down)) * cell / 8e12 * 1e3
        model_new, model_new_all = interior * cell / K / 8e12 * 1e3, interior * cell / 8e12 * 1e3
        med = lambda v: float(np.median(v))
        say("%s (%s): lnL %.3f; %d taxa x %d patterns x %d categories x %d states" % (case, inst.details.implName.decode(), lnl, t.ntaxa, P, K, S))
        say("  sampling call, %d edges: wall %.3f ms (%.3f ... %.3f), %.1f MiB of states (bytes) to the host; device %.3f ms a call in %d launches; "
            "byte model %.4f ms (one category column per interior edge; every category touched: %.4f ms); %.0f sampled changes, seed 1" %
            (len(parents), med(wall), min(wall), max(wall), (len(parents) + 1) * P / 2.0 ** 20, dev_ms / repeats, launches // repeats,
             model_new, model_new_all, float(counts.sum())))
        say("  pre-order pass + node posteriors, %d nodes: pre-order pass wall %.3f ms (%.3f ... %.3f), posteriors with sums only %.3f ms "
            "(%.3f ... %.3f), with best states %.3f ms (%.3f ... %.3f; %.1f MiB to the host); together %.3f ms with best states, "
            "%.3f ms with sums only; %d launches for the pass and the two calls; byte model %.4f ms" %
            (len(down), med(pre_ms), min(pre_ms), max(pre_ms), med(sums_ms), min(sums_ms), max(sums_ms), med(best_ms), min(best_ms), max(best_ms),
             len(down) * P * 12.0 / 2 ** 20, med(pre_ms) + med(best_ms), med(pre_ms) + med(sums_ms), old_launches // repeats, model_old))
    finally:
        bd.finalize()
