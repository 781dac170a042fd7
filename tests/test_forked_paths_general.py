"""Topology-move lists at 20 and 60-63 states on the two-wave path kernel (k_pathg): two root-ward paths that join run as ARMS
(buildPathG: MBAMD_P4_START / MBAMD_P4_JOIN; the finished arm waits in LDS, the sibling wave forms the join's factor from it).

  * CPU (`not gpu`): the host-emulation build of the same sources (the product's kernel bodies on fibers);
  * GPU (`gpu`): the product library on a MI355X, the small cases against the oracle, the baseline shapes against the fp64 engine,
    and the unmodified MrBayes binary (oracle/_ref/mb_amd) on short default-move-mix runs.

The A/B partner is MBAMD_NO_FORK_PATH=1: the same lists through the tree-walk scheduler and k_walkg.
"""
import os
import re

import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd.division import division_from_golden
from tests.engine_checks import REL_FP64
from tests.hostemu import build_emu

MAX_ENTRIES = 96                         # MBAMD_W4_INLINE: a path program travels in the kernel arguments
MIN_FORKING_PAIRS = 4


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


# ---- what the tree alone says about a move set ----------------------------------------------------------------------------
def _movable(t):
    return [i for i in range(len(t.anc)) if t.anc[i] != -1 and i != t.root]


def _depth(t, i):
    d = 0
    while t.anc[i] != -1 and t.anc[i] != t.root:
        i = t.anc[i]
        d += 1
    return d


def _rootward(t, node):
    """`node` and every node above it, the calculation root (a tip) included"""
    out = [node]
    while t.anc[out[-1]] != -1:
        out.append(t.anc[out[-1]])
    return out


def _dirty(t, b):
    """the interior nodes whose conditional likelihoods a change of branch `b` dirties (BeagleDivision.TouchBranch)"""
    return [p for p in _rootward(t, t.anc[b]) if p >= t.ntaxa]


def _forks(t, a, b, lists):
    """A pair forks when neither branch's parent node equals the other's or is an ancestor of it, and the list (the union of
    the two root-ward node sets) times the number of lists fits the program limit."""
    pa, pb = t.anc[a], t.anc[b]
    if pa in _rootward(t, pb) or pb in _rootward(t, pa):
        return False
    return len(set(_dirty(t, a)) | set(_dirty(t, b))) * lists <= MAX_ENTRIES


def _single_path_of_two(t, bs):
    """a set whose dirty nodes are ONE root-ward path of at least two operations (a list of one operation stays on the walk)"""
    sets = [set(_dirty(t, b)) for b in bs]
    union = set().union(*sets)
    return len(union) >= 2 and any(s == union for s in sets)


def _move_sets(t, lists, enumerate_pairs):
    """The fixed sequence: pairs (deepest and shallowest, two deep ones, seeded random pairs -- or, where a tree of few taxa
    makes forking pairs rare, four taken from the enumeration of all forking pairs), two triples, a branch with the one above it.
    -> (sets, number of pair sets)"""
    nodes = _movable(t)
    by_depth = sorted(nodes, key=lambda i: _depth(t, i))
    rng = np.random.default_rng(29)
    pairs = [(by_depth[-1], by_depth[0]), (by_depth[-1], by_depth[-3])]
    if enumerate_pairs:
        forking = [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:] if _forks(t, a, b, lists)]
        step = max(len(forking) // MIN_FORKING_PAIRS, 1)
        pairs += forking[::step][:MIN_FORKING_PAIRS]
        pairs += [tuple(int(x) for x in rng.choice(nodes, 2, replace=False)) for _ in range(2)]
    else:
        pairs += [tuple(int(x) for x in rng.choice(nodes, 2, replace=False)) for _ in range(8)]
    triples = [tuple(int(x) for x in rng.choice(nodes, 3, replace=False)) for _ in range(2)]
    last = [(by_depth[-1], t.anc[by_depth[-1]])]          # a branch and the one above it: one path
    return pairs + triples + last, len(pairs)


def plan_case(golden_dir, case, enumerate_pairs=False):
    """(sets, pair sets, forking pairs, single paths of >= 2 operations among the pairs) of a golden case: the tree alone decides"""
    div = division_from_golden(golden_dir, case)
    t, lists = div.tree, div.n_cijk_parts
    sets, npairs = _move_sets(t, lists, enumerate_pairs)
    nfork = sum(1 for a, b in sets[:npairs] if _forks(t, a, b, lists))
    nsingle = sum(1 for bs in sets[:npairs] if not _forks(t, bs[0], bs[1], lists) and _single_path_of_two(t, bs))
    return sets, npairs, nfork, nsingle


ENUMERATED = {"replicase_m3"}            # 9 taxa: few pairs fork -- four of the enumerated forking pairs instead of random draws
CASES = ["avian_wag_g4", "synth_aa_wag", "replicase_m3", "synth_codon_m3", "bench_c3", "bench_c5"]


@pytest.mark.parametrize("case", CASES)
def test_move_sequences_hold_four_forking_pairs(golden_dir, case):
    """The condition of the counter checks, from the committed trees alone: every case's sequence holds at least four pairs that
    fork within the 96-entry limit (and every pair of these cases that is not one path forks: the limit never sends one to the
    walk)."""
    div = division_from_golden(golden_dir, case)
    t, lists = div.tree, div.n_cijk_parts
    sets, npairs, nfork, nsingle = plan_case(golden_dir, case, case in ENUMERATED)
    assert nfork >= MIN_FORKING_PAIRS, (case, nfork)
    for a, b in sets[:npairs]:
        union = set(_dirty(t, a)) | set(_dirty(t, b))
        assert len(union) * lists <= MAX_ENTRIES, (case, a, b, len(union))
    assert any(len(bs) == 3 for bs in sets) and len(sets[-1]) == 2 and sets[-1][1] == t.anc[sets[-1][0]]


# ---- the check ----------------------------------------------------------------------------------------------------------
def check_forked_paths_general(lib, golden_dir, monkeypatch, case, oracle=None, fp64=False):
    """Step an engine through the case's move sets with accepts and rejects, once as it is and once with MBAMD_NO_FORK_PATH=1
    (k_walkg on the same lists): every log-likelihood and every per-site array equal bit for bit; the first four evaluations
    within REL_FP64 of the oracle (small cases) or every evaluation within REL_FP64 of the double-precision engine stepping through
    the same moves (baseline shapes); the list counters say exactly which pair sets ran as forked programs.  Both scaling schemes."""
    sets, npairs, nfork, nsingle = plan_case(golden_dir, case, case in ENUMERATED)
    assert nfork >= MIN_FORKING_PAIRS, (case, nfork)
    for scaling in (lk.MB_BEAGLE_SCALE_DYNAMIC, lk.MB_BEAGLE_SCALE_ALWAYS):
        runs, counts = [], []
        for off in (False, True):
            if off:
                monkeypatch.setenv("MBAMD_NO_FORK_PATH", "1")
            else:
                monkeypatch.delenv("MBAMD_NO_FORK_PATH", raising=False)
            div = division_from_golden(golden_dir, case)
            t = div.tree
            bd = lk.BeagleDivision(div, lib, scaling=scaling)
            f64 = lk.BeagleDivision(div, lib, scaling=scaling, double_precision=True) if (fp64 and not off) else None
            try:
                seq = [bd.LogLike(0)]
                bd.AcceptMove(0)
                if f64 is not None:
                    f64.LogLike(0)
                    f64.AcceptMove(0)
                before = bd.inst.get_list_counts()
                after = None
                for rep, bs in enumerate(sets):
                    old = [t.length[b] for b in bs]
                    for q, b in enumerate(bs):
                        t.length[b] = old[q] * (1.7 if (rep + q) % 2 else 0.6)
                        bd.TouchBranch(0, b)
                    lnl = bd.LogLike(0)
                    seq.append(lnl)
                    seq.append(bd.inst.get_site_log_likelihoods().copy())
                    if not off and oracle is not None and rep < 4:
                        want = oracle.tree_loglike(div, use_shortcuts=False)
                        print("%s scaling %d set %d: engine %.10f oracle %.10f" % (case, scaling, rep, lnl, want))
                        assert abs(lnl - want) / abs(want) < REL_FP64, (case, scaling, rep, lnl, want)
                    if f64 is not None:
                        for b in bs:
                            f64.TouchBranch(0, b)
                        want = f64.LogLike(0)
                        print("%s scaling %d set %d: engine %.10f fp64 engine %.10f" % (case, scaling, rep, lnl, want))
                        assert abs(lnl - want) <= REL_FP64 * abs(want), (case, scaling, rep, lnl, want)
                    if rep % 3 == 1:                        # reject: the branches back, the flips undone
                        for q, b in enumerate(bs):
                            t.length[b] = old[q]
                        bd.ResetFlips(0)
                        seq.append(bd.LogLike(0))
                        if f64 is not None:
                            f64.ResetFlips(0)
                            f64.LogLike(0)
                    bd.AcceptMove(0)
                    if f64 is not None:
                        f64.AcceptMove(0)
                    if rep == npairs - 1:
                        after = bd.inst.get_list_counts()
                counts.append([int(y) - int(x) for x, y in zip(before, after)])
            finally:
                bd.finalize()
                if f64 is not None:
                    f64.finalize()
            runs.append(seq)
        monkeypatch.delenv("MBAMD_NO_FORK_PATH", raising=False)
        assert len(runs[0]) == len(runs[1])
        for x, y in zip(runs[0], runs[1]):
            if isinstance(x, np.ndarray):
                assert np.array_equal(x, y), (case, scaling)
            else:
                assert x == y, (case, scaling, x, y)
        on, offc = counts                                   # over the pair sets only (a triple may fork, nest or collapse)
        print("%s scaling %d: forking pairs %d, single paths %d, counters %s / without %s" % (case, scaling, nfork, nsingle, on, offc))
        assert on[2] == nfork, (case, scaling, on, nfork)
        assert on[1] - on[2] == nsingle, (case, scaling, on, nsingle)
        assert on[3] == 0 and offc[3] == 0, (case, scaling, on, offc)
        assert offc[2] == 0, (case, scaling, offc)
        assert offc[4] == on[4] + nfork, (case, scaling, on, offc)


def test_forked_general_state_paths_on_emulation(emu, oracle, golden_dir, monkeypatch):
    """Protein (one list) and codon M3 (three lists of the same arms) on the host emulation of k_pathg."""
    for case in ("avian_wag_g4", "synth_codon_m3"):
        check_forked_paths_general(emu, golden_dir, monkeypatch, case, oracle=oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["avian_wag_g4", "synth_aa_wag", "replicase_m3", "synth_codon_m3"])
def test_forked_general_state_paths(gpu, oracle, golden_dir, monkeypatch, case):
    check_forked_paths_general(gpu, golden_dir, monkeypatch, case, oracle=oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["bench_c3", "bench_c5"])
def test_forked_general_state_paths_at_baseline_shapes(gpu, golden_dir, monkeypatch, case):
    """protein 200 x 10 000 and codon M3 100 x 5 000: hundreds of tiles x categories over every XCD, forked lists of up to 32
    operations (the factor ring wraps several times between START and JOIN), against the double-precision engine."""
    check_forked_paths_general(gpu, golden_dir, monkeypatch, case, fp64=True)


# ---- the unmodified binary ---------------------------------------------------------------------------------------------------
def _forked_count(out):
    m = re.findall(r"\[mbamd\] instance \d+: \d+-state lists \d+: root-ward paths \d+ \(of them forked (\d+)\)", out)
    assert m, out[-2000:]
    return sum(int(x) for x in m)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ntaxa,nsites,ngen", [("wag", 14, 300, 400), ("m3", 12, 120, 300)])
def test_unmodified_mrbayes_topology_moves(kind, ntaxa, nsites, ngen):
    """The reference binary linked to the product library, a short default-move-mix run (topology proposals all the time): the
    sampled parameters and trees are the same with the forked programs and with MBAMD_NO_FORK_PATH=1, and the engine's exit line
    says that forked programs ran in the first run only."""
    from mrbayes_amd import data as mbdata
    from mrbayes_amd import tree as mbtree
    from tools import refrun
    if not os.path.exists(refrun.REF_MB_AMD):
        pytest.skip("oracle/_ref/mb_amd was not built (needs the reference sources at build time)")
    st = mbdata.synthetic_states(ntaxa, nsites, {"wag": 20, "m3": 61}[kind], 11, 0.15, 0.03)
    tr = mbtree.random_tree(ntaxa, 12, brlen=0.05)
    nex = refrun.model_nexus(kind, st, tr, ngen=ngen, beagle="dynamic", fname="fk")
    nex = nex.replace("samplefreq=%d" % ngen, "samplefreq=%d" % (ngen // 10))
    runs = []
    for env in ({"MBAMD_STATS": "1"}, {"MBAMD_STATS": "1", "MBAMD_NO_FORK_PATH": "1"}):
        out, _, files = refrun.run_mb(refrun.REF_MB_AMD, nex, env=env, keep=("fk.p", "fk.t"))
        assert "Analysis completed" in out and "mbamd HIP gfx950" in out, out[-1500:]
        assert set(files) == {"fk.p", "fk.t"} and len(files["fk.p"].splitlines()) >= 10, files.keys()
        runs.append((files, _forked_count(out)))
    strip = lambda text: [l for l in text.splitlines() if not l.startswith("[ID:")]
    assert strip(runs[0][0]["fk.p"]) == strip(runs[1][0]["fk.p"])
    assert strip(runs[0][0]["fk.t"]) == strip(runs[1][0]["fk.t"])
    print("%s: forked programs %d / with MBAMD_NO_FORK_PATH=1 %d" % (kind, runs[0][1], runs[1][1]))
    assert runs[0][1] > 0 and runs[1][1] == 0, (runs[0][1], runs[1][1])
