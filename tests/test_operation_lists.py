"""Random operation lists (tests/list_generator.py) on every back end of both engines: what decides WHICH kernel runs on WHICH operations
and in what order -- Instance::buildWalk's hazard segments and template cache, recognisePath / pathPlan, the level scheduler, Walk4Unstored,
the plan cache, the queue of the general-state walk, Engine64::tryWalk4 and the fp64 level and chain kernels.

  * CPU (`not gpu`): the host-emulation build of the same sources -- the compiler's SEMANTICS (the emulation runs the blocks of a launch one
    after the other: a missing dependency inside a launch cannot show there);
  * GPU (`gpu`): the product library on a MI355X -- the only place the ORDERING decisions inside a launch can be caught.

Every case runs on two instances of one configuration, which serve all seeds of a test (sources are set again per case: the template and plan
caches carry over from case to case):

  (a) AS ISSUED against ONE CALL PER OPERATION with a read of its destination after each: every partials buffer the case writes, every
      exponent buffer it writes and both cumulative buffers equal bit for bit, NaN nowhere (check_hazard_lists' invariant, generalised).
      No pair of kernels had to be moved from bit-equality to the bound: nothing in the code documents two kernels that may serve the same
      operation as summing in a different order, and none was met.
  (b) the per-operation run against the long-double interpreter below, so that both runs cannot be wrong alike: per buffer the exact
      value U and the integer exponents E the engine reported along the way (E[dst] = E[c1] + E[c2] + e, e what the operation wrote or
      read), |got 2^E - U| <= ((1 + B_op)^m - 1) U per element with B_op = (2 S + 4) u of tests/test_operation_bounds.py and m the
      operations below the destination (with multiplicity: a result read twice counts twice).  The interpreter holds U = W 2^G with
      W's column maxima in [0.5, 1) -- exact powers of two --, so that twenty-four squarings stay inside the long double's range.  For
      every SCALE_WRITE the engine's own output: live column maxima in [0.5, 1) -- per (category, pattern) on the arena layouts, per
      pattern elsewhere --, dead columns zero with exponent 0; the cumulative buffers equal the sums of the written exponents.

On a failure the case is printed (family, variant, seed, shape, switches, the calls as literals, the first differing buffer and element),
then shortened greedily from the end of its last call while it still fails, and printed again.

Shapes (states, categories, patterns) and the back ends each can reach, read from the eligibility rules in the code:
  fp32 (4, 4, 130) (4, 1, 64) (4, 9, 70)   "4-state tree-walk kernels": every list is compiled by buildPath4 (recognisePath; any list of
        1 ... 96 operations that is a root-ward path, forked or not: `paths`, `forked paths` of get_list_counts) or buildWalk (`tree
        walks`).  Programs of at most 96 entries travel in the kernel arguments and run on the generic instantiation (get_walk_counts[1]);
        the plain instantiation (get_walk_counts[0]) needs a program in a device buffer (several segments, or MBAMD_NO_INLINE_PROGRAMS)
        whose children are compact tips or results of the list, with no SCALE_READ; several plain waves and unstored subtrees need it to be
        ONE segment -- the first call of `small_subtrees` under MBAMD_NO_INLINE_PROGRAMS (the UNSTORED_TIPS and PLAIN_WAVES
        configurations).  K = 9: paths are not held for a fused likelihood.
  fp32 (2, 2, 40) (8, 3, 40) (40, 2, 40)   "general-state tree-walk kernels": every call is queued (updatePartialsG) and flushed by the next
        call that depends on it, up to four lists per flush; k_walkg on buildWalk's segments (`tree walks`); no path kernel.
        40 states: the bf16 pieces -- a flush that reads a buffer no rescaling operation wrote runs range-safe (get_range_safe_counts[0]).
  fp32 (20, 4, 70) (61, 1, 33)             the same, and k_pathg for a flush that is ONE list of >= 2 operations recognisePath accepts
        (`paths`, `forked paths`); 61 states: range-safe flushes as at 40.
  fp32 (12, 2, 40)   "general-state MFMA", (33, 3, 33) "general-state vector kernels": the level scheduler (dependency levels, narrow lists,
        chains, spine chains, deferral between queued lists); the library reports no counter for them: the layout name is asserted.
  fp64 (4, 4, 130) (4, 3, 65)   Engine64::tryWalk4 takes a flush of >= 2 operations with one cumulative index and no hazard as ONE launch
        (f64_launches); anything else one launch per dependency level.  (4, 9, 70): K > 8, always the levels.
  fp64 (20, 2, 40)   the chain kernel serves a root-ward path as one launch (f64_chain_kernel_serves); (20, 5, 33), (61, 3, 40): levels only.
Switch variants: MBAMD_FORCE_GENERIC at (4, 4, 130) (vector level kernels), MBAMD_NO_WALKG at (20, 4, 70) (MFMA levels), MBAMD_NO_MFMA at
(12, 2, 40) (vector levels), F64_GENERAL_SWITCHES at (20, 2, 40) fp64 (no chain kernel: a path is a launch per operation), MBAMD_F64_NO_WALK at
(4, 4, 130) fp64 (levels), MBAMD_UNSTORED_TIPS = 0, 2, 4 with MBAMD_NO_INLINE_PROGRAMS at (4, 4, 130), MBAMD_SHARD=2 at (4, 4, 130) (two child
engines: the parent reports no counters), MBAMD_WALK_WAVES=2 with the small-list switches of tests/test_walk4_plain_waves.py at (4, 4, 130).

What a test asserts of the counters, per (configuration, family) after its seeds (printed: pytest -s): see check_reached.

Worst error / bound of oracle (b) per shape, measured over every family -- the host emulation at seeds 0 ... 19 / the MI355X at seeds
0 ... 7 where it was printed (fewer seeds: smaller or equal, but for the bf16 pieces at 40 and 61 states, whose emulated rounding differs):
  fp32  (4, 4, 130) 0.355 / 0.355 (every switch variant of the tree-walk layout the same; MBAMD_FORCE_GENERIC 0.384)   (4, 1, 64) 0.358 / 0.298
        (4, 9, 70) 0.399 / 0.365   (2, 2, 40) 0.410 / 0.339   (8, 3, 40) 0.291 / 0.272   (20, 4, 70) 0.210 / 0.210 (MBAMD_NO_WALKG 0.227)
        (40, 2, 40) 0.091 / 0.128   (61, 1, 33) 0.060 / 0.075   (12, 2, 40) 0.237 / 0.232 (MBAMD_NO_MFMA 0.237)   (33, 3, 33) 0.199 / 0.169
  fp64  (4, 4, 130) 0.406 / 0.358 (MBAMD_F64_NO_WALK 0.406)   (4, 3, 65) 0.387 / 0.309   (4, 9, 70) 0.469   (20, 2, 40) 0.173 (F64_GENERAL_SWITCHES
        0.173)   (20, 5, 33) 0.219   (61, 3, 40) 0.146
"""
import numpy as np
import pytest

from mrbayes_amd import beagle as bg
from tests import list_generator as lg
from tests.engine_checks import F64_GENERAL_SWITCHES
from tests.hostemu import build_emu
from tests.operation_reference import Reference, dense_tip
from tests.test_operation_bounds import expected_layout, f64_chain_kernel_serves, f64_launches, operation_bound, preference, stored
from tests.test_walk4_plain_waves import SMALL, WAVES

NONE = lg.NONE
LAYOUT = lg.LAYOUT
REF = Reference()
EMU_SEEDS, GPU_SEEDS = 20, 8


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


# ---- configurations ------------------------------------------------------------------------------------------------------------------
class Config:
    def __init__(self, S, K, P, dbl=False, env=(), name=None):
        self.S, self.K, self.P, self.dbl, self.env = S, K, P, dbl, dict(env)
        self.id = "%s-%dx%dx%d%s" % ("fp64" if dbl else "fp32", S, K, P, ("-" + name) if name else "")
        self.layout = expected_layout(S, K, dbl, force_generic="MBAMD_FORCE_GENERIC" in self.env, no_walkg="MBAMD_NO_WALKG" in self.env,
                                      no_mfma="MBAMD_NO_MFMA" in self.env)
        self.per_category = (not dbl) and "tree-walk" in self.layout
        self.walk4 = self.layout == "4-state tree-walk kernels"
        # a missing tip state: the 4-state single-precision kernels take the tip as the dense vector of ones (the sum of the matrix row),
        # every other kernel as the factor 1 (tests/engine_checks.py::check_single_operations, tests/test_operation_bounds.py::check_tree)
        self.missing_is_one = not self.walk4
        self.walkg = self.layout == "general-state tree-walk kernels"
        self.sharded = "MBAMD_SHARD" in self.env
        self.paths = (self.walk4 or (self.walkg and (S == 20 or 60 <= S <= 63))) and not self.sharded
        self.device_programs = self.walk4 and "MBAMD_NO_INLINE_PROGRAMS" in self.env
        # (Walk4Unstored clamps MBAMD_UNSTORED_TIPS to 2 ... 4: 0 leaves tip pairs unstored, as 2 does)
        self.unstored_tips = min(4, max(2, int(self.env.get("MBAMD_UNSTORED_TIPS", "4")))) if self.device_programs else 0


NO_INLINE = {"MBAMD_NO_INLINE_PROGRAMS": "1"}
CONFIGS = [Config(4, 4, 130), Config(4, 1, 64), Config(4, 9, 70),
           Config(2, 2, 40), Config(8, 3, 40), Config(20, 4, 70), Config(40, 2, 40), Config(61, 1, 33),
           Config(12, 2, 40), Config(33, 3, 33),
           Config(4, 4, 130, True), Config(4, 3, 65, True), Config(4, 9, 70, True), Config(20, 2, 40, True), Config(20, 5, 33, True),
           Config(61, 3, 40, True),
           Config(4, 4, 130, env={"MBAMD_FORCE_GENERIC": "1"}, name="FORCE_GENERIC"),
           Config(20, 4, 70, env={"MBAMD_NO_WALKG": "1"}, name="NO_WALKG"),
           Config(12, 2, 40, env={"MBAMD_NO_MFMA": "1"}, name="NO_MFMA"),
           Config(20, 2, 40, True, env={k: "1" for k in F64_GENERAL_SWITCHES}, name="F64_GENERAL"),
           Config(4, 4, 130, True, env={"MBAMD_F64_NO_WALK": "1"}, name="F64_NO_WALK"),
           Config(4, 4, 130, env=dict(NO_INLINE, MBAMD_UNSTORED_TIPS="0"), name="UNSTORED_TIPS_0"),
           Config(4, 4, 130, env=dict(NO_INLINE, MBAMD_UNSTORED_TIPS="2"), name="UNSTORED_TIPS_2"),
           Config(4, 4, 130, env=dict(NO_INLINE, MBAMD_UNSTORED_TIPS="4"), name="UNSTORED_TIPS_4"),
           Config(4, 4, 130, env={"MBAMD_SHARD": "2"}, name="SHARD_2"),
           Config(4, 4, 130, env=dict(SMALL, **{WAVES: "2"}), name="PLAIN_WAVES_2")]
CONFIG_IDS = [c.id for c in CONFIGS]


def make_instance(lib, cfg, monkeypatch):
    """(an instance reads the switches when it is created)"""
    for k, v in cfg.env.items():
        monkeypatch.setenv(k, v)
    try:
        inst = bg.BeagleInstance(lib, LAYOUT.TIPS, LAYOUT.N_BUFFERS - len(LAYOUT.COMPACT), len(LAYOUT.COMPACT), cfg.S, cfg.P, 1,
                                 LAYOUT.N_MATRICES, cfg.K, LAYOUT.N_SCALES, preference_flags=preference(cfg.dbl))
    finally:
        for k in cfg.env:
            monkeypatch.delenv(k, raising=False)
    name = inst.details.implName.decode()
    assert cfg.layout in name, name
    if cfg.sharded:
        assert inst.child_count() == 2
    return inst


# ---- running a case ------------------------------------------------------------------------------------------------------------------
def seed_sources(inst, case):
    for m, a in enumerate(case.matrices):
        inst.set_transition_matrix(m, a)
    for t, st in zip(LAYOUT.COMPACT, case.tips):
        inst.set_tip_states(t, st)
    inst.set_tip_partials(LAYOUT.TIP_PARTIALS, case.tip_partials)
    for b, a in case.dense.items():
        inst.set_partials(b, a)
    for c in LAYOUT.CUMULATIVE:
        inst.reset_scale_factors(c)


def apply_pre(inst, call):
    for what, idx, a in call.pre:
        if what == "matrix":
            inst.set_transition_matrix(idx, a)
        else:
            inst.set_tip_states(idx, a)


def read_out(inst, case):
    out = [("partials %d" % b, inst.get_partials(b)) for b in case.read_buffers]
    out += [("exponents %d" % s, inst.get_scale_exponents(s)) for s in case.read_scales]
    out += [("cumulative %d" % c, inst.get_scale_exponents(c)) for c in LAYOUT.CUMULATIVE]
    return out


def counters(inst, cfg):
    if cfg.dbl:
        return {}
    return {"lists": inst.get_list_counts(), "walks": inst.get_walk_counts(), "waves": inst.get_plain_wave_counts(),
            "pairs": inst.get_recompute_counts(), "subtrees": inst.get_subtree_recompute_counts(), "range_safe": inst.get_range_safe_counts()}


def _launches(inst, cfg, stats):
    """fp64: the partials launches since the last look, added to the configuration's total"""
    n = f64_launches(inst) if cfg.dbl else 0
    if stats is not None:
        stats["f64_total"] += n
    return n


def run_as_issued(inst, cfg, case, stats):
    seed_sources(inst, case)
    _launches(inst, cfg, None)
    last = None
    for call in case.calls:
        apply_pre(inst, call)
        if call.flush and last is not None:
            inst.get_partials(last)
        measured = call.expect is not None and stats is not None
        if measured:
            before = _launches(inst, cfg, stats) if cfg.dbl else inst.get_list_counts()
        inst.update_partials(call.ops, call.cum)
        last = int(call.ops[-1][0])
        if measured:
            inst.get_partials(last)
            if cfg.dbl:
                stats["launches"].append((call.expect, len(call.ops), _launches(inst, cfg, stats)))
            else:
                after = inst.get_list_counts()
                stats["expect"].append((call.expect, tuple(int(y) - int(x) for x, y in zip(before, after))))
    out = read_out(inst, case)
    _launches(inst, cfg, stats)
    return out


def run_per_operation(inst, case):
    """-> (what read_out gives, [(row, destination as read, exponents written or read or None)])"""
    seed_sources(inst, case)
    trace = []
    for call in case.calls:
        apply_pre(inst, call)
        for row in call.ops:
            inst.update_partials(row[None, :], call.cum)
            got = inst.get_partials(int(row[0]))
            s = int(row[1]) if row[1] != NONE else int(row[2])
            trace.append((call, row, got, inst.get_scale_exponents(s).astype(np.int64) if s != NONE else None))
    return read_out(inst, case), trace


# ---- oracle (b): the long-double interpreter -----------------------------------------------------------------------------------------
def _shift(wide, e):
    """wide x 2^e per (category, pattern) column, exactly"""
    e = np.broadcast_to(np.asarray(e)[:, :, None], wide.shape)
    if not REF.exact:
        return np.ldexp(wide, e.astype(np.int32))
    import fractions
    out = wide.copy()
    flat, ef = out.reshape(-1), e.reshape(-1)
    for n in range(flat.size):
        flat[n] = flat[n] * fractions.Fraction(2) ** int(ef[n])
    return out


def interpret(cfg, case, trace, cumulative):
    """hold the per-operation run to the bounds; -> worst error / bound"""
    S, K, P = cfg.S, cfg.K, cfg.P
    B = operation_bound(S, cfg.dbl)
    zero = np.zeros((K, P), dtype=np.int64)
    W = {b: REF.widen(dense_tip(case.tips[b], S, K)) for b in LAYOUT.COMPACT}
    W[LAYOUT.TIP_PARTIALS] = REF.widen(np.broadcast_to(case.tip_partials, (K, P, S)))
    W.update({b: REF.widen(a) for b, a in case.dense.items()})
    G = {b: zero for b in W}
    E = {b: zero for b in W}
    count = {b: 0 for b in W}
    states = {b: case.tips[b] for b in LAYOUT.COMPACT}

    def factor(m, c):
        f = REF.contract(M[m], W[c])
        if cfg.missing_is_one and c in states:
            f[:, states[c] >= S, :] = REF.widen(1.0)
        return f
    M = [REF.widen(m) for m in case.matrices]
    want_cum = {c: zero.copy() for c in LAYOUT.CUMULATIVE}
    worst, applied = 0.0, set()
    for n, (call, row, got, e) in enumerate(trace):
        if id(call) not in applied:
            applied.add(id(call))
            for what, idx, a in call.pre:
                if what == "matrix":
                    M[idx] = REF.widen(a)
                else:
                    W[idx], G[idx], E[idx], count[idx], states[idx] = REF.widen(dense_tip(a, S, K)), zero, zero, 0, a
        d, sw, sr, c1, m1, c2, m2 = (int(x) for x in row)
        where = "operation %d %s" % (n, row.tolist())
        assert np.isfinite(got).all(), where
        raw = factor(m1, c1) * factor(m2, c2)
        col = REF.to_float(raw.max(axis=2))
        g = np.where(col > 0, np.frexp(col)[1], 0).astype(np.int64)
        w_new, g_new = _shift(raw, -g), G[c1] + G[c2] + g
        e_new = E[c1] + E[c2] + (e if e is not None else 0)
        m_new = count[c1] + count[c2] + 1
        W[d], G[d], E[d], count[d] = w_new, g_new, e_new, m_new
        ratio = _rel(_shift(REF.widen(got), e_new - g_new), w_new) / ((1.0 + B) ** m_new - 1.0)
        bad = np.argwhere(~(ratio <= 1.0))
        assert bad.size == 0, "%s: error / bound %.3f at element %s (m = %d)" % (where, float(ratio[tuple(bad[0])]), bad[0].tolist(), m_new)
        worst = max(worst, float(ratio.max()))
        if sw != NONE:
            dead = col == 0
            mx = got.max(axis=2) if cfg.per_category else np.broadcast_to(got.max(axis=(0, 2)), (K, P))
            ref_live = ~dead if cfg.per_category else np.broadcast_to((col > 0).any(axis=0), (K, P))
            assert np.all((mx[ref_live] >= 0.5) & (mx[ref_live] < 1.0)), "%s: a live column maximum outside [0.5, 1)" % where
            assert np.all(e[~ref_live] == 0) and np.all(got[dead] == 0), "%s: a dead column" % where
            if call.cum != NONE:
                want_cum[call.cum] = want_cum[call.cum] + e
    for c in LAYOUT.CUMULATIVE:
        assert np.array_equal(cumulative[c], want_cum[c]), "cumulative buffer %d is not the sum of the written exponents" % c
    return worst


def _rel(got_wide, want):
    """|got - want| / want per element as float64; 0 where both are zero, inf where only the reference is"""
    d = np.abs(got_wide - want)
    out = np.zeros(np.shape(want))
    nz = np.asarray(want != 0, dtype=bool)
    if nz.any():
        out[nz] = REF.to_float(d[nz] / want[nz])
    out[~nz & np.asarray(got_wide != 0, dtype=bool)] = np.inf
    return out


# ---- one case, both oracles ----------------------------------------------------------------------------------------------------------
def check_case(pair, cfg, case, stats):
    issued, split = pair
    one = run_as_issued(issued, cfg, case, stats)
    many, trace = run_per_operation(split, case)
    for (name, a), (_, b) in zip(one, many):
        assert np.isfinite(a).all() and np.isfinite(b).all(), "%s holds a NaN" % name
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)[0].tolist()
            raise AssertionError("%s differs between the calls as issued and one call per operation, first at %s: %r / %r (%d elements)" %
                                 (name, at, a[tuple(at)], b[tuple(at)], int((a != b).sum())))
    cum = {c: dict(many)["cumulative %d" % c] for c in LAYOUT.CUMULATIVE}
    worst = interpret(cfg, case, trace, cum)
    if stats is not None:
        stats["worst"] = max(stats["worst"], worst)
    return worst


def check_case_reporting(pair, cfg, case, stats):
    try:
        return check_case(pair, cfg, case, stats)
    except Exception as err:
        print("\nFAILED %s, switches %s: %s\n%s" % (cfg.id, cfg.env, err, case.describe()))
        if isinstance(err, AssertionError):
            short = case
            while True:
                nxt = short.shortened()
                if nxt is None:
                    break
                try:
                    check_case(pair, cfg, nxt, None)
                    break
                except AssertionError:
                    short = nxt
            if short is not case:
                print("shortened to %d operations, still failing:\n%s" % (short.total_operations(), short.describe()))
        raise


def check_reached(cfg, family, stats, before, after, f64_issued, cases):
    """What the seed set of (configuration, family) must have reached -- a random test that silently runs on other kernels tests nothing:
      * every call the generator marks: "path" / "forked" counted as a (forked) root-ward path and no tree walk where the layout has a
        path kernel (cfg.paths); "not_path" -- the near misses -- counted as NO path and as a tree walk on every arena layout; fp64:
        a marked call is one launch where the walk (4 states, K <= 8) or the chain kernel ("path" where f64_chain_kernel_serves) takes it
        and more than one under MBAMD_F64_NO_WALK / without the chain kernel;
      * the arena layouts: tree walks > 0 in every family; 4 states: the generic instantiation > 0, and with device-buffer programs in
        `small_subtrees` the plain one > 0, buffers left unstored > 0 and materialised > 0 as MBAMD_UNSTORED_TIPS allows (0 and 2 --
        the engine clamps the value to 2 ... 4 --: tip pairs only; 4: subtrees of three and four tips too), W > 1 where
        MBAMD_WALK_WAVES forces it;
      * 40 and 61 states: range-safe flushes > 0;
      * fp64: fewer launches than operations where the walk serves (whole lists as one launch), at least one per call elsewhere."""
    d = {k: tuple(int(y) - int(x) for x, y in zip(before[k], after[k])) for k in before}
    print("%s %-14s counters %s fp64 launches (as issued) %s; marked calls %s; worst error / bound %.3f; redrawn %d of %d draws" %
          (cfg.id, family, d, f64_issued, stats["expect"] or stats["launches"], stats["worst"], sum(c.redraws for c in cases),
           sum(c.draws for c in cases)))
    if family in ("path", "forked"):
        marks = {c.calls[-1].expect for c in cases}
        assert "not_path" in marks and (("path" if family == "path" else "forked") in marks), marks
    for expect, delta in stats["expect"]:
        if cfg.sharded or not (cfg.walk4 or cfg.walkg):
            assert not any(delta), (expect, delta)              # (no counters on these layouts)
        elif cfg.paths and expect != "not_path":
            assert delta[0] == 1 and delta[1] == 1 and delta[2] == (1 if expect == "forked" else 0) and delta[4] == 0, (expect, delta)
        else:
            assert delta[0] == 1 and delta[1] == 0 and delta[2] == 0 and delta[4] == 1, (expect, delta)
    for expect, n, launches in stats["launches"]:
        walk = cfg.S == 4 and cfg.K <= 8 and "MBAMD_F64_NO_WALK" not in cfg.env
        chain = expect == "path" and f64_chain_kernel_serves(cfg.S, cfg.K) and "MBAMD_F64_NO_CHAIN" not in cfg.env
        if (walk and (expect != "not_path" or family == "forked")) or chain:
            assert launches == 1, (expect, n, launches)          # ("two_saved" is a tree without a hazard: the walk takes it)
        elif family == "path":
            # (a chain, hazard or not: a level per operation -- unless the chain kernel, which walks a chain in list order, takes a near miss)
            served = expect == "not_path" and f64_chain_kernel_serves(cfg.S, cfg.K) and "MBAMD_F64_NO_CHAIN" not in cfg.env
            assert launches == n or (served and launches == 1), (expect, n, launches)
        else:
            assert 1 < launches <= n, (expect, n, launches)
    if cfg.dbl:
        nops, ncalls = sum(c.total_operations() for c in cases), sum(len(c.calls) for c in cases)
        if cfg.S == 4 and cfg.K <= 8 and "MBAMD_F64_NO_WALK" not in cfg.env and family != "hazard":
            assert f64_issued < nops, (f64_issued, nops)
        else:
            assert f64_issued >= ncalls, (f64_issued, ncalls)
        return
    if cfg.sharded or not (cfg.walk4 or cfg.walkg):
        return
    assert d["lists"][0] > 0 and d["lists"][4] > 0 and d["lists"][5] >= d["lists"][4], d
    if cfg.walk4:
        assert d["walks"][1] > 0 or cfg.device_programs, d
        if family == "small_subtrees" and cfg.device_programs:
            assert d["walks"][0] > 0, d
            if WAVES in cfg.env:
                assert sum(d["waves"][1:]) > 0, d
            T = cfg.unstored_tips
            assert (d["pairs"][0] > 0 and d["pairs"][1] > 0) == (T >= 2), (T, d)
            assert (d["subtrees"][0] > 0 and d["subtrees"][1] > 0) == (T >= 3), (T, d)
    if cfg.walkg and (cfg.S == 40 or 60 <= cfg.S <= 63):
        assert d["range_safe"][0] > 0, d


def check_family(lib, monkeypatch, cfg, family, seeds):
    pair = (make_instance(lib, cfg, monkeypatch), make_instance(lib, cfg, monkeypatch))
    try:
        stats = {"expect": [], "launches": [], "worst": 0.0, "f64_total": 0}
        before = counters(pair[0], cfg)
        cases = []
        for seed in range(seeds):
            case = lg.make_case(family, seed, cfg.S, cfg.K, cfg.P, cfg.dbl, cfg.per_category, cfg.missing_is_one)
            cases.append(case)
            check_case_reporting(pair, cfg, case, stats)
        check_reached(cfg, family, stats, before, counters(pair[0], cfg), stats["f64_total"], cases)
        return stats["worst"]
    finally:
        for inst in pair:
            inst.finalize()


@pytest.mark.parametrize("family", lg.FAMILIES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_operation_lists_on_emulation(emu, monkeypatch, cfg, family):
    check_family(emu, monkeypatch, cfg, family, EMU_SEEDS)


@pytest.mark.gpu
@pytest.mark.parametrize("family", lg.FAMILIES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_operation_lists(gpu, monkeypatch, cfg, family):
    check_family(gpu, monkeypatch, cfg, family, GPU_SEEDS)


# ---- found by the lists above: kept as named cases ---------------------------------------------------------------------------------------
# The serial MFMA kernels (k_partials_mfma_spine / _serial: narrow lists and the spine of a level-launched list) fetch an operation's
# operands, the exponents of a SCALE_READ among them, while the operation before it computes; a list whose SCALE_READ named the buffer
# an operation just before it wrote divided by what the buffer held BEFORE the list (tree seed 3 at 20 x 4 x 70 under MBAMD_NO_WALKG,
# shortened to the first list below; off by 2^34 there).  buildGeneric now keeps such lists off the serial kernels.
SERIAL_EXPONENT_LISTS = [[[12, 42, NONE, 6, 2, 7, 5], [19, NONE, 42, 12, 1, 8, 7]],                                     # the reader next to the writer
                         [[12, 42, NONE, 6, 2, 7, 5], [13, NONE, NONE, 12, 3, 8, 0], [19, NONE, 42, 13, 1, 6, 7]],      # ... one operation later
                         [[12, 42, NONE, 6, 2, 7, 5], [13, 41, NONE, 12, 3, 8, 0], [14, NONE, NONE, 13, 4, 0, 1],
                          [19, NONE, 42, 14, 1, 6, 7], [20, NONE, 41, 19, 0, 1, 6]]]
SERIAL_CONFIGS = [c for c in CONFIGS if c.id in ("fp32-20x4x70-NO_WALKG", "fp32-12x2x40", "fp32-61x1x33", "fp64-20x2x40")]


def check_serial_exponents(lib, monkeypatch, cfg):
    pair = (make_instance(lib, cfg, monkeypatch), make_instance(lib, cfg, monkeypatch))
    try:
        for rows in SERIAL_EXPONENT_LISTS:
            for cum in (NONE, LAYOUT.CUMULATIVE[1]):
                case = lg.make_case("tree", 3, cfg.S, cfg.K, cfg.P, cfg.dbl, cfg.per_category, cfg.missing_is_one)
                case.calls = [lg.Call(rows, cum)]
                case.read_buffers = sorted({r[0] for r in rows})
                case.read_scales = sorted({r[1] for r in rows if r[1] != NONE})
                check_case_reporting(pair, cfg, case, None)
    finally:
        for inst in pair:
            inst.finalize()


@pytest.mark.parametrize("cfg", SERIAL_CONFIGS, ids=[c.id for c in SERIAL_CONFIGS])
def test_exponents_written_and_read_in_one_serial_launch_on_emulation(emu, monkeypatch, cfg):
    check_serial_exponents(emu, monkeypatch, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SERIAL_CONFIGS, ids=[c.id for c in SERIAL_CONFIGS])
def test_exponents_written_and_read_in_one_serial_launch(gpu, monkeypatch, cfg):
    check_serial_exponents(gpu, monkeypatch, cfg)


# ---- the generator itself --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (a.describe() == b.describe() and all(np.array_equal(x, y) for x, y in zip(a.tips + a.matrices + [a.tip_partials], b.tips + b.matrices + [b.tip_partials]))
            and all(np.array_equal(a.dense[k], b.dense[k]) for k in a.dense)
            and all(np.array_equal(x[2], y[2]) for p, q in zip(a.calls, b.calls) for x, y in zip(p.pre, q.pre)))


def test_generator_is_deterministic():
    for family in lg.FAMILIES:
        a, b = (lg.make_case(family, 7, 8, 3, 40, False, True) for _ in (0, 1))
        assert _same(a, b), family
        assert not _same(a, lg.make_case(family, 8, 8, 3, 40, False, True)), family


def test_generated_cases_are_what_the_families_say():
    """every row names buffers of the layout, a SCALE_READ names an exponent buffer written earlier in the case, no list is longer than
    24 operations, sources are stored values; over its seeds the hazard family holds all five hazards, the marked families their near
    misses, small_subtrees and queued every variant"""
    for family in lg.FAMILIES:
        hazards, variants = set(), set()
        for seed in range(EMU_SEEDS):
            c = lg.make_case(family, seed, 4, 4, 130, False, True)
            written = set()
            for call in c.calls:
                assert 1 <= len(call.ops) <= 24 and call.cum in (NONE,) + LAYOUT.CUMULATIVE
                for d, sw, sr, c1, m1, c2, m2 in call.ops.tolist():
                    assert LAYOUT.FIRST_RESULT <= d < LAYOUT.N_BUFFERS and d not in (c1, c2) and 0 <= c1 < LAYOUT.N_BUFFERS and 0 <= c2 < LAYOUT.N_BUFFERS
                    assert 0 <= m1 < LAYOUT.N_MATRICES and 0 <= m2 < LAYOUT.N_MATRICES
                    assert sw == NONE or sr == NONE
                    assert sr == NONE or sr in written
                    assert sw == NONE or 0 <= sw < LAYOUT.N_NODE_SCALES
                    written.add(sw)
            for a in [c.tip_partials] + list(c.dense.values()) + c.matrices:
                assert np.array_equal(a, stored(a, False))
            assert np.all(c.dense[LAYOUT.DEAD_SOURCE][:, LAYOUT.DEAD_PATTERN, :] == 0)
            hazards |= c.hazards
            variants |= set(c.variant.split(","))
        if family == "hazard":
            assert hazards == {"waw", "war", "scale_ww", "scale_wr", "scale_rw"}, hazards
        if family == "path":
            assert variants == {"ok", "outside_written_later", "scale_twice"}, variants
        if family == "forked":
            assert variants == {"two_arms", "three_arms", "two_saved"}, variants
        if family == "small_subtrees":
            assert variants == {"read_child", "matrix", "tip", "overwrite"}, variants
        if family == "queued":
            assert variants == {"independent", "reads", "overwrites", "reuses_scales"}, variants


def test_redrawn_share():
    """the range condition re-draws less than a tenth of the committed seed set's draws (every family x every shape x 20 seeds)"""
    shapes = sorted({(c.S, c.K, c.P, c.dbl, c.per_category, c.missing_is_one) for c in CONFIGS})
    draws = redraws = 0
    for shape in shapes:
        d = r = 0
        for family in lg.FAMILIES:
            for seed in range(EMU_SEEDS):
                c = lg.make_case(family, seed, *shape)
                d, r = d + c.draws, r + c.redraws
        print("%2d states x %d x %3d %s: %d of %d draws re-drawn (%.1f %%)" % (shape[0], shape[1], shape[2], "fp64" if shape[3] else "fp32", r, d, 100.0 * r / d))
        draws, redraws = draws + d, redraws + r
    print("all shapes: %d of %d draws re-drawn (%.2f %%)" % (redraws, draws, 100.0 * redraws / draws))
    assert redraws < 0.1 * draws
