"""mbamdGetStepTiming and mbamdGetKernelTiming (the launch timer of the single-precision engine, mbamd_launch_timer.h): while kernel
timing is on, every whole-tree evaluation -- transition matrices, then the operation list, then the root log-likelihood -- is one step,
from the first kernel behind the previous log-likelihood call to the end of its integration kernel; a read with `reset` starts the count
again; with timing off no step is recorded; and the launches mbamdGetKernelTiming counts do not depend on whether timing is on.

  * CPU (`not gpu`): the host-emulation build of the same sources;
  * GPU (`gpu`): the product library on a MI355X.

Shapes: 4 states x 2 categories x 70 patterns on 6 taxa (the 4-state walk; two pattern blocks, the last one partial) and 20 states x 1 x
33 on 5 taxa (the 20-state walk, whose lists are deferred and run with the log-likelihood call).
"""
import pytest

from mrbayes_amd import beagle as bg
from mrbayes_amd import likelihood as lk
from mrbayes_amd.division import synthetic_division
from tests.hostemu import build_emu

SHAPES = {"dna_4x2x70": ("gtr", 6, 70, 2), "protein_20x1x33": ("wag", 5, 33, 1)}
_divisions = {}


@pytest.fixture(scope="module")
def emu():
    return bg.library(build_emu.build())


@pytest.fixture(scope="module")
def gpu():
    lib = bg.library()
    if not lib.resources():
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X")
    return lib


def division(shape):
    if shape not in _divisions:
        kind, ntaxa, npat, ncat = SHAPES[shape]
        _divisions[shape] = synthetic_division(kind, ntaxa, npat, ncat=ncat, alpha=0.7 if ncat > 1 else None)
    return _divisions[shape]


def evaluate(bd, times):
    """whole-tree evaluations: matrices, list, root log-likelihood"""
    out = []
    for _ in range(times):
        bd.TouchAllTreeNodes(0)
        out.append(bd.LogLike(0))
    return out


def check_step_timing(lib, shape):
    bd = lk.BeagleDivision(division(shape), lib)
    inst = bd.inst
    try:
        first = evaluate(bd, 1)[0]                                   # (tips, eigen-system and the rest of the set-up are behind us)
        inst.get_kernel_timing(reset=True)
        # ---- timing off: launches are counted, steps are not
        lnl_off = evaluate(bd, 3)
        _, launches_off = inst.get_kernel_timing(reset=True)
        ms, steps = inst.get_step_timing(reset=True)
        print("%s, timing off: %d launches, %d steps, %.6f ms" % (shape, launches_off, steps, ms))
        assert steps == 0 and ms == 0.0
        assert launches_off > 0 and launches_off % 3 == 0
        # ---- timing on: three evaluations are three steps
        inst.kernel_timing(True)
        lnl_on = evaluate(bd, 3)
        kms, launches_on = inst.get_kernel_timing(reset=True)
        ms, steps = inst.get_step_timing(reset=False)
        print("%s, timing on: %d launches in %.6f ms, %d steps in %.6f ms" % (shape, launches_on, kms, steps, ms))
        assert steps == 3 and ms >= 0.0 and kms >= 0.0
        assert launches_on == launches_off
        # ---- a read with reset reports them once more, the next one nothing
        ms2, steps2 = inst.get_step_timing(reset=True)
        assert steps2 == 3 and ms2 == ms
        assert inst.get_step_timing(reset=True) == (0.0, 0)
        assert inst.get_kernel_timing(reset=True) == (0.0, 0)
        # ---- off again: no step, the same launches
        inst.kernel_timing(False)
        lnl_after = evaluate(bd, 3)
        kms, launches_after = inst.get_kernel_timing(reset=True)
        ms, steps = inst.get_step_timing(reset=True)
        print("%s, timing off again: %d launches, %d steps" % (shape, launches_after, steps))
        assert steps == 0 and ms == 0.0 and kms == 0.0
        assert launches_after == launches_off
        assert all(v == first for v in lnl_off + lnl_on + lnl_after)     # (timing changes nothing that is computed)
    finally:
        bd.finalize()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_step_timing_on_emulation(emu, shape):
    check_step_timing(emu, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_step_timing(gpu, shape):
    check_step_timing(gpu, shape)
