"""ctypes binding of the engine's C ABI (include/libhmsbeagle/beagle.h).

This is the Python twin of what an FFI client of libhmsbeagle does: plain pointers and sizes in,
status codes out.  It loads mrbayes_amd/libhmsbeagle.so -- the HIP library built by
`python -m mrbayes_amd.build` -- and raises if it is missing: there is no fallback implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "libhmsbeagle.so")

BEAGLE_SUCCESS = 0
BEAGLE_ERROR_GENERAL = -1
BEAGLE_ERROR_OUT_OF_MEMORY = -2
BEAGLE_ERROR_UNINITIALIZED_INSTANCE = -4
BEAGLE_ERROR_OUT_OF_RANGE = -5
BEAGLE_ERROR_NO_RESOURCE = -6
BEAGLE_ERROR_NO_IMPLEMENTATION = -7
BEAGLE_ERROR_FLOATING_POINT = -8
BEAGLE_OP_NONE = -1

BEAGLE_FLAG_PRECISION_SINGLE = 1 << 0
BEAGLE_FLAG_PRECISION_DOUBLE = 1 << 1
BEAGLE_FLAG_EIGEN_REAL = 1 << 4
BEAGLE_FLAG_EIGEN_COMPLEX = 1 << 5
BEAGLE_FLAG_SCALING_ALWAYS = 1 << 8
BEAGLE_FLAG_SCALERS_LOG = 1 << 10
BEAGLE_FLAG_PROCESSOR_GPU = 1 << 16
BEAGLE_FLAG_SCALING_DYNAMIC = 1 << 25


class BeagleInstanceDetails(C.Structure):
    _fields_ = [("resourceNumber", C.c_int), ("resourceName", C.c_char_p), ("implName", C.c_char_p),
                ("implDescription", C.c_char_p), ("flags", C.c_long)]


class BeagleResource(C.Structure):
    _fields_ = [("name", C.c_char_p), ("description", C.c_char_p), ("supportFlags", C.c_long),
                ("requiredFlags", C.c_long)]


class BeagleResourceList(C.Structure):
    _fields_ = [("list", C.POINTER(BeagleResource)), ("length", C.c_int)]


class BeagleOperation(C.Structure):
    _fields_ = [("destinationPartials", C.c_int), ("destinationScaleWrite", C.c_int),
                ("destinationScaleRead", C.c_int), ("child1Partials", C.c_int),
                ("child1TransitionMatrix", C.c_int), ("child2Partials", C.c_int),
                ("child2TransitionMatrix", C.c_int)]


EXPORTS = [
    "beagleGetVersion", "beagleGetCitation", "beagleGetResourceList", "beagleCreateInstance",
    "beagleFinalizeInstance", "beagleFinalize", "beagleSetTipStates", "beagleSetTipPartials", "beagleSetPartials",
    "beagleGetPartials", "beagleSetEigenDecomposition", "beagleSetStateFrequencies", "beagleSetCategoryWeights",
    "beagleSetCategoryRates", "beagleSetPatternWeights", "beagleUpdateTransitionMatrices",
    "beagleSetTransitionMatrix", "beagleGetTransitionMatrix", "beagleConvolveTransitionMatrices", "beagleTransposeTransitionMatrices",
    "beagleSetTransitionMatrices", "beagleUpdatePartials", "beagleWaitForPartials",
    "beagleAccumulateScaleFactors", "beagleRemoveScaleFactors", "beagleResetScaleFactors", "beagleCopyScaleFactors",
    "beagleGetScaleFactors", "beagleCalculateRootLogLikelihoods", "beagleCalculateEdgeLogLikelihoods",
    "beagleGetSiteLogLikelihoods", "beagleGetSiteDerivatives", "beagleUpdatePrePartials", "beagleSetDifferentialMatrix",
    "beagleCalculateEdgeDerivatives", "beagleCalculateCrossProductDerivative", "mbamdCalculateSiteModelDerivatives", "mbamdCalculateEdgeSecondDerivatives",
    "mbamdGetSecondDerivativeLaunches", "mbamdCalculateInsertionLogLikelihoods", "mbamdGetInsertionLaunches", "mbamdCalculateNodePosteriors", "mbamdGetCategoryPosteriors", "mbamdSampleAncestralStates", "mbamdCalculateAutocorrelatedLogLikelihood", "mbamdSynchronize", "mbamdGetLastError", "mbamdKernelTiming",
    "mbamdGetKernelTiming", "mbamdGetListCounts", "mbamdGetWalkCounts", "mbamdGetRangeSafeCounts", "mbamdGetPlainWaveCounts", "mbamdGetRecomputeCounts", "mbamdGetSubtreeRecomputeCounts", "mbamdGetStepTiming", "mbamdUpdateFinalPartials", "mbamdGetScaledPartials", "mbamdSetKernelPath", "mbamdSetDeferredResult", "mbamdFetchLogLikelihood", "mbamdReduceLogLikelihood", "mbamdGetResourcePciBusId", "mbamdGetInstanceDevices",
    "mbamdGetScaleExponents", "mbamdGetChildCount", "mbamdSetRateMatrices", "mbamdSetRateMatricesFrom", "mbamdGetEigenDecomposition",
    "mbamdUpdateTransitionMatricesFromRateMatrix",
    # BEAGLE v3 surface (multi-partition instances, resource benchmark)
    "beagleGetBenchmarkedResourceList", "beagleSetCPUThreadCount", "beagleSetPatternPartitions",
    "beagleSetCategoryRatesWithIndex", "beagleUpdateTransitionMatricesWithMultipleModels", "beagleUpdatePartialsByPartition",
    "beagleAccumulateScaleFactorsByPartition", "beagleRemoveScaleFactorsByPartition", "beagleResetScaleFactorsByPartition",
    "beagleCalculateRootLogLikelihoodsByPartition", "beagleCalculateEdgeLogLikelihoodsByPartition",
]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class BeagleError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        super().__init__("%s failed with code %d%s" % (where, code, (": " + detail) if detail else ""))
        self.code = code


def _d(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _opt_i(a) -> Optional[np.ndarray]:
    return None if a is None else _i(a)


def _ptr(a: Optional[np.ndarray]):
    """the int pointer of an optional index array (None: NULL)"""
    return None if a is None else a.ctypes.data_as(_ip)


class BeagleLibrary:
    """The shared library, with argument types declared."""

    def __init__(self, path: Optional[str] = None):
        path = path or os.environ.get("MBAMD_LIBRARY") or DEFAULT_LIB
        if not os.path.exists(path):
            raise FileNotFoundError(
                "%s not found: build the HIP engine first (python -m mrbayes_amd.build). "
                "There is no CPU implementation to fall back to." % path)
        self.path = path
        self.lib = C.CDLL(path)
        for name in EXPORTS:
            if not hasattr(self.lib, name):
                raise AttributeError("%s does not export %s" % (path, name))
        L = self.lib
        L.beagleGetVersion.restype = C.c_char_p
        L.beagleGetCitation.restype = C.c_char_p
        L.mbamdGetLastError.restype = C.c_char_p
        L.beagleGetResourceList.restype = C.POINTER(BeagleResourceList)
        L.beagleCreateInstance.argtypes = [C.c_int] * 9 + [_ip, C.c_int, C.c_long, C.c_long,
                                                          C.POINTER(BeagleInstanceDetails)]
        L.beagleSetTipStates.argtypes = [C.c_int, C.c_int, _ip]
        L.beagleSetTipPartials.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleSetPartials.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleGetPartials.argtypes = [C.c_int, C.c_int, C.c_int, _dp]
        L.beagleSetEigenDecomposition.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp]
        L.beagleSetStateFrequencies.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleSetCategoryWeights.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleSetCategoryRates.argtypes = [C.c_int, _dp]
        L.beagleSetPatternWeights.argtypes = [C.c_int, _dp]
        L.beagleUpdateTransitionMatrices.argtypes = [C.c_int, C.c_int, _ip, _ip, _ip, _dp, C.c_int]
        L.beagleSetTransitionMatrix.argtypes = [C.c_int, C.c_int, _dp, C.c_double]
        L.beagleGetTransitionMatrix.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleConvolveTransitionMatrices.argtypes = [C.c_int, _ip, _ip, _ip, C.c_int]
        L.beagleTransposeTransitionMatrices.argtypes = [C.c_int, _ip, _ip, C.c_int]
        L.beagleSetTransitionMatrices.argtypes = [C.c_int, _ip, _dp, _dp, C.c_int]
        L.mbamdUpdateTransitionMatricesFromRateMatrix.argtypes = [C.c_int, _dp, _ip, _ip, _ip, _dp, C.c_int]
        L.beagleUpdatePartials.argtypes = [C.c_int, C.POINTER(BeagleOperation), C.c_int, C.c_int]
        L.beagleWaitForPartials.argtypes = [C.c_int, _ip, C.c_int]
        L.beagleAccumulateScaleFactors.argtypes = [C.c_int, _ip, C.c_int, C.c_int]
        L.beagleRemoveScaleFactors.argtypes = [C.c_int, _ip, C.c_int, C.c_int]
        L.beagleResetScaleFactors.argtypes = [C.c_int, C.c_int]
        L.beagleCopyScaleFactors.argtypes = [C.c_int, C.c_int, C.c_int]
        L.beagleGetScaleFactors.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleCalculateRootLogLikelihoods.argtypes = [C.c_int, _ip, _ip, _ip, _ip, C.c_int, _dp]
        L.beagleCalculateEdgeLogLikelihoods.argtypes = [C.c_int, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip, C.c_int,
                                                        _dp, _dp, _dp]
        L.beagleGetSiteLogLikelihoods.argtypes = [C.c_int, _dp]
        L.beagleGetSiteDerivatives.argtypes = [C.c_int, _dp, _dp]
        L.beagleUpdatePrePartials.argtypes = [C.c_int, C.POINTER(BeagleOperation), C.c_int, C.c_int]
        L.beagleSetDifferentialMatrix.argtypes = [C.c_int, C.c_int, _dp]
        L.beagleCalculateEdgeDerivatives.argtypes = [C.c_int, _ip, _ip, _ip, _ip, C.c_int, _dp, _dp, _dp]
        L.beagleCalculateCrossProductDerivative.argtypes = [C.c_int, _ip, _ip, _ip, _ip, _dp, C.c_int, _dp, _dp]
        L.mbamdCalculateSiteModelDerivatives.argtypes = [C.c_int, _ip, _ip, _ip, _ip, _dp, C.c_int, _dp, _dp, _dp, _dp]
        L.mbamdCalculateEdgeSecondDerivatives.argtypes = [C.c_int, _ip, _ip, _ip, _ip, _ip, C.c_int, _dp, _dp, _dp, _dp]
        L.mbamdGetSecondDerivativeLaunches.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdCalculateInsertionLogLikelihoods.argtypes = [C.c_int, _ip, _ip, _ip, _ip, _ip, _ip, _ip, C.c_int, _dp, _dp]
        L.mbamdGetInsertionLaunches.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdCalculateNodePosteriors.argtypes = [C.c_int, _ip, _ip, _ip, C.c_int, _dp, _ip, _dp, _dp]
        L.mbamdGetCategoryPosteriors.argtypes = [C.c_int, C.c_int, _dp]
        L.mbamdSampleAncestralStates.argtypes = [C.c_int, _ip, _ip, _ip, C.c_int, C.c_int, C.c_ulonglong, _ip, _ip, _dp]
        L.mbamdCalculateAutocorrelatedLogLikelihood.argtypes = [C.c_int, C.c_int, _ip, _ip, C.c_int, _dp, _dp, _dp]
        L.mbamdGetKernelTiming.argtypes = [C.c_int, _dp, C.POINTER(C.c_long), C.c_int]
        L.mbamdGetListCounts.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdGetWalkCounts.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdGetRangeSafeCounts.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdGetPlainWaveCounts.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdGetRecomputeCounts.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdGetSubtreeRecomputeCounts.argtypes = [C.c_int, C.POINTER(C.c_long)]
        L.mbamdGetStepTiming.argtypes = [C.c_int, _dp, C.POINTER(C.c_long), C.c_int]
        L.mbamdUpdateFinalPartials.argtypes = [C.c_int, C.c_void_p, C.c_int]
        L.mbamdGetScaledPartials.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.mbamdFetchLogLikelihood.argtypes = [C.c_int, _dp]
        L.mbamdReduceLogLikelihood.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.mbamdGetResourcePciBusId.argtypes = [C.c_int, C.c_char_p, C.c_int]
        L.mbamdGetInstanceDevices.argtypes = [C.c_int, _ip, C.c_int]

    def version(self) -> str:
        return self.lib.beagleGetVersion().decode()

    def last_error(self) -> str:
        return self.lib.mbamdGetLastError().decode()

    def pci_bus_id(self, resource: int) -> str:
        """PCI bus id of a resource ("0000:c1:00.0"): which physical GPU a rank / shard runs on."""
        buf = C.create_string_buffer(64)
        rc = self.lib.mbamdGetResourcePciBusId(resource, buf, 64)
        if rc != 0:
            raise BeagleError(rc, "mbamdGetResourcePciBusId", self.last_error())
        return buf.value.decode()

    def resources(self):
        rl = self.lib.beagleGetResourceList().contents
        return [(rl.list[i].name.decode(), rl.list[i].description.decode(), rl.list[i].supportFlags)
                for i in range(rl.length)]


_default: Optional[BeagleLibrary] = None


def library(path: Optional[str] = None) -> BeagleLibrary:
    global _default
    if path is not None:
        return BeagleLibrary(path)
    if _default is None:
        _default = BeagleLibrary()
    return _default


class BeagleInstance:
    """One engine instance; methods are the beagle* functions minus the instance argument."""

    def __init__(self, lib: BeagleLibrary, tip_count, partials_buffer_count, compact_buffer_count, state_count,
                 pattern_count, eigen_buffer_count, matrix_buffer_count, category_count, scale_buffer_count,
                 resource: Optional[int] = None, preference_flags=0, requirement_flags=0):
        self._L = lib
        self.lib = lib.lib
        self.details = BeagleInstanceDetails()
        rl = None
        rc = 0
        if resource is not None:
            arr = (C.c_int * 1)(resource)
            rl, rc = C.cast(arr, _ip), 1
        self.id = self.lib.beagleCreateInstance(tip_count, partials_buffer_count, compact_buffer_count, state_count,
                                                pattern_count, eigen_buffer_count, matrix_buffer_count,
                                                category_count, scale_buffer_count, rl, rc, preference_flags,
                                                requirement_flags, C.byref(self.details))
        if self.id < 0:
            raise BeagleError(self.id, "beagleCreateInstance", lib.last_error())
        self.state_count, self.pattern_count, self.category_count = state_count, pattern_count, category_count

    def _chk(self, code: int, where: str, allow=()):
        if code != BEAGLE_SUCCESS and code not in allow:
            raise BeagleError(code, where, self._L.last_error())
        return code

    def finalize(self):
        if self.id >= 0:
            self.lib.beagleFinalizeInstance(self.id)
            self.id = -1

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    # ---- data -----------------------------------------------------------------------------------
    def set_tip_states(self, tip, states):
        a = _i(states)
        self._chk(self.lib.beagleSetTipStates(self.id, tip, a.ctypes.data_as(_ip)), "beagleSetTipStates")

    def set_tip_partials(self, tip, partials):
        a = _d(partials)
        self._chk(self.lib.beagleSetTipPartials(self.id, tip, a.ctypes.data_as(_dp)), "beagleSetTipPartials")

    def set_partials(self, idx, partials):
        a = _d(partials)
        self._chk(self.lib.beagleSetPartials(self.id, idx, a.ctypes.data_as(_dp)), "beagleSetPartials")

    def get_partials(self, idx) -> np.ndarray:
        out = np.empty((self.category_count, self.pattern_count, self.state_count))
        self._chk(self.lib.beagleGetPartials(self.id, idx, BEAGLE_OP_NONE, out.ctypes.data_as(_dp)), "beagleGetPartials")
        return out

    def set_eigen_decomposition(self, idx, evec, ivec, evals):
        """evals: S values; on a complex instance (BEAGLE_FLAG_EIGEN_COMPLEX) 2 S, the real parts then the imaginary parts."""
        a, b, c = _d(evec), _d(ivec), _d(evals)
        want = self.state_count * (2 if self.details.flags & BEAGLE_FLAG_EIGEN_COMPLEX else 1)
        if c.size != want:
            raise ValueError("set_eigen_decomposition: %d eigenvalues for an instance that reads %d" % (c.size, want))
        self._chk(self.lib.beagleSetEigenDecomposition(self.id, idx, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                       c.ctypes.data_as(_dp)), "beagleSetEigenDecomposition")

    def set_rate_matrices(self, first, qs, pi, exchangeabilities=False):
        """Extension: eigen-systems of reversible rate matrices computed on the device (mbamdSetRateMatrices)."""
        a, b = _d(np.asarray(qs, dtype=np.float64)), _d(pi)
        n = a.size // (len(b) * len(b))
        self.lib.mbamdSetRateMatrices.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int]
        self._chk(self.lib.mbamdSetRateMatrices(self.id, first, n, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                1 if exchangeabilities else 0), "mbamdSetRateMatrices")

    def set_rate_matrices_from(self, first, qs, pi, warm_first, exchangeabilities=False, shield=False):
        """Extension: the same, warm-started from the eigenvectors of eigen buffers warm_first ... (mbamdSetRateMatricesFrom)."""
        a, b = _d(np.asarray(qs, dtype=np.float64)), _d(pi)
        n = a.size // (len(b) * len(b))
        self.lib.mbamdSetRateMatricesFrom.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int]
        self._chk(self.lib.mbamdSetRateMatricesFrom(self.id, first, n, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                    (1 if exchangeabilities else 0) | (2 if shield else 0), warm_first), "mbamdSetRateMatricesFrom")

    def get_eigen_decomposition(self, idx, basis=False):
        """Extension: the doubles of an eigen buffer read back (mbamdGetEigenDecomposition): (U, U^-1, lambda), with basis=True also
        V, the orthonormal eigenvectors the device solver keeps for warm starts (an error where the solver did not write the buffer)."""
        S = self.state_count
        U, Ui, lam, V = np.empty((S, S)), np.empty((S, S)), np.empty(S), np.empty((S, S)) if basis else None
        self.lib.mbamdGetEigenDecomposition.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp]
        self._chk(self.lib.mbamdGetEigenDecomposition(self.id, idx, U.ctypes.data_as(_dp), Ui.ctypes.data_as(_dp), lam.ctypes.data_as(_dp),
                                                      V.ctypes.data_as(_dp) if basis else None), "mbamdGetEigenDecomposition")
        return (U, Ui, lam, V) if basis else (U, Ui, lam)

    def set_state_frequencies(self, idx, f):
        a = _d(f)
        self._chk(self.lib.beagleSetStateFrequencies(self.id, idx, a.ctypes.data_as(_dp)), "beagleSetStateFrequencies")

    def set_category_weights(self, idx, w):
        a = _d(w)
        self._chk(self.lib.beagleSetCategoryWeights(self.id, idx, a.ctypes.data_as(_dp)), "beagleSetCategoryWeights")

    def set_category_rates(self, r):
        a = _d(r)
        self._chk(self.lib.beagleSetCategoryRates(self.id, a.ctypes.data_as(_dp)), "beagleSetCategoryRates")

    def set_pattern_weights(self, w):
        a = _d(w)
        self._chk(self.lib.beagleSetPatternWeights(self.id, a.ctypes.data_as(_dp)), "beagleSetPatternWeights")

    # ---- matrices -------------------------------------------------------------------------------
    def update_transition_matrices(self, eigen_index, prob_indices, edge_lengths, first=None, second=None):
        """first / second: matrix buffers that take dP/dt and d2P/dt2 of the same branches (either may be None)."""
        p, e = _i(prob_indices), _d(edge_lengths)
        d1, d2 = _opt_i(first), _opt_i(second)
        self._chk(self.lib.beagleUpdateTransitionMatrices(self.id, eigen_index, p.ctypes.data_as(_ip), _ptr(d1), _ptr(d2),
                                                          e.ctypes.data_as(_dp), len(p)),
                  "beagleUpdateTransitionMatrices")

    def set_transition_matrix(self, idx, m):
        a = _d(m)
        self._chk(self.lib.beagleSetTransitionMatrix(self.id, idx, a.ctypes.data_as(_dp), 0.0), "beagleSetTransitionMatrix")

    def get_transition_matrix(self, idx) -> np.ndarray:
        out = np.empty((self.category_count, self.state_count, self.state_count))
        self._chk(self.lib.beagleGetTransitionMatrix(self.id, idx, out.ctypes.data_as(_dp)), "beagleGetTransitionMatrix")
        return out

    def convolve_transition_matrices(self, first_indices, second_indices, result_indices):
        """result[u] = first[u] x second[u] per category, on the device, in list order (a result may be an operand of a later
        entry; never of its own).  Asynchronous."""
        a, b, r = _i(first_indices), _i(second_indices), _i(result_indices)
        if not len(a) == len(b) == len(r):
            raise ValueError("convolve_transition_matrices: the three index lists differ in length")
        self._chk(self.lib.beagleConvolveTransitionMatrices(self.id, a.ctypes.data_as(_ip), b.ctypes.data_as(_ip), r.ctypes.data_as(_ip), len(r)),
                  "beagleConvolveTransitionMatrices")

    def transpose_transition_matrices(self, input_indices, result_indices):
        """result[u] = the transpose of input[u] per category, on the device (result[u] == input[u] is allowed).  Asynchronous."""
        a, r = _i(input_indices), _i(result_indices)
        if len(a) != len(r):
            raise ValueError("transpose_transition_matrices: the two index lists differ in length")
        self._chk(self.lib.beagleTransposeTransitionMatrices(self.id, a.ctypes.data_as(_ip), r.ctypes.data_as(_ip), len(r)),
                  "beagleTransposeTransitionMatrices")

    def set_transition_matrices(self, indices, matrices):
        """The batch form of set_transition_matrix: matrices [count][categories][states][states], one transfer."""
        idx = _i(indices)
        a = _d(matrices).reshape(len(idx), self.category_count, self.state_count, self.state_count)
        self._chk(self.lib.beagleSetTransitionMatrices(self.id, idx.ctypes.data_as(_ip), a.ctypes.data_as(_dp), None, len(idx)),
                  "beagleSetTransitionMatrices")

    def update_transition_matrices_from_rate_matrix(self, q, prob_indices, edge_lengths, first=None, second=None):
        """P = exp(Q r_k t) of ANY rate matrix q [states][states] (non-reversible, defective: no eigen-system), on the device;
        first / second: matrix buffers that take P' = r_k Q P and P'' = r_k Q P' (either may be None).  Asynchronous."""
        a = _d(q).reshape(self.state_count, self.state_count)
        p, e = _i(prob_indices), _d(edge_lengths)
        d1, d2 = _opt_i(first), _opt_i(second)
        if len(e) != len(p) or any(d is not None and len(d) != len(p) for d in (d1, d2)):
            raise ValueError("update_transition_matrices_from_rate_matrix: the lists differ in length")
        self._chk(self.lib.mbamdUpdateTransitionMatricesFromRateMatrix(self.id, a.ctypes.data_as(_dp), p.ctypes.data_as(_ip), _ptr(d1), _ptr(d2),
                                                                       e.ctypes.data_as(_dp), len(p)),
                  "mbamdUpdateTransitionMatricesFromRateMatrix")

    # ---- partials / scaling -----------------------------------------------------------------------
    def update_partials(self, operations, cumulative_scale_index=BEAGLE_OP_NONE):
        """operations: int array [n][7] in BeagleOperation field order, or a ctypes array."""
        if isinstance(operations, np.ndarray) or isinstance(operations, (list, tuple)):
            a = _i(operations).reshape(-1, 7)
            ptr = a.ctypes.data_as(C.POINTER(BeagleOperation))   # keeps `a` alive
            n = a.shape[0]
        else:
            ptr, n = operations, len(operations)
        self._chk(self.lib.beagleUpdatePartials(self.id, ptr, n, cumulative_scale_index), "beagleUpdatePartials")

    def wait_for_partials(self):
        self._chk(self.lib.beagleWaitForPartials(self.id, None, 0), "beagleWaitForPartials")

    def accumulate_scale_factors(self, indices, cum):
        a = _i(indices)
        self._chk(self.lib.beagleAccumulateScaleFactors(self.id, a.ctypes.data_as(_ip), len(a), cum), "beagleAccumulateScaleFactors")

    def remove_scale_factors(self, indices, cum):
        a = _i(indices)
        self._chk(self.lib.beagleRemoveScaleFactors(self.id, a.ctypes.data_as(_ip), len(a), cum), "beagleRemoveScaleFactors")

    def reset_scale_factors(self, cum):
        self._chk(self.lib.beagleResetScaleFactors(self.id, cum), "beagleResetScaleFactors")

    def copy_scale_factors(self, dst, src):
        self._chk(self.lib.beagleCopyScaleFactors(self.id, dst, src), "beagleCopyScaleFactors")

    def get_scale_factors(self, idx) -> np.ndarray:
        out = np.empty(self.pattern_count)
        self._chk(self.lib.beagleGetScaleFactors(self.id, idx, out.ctypes.data_as(_dp)), "beagleGetScaleFactors")
        return out

    def get_scale_exponents(self, idx) -> np.ndarray:
        """Engine extension: the binary exponents behind a scale buffer, [categories][patterns]."""
        out = np.empty((self.category_count, self.pattern_count), dtype=np.int32)
        self._chk(self.lib.mbamdGetScaleExponents(self.id, idx, out.ctypes.data_as(_ip)), "mbamdGetScaleExponents")
        return out

    # ---- likelihood -------------------------------------------------------------------------------
    def calculate_root_log_likelihoods(self, buffers, weights, freqs, cums):
        """Returns (return code, lnL); BEAGLE_ERROR_FLOATING_POINT is passed through, as MrBayes expects."""
        b, w, f, c = _i(buffers), _i(weights), _i(freqs), _i(cums)
        out = C.c_double(0.0)
        rc = self.lib.beagleCalculateRootLogLikelihoods(self.id, b.ctypes.data_as(_ip), w.ctypes.data_as(_ip),
                                                        f.ctypes.data_as(_ip), c.ctypes.data_as(_ip), len(b), C.byref(out))
        self._chk(rc, "beagleCalculateRootLogLikelihoods", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, out.value

    def calculate_edge_log_likelihoods(self, parents, children, probs, weights, freqs, cums):
        p, ch, pr, w, f, c = _i(parents), _i(children), _i(probs), _i(weights), _i(freqs), _i(cums)
        out = C.c_double(0.0)
        rc = self.lib.beagleCalculateEdgeLogLikelihoods(self.id, p.ctypes.data_as(_ip), ch.ctypes.data_as(_ip),
                                                        pr.ctypes.data_as(_ip), None, None, w.ctypes.data_as(_ip),
                                                        f.ctypes.data_as(_ip), c.ctypes.data_as(_ip), len(p),
                                                        C.byref(out), None, None)
        self._chk(rc, "beagleCalculateEdgeLogLikelihoods", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, out.value

    def calculate_edge_derivatives(self, parents, children, probs, first, second, weights, freqs, cums):
        """The edge log-likelihood with its first and second derivative in the branch length (`first` / `second`: the matrix
        buffers holding dP/dt and d2P/dt2; second=None: first derivative only).  Returns (rc, lnL, d1, d2); d2 is None without
        `second`.  Error codes other than BEAGLE_ERROR_FLOATING_POINT raise."""
        p, ch, pr, w, f, c = _i(parents), _i(children), _i(probs), _i(weights), _i(freqs), _i(cums)
        d1, d2 = _opt_i(first), _opt_i(second)
        out, o1, o2 = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        rc = self.lib.beagleCalculateEdgeLogLikelihoods(self.id, p.ctypes.data_as(_ip), ch.ctypes.data_as(_ip),
                                                        pr.ctypes.data_as(_ip), _ptr(d1), _ptr(d2), w.ctypes.data_as(_ip),
                                                        f.ctypes.data_as(_ip), c.ctypes.data_as(_ip), len(p),
                                                        C.byref(out), C.byref(o1) if d1 is not None else None,
                                                        C.byref(o2) if d2 is not None else None)
        self._chk(rc, "beagleCalculateEdgeLogLikelihoods", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, out.value, (o1.value if d1 is not None else None), (o2.value if d2 is not None else None)

    def get_site_derivatives(self):
        """(d1, d2): the unweighted per-pattern derivatives of the last derivative call."""
        a, b = np.empty(self.pattern_count), np.empty(self.pattern_count)
        self._chk(self.lib.beagleGetSiteDerivatives(self.id, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp)), "beagleGetSiteDerivatives")
        return a, b

    # ---- the gradient in all branch lengths: pre-order partials ------------------------------------------------
    def update_pre_partials(self, operations, cumulative_scale_index=BEAGLE_OP_NONE):
        """operations: int array [n][7] in BeagleOperation field order, with the pre-order meaning of the fields
        (pre(n), NONE, NONE, pre(parent), n's matrix, the sibling's post-order buffer or BEAGLE_OP_NONE, the sibling's matrix)."""
        a = _i(operations).reshape(-1, 7)
        self._chk(self.lib.beagleUpdatePrePartials(self.id, a.ctypes.data_as(C.POINTER(BeagleOperation)), a.shape[0],
                                                   cumulative_scale_index), "beagleUpdatePrePartials")

    def set_differential_matrix(self, idx, m):
        a = _d(m)
        self._chk(self.lib.beagleSetDifferentialMatrix(self.id, idx, a.ctypes.data_as(_dp)), "beagleSetDifferentialMatrix")

    def calculate_edge_gradient(self, posts, pres, dmats, weights, sites=True):
        """d lnL / dt over every listed branch in one call (beagleCalculateEdgeDerivatives).  Returns (rc, per-site derivatives
        [count][patterns] or None without `sites`, sums [count], sums of squares [count]); an error code raises."""
        po, pr, dm, w = _i(posts), _i(pres), _i(dmats), _i(weights)
        n = len(po)
        per = np.empty((n, self.pattern_count)) if sites else None
        sums, sq = np.zeros(n), np.zeros(n)
        rc = self.lib.beagleCalculateEdgeDerivatives(self.id, po.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), dm.ctypes.data_as(_ip),
                                                     w.ctypes.data_as(_ip), n, per.ctypes.data_as(_dp) if sites else None,
                                                     sums.ctypes.data_as(_dp), sq.ctypes.data_as(_dp))
        self._chk(rc, "beagleCalculateEdgeDerivatives")
        return rc, per, sums, sq

    def calculate_edge_second_derivatives(self, posts, pres, dmats1, dmats2, weights, sites=True):
        """d lnL / dt and d2 lnL / dt2 over every listed branch in one call (mbamdCalculateEdgeSecondDerivatives), dmats1 / dmats2
        the differential matrices r Q and r^2 Q^2.  Returns (rc, per-site d1 [count][patterns], per-site d2 -- both None without
        `sites` --, sums of d1 [count], sums of d2 [count]); an error code raises."""
        po, pr, m1, m2, w = _i(posts), _i(pres), _i(dmats1), _i(dmats2), _i(weights)
        n = len(po)
        per1 = np.empty((n, self.pattern_count)) if sites else None
        per2 = np.empty((n, self.pattern_count)) if sites else None
        sums1, sums2 = np.zeros(n), np.zeros(n)
        rc = self.lib.mbamdCalculateEdgeSecondDerivatives(self.id, po.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), m1.ctypes.data_as(_ip),
                                                          m2.ctypes.data_as(_ip), w.ctypes.data_as(_ip), n,
                                                          per1.ctypes.data_as(_dp) if sites else None, per2.ctypes.data_as(_dp) if sites else None,
                                                          sums1.ctypes.data_as(_dp), sums2.ctypes.data_as(_dp))
        self._chk(rc, "mbamdCalculateEdgeSecondDerivatives")
        return rc, per1, per2, sums1, sums2

    def get_second_derivative_launches(self):
        """(read-out launches of calculate_edge_second_derivatives on the plain kernel, on the matrix-core kernel)"""
        out = (C.c_long * 2)()
        self._chk(self.lib.mbamdGetSecondDerivativeLaunches(self.id, out), "mbamdGetSecondDerivativeLaunches")
        return tuple(int(v) for v in out)

    def calculate_insertion_log_likelihoods(self, pres, posts, post_matrices, subtrees, subtree_matrices, subtree_scales, weights, sites=True):
        """The log-likelihood with a subtree attached at every listed point, minus that of the tree without it, in one call
        (mbamdCalculateInsertionLogLikelihoods): pres[e] the pre-order buffer at the point, posts[e] the node below it,
        post_matrices[e] the matrix from the point down to that node (BEAGLE_OP_NONE: the point is the node), subtrees[e] /
        subtree_matrices[e] / subtree_scales[e] the clade to attach, its pendant matrix and its cumulative scale buffer (or
        BEAGLE_OP_NONE).  Returns (rc, per-site log ratios [count][patterns] or None without `sites`, sums [count]); -inf where the
        attachment is impossible; an error code raises."""
        arrays = [_i(v) for v in (pres, posts, post_matrices, subtrees, subtree_matrices, subtree_scales, weights)]
        n = len(arrays[0])
        if any(len(v) != n for v in arrays):
            raise ValueError("calculate_insertion_log_likelihoods: the index lists differ in length")
        per = np.empty((n, self.pattern_count)) if sites else None
        sums = np.zeros(n)
        rc = self.lib.mbamdCalculateInsertionLogLikelihoods(self.id, *[v.ctypes.data_as(_ip) for v in arrays], n,
                                                            per.ctypes.data_as(_dp) if sites else None, sums.ctypes.data_as(_dp))
        self._chk(rc, "mbamdCalculateInsertionLogLikelihoods")
        return rc, per, sums

    def get_insertion_launches(self):
        """(launches of calculate_insertion_log_likelihoods on the plain kernel, on the matrix-core kernel)"""
        out = (C.c_long * 2)()
        self._chk(self.lib.mbamdGetInsertionLaunches(self.id, out), "mbamdGetInsertionLaunches")
        return tuple(int(v) for v in out)

    def calculate_node_posteriors(self, posts, pres, weights, sites=True, best=False):
        """The marginal posterior of every state at every listed node in one call (mbamdCalculateNodePosteriors).  Returns (rc,
        posteriors [count][patterns][states] or None without `sites`, best states [count][patterns] and their posteriors
        [count][patterns] -- both None without `best` --, sums [count][states]); an error code raises."""
        po, pr, w = _i(posts), _i(pres), _i(weights)
        n, P, S = len(po), self.pattern_count, self.state_count
        per = np.empty((n, P, S)) if sites else None
        states = np.empty((n, P), dtype=np.int32) if best else None
        values = np.empty((n, P)) if best else None
        sums = np.zeros((n, S))
        rc = self.lib.mbamdCalculateNodePosteriors(self.id, po.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), w.ctypes.data_as(_ip), n,
                                                   per.ctypes.data_as(_dp) if sites else None, states.ctypes.data_as(_ip) if best else None,
                                                   values.ctypes.data_as(_dp) if best else None, sums.ctypes.data_as(_dp))
        self._chk(rc, "mbamdCalculateNodePosteriors")
        return rc, per, states, values, sums

    def get_category_posteriors(self, weights_index):
        """q [categories][patterns]: the posterior category probabilities of the latest log-likelihood call
        (mbamdGetCategoryPosteriors)."""
        q = np.empty((self.category_count, self.pattern_count))
        self._chk(self.lib.mbamdGetCategoryPosteriors(self.id, weights_index, q.ctypes.data_as(_dp)), "mbamdGetCategoryPosteriors")
        return q

    def sample_ancestral_states(self, parent_slots, posts, matrices, weights_index, seed, categories=False, changes=False):
        """One draw of all ancestral states from their joint posterior (mbamdSampleAncestralStates): slot 0 is the parent buffer of the
        latest log-likelihood call, slot i + 1 the lower end of edge i, which hangs from slot parent_slots[i] <= i.  Returns (rc,
        states [count + 1][patterns] with -1 where nothing could be drawn, categories [patterns] or None, sampled changes per edge
        [count] or None); an error code raises."""
        ps, po, m = _i(parent_slots), _i(posts), _i(matrices)
        n, P = len(ps), self.pattern_count
        if not len(po) == len(m) == n:
            raise ValueError("sample_ancestral_states: the three index lists differ in length")
        states = np.empty((n + 1, P), dtype=np.int32)
        cats = np.empty(P, dtype=np.int32) if categories else None
        counts = np.empty(n) if changes else None
        rc = self.lib.mbamdSampleAncestralStates(self.id, ps.ctypes.data_as(_ip), po.ctypes.data_as(_ip), m.ctypes.data_as(_ip), n, weights_index,
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, states.ctypes.data_as(_ip), _ptr(cats),
                                                 counts.ctypes.data_as(_dp) if changes else None)
        self._chk(rc, "mbamdSampleAncestralStates")
        return rc, states, cats, counts

    def autocorrelated_log_likelihood(self, weights_index, site_patterns, transitions, jumps=None, posteriors=False):
        """The log-likelihood of the listed sites, in their order, under a Markov chain over the rate categories along the sequence
        (mbamdCalculateAutocorrelatedLogLikelihood): site_patterns[s] is the pattern of site s, transitions [K][K] the chain's
        matrix at distance 1, jumps[s] >= 1 (s >= 1; None: all 1) the distance between site s - 1 and site s.  The operands are
        those of the latest log-likelihood call.  Returns (rc, ln H, gamma [K][sites] or None); BEAGLE_ERROR_FLOATING_POINT is
        passed through, any other error code raises."""
        c, t, j = _i(site_patterns), _d(transitions), _opt_i(jumps)
        if j is not None and len(j) != len(c):
            raise ValueError("autocorrelated_log_likelihood: site_patterns and jumps differ in length")
        if t.shape != (self.category_count, self.category_count):
            raise ValueError("autocorrelated_log_likelihood: transitions must be [categories][categories]")
        out = C.c_double(0.0)
        gamma = np.empty((self.category_count, len(c))) if posteriors else None
        rc = self.lib.mbamdCalculateAutocorrelatedLogLikelihood(self.id, weights_index, c.ctypes.data_as(_ip), _ptr(j), len(c), t.ctypes.data_as(_dp),
                                                                C.byref(out), gamma.ctypes.data_as(_dp) if posteriors else None)
        self._chk(rc, "mbamdCalculateAutocorrelatedLogLikelihood", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, out.value, gamma

    def calculate_cross_products(self, posts, pres, rates, weights, edge_lengths, squared=False):
        """The cross-product matrix of the gradient in the rate matrix over every listed branch in one call
        (beagleCalculateCrossProductDerivative).  Returns (rc, X [states][states]), row = the state on the pre-order side; an error
        code raises.  squared=True passes a buffer for the sums of squares, which the engine refuses."""
        po, pr, ra, w, t = _i(posts), _i(pres), _i(rates), _i(weights), _d(edge_lengths)
        n, S = len(po), self.state_count
        x = np.empty((S, S))
        sq = np.empty((S, S)) if squared else None
        rc = self.lib.beagleCalculateCrossProductDerivative(self.id, po.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), ra.ctypes.data_as(_ip),
                                                            w.ctypes.data_as(_ip), t.ctypes.data_as(_dp), n, x.ctypes.data_as(_dp),
                                                            sq.ctypes.data_as(_dp) if squared else None)
        self._chk(rc, "beagleCalculateCrossProductDerivative")
        return rc, x

    def calculate_site_model_derivatives(self, posts, pres, dmats, weights, edge_lengths=None, edges=True, rates=True, counts=True, root=True):
        """The gradient in the site model over every listed branch in one call (mbamdCalculateSiteModelDerivatives): dmats name the
        differential matrices (unit rate, D_k = Q, for d lnL / d r_k).  Returns (rc, per edge and category [count][categories],
        d lnL / d r_k [categories], expected sites per category [categories], d lnL / d pi_i at fixed Q [states]) -- each None unless
        asked for; `rates` needs edge_lengths.  An error code raises."""
        po, pr, dm, w = _i(posts), _i(pres), _i(dmats), _i(weights)
        t = None if edge_lengths is None else _d(edge_lengths)
        n, K, S = len(po), self.category_count, self.state_count
        per = np.empty((n, K)) if edges else None
        r = np.empty(K) if rates else None
        c = np.empty(K) if counts else None
        f = np.empty(S) if root else None
        dptr = lambda a: None if a is None else a.ctypes.data_as(_dp)
        rc = self.lib.mbamdCalculateSiteModelDerivatives(self.id, po.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), dm.ctypes.data_as(_ip),
                                                         w.ctypes.data_as(_ip), dptr(t), n, dptr(per), dptr(r), dptr(c), dptr(f))
        self._chk(rc, "mbamdCalculateSiteModelDerivatives")
        return rc, per, r, c, f

    # ---- BEAGLE v3: multi-partition instances (reference src/mbbeagle.c:1500-3010) -------------------------------
    def child_count(self) -> int:
        return int(self.lib.mbamdGetChildCount(self.id))

    def set_pattern_partitions(self, partition_count, pattern_partitions):
        a = _i(pattern_partitions)
        self._chk(self.lib.beagleSetPatternPartitions(self.id, partition_count, a.ctypes.data_as(_ip)), "beagleSetPatternPartitions")

    def set_category_rates_with_index(self, index, rates):
        a = _d(rates)
        self._chk(self.lib.beagleSetCategoryRatesWithIndex(self.id, index, a.ctypes.data_as(_dp)), "beagleSetCategoryRatesWithIndex")

    def update_transition_matrices_with_multiple_models(self, eigen_indices, rate_indices, prob_indices, edge_lengths,
                                                        first=None, second=None):
        g, r, p, e = _i(eigen_indices), _i(rate_indices), _i(prob_indices), _d(edge_lengths)
        d1, d2 = _opt_i(first), _opt_i(second)
        self._chk(self.lib.beagleUpdateTransitionMatricesWithMultipleModels(
            self.id, g.ctypes.data_as(_ip), r.ctypes.data_as(_ip), p.ctypes.data_as(_ip), _ptr(d1), _ptr(d2), e.ctypes.data_as(_dp), len(p)),
            "beagleUpdateTransitionMatricesWithMultipleModels")

    def update_partials_by_partition(self, operations):
        """operations: int array [n][9] in BeagleOperationByPartition field order."""
        a = _i(operations).reshape(-1, 9)
        self._chk(self.lib.beagleUpdatePartialsByPartition(self.id, a.ctypes.data_as(C.c_void_p), a.shape[0]),
                  "beagleUpdatePartialsByPartition")

    def reset_scale_factors_by_partition(self, cum, partition):
        self._chk(self.lib.beagleResetScaleFactorsByPartition(self.id, cum, partition), "beagleResetScaleFactorsByPartition")

    def accumulate_scale_factors_by_partition(self, idx, cum, partition):
        a = _i(idx)
        self._chk(self.lib.beagleAccumulateScaleFactorsByPartition(self.id, a.ctypes.data_as(_ip), len(a), cum, partition),
                  "beagleAccumulateScaleFactorsByPartition")

    def remove_scale_factors_by_partition(self, idx, cum, partition):
        a = _i(idx)
        self._chk(self.lib.beagleRemoveScaleFactorsByPartition(self.id, a.ctypes.data_as(_ip), len(a), cum, partition),
                  "beagleRemoveScaleFactorsByPartition")

    def calculate_edge_log_likelihoods_by_partition(self, parents, children, probs, weights, freqs, cums, partitions, count):
        """index arrays laid out [count][len(partitions)]; returns (rc, per-partition sums, total)"""
        p, ch, pr, w, f, c, pt = _i(parents), _i(children), _i(probs), _i(weights), _i(freqs), _i(cums), _i(partitions)
        by = np.zeros(len(pt))
        out = C.c_double(0.0)
        rc = self.lib.beagleCalculateEdgeLogLikelihoodsByPartition(
            self.id, p.ctypes.data_as(_ip), ch.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), None, None, w.ctypes.data_as(_ip),
            f.ctypes.data_as(_ip), c.ctypes.data_as(_ip), pt.ctypes.data_as(_ip), len(pt), count, by.ctypes.data_as(_dp),
            C.byref(out), None, None, None, None)
        self._chk(rc, "beagleCalculateEdgeLogLikelihoodsByPartition", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, by, out.value

    def calculate_edge_derivatives_by_partition(self, parents, children, probs, first, second, weights, freqs, cums, partitions):
        """index arrays laid out [1][len(partitions)]; returns (rc, lnL, d1, d2), each a pair (per-partition sums, total);
        d2 is None without `second`"""
        p, ch, pr, w, f, c, pt = _i(parents), _i(children), _i(probs), _i(weights), _i(freqs), _i(cums), _i(partitions)
        d1, d2 = _opt_i(first), _opt_i(second)
        by = [np.zeros(len(pt)) for _ in range(3)]
        tot = [C.c_double(0.0) for _ in range(3)]
        rc = self.lib.beagleCalculateEdgeLogLikelihoodsByPartition(
            self.id, p.ctypes.data_as(_ip), ch.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), _ptr(d1), _ptr(d2), w.ctypes.data_as(_ip),
            f.ctypes.data_as(_ip), c.ctypes.data_as(_ip), pt.ctypes.data_as(_ip), len(pt), 1, by[0].ctypes.data_as(_dp), C.byref(tot[0]),
            by[1].ctypes.data_as(_dp) if d1 is not None else None, C.byref(tot[1]) if d1 is not None else None,
            by[2].ctypes.data_as(_dp) if d2 is not None else None, C.byref(tot[2]) if d2 is not None else None)
        self._chk(rc, "beagleCalculateEdgeLogLikelihoodsByPartition", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return (rc, (by[0], tot[0].value), (by[1], tot[1].value) if d1 is not None else None,
                (by[2], tot[2].value) if d2 is not None else None)

    def calculate_root_log_likelihoods_by_partition(self, buffers, weights, freqs, cums, partitions, count):
        b, w, f, c, pt = _i(buffers), _i(weights), _i(freqs), _i(cums), _i(partitions)
        by = np.zeros(len(pt))
        out = C.c_double(0.0)
        rc = self.lib.beagleCalculateRootLogLikelihoodsByPartition(
            self.id, b.ctypes.data_as(_ip), w.ctypes.data_as(_ip), f.ctypes.data_as(_ip), c.ctypes.data_as(_ip),
            pt.ctypes.data_as(_ip), len(pt), count, by.ctypes.data_as(_dp), C.byref(out))
        self._chk(rc, "beagleCalculateRootLogLikelihoodsByPartition", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, by, out.value

    def get_site_log_likelihoods(self) -> np.ndarray:
        out = np.empty(self.pattern_count)
        self._chk(self.lib.beagleGetSiteLogLikelihoods(self.id, out.ctypes.data_as(_dp)), "beagleGetSiteLogLikelihoods")
        return out

    # ---- engine extensions --------------------------------------------------------------------------
    def synchronize(self):
        self._chk(self.lib.mbamdSynchronize(self.id), "mbamdSynchronize")

    def kernel_timing(self, enable: bool):
        self._chk(self.lib.mbamdKernelTiming(self.id, 1 if enable else 0), "mbamdKernelTiming")

    def get_kernel_timing(self, reset=True):
        ms, n = C.c_double(0.0), C.c_long(0)
        self._chk(self.lib.mbamdGetKernelTiming(self.id, C.byref(ms), C.byref(n), 1 if reset else 0), "mbamdGetKernelTiming")
        return ms.value, n.value

    def get_list_counts(self):
        """(lists, paths, forked paths, paths fused with their log-likelihood, tree walks, their operations) of the lists (4-state calls; 20- and 60-63-state queue flushes)."""
        out = (C.c_long * 6)()
        self._chk(self.lib.mbamdGetListCounts(self.id, out), "mbamdGetListCounts")
        return tuple(int(v) for v in out)

    def get_walk_counts(self):
        """(launches of the 4-state walk kernel's plain instantiation, launches of the generic one)"""
        out = (C.c_long * 2)()
        self._chk(self.lib.mbamdGetWalkCounts(self.id, out), "mbamdGetWalkCounts")
        return tuple(int(v) for v in out)

    def get_range_safe_counts(self):
        """(queue flushes at 40 and 60-63 states on the range-safe instantiations of k_walkg / k_pathg, on the plain ones)"""
        out = (C.c_long * 2)()
        self._chk(self.lib.mbamdGetRangeSafeCounts(self.id, out), "mbamdGetRangeSafeCounts")
        return tuple(int(v) for v in out)

    def get_plain_wave_counts(self):
        """launches of the 4-state walk kernel's plain instantiations by waves per workgroup: element W - 1, W = 1 ... 8"""
        out = (C.c_long * 8)()
        self._chk(self.lib.mbamdGetPlainWaveCounts(self.id, out), "mbamdGetPlainWaveCounts")
        return tuple(int(v) for v in out)

    def get_recompute_counts(self):
        """(tip-pair buffers that whole-tree launches left unstored, buffers materialised since, launches that materialised them)"""
        out = (C.c_long * 3)()
        self._chk(self.lib.mbamdGetRecomputeCounts(self.id, out), "mbamdGetRecomputeCounts")
        return tuple(int(v) for v in out)

    def get_subtree_recompute_counts(self):
        """the same three counters for the subtrees of three and four compact tips (MBAMD_UNSTORED_TIPS)"""
        out = (C.c_long * 3)()
        self._chk(self.lib.mbamdGetSubtreeRecomputeCounts(self.id, out), "mbamdGetSubtreeRecomputeCounts")
        return tuple(int(v) for v in out)

    # ---- reports (include/libhmsbeagle/mbamd_reports.h) --------------------------------------------
    def update_final_partials(self, operations):
        """operations: int array [n][5] in MbamdFinalOperation field order
        (destinationPartials, ancestorFinal, downPartials, transitionMatrix, rootTip)."""
        a = _i(operations).reshape(-1, 5)
        self._chk(self.lib.mbamdUpdateFinalPartials(self.id, a.ctypes.data_as(C.c_void_p), a.shape[0]), "mbamdUpdateFinalPartials")

    def get_scaled_partials(self, idx, cumulative_scale_index=BEAGLE_OP_NONE):
        """-> (partials float32 [K][P][S] with the categories of a pattern at one scale, lnScale float32 [P])."""
        out = np.empty((self.category_count, self.pattern_count, self.state_count), dtype=np.float32)
        ln = np.empty(self.pattern_count, dtype=np.float32)
        self._chk(self.lib.mbamdGetScaledPartials(self.id, idx, cumulative_scale_index, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                  ln.ctypes.data_as(C.POINTER(C.c_float))), "mbamdGetScaledPartials")
        return out, ln

    def get_step_timing(self, reset=True):
        """(ms, spans): device time of whole evaluations (all kernels of a step and the gaps between them)."""
        ms, n = C.c_double(0.0), C.c_long(0)
        self._chk(self.lib.mbamdGetStepTiming(self.id, C.byref(ms), C.byref(n), 1 if reset else 0), "mbamdGetStepTiming")
        return ms.value, n.value

    def set_deferred_result(self, enable: bool):
        self._chk(self.lib.mbamdSetDeferredResult(self.id, 1 if enable else 0), "mbamdSetDeferredResult")

    def reduce_log_likelihood(self, device_ptr, waiting_stream=0):
        """The pending sum added up on the device into the double at `device_ptr`; `waiting_stream` (raw hipStream_t) waits for it."""
        self._chk(self.lib.mbamdReduceLogLikelihood(self.id, C.c_void_p(device_ptr), C.c_void_p(waiting_stream)), "mbamdReduceLogLikelihood")

    def devices(self):
        """Resource numbers of the engine(s) behind this instance (one per shard of a sharded instance)."""
        out = (C.c_int * 64)()
        n = self.lib.mbamdGetInstanceDevices(self.id, C.cast(out, _ip), 64)
        return [int(out[i]) for i in range(min(n, 64))]

    def fetch_log_likelihood(self):
        out = C.c_double(0.0)
        rc = self.lib.mbamdFetchLogLikelihood(self.id, C.byref(out))
        self._chk(rc, "mbamdFetchLogLikelihood", allow=(BEAGLE_ERROR_FLOATING_POINT,))
        return rc, out.value
