// The engine's environment switches, host side only.  read_switches() is the one place the engine
// reads its environment; an instance keeps the copy taken when it was created (beagleCreateInstance, mbamdParsCreateInstance).
// A flag is set when the variable exists, whatever its value; an integer holds the variable's atoi value, std::nullopt when it
// is unset -- the clamps stay where the value is used.  Default settings leave every field unset.
#pragma once

#include <cstdlib>
#include <optional>
#include <string>

namespace mbamd {

struct Switches {
    // ---- diagnostics
    bool stats = false;                    // MBAMD_STATS: per-entry-point call counts and host time, printed at exit (read at load)
    bool apiTrace = false;                 // MBAMD_API_TRACE: one stderr line per C-ABI call (read at load)
    bool verbose = false;                  // MBAMD_VERBOSE: error strings and schedule summaries on stderr
    bool walkTrace = false;                // MBAMD_WALK_TRACE: in-kernel clock stamps of the level kernels' serial launch (mbamdWalkTrace)
    bool reportDevice = false;             // MBAMD_REPORT_DEVICE: one stderr line per instance naming its physical GPU
    std::string mpiRank;                   // MBAMD_MPI_RANK: the MPI rank that line names (empty: unset)
    std::optional<int> shard;              // MBAMD_SHARD=<g>: shard the patterns over g devices from the named resource
    // ---- A/B references used by tests: the single-precision engine
    bool forceGeneric = false;             // MBAMD_FORCE_GENERIC: 4-state data through the general-state kernels
    bool noWalkG = false;                  // MBAMD_NO_WALKG: 20/61 states through the level kernels instead of the tree walk
    bool noMfma = false;                   // MBAMD_NO_MFMA: vector-ALU level kernels for 5 ... 64 states
    bool mfmaWhole = false;                // MBAMD_MFMA_WHOLE: one wave per (operation, 32 patterns) instead of per factor tile
    bool noDefer = false;                  // MBAMD_NO_DEFER: every operation list runs at once, no merging of per-part lists
    bool noInlinePrograms = false;         // MBAMD_NO_INLINE_PROGRAMS: every walk program through a device buffer
    bool noPlainWalk = false;              // MBAMD_NO_PLAIN_WALK: whole-tree 4-state lists on the generic k_walk4_t instead of its plain instantiation
    bool storeTipPairs = false;            // MBAMD_STORE_TIP_PAIRS: whole-tree 4-state lists store the results of tip pairs too (no recipes, no recomputation)
    std::optional<int> unstoredTips;       // MBAMD_UNSTORED_TIPS=<T>: such lists leave subtrees of up to T compact tips unstored (clamped to 2 ... 4; 2 = tip pairs only)
    bool noPath4 = false;                  // MBAMD_NO_PATH4: 4-state root-ward paths through k_walk4_t instead of k_path4
    bool noFusePath = false;               // MBAMD_NO_FUSE_PATH: a 4-state path and its log-likelihood as two launches
    bool noForkPath = false;               // MBAMD_NO_FORK_PATH: paths that join through the tree-walk scheduler
    bool noPathG = false;                  // MBAMD_NO_PATHG: 20/61-state root-ward paths through k_walkg instead of k_pathg
    std::optional<int> mfmaSerial;         // MBAMD_MFMA_SERIAL=<ratio>: lists of <= ratio x levels operations as one serial launch (0 = never)
    bool noSpine = false;                  // MBAMD_NO_SPINE: serial launches on the plain, not software-pipelined, kernel
    std::optional<int> spineWidth;         // MBAMD_SPINE_WIDTH=<w>: trailing levels of at most w operations join the serial launch
    bool noPoll = false;                   // MBAMD_NO_POLL: wait for a result with hipStreamSynchronize (the parsimony scorer too)
    std::optional<int> walkWaves;          // MBAMD_WALK_WAVES=<W>: waves per workgroup of the tree walks
    std::optional<int> maxLdsSlots;        // MBAMD_MAX_LDS_SLOTS=<n>: LDS slots per wave of the tree walks (a plain 4-state program of several waves: of its workgroup's one pool)
    std::optional<int> walkSmallPhase;     // MBAMD_WALK_SMALL_PHASE=<n>: tree-walk schedule shape
    std::optional<int> walkPlainMinOps;    // MBAMD_WALK_PLAIN_MIN_OPS=<n>: operations per wave from which a whole-tree 4-state list runs the plain loop on several waves (32)
    std::optional<int> walkPrefetch;       // MBAMD_WALK_PREFETCH=<distance>: prefetch distance of the 4-state walk
    bool walkSafe = false;                 // MBAMD_WALK_SAFE: every wait of the 4-state walk waits for everything
    bool eigen256 = false;                 // MBAMD_EIGEN_256: the device eigen-solver on 256 threads at every state count
    bool xprodGeneric = false;             // MBAMD_XPROD_GENERIC: cross products of 16 ... 64 states on the plain kernel instead of the matrix-core one
    bool curvGeneric = false;              // MBAMD_CURV_GENERIC: second derivatives of 16 ... 64 states on the plain kernel instead of the matrix-core one
    bool insertGeneric = false;            // MBAMD_INSERT_GENERIC: insertion log-likelihoods of 16 ... 64 states on the plain kernel instead of the matrix-core one
    std::optional<int> posteriorNodes;     // MBAMD_POSTERIOR_NODES=<n>: at most n nodes per launch of mbamdCalculateNodePosteriors, or edges of mbamdCalculateSiteModelDerivatives, or entries of mbamdCalculateInsertionLogLikelihoods (test only: a chunk boundary at a small shape)
    std::optional<int> samplePatterns;     // MBAMD_SAMPLE_PATTERNS=<n>: at most n patterns in flight in mbamdSampleAncestralStates (test only: several pattern ranges at a small shape)
    // ---- A/B references used by tests: the parsimony scorer
    std::optional<int> parsPhaseLimit;     // MBAMD_PARS_PHASE_LIMIT=<n>: phases per launch of the parsimony walk
    std::optional<int> parsWaves;          // MBAMD_PARS_WAVES=<W>: waves per workgroup of the parsimony walk
    // ---- A/B references used by tests: the double-precision engine
    bool f64NoWalk = false;                // MBAMD_F64_NO_WALK: level kernels instead of the four-state tree walk
    bool f64WalkAlways = false;            // MBAMD_F64_WALK_ALWAYS: the four-state walk for every eligible list
    std::optional<int> f64WalkSlots;       // MBAMD_F64_WALK_SLOTS=<n>: LDS slots per wave of that walk
    bool f64NoRing = false;                // MBAMD_F64_NO_RING: lists staged through the synchronising buffer instead of the ring
    bool f64NoMatrixQueue = false;         // MBAMD_F64_NO_MATRIX_QUEUE: a launch per beagleUpdateTransitionMatrices call
    bool f64MfmaNoLds = false;             // MBAMD_F64_MFMA_NO_LDS: the one-wave contraction kernel without LDS-parked matrices
    bool f64NoChain = false;               // MBAMD_F64_NO_CHAIN: a launch per level also for lists that are chains
    bool f64NoTipsKernel = false;          // MBAMD_F64_NO_TIPS_KERNEL: operations on two tips on the contraction kernel
};

inline Switches read_switches()
{
    auto on = [](const char* name) { return std::getenv(name) != nullptr; };
    auto num = [](const char* name) -> std::optional<int> {
        const char* e = std::getenv(name);
        return e ? std::optional<int>(std::atoi(e)) : std::nullopt;
    };
    Switches s;
    s.stats = on("MBAMD_STATS"); s.apiTrace = on("MBAMD_API_TRACE"); s.verbose = on("MBAMD_VERBOSE"); s.walkTrace = on("MBAMD_WALK_TRACE");
    s.reportDevice = on("MBAMD_REPORT_DEVICE"); s.shard = num("MBAMD_SHARD");
    if (const char* e = std::getenv("MBAMD_MPI_RANK")) s.mpiRank = e;
    s.forceGeneric = on("MBAMD_FORCE_GENERIC"); s.noWalkG = on("MBAMD_NO_WALKG"); s.noMfma = on("MBAMD_NO_MFMA"); s.mfmaWhole = on("MBAMD_MFMA_WHOLE");
    s.noDefer = on("MBAMD_NO_DEFER"); s.noInlinePrograms = on("MBAMD_NO_INLINE_PROGRAMS"); s.noPath4 = on("MBAMD_NO_PATH4");
    s.noPlainWalk = on("MBAMD_NO_PLAIN_WALK"); s.storeTipPairs = on("MBAMD_STORE_TIP_PAIRS"); s.unstoredTips = num("MBAMD_UNSTORED_TIPS");
    s.noFusePath = on("MBAMD_NO_FUSE_PATH"); s.noForkPath = on("MBAMD_NO_FORK_PATH"); s.noPathG = on("MBAMD_NO_PATHG");
    s.mfmaSerial = num("MBAMD_MFMA_SERIAL"); s.noSpine = on("MBAMD_NO_SPINE"); s.spineWidth = num("MBAMD_SPINE_WIDTH"); s.noPoll = on("MBAMD_NO_POLL");
    s.walkWaves = num("MBAMD_WALK_WAVES"); s.maxLdsSlots = num("MBAMD_MAX_LDS_SLOTS"); s.walkSmallPhase = num("MBAMD_WALK_SMALL_PHASE");
    s.walkPlainMinOps = num("MBAMD_WALK_PLAIN_MIN_OPS");
    s.walkPrefetch = num("MBAMD_WALK_PREFETCH"); s.walkSafe = on("MBAMD_WALK_SAFE"); s.eigen256 = on("MBAMD_EIGEN_256");
    s.xprodGeneric = on("MBAMD_XPROD_GENERIC"); s.curvGeneric = on("MBAMD_CURV_GENERIC"); s.insertGeneric = on("MBAMD_INSERT_GENERIC");
    s.posteriorNodes = num("MBAMD_POSTERIOR_NODES");
    s.samplePatterns = num("MBAMD_SAMPLE_PATTERNS");
    s.parsPhaseLimit = num("MBAMD_PARS_PHASE_LIMIT"); s.parsWaves = num("MBAMD_PARS_WAVES");
    s.f64NoWalk = on("MBAMD_F64_NO_WALK"); s.f64WalkAlways = on("MBAMD_F64_WALK_ALWAYS"); s.f64WalkSlots = num("MBAMD_F64_WALK_SLOTS");
    s.f64NoRing = on("MBAMD_F64_NO_RING"); s.f64NoMatrixQueue = on("MBAMD_F64_NO_MATRIX_QUEUE"); s.f64MfmaNoLds = on("MBAMD_F64_MFMA_NO_LDS");
    s.f64NoChain = on("MBAMD_F64_NO_CHAIN"); s.f64NoTipsKernel = on("MBAMD_F64_NO_TIPS_KERNEL");
    return s;
}

}  // namespace mbamd
