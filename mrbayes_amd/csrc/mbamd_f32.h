// mbamd_f32.h -- the single-precision engine of one device: `Instance` (arenas, stream, plan cache, schedulers) with the compiled
// operation lists it runs (`Plan`, `PathStep`), its launch helpers, and new_engine(), the only place one is made.  Its scale
// buffers belong to a `ScaleStore` (mbamd_scale_store.h).  Included by mbamd_engine.cpp, whose C ABI reaches an engine through
// the public part of `Instance` and nothing else.
#ifndef MBAMD_F32_H_
#define MBAMD_F32_H_

#include <cmath>
#include <cstdlib>
#include <memory>
#include <unordered_map>

#include "mbamd_host.h"          // the HIP runtime, beagle.h, the switches, <algorithm> ... <vector>; diagnostics and the host runtime the engines share
#include "mbamd_kernels.h"
#include "mbamd_scale_store.h"   // ScaleStore: the scale buffers, whichever form holds them, and the kernels that move them between forms
#include "mbamd_reports.h"
#include "libhmsbeagle/mbamd_reports.h"
#include "mbamd_walk4_host.h"
#include "mbamd_kernels_mfma.h"
#include "mbamd_derivatives.h"   // k_edge_derivatives: lnL, d lnL / dt and d2 lnL / dt2 over one branch
#include "mbamd_preorder.h"      // k_pre_partials, k_edge_readout: the pre-order pass and the gradient in all branch lengths
#include "mbamd_crossproducts.h" // k_cross_products, k_cross_products_mfma: the cross-product matrix of the gradient in the rate matrix
#include "mbamd_posteriors.h"    // k_node_posteriors: node-state and category posteriors from the pre-order buffers
#include "mbamd_ancestral_sampling.h"   // k_sample_top, k_sample_edges: a draw of all ancestral states from their joint posterior
#include "mbamd_autocorrelated.h"  // k_hmm_products, k_hmm_vectors, k_hmm_posteriors: the site-order HMM over the rate categories
#include "mbamd_matrix_products.h" // k_matrix_products_*, k_matrix_transpose: matrices made out of matrices; MatrixLayoutF32
#include "mbamd_rate_exponential.h" // k_rate_exp_*: exp(Q t) of any rate matrix, no eigen-system

namespace mbamd {


// state counts the 20/61-state tree walk (mbamd_walkg.h) is instantiated for: amino acids, doublets, and the sense codons of
// every genetic code MrBayes knows (60 vertebrate mitochondrial ... 63; reference src/model.c SetCode)
// state counts MrBayes sends: restriction sites 2, covarion nucleotides 8, doublets 16, amino acids 20, covarion amino acids 40, the
// sense codons of every genetic code 60..63 (4 has its own kernel; anything else runs on the level kernels)
// (round 5: 3, 5, 6, 7, 9, 10 as well -- the state counts of standard (morphology) characters, whose transition-matrix classes are
//  engine instances of a few hundred patterns: a launch per dependency level of the level kernels was ten launches where this is one)
static inline bool wg_compiled(int S) { return (S >= 2 && S <= 10 && S != 4) || S == 16 || S == 20 || S == 40 || (S >= 60 && S <= 63); }
// FN<SC, WMAX, CH, DEPTH>: one row tile -> whole jobs two ahead; two row tiles -> half jobs one ahead (see k_walkg)
#if !defined(MBAMD_WG_DEPTH61)
#define MBAMD_WG_DEPTH61 1       // chunks the operand fetch of the 60..63-state kernels runs ahead (experiments: 2)
#endif
#define MBAMD_WG_DISPATCH(S, FN, ...)                                   \
    switch (S) {                                                        \
        case 2: FN<2, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 3: FN<3, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 5: FN<5, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 6: FN<6, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 7: FN<7, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 8: FN<8, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 9: FN<9, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 10: FN<10, 8, 1, 2>(__VA_ARGS__); break;                   \
        case 16: FN<16, 8, 1, 2>(__VA_ARGS__); break;                   \
        case 20: FN<20, 8, 1, 2>(__VA_ARGS__); break;                   \
        case 40: FN<40, 4, 1, 1>(__VA_ARGS__); break;                   \
        case 60: FN<60, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
        case 61: FN<61, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
        case 62: FN<62, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
        default: FN<63, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
    }

template <int SC_, int WMAX_, int CH_, int DEPTH_>
static void raise_walkg_lds(int maxLds)
{
    if (hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
        hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgsInline>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess)
        (void) hipGetLastError();
    if constexpr (WgShape<SC_>::BF) {            // (the range-safe instantiations exist where the pieces are bf16: wg_contract_bf16)
        if (hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgs, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
            hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgsInline, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess)
            (void) hipGetLastError();
    }
}

// 4-state walk: how an unstored result is made again from compact tips alone (Instance::ensureStored) -- the one to three operations of
// its subtree in post-order, the last one its own.  A child is a compact tip (its buffer index) or, `in` set, the result of an earlier
// operation of the same recipe (that operation's number): no buffer of an inner node is named.  Matrices, in the buffer's slot of the
// snapshot table: places 0 and 1 for its own operation (as a tip pair's), 2 + 2 j and 3 + 2 j for inner operation j (k_walk4_snapshot).
// (MBAMD_W4_UNSTORED_TIPS_MAX and MBAMD_W4_SNAP, the matrices of a slot: mbamd_walk4.h, beside k_walk4_snapshot)
#define MBAMD_W4_UNSTORED_TIPS_DEFAULT 4
struct Walk4Recipe {
    int nops = 0;
    struct Op { int c1, c2, mode; bool in1, in2; } op[MBAMD_W4_UNSTORED_TIPS_MAX - 1];
    bool usesTip(int tip) const
    {
        for (int j = 0; j < nops; ++j) if ((!op[j].in1 && op[j].c1 == tip) || (!op[j].in2 && op[j].c2 == tip)) return true;
        return false;
    }
};

// A compiled operation list: the device-resident table a partials kernel walks, cached under the exact
// BeagleOperation array it was built from.  MrBayes re-issues the same lists all the time (every move
// that dirties the whole tree alternates between the two buffer-flip states), so the host-side
// scheduling and the table upload happen once per distinct list, not once per generation.
struct Plan {
    std::vector<int> key;            // the BeagleOperation ints + cumulative index + layout epoch
    uint64_t hash = 0, lastUse = 0;
    uint64_t lastLaunch = 0;         // Instance::launchClock value of the latest launch that reads d_table
    PartialsOp* d_table = nullptr;
    size_t cap = 0;                  // bytes allocated for d_table
    struct Segment {                             // tree-walk path: one launch per hazard-free segment
        size_t first; int W, entries, nslots, tail = 2;
        bool plain = false, peel = false;        // 4-state walk: nothing rare in it (Walk4Template::plain / peel) -- k_walk4_t<Walk4Args, true>
        bool waves = false;                      // ... cut over W > 1 waves (Walk4Template::waves) -- k_walk4_t<Walk4Args, true, true>; nslots: of the workgroup
    };
    std::vector<Segment> segments;               // (Walk4Entry index of its program in d_table, geometry)
    std::vector<Walk4Entry> inlineProg;          // 4-state walk: a short single-segment program travels in the kernel arguments instead
    // 4-state walk: the SMALL SUBTREES (compact tips and operations of the list alone, at most MBAMD_UNSTORED_TIPS tips: tip pairs, and
    // subtrees of three and four tips) of a list that is ONE plain segment in a device buffer -- their entries carry MBAMD_W4_NOSTORE,
    // their destinations are left unstored with a recipe (Instance::leaveUnstored); empty for every other plan.  `inner`: the program
    // entries of the recipe's inner operations, which k_walk4_snapshot copies the matrices of (the side table behind the program)
    struct Unstored { int entry, dst; Walk4Recipe r; int inner[MBAMD_W4_UNSTORED_TIPS_MAX - 2]; };
    std::vector<Unstored> unstoredSubtrees;
    size_t sideFirst = 0; int sideCount = 0;     // the side table: Walk4Entry index in d_table, records (one per subtree of more than two tips)
    bool path = false;                           // 4-state walk: the list is a root-ward path -- inlineProg holds k_path4's entries
    bool forked = false;                         // ... of several arms that join (the list of a topology move)
    bool pathG = false;                          // 20/61-state walk: every list is a root-ward path of the same length -- inlineProg holds k_pathg's entries
    int lists = 1;                               // 20/61-state walk: > 1 = the segments are that many independent lists, ONE launch
    std::vector<int> start;                      // general path: first table entry of each dependency level
    bool anyScale = false;
    bool narrow = false;                         // general path: few operations per level -> one serial launch
    std::vector<std::pair<int, int>> chains;     // narrow general-state lists: (first table entry, operations) of up to four
                                                 // mutually independent sub-lists (they walk in parallel workgroups)
    std::vector<std::pair<int, int>> spineChains;   // the same for the serial tail of a level-launched list (levels >= serialFrom)
    int tipTip = 0;                              // general path: the first tipTip operations of level 0 have two compact tip children
    int serialFrom = 0;                          // general path: levels >= serialFrom are narrow (the spine towards the
                                                 // root): they run as one serial launch after the level launches
    std::vector<int> bufsRead, bufsWritten, scalesUsed;   // buffer / scale indices the list touches (deferral hazards)
};

// One operation of a root-ward path as Instance::recognisePath sees it, in buffer / matrix / scale INDICES: the path kernels'
// entries are filled from it in their own units (Instance::pathEntry).
struct PathStep {
    bool start, join;                // begins an arm (both children come from outside) / its other child is the saved result of the arm before
    bool chainTip, sibTip;           // the child is a compact tip
    int arm;                         // start: the number of operations of the arm it begins
    int dst, chain, sib;             // partials buffers: result; the child on the path (an operand only where an arm starts); the other child
    int mchain, msib;                // their transition matrices
    int scaleMode, scaleIdx;         // SCALE_NONE / SCALE_WRITE / SCALE_READ and its exponent buffer
};

// The single-precision engine of one device: arenas, stream, plan cache, schedulers.  Created by new_engine() only; the
// destructor hands everything back.  What the C ABI calls an instance is a Handle (further down), which owns one of these,
// several (pattern shards, v3 partitions), or the double-precision engine instead.
struct Instance;
static int new_engine(std::unique_ptr<Instance>& out, const Dims& d, int patternCount, int dev, const Switches& sw);

struct Instance {
    Instance() = default;
    Instance(const Instance&) = delete;
    Instance& operator=(const Instance&) = delete;
    ~Instance();
    int device = 0;
    // ---- what the C ABI calls (Handle, each_engine, integrate_any, the entry points); everything below `private:` is the engine's own
    const char* implName() const;
    void printStats(int id) const;               // MBAMD_STATS: the plan cache and list counters of instance number `id`
    int synchronize() { HIP_TRY(hipStreamSynchronize(stream)); return BEAGLE_SUCCESS; }
    int setTipStates(int tip, const int* states);
    int importPartials(int idx, const double* in, bool hasCategories);
    int getPartials(int idx, double* out);
    int setPatternWeights(const double* w, int count) { return upload(d_pweights, w, sizeof(double) * count); }
    int setEigen(int idx, const double* U, const double* Ui, const double* lam);
    int setRateMatrices(int first, int count, const double* q, const double* pi, int mode, int warmFirst = -1);
    int getEigen(int idx, double* U, double* Ui, double* lam, double* V);
    int setRates(int index, const double* r);
    // d1Idx / d2Idx: the matrix buffers that take dP/dt and d2P/dt2 of the same branches (either may be null)
    int updateMatrices(int eigenIndex, const int* probIdx, const double* lengths, int count, int rateSet = 0,
                       const int* d1Idx = nullptr, const int* d2Idx = nullptr);
    int setMatrix(int idx, const double* in);
    int getMatrix(int idx, double* out);
    // matrices made out of matrices (mbamd_matrix_products.h; semantics: beagle.h): asynchronous, every stored copy of a result written
    int convolveMatrices(const int* first, const int* second, const int* result, int count);
    int transposeMatrices(const int* input, const int* result, int count);
    int setMatrices(const int* idx, const double* in, int count);
    int updateMatricesFromRateMatrix(const double* q, const int* prob, const int* d1, const int* d2, const double* lengths, int count);
    int updatePartials(const BeagleOperation* ops, int n, int cumIdx);
    int flushPending(bool keepPath = false);
    // scale buffers, whichever of their forms holds them (ScaleStore): the range checks and the scheduling around the store's calls
    int resetScale(int idx, bool mayWait = false);
    int copyScale(int dst, int src);
    int accumulateScale(const int* idx, int n, int cumIdx, int sign, bool afterReset = false);
    // a reset that waits (resetScale) runs now: the entry points call it before anything else
    int runDeferredReset() { const int idx = deferredReset; deferredReset = -1; return idx < 0 ? BEAGLE_SUCCESS : resetScale(idx); }
    int getScaleExponents(int idx, int* out);
    // launchOnly: the result stays pending for fetchResult, as in deferred mode (children: launch everywhere first, collect afterwards)
    int integrate(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                  const int* cumIdx, int count, double* out, bool launchOnly = false);
    int fetchResult(double* out);
    void setDeferredResult(bool on) { deferred = on; }
    int reduceResult(double* deviceOut, void* waitingStream);
    bool hasSites() const { return haveSite; }
    int getSites(double* out);
    // Branch-length derivatives over one edge (mbamd_derivatives.h), synchronous: everything queued or held runs first.  prob / d1 / d2:
    // the matrix buffers holding P, P' and P'' of the branch (d2 < 0: first derivative only); out3: the weighted sums of lnL, d1, d2.
    // The per-pattern values stay with the engine: siteDerivatives(1 / 2), and getSites() returns this call's log-likelihoods.
    int edgeDerivatives(int parent, int child, int prob, int d1, int d2, int wIdx, int fIdx, int cumIdx, double out3[3]);
    bool hasDerivatives() const { return derivValid; }
    const double* siteDerivatives(int order) const { return h_deriv + (size_t) order * Ppad; }
    // The pre-order pass and the gradient in all branch lengths (mbamd_preorder.h; semantics: beagle.h), both after everything queued
    // or held.  updatePrePartials: one launch per group of mutually independent operations.  edgeReadout (beagleCalculateEdgeDerivatives
    // with dmat2 and sites2 null, mbamdCalculateEdgeSecondDerivatives otherwise, on this engine's patterns): synchronous; sums1[e] and
    // sums2[e] are this engine's weighted sums of d_c and of d_c^2 (with dmat2: of d2_c) of edge e, sites1 / sites2 (or null) take d_c /
    // d2_c of edge e at [e * siteStride + c].
    int updatePrePartials(const BeagleOperation* ops, int n, int cumIdx);
    int edgeReadout(const int* post, const int* pre, const int* dmat1, const int* dmat2, const int* wIdx, int count, double* sites1, double* sites2,
                    size_t siteStride, double* sums1, double* sums2);
    // crossProducts (beagleCalculateCrossProductDerivative on this engine's patterns): synchronous; out[S * S] is overwritten
    int crossProducts(const int* post, const int* pre, const int* rateIdx, const int* wIdx, const double* lengths, int count, double* out);
    void secondLaunchCounts(long out2[2]) const { out2[0] += secondLaunches[0]; out2[1] += secondLaunches[1]; }   // its read-out launches: plain / matrix-core kernel
    // nodePosteriors / categoryPosteriors (mbamdCalculateNodePosteriors / mbamdGetCategoryPosteriors on this engine's patterns;
    // mbamd_posteriors.h): synchronous; sums[i * S + a], per-pattern outputs (or null) at [(i * siteStride + c) * S + a] and [i * siteStride + c]
    int nodePosteriors(const int* post, const int* pre, const int* wIdx, int count, double* sites, int* bestStates, double* bestValues,
                       size_t siteStride, double* sums);
    int categoryPosteriors(int wIdx, double* out, size_t stride);
    // sampleAncestralStates (mbamdSampleAncestralStates on this engine's patterns; mbamd_ancestral_sampling.h): synchronous;
    // patternOffset = the index in the instance of this engine's pattern 0, states at [slot * stride + c], changes[i] never null
    int sampleAncestralStates(const int* parentSlots, const int* post, const int* matrices, int count, int wIdx, unsigned long long seed,
                              long long patternOffset, int* states, int* categories, double* changes, size_t stride);
    // mbamdCalculateAutocorrelatedLogLikelihood (mbamd_autocorrelated.h): the checks on this engine and where its inputs lie, then --
    // on the first engine of the instance -- the call itself over the sources of all; synchronous
    int autocorrelatedPrepare(int wIdx, HmmSource& src) { return autocorrelated_prepare(*this, wIdx, src); }
    int autocorrelatedRun(const HmmSource* sources, int sourceCount, int wIdx, const int* sitePatterns, const int* siteJumps, int n, const double* T,
                          double* outLnl, double* outPost)
    {
        return autocorrelated_run(*this, sources, sourceCount, wIdx, sitePatterns, siteJumps, n, T, outLnl, outPost);
    }
    int finalPass(const MbamdFinalOperation* ops, int count);
    int getScaledPartials(int idx, int cumIdx, float* out, float* outLn);
    void setTiming(bool on) { timing = on; }
    int kernelTiming(double* ms, long* launches, int reset);
    int stepTiming(double* ms, long* steps, int reset);
    void listCounts(long out6[6]) const { const long c[6] = {listsTotal, listsPath, forkedPaths, fusedPaths, listsWalked, opsWalked}; std::copy(c, c + 6, out6); }
    void rangeSafeCounts(long out2[2]) const { out2[0] = wgFlushesRangeSafe; out2[1] = wgFlushesPlain; }
    void walkCounts(long out2[2]) const { out2[0] = walksPlain; out2[1] = walksGeneric; }   // launches of the plain instantiations of k_walk4_t (one wave or several) / of the generic ones
    void plainWaveCounts(long out[MBAMD_W4_MAXW]) const { for (int w = 0; w < MBAMD_W4_MAXW; ++w) out[w] += walksPlainByW[w]; }   // ... of the plain ones by waves per workgroup (out[W - 1]; added: the sums over engines)
    int walkTrace(long long* out, int maxSteps, int* outSteps, int* outWaves);
    // tip-pair buffers launches left unstored / buffers materialised since / launches that materialised them (mbamdGetRecomputeCounts);
    // the same for the subtrees of three and four tips (mbamdGetSubtreeRecomputeCounts)
    void recomputeCounts(long out3[3]) const { out3[0] += leftUnstored; out3[1] += materialised; out3[2] += materialiseLaunches; }
    void subtreeRecomputeCounts(long out3[3]) const { out3[0] += leftUnstoredSub; out3[1] += materialisedSub; out3[2] += materialiseLaunchesSub; }

private:
    friend int new_engine(std::unique_ptr<Instance>&, const Dims&, int, int, const Switches&);
    hipStream_t stream{};
    int tipCount = 0, nBuffers = 0, S = 0, SP = 0, P = 0, Ppad = 0, nEigen = 0, nMatrices = 0, K = 0, nScale = 0;
    bool complexEigen = false;       // BEAGLE_FLAG_EIGEN_COMPLEX: launchMatrices takes the CX form of the matrix kernels
    bool s4 = false;                 // 4-state float4 layout + tree-walk kernel
    bool wg = false;                // 20/61-state tree-walk kernel on the matrix cores (mbamd_walkg.h) + its arenas
    bool noWalkG = false;            // the arenas of that path did not fit: level kernels with buffers allocated on first use
    bool arena() const { return s4 || wg; }   // buffers are slices of arenas, exponents are per (pattern, category)
    bool mfma = false;               // general-state path on the matrix cores (mbamd_kernels_mfma.h)
    int walkWaves = 1, lastWalkSteps = 0;   // (kernel trace bookkeeping of the serial MFMA kernels, tools/trace_*.py)
    // ---- 4-state tree-walk path (mbamd_walk4.h / mbamd_walk4_host.h) -------------------------------------------
    Walk4Builder w4;                 // launch geometry limits + the program compiler
    // Programs are a function of the list's dependency STRUCTURE only (who produces whose child, which children are
    // tips): the buffer / matrix / scale indices -- which change with every accept / reject flip -- just fill the
    // entries.  A move that touches the branches it touched before re-uses its template and only re-fills it.
    std::unordered_map<uint64_t, Walk4Template> w4templates;
    uint64_t scheduleHits = 0, scheduleMisses = 0;
    std::vector<Walk4Op> w4ops;      // scratch
    std::vector<int> w4key, w4writer, w4segList;                    // buildWalk scratch: no allocation per compiled list
    std::vector<char> w4written, w4segRead, w4segWritten, w4segScale;
    std::vector<Walk4Entry> w4table;
    int lastWalkW = 0, lastWalkSlots = 0, lastWalkEntries = 0, lastWalkPhases = 0, lastWalkCrossing = 0;
    bool walkCumFresh = false;       // the cumulative buffer of the list being submitted holds nothing yet (store, do not add)
    // ---- small subtrees a whole-tree launch did not store (MBAMD_W4_NOSTORE, mbamd_walk4.h).  Such a buffer stays `valid`: it carries a RECIPE
    // -- its compact tips, its one to three operations with their scale modes (Walk4Recipe: a closure, no inner buffer is named), and its
    // slot (its own index) in a device table of MATRIX SNAPSHOTS float [buffer][MBAMD_W4_SNAP][K][16],
    // copied by k_walk4_snapshot behind the integration launch (off the critical path) or, at the latest, before anything overwrites a
    // matrix or reads a recipe (flushSnapshot) -- so a recipe never depends on a matrix buffer the client may overwrite.  Every reader of
    // partials calls ensureStored first: the unstored buffers among those it names are recomputed into their arena slices by ONE launch of
    // the generic k_walk4_t (same source, same bits; exponent bytes go to the scratch rows, the real scale buffers were written by the
    // original launch).  A subtree of three or four tips runs its two or three operations on the plain instantiation instead, the inner
    // ones with MBAMD_W4_NOSTORE: only the named buffer is written.  Any write to a buffer drops its recipe; overwriting a tip
    // materialises the recipes that use it first.
    typedef Walk4Recipe Recipe;
    std::vector<char> unstored;      // per partials buffer: 1 = valid, not in the arena, recipes[idx] says how to make it
    std::vector<Recipe> recipes;
    int nUnstored = 0;               // every hook is one comparison while this is zero
    float* d_snap = nullptr;         // the matrix snapshots, allocated with the first unstored buffer
    Plan* snapPlan = nullptr;        // the plan whose tip-pair matrices are still to be copied there
    void* d_storeProg = nullptr;     size_t storeProgCap = 0;       // a materialising program too long for the kernel arguments
    std::vector<int> storeList;      // scratch
    std::vector<Walk4Entry> storeProg;
    long leftUnstored = 0, materialised = 0, materialiseLaunches = 0;                 // tip pairs
    long leftUnstoredSub = 0, materialisedSub = 0, materialiseLaunchesSub = 0;        // subtrees of three and four tips
    int unstoredTips() const { return std::max(2, std::min(MBAMD_W4_UNSTORED_TIPS_MAX, sw.unstoredTips.value_or(MBAMD_W4_UNSTORED_TIPS_DEFAULT))); }
    std::vector<int> w4subTips, w4subOps, w4entryOf;                // buildWalk scratch: per operation of the segment, its subtree
    int leaveUnstored(const Plan& plan);
    int flushSnapshot();
    int ensureStored(const int* bufs, int n);
    int ensureStoredSubtrees();
    int ensureStored(int a, int b = -1) { const int v[2] = {a, b}; return nUnstored ? ensureStored(v, 2) : BEAGLE_SUCCESS; }
    int storeUsersOfTip(int tip);
    void dropRecipe(int idx) { if (nUnstored && unstored[(size_t) idx]) { unstored[(size_t) idx] = 0; --nUnstored; } }
    // ---- 20/61-state tree walk: lists are deferred and merged (MrBayes submits one list per eigen-system part of a codon
    // model, reference src/mbbeagle.c:1095-1104; together they are ONE forest for the program compiler)
    std::vector<BeagleOperation> wgOps;          // operations of the deferred lists, concatenated
    std::vector<int> wgListStart, wgListCum;     // first operation / cumulative scale index (or BEAGLE_OP_NONE) of each list
    int32_t* wgCum[MBAMD_WG_MAXLISTS] = {nullptr, nullptr, nullptr, nullptr};
    int wgFresh = 0;
    // The bf16-piece contraction of 40 and 60..63 states has two instantiations (wg_contract_bf16): the plain one splits a row value
    // exactly only above about 2^-110.  wgRescaled[b]: buffer b was last written by a SCALE_WRITE operation of this layout -- every
    // column's maximum in [0.5, 1) (or, its exponent clamped, above 2^-24) --; anything else (a client's partials, an unscaled or
    // SCALE_READ result, pre-order and final partials) is of unknown magnitude.  A flush whose operations read nothing but rescaled
    // buffers and compact tips runs the plain instantiation, every other one the range-safe one (wgRangeSafe, for runWalkG).
    std::vector<uint8_t> wgRescaled;
    std::vector<int8_t> wgWrote;                 // scratch of flushWalkG
    bool wgRangeSafe = false;
    long wgFlushesRangeSafe = 0, wgFlushesPlain = 0;     // flushes at those state counts on either (mbamdGetRangeSafeCounts)
    void wgForget(int idx) { if (idx >= 0 && idx < (int) wgRescaled.size()) wgRescaled[(size_t) idx] = 0; }
    uint8_t* arenaTipStates = nullptr;           // uint8 [tile][buffer][32]
    unsigned long wgTileBytes = 0;               // partials arena: bytes between 32-pattern tiles
    unsigned wgTipTileBytes = 0;
    size_t wgTabFloats = 0;                      // first float of the tree-walk tables inside a matrix buffer
public:
    // deferred lists (`path`: a held 4-state path counts) / anything at all that flushPending would launch
    bool hasPending(bool path = true) const { return !pending.empty() || !wgListCum.empty() || (path && heldPath != nullptr); }
    bool hasWork(bool path = true) const { return hasPending(path) || !pendingJobs.empty(); }
private:
    // ---- 4-state path: a root-ward path (k_path4 plan) is HELD until the next call: if that call is the log-likelihood over the
    // path's last result, both run as one launch (k_path4_lnl); anything else runs the path first, as before
    Plan* heldPath = nullptr;
    int32_t* heldPathCum = nullptr;
    bool heldPathFresh = false;
    int heldPathDst = -1;                        // the partials buffer the path's last operation writes
    int runHeldPath();
    int integratePath4(const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx);
    int updatePartialsG(const BeagleOperation* ops, int n, int cumIdx);
    int flushWalkG();
    int runWalkG(const Plan& plan);
    int checkOperation(const BeagleOperation& b, const std::vector<char>& written, const char*& what) const;
    std::vector<PathStep> pathSteps;             // recognisePath's result (scratch of buildPath4 / buildPathG)
    bool recognisePath(const BeagleOperation* ops, int n, int L, bool& forked);
    Walk4Entry pathEntry(const PathStep& p, uint32_t pbuf, uint32_t tipb, uint32_t mbuf, int scratchRow) const;
    void pathPlan(Plan& plan, int entries, bool forked);
    bool buildPath4(Plan& plan, const BeagleOperation* ops, int n);
    bool buildPathG(Plan& plan, const BeagleOperation* ops, int n, const std::vector<int>& starts, int nl);
    Walk4Args walk4Args() const;
    WalkGArgs walkGArgs() const;
    void listLaunched(const BeagleOperation* ops, int n, bool path, bool forked);
    void postResultFlag();
    bool scaleOpsIndependentOfPending(const int* idx, int n, int cumIdx) const;
    uint64_t launchClock = 0, syncedClock = 0;   // launches issued / launches known complete (last stream synchronisation)
    uint64_t flagClock = 0;                      // launchClock when the polled result flag was queued (postResultFlag)
    uint32_t siteSeq = 0, seenSeq = 0;           // flag value behind the integration that wrote the latest site values / latest flag value fetched
    HostMirror h_freqs, h_weights;               // host mirrors of d_freqs / d_weights (setFreqs / setWeights)
    long long* d_trace = nullptr;    // MBAMD_WALK_TRACE: per-step clock stamps of workgroup 0 (timing experiments)

    int NT = 0, T = 0;               // MFMA packing: i-tiles of 32 rows, j-pairs
    size_t partialsFloats = 0, matrixFloats = 0, eigenDoubles = 0;

    std::vector<float*> partials;      // general path: allocated on first use; 4-state path: slices of the arena
    std::vector<uint8_t*> tipStates;   // non-null while the buffer holds compact tip states
    ScaleStore scales;                 // the scale buffers (mbamd_scale_store.h)
    std::vector<char> valid;          // partials buffer has been written (import or operation destination)
    // 4-state path: arenas (see mbamd_kernels.h: partials buffer-major, tips and exponents block-major), one allocation each
    float* arenaPartials = nullptr;
    uint64_t* arenaTips = nullptr;     // state bitplanes uint64 [block][buffer][4]
    BlockGeom geom{64, 64, 64};        // general path: linear [P_pad] arrays == block stride 64
    float* matrices = nullptr;
    double *d_eigen = nullptr, *d_freqs = nullptr, *d_weights = nullptr, *d_rates = nullptr, *d_pweights = nullptr;
    double *d_site = nullptr;
    // Clients that read the per-pattern values after every evaluation (MrBayes does for +I models,
    // src/mbbeagle.c:1295-1358) get them written straight into pinned host memory by the integration kernel:
    // switched on by the first beagleGetSiteLogLikelihoods call, from then on that call is a host memcpy.
    double* h_site = nullptr;
    double* h_site_dev = nullptr;
    bool siteToHost = false, siteOnHost = false;   // mode / where the latest evaluation put its values
    int nblocks = 0;                  // partial sums of the weighted site log-likelihoods (one per integration workgroup)
    // a derivative call's results, pinned host memory the kernel writes: [3][Ppad] per-pattern lnL / d1 / d2, then [3][Ppad / 64] block sums
    double* h_deriv = nullptr;
    double* h_deriv_dev = nullptr;
    bool derivValid = false;          // the last likelihood call was a derivative call: its site values are the instance's
    // ---- pre-order pass (mbamd_preorder.h) ----
    std::vector<char> preOrder;       // per partials buffer: a pre-order operation wrote it and nothing else has since
    void clearPreOrder(int idx) { if (idx >= 0 && idx < (int) preOrder.size()) preOrder[idx] = 0; }
    LnlOperands lastLnl;              // the operands of the latest log-likelihood call: what q is made of
    uint64_t qStamp = 0;              // lastLnl.stamp when d_q was computed
    double* d_q = nullptr;            size_t qCap = 0;             // [K][Ppad] posterior category probabilities
    void* d_preTable = nullptr;       size_t preTableCap = 0;      // the PreOp / GradEdge table of the call being served
    int lnlOperands(DerivArgs& a, int parent, int child, int prob, int wIdx, int fIdx, int cumIdx);
    DerivArgs layoutArgs() const;
    // f(this engine's layout as a compile-time constant): the one place that chooses among the kernels' instantiations
    template <class F> auto withLayout(F&& f) const
    {
        if (s4) return f(std::integral_constant<int, DERIV_S4>());
        if (wg) return f(std::integral_constant<int, DERIV_WG>());
        return f(std::integral_constant<int, DERIV_LEVELS>());
    }
    // ---- what the shared bodies of the pre-order, gradient and cross-product calls ask of this engine (mbamd_preorder.h) ----
    template <class E> friend int update_pre_partials(E&, const BeagleOperation*, int, int);
    template <class E> friend int ensure_posteriors(E&);
    template <class E> friend int edge_list_begin(E&, const char*);
    template <class E> friend int edge_check(const E&, const char*, int, int, int);
    template <class E> friend int edge_list_fill(E&, const int*, const int*, int, GradEdge*);
    template <class E> friend int cross_products(E&, const int*, const int*, const int*, const int*, const double*, int, double*);
    template <class E> friend int edge_readout(E&, const int*, const int*, const int*, const int*, const int*, int, double*, double*, size_t, double*, double*);
    template <class E, class L, class S> friend int chunked_readout(E&, int, const ReadoutShape&, L&&, S&&);
    template <class E> friend int node_posteriors(E&, const int*, const int*, const int*, int, double*, int*, double*, size_t, double*);
    template <class E> friend int category_posteriors(E&, int, double*, size_t);
    template <class E> friend int sample_ancestral_states(E&, const int*, const int*, const int*, int, int, unsigned long long, long long, int*, int*, double*, size_t);
    template <class E> friend int autocorrelated_prepare(E&, int, HmmSource&);
    template <class E> friend int autocorrelated_weights(E&, int, double*);
    template <class E> friend int autocorrelated_run(E&, const HmmSource*, int, int, const int*, const int*, int, const double*, double*, double*);
    template <class E> friend int matrix_list_run(E&, const char*, bool, const int*, const int*, const int*, int);
    template <class E> friend int matrix_list_set(E&, const char*, const int*, const double*, int);
    template <class E> friend int rate_exponential_run(E&, const char*, const double*, const int*, const int*, const int*, const double*, int);
    // everything queued or held runs first
    int runQueued() { return hasWork() ? flushPending() : BEAGLE_SUCCESS; }
    // ---- ... and the bodies of the matrix-product calls (mbamd_matrix_products.h) ----
    // where the copies of a matrix buffer lie: the device form of setMatrix / getMatrix
    MatrixLayoutF32 matrixLayout() const { return MatrixLayoutF32{S, SP, K, mfma ? T : 0, wg ? wgTabFloats : (size_t) 0}; }
    // what setMatrix does before a matrix changes: the matrices an unstored-subtree recipe needs are copied first
    int beforeMatrixWrite() { return snapPlan ? flushSnapshot() : BEAGLE_SUCCESS; }
    // the entry table of a list, staged as launchMatrices stages its jobs: in the pinned ring, which the kernel reads over the host link
    // (no copy launch in front of the kernel); a table too large for a quarter of the ring goes through device memory like a PreOp table
    int stageMatrixTable(const void* src, size_t bytes, const void** out)
    {
        if (((bytes + 63) & ~(size_t) 63) <= stage.capacity() / 4) return stageDirect(src, bytes, out);
        void* d = nullptr;
        const int rc = stageTable(src, bytes, &d);
        *out = d;
        return rc;
    }
    // the host image of a matrix buffer, every copy, from [K][S][S] doubles: what setMatrix uploads (h: matrixValues() floats)
    size_t matrixValues() const { return matrixFloats; }
    void matrixImage(const double* in, float* h) const;
    // (nothing to refuse: an engine of this kind holds one partition, and the C ABI turns a partitioned instance away itself)
    int refuses(const char*) const { return BEAGLE_SUCCESS; }
    // the buffer holds compact tip states / something a kernel can read (an unstored buffer is `valid`: beforeRead)
    bool holdsTip(int b) const { return operand(b).kind == CHILD_STATES; }
    bool readable(int b) const { return tipStates[b] || valid[b]; }
    // the buffer as an operand: its tip states or its partials (asPartials: partials whatever it holds now -- the list being compiled writes them)
    struct Operand { const void* ptr; ChildKind kind; };
    Operand operand(int b, bool asPartials = false) const { return tipStates[b] && !asPartials ? Operand{tipStates[b], CHILD_STATES} : Operand{partials[b], CHILD_PARTIALS}; }
    const void* operandPtr(int b) const { return operand(b).ptr; }
    // where an integration puts its per-pattern values: pinned host memory once a client has asked for them (getSites), else the device
    double* siteTarget() { siteOnHost = siteToHost && h_site_dev; return siteOnHost ? h_site_dev : d_site; }
    // the layout's strides as the kernels take them: partials (s4: f4 between blocks; wg: floats between tiles; level kernels: linear buffers)
    // and compact tips (s4: uint64 between the blocks of the bitplanes; wg: bytes between tiles; level kernels: none)
    struct Strides { size_t partials, tips; };
    Strides strides() const
    {
        return s4 ? Strides{geom.pstride, geom.tstride} : wg ? Strides{wgTileBytes / 4, wgTipTileBytes} : Strides{geom.pstride, 0};
    }
    float* partialsPtr(int b) const { return partials[b]; }
    // the buffers buf(0 .. n) that a call reads are in memory (those below zero: none)
    template <class F> int beforeRead(int n, F buf)
    {
        if (!nUnstored) return BEAGLE_SUCCESS;
        std::vector<int> reads((size_t) n);
        for (int i = 0; i < n; ++i) reads[(size_t) i] = buf(i);
        return ensureStored(reads.data(), n);
    }
    // a destination holds no recipe any more and has memory (buffers of the level kernels are allocated on first use) ...
    int beforeWrite(int d) { dropRecipe(d); return ensurePartials(d); }
    // ... nor the exponents of a final pass
    void afterWrite(int d) { if (d < (int) finalExpOf.size()) finalExpOf[d] = nullptr; wgForget(d); }
    // the PreOp / GradEdge table of a call, on the device
    int stageTable(const void* src, size_t bytes, void** out)
    {
        const int rc = grow(&d_preTable, &preTableCap, bytes);
        *out = d_preTable;
        return rc ? rc : upload(d_preTable, src, bytes);
    }
    // device memory for a call's results
    int resultScratch(size_t bytes, double** out) { const int rc = grow(&d_tmp, &tmpCap, bytes); *out = static_cast<double*>(d_tmp); return rc; }
    // the stream was synchronised: every launch so far is complete
    void afterSync() { syncedClock = launchClock; }
    // launches for kernelTiming to report
    void countLaunches(int n) { pendingLaunches += n; }
    // ... and, while timing is on, an event pair around the launches of a call (no span: such a call is no evaluation)
    int timedBegin(hipEvent_t& ev0, hipEvent_t& ev1)
    {
        if (!timing) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, stream));
        return BEAGLE_SUCCESS;
    }
    int timedEnd(hipEvent_t ev0, hipEvent_t ev1) { return launchesEnd(ev0, ev1); }
    // what getSites would return, where a kernel of this stream can read it (host: its host address where that is pinned host memory)
    int siteLogLikelihoods(const double** dev, const double** host)
    {
        if (!haveSite) return fail(BEAGLE_ERROR_GENERAL, "beagleGetSiteLogLikelihoods: no likelihood computed yet");
        *dev = derivValid ? h_deriv_dev : siteOnHost ? h_site_dev : d_site;
        *host = derivValid ? h_deriv : siteOnHost ? h_site : nullptr;
        return BEAGLE_SUCCESS;
    }
    const HostMirror& weightsMirror() const { return h_weights; }
    long secondLaunches[2] = {0, 0};  // order-2 read-out launches of edge_readout: plain / matrix-core kernel
    int posteriorOperands(DerivArgs& a);
    RateSets rateSets;                // category rates by index (beagleSetCategoryRatesWithIndex; index 0 = beagleSetCategoryRates), passed to kernels by value
    int pendingRateSet = 0;           // the rate set of the queued transition-matrix jobs
    bool haveSite = false;

    // growable device scratch
    double* d_ev = nullptr;           size_t evCap = 0;
    void* d_tmp = nullptr;            size_t tmpCap = 0;

    PinnedRing stage;                 // pinned staging ring for small asynchronous uploads and small kernel inputs: 8 MiB, 64-byte slots
    double* h_sums = nullptr;         // pinned host memory the integration kernel writes its block sums to
    double* h_sums_dev = nullptr;     // the device-side address of h_sums
    // The result is waited for by polling (CompletionWait, mbamd_host.h): the block sums are their own completion signal, armed
    // only when nothing else can still write h_sums (no unfetched result) and not in deferred mode (mbamdReduceLogLikelihood reads
    // them on the device); otherwise the stream writes the flag word behind the integration kernel (postResultFlag: wait.seq is the
    // sequence number of the last integration launched).  A wait of more than a millisecond falls back to the runtime's own.
    CompletionWait wait;
    bool sumsArmed = false, flagWritten = false;
    void armSums(bool launchOnly) { sumsArmed = !pendingResult && !deferred && !launchOnly && wait.arm(h_sums, (size_t) nblocks); }

    // timing of the partials kernels
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    double timedMs = 0.0;
    long timedLaunches = 0, pendingLaunches = 0;
    // ... and of whole evaluations: from the first kernel after a log-likelihood call (transition matrices, usually) to the
    // integration kernel's end -- every kernel of a step and the gaps between them, nothing of the host's wait
    hipEvent_t spanEv0{};
    bool spanOpen = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
    double spanMs = 0.0;
    long spanCount = 0;
    int spanBegin()
    {
        if (!timing || spanOpen) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventCreate(&spanEv0));
        HIP_TRY(hipEventRecord(spanEv0, stream));
        spanOpen = true;
        return BEAGLE_SUCCESS;
    }
    int spanEnd()
    {
        if (!spanOpen) return BEAGLE_SUCCESS;
        hipEvent_t e1{};
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e1, stream));
        spans.emplace_back(spanEv0, e1);
        spanOpen = false;
        if (spans.size() > 4096) {                   // a client that never polls: fold the finished spans into the running total
            HIP_TRY(hipStreamSynchronize(stream));
            spanFold();
        }
        return BEAGLE_SUCCESS;
    }
    int spanFold()                   // (stream synchronised by the caller)
    {
        for (auto& ev : spans) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) { spanMs += t; ++spanCount; }
            (void) hipEventDestroy(ev.first);
            (void) hipEventDestroy(ev.second);
        }
        spans.clear();
        return BEAGLE_SUCCESS;
    }
    // the bracket around the partials launches of one list (or of one merged flush): opens the evaluation's span if need be
    // and, while timing is on, records an event pair around them
    int launchesBegin(hipEvent_t& ev0, hipEvent_t& ev1)
    {
        { int src = spanBegin(); if (src) return src; }
        if (!timing) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, stream));
        return BEAGLE_SUCCESS;
    }
    int launchesEnd(hipEvent_t ev0, hipEvent_t ev1)
    {
        if (!timing) return BEAGLE_SUCCESS;
        HIP_TRY(hipEventRecord(ev1, stream));
        events.emplace_back(ev0, ev1);
        return BEAGLE_SUCCESS;
    }
    int eventsFold()                 // (stream synchronised by the caller)
    {
        for (auto& ev : events) {
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, ev.first, ev.second));
            timedMs += t;
            (void) hipEventDestroy(ev.first);
            (void) hipEventDestroy(ev.second);
        }
        events.clear();
        return BEAGLE_SUCCESS;
    }

    bool deferred = false, pendingResult = false;
    hipEvent_t reduceEvent{};        // mbamdReduceLogLikelihood: orders a client's stream behind the device-side sum
    // final pass (mbamd_reports.h): per partials buffer, the exponents [K][Ppad] its final partials carry (nullptr: not final
    // partials); owned by the top node's destination buffers
    std::vector<int32_t*> finalExpOf;
    std::unordered_map<int, int32_t*> finalExpOwn;

    std::vector<std::pair<Plan*, int>> pending;   // deferred general-path lists (plan, cumulative scale index or -1)
    std::vector<Plan*> plans;        // small LRU cache of compiled operation lists
    uint64_t planClock = 0;
    int layoutEpoch = 0;             // bumped whenever a buffer changes between compact-tip and partials form
    long planHits = 0, planMisses = 0, fusedPaths = 0, heldPaths = 0, forkedPaths = 0, listsTotal = 0, listsPath = 0, opsWalked = 0, listsWalked = 0;
    long walksPlainByW[MBAMD_W4_MAXW] = {};      // walksPlain by waves per workgroup (mbamdGetPlainWaveCounts)
    long walksPlain = 0, walksGeneric = 0;       // k_walk4_t launches: the plain instantiation / the generic ones (mbamdGetWalkCounts); materialising launches (ensureStored) are not counted

    // ---- helpers ----------------------------------------------------------------------------
    int grow(void** p, size_t* cap, size_t bytes) { return grow_device(stream, p, cap, bytes, std::max(bytes, *cap * 2)); }

    // copy host bytes to the device asynchronously through the pinned ring
    int upload(void* dst, const void* src, size_t bytes)
    {
        if (bytes == 0) return BEAGLE_SUCCESS;
        if (bytes > stage.capacity() / 2) {    // big one-off transfers (tip data): plain blocking copy
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
            return BEAGLE_SUCCESS;
        }
        // (round 6: small transfers -- eigen-systems, frequencies, weights, compiled programs -- go through the pinned ring and a copy
        //  kernel of ours: hipMemcpyAsync costs the host ~10 us a call and its blit kernel left the walk behind it 30 % slower,
        //  profiles/r06_ring_copy.txt)
        if (bytes <= ((size_t) 256 << 10) && bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) return ringCopy(dst, src, bytes);
        size_t off = 0;
        int rc = stage.put(src, bytes, stream, &off);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(dst, stage.host(off), bytes, hipMemcpyHostToDevice, stream));
        return BEAGLE_SUCCESS;
    }
    int ringCopy(void* dst, const void* src, size_t bytes);

public:
    // (idx < nEigen: checked by the C ABI)
    int setFreqs(int idx, const double* f) { return h_freqs.send((size_t) nEigen * S, (size_t) idx * S, f, (size_t) S, [&] { return upload(d_freqs + (size_t) idx * S, f, sizeof(double) * S); }); }
    int setWeights(int idx, const double* w) { return h_weights.send((size_t) nEigen * K, (size_t) idx * K, w, (size_t) K, [&] { return upload(d_weights + (size_t) idx * K, w, sizeof(double) * K); }); }
private:

    // small kernel inputs (job lists, pointer lists): placed in the pinned ring and read by the kernel
    // directly over the host link -- no copy engine, no extra stream operation
    int stageDirect(const void* src, size_t bytes, const void** devPtr) { return stage.putDirect(src, bytes, stream, devPtr); }

    int ensurePartials(int idx)
    {
        if (partials[idx]) return BEAGLE_SUCCESS;
        if (arena()) return fail(BEAGLE_ERROR_GENERAL, "partials arena not initialised");
        float* p = nullptr;
        HIP_TRY(hipMalloc(&p, partialsFloats * sizeof(float)));
        HIP_TRY(hipMemsetAsync(p, 0, partialsFloats * sizeof(float), stream));
        partials[idx] = p;
        return BEAGLE_SUCCESS;
    }
    float* matrixPtr(int idx) const { return matrices + (size_t) idx * matrixFloats; }

    int create(const Dims& dim, int patternCount, int dev, const Switches& switches);   // patternCount: this engine's (a shard's differ from dim.patternCount)

    int configureWalk();
    void wgGeometry(int lists, int& W, int& slots) const;
    int setTipMasks(int tip, const std::vector<uint8_t>& masks);
    std::vector<int> eigenWarm;      // per eigen buffer: -1 = no orthonormal basis stored (host-set), else warm starts since the last cold one
    std::vector<char> eigenShield;   // per eigen buffer: the next beagleSetEigenDecomposition is ignored (mbamdSetRateMatricesFrom, mode bit 1)
    int updatePartials4(const BeagleOperation* ops, int n, int cumIdx);
    int buildWalk(Plan& plan, const BeagleOperation* ops, int n, const int* listOf = nullptr, bool perList = false);
    int deferredReset = -1;          // a reset that waits for the call after it (resetScale, accumulateScale), or -1
    int checkIntegrate(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx, int count);
    // the (checked) operands of a log-likelihood call in device pointers: A = IntegrateArgs (level kernels) or IntegrateArgs4 (arenas)
    template <class A> int integrateOperands(A& a, const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx, int count)
    {
        std::memset(&a, 0, sizeof a);
        a.count = count;
        for (int n = 0; n < count; ++n) {
            a.parent[n] = reinterpret_cast<std::decay_t<decltype(a.parent[n])>>(partials[parent[n]]);      // (const float* / const f4*)
            if (child) {
                const Operand c = operand(child[n]);
                a.child[n] = c.ptr; a.child_kind[n] = c.kind;
                a.matrix[n] = matrixPtr(prob[n]);
            }
            a.weights[n] = d_weights + (size_t) wIdx[n] * K;
            a.freqs[n] = d_freqs + (size_t) fIdx[n] * S;
            if (cumIdx && cumIdx[n] != BEAGLE_OP_NONE) { int rc = scales.cumulativeForRead(cumIdx[n], a.cum[n]); if (rc) return rc; }
        }
        return BEAGLE_SUCCESS;
    }
    int integrate4(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                   const int* cumIdx, int count);
    int integrateLevels(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                        const int* cumIdx, int count);
    int buildGeneric(Plan& plan, std::vector<PartialsOp>& dev, const std::vector<int>& dstIdx, const std::vector<int>& c1Idx,
                     const std::vector<int>& c2Idx);
    int runWalk(const Plan& plan, int32_t* cum);
    int runGeneric(const Plan& plan, int32_t* cum);
    Plan* cachedPlan(const int* key, size_t nints, bool& build);
    int planBuilt(Plan& plan, int rc);
    int planTable(Plan& plan, const void* table, size_t bytes);
    int timedRun(const Plan& plan, int32_t* cum);
    int flushMatrices();
    template <int ORDER, bool CX = false> int launchMatrices(const MatrixJob* jobs, int count);
    std::vector<MatrixJob> pendingJobs;          // queued beagleUpdateTransitionMatrices work
    std::vector<char> pendingMatrixOut;          // matrix buffers the queued jobs write
    int submit(Plan* plan, int cumIdx, int32_t* cumPtr);
    Switches sw;                     // the environment switches, read when the instance was created (mbamd_switches.h)
    int serialRatio = 4;             // lists with <= ratio * levels operations run as ONE serial launch (0 = never; MBAMD_MFMA_SERIAL)
    bool independentOfPending(const Plan& plan, int cumIdx);
    int accumulate(const int* idx, int n, int cumIdx, int sign, bool fresh = false);   // fresh: cumIdx was reset just before -- store, do not add
    void ensureTrace();
    template <int SC_, int WMAX_, int CH_, int DEPTH_>
    static void launch_walkg_t(Instance& in, const WalkGArgs& a, int W, int nslots, const std::vector<Walk4Entry>* inlineProg);
    template <int SC_> static void launch_pathg_t(Instance& in, const WalkGArgs& a, const std::vector<Walk4Entry>& prog, bool forked);
    template <int NT_, int SC_, int KC_> static void launch_mfma_t(Instance& in, const PartialsOp* ops, int count, int32_t* cum);
    template <int NT_, int SC_, int KC_> static void launch_mfma_split_t(Instance& in, const OpTables& tabs, int count);
    template <int SC_, int KC_> static void launch_tips_t(Instance& in, const OpTables& tabs, int count);
    template <int NT_, int SC_, int KC_> static void launch_mfma_serial_t(Instance& in, const OpTables& tabs, int ntables);
    template <int NT_, int SC_, int KC_> static void launch_mfma_spine_t(Instance& in, const OpTables& tabs, int ntables);
    template <int SP_, int FK_> static void launch_gen(Instance& in, const PartialsOp* ops, int count, int32_t* cum);
    static bool launch_mfma(Instance& in, const PartialsOp* ops, int count, int32_t* cum);
    static bool launch_mfma_split(Instance& in, const OpTables& tabs, int count);
    static bool launch_mfma_serial(Instance& in, const OpTables& tabs, int ntables);
    static bool launch_tips(Instance& in, const OpTables& tabs, int count);
};

// A new engine for `patternCount` of an instance's patterns on one device -- the only place one is made.  The 20/61-state tree
// walk allocates every buffer up front (arenas); if that does not fit, the engine is set up once more on the level kernels,
// which allocate a buffer when it is first written.
static int new_engine(std::unique_ptr<Instance>& out, const Dims& d, int patternCount, int dev, const Switches& sw)
{
    for (int attempt = 0; attempt < 2; ++attempt) {
        std::unique_ptr<Instance> c(new Instance());
        c->noWalkG = attempt == 1;
        const int rc = c->create(d, patternCount, dev, sw);
        if (rc == BEAGLE_SUCCESS) { out = std::move(c); return rc; }
        const bool retry = rc == BEAGLE_ERROR_OUT_OF_MEMORY && c->wg && attempt == 0;
        c.reset();
        (void) hipGetLastError();
        if (!retry) return rc;
    }
    return BEAGLE_ERROR_OUT_OF_MEMORY;
}

// ---------------------------------------------------------------------------------------------
inline int Instance::create(const Dims& dim, int patternCount, int dev, const Switches& switches)
{
    sw = switches;
    device = dev;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    tipCount = dim.tipCount;
    nBuffers = dim.partialsBufferCount + dim.compactBufferCount;
    S = dim.stateCount;
    P = patternCount;
    Ppad = round_up(P, 64);
    K = dim.categoryCount;
    nEigen = dim.eigenBufferCount;
    nMatrices = dim.matrixBufferCount;
    nScale = dim.scaleBufferCount;
    complexEigen = dim.complexEigen;
    // the 4-state tree walk addresses buffers with 32-bit byte offsets inside a (block, category) column set (Walk4Entry)
    s4 = (S == 4 && !sw.forceGeneric && (size_t) nBuffers * K * 1024 < ((size_t) 1 << 32) && (size_t) nMatrices * K * 64 < ((size_t) 1 << 32) &&
          (size_t) (nScale + MBAMD_W4_SCRATCH_ROWS) * K * 64 < ((size_t) 1 << 32));
    // 20 / 61 states: the tree-walk kernel on the matrix cores (MBAMD_NO_WALKG=1: the level kernels of mbamd_kernels_mfma.h)
    {
        const size_t tb = wg_block_bytes(S), mf = (size_t) K * 64 * 64 + (size_t) K * wg_table_floats(S);
        wg = !s4 && wg_compiled(S) && K <= 16 && !sw.forceGeneric && !noWalkG && !sw.noWalkG &&
             (size_t) (nBuffers + 1) * K * tb < ((size_t) 1 << 32) && (size_t) nMatrices * mf * 4 < ((size_t) 1 << 32) &&
             (size_t) (nScale + MBAMD_WG_SCRATCH_ROWS) * K * 64 < ((size_t) 1 << 32) && (size_t) nBuffers * MBAMD_WG_TW < ((size_t) 1 << 32);
    }
    if (s4) SP = 4;
    else if (S <= 4) SP = 4;
    else if (S <= 8) SP = 8;
    else if (S <= 16) SP = 16;
    else if (S <= 20) SP = 20;
    else if (S <= 32) SP = 32;
    else SP = 64;
    NT = (S + 31) / 32;
    T = (S + 1) / 2;
    mfma = !s4 && !wg && S >= 5 && S <= 64 && ((NT == 1 && K <= 4) || (NT == 2 && K <= 2)) && !sw.noMfma;
    if (mfma) SP = 32 * NT;          // transposed matrices padded to the MFMA tile height
    if (sw.mfmaSerial) serialRatio = std::max(0, *sw.mfmaSerial);
    // serial / spine kernels exist for these shapes only (other category counts: level launches throughout)
    if (!((NT == 1 && (K == 1 || K == 2 || K == 4)) || (NT == 2 && (K == 1 || K == 2)))) serialRatio = 0;
    if (sw.reportDevice) {    // one line per instance: which physical GPU (multi-rank drivers collect them: bench.py mpi_mcmc)
        char bus[64] = "?";
        if (hipDeviceGetPCIBusId(bus, (int) sizeof bus, device) != hipSuccess) (void) hipGetLastError();
        std::fprintf(stderr, "[mbamd] instance on device %d pci %s mpi-rank %s\n", device, bus, sw.mpiRank.empty() ? "-" : sw.mpiRank.c_str());
    }
    partialsFloats = s4 ? (size_t) K * Ppad * 4 : (size_t) K * S * Ppad;
    matrixFloats = (size_t) K * SP * SP + (mfma ? (size_t) K * NT * T * 64 : 0);
    if (wg) {
        wgTabFloats = (size_t) K * SP * SP;
        matrixFloats = wgTabFloats + (size_t) K * wg_table_floats(S);
    }
    if (arena()) {
        int rc = configureWalk();
        if (rc) return rc;
    }
    // [U | U^-1 | lambda | V | b | side]: V = orthonormal eigenvectors kept for warm starts (k_eigen_reversible); b | side = the
    // imaginary parts and where each index's partner lies (complex_factor, mbamd_kernels.h: read on a complex instance only)
    eigenDoubles = eigen_imag_offset(S) + (size_t) 2 * S;
    partials.assign(nBuffers, nullptr);
    tipStates.assign(nBuffers, nullptr);
    valid.assign(nBuffers, 0);
    if (s4) {
        // everything up front, like the reference's InitChainCondLikes (src/mcmc.c:5756-5834): one arena per kind.  Partials
        // are BUFFER-major, [buffer][block][K][64]: the waves of a launch run the same program at about the same pace, so at any
        // moment they all write into one node's few MB -- a moving window like a fill -- instead of into a 1 KiB piece each of
        // regions 12 MB apart (block-major, rounds 1-3: the same kernel ran C4 in 0.65 to 0.84 ms depending on the box; with the
        // stores in one window 0.67 on a slow one, profiles/r03_exp_walk4_linear.txt).  Tips and exponents stay block-major.
        const size_t nb = (size_t) Ppad / 64;
        if ((size_t) nBuffers * nb * K >= ((size_t) 1 << 32)) return fail(BEAGLE_ERROR_OUT_OF_MEMORY, "beagleCreateInstance: more than 4 TiB of partials");   // (program entries hold KiB offsets in 32 bits)
        geom.pstride = (unsigned long) K * 64;
        geom.tstride = (unsigned) nBuffers * 4;
        geom.sstride = 64;
        const size_t pBytes = nb * (size_t) nBuffers * K * 64 * 16, tBytes = nb * geom.tstride * 8;
        HIP_TRY(hipMalloc(&arenaPartials, pBytes));
        HIP_TRY(hipMalloc(&arenaTips, tBytes));
        HIP_TRY(hipMemsetAsync(arenaPartials, 0, pBytes, stream));
        HIP_TRY(hipMemsetAsync(arenaTips, 0xFF, tBytes, stream));            // (a tip never set = all states compatible)
        unstored.assign((size_t) nBuffers, 0);
        recipes.assign((size_t) nBuffers, Recipe());
        if (sw.verbose)
            std::fprintf(stderr, "[mbamd] arenas: partials %p +%zu, tips %p +%zu\n", (void*) arenaPartials, pBytes, (void*) arenaTips, tBytes);
        for (int i = 0; i < nBuffers; ++i) partials[i] = arenaPartials + (size_t) i * nb * K * 64 * 4;
    }
    if (wg) {
        // the same for the 20/61-state tree walk (mbamd_walkg.h): tile-major arenas, one extra partials buffer per tile as
        // the sink of NOP entries; exponents in the 4-state path's format (two tiles per 64-pattern block)
        const size_t nt = (size_t) Ppad / MBAMD_WG_TW, tb = wg_block_bytes(S);
        wgTileBytes = (unsigned long) (nBuffers + 1) * K * tb;
        wgTipTileBytes = (unsigned) nBuffers * MBAMD_WG_TW;
        const size_t pBytes = nt * wgTileBytes, tBytes = nt * wgTipTileBytes;
        HIP_TRY(hipMalloc(&arenaPartials, pBytes));
        HIP_TRY(hipMalloc(&arenaTipStates, tBytes));
        HIP_TRY(hipMemsetAsync(arenaPartials, 0, pBytes, stream));
        HIP_TRY(hipMemsetAsync(arenaTipStates, S, tBytes, stream));           // (a tip never set = missing data)
        if (sw.verbose)
            std::fprintf(stderr, "[mbamd] arenas: partials +%zu, tips +%zu bytes\n", pBytes, tBytes);
        for (int i = 0; i < nBuffers; ++i) partials[i] = arenaPartials + (size_t) i * K * tb / 4;
    }
    // The scale buffers; arena layouts: their exponent arena, zeroed behind the other two, with scratch rows behind the buffers of a block:
    // sinks of entries that record no exponents, in rotation (an exponent byte is stored with every entry -- a conditional store would make the
    // compiler's counted waits stricter -- and all of them storing to ONE row cost a SCALE_READ evaluation 29 % at 20 states, profiles/r06_scale_read.txt)
    { int rc = scales.create(stream, &stage, K, Ppad, std::max(nScale, 1), s4 ? MBAMD_W4_SCRATCH_ROWS : MBAMD_WG_SCRATCH_ROWS, arena()); if (rc) return rc; }
    if (arena() && sw.verbose) std::fprintf(stderr, "[mbamd] arenas: exponents %p +%zu\n", (void*) scales.nodeExponents(), (size_t) Ppad / 64 * scales.blockStride());

    HIP_TRY(hipMalloc(&matrices, std::max<size_t>(1, (size_t) nMatrices * matrixFloats) * sizeof(float)));
    HIP_TRY(hipMemsetAsync(matrices, 0, std::max<size_t>(1, (size_t) nMatrices * matrixFloats) * sizeof(float), stream));
    if (wg && nMatrices > 0) {                   // the constant "missing data" column of every gather table
        const int total = nMatrices * K * S;
        MBAMD_LAUNCH(k_wg_init_tables, (unsigned) ((total + 255) / 256), 256, 0, stream, matrices, matrixFloats, wgTabFloats, S, K, total);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMalloc(&d_eigen, std::max<size_t>(1, (size_t) nEigen * eigenDoubles) * sizeof(double)));
    // (a complex instance's kernels index U with `side`: an eigen buffer never set must not send them out of the buffer)
    if (complexEigen) HIP_TRY(hipMemsetAsync(d_eigen, 0, std::max<size_t>(1, (size_t) nEigen * eigenDoubles) * sizeof(double), stream));
    HIP_TRY(hipMalloc(&d_freqs, std::max<size_t>(1, (size_t) nEigen * S) * sizeof(double)));
    HIP_TRY(hipMalloc(&d_weights, std::max<size_t>(1, (size_t) nEigen * K) * sizeof(double)));
    HIP_TRY(hipMalloc(&d_rates, (size_t) K * sizeof(double)));
    HIP_TRY(hipMalloc(&d_pweights, (size_t) Ppad * sizeof(double)));
    HIP_TRY(hipMalloc(&d_site, (size_t) Ppad * sizeof(double)));
    nblocks = Ppad / 64;
    if (!s4 && S >= 8) nblocks = Ppad / 32;      // k_integrate_lnl_wide: one block sum per 32-pattern tile
    if (wg) nblocks = Ppad / MBAMD_INTEGRATE_WG_PATTERNS;      // the tree-walk layout's integration kernel, whatever the state count
    HIP_TRY(hipHostMalloc(&h_sums, (size_t) nblocks * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipHostGetDevicePointer((void**) &h_sums_dev, h_sums, 0));
    wait.create(!sw.noPoll);
    { int rc = stage.create((size_t) 8 << 20, 64); if (rc) return rc; }

    // defaults: unit rates, uniform category weights, unit pattern weights (BEAGLE clients normally set them)
    std::vector<double> ones(std::max(Ppad, K), 1.0);
    HIP_TRY(hipMemcpy(d_rates, ones.data(), (size_t) K * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> pw(Ppad, 0.0);
    std::fill(pw.begin(), pw.begin() + P, 1.0);
    HIP_TRY(hipMemcpy(d_pweights, pw.data(), (size_t) Ppad * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> w((size_t) std::max(1, nEigen) * K, 1.0 / K);
    HIP_TRY(hipMemcpy(d_weights, w.data(), (size_t) nEigen * K * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(stream));
    return BEAGLE_SUCCESS;
}

// synchronise, free the device memory, destroy the stream
inline Instance::~Instance()
{
    (void) hipSetDevice(device);
    (void) hipStreamSynchronize(stream);
    if (arena()) {
        void* arenas[] = {arenaPartials, arenaTips, arenaTipStates};
        for (void* a : arenas) if (a) (void) hipFree(a);
    } else {
        for (float* p : partials) if (p) (void) hipFree(p);
        for (uint8_t* p : tipStates) if (p) (void) hipFree(p);
    }
    pending.clear();
    wgOps.clear(); wgListStart.clear(); wgListCum.clear();
    for (Plan* pl : plans) { if (pl->d_table) (void) hipFree(pl->d_table); delete pl; }
    plans.clear();
    void* bufs[] = {matrices, d_eigen, d_freqs, d_weights, d_rates, d_pweights, d_site,
                    d_ev, d_tmp, d_trace, d_q, d_preTable, d_snap, d_storeProg};
    for (void* b : bufs) if (b) (void) hipFree(b);
    if (h_sums) (void) hipHostFree(h_sums);
    wait.destroy();
    if (h_site) (void) hipHostFree(h_site);
    if (h_deriv) (void) hipHostFree(h_deriv);
    stage.destroy();
    for (auto& ev : events) { (void) hipEventDestroy(ev.first); (void) hipEventDestroy(ev.second); }
    for (auto& ev : spans) { (void) hipEventDestroy(ev.first); (void) hipEventDestroy(ev.second); }
    if (spanOpen) (void) hipEventDestroy(spanEv0);
    if (reduceEvent) (void) hipEventDestroy(reduceEvent);
    for (auto& kv : finalExpOwn) if (kv.second) (void) hipFree(kv.second);
    (void) hipStreamDestroy(stream);
}

// ---------------------------------------------------------------------------------------------
// Tree-walk geometry.  The grid is (pattern blocks) x (categories) workgroups of W waves; each wave owns `slots` LDS
// slots of 1 KiB.  W and the slot count are chosen so that the whole grid is resident at once when the chip allows it:
// few blocks -> more tree parallelism per block, many blocks -> single-wave workgroups with deep slot stacks.
#define MBAMD_W4_PLAIN_WAVES_PER_CU 32    // eight waves per SIMD: beyond that the grid is not resident
#define MBAMD_W4_PLAIN_MAXW 4            // (the sweep's largest)
// microseconds per entry and wave of the plain 4-state loop against the waves resident on a CU: measured on the MI355X at DNA 500 x
// 20 000 and 1000 x 50 000, W = 1 ... 4 (profiles/walk4_plain_waves.txt section 3), linear between the points and beyond the last
static inline double walk4_entry_us(double wavesPerCU)
{
    static const double x[] = {4.9, 9.8, 12.2, 14.7, 19.6, 24.4}, y[] = {0.354, 0.395, 0.428, 0.485, 0.542, 0.747};
    if (wavesPerCU <= x[0]) return y[0];
    int i = 1;
    while (i < 5 && wavesPerCU > x[i]) ++i;
    return y[i - 1] + (y[i] - y[i - 1]) * (wavesPerCU - x[i - 1]) / (x[i] - x[i - 1]);
}
inline int Instance::configureWalk()
{
    int numCU = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) numCU = prop.multiProcessorCount;
    const int maxLds = 160 * 1024;
    if (s4 && (hipFuncSetAttribute((const void*) k_walk4_t<Walk4Args>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
               hipFuncSetAttribute((const void*) k_walk4_t<Walk4Args, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
               hipFuncSetAttribute((const void*) k_walk4_t<Walk4Args, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
               hipFuncSetAttribute((const void*) k_walk4_t<Walk4ArgsInline>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess))
        (void) hipGetLastError();
    if (wg) {
        // one wave = (32-pattern tile, category); registers bound the residency: 20 states 4 waves per SIMD, 61 states 2
        const unsigned slotBytes = wg_block_bytes(S);
        MBAMD_WG_DISPATCH(S, raise_walkg_lds, maxLds);
        wgGeometry(1, w4.maxW, w4.maxSlots);
        w4.maxSlots1 = w4.maxSlots;
        if (!sw.walkWaves && !sw.maxLdsSlots) {   // a single-wave program may use the LDS of the whole workgroup
            const long wgsG = (long) (Ppad / MBAMD_WG_TW) * K;
            const int perCUG = (int) std::max(1L, (wgsG + numCU - 1) / numCU);
            w4.maxSlots1 = std::max(w4.maxSlots, std::min(24, (int) (((160 * 1024) / std::min(perCUG, 32) - 64 - MBAMD_WG_STAGE) / (int) slotBytes)));
        }
        w4.memSlots = false;
        w4.leadNops = MBAMD_WG_LEAD; w4.unroll = 3; w4.tailNops = MBAMD_WG_TAIL;
        w4.prefetchDistance = 0;
        if (sw.walkSmallPhase) w4.smallPhase = std::max(1, *sw.walkSmallPhase);
        if (sw.verbose) std::fprintf(stderr, "[mbamd] tree walk (%d states): %ld workgroups, up to %d waves x %d slots of %u bytes\n",
                                     S, (long) (Ppad / MBAMD_WG_TW) * K, w4.maxW, w4.maxSlots, slotBytes);
        return BEAGLE_SUCCESS;
    }
    const long wgs = (long) (Ppad / 64) * K;
    const int perCU = (int) std::max(1L, (wgs + numCU - 1) / numCU);          // workgroups a CU must host for full residency
    const int ldsPerWG = (160 * 1024) / std::min(perCU, 32) - 64;
    auto slotsFor = [&](int W) { return (ldsPerWG / W - MBAMD_W4_STAGE) / 1024; };
    // measured (profiles/): about 12-15 waves per CU (3-4 per SIMD) is the sweet spot -- fewer leave the scalar-load
    // latency uncovered, more cost LDS (slots) and tree-partition efficiency (phases, padding) without buying anything.
    // (Round 6, profiles/r06_walk4_waves.txt: DNA 500 x 20 000 = 4.9 workgroups per CU ran two waves each until then; with three
    //  -- 15 waves per CU, 190 entries per wave instead of 264 -- the evaluation takes 0.158-0.164 ms instead of 0.181; four: 0.192.)
    int W = (int) std::max(1L, std::min((long) MBAMD_W4_MAXW, (14L * numCU + wgs / 2) / wgs));
    while (W > 1 && slotsFor(W) < 7) --W;
    if (sw.walkWaves) W = std::max(1, std::min(MBAMD_W4_MAXW, *sw.walkWaves));
    int slots = std::max(3, std::min(48, slotsFor(W)));
    if (sw.maxLdsSlots) slots = std::max(3, std::min(150 / W, *sw.maxLdsSlots));
    w4.maxW = W;
    w4.maxSlots = slots;
    w4.maxSlots1 = sw.maxLdsSlots ? slots : std::max(slots, std::min(40, slotsFor(1)));
    if (sw.walkPrefetch) w4.prefetchDistance = std::max(0, *sw.walkPrefetch);
    w4.forward = true;
    w4.safeWaits = sw.walkSafe;
    if (sw.walkSmallPhase) w4.smallPhase = std::max(1, *sw.walkSmallPhase);
    // Whole-tree lists on the plain loop (Walk4Builder::plainWaves) have a geometry of their own.  Their time is one wave's serial chain
    // of entries, each with an exposed scalar-load round trip: more waves per workgroup shorten the chain, but every wave more on a CU
    // makes an entry slower (at 24 waves per CU 1.7 times what it is at 12), and the whole grid must stay resident.  The LDS of a
    // workgroup's share of the CU is ONE pool of slots, nothing in front of them; a list that does not fit it without an eviction, or
    // whose cut does not win against one wave, is tried on fewer waves and then gets the geometry above.
    // How many: the measured time per entry and wave against the waves on a CU (profiles/walk4_plain_waves.txt section 3) says what W
    // waves of n / W entries would take; the W with the least, and per W the longest wave that still beats one wave by 5 %.
    {
        const double wpc = (double) wgs / numCU;
        double bestTime = walk4_entry_us(wpc);
        w4.plainWaves = 1;
        for (int w = 2; w <= MBAMD_W4_PLAIN_MAXW; ++w) {
            w4.plainShare[w] = (int) (1024.0 * 0.95 * walk4_entry_us(wpc) / walk4_entry_us(wpc * w));
            if (perCU * w > MBAMD_W4_PLAIN_WAVES_PER_CU) continue;                 // (the whole grid resident)
            const double tw = walk4_entry_us(wpc * w) / w;
            if (tw < bestTime) { bestTime = tw; w4.plainWaves = w; }
        }
        w4.plainDescend = !sw.walkWaves;
    }
    if (sw.walkWaves) w4.plainWaves = W;
    if (sw.noPlainWalk) w4.plainWaves = 0;
    // (a sixteenth of the share kept back: 12 slots of the 12.2 KiB that 13 workgroups per CU leave each ran as 12 workgroups per CU and
    //  a second round, profiles/walk4_plain_waves.txt; forced: the pool is that many)
    w4.plainSlots = std::min(250, sw.maxLdsSlots ? slots : (ldsPerWG - ldsPerWG / 16) / 1024);
    if (sw.walkPlainMinOps) w4.plainMinOps = std::max(1, *sw.walkPlainMinOps);
    if (sw.verbose) std::fprintf(stderr, "[mbamd] tree walk: %ld workgroups (%d per CU), up to %d waves x %d slots\n", wgs, perCU, W, slots);
    return BEAGLE_SUCCESS;
}

// 20/61-state walk: waves per workgroup and LDS slots per wave for (tiles x categories x lists) workgroups.  Waves per
// workgroup are a power of two (two-wave workgroups are launched as four, see k_walkg; three or five leave SIMDs idle).
inline void Instance::wgGeometry(int lists, int& W, int& slots) const
{
    int numCU = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) numCU = prop.multiProcessorCount;
    // registers bound the residency: 4 (20 states) / 2 (61 states) waves per SIMD
    const int maxW = S > 32 ? 4 : 8, wavesPerCU = S > 32 ? 6 : 12;
    const int slotBytes = (int) wg_block_bytes(S);
    const long wgs = (long) (Ppad / MBAMD_WG_TW) * K * lists;
    const int perCU = (int) std::max(1L, (wgs + numCU - 1) / numCU);
    const int ldsPerWG = (160 * 1024) / std::min(perCU, 32) - 64;
    auto slotsFor = [&](int w) { return (ldsPerWG / w - MBAMD_WG_STAGE) / slotBytes; };
    long want = std::max(1L, std::min((long) maxW, ((long) wavesPerCU * numCU + wgs / 2) / wgs));
    W = 1;
    while (W * 2 <= want) W *= 2;
    while (W > 1 && slotsFor(W) < 4) W /= 2;
    if (sw.walkWaves) W = std::max(1, std::min(maxW, *sw.walkWaves));
    slots = std::max(3, std::min(24, slotsFor(W)));
    if (sw.maxLdsSlots) slots = std::max(1, std::min((160 * 1024 / W - MBAMD_WG_STAGE) / slotBytes, *sw.maxLdsSlots));
}

// 4-state path: one tip's state masks (bit i = state i compatible) -> four 64-bit bitplanes per pattern block
inline int Instance::setTipMasks(int tip, const std::vector<uint8_t>& h)
{
    const size_t nb = (size_t) Ppad / 64;
    std::vector<uint64_t> planes(nb * 4, 0);
    for (int c = 0; c < Ppad; ++c)
        for (int i = 0; i < 4; ++i)
            if (h[c] >> i & 1u) planes[(size_t) (c >> 6) * 4 + i] |= (uint64_t) 1 << (c & 63);
    if (nUnstored) {                             // recipes that read this tip are made first; whatever the buffer held is gone
        const int src = storeUsersOfTip(tip);
        if (src) return src;
        dropRecipe(tip);
    }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy2D(arenaTips + (size_t) tip * 4, (size_t) geom.tstride * 8, planes.data(), 32, 32, nb, hipMemcpyHostToDevice));
    if (!tipStates[tip]) layoutEpoch++;
    tipStates[tip] = reinterpret_cast<uint8_t*>(arenaTips + (size_t) tip * 4);
    return BEAGLE_SUCCESS;
}

inline int Instance::setTipStates(int tip, const int* states)
{
    if (tip < 0 || tip >= nBuffers) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetTipStates: tip index");
    clearPreOrder(tip);
    std::vector<uint8_t> h(Ppad, (uint8_t) S);
    for (int c = 0; c < P; ++c) h[c] = (uint8_t) ((states[c] < 0 || states[c] >= S) ? S : states[c]);
    if (s4) {
        for (int c = 0; c < Ppad; ++c) h[c] = (uint8_t) (h[c] >= 4 ? 0xF : 1u << h[c]);   // state masks (mbamd_walk4.h)
        return setTipMasks(tip, h);
    }
    if (wg) {                                    // 32 state codes per (tile, tip) in the tip arena
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy2D(arenaTipStates + (size_t) tip * MBAMD_WG_TW, (size_t) wgTipTileBytes, h.data(), MBAMD_WG_TW, MBAMD_WG_TW, (size_t) Ppad / MBAMD_WG_TW, hipMemcpyHostToDevice));
        if (!tipStates[tip]) layoutEpoch++;
        tipStates[tip] = arenaTipStates + (size_t) tip * MBAMD_WG_TW;
        return BEAGLE_SUCCESS;
    }
    if (!tipStates[tip]) { HIP_TRY(hipMalloc(&tipStates[tip], (size_t) Ppad)); layoutEpoch++; }
    return upload(tipStates[tip], h.data(), (size_t) Ppad);
}

inline int Instance::importPartials(int idx, const double* in, bool hasCategories)
{
    if (idx < 0 || idx >= nBuffers) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "partials buffer index");
    if (idx < (int) finalExpOf.size()) finalExpOf[idx] = nullptr;
    clearPreOrder(idx);
    wgForget(idx);
    if (s4 && !hasCategories) {
        // beagleSetTipPartials with 0/1 entries (IUPAC ambiguity codes, reference src/mbbeagle.c:150-166): a state mask
        // per pattern says the same thing in one byte, and the tree walk reads it like any compact tip
        std::vector<uint8_t> h(Ppad, 0xF);
        bool binary = true;
        for (int c = 0; c < P && binary; ++c) {
            unsigned m = 0;
            for (int i = 0; i < 4; ++i) {
                const double v = in[(size_t) c * 4 + i];
                if (v == 1.0) m |= 1u << i;
                else if (v != 0.0) binary = false;
            }
            h[c] = (uint8_t) m;
        }
        if (binary) return setTipMasks(idx, h);
    }
    int rc = ensurePartials(idx);
    if (rc) return rc;
    if (nUnstored) {                             // (a tip that switches to partials form: its recipes are made first)
        rc = storeUsersOfTip(idx);
        if (rc) return rc;
        dropRecipe(idx);
    }
    const size_t nIn = (size_t) (hasCategories ? K : 1) * P * S;
    rc = grow(&d_tmp, &tmpCap, nIn * sizeof(double));
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(d_tmp, in, nIn * sizeof(double), hipMemcpyHostToDevice));
    const size_t total = (size_t) K * P * S;
    const unsigned blocks = (unsigned) ((total + 255) / 256);
    withLayout([&](auto tag) { MBAMD_LAUNCH(k_import_partials<decltype(tag)::value>, blocks, 256, 0, stream, (const double*) d_tmp, hasCategories ? 1 : 0, S, K, P, Ppad, strides().partials, partials[idx]); });
    HIP_TRY(hipGetLastError());
    valid[idx] = 1;
    if (tipStates[idx]) {                        // a tip switches from compact to partials form
        HIP_TRY(hipStreamSynchronize(stream));
        if (!arena()) (void) hipFree(tipStates[idx]);
        tipStates[idx] = nullptr;
        layoutEpoch++;
    }
    return BEAGLE_SUCCESS;
}

inline int Instance::getPartials(int idx, double* out)
{
    if (idx < 0 || idx >= nBuffers || !valid[idx]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleGetPartials: buffer");
    const size_t total = (size_t) K * P * S;
    int rc = grow(&d_tmp, &tmpCap, total * sizeof(double));
    if (rc) return rc;
    rc = ensureStored(idx);
    if (rc) return rc;
    const unsigned blocks = (unsigned) ((total + 255) / 256);
    withLayout([&](auto tag) { MBAMD_LAUNCH(k_export_partials<decltype(tag)::value>, blocks, 256, 0, stream, (const float*) partials[idx], S, K, P, Ppad, strides().partials, (double*) d_tmp); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(out, d_tmp, total * sizeof(double), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}

// Eigen-systems from rate matrices (or exchangeabilities), computed on the device: k_eigen_reversible (mbamd_kernels.h).
// Nothing here waits for the device: the rate matrices travel through the pinned ring and are read by the kernel from there.
inline int Instance::setRateMatrices(int first, int count, const double* q, const double* pi, int mode, int warmFirst)
{
    if (count <= 0) return BEAGLE_SUCCESS;
    if (first < 0 || first + count > nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdSetRateMatrices: eigen index");
    if (warmFirst >= 0 && warmFirst + count > nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdSetRateMatricesFrom: warm-start eigen index");
    // (a block reads its source's V before it writes its own: the same range is fine, a shifted overlap would read a buffer a
    //  neighbouring block of the same launch is writing)
    if (warmFirst >= 0 && warmFirst != first && warmFirst < first + count && first < warmFirst + count)
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdSetRateMatricesFrom: the warm-start range overlaps the destination range with a shift");
    if (S > 64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdSetRateMatrices: more than 64 states");
    for (int i = 0; i < S; ++i)
        if (!(pi[i] > 0.0)) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdSetRateMatrices: a state frequency is not positive (no symmetric form)");
    if (eigenWarm.size() != (size_t) nEigen) { eigenWarm.assign(nEigen, -1); eigenShield.assign(nEigen, 0); }
    const size_t qd = (size_t) count * S * S, bytes = (qd + S) * sizeof(double);
    const double* dq = nullptr;
    std::vector<double> h(qd + S);
    std::memcpy(h.data(), q, qd * sizeof(double));
    std::memcpy(h.data() + qd, pi, (size_t) S * sizeof(double));
    int rc;
    if (bytes + 64 <= stage.capacity() / 2) {
        rc = stageDirect(h.data(), bytes, (const void**) &dq);
        if (rc) return rc;
    } else {                                                       // (many large matrices at once: a device copy)
        rc = grow(&d_tmp, &tmpCap, bytes);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(stream));                     // (d_tmp may still be read by an earlier import)
        HIP_TRY(hipMemcpy(d_tmp, h.data(), bytes, hipMemcpyHostToDevice));
        dq = reinterpret_cast<const double*>(d_tmp);
    }
    std::vector<EigenJob> jobs(count);
    for (int i = 0; i < count; ++i) {
        jobs[i].q = dq + (size_t) i * S * S;
        jobs[i].pi = dq + qd;
        jobs[i].out = d_eigen + (size_t) (first + i) * eigenDoubles;
        jobs[i].warm = nullptr;
        // a warm start re-uses the orthonormal basis of the source; every 64th call starts cold again (rounding drift of the basis)
        if (warmFirst >= 0 && eigenWarm[warmFirst + i] >= 0 && eigenWarm[warmFirst + i] < 64)
            jobs[i].warm = d_eigen + (size_t) (warmFirst + i) * eigenDoubles + (size_t) 2 * S * S + S;
        jobs[i].mode = mode & 1;
        jobs[i].pad_ = 0;
    }
    std::vector<int> warmAfter(count);
    for (int i = 0; i < count; ++i) warmAfter[i] = jobs[i].warm ? eigenWarm[warmFirst + i] + 1 : 0;
    const EigenJob* djobs = nullptr;
    rc = stageDirect(jobs.data(), sizeof(EigenJob) * count, (const void**) &djobs);
    if (rc) return rc;
    static std::vector<char> ldsRaised(64, 0);                      // per device: the attribute belongs to the device's code object
    if (device >= 0 && device < (int) ldsRaised.size() && !ldsRaised[device]) {
        if (hipFuncSetAttribute((const void*) k_eigen_reversible<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
            hipFuncSetAttribute((const void*) k_eigen_reversible<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void) hipGetLastError();
        ldsRaised[device] = 1;
    }
    // (beyond 32 states a step's 2 x 2 blocks are spread over 1 024 threads: four waves per SIMD hide the LDS round trips of a Jacobi step)
    if (S > 32 && !sw.eigen256)
        MBAMD_LAUNCH_BARRIER(k_eigen_reversible<32>, (unsigned) count, 1024, eigen_lds_doubles(S) * sizeof(double), stream, djobs, S, 30);
    else
        MBAMD_LAUNCH_BARRIER(k_eigen_reversible<8>, (unsigned) count, 256, eigen_lds_doubles(S) * sizeof(double), stream, djobs, S, 30);
    HIP_TRY(hipGetLastError());
    if (complexEigen)                                               // the systems of a reversible matrix are real: b = 0, side = 0
        for (int i = 0; i < count; ++i)
            HIP_TRY(hipMemsetAsync(d_eigen + (size_t) (first + i) * eigenDoubles + eigen_imag_offset(S), 0, (size_t) 2 * S * sizeof(double), stream));
    // bookkeeping only once the launch is in the stream: a failure above leaves the buffers "cold" and unshielded
    for (int i = 0; i < count; ++i) {
        eigenWarm[first + i] = warmAfter[i];
        eigenShield[first + i] = (mode & 2) ? 1 : 0;                // (a rewrite without the shield bit clears a stale shield)
    }
    return BEAGLE_SUCCESS;
}

inline int Instance::setEigen(int idx, const double* U, const double* Ui, const double* lam)
{
    if (idx < 0 || idx >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetEigenDecomposition: eigen index");
    if (eigenShield.size() == (size_t) nEigen && eigenShield[idx]) {     // the device computed this one (mbamdSetRateMatricesFrom, mode bit 1)
        eigenShield[idx] = 0;
        return BEAGLE_SUCCESS;
    }
    if (eigenWarm.size() == (size_t) nEigen) eigenWarm[idx] = -1;
    // (a complex instance: `lam` holds 2 S values, the whole buffer travels -- V, which no longer belongs to it, as zeros)
    std::vector<double> h(complexEigen ? eigenDoubles : (size_t) 2 * S * S + S, 0.0);
    std::memcpy(h.data(), U, sizeof(double) * S * S);
    std::memcpy(h.data() + (size_t) S * S, Ui, sizeof(double) * S * S);
    std::memcpy(h.data() + (size_t) 2 * S * S, lam, sizeof(double) * S);
    if (complexEigen) {
        double* im = h.data() + eigen_imag_offset(S);
        std::memcpy(im, lam + S, sizeof(double) * S);
        if (!eigen_pairs(lam, im, S, im + S))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetEigenDecomposition: an imaginary part without its adjacent conjugate, or a non-finite eigenvalue");
    }
    return upload(d_eigen + (size_t) idx * eigenDoubles, h.data(), h.size() * sizeof(double));
}

// The doubles of an eigen buffer as the matrix kernels read them: [U | U^-1 | lambda]; V (optional) only where the device solver wrote
// the buffer last -- after beagleSetEigenDecomposition the basis there belongs to no system.
inline int Instance::getEigen(int idx, double* U, double* Ui, double* lam, double* V)
{
    if (idx < 0 || idx >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetEigenDecomposition: eigen index");
    if (V && (eigenWarm.size() != (size_t) nEigen || eigenWarm[idx] < 0))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetEigenDecomposition: the device solver did not write this buffer, it holds no orthonormal basis");
    const size_t SS = (size_t) S * S;
    std::vector<double> h(2 * SS + S + (V ? SS : 0));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(h.data(), d_eigen + (size_t) idx * eigenDoubles, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(U, h.data(), SS * sizeof(double));
    std::memcpy(Ui, h.data() + SS, SS * sizeof(double));
    std::memcpy(lam, h.data() + 2 * SS, (size_t) S * sizeof(double));
    if (V) std::memcpy(V, h.data() + 2 * SS + S, SS * sizeof(double));
    return BEAGLE_SUCCESS;
}

// beagleUpdateTransitionMatrices only queues its jobs: MrBayes calls it once per eigen-system part (reference
// src/mbbeagle.c:1475-1486), and all parts of an evaluation go out as ONE launch when the next other call arrives.
inline int Instance::setRates(int index, const double* r) { return rateSets.set(index, r, K); }

inline int Instance::updateMatrices(int eigenIndex, const int* probIdx, const double* lengths, int count, int rateSet,
                                    const int* d1Idx, const int* d2Idx)
{
    if (!rateSets.has(rateSet)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: category rates index");
    if (!pendingJobs.empty() && rateSet != pendingRateSet) {       // one rate set per launch
        int frc = flushMatrices();
        if (frc) return frc;
    }
    pendingRateSet = rateSet;
    if (eigenIndex < 0 || eigenIndex >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: eigen index");
    if (count <= 0) return BEAGLE_SUCCESS;
    if (K > MBAMD_MAX_RATES) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "more than 16 rate categories");
    // the outputs of the call: probabilities, then the first / second derivative matrices where asked for (order 1 / 2 jobs)
    const int* const outIdx[3] = {probIdx, d1Idx, d2Idx};
    for (int o = 0; o < 3; ++o)
        for (int i = 0; outIdx[o] && i < count; ++i)
            if (outIdx[o][i] < 0 || outIdx[o][i] >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: matrix index");
    if (pendingMatrixOut.size() != (size_t) nMatrices) pendingMatrixOut.assign(nMatrices, 0);
    if (d1Idx || d2Idx) {                        // a derivative matrix on top of another output of the same call
        std::vector<char> seen((size_t) nMatrices, 0);
        for (int o = 0; o < 3; ++o)
            for (int i = 0; outIdx[o] && i < count; ++i) {
                if (o > 0 && seen[outIdx[o][i]]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: a derivative index equals another output of the call");
                seen[outIdx[o][i]] = 1;
            }
    }
    bool clash = false;
    size_t njobs = 0;
    for (int o = 0; o < 3; ++o) {
        if (!outIdx[o]) continue;
        njobs += (size_t) count;
        for (int i = 0; i < count && !clash; ++i) clash = pendingMatrixOut[outIdx[o][i]] != 0;
    }
    if (clash || (pendingJobs.size() + njobs) * sizeof(MatrixJob) > stage.capacity() / 4) {
        int rc = flushMatrices();
        if (rc) return rc;
    }
    const double* eig = d_eigen + (size_t) eigenIndex * eigenDoubles;
    for (int o = 0; o < 3; ++o)
        for (int i = 0; outIdx[o] && i < count; ++i) {
            MatrixJob j;
            j.out = matrixPtr(outIdx[o][i]);
            j.length = lengths[i];
            j.eig = eig;
            j.pad_ = (double) o;                 // the derivative order: flushMatrices launches per order
            pendingJobs.push_back(j);
            pendingMatrixOut[outIdx[o][i]] = 1;
        }
    // four states (one call per evaluation): the matrix kernel is launched here, so that it runs while MrBayes assembles the
    // operation list (+2 % on both chains, profiles/r06_scale_read.txt)
    if (s4) return flushMatrices();
    return BEAGLE_SUCCESS;
}

inline int Instance::flushMatrices()
{
    if (pendingJobs.empty()) return BEAGLE_SUCCESS;
    if (snapPlan) { int src = flushSnapshot(); if (src) return src; }     // (the matrices a recipe needs are copied before any is overwritten)
    { int src = spanBegin(); if (src) return src; }
    // one launch per derivative order (MatrixJob::pad_ holds a job's order: 0 -- all there is on MrBayes' path -- 1 or 2)
    bool derivatives = false;
    for (const MatrixJob& j : pendingJobs) derivatives = derivatives || j.pad_ != 0.0;
    int rc = BEAGLE_SUCCESS;
    if (!derivatives) {
        rc = launchMatrices<0>(pendingJobs.data(), (int) pendingJobs.size());
    } else {
        std::vector<MatrixJob> byOrder[3];
        for (MatrixJob j : pendingJobs) {
            const int order = j.pad_ == 1.0 ? 1 : (j.pad_ == 2.0 ? 2 : 0);
            j.pad_ = 0.0;
            byOrder[order].push_back(j);
        }
        if (!byOrder[0].empty()) rc = launchMatrices<0>(byOrder[0].data(), (int) byOrder[0].size());
        if (rc == BEAGLE_SUCCESS && !byOrder[1].empty()) rc = launchMatrices<1>(byOrder[1].data(), (int) byOrder[1].size());
        if (rc == BEAGLE_SUCCESS && !byOrder[2].empty()) rc = launchMatrices<2>(byOrder[2].data(), (int) byOrder[2].size());
    }
    pendingJobs.clear();
    std::fill(pendingMatrixOut.begin(), pendingMatrixOut.end(), 0);
    return rc;
}

// the transition-matrix launch of `count` jobs of one derivative ORDER (0: the probabilities), whichever kernel the layout takes;
// CX: the kernels' form for complex eigen-systems (mbamd_kernels.h), which a complex instance takes -- chosen here, on the host
template <int ORDER, bool CX>
inline int Instance::launchMatrices(const MatrixJob* jobs, int count)
{
    if constexpr (!CX) {
        if (complexEigen) return launchMatrices<ORDER, true>(jobs, count);
    }
    const RatesArg rates = rateSets[pendingRateSet];
    if (s4 && count <= MBAMD_S4_INLINE_JOBS && count * K <= 64) {
        // a branch move's one or two matrices: the jobs in the kernel arguments (mbamd_kernels.h)
        MatrixJobs4 ja;
        std::memset(&ja, 0, sizeof ja);
        std::memcpy(ja.j, jobs, sizeof(MatrixJob) * count);
        MBAMD_LAUNCH((k_transition_matrices_s4_inline<ORDER, CX>), 1u, 64, 0, stream, ja, rates, K, count * K);
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    const MatrixJob* djobs = nullptr;
    int rc = stageDirect(jobs, sizeof(MatrixJob) * count, (const void**) &djobs);
    if (rc) return rc;
    if (s4) {
        const int total = count * K;
        MBAMD_LAUNCH((k_transition_matrices_s4<ORDER, CX>), (unsigned) ((total + 255) / 256), 256, 0, stream, djobs, rates, K, total);
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    if (S > 8 && S <= 64) {                       // fp64 matrix cores, one wave per 16 rows
        const unsigned grid = (unsigned) (count * K);
        const int packedT = mfma ? T : 0;
        const size_t wgTab = wg ? wgTabFloats : 0;
        auto k1 = k_transition_matrices_mfma<1, ORDER, CX>;
        auto k2 = k_transition_matrices_mfma<2, ORDER, CX>;
        auto k3 = k_transition_matrices_mfma<3, ORDER, CX>;
        auto k4 = k_transition_matrices_mfma<4, ORDER, CX>;
        switch ((S + 15) / 16) {
            case 1: MBAMD_LAUNCH_BARRIER(k1, grid, 64, 0, stream, djobs, rates, S, SP, K, packedT, wgTab); break;
            case 2: MBAMD_LAUNCH_BARRIER(k2, grid, 128, 0, stream, djobs, rates, S, SP, K, packedT, wgTab); break;
            case 3: MBAMD_LAUNCH_BARRIER(k3, grid, 192, 0, stream, djobs, rates, S, SP, K, packedT, wgTab); break;
            default: MBAMD_LAUNCH_BARRIER(k4, grid, 256, 0, stream, djobs, rates, S, SP, K, packedT, wgTab); break;
        }
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    const int threads = std::min(256, round_up(S * S, 64));
    const double* evs = nullptr;                 // up to 64 states the matrix kernel forms the exponentials itself
    if (S > 64) {
        const size_t nev = (size_t) count * K * S;
        rc = grow((void**) &d_ev, &evCap, (CX ? 2 : 1) * nev * sizeof(double));
        if (rc) return rc;
        MBAMD_LAUNCH((k_eigen_exponentials<ORDER, CX>), (unsigned) ((nev + 255) / 256), 256, 0, stream, djobs, rates, S, K, (int) nev, d_ev);
        evs = d_ev;
    }
    MBAMD_LAUNCH_BARRIER((k_transition_matrices_ev<ORDER, CX>), (unsigned) (count * K), threads, 0, stream, djobs, evs, rates, S, SP, K, 1,
                         mfma ? T : 0, wg ? wgTabFloats : (size_t) 0);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

inline void Instance::matrixImage(const double* in, float* h) const
{
    std::fill(h, h + matrixFloats, 0.0f);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const float v = (float) in[((size_t) k * S + i) * S + j];
                h[(size_t) k * SP * SP + (size_t) j * SP + i] = v;
                if (mfma)
                    h[(size_t) K * SP * SP + ((size_t) (k * NT + i / 32) * T + j / 2) * 64 + (i % 32) + 32 * (j % 2)] = v;
                if (wg) wg_table_put(h + wgTabFloats + (size_t) k * wg_table_floats(S), S, i, j, v);
            }
    if (wg)
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < S; ++i) wg_table_put_missing(h + wgTabFloats + (size_t) k * wg_table_floats(S), S, i);
}
inline int Instance::setMatrix(int idx, const double* in)
{
    if (idx < 0 || idx >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetTransitionMatrix: matrix index");
    if (snapPlan) { int src = flushSnapshot(); if (src) return src; }
    std::vector<float> h(matrixFloats);
    matrixImage(in, h.data());
    return upload(matrixPtr(idx), h.data(), matrixFloats * sizeof(float));
}
inline int Instance::convolveMatrices(const int* first, const int* second, const int* result, int count)
{
    return matrix_list_run(*this, "beagleConvolveTransitionMatrices", true, first, second, result, count);
}
inline int Instance::transposeMatrices(const int* input, const int* result, int count)
{
    return matrix_list_run(*this, "beagleTransposeTransitionMatrices", false, input, (const int*) nullptr, result, count);
}
inline int Instance::setMatrices(const int* idx, const double* in, int count) { return matrix_list_set(*this, "beagleSetTransitionMatrices", idx, in, count); }
inline int Instance::updateMatricesFromRateMatrix(const double* q, const int* prob, const int* d1, const int* d2, const double* lengths, int count)
{
    return rate_exponential_run(*this, "mbamdUpdateTransitionMatricesFromRateMatrix", q, prob, d1, d2, lengths, count);
}

inline int Instance::getMatrix(int idx, double* out)
{
    if (idx < 0 || idx >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleGetTransitionMatrix: matrix index");
    std::vector<float> h(matrixFloats);
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(h.data(), matrixPtr(idx), matrixFloats * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j)
                out[((size_t) k * S + i) * S + j] = h[(size_t) k * SP * SP + (size_t) j * SP + i];
    return BEAGLE_SUCCESS;
}

// The plan cache of all three back ends: the plan compiled from exactly these ints (the operations as submitted; the
// general-state walk appends its list starts) under the current layout epoch.  A miss (`build`) hands out a new plan or the
// least recently used one, already keyed: the caller compiles into it and reports the outcome through planBuilt.
inline Plan* Instance::cachedPlan(const int* key, size_t nints, bool& build)
{
    static_assert(sizeof(BeagleOperation) == 7 * sizeof(int), "BeagleOperation is 7 ints");
    const uint64_t h = fnv1a(&layoutEpoch, 1, fnv1a(key, nints));
    build = false;
    for (Plan* pl : plans)
        if (pl->hash == h && pl->key.size() == nints + 1 && pl->key[nints] == layoutEpoch &&
            std::memcmp(pl->key.data(), key, nints * sizeof(int)) == 0) {
            pl->lastUse = ++planClock;
            planHits++;
            return pl;
        }
    planMisses++;
    build = true;
    Plan* plan;
    if (const size_t maxPlans = 24; plans.size() < maxPlans) {
        plan = new Plan();
        plans.push_back(plan);
    } else {
        plan = plans[0];
        for (Plan* pl : plans) if (pl->lastUse < plan->lastUse) plan = pl;
    }
    plan->key.assign(key, key + nints);
    plan->key.push_back(layoutEpoch);
    plan->hash = h;
    plan->lastUse = ++planClock;
    return plan;
}

// the outcome of compiling into a plan cachedPlan handed out: a failed build must not be found again
inline int Instance::planBuilt(Plan& plan, int rc)
{
    if (rc) { plan.hash = 0; plan.key.clear(); }
    return rc;
}

// One operation of a list, whichever back end compiles it: index ranges, and children that hold something (`written`: the
// buffers earlier operations of the same list write).  BEAGLE_SUCCESS, or the error code with its message in `what`.
inline int Instance::checkOperation(const BeagleOperation& b, const std::vector<char>& written, const char*& what) const
{
    what = "";
    if (b.destinationPartials < 0 || b.destinationPartials >= nBuffers || b.child1Partials < 0 ||
        b.child1Partials >= nBuffers || b.child2Partials < 0 || b.child2Partials >= nBuffers) {
        what = "beagleUpdatePartials: partials index";
    } else if (b.child1TransitionMatrix < 0 || b.child1TransitionMatrix >= nMatrices || b.child2TransitionMatrix < 0 ||
               b.child2TransitionMatrix >= nMatrices) {
        what = "beagleUpdatePartials: matrix index";
    } else if ((!written[b.child1Partials] && !tipStates[b.child1Partials] && !valid[b.child1Partials]) ||
               (!written[b.child2Partials] && !tipStates[b.child2Partials] && !valid[b.child2Partials])) {
        what = "beagleUpdatePartials: child buffer was never written";
    } else if (b.destinationScaleWrite != BEAGLE_OP_NONE) {
        if (b.destinationScaleWrite < 0 || b.destinationScaleWrite >= nScale) what = "beagleUpdatePartials: scale write index";
    } else if (b.destinationScaleRead != BEAGLE_OP_NONE) {
        if (b.destinationScaleRead < 0 || b.destinationScaleRead >= nScale) what = "beagleUpdatePartials: scale read index";
    }
    return what[0] ? BEAGLE_ERROR_OUT_OF_RANGE : BEAGLE_SUCCESS;
}

// ---------------------------------------------------------------------------------------------
// beagleUpdatePartials: resolve buffer indices to device pointers, then hand the list to the
// 4-state tree-walk kernel or to the level-synchronous general kernels.
// ---------------------------------------------------------------------------------------------
inline int Instance::updatePartials(const BeagleOperation* ops, int n, int cumIdx)
{
    if (n <= 0) return BEAGLE_SUCCESS;
    if (cumIdx != BEAGLE_OP_NONE && (cumIdx < 0 || cumIdx >= nScale))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: cumulative scale index");
    if (!finalExpOf.empty())                     // a buffer an operation overwrites no longer holds final partials
        for (int o = 0; o < n; ++o)
            if (ops[o].destinationPartials >= 0 && ops[o].destinationPartials < nBuffers) finalExpOf[ops[o].destinationPartials] = nullptr;
    if (!preOrder.empty())                       // ... nor the rest-of-tree vector of a pre-order pass
        for (int o = 0; o < n; ++o) clearPreOrder(ops[o].destinationPartials);
    if (s4) return updatePartials4(ops, n, cumIdx);
    if (wg) return updatePartialsG(ops, n, cumIdx);
    int32_t* cumPtr = nullptr;
    if (cumIdx != BEAGLE_OP_NONE) { bool fresh; int rc = scales.cumulativeForAdd(cumIdx, cumPtr, fresh); if (rc) return rc; }
    bool build;
    Plan* plan = cachedPlan(reinterpret_cast<const int*>(ops), (size_t) n * 7, build);
    if (!build) return submit(plan, cumIdx, cumPtr);
    if (!mfma || sw.mfmaWhole || sw.noDefer || pending.empty()) {
        // launch the queued transition-matrix jobs now: the kernel runs while the host compiles the list
        int mrc = flushMatrices();
        if (mrc) return planBuilt(*plan, mrc);
    }
    std::vector<PartialsOp> dev(n);
    std::vector<int> dstIdx(n), c1Idx(n), c2Idx(n);
    std::vector<char> written(nBuffers, 0);
    auto resolve = [&]() -> int {
        for (int o = 0; o < n; ++o) {
            const BeagleOperation& b = ops[o];
            PartialsOp& d = dev[o];
            std::memset(&d, 0, sizeof d);
            const char* what;
            int rc = checkOperation(b, written, what);
            if (rc) return fail(rc, what);
            rc = ensurePartials(b.destinationPartials);
            if (rc) return rc;
            d.dst = partials[b.destinationPartials];
            // (a buffer the list itself wrote is partials even if it held tip states)
            const Operand c1 = operand(b.child1Partials, written[b.child1Partials]), c2 = operand(b.child2Partials, written[b.child2Partials]);
            d.c1 = c1.ptr; d.c1_kind = c1.kind;
            d.c2 = c2.ptr; d.c2_kind = c2.kind;
            d.m1 = matrixPtr(b.child1TransitionMatrix);
            d.m2 = matrixPtr(b.child2TransitionMatrix);
            d.c1_slot = d.c2_slot = d.dst_slot = MBAMD_NO_SLOT;
            d.scale_mode = b.destinationScaleWrite != BEAGLE_OP_NONE ? SCALE_WRITE : (b.destinationScaleRead != BEAGLE_OP_NONE ? SCALE_READ : SCALE_NONE);
            if (d.scale_mode != SCALE_NONE) {
                const int si = d.scale_mode == SCALE_WRITE ? b.destinationScaleWrite : b.destinationScaleRead;
                if ((rc = scales.nodeBuffer(si, d.scale)) != BEAGLE_SUCCESS) return rc;
            }
            dstIdx[o] = b.destinationPartials;
            c1Idx[o] = b.child1Partials;
            c2Idx[o] = b.child2Partials;
            written[b.destinationPartials] = 1;
        }
        return BEAGLE_SUCCESS;
    };
    int rc = resolve();
    if (rc) return planBuilt(*plan, rc);
    for (int o = 0; o < n; ++o) valid[dstIdx[o]] = 1;
    // ---- compile the list into the plan (which may be an evicted one that is still queued: that queue runs first) -----------
    for (auto& pp : pending)
        if (pp.first == plan) { int frc = flushPending(); if (frc) return planBuilt(*plan, frc); break; }
    {
        StatTimer st_(ST_PLAN);
        rc = buildGeneric(*plan, dev, dstIdx, c1Idx, c2Idx);
    }
    if (rc) return planBuilt(*plan, rc);
    plan->bufsRead.assign(c1Idx.begin(), c1Idx.end());
    plan->bufsRead.insert(plan->bufsRead.end(), c2Idx.begin(), c2Idx.end());
    plan->bufsWritten.assign(dstIdx.begin(), dstIdx.end());
    plan->scalesUsed.clear();
    for (int o = 0; o < n; ++o) {
        if (ops[o].destinationScaleWrite != BEAGLE_OP_NONE) plan->scalesUsed.push_back(ops[o].destinationScaleWrite);
        if (ops[o].destinationScaleRead != BEAGLE_OP_NONE) plan->scalesUsed.push_back(ops[o].destinationScaleRead);
    }
    return submit(plan, cumIdx, cumPtr);
}

// Run a compiled list now, or -- general-state MFMA path -- defer it: consecutive mutually independent lists
// (one per eigen-system part, reference src/mbbeagle.c:1062-1104) are executed together, one launch per
// dependency level over all of them, when the next call that is not a beagleUpdatePartials arrives.
inline int Instance::submit(Plan* plan, int cumIdx, int32_t* cumPtr)
{
    {
        int mrc = flushMatrices();
        if (mrc) return mrc;
    }
    if (!s4 && mfma && !sw.mfmaWhole && !sw.noDefer) {
        if ((int) pending.size() >= MBAMD_MAX_TABLES || !independentOfPending(*plan, cumIdx)) {
            int rc = flushPending();
            if (rc) return rc;
        }
        pending.emplace_back(plan, cumIdx);
        return BEAGLE_SUCCESS;
    }
    (void) cumIdx;
    return timedRun(*plan, cumPtr);
}

inline bool Instance::independentOfPending(const Plan& plan, int cumIdx)
{
    if (pending.empty()) return true;
    std::vector<char> wr(nBuffers, 0), rd(nBuffers, 0), sc(scales.count(), 0);
    for (auto& pp : pending) {
        if (pp.first == &plan) return false;
        for (int b : pp.first->bufsWritten) wr[b] = 1;
        for (int b : pp.first->bufsRead) rd[b] = 1;
        for (int i : pp.first->scalesUsed) sc[i] = 1;
        if (pp.second >= 0) sc[pp.second] = 1;
    }
    for (int b : plan.bufsWritten) if (wr[b] || rd[b]) return false;
    for (int b : plan.bufsRead) if (wr[b]) return false;
    for (int i : plan.scalesUsed) if (sc[i]) return false;
    if (cumIdx >= 0 && sc[cumIdx]) return false;
    return true;
}

inline int Instance::runHeldPath()
{
    Plan* plan = heldPath;
    heldPath = nullptr;
    if (!plan) return BEAGLE_SUCCESS;
    walkCumFresh = heldPathFresh;
    return timedRun(*plan, heldPathCum);
}

inline int Instance::flushPending(bool keepPath)
{
    StatTimer st_(ST_FLUSH);
    int mrc = flushMatrices();                   // (queued matrix jobs precede the lists that read them)
    if (mrc) return mrc;
    if (heldPath && !keepPath) { int prc = runHeldPath(); if (prc) return prc; }
    if (wg) return flushWalkG();
    if (pending.empty()) return BEAGLE_SUCCESS;
    std::vector<std::pair<Plan*, int>> work;
    work.swap(pending);
    ++launchClock;
    for (auto& w : work) w.first->lastLaunch = launchClock;
    auto cumOf = [&](int idx) { int32_t* p = nullptr; bool fresh; if (idx >= 0) (void) scales.cumulativeForAdd(idx, p, fresh); return p; };   // (it exists since the list was submitted)
    // merged launches need a per-factor-tile kernel for this shape (launch_mfma_split); other shapes -- e.g. three rate
    // categories -- run their lists one after the other, in submission order
    const bool mergeable = (NT == 1 && (K == 1 || K == 2 || K == 4)) || (NT == 2 && (K == 1 || K == 2));
    if (work.size() == 1 || !mergeable) {
        for (auto& w : work) {
            const int rc = timedRun(*w.first, cumOf(w.second));
            if (rc) return rc;
        }
        return BEAGLE_SUCCESS;
    }
    hipEvent_t ev0{}, ev1{};
    { int brc = launchesBegin(ev0, ev1); if (brc) return brc; }
    size_t maxLevels = 0;
    bool allNarrow = true;
    for (auto& w : work) {
        maxLevels = std::max(maxLevels, w.first->start.size() - 1);
        allNarrow = allNarrow && w.first->narrow;
    }
    if (allNarrow) {                             // every list is a set of root-ward paths: one launch walks them all
        size_t nchains = 0;
        for (auto& w : work) nchains += w.first->chains.size();
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int t = 0;
        for (auto& w : work) {
            if (nchains <= MBAMD_MAX_TABLES) {
                for (auto& ch : w.first->chains) {
                    tabs.ops[t] = w.first->d_table + ch.first;
                    tabs.cum[t] = cumOf(w.second);
                    tabs.start[t] = ch.second;
                    ++t;
                }
            } else {                             // too many sub-lists: each list in its own order
                tabs.ops[t] = w.first->d_table;
                tabs.cum[t] = cumOf(w.second);
                tabs.start[t] = w.first->start.back();
                ++t;
            }
        }
        if (launch_mfma_serial(*this, tabs, t)) {
            pendingLaunches += 1;
            maxLevels = 0;
        }
    }
    // levels every list runs as level launches; from spineFrom on each list is a spine of single operations
    size_t spineFrom = 0;
    for (auto& w : work) spineFrom = std::max(spineFrom, (size_t) w.first->serialFrom);
    if (maxLevels > 0) {
        int spineOps = 0;
        for (auto& w : work) spineOps += std::max(0, w.first->start.back() - w.first->start[std::min(spineFrom, w.first->start.size() - 1)]);
        if (spineOps < 2) spineFrom = maxLevels;
    }
    for (size_t l = 0; l < std::min(maxLevels, spineFrom); ++l) {
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int t = 0, total = 0;
        bool tipsDone = false;
        if (l == 0) {                            // operations on two compact tips: their own kernel
            for (auto& w : work) {
                if (w.first->tipTip == 0) continue;
                tabs.ops[t] = w.first->d_table;
                tabs.cum[t] = cumOf(w.second);
                tabs.start[t] = total;
                total += w.first->tipTip;
                ++t;
            }
            for (int u = t; u <= MBAMD_MAX_TABLES; ++u) tabs.start[u] = 1 << 30;
            if (total > 0 && launch_tips(*this, tabs, total)) {
                pendingLaunches += 1;
                tipsDone = true;
            }
            std::memset(&tabs, 0, sizeof tabs);
            t = 0;
            total = 0;
        }
        for (auto& w : work) {
            const std::vector<int>& st = w.first->start;
            if (l + 1 >= st.size() || st[l + 1] == st[l]) continue;
            const int skip = (l == 0 && tipsDone) ? w.first->tipTip : 0;
            if (st[l + 1] - st[l] - skip == 0) continue;
            tabs.ops[t] = w.first->d_table + st[l] + skip;
            tabs.cum[t] = cumOf(w.second);
            tabs.start[t] = total;
            total += st[l + 1] - st[l] - skip;
            ++t;
        }
        for (int u = t; u <= MBAMD_MAX_TABLES; ++u) tabs.start[u] = 1 << 30;
        if (total == 0) continue;
        if (!launch_mfma_split(*this, tabs, total)) return fail(BEAGLE_ERROR_GENERAL, "no MFMA kernel for a deferred list");
        pendingLaunches += 1;
    }
    if (spineFrom < maxLevels) {
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int t = 0;
        for (auto& w : work) {
            const std::vector<int>& st = w.first->start;
            if (spineFrom + 1 >= st.size()) continue;
            tabs.ops[t] = w.first->d_table + st[spineFrom];
            tabs.cum[t] = cumOf(w.second);
            tabs.start[t] = st.back() - st[spineFrom];
            ++t;
        }
        if (t > 0) {
            if (!launch_mfma_serial(*this, tabs, t)) return fail(BEAGLE_ERROR_GENERAL, "no serial MFMA kernel for a deferred list");
            pendingLaunches += 1;
        }
    }
    HIP_TRY(hipGetLastError());
    return launchesEnd(ev0, ev1);
}

// upload a freshly built table (level kernels: PartialsOp; tree walks: Walk4Entry programs) into the plan's own device buffer
inline int Instance::planTable(Plan& plan, const void* table, size_t bytes)
{
    const bool inFlight = plan.lastLaunch > syncedClock;     // the old table may still be read by a running kernel
    if (bytes > plan.cap) {
        if (inFlight) { HIP_TRY(hipStreamSynchronize(stream)); syncedClock = launchClock; }
        if (plan.d_table) HIP_TRY(hipFree(plan.d_table));
        plan.d_table = nullptr;
        plan.cap = 0;
        HIP_TRY(hipMalloc(&plan.d_table, bytes + bytes / 2));
        plan.cap = bytes + bytes / 2;
    } else if (inFlight) {
        HIP_TRY(hipStreamSynchronize(stream));
        syncedClock = launchClock;
    }
    return upload(plan.d_table, table, bytes);
}

inline int Instance::timedRun(const Plan& plan, int32_t* cum)
{
    const_cast<Plan&>(plan).lastLaunch = ++launchClock;
    hipEvent_t ev0{}, ev1{};
    { int brc = launchesBegin(ev0, ev1); if (brc) return brc; }
    const int rc = s4 ? runWalk(plan, cum) : (wg ? runWalkG(plan) : runGeneric(plan, cum));
    { int erc = launchesEnd(ev0, ev1); if (erc) return erc; }
    if (events.size() > 4096) {                   // a client that never asks: fold the finished ones into the running total
        HIP_TRY(hipStreamSynchronize(stream));
        spanFold();
        int frc = eventsFold();
        if (frc) return frc;
    }
    return rc;
}

// ---------------------------------------------------------------------------------------------
// 4-state path: beagleUpdatePartials -> per-wave programs of the tree-walk kernel (mbamd_walk4.h).
// ---------------------------------------------------------------------------------------------
// A compiled list of an arena layout was launched (or is held), compiled now or before: its destinations are valid and hold no recipe (overwritten;
// the launch leaves its own small subtrees unstored afresh, runWalk), the exponent buffers it writes hold node exponents; the list counters
inline void Instance::listLaunched(const BeagleOperation* ops, int n, bool path, bool forked)
{
    for (int o = 0; o < n; ++o) {
        valid[ops[o].destinationPartials] = 1;
        dropRecipe(ops[o].destinationPartials);
        if (ops[o].destinationScaleWrite != BEAGLE_OP_NONE) scales.nodeWritten(ops[o].destinationScaleWrite);
    }
    listsTotal++;
    if (path) { listsPath++; if (forked) forkedPaths++; }
    else { listsWalked++; opsWalked += n; }
}

inline int Instance::updatePartials4(const BeagleOperation* ops, int n, int cumIdx)
{
    if (heldPath) { int prc = runHeldPath(); if (prc) return prc; }      // (a list behind a held path: the path runs first)
    if (snapPlan) { int src = flushSnapshot(); if (src) return src; }    // (no integration followed the launch; this call may recompile the plan)
    if (nUnstored) {
        // children from outside the list that an earlier launch left unstored: made now, before a path is held -- the launch runs
        // while the host compiles or looks up the list
        std::vector<int>& ext = w4segList;
        std::vector<char>& written = w4written;
        ext.clear();
        written.assign((size_t) nBuffers, 0);
        for (int o = 0; o < n; ++o) {
            for (const int c : {ops[o].child1Partials, ops[o].child2Partials})
                if (c >= 0 && c < nBuffers && unstored[(size_t) c] && !written[(size_t) c]) ext.push_back(c);
            if (ops[o].destinationPartials >= 0 && ops[o].destinationPartials < nBuffers) written[(size_t) ops[o].destinationPartials] = 1;
        }
        if (!ext.empty()) { int src = ensureStored(ext.data(), (int) ext.size()); if (src) return src; }
    }
    int32_t* cumPtr = nullptr;
    walkCumFresh = false;
    if (cumIdx != BEAGLE_OP_NONE) { int rc = scales.cumulativeForAdd(cumIdx, cumPtr, walkCumFresh); if (rc) return rc; }
    bool build;
    Plan* plan = cachedPlan(reinterpret_cast<const int*>(ops), (size_t) n * 7, build);
    if (build) {
        int rc = flushMatrices();                // the matrix kernel runs while the host compiles the list
        if (rc == BEAGLE_SUCCESS) {
            StatTimer st_(ST_PLAN);
            plan->path = plan->forked = false;
            plan->unstoredSubtrees.clear();
            rc = buildPath4(*plan, ops, n) ? BEAGLE_SUCCESS : buildWalk(*plan, ops, n);
        }
        if (planBuilt(*plan, rc)) return rc;
    }
    listLaunched(ops, n, plan->path, plan->forked);
    int mrc = flushMatrices();
    if (mrc) return mrc;
    if (plan->path && !sw.noFusePath && K <= 8 && plan->inlineProg.size() <= MBAMD_W4_INLINE) {
        // hold it: the next call decides (runHeldPath / integratePath4)
        heldPath = plan;
        heldPaths++;
        heldPathCum = cumPtr;
        heldPathFresh = walkCumFresh;
        heldPathDst = ops[n - 1].destinationPartials;
        return BEAGLE_SUCCESS;
    }
    return timedRun(*plan, cumPtr);
}

// Compile one operation list: validate, cut into hazard-free segments, build (or re-use) the structural template of
// each segment and fill it with this list's buffer / matrix / scale indices.
inline int Instance::buildWalk(Plan& plan, const BeagleOperation* ops, int n, const int* listOf, bool perList)
{
    const int scratchScale = (int) scales.count();              // sink / source of entries that do not rescale
    std::vector<int>& segList = w4segList;                     // (20/61-state walk) merged-list index of each operation of the segment
    segList.clear();
    std::vector<char>& written = w4written;
    written.assign((size_t) nBuffers, 0);
    w4table.clear();
    plan.segments.clear();
    plan.unstoredSubtrees.clear();
    std::vector<Walk4Op>& seg = w4ops;
    seg.clear();
    // segment state: buffers / exponent buffers the current segment has read or written
    std::vector<char>&segRead = w4segRead, &segWritten = w4segWritten, &segScale = w4segScale;
    segRead.assign((size_t) nBuffers, 0); segWritten.assign((size_t) nBuffers, 0); segScale.assign(scales.count() + 1, 0);
    if (w4writer.size() < (size_t) nBuffers) w4writer.assign((size_t) nBuffers, -1);
    int reloads = 0, externals = 0, phases = 0;
    auto flushSegment = [&]() -> int {
        if (seg.empty()) return BEAGLE_SUCCESS;
        // structural key
        std::vector<int>& key = w4key;
        key.clear();
        key.reserve(seg.size() * 3 + 4);
        key.push_back((int) seg.size()); key.push_back(w4.maxW); key.push_back(w4.maxSlots + 256 * w4.maxSlots1);
        key.push_back(w4.prefetchDistance * 2 + (w4.safeWaits ? 1 : 0));
        key.push_back(w4.plainWaves + 16 * w4.plainSlots); key.push_back(w4.plainMinOps + 64 * w4.plainShare[std::max(2, std::min(8, w4.plainWaves))] + (w4.plainDescend ? 1 << 20 : 0));
        {
            std::vector<int>& writer = w4writer;          // buffer -> operation of this segment that writes it (-1 outside this block)
            // (4-state walk) per operation: the tips of its subtree if that is compact tips and operations of this segment alone and has at
            // most MBAMD_W4_UNSTORED_TIPS_MAX of them, else 0; and the subtree's operations in list order, its own last
            constexpr int RO = MBAMD_W4_UNSTORED_TIPS_MAX - 1;
            w4subTips.assign(wg ? 0 : seg.size(), 0);
            w4subOps.assign(wg ? 0 : seg.size() * RO, -1);
            for (size_t o = 0; o < seg.size() && !wg; ++o) {
                const Walk4Op& op = seg[o];
                const int w1 = op.tip1 ? -1 : writer[op.c1], w2 = op.tip2 ? -1 : writer[op.c2];
                const int t1 = op.tip1 ? 1 : (w1 >= 0 ? w4subTips[(size_t) w1] : 0), t2 = op.tip2 ? 1 : (w2 >= 0 ? w4subTips[(size_t) w2] : 0);
                if (t1 && t2 && t1 + t2 <= MBAMD_W4_UNSTORED_TIPS_MAX && (op.tip1 || op.tip2 || op.c1 != op.c2)) {
                    w4subTips[o] = t1 + t2;
                    int below = 0, *mine = &w4subOps[o * RO];
                    for (const int w : {std::min(w1, w2), std::max(w1, w2)})          // (two inner children: two tip pairs, list order)
                        for (int j = 0; w >= 0 && j < RO && w4subOps[(size_t) w * RO + j] >= 0; ++j) mine[below++] = w4subOps[(size_t) w * RO + j];
                    mine[below] = (int) o;
                }
                writer[op.dst] = (int) o;
            }
            for (size_t o = 0; o < seg.size() && !wg; ++o) writer[seg[o].dst] = -1;
            for (size_t o = 0; o < seg.size(); ++o) {
                key.push_back(seg[o].tip1 ? -1 : writer[seg[o].c1]);
                key.push_back(seg[o].tip2 ? -1 : writer[seg[o].c2]);
                key.push_back((int) seg[o].tip1 | ((int) seg[o].tip2 << 1) | ((!seg[o].tip1 && !seg[o].tip2 && seg[o].c1 == seg[o].c2) ? 4 : 0) |
                              ((seg[o].scaleWrite < 0 && seg[o].scaleRead >= 0) ? 8 : 0));   // (SCALE_READ entries wait for an exponent DMA)
                writer[seg[o].dst] = (int) o;
            }
            for (size_t o = 0; o < seg.size(); ++o) writer[seg[o].dst] = -1;
        }
        const uint64_t kh = fnv1a(key.data(), key.size());
        auto it = w4templates.find(kh);
        if (it == w4templates.end() || it->second.key != key) {
            scheduleMisses++;
            if (w4templates.size() >= 8192) w4templates.clear();
            Walk4Template& t = w4templates[kh];
            bool ok = w4.build(seg, t);
            if (!ok) {                           // out of slots with look-ahead prefetches: retry without, then on one wave
                Walk4Builder plain = w4;
                plain.prefetchDistance = 0;
                ok = plain.build(seg, t);
                if (!ok) { plain.maxW = 1; ok = plain.build(seg, t); }
            }
            if (!ok) { w4templates.erase(kh); return fail(BEAGLE_ERROR_GENERAL, "tree-walk scheduler: cannot place this list"); }
            t.key = key;
            it = w4templates.find(kh);
        } else {
            scheduleHits++;
        }
        const Walk4Template& t = it->second;
        reloads += t.reloads; externals += t.externals; phases = std::max(phases, t.phases);
        Plan::Segment sg;
        sg.first = w4table.size();
        sg.W = t.W; sg.entries = t.entries; sg.nslots = t.nslots; sg.tail = t.tail;
        sg.plain = t.plain && !wg; sg.peel = t.peel; sg.waves = sg.plain && t.waves;
        plan.segments.push_back(sg);
        w4table.resize(sg.first + t.prog.size());
        // bytes per buffer inside a block / tile, bytes per LDS slot
        const uint32_t slotb = wg ? wg_block_bytes(S) : 1024u;
        // a partials buffer inside a tile (20/61-state walk: bytes) / in the buffer-major 4-state arena (KiB: P_pad/64 x K of them)
        const uint32_t pbuf = wg ? (uint32_t) K * slotb : (uint32_t) ((size_t) (Ppad / 64) * K);
        const uint32_t ebuf = (uint32_t) K * 64u, mbuf = wg ? (uint32_t) (matrixFloats * 4) : (uint32_t) K * 64u;
        int prevKept = -1;                           // (20/61-state walk) slot the previous operation of the same program kept its result in
        w4entryOf.assign(seg.size(), -1);            // (4-state walk) operation -> its entry, for the recipes of a plain program (entries are filled wave by wave: a subtree with an inner operation on a LATER wave than its own finds -1 there and is stored, `placed` below)
        for (size_t i = 0; i < t.prog.size(); ++i) {
            const Walk4Template::Entry& te = t.prog[i];
            Walk4Entry& e = w4table[sg.first + i];
            std::memset(&e, 0, sizeof e);
            if (i % (size_t) t.entries == 0) prevKept = -1;
            uint32_t flags = te.flags, mode = SCALE_NONE, keep = 0;
            e.ewrite = (uint32_t) scratchScale * ebuf;
            e.eread = (uint32_t) scratchScale * ebuf;
            e.ewrite = (uint32_t) (scratchScale + (int) (i % (size_t) (wg ? MBAMD_WG_SCRATCH_ROWS : MBAMD_W4_SCRATCH_ROWS))) * ebuf;   // (neighbouring entries: different scratch rows)
            if (wg) {
                // k_walkg (mbamd_walkg.h): no prefetch entries; a child that is neither a tip nor in a slot is read from
                // HBM by the operand pipeline; NOP entries store zeros to the extra buffer of the tile
                e.dst = (uint32_t) nBuffers * pbuf;
                if (te.op >= 0) {
                    const Walk4Op& op = seg[te.op];
                    e.dst = (uint32_t) op.dst * pbuf;
                    if (op.tip1) { e.c1 = (uint32_t) op.c1 * (uint32_t) MBAMD_WG_TW; flags |= MBAMD_W4_TIP1; }
                    else if (te.c1slot == 0xFF) { e.c1 = (uint32_t) op.c1 * pbuf; flags |= MBAMD_WG_MEM1; }
                    else e.c1 = (uint32_t) te.c1slot * slotb;
                    if (op.tip2) { e.c2 = (uint32_t) op.c2 * (uint32_t) MBAMD_WG_TW; flags |= MBAMD_W4_TIP2; }
                    else if (te.c2slot == 0xFF) { e.c2 = (uint32_t) op.c2 * pbuf; flags |= MBAMD_WG_MEM2; }
                    else e.c2 = (uint32_t) te.c2slot * slotb;
                    e.m1 = (uint32_t) op.m1 * mbuf;
                    e.m2 = (uint32_t) op.m2 * mbuf;
                    if (te.dslot != 0xFF) { keep = te.dslot; flags |= MBAMD_W4_KEEP; }
                    if (!op.tip1 && te.c1slot != 0xFF && (int) te.c1slot == prevKept) flags |= MBAMD_WG_PREV1;
                    if (!op.tip2 && te.c2slot != 0xFF && (int) te.c2slot == prevKept) flags |= MBAMD_WG_PREV2;
                    prevKept = te.dslot != 0xFF ? (int) te.dslot : -1;
                    mode = op.scaleWrite >= 0 ? SCALE_WRITE : (op.scaleRead >= 0 ? SCALE_READ : SCALE_NONE);
                    if (op.scaleWrite >= 0) e.ewrite = (uint32_t) op.scaleWrite * ebuf;
                    if (op.scaleRead >= 0) e.eread = (uint32_t) op.scaleRead * ebuf;
                    e.ctl = flags | (mode << 8) | ((uint32_t) segList[te.op] << 10) | (keep << 16);
                } else {
                    e.ctl = (flags & (MBAMD_W4_NOP | MBAMD_W4_BARRIER)) | MBAMD_W4_NOP;
                }
                continue;
            }
            if (te.pfOp[0] >= 0) {                          // PF entry
                const Walk4Op& p0 = seg[te.pfOp[0]];
                e.dst = (uint32_t) (te.pfChild[0] == 0 ? p0.c1 : p0.c2) * pbuf;
                e.c1 = (uint32_t) te.pfSlot[0] * 1024u;
                flags |= MBAMD_W4_PF0 | MBAMD_W4_NOP;
                if (te.pfOp[1] >= 0) {
                    const Walk4Op& p1 = seg[te.pfOp[1]];
                    e.c2 = (uint32_t) (te.pfChild[1] == 0 ? p1.c1 : p1.c2) * pbuf;
                    e.m1 = (uint32_t) te.pfSlot[1] * 1024u;
                    flags |= MBAMD_W4_PF1;
                }
            } else if (te.op >= 0) {
                const Walk4Op& op = seg[te.op];
                e.dst = (uint32_t) op.dst * pbuf;
                if (op.tip1) { e.c1 = (uint32_t) op.c1 * 32u; flags |= MBAMD_W4_TIP1; }
                else if (te.c1slot == 0xFE) flags |= MBAMD_W4_FWD1;
                else e.c1 = (uint32_t) te.c1slot * 1024u;
                if (op.tip2) { e.c2 = (uint32_t) op.c2 * 32u; flags |= MBAMD_W4_TIP2; }
                else if (te.c2slot == 0xFE) flags |= MBAMD_W4_FWD2;
                else e.c2 = (uint32_t) te.c2slot * 1024u;
                e.m1 = (uint32_t) op.m1 * mbuf;
                e.m2 = (uint32_t) op.m2 * mbuf;
                if (te.dslot != 0xFF) { keep = te.dslot; flags |= MBAMD_W4_KEEP; }
                mode = op.scaleWrite >= 0 ? SCALE_WRITE : (op.scaleRead >= 0 ? SCALE_READ : SCALE_NONE);
                if (op.scaleWrite >= 0) e.ewrite = (uint32_t) op.scaleWrite * ebuf;
                if (op.scaleRead >= 0) e.eread = (uint32_t) op.scaleRead * ebuf;
                w4entryOf[(size_t) te.op] = (int) (sg.first + i);
                const int subTips = w4subTips[(size_t) te.op];
                if (sg.plain && subTips >= 2 && subTips <= unstoredTips()) {     // (kept or dropped below)
                    // the recipe: the subtree's operations with their children as tips or as operations of the recipe; every one of them
                    // ran earlier in this program (a child runs before its parent), so its entry is known
                    constexpr int RO = MBAMD_W4_UNSTORED_TIPS_MAX - 1;
                    const int* const sub = &w4subOps[(size_t) te.op * RO];
                    Plan::Unstored u;
                    u.entry = (int) (sg.first + i); u.dst = op.dst;
                    for (int& x : u.inner) x = -1;
                    bool placed = true;
                    for (int j = 0; j < RO && sub[j] >= 0; ++j) {
                        const Walk4Op& so = seg[(size_t) sub[j]];
                        Walk4Recipe::Op& ro = u.r.op[u.r.nops++];
                        ro.mode = so.scaleWrite >= 0 ? SCALE_WRITE : (so.scaleRead >= 0 ? SCALE_READ : SCALE_NONE);
                        ro.in1 = !so.tip1; ro.in2 = !so.tip2;
                        ro.c1 = so.c1; ro.c2 = so.c2;
                        for (int q = 0; q < j; ++q) {
                            if (ro.in1 && seg[(size_t) sub[q]].dst == so.c1) ro.c1 = q;
                            if (ro.in2 && seg[(size_t) sub[q]].dst == so.c2) ro.c2 = q;
                        }
                        if (sub[j] != te.op) { u.inner[j] = w4entryOf[(size_t) sub[j]]; placed = placed && u.inner[j] >= 0; }
                    }
                    if (placed) plan.unstoredSubtrees.push_back(u);
                }
            }
            if (te.vmwait != 0xFF) flags |= MBAMD_W4_VMWAIT;
            // the entry in front of a SCALE_READ entry of the same wave fetches that entry's stored exponents (mbamd_walk4.h)
            if ((i + 1) % (size_t) t.entries != 0) {
                const Walk4Template::Entry& tn = t.prog[i + 1];
                if (tn.op >= 0 && seg[tn.op].scaleWrite < 0 && seg[tn.op].scaleRead >= 0) flags |= MBAMD_W4_NEXT_READS;
            }
            e.ctl = flags | (mode << 8) | ((uint32_t) (te.vmwait == 0xFF ? 0 : te.vmwait) << 10) | (keep << 16);
            // a segment for the plain kernel: every operation says once what pair of child kinds it is (MBAMD_W4_KIND_*: the loop body it
            // runs in), and every entry -- the read-ahead tail included -- carries child 1's "plane offset or 0" ready-made in `eread`,
            // which nothing else reads in such a program (no entry divides by stored exponents)
            if (sg.plain) {
                if (te.op >= 0) e.ctl |= walk4_kind_of(flags);
                e.eread = (flags & MBAMD_W4_TIP1) ? e.c1 : 0u;
            }
        }
        if (sg.waves) {
            // the phase table behind the program (walk4_waves_table_entries)
            const size_t at = w4table.size();
            w4table.resize(at + walk4_waves_table_entries(t.W, t.phases));
            std::memset(&w4table[at], 0, (w4table.size() - at) * sizeof(Walk4Entry));
            uint32_t* const tab = reinterpret_cast<uint32_t*>(&w4table[at]);
            tab[0] = (uint32_t) t.phases;
            for (size_t q = 0; q < t.phaseCount.size(); ++q) tab[1 + q] = (uint32_t) t.phaseCount[q];
        }
        lastWalkW = t.W; lastWalkSlots = t.nslots; lastWalkEntries = t.entries; lastWalkPhases = t.phases; lastWalkCrossing = t.crossing;
        seg.clear();
        segList.clear();
        std::fill(segRead.begin(), segRead.end(), 0);
        std::fill(segWritten.begin(), segWritten.end(), 0);
        std::fill(segScale.begin(), segScale.end(), 0);
        return BEAGLE_SUCCESS;
    };
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        const char* what;
        if (const int crc = checkOperation(b, written, what)) return fail(crc, what);
        Walk4Op w;
        w.dst = b.destinationPartials;
        w.c1 = b.child1Partials; w.c2 = b.child2Partials;
        w.m1 = b.child1TransitionMatrix; w.m2 = b.child2TransitionMatrix;
        const uint8_t tip[2] = {(uint8_t) (tipStates[w.c1] && !written[w.c1]), (uint8_t) (tipStates[w.c2] && !written[w.c2])};
        w.tip1 = tip[0]; w.tip2 = tip[1];
        w.scaleWrite = w.scaleRead = -1;
        if (b.destinationScaleWrite != BEAGLE_OP_NONE) {
            w.scaleWrite = b.destinationScaleWrite;
        } else if (b.destinationScaleRead != BEAGLE_OP_NONE) {
            if (scales.isCumulative(b.destinationScaleRead) && !segScale[b.destinationScaleRead])
                return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleUpdatePartials: destinationScaleRead names a cumulative buffer");
            w.scaleRead = b.destinationScaleRead;
        }
        // hazards that the in-launch dependency analysis does not cover end the segment (MrBayes never produces them):
        // a buffer written twice or written after it was read, an exponent buffer touched twice unless only read
        bool hazard = segWritten[w.dst] || segRead[w.dst];
        if (perList && o > 0 && listOf[o] != listOf[o - 1]) hazard = true;       // (independent lists: one program set each)
        if (w.scaleWrite >= 0 && segScale[w.scaleWrite]) hazard = true;
        if (w.scaleRead >= 0 && segScale[w.scaleRead] == 2) hazard = true;
        if (hazard) {
            int rc = flushSegment();
            if (rc) return rc;
        }
        segWritten[w.dst] = 1;
        if (!tip[0]) segRead[w.c1] = 1;
        if (!tip[1]) segRead[w.c2] = 1;
        if (w.scaleWrite >= 0) segScale[w.scaleWrite] = 2;
        if (w.scaleRead >= 0 && !segScale[w.scaleRead]) segScale[w.scaleRead] = 1;
        written[w.dst] = 1;
        seg.push_back(w);
        segList.push_back(listOf ? listOf[o] : 0);
    }
    int rc = flushSegment();
    if (rc) return rc;
    if (sw.verbose)
        std::fprintf(stderr, "[mbamd] walk plan: %d ops, %zu segment(s), W=%d, %d entries/wave, %d slots/%s, %d phases, %d reloads, %d external children, %d values cross waves in LDS%s\n",
                     n, plan.segments.size(), lastWalkW, lastWalkEntries, lastWalkSlots, plan.segments.back().waves ? "workgroup" : "wave", phases, reloads, externals,
                     lastWalkCrossing, plan.segments.back().plain ? " (plain)" : "");
    // a short program goes out with the launch itself (k_walk4_t<Walk4ArgsInline>, k_walkg<..., WalkGArgsInline>)
    plan.inlineProg.clear();
    // (a plain program of several waves has no generic reading: the slots of its entries are the workgroup's)
    const bool inlineForm = !sw.noInlinePrograms && plan.segments.size() == 1 && w4table.size() <= (size_t) MBAMD_W4_INLINE && !plan.segments[0].waves;
    // Small subtrees are not stored where nothing can read the HBM copy in the launch that makes them: the list is ONE segment and that
    // segment runs on the plain kernel, on one wave or several (no prefetch: every child is a tip, a slot -- also of a value from another
    // wave -- or the forwarded result).  Lists cut over several segments, programs in the kernel arguments and the generic / path
    // kernels store everything.
    plan.sideFirst = 0; plan.sideCount = 0;
    if (s4 && !sw.storeTipPairs && !sw.noPlainWalk && !inlineForm && plan.segments.size() == 1 && plan.segments[0].plain) {
        for (const Plan::Unstored& u : plan.unstoredSubtrees) w4table[(size_t) u.entry].ctl |= MBAMD_W4_NOSTORE;
        // the side table k_walk4_snapshot reads, behind the program: per subtree of more than two tips its own entry and its inner ones
        plan.sideFirst = w4table.size();
        for (const Plan::Unstored& u : plan.unstoredSubtrees) {
            if (u.r.nops < 2) continue;
            Walk4Entry side;
            std::memset(&side, 0, sizeof side);
            side.ctl = (uint32_t) u.entry; side.dst = (uint32_t) (u.r.nops - 1);
            side.c1 = (uint32_t) u.inner[0]; side.c2 = (uint32_t) (u.r.nops > 2 ? u.inner[1] : u.inner[0]);
            w4table.push_back(side);
            plan.sideCount++;
        }
    } else {
        plan.unstoredSubtrees.clear();
    }
    if (inlineForm) {
        plan.inlineProg = w4table;
        return BEAGLE_SUCCESS;
    }
    return planTable(plan, w4table.data(), w4table.size() * sizeof(Walk4Entry));
}

// host data -> the pinned ring -> a device buffer, by a launch of ours on the instance's stream
inline int Instance::ringCopy(void* dst, const void* src, size_t bytes)
{
    const void* ring = nullptr;
    int rc = stageDirect(src, bytes, &ring);
    if (rc) return rc;
    if (bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const unsigned n16 = (unsigned) (bytes / 16);
        MBAMD_LAUNCH(k_copy_from_ring, (n16 + 255u) / 256u, 256, 0, stream, static_cast<const copy16_t*>(ring), static_cast<copy16_t*>(dst), n16);
    } else {
        const unsigned n4 = (unsigned) (bytes / 4);
        MBAMD_LAUNCH(k_copy_from_ring4, (n4 + 255u) / 256u, 256, 0, stream, static_cast<const unsigned*>(ring), static_cast<unsigned*>(dst), n4);
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// A root-ward path (the list of a move that dirtied one branch): operation i has the result of operation i - 1 as one child; its
// other child -- and both children of operation 0 -- are compact tips or buffers the list does not write; no buffer or exponent
// buffer is written twice or read after it is written.  Round 6: also FORKED paths (the list of a topology move: root-ward paths
// that join, in post-order) -- an operation that does not read its predecessor's result begins a new ARM (the predecessor's
// result is saved), an operation whose other child is the saved result JOINS the arms; one saved result at a time.
// ops[0, n) are n / L lists of L operations (one list; or the mutually independent lists of the eigen-system parts of a codon
// model), every one such a path, and the hazard rules hold over all of them.  true: pathSteps describes the operations.  Anything
// else (false) is compiled by buildWalk, which also reports what is wrong with an operation.
inline bool Instance::recognisePath(const BeagleOperation* ops, int n, int L, bool& forked)
{
    std::vector<char>& written = w4written;          // buffers earlier operations write; after this loop: any operation
    written.assign((size_t) nBuffers, 0);
    std::vector<char>& named = w4segScale;           // how many scale fields of the operations name an exponent buffer (3 = more)
    named.assign(scales.count() + 1, 0);
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        const char* what;
        if (checkOperation(b, written, what) != BEAGLE_SUCCESS) return false;
        if (tipStates[b.destinationPartials] || written[b.destinationPartials]) return false;
        written[b.destinationPartials] = 1;
        for (int f : {b.destinationScaleWrite, b.destinationScaleRead})
            if (f >= 0 && f < nScale && named[f] < 3) ++named[f];
    }
    pathSteps.resize((size_t) n);
    forked = false;
    int saved = -1;                              // buffer of the saved result (an arm that waits for its join), or -1
    int armStart = 0, arms = 0;
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        PathStep& p = pathSteps[(size_t) o];
        const bool first = o % L == 0;
        const int prev = first ? -1 : ops[o - 1].destinationPartials;
        const bool one = !first && b.child1Partials == prev, two = !first && b.child2Partials == prev;
        if (one && two) return false;
        p.start = !one && !two;
        p.join = false;
        p.arm = 0;
        p.dst = b.destinationPartials;
        p.chain = two ? b.child2Partials : b.child1Partials; p.sib = two ? b.child1Partials : b.child2Partials;
        p.mchain = two ? b.child2TransitionMatrix : b.child1TransitionMatrix; p.msib = two ? b.child1TransitionMatrix : b.child2TransitionMatrix;
        if (p.start) {
            if (!first) {
                if (saved >= 0) return false;                                 // (two results waiting: not the path kernels' shape)
                saved = prev;
                pathSteps[(size_t) armStart].arm = o - armStart;
            }
            armStart = o;
            ++arms;
        } else if (saved >= 0 && p.sib == saved) {
            p.join = true;
            saved = -1;
        }
        // what comes from outside must not be written anywhere in the lists (before: a second dependency; after: a hazard)
        if ((!p.join && written[p.sib]) || (p.start && written[p.chain])) return false;
        p.chainTip = p.start && tipStates[p.chain] != nullptr;
        p.sibTip = !p.join && tipStates[p.sib] != nullptr;
        p.scaleMode = SCALE_NONE;
        p.scaleIdx = -1;
        if (b.destinationScaleWrite != BEAGLE_OP_NONE) {
            // the operation's own: nobody else's scale fields name it
            if (named[b.destinationScaleWrite] != 1 + (b.destinationScaleRead == b.destinationScaleWrite ? 1 : 0)) return false;
            p.scaleMode = SCALE_WRITE;
            p.scaleIdx = b.destinationScaleWrite;
        } else if (b.destinationScaleRead != BEAGLE_OP_NONE) {
            if (scales.isCumulative(b.destinationScaleRead)) return false;
            p.scaleMode = SCALE_READ;
            p.scaleIdx = b.destinationScaleRead;
        }
        if (o % L == L - 1) {                    // the end of a list
            if (saved >= 0) return false;        // (an arm nobody joins: two trees in one list)
            pathSteps[(size_t) armStart].arm = o + 1 - armStart;
            forked = forked || arms > 1;
            arms = 0;
        }
    }
    return true;
}

// A step as an entry of k_path4 / k_pathg, offsets in the caller's units: a partials buffer, a compact tip, a matrix buffer, and
// the scratch exponent row an operation that records no exponents stores to.
inline Walk4Entry Instance::pathEntry(const PathStep& p, uint32_t pbuf, uint32_t tipb, uint32_t mbuf, int scratchRow) const
{
    const uint32_t ebuf = (uint32_t) K * 64u;
    Walk4Entry e;
    std::memset(&e, 0, sizeof e);
    uint32_t flags = 0;
    e.dst = (uint32_t) p.dst * pbuf;
    if (p.start) {
        flags |= MBAMD_P4_START;
        if (p.chainTip) { e.c1 = (uint32_t) p.chain * tipb; flags |= MBAMD_W4_TIP1; }
        else e.c1 = (uint32_t) p.chain * pbuf;
    }
    if (p.join) flags |= MBAMD_P4_JOIN;
    else if (p.sibTip) { e.c2 = (uint32_t) p.sib * tipb; flags |= MBAMD_W4_TIP2; }
    else e.c2 = (uint32_t) p.sib * pbuf;
    e.m1 = (uint32_t) p.mchain * mbuf;
    e.m2 = (uint32_t) p.msib * mbuf;
    e.ewrite = (uint32_t) scratchRow * ebuf;
    e.eread = (uint32_t) scales.count() * ebuf;
    if (p.scaleMode == SCALE_WRITE) e.ewrite = (uint32_t) p.scaleIdx * ebuf;
    else if (p.scaleMode == SCALE_READ) e.eread = (uint32_t) p.scaleIdx * ebuf;
    e.ctl = flags | ((uint32_t) p.scaleMode << 8);
    return e;
}

// a path plan's geometry: one single-wave program of `entries` per list, no LDS slots, no read-ahead tail
inline void Instance::pathPlan(Plan& plan, int entries, bool forked)
{
    plan.forked = forked;
    plan.segments.clear();
    Plan::Segment sg;
    sg.first = 0; sg.W = 1; sg.entries = entries; sg.nslots = 0; sg.tail = 0;
    plan.segments.push_back(sg);
    lastWalkW = 1; lastWalkSlots = 0; lastWalkEntries = entries; lastWalkPhases = 1;
}

// One list as k_path4's entries (mbamd_walk4.h): partials buffers in KiB of the buffer-major arena, 32 bytes of state bitplanes
// per tip, matrices [K][4][4]; the first entry of an arm carries the arm's length.
inline bool Instance::buildPath4(Plan& plan, const BeagleOperation* ops, int n)
{
    if (sw.noPath4 || n < 1 || n > MBAMD_W4_INLINE) return false;
    bool forked;
    if (!recognisePath(ops, n, n, forked) || (forked && sw.noForkPath)) return false;
    const uint32_t pbuf = (uint32_t) ((size_t) (Ppad / 64) * K), mbuf = (uint32_t) K * 64u;
    plan.inlineProg.resize((size_t) n);
    for (int i = 0; i < n; ++i) {
        const PathStep& p = pathSteps[(size_t) i];
        plan.inlineProg[(size_t) i] = pathEntry(p, pbuf, 32u, mbuf, (int) scales.count());
        plan.inlineProg[(size_t) i].ctl |= (uint32_t) p.arm << 16;
    }
    plan.path = true;
    pathPlan(plan, n, forked);
    return true;
}

// The same for the 20/61-state walk (k_pathg, mbamd_pathg_kernel.h): `nl` mutually independent lists (the eigen-system parts of a
// codon model; one for a protein model), each a root-ward path -- or root-ward paths that join, at the same positions in every
// list --, all of the same length.  Entries [list][operation] in the tile arena's units (byte offsets of a buffer inside a tile,
// tip states at 32 bytes per buffer, matrix buffers in bytes); an entry carries its list's index.
static inline bool pathg_compiled(int S) { return S == 20 || (S >= 60 && S <= 63); }
inline bool Instance::buildPathG(Plan& plan, const BeagleOperation* ops, int n, const std::vector<int>& starts, int nl)
{
    if (sw.noPathG || !pathg_compiled(S) || nl < 1 || nl > MBAMD_WG_MAXLISTS || n < nl || n % nl != 0) return false;
    const int L = n / nl;
    if (L < 2 || (size_t) n > (size_t) MBAMD_W4_INLINE) return false;      // (a single operation gains nothing; the program travels in the kernel arguments)
    for (int q = 0; q < nl; ++q) if (starts[(size_t) q] != q * L) return false;
    bool forked;
    if (!recognisePath(ops, n, L, forked) || (forked && sw.noForkPath)) return false;
    // every list the same arms: the workgroups of one launch run the same program shape
    for (int o = L; o < n; ++o)
        if (pathSteps[(size_t) o].start != pathSteps[(size_t) (o % L)].start || pathSteps[(size_t) o].join != pathSteps[(size_t) (o % L)].join) return false;
    const uint32_t pbuf = (uint32_t) K * wg_block_bytes(S), mbuf = (uint32_t) (matrixFloats * 4);
    plan.inlineProg.resize((size_t) n);
    for (int o = 0; o < n; ++o) {
        // (a different scratch row for neighbouring entries, see the arena)
        plan.inlineProg[(size_t) o] = pathEntry(pathSteps[(size_t) o], pbuf, (uint32_t) MBAMD_WG_TW, mbuf, (int) scales.count() + (o % L) % MBAMD_WG_SCRATCH_ROWS);
        plan.inlineProg[(size_t) o].ctl |= (uint32_t) (o / L) << 10;
    }
    if (sw.verbose) std::fprintf(stderr, "[mbamd] walk plan: %d list(s) of %d operations each: root-ward paths%s (k_pathg)\n", nl, L, forked ? " that join" : "");
    plan.pathG = true;
    plan.lists = nl;
    pathPlan(plan, L, forked);
    return true;
}

// the instance's side of a 4-state kernel's arguments; the call site adds program, geometry and cumulative buffer
inline Walk4Args Instance::walk4Args() const
{
    Walk4Args a{};
    a.partials = reinterpret_cast<f4*>(arenaPartials);
    a.pstride = geom.pstride;
    a.tips = arenaTips;
    a.tstride = geom.tstride;
    a.exps = scales.nodeExponents();
    a.estride = scales.blockStride();
    a.matrices = matrices;
    a.K = K;
    a.Ppad = Ppad;
    a.nblocks = Ppad / 64;
    return a;
}

inline int Instance::runWalk(const Plan& plan, int32_t* cum)
{
    Walk4ArgsInline ai;
    Walk4Args& a = ai.a;
    a = walk4Args();
    a.cum = cum;
    if (!plan.inlineProg.empty()) std::memcpy(ai.inl, plan.inlineProg.data(), plan.inlineProg.size() * sizeof(Walk4Entry));
    if (plan.path) {
        a.entries = (int) plan.inlineProg.size();
        a.cumFresh = walkCumFresh ? 1 : 0;
        auto kernel = k_path4<Walk4ArgsInline>;
        MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, path4_lds_bytes((int) plan.inlineProg.size()), stream, ai);    // (lanes exchange through LDS: the emulation runs them as fibers)
        HIP_TRY(hipGetLastError());
        pendingLaunches += 1;
        return BEAGLE_SUCCESS;
    }
    for (const Plan::Segment& sg : plan.segments) {
        a.entries = sg.entries;
        a.nslots = sg.nslots;
        a.cumFresh = (walkCumFresh && &sg == &plan.segments.front()) ? 1 : 0;
        a.tail = sg.tail;
        bool plainHere = false;
        if (!plan.inlineProg.empty()) {
            auto kernel = k_walk4_t<Walk4ArgsInline>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64 * sg.W, walk4_lds_bytes(sg.W, sg.nslots), stream, ai);
        } else if (sg.waves) {
            // a whole-tree list cut over several waves, each on the plain loop: the program's own layout, no other kernel reads it
            a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
            auto kernel = k_walk4_t<Walk4Args, true, true>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64 * sg.W, walk4_waves_lds_bytes(sg.W, sg.nslots), stream, a);
            plainHere = true;
            if (!plan.unstoredSubtrees.empty()) { const int urc = leaveUnstored(plan); if (urc) return urc; }
        } else if (sg.plain && !sw.noPlainWalk) {
            // nothing rare in the program (a whole-tree list): the instantiation without that code; an odd operation count's padding entry joins the tail
            a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
            a.tail = sg.tail + (sg.peel ? 1 : 0);
            auto kernel = k_walk4_t<Walk4Args, true>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, sg.nslots), stream, a);
            plainHere = true;
            if (!plan.unstoredSubtrees.empty()) { const int urc = leaveUnstored(plan); if (urc) return urc; }
        } else {
            a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
            auto kernel = k_walk4_t<Walk4Args>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64 * sg.W, walk4_lds_bytes(sg.W, sg.nslots), stream, a);
        }
        HIP_TRY(hipGetLastError());
        ++(plainHere ? walksPlain : walksGeneric);
        if (plainHere) ++walksPlainByW[(sg.waves ? sg.W : 1) - 1];
        pendingLaunches += 1;
    }
    return BEAGLE_SUCCESS;
}

// ---------------------------------------------------------------------------------------------
// Small subtrees -- tip pairs, and subtrees of three and four compact tips -- that a whole-tree launch did not store (see the
// members: Recipe, unstored, d_snap).
// ---------------------------------------------------------------------------------------------
// behind a launch of the plain kernel whose program carries MBAMD_W4_NOSTORE entries: their destinations hold recipes from now on
inline int Instance::leaveUnstored(const Plan& plan)
{
    if (!d_snap) HIP_TRY(hipMalloc(&d_snap, (size_t) nBuffers * MBAMD_W4_SNAP * K * 16 * sizeof(float)));
    if (snapPlan && snapPlan != &plan) { int rc = flushSnapshot(); if (rc) return rc; }     // (the matrices are what they were at that launch: nothing overwrote one since)
    for (const Plan::Unstored& u : plan.unstoredSubtrees) {
        if (!unstored[(size_t) u.dst]) ++nUnstored;
        unstored[(size_t) u.dst] = 1;
        recipes[(size_t) u.dst] = u.r;
        ++(u.r.nops > 1 ? leftUnstoredSub : leftUnstored);
    }
    snapPlan = const_cast<Plan*>(&plan);
    return BEAGLE_SUCCESS;
}

// the waiting copy of the matrices of a launch's unstored subtrees into the snapshot table, now (k_walk4_snapshot reads the plan's own program)
inline int Instance::flushSnapshot()
{
    Plan* const plan = snapPlan;
    snapPlan = nullptr;
    if (!plan || plan->segments.size() != 1 || !plan->d_table) return BEAGLE_SUCCESS;
    const Plan::Segment& sg = plan->segments[0];
    plan->lastLaunch = ++launchClock;            // (the program must stay what it is until this launch has run: planTable)
    const unsigned nprog = sg.waves ? (unsigned) (sg.W * sg.entries) : (unsigned) (sg.entries - sg.tail);   // (several waves: [W][entries], the padding carries no flag)
    MBAMD_LAUNCH(k_walk4_snapshot, nprog + (unsigned) plan->sideCount, 64, 0, stream, reinterpret_cast<const Walk4Entry*>(plan->d_table) + sg.first,
                 nprog, reinterpret_cast<const Walk4Entry*>(plan->d_table) + plan->sideFirst, (unsigned) ((size_t) (Ppad / 64) * K), (const float*) matrices, d_snap, K);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// Every reader of partials, before its launch: the unstored buffers among `bufs` (indices out of range, tips and stored buffers are
// passed over) are recomputed into the arena by one launch of the generic k_walk4_t -- entries with both children tips, matrices from
// the snapshot table, no cumulative buffer, the exponent byte to the scratch rows -- and drop their recipes.  With a subtree of three or
// four tips among them the one launch is of the plain instantiation, through a device buffer (ensureStoredSubtrees).
inline int Instance::ensureStored(const int* bufs, int n)
{
    if (nUnstored == 0) return BEAGLE_SUCCESS;
    std::vector<int>& list = storeList;
    list.clear();
    for (int i = 0; i < n; ++i) {
        const int b = bufs[i];
        if (b < 0 || b >= nBuffers || unstored[(size_t) b] != 1) continue;
        unstored[(size_t) b] = 2;                // (named twice: listed once)
        list.push_back(b);
    }
    for (int b : list) unstored[(size_t) b] = 1;
    if (list.empty()) return BEAGLE_SUCCESS;
    int rc = flushSnapshot();
    if (rc) return rc;
    for (int b : list) if (recipes[(size_t) b].nops > 1) return ensureStoredSubtrees();
    const int m = (int) list.size(), entries = (m + 1) / 2 * 2 + 2;              // the kernel's loop runs two entries a turn and reads two ahead
    const uint32_t pbuf = (uint32_t) ((size_t) (Ppad / 64) * K), ebuf = (uint32_t) K * 64u, mbuf = (uint32_t) K * 64u;
    const uint32_t scratch = (uint32_t) scales.count();
    storeProg.resize((size_t) entries);
    for (int i = 0; i < entries; ++i) {
        Walk4Entry& e = storeProg[(size_t) i];
        std::memset(&e, 0, sizeof e);
        e.ctl = MBAMD_W4_NOP;
        e.ewrite = (scratch + (uint32_t) (i % MBAMD_W4_SCRATCH_ROWS)) * ebuf;
        e.eread = scratch * ebuf;
        if (i >= m) continue;
        const uint32_t b = (uint32_t) list[(size_t) i];
        const Recipe& r = recipes[b];
        e.ctl = MBAMD_W4_TIP1 | MBAMD_W4_TIP2 | ((uint32_t) r.op[0].mode << 8);
        e.dst = b * pbuf;
        e.c1 = (uint32_t) r.op[0].c1 * 32u;
        e.c2 = (uint32_t) r.op[0].c2 * 32u;
        e.m1 = ((uint32_t) MBAMD_W4_SNAP * b) * mbuf;
        e.m2 = ((uint32_t) MBAMD_W4_SNAP * b + 1u) * mbuf;
    }
    Walk4ArgsInline ai;
    Walk4Args& a = ai.a;
    a = walk4Args();
    a.matrices = d_snap;
    a.cum = nullptr;
    a.cumFresh = 0;
    a.entries = entries;
    a.nslots = 1;
    a.tail = 2;
    ++launchClock;
    if (entries <= MBAMD_W4_INLINE) {
        std::memcpy(ai.inl, storeProg.data(), (size_t) entries * sizeof(Walk4Entry));
        auto kernel = k_walk4_t<Walk4ArgsInline>;
        MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, 1), stream, ai);
    } else {
        const size_t bytes = (size_t) entries * sizeof(Walk4Entry);
        rc = grow(&d_storeProg, &storeProgCap, bytes);
        if (rc) return rc;
        rc = upload(d_storeProg, storeProg.data(), bytes);
        if (rc) return rc;
        a.prog = static_cast<const Walk4Entry*>(d_storeProg);
        auto kernel = k_walk4_t<Walk4Args>;
        MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, 1), stream, a);
    }
    HIP_TRY(hipGetLastError());
    for (int b : list) unstored[(size_t) b] = 0;
    nUnstored -= m;
    materialised += m;
    materialiseLaunches += 1;
    return BEAGLE_SUCCESS;
}

// storeList (every buffer in it unstored, the matrices snapshot) holds a subtree of three or four tips: ONE launch of the plain
// instantiation k_walk4_t<Walk4Args, true> -- the kernel and the entry kinds of the original launch: the same bits -- over the recipes'
// operations in post-order.  An inner operation carries MBAMD_W4_NOSTORE: its result reaches its parent through the forwarding
// registers or LDS slot 0 (the first tip pair of a balanced four) and lands nowhere else -- the arena slice of the inner buffer may
// hold something else by now.  Matrices from the buffer's snapshot slots, exponent bytes to the scratch rows, no cumulative buffer.
// A plain program has no form in the kernel arguments: it goes through d_storeProg, however short.
inline int Instance::ensureStoredSubtrees()
{
    const std::vector<int>& list = storeList;
    const uint32_t pbuf = (uint32_t) ((size_t) (Ppad / 64) * K), ebuf = (uint32_t) K * 64u, mbuf = (uint32_t) K * 64u;
    const uint32_t scratch = (uint32_t) scales.count();
    storeProg.clear();
    int pairs = 0, subtrees = 0;
    for (int b : list) {
        const Recipe& r = recipes[(size_t) b];
        ++(r.nops > 1 ? subtrees : pairs);
        for (int j = 0; j < r.nops; ++j) {
            const Recipe::Op& o = r.op[j];
            Walk4Entry e;
            std::memset(&e, 0, sizeof e);
            const bool last = j == r.nops - 1;
            // matrices: the buffer's own operation in snapshot slots 0 and 1, inner operation j in 2 + 2 j and 3 + 2 j
            const uint32_t mslot = (uint32_t) MBAMD_W4_SNAP * (uint32_t) b + (last ? 0u : 2u + 2u * (uint32_t) j);
            uint32_t flags = 0;
            // a child made by the operation in front is forwarded; one made two in front (the first tip pair of a balanced four) waits in slot 0
            if (!o.in1) { flags |= MBAMD_W4_TIP1; e.c1 = (uint32_t) o.c1 * 32u; }
            else if (o.c1 == j - 1) flags |= MBAMD_W4_FWD1;
            if (!o.in2) { flags |= MBAMD_W4_TIP2; e.c2 = (uint32_t) o.c2 * 32u; }
            else if (o.c2 == j - 1) flags |= MBAMD_W4_FWD2;
            for (int q = j + 2; q < r.nops; ++q)
                if ((r.op[q].in1 && r.op[q].c1 == j) || (r.op[q].in2 && r.op[q].c2 == j)) flags |= MBAMD_W4_KEEP;   // (slot 0: [23:16] stays zero)
            e.ctl = flags | ((uint32_t) o.mode << 8) | walk4_kind_of(flags) | (last ? 0u : MBAMD_W4_NOSTORE);
            e.dst = last ? (uint32_t) b * pbuf : 0u;
            e.m1 = mslot * mbuf;
            e.m2 = (mslot + 1u) * mbuf;
            e.ewrite = (scratch + (uint32_t) (storeProg.size() % MBAMD_W4_SCRATCH_ROWS)) * ebuf;
            e.eread = (flags & MBAMD_W4_TIP1) ? e.c1 : 0u;                   // (a plain program: child 1's plane offset or 0, Instance::buildWalk)
            storeProg.push_back(e);
        }
    }
    const int nops = (int) storeProg.size(), entries = (nops + 1) / 2 * 2 + 2;   // the read-ahead tail: valid offsets, nothing executed
    for (int i = nops; i < entries; ++i) {
        Walk4Entry e;
        std::memset(&e, 0, sizeof e);
        e.ctl = MBAMD_W4_NOP;
        e.ewrite = (scratch + (uint32_t) (i % MBAMD_W4_SCRATCH_ROWS)) * ebuf;
        storeProg.push_back(e);
    }
    Walk4Args a = walk4Args();
    a.matrices = d_snap;
    a.cum = nullptr;
    a.cumFresh = 0;
    a.entries = entries;
    a.nslots = 1;
    a.tail = entries - nops;
    ++launchClock;
    const size_t bytes = (size_t) entries * sizeof(Walk4Entry);
    int rc = grow(&d_storeProg, &storeProgCap, bytes);
    if (rc) return rc;
    rc = upload(d_storeProg, storeProg.data(), bytes);
    if (rc) return rc;
    a.prog = static_cast<const Walk4Entry*>(d_storeProg);
    auto kernel = k_walk4_t<Walk4Args, true>;
    MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, 1), stream, a);
    HIP_TRY(hipGetLastError());
    for (int b : list) unstored[(size_t) b] = 0;
    nUnstored -= (int) list.size();
    materialised += pairs;
    materialiseLaunches += pairs ? 1 : 0;
    materialisedSub += subtrees;
    materialiseLaunchesSub += 1;
    return BEAGLE_SUCCESS;
}

// a compact tip is about to change (new states, or partials in its place): the unstored buffers made from it are stored first
inline int Instance::storeUsersOfTip(int tip)
{
    if (nUnstored == 0) return BEAGLE_SUCCESS;
    std::vector<int> users;
    for (int b = 0; b < nBuffers; ++b)
        if (unstored[(size_t) b] && recipes[(size_t) b].usesTip(tip)) users.push_back(b);
    return users.empty() ? BEAGLE_SUCCESS : ensureStored(users.data(), (int) users.size());
}

// ---------------------------------------------------------------------------------------------
// 20/61-state tree walk (mbamd_walkg.h).  beagleUpdatePartials only queues: MrBayes submits one list per eigen-system
// part of a codon model (reference src/mbbeagle.c:1095-1104), and a forest of three trees fills the chip where one tree
// cannot.  The queue runs -- as ONE program per wave, hazards cut into segments like any list -- when the next call
// arrives that depends on it.
// ---------------------------------------------------------------------------------------------
inline int Instance::updatePartialsG(const BeagleOperation* ops, int n, int cumIdx)
{
    bool clash = (int) wgListCum.size() >= MBAMD_WG_MAXLISTS;
    if (cumIdx != BEAGLE_OP_NONE)
        for (int c : wgListCum) clash |= c == cumIdx;            // one list per cumulative buffer and launch
    if (clash) {
        int rc = flushPending();
        if (rc) return rc;
    }
    wgListStart.push_back((int) wgOps.size());
    wgListCum.push_back(cumIdx);
    wgOps.insert(wgOps.end(), ops, ops + n);
    if (sw.noDefer) return flushPending();
    return BEAGLE_SUCCESS;
}

// does a beagle{Accumulate,Remove}ScaleFactors call commute with the queued lists?  (MrBayes removes the old node factors
// of part j+1 between the lists of parts j and j+1, reference src/mbbeagle.c:1086-1104)
inline bool Instance::scaleOpsIndependentOfPending(const int* idx, int n, int cumIdx) const
{
    for (int c : wgListCum) if (c == cumIdx) return false;
    for (const BeagleOperation& b : wgOps) {
        if (b.destinationScaleWrite == cumIdx || b.destinationScaleRead == cumIdx) return false;
        for (int i = 0; i < n; ++i)
            if (b.destinationScaleWrite == idx[i]) return false;
    }
    for (int i = 0; i < n; ++i)
        for (int c : wgListCum) if (c == idx[i]) return false;
    return true;
}

inline int Instance::flushWalkG()
{
    if (wgListCum.empty()) return BEAGLE_SUCCESS;
    std::vector<BeagleOperation> ops;
    std::vector<int> starts, cums;
    ops.swap(wgOps); starts.swap(wgListStart); cums.swap(wgListCum);
    const int n = (int) ops.size();
    int nl = (int) cums.size();
    std::vector<int> listOf(n, 0);
    for (int q = 0; q < nl; ++q)
        for (int o = starts[q]; o < (q + 1 < nl ? starts[q + 1] : n); ++o) listOf[o] = q;
    // ---- plan cache key: the operations as submitted and the list boundaries ---------------------------------------------
    std::vector<int> key(reinterpret_cast<const int*>(ops.data()), reinterpret_cast<const int*>(ops.data()) + (size_t) n * 7);
    for (int q = 0; q < nl; ++q) key.push_back(starts[q]);
    // One list that does not rescale may hold several independent trees: without a cumulative buffer MrBayes submits the
    // operations of all eigen-system parts as ONE list (reference src/mbbeagle.c:1029-1104, No_Rescale), and a move dirties
    // the same root-ward path in each part.  Its connected components are treated like lists of their own.
    if (nl == 1 && cums[0] == BEAGLE_OP_NONE && n >= 2) {
        std::vector<int> comp(n);
        for (int o = 0; o < n; ++o) comp[o] = o;
        auto find = [&](int x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
        std::unordered_map<int, int> writer, scaleUser;
        bool ok = true;
        for (int o = 0; o < n && ok; ++o) {
            const BeagleOperation& b = ops[o];
            for (int c : {b.child1Partials, b.child2Partials}) {
                auto it = writer.find(c);
                if (it != writer.end()) comp[find(o)] = find(it->second);
            }
            if (writer.count(b.destinationPartials)) ok = false;            // (written twice: leave it to the hazard segments)
            writer[b.destinationPartials] = o;
            for (int sc : {b.destinationScaleWrite, b.destinationScaleRead})
                if (sc != BEAGLE_OP_NONE) {
                    auto it = scaleUser.find(sc);
                    if (it != scaleUser.end()) comp[find(o)] = find(it->second); else scaleUser[sc] = o;
                }
        }
        for (int o = 0; o < n && ok; ++o)                                    // a buffer read before a later operation writes it
            for (int c : {ops[o].child1Partials, ops[o].child2Partials}) {
                auto it = writer.find(c);
                if (it != writer.end() && it->second > o) ok = false;
            }
        std::vector<int> roots;
        for (int o = 0; o < n && ok; ++o) if (find(o) == o) roots.push_back(o);
        if (ok && roots.size() >= 2 && roots.size() <= (size_t) MBAMD_WG_MAXLISTS) {
            std::vector<BeagleOperation> sorted;
            sorted.reserve(n);
            starts.clear();
            for (size_t q = 0; q < roots.size(); ++q) {
                starts.push_back((int) sorted.size());
                for (int o = 0; o < n; ++o) if (find(o) == roots[q]) sorted.push_back(ops[o]);
            }
            ops.swap(sorted);
            nl = (int) roots.size();
            cums.assign(nl, BEAGLE_OP_NONE);
            for (int q = 0; q < nl; ++q)
                for (int o = starts[q]; o < (q + 1 < nl ? starts[q + 1] : n); ++o) listOf[o] = q;
        }
    }
    wgFresh = 0;
    for (int q = 0; q < MBAMD_WG_MAXLISTS; ++q) wgCum[q] = nullptr;
    for (int q = 0; q < nl; ++q) {
        const int ci = cums[q];
        if (ci == BEAGLE_OP_NONE) continue;
        bool fresh;
        int rc = scales.cumulativeForAdd(ci, wgCum[q], fresh);
        if (rc) return rc;
        if (fresh) wgFresh |= 1 << q;
    }
    bool build;
    Plan* plan = cachedPlan(key.data(), key.size(), build);
    if (build) {
        // Mutually independent lists (the eigen-system parts of a codon model) run as separate workgroups of ONE launch --
        // three times the workgroups for a grid that does not fill the chip otherwise -- if they compile to the same geometry;
        // anything else is one merged forest.
        bool independent = nl > 1;
        if (independent) {
            std::vector<int> wr(nBuffers, -1), rd(nBuffers, -1);
            std::vector<int> sc(scales.count(), -1);
            for (int o = 0; o < n && independent; ++o) {
                const BeagleOperation& b = ops[o];
                const int q = listOf[o];
                auto clash = [&](std::vector<int>& v, int i) { if (i < 0 || i >= (int) v.size()) return false; if (v[i] >= 0 && v[i] != q) return true; v[i] = q; return false; };
                if (clash(wr, b.destinationPartials) || (b.destinationPartials >= 0 && b.destinationPartials < nBuffers && rd[b.destinationPartials] >= 0 && rd[b.destinationPartials] != q)) independent = false;
                for (int c : {b.child1Partials, b.child2Partials})
                    if (c >= 0 && c < nBuffers && !(tipStates[c] && wr[c] < 0)) {
                        if (wr[c] >= 0 && wr[c] != q) independent = false;
                        if (rd[c] < 0) rd[c] = q; else if (rd[c] != q) rd[c] = 1 << 20;      // (read by several lists: fine unless one writes it)
                    }
                if (b.destinationScaleWrite != BEAGLE_OP_NONE && clash(sc, b.destinationScaleWrite)) independent = false;
                if (b.destinationScaleRead != BEAGLE_OP_NONE && b.destinationScaleRead >= 0 && b.destinationScaleRead < (int) sc.size() &&
                    sc[b.destinationScaleRead] >= 0 && sc[b.destinationScaleRead] != q) independent = false;
            }
            for (int o = 0; o < n && independent; ++o)                  // a buffer one list writes must not be read by another
                for (int c : {ops[o].child1Partials, ops[o].child2Partials})
                    if (c >= 0 && c < nBuffers && wr[c] >= 0 && wr[c] != listOf[o]) independent = false;
            if (sw.verbose) std::fprintf(stderr, "[mbamd] %d queued lists, %d operations: %s\n", nl, n, independent ? "independent" : "one forest");
        }
        int rc;
        {
            StatTimer st_(ST_PLAN);
            plan->lists = 1;
            plan->pathG = plan->forked = false;
            rc = BEAGLE_SUCCESS;
            bool done = (nl == 1 || independent) && buildPathG(*plan, ops.data(), n, starts, nl);
            if (!done) { plan->inlineProg.clear(); plan->pathG = plan->forked = false; }
            if (!done && independent) {
                const int keepW = w4.maxW, keepS = w4.maxSlots, keepS1 = w4.maxSlots1;
                wgGeometry(nl, w4.maxW, w4.maxSlots);
                w4.maxSlots1 = w4.maxSlots;
                rc = buildWalk(*plan, ops.data(), n, listOf.data(), true);
                w4.maxW = keepW; w4.maxSlots = keepS; w4.maxSlots1 = keepS1;
                bool same = rc == BEAGLE_SUCCESS && (int) plan->segments.size() == nl;
                for (size_t i = 1; same && i < plan->segments.size(); ++i)
                    same = plan->segments[i].W == plan->segments[0].W && plan->segments[i].entries == plan->segments[0].entries &&
                           plan->segments[i].first == plan->segments[0].first + i * (size_t) plan->segments[0].W * plan->segments[0].entries;
                if (same) {
                    int ns = 0;
                    for (const Plan::Segment& sg : plan->segments) ns = std::max(ns, sg.nslots);
                    for (Plan::Segment& sg : plan->segments) sg.nslots = ns;
                    plan->lists = nl;
                    done = true;
                    // (several independent lists = several segments, one launch: short enough, they travel in its arguments too)
                    if (!sw.noInlinePrograms && w4table.size() <= (size_t) MBAMD_W4_INLINE) plan->inlineProg = w4table;
                }
            }
            if (!done) rc = buildWalk(*plan, ops.data(), n, listOf.data(), false);
        }
        if (planBuilt(*plan, rc)) return rc;
    }
    // one flush = one list event, however many eigen-system parts it carries
    listLaunched(ops.data(), n, plan->pathG, plan->forked);
    // Which instantiation of the bf16-piece contraction (wgRescaled).  Here, not earlier: the plan exists, so every index of every
    // operation has been checked (checkOperation, when this list or an identical one was compiled).  The operations in the order
    // they run: a child an earlier operation of the flush writes is what that operation leaves (wgWrote: -1 not written, else
    // whether it rescales), whatever the buffer held before -- compact states included.  The buffers' own marks change only once
    // the launch has been accepted; a launch that failed leaves results nobody knows.
    const bool pieces = S >= MBAMD_WG_BF_MIN;
    wgRangeSafe = false;
    if (pieces) {
        if (wgRescaled.size() != (size_t) nBuffers) wgRescaled.assign((size_t) nBuffers, 0);
        wgWrote.assign((size_t) nBuffers, -1);
        for (const BeagleOperation& b : ops) {
            for (int c : {b.child1Partials, b.child2Partials}) {
                const int8_t w = wgWrote[(size_t) c];
                if (w >= 0 ? w == 0 : (!tipStates[c] && !wgRescaled[(size_t) c])) wgRangeSafe = true;
            }
            wgWrote[(size_t) b.destinationPartials] = b.destinationScaleWrite != BEAGLE_OP_NONE ? 1 : 0;
        }
        ++(wgRangeSafe ? wgFlushesRangeSafe : wgFlushesPlain);
    }
    const int rrc = timedRun(*plan, nullptr);
    if (pieces)
        for (const BeagleOperation& b : ops) wgRescaled[(size_t) b.destinationPartials] = rrc == BEAGLE_SUCCESS && wgWrote[(size_t) b.destinationPartials] == 1 ? 1 : 0;
    return rrc;
}

template <int SC_, int WMAX_, int CH_, int DEPTH_>
inline void Instance::launch_walkg_t(Instance& in, const WalkGArgs& a, int W, int nslots, const std::vector<Walk4Entry>* inlineProg)
{
    if (inlineProg && !inlineProg->empty()) {
        WalkGArgsInline ai;
        ai.a = a;
        ai.a.prog = nullptr;
        std::memcpy(ai.inl, inlineProg->data(), inlineProg->size() * sizeof(Walk4Entry));
        if constexpr (WgShape<SC_>::BF) {
            if (in.wgRangeSafe) {
                auto safe = k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgsInline, true>;
                MBAMD_LAUNCH_BARRIER(safe, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 64 * W * (a.spread ? 2 : 1), wg_lds_bytes(W, nslots, in.S), in.stream, ai);
                return;
            }
        }
        auto kern = k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgsInline>;
        MBAMD_LAUNCH_BARRIER(kern, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 64 * W * (a.spread ? 2 : 1), wg_lds_bytes(W, nslots, in.S), in.stream, ai);
        return;
    }
    if constexpr (WgShape<SC_>::BF) {
        if (in.wgRangeSafe) {
            auto safe = k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgs, true>;
            MBAMD_LAUNCH_BARRIER(safe, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 64 * W * (a.spread ? 2 : 1), wg_lds_bytes(W, nslots, in.S), in.stream, a);
            return;
        }
    }
    auto kern = k_walkg<SC_, WMAX_, CH_, DEPTH_>;
    MBAMD_LAUNCH_BARRIER(kern, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 64 * W * (a.spread ? 2 : 1), wg_lds_bytes(W, nslots, in.S), in.stream, a);
}

template <int SC_>
inline void Instance::launch_pathg_t(Instance& in, const WalkGArgs& a, const std::vector<Walk4Entry>& prog, bool forked)
{
    WalkGArgsInline ai;
    ai.a = a;
    ai.a.prog = nullptr;
    std::memcpy(ai.inl, prog.data(), prog.size() * sizeof(Walk4Entry));
    if constexpr (WgShape<SC_>::BF) {
        if (in.wgRangeSafe) {
            if (forked) {
                auto safe = k_pathg<SC_, WalkGArgsInline, true, true>;
                MBAMD_LAUNCH_BARRIER(safe, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 128, pathg_lds_bytes(in.S, true), in.stream, ai);
            } else {
                auto safe = k_pathg<SC_, WalkGArgsInline, false, true>;
                MBAMD_LAUNCH_BARRIER(safe, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 128, pathg_lds_bytes(in.S), in.stream, ai);
            }
            return;
        }
    }
    if (forked) {
        auto kern = k_pathg<SC_, WalkGArgsInline, true>;
        MBAMD_LAUNCH_BARRIER(kern, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 128, pathg_lds_bytes(in.S, true), in.stream, ai);
        return;
    }
    auto kern = k_pathg<SC_, WalkGArgsInline>;
    MBAMD_LAUNCH_BARRIER(kern, walkg_grid(in.Ppad / MBAMD_WG_TW, in.K * a.lists), 128, pathg_lds_bytes(in.S), in.stream, ai);
}

// the instance's side of a general-state walk's arguments, with the cumulative buffers of the lists being flushed; the call
// site adds program, geometry and which of those buffers are fresh
inline WalkGArgs Instance::walkGArgs() const
{
    WalkGArgs a;
    std::memset(&a, 0, sizeof a);
    a.partials = arenaPartials;
    a.tileBytes = wgTileBytes;
    a.tips = arenaTipStates;
    a.tipTileBytes = wgTipTileBytes;
    a.exps = scales.nodeExponents();
    a.estride = scales.blockStride();
    a.matrices = matrices;
    a.tabOff = (unsigned) (wgTabFloats * 4);
    a.tabBytes = (unsigned) (wg_table_floats(S) * 4);
    for (int q = 0; q < MBAMD_WG_MAXLISTS; ++q) a.cum[q] = wgCum[q];
    a.K = K; a.Ppad = Ppad; a.ntiles = Ppad / MBAMD_WG_TW; a.S = S; a.SP = SP;
    return a;
}

inline int Instance::runWalkG(const Plan& plan)
{
    WalkGArgs a = walkGArgs();
    a.lists = plan.lists;
    if (plan.pathG) {
        a.entries = plan.segments.front().entries;
        a.cumFresh = wgFresh;
        switch (S) {
            case 20: launch_pathg_t<20>(*this, a, plan.inlineProg, plan.forked); break;
            case 60: launch_pathg_t<60>(*this, a, plan.inlineProg, plan.forked); break;
            case 61: launch_pathg_t<61>(*this, a, plan.inlineProg, plan.forked); break;
            case 62: launch_pathg_t<62>(*this, a, plan.inlineProg, plan.forked); break;
            default: launch_pathg_t<63>(*this, a, plan.inlineProg, plan.forked); break;
        }
        HIP_TRY(hipGetLastError());
        pendingLaunches += 1;
        return BEAGLE_SUCCESS;
    }
    for (const Plan::Segment& sg : plan.segments) {
        if (plan.lists > 1 && &sg != &plan.segments.front()) break;     // (independent lists: one launch covers all segments)
        a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
        a.entries = sg.entries;
        a.nslots = sg.nslots;
        a.cumFresh = (&sg == &plan.segments.front()) ? wgFresh : 0;
        a.spread = sg.W == 2 ? 1 : 0;     // two-wave workgroups are launched as four (see k_walkg)
        MBAMD_WG_DISPATCH(S, launch_walkg_t, *this, a, sg.W, sg.nslots, &plan.inlineProg);
        HIP_TRY(hipGetLastError());
        pendingLaunches += 1;
    }
    return BEAGLE_SUCCESS;
}

template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_t(Instance& in, const PartialsOp* ops, int count, int32_t* cum)
{
    const int gx = (in.Ppad + 127) / 128;
    const unsigned grid = (unsigned) (8 * ((gx + 7) / 8) * count);
    auto kern = k_partials_mfma<NT_, SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, grid, 256, 0, in.stream, ops, in.S, in.SP, in.Ppad, gx, cum);
}
template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_split_t(Instance& in, const OpTables& tabs, int count)
{
    constexpr int NP = 2 * KC_ * NT_;
    const int gx = in.Ppad / 32;
    auto kern = k_partials_mfma_split<NT_, SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx * count), 64 * NP, (size_t) NP * (8 * 64 + 32 + 16 * 32) * sizeof(float), in.stream, tabs, in.S,
                 in.SP, in.Ppad, gx);
}
// one launch over up to four operation tables (false: no split kernel for this shape)
inline bool Instance::launch_mfma_split(Instance& in, const OpTables& tabs, int count)
{
    const int S = in.S, K = in.K;
    if (in.NT == 1 && S == 20 && K == 4) { launch_mfma_split_t<1, 20, 4>(in, tabs, count); return true; }
    if (in.NT == 1 && S == 20 && K == 1) { launch_mfma_split_t<1, 20, 1>(in, tabs, count); return true; }
    if (in.NT == 2 && S == 61 && K == 1) { launch_mfma_split_t<2, 61, 1>(in, tabs, count); return true; }
    if (in.NT == 1 && K == 1) { launch_mfma_split_t<1, 0, 1>(in, tabs, count); return true; }
    if (in.NT == 1 && K == 2) { launch_mfma_split_t<1, 0, 2>(in, tabs, count); return true; }
    if (in.NT == 1 && K == 4) { launch_mfma_split_t<1, 0, 4>(in, tabs, count); return true; }
    if (in.NT == 2 && K == 1) { launch_mfma_split_t<2, 0, 1>(in, tabs, count); return true; }
    if (in.NT == 2 && K == 2) { launch_mfma_split_t<2, 0, 2>(in, tabs, count); return true; }
    return false;
}
template <int SC_, int KC_>
inline void Instance::launch_tips_t(Instance& in, const OpTables& tabs, int count)
{
    const int gx4 = (in.Ppad + 127) / 128;
    auto kern = k_partials_tips<SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx4 * count), 256, (size_t) 4 * in.S * 32 * sizeof(float), in.stream, tabs, in.S, in.SP, in.Ppad, gx4);
}
// operations on two compact tips, up to four tables (false: no kernel for this shape)
inline bool Instance::launch_tips(Instance& in, const OpTables& tabs, int count)
{
    const int S = in.S, K = in.K;
    if (S > 64) return false;
    if (S == 20 && K == 4) { launch_tips_t<20, 4>(in, tabs, count); return true; }
    if (S == 20 && K == 1) { launch_tips_t<20, 1>(in, tabs, count); return true; }
    if (S == 61 && K == 1) { launch_tips_t<61, 1>(in, tabs, count); return true; }
    if (K == 1) { launch_tips_t<0, 1>(in, tabs, count); return true; }
    if (K == 2 && S <= 32) { launch_tips_t<0, 2>(in, tabs, count); return true; }
    return false;
}
// MBAMD_WALK_TRACE: the buffer the serial MFMA kernels stamp their steps into, allocated when the first of them is launched
inline void Instance::ensureTrace()
{
    if (d_trace || !sw.walkTrace) return;
    if (hipMalloc(&d_trace, (size_t) 4096 * 8 * 3 * sizeof(long long)) != hipSuccess) d_trace = nullptr;
    else (void) hipMemset(d_trace, 0, (size_t) 4096 * 8 * 3 * sizeof(long long));
}
template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_serial_t(Instance& in, const OpTables& tabs, int ntables)
{
    constexpr int NP = 2 * KC_ * NT_;
    const int gx = in.Ppad / 32;
    auto kern = k_partials_mfma_serial<NT_, SC_, KC_>;
    in.ensureTrace();
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx * ntables), 64 * NP, (size_t) NP * (8 * 64 + 32 + 16 * 32) * sizeof(float), in.stream, tabs, in.S,
                 in.SP, in.Ppad, gx, in.d_trace);
    if (in.d_trace) { in.lastWalkSteps = tabs.start[0]; in.walkWaves = NP - 1; }
}
template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_spine_t(Instance& in, const OpTables& tabs, int ntables)
{
    constexpr int NP = 2 * KC_ * NT_;
    const int gx = in.Ppad / 32;
    in.ensureTrace();
    auto kern = k_partials_mfma_spine<NT_, SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx * ntables), 64 * (NP + 1), ((size_t) NP * (8 * 64 + 32) + (size_t) 2 * KC_ * SC_ * 32) * sizeof(float),
                 in.stream, tabs, in.SP, gx, in.d_trace);
    if (in.d_trace) { in.lastWalkSteps = tabs.start[0]; in.walkWaves = NP - 1; }
}
// one launch that walks up to four whole (narrow) operation lists; tabs.start[t] = operations of list t
inline bool Instance::launch_mfma_serial(Instance& in, const OpTables& tabs, int ntables)
{
    const int S = in.S, K = in.K;
    if (!in.sw.noSpine) {                           // software-pipelined variant (MBAMD_NO_SPINE=1: plain serial kernel)
        if (in.NT == 1 && S == 20 && K == 4) { launch_mfma_spine_t<1, 20, 4>(in, tabs, ntables); return true; }
        if (in.NT == 1 && S == 20 && K == 1) { launch_mfma_spine_t<1, 20, 1>(in, tabs, ntables); return true; }
        if (in.NT == 2 && S == 61 && K == 1) { launch_mfma_spine_t<2, 61, 1>(in, tabs, ntables); return true; }
    }
    if (in.NT == 1 && S == 20 && K == 4) { launch_mfma_serial_t<1, 20, 4>(in, tabs, ntables); return true; }
    if (in.NT == 1 && S == 20 && K == 1) { launch_mfma_serial_t<1, 20, 1>(in, tabs, ntables); return true; }
    if (in.NT == 2 && S == 61 && K == 1) { launch_mfma_serial_t<2, 61, 1>(in, tabs, ntables); return true; }
    if (in.NT == 1 && K == 1) { launch_mfma_serial_t<1, 0, 1>(in, tabs, ntables); return true; }
    if (in.NT == 1 && K == 2) { launch_mfma_serial_t<1, 0, 2>(in, tabs, ntables); return true; }
    if (in.NT == 1 && K == 4) { launch_mfma_serial_t<1, 0, 4>(in, tabs, ntables); return true; }
    if (in.NT == 2 && K == 1) { launch_mfma_serial_t<2, 0, 1>(in, tabs, ntables); return true; }
    if (in.NT == 2 && K == 2) { launch_mfma_serial_t<2, 0, 2>(in, tabs, ntables); return true; }
    return false;
}
inline bool Instance::launch_mfma(Instance& in, const PartialsOp* ops, int count, int32_t* cum)
{
    const int S = in.S, K = in.K;
    if (!in.sw.mfmaWhole) {                 // default: one wave per factor tile (MBAMD_MFMA_WHOLE=1 selects the wave-per-tile-column kernel)
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        tabs.ops[0] = ops;
        tabs.cum[0] = cum;
        for (int t = 1; t <= MBAMD_MAX_TABLES; ++t) tabs.start[t] = 1 << 30;
        if (launch_mfma_split(in, tabs, count)) return true;
    }
    if (in.NT == 1) {
        if (S == 20 && K == 4) launch_mfma_t<1, 20, 4>(in, ops, count, cum);
        else if (S == 20 && K == 1) launch_mfma_t<1, 20, 1>(in, ops, count, cum);
        else if (K == 1) launch_mfma_t<1, 0, 1>(in, ops, count, cum);
        else if (K == 2) launch_mfma_t<1, 0, 2>(in, ops, count, cum);
        else if (K == 3) launch_mfma_t<1, 0, 3>(in, ops, count, cum);
        else if (K == 4) launch_mfma_t<1, 0, 4>(in, ops, count, cum);
        else return false;
    } else {
        if (S == 61 && K == 1) launch_mfma_t<2, 61, 1>(in, ops, count, cum);
        else if (K == 1) launch_mfma_t<2, 0, 1>(in, ops, count, cum);
        else if (K == 2) launch_mfma_t<2, 0, 2>(in, ops, count, cum);
        else return false;
    }
    return true;
}

template <int SP_, int FK_>
inline void Instance::launch_gen(Instance& in, const PartialsOp* ops, int count, int32_t* cum)
{
    auto kern = k_partials_gen<SP_, FK_>;
    MBAMD_LAUNCH(kern, dim3(in.Ppad / 64, count), 64, 0, in.stream, ops, in.S, in.K, in.Ppad, cum);
}

// General path: order the operations by dependency level (RAW, WAR and WAW on buffer indices) and
// launch one grid per level.
inline int Instance::buildGeneric(Plan& plan, std::vector<PartialsOp>& dev, const std::vector<int>& dstIdx,
                           const std::vector<int>& c1Idx, const std::vector<int>& c2Idx)
{
    const int n = (int) dev.size();
    std::vector<int> lastWrite(nBuffers, -1), lastRead(nBuffers, -1), level(n, 0);
    // scale buffers are dependencies too: an operation that divides by the factors of a buffer (SCALE_READ) must run after
    // the operation of this list that writes them, a second writer after the first writer and all its readers
    std::unordered_map<const void*, std::pair<int, int>> scaleLevels;     // scale buffer -> (last write level, last read level)
    int nLevels = 0;
    for (int o = 0; o < n; ++o) {
        int l = 0;
        l = std::max(l, lastWrite[c1Idx[o]] + 1);
        l = std::max(l, lastWrite[c2Idx[o]] + 1);
        l = std::max(l, lastWrite[dstIdx[o]] + 1);
        l = std::max(l, lastRead[dstIdx[o]] + 1);
        if (dev[o].scale_mode != SCALE_NONE) {
            auto it = scaleLevels.find(dev[o].scale);
            if (it != scaleLevels.end()) {
                l = std::max(l, it->second.first + 1);
                if (dev[o].scale_mode == SCALE_WRITE) l = std::max(l, it->second.second + 1);
            }
        }
        level[o] = l;
        if (dev[o].scale_mode != SCALE_NONE) {
            auto& sl = scaleLevels.emplace(dev[o].scale, std::make_pair(-1, -1)).first->second;
            if (dev[o].scale_mode == SCALE_WRITE) sl.first = l; else sl.second = std::max(sl.second, l);
        }
        lastWrite[dstIdx[o]] = l;
        lastRead[c1Idx[o]] = std::max(lastRead[c1Idx[o]], l);
        lastRead[c2Idx[o]] = std::max(lastRead[c2Idx[o]], l);
        nLevels = std::max(nLevels, l + 1);
    }
    std::vector<int> start(nLevels + 1, 0);
    for (int o = 0; o < n; ++o) start[level[o] + 1]++;
    for (int l = 0; l < nLevels; ++l) start[l + 1] += start[l];
    std::vector<PartialsOp> sorted(n);
    {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int o = 0; o < n; ++o) sorted[fill[level[o]]++] = dev[o];
    }
    // level 0: operations on two compact tips first (they get their own kernel)
    auto tipPair = [](const PartialsOp& d) { return d.c1_kind == CHILD_STATES && d.c2_kind == CHILD_STATES; };
    plan.tipTip = nLevels > 0 ? (int) (std::stable_partition(sorted.begin(), sorted.begin() + start[1], tipPair) - sorted.begin()) : 0;
    plan.anyScale = false;
    for (const PartialsOp& d : sorted) plan.anyScale |= d.scale_mode != SCALE_NONE;
    plan.start = start;
    plan.narrow = serialRatio > 0 && n <= serialRatio * nLevels;
    // Independent sub-lists.  A list often is several root-ward paths interleaved (MrBayes puts the operations of all
    // eigen-system parts of a codon model into one list, reference src/mbbeagle.c:1029-1100).  chainsOf() splits a
    // subset of the list (original indices, list order) into connected components of the "touches a buffer a member
    // writes" relation and packs them into at most MBAMD_MAX_TABLES bins; the serial kernel walks the bins side by side.
    auto chainsOf = [&](const std::vector<int>& sub) {
        const int m = (int) sub.size();
        std::vector<int> comp(m);
        for (int x = 0; x < m; ++x) comp[x] = x;
        auto find = [&](int x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
        auto unite = [&](int a, int b) { a = find(a); b = find(b); if (a != b) comp[std::max(a, b)] = std::min(a, b); };
        std::vector<int> owner(nBuffers, -1);                    // a member that writes the buffer
        for (int x = 0; x < m; ++x) {
            const int o = sub[x];
            if (owner[dstIdx[o]] >= 0) unite(x, owner[dstIdx[o]]);
            owner[dstIdx[o]] = x;
        }
        for (int x = 0; x < m; ++x) {
            const int o = sub[x];
            if (owner[c1Idx[o]] >= 0) unite(x, owner[c1Idx[o]]);
            if (owner[c2Idx[o]] >= 0) unite(x, owner[c2Idx[o]]);
        }
        for (int x = 0; x < m; ++x)                              // node scale buffers written by one, used by another
            for (int y = x + 1; y < m; ++y) {
                const PartialsOp &dx = dev[sub[x]], &dy = dev[sub[y]];
                if (dx.scale == dy.scale && dx.scale_mode != SCALE_NONE && dy.scale_mode != SCALE_NONE &&
                    (dx.scale_mode == SCALE_WRITE || dy.scale_mode == SCALE_WRITE))
                    unite(x, y);
            }
        std::vector<int> roots, size(m, 0);
        for (int x = 0; x < m; ++x) { size[find(x)]++; if (find(x) == x) roots.push_back(x); }
        std::sort(roots.begin(), roots.end(), [&](int a, int b) { return size[a] > size[b]; });
        const int nb = std::min<int>(MBAMD_MAX_TABLES, (int) roots.size());
        std::vector<int> binLen(nb, 0), binOf(m, 0);
        for (int r : roots) {                                    // largest first, each into the currently shortest bin
            const int bsel = (int) (std::min_element(binLen.begin(), binLen.end()) - binLen.begin());
            binOf[r] = bsel;
            binLen[bsel] += size[r];
        }
        std::vector<std::vector<int>> bins(nb);
        for (int x = 0; x < m; ++x) bins[binOf[find(x)]].push_back(sub[x]);
        return bins;
    };
    auto appendBins = [&](const std::vector<std::vector<int>>& bins, std::vector<std::pair<int, int>>& out) {
        for (const auto& bin : bins) {
            if (bin.empty()) continue;
            out.emplace_back((int) sorted.size(), (int) bin.size());
            for (int o : bin) sorted.push_back(dev[o]);          // (list order inside a bin = dependency order)
        }
    };
    plan.chains.clear();
    plan.spineChains.clear();
    plan.serialFrom = nLevels;
    if (plan.narrow) {
        std::vector<int> all(n);
        for (int o = 0; o < n; ++o) all[o] = o;
        const auto bins = chainsOf(all);
        if (bins.size() > 1) appendBins(bins, plan.chains);
        else plan.chains.emplace_back(0, n);
    } else if (serialRatio > 0) {
        // the tail of a level-launched list: trailing levels of a few operations each.  If they fall apart into parallel
        // chains (three codon parts -> three chains) one serial launch walks them side by side; otherwise only the
        // strictly single-operation levels (the spine towards the root) go serial.
        int from = nLevels;
        while (from > 0 && start[from] - start[from - 1] <= MBAMD_MAX_TABLES) from--;
        if (nLevels - from >= 2) {
            std::vector<int> sub;
            for (int o = 0; o < n; ++o) if (level[o] >= from) sub.push_back(o);
            const auto bins = chainsOf(sub);
            size_t longest = 0;
            for (const auto& bin : bins) longest = std::max(longest, bin.size());
            if (bins.size() >= 2 && 4 * longest <= 5 * (size_t) (nLevels - from)) {
                plan.serialFrom = from;
                appendBins(bins, plan.spineChains);
            }
        }
        if (plan.spineChains.empty()) {
            from = nLevels;
            const int spineWidth = std::max(1, sw.spineWidth.value_or(1));   // trailing levels of at most this many operations join
            while (from > 0 && start[from] - start[from - 1] <= spineWidth) from--;
            if (nLevels - from >= 2) {
                plan.serialFrom = from;
                plan.spineChains.emplace_back(start[from], n - start[from]);
            }
        }
    }
    return planTable(plan, sorted.data(), sorted.size() * sizeof(PartialsOp));
}

inline int Instance::runGeneric(const Plan& plan, int32_t* cum)
{
    const std::vector<int>& start = plan.start;
    const int nLevels = (int) start.size() - 1;
    const bool anyScale = plan.anyScale;
    if (plan.narrow && mfma && !sw.mfmaWhole) {
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int nt = 0;
        for (auto& ch : plan.chains) {
            tabs.ops[nt] = plan.d_table + ch.first;
            tabs.cum[nt] = cum;
            tabs.start[nt] = ch.second;
            ++nt;
        }
        if (launch_mfma_serial(*this, tabs, nt)) {
            pendingLaunches += 1;
            HIP_TRY(hipGetLastError());
            return BEAGLE_SUCCESS;
        }
    }
    int levelEnd = nLevels;
    if (mfma && !sw.mfmaWhole) levelEnd = plan.serialFrom;
    for (int l = 0; l < levelEnd; ++l) {
        int off = start[l];
        int remaining = start[l + 1] - start[l];
        if (l == 0 && mfma && !sw.mfmaWhole && plan.tipTip > 0 && plan.tipTip <= 8192) {
            OpTables tabs;
            std::memset(&tabs, 0, sizeof tabs);
            tabs.ops[0] = plan.d_table;
            tabs.cum[0] = cum;
            for (int t = 1; t <= MBAMD_MAX_TABLES; ++t) tabs.start[t] = 1 << 30;
            if (launch_tips(*this, tabs, plan.tipTip)) {
                pendingLaunches += 1;
                off += plan.tipTip;
                remaining -= plan.tipTip;
            }
        }
        while (remaining > 0) {
            const int count = std::min(remaining, 32768);
            const PartialsOp* ops = plan.d_table + off;
            bool fused = true;
            if (mfma && launch_mfma(*this, ops, std::min(count, 8192), cum)) {
                const int done = std::min(count, 8192);
                pendingLaunches += 1;
                off += done;
                remaining -= done;
                continue;
            }
            if (SP == 20 && K == 4) launch_gen<20, 4>(*this, ops, count, cum);
            else if (SP == 20 && K == 1) launch_gen<20, 1>(*this, ops, count, cum);
            else if (SP == 64 && K == 1) launch_gen<64, 1>(*this, ops, count, cum);
            else if (SP == 4 && K == 4) launch_gen<4, 4>(*this, ops, count, cum);
            else if (SP == 4 && K == 1) launch_gen<4, 1>(*this, ops, count, cum);
            else {
                fused = false;
                switch (SP) {
                    case 4: launch_gen<4, 0>(*this, ops, count, cum); break;
                    case 8: launch_gen<8, 0>(*this, ops, count, cum); break;
                    case 16: launch_gen<16, 0>(*this, ops, count, cum); break;
                    case 20: launch_gen<20, 0>(*this, ops, count, cum); break;
                    case 32: launch_gen<32, 0>(*this, ops, count, cum); break;
                    default: launch_gen<64, 0>(*this, ops, count, cum); break;
                }
            }
            pendingLaunches += 1;
            if (!fused && anyScale) {
                MBAMD_LAUNCH(k_rescale_gen, dim3(Ppad / 64, count), 64, 0, stream, ops, S, K, Ppad, cum);
                pendingLaunches += 1;
            }
            off += count;
            remaining -= count;
        }
    }
    if (levelEnd < nLevels) {                    // the spine: one launch walks it
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int nt = 0;
        for (auto& ch : plan.spineChains) {
            tabs.ops[nt] = plan.d_table + ch.first;
            tabs.cum[nt] = cum;
            tabs.start[nt] = ch.second;
            ++nt;
        }
        if (!launch_mfma_serial(*this, tabs, nt)) return fail(BEAGLE_ERROR_GENERAL, "no serial MFMA kernel for this shape");
        pendingLaunches += 1;
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

inline int Instance::accumulate(const int* idx, int n, int cumIdx, int sign, bool fresh)
{
    if (cumIdx < 0 || cumIdx >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "scale factors: cumulative index");
    if (n <= 0) return BEAGLE_SUCCESS;
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "scale factors: index");
    return scales.accumulate(idx, n, cumIdx, sign, fresh);
}

// mayWait (beagleResetScaleFactors on the one engine behind a plain handle): on the level kernels the reset of an allocated buffer
// is not launched but waits for the call that follows -- if that is beagleAccumulateScaleFactors into this buffer, one launch does
// both (accumulateScale); any other entry point runs the reset first (runDeferredReset).  Children reset at once.
inline int Instance::resetScale(int idx, bool mayWait)
{
    if (mayWait && idx >= 0 && idx < nScale && scales.allocated(idx)) {
        deferredReset = idx;
        return BEAGLE_SUCCESS;
    }
    if (idx < 0 || idx >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleResetScaleFactors: index");
    return scales.reset(idx);
}

inline int Instance::copyScale(int dst, int src)
{
    if (dst < 0 || dst >= nScale || src < 0 || src >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCopyScaleFactors: index");
    return scales.copy(dst, src);
}

// beagleAccumulate / RemoveScaleFactors (sign -1).  afterReset (beagleAccumulateScaleFactors only): Reset + Accumulate of one
// cumulative buffer, back to back (rescaling the MrBayes way, reference src/mbbeagle.c:1080-1098) -- the reset was not launched
// (resetScale), this launch stores instead of adding.  Any other waiting reset runs first.
inline int Instance::accumulateScale(const int* idx, int n, int cumIdx, int sign, bool afterReset)
{
    bool fuse = false;
    if (deferredReset >= 0) {
        fuse = afterReset && deferredReset == cumIdx && n > 0;
        for (int i = 0; fuse && i < n; ++i)
            if (idx[i] == cumIdx) fuse = false;     // (the buffer among its own sources: reset-then-add, not a store)
        if (!fuse) {
            int drc = runDeferredReset();
            if (drc != BEAGLE_SUCCESS) return drc;
        }
    }
    // queued 20/61-state lists run first unless the call commutes with them (MrBayes removes the old node factors of
    // eigen-system part j+1 between the lists of parts j and j+1: flushing there would undo the merge of the parts)
    if (hasPending() && !(wg && scaleOpsIndependentOfPending(idx, n, cumIdx))) {
        int frc = flushPending();
        if (frc != BEAGLE_SUCCESS) return frc;
    }
    if (!fuse) return accumulate(idx, n, cumIdx, sign);
    const int arc = accumulate(idx, n, cumIdx, +1, true);
    if (arc == BEAGLE_SUCCESS) { deferredReset = -1; return arc; }
    // the store did not happen (an index out of range, ...): the reset the caller asked for still does, then the error is theirs
    const int drc = runDeferredReset();
    return drc != BEAGLE_SUCCESS ? drc : arc;
}

// The arguments of a log-likelihood call (child == nullptr: at the root), whichever kernel serves it.
inline int Instance::checkIntegrate(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx, int count)
{
    for (int n = 0; n < count; ++n) {
        // (arena layouts: a buffer that holds compact tip states has no partials to integrate over)
        if (parent[n] < 0 || parent[n] >= nBuffers || !valid[parent[n]] || (arena() && tipStates[parent[n]]))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "log-likelihood: parent buffer");
        if (child) {
            const int ci = child[n];
            if (ci < 0 || ci >= nBuffers || prob[n] < 0 || prob[n] >= nMatrices)
                return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge log-likelihood: child buffer / matrix");
            if (!tipStates[ci] && !valid[ci]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge log-likelihood: child buffer was never written");
        }
        if (wIdx[n] < 0 || wIdx[n] >= nEigen || fIdx[n] < 0 || fIdx[n] >= nEigen)
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "log-likelihood: weights / frequencies index");
        if (cumIdx && cumIdx[n] != BEAGLE_OP_NONE && (cumIdx[n] < 0 || cumIdx[n] >= nScale))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "log-likelihood: cumulative scale index");
    }
    return BEAGLE_SUCCESS;
}

inline int Instance::integrate(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                        const int* cumIdx, int count, double* out, bool launchOnly)
{
    if (count < 1 || count > MBAMD_MAX_SUBSETS) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "log-likelihood: subset count");
    int rc = checkIntegrate(parent, child, prob, wIdx, fIdx, cumIdx, count);
    if (rc) {                                    // (a held path is not lost to a bad call: it runs, then the error is the caller's)
        if (heldPath) { int prc = runHeldPath(); if (prc) return prc; }
        return rc;
    }
    lastLnl.remember(parent, child, prob, wIdx, fIdx, cumIdx, count);
    if (nUnstored) {                             // (an edge call over a tip pair, a tree of three tips: made before the launch that reads it)
        std::vector<int> ops(parent, parent + count);
        if (child) ops.insert(ops.end(), child, child + count);
        rc = ensureStored(ops.data(), (int) ops.size());
        if (rc) return rc;
    }
    armSums(launchOnly);
    if (!arena()) {
        rc = integrateLevels(parent, child, prob, wIdx, fIdx, cumIdx, count);
    } else if (heldPath && count == 1 && parent[0] == heldPathDst && !(child && tipStates[child[0]] == nullptr && child[0] == heldPathDst)) {
        rc = integratePath4(child, prob, wIdx, fIdx, cumIdx);                  // the held path and this integration: one launch
    } else {
        if (heldPath) { rc = runHeldPath(); if (rc) return rc; }
        rc = integrate4(parent, child, prob, wIdx, fIdx, cumIdx, count);
    }
    if (rc) return rc;
    rc = spanEnd();
    if (rc) return rc;
    postResultFlag();
    // the matrices of the tip pairs the evaluation left unstored are copied behind the integration: nobody waits for that launch
    if (snapPlan) { rc = flushSnapshot(); if (rc) return rc; }
    haveSite = true;
    derivValid = false;
    pendingResult = true;
    if (deferred || launchOnly) {
        if (out) *out = 0.0;
        return BEAGLE_SUCCESS;
    }
    return fetchResult(out);
}

// the level kernels' integration (arguments checked by integrate)
inline int Instance::integrateLevels(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                              const int* cumIdx, int count)
{
    IntegrateArgs a;
    { int rc = integrateOperands(a, parent, child, prob, wIdx, fIdx, cumIdx, count); if (rc) return rc; }
    double* const siteOut = siteTarget();
    if (S >= 8) MBAMD_LAUNCH_BARRIER(k_integrate_lnl_wide, (unsigned) nblocks, 256, 0, stream, a, S, SP, K, P, Ppad, (const double*) d_pweights, siteOut, h_sums_dev);
    else
        MBAMD_LAUNCH(k_integrate_lnl, (unsigned) nblocks, 64, 0, stream, a, S, SP, K, P, Ppad, (const double*) d_pweights, siteOut, h_sums_dev);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// the held root-ward path (k_path4 plan) and the log-likelihood over its last result as ONE launch (k_path4_lnl, mbamd_walk4.h;
// arguments checked by integrate).  The path stays held until that launch is in the stream: whatever fails before, the path
// still runs on its own and the error is returned.
inline int Instance::integratePath4(const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx)
{
    Plan* plan = heldPath;
    PathLnl4 t;
    std::memset(&t, 0, sizeof t);
    if (child) {
        const Operand c = operand(child[0]);
        t.child = c.ptr; t.child_kind = c.kind;
        t.matrix = matrixPtr(prob[0]);
    }
    t.weights = d_weights + (size_t) wIdx[0] * K;
    t.freqs = d_freqs + (size_t) fIdx[0] * S;
    int rc = BEAGLE_SUCCESS;
    if (cumIdx && cumIdx[0] != BEAGLE_OP_NONE) rc = scales.cumulativeForRead(cumIdx[0], t.cum);
    t.pattern_weights = d_pweights;
    t.site = siteTarget();
    t.wsite = h_sums_dev;
    t.P = P;
    hipEvent_t ev0{}, ev1{};
    if (rc == BEAGLE_SUCCESS) rc = launchesBegin(ev0, ev1);
    if (rc == BEAGLE_SUCCESS) {
        plan->lastLaunch = ++launchClock;
        Walk4ArgsInline ai;
        ai.a = walk4Args();
        ai.a.entries = (int) plan->inlineProg.size();
        ai.a.cum = heldPathCum;
        ai.a.cumFresh = heldPathFresh ? 1 : 0;
        std::memcpy(ai.inl, plan->inlineProg.data(), plan->inlineProg.size() * sizeof(Walk4Entry));
        auto kernel = k_path4_lnl<Walk4ArgsInline>;
        MBAMD_LAUNCH_BARRIER(kernel, 8u * (unsigned) ((Ppad / 64 + 7) / 8), 64 * K, path4_lnl_lds_bytes(ai.a.entries, K), stream, ai, t);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = hip_fail(le, "k_path4_lnl");
    }
    if (rc) {
        (void) runHeldPath();
        return rc;
    }
    heldPath = nullptr;
    fusedPaths++;
    pendingLaunches += 1;
    return launchesEnd(ev0, ev1);
}

// the arena layouts' integration (arguments checked by integrate)
inline int Instance::integrate4(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                         const int* cumIdx, int count)
{
    IntegrateArgs4 a;
    { int rc = integrateOperands(a, parent, child, prob, wIdx, fIdx, cumIdx, count); if (rc) return rc; }
    double* const siteOut = siteTarget();
    if (wg) {
        WgGeom g;
        g.tileFloats = strides().partials; g.tipTileBytes = (unsigned) strides().tips; g.TP = wg_pairs_padded(S);
        MBAMD_LAUNCH_BARRIER(k_integrate_lnl_wg_wide, (unsigned) nblocks, MBAMD_INTEGRATE_WG_THREADS, 0, stream, a, S, SP, K, P, Ppad, g, (const double*) d_pweights, siteOut, h_sums_dev);
    } else {
        MBAMD_LAUNCH(k_integrate_lnl_s4, (unsigned) nblocks, 64, 0, stream, a, K, P, Ppad, geom, (const double*) d_pweights, siteOut, h_sums_dev);
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// the partials / matrix / tip layout of this engine, as the read-out kernels take it (patterns [0, P))
inline DerivArgs Instance::layoutArgs() const
{
    DerivArgs a;
    std::memset(&a, 0, sizeof a);
    a.pstride = strides().partials;
    a.tstride = (unsigned) strides().tips;
    a.S = S; a.SP = SP; a.K = K; a.Ppad = Ppad;
    a.first = 0; a.last = P;
    return a;
}
// ... with the (checked) operands of a log-likelihood call over one subset in device pointers; child < 0: a root call
inline int Instance::lnlOperands(DerivArgs& a, int parent, int child, int prob, int wIdx, int fIdx, int cumIdx)
{
    a = layoutArgs();
    a.parent = partials[parent];
    if (child >= 0) {
        a.child_tip = holdsTip(child) ? 1 : 0;
        a.child = operandPtr(child);
        a.matrix[0] = matrixPtr(prob);
    }
    a.weights = d_weights + (size_t) wIdx * K;
    a.freqs = d_freqs + (size_t) fIdx * S;
    return cumIdx != BEAGLE_OP_NONE ? scales.cumulativeForRead(cumIdx, a.cum) : BEAGLE_SUCCESS;
}

// The pre-order pass, the gradient in all branch lengths and the cross products: the bodies are shared with the double-precision
// engine (mbamd_preorder.h, mbamd_crossproducts.h).
inline int Instance::updatePrePartials(const BeagleOperation* ops, int n, int cumIdx) { return update_pre_partials(*this, ops, n, cumIdx); }
inline int Instance::edgeReadout(const int* post, const int* pre, const int* dmat1, const int* dmat2, const int* wIdx, int count, double* sites1,
                                 double* sites2, size_t siteStride, double* sums1, double* sums2)
{
    return edge_readout(*this, post, pre, dmat1, dmat2, wIdx, count, sites1, sites2, siteStride, sums1, sums2);
}
inline int Instance::crossProducts(const int* post, const int* pre, const int* rateIdx, const int* wIdx, const double* lengths, int count, double* out)
{
    return cross_products(*this, post, pre, rateIdx, wIdx, lengths, count, out);
}
inline int Instance::nodePosteriors(const int* post, const int* pre, const int* wIdx, int count, double* sites, int* bestStates, double* bestValues,
                                    size_t siteStride, double* sums)
{
    return node_posteriors(*this, post, pre, wIdx, count, sites, bestStates, bestValues, siteStride, sums);
}
inline int Instance::categoryPosteriors(int wIdx, double* out, size_t stride) { return category_posteriors(*this, wIdx, out, stride); }
inline int Instance::sampleAncestralStates(const int* parentSlots, const int* post, const int* matrices, int count, int wIdx, unsigned long long seed,
                                           long long patternOffset, int* states, int* categories, double* changes, size_t stride)
{
    return sample_ancestral_states(*this, parentSlots, post, matrices, count, wIdx, seed, patternOffset, states, categories, changes, stride);
}
// what ensure_posteriors asks for: the latest log-likelihood call's operands, checked and in memory, and room for q
inline int Instance::posteriorOperands(DerivArgs& a)
{
    const LnlOperands& l = lastLnl;
    int cum = l.cum;
    int rc = checkIntegrate(&l.parent, l.child >= 0 ? &l.child : nullptr, &l.prob, &l.weights, &l.freqs, &cum, 1);
    if (rc) return rc;
    rc = grow((void**) &d_q, &qCap, (size_t) K * Ppad * sizeof(double));
    if (rc) return rc;
    rc = ensureStored(l.parent, l.child);
    if (rc) return rc;
    return lnlOperands(a, l.parent, l.child, l.prob, l.weights, l.freqs, l.cum);
}

// Branch-length derivatives over one edge: one launch of k_edge_derivatives on this engine's partials layout, then a wait.  Never the
// fused path-and-likelihood launch: a held path runs first, like every queued list and matrix job.
inline int Instance::edgeDerivatives(int parent, int child, int prob, int d1, int d2, int wIdx, int fIdx, int cumIdx, double out3[3])
{
    if (hasWork()) { int frc = flushPending(); if (frc) return frc; }
    int rc = checkIntegrate(&parent, &child, &prob, &wIdx, &fIdx, &cumIdx, 1);
    if (rc) return rc;
    if (d1 < 0 || d1 >= nMatrices || d2 >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge derivatives: derivative matrix index");
    const int nb = Ppad / 64;
    if (!h_deriv) {
        HIP_TRY(hipHostMalloc(&h_deriv, (size_t) 3 * (Ppad + nb) * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipHostGetDevicePointer((void**) &h_deriv_dev, h_deriv, 0));
    }
    lastLnl.remember(&parent, &child, &prob, &wIdx, &fIdx, &cumIdx, 1);
    rc = ensureStored(parent, child);
    if (rc) return rc;
    DerivArgs a;
    rc = lnlOperands(a, parent, child, prob, wIdx, fIdx, cumIdx);
    if (rc) return rc;
    a.matrix[1] = matrixPtr(d1);
    a.matrix[2] = d2 >= 0 ? matrixPtr(d2) : nullptr;
    a.pattern_weights = d_pweights;
    a.site = h_deriv_dev;
    a.sums = h_deriv_dev + (size_t) 3 * Ppad;
    a.first = 0; a.last = P;
    a.sumStride = nb;
    withLayout([&](auto L) {
        auto kernel = k_edge_derivatives<L(), float>;
        MBAMD_LAUNCH(kernel, (unsigned) nb, 64, 0, stream, a);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    syncedClock = launchClock;
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += h_deriv[(size_t) 3 * Ppad + (size_t) q * nb + b];
        out3[q] = s;
    }
    haveSite = true;
    derivValid = true;
    if (!(out3[0] == out3[0]) || out3[0] > 1.79e308 || out3[0] < -1.79e308) return BEAGLE_ERROR_FLOATING_POINT;
    return BEAGLE_SUCCESS;
}

// the stream writes the sequence number of this integration behind its kernel: what fetchResult polls
inline void Instance::postResultFlag()
{
    if (!wait.poll) return;
    flagWritten = !sumsArmed;                    // (a result awaited through its block sums needs no stream operation behind the kernel)
    if (!flagWritten) ++wait.seq;                // (the sequence moves on: nobody will see this number in the flag word, a later one is larger)
    else (void) wait.post(stream);               // (refused: polling is off from now on, fetchResult synchronises)
    flagClock = launchClock;                     // what the stream has finished when the flag shows wait.seq -- and nothing younger
    siteSeq = wait.seq;                          // (the integration in front of this flag wrote the site values)
}

inline int Instance::fetchResult(double* out)
{
    if (!pendingResult) return fail(BEAGLE_ERROR_GENERAL, "no log-likelihood pending");
    {
        StatTimer st_(ST_WAIT);
        bool landed = false, bySums = false;
        const std::chrono::milliseconds limit(1);                     // of spinning; then the runtime's wait
        if (sumsArmed) {
            landed = bySums = CompletionWait::sumsLanded(h_sums, (size_t) nblocks, limit);
            sumsArmed = false;
        }
        // (the block sums were written before the flag: they are read after it)
        if (!landed && wait.poll && flagWritten) landed = wait.flagLanded(limit);
        // the flag covers the launches up to the integration it follows; launches queued behind it in deferred mode (the reduction of
        // mbamdReduceLogLikelihood, further lists) are complete only after a real synchronisation
        if (landed) syncedClock = std::max(syncedClock, flagClock);
        else { HIP_TRY(hipStreamSynchronize(stream)); syncedClock = launchClock; }
        // (seen through the sums: the kernel's other stores -- the site values -- may still be on their way; getSites then synchronises)
        if (!bySums || wait.flagShowsSeq()) seenSeq = wait.seq;
    }
    pendingResult = false;
    double s = 0.0;
    for (int i = 0; i < nblocks; ++i) s += h_sums[i];
    if (out) *out = s;
    if (!(s == s) || s > 1.79e308 || s < -1.79e308) return BEAGLE_ERROR_FLOATING_POINT;
    return BEAGLE_SUCCESS;
}

// mbamdReduceLogLikelihood: the pending result summed on the device into deviceOut; a stream named there waits for the sum
inline int Instance::reduceResult(double* deviceOut, void* waitingStream)
{
    if (!pendingResult) return fail(BEAGLE_ERROR_GENERAL, "no log-likelihood pending");
    if (deviceOut == nullptr) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdReduceLogLikelihood: null output");
    MBAMD_LAUNCH_BARRIER(k_sum_block_sums, 1u, 256, 256 * sizeof(double), stream, (const double*) h_sums_dev, nblocks, deviceOut);
    HIP_TRY(hipGetLastError());
    if (waitingStream != nullptr) {
        if (!reduceEvent) HIP_TRY(hipEventCreateWithFlags(&reduceEvent, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(reduceEvent, stream));
        hipStream_t ws{};
        std::memcpy(&ws, &waitingStream, std::min(sizeof ws, sizeof waitingStream));
        HIP_TRY(hipStreamWaitEvent(ws, reduceEvent, 0));
    }
    return BEAGLE_SUCCESS;
}

// ---- what mbamdGetKernelTiming / StepTiming / ListCounts / WalkTrace and MBAMD_STATS read (the engine's device is current) ----
inline int Instance::kernelTiming(double* ms, long* launches, int reset)
{
    HIP_TRY(hipStreamSynchronize(stream));
    { int frc = eventsFold(); if (frc) return frc; }
    timedLaunches += pendingLaunches;
    pendingLaunches = 0;
    *ms += timedMs;
    *launches += timedLaunches;
    if (reset) { timedMs = 0.0; timedLaunches = 0; }
    return BEAGLE_SUCCESS;
}
inline int Instance::stepTiming(double* ms, long* steps, int reset)
{
    HIP_TRY(hipStreamSynchronize(stream));
    spanFold();
    *ms += spanMs;
    *steps += spanCount;
    if (reset) { spanMs = 0.0; spanCount = 0; }
    return BEAGLE_SUCCESS;
}
inline int Instance::walkTrace(long long* out, int maxSteps, int* outSteps, int* outWaves)
{
    if (!d_trace) return fail(BEAGLE_ERROR_GENERAL, "set MBAMD_WALK_TRACE before creating the instance");
    HIP_TRY(hipStreamSynchronize(stream));
    const int n = std::min(maxSteps, std::min(4096, lastWalkSteps));
    HIP_TRY(hipMemcpy(out, d_trace, (size_t) n * 8 * 3 * sizeof(long long), hipMemcpyDeviceToHost));
    if (outSteps) *outSteps = n;
    if (outWaves) *outWaves = walkWaves + 1;
    return BEAGLE_SUCCESS;
}
inline void Instance::printStats(int id) const
{
    std::fprintf(stderr, "[mbamd] instance %d: plan cache %ld hits / %ld misses; tree-walk schedules re-used %llu / built %llu; root-ward paths held %ld, run with their log-likelihood as one launch %ld\n", id,
                 planHits, planMisses, (unsigned long long) scheduleHits, (unsigned long long) scheduleMisses, heldPaths, fusedPaths);
    if (listsTotal)
        std::fprintf(stderr, "[mbamd] instance %d: %d-state lists %ld: root-ward paths %ld (of them forked %ld), tree walks %ld (%.1f operations each)\n", id,
                     S, listsTotal, listsPath, forkedPaths, listsWalked, listsWalked ? (double) opsWalked / listsWalked : 0.0);
}
inline const char* Instance::implName() const
{
    return s4 ? MBAMD_IMPL_NAME ": 4-state tree-walk kernels"
         : wg ? (wg_bf16(S) ? MBAMD_IMPL_NAME ": general-state tree-walk kernels (fp32 arithmetic as three exact bf16 pieces on v_mfma_f32_32x32x16_bf16)"
                            : MBAMD_IMPL_NAME ": general-state tree-walk kernels (v_mfma_f32_32x32x2_f32)")
         : mfma ? MBAMD_IMPL_NAME ": general-state MFMA (v_mfma_f32_32x32x2_f32) kernels"
                : MBAMD_IMPL_NAME ": general-state vector kernels";
}

// ---------------------------------------------------------------------------------------------
// per-pattern read-outs as Instance methods (a handle of children gathers them)
// ---------------------------------------------------------------------------------------------

inline int Instance::getSites(double* out)
{
    if (!haveSite) return fail(BEAGLE_ERROR_GENERAL, "beagleGetSiteLogLikelihoods: no likelihood computed yet");
    if (derivValid) {                            // (a derivative call is synchronous: its values are in place)
        std::memcpy(out, h_deriv, (size_t) P * sizeof(double));
        return BEAGLE_SUCCESS;
    }
    // (a result that was fetched -- the stream's flag behind the integration kernel was seen, or the stream synchronised -- has its
    //  site values in place: no second wait; a runtime synchronisation of an idle stream still costs ~25 us)
    if (!(siteOnHost && siteSeq != 0 && seenSeq == siteSeq && !pendingResult)) HIP_TRY(hipStreamSynchronize(stream));
    if (siteOnHost) {
        std::memcpy(out, h_site, (size_t) P * sizeof(double));
    } else {
        HIP_TRY(hipMemcpy(out, d_site, (size_t) P * sizeof(double), hipMemcpyDeviceToHost));
        if (!h_site && hipHostMalloc((void**) &h_site, (size_t) Ppad * sizeof(double), hipHostMallocDefault) == hipSuccess) {
            if (hipHostGetDevicePointer((void**) &h_site_dev, h_site, 0) != hipSuccess) h_site_dev = nullptr;
        }
        siteToHost = h_site_dev != nullptr;   // this client reads them: later evaluations write to the host directly
    }
    return BEAGLE_SUCCESS;
}

// the binary exponents behind a scale buffer, out[k * P + c]
inline int Instance::getScaleExponents(int idx, int* out)
{
    if (idx < 0 || idx >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "scale exponents: index");
    HIP_TRY(hipStreamSynchronize(stream));
    return scales.download(idx, P, out, [&](size_t bytes, void** p) { const int rc = grow(&d_tmp, &tmpCap, bytes); *p = d_tmp; return rc; });
}

// ---- reports (csrc/mbamd_reports.h, include/libhmsbeagle/mbamd_reports.h) -------------------------------------------
inline int Instance::finalPass(const MbamdFinalOperation* ops, int count)
{
    if (S > MBAMD_REP_MAXS) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "mbamdUpdateFinalPartials: more than 64 states");
    for (int o = 0; o < count; ++o) {
        const MbamdFinalOperation& b = ops[o];
        if (b.destinationPartials < 0 || b.destinationPartials >= nBuffers || b.downPartials < 0 || b.downPartials >= nBuffers ||
            b.ancestorFinal >= nBuffers || b.rootTip >= nBuffers)
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: partials index");
        if (b.transitionMatrix < 0 || b.transitionMatrix >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: matrix index");
        if (!valid[b.downPartials] || tipStates[b.downPartials]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: down partials were never computed");
        if (b.ancestorFinal >= 0 && (!valid[b.ancestorFinal] || tipStates[b.ancestorFinal]))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: the ancestor's final partials are not there");
        if (tipStates[b.destinationPartials]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: the destination holds compact tip states");
        int rc = ensurePartials(b.destinationPartials);
        if (rc) return rc;
        if (nUnstored) {
            const int reads[3] = {b.downPartials, b.ancestorFinal, b.rootTip};
            rc = ensureStored(reads, 3);
            if (rc) return rc;
            dropRecipe(b.destinationPartials);
        }
        // the exponents of the final pass: written by the top node's launch, inherited by everything below it
        if (finalExpOf.size() != (size_t) nBuffers) finalExpOf.assign((size_t) nBuffers, nullptr);
        if (b.ancestorFinal < 0) {
            int32_t*& own = finalExpOwn[b.destinationPartials];
            if (!own) HIP_TRY(hipMalloc(&own, (size_t) K * Ppad * sizeof(int32_t)));
            // a new pass from this top node rewrites `own` in place: whatever an EARLIER pass left below it would be read with
            // this pass's exponents from now on -- those buffers no longer hold final partials (they are re-made by this pass, or not)
            for (size_t q = 0; q < finalExpOf.size(); ++q)
                if (finalExpOf[q] == own && (int) q != b.destinationPartials) finalExpOf[q] = nullptr;
            finalExpOf[b.destinationPartials] = own;
        } else {
            if (!finalExpOf[b.ancestorFinal]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: the ancestor's buffer does not hold final partials");
            finalExpOf[b.destinationPartials] = finalExpOf[b.ancestorFinal];
        }
        FinalOp f;
        std::memset(&f, 0, sizeof f);
        f.Ppad = Ppad;
        f.fexp = finalExpOf[b.destinationPartials];
        f.dst = partials[b.destinationPartials];
        f.anc = b.ancestorFinal >= 0 ? partials[b.ancestorFinal] : nullptr;
        f.down = partials[b.downPartials];
        f.matrix = matrixPtr(b.transitionMatrix);
        if (b.ancestorFinal < 0 && b.rootTip >= 0) {
            if (!readable(b.rootTip)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdUpdateFinalPartials: the root tip was never set");
            const Operand t = operand(b.rootTip);
            f.tip = t.ptr; f.tipKind = t.kind;
        }
        const dim3 grid((unsigned) ((P + 63) / 64), (unsigned) K);
        withLayout([&](auto tag) { MBAMD_LAUNCH(k_final_pass<decltype(tag)::value>, grid, 64, 0, stream, f, S, SP, K, P, strides().partials, strides().tips); });
        HIP_TRY(hipGetLastError());
        valid[b.destinationPartials] = 1;
        clearPreOrder(b.destinationPartials);
        wgForget(b.destinationPartials);
    }
    return BEAGLE_SUCCESS;
}

inline int Instance::getScaledPartials(int idx, int cumIdx, float* out, float* outLn)
{
    if (idx < 0 || idx >= nBuffers || !valid[idx] || tipStates[idx]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetScaledPartials: buffer");
    if (cumIdx != BEAGLE_OP_NONE && (cumIdx < 0 || cumIdx >= nScale)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "mbamdGetScaledPartials: cumulative scale index");
    const int32_t *wide = nullptr, *narrow = nullptr;              // exponents per (pattern, category) / per pattern
    if (cumIdx != BEAGLE_OP_NONE) {
        const int32_t* exps = nullptr;
        bool perCategory = false;
        { int rc = scales.cumulativeForRead(cumIdx, exps, &perCategory); if (rc) return rc; }
        (perCategory ? wide : narrow) = exps;
    }
    const size_t total = (size_t) K * P * S;
    int rc = grow(&d_tmp, &tmpCap, (total + (size_t) Ppad) * sizeof(float));
    if (rc) return rc;
    rc = ensureStored(idx);
    if (rc) return rc;
    float* d_out = static_cast<float*>(d_tmp);
    float* d_ln = d_out + total;
    const unsigned blocks = (unsigned) ((total + 255) / 256);
    const int32_t* extra = (idx < (int) finalExpOf.size()) ? finalExpOf[idx] : nullptr;      // final partials carry their pass's own exponents
    withLayout([&](auto tag) { MBAMD_LAUNCH(k_export_scaled<decltype(tag)::value>, blocks, 256, 0, stream, (const float*) partials[idx], wide, narrow, extra, S, K, P, Ppad, strides().partials, d_out, d_ln); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    syncedClock = launchClock;
    HIP_TRY(hipMemcpy(out, d_out, total * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(outLn, d_ln, (size_t) P * sizeof(float), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd

#endif  // MBAMD_F32_H_
