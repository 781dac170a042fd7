// mbamd_f32.h -- the single-precision engine of one device: the declaration of `Instance` (arenas, stream, plan cache, schedulers)
// and new_engine(), the only place one is made.  Defined here: create and ~Instance; data in and out (tips, partials, eigen-systems,
// matrices); the plan cache; updatePartials, submit, flushPending, timedRun; the scale calls; integrate, fetchResult, reduceResult;
// the forwards to the bodies shared with the double-precision engine; stats and the reports.  The three back ends define their
// members in headers of their own, included below the declaration: mbamd_f32_walk.h (the program compiler front of both tree walks),
// mbamd_f32_walk4.h (4 states), mbamd_f32_walkg.h (20/61 states), mbamd_f32_levels.h (level / MFMA kernels).  The compiled lists
// are plain data (`Plan`, `PathStep`: mbamd_plan.h); the scale buffers belong to a `ScaleStore` (mbamd_scale_store.h), the unstored
// subtrees of the 4-state walk to a `Walk4Unstored` (mbamd_walk4_unstored.h), launch counts and timing events to a `LaunchTimer`
// (mbamd_launch_timer.h).  Included by mbamd_engine.cpp, whose C ABI reaches an engine through the public part of `Instance` and
// nothing else.
#ifndef MBAMD_F32_H_
#define MBAMD_F32_H_

#include <cmath>
#include <cstdlib>
#include <memory>
#include <unordered_map>

#include "mbamd_host.h"          // the HIP runtime, beagle.h, the switches, <algorithm> ... <vector>; diagnostics and the host runtime the engines share
#include "mbamd_kernels.h"
#include "mbamd_plan.h"          // Plan, Walk4Recipe, PathStep: the compiled operation lists
#include "mbamd_scale_store.h"   // ScaleStore: the scale buffers, whichever form holds them, and the kernels that move them between forms
#include "mbamd_walk4_unstored.h"   // Walk4Unstored: the small subtrees a 4-state launch did not store, their recipes and matrix snapshots
#include "mbamd_launch_timer.h"  // LaunchTimer: launch counts, and the events of kernel and step timing
#include "mbamd_reports.h"
#include "libhmsbeagle/mbamd_reports.h"
#include "mbamd_walk4_host.h"
#include "mbamd_kernels_mfma.h"
#include "mbamd_derivatives.h"   // k_edge_derivatives: lnL, d lnL / dt and d2 lnL / dt2 over one branch
#include "mbamd_preorder.h"      // k_pre_partials, k_edge_readout: the pre-order pass and the gradient in all branch lengths
#include "mbamd_crossproducts.h" // k_cross_products, k_cross_products_mfma: the cross-product matrix of the gradient in the rate matrix
#include "mbamd_posteriors.h"    // k_node_posteriors: node-state and category posteriors from the pre-order buffers
#include "mbamd_insertions.h"    // k_insertion_readout: the log-likelihood with a subtree attached at every listed point
#include "mbamd_ancestral_sampling.h"   // k_sample_top, k_sample_edges: a draw of all ancestral states from their joint posterior
#include "mbamd_site_model.h"    // k_edge_category_readout, k_root_frequency_readout: the gradient in category rates, weights and root frequencies
#include "mbamd_autocorrelated.h"  // k_hmm_products, k_hmm_vectors, k_hmm_posteriors: the site-order HMM over the rate categories
#include "mbamd_matrix_products.h" // k_matrix_products_*, k_matrix_transpose: matrices made out of matrices; MatrixLayoutF32
#include "mbamd_rate_exponential.h" // k_rate_exp_*: exp(Q t) of any rate matrix, no eigen-system

namespace mbamd {

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
    // insertionLogLikelihoods (mbamdCalculateInsertionLogLikelihoods on this engine's patterns; mbamd_insertions.h): synchronous;
    // sums[i] (or null), per-pattern log ratios (or null) at [i * siteStride + c]
    int insertionLogLikelihoods(const int* pre, const int* post, const int* postM, const int* sub, const int* subM, const int* subScale,
                                const int* wIdx, int count, double* sites, size_t siteStride, double* sums);
    void insertionLaunchCounts(long out2[2]) const { out2[0] += insertionLaunches[0]; out2[1] += insertionLaunches[1]; }   // its launches: plain / matrix-core form
    // siteModelDerivatives (mbamdCalculateSiteModelDerivatives on this engine's patterns; mbamd_site_model.h): synchronous; edgeCat
    // [count][K], counts [K], rootFreq [S], each or null
    int siteModelDerivatives(const int* post, const int* pre, const int* dmat, const int* wIdx, int count, double* edgeCat, double* counts,
                             double* rootFreq);
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
    void setTiming(bool on) { timer.enable(on); }
    int kernelTiming(double* ms, long* launches, int reset) { return timer.kernelTiming(ms, launches, reset); }
    int stepTiming(double* ms, long* steps, int reset) { return timer.stepTiming(ms, steps, reset); }
    void listCounts(long out6[6]) const { const long c[6] = {listsTotal, listsPath, forkedPaths, fusedPaths, listsWalked, opsWalked}; std::copy(c, c + 6, out6); }
    void rangeSafeCounts(long out2[2]) const { out2[0] = wgFlushesRangeSafe; out2[1] = wgFlushesPlain; }
    void walkCounts(long out2[2]) const { out2[0] = walksPlain; out2[1] = walksGeneric; }   // launches of the plain instantiations of k_walk4_t (one wave or several) / of the generic ones
    void plainWaveCounts(long out[MBAMD_W4_MAXW]) const { for (int w = 0; w < MBAMD_W4_MAXW; ++w) out[w] += walksPlainByW[w]; }   // ... of the plain ones by waves per workgroup (out[W - 1]; added: the sums over engines)
    int walkTrace(long long* out, int maxSteps, int* outSteps, int* outWaves);
    // tip-pair buffers launches left unstored / buffers materialised since / launches that materialised them (mbamdGetRecomputeCounts);
    // the same for the subtrees of three and four tips (mbamdGetSubtreeRecomputeCounts)
    void recomputeCounts(long out3[3]) const { unstored4.pairCounts(out3); }
    void subtreeRecomputeCounts(long out3[3]) const { unstored4.subtreeCounts(out3); }

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
    // ---- the program compiler front of both tree walks (mbamd_f32_walk.h; scheduler: mbamd_walk4_host.h) -------------
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
    std::vector<int> w4subTips, w4subOps, w4entryOf;                // buildWalk scratch: per operation of the segment, its subtree
    std::vector<PathStep> pathSteps;             // recognisePath's result (scratch of buildPath4 / buildPathG)
    bool recognisePath(const BeagleOperation* ops, int n, int L, bool& forked);
    Walk4Entry pathEntry(const PathStep& p, uint32_t pbuf, uint32_t tipb, uint32_t mbuf, int scratchRow) const;
    void pathPlan(Plan& plan, int entries, bool forked);
    int buildWalk(Plan& plan, const BeagleOperation* ops, int n, const int* listOf = nullptr, bool perList = false);
    // ---- the 4-state tree walk (mbamd_f32_walk4.h; kernels: mbamd_walk4.h) --------------------------------------------
    bool walkCumFresh = false;       // the cumulative buffer of the list being submitted holds nothing yet (store, do not add)
    // the small subtrees a whole-tree launch did not store (MBAMD_W4_NOSTORE, mbamd_walk4.h): such a buffer stays `valid` and holds a recipe
    // (mbamd_walk4_unstored.h).  Every reader of partials calls ensureStored first; a matrix changes only behind snapshotNow
    Walk4Unstored unstored4;
    int ensureStored(const int* bufs, int n) { return unstored4.any() ? unstored4.ensureStored(bufs, n, walk4Args(), (int) scales.count()) : BEAGLE_SUCCESS; }
    int ensureStored(int a, int b = -1) { const int v[2] = {a, b}; return ensureStored(v, 2); }
    int snapshotNow() { return unstored4.snapshotWaiting() ? unstored4.flushSnapshot(walk4Args()) : BEAGLE_SUCCESS; }
    // ---- 4-state path: a root-ward path (k_path4 plan) is HELD until the next call: if that call is the log-likelihood over the
    // path's last result, both run as one launch (k_path4_lnl); anything else runs the path first, as before
    Plan* heldPath = nullptr;
    int32_t* heldPathCum = nullptr;
    bool heldPathFresh = false;
    int heldPathDst = -1;                        // the partials buffer the path's last operation writes
    int runHeldPath();
    int integratePath4(const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx);
    int configureWalk();
    int updatePartials4(const BeagleOperation* ops, int n, int cumIdx);
    void listLaunched(const BeagleOperation* ops, int n, bool path, bool forked);
    bool buildPath4(Plan& plan, const BeagleOperation* ops, int n);
    Walk4Args walk4Args() const;
    int runWalk(const Plan& plan, int32_t* cum);
    // ---- the 20/61-state tree walk (mbamd_f32_walkg.h; kernels: mbamd_walkg.h): lists are deferred and merged (MrBayes submits one
    // list per eigen-system part of a codon model, reference src/mbbeagle.c:1095-1104; together they are ONE forest for the program compiler)
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
    void wgGeometry(int lists, int& W, int& slots) const;
    int updatePartialsG(const BeagleOperation* ops, int n, int cumIdx);
    int flushWalkG();
    int runWalkG(const Plan& plan);
    bool scaleOpsIndependentOfPending(const int* idx, int n, int cumIdx) const;
    bool buildPathG(Plan& plan, const BeagleOperation* ops, int n, const std::vector<int>& starts, int nl);
    template <int SC_, int WMAX_, int CH_, int DEPTH_>
    static void launch_walkg_t(Instance& in, const WalkGArgs& a, int W, int nslots, const std::vector<Walk4Entry>* inlineProg);
    template <int SC_> static void launch_pathg_t(Instance& in, const WalkGArgs& a, const std::vector<Walk4Entry>& prog, bool forked);
    WalkGArgs walkGArgs() const;
public:
    // deferred lists (`path`: a held 4-state path counts) / anything at all that flushPending would launch
    bool hasPending(bool path = true) const { return !pending.empty() || !wgListCum.empty() || (path && heldPath != nullptr); }
    bool hasWork(bool path = true) const { return hasPending(path) || !pendingJobs.empty(); }
private:
    // ---- the level / MFMA kernels (mbamd_f32_levels.h; kernels: mbamd_kernels.h, mbamd_kernels_mfma.h) and their deferral queue ----
    int walkWaves = 1, lastWalkSteps = 0;   // (kernel trace bookkeeping of the serial MFMA kernels, tools/trace_*.py)
    long long* d_trace = nullptr;    // MBAMD_WALK_TRACE: per-step clock stamps of workgroup 0 (timing experiments)
    int NT = 0, T = 0;               // MFMA packing: i-tiles of 32 rows, j-pairs
    std::vector<std::pair<Plan*, int>> pending;   // deferred general-path lists (plan, cumulative scale index or -1)
    int serialRatio = 4;             // lists with <= ratio * levels operations run as ONE serial launch (0 = never; MBAMD_MFMA_SERIAL)
    bool independentOfPending(const Plan& plan, int cumIdx);
    int32_t* cumulativeOf(int idx) { int32_t* p = nullptr; bool fresh; if (idx >= 0) (void) scales.cumulativeForAdd(idx, p, fresh); return p; }   // of a queued list (it exists since the list was submitted)
    int flushMerged(std::vector<std::pair<Plan*, int>>& work);
    int buildGeneric(Plan& plan, std::vector<PartialsOp>& dev, const std::vector<int>& dstIdx, const std::vector<int>& c1Idx,
                     const std::vector<int>& c2Idx);
    int runGeneric(const Plan& plan, int32_t* cum);
    int integrateLevels(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                        const int* cumIdx, int count);
    void ensureTrace();
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
    // ---- what every back end shares -----------------------------------------------------------------------------------------
    int checkOperation(const BeagleOperation& b, const std::vector<char>& written, const char*& what) const;
    void postResultFlag();
    uint64_t launchClock = 0, syncedClock = 0;   // launches issued / launches known complete (last stream synchronisation)
    uint64_t flagClock = 0;                      // launchClock when the polled result flag was queued (postResultFlag)
    uint32_t siteSeq = 0, seenSeq = 0;           // flag value behind the integration that wrote the latest site values / latest flag value fetched
    HostMirror h_freqs, h_weights;               // host mirrors of d_freqs / d_weights (setFreqs / setWeights)

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
    template <class E> friend int insertion_log_likelihoods(E&, const int*, const int*, const int*, const int*, const int*, const int*, const int*, int, double*, size_t, double*);
    template <class E> friend int site_model_derivatives(E&, const int*, const int*, const int*, const int*, int, double*, double*, double*);
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
    int beforeMatrixWrite() { return snapshotNow(); }
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
        if (!unstored4.any()) return BEAGLE_SUCCESS;
        std::vector<int> reads((size_t) n);
        for (int i = 0; i < n; ++i) reads[(size_t) i] = buf(i);
        return ensureStored(reads.data(), n);
    }
    // a destination holds no recipe any more and has memory (buffers of the level kernels are allocated on first use) ...
    int beforeWrite(int d) { unstored4.forget(d); return ensurePartials(d); }
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
    void countLaunches(int n) { timer.count(n); }
    // ... and, while timing is on, an event pair around the launches of a call (no span: such a call is no evaluation)
    int timedBegin(hipEvent_t& ev0, hipEvent_t& ev1) { return timer.timedBegin(ev0, ev1); }
    int timedEnd(hipEvent_t ev0, hipEvent_t ev1) { return timer.launchesEnd(ev0, ev1); }
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
    long insertionLaunches[2] = {0, 0};   // launches of insertion_log_likelihoods: plain / matrix-core form
    // the cumulative exponents of a scale buffer as a kernel reads them ([K][Ppad] on the arena layouts, [Ppad] otherwise; null: all zero)
    int cumulativeExponents(int idx, const int32_t*& out) { return scales.cumulativeForRead(idx, out); }
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

    // launches counted for mbamdGetKernelTiming and, while timing is on, the event pairs around the partials launches of a list and
    // the spans of whole evaluations (mbamd_launch_timer.h)
    LaunchTimer timer;

    bool deferred = false, pendingResult = false;
    hipEvent_t reduceEvent{};        // mbamdReduceLogLikelihood: orders a client's stream behind the device-side sum
    // final pass (mbamd_reports.h): per partials buffer, the exponents [K][Ppad] its final partials carry (nullptr: not final
    // partials); owned by the top node's destination buffers
    std::vector<int32_t*> finalExpOf;
    std::unordered_map<int, int32_t*> finalExpOwn;

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

    int setTipMasks(int tip, const std::vector<uint8_t>& masks);
    std::vector<int> eigenWarm;      // per eigen buffer: -1 = no orthonormal basis stored (host-set), else warm starts since the last cold one
    std::vector<char> eigenShield;   // per eigen buffer: the next beagleSetEigenDecomposition is ignored (mbamdSetRateMatricesFrom, mode bit 1)
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
    int accumulate(const int* idx, int n, int cumIdx, int sign, bool fresh = false);   // fresh: cumIdx was reset just before -- store, do not add
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

}  // namespace mbamd

// the members the back ends define (each header says which)
#include "mbamd_f32_walk.h"
#include "mbamd_f32_walk4.h"
#include "mbamd_f32_walkg.h"
#include "mbamd_f32_levels.h"

namespace mbamd {

// ---------------------------------------------------------------------------------------------
inline int Instance::create(const Dims& dim, int patternCount, int dev, const Switches& switches)
{
    sw = switches;
    device = dev;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    timer.create(stream);
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
    if (!mfma_shape_compiled(NT, K)) serialRatio = 0;
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
        unstored4.create(stream, nBuffers, K, Ppad, &launchClock, [this](void* dst, const void* src, size_t bytes) { return upload(dst, src, bytes); }, sw.unstoredTips);
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

// synchronise, free the device memory, destroy the stream (the scale store, the unstored subtrees and the timer free their own behind it)
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
                    d_ev, d_tmp, d_trace, d_q, d_preTable};
    for (void* b : bufs) if (b) (void) hipFree(b);
    if (h_sums) (void) hipHostFree(h_sums);
    wait.destroy();
    if (h_site) (void) hipHostFree(h_site);
    if (h_deriv) (void) hipHostFree(h_deriv);
    stage.destroy();
    if (reduceEvent) (void) hipEventDestroy(reduceEvent);
    for (auto& kv : finalExpOwn) if (kv.second) (void) hipFree(kv.second);
    (void) hipStreamDestroy(stream);
}

// 4-state path: one tip's state masks (bit i = state i compatible) -> four 64-bit bitplanes per pattern block
inline int Instance::setTipMasks(int tip, const std::vector<uint8_t>& h)
{
    const size_t nb = (size_t) Ppad / 64;
    std::vector<uint64_t> planes(nb * 4, 0);
    for (int c = 0; c < Ppad; ++c)
        for (int i = 0; i < 4; ++i)
            if (h[c] >> i & 1u) planes[(size_t) (c >> 6) * 4 + i] |= (uint64_t) 1 << (c & 63);
    if (unstored4.any()) {                       // recipes that read this tip are made first; whatever the buffer held is gone
        const int src = unstored4.tipChanging(tip, walk4Args(), (int) scales.count());
        if (src) return src;
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
    if (unstored4.any()) {                       // (a tip that switches to partials form: its recipes are made first)
        rc = unstored4.tipChanging(idx, walk4Args(), (int) scales.count());
        if (rc) return rc;
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
    { int src = snapshotNow(); if (src) return src; }                     // (the matrices a recipe needs are copied before any is overwritten)
    { int src = timer.spanBegin(); if (src) return src; }
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
    { int src = snapshotNow(); if (src) return src; }
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
    // merged launches need a per-factor-tile kernel for this shape (launch_mfma_split); other shapes -- e.g. three rate
    // categories -- run their lists one after the other, in submission order
    const bool mergeable = mfma_shape_compiled(NT, K);
    if (work.size() == 1 || !mergeable) {
        for (auto& w : work) {
            const int rc = timedRun(*w.first, cumulativeOf(w.second));
            if (rc) return rc;
        }
        return BEAGLE_SUCCESS;
    }
    return flushMerged(work);
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
    { int brc = timer.launchesBegin(ev0, ev1); if (brc) return brc; }
    const int rc = s4 ? runWalk(plan, cum) : (wg ? runWalkG(plan) : runGeneric(plan, cum));
    { int erc = timer.launchesEnd(ev0, ev1); if (erc) return erc; }
    { int frc = timer.foldIfMany(); if (frc) return frc; }
    return rc;
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
    if (unstored4.any()) {                       // (an edge call over a tip pair, a tree of three tips: made before the launch that reads it)
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
    rc = timer.spanEnd();
    if (rc) return rc;
    postResultFlag();
    // the matrices of the tip pairs the evaluation left unstored are copied behind the integration: nobody waits for that launch
    rc = snapshotNow();
    if (rc) return rc;
    haveSite = true;
    derivValid = false;
    pendingResult = true;
    if (deferred || launchOnly) {
        if (out) *out = 0.0;
        return BEAGLE_SUCCESS;
    }
    return fetchResult(out);
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
inline int Instance::insertionLogLikelihoods(const int* pre, const int* post, const int* postM, const int* sub, const int* subM, const int* subScale,
                                             const int* wIdx, int count, double* sites, size_t siteStride, double* sums)
{
    return insertion_log_likelihoods(*this, pre, post, postM, sub, subM, subScale, wIdx, count, sites, siteStride, sums);
}
inline int Instance::siteModelDerivatives(const int* post, const int* pre, const int* dmat, const int* wIdx, int count, double* edgeCat,
                                          double* counts, double* rootFreq)
{
    return site_model_derivatives(*this, post, pre, dmat, wIdx, count, edgeCat, counts, rootFreq);
}
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

// ---- what mbamdWalkTrace and MBAMD_STATS read (the engine's device is current; the timings: mbamd_launch_timer.h) ----
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
        if (unstored4.any()) {
            const int reads[3] = {b.downPartials, b.ancestorFinal, b.rootTip};
            rc = ensureStored(reads, 3);
            if (rc) return rc;
            unstored4.forget(b.destinationPartials);
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
