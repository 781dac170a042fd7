// mbamd_f64.h -- the double-precision engine behind BEAGLE_FLAG_PRECISION_DOUBLE (`set beagleprecision=double`, reference
// src/command.c:6760-6766; the build it corresponds to is the reference with CLFlt = double, src/bayes.h:110-112).
// Included by mbamd_engine.cpp, whose C ABI reaches the engine through the public part of `Engine64` and nothing else.  Any state
// count <= 64: conditional likelihoods, transition matrices, sums and logarithms all in fp64; rescaling by exact powers of two with
// integer exponents, like the fp32 engine.  What runs an operation list:
//   four states        the tree walk k64_walk4 -- one launch per list, a wave owns its patterns with all their categories (tryWalk4);
//                      lists it does not take, and mid-sized full evaluations, go by dependency level on k64_partials_fused / k64_partials
//   16 to 64 states    one launch per dependency level on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): k64_partials_mfma, or with
//                      the matrices parked in LDS k64_partials_mfma_lds (four or eight waves per workgroup), the rescale fused while all
//                      categories' tiles fit into registers; operations on two compact tips on the gather kernels k64_partials_tips[_lds];
//                      a list that is nothing but chains (the root-ward path of a move) as ONE launch of k64_partials_chain
//   other state counts one launch per level of k64_partials on the vector ALU, then k64_rescale
// Operation lists and matrix updates are queued and run together when anything else is asked of the engine (flushQueue, flushMatrices);
// small host -> device transfers go through a pinned ring.  MBAMD_F64_* switches select the plain paths (mbamd_switches.h).
//
// HBM layout: partials double [buffer][K][S][P_pad] (a thread owns one pattern; every access is coalesced across
// patterns), compact tips uint8 [P_pad], matrices double [buffer][K][S][S] (row = from-state, for the edge integration)
// followed by the transposed copy [K][S][SPAD] with zero-padded rows (the operand of the partials kernel: wave-uniform,
// read through the scalar cache), scale buffers int32 [P_pad] (binary exponents; cumulative buffers are their sums).
#ifndef MBAMD_F64_H_
#define MBAMD_F64_H_

#include <memory>
#include <unordered_map>
#include <utility>

#include "mbamd_host.h"          // fail / HIP_TRY, StatTimer, Switches, Dims; PinnedRing, HostMirror, grow_*, RateSets
#include "mbamd_f64_kernels.h"   // Op64, Walk64Entry / Walk64Args, MatrixJob64, IntegrateArgs64 and the k64_* kernels
#include "mbamd_walk4_host.h"    // Walk4Builder: the program compiler of the four-state walk
#include "mbamd_derivatives.h"   // k_edge_derivatives<DERIV_F64, double>: branch-length derivatives over one edge
#include "mbamd_preorder.h"      // k_pre_partials, k_edge_readout <DERIV_F64, double, 1 and 2>: the pre-order pass and the gradient in all branch lengths
#include "mbamd_crossproducts.h" // k_cross_products <DERIV_F64, double>: the cross-product matrix of the gradient in the rate matrix
#include "mbamd_posteriors.h"    // k_node_posteriors <DERIV_F64, double>: node-state and category posteriors from the pre-order buffers
#include "mbamd_insertions.h"    // k_insertion_readout <DERIV_F64, double, 0>: the log-likelihood with a subtree attached at every listed point
#include "mbamd_ancestral_sampling.h"   // k_sample_top, k_sample_edges <DERIV_F64, double>: a draw of all ancestral states from their joint posterior
#include "mbamd_site_model.h"    // k_edge_category_readout, k_root_frequency_readout <DERIV_F64, double>: the gradient in category rates, weights and root frequencies
#include "mbamd_autocorrelated.h"  // k_hmm_products, k_hmm_vectors, k_hmm_posteriors: the site-order HMM over the rate categories
#include "mbamd_matrix_products.h" // k_matrix_products_*, k_matrix_transpose: matrices made out of matrices; MatrixLayoutF64
#include "mbamd_rate_exponential.h" // k_rate_exp_*: exp(Q t) of any rate matrix, no eigen-system

namespace mbamd {

// ------------------------------------------------------------------------------------------------------------------
// The double-precision engine of one device.  What the C ABI (mbamd_engine.cpp) calls is public; everything below `private:` is the
// engine's own.  Operation lists and matrix updates are QUEUED (updatePartialsEx, updateMatrices): every other entry point runs
// the queues first.
class Engine64 {
public:
    ~Engine64() { destroy(); }
    int create(const Dims& dim, int patterns, int dev, const Switches& switches);
    const char* implName() const;
    int setPartitions(int count, const int* ids);
    int childCount() const { return std::max<int>(1, (int) parts.size()); }
    int setTipStates(int tip, const int* states);
    // in: [K][P][S] (withCategories) or [P][S] replicated over the categories
    int setPartials(int idx, const double* in, bool withCategories);
    int getPartials(int idx, double* out);
    int setEigen(int idx, const double* U, const double* Ui, const double* lam);
    int setFreqs(int idx, const double* f);
    int setWeights(int idx, const double* w);
    int setRates(int index, const double* r);
    int setPatternWeights(const double* w);
    // d1 / d2: the matrix buffers that take the first / second derivative of the same branches (either may be null)
    int updateMatrices(int eigenIdx, int rateIdx, const int* prob, const double* lengths, int count, const int* d1 = nullptr, const int* d2 = nullptr);
    // v3: an eigen-system and a category-rate vector per matrix; one launch per run of equal rate vectors
    int updateMatricesMulti(const int* eigenIdx, const int* rateIdx, const int* prob, const double* lengths, int count,
                            const int* d1 = nullptr, const int* d2 = nullptr);
    // in: [K][S][S] row = from-state (BEAGLE's order)
    int setMatrix(int idx, const double* m);
    int getMatrix(int idx, double* out);
    // matrices made out of matrices (mbamd_matrix_products.h; semantics: beagle.h): asynchronous, both stored copies of a result written
    int convolveMatrices(const int* first, const int* second, const int* result, int count);
    int transposeMatrices(const int* input, const int* result, int count);
    int setMatrices(const int* idx, const double* in, int count);
    int updateMatricesFromRateMatrix(const double* q, const int* prob, const int* d1, const int* d2, const double* lengths, int count);
    int updatePartials(const BeagleOperation* ops, int n, int cumIdx);
    // (operations `stride` bytes apart, queued: see the definition)
    int updatePartialsEx(const void* opsRaw, size_t stride, int n, const int* partition, const int* cumOf);
    int synchronize();
    int accumulateScale(const int* idx, int count, int cumIdx, int sign, int partition = -1);
    int resetScale(int idx, int partition = -1);
    int copyScale(int dst, int src);
    int getScaleExponents(int idx, int* out);           // [K][P]: every category row the same
    int getScaleFactors(int idx, double* out);
    // index arrays are [count][partitionCount] when `partitions` is given (reference src/mbbeagle.c:2781-2800), else [count]
    int logLikelihoods(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx, int count,
                       double* out, const int* partitions = nullptr, int partitionCount = 1, double* outByPartition = nullptr);
    // Branch-length derivatives over one edge (mbamd_derivatives.h), per named partition: index arrays are [partitionCount]
    // (`partitions` null: one entry, all patterns); d2 null: first derivative only.  sums: [partitionCount][3] weighted sums of
    // lnL, d1, d2.  Synchronous; the per-pattern values are kept for getSites / siteDerivatives.
    int edgeDerivatives(const int* parent, const int* child, const int* prob, const int* d1, const int* d2, const int* wIdx, const int* fIdx,
                        const int* cumIdx, const int* partitions, int partitionCount, double* sums);
    bool hasDerivatives() const { return derivValid; }
    const double* siteDerivatives(int order) const { return derivSite.data() + (size_t) order * Ppad; }
    // The pre-order pass and the gradient in all branch lengths (mbamd_preorder.h; semantics: beagle.h), as on the single-precision
    // engine: one launch per group of independent operations; the gradient and second-derivative call (edgeReadout) is synchronous.
    int updatePrePartials(const BeagleOperation* ops, int n, int cumIdx);
    int edgeReadout(const int* post, const int* pre, const int* dmat1, const int* dmat2, const int* wIdx, int count, double* sites1, double* sites2,
                    double* sums1, double* sums2);
    int crossProducts(const int* post, const int* pre, const int* rateIdx, const int* wIdx, const double* lengths, int count, double* out);
    void secondLaunchCounts(long out2[2]) const { out2[0] += secondLaunches[0]; out2[1] += secondLaunches[1]; }   // its read-out launches: plain / matrix-core kernel (none here)
    // node-state and category posteriors (mbamd_posteriors.h), as on the single-precision engine: synchronous
    int nodePosteriors(const int* post, const int* pre, const int* wIdx, int count, double* sites, int* bestStates, double* bestValues, double* sums);
    int categoryPosteriors(int wIdx, double* out);
    // insertion log-likelihoods (mbamd_insertions.h), as on the single-precision engine: synchronous
    int insertionLogLikelihoods(const int* pre, const int* post, const int* postM, const int* sub, const int* subM, const int* subScale,
                                const int* wIdx, int count, double* sites, double* sums);
    void insertionLaunchCounts(long out2[2]) const { out2[0] += insertionLaunches[0]; out2[1] += insertionLaunches[1]; }   // its launches: plain / matrix-core form (none here)
    // the gradient in the site model (mbamd_site_model.h), as on the single-precision engine: synchronous
    int siteModelDerivatives(const int* post, const int* pre, const int* dmat, const int* wIdx, int count, double* edgeCat, double* counts,
                             double* rootFreq);
    // a draw of all ancestral states from their joint posterior (mbamd_ancestral_sampling.h), as on the single-precision engine: synchronous
    int sampleAncestralStates(const int* parentSlots, const int* post, const int* matrices, int count, int wIdx, unsigned long long seed,
                              long long patternOffset, int* states, int* categories, double* changes, size_t stride);
    // mbamdCalculateAutocorrelatedLogLikelihood (mbamd_autocorrelated.h), as on the single-precision engine: synchronous
    int autocorrelatedPrepare(int wIdx, HmmSource& src) { return autocorrelated_prepare(*this, wIdx, src); }
    int autocorrelatedRun(const HmmSource* sources, int sourceCount, int wIdx, const int* sitePatterns, const int* siteJumps, int n, const double* T,
                          double* outLnl, double* outPost)
    {
        return autocorrelated_run(*this, sources, sourceCount, wIdx, sitePatterns, siteJumps, n, T, outLnl, outPost);
    }
    int getSites(double* out);
    // as Instance::kernelTiming: no device timing on this engine, the partials launches (walks and levels) are counted
    int kernelTiming(double* ms, long* launches, int reset);

private:
    int device = 0, tipCount = 0, nBuffers = 0, S = 0, SPAD = 0, IB = 4, P = 0, Ppad = 0, K = 1, nEigen = 0, nMatrices = 0, nScale = 0;
    size_t bufDoubles = 0, matDoubles = 0, eigDoubles = 0;
    bool complexEigen = false;             // BEAGLE_FLAG_EIGEN_COMPLEX: runMatrices takes the CX form of the matrix kernels
    hipStream_t stream{};
    bool live = false;
    Switches sw;                           // the environment switches, read when the instance was created (mbamd_switches.h)
    // ---- device memory ----
    double* d_partials = nullptr;          // [nBuffers][K*S*Ppad]
    uint8_t* d_states = nullptr;           // [tipCount][Ppad]
    std::vector<char> isTip, valid;
    std::vector<int> stateSlot;            // buffer -> row of d_states (MrBayes numbers its tips i * nCijkParts, reference src/mbbeagle.c:148)
    int slotsUsed = 0;
    double* d_matrices = nullptr;          // [nMatrices][K*S*S + K*S*SPAD]
    double* d_eigen = nullptr;             // [nEigen][2*S*S + S]
    double* d_freqs = nullptr;             // [nEigen][S]
    double* d_weights = nullptr;           // [nEigen][K]
    double* d_pweights = nullptr;          // [Ppad]
    int32_t* d_scale = nullptr;            // [nScale][Ppad]
    double* d_site = nullptr;              // [Ppad]
    double* d_sums = nullptr;              // [partitions of a call][Ppad/64]
    double* d_ev = nullptr;
    void* d_stage = nullptr;
    size_t sumsCap = 0, evCap = 0, stageCap = 0, hSumsCap = 0;      // bytes behind d_sums, d_ev, d_stage, h_sums
    double* d_deriv = nullptr;             // [3][Ppad] per-pattern values, then [partitions of a call][3][Ppad / 64] block sums
    size_t derivCap = 0;
    // ---- host side of the transfers ----
    // small host -> device transfers (operation lists, matrix jobs, weights, frequencies) go through a ring: the bytes are copied into
    // pinned host memory, from there asynchronously into the device ring's slot of the same offset, and a slot is written again only
    // after the ring wrapped -- one stream synchronisation per RING_BYTES instead of one per call (a codon M3 evaluation made ten).
    static constexpr size_t RING_BYTES = 4u << 20, RING_MAX_ITEM = 256u << 10;
    PinnedRing ring;                       // 256-byte slots, allocated on first use ...
    uint8_t* d_ring = nullptr;             // ... with its device-side twin
    double* h_sums = nullptr;              // pinned: the block sums of a log-likelihood call
    HostMirror hostFreqs, hostWeights;     // of d_freqs / d_weights
    RateSets rateSets;
    bool haveSite = false;
    std::vector<double> derivSite;         // host copy of the per-pattern values of the last derivative call
    bool derivValid = false;
    std::vector<std::pair<int, int>> parts;       // v3: [first, last) of every pattern partition (empty: none were set)
    // ---- four-state tree walk (k64_walk4): the program compiler, its latest program (re-used when the same list comes again) ----
    Walk4Builder walkBuilder;
    Walk4Template walkTemplate;
    std::vector<int> walkKey;
    std::vector<Walk4Op> walkOps;
    std::vector<Walk64Entry> walkProg;
    // ---- operation lists waiting to run (see updatePartialsEx) ----
    struct QueuedOp { BeagleOperation op; int partition, cum; char tip1, tip2; };
    std::vector<QueuedOp> queue;
    std::vector<char> queuedScale;          // [nScale]: an exponent buffer some queued operation reads, writes or accumulates into
    uint64_t walkLaunches = 0, levelLaunches = 0, preLaunches = 0;
    // ---- pre-order pass (mbamd_preorder.h) ----
    std::vector<char> preOrder;            // per partials buffer: a pre-order operation wrote it and nothing else has since
    LnlOperands lastLnl;                   // the operands of the latest log-likelihood call: what q is made of
    uint64_t qStamp = 0;                   // lastLnl.stamp when d_q was computed
    double* d_q = nullptr;                 // [K][Ppad] posterior category probabilities
    double* d_grad = nullptr;              // a gradient chunk's per-site values, block sums and sums
    size_t qCap = 0, gradCap = 0;
    DerivArgs layoutArgs() const;
    // ---- what the shared bodies of the pre-order, gradient and cross-product calls ask of this engine (mbamd_preorder.h); they also
    // use partialsPtr() and matrixPtr() below ----
    template <class E> friend int update_pre_partials(E&, const BeagleOperation*, int, int);
    template <class E> friend int ensure_posteriors(E&);
    template <class E> friend int edge_list_begin(E&, const char*);
    template <class E> friend int edge_check(const E&, const char*, int, int, int);
    template <class E> friend int edge_list_fill(E&, const int*, const int*, int, GradEdge*);
    template <class E> friend int cross_products(E&, const int*, const int*, const int*, const int*, const double*, int, double*);
    template <class E> friend int edge_readout(E&, const int*, const int*, const int*, const int*, const int*, int, double*, double*, size_t, double*, double*);
    template <class E, class L, class S> friend int chunked_readout(E&, int, const ReadoutShape&, L&&, S&&);
    template <class E> friend int node_posteriors(E&, const int*, const int*, const int*, int, double*, int*, double*, size_t, double*);
    template <class E> friend int insertion_log_likelihoods(E&, const int*, const int*, const int*, const int*, const int*, const int*, const int*, int, double*, size_t, double*);
    template <class E> friend int category_posteriors(E&, int, double*, size_t);
    template <class E> friend int site_model_derivatives(E&, const int*, const int*, const int*, const int*, int, double*, double*, double*);
    template <class E> friend int sample_ancestral_states(E&, const int*, const int*, const int*, int, int, unsigned long long, long long, int*, int*, double*, size_t);
    template <class E> friend int autocorrelated_prepare(E&, int, HmmSource&);
    template <class E> friend int autocorrelated_weights(E&, int, double*);
    template <class E> friend int autocorrelated_run(E&, const HmmSource*, int, int, const int*, const int*, int, const double*, double*, double*);
    template <class E> friend int matrix_list_run(E&, const char*, bool, const int*, const int*, const int*, int);
    template <class E> friend int matrix_list_set(E&, const char*, const int*, const double*, int);
    template <class E> friend int rate_exponential_run(E&, const char*, const double*, const int*, const int*, const int*, const double*, int);
    // everything queued runs first
    int runQueued() { return flushQueue(); }
    // ---- ... and the bodies of the matrix-product calls (mbamd_matrix_products.h) ----
    // where the two copies of a matrix buffer lie: the device form of setMatrix / getMatrix
    MatrixLayoutF64 matrixLayout() const { return MatrixLayoutF64{S, SPAD, K}; }
    // (setMatrix runs the queues before a matrix changes: runQueued has)
    int beforeMatrixWrite() { return BEAGLE_SUCCESS; }
    // the entry table of a list, staged as runMatrices stages its jobs
    int stageMatrixTable(const void* src, size_t bytes, const void** out) { void* d = nullptr; const int rc = stage(src, bytes, &d); *out = d; return rc; }
    // the host image of a matrix buffer, both copies, from [K][S][S] doubles: what setMatrix uploads (h: matrixValues() doubles)
    size_t matrixValues() const { return matDoubles; }
    void matrixImage(const double* m, double* h) const;
    // pattern partitions are not served
    int refuses(const char* who) const { return parts.size() > 1 ? fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "not on a multi-partition instance") : BEAGLE_SUCCESS; }
    // the buffer holds compact tip states / something a kernel can read (`valid` covers tips here)
    bool holdsTip(int b) const { return isTip[b] != 0; }
    bool readable(int b) const { return valid[b] != 0; }
    // the buffer as an operand: its tip states or its partials
    const void* operandPtr(int b) const { return isTip[b] ? (const void*) statesPtr(b) : (const void*) partialsPtr(b); }
    // (every buffer is in memory, allocated, and carries nothing a write would have to clear: a tip destination is refused)
    template <class F> int beforeRead(int, F) { return BEAGLE_SUCCESS; }
    int beforeWrite(int) { return BEAGLE_SUCCESS; }
    void afterWrite(int) {}
    // the PreOp / GradEdge table of a call, on the device
    int stageTable(const void* src, size_t bytes, void** out) { return stage(src, bytes, out); }
    // device memory for a call's results
    int resultScratch(size_t bytes, double** out) { const int rc = grow_device(stream, (void**) &d_grad, &gradCap, bytes, bytes); *out = d_grad; return rc; }
    // (nothing is kept of a synchronisation)
    void afterSync() {}
    // launches for kernelTiming to report
    void countLaunches(int n) { preLaunches += (uint64_t) n; }
    // (no device timing on this engine)
    int timedBegin(hipEvent_t&, hipEvent_t&) { return BEAGLE_SUCCESS; }
    int timedEnd(hipEvent_t, hipEvent_t) { return BEAGLE_SUCCESS; }
    // what getSites would return, in d_site (after a derivative call its values are the host's: they are sent back)
    int siteLogLikelihoods(const double** dev, const double** host)
    {
        if (!haveSite) return fail(BEAGLE_ERROR_GENERAL, "beagleGetSiteLogLikelihoods: no log-likelihood was calculated");
        if (derivValid) {
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipMemcpy(d_site, derivSite.data(), (size_t) P * sizeof(double), hipMemcpyHostToDevice));
        }
        *dev = d_site;
        *host = nullptr;
        return BEAGLE_SUCCESS;
    }
    const HostMirror& weightsMirror() const { return hostWeights; }
    long secondLaunches[2] = {0, 0};  // order-2 read-out launches of edge_readout: plain / matrix-core kernel
    long insertionLaunches[2] = {0, 0};   // launches of insertion_log_likelihoods: plain / matrix-core form
    // the cumulative exponents of a scale buffer as a kernel reads them: [Ppad]
    int cumulativeExponents(int idx, const int32_t*& out) { out = d_scale + (size_t) idx * Ppad; return BEAGLE_SUCCESS; }
    // f(this engine's layout as a compile-time constant)
    template <class F> auto withLayout(F&& f) const { return f(std::integral_constant<int, DERIV_F64>()); }
    int posteriorOperands(DerivArgs& a);
    // ---- matrix updates waiting to run ----
    // Matrix updates are queued like operation lists: MrBayes updates a codon model's eigen parts one call each (src/mbbeagle.c:1475-1486),
    // and three launches of 200 matrices fill the chip worse than one of 600.  Every other entry point flushes (flushQueue); a second
    // update of a queued matrix, or another category-rate vector, flushes first.
    std::vector<MatrixJob64> matQueue;
    std::vector<char> matQueued;               // per matrix buffer: an update is in the queue
    int matQueueRate = -1;

    static int blockOf(int S) { return S <= 4 ? 4 : S <= 8 ? 8 : S <= 16 ? 16 : S <= 20 ? 20 : 32; }
    double* partialsPtr(int b) const { return d_partials + (size_t) b * bufDoubles; }
    uint8_t* statesPtr(int b) const { return d_states + (size_t) stateSlot[b] * Ppad; }
    double* matrixPtr(int m) const { return d_matrices + (size_t) m * matDoubles; }
    void destroy();
    int ringPut(const void* src, size_t bytes, uint8_t** hostSlot, uint8_t** devSlot);
    int stage(const void* src, size_t bytes, void** out);
    int upload(void* dst, const void* src, size_t bytes);
    int partitionRange(int partition, int* first, int* last, const char* what) const;
    int downloadScale(int idx, const char* what, std::vector<int32_t>& h);
    template <int ORDER, bool CX> void launchMatrices(const MatrixJob64* dj, int count);
    template <int ORDER, bool CX = false> int runMatrices(const std::vector<MatrixJob64>& jobs);
    int flushMatrices();
    int flushQueue();
    int runPartials(const QueuedOp* qd, int n);
    template <int KP> void launchWalk(const Walk64Args& wa);
    int tryWalk4(const QueuedOp* q, int n);
    // a list's descriptors in the order they are launched: level-major, one contiguous run per level
    struct LevelList {
        std::vector<Op64> ops;
        std::vector<int> start;                  // first operation of each level, and the end
        std::vector<int> tipsOf;                 // per level: that many operations on two compact tips, first in the level's run
        int levels() const { return (int) tipsOf.size(); }
    };
    int describeOps(const QueuedOp* qd, int n, std::vector<Op64>& h, std::vector<int>& level, int* levels);
    void sortByLevel(const std::vector<Op64>& h, const std::vector<int>& level, int nLevels, LevelList& out);
    bool chainKernelServes(int n) const;
    bool findChains(const std::vector<Op64>& sorted, std::vector<Op64>& chained, std::vector<int>& chainStart) const;
    int launchChains(const std::vector<Op64>& chained, const std::vector<int>& chainStart);
    void launchLevel(const LevelList& list, const Op64* dops, int l);
    template <int NT, int KF> void launchMfma(bool viaLds, bool wide, dim3 grid, dim3 lgrid, size_t ldsBytes, const Op64* ops);
    template <int IB_> void launchPartials(const Op64* ops, int n);
};

// ---- the instance: beagleCreateInstance / beagleFinalizeInstance ----
inline int Engine64::create(const Dims& dim, int patterns, int dev, const Switches& switches)
{
    sw = switches;
    device = dev; tipCount = dim.tipCount; nBuffers = dim.partialsBufferCount + dim.compactBufferCount; S = dim.stateCount; P = patterns; Ppad = round_up(patterns, 64);
    K = dim.categoryCount; nEigen = dim.eigenBufferCount; nMatrices = dim.matrixBufferCount; nScale = dim.scaleBufferCount;
    IB = blockOf(S);
    SPAD = (S + IB - 1) / IB * IB;
    bufDoubles = (size_t) K * S * Ppad;
    matDoubles = (size_t) K * S * S + (size_t) K * S * SPAD;
    complexEigen = dim.complexEigen;
    eigDoubles = eigen_imag_offset64(S) + (size_t) 2 * S;      // [U | U^-1 | lambda | b | side]: the last two are a complex instance's (k64_exponentials)
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    live = true;
    HIP_TRY(hipMalloc(&d_partials, std::max<size_t>(1, (size_t) nBuffers * bufDoubles) * sizeof(double)));
    HIP_TRY(hipMalloc(&d_states, std::max<size_t>(1, (size_t) tipCount * Ppad)));
    HIP_TRY(hipMalloc(&d_matrices, std::max<size_t>(1, (size_t) nMatrices * matDoubles) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(d_matrices, 0, std::max<size_t>(1, (size_t) nMatrices * matDoubles) * sizeof(double), stream));
    HIP_TRY(hipMalloc(&d_eigen, std::max<size_t>(1, (size_t) nEigen * eigDoubles) * sizeof(double)));
    // (a complex instance's kernels index U with `side`: an eigen buffer never set must not send them out of the buffer)
    if (complexEigen) HIP_TRY(hipMemsetAsync(d_eigen, 0, std::max<size_t>(1, (size_t) nEigen * eigDoubles) * sizeof(double), stream));
    HIP_TRY(hipMalloc(&d_freqs, std::max<size_t>(1, (size_t) nEigen * S) * sizeof(double)));
    HIP_TRY(hipMalloc(&d_weights, std::max<size_t>(1, (size_t) nEigen * K) * sizeof(double)));
    HIP_TRY(hipMalloc(&d_pweights, (size_t) Ppad * sizeof(double)));
    HIP_TRY(hipMemsetAsync(d_pweights, 0, (size_t) Ppad * sizeof(double), stream));
    // (one row more than the caller's: the scratch row the walk's entries without a scale buffer write their zero exponents to)
    HIP_TRY(hipMalloc(&d_scale, (size_t) (nScale + 1) * Ppad * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(d_scale, 0, (size_t) (nScale + 1) * Ppad * sizeof(int32_t), stream));
    HIP_TRY(hipMalloc(&d_site, (size_t) Ppad * sizeof(double)));
    HIP_TRY(hipMalloc(&d_sums, (size_t) (Ppad / 64) * sizeof(double)));
    sumsCap = (size_t) (Ppad / 64) * sizeof(double);
    isTip.assign((size_t) nBuffers, 0);
    stateSlot.assign((size_t) nBuffers, -1);
    valid.assign((size_t) nBuffers, 0);
    std::vector<double> ones((size_t) Ppad, 0.0);
    for (int c = 0; c < P; ++c) ones[c] = 1.0;
    HIP_TRY(hipMemcpyAsync(d_pweights, ones.data(), (size_t) Ppad * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return BEAGLE_SUCCESS;
}
inline void Engine64::destroy()
{
    if (!live) return;
    (void) hipSetDevice(device);
    (void) hipStreamSynchronize(stream);
    void* all[] = {d_partials, d_states, d_matrices, d_eigen, d_freqs, d_weights, d_pweights, d_scale, d_site, d_sums, d_ev, d_stage, d_deriv, d_q, d_grad};
    for (void* p : all)
        if (p) (void) hipFree(p);
    if (d_ring) (void) hipFree(d_ring);
    ring.destroy();
    if (h_sums) (void) hipHostFree(h_sums);
    (void) hipStreamDestroy(stream);
    live = false;
}

// ---- small host -> device transfers: through the ring, or (too large for it) the staging buffer ----
// a ring slot holding `bytes` from src (host and device side), or nullptr when the item is too large for the ring
inline int Engine64::ringPut(const void* src, size_t bytes, uint8_t** hostSlot, uint8_t** devSlot)
{
    *hostSlot = *devSlot = nullptr;
    if (bytes > RING_MAX_ITEM || sw.f64NoRing) return BEAGLE_SUCCESS;
    if (!ring.live()) { const int rc = ring.create(RING_BYTES, 256); if (rc) return rc; }
    if (d_ring == nullptr) HIP_TRY(hipMalloc((void**) &d_ring, RING_BYTES));
    size_t off = 0;
    const int rc = ring.put(src, bytes, stream, &off);      // (wrapped: every slot's copy and its readers are behind us)
    if (rc) return rc;
    *hostSlot = ring.host(off);
    *devSlot = d_ring + off;
    return BEAGLE_SUCCESS;
}
inline int Engine64::stage(const void* src, size_t bytes, void** out)
{
    {
        uint8_t *hs, *ds;
        int rc = ringPut(src, bytes, &hs, &ds);
        if (rc) return rc;
        if (ds != nullptr) {
            HIP_TRY(hipMemcpyAsync(ds, hs, bytes, hipMemcpyHostToDevice, stream));
            *out = ds;
            return BEAGLE_SUCCESS;
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));                  // (the staging buffer is re-used: wait for its last reader)
    { const int rc = grow_device(stream, &d_stage, &stageCap, bytes, std::max(bytes * 2, (size_t) 65536)); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(d_stage, src, bytes, hipMemcpyHostToDevice, stream));
    *out = d_stage;
    return BEAGLE_SUCCESS;
}
inline int Engine64::upload(void* dst, const void* src, size_t bytes)
{
    {
        uint8_t *hs, *ds;
        int rc = ringPut(src, bytes, &hs, &ds);
        if (rc) return rc;
        if (hs != nullptr) {                                 // (stream order keeps it behind the earlier readers of dst)
            HIP_TRY(hipMemcpyAsync(dst, hs, bytes, hipMemcpyHostToDevice, stream));
            return BEAGLE_SUCCESS;
        }
    }
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return BEAGLE_SUCCESS;
}

// ---- beagleSetPatternPartitions, beagleSetTipStates ... beagleSetPatternWeights ----
inline int Engine64::setPartitions(int count, const int* ids)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    std::vector<std::pair<int, int>> r;
    { const int rc = pattern_partition_ranges(ids, P, count, r); if (rc) return rc; }
    for (std::pair<int, int>& range : r) range.second += range.first;      // (first, count) -> [first, last)
    parts = r;
    return BEAGLE_SUCCESS;
}
inline int Engine64::partitionRange(int partition, int* first, int* last, const char* what) const
{
    if (partition < 0) { *first = 0; *last = Ppad; return BEAGLE_SUCCESS; }
    if (parts.empty() ? partition != 0 : partition >= (int) parts.size()) return fail(BEAGLE_ERROR_OUT_OF_RANGE, what, "partition index");
    if (parts.empty()) { *first = 0; *last = Ppad; return BEAGLE_SUCCESS; }
    *first = parts[partition].first;
    *last = parts[partition].second;
    return BEAGLE_SUCCESS;
}
inline int Engine64::setTipStates(int tip, const int* states)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (tip < 0 || tip >= nBuffers) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetTipStates: tip index");
    if (stateSlot[tip] < 0) {
        if (slotsUsed >= tipCount) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetTipStates: more compact buffers than tips");
        stateSlot[tip] = slotsUsed++;
    }
    std::vector<uint8_t> h((size_t) Ppad, (uint8_t) S);
    for (int c = 0; c < P; ++c) h[c] = (uint8_t) ((states[c] < 0 || states[c] >= S) ? S : states[c]);
    isTip[tip] = 1;
    valid[tip] = 1;
    if (!preOrder.empty()) preOrder[tip] = 0;
    return upload(statesPtr(tip), h.data(), (size_t) Ppad);
}
inline int Engine64::setPartials(int idx, const double* in, bool withCategories)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nBuffers) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetPartials: buffer index");
    std::vector<double> h(bufDoubles, 0.0);
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < P; ++c)
            for (int i = 0; i < S; ++i)
                h[((size_t) k * S + i) * Ppad + c] = in[((size_t) (withCategories ? k : 0) * P + c) * S + i];
    isTip[idx] = 0;
    valid[idx] = 1;
    if (!preOrder.empty()) preOrder[idx] = 0;
    return upload(partialsPtr(idx), h.data(), bufDoubles * sizeof(double));
}
inline int Engine64::getPartials(int idx, double* out)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nBuffers || !valid[idx]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleGetPartials: buffer index");
    if (isTip[idx]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleGetPartials: a compact (tip state) buffer");
    std::vector<double> h(bufDoubles);
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(h.data(), partialsPtr(idx), bufDoubles * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < P; ++c)
            for (int i = 0; i < S; ++i) out[((size_t) k * P + c) * S + i] = h[((size_t) k * S + i) * Ppad + c];
    return BEAGLE_SUCCESS;
}
inline int Engine64::setEigen(int idx, const double* U, const double* Ui, const double* lam)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetEigenDecomposition: eigen index");
    std::vector<double> h(eigDoubles, 0.0);
    std::memcpy(h.data(), U, sizeof(double) * S * S);
    std::memcpy(h.data() + (size_t) S * S, Ui, sizeof(double) * S * S);
    std::memcpy(h.data() + (size_t) 2 * S * S, lam, sizeof(double) * S);
    if (complexEigen) {                    // `lam` holds 2 S values: the real parts, then the imaginary parts
        double* im = h.data() + eigen_imag_offset64(S);
        std::memcpy(im, lam + S, sizeof(double) * S);
        if (!eigen_pairs(lam, im, S, im + S))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetEigenDecomposition: an imaginary part without its adjacent conjugate, or a non-finite eigenvalue");
    }
    return upload(d_eigen + (size_t) idx * eigDoubles, h.data(), eigDoubles * sizeof(double));
}
inline int Engine64::setFreqs(int idx, const double* f)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetStateFrequencies: index");
    // (MrBayes sets the frequencies and category weights of every eigen part before every evaluation: unchanged values are not sent again)
    return hostFreqs.send((size_t) nEigen * S, (size_t) idx * S, f, (size_t) S, [&] { return upload(d_freqs + (size_t) idx * S, f, (size_t) S * sizeof(double)); });
}
inline int Engine64::setWeights(int idx, const double* w)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetCategoryWeights: index");
    return hostWeights.send((size_t) nEigen * K, (size_t) idx * K, w, (size_t) K, [&] { return upload(d_weights + (size_t) idx * K, w, (size_t) K * sizeof(double)); });
}
inline int Engine64::setRates(int index, const double* r)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    return rateSets.set(index, r, K);
}
inline int Engine64::setPatternWeights(const double* w)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    std::vector<double> h((size_t) Ppad, 0.0);
    std::memcpy(h.data(), w, (size_t) P * sizeof(double));
    return upload(d_pweights, h.data(), (size_t) Ppad * sizeof(double));
}

// ---- beagleUpdateTransitionMatrices, beagleSet / GetTransitionMatrix ----
template <int ORDER, bool CX> inline void Engine64::launchMatrices(const MatrixJob64* dj, int count)
{
    if (S >= 16 && S <= 64) {
        const unsigned grid = (unsigned) (count * K);
        switch ((S + 15) / 16) {
            case 1: MBAMD_LAUNCH_BARRIER((k64_matrices_mfma<1, ORDER, CX>), grid, 64, 0, stream, dj, (const double*) d_ev, S, SPAD, K); break;
            case 2: MBAMD_LAUNCH_BARRIER((k64_matrices_mfma<2, ORDER, CX>), grid, 128, 0, stream, dj, (const double*) d_ev, S, SPAD, K); break;
            case 3: MBAMD_LAUNCH_BARRIER((k64_matrices_mfma<3, ORDER, CX>), grid, 192, 0, stream, dj, (const double*) d_ev, S, SPAD, K); break;
            default: MBAMD_LAUNCH_BARRIER((k64_matrices_mfma<4, ORDER, CX>), grid, 256, 0, stream, dj, (const double*) d_ev, S, SPAD, K); break;
        }
        return;
    }
    MBAMD_LAUNCH((k64_matrices<ORDER, CX>), (unsigned) (count * K), 256, 0, stream, dj, (const double*) d_ev, S, SPAD, K);
}
// the exponentials and the matrices of `jobs`, all of one derivative ORDER (the launches share d_ev: stream order keeps them apart);
// CX: the kernels' form for complex eigen-systems, which a complex instance takes (d_ev then holds the factor pair: twice the doubles)
template <int ORDER, bool CX> inline int Engine64::runMatrices(const std::vector<MatrixJob64>& jobs)
{
    if (jobs.empty()) return BEAGLE_SUCCESS;
    if constexpr (!CX) {
        if (complexEigen) return runMatrices<ORDER, true>(jobs);
    }
    const int count = (int) jobs.size();
    void* dj = nullptr;
    int rc = stage(jobs.data(), jobs.size() * sizeof(MatrixJob64), &dj);
    if (rc) return rc;
    const size_t need = (size_t) (CX ? 2 : 1) * count * K * S * sizeof(double);
    rc = grow_device(stream, (void**) &d_ev, &evCap, need, need * 2);
    if (rc) return rc;
    const int total = count * K * S;
    MBAMD_LAUNCH((k64_exponentials<ORDER, CX>), (unsigned) ((total + 255) / 256), 256, 0, stream, (const MatrixJob64*) dj, rateSets[matQueueRate], S, K, total, d_ev);
    launchMatrices<ORDER, CX>((const MatrixJob64*) dj, count);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}
inline int Engine64::flushMatrices()
{
    if (matQueue.empty()) return BEAGLE_SUCCESS;
    std::vector<MatrixJob64> jobs;
    jobs.swap(matQueue);
    std::fill(matQueued.begin(), matQueued.end(), 0);
    bool derivatives = false;
    for (const MatrixJob64& j : jobs) derivatives = derivatives || j.pad_ != 0.0;
    if (!derivatives) return runMatrices<0>(jobs);
    std::vector<MatrixJob64> byOrder[3];       // one launch per derivative order (MatrixJob64::pad_)
    for (MatrixJob64 j : jobs) {
        const int order = j.pad_ == 1.0 ? 1 : (j.pad_ == 2.0 ? 2 : 0);
        j.pad_ = 0.0;
        byOrder[order].push_back(j);
    }
    int rc = runMatrices<0>(byOrder[0]);
    if (rc == BEAGLE_SUCCESS) rc = runMatrices<1>(byOrder[1]);
    if (rc == BEAGLE_SUCCESS) rc = runMatrices<2>(byOrder[2]);
    return rc;
}
inline int Engine64::updateMatrices(int eigenIdx, int rateIdx, const int* prob, const double* lengths, int count, const int* d1, const int* d2)
{
    if (!queue.empty()) { const int rcq = flushQueue(); if (rcq) return rcq; }        // (queued operations read the matrices as they are now)
    if (count <= 0) return BEAGLE_SUCCESS;
    if (eigenIdx < 0 || eigenIdx >= nEigen) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: eigen index");
    if (!rateSets.has(rateIdx)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: rate index");
    const int* const outIdx[3] = {prob, d1, d2};
    std::vector<char> seen;
    if (d1 || d2) seen.assign((size_t) nMatrices, 0);
    size_t njobs = 0;
    for (int o = 0; o < 3; ++o)
        for (int i = 0; outIdx[o] && i < count; ++i) {
            const int m = outIdx[o][i];
            if (m < 0 || m >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: matrix index");
            if (!seen.empty()) {
                if (o > 0 && seen[(size_t) m]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdateTransitionMatrices: a derivative index equals another output of the call");
                seen[(size_t) m] = 1;
            }
            ++njobs;
        }
    if (!matQueue.empty() && (matQueueRate != rateIdx || matQueue.size() + njobs > 60000)) { const int rc = flushMatrices(); if (rc) return rc; }
    if (matQueued.size() != (size_t) nMatrices) matQueued.assign((size_t) nMatrices, 0);
    matQueueRate = rateIdx;
    for (int o = 0; o < 3; ++o)
        for (int i = 0; outIdx[o] && i < count; ++i) {
            const int m = outIdx[o][i];
            if (matQueued[(size_t) m]) { const int rc = flushMatrices(); if (rc) return rc; }
            matQueued[(size_t) m] = 1;
            matQueue.push_back({matrixPtr(m), lengths[i], d_eigen + (size_t) eigenIdx * eigDoubles, (double) o});
        }
    return sw.f64NoMatrixQueue ? flushMatrices() : BEAGLE_SUCCESS;
}
inline int Engine64::updateMatricesMulti(const int* eigenIdx, const int* rateIdx, const int* prob, const double* lengths, int count,
                        const int* d1, const int* d2)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    int i = 0;
    while (i < count) {
        int j = i + 1;
        while (j < count && eigenIdx[j] == eigenIdx[i] && rateIdx[j] == rateIdx[i]) ++j;
        const int rc = updateMatrices(eigenIdx[i], rateIdx[i], prob + i, lengths + i, j - i, d1 ? d1 + i : nullptr, d2 ? d2 + i : nullptr);
        if (rc) return rc;
        i = j;
    }
    return BEAGLE_SUCCESS;
}
inline void Engine64::matrixImage(const double* m, double* h) const
{
    std::fill(h, h + matDoubles, 0.0);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const double v = m[((size_t) k * S + i) * S + j];
                h[((size_t) k * S + i) * S + j] = v;
                h[(size_t) K * S * S + ((size_t) k * S + j) * SPAD + i] = v;
            }
}
inline int Engine64::setMatrix(int idx, const double* m)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleSetTransitionMatrix: matrix index");
    std::vector<double> h(matDoubles);
    matrixImage(m, h.data());
    return upload(matrixPtr(idx), h.data(), matDoubles * sizeof(double));
}
inline int Engine64::convolveMatrices(const int* first, const int* second, const int* result, int count)
{
    return matrix_list_run(*this, "beagleConvolveTransitionMatrices", true, first, second, result, count);
}
inline int Engine64::transposeMatrices(const int* input, const int* result, int count)
{
    return matrix_list_run(*this, "beagleTransposeTransitionMatrices", false, input, (const int*) nullptr, result, count);
}
inline int Engine64::setMatrices(const int* idx, const double* in, int count) { return matrix_list_set(*this, "beagleSetTransitionMatrices", idx, in, count); }
inline int Engine64::updateMatricesFromRateMatrix(const double* q, const int* prob, const int* d1, const int* d2, const double* lengths, int count)
{
    return rate_exponential_run(*this, "mbamdUpdateTransitionMatricesFromRateMatrix", q, prob, d1, d2, lengths, count);
}
inline int Engine64::getMatrix(int idx, double* out)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleGetTransitionMatrix: matrix index");
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(out, matrixPtr(idx), (size_t) K * S * S * sizeof(double), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}

// ---- beagleUpdatePartials: the queue, and what a flush runs ----
inline int Engine64::updatePartials(const BeagleOperation* ops, int n, int cumIdx)
{
    std::vector<int> part((size_t) std::max(n, 0), -1), cum((size_t) std::max(n, 0), cumIdx);
    return updatePartialsEx(ops, sizeof(BeagleOperation), n, part.data(), cum.data());
}
// `stride` bytes between operations (BeagleOperation or BeagleOperationByPartition: the first seven ints are the same);
// partition[i] < 0: all patterns.
// Lists are QUEUED, not run: MrBayes submits one list per eigen-system part of a codon model (reference src/mbbeagle.c:1088-1104,
// with at most a beagleRemoveScaleFactors of the next part's buffers in between), and a launch per dependency level of every
// list is three times the launches of one launch per level of all of them (codon M3 100 x 5 000: 51 -> 17 launches, 1.37 -> 1.0 ms per evaluation).
// Every other call of the engine runs the queue first (flushQueue); everything that can fail is checked here, when the list comes.
inline int Engine64::updatePartialsEx(const void* opsRaw, size_t stride, int n, const int* partition, const int* cumOf)
{
    if (n <= 0) return BEAGLE_SUCCESS;
    // (the matrix updates are complete when the first operation list comes: the device computes them while the host queues and sorts the lists)
    if (!matQueue.empty()) { const int rcm = flushMatrices(); if (rcm) return rcm; }
    const size_t mark = queue.size();
    const int np = std::max<int>(1, (int) parts.size());
    for (int i = 0; i < n; ++i) {
        const BeagleOperation& o = *reinterpret_cast<const BeagleOperation*>(static_cast<const char*>(opsRaw) + (size_t) i * stride);
        const int cumIdx = cumOf[i];
        int rc = BEAGLE_SUCCESS;
        int first = 0, last = Ppad;
        const int d = o.destinationPartials, c1 = o.child1Partials, c2 = o.child2Partials;
        const int sw = o.destinationScaleWrite, sr = o.destinationScaleRead;
        if (cumIdx != BEAGLE_OP_NONE && (cumIdx < 0 || cumIdx >= nScale)) rc = fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: cumulative scale index");
        else if ((rc = partitionRange(partition[i], &first, &last, "beagleUpdatePartialsByPartition")) != BEAGLE_SUCCESS) { }
        else if (d < 0 || d >= nBuffers || c1 < 0 || c1 >= nBuffers || c2 < 0 || c2 >= nBuffers)
            rc = fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: buffer index");
        else if (o.child1TransitionMatrix < 0 || o.child1TransitionMatrix >= nMatrices || o.child2TransitionMatrix < 0 || o.child2TransitionMatrix >= nMatrices)
            rc = fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: matrix index");
        else if (!valid[c1] || !valid[c2]) rc = fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: a child buffer was never written");
        else if (isTip[d]) rc = fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: destination is a compact tip buffer");
        else if ((sw != BEAGLE_OP_NONE && (sw < 0 || sw >= nScale)) || (sr != BEAGLE_OP_NONE && (sr < 0 || sr >= nScale)))
            rc = fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePartials: scale index");
        if (rc != BEAGLE_SUCCESS) { queue.resize(mark); return rc; }          // (nothing of a rejected list runs)
        QueuedOp e;
        e.op = o; e.partition = partition[i]; e.cum = cumIdx;
        e.tip1 = isTip[c1]; e.tip2 = isTip[c2];                                // (what the children are NOW: a later operation may overwrite a tip buffer)
        queue.push_back(e);
        valid[d] = 1;
        isTip[d] = 0;
        if (!preOrder.empty()) preOrder[d] = 0;              // (no longer the rest-of-tree vector of a pre-order pass)
        if (queuedScale.size() != (size_t) std::max(nScale, 1)) queuedScale.assign((size_t) std::max(nScale, 1), 0);
        if (sw != BEAGLE_OP_NONE) queuedScale[sw] = 1;
        if (sr != BEAGLE_OP_NONE) queuedScale[sr] = 1;
        if (cumIdx != BEAGLE_OP_NONE) queuedScale[cumIdx] = 1;
    }
    (void) np;
    return BEAGLE_SUCCESS;
}
// run what updatePartials queued; called first by every other entry point
// (an error returned from here means the queued lists were DROPPED -- the queue is empty afterwards, whichever entry point
//  reported it: the client resubmits them, as after any failed beagleUpdatePartials)
inline int Engine64::flushQueue()
{
    { const int rcm = flushMatrices(); if (rcm) return rcm; }
    if (queue.empty()) return BEAGLE_SUCCESS;
    std::vector<QueuedOp> q;
    q.swap(queue);
    std::fill(queuedScale.begin(), queuedScale.end(), 0);
    return runPartials(q.data(), (int) q.size());
}
inline int Engine64::runPartials(const QueuedOp* qd, int n)
{
    {
        int rcw = tryWalk4(qd, n);
        if (rcw != 1) return rcw;                      // (1: not a list for the walk -- the level path below takes it)
    }
    std::vector<Op64> h;
    std::vector<int> level;
    int nLevels = 0;
    { const int rcp = describeOps(qd, n, h, level, &nLevels); if (rcp) return rcp; }
    LevelList list;
    sortByLevel(h, level, nLevels, list);
    if (chainKernelServes(n)) {
        std::vector<Op64> chained;
        std::vector<int> chainStart;
        if (findChains(list.ops, chained, chainStart)) {
            const int rcc = launchChains(chained, chainStart);
            if (rcc != 1) return rcc;
        }
    }
    void* dv = nullptr;
    int rc = stage(list.ops.data(), list.ops.size() * sizeof(Op64), &dv);
    if (rc) return rc;
    for (int l = 0; l < list.levels(); ++l) launchLevel(list, static_cast<const Op64*>(dv), l);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// ---- four states: the tree walk ----
template <int KP> inline void Engine64::launchWalk(const Walk64Args& wa)
{
    auto kern = k64_walk4<KP>;
    const size_t lds = ((size_t) wa.nslots * 4 * 64 + (size_t) 2 * KP * 18) * sizeof(double);
    static char raised[64] = {0};                // per device (and per KP: a static of this template instance)
    if (device >= 0 && device < 64 && !raised[device]) {
        if (hipFuncSetAttribute((const void*) kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void) hipGetLastError();
        raised[device] = 1;
    }
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (Ppad / (64 / KP)), 64, lds, stream, wa);
}
// The walk serves what MrBayes sends for nucleotides: four states, up to eight categories, no pattern partitions, one
// cumulative buffer for the whole list, no buffer hazards inside the list.  Returns 1 when the list is not of that kind.
inline int Engine64::tryWalk4(const QueuedOp* q, int n)
{
    // (the kernel addresses with 32-bit lane offsets: a plane of partials and the whole exponent array below 4 GiB)
    if (sw.f64NoWalk || S != 4 || K > 8 || !parts.empty() || n < 2 || (bufDoubles >> 29) != 0 || (((size_t) nScale + 1) * Ppad >> 30) != 0 || ((size_t) nMatrices * matDoubles >> 29) != 0) return 1;
    // the walk is one latency chain per wave: it wins when there are enough waves (break-even about 1.2 per SIMD) and on short lists (a
    // root-ward path: one launch instead of one per operation); mid-sized full evaluations stay on the level kernels
    // (measured: profiles/r03_f64_walk.txt).  MBAMD_F64_WALK_ALWAYS=1: every eligible list.
    if (!sw.f64WalkAlways && n > 64 && (long) (Ppad / 64) * K < 1200) return 1;
    std::unique_ptr<StatTimer> st_(new StatTimer(ST_PLAN));      // (MBAMD_STATS: the host side of the walk, up to the upload)
    std::vector<Walk4Op>& wops = walkOps;
    wops.clear();
    std::vector<char> written((size_t) nBuffers, 0), readB((size_t) nBuffers, 0), sc((size_t) std::max(nScale, 1), 0);
    for (int i = 0; i < n; ++i) {
        const BeagleOperation& o = q[i].op;                                       // (indices were checked when the list was queued)
        if (q[i].partition >= 0 || q[i].cum != q[0].cum) return 1;
        const int d = o.destinationPartials, c1 = o.child1Partials, c2 = o.child2Partials;
        const int sw = o.destinationScaleWrite, sr = o.destinationScaleRead;
        if (written[d] || readB[d]) return 1;                                     // buffer hazards: levels
        if (sw != BEAGLE_OP_NONE && sc[sw]) return 1;
        if (sw == BEAGLE_OP_NONE && sr != BEAGLE_OP_NONE && sc[sr] == 2) return 1;
        if (q[0].cum != BEAGLE_OP_NONE && (sw == q[0].cum || sr == q[0].cum)) return 1;
        Walk4Op w;
        w.dst = d; w.c1 = c1; w.c2 = c2; w.m1 = o.child1TransitionMatrix; w.m2 = o.child2TransitionMatrix;
        w.tip1 = q[i].tip1;
        w.tip2 = q[i].tip2;
        w.scaleWrite = sw != BEAGLE_OP_NONE ? sw : -1;
        w.scaleRead = (sw == BEAGLE_OP_NONE && sr != BEAGLE_OP_NONE) ? sr : -1;
        written[d] = 1; readB[c1] = 1; readB[c2] = 1;
        if (sw != BEAGLE_OP_NONE) sc[sw] = 2; else if (sr != BEAGLE_OP_NONE && !sc[sr]) sc[sr] = 1;
        wops.push_back(w);
    }
    const int cumIdx = q[0].cum;
    // launch geometry: a wave owns 64 / KP patterns (KP = K rounded up to a power of two) and is its own workgroup; every wave
    // resident at once where the chip allows, the LDS of a CU split between the waves it hosts; a slot holds one node's
    // 4 x 64 doubles of the wave
    const int KP = K <= 1 ? 1 : (K <= 2 ? 2 : (K <= 4 ? 4 : 8));
    const int slotBytes = 4 * 64 * (int) sizeof(double);
    const long waves = Ppad / (64 / KP);
    const int perCU = (int) std::min(16L, std::max(1L, (waves + 255) / 256));
    const int fixedBytes = 2 * KP * 18 * (int) sizeof(double) + 64;      // the parked matrices (+ allocation granularity)
    int nslots = std::max(2, std::min(24, ((160 * 1024) / perCU - fixedBytes) / slotBytes));
    if (sw.f64WalkSlots) nslots = std::max(2, std::min((160 * 1024 - fixedBytes) / slotBytes, *sw.f64WalkSlots));
    // structure key: who produces whose child, which children are tips (the indices only fill the program)
    std::vector<int> key;
    key.reserve((size_t) n * 3 + 2);
    key.push_back(n); key.push_back(nslots);
    {
        std::vector<int> writer((size_t) nBuffers, -1);
        for (int o = 0; o < n; ++o) {
            key.push_back(wops[o].tip1 ? -1 : writer[wops[o].c1]);
            key.push_back(wops[o].tip2 ? -1 : writer[wops[o].c2]);
            key.push_back((int) wops[o].tip1 | ((int) wops[o].tip2 << 1));
            writer[wops[o].dst] = o;
        }
    }
    if (key != walkKey) {
        Walk4Builder& b = walkBuilder;
        b.maxW = 1; b.maxSlots = nslots; b.maxSlots1 = nslots; b.prefetchDistance = 0; b.memSlots = false;
        b.leadNops = 0; b.unroll = 1; b.tailNops = 0; b.forward = false; b.smallPhase = 1 << 30;
        if (!b.build(wops, walkTemplate)) { walkKey.clear(); return 1; }
        walkKey = key;
    }
    const Walk4Template& t = walkTemplate;
    if (t.W != 1) return 1;
    walkProg.assign((size_t) t.entries, Walk64Entry());
    const unsigned scratch = (unsigned) nScale;                 // the extra exponent row: what entries without a scale buffer "write"
    for (int i = 0; i < t.entries; ++i) {
        const Walk4Template::Entry& te = t.prog[i];
        Walk64Entry& e = walkProg[i];
        std::memset(&e, 0, sizeof e);
        e.scaleR = e.scaleW = scratch;
        unsigned kind1 = 0, kind2 = 0, slot1 = 0, slot2 = 0;
        if (te.op < 0) { e.ctl = 1u << 6; continue; }                     // (dropped below)
        const Walk4Op& w = wops[te.op];
        e.dst = (uint32_t) w.dst; e.m1 = (uint32_t) w.m1; e.m2 = (uint32_t) w.m2;
        if (w.tip1) { kind1 = 2; e.c1 = (uint32_t) stateSlot[w.c1]; }
        else if (te.c1slot == 0xFF) { kind1 = 1; e.c1 = (uint32_t) w.c1; }
        else { kind1 = 0; slot1 = te.c1slot; }
        if (w.tip2) { kind2 = 2; e.c2 = (uint32_t) stateSlot[w.c2]; }
        else if (te.c2slot == 0xFF) { kind2 = 1; e.c2 = (uint32_t) w.c2; }
        else { kind2 = 0; slot2 = te.c2slot; }
        const unsigned mode = w.scaleWrite >= 0 ? 1u : (w.scaleRead >= 0 ? 2u : 0u);
        if (mode == 1u) e.scaleW = (uint32_t) w.scaleWrite;
        if (mode == 2u) e.scaleR = (uint32_t) w.scaleRead;
        e.ctl = kind1 | (kind2 << 2) | (mode << 4) | (slot1 << 8) | (slot2 << 16) | ((unsigned) te.dslot << 24);
    }
    // the kernel's entries all compute (see k64_walk4): drop the no-operation entries of the builder (one wave: they order nothing)
    walkProg.erase(std::remove_if(walkProg.begin(), walkProg.end(), [](const Walk64Entry& e) { return ((e.ctl >> 6) & 1u) != 0; }), walkProg.end());
    if (walkProg.empty()) return 1;
    {   // the kernel fetches entry i's memory children while entry i-1 runs: their producer must be entry i-2 or earlier
        std::vector<int> writtenAt((size_t) nBuffers, -1000);
        for (size_t i = 0; i < walkProg.size(); ++i) {
            const Walk64Entry& e = walkProg[i];
            if (((e.ctl & 3u) == 1u && writtenAt[e.c1] >= (int) i - 1) || (((e.ctl >> 2) & 3u) == 1u && writtenAt[e.c2] >= (int) i - 1)) { walkKey.clear(); return 1; }
            writtenAt[e.dst] = (int) i;
        }
    }
    if (sw.verbose) {
        int mem = 0, tips = 0;
        for (const Walk64Entry& e : walkProg) {
            mem += ((e.ctl & 3u) == 1u) + (((e.ctl >> 2) & 3u) == 1u);
            tips += ((e.ctl & 3u) == 2u) + (((e.ctl >> 2) & 3u) == 2u);
        }
        std::fprintf(stderr, "[mbamd] fp64 walk: %zu entries, %d slots, children: %d compact tips, %d from memory, %zu from LDS\n", walkProg.size(),
                     t.nslots, tips, mem, 2 * walkProg.size() - (size_t) tips - (size_t) mem);
    }
    st_.reset();
    void* dv = nullptr;
    int rc = stage(walkProg.data(), walkProg.size() * sizeof(Walk64Entry), &dv);
    if (rc) return rc;
    Walk64Args wa;
    wa.prog = static_cast<const Walk64Entry*>(dv);
    wa.entries = (int) walkProg.size(); wa.nslots = t.nslots;
    wa.partials = d_partials; wa.bufDoubles = (unsigned) bufDoubles;
    wa.states = d_states;
    wa.matricesT = d_matrices + (size_t) K * S * S; wa.matDoubles = (unsigned) matDoubles;
    wa.scale = d_scale;
    wa.cum = cumIdx != BEAGLE_OP_NONE ? d_scale + (size_t) cumIdx * Ppad : nullptr;
    wa.Ppad = (int) Ppad;
    wa.scratchRow = nScale;
    wa.K = K;
    switch (KP) {
        case 1: launchWalk<1>(wa); break;
        case 2: launchWalk<2>(wa); break;
        case 4: launchWalk<4>(wa); break;
        default: launchWalk<8>(wa); break;
    }
    HIP_TRY(hipGetLastError());
    walkLaunches++;
    return BEAGLE_SUCCESS;
}

// ---- any state count: dependency levels, chains ----
// One launch per dependency level: an operation goes one level above the last operation that wrote a buffer it reads,
// read or wrote the buffer it writes, or touched its scale buffer.
// Hazards are tracked per (buffer, partition): the same buffer index in two partitions is two disjoint pattern ranges.
// -> the level of every operation, its descriptor h[i], and the number of levels
inline int Engine64::describeOps(const QueuedOp* qd, int n, std::vector<Op64>& h, std::vector<int>& level, int* levels)
{
    const int np = std::max<int>(1, (int) parts.size());
    std::vector<int> lastTouchBuf((size_t) nBuffers * np, -1), lastWriteBuf((size_t) nBuffers * np, -1),
        lastTouchScale((size_t) std::max(nScale, 1) * np, -1);
    level.assign((size_t) n, 0);
    h.assign((size_t) n, Op64());
    int nLevels = 0;
    for (int i = 0; i < n; ++i) {
        const BeagleOperation& o = qd[i].op;
        const int cumIdx = qd[i].cum;
        int first = 0, last = Ppad;
        int rcp = partitionRange(qd[i].partition, &first, &last, "beagleUpdatePartialsByPartition");
        if (rcp) return rcp;
        const int p0 = qd[i].partition < 0 ? 0 : std::min(qd[i].partition, np - 1), p1 = qd[i].partition < 0 ? np : p0 + 1;
        const int d = o.destinationPartials, c1 = o.child1Partials, c2 = o.child2Partials;
        const int sw = o.destinationScaleWrite, sr = o.destinationScaleRead;
        const int sc = sw != BEAGLE_OP_NONE ? sw : sr;
        int lv = 0;
        for (int q = p0; q < p1; ++q) {
            lv = std::max(lv, std::max(std::max(lastWriteBuf[(size_t) c1 * np + q], lastWriteBuf[(size_t) c2 * np + q]), lastTouchBuf[(size_t) d * np + q]) + 1);
            if (sc != BEAGLE_OP_NONE) lv = std::max(lv, lastTouchScale[(size_t) sc * np + q] + 1);
            // (lists of several calls run as one: two operations adding to the same cumulative buffer in one launch are atomic adds)
        }
        level[i] = lv;
        nLevels = std::max(nLevels, lv + 1);
        for (int q = p0; q < p1; ++q) {
            lastWriteBuf[(size_t) d * np + q] = lv;
            lastTouchBuf[(size_t) d * np + q] = std::max(lastTouchBuf[(size_t) d * np + q], lv);
            lastTouchBuf[(size_t) c1 * np + q] = std::max(lastTouchBuf[(size_t) c1 * np + q], lv);
            lastTouchBuf[(size_t) c2 * np + q] = std::max(lastTouchBuf[(size_t) c2 * np + q], lv);
            if (sc != BEAGLE_OP_NONE) lastTouchScale[(size_t) sc * np + q] = lv;
        }
        Op64& q = h[i];
        q.dst = partialsPtr(d);
        q.c1 = qd[i].tip1 ? (const void*) statesPtr(c1) : (const void*) partialsPtr(c1);
        q.c2 = qd[i].tip2 ? (const void*) statesPtr(c2) : (const void*) partialsPtr(c2);
        q.c1_tip = qd[i].tip1;
        q.c2_tip = qd[i].tip2;
        q.m1T = matrixPtr(o.child1TransitionMatrix) + (size_t) K * S * S;
        q.m2T = matrixPtr(o.child2TransitionMatrix) + (size_t) K * S * S;
        q.mode = sw != BEAGLE_OP_NONE ? 1 : sr != BEAGLE_OP_NONE ? 2 : 0;
        q.scale = sc != BEAGLE_OP_NONE ? d_scale + (size_t) sc * Ppad : nullptr;
        q.cum = cumIdx != BEAGLE_OP_NONE ? d_scale + (size_t) cumIdx * Ppad : nullptr;
        q.first = first;
        q.last = last;
        q.pad_ = 0;
    }
    *levels = nLevels;
    return BEAGLE_SUCCESS;
}
inline void Engine64::sortByLevel(const std::vector<Op64>& h, const std::vector<int>& level, int nLevels, LevelList& out)
{
    const int n = (int) h.size();
    // operations sorted by level (stable), one contiguous run per level
    std::vector<int> order((size_t) n);
    std::vector<int>& start = out.start;
    start.assign((size_t) nLevels + 1, 0);
    for (int i = 0; i < n; ++i) start[(size_t) level[i] + 1]++;
    for (int l = 0; l < nLevels; ++l) start[(size_t) l + 1] += start[l];
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i) order[(size_t) fill[level[i]]++] = i;
    // (within a level the operations on two compact tips first: they have a kernel of their own)
    std::vector<int>& tipsOf = out.tipsOf;
    tipsOf.assign((size_t) nLevels, 0);
    for (int l = 0; l < nLevels; ++l) {
        auto mid = std::stable_partition(order.begin() + start[l], order.begin() + start[(size_t) l + 1],
                                         [&](int i) { return h[(size_t) i].c1_tip && h[(size_t) i].c2_tip; });
        tipsOf[l] = (int) (mid - (order.begin() + start[l]));
    }
    out.ops.resize((size_t) n);
    for (int i = 0; i < n; ++i) out.ops[i] = h[order[i]];
}
// A list that is nothing but chains (the root-ward path of a move; one chain per eigen part) runs as one launch of
// k64_partials_chain: is the kernel there for this instance at all ...
inline bool Engine64::chainKernelServes(int n) const
{
    const int NTr = (S + 15) / 16;
    return n >= 2 && S > 16 && S <= 64 && parts.empty() && K >= 1 && K <= 4 && NTr * K <= 8 && f64_frag_lds_bytes(S, NTr, K) <= 65536 && !sw.f64MfmaNoLds &&
           !sw.f64NoChain;
}
// ... and is this list (level-major) nothing but chains?  If so: its descriptors chain by chain, Op64::pad_ saying which child is the
// previous result, and the first descriptor of every chain (and the end)
inline bool Engine64::findChains(const std::vector<Op64>& sorted, std::vector<Op64>& chained, std::vector<int>& chainStart) const
{
    const int n = (int) sorted.size();
    std::vector<int> root((size_t) n);
    for (int i = 0; i < n; ++i) root[i] = i;
    auto find = [&](int x) { while (root[x] != x) x = root[x] = root[root[x]]; return x; };
    std::unordered_map<const void*, int> owner;
    for (int i = 0; i < n; ++i) {
        const Op64& q = sorted[(size_t) i];
        // (the cumulative buffer an operation adds to is a key like its scale buffer: two operations that meet in one --
        //  one adding atomically, the other storing or reading it as its scale buffer -- must not run as independent chains)
        const void* keys[5] = {q.dst, q.c1_tip ? nullptr : q.c1, q.c2_tip ? nullptr : q.c2, q.mode != 0 ? (const void*) q.scale : nullptr, (const void*) q.cum};
        for (const void* key : keys) {
            if (key == nullptr) continue;
            auto it = owner.find(key);
            if (it == owner.end()) owner.emplace(key, i);
            else { const int a = find(i), b = find(it->second); if (a != b) root[std::max(a, b)] = std::min(a, b); }
        }
    }
    std::vector<int> chainOf((size_t) n, -1);
    std::vector<std::vector<int>> members;
    for (int i = 0; i < n; ++i) {                 // (`sorted` is level-major: a chain's members come in dependency order)
        const int r = find(i);
        if (chainOf[r] < 0) { chainOf[r] = (int) members.size(); members.emplace_back(); }
        members[(size_t) chainOf[r]].push_back(i);
    }
    bool ok = true;
    chained.clear();
    chainStart.clear();
    chained.reserve((size_t) n);
    for (const auto& mem : members) {
        chainStart.push_back((int) chained.size());
        const double* last = nullptr;
        std::vector<const void*> written;
        for (size_t m = 0; m < mem.size() && ok; ++m) {
            Op64 q = sorted[(size_t) mem[m]];
            const bool one = !q.c1_tip && q.c1 == (const void*) last, two = !q.c2_tip && q.c2 == (const void*) last;
            if (m == 0) q.pad_ = 0;
            else if (one != two) q.pad_ = one ? 1 : 2;
            else ok = false;                     // not the previous result (or both children are): not a chain
            // (the other child must come from outside this launch, the scale buffer must not be one written earlier in it)
            const void* other = m == 0 ? nullptr : (one ? (q.c2_tip ? nullptr : q.c2) : (q.c1_tip ? nullptr : q.c1));
            for (const void* w : written) ok = ok && w != other && w != (const void*) q.dst && (q.mode != 2 || w != (const void*) q.scale);
            written.push_back(q.dst);
            if (q.mode == 1) written.push_back(q.scale);
            last = q.dst;
            chained.push_back(q);
        }
    }
    chainStart.push_back((int) chained.size());
    return ok;
}
// the launch of a chain list; 1: no instantiation for this tile and category count (the levels take the list)
inline int Engine64::launchChains(const std::vector<Op64>& chained, const std::vector<int>& chainStart)
{
    const int NTr = (S + 15) / 16;
    const size_t ldsBytes = f64_frag_lds_bytes(S, NTr, K);
    void *dt = nullptr, *dc = nullptr;
    int rct = stage(chained.data(), chained.size() * sizeof(Op64), &dt);
    if (rct) return rct;
    rct = stage(chainStart.data(), chainStart.size() * sizeof(int), &dc);
    if (rct) return rct;
    const dim3 cgrid((unsigned) (Ppad / 64), (unsigned) (chainStart.size() - 1));
    const Op64* dto = static_cast<const Op64*>(dt);
    const int* dco = static_cast<const int*>(dc);
#define MBAMD_F64_CHAIN_CASE(NT_, KF_) case NT_ * 8 + KF_: MBAMD_LAUNCH_BARRIER((k64_partials_chain<NT_, KF_>), cgrid, 256, ldsBytes, stream, dto, dco, S, SPAD, Ppad); break
    switch (NTr * 8 + K) {
        MBAMD_F64_CHAIN_CASE(2, 1); MBAMD_F64_CHAIN_CASE(2, 2); MBAMD_F64_CHAIN_CASE(2, 3); MBAMD_F64_CHAIN_CASE(2, 4);
        MBAMD_F64_CHAIN_CASE(3, 1);
        MBAMD_F64_CHAIN_CASE(4, 1);
        default: return 1;
    }
#undef MBAMD_F64_CHAIN_CASE
    levelLaunches++;
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}
// the launches of level l of a list whose descriptors are at dops
inline void Engine64::launchLevel(const LevelList& list, const Op64* dops, int l)
{
    const std::vector<Op64>& sorted = list.ops;
    const std::vector<int>& tipsOf = list.tipsOf;
    const int first = list.start[l], cnt = list.start[(size_t) l + 1] - first;
    if (cnt <= 0) return;
    levelLaunches++;
    const bool fused = K == 4 && IB == 4 && S <= IB;
    if (fused) {
        const dim3 grid((unsigned) (Ppad / 64), (unsigned) cnt);
        auto kern = k64_partials_fused<4, 4>;
        MBAMD_LAUNCH(kern, grid, 64, 0, stream, dops + first, S, SPAD, Ppad);
        return;
    }
    if (S >= 16 && S <= 64) {
        const int NTr = (S + 15) / 16;
        const bool fuse = K >= 1 && K <= 4 && NTr * K <= 8;   // all K categories' tiles in registers
        // operations on two compact tips: the gather kernel (fused rescale only, K x ceil(S / 4) <= 32 products per lane)
        const int NSL = (S + 3) / 4 <= 5 ? 5 : (S + 3) / 4 <= 8 ? 8 : 16;
        int ntt = (fuse && NSL * K <= 32 && !sw.f64NoTipsKernel) ? tipsOf[l] : 0;
        const size_t tipsLds = (size_t) 2 * K * S * (SPAD | 1) * sizeof(double);
        if (ntt > 0 && tipsLds <= 65536) {
            const dim3 tgrid((unsigned) ((Ppad + 255) / 256), (unsigned) ntt);
            MBAMD_LAUNCH_BARRIER(k64_partials_tips_lds, tgrid, 256, tipsLds, stream, dops + first, S, SPAD, K, Ppad);
        } else if (ntt > 0) {
            const dim3 tgrid((unsigned) (Ppad / 16), (unsigned) ntt);
#define MBAMD_F64_TIPS_CASE(NSL_, KF_) case NSL_ * 8 + KF_: MBAMD_LAUNCH_BARRIER((k64_partials_tips<NSL_, KF_>), tgrid, 64, 0, stream, dops + first, S, SPAD, Ppad); break
            // (both matrices beyond 64 KiB, K S (SPAD | 1) > 4096: 32 states x 4, 64 states x 1, 33 ... 64 states x 2 -- nothing else gets here)
            switch (NSL * 8 + K) {
                MBAMD_F64_TIPS_CASE(8, 4); MBAMD_F64_TIPS_CASE(16, 1); MBAMD_F64_TIPS_CASE(16, 2);
                default: ntt = 0; break;
            }
#undef MBAMD_F64_TIPS_CASE
        }
        if (ntt == cnt) return;
        const dim3 grid((unsigned) (Ppad / 16), (unsigned) (cnt - ntt), (unsigned) (fuse ? 1 : K));
        // (matrices through LDS, four waves per workgroup, when both fit into 64 KiB)
        const size_t ldsBytes = f64_frag_lds_bytes(S, NTr, fuse ? K : 1);
        // (codon M3 0.90 -> 0.81 ms per evaluation; at 20 states x 4 categories the matrices are 5 KiB each and stay in the L1: 1.19 -> 1.16 ms
        //  with four waves per workgroup since all eight are parked in ONE batch of loads -- a batch per category was 1.38)
        const bool viaLds = NTr >= 2 && ldsBytes <= 65536 && !sw.f64MfmaNoLds;
        // (eight waves per workgroup where that still gives every CU two workgroups; beyond 32 states: with four categories' accumulators
        //  the 128 registers of four waves per SIMD mean spills, 1.55 ms)
        const bool wide = NTr >= 3 && (size_t) ((Ppad + 127) / 128) * (size_t) (cnt - ntt) >= 512;
        const dim3 lgrid((unsigned) (wide ? (Ppad + 127) / 128 : Ppad / 64), (unsigned) (cnt - ntt), (unsigned) (fuse ? 1 : K));
        const Op64* lops = dops + first + ntt;
#define MBAMD_F64_MFMA_CASE(NT_, KF_) case NT_ * 8 + KF_: launchMfma<NT_, KF_>(viaLds, wide, grid, lgrid, ldsBytes, lops); break
        switch (NTr * 8 + (fuse ? K : 0)) {
            MBAMD_F64_MFMA_CASE(1, 0); MBAMD_F64_MFMA_CASE(1, 1); MBAMD_F64_MFMA_CASE(1, 2); MBAMD_F64_MFMA_CASE(1, 3); MBAMD_F64_MFMA_CASE(1, 4);
            MBAMD_F64_MFMA_CASE(2, 0); MBAMD_F64_MFMA_CASE(2, 1); MBAMD_F64_MFMA_CASE(2, 2); MBAMD_F64_MFMA_CASE(2, 3); MBAMD_F64_MFMA_CASE(2, 4);
            MBAMD_F64_MFMA_CASE(3, 0); MBAMD_F64_MFMA_CASE(3, 1); MBAMD_F64_MFMA_CASE(3, 2);
            MBAMD_F64_MFMA_CASE(4, 0); MBAMD_F64_MFMA_CASE(4, 1);
            default: launchMfma<4, 2>(viaLds, wide, grid, lgrid, ldsBytes, lops); break;          // (4 * 8 + 2)
        }
#undef MBAMD_F64_MFMA_CASE
        if (fuse) return;
    } else
    switch (IB) {                                         // (fewer than 16 states)
        case 4: launchPartials<4>(dops + first, cnt); break;
        case 8: launchPartials<8>(dops + first, cnt); break;
        default: launchPartials<16>(dops + first, cnt); break;
    }
    bool anyScale = false;
    for (int i = first; i < first + cnt; ++i) anyScale |= sorted[i].mode != 0;
    if (anyScale)
        MBAMD_LAUNCH(k64_rescale, dim3((unsigned) (Ppad / 64), (unsigned) cnt), 64, 0, stream, dops + first, S, K, Ppad);
}
// The matrix-core level kernel of NT tiles and KF fused categories, in the widest form the level allows: eight waves per workgroup
// with the matrices in LDS (`wide`, NT >= 3), four (`viaLds`, NT >= 2), or one wave reading its matrices itself.  Only what the
// conditions of launchLevel can select is instantiated.
template <int NT, int KF> inline void Engine64::launchMfma(bool viaLds, bool wide, dim3 grid, dim3 lgrid, size_t ldsBytes, const Op64* ops)
{
    if constexpr (NT >= 3)
        if (viaLds && wide) { MBAMD_LAUNCH_BARRIER((k64_partials_mfma_lds<NT, KF, 8>), lgrid, 512, ldsBytes, stream, ops, S, SPAD, Ppad); return; }
    if constexpr (NT >= 2)
        if (viaLds) { MBAMD_LAUNCH_BARRIER((k64_partials_mfma_lds<NT, KF, 4>), lgrid, 256, ldsBytes, stream, ops, S, SPAD, Ppad); return; }
    MBAMD_LAUNCH_BARRIER((k64_partials_mfma<NT, KF>), grid, 64, 0, stream, ops, S, SPAD, Ppad);
}
template <int IB_> inline void Engine64::launchPartials(const Op64* ops, int n)
{
    MBAMD_LAUNCH(k64_partials<IB_>, dim3((unsigned) (Ppad / 64), (unsigned) n, (unsigned) (K * (SPAD / IB_))), 64, 0, stream, ops, S, SPAD, K, Ppad);
}

// ---- scale factors ----
inline int Engine64::accumulateScale(const int* idx, int count, int cumIdx, int sign, int partition)
{
    {   // (between the lists of a codon model's parts MrBayes removes the NEXT part's scale factors from ITS cumulative buffer:
        //  buffers no queued operation touches -- that may run ahead of the queue)
        bool touches = cumIdx >= 0 && cumIdx < (int) queuedScale.size() && queuedScale[cumIdx];
        for (int i = 0; i < count && !touches; ++i) touches = idx[i] >= 0 && idx[i] < (int) queuedScale.size() && queuedScale[idx[i]];
        if (touches || queuedScale.empty()) { const int rcq = flushQueue(); if (rcq) return rcq; }
    }
    if (count <= 0) return BEAGLE_SUCCESS;
    int first = 0, last = Ppad;
    int rcp = partitionRange(partition, &first, &last, "scale factors by partition");
    if (rcp) return rcp;
    if (cumIdx < 0 || cumIdx >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "scale factors: cumulative index");
    std::vector<const int32_t*> src((size_t) count);
    for (int i = 0; i < count; ++i) {
        if (idx[i] < 0 || idx[i] >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "scale factors: index");
        src[i] = d_scale + (size_t) idx[i] * Ppad;
    }
    void* dv = nullptr;
    int rc = stage(src.data(), src.size() * sizeof(const int32_t*), &dv);
    if (rc) return rc;
    MBAMD_LAUNCH(k64_scale_accumulate, (unsigned) ((last - first + 255) / 256), 256, 0, stream, (const int32_t* const*) dv, count, sign, first, last, d_scale + (size_t) cumIdx * Ppad);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}
inline int Engine64::resetScale(int idx, int partition)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleResetScaleFactors: index");
    int first = 0, last = Ppad;
    int rc = partitionRange(partition, &first, &last, "beagleResetScaleFactorsByPartition");
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_scale + (size_t) idx * Ppad + first, 0, (size_t) (last - first) * sizeof(int32_t), stream));
    return BEAGLE_SUCCESS;
}
inline int Engine64::copyScale(int dst, int src)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (dst < 0 || dst >= nScale || src < 0 || src >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCopyScaleFactors: index");
    HIP_TRY(hipMemcpyAsync(d_scale + (size_t) dst * Ppad, d_scale + (size_t) src * Ppad, (size_t) Ppad * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    return BEAGLE_SUCCESS;
}
// the exponents of scale buffer idx, once everything queued has run
inline int Engine64::downloadScale(int idx, const char* what, std::vector<int32_t>& h)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (idx < 0 || idx >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, what);
    h.resize((size_t) Ppad);
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(h.data(), d_scale + (size_t) idx * Ppad, (size_t) Ppad * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}
inline int Engine64::getScaleExponents(int idx, int* out)            // [K][P]: every category row the same
{
    std::vector<int32_t> h;
    { const int rc = downloadScale(idx, "scale factors: index", h); if (rc) return rc; }
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < P; ++c) out[(size_t) k * P + c] = h[c];
    return BEAGLE_SUCCESS;
}
inline int Engine64::getScaleFactors(int idx, double* out)
{
    std::vector<int32_t> h;
    { const int rc = downloadScale(idx, "beagleGetScaleFactors: index", h); if (rc) return rc; }
    for (int c = 0; c < P; ++c) out[c] = h[c] * 0.69314718055994530942;
    return BEAGLE_SUCCESS;
}

// ---- beagleCalculate*LogLikelihoods, derivatives, per-pattern read-outs, beagleWaitForPartials ----
inline int Engine64::logLikelihoods(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx, int count,
                   double* out, const int* partitions, int partitionCount, double* outByPartition)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (count < 1 || count > MBAMD_MAX_SUBSETS) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "log-likelihood: more than 8 subsets");
    const int pc = partitions ? partitionCount : 1;
    if (pc == 1) lastLnl.remember(parent, child, prob, wIdx, fIdx, cumIdx, count);
    const int nblocks = Ppad / 64;
    const size_t nsums = (size_t) nblocks * pc;
    { const int rc = grow_pinned(stream, (void**) &h_sums, &hSumsCap, nsums * sizeof(double), nsums * sizeof(double)); if (rc) return rc; }
    { const int rc = grow_device(stream, (void**) &d_sums, &sumsCap, nsums * sizeof(double), nsums * sizeof(double)); if (rc) return rc; }
    double* const h = h_sums;
    std::vector<int> blocksOf((size_t) pc);
    for (int d = 0; d < pc; ++d) {
        int first = 0, last = P;
        if (partitions) {
            int rc = partitionRange(partitions[d], &first, &last, "log-likelihood by partition");
            if (rc) return rc;
            last = std::min(last, P);
        }
        IntegrateArgs64 a;
        std::memset(&a, 0, sizeof a);
        a.count = count;
        for (int n = 0; n < count; ++n) {
            const int j = n * pc + d;
            if (parent[j] < 0 || parent[j] >= nBuffers || !valid[parent[j]] || isTip[parent[j]])
                return fail(BEAGLE_ERROR_OUT_OF_RANGE, "log-likelihood: parent buffer");
            a.parent[n] = partialsPtr(parent[j]);
            if (child) {
                const int ci = child[j];
                if (ci < 0 || ci >= nBuffers || !valid[ci] || prob[j] < 0 || prob[j] >= nMatrices)
                    return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge log-likelihood: child buffer / matrix");
                a.child[n] = isTip[ci] ? (const void*) statesPtr(ci) : (const void*) partialsPtr(ci);
                a.child_tip[n] = (uint8_t) isTip[ci];
                a.matrix[n] = matrixPtr(prob[j]);
            }
            if (wIdx[j] < 0 || wIdx[j] >= nEigen || fIdx[j] < 0 || fIdx[j] >= nEigen)
                return fail(BEAGLE_ERROR_OUT_OF_RANGE, "log-likelihood: weights / frequencies index");
            a.weights[n] = d_weights + (size_t) wIdx[j] * K;
            a.freqs[n] = d_freqs + (size_t) fIdx[j] * S;
            if (cumIdx && cumIdx[j] != BEAGLE_OP_NONE) {
                if (cumIdx[j] < 0 || cumIdx[j] >= nScale) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "log-likelihood: cumulative scale index");
                a.cum[n] = d_scale + (size_t) cumIdx[j] * Ppad;
            }
        }
        blocksOf[d] = (last + 63) / 64 - first / 64;
        if (blocksOf[d] <= 0) continue;
        if (S >= 16)
            MBAMD_LAUNCH_BARRIER(k64_integrate_wide, (unsigned) blocksOf[d], 512, (size_t) a.count * 8 * 64 * sizeof(double), stream, a, S, K, first, last, Ppad, (const double*) d_pweights, d_site,
                                 d_sums + (size_t) d * nblocks);
        else
            MBAMD_LAUNCH(k64_integrate, (unsigned) blocksOf[d], 64, 0, stream, a, S, K, first, last, Ppad, (const double*) d_pweights, d_site,
                         d_sums + (size_t) d * nblocks);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, d_sums, nsums * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    double total = 0.0;
    for (int d = 0; d < pc; ++d) {
        double s = 0.0;
        for (int i = 0; i < blocksOf[d]; ++i) s += h[(size_t) d * nblocks + i];
        if (outByPartition) outByPartition[d] = s;
        total += s;
    }
    haveSite = true;
    derivValid = false;
    if (out) *out = total;
    if (!(total == total) || total > 1.79e308 || total < -1.79e308) return BEAGLE_ERROR_FLOATING_POINT;
    return BEAGLE_SUCCESS;
}
inline int Engine64::edgeDerivatives(const int* parent, const int* child, const int* prob, const int* d1, const int* d2, const int* wIdx, const int* fIdx,
                    const int* cumIdx, const int* partitions, int partitionCount, double* sums)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    const int pc = partitions ? partitionCount : 1;
    if (pc == 1) lastLnl.remember(parent, child, prob, wIdx, fIdx, cumIdx, 1);
    const int nblocks = Ppad / 64;
    const size_t nsite = (size_t) 3 * Ppad, nsums = (size_t) pc * 3 * nblocks;
    { const int rc = grow_device(stream, (void**) &d_deriv, &derivCap, (nsite + nsums) * sizeof(double), (nsite + nsums) * sizeof(double)); if (rc) return rc; }
    std::vector<int> blocksOf((size_t) pc, 0);
    for (int d = 0; d < pc; ++d) {
        int first = 0, last = P;
        if (partitions) {
            int rc = partitionRange(partitions[d], &first, &last, "edge derivatives by partition");
            if (rc) return rc;
            last = std::min(last, P);
        }
        if (parent[d] < 0 || parent[d] >= nBuffers || !valid[parent[d]] || isTip[parent[d]])
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge derivatives: parent buffer");
        const int ci = child[d];
        if (ci < 0 || ci >= nBuffers || !valid[ci] || prob[d] < 0 || prob[d] >= nMatrices || d1[d] < 0 || d1[d] >= nMatrices ||
            (d2 && (d2[d] < 0 || d2[d] >= nMatrices)))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge derivatives: child buffer / matrix");
        if (wIdx[d] < 0 || wIdx[d] >= nEigen || fIdx[d] < 0 || fIdx[d] >= nEigen)
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge derivatives: weights / frequencies index");
        if (cumIdx && cumIdx[d] != BEAGLE_OP_NONE && (cumIdx[d] < 0 || cumIdx[d] >= nScale))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "edge derivatives: cumulative scale index");
        DerivArgs a;
        std::memset(&a, 0, sizeof a);
        a.parent = partialsPtr(parent[d]);
        a.child = isTip[ci] ? (const void*) statesPtr(ci) : (const void*) partialsPtr(ci);
        a.child_tip = isTip[ci] ? 1 : 0;
        a.matrix[0] = matrixPtr(prob[d]);
        a.matrix[1] = matrixPtr(d1[d]);
        a.matrix[2] = d2 ? matrixPtr(d2[d]) : nullptr;
        a.weights = d_weights + (size_t) wIdx[d] * K;
        a.freqs = d_freqs + (size_t) fIdx[d] * S;
        if (cumIdx && cumIdx[d] != BEAGLE_OP_NONE) a.cum = d_scale + (size_t) cumIdx[d] * Ppad;
        a.pattern_weights = d_pweights;
        a.site = d_deriv;
        a.sums = d_deriv + nsite + (size_t) d * 3 * nblocks;
        a.S = S; a.SP = S; a.K = K; a.Ppad = Ppad;
        a.first = first; a.last = last;
        a.sumStride = nblocks;
        blocksOf[d] = (last + 63) / 64 - first / 64;
        if (blocksOf[d] <= 0) continue;
        auto kernel = k_edge_derivatives<DERIV_F64, double>;
        MBAMD_LAUNCH(kernel, (unsigned) blocksOf[d], 64, 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    derivSite.resize(nsite + nsums);
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(derivSite.data(), d_deriv, (nsite + nsums) * sizeof(double), hipMemcpyDeviceToHost));
    bool finite = true;
    for (int d = 0; d < pc; ++d)
        for (int q = 0; q < 3; ++q) {
            double t = 0.0;
            for (int i = 0; i < blocksOf[d]; ++i) t += derivSite[nsite + ((size_t) d * 3 + q) * nblocks + i];
            sums[d * 3 + q] = t;
            if (q == 0 && (!(t == t) || t > 1.79e308 || t < -1.79e308)) finite = false;
        }
    haveSite = true;
    derivValid = true;
    return finite ? BEAGLE_SUCCESS : BEAGLE_ERROR_FLOATING_POINT;
}
// ---- the pre-order pass, the gradient in all branch lengths and the cross products: the bodies are shared with the single-precision
// engine (mbamd_preorder.h, mbamd_crossproducts.h); here the plain kernels run in double precision ----
inline DerivArgs Engine64::layoutArgs() const
{
    DerivArgs a;
    std::memset(&a, 0, sizeof a);
    a.S = S; a.SP = S; a.K = K; a.Ppad = Ppad;
    a.first = 0; a.last = P;
    return a;
}
inline int Engine64::updatePrePartials(const BeagleOperation* ops, int n, int cumIdx) { return update_pre_partials(*this, ops, n, cumIdx); }
inline int Engine64::edgeReadout(const int* post, const int* pre, const int* dmat1, const int* dmat2, const int* wIdx, int count, double* sites1,
                                 double* sites2, double* sums1, double* sums2)
{
    return edge_readout(*this, post, pre, dmat1, dmat2, wIdx, count, sites1, sites2, (size_t) P, sums1, sums2);
}
inline int Engine64::crossProducts(const int* post, const int* pre, const int* rateIdx, const int* wIdx, const double* lengths, int count, double* out)
{
    return cross_products(*this, post, pre, rateIdx, wIdx, lengths, count, out);
}
inline int Engine64::nodePosteriors(const int* post, const int* pre, const int* wIdx, int count, double* sites, int* bestStates, double* bestValues,
                                    double* sums)
{
    return node_posteriors(*this, post, pre, wIdx, count, sites, bestStates, bestValues, (size_t) P, sums);
}
inline int Engine64::categoryPosteriors(int wIdx, double* out) { return category_posteriors(*this, wIdx, out, (size_t) P); }
inline int Engine64::insertionLogLikelihoods(const int* pre, const int* post, const int* postM, const int* sub, const int* subM, const int* subScale,
                                             const int* wIdx, int count, double* sites, double* sums)
{
    return insertion_log_likelihoods(*this, pre, post, postM, sub, subM, subScale, wIdx, count, sites, (size_t) P, sums);
}
inline int Engine64::siteModelDerivatives(const int* post, const int* pre, const int* dmat, const int* wIdx, int count, double* edgeCat,
                                          double* counts, double* rootFreq)
{
    return site_model_derivatives(*this, post, pre, dmat, wIdx, count, edgeCat, counts, rootFreq);
}
inline int Engine64::sampleAncestralStates(const int* parentSlots, const int* post, const int* matrices, int count, int wIdx, unsigned long long seed,
                                           long long patternOffset, int* states, int* categories, double* changes, size_t stride)
{
    return sample_ancestral_states(*this, parentSlots, post, matrices, count, wIdx, seed, patternOffset, states, categories, changes, stride);
}
// what ensure_posteriors asks for: the latest log-likelihood call's operands, checked, and room for q
inline int Engine64::posteriorOperands(DerivArgs& a)
{
    const LnlOperands& l = lastLnl;
    if (l.parent < 0 || l.parent >= nBuffers || !valid[l.parent] || isTip[l.parent] || l.weights < 0 || l.weights >= nEigen || l.freqs < 0 || l.freqs >= nEigen ||
        (l.child >= 0 && (l.child >= nBuffers || !valid[l.child] || l.prob < 0 || l.prob >= nMatrices)) || (l.cum != BEAGLE_OP_NONE && (l.cum < 0 || l.cum >= nScale)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleCalculateEdgeDerivatives: the operands of the latest log-likelihood call");
    { const int rc = grow_device(stream, (void**) &d_q, &qCap, (size_t) K * Ppad * sizeof(double), (size_t) K * Ppad * sizeof(double)); if (rc) return rc; }
    a = layoutArgs();
    a.parent = partialsPtr(l.parent);
    if (l.child >= 0) {
        a.child_tip = isTip[l.child] ? 1 : 0;
        a.child = operandPtr(l.child);
        a.matrix[0] = matrixPtr(l.prob);
    }
    a.weights = d_weights + (size_t) l.weights * K;
    a.freqs = d_freqs + (size_t) l.freqs * S;
    if (l.cum != BEAGLE_OP_NONE) a.cum = d_scale + (size_t) l.cum * Ppad;
    return BEAGLE_SUCCESS;
}
inline int Engine64::getSites(double* out)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    if (!haveSite) return fail(BEAGLE_ERROR_GENERAL, "beagleGetSiteLogLikelihoods: no log-likelihood was calculated");
    if (derivValid) { std::memcpy(out, derivSite.data(), (size_t) P * sizeof(double)); return BEAGLE_SUCCESS; }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(out, d_site, (size_t) P * sizeof(double), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}
inline int Engine64::synchronize()
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    HIP_TRY(hipStreamSynchronize(stream));
    return BEAGLE_SUCCESS;
}

// ---- what mbamdGetKernelTiming and beagleCreateInstance's return info read ----
inline int Engine64::kernelTiming(double* ms, long* launches, int reset)
{
    { const int rcq = flushQueue(); if (rcq) return rcq; }
    *ms += 0.0;
    *launches += (long) (walkLaunches + levelLaunches + preLaunches);
    if (reset) walkLaunches = levelLaunches = preLaunches = 0;
    return BEAGLE_SUCCESS;
}
inline const char* Engine64::implName() const
{
    return S == 4 ? MBAMD_IMPL_NAME ": double-precision kernels (four states: tree walk)" : MBAMD_IMPL_NAME ": double-precision level kernels";
}

}  // namespace mbamd
#endif
