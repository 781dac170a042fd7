/*
 * libhmsbeagle/beagle.h -- C ABI of the MI355X-native conditional-likelihood engine.
 *
 * This is the drop-in boundary: MrBayes' own adapter, reference
 * src/mbbeagle.c + src/likelihood.c + src/mcmc.c, includes "libhmsbeagle/beagle.h"
 * (reference src/bayes.h:62-64) and calls the functions declared here; building the
 * unmodified reference with -DBEAGLE_ENABLED against this header and linking
 * mrbayes_amd/libhmsbeagle.so makes `set usebeagle=yes` run on the HIP engine.
 *
 * The upstream header (beagle-dev/beagle-lib, "release 3.1.2 ... also 2.1.3", reference
 * INSTALL:199-201) is not vendored in the reference tree, so this file is authored from the
 * reference's call sites (cited per declaration) and the published BEAGLE API (Ayres et al.
 * 2012/2019); numeric constant values follow the published API so existing clients keep working.
 *
 * Every pointer argument is caller-owned host memory, read (or written) during the call; no
 * device or framework types appear in any signature.  All calls on one instance must come from
 * one host thread at a time (MrBayes is single-threaded, reference src/mcmc.c:16718).
 *
 * Conventions:  partials [category][pattern][state], transition matrices [category][from][to]
 * (row-major), eigenvectors row-major S x S, all double at the boundary; single precision inside.
 */
#ifndef MBAMD_LIBHMSBEAGLE_BEAGLE_H_
#define MBAMD_LIBHMSBEAGLE_BEAGLE_H_

#ifdef __cplusplus
extern "C" {
#endif

#define BEAGLE_DLLEXPORT __attribute__((visibility("default")))

/* return codes (reference use: src/mbbeagle.c:471,1283,1291) */
enum BeagleReturnCodes {
    BEAGLE_SUCCESS                      =  0,
    BEAGLE_ERROR_GENERAL                = -1,
    BEAGLE_ERROR_OUT_OF_MEMORY          = -2,
    BEAGLE_ERROR_UNIDENTIFIED_EXCEPTION = -3,
    BEAGLE_ERROR_UNINITIALIZED_INSTANCE = -4,
    BEAGLE_ERROR_OUT_OF_RANGE           = -5,
    BEAGLE_ERROR_NO_RESOURCE            = -6,
    BEAGLE_ERROR_NO_IMPLEMENTATION      = -7,
    BEAGLE_ERROR_FLOATING_POINT         = -8
};

/* capability / preference / requirement flags (reference use: src/mbbeagle.c:685-753,
 * src/command.c:6637-7090, src/bayes.c:608-640) */
enum BeagleFlags {
    BEAGLE_FLAG_PRECISION_SINGLE    = 1 << 0,   /* the tuned engines (fp32 conditional likelihoods, fp64 sums and logs) */
    BEAGLE_FLAG_PRECISION_DOUBLE    = 1 << 1,   /* required, or preferred without SINGLE (`set beagleprecision=double`): the fp64 engine */
    BEAGLE_FLAG_COMPUTATION_SYNCH   = 1 << 2,
    BEAGLE_FLAG_COMPUTATION_ASYNCH  = 1 << 3,
    BEAGLE_FLAG_EIGEN_REAL          = 1 << 4,
    BEAGLE_FLAG_EIGEN_COMPLEX       = 1 << 5,
    BEAGLE_FLAG_SCALING_MANUAL      = 1 << 6,
    BEAGLE_FLAG_SCALING_AUTO        = 1 << 7,
    BEAGLE_FLAG_SCALING_ALWAYS      = 1 << 8,
    BEAGLE_FLAG_SCALERS_RAW         = 1 << 9,
    BEAGLE_FLAG_SCALERS_LOG         = 1 << 10,
    BEAGLE_FLAG_VECTOR_SSE          = 1 << 11,
    BEAGLE_FLAG_VECTOR_NONE         = 1 << 12,
    BEAGLE_FLAG_THREADING_OPENMP    = 1 << 13,
    BEAGLE_FLAG_THREADING_NONE      = 1 << 14,
    BEAGLE_FLAG_PROCESSOR_CPU       = 1 << 15,
    BEAGLE_FLAG_PROCESSOR_GPU       = 1 << 16,
    BEAGLE_FLAG_PROCESSOR_FPGA      = 1 << 17,
    BEAGLE_FLAG_PROCESSOR_CELL      = 1 << 18,
    BEAGLE_FLAG_PROCESSOR_PHI       = 1 << 19,
    BEAGLE_FLAG_INVEVEC_STANDARD    = 1 << 20,
    BEAGLE_FLAG_INVEVEC_TRANSPOSED  = 1 << 21,
    BEAGLE_FLAG_FRAMEWORK_CUDA      = 1 << 22,
    BEAGLE_FLAG_FRAMEWORK_OPENCL    = 1 << 23,
    BEAGLE_FLAG_VECTOR_AVX          = 1 << 24,
    BEAGLE_FLAG_SCALING_DYNAMIC     = 1 << 25,
    BEAGLE_FLAG_PROCESSOR_OTHER     = 1 << 26,
    BEAGLE_FLAG_FRAMEWORK_CPU       = 1 << 27,
    BEAGLE_FLAG_PARALLELOPS_STREAMS = 1 << 28,
    BEAGLE_FLAG_PARALLELOPS_GRID    = 1 << 29,
    BEAGLE_FLAG_THREADING_CPP       = 1 << 30
};
/* this engine: native HIP on AMD CDNA; reported in BeagleInstanceDetails.flags next to
   PROCESSOR_GPU.  Deliberately NOT FRAMEWORK_CUDA/OPENCL (those switch MrBayes' v3 build to
   level-order operation lists, reference src/mbbeagle.c:363-381; the engine levels ops itself). */
#define BEAGLE_FLAG_FRAMEWORK_HIP (1L << 31)

/* benchmarking hints of the v3 resource benchmark (reference src/mbbeagle.c:220-228) */
enum BeagleBenchmarkFlags {
    BEAGLE_BENCHFLAG_SCALING_NONE    = 1 << 0,
    BEAGLE_BENCHFLAG_SCALING_ALWAYS  = 1 << 1,
    BEAGLE_BENCHFLAG_SCALING_DYNAMIC = 1 << 2
};

enum BeagleOpCodes {
    BEAGLE_OP_COUNT           = 7,   /* ints per BeagleOperation */
    BEAGLE_PARTITION_OP_COUNT = 9,   /* ints per BeagleOperationByPartition */
    BEAGLE_OP_NONE            = -1   /* "no buffer" sentinel (reference src/mbbeagle.c:834-860) */
};

/* filled by beagleCreateInstance (reference src/mbbeagle.c:178, 329-356) */
typedef struct {
    int   resourceNumber;
    char* resourceName;
    char* implName;
    char* implDescription;
    long  flags;
} BeagleInstanceDetails;

/* one entry of beagleGetResourceList (reference src/mbbeagle.c:609-660) */
typedef struct {
    char* name;
    char* description;
    long  supportFlags;
    long  requiredFlags;
} BeagleResource;

typedef struct {
    BeagleResource* list;
    int             length;
} BeagleResourceList;

/* v3 benchmark list (reference src/mbbeagle.c:231-307) */
typedef struct {
    int    number;
    char*  name;
    char*  description;
    long   supportFlags;
    long   requiredFlags;
    int    returnCode;
    char*  implName;
    long   benchedFlags;
    double benchmarkResult;
    double performanceRatio;
} BeagleBenchmarkedResource;

typedef struct {
    BeagleBenchmarkedResource* list;
    int                        length;
} BeagleBenchmarkedResourceList;

/* one partial-likelihood update (reference src/mbbeagle.c:817-846, 919-947, 1042-1075):
 *   dest[k,c,i] = (sum_j P1_k[i,j] child1[k,c,j]) * (sum_j P2_k[i,j] child2[k,c,j])
 * destinationScaleWrite >= 0: rescale dest per pattern, store the factors in that scale buffer and,
 *   if updatePartials' cumulativeScaleIndex >= 0, add their logs to that cumulative buffer;
 * destinationScaleRead  >= 0: divide dest by the factors already stored in that buffer. */
typedef struct {
    int destinationPartials;
    int destinationScaleWrite;
    int destinationScaleRead;
    int child1Partials;
    int child1TransitionMatrix;
    int child2Partials;
    int child2TransitionMatrix;
} BeagleOperation;

/* v3 multi-partition form (reference src/mbbeagle.c:2292) */
typedef struct {
    int destinationPartials;
    int destinationScaleWrite;
    int destinationScaleRead;
    int child1Partials;
    int child1TransitionMatrix;
    int child2Partials;
    int child2TransitionMatrix;
    int partition;
    int cumulativeScaleIndex;
} BeagleOperationByPartition;

/* ---------------------------------------------------------------------------------------------
 * library-level queries
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:345,350,659 */
BEAGLE_DLLEXPORT const char* beagleGetVersion(void);
BEAGLE_DLLEXPORT const char* beagleGetCitation(void);
/* reference src/mbbeagle.c:614,645: one resource per visible AMD GPU (supportFlags has
 * PROCESSOR_GPU, which `set beagledevice=gpu` filters on, src/mbbeagle.c:620) */
BEAGLE_DLLEXPORT BeagleResourceList* beagleGetResourceList(void);

/* ---------------------------------------------------------------------------------------------
 * instance life cycle
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:313-326.  Returns instance id >= 0 or a negative BeagleReturnCodes.
 * resourceList == NULL / resourceCount == 0 lets the library choose the device
 * (src/mbbeagle.c:322-323). */
BEAGLE_DLLEXPORT int beagleCreateInstance(int tipCount, int partialsBufferCount, int compactBufferCount,
                                          int stateCount, int patternCount, int eigenBufferCount,
                                          int matrixBufferCount, int categoryCount, int scaleBufferCount,
                                          int* resourceList, int resourceCount,
                                          long preferenceFlags, long requirementFlags,
                                          BeagleInstanceDetails* returnInfo);
/* reference src/mbbeagle.c:340, src/mcmc.c:4602 */
BEAGLE_DLLEXPORT int beagleFinalizeInstance(int instance);
BEAGLE_DLLEXPORT int beagleFinalize(void);

/* ---------------------------------------------------------------------------------------------
 * data upload
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:148: patternCount ints, value >= stateCount = missing/gap */
BEAGLE_DLLEXPORT int beagleSetTipStates(int instance, int tipIndex, const int* inStates);
/* reference src/mbbeagle.c:165: [pattern][state] doubles, replicated over categories */
BEAGLE_DLLEXPORT int beagleSetTipPartials(int instance, int tipIndex, const double* inPartials);
/* [category][pattern][state] doubles */
BEAGLE_DLLEXPORT int beagleSetPartials(int instance, int bufferIndex, const double* inPartials);
/* read a partials buffer back, [category][pattern][state]; scaleIndex must be BEAGLE_OP_NONE */
BEAGLE_DLLEXPORT int beagleGetPartials(int instance, int bufferIndex, int scaleIndex, double* outPartials);
/* reference src/likelihood.c:10652,10752: row-major U, U^-1 (S x S) and S real eigenvalues.
 *
 * COMPLEX INSTANCES (the rate matrices of non-reversible models; not used by MrBayes, which rejects complex eigenvalues).  An
 * instance is complex when BEAGLE_FLAG_EIGEN_COMPLEX is in the requirement flags of beagleCreateInstance, or in the preference
 * flags while BEAGLE_FLAG_EIGEN_REAL is not required; requiring both flags is BEAGLE_ERROR_NO_IMPLEMENTATION.  Its details.flags
 * carry EIGEN_COMPLEX instead of EIGEN_REAL; every other instance is what it always was.  On a complex instance inEigenValues
 * holds 2 * stateCount values: the real parts a_s, then the imaginary parts b_s.  b_s == 0 is a real eigenvalue; b_p != 0 must be
 * the first of an adjacent pair (p, p+1) with a_(p+1) == a_p and b_(p+1) == -b_p; an unpaired or non-finite value is
 * BEAGLE_ERROR_OUT_OF_RANGE.  inEigenVectors = V and inInverseEigenVectors = V^-1 stay real S x S: the real block form of the
 * decomposition (upstream's EigenDecompositionSquare convention), defined by
 *     Q = V D V^-1,   D block-diagonal:  [a_s] for a real s,   [[a_p, b_p], [-b_p, a_p]] for a pair (p, p+1)
 * -- for an eigenvector v of a_p + i b_p, columns p and p+1 of V are Re v and Im v.  beagleUpdateTransitionMatrices[WithMultiple-
 * Models] then gives, with r_k the category rate, mu = r_k (a_p + i b_p), o the derivative order and z = mu^o exp(mu t),
 *     d^o P_k / dt^o = V B V^-1,   B = [Re z] for a real s,   [[Re z, Im z], [-Im z, Re z]] for a pair
 * order 0 clamped at zero, orders 1 and 2 not, a rate of exactly 0.0 giving P' = P'' = 0 exactly; everything else about those
 * calls is unchanged.  mbamdSetRateMatrices[From] stays the reversible solver and leaves zero imaginary parts. */
BEAGLE_DLLEXPORT int beagleSetEigenDecomposition(int instance, int eigenIndex, const double* inEigenVectors,
                                                 const double* inInverseEigenVectors, const double* inEigenValues);
/* reference src/mbbeagle.c:1179 */
BEAGLE_DLLEXPORT int beagleSetStateFrequencies(int instance, int stateFrequenciesIndex, const double* inStateFrequencies);
/* reference src/mbbeagle.c:1201,1210; src/mcmc.c:6289,6293 */
BEAGLE_DLLEXPORT int beagleSetCategoryWeights(int instance, int categoryWeightsIndex, const double* inCategoryWeights);
/* reference src/mbbeagle.c:1409 */
BEAGLE_DLLEXPORT int beagleSetCategoryRates(int instance, const double* inCategoryRates);
/* reference src/mcmc.c:6264, src/mbbeagle.c:1225 */
BEAGLE_DLLEXPORT int beagleSetPatternWeights(int instance, const double* inPatternWeights);

/* ---------------------------------------------------------------------------------------------
 * transition matrices
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:1477-1483: P_k = U diag(exp(lambda * rate_k * t)) U^-1 for each listed
 * branch, negatives clamped to 0 like the native path (src/likelihood.c:9540).  Either derivative index
 * list may be NULL (MrBayes always passes NULL), independently of the other; where given, matrix buffer
 * firstDerivativeIndices[i] takes P'_k = dP_k/dt = U diag(lambda rate_k exp(lambda rate_k t)) U^-1 and
 * secondDerivativeIndices[i] takes P''_k = U diag((lambda rate_k)^2 exp(lambda rate_k t)) U^-1 of branch i.  They
 * are ordinary matrix buffers (read back by beagleGetTransitionMatrix as [category][from][to]) and are not
 * clamped: their entries are legitimately negative.  A derivative index equal to another output of the same
 * call is BEAGLE_ERROR_OUT_OF_RANGE. */
BEAGLE_DLLEXPORT int beagleUpdateTransitionMatrices(int instance, int eigenIndex, const int* probabilityIndices,
                                                    const int* firstDerivativeIndices,
                                                    const int* secondDerivativeIndices,
                                                    const double* edgeLengths, int count);
/* [category][from][to] doubles; paddedValue is ignored */
BEAGLE_DLLEXPORT int beagleSetTransitionMatrix(int instance, int matrixIndex, const double* inMatrix, double paddedValue);
BEAGLE_DLLEXPORT int beagleGetTransitionMatrix(int instance, int matrixIndex, double* outMatrix);

/* Transition matrices made out of transition matrices, on the device (upstream BEAGLE's names and argument order; MrBayes calls
 * none of them).  Common to the three calls: they are asynchronous on the instance's stream, like beagleUpdateTransitionMatrices;
 * count == 0 is a successful no-op; a NULL array, a negative count or an index outside [0, matrixBufferCount) is
 * BEAGLE_ERROR_OUT_OF_RANGE; EVERY entry is checked before any matrix is written, so a refused call leaves all matrices as they
 * were.  A result is an ordinary matrix buffer: every copy the engine keeps of it is written, and nothing tells it from the same
 * values given to beagleSetTransitionMatrix.  On a sharded or multi-partition instance every child engine does the same.
 *
 * beagleConvolveTransitionMatrices: for entry u and every category k
 *     R_k[i,j] = sum_l A_k[i,l] B_k[l,j]     A = firstIndices[u] (the segment on the from-state / parent side), B = secondIndices[u],
 *                                            R = resultIndices[u]; [category][from][to] as beagleGetTransitionMatrix returns them
 * -- the matrix P(t1; Q1) P(t2; Q2) of a branch that crosses a change of rate matrix.  Nothing is clamped: the buffers may hold P'
 * or P''.  The operands are read as stored (fp32 on the single-precision engine, fp64 on the double-precision one), products and
 * sums are formed in double, and ONE rounding goes to the stored type.  Entries take effect in list order: a result may be an
 * operand of a later entry (P1 P2 -> tmp, tmp P3 -> out), and of two entries that write one result the later wins; entries that
 * do not depend on one another run in one launch.  resultIndices[u] equal to firstIndices[u] or secondIndices[u] is
 * BEAGLE_ERROR_OUT_OF_RANGE (no convolution in place, as upstream). */
BEAGLE_DLLEXPORT int beagleConvolveTransitionMatrices(int instance, const int* firstIndices, const int* secondIndices,
                                                      const int* resultIndices, int matrixCount);
/* R_k = A_k^T for every category, exact; A = inputIndices[u], R = resultIndices[u], which may be the same buffer.  List order and
 * launches as for beagleConvolveTransitionMatrices. */
BEAGLE_DLLEXPORT int beagleTransposeTransitionMatrices(int instance, const int* inputIndices, const int* resultIndices, int matrixCount);
/* The batch form of beagleSetTransitionMatrix: inMatrices holds `count` matrices of categoryCount * stateCount * stateCount
 * doubles, matrix u for buffer matrixIndices[u]; paddedValues is ignored, as paddedValue is there (it may be NULL).  The stored
 * values, every copy, are bit-identical to `count` single calls in list order (of an index named twice the later matrix stays);
 * the call makes one host-to-device transfer. */
BEAGLE_DLLEXPORT int beagleSetTransitionMatrices(int instance, const int* matrixIndices, const double* inMatrices,
                                                 const double* paddedValues, int count);

/* ---------------------------------------------------------------------------------------------
 * partial likelihoods and scale factors
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:868, 978, 1100: operations are in dependency order (post-order) */
BEAGLE_DLLEXPORT int beagleUpdatePartials(int instance, const BeagleOperation* operations, int operationCount,
                                          int cumulativeScaleIndex);
BEAGLE_DLLEXPORT int beagleWaitForPartials(int instance, const int* destinationPartials, int destinationPartialsCount);
/* reference src/likelihood.c:8088 / src/mbbeagle.c:1094 / src/mbbeagle.c:419,512,567 */
BEAGLE_DLLEXPORT int beagleAccumulateScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex);
BEAGLE_DLLEXPORT int beagleRemoveScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex);
BEAGLE_DLLEXPORT int beagleResetScaleFactors(int instance, int cumulativeScaleIndex);
BEAGLE_DLLEXPORT int beagleCopyScaleFactors(int instance, int destScalingIndex, int srcScalingIndex);
/* log scale factors of one buffer, patternCount doubles */
BEAGLE_DLLEXPORT int beagleGetScaleFactors(int instance, int srcScalingIndex, double* outScaleFactors);

/* ---------------------------------------------------------------------------------------------
 * log-likelihood integration
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:1251-1257 (rooted trees) */
BEAGLE_DLLEXPORT int beagleCalculateRootLogLikelihoods(int instance, const int* bufferIndices,
                                                       const int* categoryWeightsIndices,
                                                       const int* stateFrequenciesIndices,
                                                       const int* cumulativeScaleIndices, int count,
                                                       double* outSumLogLikelihood);
/* reference src/mbbeagle.c:1262-1274 (unrooted trees: integrate across the root branch).
 * Returns BEAGLE_ERROR_FLOATING_POINT when the sum is NaN or infinite -- the signal MrBayes'
 * dynamic-rescaling state machine reacts to (src/mbbeagle.c:471-535).
 *
 * Branch-length derivatives (upstream BEAGLE's semantics; MrBayes passes NULL throughout): with count == 1,
 * firstDerivativeIndices / secondDerivativeIndices name the matrix buffers holding P' and P'' of the branch
 * (beagleUpdateTransitionMatrices).  Per pattern c, with L_c = sum_k w_k sum_i pi_i parent[k,c,i] sum_j P_k[i,j] child[k,c,j]
 * and D1_c, D2_c the same sums with P' and P'':  d1_c = D1_c / L_c,  d2_c = D2_c / L_c - d1_c^2, and
 *     *outSumFirstDerivative = sum_c weight_c d1_c,   *outSumSecondDerivative = sum_c weight_c d2_c
 * are the first and second derivative of the log-likelihood in the branch length; *outSumLogLikelihood is as without
 * derivatives.  The first derivative alone (second index and output NULL) is allowed; a second derivative without a
 * first, or an index array without its output pointer (or the reverse), is BEAGLE_ERROR_OUT_OF_RANGE; count > 1 with
 * derivatives is BEAGLE_ERROR_NO_IMPLEMENTATION (one subset at a time, as upstream).  A derivative call is synchronous. */
BEAGLE_DLLEXPORT int beagleCalculateEdgeLogLikelihoods(int instance, const int* parentBufferIndices,
                                                       const int* childBufferIndices,
                                                       const int* probabilityIndices,
                                                       const int* firstDerivativeIndices,
                                                       const int* secondDerivativeIndices,
                                                       const int* categoryWeightsIndices,
                                                       const int* stateFrequenciesIndices,
                                                       const int* cumulativeScaleIndices, int count,
                                                       double* outSumLogLikelihood,
                                                       double* outSumFirstDerivative,
                                                       double* outSumSecondDerivative);
/* reference src/mbbeagle.c:1295,1309,1329: per-pattern log-likelihoods of the last Calculate call */
BEAGLE_DLLEXPORT int beagleGetSiteLogLikelihoods(int instance, double* outLogLikelihoods);
/* patternCount unweighted d1_c / d2_c of the last Calculate call, if it computed derivatives (BEAGLE_ERROR_GENERAL
 * otherwise); either pointer may be NULL */
BEAGLE_DLLEXPORT int beagleGetSiteDerivatives(int instance, double* outFirstDerivatives, double* outSecondDerivatives);

/* ---------------------------------------------------------------------------------------------
 * the gradient in all branch lengths: pre-order partials (upstream BEAGLE 4's names and argument order;
 * MrBayes calls none of them).  The order a client follows:
 *   1. the log-likelihood (beagleUpdatePartials ..., beagleCalculate{Root,Edge}LogLikelihoods with count == 1);
 *   2. beagleUpdatePrePartials with the pre-order list of the tree;
 *   3. beagleCalculateEdgeDerivatives over any number of branches -- again after every branch-length change, from step 1.
 * None of the three is served on a multi-partition instance (BEAGLE_ERROR_NO_IMPLEMENTATION).
 * ------------------------------------------------------------------------------------------- */
/* The top-down pass.  An operation computes pre(n), the conditional likelihoods of the REST of the tree at the child end
 * of n's branch, from its parent's:
 *     destinationPartials = pre(n)             child1Partials = pre(parent of n)     child1TransitionMatrix = P of n's branch
 *     child2Partials = post-order partials, or compact tip states, of n's sibling    child2TransitionMatrix = the sibling's P
 *     tmp[k,c,i]   = pre_parent[k,c,i] * sum_j P_sib,k[i,j] post_sib[k,c,j]
 *     pre_n[k,c,j] = sum_i P_n,k[i,j] tmp[k,c,i]                                     (the transpose)
 * so that sum_j pre_n[k,c,j] post_n[k,c,j] is category k's site likelihood at every node.  A missing tip state in the
 * sibling is the factor 1.  child2Partials == BEAGLE_OP_NONE (the one extension) means there is no sibling factor: MrBayes'
 * unrooted trees hang from a tip, so the top interior node's "parent" has a single child; the client supplies that parent's
 * vector, pi_i * tip_root[c,i], with beagleSetPartials (on a rooted tree it supplies pi, as upstream clients do).
 * Operations come in dependency order (top-down); operations that do not depend on one another run in one launch.
 * Every destination column (pattern, category) is renormalised by its own power of two and the exponent is DISCARDED:
 * pre-order buffers are always self-normalised, so destinationScaleWrite, destinationScaleRead and cumulativeScaleIndex must
 * be BEAGLE_OP_NONE (BEAGLE_ERROR_NO_IMPLEMENTATION otherwise), and beagleGetPartials of such a buffer returns columns each
 * scaled by an unspecified power of two.  A buffer stays a pre-order buffer until anything else writes it. */
BEAGLE_DLLEXPORT int beagleUpdatePrePartials(int instance, const BeagleOperation* operations, int operationCount,
                                             int cumulativeScaleIndex);
/* beagleSetTransitionMatrix without paddedValue: nothing is clamped.  For the branch-length gradient the client passes
 * D_k = r_k Q, [category][from][to], r_k the category rates; the P'_k that beagleUpdateTransitionMatrices makes at edge
 * length zero is the same matrix. */
BEAGLE_DLLEXPORT int beagleSetDifferentialMatrix(int instance, int matrixIndex, const double* inMatrix);
/* For edge e = 0 .. count-1, between postBufferIndices[e] (post-order partials or compact tip states of node n) and
 * preBufferIndices[e] (pre(n), written by beagleUpdatePrePartials and by nothing since: BEAGLE_ERROR_OUT_OF_RANGE
 * otherwise), with D = derivativeMatrixIndices[e]:
 *     g_k(c) = (sum_l pre[k,c,l] sum_j D_k[l,j] post[k,c,j]) / (sum_l pre[k,c,l] post[k,c,l])
 *     d_c    = sum_k q_k(c) g_k(c)            the derivative of pattern c's log-likelihood in the branch length
 *     outDerivatives[e * patternCount + c] = d_c (unweighted),   outSumDerivatives[e] = sum_c weight_c d_c,
 *     outSumSquaredDerivatives[e] = sum_c weight_c d_c^2;   each of the three may be NULL.
 * q_k(c) are the posterior category probabilities of pattern c.  They are the same for every branch and are computed, at the
 * first call after a log-likelihood call, from the operands of that latest beagleCalculate{Root,Edge}LogLikelihoods call as
 * they are then.  With more than one category: no such call yet is BEAGLE_ERROR_GENERAL, one with count > 1 is
 * BEAGLE_ERROR_NO_IMPLEMENTATION, and categoryWeightsIndices[e] must be that call's weights index
 * (BEAGLE_ERROR_OUT_OF_RANGE).  The call is synchronous. */
BEAGLE_DLLEXPORT int beagleCalculateEdgeDerivatives(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                                    const int* derivativeMatrixIndices, const int* categoryWeightsIndices,
                                                    int count, double* outDerivatives, double* outSumDerivatives,
                                                    double* outSumSquaredDerivatives);
/* The curvature beside the gradient (an engine extension: upstream has no such call): the first AND the second derivative of
 * every listed branch from one read of its buffers -- what a Newton step over all branch lengths, a Laplace approximation or a
 * diagonal mass matrix asks for.  Edge e = 0 .. count-1 names its buffers exactly as beagleCalculateEdgeDerivatives does;
 * D1 = firstDerivativeMatrixIndices[e] and D2 = secondDerivativeMatrixIndices[e] are differential matrices
 * (beagleSetDifferentialMatrix): for a branch length D1_k = r_k Q and D2_k = r_k^2 Q^2.
 *     den_k    = sum_l pre[k,c,l] post[k,c,l]
 *     g1_k(c)  = (sum_l pre[k,c,l] sum_j D1_k[l,j] post[k,c,j]) / den_k,      g2_k(c) the same with D2_k
 *     d1_c     = sum_k q_k(c) g1_k(c)                      (beagleCalculateEdgeDerivatives' d_c)
 *     d2_c     = sum_k q_k(c) g2_k(c) - d1_c^2             the second derivative of pattern c's log-likelihood
 *     outFirstDerivatives[e * patternCount + c] = d1_c,  outSecondDerivatives[e * patternCount + c] = d2_c (unweighted),
 *     outSumFirstDerivatives[e] = sum_c weight_c d1_c,   outSumSecondDerivatives[e] = sum_c weight_c d2_c;  each of the four may
 *     be NULL.
 * q_k(c) are the posterior category probabilities of beagleCalculateEdgeDerivatives (1 with one category); a category whose den
 * is not positive has underflowed and is skipped in both sums.  A compact tip is its indicator vector; a MISSING state is the
 * vector of ones in den and contributes nothing to either numerator where the layout stores state codes: differential
 * matrices are taken to have zero row sums there, as beagleCalculateEdgeDerivatives takes them.  The rules of
 * beagleCalculateEdgeDerivatives on the latest log-likelihood call, on categoryWeightsIndices, on pre-order buffers, on
 * multi-partition instances (BEAGLE_ERROR_NO_IMPLEMENTATION), on NULL index arrays and on count == 0 hold unchanged; a second
 * matrix index out of range is BEAGLE_ERROR_OUT_OF_RANGE like a first.  A refused call writes nothing.  The call is synchronous. */
BEAGLE_DLLEXPORT int mbamdCalculateEdgeSecondDerivatives(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                                         const int* firstDerivativeMatrixIndices,
                                                         const int* secondDerivativeMatrixIndices, const int* categoryWeightsIndices,
                                                         int count, double* outFirstDerivatives, double* outSecondDerivatives,
                                                         double* outSumFirstDerivatives, double* outSumSecondDerivatives);
/* its read-out launches since the instance was created: out2[0] on the plain kernel, out2[1] on the matrix-core kernel (16 ... 64
 * states in single precision unless MBAMD_CURV_GENERIC is set); one per chunk of edges */
BEAGLE_DLLEXPORT int mbamdGetSecondDerivativeLaunches(int instance, long* out2);

/* Regraft and placement scores (an engine extension: upstream has no such call): what the log-likelihood WOULD be with a subtree
 * attached at each of `count` points of the tree, from one read of the buffers the gradient call reads -- every regraft position
 * of a pruned clade, or every placement of a query sequence on a fixed tree, in one call.  Entry e = 0 .. count-1 names
 *     preBufferIndices[e]       the pre-order buffer AT the insertion point (beagleUpdatePrePartials wrote it)
 *     postBufferIndices[e]      post-order partials or compact tip states of the node below the point
 *     postMatrixIndices[e]      the matrix from the point down to that node; BEAGLE_OP_NONE: the point IS the node
 *     subtreeBufferIndices[e]   post-order partials or compact tip states of the clade / query to attach
 *     subtreeMatrixIndices[e]   the matrix of the pendant branch
 *     subtreeScaleIndices[e]    the cumulative scale buffer of the subtree, or BEAGLE_OP_NONE
 * and for pattern c and category k, with a = pre[k,c,:],
 *     b[m]   = post[k,c,m]                         (postMatrix NONE)    or   sum_j Pb_k[m,j] post[k,c,j]
 *     s[m]   = sum_j Pc_k[m,j] sub[k,c,j]
 *     den_k  = sum_m a[m] b[m]          num_k = sum_m a[m] b[m] s[m]
 *     R_c    = sum_k q_k(c) (num_k / den_k) 2^{x_k(c)}
 *     outSiteLogRatios[e * patternCount + c] = log R_c (unweighted),   outSumLogRatios[e] = sum_c weight_c log R_c;
 * either output may be NULL.  q_k(c) are the posterior category probabilities of beagleCalculateEdgeDerivatives (1 with one
 * category), from the latest log-likelihood call.  x_k(c) is the subtree's cumulative exponent -- what subtreeScaleIndices[e]
 * holds for the pattern (and, where the implementation keeps one per category, for the category) -- plus the power of two the
 * call takes out of the subtree's own column before its first product (exact; an unscaled column may lie anywhere down to the
 * smallest subnormal).  log R_c is the log-likelihood of pattern c on the tree with the subtree attached minus that on the tree
 * without it, to rounding: the powers of two `pre` and `post` carry per (pattern, category) cancel in num_k / den_k, the
 * subtree's does not and comes out exactly.  A category whose den_k is not positive has underflowed and is skipped.  R_c = 0 --
 * the attachment is impossible for that pattern -- gives -infinity there and in the sum; the call still succeeds.  A compact tip
 * in `post` or `sub` is its indicator column; a missing state is the vector of ones (under a matrix: the factor 1) where the
 * implementation stores state codes, the four-state bitplanes add the compatible columns.  An entry's result does not depend
 * on the other entries of the list or on their order.
 *   Insertion at the CHILD END of the branch above node n: pass pre(n), post(n) and postMatrix = BEAGLE_OP_NONE; nothing else
 * is needed.  One call over all branches ranks every regraft position of a pruned clade: the tree without the clade is the one
 * whose log-likelihood and pre-order list were just run.
 *   Insertion ELSEWHERE on the branch: write the pre-order vector at that point with one ordinary pre-order operation into a
 * scratch buffer -- the parent's pre-order buffer, the sibling, and as its own matrix the UPPER part of the branch (all
 * candidates are independent: beagleUpdatePrePartials runs them in one launch) -- and pass the LOWER part of the branch as
 * postMatrix.
 *   Refusals, the same on both engines; a refused call writes nothing.  BEAGLE_ERROR_NO_IMPLEMENTATION: a multi-partition
 * instance, or a latest log-likelihood call over several subsets.  BEAGLE_ERROR_GENERAL: more than one category and no
 * log-likelihood call yet.  BEAGLE_ERROR_OUT_OF_RANGE: a weights index other than that call's, a pre index that no pre-order
 * operation wrote (or that was overwritten since), a post or subtree buffer that holds nothing, a matrix or scale index out of
 * range, a subtree matrix of BEAGLE_OP_NONE, NULL index arrays with count > 0, count < 0.  count == 0 succeeds; with both
 * outputs NULL the call succeeds after the checks.  The call is synchronous. */
BEAGLE_DLLEXPORT int mbamdCalculateInsertionLogLikelihoods(int instance, const int* preBufferIndices, const int* postBufferIndices,
                                                           const int* postMatrixIndices, const int* subtreeBufferIndices,
                                                           const int* subtreeMatrixIndices, const int* subtreeScaleIndices,
                                                           const int* categoryWeightsIndices, int count, double* outSiteLogRatios,
                                                           double* outSumLogRatios);
/* its launches since the instance was created: out2[0] on the plain kernel, out2[1] on the matrix-core kernel (16 ... 64 states
 * in single precision unless MBAMD_INSERT_GENERIC is set); one per chunk of entries */
BEAGLE_DLLEXPORT int mbamdGetInsertionLaunches(int instance, long* out2);

/* The gradient in the rate matrix (upstream's name and argument order): the S x S cross-product matrix a client contracts with
 * dQ / d theta.  Edge e = 0 .. count-1 names postBufferIndices[e] and preBufferIndices[e] exactly as
 * beagleCalculateEdgeDerivatives does (a post-order buffer may hold partials or compact tip states: a tip is its indicator
 * vector, a missing state the vector of ones).  outSumDerivatives holds stateCount * stateCount doubles, row-major [i * S + j],
 * row i the state on the pre-order side ("from"), column j the state on the post-order side ("to"); it is OVERWRITTEN:
 *     den_e,k(c) = sum_l pre_e[k,c,l] post_e[k,c,l]
 *     X[i,j]     = sum_e t_e sum_c weight_c sum_k q_k(c) r_k pre_e[k,c,i] post_e[k,c,j] / den_e,k(c)
 * with t_e = edgeLengths[e], r_k the category rates of categoryRateIndices[e] (beagleSetCategoryRates[WithIndex]), q_k(c) the
 * posterior category probabilities of beagleCalculateEdgeDerivatives (1 with one category) and weight_c the pattern weights.  A
 * category whose den is not positive has underflowed and is skipped.  Every scale factor of either buffer cancels per (pattern,
 * category) -- for operands down to the smallest subnormal: this call, beagleUpdatePrePartials, beagleCalculateEdgeDerivatives,
 * mbamdCalculateEdgeSecondDerivatives and the derivative arguments of beagleCalculateEdgeLogLikelihoods take the own power of two
 * out of every post-order column (exactly) before its first product, so an UNSCALED column of a dynamically rescaling client, at
 * 2^-140 say, is read with the bits it holds and den never flushes for a live column.  All of them are functions of the buffers AS
 * STORED: an unscaled column below 2^-126 holds fewer than 24 bits (three at 2^-146), and a client that wants derivatives of full
 * accuracy that close to underflow must rescale.  This is upstream's quantity: sum_ij X[i,j] M[i,j] is exactly d lnL / d epsilon for Q -> Q + epsilon M whenever M
 * commutes with Q (M = Q gives sum_e t_e d lnL / d t_e), and upstream's approximation otherwise.
 * outSumSquaredDerivatives must be NULL (BEAGLE_ERROR_NO_IMPLEMENTATION otherwise: upstream's implementations do not fill it
 * either); not served on a multi-partition instance (BEAGLE_ERROR_NO_IMPLEMENTATION).  With more than one category the rules of
 * beagleCalculateEdgeDerivatives on the latest log-likelihood call and on categoryWeightsIndices hold.  A pre index that is no
 * pre-order buffer, an invalid post buffer, an unknown rates index, a NULL array, an edge length that is negative or not finite:
 * BEAGLE_ERROR_OUT_OF_RANGE.  count == 0 writes zeros.  The call is synchronous. */
BEAGLE_DLLEXPORT int beagleCalculateCrossProductDerivative(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                                           const int* categoryRateIndices, const int* categoryWeightsIndices,
                                                           const double* edgeLengths, int count, double* outSumDerivatives,
                                                           double* outSumSquaredDerivatives);
/* The gradient in the SITE MODEL (an engine extension: upstream has no such call): the rate of every category, the weight of every
 * category and the direct term of the state frequencies at the root -- the gamma shape, FreeRate's rates and weights, a zero-rate
 * "+I" category, pi -- from the buffers the branch-length gradient reads.  Edge e = 0 .. count-1 names its buffers and its
 * differential matrix D = derivativeMatrixIndices[e] exactly as beagleCalculateEdgeDerivatives does; q_k(c), den, compact tips,
 * missing states, skipped categories and the power of two taken out of post-order columns are those of that call.  With K the
 * category count, S the state count and weight_c the pattern weights:
 *     den_k(c)   = sum_l pre_e[k,c,l] post_e[k,c,l]
 *     g_e,k(c)   = (sum_l pre_e[k,c,l] sum_j D_k[l,j] post_e[k,c,j]) / den_k(c)
 *     outEdgeCategoryDerivatives[e * K + k] = sum_c weight_c q_k(c) g_e,k(c)           (a category with den <= 0 is skipped)
 *     outRateDerivatives[k] = sum_e edgeLengths[e] outEdgeCategoryDerivatives[e * K + k]     (the edges in their order, in double)
 *     outCategoryCounts[k]  = sum_c weight_c q_k(c)                                    the expected number of sites in category k
 *     outRootFrequencyDerivatives[i] = sum_c weight_c sum_k q_k(c) parent[k,c,i] f_k(c,i) / sum_l pi_l parent[k,c,l] f_k(c,l)
 * each of the four may be NULL (all four: BEAGLE_ERROR_OUT_OF_RANGE), and each is the same, bit for bit, whichever others are asked
 * for.  With D_k = Q for every k (UNIT rate) outRateDerivatives[k] is exactly d lnL / d r_k, r_k the rate of category k -- also
 * where r_k = 0, there is no division by a rate; with D_k = r_k Q the sum over k of outEdgeCategoryDerivatives[e * K + k] is
 * beagleCalculateEdgeDerivatives' outSumDerivatives[e].  d lnL / d w_k is outCategoryCounts[k] / w_k, w_k the category weights
 * (one category: q = 1, the count is sum_c weight_c).  In the root term parent, pi and f_k are the operands of the latest
 * beagleCalculate{Root,Edge}LogLikelihoods call as they are now: f_k = 1 for a root call, f_k(c,i) = sum_j P_k[i,j] child[k,c,j]
 * for an edge call; a category whose denominator is not positive is skipped.  It is d lnL / d pi_i at FIXED Q -- the direct
 * term only, the term through Q is beagleCalculateCrossProductDerivative's -- and has no division by pi_i: pi_i = 0 is served.
 * Every scale of every buffer cancels inside its (pattern, category) ratio.  MrBayes' host-side pInvar mixing stays outside, as
 * for the other calls of this family.
 * The rules of beagleCalculateEdgeDerivatives on the latest log-likelihood call, on categoryWeightsIndices, on pre-order buffers,
 * on multi-partition instances (BEAGLE_ERROR_NO_IMPLEMENTATION), on NULL index arrays and on indices out of range hold unchanged,
 * with its statuses.  edgeLengths may be NULL only if outRateDerivatives is; a length that is negative or not finite is
 * BEAGLE_ERROR_OUT_OF_RANGE.  outRootFrequencyDerivatives needs a log-likelihood call even with one category
 * (BEAGLE_ERROR_GENERAL without, as mbamdSampleAncestralStates answers); with one category and that output NULL none is needed.
 * count == 0 is legal: outRateDerivatives is zeros, the counts and the root term are computed.  A refused call writes nothing.
 * The call is synchronous. */
BEAGLE_DLLEXPORT int mbamdCalculateSiteModelDerivatives(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                                        const int* derivativeMatrixIndices, const int* categoryWeightsIndices,
                                                        const double* edgeLengths, int count, double* outEdgeCategoryDerivatives,
                                                        double* outRateDerivatives, double* outCategoryCounts,
                                                        double* outRootFrequencyDerivatives);

/* ---------------------------------------------------------------------------------------------
 * engine extensions (not part of the upstream API; used by bench.py / the multi-GPU driver)
 * ------------------------------------------------------------------------------------------- */
/* Block until all queued device work of the instance has finished. */
/* ---------------------------------------------------------------------------------------------
 * BEAGLE v3 surface (compiled into MrBayes when the library exports beagleSetCPUThreadCount, reference
 * configure.ac:220-223): resource benchmark, multi-partition instances.  A multi-partition instance holds the site
 * patterns of ALL data divisions (same state / category / eigen-part counts); operations, scale-factor bookkeeping and
 * log-likelihood calls name the partition they act on.  In this engine such an instance is a facade over one child engine
 * per partition: the children run on their own streams, only the sums meet on the host.
 * ------------------------------------------------------------------------------------------- */
/* reference src/mbbeagle.c:232-245 */
BEAGLE_DLLEXPORT BeagleBenchmarkedResourceList* beagleGetBenchmarkedResourceList(
    int tipCount, int compactBufferCount, int stateCount, int patternCount, int categoryCount, int* resourceList,
    int resourceCount, long preferenceFlags, long requirementFlags, int eigenModelCount, int partitionCount,
    int calculateDerivatives, long benchmarkFlags);
/* reference src/mbbeagle.c:386 (CPU implementations only; a no-op here) */
BEAGLE_DLLEXPORT int beagleSetCPUThreadCount(int instance, int threadCount);
/* reference src/mcmc.c:6464: patternCount ints, partitions are contiguous increasing pattern ranges; call before the
 * first matrix / partials update (tip data and pattern weights may already be set) */
BEAGLE_DLLEXPORT int beagleSetPatternPartitions(int instance, int partitionCount, const int* inPatternPartitions);
/* reference src/mbbeagle.c:2055 */
BEAGLE_DLLEXPORT int beagleSetCategoryRatesWithIndex(int instance, int categoryRatesIndex, const double* inCategoryRates);
/* reference src/mbbeagle.c:2140-2147; derivative index lists as for beagleUpdateTransitionMatrices */
BEAGLE_DLLEXPORT int beagleUpdateTransitionMatricesWithMultipleModels(int instance, const int* eigenIndices,
                                                                      const int* categoryRateIndices,
                                                                      const int* probabilityIndices,
                                                                      const int* firstDerivativeIndices,
                                                                      const int* secondDerivativeIndices,
                                                                      const double* edgeLengths, int count);
/* reference src/mbbeagle.c:2292, 2440, 2616 */
BEAGLE_DLLEXPORT int beagleUpdatePartialsByPartition(int instance, const BeagleOperationByPartition* operations, int operationCount);
/* reference src/likelihood.c:8096-8103, 8134; src/mbbeagle.c:593, 1736, 1913, 2566 */
BEAGLE_DLLEXPORT int beagleAccumulateScaleFactorsByPartition(int instance, const int* scaleIndices, int count,
                                                             int cumulativeScaleIndex, int partitionIndex);
BEAGLE_DLLEXPORT int beagleRemoveScaleFactorsByPartition(int instance, const int* scaleIndices, int count,
                                                         int cumulativeScaleIndex, int partitionIndex);
BEAGLE_DLLEXPORT int beagleResetScaleFactorsByPartition(int instance, int cumulativeScaleIndex, int partitionIndex);
/* reference src/mbbeagle.c:2817-2850: index arrays are [count][partitionCount]; outSumLogLikelihoodByPartition has one
 * value per named partition */
BEAGLE_DLLEXPORT int beagleCalculateRootLogLikelihoodsByPartition(int instance, const int* bufferIndices,
                                                                  const int* categoryWeightsIndices,
                                                                  const int* stateFrequenciesIndices,
                                                                  const int* cumulativeScaleIndices,
                                                                  const int* partitionIndices, int partitionCount, int count,
                                                                  double* outSumLogLikelihoodByPartition,
                                                                  double* outSumLogLikelihood);
/* derivative arguments as for beagleCalculateEdgeLogLikelihoods, per named partition (count == 1): the ...ByPartition
 * outputs get one value per partition, the plain outputs the totals */
BEAGLE_DLLEXPORT int beagleCalculateEdgeLogLikelihoodsByPartition(
    int instance, const int* parentBufferIndices, const int* childBufferIndices, const int* probabilityIndices,
    const int* firstDerivativeIndices, const int* secondDerivativeIndices, const int* categoryWeightsIndices,
    const int* stateFrequenciesIndices, const int* cumulativeScaleIndices, const int* partitionIndices, int partitionCount,
    int count, double* outSumLogLikelihoodByPartition, double* outSumLogLikelihood, double* outSumFirstDerivativeByPartition,
    double* outSumFirstDerivative, double* outSumSecondDerivativeByPartition, double* outSumSecondDerivative);

/* ---------------------------------------------------------------------------------------------
 * engine extensions (mbamd*)
 * ------------------------------------------------------------------------------------------- */
/* child engines behind an instance: pattern partitions x shards (1: an ordinary instance).  Site patterns of one
 * partition are sharded over several GPUs when beagleCreateInstance names several resources, or MBAMD_SHARD=<g> is set
 * (MrBayes names at most one resource, reference src/mbbeagle.c:322-323). */
BEAGLE_DLLEXPORT int mbamdGetChildCount(int instance);
BEAGLE_DLLEXPORT int mbamdSynchronize(int instance);
/* The binary exponents behind a scale buffer: out[k * patternCount + c].  The 4-state path keeps one exponent per
 * (pattern, category) -- beagleGetScaleFactors reports the largest of a pattern's exponents times ln 2; the general-state
 * path keeps one per pattern (every category row is the same). */
BEAGLE_DLLEXPORT int mbamdGetScaleExponents(int instance, int srcScalingIndex, int* out);
/* Eigen-systems computed ON THE DEVICE (the host step it replaces: UpDateCijk -> GetEigens, reference
 * src/likelihood.c:10476-10804, src/utils.c:11201): `count` reversible rate matrices q (count x S x S doubles, row-major,
 * rows summing to zero; mode 1: symmetric exchangeabilities r_ij instead, Q_ij = r_ij pi_j is built and normalised on the
 * device) with stationary frequencies pi (all positive) -> [U | U^-1 | lambda] of eigen buffers firstEigenIndex ...
 * The unmodified MrBayes does not call it (the BEAGLE API takes finished eigen-systems: beagleSetEigenDecomposition);
 * hosts that own their model code do (mrbayes_amd/likelihood.py, device_eigen=True). */
BEAGLE_DLLEXPORT int mbamdSetRateMatrices(int instance, int firstEigenIndex, int count, const double* q, const double* pi, int mode);
/* The same for a client whose rate matrices change a little from call to call -- an MCMC move on the substitution parameters:
 * warmFirstEigenIndex (>= 0) names the eigen buffers that hold the systems of the state the proposal started from (MrBayes:
 * m->cijkScratchIndex after FlipCijkSpace, reference src/likelihood.c:5614-5622); if the device computed those too, the
 * iteration starts from their eigenvectors and needs two or three sweeps instead of nine.  All `count` systems -- the parts of a
 * codon or covarion model -- in ONE asynchronous launch; nothing waits.
 * mode bit 0: q are exchangeabilities (as mbamdSetRateMatrices); bit 1 (2): shield -- the NEXT beagleSetEigenDecomposition on
 * each of these eigen buffers is ignored, for clients whose own code path still sends its host result afterwards (the binding
 * of reference UpDateCijk, src/likelihood.c:10476-10804: integration/mrbayes/mbamd_eigen_glue.c). */
BEAGLE_DLLEXPORT int mbamdSetRateMatricesFrom(int instance, int firstEigenIndex, int count, const double* q, const double* pi, int mode,
                                              int warmFirstEigenIndex);
/* Transition matrices of ANY rate matrix, with no eigen-system: for every listed branch i and every category k, with r_k the
 * instance's category rate (beagleSetCategoryRates), matrix buffer probabilityIndices[i] takes P_k = exp(Q r_k t_i) and, where the
 * lists are given (either may be NULL, independently), firstDerivativeIndices[i] takes P'_k = r_k Q P_k and
 * secondDerivativeIndices[i] takes P''_k = r_k Q P'_k -- ordinary, unclamped matrix buffers, as beagleUpdateTransitionMatrices
 * fills them.  Computed on the device by uniformization with scaling and squaring: every quantity is non-negative,
 * so no entry of P is negative, structural zeros of P are exact, and defective or non-reversible matrices (absorbing states,
 * one-way chains, complex eigenvalues) are served like any other.  Asynchronous on the instance's stream.  Q travels with the call
 * and is not stored: a client with several rate matrices calls once per matrix.
 *   rateMatrix   S x S doubles, row-major.  Entries finite, off-diagonals >= 0, each diagonal minus its row's off-diagonal sum to
 *                within S 2^-52 of that sum (what summing in double, in any order, can lose); else BEAGLE_ERROR_OUT_OF_RANGE.  The
 *                engine then uses the off-diagonals only and forms the diagonal itself.  A Q of all zeros gives identities and
 *                zero derivatives.
 *   edgeLengths  t_i finite and >= 0, and mu r_k t_i <= 2^20 for every k, mu = max_i sum_{j != i} q_ij; else
 *                BEAGLE_ERROR_OUT_OF_RANGE (as for a category rate that is negative or not finite).  t = 0 or r_k = 0.0 gives
 *                P = I exactly, P' = r_k Q and P'' = r_k^2 Q^2 rounded once -- exact zeros for r_k = 0.0.
 *   indices      BEAGLE_ERROR_OUT_OF_RANGE for an index outside the matrix buffers, for a NULL rateMatrix, probabilityIndices or
 *                edgeLengths with count > 0, for a negative count, and for an output index that occurs twice among the three
 *                lists.  count == 0 is a successful no-op.
 * Everything is checked before anything is written: a refused call changes no matrix.  Served on both engines, on real and complex
 * instances alike (no eigen buffer is read), on 2 ... 64 states, and on pattern-sharded instances (every shard computes its own
 * copy); BEAGLE_ERROR_NO_IMPLEMENTATION on a multi-partition instance (beagleSetPatternPartitions).  The result is an ordinary
 * matrix buffer: every copy the engine keeps is written, and nothing tells it from the same values given to
 * beagleSetTransitionMatrix. */
BEAGLE_DLLEXPORT int mbamdUpdateTransitionMatricesFromRateMatrix(int instance, const double* rateMatrix, const int* probabilityIndices,
                                                                 const int* firstDerivativeIndices, const int* secondDerivativeIndices,
                                                                 const double* edgeLengths, int count);
/* The doubles of an eigen buffer read back (single-precision engine; waits for the instance's stream): outU, outUi S x S each,
 * outLambda S values -- what the matrix kernels read, whoever wrote them.  outV (may be NULL): the S x S orthonormal eigenvectors of
 * the symmetrised matrix that the device solver keeps for warm starts; BEAGLE_ERROR_OUT_OF_RANGE where the buffer was last written by
 * beagleSetEigenDecomposition (it holds no such basis) and for an index out of range.  Made for tests of the solver's accuracy. */
BEAGLE_DLLEXPORT int mbamdGetEigenDecomposition(int instance, int eigenIndex, double* outU, double* outUi, double* outLambda, double* outV);
/* Last HIP/engine error text of the calling thread ("" if none). */
BEAGLE_DLLEXPORT const char* mbamdGetLastError(void);
/* Device-side timing of the partials kernels: accumulates HIP-event time (ms) and launch count of every
 * beagleUpdatePartials since the last reset.  enable=0 turns it off (default). */
BEAGLE_DLLEXPORT int mbamdKernelTiming(int instance, int enable);
BEAGLE_DLLEXPORT int mbamdGetKernelTiming(int instance, double* outMilliseconds, long* outLaunches, int reset);
/* How the 4-state beagleUpdatePartials lists of this instance were run since it was made: out[0] lists, out[1] of them root-ward
 * paths (k_path4), out[2] of those forked (arms that join: the lists of topology moves), out[3] paths run together with the
 * log-likelihood behind them as one launch, out[4] lists compiled for the tree-walk kernel, out[5] their operations.  (Counters for
 * tests and MBAMD_STATS; a facade or a double-precision instance reports zeros.) */
BEAGLE_DLLEXPORT int mbamdGetListCounts(int instance, long* out6);
/* Launches of the 4-state tree-walk kernel since the instance was made: out[0] on its plain instantiations (whole-tree lists:
 * every entry an operation, no prefetch, wait or stored exponent; one wave or several, mbamdGetPlainWaveCounts), out[1] on the generic one.  (As above: for tests;
 * a facade or a double-precision instance reports zeros; a null pointer is BEAGLE_ERROR_OUT_OF_RANGE.) */
BEAGLE_DLLEXPORT int mbamdGetWalkCounts(int instance, long* out2);
/* Queue flushes of the tree-walk layout at 40 and 60 ... 63 states since the instance was made: out[0] on the range-safe instantiations
 * of k_walkg / k_pathg (a list that reads partials of unknown magnitude: set by the client, or written by an operation that did not
 * rescale -- their bf16 pieces are formed from the value times 2^24, exact down to the smallest subnormal), out[1] on the plain ones
 * (every partials operand written by a SCALE_WRITE operation, or a compact tip: always-rescaling clients).  A list on the range-safe
 * ones must keep its partials operands and the factors formed from them below 2^103 (they are scaled by 2^24 on the way).  (For tests; a
 * facade or a double-precision instance reports zeros; a null pointer is BEAGLE_ERROR_OUT_OF_RANGE.) */
BEAGLE_DLLEXPORT int mbamdGetRangeSafeCounts(int instance, long* out2);
/* The launches on the plain instantiations by waves per workgroup: out[W - 1], W = 1 ... 8, launches of plain programs of W waves (a
 * whole-tree list cut over W > 1 waves runs the plain loop on each, values that cross waves travel through LDS; a list that would need
 * an eviction, a prefetch or a stored exponent at that geometry runs on the generic instantiation and is counted there).  (For tests:
 * the sums over the engines behind the instance; a double-precision instance reports zeros; a null pointer is
 * BEAGLE_ERROR_OUT_OF_RANGE.) */
BEAGLE_DLLEXPORT int mbamdGetPlainWaveCounts(int instance, long* out8);
/* Tip pairs (operations on two compact tips) of whole-tree 4-state lists are not stored by the plain tree-walk kernel: the buffer keeps
 * a recipe and is recomputed, bit for bit, before the first call that reads it (MBAMD_STORE_TIP_PAIRS=1 stores everything).  Since the
 * instance was made: out[0] buffers launches left unstored, out[1] buffers materialised since, out[2] launches that materialised them.
 * (For tests: the sums over the engines behind the instance; a double-precision instance reports zeros; a null pointer is
 * BEAGLE_ERROR_OUT_OF_RANGE.) */
BEAGLE_DLLEXPORT int mbamdGetRecomputeCounts(int instance, long* out3);
/* The same three counters for the subtrees of three and four compact tips that such a launch leaves unstored as well
 * (MBAMD_UNSTORED_TIPS=<T>, 2 ... 4: the largest subtree left unstored; 2 = tip pairs only, and zeros here).  mbamdGetRecomputeCounts
 * counts tip pairs only; out[2] here: launches that materialised at least one such subtree.  Same error codes. */
BEAGLE_DLLEXPORT int mbamdGetSubtreeRecomputeCounts(int instance, long* out3);
/* While the timing is on: device time (ms) of whole evaluations -- from the first kernel launched after a
 * Calculate*LogLikelihoods call to the end of the next integration kernel, i.e. every kernel of a step (transition matrices,
 * partials, integration) and the gaps between them -- and how many such spans were closed. */
BEAGLE_DLLEXPORT int mbamdGetStepTiming(int instance, double* outMilliseconds, long* outSteps, int reset);
/* Accepted and ignored (kept for clients that call it): an instance picks its kernel family from its dimensions, and the A/B
 * switches are environment variables.  path outside 0..3: BEAGLE_ERROR_OUT_OF_RANGE, as before. */
BEAGLE_DLLEXPORT int mbamdSetKernelPath(int instance, int path);
/* Calculate*LogLikelihoods without the device->host copy: leaves the sum on the device and returns
 * immediately; mbamdFetchLogLikelihood blocks and returns it (same error convention). */
BEAGLE_DLLEXPORT int mbamdSetDeferredResult(int instance, int enable);
/* timing experiments only: per-step clock stamps of workgroup 0 of the tree-walk kernel (needs MBAMD_WALK_TRACE
 * in the environment when the instance is created); out: [steps][8][3] 64-bit stamps */
BEAGLE_DLLEXPORT int mbamdWalkTrace(int instance, long long* out, int maxSteps, int* outSteps, int* outWaves);
BEAGLE_DLLEXPORT int mbamdFetchLogLikelihood(int instance, double* outSumLogLikelihood);
/* The pending (deferred) sum, added up ON THE DEVICE into *deviceOut (device memory of the instance's GPU) in a fixed order, after
 * the integration that produced it; `waitingStream` (a hipStream_t, may be null) is made to wait for it.  No host synchronisation:
 * a multi-GPU client all-reduces deviceOut over RCCL on its own stream and reads one number per step (bench.py, pattern_sharded).
 * The value stays pending: mbamdFetchLogLikelihood still returns it. */
BEAGLE_DLLEXPORT int mbamdReduceLogLikelihood(int instance, double* deviceOut, void* waitingStream);
/* Which GPUs: the PCI bus id ("0000:c1:00.0") of a resource of beagleGetResourceList, and the resource numbers of the child engines
 * of an instance (a plain instance: one; a sharded one: a device per shard) -- so that a multi-GPU driver can PROVE that its ranks /
 * shards sit on different devices.  mbamdGetInstanceDevices returns the number of children (<= maxCount written). */
BEAGLE_DLLEXPORT int mbamdGetResourcePciBusId(int resource, char* out, int length);
BEAGLE_DLLEXPORT int mbamdGetInstanceDevices(int instance, int* outResources, int maxCount);

#ifdef __cplusplus
}
#endif
#endif /* MBAMD_LIBHMSBEAGLE_BEAGLE_H_ */
