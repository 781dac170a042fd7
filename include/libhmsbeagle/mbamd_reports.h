/*
 * mbamd_reports.h -- engine extension: the final ("up") pass over conditional likelihoods and their scaled read-out.
 *
 * What MrBayes needs when a run reports ancestral states, site rates, positively selected sites or site omegas
 * (`report ancstates / siterates / possel / siteomega`): reference CondLikeUp_Bin / _Gen / _NUC4 (src/likelihood.c:4574-4795)
 * and the inputs of PrintAncStates_*, PrintSiteRates_Gen, PosSelProbs, SiteOmegas (src/mcmc.c:10108-11070, 12212).  The
 * reference switches BEAGLE off for such divisions (src/mcmc.c:5760-5765); with this extension and the binding in
 * integration/mrbayes/mbamd_reports_glue.c ("Reports and covarion") they stay on the engine.
 * SURVEY 8(f) row 3.  Same conventions as beagle.h: plain pointers and sizes in, status codes out.
 */
#ifndef MBAMD_REPORTS_ABI_H_
#define MBAMD_REPORTS_ABI_H_

#include "libhmsbeagle/beagle.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step of the final pass: the "final" conditional likelihoods of a node from those of its ancestor
 * (reference CondLikeUp_*: `clFP` from `clFA`, `clDP`, `tiP`).  All indices are partials / matrix buffer indices of the
 * instance; the destination is any partials buffer the client owns (MrBayes: m->condLikeScratchIndex[node]).
 *   ancestorFinal >= 0 : destination = up-pass of (ancestorFinal, downPartials, transitionMatrix)
 *   ancestorFinal <  0 : the top interior node: destination = downPartials, times -- rootTip >= 0, unrooted trees -- the
 *                        factor of the tip across transitionMatrix (what CondLikeRoot_* includes natively,
 *                        src/likelihood.c:2152-4500; BEAGLE mode integrates that branch at the end instead) */
typedef struct {
    int destinationPartials;
    int ancestorFinal;
    int downPartials;
    int transitionMatrix;
    int rootTip;
} MbamdFinalOperation;

/* Operations run in list order (an ancestor's final partials must be listed before its descendants'). */
BEAGLE_DLLEXPORT int mbamdUpdateFinalPartials(int instance, const MbamdFinalOperation* operations, int operationCount);

/* Read a partials buffer the way the reference's read-outs expect it: outPartials[k][pattern][state] (floats, categories
 * slowest: reference src/likelihood.c:860-876) with all categories of a pattern at ONE common scale, and that scale as the
 * natural-log site scaler outLnScale[pattern] (true value = outPartials * exp(outLnScale); reference `lnScaler`).
 * cumulativeScaleIndex: the cumulative scale buffer of the tree the buffer belongs to (BEAGLE_OP_NONE: unscaled).
 * Final partials of every node, and the top node's, carry exactly the tree's cumulative factor (see csrc/mbamd_reports.h). */
BEAGLE_DLLEXPORT int mbamdGetScaledPartials(int instance, int bufferIndex, int cumulativeScaleIndex, float* outPartials,
                                            float* outLnScale);

/* The same reports from the buffers the gradient calls read, on the single- AND the double-precision engine: the marginal
 * posterior of every state at every listed node, all nodes of a tree in one call.  Node i = 0 .. count-1 names
 * postBufferIndices[i] (its post-order partials, or compact tip states) and preBufferIndices[i] (pre(node), written by
 * beagleUpdatePrePartials and by nothing since) exactly as an edge of beagleCalculateEdgeDerivatives does.  Per pattern c:
 *     j_k(a)  = pre[k,c,a] * post[k,c,a]                     the joint of state a with all the data, in category k
 *     den_k   = sum_a j_k(a)
 *     p_c(a)  = sum_k q_k(c) j_k(a) / den_k                  the posterior of state a at the node
 *     outPosteriors[(i * patternCount + c) * stateCount + a] = p_c(a)                                     (or NULL)
 *     outBestStates[i * patternCount + c]     = the smallest a that attains max_a p_c(a)                  (or NULL)
 *     outBestPosteriors[i * patternCount + c] = that maximum                                              (or NULL)
 *     outSumPosteriors[i * stateCount + a]    = sum_c weight_c p_c(a)      the expected number of sites in state a; never NULL
 * The products are formed in the engine's precision, the sums in double.  Whatever scale a column (pattern, category) of
 * either buffer carries leaves the ratio j_k / den_k: no scale buffer is named -- and this holds for operands down to the
 * smallest subnormal: the own power of two of a post-order column is taken out, exactly, before the first product, here and in
 * mbamdGetCategoryPosteriors (where it joins the category's exponent).  Both calls are functions of the buffers AS STORED: an
 * unscaled column below 2^-126 holds fewer than 24 bits, and a client that wants posteriors of full accuracy that close to
 * underflow must rescale.  q_k(c) are the posterior category
 * probabilities of beagleCalculateEdgeDerivatives (1 with one category: nothing is then asked of a log-likelihood call); a
 * category whose den is not positive has underflowed and is skipped.  A compact tip is its indicator vector, a MISSING state the
 * vector of ones (p_c is then the normalised mixture of the pre-order columns), four-state bitplanes give the compatible
 * states; where exactly one state is compatible p_c is that indicator, exactly 1 and 0.  The sums are reduced on the device in a
 * fixed order and do not depend on which per-pattern outputs are asked for.  The rules of beagleCalculateEdgeDerivatives on the
 * latest log-likelihood call, on categoryWeightsIndices, on pre-order and post-order buffers, on multi-partition instances
 * (BEAGLE_ERROR_NO_IMPLEMENTATION), on NULL index arrays and on count == 0 hold unchanged; a NULL outSumPosteriors is
 * BEAGLE_ERROR_OUT_OF_RANGE.  A refused call writes nothing.  The call is synchronous. */
BEAGLE_DLLEXPORT int mbamdCalculateNodePosteriors(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                                  const int* categoryWeightsIndices, int count, double* outPosteriors,
                                                  int* outBestStates, double* outBestPosteriors, double* outSumPosteriors);

/* q_k(c), the posterior probability of rate category k at pattern c under the operands of the latest
 * beagleCalculate{Root,Edge}LogLikelihoods call as they are now: outPosteriors[k * patternCount + c].  From them come the site
 * rates (sum_k q_k(c) r_k) and, where the categories are omega classes, the positive-selection probabilities and site omegas.
 * One category: ones.  With more: no log-likelihood call yet is BEAGLE_ERROR_GENERAL, one with count > 1
 * BEAGLE_ERROR_NO_IMPLEMENTATION, and categoryWeightsIndex must be that call's weights index (BEAGLE_ERROR_OUT_OF_RANGE).  Not on
 * a multi-partition instance (BEAGLE_ERROR_NO_IMPLEMENTATION).  The call is synchronous. */
BEAGLE_DLLEXPORT int mbamdGetCategoryPosteriors(int instance, int categoryWeightsIndex, double* outPosteriors);

/* One draw of ALL ancestral states from their JOINT posterior given the data, on the single- AND the double-precision engine: what
 * a stochastic character map, a count of substitutions per branch, a posterior-predictive check or a data-augmentation move starts
 * from.  (The posteriors above are marginal: the best states of two adjacent nodes can be jointly impossible.)  Only post-order
 * buffers and transition matrices are read: no pre-order pass is needed.
 *
 * Slots.  Slot 0 is the TOP: the parent buffer of the latest beagleCalculate{Root,Edge}LogLikelihoods call.  Slot i + 1 is the
 * lower end of edge i = 0 .. count-1, which hangs from slot parentSlots[i], 0 <= parentSlots[i] <= i (anything else:
 * BEAGLE_ERROR_OUT_OF_RANGE) -- a parent is listed before its children by construction.  postBufferIndices[i] is the child's
 * post-order partials or its compact tip states, matrixIndices[i] the transition matrix of its branch.  Where the latest
 * log-likelihood call was an edge call, its child (MrBayes' root tip) may be listed as an ordinary edge from slot 0 with that call's
 * matrix.  Edges are launched in groups of consecutive edges whose parent slots all lie before the group's first slot (at most
 * 32768 each): a breadth-first list costs one launch per level of the tree, a depth-first list up to one per edge; the draw is the
 * same.
 *
 * Distribution.  Per pattern c, with k* the drawn category:
 *     P(k)                    = q_k(c)                                   the doubles mbamdGetCategoryPosteriors returns; one
 *                                                                        category: k* = 0 and nothing is drawn
 *     P(a at the top | k)     ~ freqs[a] * parent[k,c,a] * f_k(a)        f_k(a) = sum_j P_k[a,j] child[k,c,j], the factor of the
 *                                                                        log-likelihood call's child across its matrix (a root
 *                                                                        call: f = 1); freqs: that call's state frequencies
 *     P(b at a child | a, k)  ~ P_k[a,b] * post_child[k,c,b]             a = the state drawn at its parent slot
 * A compact tip contributes its indicator: exactly one compatible state is that state, WITHOUT arithmetic; a missing state leaves
 * the row P_k[a,.]; four-state bitplanes leave the compatible columns.
 *
 * Arithmetic.  Each weight is ONE product in the engine's precision (the top's: (parent * f) in the engine's precision, f an
 * ascending FMA chain, times freqs[a] in double), widened to double; sums are in double, in ascending state order.
 *
 * Selection rule.  With the weights v_0 .. v_{n-1} and T their ascending sum: unless T > 0 the answer is -1.  Otherwise x = u * T
 * and the answer is the smallest index with x < v_0 + ... + v_index (the same running sum); if rounding leaves none, the largest
 * index of positive weight.  A state of weight 0 is never chosen.  A slot whose parent slot holds -1, and every slot of a pattern
 * whose category is -1, is -1.
 *
 * Uniforms: counter-based, so that a client can reproduce a draw.  All arithmetic mod 2^64:
 *     mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *     G = 0x9E3779B97F4A7C15
 *     u(seed, stream, c) = (mix(mix(seed + G * (stream + 1)) + G * (c + 1)) >> 11) * 2^-53
 * Stream 0 draws the category, stream 1 the top, stream 2 + i edge i; c is the pattern's index IN THE INSTANCE: a pattern-sharded
 * instance returns the draw of an unsharded one.
 *
 * Outputs.
 *     outStates[slot * patternCount + c]     count + 1 rows; never NULL
 *     outCategories[c]                       k* (or NULL)
 *     outChangeCounts[i] = sum_c weight_c [state(child) != state(parent), both >= 0]      the sampled number of substitutions on
 *                                            branch i (or NULL); reduced on the device in a fixed order, summed over pattern
 *                                            shards in pattern order
 *
 * Refusals.  Not on a multi-partition instance (BEAGLE_ERROR_NO_IMPLEMENTATION).  No log-likelihood call yet is
 * BEAGLE_ERROR_GENERAL -- with one category too: the top's frequencies come from it --, one with count > 1
 * BEAGLE_ERROR_NO_IMPLEMENTATION; categoryWeightsIndex must be that call's weights index, every post buffer readable, every matrix
 * index in range, no index array NULL with count > 0, outStates not NULL (BEAGLE_ERROR_OUT_OF_RANGE each).  A refused call writes
 * nothing.  count == 0 is legal and samples the top alone.  The call is synchronous. */
BEAGLE_DLLEXPORT int mbamdSampleAncestralStates(int instance, const int* parentSlots, const int* postBufferIndices,
                                                const int* matrixIndices, int count, int categoryWeightsIndex,
                                                unsigned long long seed, int* outStates, int* outCategories,
                                                double* outChangeCounts);

/* The log-likelihood of the sites in their ORDER along the sequence under a hidden Markov chain over the rate categories -- Yang's
 * autocorrelated discrete gamma (rates=adgamma), in general the Felsenstein-Churchill HMM --, and the per-site category posteriors
 * of that chain, on the single- AND the double-precision engine.
 *
 * With the sites s = 0 .. n-1 (n = siteCount), K the category count, c_s = sitePatterns[s], w the weights of categoryWeightsIndex,
 * T = categoryTransitions (row-major, T[a][b] = P(next site in b | this site in a) at distance 1), T^(j) its j-th power,
 * j_s = siteJumps[s] >= 1 for s >= 1 (siteJumps[0] is ignored; a NULL array: all jumps are 1), L_k(c) the likelihood of pattern c in
 * category k and L(c) = sum_k w_k L_k(c):
 *
 *     H = sum over all paths k_0 ... k_{n-1} of  w_{k_0} L_{k_0}(c_0) * prod_{s>=1} T^(j_s)[k_{s-1}, k_s] * L_{k_s}(c_s)
 *
 * With q_k(c) = w_k L_k(c) / L(c) -- exactly the doubles mbamdGetCategoryPosteriors returns -- and l(c) = ln L(c) -- exactly the
 * doubles beagleGetSiteLogLikelihoods returns --,
 *
 *     ln H = sum_s l(c_s)  +  ln( u^T A_1 A_2 ... A_{n-1} 1 ),      u[k] = q_k(c_0),      A_s = T^(j_s) diag( q_k(c_s) / w_k )
 *
 * The second term is a correction to the plain mixture likelihood, made of numbers in [0, 1 / min w]; it vanishes where every row of
 * T equals w (independent sites).  The per-site category posteriors are the forward-backward quantities of the same chain,
 *
 *     gamma_s(k) = alpha_s(k) beta_s(k) / sum_k alpha_s(k) beta_s(k),   alpha_s^T = u^T A_1 ... A_s,   beta_s = A_{s+1} ... A_{n-1} 1
 *     outSiteCategoryPosteriors[k * siteCount + s] = gamma_s(k)                     (or NULL)
 *
 * -- the site rates under the HMM are sum_k gamma_s(k) r_k.  Pattern weights play no part: sites are listed explicitly.  Row sums of T
 * are the caller's business: the formulas above are what is computed.
 *
 * Arithmetic: all in double.  T^(j) is formed on the host, once per distinct jump value of the call, by LEFT-TO-RIGHT BINARY
 * EXPONENTIATION: from T, for every bit of j below its highest, from the high end, square, then, where the bit is set, multiply by
 * T on the right.  Any jump is served, any number of distinct jumps.  The ordered product is a tree reduction on the device with the
 * chunk length 64 (HMM_CHUNK, csrc/mbamd_autocorrelated.h): every run of 64 consecutive sites becomes its ordered K x K product, every
 * run of 64 products one, until one is left; after every factor the product is scaled by an exact power of two and an integer
 * exponent is carried beside it, so that scaling rounds nothing and nothing underflows at any n.  sum_s l(c_s) is added in the
 * same tree: site order within a chunk, chunk order within a run of chunks.  The same inputs give the same bits, call after call;
 * outLogLikelihood does not depend on whether the posteriors are asked for; a pattern-sharded instance returns the bits of an
 * unsharded one (the shards' columns are gathered on the first device).
 *
 * Operands: those of the latest beagleCalculate{Root,Edge}LogLikelihoods call, as for mbamdGetCategoryPosteriors; q is kept with
 * that call, so a second call after it -- another T: the correlation move -- costs the reduction alone.  One category: ln H =
 * sum_s l(c_s), gamma = 1, and T is read only to be checked.
 *
 * Refusals.  No log-likelihood call yet is BEAGLE_ERROR_GENERAL, one with count > 1 BEAGLE_ERROR_NO_IMPLEMENTATION, a
 * categoryWeightsIndex that is not that call's BEAGLE_ERROR_OUT_OF_RANGE; not on a multi-partition instance
 * (BEAGLE_ERROR_NO_IMPLEMENTATION); whatever makes beagleGetSiteLogLikelihoods refuse makes this call refuse alike.
 * BEAGLE_ERROR_OUT_OF_RANGE: siteCount < 1; sitePatterns, categoryTransitions or outLogLikelihood NULL; a pattern index outside
 * [0, patternCount); a jump < 1 at s >= 1; an entry of T that is negative or not finite; a weight w_k that is not positive (the
 * emission of such a category is not in q).  A refused call writes nothing.  The call is synchronous.
 *
 * A listed site whose pattern has L(c) not positive has all its q zero: the result (-inf) is written and
 * BEAGLE_ERROR_FLOATING_POINT returned, as by the log-likelihood calls; the gamma of a call whose product is zero are all 0. */
BEAGLE_DLLEXPORT int mbamdCalculateAutocorrelatedLogLikelihood(int instance, int categoryWeightsIndex, const int* sitePatterns,
                                                               const int* siteJumps, int siteCount,
                                                               const double* categoryTransitions,       /* [K][K] */
                                                               double* outLogLikelihood,                /* never NULL */
                                                               double* outSiteCategoryPosteriors);      /* [K][siteCount], or NULL */

#ifdef __cplusplus
}
#endif
#endif
