// mbamd_posteriors.h -- what happened at the nodes and at the sites, read from the buffers the gradient reads: the marginal posterior
// of every state at every listed node (mbamdCalculateNodePosteriors) and the posterior category probabilities of every pattern
// (mbamdGetCategoryPosteriors); semantics: include/libhmsbeagle/mbamd_reports.h, DESIGN 4.4.7.  Included by mbamd_f32.h and
// mbamd_f64.h; product and TEST-ONLY host emulation compile this same kernel.
//
// pre_n[k,c,a] post_n[k,c,a] is the joint of state a at node n with all the data of pattern c in category k, up to the power of two
// the pre-order pass discarded (mbamd_preorder.h) and whatever scale the post-order buffer carries -- one factor per (pattern,
// category), which leaves the ratio inside a category:
//     j_k(a) = pre_n[k,c,a] post_n[k,c,a],     den_k = sum_a j_k(a),     p_c(a) = sum_k q_k(c) j_k(a) / den_k
// with q the posterior category probabilities of the pattern (k_category_posteriors; one category: q = 1).  This is DESIGN 4.4.2's
// argument with the identity in the place of the differential matrix: no matrix, no quotient of two buffers, no exponents (the
// post-order column's own power of two is taken out before the product, mbamd_derivatives.h: an unscaled column may be subnormal).  A
// category whose den_k is zero has underflowed and is skipped, as k_edge_readout skips it.  A compact tip is the indicator of its
// state, a missing state the vector of ones, the four-state bitplanes give the compatible columns; where ONE state is compatible
// the posterior is that indicator and is written as such -- exactly 1 and 0, where the formula would give sum_k q_k.
//
// Arithmetic as in k_edge_readout: the product in the engine's precision, den_k and the sum over the categories in double (the
// division once per category: q_k / den_k), block sums through mbd_wave_sum_store, then k_gradient_sums over the S rows of a node.
#ifndef MBAMD_POSTERIORS_H_
#define MBAMD_POSTERIORS_H_

#include "mbamd_preorder.h"      // GradEdge, DerivArgs and the layout accessors, k_gradient_sums, the edge_list_* checks

namespace mbamd {

struct PosteriorArgs {
    DerivArgs       g;
    const GradEdge* nodes;        // the nodes of this launch (grid y); D is not used
    const double*   q;            // [K][Ppad] posterior category probabilities, or null (one category: q = 1)
    const double*   pattern_weights;
    double*         site;         // [nodes][S][Ppad] p_c(a), or null
    double*         best;         // [nodes][Ppad] max_a p_c(a), or null
    int*            bestState;    // [nodes][Ppad] the smallest a that attains it (with `best`)
    double*         sums;         // [nodes][S][nb]: weight_c p_c(a), one per 64-pattern block
    int             nb;
};

// dynamic LDS of the general form: one column of S doubles per thread, [state][thread]
inline size_t posterior_lds_bytes(int S) { return (size_t) S * 64 * sizeof(double); }

// Grid (64-pattern blocks, nodes), one thread per pattern, looping over the categories: the sibling of k_edge_readout.
// Four states (DERIV_S4): two f4 loads per category (one and the bitplanes at a compact tip), the four running sums in registers.
// Other layouts: the thread's running column p(.) lies in LDS, [state][thread] (as a private array indexed at run time it would be
// scratch: k_final_pass, k_pre_partials), and a category is walked twice -- den_k, then the accumulation; the second walk finds the
// 2 S values of the thread where the first left them, in the cache.  No thread reads another's column: no barrier.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_node_posteriors(PosteriorArgs a)
{
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K;
    const int c = (int) blockIdx.x * 64 + (int) threadIdx.x;
    const bool live = c < g.last;
    const size_t node = blockIdx.y;
    const GradEdge nd = a.nodes[node];
    const double pw = live ? a.pattern_weights[c] : 0.0;
    const unsigned tip = live && nd.postTip ? deriv_tip<LAYOUT>(nd.post, g, c) : 0u;
    double bestValue = -1.0;
    int bestAt = 0;
    if constexpr (LAYOUT == DERIV_S4) {
        double p[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            if (nd.postTip && tip != 0u && (tip & (tip - 1u)) == 0u) {
#pragma unroll
                for (int l = 0; l < 4; ++l) p[l] = (tip >> l & 1u) ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < K; ++k) {
                    const size_t at = blk_index(c, g.pstride) + (size_t) k * 64;
                    const f4 p4 = reinterpret_cast<const f4*>(nd.pre)[at];
                    float j[4] = {p4.x, p4.y, p4.z, p4.w};
                    if (nd.postTip) {
#pragma unroll
                        for (int l = 0; l < 4; ++l) j[l] = (tip >> l & 1u) ? j[l] : 0.0f;
                    } else {
                        const f4 q4 = reinterpret_cast<const f4*>(nd.post)[at];
                        float v[4] = {q4.x, q4.y, q4.z, q4.w};
                        pre_scale4(v);
                        j[0] *= v[0]; j[1] *= v[1]; j[2] *= v[2]; j[3] *= v[3];
                    }
                    double den = 0.0;
#pragma unroll
                    for (int l = 0; l < 4; ++l) den += (double) j[l];
                    if (den > 0.0) {
                        const double f = (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) / den;
#pragma unroll
                        for (int l = 0; l < 4; ++l) p[l] += f * (double) j[l];
                    }
                }
            }
        }
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (live && a.site != nullptr) a.site[(node * 4 + l) * (size_t) g.Ppad + c] = p[l];
            if (p[l] > bestValue) { bestValue = p[l]; bestAt = l; }
            mbd_wave_sum_store(pw * p[l], a.sums + (node * 4 + l) * (size_t) a.nb + blockIdx.x);
        }
    } else {
        double* const col = mbd_dyn_lds<double>() + threadIdx.x;         // p(l) of this thread's pattern: col[l * 64]
        if (live) {
            if (nd.postTip && tip < (unsigned) S) {
                for (int l = 0; l < S; ++l) col[l * 64] = tip == (unsigned) l ? 1.0 : 0.0;
            } else {
                for (int l = 0; l < S; ++l) col[l * 64] = 0.0;
                for (int k = 0; k < K; ++k) {
                    // (the post-order column's own power of two goes out before the first product: an unscaled column may be
                    //  subnormal.  Staging the column in LDS instead of walking it a third time was measured: slower, +54 %
                    //  on the call against +15 %, profiles/preorder_exponent_range.txt)
                    const PostColumn<LAYOUT, Real> post(nd.postTip ? nullptr : nd.post, g, k, c);
                    double den = 0.0;
                    for (int l = 0; l < S; ++l) {
                        const Real p = deriv_partial<LAYOUT, Real>(nd.pre, g, k, l, c);
                        // (a compact tip here has a missing state: the vector of ones)
                        den += (double) (nd.postTip ? p : p * post[l]);
                    }
                    if (den > 0.0) {
                        const double f = (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) / den;
                        for (int l = 0; l < S; ++l) {
                            const Real p = deriv_partial<LAYOUT, Real>(nd.pre, g, k, l, c);
                            col[l * 64] += f * (double) (nd.postTip ? p : p * post[l]);
                        }
                    }
                }
            }
        }
        for (int l = 0; l < S; ++l) {
            const double v = live ? col[l * 64] : 0.0;
            if (live && a.site != nullptr) a.site[(node * S + l) * (size_t) g.Ppad + c] = v;
            if (v > bestValue) { bestValue = v; bestAt = l; }
            mbd_wave_sum_store(pw * v, a.sums + (node * S + l) * (size_t) a.nb + blockIdx.x);
        }
    }
    if (live && a.best != nullptr) {
        a.best[node * (size_t) g.Ppad + c] = bestValue;
        a.bestState[node * (size_t) g.Ppad + c] = bestAt;
    }
}

// ---- host side, shared by the two engines (the hooks: mbamd_preorder.h) ------------------------------------------------------

template <int LAYOUT, class Real>
inline void launch_node_posteriors(hipStream_t stream, const PosteriorArgs& a, int nn)
{
    auto kernel = k_node_posteriors<LAYOUT, Real>;
    const dim3 grid((unsigned) a.nb, (unsigned) nn);
    if constexpr (LAYOUT == DERIV_S4) {
        MBAMD_LAUNCH(kernel, grid, 64, 0, stream, a);
    } else {
        const size_t lds = posterior_lds_bytes(a.g.S);
        if (lds > (size_t) 48 * 1024 && hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            (void) hipGetLastError();
        MBAMD_LAUNCH(kernel, grid, 64, lds, stream, a);
    }
}

// mbamdCalculateNodePosteriors on the engine's patterns, through chunked_readout (mbamd_preorder.h): per chunk of nodes one launch
// of k_node_posteriors and k_gradient_sums over the chunk's nodes x S rows.  sums[i * S + a] is this engine's weighted sum of state
// a at node i; sites (or null) takes p_c(a) of node i at sites[(i * siteStride + c) * S + a] -- the staging is [state][pattern], the
// copy transposes --, bestStates / bestValues (or null, each) the best state of pattern c and its posterior at [i * siteStride + c].
template <class Engine>
inline int node_posteriors(Engine& e, const int* post, const int* pre, const int* wIdx, int count, double* sites, int* bestStates,
                           double* bestValues, size_t siteStride, double* sums)
{
    const char* const who = "mbamdCalculateNodePosteriors";
    { const int rc = edge_list_begin(e, who); if (rc) return rc; }
    for (int i = 0; i < count; ++i) {
        const int rc = edge_check(e, who, post[i], pre[i], wIdx[i]);
        if (rc) return rc;
    }
    if (count <= 0) return BEAGLE_SUCCESS;
    std::vector<GradEdge> table((size_t) count);
    { const int rc = edge_list_fill(e, post, pre, count, table.data()); if (rc) return rc; }
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size() * sizeof(GradEdge), &d_table); if (rc) return rc; }
    const int S = e.S, P = e.P;
    const size_t Ppad = (size_t) e.Ppad;
    const bool best = bestStates != nullptr || bestValues != nullptr;
    // the per-pattern outputs: the posteriors, then the best values and the best states
    ReadoutShape shape = {};
    if (sites) shape.site[shape.siteCount++] = {S, sizeof(double)};
    const int bestAt = shape.siteCount;
    if (best) {
        shape.site[shape.siteCount++] = {1, sizeof(double)};
        shape.site[shape.siteCount++] = {1, sizeof(int)};
    }
    shape.sumPlanes = 1;
    shape.sumRows = S;
    shape.cap = e.sw.posteriorNodes.value_or(0);
    PosteriorArgs a;
    a.g = e.layoutArgs();
    a.q = e.K > 1 ? e.d_q : nullptr;
    a.pattern_weights = e.d_pweights;
    a.nb = e.Ppad / 64;
    return chunked_readout(e, count, shape,
        [&](const ReadoutChunk& ch) {
            a.nodes = static_cast<const GradEdge*>(d_table) + ch.first;
            a.site = sites ? static_cast<double*>(ch.site[0]) : nullptr;
            a.best = best ? static_cast<double*>(ch.site[bestAt]) : nullptr;
            a.bestState = best ? static_cast<int*>(ch.site[bestAt + 1]) : nullptr;
            a.sums = ch.sums;
            e.withLayout([&](auto L) { launch_node_posteriors<L(), deriv_real<L()>>(e.stream, a, ch.count); });
        },
        [&](const ReadoutChunk& ch, int i) {
            const size_t to = (size_t) (ch.first + i) * siteStride;
            if (sites) {
                const double* const from = static_cast<const double*>(ch.site[0]) + (size_t) i * S * Ppad;
                for (int s = 0; s < S; ++s)
                    for (int c = 0; c < P; ++c) sites[(to + c) * S + s] = from[(size_t) s * Ppad + c];
            }
            if (bestValues) std::memcpy(bestValues + to, static_cast<const double*>(ch.site[bestAt]) + (size_t) i * Ppad, (size_t) P * sizeof(double));
            if (bestStates) std::memcpy(bestStates + to, static_cast<const int*>(ch.site[bestAt + 1]) + (size_t) i * Ppad, (size_t) P * sizeof(int));
            std::memcpy(sums + (size_t) (ch.first + i) * S, ch.sums + (size_t) i * S, (size_t) S * sizeof(double));
        });
}

// mbamdGetCategoryPosteriors on the engine's patterns: q_k(c) of the latest log-likelihood call at out[k * stride + c] (d_q without
// its padding); one category: ones, and nothing is asked of a log-likelihood call.  Synchronous.
template <class Engine>
inline int category_posteriors(Engine& e, int wIdx, double* out, size_t stride)
{
    const char* const who = "mbamdGetCategoryPosteriors";
    { const int rc = edge_list_begin(e, who); if (rc) return rc; }
    const int K = e.K, P = e.P, Ppad = e.Ppad;
    if (K == 1) {
        std::fill(out, out + P, 1.0);
        return BEAGLE_SUCCESS;
    }
    if (wIdx != e.lastLnl.weights) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "category weights index differs from the latest log-likelihood call's");
    { const int rc = ensure_posteriors(e); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(e.stream));
    e.afterSync();
    std::vector<double> h((size_t) K * Ppad);
    HIP_TRY(hipMemcpy(h.data(), e.d_q, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k) std::memcpy(out + (size_t) k * stride, h.data() + (size_t) k * Ppad, (size_t) P * sizeof(double));
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd
#endif
