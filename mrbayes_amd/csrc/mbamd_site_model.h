// mbamd_site_model.h -- the gradient of the log-likelihood in the SITE MODEL: the rate of every category, the weight of every
// category and the direct term of the state frequencies at the root (mbamdCalculateSiteModelDerivatives; semantics:
// include/libhmsbeagle/beagle.h).  Included by mbamd_f32.h and mbamd_f64.h; product and TEST-ONLY host emulation
// compile these same kernels.
//
// Per edge e, category k and pattern c, from the buffers the gradient call reads (mbamd_preorder.h),
//     den_k(c)   = sum_l pre_e[k,c,l] post_e[k,c,l]
//     g_e,k(c)   = (sum_l pre_e[k,c,l] sum_j D_k[l,j] post_e[k,c,j]) / den_k(c)
//     G[e][k]    = sum_c weight_c q_k(c) g_e,k(c)
// -- k_edge_readout's terms, kept apart by category instead of added over them.  With D_k = Q (unit rate) sum_e t_e G[e][k] is
// d lnL / d r_k: the branch of category k has the length r_k t_e, and d lnL / d (r_k t_e) = G[e][k] whatever r_k is -- a category
// of rate zero is served without a division by it.  The two other outputs read no pre-order buffer:
//     C[k]       = sum_c weight_c q_k(c)                                         the expected number of sites in category k
//     F[i]       = sum_c weight_c sum_k q_k(c) parent[k,c,i] f_k(c,i) / sum_l pi_l parent[k,c,l] f_k(c,l)
// with parent, f_k (1 for a root call, sum_j P_k[i,j] child[k,c,j] for an edge call) and pi the operands of the latest
// log-likelihood call -- the terms k_category_posteriors and k_sample_top form.  d lnL / d w_k = C[k] / w_k; F[i] is d lnL / d pi_i at
// fixed Q, without a division by pi_i.
//
// Every output is a sum of RATIOS taken inside one (pattern, category) column pair: the power of two the pre-order pass discarded,
// whatever scale a post-order column carries (its own power of two goes out before the first product, mbamd_derivatives.h) and the
// category's exponent of the log-likelihood call all leave numerator and denominator alike; q carries the categories' relative
// sizes (k_category_posteriors).  A category whose denominator is not positive has underflowed and is skipped.
//
// Arithmetic as in k_edge_readout: products in the engine's precision, sums over states in double, one division per category,
// block sums through mbd_wave_sum_store, then k_gradient_sums -- one block sum per (edge, category), (category) or (state), so a
// value depends neither on how the edges are cut into chunks nor on which other outputs are asked for.
#ifndef MBAMD_SITE_MODEL_H_
#define MBAMD_SITE_MODEL_H_

#include "mbamd_preorder.h"      // GradEdge, ReadoutArgs, DerivArgs and the layout accessors, k_gradient_sums, chunked_readout, the engine hooks

namespace mbamd {

// the arguments of the two read-outs that need no edge: g = the operands of the latest log-likelihood call (k_root_frequency_readout)
// or the layout alone (k_category_counts)
struct SiteModelTopArgs {
    DerivArgs     g;
    const double* q;              // [K][Ppad] posterior category probabilities, or null (one category: q = 1)
    const double* pattern_weights;
    double*       sums;           // counts: [K][nb], root frequencies: [S][nb] -- one per 64-pattern block
    int           nb;
};

// dynamic LDS of k_root_frequency_readout beyond four states: one column of S doubles per thread, [state][thread]
inline size_t root_frequency_lds_bytes(int S) { return (size_t) S * 64 * sizeof(double); }

// G[e][k] of every edge of the launch: grid (64-pattern blocks, edges), one thread per pattern -- k_edge_readout at order 1 with the
// category loop outermost and nothing carried from one category to the next: weight_c q_k num / den goes to the block sum of
// (edge, category) as soon as the category is done, a.sums = [edges][K][nb].  (a.site, a.site2, a.D2 and a.edgeCount are not read.)
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_edge_category_readout(ReadoutArgs a)
{
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K;
    const int c = (int) blockIdx.x * 64 + (int) threadIdx.x;
    const bool live = c < g.last;
    const GradEdge ed = a.edges[blockIdx.y];
    const double pw = live ? a.pattern_weights[c] : 0.0;
    const unsigned tip = live && ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
    double* const sums = a.sums + (size_t) blockIdx.y * K * a.nb + blockIdx.x;
    for (int k = 0; k < K; ++k) {
        double num = 0.0, den = 0.0;
        if (live) {
            if constexpr (LAYOUT == DERIV_S4) {
                const size_t at = blk_index(c, g.pstride) + (size_t) k * 64;
                const f4 p4 = reinterpret_cast<const f4*>(ed.pre)[at];
                const float p[4] = {p4.x, p4.y, p4.z, p4.w};
                float v[4];
                if (ed.postTip) {
                    for (int j = 0; j < 4; ++j) v[j] = (tip >> j & 1u) ? 1.0f : 0.0f;
                } else {
                    const f4 q4 = reinterpret_cast<const f4*>(ed.post)[at];
                    v[0] = q4.x; v[1] = q4.y; v[2] = q4.z; v[3] = q4.w;
                    pre_scale4(v);
                }
                const MBAMD_AS_CONST float* m = as_const(reinterpret_cast<const float*>(ed.D)) + k * 16;          // m[j * 4 + l] = D(l -> j)
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const float f = fmaf(m[12 + l], v[3], fmaf(m[8 + l], v[2], fmaf(m[4 + l], v[1], m[l] * v[0])));
                    num += (double) (p[l] * f);
                    den += (double) (p[l] * v[l]);
                }
            } else {
                const PostColumn<LAYOUT, Real> post(ed.postTip ? nullptr : ed.post, g, k, c);
                for (int l = 0; l < S; ++l) {
                    const Real p = deriv_partial<LAYOUT, Real>(ed.pre, g, k, l, c);
                    Real f = (Real) 0, v;
                    if (ed.postTip) {
                        // (a missing state is the vector of ones: the rows of a differential matrix sum to zero)
                        v = (tip >= (unsigned) S || tip == (unsigned) l) ? (Real) 1 : (Real) 0;
                        if (tip < (unsigned) S) f = deriv_matrix<LAYOUT, Real>(ed.D, g, k, l, (int) tip);
                    } else {
                        for (int j = 0; j < S; ++j) f = deriv_fma(deriv_matrix<LAYOUT, Real>(ed.D, g, k, l, j), post[j], f);
                        v = post[l];
                    }
                    num += (double) (p * f);
                    den += (double) (p * v);
                }
            }
        }
        double v = 0.0;
        if (den > 0.0) v = (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) * (num / den);
        mbd_wave_sum_store(pw * v, sums + (size_t) k * a.nb);
    }
}

// C[k]: grid (64-pattern blocks, categories), one thread per pattern
__global__ void __launch_bounds__(64)
k_category_counts(SiteModelTopArgs a)
{
    const int c = (int) blockIdx.x * 64 + (int) threadIdx.x;
    double v = 0.0;
    if (c < a.g.last) v = a.pattern_weights[c] * (a.q != nullptr ? a.q[(size_t) blockIdx.y * a.g.Ppad + c] : 1.0);
    mbd_wave_sum_store(v, a.sums + (size_t) blockIdx.y * a.nb + blockIdx.x);
}

// F[i]: grid = the 64-pattern blocks, one thread per pattern, looping over the categories.  The term of state i in category k is
// the one k_category_posteriors adds to `cat`, before the frequency: parent[k,c,i] f_k(c,i), both columns with their own power of
// two taken out.  Four states: the running column in registers.  Other layouts: it lies in LDS, [state][thread] (as a private array
// indexed at run time it would be scratch), and a category is walked twice -- the denominator, then the accumulation --, as in
// k_node_posteriors.  No thread reads another's column: no barrier.  This kernel runs once per call.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_root_frequency_readout(SiteModelTopArgs a)
{
    const DerivArgs& g = a.g;
    const int S = LAYOUT == DERIV_S4 ? 4 : g.S, K = g.K;
    const int c = (int) blockIdx.x * 64 + (int) threadIdx.x;
    const bool live = c < g.last;
    const double pw = live ? a.pattern_weights[c] : 0.0;
    const unsigned tip = live && g.child_tip ? deriv_tip<LAYOUT>(g.child, g, c) : 0u;
    double p4[4] = {0.0, 0.0, 0.0, 0.0};
    double* col = nullptr;                                               // F's column of this thread's pattern: col[i * 64]
    if constexpr (LAYOUT != DERIV_S4) {
        col = mbd_dyn_lds<double>() + threadIdx.x;
        for (int i = 0; i < S; ++i) col[i * 64] = 0.0;
    }
    for (int k = 0; live && k < K; ++k) {
        const PostColumn<LAYOUT, Real> parent(g.parent, g, k, c), child(g.child_tip ? nullptr : g.child, g, k, c);
        if (!parent.live || !child.live) continue;
        auto term = [&](int i) -> Real {
            Real f = (Real) 1;
            if (g.child != nullptr) {
                if (g.child_tip && LAYOUT != DERIV_S4) {
                    if (tip < (unsigned) S) f = deriv_matrix<LAYOUT, Real>(g.matrix[0], g, k, i, (int) tip);
                } else {
                    f = (Real) 0;
                    for (int j = 0; j < S; ++j) {
                        const Real v = g.child_tip ? ((tip >> j & 1u) ? (Real) 1 : (Real) 0) : child[j];
                        f = deriv_fma(deriv_matrix<LAYOUT, Real>(g.matrix[0], g, k, i, j), v, f);
                    }
                }
            }
            return parent[i] * f;
        };
        double den = 0.0;
        if constexpr (LAYOUT == DERIV_S4) {
            double t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { t[i] = (double) term(i); den += t[i] * g.freqs[i]; }
            if (den > 0.0) {
                const double f = (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) / den;
#pragma unroll
                for (int i = 0; i < 4; ++i) p4[i] += f * t[i];
            }
        } else {
            for (int i = 0; i < S; ++i) den += (double) term(i) * g.freqs[i];
            if (den > 0.0) {
                const double f = (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) / den;
                for (int i = 0; i < S; ++i) col[i * 64] += f * (double) term(i);
            }
        }
    }
    if constexpr (LAYOUT == DERIV_S4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mbd_wave_sum_store(pw * p4[i], a.sums + (size_t) i * a.nb + blockIdx.x);
    } else {
        for (int i = 0; i < S; ++i) mbd_wave_sum_store(pw * col[i * 64], a.sums + (size_t) i * a.nb + blockIdx.x);
    }
}

// ---- host side, shared by the two engines (the hooks: mbamd_preorder.h) ------------------------------------------------------

template <int LAYOUT, class Real>
inline void launch_root_frequency_readout(hipStream_t stream, const SiteModelTopArgs& a)
{
    auto kernel = k_root_frequency_readout<LAYOUT, Real>;
    if constexpr (LAYOUT == DERIV_S4) {
        MBAMD_LAUNCH(kernel, (unsigned) a.nb, 64, 0, stream, a);
    } else {
        const size_t lds = root_frequency_lds_bytes(a.g.S);
        if (lds > (size_t) 48 * 1024 && hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            (void) hipGetLastError();
        MBAMD_LAUNCH(kernel, (unsigned) a.nb, 64, lds, stream, a);
    }
}

// mbamdCalculateSiteModelDerivatives on the engine's patterns.  edgeCat (or null) takes this engine's G[e][k] at [e * K + k], counts
// (or null) C[k], rootFreq (or null) F[i]; the list is checked whatever is asked for, and nothing is written before it is good.
// Launches: k_category_posteriors where q is not that of the latest log-likelihood call yet (ensure_posteriors); for counts and
// rootFreq one kernel each and ONE k_gradient_sums over their K + S rows; for edgeCat, per chunk of edges (chunked_readout; the cap
// is MBAMD_POSTERIOR_NODES, test only), k_edge_category_readout and k_gradient_sums over the chunk's edges x K rows.  Synchronous.
template <class Engine>
inline int site_model_derivatives(Engine& e, const int* post, const int* pre, const int* dmat, const int* wIdx, int count, double* edgeCat,
                                  double* counts, double* rootFreq)
{
    const char* const who = "mbamdCalculateSiteModelDerivatives";
    { const int rc = edge_list_begin(e, who); if (rc) return rc; }
    if (rootFreq) {
        if (e.lastLnl.count == 0)
            return fail(BEAGLE_ERROR_GENERAL, who, "no log-likelihood was calculated yet: the root's operands and frequencies are that call's");
        if (e.lastLnl.count > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "the latest log-likelihood call had more than one subset");
    }
    for (int i = 0; i < count; ++i) {
        const int rc = edge_check(e, who, post[i], pre[i], wIdx[i]);
        if (rc) return rc;
        if (dmat[i] < 0 || dmat[i] >= e.nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "differential matrix index");
    }
    const int S = e.S, K = e.K, nb = e.Ppad / 64;
    if (counts || rootFreq) {
        if (K > 1) { const int rc = ensure_posteriors(e); if (rc) return rc; }
        SiteModelTopArgs a;
        std::memset(&a, 0, sizeof a);
        if (rootFreq) { const int rc = e.posteriorOperands(a.g); if (rc) return rc; }
        else a.g = e.layoutArgs();
        const int rows = (counts ? K : 0) + (rootFreq ? S : 0);
        double* d_sums = nullptr;
        { const int rc = e.resultScratch(((size_t) rows * nb + rows) * sizeof(double), &d_sums); if (rc) return rc; }
        double* const d_out = d_sums + (size_t) rows * nb;
        a.q = K > 1 ? e.d_q : nullptr;
        a.pattern_weights = e.d_pweights;
        a.nb = nb;
        if (counts) {
            a.sums = d_sums;
            MBAMD_LAUNCH(k_category_counts, dim3((unsigned) nb, (unsigned) K), 64, 0, e.stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (rootFreq) {
            a.sums = d_sums + (size_t) (counts ? K : 0) * nb;
            e.withLayout([&](auto L) { launch_root_frequency_readout<L(), deriv_real<L()>>(e.stream, a); });
            HIP_TRY(hipGetLastError());
        }
        MBAMD_LAUNCH(k_gradient_sums, dim3((unsigned) rows, 1u), 64, 0, e.stream, (const double*) d_sums, nb, rows, d_out);
        HIP_TRY(hipGetLastError());
        e.countLaunches((counts ? 1 : 0) + (rootFreq ? 1 : 0) + 1);
        HIP_TRY(hipStreamSynchronize(e.stream));
        e.afterSync();
        std::vector<double> h((size_t) rows);
        HIP_TRY(hipMemcpy(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (counts) std::copy(h.begin(), h.begin() + K, counts);
        if (rootFreq) std::copy(h.end() - S, h.end(), rootFreq);
    }
    if (!edgeCat || count <= 0) return BEAGLE_SUCCESS;
    std::vector<GradEdge> table((size_t) count);
    { const int rc = edge_list_fill(e, post, pre, count, table.data()); if (rc) return rc; }
    for (int i = 0; i < count; ++i) table[(size_t) i].D = e.matrixPtr(dmat[i]);
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size() * sizeof(GradEdge), &d_table); if (rc) return rc; }
    ReadoutShape shape = {};
    shape.sumPlanes = 1;
    shape.sumRows = K;
    shape.cap = e.sw.posteriorNodes.value_or(0);
    ReadoutArgs a;
    std::memset(&a, 0, sizeof a);
    a.g = e.layoutArgs();
    a.q = K > 1 ? e.d_q : nullptr;
    a.pattern_weights = e.d_pweights;
    a.nb = nb;
    return chunked_readout(e, count, shape,
        [&](const ReadoutChunk& ch) {
            a.edges = static_cast<const GradEdge*>(d_table) + ch.first;
            a.edgeCount = ch.count;
            a.sums = ch.sums;
            e.withLayout([&](auto L) {
                auto kernel = k_edge_category_readout<L(), deriv_real<L()>>;
                MBAMD_LAUNCH(kernel, dim3((unsigned) nb, (unsigned) ch.count), 64, 0, e.stream, a);
            });
        },
        [&](const ReadoutChunk& ch, int i) {
            std::memcpy(edgeCat + (size_t) (ch.first + i) * K, ch.sums + (size_t) i * K, (size_t) K * sizeof(double));
        });
}

}  // namespace mbamd
#endif
