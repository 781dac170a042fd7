// mbamd_crossproducts.h -- the gradient in the rate matrix: the S x S cross-product matrix of upstream BEAGLE 4's
// beagleCalculateCrossProductDerivative (semantics: include/libhmsbeagle/beagle.h), read from the same pre-order and
// post-order buffers as the branch-length gradient (mbamd_preorder.h).  Included by mbamd_f32.h and mbamd_f64.h; product and
// TEST-ONLY host emulation compile these same kernels.
//
// Over the edges e of the call, the patterns c and the categories k
//     den      = sum_l pre_e[k,c,l] post_e[k,c,l]
//     X[i,j]  += (weight_c q_k(c) t_e r_k / den) pre_e[k,c,i] post_e[k,c,j]
// -- per edge and category a product A B^T of two [S x patterns] matrices, A the pre-order columns times one coefficient per pattern,
// B the post-order columns: a GEMM with an S x S result whose reduction runs over edges x categories x patterns.  Every scale factor
// of either buffer cancels per (pattern, category); a category with den <= 0 has underflowed and is skipped, as in k_edge_readout.
// The post-order column has its own power of two taken out before its first product (pre_exponent / pre_scaled of
// mbamd_derivatives.h, on the staged column in LDS or in registers -- no second pass over memory): den is formed from columns at
// [0.5, 1) and the coefficient ... / den cannot overflow over a subnormal den.
//
// Grid (64-pattern blocks, edge chunks), one wave per workgroup; the wave LOOPS over the edges of its chunk, so that what a launch
// leaves behind is one S x S double matrix per (block, chunk) -- never one per edge.  Arithmetic as in k_edge_readout: products in
// the engine's precision, den summed in double; the coefficient is formed in double, rounded ONCE to the engine's precision and
// multiplied into the pre-order column; the products A[i,c] B[j,c] are
//   * added in double as they come (k_cross_products: four states in registers, other layouts from LDS), or
//   * added in fp32 by the matrix core (k_cross_products_mfma), where an fp32 accumulator takes at most 64 K products -- the 64
//     patterns and K categories of ONE edge -- before it is added into its double partner in registers and cleared (the flush rule
//     the test bound counts on).
// k_cross_product_sums then adds the (block, chunk) matrices per entry in a fixed order.
#ifndef MBAMD_CROSSPRODUCTS_H_
#define MBAMD_CROSSPRODUCTS_H_

#include "mbamd_preorder.h"      // GradEdge, DerivArgs and the layout accessors

namespace mbamd {

struct CrossArgs {
    DerivArgs       g;
    const GradEdge* edges;            // the edges of the call (D unused)
    const double*   tr;               // [edges][K]: t_e r_k
    const double*   q;                // [K][Ppad] posterior category probabilities, or null (one category: q = 1)
    const double*   pattern_weights;
    double*         partial;          // [chunks][nb][S * S]
    int             nb, edgeCount, perChunk;      // edges [y perChunk, (y + 1) perChunk) belong to chunk y
    int             slab;             // k_cross_products, other than four states: entries [256 slab, 256 slab + 256) of the matrix
};

// LDS columns are [state][thread] with a row of 65: lanes that read one pattern of 32 consecutive states hit 32 banks, and so do the
// 64 lanes that write one state of their own patterns
#define MBAMD_XP_ROW 65
template <class Real> inline size_t cross_lds_bytes(int rows) { return (size_t) 2 * rows * MBAMD_XP_ROW * sizeof(Real); }

// the chunk count of a call: about 4096 waves where the edges allow, at least four edges to a chunk (a chunk leaves S S doubles behind,
// about what it reads per edge and category), and the (block, chunk) matrices within 8 Mi doubles
inline int cross_chunks(int count, int nb, int S)
{
    const size_t room = ((size_t) 8 << 20) / ((size_t) nb * S * S);
    const size_t want = (size_t) (4096 + nb - 1) / nb;
    return (int) std::max<size_t>(1, std::min<size_t>(std::min<size_t>(room, want), std::min<size_t>(((size_t) count + 3) / 4, 32768)));
}

// Pattern p of the block (thread p) stages its two columns of (edge, category k): colA = coefficient x pre, colB = post (a compact
// tip: its indicator vector, a missing state the vector of ones).  A pattern beyond the last, or a category without a denominator,
// stages zeros in colA.  Rows S .. of the columns are not touched.
template <int LAYOUT, class Real>
__device__ __forceinline__ void cross_stage(const CrossArgs& a, const GradEdge& ed, int e, int k, int c, bool live, unsigned tip, double pw,
                                            Real* colA, Real* colB)
{
    const DerivArgs& g = a.g;
    const int S = g.S;
    double den = 0.0;
    if (live) {
        Real mx = (Real) 0;
        // (sixteen states at a time: their loads are issued together -- one state after the other, every load's latency is waited for)
        for (int l0 = 0; l0 < S; l0 += 16) {
            Real p[16], v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int l = l0 + u < S ? l0 + u : S - 1;
                p[u] = deriv_partial<LAYOUT, Real>(ed.pre, g, k, l, c);
                if (ed.postTip) v[u] = (tip >= (unsigned) S || tip == (unsigned) l) ? (Real) 1 : (Real) 0;
                else v[u] = deriv_partial<LAYOUT, Real>(ed.post, g, k, l, c);
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (l0 + u < S) {
                    colA[(l0 + u) * MBAMD_XP_ROW] = p[u];
                    colB[(l0 + u) * MBAMD_XP_ROW] = v[u];
                    mx = v[u] > mx ? v[u] : mx;
                }
            }
        }
        // the post-order column's own power of two goes out where it lies, in LDS, before its first product (mbamd_derivatives.h:
        // an unscaled column may be subnormal); a compact tip's power is 2^0
        const int ev = ed.postTip ? 0 : pre_exponent(mx);
        for (int l = 0; l < S; ++l) {
            const Real v = pre_scaled(colB[l * MBAMD_XP_ROW], ev);
            colB[l * MBAMD_XP_ROW] = v;
            den += (double) (colA[l * MBAMD_XP_ROW] * v);
        }
    }
    Real coef = (Real) 0;
    if (live && den > 0.0) coef = (Real) (pw * (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) * a.tr[(size_t) e * g.K + k] / den);
    if (coef > (Real) 0) {
        for (int l = 0; l < S; ++l) colA[l * MBAMD_XP_ROW] *= coef;
    } else {
        for (int l = 0; l < S; ++l) colA[l * MBAMD_XP_ROW] = (Real) 0;
        if (!live) for (int l = 0; l < S; ++l) colB[l * MBAMD_XP_ROW] = (Real) 0;
    }
}

// Four states (DERIV_S4): a thread owns a pattern -- one f4 load per operand (bitplanes for a tip), the 16 entries in double
// registers across categories and edges, 16 wave sums at the end; no LDS.
// Other layouts: the two columns of the block are staged in dynamic LDS ([state][thread], cross_stage); lane l owns the entries
// ij = 256 slab + l, + 64, + 128, + 192 and adds their 64 products per (edge, category) in double.  A matrix of more than 256 entries
// takes ceil(S S / 256) launches, each of which stages the columns again: the plain reference beside k_cross_products_mfma, and what the
// double-precision engine runs.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_cross_products(CrossArgs a)
{
    const DerivArgs& g = a.g;
    const int K = g.K, lane = (int) threadIdx.x;
    const int c = (int) blockIdx.x * 64 + lane;
    const bool live = c < g.last;
    const double pw = live ? a.pattern_weights[c] : 0.0;
    const int e0 = (int) blockIdx.y * a.perChunk, e1 = e0 + a.perChunk < a.edgeCount ? e0 + a.perChunk : a.edgeCount;
    if constexpr (LAYOUT == DERIV_S4) {
        double acc[16];
#pragma unroll
        for (int ij = 0; ij < 16; ++ij) acc[ij] = 0.0;
        for (int e = e0; e < e1; ++e) {
            const GradEdge ed = a.edges[e];
            const unsigned tip = live && ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
            for (int k = 0; k < K && live; ++k) {
                const size_t at = (size_t) blockIdx.x * g.pstride + (size_t) k * 64 + lane;
                const f4 p4 = reinterpret_cast<const f4*>(ed.pre)[at];
                const float p[4] = {p4.x, p4.y, p4.z, p4.w};
                float v[4];
                if (ed.postTip) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (tip >> j & 1u) ? 1.0f : 0.0f;
                } else {
                    const f4 q4 = reinterpret_cast<const f4*>(ed.post)[at];
                    v[0] = q4.x; v[1] = q4.y; v[2] = q4.z; v[3] = q4.w;
                    pre_scale4(v);
                }
                double den = 0.0;
#pragma unroll
                for (int l = 0; l < 4; ++l) den += (double) (p[l] * v[l]);
                if (!(den > 0.0)) continue;
                const float coef = (float) (pw * (a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0) * a.tr[(size_t) e * K + k] / den);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ap = coef * p[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i * 4 + j] += (double) (ap * v[j]);
                }
            }
        }
        double* const out = a.partial + ((size_t) blockIdx.y * a.nb + blockIdx.x) * 16;
#pragma unroll
        for (int ij = 0; ij < 16; ++ij) mbd_wave_sum_store(acc[ij], out + ij);
    } else {
        const int S = g.S, SS = S * S;
        Real* const rowA = mbd_dyn_lds<Real>();
        Real* const rowB = rowA + (size_t) S * MBAMD_XP_ROW;
        int ia[4], jb[4];
        double acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int ij = a.slab * 256 + lane + 64 * n, i = ij < SS ? ij / S : 0, j = ij < SS ? ij - i * S : 0;
            ia[n] = i * MBAMD_XP_ROW; jb[n] = j * MBAMD_XP_ROW;
            acc[n] = 0.0;
        }
        for (int e = e0; e < e1; ++e) {
            const GradEdge ed = a.edges[e];
            const unsigned tip = live && ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
            for (int k = 0; k < K; ++k) {
                cross_stage<LAYOUT, Real>(a, ed, e, k, c, live, tip, pw, rowA + lane, rowB + lane);
                MBAMD_SYNC();
                for (int p = 0; p < 64; ++p) {
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[n] += (double) (rowA[ia[n] + p] * rowB[jb[n] + p]);
                }
                MBAMD_SYNC();
            }
        }
        double* const out = a.partial + ((size_t) blockIdx.y * a.nb + blockIdx.x) * SS;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int ij = a.slab * 256 + lane + 64 * n;
            if (ij < SS) out[ij] = acc[n];
        }
    }
}

// 16 .. 64 states on the fp32 engine: the same staging with rows S .. 32 TILES - 1 zero, then D (32 x 32) += A (32 x 2) B (2 x 32) with
// mbd_mfma_f32_32x32x2, the reduction index being the pattern -- lane l feeds A[l & 31][l >> 5] = colA[state l & 31][pattern 2 s + (l >> 5)]
// and B[l >> 5][l & 31] = colB[state l & 31][the same pattern], s = 0 .. 31: 32 instructions per tile, block and category.  TILES = 2:
// the four tiles are four independent accumulators.  TILES = 1: two accumulators, even and odd pattern pairs, added when they are
// flushed (a single chain would wait for the instruction's dependent-accumulator latency every time).  The accumulator layout (column
// l & 31, register r = row (r & 3) + 8 (r >> 2) + 4 (l >> 5)) is mbd_mfma_f32_32x32x2's (device/mbamd_dev_walkg_kernel.h).
template <int LAYOUT, int TILES>
__global__ void __launch_bounds__(64)
k_cross_products_mfma(CrossArgs a)
{
    constexpr int ROWS = 32 * TILES, NT = TILES * TILES, NACC = TILES == 1 ? 2 : NT;
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K, lane = (int) threadIdx.x;
    const int c = (int) blockIdx.x * 64 + lane;
    const bool live = c < g.last;
    const double pw = live ? a.pattern_weights[c] : 0.0;
    const int e0 = (int) blockIdx.y * a.perChunk, e1 = e0 + a.perChunk < a.edgeCount ? e0 + a.perChunk : a.edgeCount;
    float* const rowA = mbd_dyn_lds<float>();
    float* const rowB = rowA + (size_t) ROWS * MBAMD_XP_ROW;
    for (int l = S; l < ROWS; ++l) { rowA[l * MBAMD_XP_ROW + lane] = 0.0f; rowB[l * MBAMD_XP_ROW + lane] = 0.0f; }
    const float* const readA = rowA + (lane & 31) * MBAMD_XP_ROW + (lane >> 5);
    const float* const readB = rowB + (lane & 31) * MBAMD_XP_ROW + (lane >> 5);
    double sum[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[t][r] = 0.0;
    for (int e = e0; e < e1; ++e) {
        const GradEdge ed = a.edges[e];
        const unsigned tip = live && ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
        mbd_acc16 acc[NACC];
#pragma unroll
        for (int t = 0; t < NACC; ++t) acc[t] = (mbd_acc16) (0.0f);
        for (int k = 0; k < K; ++k) {
            cross_stage<LAYOUT, float>(a, ed, e, k, c, live, tip, pw, rowA + lane, rowB + lane);
            MBAMD_SYNC();
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                if constexpr (TILES == 1) {
                    acc[s & 1] = mbd_mfma_f32_32x32x2(readA[2 * s], readB[2 * s], acc[s & 1]);
                } else {
                    const float a0 = readA[2 * s], a1 = readA[32 * MBAMD_XP_ROW + 2 * s];
                    const float b0 = readB[2 * s], b1 = readB[32 * MBAMD_XP_ROW + 2 * s];
                    acc[0] = mbd_mfma_f32_32x32x2(a0, b0, acc[0]);
                    acc[1] = mbd_mfma_f32_32x32x2(a0, b1, acc[1]);
                    acc[2] = mbd_mfma_f32_32x32x2(a1, b0, acc[2]);
                    acc[3] = mbd_mfma_f32_32x32x2(a1, b1, acc[3]);
                }
            }
            MBAMD_SYNC();
        }
        // the flush: 64 K products at most went into an fp32 accumulator
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (TILES == 1) {
                sum[0][r] += (double) acc[0][r] + (double) acc[1][r];
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) sum[t][r] += (double) acc[t][r];
            }
        }
    }
    double* const out = a.partial + ((size_t) blockIdx.y * a.nb + blockIdx.x) * ((size_t) S * S);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 32 * (t % TILES) + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * (t / TILES) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (i < S && j < S) out[(size_t) i * S + j] = sum[t][r];
        }
    }
}

// out[ij] = the sum of the n (block, chunk) matrices' entry ij, in a fixed order, like k_gradient_sums: grid (S S), one wave per entry
__global__ void __launch_bounds__(64)
k_cross_product_sums(const double* __restrict__ partial, int n, int SS, double* __restrict__ out)
{
    const size_t ij = blockIdx.x;
    double s = 0.0;
    for (int b = (int) threadIdx.x; b < n; b += 64) s += partial[(size_t) b * SS + ij];
    mbd_wave_sum_store(s, out + ij);
}

// ---- host side, shared by the two engines ----------------------------------------------------------------------------------------

// the check of the edge lengths (those on buffers and indices: edge_check, as in edge_readout)
inline int cross_check_lengths(const char* who, const double* t, int count)
{
    for (int e = 0; e < count; ++e)
        if (!(t[e] >= 0.0) || t[e] > 1.79e308) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "an edge length is negative or not finite");
    return BEAGLE_SUCCESS;
}

// the launches of one call: a.partial holds chunks x nb matrices afterwards.  Returns the number of launches.
template <int LAYOUT, class Real>
inline int launch_cross_products(hipStream_t stream, CrossArgs a, int chunks, bool mfma)
{
    const int S = a.g.S;
    const dim3 grid((unsigned) a.nb, (unsigned) chunks);
    if constexpr (LAYOUT == DERIV_S4) {
        auto kernel = k_cross_products<DERIV_S4, float>;
        MBAMD_LAUNCH(kernel, grid, 64, 0, stream, a);
        return 1;
    } else {
        if constexpr (LAYOUT != DERIV_F64) {
            if (mfma) {
                const size_t lds = cross_lds_bytes<float>(S <= 32 ? 32 : 64);
                if (S <= 32) { auto kernel = k_cross_products_mfma<LAYOUT, 1>; MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a); }
                else { auto kernel = k_cross_products_mfma<LAYOUT, 2>; MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a); }
                return 1;
            }
        }
        auto kernel = k_cross_products<LAYOUT, Real>;
        const size_t lds = cross_lds_bytes<Real>(S);
        if (lds > (size_t) 48 * 1024 && hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            (void) hipGetLastError();
        const int slabs = (S * S + 255) / 256;
        for (a.slab = 0; a.slab < slabs; ++a.slab) MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a);
        return slabs;
    }
}

// beagleCalculateCrossProductDerivative on the engine's patterns: the edge table -- GradEdge and, behind the edges, t_e r_k as
// doubles -- is staged; the edges are cut into chunks (cross_chunks), one launch (the plain kernel beyond 256 entries: one per 256)
// leaves a matrix per (block, chunk) in the result scratch, k_cross_product_sums adds them and S * S doubles come back: out[S * S] is
// overwritten.  Synchronous.  The matrix-core kernel serves 16 .. 64 states in single precision (MBAMD_XPROD_GENERIC: the plain one).
template <class Engine>
inline int cross_products(Engine& e, const int* post, const int* pre, const int* rateIdx, const int* wIdx, const double* lengths, int count, double* out)
{
    const char* const who = "beagleCalculateCrossProductDerivative";
    { const int rc = edge_list_begin(e, who); if (rc) return rc; }
    for (int i = 0; i < count; ++i) {
        const int rc = edge_check(e, who, post[i], pre[i], wIdx[i]);
        if (rc) return rc;
        if (!e.rateSets.has(rateIdx[i])) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "category rates index");
    }
    { const int rc = cross_check_lengths(who, lengths, count); if (rc) return rc; }
    const int S = e.S, K = e.K;
    const size_t SS = (size_t) S * S;
    std::fill_n(out, SS, 0.0);
    if (count <= 0) return BEAGLE_SUCCESS;
    const size_t edgeBytes = (size_t) count * sizeof(GradEdge);
    std::vector<unsigned char> table(edgeBytes + (size_t) count * K * sizeof(double), 0);
    { const int rc = edge_list_fill(e, post, pre, count, reinterpret_cast<GradEdge*>(table.data())); if (rc) return rc; }
    double* const tr = reinterpret_cast<double*>(table.data() + edgeBytes);
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < K; ++k) tr[(size_t) i * K + k] = lengths[i] * e.rateSets[rateIdx[i]].r[k];
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size(), &d_table); if (rc) return rc; }
    const int nb = e.Ppad / 64;
    const int chunks = cross_chunks(count, nb, S);
    CrossArgs a;
    std::memset(&a, 0, sizeof a);
    { const int rc = e.resultScratch(((size_t) chunks * nb + 1) * SS * sizeof(double), &a.partial); if (rc) return rc; }
    a.g = e.layoutArgs();
    a.edges = static_cast<const GradEdge*>(d_table);
    a.tr = reinterpret_cast<const double*>(static_cast<const unsigned char*>(d_table) + edgeBytes);
    a.q = K > 1 ? e.d_q : nullptr;
    a.pattern_weights = e.d_pweights;
    a.nb = nb;
    a.edgeCount = count;
    a.perChunk = (count + chunks - 1) / chunks;
    const int used = (count + a.perChunk - 1) / a.perChunk;          // (the last chunks may be empty: not launched)
    double* const d_out = a.partial + (size_t) used * nb * SS;
    const bool mfma = S >= 16 && S <= 64 && !e.sw.xprodGeneric;
    const int launches = e.withLayout([&](auto L) { return launch_cross_products<L(), deriv_real<L()>>(e.stream, a, used, mfma); });
    MBAMD_LAUNCH(k_cross_product_sums, (unsigned) SS, 64, 0, e.stream, (const double*) a.partial, used * nb, (int) SS, d_out);
    HIP_TRY(hipGetLastError());
    e.countLaunches(launches + 1);
    HIP_TRY(hipStreamSynchronize(e.stream));
    e.afterSync();
    HIP_TRY(hipMemcpy(out, d_out, SS * sizeof(double), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd
#endif
