// mbamd_preorder.h -- the top-down ("pre-order") pass and the gradient of the log-likelihood in ALL branch lengths (upstream BEAGLE 4's
// beagleUpdatePrePartials / beagleSetDifferentialMatrix / beagleCalculateEdgeDerivatives; semantics: include/libhmsbeagle/beagle.h,
// DESIGN 4.4.2).  Included by mbamd_f32.h and mbamd_f64.h; product and TEST-ONLY host emulation compile these same kernels.
//
// pre(n), at the child end of n's branch, is the conditional likelihood of the REST of the tree:
//     tmp[k,c,i]   = pre_parent[k,c,i] * sum_j P_sib,k[i,j] post_sib[k,c,j]         (no sibling: the factor 1)
//     pre_n[k,c,j] = sum_i P_n,k[i,j] tmp[k,c,i]                                    (the transpose)
// so that sum_j pre_n[j] post_n[j] is the category's site likelihood at every node.  Every destination column (pattern, category) is
// brought to [0.5, 1) by its own power of two -- frexp of the column maximum, exact -- and THE EXPONENT IS DISCARDED: per category
//     g_k(c) = (sum_l pre[l] sum_j D_k[l,j] post[j]) / (sum_l pre[l] post[l]),      D_k = r_k Q
// is free of any per-(pattern, category) scale of either buffer, and the derivative of the site log-likelihood in the branch length is
//     d_c = sum_k q_k(c) g_k(c),     q_k(c) = w_k l_k(c) / sum_k' w_k' l_k'(c)
// with q the posterior category probabilities of the pattern -- the same for every branch, computed once per log-likelihood call by
// k_category_posteriors from that call's operands (the L-sum of k_edge_derivatives, per-category exponents recombined).  A category
// whose denominator is zero has underflowed and carries nothing: it is skipped.
//
// Post-order operands may be UNSCALED (a dynamically rescaling client rescales only after an underflow): columns anywhere down to
// 2^-149.  Every kernel here, in mbamd_crossproducts.h, mbamd_posteriors.h and mbamd_derivatives.h therefore takes the own power of
// two out of a post-order column before its first product (pre_exponent / pre_scaled of mbamd_derivatives.h: on the column where a
// kernel stages it, in LDS or in registers, pre_scale4; PostColumn where it is read straight from memory) -- exact, and invisible
// on columns in the normal range.  The ratios drop the exponent; where categories are combined (k_category_posteriors,
// k_edge_derivatives) it joins the category's exponent.  An all-zero column stays a skipped category.
//
// Arithmetic as everywhere: products in the engine's precision (FMA chains over the states, ascending), sums over states and
// categories of the read-outs in double, block sums through mbd_wave_sum_store (fixed order).
//
// The same read with a second differential matrix gives the second derivative beside the first (mbamdCalculateEdgeSecondDerivatives:
// k_edge_readout at order 2, k_edge_second_mfma and edge_readout below).
#ifndef MBAMD_PREORDER_H_
#define MBAMD_PREORDER_H_

#include <math.h>

#include <type_traits>

#include "mbamd_host.h"          // beagle.h, fail / HIP_TRY, <algorithm>, <cstring>, <vector>
#include "mbamd_derivatives.h"

namespace mbamd {

// one pre-order operation in device pointers.  sibKind: 0 post-order partials, 1 compact tip states, -1 no sibling factor
struct PreOp {
    void*       dst;
    const void* parent;
    const void* sib;
    const void* mOwn;
    const void* mSib;
    int         sibKind;
    int         pad_;
};
// g: the layout (S, SP, K, Ppad, pstride, tstride; last = the pattern count).  One launch runs ops[0 .. grid) -- operations that
// neither read nor write what another of them writes.
struct PreArgs {
    DerivArgs    g;
    const PreOp* ops;
};

// one branch of a gradient call
struct GradEdge {
    const void* pre;
    const void* post;             // post-order partials, or compact tip states (postTip)
    const void* D;                // the differential matrix, an ordinary matrix buffer
    int         postTip;
    int         pad_;
};
// the arguments of the read-out kernels of the gradient call (order 1) and of the second-derivative call (order 2)
struct ReadoutArgs {
    DerivArgs          g;
    const GradEdge*    edges;     // the edges of this launch (grid y); D = the first differential matrix
    const void* const* D2;        // order 2: the edges' second differential matrices (they follow the edge table); order 1: not read
    const double*      q;         // [K][Ppad] posterior category probabilities, or null (one category: q = 1)
    const double*      pattern_weights;
    double*            site;      // [edges][Ppad] unweighted d_c (order 2: d1_c), or null: block sums only
    double*            site2;     // order 2: [edges][Ppad] unweighted d2_c, or null; order 1: not read
    double*            sums;      // [2][edges][nb]: weight_c d_c and weight_c d_c^2 (order 2: weight_c d2_c), one per 64-pattern block
    int                nb, edgeCount;
};

// (pre_exponent, pre_scaled and PostColumn, the power of two of a column: mbamd_derivatives.h)

// dynamic LDS of the general kernel: the two matrices [from][to], then two columns [state][thread]
template <class Real> inline size_t pre_lds_bytes(int S) { return ((size_t) 2 * S * S + (size_t) 2 * S * 64) * sizeof(Real); }

// Four states (DERIV_S4): a thread owns a (pattern, category) column -- one f4 load per operand (bitplanes for a tip sibling), both
// 4 x 4 matrices in registers (wave-uniform: a wave is one category of one block), one f4 store; no LDS.  Grid (waves / 4, operations).
// Other layouts: grid (64-pattern blocks, categories, operations), 64 threads; the two matrices of the operation are staged into LDS
// once per workgroup and a thread walks its own column in LDS, [state][thread] (see k_final_pass: as private arrays indexed at run
// time these are scratch).  Threads beyond the last pattern only take part in the barrier.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(LAYOUT == DERIV_S4 ? 256 : 64)
k_pre_partials(PreArgs a)
{
    const DerivArgs& g = a.g;
    if constexpr (LAYOUT == DERIV_S4) {
        const PreOp op = a.ops[blockIdx.y];
        const int wave = (int) blockIdx.x * 4 + mbd_wave_index();
        if (wave >= g.Ppad / 64 * g.K) return;
        const int b = wave / g.K, k = wave - b * g.K, lane = (int) (threadIdx.x & 63u);
        if (b * 64 + lane >= g.last) return;
        const size_t at = (size_t) b * g.pstride + (size_t) k * 64 + lane;
        f4 t = reinterpret_cast<const f4*>(op.parent)[at];
        if (op.sibKind >= 0) {
            float v[4];
            if (op.sibKind == 1) {
                const uint64_t* planes = reinterpret_cast<const uint64_t*>(op.sib) + (size_t) b * g.tstride;
                for (int j = 0; j < 4; ++j) v[j] = (planes[j] >> lane & 1u) ? 1.0f : 0.0f;
            } else {
                const f4 q = reinterpret_cast<const f4*>(op.sib)[at];
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                pre_scale4(v);
            }
            const MBAMD_AS_CONST float* m = as_const(reinterpret_cast<const float*>(op.mSib)) + k * 16;      // m[j * 4 + i] = P(i -> j)
            t.x *= fmaf(m[12], v[3], fmaf(m[8], v[2], fmaf(m[4], v[1], m[0] * v[0])));
            t.y *= fmaf(m[13], v[3], fmaf(m[9], v[2], fmaf(m[5], v[1], m[1] * v[0])));
            t.z *= fmaf(m[14], v[3], fmaf(m[10], v[2], fmaf(m[6], v[1], m[2] * v[0])));
            t.w *= fmaf(m[15], v[3], fmaf(m[11], v[2], fmaf(m[7], v[1], m[3] * v[0])));
        }
        const MBAMD_AS_CONST float* m = as_const(reinterpret_cast<const float*>(op.mOwn)) + k * 16;
        f4 r;
        r.x = fmaf(m[3], t.w, fmaf(m[2], t.z, fmaf(m[1], t.y, m[0] * t.x)));
        r.y = fmaf(m[7], t.w, fmaf(m[6], t.z, fmaf(m[5], t.y, m[4] * t.x)));
        r.z = fmaf(m[11], t.w, fmaf(m[10], t.z, fmaf(m[9], t.y, m[8] * t.x)));
        r.w = fmaf(m[15], t.w, fmaf(m[14], t.z, fmaf(m[13], t.y, m[12] * t.x)));
        const int e = pre_exponent(fmaxf(fmaxf(r.x, r.y), fmaxf(r.z, r.w)));
        r.x = pre_scaled(r.x, e); r.y = pre_scaled(r.y, e); r.z = pre_scaled(r.z, e); r.w = pre_scaled(r.w, e);
        reinterpret_cast<f4*>(op.dst)[at] = r;
    } else {
        const int S = g.S;
        const PreOp op = a.ops[blockIdx.z];
        const int c = (int) blockIdx.x * 64 + (int) threadIdx.x, k = (int) blockIdx.y;
        Real* const mOwn = mbd_dyn_lds<Real>();
        Real* const mSib = mOwn + (size_t) S * S;
        Real* const colA = mSib + (size_t) S * S + threadIdx.x;       // element i of this thread's column: colA[i * 64]
        Real* const colB = colA + (size_t) S * 64;
        for (int e = (int) threadIdx.x; e < S * S; e += 64) {
            // (in storage order: the fp32 engine keeps matrices transposed)
            const int i = LAYOUT == DERIV_F64 ? e / S : e % S, j = LAYOUT == DERIV_F64 ? e % S : e / S;
            mOwn[i * S + j] = deriv_matrix<LAYOUT, Real>(op.mOwn, g, k, i, j);
            if (op.sibKind >= 0) mSib[i * S + j] = deriv_matrix<LAYOUT, Real>(op.mSib, g, k, i, j);
        }
        MBAMD_SYNC();
        if (c >= g.last) return;
        unsigned tip = 0;
        if (op.sibKind == 1) tip = deriv_tip<LAYOUT>(op.sib, g, c);
        else if (op.sibKind == 0) {
            // (the sibling's column with its own power of two taken out, where it lies: mbamd_derivatives.h)
            Real sx = (Real) 0;
            for (int j = 0; j < S; ++j) {
                const Real v = deriv_partial<LAYOUT, Real>(op.sib, g, k, j, c);
                colA[j * 64] = v;
                sx = v > sx ? v : sx;
            }
            const int es = pre_exponent(sx);
            for (int j = 0; j < S; ++j) colA[j * 64] = pre_scaled(colA[j * 64], es);
        }
        for (int i = 0; i < S; ++i) {
            Real f = (Real) 1;
            if (op.sibKind == 1) {
                if (tip < (unsigned) S) f = mSib[i * S + (int) tip];
            } else if (op.sibKind == 0) {
                f = (Real) 0;
                for (int j = 0; j < S; ++j) f = deriv_fma(mSib[i * S + j], colA[j * 64], f);
            }
            colB[i * 64] = deriv_partial<LAYOUT, Real>(op.parent, g, k, i, c) * f;
        }
        Real mx = (Real) 0;
        for (int j = 0; j < S; ++j) {
            Real r = (Real) 0;
            for (int i = 0; i < S; ++i) r = deriv_fma(mOwn[i * S + j], colB[i * 64], r);
            colA[j * 64] = r;
            mx = r > mx ? r : mx;
        }
        const int e = pre_exponent(mx);
        Real* const dst = reinterpret_cast<Real*>(op.dst);
        for (int j = 0; j < S; ++j) {
            const Real r = pre_scaled(colA[j * 64], e);
            if constexpr (LAYOUT == DERIV_F64) dst[((size_t) k * S + j) * (size_t) g.Ppad + c] = r;
            else if constexpr (LAYOUT == DERIV_WG) dst[wg_index(S, g.pstride, k, j, c)] = r;
            else dst[gen_index(g.K, S, k, j, c)] = r;
        }
    }
}

template <bool PER_CATEGORY>
__device__ __forceinline__ int category_exponent(const DerivArgs& a, int k, int c)
{
    return PER_CATEGORY && a.cum != nullptr ? a.cum[(size_t) k * a.Ppad + c] : 0;
}

// q[k][c]: the posterior probability of category k at pattern c under the operands of a log-likelihood call (a: as for
// k_edge_derivatives -- parent, child or null, matrix[0], weights, freqs, cum; site = q, [K][Ppad]).  One thread per pattern.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_category_posteriors(DerivArgs a)
{
    constexpr bool PER_CATEGORY = LAYOUT == DERIV_S4 || LAYOUT == DERIV_WG;
    const int S = a.S, K = a.K;
    const int c = (int) blockIdx.x * 64 + (int) threadIdx.x;
    if (c >= a.last) return;
    // as k_edge_derivatives: the categories meet at the largest exponent among the live ones (the stored one + the powers of two
    // taken out of the two columns); a.site holds the categories' own sums until that exponent is known
    const unsigned tip = a.child_tip ? deriv_tip<LAYOUT>(a.child, a, c) : 0u;
    int emax = 0;
    bool any = false;
    for (int k = 0; k < K; ++k) {
        const PostColumn<LAYOUT, Real> parent(a.parent, a, k, c), child(a.child_tip ? nullptr : a.child, a, k, c);
        double cat = 0.0;
        for (int i = 0; i < S && parent.live && child.live; ++i) {
            Real f = (Real) 1;
            if (a.child != nullptr) {
                if (a.child_tip && LAYOUT != DERIV_S4) {
                    if (tip < (unsigned) S) f = deriv_matrix<LAYOUT, Real>(a.matrix[0], a, k, i, (int) tip);
                } else {
                    f = (Real) 0;
                    for (int j = 0; j < S; ++j) {
                        const Real v = a.child_tip ? ((tip >> j & 1u) ? (Real) 1 : (Real) 0) : child[j];
                        f = deriv_fma(deriv_matrix<LAYOUT, Real>(a.matrix[0], a, k, i, j), v, f);
                    }
                }
            }
            cat += (double) (parent[i] * f) * a.freqs[i];
        }
        a.site[(size_t) k * a.Ppad + c] = cat * a.weights[k];
        if (cat > 0.0) {
            const int E = category_exponent<PER_CATEGORY>(a, k, c) + parent.e + child.e;
            emax = !any || E > emax ? E : emax;
            any = true;
        }
    }
    double L = 0.0;
    for (int k = 0; k < K; ++k) {
        double l = a.site[(size_t) k * a.Ppad + c];
        if (l > 0.0) {
            // (the columns once more, for their powers of two: K integers have no room in registers for every K)
            const PostColumn<LAYOUT, Real> parent(a.parent, a, k, c), child(a.child_tip ? nullptr : a.child, a, k, c);
            l = ldexp(l, category_exponent<PER_CATEGORY>(a, k, c) + parent.e + child.e - emax);
        }
        a.site[(size_t) k * a.Ppad + c] = l;
        L += l;
    }
    for (int k = 0; k < K; ++k) a.site[(size_t) k * a.Ppad + c] = L > 0.0 ? a.site[(size_t) k * a.Ppad + c] / L : 0.0;
}

// d_c of every edge of the launch: grid (64-pattern blocks, edges), one thread per pattern, looping over the categories.  ORDER 2 meets
// every row of D2 with the post-order value the same row of D meets, and its d is the d of ORDER 1, operation for operation.
template <int LAYOUT, class Real, int ORDER>
__global__ void __launch_bounds__(64)
k_edge_readout(ReadoutArgs a)
{
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K;
    const int c = (int) blockIdx.x * 64 + (int) threadIdx.x;
    const GradEdge ed = a.edges[blockIdx.y];
    const void* D2 = nullptr;
    if constexpr (ORDER == 2) D2 = a.D2[blockIdx.y];
    double d = 0.0, d2 = 0.0, pw = 0.0;
    if (c < g.last) {
        const unsigned tip = ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
        for (int k = 0; k < K; ++k) {
            double num = 0.0, num2 = 0.0, den = 0.0;
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
                    if constexpr (ORDER == 2) {
                        const MBAMD_AS_CONST float* m2 = as_const(reinterpret_cast<const float*>(D2)) + k * 16;
                        const float f2 = fmaf(m2[12 + l], v[3], fmaf(m2[8 + l], v[2], fmaf(m2[4 + l], v[1], m2[l] * v[0])));
                        num2 += (double) (p[l] * f2);
                    }
                    den += (double) (p[l] * v[l]);
                }
            } else {
                const PostColumn<LAYOUT, Real> post(ed.postTip ? nullptr : ed.post, g, k, c);
                for (int l = 0; l < S; ++l) {
                    const Real p = deriv_partial<LAYOUT, Real>(ed.pre, g, k, l, c);
                    Real f = (Real) 0, f2 = (Real) 0, v;
                    if (ed.postTip) {
                        // (a missing state is the vector of ones: the rows of a differential matrix sum to zero)
                        v = (tip >= (unsigned) S || tip == (unsigned) l) ? (Real) 1 : (Real) 0;
                        if (tip < (unsigned) S) {
                            f = deriv_matrix<LAYOUT, Real>(ed.D, g, k, l, (int) tip);
                            if constexpr (ORDER == 2) f2 = deriv_matrix<LAYOUT, Real>(D2, g, k, l, (int) tip);
                        }
                    } else {
                        for (int j = 0; j < S; ++j) {
                            const Real x = post[j];
                            f = deriv_fma(deriv_matrix<LAYOUT, Real>(ed.D, g, k, l, j), x, f);
                            if constexpr (ORDER == 2) f2 = deriv_fma(deriv_matrix<LAYOUT, Real>(D2, g, k, l, j), x, f2);
                        }
                        v = post[l];
                    }
                    num += (double) (p * f);
                    if constexpr (ORDER == 2) num2 += (double) (p * f2);
                    den += (double) (p * v);
                }
            }
            if (den > 0.0) {
                const double qk = a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0;
                d += qk * (num / den);
                if constexpr (ORDER == 2) d2 += qk * (num2 / den);
            }
        }
        if constexpr (ORDER == 2) d2 -= d * d;
        if (a.site != nullptr) a.site[(size_t) blockIdx.y * g.Ppad + c] = d;
        if constexpr (ORDER == 2) { if (a.site2 != nullptr) a.site2[(size_t) blockIdx.y * g.Ppad + c] = d2; }
        pw = a.pattern_weights[c];
    }
    mbd_wave_sum_store(pw * d, a.sums + (size_t) blockIdx.y * a.nb + blockIdx.x);
    mbd_wave_sum_store(ORDER == 2 ? pw * d2 : pw * d * d, a.sums + ((size_t) a.edgeCount + blockIdx.y) * a.nb + blockIdx.x);
}

// out[q * edges + e] = the sum of the nb block sums of (q, e), in a fixed order: grid (edges, 2), one wave each
__global__ void __launch_bounds__(64)
k_gradient_sums(const double* __restrict__ sums, int nb, int edges, double* __restrict__ out)
{
    const size_t row = (size_t) blockIdx.y * edges + blockIdx.x;
    double s = 0.0;
    for (int b = (int) threadIdx.x; b < nb; b += 64) s += sums[row * nb + b];
    mbd_wave_sum_store(s, out + row);
}

// ---- first AND second derivative of every branch (mbamdCalculateEdgeSecondDerivatives; semantics: beagle.h) --------
// With a second differential matrix D2_k (r_k^2 Q^2 for a branch length) beside D1_k, per category
//     g1_k(c), g2_k(c) = (sum_l pre[l] sum_j D1_k / D2_k [l,j] post[j]) / (sum_l pre[l] post[l])
// from ONE read of the two columns, and
//     d1_c = sum_k q_k(c) g1_k(c),     d2_c = sum_k q_k(c) g2_k(c) - d1_c^2
// The plain kernel is k_edge_readout at ORDER 2.  A compact tip with a missing state: the vector of ones in the denominator and
// nothing in either numerator (the rows of a differential matrix sum to zero) where the layout stores state codes; the four-state
// bitplanes add the compatible columns.

// dynamic LDS of the matrix-core kernel: the post-order and the pre-order column of the block, [state][thread], 32 TILES rows each
inline size_t second_lds_bytes(int tiles) { return (size_t) 2 * 32 * tiles * 64 * sizeof(float); }

// 16 .. 64 states on the fp32 engine: grid (64-pattern blocks, edges), one wave per workgroup, ONE EDGE per workgroup (the two
// matrices change with the edge and the category, so a wave that looped over edges would keep nothing but its sums; see DESIGN
// 4.4.6 for the register and LDS budget).  Per category the wave stages its 64 patterns' columns (thread = pattern; den is summed
// there, in k_edge_readout's order) and forms F1 = D1 post, F2 = D2 post, 32 TILES states x 64 patterns each, with
// mbd_mfma_f32_32x32x2: row tiles hold states, the two column tiles patterns 0 .. 31 and 32 .. 63, the reduction runs over the
// post-order state j, two per instruction -- lane l feeds A[l & 31][l >> 5] = D(32 rt + (l & 31) -> 2 s + (l >> 5)), read from the
// matrix buffer where it lies (zero beyond S), and B[l >> 5][l & 31] = post[2 s + (l >> 5)][pattern 32 ct + (l & 31)] from LDS.
// 4 TILES independent accumulators.  Then lane l holds, of column 32 ct + (l & 31), the rows (r & 3) + 8 (r >> 2) + 4 (l >> 5) of
// every row tile (mbd_mfma_f32_32x32x2's layout): it multiplies them with the pre-order column from LDS, adds the products in
// double, the two half-waves of a column are joined by mbd_shfl_xor(., 32), and lane l takes the column of ITS pattern.
template <int LAYOUT, int TILES>
__global__ void __launch_bounds__(64)
k_edge_second_mfma(ReadoutArgs a)
{
    constexpr int ROWS = 32 * TILES;
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K, lane = (int) threadIdx.x, half = lane >> 5, col = lane & 31;
    const int c = (int) blockIdx.x * 64 + lane;
    const bool live = c < g.last;
    const GradEdge ed = a.edges[blockIdx.y];
    const void* const D2 = a.D2[blockIdx.y];
    float* const post = mbd_dyn_lds<float>() + lane;          // element j of this thread's column: post[j * 64]
    float* const pre = post + (size_t) ROWS * 64;
    const float* const readPost = mbd_dyn_lds<float>() + half * 64 + col;
    const float* const readPre = mbd_dyn_lds<float>() + (size_t) ROWS * 64 + col;
    const unsigned tip = live && ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
    // (a reduction index beyond S meets a zero of the matrix: the column holds a zero there too, not whatever LDS held)
    if (S & 1) post[S * 64] = 0.0f;
    if (!live) for (int l = 0; l < S; ++l) { post[l * 64] = 0.0f; pre[l * 64] = 0.0f; }
    double d = 0.0, d2 = 0.0;
    for (int k = 0; k < K; ++k) {
        double den = 0.0;
        if (live) {
            float mx = 0.0f;
            // (sixteen states at a time, as cross_stage: their loads are issued together)
            for (int l0 = 0; l0 < S; l0 += 16) {
                float p[16], v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int l = l0 + u < S ? l0 + u : S - 1;
                    p[u] = deriv_partial<LAYOUT, float>(ed.pre, g, k, l, c);
                    if (ed.postTip) v[u] = (tip >= (unsigned) S || tip == (unsigned) l) ? 1.0f : 0.0f;
                    else v[u] = deriv_partial<LAYOUT, float>(ed.post, g, k, l, c);
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    if (l0 + u < S) {
                        pre[(l0 + u) * 64] = p[u];
                        post[(l0 + u) * 64] = (ed.postTip && tip >= (unsigned) S) ? 0.0f : v[u];
                        if (ed.postTip) den += (double) (p[u] * v[u]);
                        mx = v[u] > mx ? v[u] : mx;
                    }
                }
            }
            if (!ed.postTip) {
                // (the post-order column's own power of two goes out where it lies, before its first product, as in cross_stage)
                const int ev = pre_exponent(mx);
                for (int l = 0; l < S; ++l) {
                    const float v = pre_scaled(post[l * 64], ev);
                    post[l * 64] = v;
                    den += (double) (pre[l * 64] * v);
                }
            }
        }
        MBAMD_SYNC();
        mbd_acc16 acc1[TILES][2], acc2[TILES][2];
#pragma unroll
        for (int rt = 0; rt < TILES; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) { acc1[rt][ct] = (mbd_acc16) (0.0f); acc2[rt][ct] = (mbd_acc16) (0.0f); }
        for (int s = 0; 2 * s < S; ++s) {
            const int j = 2 * s + half;
            const float b0 = readPost[2 * s * 64], b1 = readPost[2 * s * 64 + 32];
#pragma unroll
            for (int rt = 0; rt < TILES; ++rt) {
                const int l = 32 * rt + col;
                const bool in = l < S && j < S;
                const float x1 = in ? deriv_matrix<LAYOUT, float>(ed.D, g, k, l, j) : 0.0f;
                const float x2 = in ? deriv_matrix<LAYOUT, float>(D2, g, k, l, j) : 0.0f;
                acc1[rt][0] = mbd_mfma_f32_32x32x2(x1, b0, acc1[rt][0]);
                acc1[rt][1] = mbd_mfma_f32_32x32x2(x1, b1, acc1[rt][1]);
                acc2[rt][0] = mbd_mfma_f32_32x32x2(x2, b0, acc2[rt][0]);
                acc2[rt][1] = mbd_mfma_f32_32x32x2(x2, b1, acc2[rt][1]);
            }
        }
        double n1[2] = {0.0, 0.0}, n2[2] = {0.0, 0.0};
#pragma unroll
        for (int rt = 0; rt < TILES; ++rt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < S) {
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const float p = readPre[row * 64 + 32 * ct];
                        n1[ct] += (double) (acc1[rt][ct][r] * p);
                        n2[ct] += (double) (acc2[rt][ct][r] * p);
                    }
                }
            }
        }
        MBAMD_SYNC();
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) { n1[ct] += mbd_shfl_xor(n1[ct], 32); n2[ct] += mbd_shfl_xor(n2[ct], 32); }
        const double num = half ? n1[1] : n1[0], num2 = half ? n2[1] : n2[0];
        if (live && den > 0.0) {
            const double qk = a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0;
            d += qk * (num / den);
            d2 += qk * (num2 / den);
        }
    }
    double pw = 0.0;
    if (live) {
        d2 -= d * d;
        if (a.site != nullptr) a.site[(size_t) blockIdx.y * g.Ppad + c] = d;
        if (a.site2 != nullptr) a.site2[(size_t) blockIdx.y * g.Ppad + c] = d2;
        pw = a.pattern_weights[c];
    }
    mbd_wave_sum_store(pw * d, a.sums + (size_t) blockIdx.y * a.nb + blockIdx.x);
    mbd_wave_sum_store(pw * d2, a.sums + ((size_t) a.edgeCount + blockIdx.y) * a.nb + blockIdx.x);
}

// ---- host side, shared by the two engines ----------------------------------------------------------------------------------------
// The calls are written once, as templates on the engine (Instance, Engine64).  They read its members of the same name -- the sizes
// S, K, P, Ppad, nBuffers, nMatrices, nScale, stream, valid, preOrder, lastLnl, qStamp, d_q, d_pweights, rateSets, sw, secondLaunches, insertionLaunches, layoutArgs(),
// partialsPtr(), matrixPtr() -- and ask it for the rest through a few small hooks, which each engine keeps in one block:
//     runQueued, refuses                  before anything else: what is queued or held runs; an instance the calls do not serve
//     holdsTip, readable, operandPtr      a buffer holds compact tip states / something to read; where that is
//     beforeRead, beforeWrite, afterWrite around the partials buffers of a call
//     stageTable, resultScratch           device memory for the call's table and for its results
//     afterSync, countLaunches            bookkeeping
//     timedBegin, timedEnd                an event pair around a call's launches while kernel timing is on (the sampling call)
//     withLayout                          f(layout as a compile-time constant)
//     posteriorOperands                   the checked operands of the latest log-likelihood call
//     cumulativeExponents                 a scale buffer's cumulative exponents as a kernel reads them (the insertion call of mbamd_insertions.h)
//     siteLogLikelihoods, weightsMirror   its site log-likelihoods where a kernel can read them; the host copy of the category weights
//                                         (the site-order HMM of mbamd_autocorrelated.h)

// the arithmetic type of a layout
template <int LAYOUT> using deriv_real = std::conditional_t<LAYOUT == DERIV_F64, double, float>;

// What an engine remembers of its latest beagleCalculate{Root,Edge}LogLikelihoods call (integers only): the operands q is made of.
struct LnlOperands {
    uint64_t stamp = 0;           // bumped by every such call
    int count = 0;                // its subset count (0: no call yet)
    int parent = -1, child = -1, prob = -1, weights = -1, freqs = -1, cum = -1;      // of subset 0 (child < 0: a root call)
    void remember(const int* p, const int* ch, const int* pr, const int* w, const int* f, const int* cu, int n)
    {
        ++stamp;
        count = n;
        parent = p[0]; child = ch ? ch[0] : -1; prob = ch ? pr[0] : -1; weights = w[0]; freqs = f[0]; cum = cu ? cu[0] : -1;
    }
};

// A pre-order list cut into launches: start[g] .. start[g + 1] are the operations of launch g.  A new launch begins where an operation
// reads or writes a buffer the current launch writes, or writes a buffer the current launch reads.
inline void pre_order_groups(const BeagleOperation* ops, int n, int nBuffers, std::vector<int>& start)
{
    const int maxOps = 32768;                    // (the operation index is a grid dimension)
    std::vector<char> reads((size_t) nBuffers, 0), writes((size_t) nBuffers, 0);
    start.assign(1, 0);
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        const int d = b.destinationPartials, p = b.child1Partials, s = b.child2Partials;
        const bool cut = writes[p] || (s >= 0 && writes[s]) || writes[d] || reads[d] || o - start.back() >= maxOps;
        if (cut && o > start.back()) {
            std::fill(reads.begin(), reads.end(), 0);
            std::fill(writes.begin(), writes.end(), 0);
            start.push_back(o);
        }
        reads[p] = 1;
        if (s >= 0) reads[s] = 1;
        writes[d] = 1;
    }
    start.push_back(n);
}

template <int LAYOUT, class Real>
inline void launch_pre_partials(hipStream_t stream, const PreArgs& a, int count)
{
    auto kernel = k_pre_partials<LAYOUT, Real>;
    if constexpr (LAYOUT == DERIV_S4) {
        const unsigned waves = (unsigned) (a.g.Ppad / 64 * a.g.K);
        MBAMD_LAUNCH(kernel, dim3((waves + 3) / 4, (unsigned) count), 256, 0, stream, a);
    } else {
        const size_t lds = pre_lds_bytes<Real>(a.g.S);
        if (lds > (size_t) 48 * 1024 && hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            (void) hipGetLastError();
        MBAMD_LAUNCH_BARRIER(kernel, dim3((unsigned) (a.g.Ppad / 64), (unsigned) a.g.K, (unsigned) count), 64, lds, stream, a);
    }
}

// beagleUpdatePrePartials: the list is checked as a whole, cut into launches (pre_order_groups) and run, one launch per group.
template <class Engine>
inline int update_pre_partials(Engine& e, const BeagleOperation* ops, int n, int cumIdx)
{
    { const int rc = e.runQueued(); if (rc) return rc; }
    if (n <= 0) return BEAGLE_SUCCESS;
    { const int rc = e.refuses("beagleUpdatePrePartials"); if (rc) return rc; }
    if (cumIdx != BEAGLE_OP_NONE) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleUpdatePrePartials: pre-order buffers are always self-normalised (cumulativeScaleIndex must be BEAGLE_OP_NONE)");
    const int nBuffers = e.nBuffers, nMatrices = e.nMatrices;
    std::vector<char> written((size_t) nBuffers, 0);
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        if (b.destinationScaleWrite != BEAGLE_OP_NONE || b.destinationScaleRead != BEAGLE_OP_NONE)
            return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleUpdatePrePartials: pre-order buffers are always self-normalised (scale indices must be BEAGLE_OP_NONE)");
        const int d = b.destinationPartials, p = b.child1Partials, sib = b.child2Partials;
        if (d < 0 || d >= nBuffers || p < 0 || p >= nBuffers || (sib != BEAGLE_OP_NONE && (sib < 0 || sib >= nBuffers)))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: partials index");
        if (b.child1TransitionMatrix < 0 || b.child1TransitionMatrix >= nMatrices ||
            (sib != BEAGLE_OP_NONE && (b.child2TransitionMatrix < 0 || b.child2TransitionMatrix >= nMatrices)))
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: matrix index");
        // (a destination never holds tip states, so neither does a buffer this list has written)
        if (e.holdsTip(d)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: the destination holds compact tip states");
        if (e.holdsTip(p) || (!e.valid[p] && !written[p])) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: the parent's pre-order buffer holds no partials");
        if (sib != BEAGLE_OP_NONE && !e.readable(sib) && !written[sib])
            return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: the sibling's buffer was never written");
        if (d == p || d == sib) return fail(BEAGLE_ERROR_OUT_OF_RANGE, "beagleUpdatePrePartials: the destination is an operand");
        written[d] = 1;
    }
    { const int rc = e.beforeRead(2 * n, [&](int i) { return i & 1 ? ops[i / 2].child2Partials : ops[i / 2].child1Partials; }); if (rc) return rc; }
    std::vector<PreOp> table((size_t) n);
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        const int rc = e.beforeWrite(b.destinationPartials);
        if (rc) return rc;
        PreOp& t = table[(size_t) o];
        std::memset(&t, 0, sizeof t);
        t.dst = e.partialsPtr(b.destinationPartials);
        t.parent = e.partialsPtr(b.child1Partials);
        t.mOwn = e.matrixPtr(b.child1TransitionMatrix);
        t.sibKind = -1;
        if (b.child2Partials != BEAGLE_OP_NONE) {
            t.sibKind = e.holdsTip(b.child2Partials) ? 1 : 0;
            t.sib = e.operandPtr(b.child2Partials);
            t.mSib = e.matrixPtr(b.child2TransitionMatrix);
        }
    }
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size() * sizeof(PreOp), &d_table); if (rc) return rc; }
    if (e.preOrder.size() != (size_t) nBuffers) e.preOrder.assign((size_t) nBuffers, 0);
    std::vector<int> start;
    pre_order_groups(ops, n, nBuffers, start);
    PreArgs a;
    a.g = e.layoutArgs();
    for (size_t gI = 0; gI + 1 < start.size(); ++gI) {
        a.ops = static_cast<const PreOp*>(d_table) + start[gI];
        const int count = start[gI + 1] - start[gI];
        e.withLayout([&](auto L) { launch_pre_partials<L(), deriv_real<L()>>(e.stream, a, count); });
        HIP_TRY(hipGetLastError());
        e.countLaunches(1);
    }
    for (int o = 0; o < n; ++o) {
        const int d = ops[o].destinationPartials;
        e.valid[d] = 1;
        e.preOrder[d] = 1;
        e.afterWrite(d);
    }
    return BEAGLE_SUCCESS;
}

// q [K][Ppad] of the latest log-likelihood call's operands as they are now, unless d_q holds it already
template <class Engine>
inline int ensure_posteriors(Engine& e)
{
    if (e.qStamp == e.lastLnl.stamp && e.d_q) return BEAGLE_SUCCESS;
    DerivArgs a;
    { const int rc = e.posteriorOperands(a); if (rc) return rc; }
    a.site = e.d_q;
    e.withLayout([&](auto L) {
        auto kernel = k_category_posteriors<L(), deriv_real<L()>>;
        MBAMD_LAUNCH(kernel, (unsigned) (e.Ppad / 64), 64, 0, e.stream, a);
    });
    HIP_TRY(hipGetLastError());
    e.qStamp = e.lastLnl.stamp;
    return BEAGLE_SUCCESS;
}

// What the calls over a list of (post, pre) edges share -- the gradient below, the cross products of mbamd_crossproducts.h.
// Before the list is looked at:
template <class Engine>
inline int edge_list_begin(Engine& e, const char* who)
{
    { const int rc = e.runQueued(); if (rc) return rc; }
    { const int rc = e.refuses(who); if (rc) return rc; }
    if (e.K > 1) {
        if (e.lastLnl.count == 0) return fail(BEAGLE_ERROR_GENERAL, who, "no log-likelihood was calculated yet: the category posteriors come from its operands");
        if (e.lastLnl.count > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "the latest log-likelihood call had more than one subset");
    }
    return BEAGLE_SUCCESS;
}
// ... the checks of one edge, in front of the call's own:
template <class Engine>
inline int edge_check(const Engine& e, const char* who, int post, int pre, int wIdx)
{
    if (e.K > 1 && wIdx != e.lastLnl.weights) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "category weights index differs from the latest log-likelihood call's");
    if (pre < 0 || pre >= e.nBuffers || (size_t) pre >= e.preOrder.size() || !e.preOrder[pre])
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a pre-order index names a buffer that no pre-order operation wrote (or that was overwritten since)");
    if (post < 0 || post >= e.nBuffers || !e.readable(post)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "post-order buffer");
    return BEAGLE_SUCCESS;
}
// ... and once the list is good: its buffers are in memory, q is that of the latest log-likelihood call, the edges are in `table`
template <class Engine>
inline int edge_list_fill(Engine& e, const int* post, const int* pre, int count, GradEdge* table)
{
    { const int rc = e.beforeRead(2 * count, [&](int i) { return i < count ? post[i] : pre[i - count]; }); if (rc) return rc; }
    if (e.K > 1) { const int rc = ensure_posteriors(e); if (rc) return rc; }
    for (int i = 0; i < count; ++i) {
        std::memset(&table[i], 0, sizeof table[i]);
        table[i].pre = e.partialsPtr(pre[i]);
        table[i].postTip = e.holdsTip(post[i]) ? 1 : 0;
        table[i].post = e.operandPtr(post[i]);
    }
    return BEAGLE_SUCCESS;
}

// ---- the chunked read-out: the gradient and second-derivative call below, the node posteriors of mbamd_posteriors.h ---------------
// Such a call answers, per item of its list (an edge, a node), with rows of [Ppad] per-pattern values, if asked for, and with
// weighted sums over the patterns.  The items pass through the device in chunks; per chunk the call's own read-out kernel leaves the
// per-pattern rows and one block sum per sum row and 64-pattern block, k_gradient_sums adds the block sums, and the chunk's
// results come back.  Synchronous.

// one per-pattern output: `rows` rows of [Ppad] values of `elem` bytes (at most a double's) per item, staged [item][row][Ppad]
struct ReadoutSites {
    int    rows;
    size_t elem;
};
// what a call stages per item: siteCount per-pattern outputs, and block sums [sumPlanes][items][sumRows][nb]
struct ReadoutShape {
    ReadoutSites site[3];
    int          siteCount;
    int          sumPlanes, sumRows;
    int          cap;             // > 0 (MBAMD_POSTERIOR_NODES, test only): at most that many items per chunk
};
// items first .. first + count of the list as the launch of their chunk sees them (device memory: site[s] to fill, sums = the block
// sums to fill) and, afterwards, its scatter (the host's copy: sums = the sums, [sumPlanes][count][sumRows])
struct ReadoutChunk {
    int     first, count;
    void*   site[3];              // in the order of ReadoutShape::site
    double* sums;
};

// items per chunk: the staging behind one launch (`per` doubles per item: per-pattern rows, block sums, sums) stays within 4 Mi doubles
inline int readout_chunk(int count, size_t per, int cap)
{
    size_t n = std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t) count, 32768), ((size_t) 4 << 20) / per));
    if (cap > 0) n = std::min<size_t>(n, (size_t) cap);
    return (int) n;
}

// launch(chunk) enqueues the read-out kernel of a chunk, scatter(chunk, i) takes the results of its item i to the caller's arrays
template <class Engine, class Launch, class Scatter>
inline int chunked_readout(Engine& e, int count, const ReadoutShape& shape, Launch&& launch, Scatter&& scatter)
{
    const size_t Ppad = (size_t) e.Ppad, nb = Ppad / 64, sumRows = (size_t) shape.sumPlanes * shape.sumRows;
    size_t siteRows = 0;
    for (int s = 0; s < shape.siteCount; ++s) siteRows += (size_t) shape.site[s].rows;
    const int chunk = readout_chunk(count, sumRows * nb + sumRows + siteRows * Ppad, shape.cap);
    const size_t nSite = (size_t) chunk * siteRows * Ppad, nBlock = (size_t) chunk * sumRows * nb, nOut = (size_t) chunk * sumRows;
    double* d_site = nullptr;
    { const int rc = e.resultScratch((nSite + nBlock + nOut) * sizeof(double), &d_site); if (rc) return rc; }
    double* const d_out = d_site + nSite + nBlock;
    std::vector<double> h(nSite + nOut);
    ReadoutChunk dev, host;
    size_t at = 0;
    for (int s = 0; s < shape.siteCount; ++s) {
        dev.site[s] = d_site + at;
        host.site[s] = h.data() + at;
        at += (size_t) chunk * shape.site[s].rows * Ppad;         // (a narrower element in the room of a double)
    }
    dev.sums = d_site + nSite;
    host.sums = h.data() + nSite;
    for (int first = 0; first < count; first += chunk) {
        const int n = std::min(chunk, count - first);
        dev.first = host.first = first;
        dev.count = host.count = n;
        launch(dev);
        MBAMD_LAUNCH(k_gradient_sums, dim3((unsigned) (n * shape.sumRows), (unsigned) shape.sumPlanes), 64, 0, e.stream, (const double*) dev.sums,
                     (int) nb, n * shape.sumRows, d_out);
        HIP_TRY(hipGetLastError());
        e.countLaunches(2);
        HIP_TRY(hipStreamSynchronize(e.stream));
        e.afterSync();
        for (int s = 0; s < shape.siteCount; ++s)
            HIP_TRY(hipMemcpy(host.site[s], dev.site[s], (size_t) n * shape.site[s].rows * Ppad * shape.site[s].elem, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(host.sums, d_out, (size_t) n * sumRows * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) scatter(host, i);
    }
    return BEAGLE_SUCCESS;
}

// the read-out launch of one chunk of edges; returns whether the matrix-core kernel took it
template <int LAYOUT, class Real, int ORDER>
inline bool launch_edge_readout(hipStream_t stream, const ReadoutArgs& a, bool mfma)
{
    const dim3 grid((unsigned) a.nb, (unsigned) a.edgeCount);
    if constexpr (ORDER == 2 && (LAYOUT == DERIV_WG || LAYOUT == DERIV_LEVELS)) {
        if (mfma) {
            const int tiles = a.g.S <= 32 ? 1 : 2;
            const size_t lds = second_lds_bytes(tiles);
            if (tiles == 1) { auto kernel = k_edge_second_mfma<LAYOUT, 1>; MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a); }
            else { auto kernel = k_edge_second_mfma<LAYOUT, 2>; MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a); }
            return true;
        }
    }
    auto kernel = k_edge_readout<LAYOUT, Real, ORDER>;
    MBAMD_LAUNCH(kernel, grid, 64, 0, stream, a);
    return false;
}

// beagleCalculateEdgeDerivatives (dmat2 null: order 1) and mbamdCalculateEdgeSecondDerivatives (order 2) on the engine's patterns,
// through chunked_readout.  The read-out kernel is k_edge_readout at that order, or at order 2, for 16 .. 64 states in single
// precision, k_edge_second_mfma (MBAMD_CURV_GENERIC: the plain one); the engine's secondLaunches[0 / 1] count the order-2 launches
// of the plain and of the matrix-core kernel.  sums1[i] is the weighted sum of d_c of edge i, sums2[i] that of d_c^2 (order 1) or of
// d2_c (order 2); sites1 (or null) takes d_c of edge i at [i * siteStride + c], sites2 (or null; order 2) d2_c.
template <class Engine>
inline int edge_readout(Engine& e, const int* post, const int* pre, const int* dmat1, const int* dmat2, const int* wIdx, int count,
                        double* sites1, double* sites2, size_t siteStride, double* sums1, double* sums2)
{
    const char* const who = dmat2 ? "mbamdCalculateEdgeSecondDerivatives" : "beagleCalculateEdgeDerivatives";
    { const int rc = edge_list_begin(e, who); if (rc) return rc; }
    for (int i = 0; i < count; ++i) {
        const int rc = edge_check(e, who, post[i], pre[i], wIdx[i]);
        if (rc) return rc;
        if (dmat1[i] < 0 || dmat1[i] >= e.nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "differential matrix index");
        if (dmat2 && (dmat2[i] < 0 || dmat2[i] >= e.nMatrices)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "second differential matrix index");
    }
    if (count <= 0) return BEAGLE_SUCCESS;
    // the table: the edges, then (order 2) their second matrices
    const size_t edgeBytes = (size_t) count * sizeof(GradEdge);
    std::vector<unsigned char> table(edgeBytes + (dmat2 ? (size_t) count * sizeof(void*) : 0), 0);
    GradEdge* const edges = reinterpret_cast<GradEdge*>(table.data());
    { const int rc = edge_list_fill(e, post, pre, count, edges); if (rc) return rc; }
    const void** const second = reinterpret_cast<const void**>(table.data() + edgeBytes);
    for (int i = 0; i < count; ++i) {
        edges[i].D = e.matrixPtr(dmat1[i]);
        if (dmat2) second[i] = e.matrixPtr(dmat2[i]);
    }
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size(), &d_table); if (rc) return rc; }
    ReadoutShape shape = {};
    if (sites1) shape.site[shape.siteCount++] = {1, sizeof(double)};
    if (sites2) shape.site[shape.siteCount++] = {1, sizeof(double)};
    shape.sumPlanes = 2;
    shape.sumRows = 1;
    ReadoutArgs a;
    a.g = e.layoutArgs();
    a.q = e.K > 1 ? e.d_q : nullptr;
    a.pattern_weights = e.d_pweights;
    a.nb = e.Ppad / 64;
    const bool mfma = e.S >= 16 && e.S <= 64 && !e.sw.curvGeneric;
    const size_t P = (size_t) e.P;
    return chunked_readout(e, count, shape,
        [&](const ReadoutChunk& ch) {
            a.edges = static_cast<const GradEdge*>(d_table) + ch.first;
            a.D2 = dmat2 ? reinterpret_cast<const void* const*>(static_cast<const unsigned char*>(d_table) + edgeBytes) + ch.first : nullptr;
            a.edgeCount = ch.count;
            a.site = sites1 ? static_cast<double*>(ch.site[0]) : nullptr;
            a.site2 = sites2 ? static_cast<double*>(ch.site[sites1 ? 1 : 0]) : nullptr;
            a.sums = ch.sums;
            if (dmat2) {
                const bool core = e.withLayout([&](auto L) { return launch_edge_readout<L(), deriv_real<L()>, 2>(e.stream, a, mfma); });
                ++e.secondLaunches[core ? 1 : 0];
            } else {
                e.withLayout([&](auto L) { launch_edge_readout<L(), deriv_real<L()>, 1>(e.stream, a, false); });
            }
        },
        [&](const ReadoutChunk& ch, int i) {
            const size_t to = (size_t) (ch.first + i), from = (size_t) i * e.Ppad;
            if (sites1) std::memcpy(sites1 + to * siteStride, static_cast<const double*>(ch.site[0]) + from, P * sizeof(double));
            if (sites2) std::memcpy(sites2 + to * siteStride, static_cast<const double*>(ch.site[sites1 ? 1 : 0]) + from, P * sizeof(double));
            if (sums1) sums1[to] = ch.sums[i];
            if (sums2) sums2[to] = ch.sums[(size_t) ch.count + i];
        });
}

}  // namespace mbamd
#endif
