// mbamd_derivatives.h -- first and second derivative of the edge log-likelihood in the branch length (BEAGLE's
// beagleCalculateEdgeLogLikelihoods with derivative arguments; what a Newton step on one branch, or a gradient-based branch-length
// proposal, asks for).  Included by mbamd_f32.h and mbamd_f64.h; product and TEST-ONLY host emulation compile this same kernel.
//
// Per pattern c, over the two ends of one branch (parent partials, child partials or compact tip), with P, P' = dP/dt and
// P'' = d2P/dt2 of that branch in three ordinary matrix buffers (the ORDER 0 / 1 / 2 jobs of the matrix kernels):
//     L_c  = sum_k w_k sum_i pi_i parent[k,c,i] sum_j P_k [i,j] child[k,c,j]
//     D1_c = the same with P'_k,   D2_c = the same with P''_k
//     lnL_c = log L_c (+ the cumulative exponents),   d1_c = D1_c / L_c,   d2_c = D2_c / L_c - d1_c^2
// One pass: the child's values are loaded once and meet the three matrices together.  The arithmetic is the plain integration
// kernels' (k_integrate_lnl, k_integrate_lnl_s4, k_integrate_lnl_wg_wide, k64_integrate): the matrix-vector product in the engine's
// own precision (fp32 FMA chain over j, ascending; fp64 on the double-precision engine), every sum over states and categories in
// double.  Scale factors cancel in the two ratios.  Both columns of a category are read with their own power of two taken out
// (PostColumn below: unscaled operands may lie anywhere down to 2^-149), and the three sums are recombined with the same
// 2^(E_k - E_max) factors, E_k = the exponent a layout keeps per (pattern, category), if it keeps one, + the two powers taken out.  A compact tip selects matrix columns: a missing state is the factor 1 for
// P and 0 for its derivatives (the rows of P sum to one) on the layouts that store state codes; the four-state bitplanes add the
// compatible columns, as the plain kernel does.
//
// One thread per pattern, 64 per workgroup, one workgroup per 64-pattern block: this is a read-out, not a throughput kernel.
// site[0 / 1 / 2][c] = lnL_c, d1_c, d2_c;  sums[0 / 1 / 2][block] = the block's weighted sums (mbd_wave_sum_store: fixed order).
#ifndef MBAMD_DERIVATIVES_H_
#define MBAMD_DERIVATIVES_H_

#include "mbamd_kernels.h"

namespace mbamd {

// partials layouts (the first three are k_export_partials'): 0 level kernels, tile-major (with or without the MFMA copy of the
// matrices: the partials are the same); 1 four-state float4 blocks, tips as bitplanes; 2 tree-walk tiles; 3 double-precision engine
enum DerivLayout { DERIV_LEVELS = 0, DERIV_S4 = 1, DERIV_WG = 2, DERIV_F64 = 3 };

struct DerivArgs {
    const void*    parent;
    const void*    child;            // partials, or compact tip states (child_tip): bitplanes of block 0 (layout 1) / state codes
    const void*    matrix[3];        // P, P', P'' (matrix[2] may be null: first derivative only)
    const double*  weights;          // K category weights
    const double*  freqs;            // S state frequencies
    const int32_t* cum;              // cumulative exponents ([K][Ppad] on layouts 1 and 2, [Ppad] otherwise) or null
    const double*  pattern_weights;
    double*        site;             // [3][Ppad]
    double*        sums;             // [3][sumStride]
    size_t         pstride;          // layout 1: f4 elements between blocks; layout 2: floats between tiles
    unsigned       tstride;          // layout 1: uint64 between the blocks of the bitplanes; layout 2: bytes between the tiles of the tip states
    int            child_tip;
    int            S, SP, K, Ppad;
    int            first, last;      // patterns [first, last): blocks are counted from the one that holds `first`
    int            sumStride;
};

template <int LAYOUT, class Real>
__device__ __forceinline__ Real deriv_partial(const void* buf, const DerivArgs& a, int k, int i, int c)
{
    if constexpr (LAYOUT == DERIV_F64) return reinterpret_cast<const Real*>(buf)[((size_t) k * a.S + i) * (size_t) a.Ppad + c];
    else if constexpr (LAYOUT == DERIV_S4) return reinterpret_cast<const Real*>(buf)[(blk_index(c, a.pstride) + (size_t) k * 64) * 4 + i];
    else if constexpr (LAYOUT == DERIV_WG) return reinterpret_cast<const Real*>(buf)[wg_index(a.S, a.pstride, k, i, c)];
    else return reinterpret_cast<const Real*>(buf)[gen_index(a.K, a.S, k, i, c)];
}
// P_k(i -> j) of a matrix buffer: fp32 engine [K][SP][SP] transposed, double-precision engine [K][S][S]
template <int LAYOUT, class Real>
__device__ __forceinline__ Real deriv_matrix(const void* m, const DerivArgs& a, int k, int i, int j)
{
    if constexpr (LAYOUT == DERIV_F64) return reinterpret_cast<const Real*>(m)[((size_t) k * a.S + i) * a.S + j];
    else return reinterpret_cast<const Real*>(m)[(size_t) k * a.SP * a.SP + (size_t) j * a.SP + i];
}

// the compact tip of pattern c: a mask of compatible states (four-state bitplanes) or a state code (>= S: missing)
template <int LAYOUT>
__device__ __forceinline__ unsigned deriv_tip(const void* states, const DerivArgs& a, int c)
{
    if constexpr (LAYOUT == DERIV_S4) {
        const uint64_t* planes = reinterpret_cast<const uint64_t*>(states) + (size_t) (c >> 6) * a.tstride;
        unsigned tip = 0;
        for (int i = 0; i < 4; ++i) tip |= (unsigned) (planes[i] >> (c & 63) & 1u) << i;
        return tip;
    } else if constexpr (LAYOUT == DERIV_WG) {
        return reinterpret_cast<const uint8_t*>(states)[(size_t) (c / MBAMD_WG_TW) * a.tstride + (c % MBAMD_WG_TW)];
    } else {
        return reinterpret_cast<const uint8_t*>(states)[c];
    }
}

__device__ __forceinline__ float deriv_fma(float x, float y, float z) { return fmaf(x, y, z); }
__device__ __forceinline__ double deriv_fma(double x, double y, double z) { return fma(x, y, z); }

// The power of two of a column: frexp's exponent of its maximum (0 for a column that is all zero, or not finite), and a value with
// that power taken out.  Exact for normal and subnormal values alike -- a column at 2^-146 comes out at [0.5, 1) with the bits it has.
__device__ __forceinline__ int pre_exponent(float mx) { return (mx > 0.0f && mx < 3.0e38f) ? mbd_frexp_exp(mx) : 0; }
__device__ __forceinline__ int pre_exponent(double mx) { int e = 0; if (mx > 0.0 && mx < 1.0e300) (void) frexp(mx, &e); return e; }
__device__ __forceinline__ float pre_scaled(float v, int e) { return mbd_ldexp(v, -e); }
__device__ __forceinline__ double pre_scaled(double v, int e) { return ldexp(v, -e); }
__device__ __forceinline__ void pre_scale4(float* v)
{
    const int e = pre_exponent(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    v[0] = pre_scaled(v[0], e); v[1] = pre_scaled(v[1], e); v[2] = pre_scaled(v[2], e); v[3] = pre_scaled(v[3], e);
}

// A post-order column (k, c) as the calls on the pre-order buffers and the one-branch derivative call read it: every kernel of that
// family takes the column's own power of two out BEFORE the first product, so that no product, and no step of an FMA chain, is
// rounded to a subnormal -- an unscaled column of a dynamically rescaling client may lie anywhere down to 2^-149 (the double-precision
// engine: 2^-1074).  What the calls return are ratios in which that power cancels; where categories are combined it joins the
// category's exponent.  On a column in the normal range scaling by a power of two commutes with every rounding: nothing changes.
// One extra pass over the column (the maximum), which the reads that follow find in the cache: for the kernels that read a
// column from memory as they go (k_edge_readout's general body, k_category_posteriors, k_edge_derivatives).  A kernel that stages
// the column in LDS or holds it in registers (k_pre_partials, cross_stage, k_edge_second_mfma, the four-state bodies) applies pre_exponent / pre_scaled there -- an extra pass over memory cost up to a factor two in the cross products.
template <int LAYOUT, class Real>
struct PostColumn {
    const void*      buf;
    const DerivArgs& g;
    int              k, c, e;      // e: the power of two taken out; `live`: the column holds a positive value
    bool             live;
    // (b null -- a compact tip, no child: nothing is read, the power is 2^0)
    __device__ __forceinline__ PostColumn(const void* b, const DerivArgs& a, int kk, int cc) : buf(b), g(a), k(kk), c(cc), e(0), live(true)
    {
        if (b == nullptr) return;
        // (sixteen states at a time, as cross_stage: their loads are issued together; a state beyond the last repeats the last)
        Real mx = (Real) 0;
        for (int j0 = 0; j0 < a.S; j0 += 16) {
            Real v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = deriv_partial<LAYOUT, Real>(b, a, kk, j0 + u < a.S ? j0 + u : a.S - 1, cc);
#pragma unroll
            for (int u = 0; u < 16; ++u) mx = v[u] > mx ? v[u] : mx;
        }
        e = pre_exponent(mx);
        live = mx > (Real) 0;
    }
    __device__ __forceinline__ Real operator[](int j) const { return pre_scaled(deriv_partial<LAYOUT, Real>(buf, g, k, j, c), e); }
};

template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_edge_derivatives(DerivArgs a)
{
    constexpr bool PER_CATEGORY = LAYOUT == DERIV_S4 || LAYOUT == DERIV_WG;      // an exponent per (pattern, category)
    const int S = a.S, K = a.K;
    const int c = (a.first / 64 + (int) blockIdx.x) * 64 + (int) threadIdx.x;
    const bool second = a.matrix[2] != nullptr;
    double wl = 0.0, w1 = 0.0, w2 = 0.0;
    if (c >= a.first && c < a.last) {
        // the categories are combined at the largest exponent met so far among the live ones: E_k = the stored exponent of the
        // category (or none) + the powers of two taken out of its two columns; what was summed before moves by an exact power of two
        int emax = 0;
        bool any = false;
        const unsigned tip = a.child_tip ? deriv_tip<LAYOUT>(a.child, a, c) : 0u;
        double L = 0.0, D1 = 0.0, D2 = 0.0;
        for (int k = 0; k < K; ++k) {
            const PostColumn<LAYOUT, Real> parent(a.parent, a, k, c), child(a.child_tip ? nullptr : a.child, a, k, c);
            if (!parent.live || !child.live) continue;
            double cat0 = 0.0, cat1 = 0.0, cat2 = 0.0;
            for (int i = 0; i < S; ++i) {
                Real f0, f1, f2 = (Real) 0;
                if (a.child_tip && LAYOUT != DERIV_S4) {
                    if (tip >= (unsigned) S) {
                        f0 = (Real) 1; f1 = (Real) 0;
                    } else {
                        f0 = deriv_matrix<LAYOUT, Real>(a.matrix[0], a, k, i, (int) tip);
                        f1 = deriv_matrix<LAYOUT, Real>(a.matrix[1], a, k, i, (int) tip);
                        if (second) f2 = deriv_matrix<LAYOUT, Real>(a.matrix[2], a, k, i, (int) tip);
                    }
                } else {
                    f0 = f1 = (Real) 0;
                    for (int j = 0; j < S; ++j) {
                        const Real v = a.child_tip ? ((tip >> j & 1u) ? (Real) 1 : (Real) 0) : child[j];
                        f0 = deriv_fma(deriv_matrix<LAYOUT, Real>(a.matrix[0], a, k, i, j), v, f0);
                        f1 = deriv_fma(deriv_matrix<LAYOUT, Real>(a.matrix[1], a, k, i, j), v, f1);
                        if (second) f2 = deriv_fma(deriv_matrix<LAYOUT, Real>(a.matrix[2], a, k, i, j), v, f2);
                    }
                }
                const Real p = parent[i];
                const double pi = a.freqs[i];
                cat0 += (double) (p * f0) * pi;
                cat1 += (double) (p * f1) * pi;
                cat2 += (double) (p * f2) * pi;
            }
            const double w = a.weights[k];
            const int E = (PER_CATEGORY && a.cum != nullptr ? a.cum[(size_t) k * a.Ppad + c] : 0) + parent.e + child.e;
            if (!any || E > emax) {
                if (any) { L = ldexp(L, emax - E); D1 = ldexp(D1, emax - E); D2 = ldexp(D2, emax - E); }
                emax = E;
                any = true;
            }
            L += ldexp(cat0 * w, E - emax);
            D1 += ldexp(cat1 * w, E - emax);
            D2 += ldexp(cat2 * w, E - emax);
        }
        if (!PER_CATEGORY && a.cum != nullptr) emax += a.cum[c];
        const double lnl = log(L) + (double) emax * 0.69314718055994530942;
        const double d1 = D1 / L;
        const double d2 = second ? D2 / L - d1 * d1 : 0.0;
        a.site[c] = lnl;
        a.site[(size_t) a.Ppad + c] = d1;
        a.site[(size_t) 2 * a.Ppad + c] = d2;
        const double pw = a.pattern_weights[c];
        wl = lnl * pw;
        w1 = d1 * pw;
        w2 = d2 * pw;
    }
    mbd_wave_sum_store(wl, a.sums + blockIdx.x);
    mbd_wave_sum_store(w1, a.sums + (size_t) a.sumStride + blockIdx.x);
    mbd_wave_sum_store(w2, a.sums + (size_t) 2 * a.sumStride + blockIdx.x);
}

}  // namespace mbamd
#endif
