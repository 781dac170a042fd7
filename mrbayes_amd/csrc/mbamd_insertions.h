// mbamd_insertions.h -- what the likelihood WOULD be with a subtree attached somewhere else, read from the buffers the gradient reads
// (mbamdCalculateInsertionLogLikelihoods; semantics: include/libhmsbeagle/beagle.h): the scores of every regraft
// position of a pruned clade, or of every placement of a query sequence on a fixed tree, from ONE call.  Included by mbamd_f32.h
// and mbamd_f64.h; product and TEST-ONLY host emulation compile these same kernels.
//
// At a point of a branch, a = pre[k,c,:] is the rest of the tree seen from there and b[m] = post[k,c,m] (the point is the node
// below) or sum_j Pb_k[m,j] post[k,c,j] (the point lies Pb above it) what hangs below.  A subtree hung there across the pendant
// matrix Pc is one more factor s[m] = sum_j Pc_k[m,j] sub[k,c,j] in the product over the point's states:
//     den_k = sum_m a[m] b[m]          num_k = sum_m a[m] b[m] s[m]
//     R_c   = sum_k q_k(c) (num_k / den_k) 2^{x_k(c)}          log R_c = lnL_c(with the subtree) - lnL_c(without it)
// q: the posterior category probabilities of the latest log-likelihood call (ensure_posteriors), q_k = w_k l_k / L, so that
// q_k num_k / den_k = w_k (the category's likelihood with the subtree) / L.  Whatever power of two `pre` and `post` carry per
// (pattern, category) cancels in num_k / den_k; the subtree's does not: x_k(c) is its cumulative exponent (per category where the
// layout keeps one per category, per pattern otherwise) plus the power of two taken out of its column before the first product
// (pre_exponent / pre_scaled: a column may be unscaled, anywhere down to the smallest subnormal).  The categories meet at the
// largest x_k among those that carry something, as in k_edge_derivatives; exact.  A category whose den_k is zero is skipped;
// R_c = 0 (the attachment is impossible) gives -infinity.
//
// The pendant column s does not change with the branch: a wave takes a RUN of consecutive entries, with the categories outermost,
// and forms s_k once per (category, stretch of consecutive entries that name the same subtree buffer and pendant matrix).  It
// stays in LDS, [state][thread] (four states: in registers), the per-entry mixtures R and their exponents in registers.  An entry
// at the child end (no postMatrix) then costs one read of a and b and 2 S multiply-adds.  s_k is formed by the same operations
// wherever the stretch begins, so an entry's result does not depend on its neighbours, on the chunk or on the order of the list.
//
// Arithmetic as in k_edge_readout: products in the engine's precision (FMA chains over the states, ascending), den_k, num_k and the
// sum over the categories in double, block sums through mbd_wave_sum_store, then k_gradient_sums.
#ifndef MBAMD_INSERTIONS_H_
#define MBAMD_INSERTIONS_H_

#include "mbamd_preorder.h"      // DerivArgs and the layout accessors, PostColumn, k_gradient_sums, chunked_readout, the edge_list_* checks

namespace mbamd {

// one candidate of an insertion call, in device pointers
struct InsertEntry {
    const void*    pre;
    const void*    post;          // post-order partials, or compact tip states (postTip)
    const void*    mPost;         // the matrix from the point down to `post`, or null: the point is that node
    const void*    sub;           // the subtree's partials, or compact tip states (subTip)
    const void*    mSub;          // the pendant matrix
    const int32_t* cum;           // the subtree's cumulative exponents ([K][Ppad] on DERIV_S4 / DERIV_WG, [Ppad] otherwise), or null
    int            postTip, subTip;
};
struct InsertArgs {
    DerivArgs          g;
    const InsertEntry* entries;   // the entries of this launch: grid y = runs of INSERT_RUN of them
    const double*      q;         // [K][Ppad] posterior category probabilities, or null (one category: q = 1)
    const double*      pattern_weights;
    double*            site;      // [entries][Ppad] unweighted log R_c, or null: block sums only
    double*            sums;      // [entries][nb]: weight_c log R_c, one per 64-pattern block
    int                nb, count;
};

// entries per wave: R and its exponent, 3 registers per entry -- 24 VGPRs at 8, beside the 64 accumulator registers of the matrix-core
// form at 2 x 2 tiles and the four-state body's 40.  A longer run saves nothing once s_k is amortised over 8 entries (1 / 8 of a
// matrix-vector product per entry against the 2 S multiply-adds the entry costs anyway) and leaves fewer waves for a short list.
constexpr int INSERT_RUN = 8;

// dynamic LDS, [state][thread] columns.  Plain form: the staged operand column and s.  Matrix-core form (TILES row tiles of 32
// states): the staged operand column, s and b, 32 TILES rows each -- 48 KiB at 2 tiles.  Four states: none.
template <class Real> inline size_t insertion_lds_bytes(int S, int tiles)
{
    return tiles > 0 ? (size_t) 3 * 32 * tiles * 64 * sizeof(float) : (size_t) 2 * S * 64 * sizeof(Real);
}

// R[u] and ex[u] of a run: vector types, indexed by the wave-uniform u -- such a value lives in registers (an array indexed at run
// time would be scratch)
typedef double insert_r8 __attribute__((ext_vector_type(INSERT_RUN)));
typedef int insert_e8 __attribute__((ext_vector_type(INSERT_RUN)));
// R 2^ex += term 2^E, at the larger of the two exponents (what was summed before moves by an exact power of two)
__device__ __forceinline__ void insert_mix(insert_r8& R, insert_e8& ex, int u, double term, int E)
{
    if (!(term > 0.0)) return;
    double r = R[u];
    int e = ex[u];
    if (r == 0.0 || E > e) {
        r = r == 0.0 ? 0.0 : ldexp(r, e - E);
        e = E;
    } else {
        term = ldexp(term, E - e);
    }
    R[u] = r + term;
    ex[u] = e;
}

// The partials column (k, c) of `buf` into `col` ([state][thread]) with its own power of two taken out, which is returned; a
// thread beyond the last pattern stages zeros (the matrix-core form reads every column of the block).
template <int LAYOUT, class Real>
__device__ __forceinline__ int insert_stage(const void* buf, const DerivArgs& g, int k, int c, bool live, Real* col)
{
    const int S = g.S;
    if (!live) {
        for (int j = 0; j < S; ++j) col[j * 64] = (Real) 0;
        return 0;
    }
    Real mx = (Real) 0;
    // (sixteen states at a time, as cross_stage: their loads are issued together)
    for (int j0 = 0; j0 < S; j0 += 16) {
        Real v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = deriv_partial<LAYOUT, Real>(buf, g, k, j0 + u < S ? j0 + u : S - 1, c);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (j0 + u < S) {
                col[(j0 + u) * 64] = v[u];
                mx = v[u] > mx ? v[u] : mx;
            }
        }
    }
    const int e = pre_exponent(mx);
    for (int j = 0; j < S; ++j) col[j * 64] = pre_scaled(col[j * 64], e);
    return e;
}

// out[m] = sum_j M_k(m -> j) in[j] for the block's 64 columns, both [state][thread] in LDS.  Plain form (TILES == 0): every thread its
// own column, an FMA chain over j, ascending; no thread reads another's column.  Matrix-core form: 32 TILES states x 64 patterns on
// mbd_mfma_f32_32x32x2 with the operand placement of k_edge_second_mfma -- row tiles hold states, the two column tiles patterns
// 0 .. 31 and 32 .. 63, the reduction runs over j, two per instruction: lane l feeds A[l & 31][l >> 5] = M(32 rt + (l & 31) ->
// 2 s + (l >> 5)), read from the matrix buffer where it lies (zero beyond S), and B[l >> 5][l & 31] = in[2 s + (l >> 5)][pattern
// 32 ct + (l & 31)]; lane l then holds, of column 32 ct + (l & 31), the rows (r & 3) + 8 (r >> 2) + 4 (l >> 5) of every row tile and
// writes them to `out`.  `in0` / `out0`: the columns of thread 0.  Every thread of the wave calls (barriers).
template <int LAYOUT, class Real, int TILES>
__device__ __forceinline__ void insert_matvec(const void* M, const DerivArgs& g, int k, bool live, const Real* in0, Real* out0)
{
    const int S = g.S, lane = (int) threadIdx.x;
    if constexpr (TILES == 0) {
        if (!live) return;
        for (int m = 0; m < S; ++m) {
            Real f = (Real) 0;
            for (int j = 0; j < S; ++j) f = deriv_fma(deriv_matrix<LAYOUT, Real>(M, g, k, m, j), in0[j * 64 + lane], f);
            out0[m * 64 + lane] = f;
        }
    } else {
        const int half = lane >> 5, col = lane & 31;
        MBAMD_SYNC();
        mbd_acc16 acc[TILES][2];
#pragma unroll
        for (int rt = 0; rt < TILES; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = (mbd_acc16) (0.0f);
        const float* const read = in0 + half * 64 + col;
        for (int s = 0; 2 * s < S; ++s) {
            const int j = 2 * s + half;
            const float b0 = read[2 * s * 64], b1 = read[2 * s * 64 + 32];
#pragma unroll
            for (int rt = 0; rt < TILES; ++rt) {
                const int m = 32 * rt + col;
                const float x = (m < S && j < S) ? deriv_matrix<LAYOUT, float>(M, g, k, m, j) : 0.0f;
                acc[rt][0] = mbd_mfma_f32_32x32x2(x, b0, acc[rt][0]);
                acc[rt][1] = mbd_mfma_f32_32x32x2(x, b1, acc[rt][1]);
            }
        }
#pragma unroll
        for (int rt = 0; rt < TILES; ++rt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < S) {
                    out0[row * 64 + col] = acc[rt][0][r];
                    out0[row * 64 + 32 + col] = acc[rt][1][r];
                }
            }
        }
        MBAMD_SYNC();
    }
}

// Grid (64-pattern blocks, runs of INSERT_RUN entries), one wave per workgroup, a thread is a pattern.  TILES > 0: the matrix-core
// form of 16 .. 64 states on the fp32 engine (DERIV_WG, DERIV_LEVELS) -- the two matrix-vector products of partials columns run on
// the matrix cores (insert_matvec), everything else is the plain form's.  Four states (DERIV_S4): columns and matrices in
// registers as in k_pre_partials' four-state body, bitplane tips, no LDS.  A compact tip selects a matrix column; a missing state
// is the factor 1 where the layout stores state codes (k_pre_partials), the four-state bitplanes add the compatible columns.
template <int LAYOUT, class Real, int TILES>
__global__ void __launch_bounds__(64)
k_insertion_readout(InsertArgs a)
{
    constexpr bool PER_CATEGORY = LAYOUT == DERIV_S4 || LAYOUT == DERIV_WG;      // an exponent per (pattern, category)
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K, lane = (int) threadIdx.x;
    const int c = (int) blockIdx.x * 64 + lane;
    const bool live = c < g.last;
    const int first = (int) blockIdx.y * INSERT_RUN;
    const int n = a.count - first < INSERT_RUN ? a.count - first : INSERT_RUN;
    insert_r8 R = (insert_r8) (0.0);
    insert_e8 ex = (insert_e8) (0);
    if constexpr (LAYOUT == DERIV_S4) {
        const size_t at0 = blk_index(c, g.pstride);
        for (int k = 0; k < K && live; ++k) {
            const size_t at = at0 + (size_t) k * 64;
            const double qk = a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int es = 0;
            for (int u = 0; u < n; ++u) {
                const InsertEntry en = a.entries[first + u];
                if (u == 0 || en.sub != a.entries[first + u - 1].sub || en.mSub != a.entries[first + u - 1].mSub) {
                    float v[4];
                    es = 0;
                    if (en.subTip) {
                        const unsigned tip = deriv_tip<LAYOUT>(en.sub, g, c);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = (tip >> j & 1u) ? 1.0f : 0.0f;
                    } else {
                        const f4 q4 = reinterpret_cast<const f4*>(en.sub)[at];
                        v[0] = q4.x; v[1] = q4.y; v[2] = q4.z; v[3] = q4.w;
                        es = pre_exponent(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = pre_scaled(v[j], es);
                    }
                    const MBAMD_AS_CONST float* m = as_const(reinterpret_cast<const float*>(en.mSub)) + k * 16;       // m[j * 4 + l] = P(l -> j)
#pragma unroll
                    for (int l = 0; l < 4; ++l) s[l] = fmaf(m[12 + l], v[3], fmaf(m[8 + l], v[2], fmaf(m[4 + l], v[1], m[l] * v[0])));
                }
                const f4 p4 = reinterpret_cast<const f4*>(en.pre)[at];
                const float p[4] = {p4.x, p4.y, p4.z, p4.w};
                float b[4];
                if (en.postTip) {
                    const unsigned tip = deriv_tip<LAYOUT>(en.post, g, c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = (tip >> j & 1u) ? 1.0f : 0.0f;
                } else {
                    const f4 q4 = reinterpret_cast<const f4*>(en.post)[at];
                    b[0] = q4.x; b[1] = q4.y; b[2] = q4.z; b[3] = q4.w;
                    pre_scale4(b);
                }
                if (en.mPost != nullptr) {
                    const MBAMD_AS_CONST float* m = as_const(reinterpret_cast<const float*>(en.mPost)) + k * 16;
                    const float v[4] = {b[0], b[1], b[2], b[3]};
#pragma unroll
                    for (int l = 0; l < 4; ++l) b[l] = fmaf(m[12 + l], v[3], fmaf(m[8 + l], v[2], fmaf(m[4 + l], v[1], m[l] * v[0])));
                }
                double num = 0.0, den = 0.0;
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const float ab = p[l] * b[l];
                    den += (double) ab;
                    num += (double) (ab * s[l]);
                }
                if (den > 0.0) insert_mix(R, ex, u, qk * (num / den), es + (en.cum != nullptr ? en.cum[(size_t) k * g.Ppad + c] : 0));
            }
        }
    } else {
        constexpr int ROWS = 32 * TILES;
        const size_t rows = TILES > 0 ? (size_t) ROWS : (size_t) S;
        Real* const colT0 = mbd_dyn_lds<Real>();                 // the staged operand column of thread 0 ...
        Real* const colS0 = colT0 + rows * 64;                   // ... its s ...
        Real* const colB0 = colS0 + rows * 64;                   // ... and (matrix-core form) its b
        Real* const colT = colT0 + lane;                         // element j of this thread's column: colT[j * 64]
        const Real* const colS = colS0 + lane;
        // (matrix-core form: a reduction index beyond S meets a zero of the matrix: the column holds a zero there too, not whatever LDS held)
        if (TILES > 0 && (S & 1)) colT[S * 64] = (Real) 0;
        for (int k = 0; k < K; ++k) {
            const double qk = live && a.q != nullptr ? a.q[(size_t) k * g.Ppad + c] : 1.0;
            int es = 0;
            for (int u = 0; u < n; ++u) {
                const InsertEntry en = a.entries[first + u];
                if (u == 0 || en.sub != a.entries[first + u - 1].sub || en.mSub != a.entries[first + u - 1].mSub) {
                    es = 0;
                    if (en.subTip) {
                        if (live) {
                            const unsigned tip = deriv_tip<LAYOUT>(en.sub, g, c);
                            for (int m = 0; m < S; ++m)
                                colS0[m * 64 + lane] = tip < (unsigned) S ? deriv_matrix<LAYOUT, Real>(en.mSub, g, k, m, (int) tip) : (Real) 1;
                        }
                    } else {
                        es = insert_stage<LAYOUT, Real>(en.sub, g, k, c, live, colT);
                        insert_matvec<LAYOUT, Real, TILES>(en.mSub, g, k, live, colT0, colS0);
                    }
                }
                const bool through = en.mPost != nullptr && !en.postTip;         // b = Pb post of a partials column
                if (TILES > 0 && through) {
                    (void) insert_stage<LAYOUT, Real>(en.post, g, k, c, live, colT);
                    insert_matvec<LAYOUT, Real, TILES>(en.mPost, g, k, live, colT0, colB0);
                }
                if (!live) continue;
                double num = 0.0, den = 0.0;
                if (en.postTip) {
                    const unsigned tip = deriv_tip<LAYOUT>(en.post, g, c);
                    if (en.mPost == nullptr && tip < (unsigned) S) {
                        const Real p = deriv_partial<LAYOUT, Real>(en.pre, g, k, (int) tip, c);
                        den = (double) p;
                        num = (double) (p * colS[(int) tip * 64]);
                    } else {
                        for (int m = 0; m < S; ++m) {
                            const Real b = en.mPost != nullptr && tip < (unsigned) S ? deriv_matrix<LAYOUT, Real>(en.mPost, g, k, m, (int) tip) : (Real) 1;
                            const Real ab = deriv_partial<LAYOUT, Real>(en.pre, g, k, m, c) * b;
                            den += (double) ab;
                            num += (double) (ab * colS[m * 64]);
                        }
                    }
                } else if (!through) {
                    const PostColumn<LAYOUT, Real> post(en.post, g, k, c);
                    for (int m = 0; m < S; ++m) {
                        const Real ab = deriv_partial<LAYOUT, Real>(en.pre, g, k, m, c) * post[m];
                        den += (double) ab;
                        num += (double) (ab * colS[m * 64]);
                    }
                } else {
                    if constexpr (TILES == 0) (void) insert_stage<LAYOUT, Real>(en.post, g, k, c, live, colT);
                    for (int m = 0; m < S; ++m) {
                        Real b;
                        if constexpr (TILES == 0) {
                            b = (Real) 0;
                            for (int j = 0; j < S; ++j) b = deriv_fma(deriv_matrix<LAYOUT, Real>(en.mPost, g, k, m, j), colT[j * 64], b);
                        } else {
                            b = colB0[m * 64 + lane];
                        }
                        const Real ab = deriv_partial<LAYOUT, Real>(en.pre, g, k, m, c) * b;
                        den += (double) ab;
                        num += (double) (ab * colS[m * 64]);
                    }
                }
                if (den > 0.0) {
                    const int x = en.cum == nullptr ? 0 : PER_CATEGORY ? en.cum[(size_t) k * g.Ppad + c] : en.cum[c];
                    insert_mix(R, ex, u, qk * (num / den), es + x);
                }
            }
        }
    }
    for (int u = 0; u < n; ++u) {
        double w = 0.0;
        if (live) {
            const double v = log(R[u]) + (double) ex[u] * 0.69314718055994530942;
            if (a.site != nullptr) a.site[(size_t) (first + u) * g.Ppad + c] = v;
            const double pw = a.pattern_weights[c];
            w = pw != 0.0 ? pw * v : 0.0;
        }
        mbd_wave_sum_store(w, a.sums + (size_t) (first + u) * a.nb + blockIdx.x);
    }
}

// ---- host side, shared by the two engines (the hooks: mbamd_preorder.h; cumulativeExponents: the scale buffer as a kernel reads it) ----

// the launch of one chunk of entries; returns whether the matrix-core form took it
template <int LAYOUT, class Real>
inline bool launch_insertion_readout(hipStream_t stream, const InsertArgs& a, bool mfma)
{
    const dim3 grid((unsigned) a.nb, (unsigned) ((a.count + INSERT_RUN - 1) / INSERT_RUN));
    if constexpr (LAYOUT == DERIV_S4) {
        auto kernel = k_insertion_readout<LAYOUT, Real, 0>;
        MBAMD_LAUNCH(kernel, grid, 64, 0, stream, a);
        return false;
    } else {
        if constexpr (LAYOUT == DERIV_WG || LAYOUT == DERIV_LEVELS) {
            if (mfma) {
                const int tiles = a.g.S <= 32 ? 1 : 2;
                const size_t lds = insertion_lds_bytes<float>(a.g.S, tiles);
                if (tiles == 1) { auto kernel = k_insertion_readout<LAYOUT, float, 1>; MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a); }
                else { auto kernel = k_insertion_readout<LAYOUT, float, 2>; MBAMD_LAUNCH_BARRIER(kernel, grid, 64, lds, stream, a); }
                return true;
            }
        }
        auto kernel = k_insertion_readout<LAYOUT, Real, 0>;
        const size_t lds = insertion_lds_bytes<Real>(a.g.S, 0);
        if (lds > (size_t) 48 * 1024 && hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            (void) hipGetLastError();
        MBAMD_LAUNCH(kernel, grid, 64, lds, stream, a);
        return false;
    }
}

// mbamdCalculateInsertionLogLikelihoods on the engine's patterns, through chunked_readout: per chunk of entries one launch of
// k_insertion_readout and k_gradient_sums over the chunk's entries.  sums[i] is this engine's weighted sum of log R_c of entry i;
// sites (or null) takes log R_c of entry i at [i * siteStride + c].  The engine's insertionLaunches[0 / 1] count the launches of the
// plain and of the matrix-core form (16 .. 64 states in single precision unless MBAMD_INSERT_GENERIC is set).
template <class Engine>
inline int insertion_log_likelihoods(Engine& e, const int* pre, const int* post, const int* postM, const int* sub, const int* subM,
                                     const int* subScale, const int* wIdx, int count, double* sites, size_t siteStride, double* sums)
{
    const char* const who = "mbamdCalculateInsertionLogLikelihoods";
    { const int rc = edge_list_begin(e, who); if (rc) return rc; }
    for (int i = 0; i < count; ++i) {
        const int rc = edge_check(e, who, post[i], pre[i], wIdx[i]);
        if (rc) return rc;
        if (sub[i] < 0 || sub[i] >= e.nBuffers || !e.readable(sub[i])) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "subtree buffer");
        if (postM[i] != BEAGLE_OP_NONE && (postM[i] < 0 || postM[i] >= e.nMatrices)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "post matrix index");
        if (subM[i] < 0 || subM[i] >= e.nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "subtree matrix index");
        if (subScale[i] != BEAGLE_OP_NONE && (subScale[i] < 0 || subScale[i] >= e.nScale)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "subtree scale index");
    }
    if (count <= 0 || (!sites && !sums)) return BEAGLE_SUCCESS;
    { const int rc = e.beforeRead(3 * count, [&](int i) { return i < count ? post[i] : i < 2 * count ? pre[i - count] : sub[i - 2 * count]; }); if (rc) return rc; }
    if (e.K > 1) { const int rc = ensure_posteriors(e); if (rc) return rc; }
    std::vector<InsertEntry> table((size_t) count);
    for (int i = 0; i < count; ++i) {
        InsertEntry& t = table[(size_t) i];
        std::memset(&t, 0, sizeof t);
        t.pre = e.partialsPtr(pre[i]);
        t.postTip = e.holdsTip(post[i]) ? 1 : 0;
        t.post = e.operandPtr(post[i]);
        t.mPost = postM[i] != BEAGLE_OP_NONE ? e.matrixPtr(postM[i]) : nullptr;
        t.subTip = e.holdsTip(sub[i]) ? 1 : 0;
        t.sub = e.operandPtr(sub[i]);
        t.mSub = e.matrixPtr(subM[i]);
        if (subScale[i] != BEAGLE_OP_NONE) { const int rc = e.cumulativeExponents(subScale[i], t.cum); if (rc) return rc; }
    }
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size() * sizeof(InsertEntry), &d_table); if (rc) return rc; }
    ReadoutShape shape = {};
    if (sites) shape.site[shape.siteCount++] = {1, sizeof(double)};
    shape.sumPlanes = 1;
    shape.sumRows = 1;
    shape.cap = e.sw.posteriorNodes.value_or(0);
    InsertArgs a;
    a.g = e.layoutArgs();
    a.q = e.K > 1 ? e.d_q : nullptr;
    a.pattern_weights = e.d_pweights;
    a.nb = e.Ppad / 64;
    const bool mfma = e.S >= 16 && e.S <= 64 && !e.sw.insertGeneric;
    const size_t P = (size_t) e.P;
    return chunked_readout(e, count, shape,
        [&](const ReadoutChunk& ch) {
            a.entries = static_cast<const InsertEntry*>(d_table) + ch.first;
            a.count = ch.count;
            a.site = sites ? static_cast<double*>(ch.site[0]) : nullptr;
            a.sums = ch.sums;
            const bool core = e.withLayout([&](auto L) { return launch_insertion_readout<L(), deriv_real<L()>>(e.stream, a, mfma); });
            ++e.insertionLaunches[core ? 1 : 0];
        },
        [&](const ReadoutChunk& ch, int i) {
            const size_t to = (size_t) (ch.first + i);
            if (sites) std::memcpy(sites + to * siteStride, static_cast<const double*>(ch.site[0]) + (size_t) i * e.Ppad, P * sizeof(double));
            if (sums) sums[to] = ch.sums[i];
        });
}

}  // namespace mbamd
#endif
