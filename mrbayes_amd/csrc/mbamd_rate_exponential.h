// mbamd_rate_exponential.h -- transition matrices of ANY rate matrix, without an eigen-system:
//   mbamdUpdateTransitionMatricesFromRateMatrix   P_k = exp(Q r_k t), P'_k = r_k Q P_k, P''_k = r_k Q P'_k   (semantics: beagle.h)
// by uniformization with scaling and squaring.  Q is a generator, so with mu = max_i sum_{j != i} q_ij and
// R = I + Q / mu every quantity in
//     exp(Q tau) = ( sum_{n <= N} e^-y y^n / n!  R^n )^(2^s),     y = mu tau / 2^s <= 1
// is non-negative: nothing cancels, the result needs no clamp and its structural zeros are exact.  Defective and non-reversible
// matrices are served like any other.  Included by both engine headers; written against MatrixLayoutF32 / MatrixLayoutF64
// (mbamd_matrix_products.h), whose store() writes every copy of a matrix buffer.  All arithmetic is double, ONE rounding at the store.
//
// A call is two kinds of launch:
//   k_rate_powers_*   once per call, one workgroup: R^1 ... R^N and Q as zero-padded images in a device scratch, shared by every
//                     branch and category -- the series of a matrix is then a weighted sum and costs no product
//   k_rate_exp_*      one workgroup per (entry, category) (4 states: one thread): the series into LDS, s squarings between two LDS
//                     images with nothing going to global memory, P stored; then P' and P'' from the same image, Q from the scratch
// Three size classes, as the product kernels have: 4 states in registers; 9 ... 64 states on the fp64 matrix cores
// (mbd_mfma_f64_16x16x4, the tiling of k_matrix_products_mfma<NJ> with both operands in LDS); 2, 3, 5 ... 8 a thread per element.
//
// The operation order the tests' bound counts (tests/test_rate_exponential.py):
//   host     sum_i sequential, R_ij = q_ij / mu, R_ii = (mu - sum_i) / mu, x = mu (r t), y = x / 2^s exact, e^-y from libm
//   powers   R^n = R^(n-1) R: a chain of fused multiply-adds over l = 0, 1, ... (4 ceil(S / 4) of them on the matrix cores)
//   weights  w_0 = e^-y, w_n = (w_(n-1) y) / n
//   series   T = w_0 I, then T = fma(w_n, R^n, T) for n = 1 ... N; the row of an absorbing state: the unit vector
//   squaring the same chain as a power; P' = r (Q P), P'' = r (Q P'): the chain, then one product with r
//
// Only the primitives of <mbamd_dev_base.h> are used: the TEST-ONLY host emulation compiles these same bodies.
#ifndef MBAMD_RATE_EXPONENTIAL_H_
#define MBAMD_RATE_EXPONENTIAL_H_

#include "mbamd_matrix_products.h"           // the layouts, MBAMD_MATRIX_LIST_MAX; mbamd_host.h
#include "mbamd_rate_exponential_table.h"    // what the host checks and sends

namespace mbamd {

// One entry of the call, resolved to device pointers by the host (d1, d2: null where the list was not given)
struct alignas(16) RateExpEntry {
    void* prob;
    void* d1;
    void* d2;
    void* pad_;
};
static_assert(sizeof(RateExpEntry) == 32, "RateExpEntry must be 32 bytes");

// An image of an S x S matrix, in the scratch and in LDS: rows of rx_ld doubles.  Above 8 states rows and columns are padded with
// ZEROS to a multiple of 16 (the matrix cores' tiles: a padded product is dead, not garbage), and a row takes two doubles more --
// the A operand's 16 lanes of a column then fall on 16 different bank pairs (the B operand keeps a two-way conflict).
__host__ __device__ inline int rx_dim(int S) { return S > 8 ? (S + 15) / 16 * 16 : S; }
__host__ __device__ inline int rx_ld(int S) { return S > 8 ? rx_dim(S) + 2 : S; }
__host__ __device__ inline size_t rx_image(int S) { return (size_t) rx_dim(S) * rx_ld(S); }
// the scratch: image 0 = Q, image n = R^n (n = 1 ... N)
inline size_t rx_scratch_doubles(int S) { return (size_t) (MBAMD_RATE_EXP_TERMS + 1) * rx_image(S); }

// w[n] = e^-y y^n / n!, by one thread
__device__ __forceinline__ void rx_weights(const RateExpArg& a, double* w)
{
    w[0] = a.ey;
    for (int n = 1; n <= MBAMD_RATE_EXP_TERMS; ++n) w[n] = (w[n - 1] * a.y) / (double) n;
}

// A state nothing leaves (R_ii = 1: its row sum is zero) keeps its row of P the unit vector EXACTLY: the series would give the
// rounded sum of the weights, 1 to a few roundings, and the squarings would raise that to the power 2^s.  A row of zeros and a one
// passes every squaring unchanged.
__device__ __forceinline__ bool rx_absorbing(double rii) { return rii == 1.0; }

// ---- 9 ... 64 states: the fp64 matrix cores ------------------------------------------------------------------------------------------
// acc (16 x 16 per column tile) = rows 16 wave ... of A times B, both zero-padded images of row length LD: one wave per 16 rows,
// NJ column tiles, `steps` contraction steps of four.
//     A operand (16 x 4)  = A[16 wave + (lane & 15)][4 st + (lane >> 4)]
//     B operand (4 x 16)  = B[4 st + (lane >> 4)][16 jt + (lane & 15)]
//     D (16 x 16)         : lane holds column 16 jt + (lane & 15), register r = row 16 wave + (lane >> 4) + 4 r
template <int NJ>
__device__ __forceinline__ void rx_tile_product(const double* A, const double* B, int steps, int wave, int li, int ls, f64x4 (&acc)[NJ])
{
    constexpr int LD = 16 * NJ + 2;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) acc[jt] = (f64x4) (0.0);
    const double* a = A + (size_t) (16 * wave + li) * LD + ls;
    const double* b = B + (size_t) ls * LD + li;
    for (int st = 0; st < steps; ++st) {
        const double av = a[4 * st];
        double bv[NJ];
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) bv[jt] = b[(size_t) 4 * st * LD + 16 * jt];
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) acc[jt] = mbd_mfma_f64_16x16x4(av, bv[jt], acc[jt]);
    }
}
// ... times `scale` (1.0: as it is) into the image C
template <int NJ>
__device__ __forceinline__ void rx_tile_put(double* C, int wave, int li, int ls, double scale, f64x4 (&acc)[NJ])
{
    constexpr int LD = 16 * NJ + 2;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (scale != 1.0) acc[jt][r] *= scale;
            C[(size_t) (16 * wave + ls + 4 * r) * LD + 16 * jt + li] = acc[jt][r];
        }
}
// ... and through the layout into a matrix buffer
template <int NJ, class Layout>
__device__ __forceinline__ void rx_tile_store(const Layout& L, typename Layout::Real* out, int k, int wave, int li, int ls, const f64x4 (&acc)[NJ])
{
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + ls + 4 * r, j = 16 * jt + li;
            if (row < L.S && j < L.S) L.store(out, k, row, j, Layout::round(acc[jt][r]));
        }
}

// rq: R then Q, [S][S] doubles each, as the host made them.  One workgroup of NJ waves; R, and two images that take turns as R^(n-1)
// and R^n, stay in LDS.
template <int NJ>
__global__ void __launch_bounds__(64 * NJ)
k_rate_powers_mfma(const double* __restrict__ rq, double* __restrict__ scratch, int S)
{
    constexpr int DIM = 16 * NJ, LD = DIM + 2, IMG = DIM * LD;
    __shared__ double rimg[IMG], pimg[2 * IMG];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, ls = lane >> 4;
    for (int idx = tid; idx < IMG; idx += blockDim.x) {
        const int i = idx / LD, j = idx % LD;
        const bool live = i < S && j < S;
        const double r = live ? rq[i * S + j] : 0.0;
        rimg[idx] = r;
        pimg[idx] = r;
        pimg[IMG + idx] = 0.0;
        scratch[idx] = live ? rq[S * S + i * S + j] : 0.0;
        scratch[IMG + idx] = r;
    }
    const int steps = (S + 3) / 4;
    int cur = 0;
    for (int n = 2; n <= MBAMD_RATE_EXP_TERMS; ++n) {
        MBAMD_SYNC();
        f64x4 acc[NJ];
        rx_tile_product<NJ>(pimg + cur * IMG, rimg, steps, wave, li, ls, acc);
        rx_tile_put<NJ>(pimg + (1 - cur) * IMG, wave, li, ls, 1.0, acc);
        rx_tile_put<NJ>(scratch + (size_t) n * IMG, wave, li, ls, 1.0, acc);
        cur = 1 - cur;
    }
}

template <int NJ, class Layout>
__global__ void __launch_bounds__(64 * NJ)
k_rate_exp_mfma(const RateExpEntry* __restrict__ entries, const RateExpArg* __restrict__ args, const double* __restrict__ scratch, Layout L)
{
    typedef typename Layout::Real Real;
    constexpr int DIM = 16 * NJ, LD = DIM + 2, IMG = DIM * LD;
    __shared__ double img[2 * IMG], w[MBAMD_RATE_EXP_TERMS + 1];
    const int S = L.S;
    const int u = blockIdx.x / L.K, k = blockIdx.x % L.K;
    const RateExpEntry e = entries[u];
    const RateExpArg a = args[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, ls = lane >> 4;
    if (tid == 0) rx_weights(a, w);
    for (int idx = tid; idx < 2 * IMG; idx += blockDim.x) img[idx] = 0.0;
    MBAMD_SYNC();
    for (int idx = tid; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx % S, at = i * LD + j;
        double t = i == j ? w[0] : 0.0;
        for (int n = 1; n <= MBAMD_RATE_EXP_TERMS; ++n) t = fma(w[n], scratch[(size_t) n * IMG + at], t);
        img[at] = rx_absorbing(scratch[IMG + i * LD + i]) ? (i == j ? 1.0 : 0.0) : t;
    }
    const int steps = (S + 3) / 4;
    int cur = 0;
    f64x4 acc[NJ];
    for (int m = 0; m < a.s; ++m) {                 // (s is uniform over the workgroup)
        MBAMD_SYNC();
        rx_tile_product<NJ>(img + cur * IMG, img + cur * IMG, steps, wave, li, ls, acc);
        rx_tile_put<NJ>(img + (1 - cur) * IMG, wave, li, ls, 1.0, acc);
        cur = 1 - cur;
    }
    MBAMD_SYNC();
    const double* P = img + cur * IMG;
    double* D = img + (1 - cur) * IMG;              // (last read before the barrier above)
    Real* out = static_cast<Real*>(e.prob);
    for (int idx = tid; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx % S;
        L.store(out, k, i, j, Layout::round(P[i * LD + j]));
    }
    if (!e.d1 && !e.d2) return;
    rx_tile_product<NJ>(scratch, P, steps, wave, li, ls, acc);
    rx_tile_put<NJ>(D, wave, li, ls, a.rate, acc);
    if (e.d1) rx_tile_store<NJ>(L, static_cast<Real*>(e.d1), k, wave, li, ls, acc);
    if (!e.d2) return;
    MBAMD_SYNC();
    rx_tile_product<NJ>(scratch, D, steps, wave, li, ls, acc);
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) acc[jt] *= a.rate;
    rx_tile_store<NJ>(L, static_cast<Real*>(e.d2), k, wave, li, ls, acc);
}

// ---- 2, 3, 5 ... 8 states: a thread per element, 64 threads ---------------------------------------------------------------------------
// c_ij = sum_l a_il b_lj as a chain of fused multiply-adds over l = 0, 1, ...
__device__ __forceinline__ double rx_dot(const double* a, const double* b, int S, int i, int j)
{
    double sum = 0.0;
    for (int l = 0; l < S; ++l) sum = fma(a[i * S + l], b[l * S + j], sum);
    return sum;
}

__global__ void __launch_bounds__(64)
k_rate_powers_small(const double* __restrict__ rq, double* __restrict__ scratch, int S)
{
    __shared__ double r[64], p[2 * 64];
    const int tid = threadIdx.x, SS = S * S, i = tid / S, j = tid % S;
    const bool live = tid < SS;
    if (live) {
        r[tid] = p[tid] = rq[tid];
        scratch[tid] = rq[SS + tid];
        scratch[SS + tid] = rq[tid];
    }
    int cur = 0;
    for (int n = 2; n <= MBAMD_RATE_EXP_TERMS; ++n) {
        MBAMD_SYNC();
        if (live) {
            const double v = rx_dot(p + cur * 64, r, S, i, j);
            p[(1 - cur) * 64 + tid] = v;
            scratch[(size_t) n * SS + tid] = v;
        }
        cur = 1 - cur;
    }
}

template <class Layout>
__global__ void __launch_bounds__(64)
k_rate_exp_small(const RateExpEntry* __restrict__ entries, const RateExpArg* __restrict__ args, const double* __restrict__ scratch, Layout L)
{
    typedef typename Layout::Real Real;
    __shared__ double img[2 * 64], q[64], w[MBAMD_RATE_EXP_TERMS + 1];
    const int S = L.S, SS = S * S;
    const int u = blockIdx.x / L.K, k = blockIdx.x % L.K;
    const RateExpEntry e = entries[u];
    const RateExpArg a = args[blockIdx.x];
    const int tid = threadIdx.x, i = tid / S, j = tid % S;
    const bool live = tid < SS;
    if (tid == 0) rx_weights(a, w);
    MBAMD_SYNC();
    if (live) {
        double t = i == j ? w[0] : 0.0;
        for (int n = 1; n <= MBAMD_RATE_EXP_TERMS; ++n) t = fma(w[n], scratch[(size_t) n * SS + tid], t);
        img[tid] = rx_absorbing(scratch[SS + i * S + i]) ? (i == j ? 1.0 : 0.0) : t;
        q[tid] = scratch[tid];
    }
    int cur = 0;
    for (int m = 0; m < a.s; ++m) {                 // (s is uniform over the workgroup)
        MBAMD_SYNC();
        if (live) img[(1 - cur) * 64 + tid] = rx_dot(img + cur * 64, img + cur * 64, S, i, j);
        cur = 1 - cur;
    }
    MBAMD_SYNC();
    const double* P = img + cur * 64;
    double* D = img + (1 - cur) * 64;
    if (live) L.store(static_cast<Real*>(e.prob), k, i, j, Layout::round(P[tid]));
    if (!e.d1 && !e.d2) return;
    if (live) {
        const double v = a.rate * rx_dot(q, P, S, i, j);
        D[tid] = v;
        if (e.d1) L.store(static_cast<Real*>(e.d1), k, i, j, Layout::round(v));
    }
    if (!e.d2) return;
    MBAMD_SYNC();
    if (live) L.store(static_cast<Real*>(e.d2), k, i, j, Layout::round(a.rate * rx_dot(q, D, S, i, j)));
}

// ---- four states: one thread per (entry, category), everything in registers ------------------------------------------------------------
__device__ __forceinline__ void rx_mul4(const double (&a)[16], const double (&b)[16], double (&c)[16])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double sum = 0.0;
#pragma unroll
            for (int l = 0; l < 4; ++l) sum = fma(a[4 * i + l], b[4 * l + j], sum);
            c[4 * i + j] = sum;
        }
}

template <class Layout>
__global__ void __launch_bounds__(256)
k_rate_exp_s4(const RateExpEntry* __restrict__ entries, const RateExpArg* __restrict__ args, const double* __restrict__ scratch, Layout L, int total)
{
    typedef typename Layout::Real Real;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int u = g / L.K, k = g % L.K;
    const RateExpEntry e = entries[u];
    const RateExpArg a = args[g];
    double p[16], t[16];
    double w = a.ey;
#pragma unroll
    for (int x = 0; x < 16; ++x) p[x] = (x % 5 == 0) ? w : 0.0;
    for (int n = 1; n <= MBAMD_RATE_EXP_TERMS; ++n) {
        w = (w * a.y) / (double) n;
#pragma unroll
        for (int x = 0; x < 16; ++x) p[x] = fma(w, scratch[n * 16 + x], p[x]);
    }
#pragma unroll
    for (int x = 0; x < 16; ++x)
        if (rx_absorbing(scratch[16 + 5 * (x / 4)])) p[x] = (x % 5 == 0) ? 1.0 : 0.0;
    for (int m = 0; m < a.s; ++m) {
        rx_mul4(p, p, t);
#pragma unroll
        for (int x = 0; x < 16; ++x) p[x] = t[x];
    }
#pragma unroll
    for (int x = 0; x < 16; ++x) L.store(static_cast<Real*>(e.prob), k, x / 4, x % 4, Layout::round(p[x]));
    if (!e.d1 && !e.d2) return;
    double q[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) q[x] = scratch[x];
    rx_mul4(q, p, t);
#pragma unroll
    for (int x = 0; x < 16; ++x) t[x] *= a.rate;
    if (e.d1) {
#pragma unroll
        for (int x = 0; x < 16; ++x) L.store(static_cast<Real*>(e.d1), k, x / 4, x % 4, Layout::round(t[x]));
    }
    if (!e.d2) return;
    rx_mul4(q, t, p);
#pragma unroll
    for (int x = 0; x < 16; ++x) L.store(static_cast<Real*>(e.d2), k, x / 4, x % 4, Layout::round(a.rate * p[x]));
}

// ---- the host side: one body for both engines -------------------------------------------------------------------------------------
inline void launch_rate_powers(hipStream_t stream, int S, const double* rq, double* scratch)
{
    if (S <= 8) {
        MBAMD_LAUNCH_BARRIER(k_rate_powers_small, 1, 64, 0, stream, rq, scratch, S);
        return;
    }
    switch ((S + 15) / 16) {
        case 1: MBAMD_LAUNCH_BARRIER((k_rate_powers_mfma<1>), 1, 64, 0, stream, rq, scratch, S); break;
        case 2: MBAMD_LAUNCH_BARRIER((k_rate_powers_mfma<2>), 1, 128, 0, stream, rq, scratch, S); break;
        case 3: MBAMD_LAUNCH_BARRIER((k_rate_powers_mfma<3>), 1, 192, 0, stream, rq, scratch, S); break;
        default: MBAMD_LAUNCH_BARRIER((k_rate_powers_mfma<4>), 1, 256, 0, stream, rq, scratch, S); break;
    }
}
template <class Layout>
inline void launch_rate_exponentials(hipStream_t stream, const Layout& L, const RateExpEntry* entries, const RateExpArg* args, const double* scratch, int count)
{
    const int S = L.S;
    const unsigned grid = (unsigned) (count * L.K);
    if (S == 4) {
        MBAMD_LAUNCH((k_rate_exp_s4<Layout>), (grid + 255u) / 256u, 256, 0, stream, entries, args, scratch, L, (int) grid);
    } else if (S <= 8) {
        MBAMD_LAUNCH_BARRIER((k_rate_exp_small<Layout>), grid, 64, 0, stream, entries, args, scratch, L);
    } else {
        switch ((S + 15) / 16) {
            case 1: MBAMD_LAUNCH_BARRIER((k_rate_exp_mfma<1, Layout>), grid, 64, 0, stream, entries, args, scratch, L); break;
            case 2: MBAMD_LAUNCH_BARRIER((k_rate_exp_mfma<2, Layout>), grid, 128, 0, stream, entries, args, scratch, L); break;
            case 3: MBAMD_LAUNCH_BARRIER((k_rate_exp_mfma<3, Layout>), grid, 192, 0, stream, entries, args, scratch, L); break;
            default: MBAMD_LAUNCH_BARRIER((k_rate_exp_mfma<4, Layout>), grid, 256, 0, stream, entries, args, scratch, L); break;
        }
    }
}

// mbamdUpdateTransitionMatricesFromRateMatrix on one engine.  Everything is checked before anything is written; then what is queued
// on the engine runs and the engine does what its setMatrix does before a matrix changes (the hooks of matrix_list_run); R, Q, the
// entries and their arguments travel as ONE staged block; one launch makes the powers, one per MBAMD_MATRIX_LIST_MAX entries the
// matrices.  Asynchronous.
template <class Engine>
inline int rate_exponential_run(Engine& e, const char* who, const double* q, const int* prob, const int* d1, const int* d2,
                                const double* lengths, int count)
{
    { const int rc = e.refuses(who); if (rc) return rc; }
    if (count < 0) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "negative count");
    if (count == 0) return BEAGLE_SUCCESS;
    if (!q || !prob || !lengths) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null array");
    const int S = e.S, K = e.K;
    if (S < 2 || S > 64) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "fewer than 2 or more than 64 states");
    if (const char* why = rate_exp_indices(e.nMatrices, prob, d1, d2, count)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, why);
    RateExpMatrix m;
    if (const char* why = rate_exp_matrix(q, S, m)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, why);
    const size_t SS = (size_t) S * S;
    const size_t entriesAt = 2 * SS * sizeof(double), argsAt = entriesAt + (size_t) count * sizeof(RateExpEntry);
    std::vector<unsigned char> block(argsAt + (size_t) count * K * sizeof(RateExpArg), 0);
    if (const char* why = rate_exp_args(m.mu, e.rateSets[0].r, K, lengths, count, reinterpret_cast<RateExpArg*>(block.data() + argsAt)))
        return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, why);
    { const int rc = e.runQueued(); if (rc) return rc; }
    { const int rc = e.beforeMatrixWrite(); if (rc) return rc; }
    std::memcpy(block.data(), m.R.data(), SS * sizeof(double));
    std::memcpy(block.data() + SS * sizeof(double), m.Q.data(), SS * sizeof(double));
    RateExpEntry* table = reinterpret_cast<RateExpEntry*>(block.data() + entriesAt);
    for (int u = 0; u < count; ++u) {
        table[u].prob = e.matrixPtr(prob[u]);
        table[u].d1 = d1 ? e.matrixPtr(d1[u]) : nullptr;
        table[u].d2 = d2 ? e.matrixPtr(d2[u]) : nullptr;
        table[u].pad_ = nullptr;
    }
    double* scratch = nullptr;
    { const int rc = e.resultScratch(rx_scratch_doubles(S) * sizeof(double), &scratch); if (rc) return rc; }
    void* d_block = nullptr;
    { const int rc = e.stageTable(block.data(), block.size(), &d_block); if (rc) return rc; }
    const unsigned char* d = static_cast<const unsigned char*>(d_block);
    launch_rate_powers(e.stream, S, reinterpret_cast<const double*>(d), scratch);
    const auto L = e.matrixLayout();
    for (int u0 = 0; u0 < count; u0 += MBAMD_MATRIX_LIST_MAX) {           // (entries x categories is a grid dimension)
        const int n = std::min(MBAMD_MATRIX_LIST_MAX, count - u0);
        launch_rate_exponentials(e.stream, L, reinterpret_cast<const RateExpEntry*>(d + entriesAt) + u0,
                                 reinterpret_cast<const RateExpArg*>(d + argsAt) + (size_t) u0 * K, scratch, n);
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd
#endif
