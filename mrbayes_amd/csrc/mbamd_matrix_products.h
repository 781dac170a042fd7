// mbamd_matrix_products.h -- transition matrices made out of transition matrices, on the device (semantics: beagle.h):
//   beagleConvolveTransitionMatrices   R_k = A_k B_k per category: the matrix of a branch that crosses a rate-matrix change
//   beagleTransposeTransitionMatrices  R_k = A_k^T, exact; in place where the client says so
//   beagleSetTransitionMatrices        the batch form of beagleSetTransitionMatrix: one transfer, one scatter launch
// Included by both engine headers.  A matrix buffer is not one array: each engine keeps derived copies beside the matrix its
// beagleGetTransitionMatrix reads (the MFMA A-operand image and the tree walk's tables of the single-precision engine, the padded
// transpose of the double-precision one).  The kernels below are therefore written against a LAYOUT functor -- MatrixLayoutF32 /
// MatrixLayoutF64, the device form of what Instance::setMatrix / getMatrix and Engine64::setMatrix / getMatrix do on the host --
// whose store() writes every copy: one kernel body per size class, instantiated per layout.
//
// Arithmetic of a product: the operands are read as stored (fp32 / fp64) and converted to double, products and sums are double,
// and Layout::round rounds ONCE to the stored type.  Nothing is clamped: the operands may be P' or P''.
//
// Only the primitives of <mbamd_dev_base.h> are used: the TEST-ONLY host emulation compiles these same bodies.
#ifndef MBAMD_MATRIX_PRODUCTS_H_
#define MBAMD_MATRIX_PRODUCTS_H_

#include "mbamd_host.h"          // beagle.h, fail / HIP_TRY, <algorithm>, <cstring>, <vector>
#include "mbamd_kernels.h"       // the device primitives; wg_table_put (mbamd_walkg.h)

namespace mbamd {

// ---- the two layouts ------------------------------------------------------------------------------------------------------------------
// (k, i, j) = (category, from-state, to-state).  load() reads the copy the engine's getMatrix reads; store() writes all copies.
// The padding of a buffer (rows and columns beyond S, the walk tables' constant "missing" column) is never written after the
// instance was made -- neither by the engines' own matrix kernels nor here.
struct MatrixLayoutF32 {
    typedef float Real;
    int S, SP, K;
    int packedT;                 // > 0: the MFMA A-operand image behind the K transposed matrices (mbamd_kernels.h)
    size_t wgTab;                // > 0: the tree walk's tables begin that many floats into the buffer (mbamd_walkg.h)
    __host__ __device__ static float round(double v) { return (float) v; }
    __host__ __device__ double load(const float* buf, int k, int i, int j) const { return (double) buf[(size_t) k * SP * SP + (size_t) j * SP + i]; }
    __host__ __device__ void store(float* buf, int k, int i, int j, float v) const
    {
        buf[(size_t) k * SP * SP + (size_t) j * SP + i] = v;
        if (packedT > 0) {
            const int NT = (S + 31) / 32;
            buf[(size_t) K * SP * SP + ((size_t) (k * NT + i / 32) * packedT + j / 2) * 64 + (i % 32) + 32 * (j % 2)] = v;
        }
        if (wgTab > 0) wg_table_put(buf + wgTab + (size_t) k * wg_table_floats(S), S, i, j, v);
    }
};
struct MatrixLayoutF64 {
    typedef double Real;
    int S, SPAD, K;
    __host__ __device__ static double round(double v) { return v; }
    __host__ __device__ double load(const double* buf, int k, int i, int j) const { return buf[((size_t) k * S + i) * S + j]; }
    __host__ __device__ void store(double* buf, int k, int i, int j, double v) const
    {
        buf[((size_t) k * S + i) * S + j] = v;
        buf[(size_t) K * S * S + ((size_t) k * S + j) * SPAD + i] = v;
    }
};

// One entry of a list, resolved to device pointers by the host (a transpose has no `second`)
struct alignas(16) MatrixProductEntry {
    void* result;
    const void* first;
    const void* second;
    const void* pad_;
};
static_assert(sizeof(MatrixProductEntry) == 32, "MatrixProductEntry must be 32 bytes");

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
// Four states: one thread per (entry, category), both operands and the result in registers.
template <class Layout>
__global__ void __launch_bounds__(256)
k_matrix_products_s4(const MatrixProductEntry* __restrict__ entries, Layout L, int total)
{
    typedef typename Layout::Real Real;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int u = g / L.K, k = g % L.K;
    const MatrixProductEntry e = entries[u];
    const Real* A = static_cast<const Real*>(e.first);
    const Real* B = static_cast<const Real*>(e.second);
    Real* R = static_cast<Real*>(e.result);
    double a[4][4], b[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[i][j] = L.load(A, k, i, j);
            b[i][j] = L.load(B, k, i, j);
        }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double sum = a[i][0] * b[0][j];
#pragma unroll
            for (int l = 1; l < 4; ++l) sum += a[i][l] * b[l][j];
            L.store(R, k, i, j, Layout::round(sum));
        }
}

// 9 ... 64 states: the fp64 matrix cores (mbd_mfma_f64_16x16x4), the tiling of k_transition_matrices_mfma<NJ>: one workgroup per
// (entry, category), one wave per 16 result rows, NJ = ceil(S / 16) column tiles per wave.
//     A operand (16 x 4)  = A_k[16 wave + (lane & 15)][4 st + (lane >> 4)]      zero beyond S: kills the padded terms
//     B operand (4 x 16)  = B_k[4 st + (lane >> 4)][16 jt + (lane & 15)]        (indices clamped: a valid address, a dead product)
//     D (16 x 16)         : lane holds column 16 jt + (lane & 15), register r = row 16 wave + (lane >> 4) + 4 r
// The operands of a chunk of four contraction steps are loaded (and converted to double) before its MFMAs.  An entry's result is
// never one of its operands and no other entry of the launch touches it (matrix_list_groups): nothing is staged.
template <int NJ, class Layout>
__global__ void __launch_bounds__(64 * NJ)
k_matrix_products_mfma(const MatrixProductEntry* __restrict__ entries, Layout L)
{
    typedef typename Layout::Real Real;
    const int S = L.S;
    const int u = blockIdx.x / L.K, k = blockIdx.x % L.K;
    const MatrixProductEntry e = entries[u];
    const Real* A = static_cast<const Real*>(e.first);
    const Real* B = static_cast<const Real*>(e.second);
    Real* R = static_cast<Real*>(e.result);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, ls = lane >> 4;
    const int i = 16 * wave + li;
    const int ic = min(i, S - 1);
    int jc[NJ];
    f64x4 acc[NJ];
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
        acc[jt] = (f64x4) (0.0);
        jc[jt] = min(16 * jt + li, S - 1);
    }
    constexpr int CH = 4;
    const int steps = (S + 3) / 4;
    for (int st0 = 0; st0 < steps; st0 += CH) {
        double a[CH], bb[NJ][CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int s = 4 * (st0 + c) + ls;
            const int sc = min(s, S - 1);
            const double av = L.load(A, k, ic, sc);
            a[c] = (s < S && i < S) ? av : 0.0;
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt) bb[jt][c] = L.load(B, k, sc, jc[jt]);
        }
        MBD_SCHED_BARRIER();                        // (all operand loads of the chunk in front of its MFMAs)
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt) acc[jt] = mbd_mfma_f64_16x16x4(a[c], bb[jt][c], acc[jt]);
    }
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + ls + 4 * r, j = 16 * jt + li;
            if (row < S && j < S) L.store(R, k, row, j, Layout::round(acc[jt][r]));
        }
}

// Every other state count (2, 3, 5 ... 8; and whatever lies beyond 64): one workgroup per (entry, category), a thread per result
// element.  Up to 8 states both operands are staged in LDS as doubles; beyond, the threads read them where they lie.
template <class Layout>
__global__ void __launch_bounds__(256)
k_matrix_products_lds(const MatrixProductEntry* __restrict__ entries, Layout L)
{
    typedef typename Layout::Real Real;
    __shared__ double sa[64], sb[64];
    const int S = L.S;
    const int u = blockIdx.x / L.K, k = blockIdx.x % L.K;
    const MatrixProductEntry e = entries[u];
    const Real* A = static_cast<const Real*>(e.first);
    const Real* B = static_cast<const Real*>(e.second);
    Real* R = static_cast<Real*>(e.result);
    const bool staged = S <= 8;                     // (uniform over the workgroup)
    if (staged) {
        for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
            sa[idx] = L.load(A, k, idx / S, idx % S);
            sb[idx] = L.load(B, k, idx / S, idx % S);
        }
        MBAMD_SYNC();
    }
    for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx % S;
        double sum = 0.0;
        if (staged) {
            for (int l = 0; l < S; ++l) sum += sa[i * S + l] * sb[l * S + j];
        } else {
            for (int l = 0; l < S; ++l) sum += L.load(A, k, i, l) * L.load(B, k, l, j);
        }
        L.store(R, k, i, j, Layout::round(sum));
    }
}

// The transpose: one workgroup per (entry, category) reads the whole category matrix into LDS (S * S values of the stored type,
// dynamic), and writes only after the barrier -- so the result may be the operand itself.  Exact: values move, nothing is computed.
template <class Layout>
__global__ void __launch_bounds__(256)
k_matrix_transpose(const MatrixProductEntry* __restrict__ entries, Layout L)
{
    typedef typename Layout::Real Real;
    Real* t = mbd_dyn_lds<Real>();
    const int S = L.S;
    const int u = blockIdx.x / L.K, k = blockIdx.x % L.K;
    const MatrixProductEntry e = entries[u];
    const Real* A = static_cast<const Real*>(e.first);
    Real* R = static_cast<Real*>(e.result);
    for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) t[idx] = Layout::round(L.load(A, k, idx / S, idx % S));
    MBAMD_SYNC();
    for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx % S;
        L.store(R, k, i, j, t[j * S + i]);
    }
}

// beagleSetTransitionMatrices: the host images of the call's matrices and the entry table behind them, staged as ONE block, go to
// their buffers.  The table begins `tableAt` bytes into the block; `first` of an entry is its image's byte offset in the block.
// grid = (pieces of 256 words, entries); an index named twice is scattered once, from its last image (the host sees to that).
__global__ void __launch_bounds__(256)
k_matrix_scatter(const unsigned char* __restrict__ block, size_t tableAt, unsigned words)
{
    const MatrixProductEntry e = reinterpret_cast<const MatrixProductEntry*>(block + tableAt)[blockIdx.y];
    const unsigned* src = reinterpret_cast<const unsigned*>(block + reinterpret_cast<uintptr_t>(e.first));
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < words) static_cast<unsigned*>(e.result)[w] = src[w];
}

// ---- the host side: one body for both engines -------------------------------------------------------------------------------------
// A list cut into launches: start[g] .. start[g + 1] are the entries of launch g.  A new launch begins exactly where an entry reads or
// writes a buffer the current launch writes, or writes a buffer the current launch reads -- the rule of pre_order_groups
// (mbamd_preorder.h).  second == nullptr: a transpose list (an entry may then write the buffer it reads itself).
#define MBAMD_MATRIX_LIST_MAX 16384              // entries per launch (entries x categories is a grid dimension)
inline void matrix_list_groups(const int* first, const int* second, const int* result, int n, int nMatrices, std::vector<int>& start)
{
    std::vector<char> reads((size_t) nMatrices, 0), writes((size_t) nMatrices, 0);
    start.assign(1, 0);
    for (int u = 0; u < n; ++u) {
        const int a = first[u], b = second ? second[u] : first[u], r = result[u];
        const bool cut = writes[a] || writes[b] || writes[r] || reads[r] || u - start.back() >= MBAMD_MATRIX_LIST_MAX;
        if (cut && u > start.back()) {
            std::fill(reads.begin(), reads.end(), 0);
            std::fill(writes.begin(), writes.end(), 0);
            start.push_back(u);
        }
        reads[a] = 1;
        reads[b] = 1;
        writes[r] = 1;
    }
    start.push_back(n);
}

template <class Layout>
inline void launch_matrix_products(hipStream_t stream, const Layout& L, const MatrixProductEntry* entries, int count)
{
    const int S = L.S;
    const unsigned grid = (unsigned) (count * L.K);
    if (S == 4) {
        MBAMD_LAUNCH((k_matrix_products_s4<Layout>), (grid + 255u) / 256u, 256, 0, stream, entries, L, (int) grid);
    } else if (S > 8 && S <= 64) {
        switch ((S + 15) / 16) {
            case 1: MBAMD_LAUNCH_BARRIER((k_matrix_products_mfma<1, Layout>), grid, 64, 0, stream, entries, L); break;
            case 2: MBAMD_LAUNCH_BARRIER((k_matrix_products_mfma<2, Layout>), grid, 128, 0, stream, entries, L); break;
            case 3: MBAMD_LAUNCH_BARRIER((k_matrix_products_mfma<3, Layout>), grid, 192, 0, stream, entries, L); break;
            default: MBAMD_LAUNCH_BARRIER((k_matrix_products_mfma<4, Layout>), grid, 256, 0, stream, entries, L); break;
        }
    } else {
        MBAMD_LAUNCH_BARRIER((k_matrix_products_lds<Layout>), grid, std::min(256, (S * S + 63) / 64 * 64), 0, stream, entries, L);
    }
}
template <class Layout>
inline void launch_matrix_transpose(hipStream_t stream, const Layout& L, const MatrixProductEntry* entries, int count)
{
    const size_t lds = (size_t) L.S * L.S * sizeof(typename Layout::Real);
    MBAMD_LAUNCH_BARRIER((k_matrix_transpose<Layout>), (unsigned) (count * L.K), std::min(256, (L.S * L.S + 63) / 64 * 64), lds, stream, entries, L);
}

// What the three calls check first, the same on both engines (same status, same text): nothing is written before every entry passed.
inline int matrix_list_check(const char* who, int nMatrices, const int* const* lists, int nLists, int count)
{
    if (count < 0) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "negative count");
    if (count == 0) return BEAGLE_SUCCESS;
    for (int l = 0; l < nLists; ++l)
        if (!lists[l]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null array");
    for (int u = 0; u < count; ++u)
        for (int l = 0; l < nLists; ++l)
            if (lists[l][u] < 0 || lists[l][u] >= nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "matrix index");
    return BEAGLE_SUCCESS;
}

// beagleConvolveTransitionMatrices (`product`) and beagleTransposeTransitionMatrices (no `second`) on one engine: the list is
// checked as a whole, what is queued on the engine runs (a queued update of an operand, a list that reads a result), the engine does
// what its setMatrix does before a matrix changes, and the list runs, one launch per group.  Asynchronous.
template <class Engine>
inline int matrix_list_run(Engine& e, const char* who, bool product, const int* first, const int* second, const int* result, int count)
{
    const int* const lists[3] = {first, result, second};
    { const int rc = matrix_list_check(who, e.nMatrices, lists, product ? 3 : 2, count); if (rc) return rc; }
    if (product)
        for (int u = 0; u < count; ++u)
            if (result[u] == first[u] || result[u] == second[u]) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a result is one of its operands");
    if (count == 0) return BEAGLE_SUCCESS;
    if (!product) second = nullptr;
    const auto L = e.matrixLayout();
    typedef typename std::decay<decltype(L)>::type Layout;
    if (!product && (size_t) L.S * L.S * sizeof(typename Layout::Real) > (size_t) 48 * 1024)
        return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "a category matrix does not fit the workgroup's local memory");
    { const int rc = e.runQueued(); if (rc) return rc; }
    { const int rc = e.beforeMatrixWrite(); if (rc) return rc; }
    std::vector<MatrixProductEntry> table((size_t) count);
    for (int u = 0; u < count; ++u) {
        MatrixProductEntry& t = table[(size_t) u];
        t.result = e.matrixPtr(result[u]);
        t.first = e.matrixPtr(first[u]);
        t.second = product ? e.matrixPtr(second[u]) : nullptr;
        t.pad_ = nullptr;
    }
    const void* d_table = nullptr;                  // (staged the way the engine stages its matrix jobs)
    { const int rc = e.stageMatrixTable(table.data(), table.size() * sizeof(MatrixProductEntry), &d_table); if (rc) return rc; }
    std::vector<int> start;
    matrix_list_groups(first, second, result, count, e.nMatrices, start);
    for (size_t g = 0; g + 1 < start.size(); ++g) {
        const MatrixProductEntry* entries = static_cast<const MatrixProductEntry*>(d_table) + start[g];
        const int n = start[g + 1] - start[g];
        if (product) launch_matrix_products(e.stream, L, entries, n);
        else launch_matrix_transpose(e.stream, L, entries, n);
        HIP_TRY(hipGetLastError());
    }
    return BEAGLE_SUCCESS;
}

// beagleSetTransitionMatrices on one engine: the images Engine::matrixImage makes -- the one beagleSetTransitionMatrix uploads, so
// every stored copy has the bits of `count` single calls -- and the entry table travel as ONE staged block; one launch scatters them.
template <class Engine>
inline int matrix_list_set(Engine& e, const char* who, const int* indices, const double* in, int count)
{
    const int* const lists[1] = {indices};
    { const int rc = matrix_list_check(who, e.nMatrices, lists, 1, count); if (rc) return rc; }
    if (count > 0 && !in) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "null array");
    if (count == 0) return BEAGLE_SUCCESS;
    typedef typename std::decay<decltype(e.matrixLayout())>::type::Real Real;
    { const int rc = e.runQueued(); if (rc) return rc; }
    { const int rc = e.beforeMatrixWrite(); if (rc) return rc; }
    const size_t values = e.matrixValues(), in1 = (size_t) e.K * e.S * e.S;
    std::vector<int> last((size_t) e.nMatrices, -1);         // an index named twice: the later matrix wins
    for (int u = 0; u < count; ++u) last[(size_t) indices[u]] = u;
    std::vector<int> kept;
    for (int u = 0; u < count; ++u)
        if (last[(size_t) indices[u]] == u) kept.push_back(u);
    const size_t imageBytes = (kept.size() * values * sizeof(Real) + 15) / 16 * 16;
    std::vector<unsigned char> block(imageBytes + kept.size() * sizeof(MatrixProductEntry), 0);
    for (size_t n = 0; n < kept.size(); ++n) e.matrixImage(in + (size_t) kept[n] * in1, reinterpret_cast<Real*>(block.data()) + n * values);
    MatrixProductEntry* table = reinterpret_cast<MatrixProductEntry*>(block.data() + imageBytes);
    for (size_t n = 0; n < kept.size(); ++n) {
        table[n].result = e.matrixPtr(indices[kept[n]]);
        table[n].first = reinterpret_cast<const void*>((uintptr_t) (n * values * sizeof(Real)));
    }
    void* d_block = nullptr;
    { const int rc = e.stageTable(block.data(), block.size(), &d_block); if (rc) return rc; }
    const unsigned words = (unsigned) (values * sizeof(Real) / 4);
    for (size_t n0 = 0; n0 < kept.size(); n0 += MBAMD_MATRIX_LIST_MAX) {         // (the entry index is a grid dimension)
        const unsigned n = (unsigned) std::min<size_t>(MBAMD_MATRIX_LIST_MAX, kept.size() - n0);
        MBAMD_LAUNCH(k_matrix_scatter, dim3((words + 255u) / 256u, n), 256, 0, e.stream, static_cast<const unsigned char*>(d_block),
                     imageBytes + n0 * sizeof(MatrixProductEntry), words);
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd
#endif
