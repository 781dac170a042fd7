// mbamd_f64_kernels.h -- the device side of the double-precision engine (Engine64, mbamd_f64.h): the operation and job descriptors
// the host fills, the device helpers the partials kernels share, and every __global__ kernel of that engine (k64_*).  The memory
// layouts are described at the top of mbamd_f64.h.
#ifndef MBAMD_F64_KERNELS_H_
#define MBAMD_F64_KERNELS_H_

#include <cstddef>
#include <cstdint>

#include "mbamd_kernels.h"       // the device primitives, RatesArg, deriv_exponential, MBAMD_MAX_SUBSETS

namespace mbamd {

struct Op64 {
    double* dst;
    const void* c1;              // partials (double) or compact states (uint8)
    const void* c2;
    const double* m1T;           // transposed matrices of child 1: [K][S][SPAD]
    const double* m2T;
    int32_t* scale;              // exponents written (mode 1) or read (mode 2)
    int32_t* cum;                // cumulative exponents the written ones are added to, or null
    int c1_tip, c2_tip, mode;
    int first, last;             // the operation covers patterns [first, last): everything, or one partition (v3 *ByPartition)
    int pad_;
};

template <int IB>
__device__ __forceinline__ void f64_child_factor(const void* ptr, int tip, const double* __restrict__ mT, int S, int SPAD, int k,
                                                 size_t Ppad, size_t c, int i0, double (&f)[IB])
{
    if (tip) {
        const unsigned s = reinterpret_cast<const uint8_t*>(ptr)[c];
        if (s >= (unsigned) S) {
#pragma unroll
            for (int i = 0; i < IB; ++i) f[i] = 1.0;
        } else {
            const double* col = mT + (size_t) s * SPAD + i0;           // P(i -> s), all i: contiguous
#pragma unroll
            for (int i = 0; i < IB; ++i) f[i] = col[i];
        }
    } else {
        const double* cl = reinterpret_cast<const double*>(ptr) + (size_t) k * S * Ppad + c;
#pragma unroll
        for (int i = 0; i < IB; ++i) f[i] = 0.0;
        for (int j = 0; j < S; ++j) {
            const double vj = cl[(size_t) j * Ppad];
            const double* __restrict__ col = mT + (size_t) j * SPAD + i0;
#pragma unroll
            for (int i = 0; i < IB; ++i) f[i] = fma(col[i], vj, f[i]);
        }
    }
}

// ---- what the partials kernels share: the rescale (CondLikeScaler_*: an exact power of two per pattern) and a wave's tiles ----------
// The exponent a pattern's maximum `mx` asks for (mode 1): stored, and added to the cumulative buffer, by the lane that is `writer`.
// OpPtr: however the kernel holds its descriptor (through the scalar cache, in memory, a copy in registers).
template <class OpPtr>
__device__ __forceinline__ int f64_new_exponent(OpPtr op, size_t c, double mx, bool writer)
{
    int e = 0;
    if (mx > 0.0 && mx < 1.0e300) (void) frexp(mx, &e);
    e = e < -1000 ? -1000 : e;
    if (writer) {
        as_global(op->scale)[c] = e;
        if (op->cum != nullptr && e != 0) atomicAdd(op->cum + c, e);
    }
    return e;
}
// the exponent of an operation's result at pattern c: a new one (mode 1), the stored one (mode 2), none
template <class OpPtr>
__device__ __forceinline__ int f64_scale_exponent(OpPtr op, size_t c, double mx, bool writer)
{
    if (op->mode == 1) return f64_new_exponent(op, c, mx, writer);
    if (op->mode == 2) return as_global(op->scale)[c];
    return 0;
}
// a pattern's four lane groups (states g, g + 4, ...) meet through two lane exchanges
__device__ __forceinline__ double f64_pattern_max(double mx)
{
    mx = fmax(mx, mbd_shfl_xor(mx, 16));
    mx = fmax(mx, mbd_shfl_xor(mx, 32));
    return mx;
}
// A wave's NT tiles of one category: register r of tile it at lane (n, g) is state 16 it + g + 4 r of pattern n.
template <int NT>
__device__ __forceinline__ double f64_tiles_max(const double __attribute__((ext_vector_type(4))) (&p)[NT], int S, int g, double mx)
{
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * it + g + 4 * r < S) mx = fmax(mx, p[it][r]);
    return mx;
}
// ... stored to dst (the category's plane at this lane's pattern), divided by 2^e
// (the fused level kernels keep this loop in their own text: called from there, the one-wave kernels of two tiles and three or four
//  categories allocate two vector registers more)
template <int NT>
__device__ __forceinline__ void f64_store_tiles(MBAMD_AS_GLOBAL double* dst, const double __attribute__((ext_vector_type(4))) (&p)[NT], int S, size_t Ppad,
                                                int g, int e)
{
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * it + g + 4 * r;
            if (i < S) dst[(size_t) i * Ppad] = e != 0 ? ldexp(p[it][r], -e) : p[it][r];
        }
}
// ---- a transposed matrix in FRAGMENT order (the LDS image of the four-wave kernels): the 64 lanes' A operands of (step t, tile it)
// are 64 consecutive doubles, element (t, it, lane = (n', g')) = mT[(4 t + g') * SPAD + 16 it + n'], zero beyond S --------------------
// steps of four in-states, padded to the groups of four the contraction runs
constexpr int f64_steps_padded(int S) { return (((S + 3) / 4) + 3) & ~3; }
// one matrix (one category) in fragment order: its doubles, its 16-byte units
constexpr int f64_frag_doubles(int S, int NT) { return f64_steps_padded(S) * NT * 64; }
constexpr int f64_frag_units(int S, int NT) { return f64_steps_padded(S) * NT * 32; }
// dynamic LDS of a workgroup that parks both children's matrices of KL categories
constexpr size_t f64_frag_lds_bytes(int S, int NT, int KL) { return (size_t) 2 * KL * f64_frag_doubles(S, NT) * sizeof(double); }
// Unit u = doubles 2u, 2u + 1 of the image = lanes (g', n' = 2 n2), (g', 2 n2 + 1) of block u / 32: two adjacent columns, one
// 16-byte load -- half the load instructions of a double per lane.  Its source row j and column i (units beyond the image: the last
// one) and whether its two doubles are inside the matrix.
struct F64FragUnit { int j, i; bool x, y; };
template <int NT>
__device__ __forceinline__ F64FragUnit f64_frag_unit(int u, int S)
{
    const int units = f64_frag_units(S, NT), uc = u < units ? u : units - 1;
    const int bc = uc >> 5, w = uc & 31, gg = w >> 3, n2 = w & 7;
    const int it = bc % NT, t = bc / NT;
    const int j = 4 * t + gg, i = 16 * it + 2 * n2;
    return {j, i, j < S && i < S, j < S && i + 1 < S};
}
// the unit as loaded: a clamped address, never a branch (so that all of a thread's loads are in flight together) ...
template <int NT>
__device__ __forceinline__ double __attribute__((ext_vector_type(2))) f64_frag_load(const MBAMD_AS_GLOBAL double* mT, int u, int S, int SPAD)
{
    const F64FragUnit f = f64_frag_unit<NT>(u, S);
    const MBAMD_AS_GLOBAL double* src = mT + (size_t) (f.j < S ? f.j : S - 1) * SPAD + (f.i < S ? f.i : 0);
    double __attribute__((ext_vector_type(2))) v;
    __builtin_memcpy(&v, (const void*) src, sizeof v);    // (one 16-byte load; the transposed copies start at an odd multiple of 8 bytes at 61 states)
    return v;
}
// ... and as parked: what is outside the matrix multiplied by zero (a select would be turned into a branch around the load)
template <int NT>
__device__ __forceinline__ double __attribute__((ext_vector_type(2))) f64_frag_mask(double __attribute__((ext_vector_type(2))) v, int u, int S)
{
    const F64FragUnit f = f64_frag_unit<NT>(u, S);
    v.x *= f.x ? 1.0 : 0.0;
    v.y *= f.y ? 1.0 : 0.0;
    return v;
}

// CondLikeDown_* in fp64 (reference src/likelihood.c:204-375 with CLFlt = double): grid (P_pad/64, operations of a level)
template <int IB>
__global__ void __launch_bounds__(64)
k64_partials(const Op64* __restrict__ ops, int S, int SPAD, int K, int Ppad_)
{
    const Op64& op = ops[blockIdx.y];
    const size_t Ppad = (size_t) Ppad_, c = (size_t) blockIdx.x * 64 + threadIdx.x;
    if (c < (size_t) op.first || c >= (size_t) op.last) return;
    // blockIdx.z = (category, state block): a few hundred waves of patterns alone leave the chip empty
    const int nib = SPAD / IB, k = (int) blockIdx.z / nib, i0 = ((int) blockIdx.z % nib) * IB;
    (void) K;
    double f1[IB], f2[IB];
    f64_child_factor<IB>(op.c1, op.c1_tip, op.m1T + (size_t) k * S * SPAD, S, SPAD, k, Ppad, c, i0, f1);
    f64_child_factor<IB>(op.c2, op.c2_tip, op.m2T + (size_t) k * S * SPAD, S, SPAD, k, Ppad, c, i0, f2);
#pragma unroll
    for (int i = 0; i < IB; ++i)
        if (i0 + i < S) op.dst[((size_t) k * S + i0 + i) * Ppad + c] = f1[i] * f2[i];
}


// CondLikeDown_Gen / _NY98 in fp64 on the fp64 MATRIX cores (v_mfma_f64_16x16x4_f64) for 16 <= S <= 64: a wave owns 16 patterns of
// one category and all states of the destination -- NT = ceil(S / 16) output tiles of 16 states x 16 patterns, each the sum over
// ceil(S / 4) steps of A (16 out-states x 4 in-states, from the TRANSPOSED matrix copy: 16 consecutive doubles per lane row) times
// B (4 in-states x 16 patterns of the child: 16 consecutive doubles).  Accumulator register r of lane (n = lane & 15, g = lane >> 4)
// is state 16 it + g + 4 r of pattern n.  A compact tip's factor is a gather from the transposed matrix laid out for the same
// registers.  grid (P_pad / 16, operations of a level, K).  Round 2's k64_partials<IB> ran this contraction on the vector ALU with
// the matrix column through the scalar cache: 154 us per level at protein 200 x 10 000, 8.7 ms per codon M3 evaluation.
// the 16-pattern product tiles of category k: p[it][r] = state 16 it + g + 4 r of pattern n
template <int NT>
__device__ __forceinline__ void f64_mfma_tiles(const MBAMD_AS_CONST Op64* op, int S, int SPAD, size_t Ppad, int k, size_t c, int n, int g,
                                               double __attribute__((ext_vector_type(4))) (&p)[NT])
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int steps = (S + 3) / 4;
    d4 f[2][NT];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const void* ptr = ch ? op->c2 : op->c1;
        const bool tip = ch ? op->c2_tip : op->c1_tip;
        const MBAMD_AS_GLOBAL double* mT = as_global(ch ? op->m2T : op->m1T) + (size_t) k * S * SPAD;
        if (tip) {
            const unsigned st = as_global(reinterpret_cast<const uint8_t*>(ptr))[c];
#pragma unroll
            for (int it = 0; it < NT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * it + g + 4 * r;
                    f[ch][it][r] = st >= (unsigned) S ? 1.0 : (i < S ? mT[(size_t) st * SPAD + i] : 0.0);
                }
            continue;
        }
        const MBAMD_AS_GLOBAL double* cl = as_global(reinterpret_cast<const double*>(ptr)) + (size_t) k * S * Ppad + c;
#pragma unroll
        for (int it = 0; it < NT; ++it) f[ch][it] = (d4) (0.0);
        for (int t0 = 0; t0 < steps; t0 += 4) {              // four steps' operands in flight
            double b[4], a[4][NT];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = 4 * (t0 + u) + g;              // in-state of this lane's operand rows
                const int jc = j < S ? j : S - 1;
                b[u] = j < S ? cl[(size_t) jc * Ppad] : 0.0;
#pragma unroll
                for (int it = 0; it < NT; ++it) {
                    const int i = 16 * it + n;               // out-state of this lane's A row
                    a[u][it] = (j < S && i < S) ? mT[(size_t) jc * SPAD + (i < SPAD ? i : 0)] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int it = 0; it < NT; ++it) f[ch][it] = mbd_mfma_f64_16x16x4(a[u][it], b[u], f[ch][it]);
        }
    }
#pragma unroll
    for (int it = 0; it < NT; ++it) p[it] = f[0][it] * f[1][it];
}

// KF = 0: one category per wave (blockIdx.z), the rescale in its own pass (k64_rescale); KF = K > 0: a wave computes all K
// categories of its 16 patterns and rescales in registers (CondLikeScaler_*: per-pattern maximum over categories and states --
// the four lane groups of a pattern meet through two lane exchanges), one pass over HBM instead of three.
template <int NT, int KF>
__global__ void __launch_bounds__(64)
k64_partials_mfma(const Op64* __restrict__ ops, int S, int SPAD, int Ppad_)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const MBAMD_AS_CONST Op64* op = as_const(ops) + blockIdx.y;
    const size_t Ppad = (size_t) Ppad_;
    const int lane = (int) threadIdx.x, n = lane & 15, g = lane >> 4;
    const size_t c = (size_t) blockIdx.x * 16 + n;
    if ((size_t) blockIdx.x * 16 + 16 <= (size_t) op->first || (size_t) blockIdx.x * 16 >= (size_t) op->last) return;   // (wave-uniform)
    const bool mine = c >= (size_t) op->first && c < (size_t) op->last;
    if constexpr (KF == 0) {
        const int k = (int) blockIdx.z;
        d4 p[NT];
        f64_mfma_tiles<NT>(op, S, SPAD, Ppad, k, c, n, g, p);
        if (mine) f64_store_tiles<NT>(as_global(op->dst) + (size_t) k * S * Ppad + c, p, S, Ppad, g, 0);
    } else {
        d4 p[KF][NT];
        double mx = 0.0;
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            f64_mfma_tiles<NT>(op, S, SPAD, Ppad, k, c, n, g, p[k]);
            mx = f64_tiles_max<NT>(p[k], S, g, mx);
        }
        const int e = f64_scale_exponent(op, c, f64_pattern_max(mx), mine && g == 0);
        if (mine) {
#pragma unroll
            for (int k = 0; k < KF; ++k) {
                MBAMD_AS_GLOBAL double* dst = as_global(op->dst) + (size_t) k * S * Ppad + c;
#pragma unroll
                for (int it = 0; it < NT; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * it + g + 4 * r;
                        if (i < S) dst[(size_t) i * Ppad] = e != 0 ? ldexp(p[k][it][r], -e) : p[k][it][r];
                    }
            }
        }
    }
}

// The same contraction with the matrices through LDS.  On the kernel above every wave fetches both transposed matrices itself -- at 61
// states 62 KiB through the CU's L1 for 16 patterns, 20 eight-byte loads per 16 matrix instructions, and the L1's 64 B/clk are spent
// at a quarter of the matrix cores' rate.  Here a workgroup of four waves (64 patterns of one operation) parks the matrices of its
// non-tip children in LDS once, in FRAGMENT order -- the 64 lanes' A operands of (step t, tile it) are 64 consecutive doubles, so a
// wave's read is one conflict-free ds_read_b64 -- and only the child's partials (one load per four matrix instructions, the next
// group's in flight behind the current group's arithmetic) still come through the L1.  Same instructions on the same operands in
// the same order as above: the results are bit-identical.  grid (P_pad / 64, operations, K if unfused), 256 threads,
// dynamic LDS 2 * max(KF, 1) * stepsP * NT * 64 doubles, stepsP = ceil(S / 4) rounded up to a multiple of four (64 KiB at 61 states).
// (PRE: the first group's partials of both children were loaded before the matrices were parked -- `pre`.  Requesting ALL of a child's
//  partials ahead was measured on the four-wave workgroups of the narrow levels, where nothing else hides a cold load: at the start of
//  its contraction 2.8 -> 3.6 us per child, before the matrices are parked 2.8 -> 2.3 us but the load phase 3.3 -> 5.0 us -- that phase is
//  the level's read burst at HBM bandwidth (every workgroup of the level loads at the same time), not latency.  profiles/r04_f64.txt)
template <int NT, bool PRE>
__device__ __forceinline__ void f64_mfma_tiles_lds(const MBAMD_AS_CONST Op64* op, int S, int SPAD, size_t Ppad, int k, size_t c, int n, int g, int lane,
                                                   const double* lds1, const double* lds2, const double (&pre)[2][4],
                                                   double __attribute__((ext_vector_type(4))) (&p)[NT]
                                                   )
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int stepsP = f64_steps_padded(S);
    d4 f[2][NT];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const void* ptr = ch ? op->c2 : op->c1;
        const bool tip = ch ? op->c2_tip : op->c1_tip;
        if (tip) {
            // the column of the tip's state from the PARKED matrix (element (row st, column i) of fragment order; zero beyond S): gathered
            // from global memory this was 256 L2 requests per wave, as many as everything else the wave reads
            const unsigned st = as_global(reinterpret_cast<const uint8_t*>(ptr))[c];
            const unsigned sc = st >= (unsigned) S ? 0u : st;
            const double* row = (ch ? lds2 : lds1) + (size_t) ((sc >> 2) * NT) * 64 + (sc & 3u) * 16 + g;
#pragma unroll
            for (int it = 0; it < NT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = row[it * 64 + 4 * r];
                    f[ch][it][r] = st >= (unsigned) S ? 1.0 : v;
                }
            continue;
        }
        const double* la = (ch ? lds2 : lds1) + lane;
        const MBAMD_AS_GLOBAL double* cl = as_global(reinterpret_cast<const double*>(ptr)) + (size_t) k * S * Ppad + c;
#pragma unroll
        for (int it = 0; it < NT; ++it) f[ch][it] = (d4) (0.0);
        // (every load below is unconditional -- clamped row, the value MULTIPLIED by one or zero: a select would be turned into a branch
        //  around the load -- and the loop body straight-line code: a load inside a branch makes the compiler wait for ALL loads at the
        //  join, the prefetched ones included)
        double b[4], bn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * u + g;
            if constexpr (PRE) b[u] = pre[ch][u] * (j < S ? 1.0 : 0.0);       // (multiplied here, not where it was loaded: that would wait for it there)
            else b[u] = cl[(size_t) (j < S ? j : S - 1) * Ppad] * (j < S ? 1.0 : 0.0);
        }
        for (int t0 = 0; t0 < stepsP; t0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {                    // the next group's partials, behind this group's arithmetic
                const int j = 4 * (t0 + 4 + u) + g;
                bn[u] = cl[(size_t) (j < S ? j : S - 1) * Ppad] * (j < S ? 1.0 : 0.0);
            }
            double a[4][NT];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int it = 0; it < NT; ++it) a[u][it] = la[(size_t) ((t0 + u) * NT + it) * 64];      // (zero rows beyond S)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int it = 0; it < NT; ++it) f[ch][it] = mbd_mfma_f64_16x16x4(a[u][it], b[u], f[ch][it]);
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = bn[u];
        }
    }
#pragma unroll
    for (int it = 0; it < NT; ++it) p[it] = f[0][it] * f[1][it];
}

// NW waves per workgroup (16 NW patterns): 8 on the large levels -- the LDS the matrices take allows two workgroups per CU, and two
// waves per SIMD leave the matrix cores idle 60 % of the time (a wave also gathers tips, stores, and waits for its stores to drain);
// 4 on the small ones, where 8 would leave CUs without work.
// (one operation on the workgroup's 16 NW patterns; every thread of the workgroup passes the one barrier inside.  Walking the narrow
//  levels at the top of the tree as chains inside ONE launch of this function -- a workgroup's patterns only depend on the same patterns
//  of the children -- was measured and dropped: 152 us against 158 us for the eleven launches it replaced, an operation is a 11 us latency
//  chain in either form, profiles/r04_f64.txt.)
template <int NT, int KF, int NW>
__device__ __forceinline__ void f64_lds_operation(const MBAMD_AS_CONST Op64* op, double* lds, int S, int SPAD, size_t Ppad)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    constexpr int KL = KF > 0 ? KF : 1;                      // (a matrix is at most 4 NT steps x NT tiles blocks of 64 lanes)
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
    // (= f64_steps_padded, f64_frag_doubles, f64_frag_units, spelled out: through the functions three instantiations allocate other SGPRs)
    const int stepsP = (((S + 3) / 4) + 3) & ~3, nb = stepsP * NT, frag = nb * 64, units = nb * 32;
    const bool inRange = !((size_t) blockIdx.x * (16 * NW) + 16 * NW <= (size_t) op->first || (size_t) blockIdx.x * (16 * NW) >= (size_t) op->last);   // (workgroup-uniform)
    const size_t tile0 = (size_t) blockIdx.x * (16 * NW) + (size_t) wave * 16;
    const bool waveIn = inRange && !(tile0 + 16 <= (size_t) op->first || tile0 >= (size_t) op->last);      // (wave-uniform)
    const size_t c = tile0 + n;
    // ---- the first group of the children's partials (first category): in flight while the matrices are parked ---------------------------------
    double pre[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    if (waveIn) {
        const int k0 = KF > 0 ? 0 : (int) blockIdx.z;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            if (ch ? op->c2_tip : op->c1_tip) continue;
            const MBAMD_AS_GLOBAL double* cl = as_global(reinterpret_cast<const double*>(ch ? op->c2 : op->c1)) + (size_t) k0 * S * Ppad + c;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = 4 * u + g;
                pre[ch][u] = cl[(size_t) (j < S ? j : S - 1) * Ppad];
            }
        }
    }
    // ---- the matrices into LDS, in fragment order (f64_frag_unit) ------------------------------------------------------------------------------
    // (branch-free -- a tip child's matrix is parked too, unused -- so that all loads, up to 32 per thread, are in flight together:
    //  clamped addresses, values multiplied by one or zero, then the LDS stores)
    if (inRange) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        constexpr int R2 = (2 * NT * NT + NW - 1) / NW;       // units per thread and matrix: 32 per block over 64 NW threads
        d2 tmp[KL][2][R2];
#pragma unroll
        for (int kk = 0; kk < KL; ++kk) {
            const int k = KF > 0 ? kk : (int) blockIdx.z;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const MBAMD_AS_GLOBAL double* mT = as_global(ch ? op->m2T : op->m1T) + (size_t) k * S * SPAD;
#pragma unroll
                for (int r = 0; r < R2; ++r) {
                    const int u = r * (64 * NW) + tid;
                    tmp[kk][ch][r] = f64_frag_mask<NT>(f64_frag_load<NT>(mT, u, S, SPAD), u, S);
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < KL; ++kk)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                d2* dstl = reinterpret_cast<d2*>(lds + (size_t) (ch * KL + kk) * frag);
#pragma unroll
                for (int r = 0; r < R2; ++r)
                    if (r * (64 * NW) + tid < units) dstl[r * (64 * NW) + tid] = tmp[kk][ch][r];
            }
    }
    MBAMD_SYNC();
    if (!waveIn) return;                                     // (no barrier below)
    const bool mine = c >= (size_t) op->first && c < (size_t) op->last;
    if constexpr (KF == 0) {
        const int k = (int) blockIdx.z;
        d4 p[NT];
        f64_mfma_tiles_lds<NT, true>(op, S, SPAD, Ppad, k, c, n, g, lane, lds, lds + frag, pre, p);
        if (mine) f64_store_tiles<NT>(as_global(op->dst) + (size_t) k * S * Ppad + c, p, S, Ppad, g, 0);
    } else {
        d4 p[KF][NT];
        double mx = 0.0;
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            if (k == 0) f64_mfma_tiles_lds<NT, true>(op, S, SPAD, Ppad, k, c, n, g, lane, lds + (size_t) k * frag, lds + (size_t) (KF + k) * frag, pre, p[k]);
            else f64_mfma_tiles_lds<NT, false>(op, S, SPAD, Ppad, k, c, n, g, lane, lds + (size_t) k * frag, lds + (size_t) (KF + k) * frag, pre, p[k]);
            mx = f64_tiles_max<NT>(p[k], S, g, mx);
        }
        const int e = f64_scale_exponent(op, c, f64_pattern_max(mx), mine && g == 0);
        if (mine) {
#pragma unroll
            for (int k = 0; k < KF; ++k) {
                MBAMD_AS_GLOBAL double* dst = as_global(op->dst) + (size_t) k * S * Ppad + c;
#pragma unroll
                for (int it = 0; it < NT; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * it + g + 4 * r;
                        if (i < S) dst[(size_t) i * Ppad] = e != 0 ? ldexp(p[k][it][r], -e) : p[k][it][r];
                    }
            }
        }
    }
}

// (second launch bound: four waves per SIMD leave 128 registers -- the wide instantiations, NT x KF >= 6, spilled 5 ... 53 of theirs to
//  scratch at eight waves per workgroup; they get two waves per SIMD, i.e. one such workgroup per CU, and no scratch)
template <int NT, int KF, int NW>
__global__ void __launch_bounds__(64 * NW, (NW == 8 && NT * KF >= 6) ? 2 : NW / 2)
k64_partials_mfma_lds(const Op64* __restrict__ ops, int S, int SPAD, int Ppad_)
{
    f64_lds_operation<NT, KF, NW>(as_const(ops) + blockIdx.y, mbd_dyn_lds<double>(), S, SPAD, (size_t) Ppad_);
}

// (a descriptor by value, member by member: the scalar loads are issued where this is called, the wait is where a member is first used)
__device__ __forceinline__ Op64 f64_load_op(const MBAMD_AS_CONST Op64* p)
{
    Op64 d;
    d.dst = p->dst; d.c1 = p->c1; d.c2 = p->c2; d.m1T = p->m1T; d.m2T = p->m2T; d.scale = p->scale; d.cum = p->cum;
    d.c1_tip = p->c1_tip; d.c2_tip = p->c2_tip; d.mode = p->mode; d.first = p->first; d.last = p->last; d.pad_ = p->pad_;
    return d;
}

// A CHAIN of operations -- each one's result a child of the next: the root-ward path of an MCMC move -- in one launch, the running result
// kept in registers.  The accumulator layout of v_mfma_f64_16x16x4_f64 IS its B layout: register r of output tile it at lane (n, g) holds
// state 16 it + g + 4 r of pattern n, which is what step t = 4 it + r of the next contraction wants from that lane.  So the result of an
// operation feeds the next one's matrix instructions as it stands (the rescaled values -- the same doubles that go to HBM for later
// lists), and a level costs the matrix instructions of its two contractions instead of a launch, a read burst from HBM and a drain
// (11 - 15 us per level on the level kernels).  Per operation: the matrices (fetched into registers during the previous operation) are
// parked in LDS in fragment order, the SIBLING's partials (fetched then too) and the running result are contracted, product, rescale,
// store; a tip sibling is a column of the parked matrix.  A workgroup = four waves = 64 patterns of one chain (a codon model's eigen
// parts are chains of their own); no pattern partitions.  Op64::pad_: 0 first operation of a chain (child 1 from memory or a tip,
// child 2 the "sibling"), 1 / 2 = child 1 / 2 is the previous result.  The same instructions on the same operands: bit-identical to
// the level kernels.  grid (P_pad / 64, chains), 256 threads, dynamic LDS as k64_partials_mfma_lds.
template <int NT, int KF>
__global__ void __launch_bounds__(256)
k64_partials_chain(const Op64* __restrict__ ops, const int* __restrict__ chainStart, int S, int SPAD, int Ppad_)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int NW = 4, R2 = (2 * NT * NT + NW - 1) / NW;
    double* lds = mbd_dyn_lds<double>();
    const size_t Ppad = (size_t) Ppad_;
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int stepsP = f64_steps_padded(S), nb = stepsP * NT, frag = f64_frag_doubles(S, NT);
    const int ob = chainStart[blockIdx.y], oe = chainStart[blockIdx.y + 1];
    const size_t c = (size_t) blockIdx.x * 64 + (size_t) wave * 16 + n;
    d4 prev[KF][NT];                                         // the previous operation's (rescaled) result
    d2 mt[KF][2][R2];                                        // the next operation's matrices on their way to LDS
    double sib[KF][NT][4];                                   // the next operation's sibling partials: [category][group of four steps][step]
#pragma unroll
    for (int k = 0; k < KF; ++k)
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            prev[k][it] = (d4) (0.0);
#pragma unroll
            for (int u = 0; u < 4; ++u) sib[k][it][u] = 0.0;
        }
    auto fetchMatrices = [&](const Op64& d) {
#pragma unroll
        for (int k = 0; k < KF; ++k)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const MBAMD_AS_GLOBAL double* mT = as_global(ch ? d.m2T : d.m1T) + (size_t) k * S * SPAD;
#pragma unroll
                for (int r = 0; r < R2; ++r)                 // (as loaded: masked where it is written to LDS -- a multiplication here would wait for the load)
                    mt[k][ch][r] = f64_frag_load<NT>(mT, r * (64 * NW) + tid, S, SPAD);
            }
    };
    unsigned sibState = 0;                                   // the next operation's sibling, if it is a tip: its state
    int storedExp = 0;                                       // the next operation's exponent, if it re-uses a stored one (mode 2)
    auto fetchSibling = [&](const Op64& d) {
        // (the same loads whatever the sibling is -- a tip's "partials" are read from the operation's own destination, a node's "state"
        //  from the chain table, both unused: a load inside a branch would make every later wait a wait for everything in flight)
        const int si = d.pad_ == 2 ? 0 : 1;                // the sibling is child 2 unless child 2 is the chain
        const bool tip = si ? d.c2_tip : d.c1_tip;
        const void* sp = si ? d.c2 : d.c1;
        sibState = as_global(reinterpret_cast<const uint8_t*>(tip ? sp : (const void*) chainStart))[tip ? c : 0];
        storedExp = as_global(d.mode == 2 ? (const int32_t*) d.scale : (const int32_t*) chainStart)[d.mode == 2 ? c : 0];   // (a stored exponent: ahead as well)
        const MBAMD_AS_GLOBAL double* cl = as_global(tip ? (const double*) d.dst : reinterpret_cast<const double*>(sp)) + c;
#pragma unroll
        for (int k = 0; k < KF; ++k)
#pragma unroll
            for (int gq = 0; gq < NT; ++gq)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = 4 * (4 * gq + u) + g;
                    sib[k][gq][u] = cl[(size_t) k * S * Ppad + (size_t) (j < S ? j : S - 1) * Ppad];
                }
    };
    // the descriptors through the scalar cache TWO operations ahead (a first touch is ~1 us: read where they are used, that is two or
    // three serial misses per operation)
    if (ob >= oe) return;
    Op64 dcur = f64_load_op(as_const(ops) + ob), dnxt = f64_load_op(as_const(ops) + (ob + 1 < oe ? ob + 1 : ob));
    fetchMatrices(dcur);
    fetchSibling(dcur);
    for (int o = ob; o < oe; ++o) {
        const Op64 dnn = f64_load_op(as_const(ops) + (o + 2 < oe ? o + 2 : oe - 1));
        const Op64* op = &dcur;
#pragma unroll
        for (int k = 0; k < KF; ++k)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                d2* dstl = reinterpret_cast<d2*>(lds + (size_t) (ch * KF + k) * frag);
#pragma unroll
                for (int r = 0; r < R2; ++r) {
                    const int u = r * (64 * NW) + tid;
                    if (u < nb * 32) {
                        const int bc = u >> 5, w = u & 31, it = bc % NT, t = bc / NT;
                        const int j = 4 * t + (w >> 3), i = 16 * it + 2 * (w & 7);
                        d2 v = mt[k][ch][r];
                        v.x *= (j < S && i < S) ? 1.0 : 0.0;
                        v.y *= (j < S && i + 1 < S) ? 1.0 : 0.0;
                        dstl[u] = v;
                    }
                }
            }
        if (o + 1 < oe) fetchMatrices(dnxt);               // (in flight during this operation's arithmetic)
        MBAMD_SYNC();
        const int cc = op->pad_, si = cc == 2 ? 0 : 1;       // chain child code, sibling's child index
        d4 p[KF][NT];
        double mx = 0.0;
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            d4 f[2][NT];
            // one child's factor tiles: a tip's column from the parked matrix, or NT groups of four steps with b(gq, u) as operand
            auto column = [&](int ch, unsigned st) {
                const unsigned sc = st >= (unsigned) S ? 0u : st;
                const double* row = lds + (size_t) (ch * KF + k) * frag + (size_t) ((sc >> 2) * NT) * 64 + (sc & 3u) * 16 + g;
#pragma unroll
                for (int it = 0; it < NT; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double v = row[it * 64 + 4 * r];
                        f[ch][it][r] = st >= (unsigned) S ? 1.0 : v;
                    }
            };
            auto contract = [&](int ch, auto bval) {
                const double* la = lds + (size_t) (ch * KF + k) * frag + lane;
#pragma unroll
                for (int it = 0; it < NT; ++it) f[ch][it] = (d4) (0.0);
#pragma unroll
                for (int gq = 0; gq < NT; ++gq) {
                    if (4 * gq >= stepsP) break;             // (wave-uniform)
                    double a[4][NT];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int it = 0; it < NT; ++it) a[u][it] = la[(size_t) ((4 * gq + u) * NT + it) * 64];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double bu = bval(gq, u) * ((4 * (4 * gq + u) + g) < S ? 1.0 : 0.0);
#pragma unroll
                        for (int it = 0; it < NT; ++it) f[ch][it] = mbd_mfma_f64_16x16x4(a[u][it], bu, f[ch][it]);
                    }
                }
            };
            // the running result first -- it needs nothing from memory, and the sibling's partials get that much longer to arrive --
            // or (first operation of a chain) child 1: a tip or partials in memory
            if (cc != 0) contract(1 - si, [&](int gq, int u) { return prev[k][gq][u]; });
            else if (op->c1_tip) column(0, as_global(reinterpret_cast<const uint8_t*>(op->c1))[c]);
            else {
                const MBAMD_AS_GLOBAL double* cl = as_global(reinterpret_cast<const double*>(op->c1)) + (size_t) k * S * Ppad + c;
                double first[NT][4];
#pragma unroll
                for (int gq = 0; gq < NT; ++gq)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = 4 * (4 * gq + u) + g;
                        first[gq][u] = cl[(size_t) (j < S ? j : S - 1) * Ppad];
                    }
                contract(0, [&](int gq, int u) { return first[gq][u]; });
            }
            if (si ? op->c2_tip : op->c1_tip) column(si, sibState);
            else contract(si, [&](int gq, int u) { return sib[k][gq][u]; });
#pragma unroll
            for (int it = 0; it < NT; ++it) p[k][it] = f[0][it] * f[1][it];
            mx = f64_tiles_max<NT>(p[k], S, g, mx);
        }
        const int eStored = storedExp;
        if (o + 1 < oe) fetchSibling(dnxt);                // (every category's sibling values have been used)
        mx = f64_pattern_max(mx);
        int e = 0;
        if (op->mode == 1) e = f64_new_exponent(op, c, mx, g == 0);
        else if (op->mode == 2) e = eStored;
#pragma unroll
        for (int k = 0; k < KF; ++k) {                       // (the rescaled values: the next operation's operand, and what goes to HBM)
#pragma unroll
            for (int it = 0; it < NT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) prev[k][it][r] = e != 0 ? ldexp(p[k][it][r], -e) : p[k][it][r];
            f64_store_tiles<NT>(as_global(op->dst) + (size_t) k * S * Ppad + c, prev[k], S, Ppad, g, 0);
        }
        MBAMD_SYNC();                                        // every wave is done with the parked matrices
        dcur = dnxt;
        dnxt = dnn;
    }
}

// Both children compact tips: no contraction, the product of two matrix columns -- a gather.  On the kernel above that is 32 scattered
// loads and 16 stores per wave at two waves per SIMD (its accumulators), 1.2 us per codon operation against 0.5 us of stores; here a
// lane owns states g, g + 4, ... of pattern n (NSL of them per category, KF categories: KF x NSL <= 32 products in registers), the
// same product and the same rescale, eight waves per SIMD.  grid (P_pad / 16, operations).
template <int NSL, int KF>
__global__ void __launch_bounds__(64)
k64_partials_tips(const Op64* __restrict__ ops, int S, int SPAD, int Ppad_)
{
    const MBAMD_AS_CONST Op64* op = as_const(ops) + blockIdx.y;
    const size_t Ppad = (size_t) Ppad_;
    const int lane = (int) threadIdx.x, n = lane & 15, g = lane >> 4;
    const size_t c = (size_t) blockIdx.x * 16 + n;
    if ((size_t) blockIdx.x * 16 + 16 <= (size_t) op->first || (size_t) blockIdx.x * 16 >= (size_t) op->last) return;   // (wave-uniform)
    const bool mine = c >= (size_t) op->first && c < (size_t) op->last;
    const unsigned s1 = as_global(reinterpret_cast<const uint8_t*>(op->c1))[c], s2 = as_global(reinterpret_cast<const uint8_t*>(op->c2))[c];
    const bool gap1 = s1 >= (unsigned) S, gap2 = s2 >= (unsigned) S;
    const MBAMD_AS_GLOBAL double* r1 = as_global(op->m1T) + (size_t) (gap1 ? 0u : s1) * SPAD;
    const MBAMD_AS_GLOBAL double* r2 = as_global(op->m2T) + (size_t) (gap2 ? 0u : s2) * SPAD;
    double p[KF][NSL];
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k < KF; ++k)
#pragma unroll
        for (int q = 0; q < NSL; ++q) {
            const int i = g + 4 * q, ic = i < S ? i : S - 1;
            const double a = r1[(size_t) k * S * SPAD + ic], b = r2[(size_t) k * S * SPAD + ic];
            p[k][q] = i < S ? (gap1 ? 1.0 : a) * (gap2 ? 1.0 : b) : 0.0;
            mx = fmax(mx, p[k][q]);
        }
    const int e = f64_scale_exponent(op, c, f64_pattern_max(mx), mine && g == 0);
    if (mine) {
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            MBAMD_AS_GLOBAL double* dst = as_global(op->dst) + (size_t) k * S * Ppad + c;
#pragma unroll
            for (int q = 0; q < NSL; ++q) {
                const int i = g + 4 * q;
                if (i < S) dst[(size_t) i * Ppad] = e != 0 ? ldexp(p[k][q], -e) : p[k][q];
            }
        }
    }
}

// The same for 256 patterns per workgroup with both matrices parked in LDS (rows SPAD | 1 doubles apart, so that the lanes' rows fall on
// different banks): the gather above makes 512 L2 requests per wave of 16 patterns -- 1 GB through the L1 miss queues for 244 MB of
// results at codon size, 121 us where the stores alone take 36 (tools/microbench/store_patterns.hip) -- here a workgroup reads its two
// matrices once, coalesced.  lane = pattern: every store is 512 contiguous bytes.  Two passes over LDS (maximum, then products) instead
// of K x S products in registers.  Same products, same rescale.  grid (ceil(P_pad / 256), operations), dynamic LDS 2 K S (SPAD | 1) doubles.
__global__ void __launch_bounds__(256)
k64_partials_tips_lds(const Op64* __restrict__ ops, int S, int SPAD, int K, int Ppad_)
{
    double* lds = mbd_dyn_lds<double>();
    const MBAMD_AS_CONST Op64* op = as_const(ops) + blockIdx.y;
    const size_t Ppad = (size_t) Ppad_;
    const int tid = (int) threadIdx.x;
    const int SL = SPAD | 1, rows = K * S;
    if ((size_t) blockIdx.x * 256 + 256 <= (size_t) op->first || (size_t) blockIdx.x * 256 >= (size_t) op->last) return;   // (workgroup-uniform)
    {   // rows [k][state] of both transposed matrices, 16 loads per thread in flight
        const MBAMD_AS_GLOBAL double* m1 = as_global(op->m1T);
        const MBAMD_AS_GLOBAL double* m2 = as_global(op->m2T);
        const int total = rows * SPAD;                       // elements of one matrix (all categories)
        for (int base = 0; base < total; base += 256 * 8) {
            double t1[8], t2[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + u * 256 + tid, ic = idx < total ? idx : total - 1;
                t1[u] = m1[ic];
                t2[u] = m2[ic];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + u * 256 + tid;
                if (idx < total) {
                    const int r = idx / SPAD, i = idx - r * SPAD;
                    lds[(size_t) r * SL + i] = t1[u];
                    lds[(size_t) (rows + r) * SL + i] = t2[u];
                }
            }
        }
    }
    MBAMD_SYNC();
    const size_t c = (size_t) blockIdx.x * 256 + tid;
    if (c >= Ppad) return;                                   // (whole waves: P_pad is a multiple of 64; no barrier below)
    const bool mine = c >= (size_t) op->first && c < (size_t) op->last;
    const unsigned s1 = as_global(reinterpret_cast<const uint8_t*>(op->c1))[c], s2 = as_global(reinterpret_cast<const uint8_t*>(op->c2))[c];
    const bool gap1 = s1 >= (unsigned) S, gap2 = s2 >= (unsigned) S;
    const double* r1 = lds + (size_t) (gap1 ? 0u : s1) * SL;
    const double* r2 = lds + (size_t) rows * SL + (size_t) (gap2 ? 0u : s2) * SL;
    const size_t kstep = (size_t) S * SL;                    // a category further
    double mx = 0.0;
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < S; ++i) {
            const double a = r1[k * kstep + i], b = r2[k * kstep + i];
            mx = fmax(mx, (gap1 ? 1.0 : a) * (gap2 ? 1.0 : b));
        }
    const int e = f64_scale_exponent(op, c, mx, mine);
    if (!mine) return;
    MBAMD_AS_GLOBAL double* dst = as_global(op->dst) + c;
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < S; ++i) {
            const double a = r1[k * kstep + i], b = r2[k * kstep + i];
            const double p = (gap1 ? 1.0 : a) * (gap2 ? 1.0 : b);
            dst[((size_t) k * S + i) * Ppad] = e != 0 ? ldexp(p, -e) : p;
        }
}


// The same with the rescale fused (K == KF categories, S <= IB: all K x S results of a pattern stay in registers): one pass
// over HBM instead of three.  Instantiated for four states and the default four gamma categories (at 20 states the K x S
// results need all 256 VGPRs and the fused kernel is no faster: measured, dropped).
template <int IB, int KF>
__global__ void __launch_bounds__(64)
k64_partials_fused(const Op64* __restrict__ ops, int S, int SPAD, int Ppad_)
{
    const Op64& op = ops[blockIdx.y];
    const size_t Ppad = (size_t) Ppad_, c = (size_t) blockIdx.x * 64 + threadIdx.x;
    if (c < (size_t) op.first || c >= (size_t) op.last) return;
    int32_t* cumulative = op.cum;
    double out[KF][IB];
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
        double f2[IB];
        f64_child_factor<IB>(op.c1, op.c1_tip, op.m1T + (size_t) k * S * SPAD, S, SPAD, k, Ppad, c, 0, out[k]);
        f64_child_factor<IB>(op.c2, op.c2_tip, op.m2T + (size_t) k * S * SPAD, S, SPAD, k, Ppad, c, 0, f2);
#pragma unroll
        for (int i = 0; i < IB; ++i) {
            out[k][i] *= f2[i];
            if (i < S) mx = fmax(mx, out[k][i]);
        }
    }
    int e = 0;
    if (op.mode == 1) {
        if (mx > 0.0 && mx < 1.0e300) (void) frexp(mx, &e);
        e = e < -1000 ? -1000 : e;
        op.scale[c] = e;
        if (cumulative != nullptr && e != 0) atomicAdd(cumulative + c, e);
    } else if (op.mode == 2) {
        e = op.scale[c];
    }
#pragma unroll
    for (int k = 0; k < KF; ++k)
#pragma unroll
        for (int i = 0; i < IB; ++i)
            if (i < S) op.dst[((size_t) k * S + i) * Ppad + c] = e != 0 ? ldexp(out[k][i], -e) : out[k][i];
}

// CondLikeScaler_* (reference src/likelihood.c:4939-4988): per-pattern maximum over categories and states, exact
// power-of-two rescale, exponent kept (and added to the cumulative buffer of the call)
__global__ void __launch_bounds__(64)
k64_rescale(const Op64* __restrict__ ops, int S, int K, int Ppad_)
{
    const Op64& op = ops[blockIdx.y];
    if (op.mode == 0) return;
    const size_t Ppad = (size_t) Ppad_, c = (size_t) blockIdx.x * 64 + threadIdx.x;
    if (c < (size_t) op.first || c >= (size_t) op.last) return;
    int32_t* cumulative = op.cum;
    double* dst = op.dst + c;
    const int n = K * S;
    int e = 0;
    if (op.mode == 1) {
        double mx = 0.0;
        for (int r = 0; r < n; ++r) mx = fmax(mx, dst[(size_t) r * Ppad]);
        if (mx > 0.0 && mx < 1.0e300) (void) frexp(mx, &e);
        e = e < -1000 ? -1000 : e;
        op.scale[c] = e;
        if (cumulative != nullptr && e != 0) atomicAdd(cumulative + c, e);
    } else {
        e = op.scale[c];
    }
    if (e != 0)
        for (int r = 0; r < n; ++r) dst[(size_t) r * Ppad] = ldexp(dst[(size_t) r * Ppad], -e);
}


// ---------------------------------------------------------------------------------------------------------------------------
// Four states: the tree walk in fp64 -- ONE launch per operation list instead of one per dependency level.  A WAVE owns PW = 64 / KP
// patterns with all their categories: lane = category * PW + pattern (KP = the category count rounded up to a power of two; the
// lanes of a category beyond the last repeat the last one, bit for bit, and store the same values to the same addresses).  The
// rescaling maximum is per PATTERN (CondLikeScaler_*): the categories of a pattern meet through log2(KP) lane exchanges -- no
// barrier, no LDS exchange, a workgroup is one wave.  All waves interpret one program compiled by the same Walk4Builder as the
// fp32 walks (mbamd_walk4_host.h, register-fed mode: a child is a compact tip, a slot of the wave's LDS, or read from HBM in
// place).  Results are stored once and children the wave produced itself are read back from LDS: HBM sees (almost) only the
// write stream -- the level kernels read every child back.  Arithmetic and its order are those of k64_partials_fused: the two
// paths give the same bits (MBAMD_F64_NO_WALK=1 selects the levels).
// (Round 3's version -- a workgroup of K waves, one per category, the maxima exchanged through LDS behind a barrier per
//  operation, matrices as scalar operands, every load issued where it was used: 2.50 ms per evaluation at 1000 x 50 000, the
//  barrier version with this file's fetch-ahead 1.64 ms; 782 four-wave workgroups also spread unevenly over 256 CUs.)
struct Walk64Entry {             // 32 bytes, one scalar load: INDICES (buffer, matrix, exponent row), the bases are kernel arguments
    uint32_t dst;                // partials buffer written
    uint32_t c1, c2;             // memory child: partials buffer; compact tip: row of the state array; LDS child: unused
    uint32_t m1, m2;             // matrix buffers
    uint32_t scaleR, scaleW;     // exponent rows read (mode 2) / written (mode 1); the instance's scratch row when unused
    uint32_t ctl;                // kind1 | kind2 << 2 | mode << 4 | nop << 6 | slot1 << 8 | slot2 << 16 | keep << 24
};                               //   kind: 0 LDS slot, 1 memory, 2 compact tip; keep: slot the result is also written to, 0xFF none
static_assert(sizeof(Walk64Entry) == 32, "Walk64Entry is one 32-byte scalar load");
struct Walk64Args {
    const Walk64Entry* prog;
    int entries, nslots;
    double* partials;            // [buffer][K][4][Ppad]
    unsigned bufDoubles;         // doubles per buffer (K x 4 x Ppad)
    const uint8_t* states;       // [row][Ppad]
    const double* matricesT;     // transposed copy [K][4][4] of matrix 0; matrix m is matDoubles further
    unsigned matDoubles;
    int32_t* scale;              // [row][Ppad]
    int32_t* cum;                // cumulative row of the list, or nullptr
    int Ppad;
    int scratchRow;              // exponent row nobody reads
    int K;                       // categories (<= KP of the instantiation)
};
__device__ __forceinline__ Walk64Entry w64_load(const MBAMD_AS_CONST Walk64Entry* p)
{
    Walk64Entry e;
    e.dst = p->dst; e.c1 = p->c1; e.c2 = p->c2; e.m1 = p->m1; e.m2 = p->m2; e.scaleR = p->scaleR; e.scaleW = p->scaleW; e.ctl = p->ctl;
    return e;
}
// Vector-memory results return in order behind everything issued before them: a load issued after an entry's stores waits for
// those stores to reach HBM (microseconds under a write stream).  What every entry loads -- the states of its compact tips (a
// byte per lane) and its two 4 x 4 matrices per category -- is therefore fetched ONE ENTRY AHEAD, before the previous entry's
// stores, by loads that every entry issues whatever its children are (an entry without tips reads one harmless, cached byte):
// straight-line code, so the compiler's wait counts are exact and leave the stores in flight.  Children that live in HBM (evicted
// from the LDS slots: 3 of 996 at 500 taxa with four slots, none with five) and stored exponents (SCALE_READ) are loaded where
// they are used and CONSUMED there (a load still pending where branches meet makes the compiler wait for every vector-memory
// instruction, the previous entry's stores included, on all paths).  An entry without a scale buffer writes its zero exponents
// to the instance's scratch row (the same five stores for every entry); the host leaves no no-operation entries in the program;
// the loop is entered after a whole first entry, so that both ways into the loop head end with the same instruction sequence.
__device__ __forceinline__ unsigned w64_fetch_state(const Walk64Args& a, unsigned kind, unsigned row, unsigned c)
{
    const unsigned long idle = (unsigned long) a.prog;
    const unsigned long tip = kind == 2u ? ~0ul : 0ul;
    const unsigned long base = idle + ((((unsigned long) a.states + (unsigned long) row * (unsigned) a.Ppad) - idle) & tip);
    return *reinterpret_cast<const MBAMD_AS_GLOBAL uint8_t*>(base + (c & (unsigned) tip));
}
// The matrices of an entry: 2 children x KP categories x 16 doubles = KP / 2 doubles per lane (element g = t * 64 + lane:
// child g / (16 KP), category (g / 16) % KP, entry g % 16), parked in LDS as [child][category][18] (the two pad doubles keep
// the KP lane groups, which read at the same offset of different categories, on different banks) and read back by every lane
// from ITS category's rows.
template <int KP> struct Walk64Fetched {
    static constexpr int NL = KP >= 2 ? KP / 2 : 1;
    double m[NL];
    unsigned st1, st2;
};
template <int KP>
__device__ __forceinline__ void w64_fetch(const Walk64Args& a, const Walk64Entry& e, unsigned c, int lane, Walk64Fetched<KP>& f)
{
    const unsigned o1 = e.m1 * a.matDoubles * 8u, o2 = e.m2 * a.matDoubles * 8u;           // (below 4 GiB: the host checks)
#pragma unroll
    for (int t = 0; t < Walk64Fetched<KP>::NL; ++t) {
        const int g = (t * 64 + lane) & (32 * KP - 1);                                     // (KP = 1: lanes 32 .. 63 repeat)
        const int child = g / (16 * KP), cat = (g / 16) % KP, el = g % 16;
        const int kc = cat < a.K ? cat : a.K - 1;
        const unsigned off = (child ? o2 : o1) + (unsigned) (kc * 16 + el) * 8u;
        f.m[t] = *reinterpret_cast<const MBAMD_AS_GLOBAL double*>((unsigned long) a.matricesT + off);
    }
    f.st1 = w64_fetch_state(a, e.ctl & 3u, e.c1, c);
    f.st2 = w64_fetch_state(a, (e.ctl >> 2) & 3u, e.c2, c);
}

template <int KP>
__global__ void __launch_bounds__(64, 4)
k64_walk4(Walk64Args a)
{
    constexpr int PW = 64 / KP;                        // patterns per wave
    constexpr int NL = Walk64Fetched<KP>::NL;
    double* const slots = mbd_dyn_lds<double>();      // [slot][4][64] | matrices [2][KP][18]
    double* const mats = slots + (size_t) a.nslots * 4 * 64;
    const unsigned Ppad = (unsigned) a.Ppad;
    const int lane = (int) threadIdx.x & 63, kk = lane / PW;
    const int kc = kk < a.K ? kk : a.K - 1;            // (lanes beyond the last category repeat it)
    const unsigned c = blockIdx.x * (unsigned) PW + (unsigned) (lane % PW);
    const unsigned laneOff = ((unsigned) kc * 4u * Ppad + c) * 8u;        // this lane's (category, pattern) inside a buffer, bytes
    const unsigned scratchOff = (unsigned) a.scratchRow * Ppad * 4u + c * 4u;
    double* const mySlots = slots + lane;              // + slot * 256 + q * 64
    const double* const myMats = mats + kk * 18;       // + child * KP * 18
    int sum = 0;
    const MBAMD_AS_CONST Walk64Entry* cprog = as_const(a.prog);
    const int last = a.entries - 1;
    Walk64Entry cur = w64_load(cprog), nxt = w64_load(cprog + (last > 0 ? 1 : 0));
    // one entry: what it needs from HBM in `in` (fetched during the previous entry), the next entry's fetched into `next`
    auto step = [&](int j, const Walk64Fetched<KP>& in, Walk64Fetched<KP>& next) {
        w64_fetch<KP>(a, nxt, c, lane, next);          // (a harmless repeat of the last entry at the end)
        const unsigned kind1 = cur.ctl & 3u, kind2 = (cur.ctl >> 2) & 3u, mode = (cur.ctl >> 4) & 3u;
        const unsigned slot1 = (cur.ctl >> 8) & 0xFFu, slot2 = (cur.ctl >> 16) & 0xFFu, keep = cur.ctl >> 24;
#pragma unroll
        for (int t = 0; t < NL; ++t) {
            const int g = (t * 64 + lane) & (32 * KP - 1);
            mats[(g / 16) * 18 + g % 16] = in.m[t];
        }
        MBAMD_WAVE_SYNC();
        double out[4], f2[4], mx = 0.0;
        // a compact tip's factor is the row of its state (the gather the level kernels do; the product with an indicator vector
        // would add exact zeros to the same bits), missing data = 1
        auto factor = [&](unsigned kind, unsigned slot, unsigned buf, unsigned st, const double* m, double (&f)[4]) {
            if (kind == 2u) {
                const double* row = m + (st < 4u ? st : 0u) * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = st < 4u ? row[i] : 1.0;
                return;
            }
            double v[4];
            if (kind == 0u) {
                const double* sl = mySlots + (size_t) slot * 256;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = sl[q * 64];
            } else {
                const unsigned long base = (unsigned long) a.partials + (unsigned long) buf * a.bufDoubles * 8;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const MBAMD_AS_GLOBAL double*>(base + (unsigned long) q * Ppad * 8 + laneOff);
                MBAMD_CONSUME4(v[0], v[1], v[2], v[3]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) f[i] = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = fma(m[q * 4 + i], v[q], f[i]);
        };
        factor(kind1, slot1, cur.c1, in.st1, myMats, out);
        factor(kind2, slot2, cur.c2, in.st2, myMats + KP * 18, f2);
        MBAMD_WAVE_SYNC();                               // (the next entry's matrices overwrite these)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            out[i] *= f2[i];
            mx = fmax(mx, out[i]);
        }
        int ex = 0;
        if (mode == 1u) {
            mx = mbd_max_across_groups<PW>(mx);
            if (mx > 0.0 && mx < 1.0e300) (void) frexp(mx, &ex);
            ex = ex < -1000 ? -1000 : ex;
            sum += ex;
        } else if (mode == 2u) {
            ex = *reinterpret_cast<const MBAMD_AS_GLOBAL int32_t*>((unsigned long) a.scale + (unsigned long) cur.scaleR * Ppad * 4 + c * 4u);
            MBAMD_CONSUME1(ex);
        }
        const unsigned long dst = (unsigned long) a.partials + (unsigned long) cur.dst * a.bufDoubles * 8;
        // (category 0's lanes store the pattern's exponent; an entry without a scale buffer: scaleW is the scratch row)
        const unsigned scaleOff = kk == 0 ? cur.scaleW * Ppad * 4u + c * 4u : scratchOff;
        // the descriptor after next: a scalar load that the stores below and the next entry's fetch hide
        cur = nxt;
        nxt = w64_load(cprog + (j + 2 < last ? j + 2 : last));
        double v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = ex != 0 ? ldexp(out[i], -ex) : out[i];
            // (non-temporal: with write-allocate the result stream evicts matrices and programs from L2)
            MBAMD_STORE_NT(v[i], reinterpret_cast<MBAMD_AS_GLOBAL double*>(dst + (unsigned long) i * Ppad * 8 + laneOff));
        }
        *reinterpret_cast<MBAMD_AS_GLOBAL int32_t*>((unsigned long) a.scale + scaleOff) = ex;
        if (keep != 0xFFu) {
            double* sl = mySlots + (size_t) keep * 256;
#pragma unroll
            for (int i = 0; i < 4; ++i) sl[i * 64] = v[i];
        }
    };
    Walk64Fetched<KP> A, B;
    w64_fetch<KP>(a, cur, c, lane, A);
    step(0, A, B);
    for (int j = 1; j <= last; j += 2) {
        step(j, B, A);
        if (j + 1 > last) break;
        step(j + 1, A, B);
    }
    if (kk == 0 && a.cum != nullptr && sum != 0) as_global(a.cum)[c] += sum;
}

struct MatrixJob64 {
    double* out;                 // [K][S][S] then transposed [K][S][SPAD]
    double length;
    const double* eig;           // [U | U^-1 | lambda]
    double pad_;                 // host side: the derivative order of the job (0, 1, 2), one launch per order
};
// (ORDER: 0 = the probabilities, 1 / 2 = their first / second derivative in the branch length -- deriv_exponential, mbamd_kernels.h)
// CX: a complex eigen-system (complex_factor, mbamd_kernels.h), [U | U^-1 | lambda | b | side] in this engine.  The factor pair goes
// to ev[g] (C) and ev[total + g] (G); the matrix kernels' left operand is U[i,s] C[s] + U[i,partner[s]] G[s], partner[s] = s + side[s].
__host__ __device__ inline size_t eigen_imag_offset64(int S) { return (size_t) 2 * S * S + S; }
template <int ORDER, bool CX = false>
__global__ void __launch_bounds__(256)
k64_exponentials(const MatrixJob64* __restrict__ jobs, RatesArg rates, int S, int K, int total, double* __restrict__ ev)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int s = g % S, bk = g / S;
    const int b = bk / K, k = bk % K;
    if constexpr (CX) {
        const EigenFactor f = complex_factor<ORDER>(jobs[b].eig + eigen_imag_offset64(S), S, s, jobs[b].eig[(size_t) 2 * S * S + s], jobs[b].length, rates.r[k]);
        ev[g] = f.c;
        ev[(size_t) total + g] = f.g;
    } else {
        ev[g] = deriv_exponential<ORDER>(exp(jobs[b].eig[(size_t) 2 * S * S + s] * jobs[b].length * rates.r[k]), jobs[b].eig[(size_t) 2 * S * S + s], rates.r[k]);
    }
}
// TiProbs_Gen (reference src/likelihood.c:9498-9545): P_k = U diag(exp(lambda t r_k)) U^-1, negatives clamped to zero
template <int ORDER> __device__ __forceinline__ double matrix_entry64(double sum)
{
    if constexpr (ORDER == 0) return sum < 0.0 ? 0.0 : sum;
    return sum;
}
template <int ORDER, bool CX = false>
__global__ void __launch_bounds__(256)
k64_matrices(const MatrixJob64* __restrict__ jobs, const double* __restrict__ ev, int S, int SPAD, int K)
{
    const int b = blockIdx.x / K, k = blockIdx.x % K;
    const double* __restrict__ U = jobs[b].eig;
    const double* __restrict__ Ui = jobs[b].eig + (size_t) S * S;
    const double* __restrict__ e = ev + (size_t) blockIdx.x * S;
    double* __restrict__ M = jobs[b].out + (size_t) k * S * S;
    double* __restrict__ MT = jobs[b].out + (size_t) K * S * S + (size_t) k * S * SPAD;
    for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx % S;
        double sum = 0.0;
        if constexpr (CX) {
            const double* __restrict__ g = e + (size_t) gridDim.x * S;
            const double* __restrict__ side = jobs[b].eig + eigen_imag_offset64(S) + S;
            for (int s = 0; s < S; ++s) sum += (U[i * S + s] * e[s] + U[i * S + s + (int) side[s]] * g[s]) * Ui[s * S + j];
        } else {
            for (int s = 0; s < S; ++s) sum += U[i * S + s] * e[s] * Ui[s * S + j];
        }
        const double v = matrix_entry64<ORDER>(sum);
        M[(size_t) i * S + j] = v;
        MT[(size_t) j * SPAD + i] = v;
    }
}

// the same product on the fp64 matrix cores for 16 <= S <= 64 (one wave per 16 rows, as k_transition_matrices_mfma of the fp32 engine)
template <int NJ, int ORDER, bool CX = false>
__global__ void __launch_bounds__(64 * NJ)
k64_matrices_mfma(const MatrixJob64* __restrict__ jobs, const double* __restrict__ ev, int S, int SPAD, int K)
{
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int b = blockIdx.x / K, k = blockIdx.x % K;
    const MBAMD_AS_GLOBAL double* __restrict__ U = as_global(jobs[b].eig);
    const MBAMD_AS_GLOBAL double* __restrict__ Ui = U + (size_t) S * S;
    const MBAMD_AS_GLOBAL double* __restrict__ e = as_global(ev) + (size_t) blockIdx.x * S;    const int wave = (int) threadIdx.x >> 6, lane = (int) threadIdx.x & 63, li = lane & 15, ls = lane >> 4;
    const int i = 16 * wave + li, ic = i < S ? i : S - 1;
    d4 acc[NJ];
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) acc[jt] = (d4) (0.0);
    int jc[NJ];
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) jc[jt] = 16 * jt + li < S ? 16 * jt + li : S - 1;
    const int steps = (S + 3) / 4;
    for (int st0 = 0; st0 < steps; st0 += 4) {
        double a[4], bb[4][NJ];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = 4 * (st0 + u) + ls, sc = s < S ? s : S - 1;
            if constexpr (CX) {         // G lies behind the C of every block; the partner column is a second load of U
                const MBAMD_AS_GLOBAL double* __restrict__ eg = e + (size_t) gridDim.x * S;
                const int sp = sc + (int) U[eigen_imag_offset64(S) + S + sc];
                a[u] = (s < S && i < S) ? U[(size_t) ic * S + sc] * e[sc] + U[(size_t) ic * S + sp] * eg[sc] : 0.0;
            } else {
                a[u] = (s < S && i < S) ? U[(size_t) ic * S + sc] * e[sc] : 0.0;
            }
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt) bb[u][jt] = Ui[(size_t) sc * S + jc[jt]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt) acc[jt] = mbd_mfma_f64_16x16x4(a[u], bb[u][jt], acc[jt]);
    }
    MBAMD_AS_GLOBAL double* __restrict__ M = as_global(jobs[b].out) + (size_t) k * S * S;
    MBAMD_AS_GLOBAL double* __restrict__ MT = as_global(jobs[b].out) + (size_t) K * S * S + (size_t) k * S * SPAD;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + ls + 4 * r, j = 16 * jt + li;
            if (row < S && j < S) {
                const double v = matrix_entry64<ORDER>(acc[jt][r]);
                M[(size_t) row * S + j] = v;
                MT[(size_t) j * SPAD + row] = v;
            }
        }
}

// Likelihood_* (reference src/likelihood.c:5764-5917, 6975-7040) with BEAGLE's root / edge semantics; one thread per pattern
struct IntegrateArgs64 {
    const double*  parent[MBAMD_MAX_SUBSETS];
    const void*    child[MBAMD_MAX_SUBSETS];      // nullptr: root integration
    const double*  matrix[MBAMD_MAX_SUBSETS];     // [K][S][S]
    const double*  weights[MBAMD_MAX_SUBSETS];
    const double*  freqs[MBAMD_MAX_SUBSETS];
    const int32_t* cum[MBAMD_MAX_SUBSETS];
    uint8_t        child_tip[MBAMD_MAX_SUBSETS];
    int            count;
};
// category k's term of subset n at pattern c, over the from-states i0, i0 + istep, ...: parent x (what the child end contributes) x frequency
__device__ __forceinline__ double f64_category_term(const IntegrateArgs64& a, int n, int k, size_t c, int S, size_t Ppad, int i0, int istep)
{
    const double* par = a.parent[n] + (size_t) k * S * Ppad + c;
    double cat = 0.0;
    if (a.child[n] == nullptr) {
        for (int i = i0; i < S; i += istep) cat += par[(size_t) i * Ppad] * a.freqs[n][i];
    } else if (a.child_tip[n]) {
        const unsigned s = reinterpret_cast<const uint8_t*>(a.child[n])[c];
        for (int i = i0; i < S; i += istep) {
            const double pc = s >= (unsigned) S ? 1.0 : a.matrix[n][((size_t) k * S + i) * S + s];
            cat += par[(size_t) i * Ppad] * pc * a.freqs[n][i];
        }
    } else {
        const double* ch = reinterpret_cast<const double*>(a.child[n]) + (size_t) k * S * Ppad + c;
        for (int i = i0; i < S; i += istep) {
            const double* row = a.matrix[n] + ((size_t) k * S + i) * S;
            double acc = 0.0;
            for (int j = 0; j < S; ++j) acc = fma(row[j], ch[(size_t) j * Ppad], acc);
            cat += par[(size_t) i * Ppad] * acc * a.freqs[n][i];
        }
    }
    return cat;
}
__global__ void __launch_bounds__(64)
k64_integrate(IntegrateArgs64 a, int S, int K, int first, int last, int Ppad_, const double* __restrict__ pattern_weights,
              double* __restrict__ site, double* __restrict__ wsite)
{
    // patterns [first, last): everything, or one partition; blocks are counted from the 64-pattern block that holds `first`
    const size_t Ppad = (size_t) Ppad_, c = (size_t) (first / 64 + (int) blockIdx.x) * 64 + threadIdx.x;
    double wl = 0.0;
    if (c >= (size_t) first && c < (size_t) last) {
        int emax = -2147483647;
        for (int n = 0; n < a.count; ++n) {
            const int e = a.cum[n] ? a.cum[n][c] : 0;
            emax = e > emax ? e : emax;
        }
        double total = 0.0;
        for (int n = 0; n < a.count; ++n) {
            double like = 0.0;
            for (int k = 0; k < K; ++k) like += f64_category_term(a, n, k, c, S, Ppad, 0, 1) * a.weights[n][k];
            const int e = a.cum[n] ? a.cum[n][c] : 0;
            total += ldexp(like, e - emax);
        }
        const double lnl = log(total) + (double) emax * 0.69314718055994530942;
        site[c] = lnl;
        wl = lnl * pattern_weights[c];
    }
    mbd_wave_sum_store(wl, wsite + blockIdx.x);
}

// The same for larger state counts: eight threads per pattern (thread group g takes the from-states i = g, g + 8, ...), their
// partial sums added in a fixed order by the pattern's first thread -- an eighth of the serial chain (61 states, three omega
// classes, one thread per pattern: 78 us for 5 000 patterns).  block = 512: thread = g * 64 + pattern.
__global__ void __launch_bounds__(512)
k64_integrate_wide(IntegrateArgs64 a, int S, int K, int first, int last, int Ppad_, const double* __restrict__ pattern_weights,
                   double* __restrict__ site, double* __restrict__ wsite)
{
    double (*part)[8][64] = reinterpret_cast<double (*)[8][64]>(mbd_dyn_lds<double>());       // [subset][group][pattern]
    const int p = (int) threadIdx.x & 63, g = (int) threadIdx.x >> 6;
    const size_t Ppad = (size_t) Ppad_, c = (size_t) (first / 64 + (int) blockIdx.x) * 64 + p;
    const bool live = c >= (size_t) first && c < (size_t) last;
    for (int n = 0; n < a.count; ++n) {
        double like = 0.0;
        if (live) {
            for (int k = 0; k < K; ++k) like += f64_category_term(a, n, k, c, S, Ppad, g, 8) * a.weights[n][k];
        }
        part[n][g][p] = like;
    }
    MBAMD_SYNC();
    if (g != 0) return;
    double wl = 0.0;
    if (live) {
        int emax = -2147483647;
        for (int n = 0; n < a.count; ++n) {
            const int e = a.cum[n] ? a.cum[n][c] : 0;
            emax = e > emax ? e : emax;
        }
        double total = 0.0;
        for (int n = 0; n < a.count; ++n) {
            const double like = ((part[n][0][p] + part[n][1][p]) + (part[n][2][p] + part[n][3][p])) +
                                ((part[n][4][p] + part[n][5][p]) + (part[n][6][p] + part[n][7][p]));
            const int e = a.cum[n] ? a.cum[n][c] : 0;
            total += ldexp(like, e - emax);
        }
        const double lnl = log(total) + (double) emax * 0.69314718055994530942;
        site[c] = lnl;
        wl = lnl * pattern_weights[c];
    }
    mbd_wave_sum_store(wl, wsite + blockIdx.x);
}

__global__ void __launch_bounds__(256)
k64_scale_accumulate(const int32_t* const* __restrict__ src, int count, int sign, int first, int last, int32_t* __restrict__ cum)
{
    const int c = first + (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= last) return;
    int s = 0;
    for (int i = 0; i < count; ++i) s += src[i][c];
    cum[c] += sign * s;
}

}  // namespace mbamd
#endif
