// mbamd_ancestral_sampling.h -- one draw of all ancestral states from their JOINT posterior given the data
// (mbamdSampleAncestralStates; semantics: include/libhmsbeagle/mbamd_reports.h).  Included by mbamd_f32.h and
// mbamd_f64.h; product and TEST-ONLY host emulation compile these same kernels.
//
// The joint posterior of a pattern factorises down the tree: a rate category k from the posterior category probabilities q_k(c) of
// the latest log-likelihood call, the state at the top given k from that call's operands, then every child given ITS PARENT'S
// SAMPLED STATE a and k,
//     P(b | a, k) ~ P_k[a,b] post_child[k,c,b]
// -- the child's post-order column is all the data below it, and given the parent's state nothing above the branch matters.  So the
// draw reads post-order buffers only: no pre-order pass, no pre-order buffer, and of each child ONE category column and ONE matrix
// row.  Whatever scale a column (pattern, category) carries leaves the normalised weights.
//
// Arithmetic: each weight is one product in the engine's precision (the top's: the `cat` terms of k_category_posteriors), widened
// to double; sample_pick sums them in double in ascending state order, twice -- the total, then the running sum that meets
// x = u T -- with contraction off, so that both walks add the same rounded weights.  Uniforms are counter-based (sample_uniform):
// a draw depends on (seed, stream, the pattern's index in the instance) and on nothing else.
#ifndef MBAMD_ANCESTRAL_SAMPLING_H_
#define MBAMD_ANCESTRAL_SAMPLING_H_

#include "mbamd_preorder.h"      // DerivArgs and the layout accessors, k_gradient_sums, ensure_posteriors, the engine hooks

namespace mbamd {

// one edge of a sampling call
struct SampleEdge {
    const void* post;             // the child's post-order partials, or compact tip states (postTip)
    const void* matrix;           // the transition matrix of its branch
    int         postTip;
    int         parentSlot;       // the slot the edge hangs from
};
// g: for k_sample_top the operands of the latest log-likelihood call (ensure_posteriors' DerivArgs), for k_sample_edges the layout.
// Patterns first .. first + width of the engine are in flight (width a multiple of 64): the per-pattern arrays are indexed from `first`.
struct SampleArgs {
    DerivArgs          g;
    const SampleEdge*  edges;     // the edges of this launch (grid y); edge blockIdx.y of the launch is edge firstEdge + blockIdx.y of the call
    const double*      q;         // [K][Ppad] posterior category probabilities, or null (one category: k = 0)
    const double*      pattern_weights;
    int32_t*           cat;       // [width] the drawn category, -1: none
    uint8_t*           states;    // [slots][width] the drawn states, 255: none
    double*            sums;      // [edges of the call][nb]: weight_c [state(child) != state(parent)], one per 64-pattern block
    unsigned long long seed;
    long long          patternOffset;      // the index in the instance of the engine's pattern 0
    int                first, width, nb;   // nb: the 64-pattern blocks of this launch (the grid's x), at most width / 64
    int                firstEdge;
};

constexpr uint8_t SAMPLE_NONE = 255;

__host__ __device__ __forceinline__ unsigned long long sample_mix(unsigned long long x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// u(seed, stream, c) in [0, 1): stream 0 the category, 1 the top, 2 + i edge i; c the pattern's index in the instance
__host__ __device__ __forceinline__ double sample_uniform(unsigned long long seed, unsigned long long stream, unsigned long long c)
{
    const unsigned long long G = 0x9E3779B97F4A7C15ull;
    return (double) (sample_mix(sample_mix(seed + G * (stream + 1)) + G * (c + 1)) >> 11) * 0x1.0p-53;
}

// The selection rule over the weights weight(0 .. n): -1 unless their ascending sum T is positive; else the smallest index whose
// running sum exceeds x = u T, or, where rounding leaves none, the largest index of positive weight.  A weight of 0 is never chosen.
template <class W>
__device__ __forceinline__ int sample_pick(int n, double u, W&& weight)
{
#pragma clang fp contract(off)
    double T = 0.0;
    for (int i = 0; i < n; ++i) T += weight(i);
    if (!(T > 0.0)) return -1;
    const double x = u * T;
    double run = 0.0;
    int last = -1;
    for (int i = 0; i < n; ++i) {
        const double v = weight(i);
        run += v;
        if (v > 0.0) {
            if (x < run) return i;
            last = i;
        }
    }
    return last;
}
// ... over four weights in registers
__device__ __forceinline__ int sample_pick4(double v0, double v1, double v2, double v3, double u)
{
#pragma clang fp contract(off)
    const double r1 = v0 + v1, r2 = r1 + v2, T = r2 + v3;
    if (!(T > 0.0)) return -1;
    const double x = u * T;
    if (v0 > 0.0 && x < v0) return 0;
    if (v1 > 0.0 && x < r1) return 1;
    if (v2 > 0.0 && x < r2) return 2;
    if (v3 > 0.0 && x < T) return 3;
    return v3 > 0.0 ? 3 : v2 > 0.0 ? 2 : v1 > 0.0 ? 1 : 0;
}

// The category and the top state of every pattern: one thread per pattern, grid = the 64-pattern blocks in flight.  The top's weight
// of state i in category k is the term k_category_posteriors adds to `cat`: freqs[i] parent[k,c,i] f_k(i), f the factor of the
// log-likelihood call's child across its matrix (a root call: 1).  f is an S-term chain, and the column is walked twice (sample_pick):
// this kernel runs once per call.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_sample_top(SampleArgs a)
{
    const DerivArgs& g = a.g;
    const int S = g.S, K = g.K;
    const int at = (int) blockIdx.x * 64 + (int) threadIdx.x;
    const int c = a.first + at;
    if (c >= g.last) return;
    const unsigned long long ci = (unsigned long long) (a.patternOffset + c);
    int k = 0;
    if (a.q != nullptr) k = sample_pick(K, sample_uniform(a.seed, 0, ci), [&](int kk) { return a.q[(size_t) kk * g.Ppad + c]; });
    int top = -1;
    if (k >= 0) {
        const unsigned tip = g.child_tip ? deriv_tip<LAYOUT>(g.child, g, c) : 0u;
        top = sample_pick(S, sample_uniform(a.seed, 1, ci), [&](int i) {
            Real f = (Real) 1;
            if (g.child != nullptr) {
                if (g.child_tip && LAYOUT != DERIV_S4) {
                    if (tip < (unsigned) S) f = deriv_matrix<LAYOUT, Real>(g.matrix[0], g, k, i, (int) tip);
                } else {
                    f = (Real) 0;
                    for (int j = 0; j < S; ++j) {
                        const Real v = g.child_tip ? ((tip >> j & 1u) ? (Real) 1 : (Real) 0) : deriv_partial<LAYOUT, Real>(g.child, g, k, j, c);
                        f = deriv_fma(deriv_matrix<LAYOUT, Real>(g.matrix[0], g, k, i, j), v, f);
                    }
                }
            }
            return (double) (deriv_partial<LAYOUT, Real>(g.parent, g, k, i, c) * f) * g.freqs[i];
        });
    }
    a.cat[at] = k;
    a.states[at] = top < 0 ? SAMPLE_NONE : (uint8_t) top;
}

// The lower ends of the edges of one launch, whose parents' states are all there: grid (64-pattern blocks in flight, edges), one
// thread per pattern.  A thread reads its pattern's category and its parent's state, then ONE category column of the child and ONE
// matrix row -- in the four-state layout an f4 and four matrix values; in the other layouts the column is not kept (as a private
// array indexed at run time it would be scratch: k_node_posteriors) but walked twice, the second walk finding the S values in the
// cache.  A compact tip with one compatible state is that state, without arithmetic; a missing state leaves the matrix row, the
// four-state bitplanes the compatible columns.
template <int LAYOUT, class Real>
__global__ void __launch_bounds__(64)
k_sample_edges(SampleArgs a)
{
    const DerivArgs& g = a.g;
    const int S = g.S;
    const int at = (int) blockIdx.x * 64 + (int) threadIdx.x;
    const int c = a.first + at;
    const size_t edge = (size_t) a.firstEdge + blockIdx.y;
    const SampleEdge ed = a.edges[blockIdx.y];
    double changed = 0.0;
    if (c < g.last) {
        const int k = a.cat[at];
        const uint8_t up = a.states[(size_t) ed.parentSlot * a.width + at];
        int b = -1;
        if (k >= 0 && up != SAMPLE_NONE) {
            const int from = (int) up;
            const unsigned tip = ed.postTip ? deriv_tip<LAYOUT>(ed.post, g, c) : 0u;
            const double u = sample_uniform(a.seed, 2 + (unsigned long long) edge, (unsigned long long) (a.patternOffset + c));
            if constexpr (LAYOUT == DERIV_S4) {
                if (ed.postTip && tip != 0u && (tip & (tip - 1u)) == 0u) {
                    b = (tip & 1u) ? 0 : (tip & 2u) ? 1 : (tip & 4u) ? 2 : 3;
                } else {
                    const float* m = reinterpret_cast<const float*>(ed.matrix) + k * 16 + from;          // m[j * 4] = P(from -> j)
                    float w[4] = {m[0], m[4], m[8], m[12]};
                    if (ed.postTip) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) w[j] = (tip >> j & 1u) ? w[j] : 0.0f;
                    } else {
                        const f4 p4 = reinterpret_cast<const f4*>(ed.post)[blk_index(c, g.pstride) + (size_t) k * 64];
                        w[0] *= p4.x; w[1] *= p4.y; w[2] *= p4.z; w[3] *= p4.w;
                    }
                    b = sample_pick4((double) w[0], (double) w[1], (double) w[2], (double) w[3], u);
                }
            } else {
                if (ed.postTip && tip < (unsigned) S) {
                    b = (int) tip;
                } else {
                    b = sample_pick(S, u, [&](int j) {
                        const Real p = deriv_matrix<LAYOUT, Real>(ed.matrix, g, k, from, j);
                        // (a compact tip here has a missing state: the vector of ones)
                        return (double) (ed.postTip ? p : p * deriv_partial<LAYOUT, Real>(ed.post, g, k, j, c));
                    });
                }
            }
            if (b >= 0 && b != from) changed = a.pattern_weights[c];
        }
        a.states[(edge + 1) * a.width + at] = b < 0 ? SAMPLE_NONE : (uint8_t) b;
    }
    mbd_wave_sum_store(changed, a.sums + edge * a.nb + blockIdx.x);
}

// ---- host side, shared by the two engines (the hooks: mbamd_preorder.h) ------------------------------------------------------

// An edge list cut into launches: start[g] .. start[g + 1] are the edges of launch g.  A launch holds consecutive edges whose parent
// slots all lie before its first slot -- the greedy cut of pre_order_groups --, at most 32768 of them (the edge is a grid
// dimension).  A breadth-first list gives one launch per level of the tree.
inline void sample_groups(const int* parentSlots, int n, std::vector<int>& start)
{
    const int maxEdges = 32768;
    start.assign(1, 0);
    for (int i = 0; i < n; ++i) {
        // (slot i + 1 is edge i's: the launch that begins with edge s has slots 0 .. s before it)
        if (parentSlots[i] > start.back() || i - start.back() >= maxEdges) start.push_back(i);
    }
    if (n > 0) start.push_back(n);
}

// mbamdSampleAncestralStates on the engine's patterns.  patternOffset is the index in the instance of the engine's pattern 0 (the
// uniforms are the instance's); states (never null) takes slot s of pattern c at [s * stride + c], categories (or null) k of
// pattern c at [c], changes (never null here) the engine's weighted number of changes on edge i at [i].  The device keeps the drawn
// states as bytes, [slot][width], for the patterns in flight: all of the engine's, or, where that much scratch cannot be had
// (MBAMD_SAMPLE_PATTERNS, test only: at most that many), one range of them after another -- patterns are independent, and the
// ranges' sums are added in pattern order.  Per range: k_sample_top, one k_sample_edges per group, k_gradient_sums (mbamdKernelTiming
// reports their launches and, on the single-precision engine, their device time).  Synchronous.
template <class Engine>
inline int sample_ancestral_states(Engine& e, const int* parentSlots, const int* post, const int* matrices, int count, int wIdx,
                                   unsigned long long seed, long long patternOffset, int* states, int* categories, double* changes, size_t stride)
{
    const char* const who = "mbamdSampleAncestralStates";
    { const int rc = e.runQueued(); if (rc) return rc; }
    { const int rc = e.refuses(who); if (rc) return rc; }
    if (e.lastLnl.count == 0)
        return fail(BEAGLE_ERROR_GENERAL, who, "no log-likelihood was calculated yet: the top's frequencies and the category posteriors come from its operands");
    if (e.lastLnl.count > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "the latest log-likelihood call had more than one subset");
    if (wIdx != e.lastLnl.weights) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "category weights index differs from the latest log-likelihood call's");
    if (e.S >= (int) SAMPLE_NONE) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "more than 254 states");
    for (int i = 0; i < count; ++i) {
        if (parentSlots[i] < 0 || parentSlots[i] > i) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a parent slot is not an earlier slot of the list");
        if (post[i] < 0 || post[i] >= e.nBuffers || !e.readable(post[i])) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "post-order buffer");
        if (matrices[i] < 0 || matrices[i] >= e.nMatrices) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "matrix index");
    }
    count = std::max(count, 0);
    SampleArgs top;
    std::memset(&top, 0, sizeof top);
    // the buffers are in memory, q is that of the latest log-likelihood call, and its operands (checked) are the top's
    { const int rc = e.beforeRead(count, [&](int i) { return post[i]; }); if (rc) return rc; }
    if (e.K > 1) { const int rc = ensure_posteriors(e); if (rc) return rc; }
    { const int rc = e.posteriorOperands(top.g); if (rc) return rc; }
    std::vector<SampleEdge> table((size_t) std::max(count, 1));
    for (int i = 0; i < count; ++i) {
        SampleEdge& t = table[(size_t) i];
        std::memset(&t, 0, sizeof t);
        t.postTip = e.holdsTip(post[i]) ? 1 : 0;
        t.post = e.operandPtr(post[i]);
        t.matrix = e.matrixPtr(matrices[i]);
        t.parentSlot = parentSlots[i];
    }
    void* d_table = nullptr;
    if (count > 0) { const int rc = e.stageTable(table.data(), (size_t) count * sizeof(SampleEdge), &d_table); if (rc) return rc; }
    std::vector<int> start;
    sample_groups(parentSlots, count, start);

    // the patterns in flight, and the scratch behind them: block sums and sums (doubles), categories, states
    const size_t slots = (size_t) count + 1;
    int width = e.Ppad;
    if (e.sw.samplePatterns.value_or(0) > 0) width = std::min(width, (*e.sw.samplePatterns + 63) / 64 * 64);
    double* d_scratch = nullptr;
    auto scratch_bytes = [&](int w) { return ((size_t) count * (w / 64) + count) * sizeof(double) + (size_t) w * sizeof(int32_t) + slots * w; };
    for (;;) {
        const int rc = e.resultScratch(scratch_bytes(width), &d_scratch);
        if (rc == BEAGLE_SUCCESS) break;
        if (rc != BEAGLE_ERROR_OUT_OF_MEMORY || width <= 64) return rc;
        (void) hipGetLastError();
        width = (width / 2 + 63) / 64 * 64;
    }
    const int nb = width / 64;
    double* const d_sums = d_scratch;
    double* const d_out = d_sums + (size_t) count * nb;
    int32_t* const d_cat = reinterpret_cast<int32_t*>(d_out + count);
    uint8_t* const d_states = reinterpret_cast<uint8_t*>(d_cat + width);

    top.q = e.K > 1 ? e.d_q : nullptr;
    top.pattern_weights = e.d_pweights;
    top.cat = d_cat;
    top.states = d_states;
    top.sums = d_sums;
    top.seed = seed;
    top.patternOffset = patternOffset;
    top.width = width;
    SampleArgs edges = top;
    edges.g = e.layoutArgs();
    std::vector<uint8_t> hStates(slots * (size_t) width);
    std::vector<int32_t> hCat((size_t) width);
    std::vector<double> hSums((size_t) count);
    std::fill(changes, changes + count, 0.0);
    for (int first = 0; first < e.P; first += width) {
        const int n = std::min(width, e.P - first), blocks = (n + 63) / 64;
        top.first = edges.first = first;
        top.nb = edges.nb = blocks;
        hipEvent_t ev0{}, ev1{};
        { const int rc = e.timedBegin(ev0, ev1); if (rc) return rc; }
        e.withLayout([&](auto L) {
            auto kernel = k_sample_top<L(), deriv_real<L()>>;
            MBAMD_LAUNCH(kernel, (unsigned) blocks, 64, 0, e.stream, top);
        });
        HIP_TRY(hipGetLastError());
        for (size_t gI = 0; gI + 1 < start.size(); ++gI) {
            edges.edges = static_cast<const SampleEdge*>(d_table) + start[gI];
            edges.firstEdge = start[gI];
            const dim3 grid((unsigned) blocks, (unsigned) (start[gI + 1] - start[gI]));
            e.withLayout([&](auto L) {
                auto kernel = k_sample_edges<L(), deriv_real<L()>>;
                MBAMD_LAUNCH(kernel, grid, 64, 0, e.stream, edges);
            });
            HIP_TRY(hipGetLastError());
        }
        if (count > 0) {
            MBAMD_LAUNCH(k_gradient_sums, dim3((unsigned) count, 1u), 64, 0, e.stream, (const double*) d_sums, blocks, count, d_out);
            HIP_TRY(hipGetLastError());
        }
        { const int rc = e.timedEnd(ev0, ev1); if (rc) return rc; }
        e.countLaunches((int) start.size() + (count > 0 ? 1 : 0));
        HIP_TRY(hipStreamSynchronize(e.stream));
        e.afterSync();
        HIP_TRY(hipMemcpy(hStates.data(), d_states, hStates.size(), hipMemcpyDeviceToHost));
        if (categories) HIP_TRY(hipMemcpy(hCat.data(), d_cat, hCat.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (count > 0) HIP_TRY(hipMemcpy(hSums.data(), d_out, hSums.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < slots; ++s)
            for (int c = 0; c < n; ++c) {
                const uint8_t v = hStates[s * width + c];
                states[s * stride + first + c] = v == SAMPLE_NONE ? -1 : (int) v;
            }
        if (categories) std::memcpy(categories + first, hCat.data(), (size_t) n * sizeof(int32_t));
        for (int i = 0; i < count; ++i) changes[i] += hSums[(size_t) i];
    }
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd
#endif
