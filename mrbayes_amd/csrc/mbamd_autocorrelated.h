// mbamd_autocorrelated.h -- the site-order hidden Markov model over the rate categories (Yang's autocorrelated discrete gamma, the
// Felsenstein-Churchill HMM) on the device: mbamdCalculateAutocorrelatedLogLikelihood (semantics: include/libhmsbeagle/mbamd_reports.h,
// DESIGN 4.4.9).  Included by mbamd_f32.h and mbamd_f64.h; product and TEST-ONLY host emulation compile these same kernels.
//
// The call reads two arrays of doubles that both engines keep of their latest log-likelihood call -- q [K][Ppad], the category
// posteriors (ensure_posteriors), and the site log-likelihoods l -- and never the partials: ONE code path, all of it in double.
//     ln H = sum_s l(c_s) + ln( 1^T A_0 A_1 ... A_{n-1} 1 )
//     A_0 = diag(q_k(c_0)),   A_s = T^(j_s) diag(q_k(c_s) / w_k)   (s >= 1)
// (1^T A_0 = u^T of the header).  The ordered product is associative: a tree reduction with ONE chunk length, HMM_CHUNK.
//     k_hmm_products<true>    every run of HMM_CHUNK sites  -> its ordered K x K product, the sum of its l (in site order)
//     k_hmm_products<false>   every run of HMM_CHUNK products -> one, level after level until one is left
// One wave per chunk; entry [a][b] of the running product belongs to lane (a K + b) mod 64 (four entries per lane at K = 16), the
// row of the left factor is exchanged through LDS, the items of a chunk go one after the other.  After EVERY item the product is
// scaled by an exact power of two that takes its largest entry into [1, 2) (frexp / ldexp), and the integer exponent is carried
// beside the product: scaling rounds nothing, and nothing underflows at any n.
//
// The posteriors gamma_s(k), if asked for, come from the same products: k_hmm_vectors hands the entry vector (1^T times everything
// before) and the exit vector (everything behind times 1) of every node of a level down to its children -- vector x matrix steps,
// the forward walk in the lower half-wave, the backward walk in the upper --, then k_hmm_posteriors re-walks every chunk of sites
// from its two vectors and writes alpha_s(k) beta_s(k), normalised per site.  The vectors are scaled like the products; their
// exponents cancel in gamma and are not kept.
#ifndef MBAMD_AUTOCORRELATED_H_
#define MBAMD_AUTOCORRELATED_H_

#include <math.h>

#include <cmath>

#include "mbamd_preorder.h"      // ensure_posteriors, the engine hooks

namespace mbamd {

constexpr int HMM_CHUNK = 64;    // R: items per chunk, at every level of the reduction

// where the inputs of one engine lie (device-readable): q [K][qStride] (null: one category), the site log-likelihoods (siteHost:
// their host address where they lie in pinned host memory, else null), and the patterns of the instance they stand for
struct HmmSource {
    const double* q;
    const double* site;
    const double* siteHost;
    size_t        qStride;
    int           start, count;
};

// One level of the reduction: `count` items (sites at the leaf level, products above) become ceil(count / HMM_CHUNK) products.
struct HmmArgs {
    // the call (leaf level and k_hmm_posteriors)
    const double* q;              // [K][qStride], or null (one category)
    const double* site;           // [patterns] site log-likelihoods
    const double* weights;        // [K] category weights
    const double* powers;         // [distinct jumps][K][K]: T^(j)
    const int*    patterns;       // [n] c_s
    const int*    jumps;          // [n] the row of `powers` of site s (site 0: unused), or null (one row)
    size_t        qStride;
    int           K, n;
    // the items of this level (null at the leaf level) and what it leaves
    const double* inProd;         // [count][K][K]
    const double* inSum;          // [count]
    const int*    inExp;          // [count]
    int           count;
    double*       prod;           // [chunks][K][K]
    double*       sum;            // [chunks] the sum of l over the chunk's sites
    int*          exp;            // [chunks] the product is prod * 2^exp
    // the vectors: of this level's nodes (null: the top, ones) and, to fill, of its items
    const double* entry;          // [chunks][K]
    const double* exit;           // [chunks][K]
    double*       inEntry;        // [count][K]
    double*       inExit;         // [count][K]
    double*       gamma;          // [K][n] (k_hmm_posteriors)
};

// v scaled by the power of two that takes m (the largest of the values scaled together, >= 0) into [1, 2); the exponent taken out
__device__ __forceinline__ int hmm_exponent(double m)
{
    int ex = 0;
    if (m > 0.0 && m < INFINITY) { (void) frexp(m, &ex); --ex; }
    return ex;
}

// d_s[k] = q_k(c_s) / w_k, at site 0 q_k(c_0) itself (A_0 has no transition in front); one category: 1
__device__ __forceinline__ double hmm_emission(const HmmArgs& a, int s, int k)
{
    if (a.q == nullptr) return 1.0;
    const double q = a.q[(size_t) k * a.qStride + a.patterns[s]];
    return s == 0 ? q : q / a.weights[k];
}

// the row of `powers` that stands in front of site s (no array: every jump is the same)
__device__ __forceinline__ int hmm_row(const HmmArgs& a, int s) { return s == 0 || a.jumps == nullptr ? 0 : a.jumps[s]; }

// The exponent that takes the largest of the wave's values `mine` (>= 0) into [1, 2).  Non-negative doubles are ordered like their
// high words, so ONE 32-bit word per lane is exchanged; only where that word shows no normal number (zero, a denormal, not finite)
// -- the same in every lane -- are the doubles themselves compared.
__device__ __forceinline__ int hmm_wave_exponent(double mine)
{
    int hi = (int) (__builtin_bit_cast(unsigned long long, mine) >> 32);
    for (int w = 32; w > 0; w >>= 1) {
        const int other = __builtin_bit_cast(int, mbd_shfl_xor(__builtin_bit_cast(float, hi), w));
        hi = other > hi ? other : hi;
    }
    const int field = hi >> 20 & 0x7ff;
    if (field != 0 && field != 0x7ff) return field - 1023;
    double mx = mine;
    for (int w = 32; w > 0; w >>= 1) mx = fmax(mx, mbd_shfl_xor(mx, w));
    return hmm_exponent(mx);
}

// Grid: the chunks of the level.  LEAF: the items are sites, item s the matrix A_s; else the products of the level below.  The right
// factor of an item -- T^(j_s), or the item itself -- is fetched one item ahead into registers and handed to LDS with the running
// product, so that no step waits for memory.
template <bool LEAF>
__global__ void __launch_bounds__(64)
k_hmm_products(HmmArgs a)
{
    __shared__ double M[MBAMD_MAX_RATES * MBAMD_MAX_RATES];        // the running product, [a][b]
    __shared__ double F[MBAMD_MAX_RATES * MBAMD_MAX_RATES];        // the right factor of the step
    __shared__ double dS[LEAF ? HMM_CHUNK * MBAMD_MAX_RATES : 1];  // d_s[k] of the chunk's sites, [site][k]
    __shared__ double lS[HMM_CHUNK];
    __shared__ int jS[LEAF ? HMM_CHUNK : 1];                       // the chunk's rows of `powers`
    const int K = a.K, KK = K * K, lane = (int) threadIdx.x;
    const int first = (int) blockIdx.x * HMM_CHUNK, last = first + HMM_CHUNK < a.count ? first + HMM_CHUNK : a.count, cnt = last - first;
    lS[lane] = lane < cnt ? (LEAF ? a.site[a.patterns[first + lane]] : a.inSum[first + lane]) : 0.0;
    if (LEAF) {
        jS[lane] = lane < cnt ? hmm_row(a, first + lane) : 0;
        for (int i = lane; i < cnt * K; i += 64) dS[(i / K) * MBAMD_MAX_RATES + i % K] = hmm_emission(a, first + i / K, i % K);
    }
    MBAMD_SYNC();
    auto fetch = [&](int t, double* f) {
        const double* const src = LEAF ? a.powers + (size_t) jS[t - first] * KK : a.inProd + (size_t) t * KK;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int e = lane + 64 * i; f[i] = e < KK ? src[e] : 0.0; }
    };
    double m[4] = {0.0, 0.0, 0.0, 0.0}, f[4], next[4] = {0.0, 0.0, 0.0, 0.0};
    fetch(first, f);
    int E = 0;
    for (int t = first; t < last; ++t) {
        const double* const d = dS + (LEAF ? (t - first) * MBAMD_MAX_RATES : 0);
        if (t > first) {
            MBAMD_SYNC();
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int e = lane + 64 * i; if (e < KK) { M[e] = m[i]; F[e] = f[i]; } }
            MBAMD_SYNC();
        }
        if (t + 1 < last) fetch(t + 1, next);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane + 64 * i;
            if (e >= KK) continue;
            const int r = e / K, b = e % K;
            double v;
            if (t == first) {
                v = !LEAF ? f[i] : t == 0 ? (r == b ? d[b] : 0.0) : f[i] * d[b];
            } else {
                v = 0.0;
                for (int j = 0; j < K; ++j) v = fma(M[r * K + j], F[j * K + b], v);
                if (LEAF) v *= d[b];
            }
            m[i] = v;
        }
        if (!LEAF) E += a.inExp[t];
        const int ex = hmm_wave_exponent(fmax(fmax(m[0], m[1]), fmax(m[2], m[3])));
        if (ex != 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = ldexp(m[i], -ex);
            E += ex;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = next[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int e = lane + 64 * i; if (e < KK) a.prod[(size_t) blockIdx.x * KK + e] = m[i]; }
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < cnt; ++i) s += lS[i];
        a.sum[blockIdx.x] = s;
        a.exp[blockIdx.x] = E;
    }
}

// the largest of v over the 16 lanes of a quarter-wave, then v scaled into [1, 2) by it
__device__ __forceinline__ double hmm_scale16(double v)
{
    double mx = v;
    for (int w = 8; w > 0; w >>= 1) mx = fmax(mx, mbd_shfl_xor(mx, w));
    const int ex = hmm_exponent(mx);
    return ex != 0 ? ldexp(v, -ex) : v;
}

// Grid: the nodes of a level above the leaves.  Node g hands its entry vector x^T (the top: ones) forward through its items C_t,
//     entry(t) = x^T C_first ... C_{t-1}        (lanes 0 .. K-1, lane k the component k),
// and its exit vector y backward,
//     exit(t) = C_{t+1} ... C_{last-1} y        (lanes 32 .. 32+K-1),
// one item per step, both walks in the same loop.
__global__ void __launch_bounds__(64)
k_hmm_vectors(HmmArgs a)
{
    __shared__ double V[2][MBAMD_MAX_RATES];
    const int K = a.K, KK = K * K, lane = (int) threadIdx.x, half = lane >> 5, k = lane & 31;
    const bool on = k < K;
    const int first = (int) blockIdx.x * HMM_CHUNK, last = first + HMM_CHUNK < a.count ? first + HMM_CHUNK : a.count, cnt = last - first;
    const double* const mine = half ? a.exit : a.entry;
    double x = on ? (mine != nullptr ? mine[(size_t) blockIdx.x * K + k] : 1.0) : 0.0;
    for (int i = 0; i < cnt; ++i) {
        const int t = half ? last - 1 - i : first + i;
        if (on) (half ? a.inExit : a.inEntry)[(size_t) t * K + k] = x;
        MBAMD_SYNC();
        if (on) V[half][k] = x;
        MBAMD_SYNC();
        double v = 0.0;
        if (on) {
            const double* const C = a.inProd + (size_t) t * KK;
            for (int j = 0; j < K; ++j) v = fma(V[half][j], half ? C[k * K + j] : C[j * K + k], v);
        }
        x = hmm_scale16(v);
    }
}

// Grid: the chunks of sites.  From the chunk's entry and exit vectors (null: the only chunk, ones) the forward walk leaves
// alpha_s in LDS (lower half-wave), the backward walk beta_s (upper half-wave); then lane i writes gamma of the chunk's site i.
__global__ void __launch_bounds__(64)
k_hmm_posteriors(HmmArgs a)
{
    __shared__ double dS[HMM_CHUNK * MBAMD_MAX_RATES];             // [site][k], as in k_hmm_products
    __shared__ double AB[2][HMM_CHUNK * MBAMD_MAX_RATES];          // alpha_s[k] | beta_s[k]
    __shared__ double V[2][MBAMD_MAX_RATES];
    __shared__ int jS[HMM_CHUNK];
    const int K = a.K, KK = K * K, lane = (int) threadIdx.x, half = lane >> 5, k = lane & 31;
    const bool on = k < K;
    const int first = (int) blockIdx.x * HMM_CHUNK, last = first + HMM_CHUNK < a.n ? first + HMM_CHUNK : a.n, cnt = last - first;
    jS[lane] = lane < cnt ? hmm_row(a, first + lane) : 0;
    for (int i = lane; i < cnt * K; i += 64) dS[(i / K) * MBAMD_MAX_RATES + i % K] = hmm_emission(a, first + i / K, i % K);
    const double* const mine = half ? a.exit : a.entry;
    double x = on ? (mine != nullptr ? mine[(size_t) blockIdx.x * K + k] : 1.0) : 0.0;
    for (int i = 0; i < cnt; ++i) {
        // forward: alpha_s = (x^T T^(j_s)) o d_s, at site 0 x o d_0;  backward: beta_s = x, then x = T^(j_s) (d_s o x) for site s - 1
        const int at = half ? cnt - 1 - i : i, s = first + at;
        const double* const d = dS + at * MBAMD_MAX_RATES;
        MBAMD_SYNC();
        if (on) {
            if (half) AB[1][at * MBAMD_MAX_RATES + k] = x;
            V[half][k] = half ? d[k] * x : x;
        }
        MBAMD_SYNC();
        double v = 0.0;
        if (on) {
            if (s == 0) {
                v = half ? 0.0 : x * d[k];
            } else {
                const double* const Tj = a.powers + (size_t) jS[at] * KK;
                for (int j = 0; j < K; ++j) v = fma(V[half][j], half ? Tj[k * K + j] : Tj[j * K + k], v);
                if (!half) v *= d[k];
            }
        }
        x = hmm_scale16(v);
        if (on && !half) AB[0][at * MBAMD_MAX_RATES + k] = x;
    }
    MBAMD_SYNC();
    if (lane < cnt) {
        const double* const al = AB[0] + lane * MBAMD_MAX_RATES;
        const double* const be = AB[1] + lane * MBAMD_MAX_RATES;
        double total = 0.0;
        for (int j = 0; j < K; ++j) total += al[j] * be[j];
        for (int j = 0; j < K; ++j) a.gamma[(size_t) j * a.n + first + lane] = total > 0.0 && total < INFINITY ? al[j] * be[j] / total : 0.0;
    }
}

// ---- host side, shared by the two engines (the hooks: mbamd_preorder.h) ------------------------------------------------------

// T^(j), j >= 1, [K][K] doubles: left-to-right binary exponentiation -- from T, for every bit of j below its highest, from the
// high end: square, then, where the bit is set, times T on the right.  Sums ascending.
inline void hmm_power(const double* T, int K, int j, double* out)
{
    const size_t KK = (size_t) K * K;
    std::vector<double> tmp(KK);
    auto times = [&](const double* A, const double* B) {
        for (int r = 0; r < K; ++r)
            for (int b = 0; b < K; ++b) {
                double v = 0.0;
                for (int m = 0; m < K; ++m) v += A[r * K + m] * B[m * K + b];
                tmp[(size_t) r * K + b] = v;
            }
        std::copy(tmp.begin(), tmp.end(), out);
    };
    std::copy(T, T + KK, out);
    int top = 0;
    while ((j >> (top + 1)) != 0) ++top;
    for (int bit = top - 1; bit >= 0; --bit) {
        times(out, out);
        if (j >> bit & 1) times(out, T);
    }
}

// The checks of the call on one engine, and where its inputs lie: what is queued runs, the latest log-likelihood call is the
// one the header asks for, q is computed unless d_q holds it (one launch, counted), the stream is idle afterwards.
template <class Engine>
inline int autocorrelated_prepare(Engine& e, int wIdx, HmmSource& src)
{
    const char* const who = "mbamdCalculateAutocorrelatedLogLikelihood";
    { const int rc = e.runQueued(); if (rc) return rc; }
    { const int rc = e.refuses(who); if (rc) return rc; }
    if (e.lastLnl.count == 0) return fail(BEAGLE_ERROR_GENERAL, who, "no log-likelihood was calculated yet: the category posteriors and the site log-likelihoods are its");
    if (e.lastLnl.count > 1) return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, who, "the latest log-likelihood call had more than one subset");
    if (wIdx != e.lastLnl.weights) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "category weights index differs from the latest log-likelihood call's");
    src.q = nullptr;
    { const int rc = e.siteLogLikelihoods(&src.site, &src.siteHost); if (rc) return rc; }
    if (e.K > 1) {
        const bool held = e.qStamp == e.lastLnl.stamp && e.d_q;
        const int rc = ensure_posteriors(e);
        if (rc) return rc;
        if (!held) e.countLaunches(1);
        src.q = e.d_q;
    }
    src.qStride = (size_t) e.Ppad;
    src.count = e.P;
    HIP_TRY(hipStreamSynchronize(e.stream));
    e.afterSync();
    return BEAGLE_SUCCESS;
}

// the weights of index wIdx as the engine's kernels read them: the host mirror where the client has sent them, else the device's
template <class Engine>
inline int autocorrelated_weights(Engine& e, int wIdx, double* w)
{
    const std::vector<double>& m = e.weightsMirror().last;
    const size_t at = (size_t) wIdx * e.K;
    if (m.size() >= at + e.K && m[at] == m[at]) { std::copy(m.begin() + (long) at, m.begin() + (long) (at + e.K), w); return BEAGLE_SUCCESS; }
    HIP_TRY(hipMemcpy(w, e.d_weights + at, (size_t) e.K * sizeof(double), hipMemcpyDeviceToHost));
    return BEAGLE_SUCCESS;
}

// The call proper, on engine e (of a pattern-sharded instance: the first), after autocorrelated_prepare on every engine.  One
// source that begins at pattern 0 is read where it lies; several are first gathered, in instance pattern order, into q [K][P] and
// l [P] on e's device, so that the kernels see what an unsharded instance's see.  The arguments are checked (the C ABI).
// Launches: ceil(log_R n) of k_hmm_products; with posteriors one k_hmm_vectors per level above the leaves and k_hmm_posteriors.
template <class Engine>
inline int autocorrelated_run(Engine& e, const HmmSource* sources, int sourceCount, int wIdx, const int* sitePatterns, const int* siteJumps,
                              int n, const double* T, double* outLnl, double* outPost)
{
    const char* const who = "mbamdCalculateAutocorrelatedLogLikelihood";
    const int K = e.K, KK = K * K, R = HMM_CHUNK;
    double w[MBAMD_MAX_RATES];
    { const int rc = autocorrelated_weights(e, wIdx, w); if (rc) return rc; }
    for (int k = 0; k < K; ++k)
        if (!(w[k] > 0.0) || !(w[k] < INFINITY)) return fail(BEAGLE_ERROR_OUT_OF_RANGE, who, "a category weight is not positive");
    // the table: T^(j) per distinct jump (ascending), the weights, the patterns, every site's row of the powers (several rows only)
    std::vector<int> distinct(1, 1);
    if (siteJumps != nullptr && K > 1) {
        distinct.assign(siteJumps + 1, siteJumps + n);
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        if (distinct.empty()) distinct.assign(1, 1);
    }
    const size_t D = distinct.size(), tableDoubles = D * KK + (size_t) K;
    std::vector<unsigned char> table(tableDoubles * sizeof(double) + (size_t) (D > 1 ? 2 : 1) * n * sizeof(int));
    double* const hPowers = reinterpret_cast<double*>(table.data());
    int* const hPatterns = reinterpret_cast<int*>(table.data() + tableDoubles * sizeof(double));
    int* const hJumps = hPatterns + n;
    for (size_t i = 0; i < D; ++i) {
        if (K == 1) hPowers[i] = 1.0;              // (one category: T is not read)
        else hmm_power(T, K, distinct[i], hPowers + i * KK);
    }
    std::copy(w, w + K, hPowers + D * KK);
    std::copy(sitePatterns, sitePatterns + n, hPatterns);
    for (int s = 0; s < n && D > 1; ++s)
        hJumps[s] = s == 0 ? 0 : (int) (std::lower_bound(distinct.begin(), distinct.end(), siteJumps[s]) - distinct.begin());
    void* d_table = nullptr;
    { const int rc = e.stageTable(table.data(), table.size(), &d_table); if (rc) return rc; }

    // the levels: count[l] items become count[l + 1] products; the last level leaves one
    std::vector<int> count(1, n);
    do count.push_back((count.back() + R - 1) / R); while (count.back() > 1);
    const int levels = (int) count.size() - 1;
    // scratch, in doubles: the gathered inputs | per level: products, sums, exponents, (entry and exit vectors) | gamma
    const bool gather = sourceCount > 1 || sources[0].start != 0;
    size_t P = 0;
    for (int i = 0; i < sourceCount; ++i) P += (size_t) sources[i].count;
    const size_t gatherDoubles = gather ? (size_t) (K > 1 ? K + 1 : 1) * P : 0;
    std::vector<size_t> at((size_t) levels);
    size_t total = gatherDoubles;
    auto level_doubles = [&](int l) { const size_t c = (size_t) count[(size_t) l + 1]; return c * KK + c + (c + 1) / 2 + (outPost ? 2 * c * K : 0); };
    for (int l = 0; l < levels; ++l) { at[(size_t) l] = total; total += level_doubles(l); }
    const size_t gammaAt = total;
    if (outPost) total += (size_t) K * n;
    double* d_scratch = nullptr;
    { const int rc = e.resultScratch(total * sizeof(double), &d_scratch); if (rc) return rc; }

    HmmArgs a;
    std::memset(&a, 0, sizeof a);
    if (gather) {
        double* const gq = d_scratch + P, * const gl = d_scratch;
        for (int i = 0; i < sourceCount; ++i) {
            const HmmSource& s = sources[i];
            if (s.siteHost) HIP_TRY(hipMemcpy(gl + s.start, s.siteHost, (size_t) s.count * sizeof(double), hipMemcpyHostToDevice));
            else HIP_TRY(hipMemcpy(gl + s.start, s.site, (size_t) s.count * sizeof(double), hipMemcpyDeviceToDevice));
            for (int k = 0; k < K && K > 1; ++k)
                HIP_TRY(hipMemcpy(gq + (size_t) k * P + s.start, s.q + (size_t) k * s.qStride, (size_t) s.count * sizeof(double), hipMemcpyDeviceToDevice));
        }
        a.q = K > 1 ? gq : nullptr;
        a.site = gl;
        a.qStride = P;
    } else {
        a.q = sources[0].q;
        a.site = sources[0].site;
        a.qStride = sources[0].qStride;
    }
    a.powers = static_cast<const double*>(d_table);
    a.weights = a.powers + D * KK;
    a.patterns = reinterpret_cast<const int*>(a.powers + tableDoubles);
    a.jumps = D > 1 ? a.patterns + n : nullptr;
    a.K = K;
    a.n = n;
    struct Level { double* prod; double* sum; int* exp; double* entry; double* exit; };
    std::vector<Level> lv((size_t) levels);
    for (int l = 0; l < levels; ++l) {
        const size_t c = (size_t) count[(size_t) l + 1];
        Level& v = lv[(size_t) l];
        v.prod = d_scratch + at[(size_t) l];
        v.sum = v.prod + c * KK;
        v.exp = reinterpret_cast<int*>(v.sum + c);
        v.entry = outPost ? v.sum + c + (c + 1) / 2 : nullptr;
        v.exit = outPost ? v.entry + c * K : nullptr;
    }
    auto level_args = [&](int l) {
        HmmArgs b = a;
        b.count = count[(size_t) l];
        if (l > 0) { b.inProd = lv[(size_t) l - 1].prod; b.inSum = lv[(size_t) l - 1].sum; b.inExp = lv[(size_t) l - 1].exp; }
        b.prod = lv[(size_t) l].prod; b.sum = lv[(size_t) l].sum; b.exp = lv[(size_t) l].exp;
        return b;
    };
    hipEvent_t ev0{}, ev1{};
    { const int rc = e.timedBegin(ev0, ev1); if (rc) return rc; }
    int launches = 0;
    for (int l = 0; l < levels; ++l) {
        const HmmArgs b = level_args(l);
        if (l == 0) { auto kernel = k_hmm_products<true>; MBAMD_LAUNCH_BARRIER(kernel, (unsigned) count[1], 64, 0, e.stream, b); }
        else { auto kernel = k_hmm_products<false>; MBAMD_LAUNCH_BARRIER(kernel, (unsigned) count[(size_t) l + 1], 64, 0, e.stream, b); }
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    if (outPost) {
        // top-down: the vectors of level l's nodes (the top: ones) go to the nodes of level l - 1, at last to the chunks of sites
        for (int l = levels - 1; l >= 0; --l) {
            HmmArgs b = level_args(l);
            const bool top = l == levels - 1;
            b.entry = top ? nullptr : lv[(size_t) l].entry;
            b.exit = top ? nullptr : lv[(size_t) l].exit;
            if (l > 0) {
                b.inEntry = lv[(size_t) l - 1].entry;
                b.inExit = lv[(size_t) l - 1].exit;
                MBAMD_LAUNCH_BARRIER(k_hmm_vectors, (unsigned) count[(size_t) l + 1], 64, 0, e.stream, b);
            } else {
                b.gamma = d_scratch + gammaAt;
                MBAMD_LAUNCH_BARRIER(k_hmm_posteriors, (unsigned) count[1], 64, 0, e.stream, b);
            }
            HIP_TRY(hipGetLastError());
            ++launches;
        }
    }
    { const int rc = e.timedEnd(ev0, ev1); if (rc) return rc; }
    e.countLaunches(launches);
    HIP_TRY(hipStreamSynchronize(e.stream));
    e.afterSync();
    // the top: one product, its sum of l and its exponent lie side by side
    std::vector<double> h((size_t) KK + 2);
    HIP_TRY(hipMemcpy(h.data(), lv[(size_t) levels - 1].prod, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    int E = 0;
    std::memcpy(&E, &h[(size_t) KK + 1], sizeof E);
    double all = 0.0;
    for (int i = 0; i < KK; ++i) all += h[(size_t) i];
    const double lnH = h[(size_t) KK] + (std::log(all) + (double) E * 0.693147180559945309417232121458176568);
    if (outPost) HIP_TRY(hipMemcpy(outPost, d_scratch + gammaAt, (size_t) K * n * sizeof(double), hipMemcpyDeviceToHost));
    *outLnl = lnH;
    return std::isfinite(lnH) ? BEAGLE_SUCCESS : BEAGLE_ERROR_FLOATING_POINT;
}

}  // namespace mbamd
#endif
