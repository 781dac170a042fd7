// mbamd_rate_exponential_table.h -- the host side of mbamdUpdateTransitionMatricesFromRateMatrix that touches no device: what the
// call checks before anything is written, and the numbers it sends (semantics: beagle.h; the kernels: mbamd_rate_exponential.h).
// Plain C++ on purpose (<cmath>, <vector> and nothing of the runtime): a stand-alone program can run it under the host sanitizers
// (tools/rate_exponential_host_check.cpp).
//
//     exp(Q tau) = ( sum_{n <= N} e^-y y^n / n!  R^n )^(2^s),     R = I + Q / mu,  mu = max_i sum_{j != i} q_ij,  y = mu tau / 2^s <= 1
//
// Every refusal is a text (nullptr: nothing to refuse); the caller turns it into BEAGLE_ERROR_OUT_OF_RANGE.
#ifndef MBAMD_RATE_EXPONENTIAL_TABLE_H_
#define MBAMD_RATE_EXPONENTIAL_TABLE_H_

#include <cmath>
#include <cstddef>
#include <vector>

namespace mbamd {

// N: the last term of the series.  The terms left out sum to e^-y sum_{n > N} y^n / n! <= y^(N+1) / (N+1)! (Lagrange's remainder
// times e^-y); a squaring at most doubles an absolute error of a sub-stochastic matrix, so 2^s of them reach P.  At the cap, s = 20
// and y = 1:  2^20 / 26! = 2^20 2^-88.3 = 2^-68.3 < 2^-64;  N = 24 would give 2^20 / 25! = 2^-63.7.
#define MBAMD_RATE_EXP_TERMS 25
// mu r t <= 2^20: s <= 20 squarings
#define MBAMD_RATE_EXP_MAX_SQUARINGS 20

// what one (entry, category) is made from: P = T(y)^(2^s), T(y) = sum_n ey y^n / n! R^n; the derivatives take `rate`
struct alignas(16) RateExpArg {
    double y, ey, rate;
    int s, pad_;
};
static_assert(sizeof(RateExpArg) == 32, "RateExpArg must be 32 bytes");

// Q as the engine uses it: the off-diagonals as given, the diagonal minus the row sum it formed itself
struct RateExpMatrix {
    double mu = 0.0;
    std::vector<double> R;           // [S][S]  R_ij = q_ij / mu, R_ii = (mu - sum_i) / mu: non-negative (mu = 0: the identity)
    std::vector<double> Q;           // [S][S]  q_ij, Q_ii = -sum_i
};

// Entries finite, off-diagonals >= 0, each diagonal minus its row's off-diagonal sum to within S 2^-52 of that sum -- what summing
// in double, in any order, can lose.  Fills `m`.
inline const char* rate_exp_matrix(const double* q, int S, RateExpMatrix& m)
{
    for (int i = 0; i < S * S; ++i)
        if (!std::isfinite(q[i])) return "a rate-matrix entry is not finite";
    std::vector<double> sum((size_t) S, 0.0);
    m.mu = 0.0;
    for (int i = 0; i < S; ++i) {
        double s = 0.0;
        for (int j = 0; j < S; ++j) {
            if (j == i) continue;
            if (q[i * S + j] < 0.0) return "a negative off-diagonal rate";
            s += q[i * S + j];
        }
        if (!std::isfinite(s)) return "a row sum of the rate matrix is not finite";
        if (!(std::fabs(q[i * S + i] + s) <= (double) S * 0x1p-52 * s)) return "a diagonal entry is not minus the sum of its row";
        sum[(size_t) i] = s;
        if (s > m.mu) m.mu = s;
    }
    m.R.assign((size_t) S * S, 0.0);
    m.Q.assign((size_t) S * S, 0.0);
    for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) {
            const size_t at = (size_t) i * S + j;
            if (i == j) {
                m.Q[at] = -sum[(size_t) i];
                m.R[at] = m.mu > 0.0 ? (m.mu - sum[(size_t) i]) / m.mu : 1.0;
            } else {
                m.Q[at] = q[at];
                m.R[at] = m.mu > 0.0 ? q[at] / m.mu : 0.0;
            }
        }
    return nullptr;
}

// The squaring count and the reduced argument of x = mu r t: the smallest s with x / 2^s <= 1 (the division is exact)
inline void rate_exp_reduce(double x, int* s, double* y)
{
    *s = 0;
    if (x > 1.0) {
        int e = 0;
        const double f = std::frexp(x, &e);          // x = f 2^e, 0.5 <= f < 1
        *s = f == 0.5 ? e - 1 : e;
    }
    *y = std::ldexp(x, -*s);
}

// out[u * K + k] for `count` edge lengths and the K category rates: t finite and >= 0, rates finite and >= 0, mu r t <= 2^20
inline const char* rate_exp_args(double mu, const double* rates, int K, const double* t, int count, RateExpArg* out)
{
    for (int k = 0; k < K; ++k)
        if (!(rates[k] >= 0.0) || !std::isfinite(rates[k])) return "a category rate is negative or not finite";
    for (int u = 0; u < count; ++u) {
        if (!(t[u] >= 0.0) || !std::isfinite(t[u])) return "an edge length is negative or not finite";
        for (int k = 0; k < K; ++k) {
            const double x = mu * (rates[k] * t[u]);
            if (!(x <= 0x1p20)) return "rate x edge length beyond 2^20 expected substitutions";
            RateExpArg& a = out[(size_t) u * K + k];
            rate_exp_reduce(x, &a.s, &a.y);
            a.ey = std::exp(-a.y);
            a.rate = rates[k];
            a.pad_ = 0;
        }
    }
    return nullptr;
}

// The three output lists: prob there, every index a matrix buffer, none named twice among them (d1, d2: may be null)
inline const char* rate_exp_indices(int nMatrices, const int* prob, const int* d1, const int* d2, int count)
{
    if (!prob) return "null array";
    const int* const lists[3] = {prob, d1, d2};
    std::vector<char> seen((size_t) (nMatrices > 0 ? nMatrices : 0), 0);
    for (int l = 0; l < 3; ++l) {
        if (!lists[l]) continue;
        for (int u = 0; u < count; ++u) {
            const int m = lists[l][u];
            if (m < 0 || m >= nMatrices) return "matrix index";
            if (seen[(size_t) m]) return "a matrix index occurs twice among the outputs";
            seen[(size_t) m] = 1;
        }
    }
    return nullptr;
}

}  // namespace mbamd
#endif
