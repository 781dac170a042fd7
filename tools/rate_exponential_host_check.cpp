// rate_exponential_host_check.cpp -- the host side of mbamdUpdateTransitionMatricesFromRateMatrix that touches no device
// (mrbayes_amd/csrc/mbamd_rate_exponential_table.h: what the call checks, and the entry table it sends) as a stand-alone program, made to
// be run under the host sanitizers.  No GPU, no Python, nothing preloaded:
//     clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mrbayes_amd/csrc tools/rate_exponential_host_check.cpp -o rx_check && ./rx_check
// Every refusal of the call's contract is given once, then one valid list; the exit status is the number of wrong answers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mbamd_rate_exponential_table.h"

using namespace mbamd;

static int wrong = 0;
static void expect(bool ok, const char* what)
{
    if (!ok) { std::printf("WRONG: %s\n", what); ++wrong; }
}

static std::vector<double> generator(int S)
{
    std::vector<double> q((size_t) S * S, 0.0);
    for (int i = 0; i < S; ++i) {
        double sum = 0.0;
        for (int j = 0; j < S; ++j)
            if (j != i) { q[(size_t) i * S + j] = ((i * 7 + j * 3) % 5 == 0) ? 0.0 : 0.01 + 0.37 * ((i * 31 + j * 17) % 11); sum += q[(size_t) i * S + j]; }
        q[(size_t) i * S + i] = -sum;
    }
    return q;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int S : {2, 3, 4, 5, 20, 61, 64}) {
        const std::vector<double> q = generator(S);
        RateExpMatrix m;
        expect(rate_exp_matrix(q.data(), S, m) == nullptr, "a valid rate matrix");
        expect(m.R.size() == (size_t) S * S && m.Q.size() == (size_t) S * S && m.mu > 0.0, "the sizes of R and Q");
        for (int i = 0; i < S; ++i) {
            double row = 0.0;
            for (int j = 0; j < S; ++j) { expect(m.R[(size_t) i * S + j] >= 0.0, "R is non-negative"); row += m.R[(size_t) i * S + j]; }
            expect(std::fabs(row - 1.0) <= 4.0 * S * 0x1p-53, "a row of R sums to one");
        }
        // -- the refusals of Q
        std::vector<double> bad = q;
        bad[(size_t) (S - 1) * S] = -1e-3;
        expect(rate_exp_matrix(bad.data(), S, m) != nullptr, "a negative off-diagonal");
        bad = q; bad[(size_t) (S - 1) * S + S - 2] = nan;
        expect(rate_exp_matrix(bad.data(), S, m) != nullptr, "a NaN entry");
        bad = q; bad[1] = inf;
        expect(rate_exp_matrix(bad.data(), S, m) != nullptr, "an infinite entry");
        bad = q; bad[(size_t) S * S - 1] += 1e-6;
        expect(rate_exp_matrix(bad.data(), S, m) != nullptr, "a diagonal off by 1e-6");
        bad = q; bad[0] = bad[0] * (1.0 + 0x1p-52);
        expect(rate_exp_matrix(bad.data(), S, m) == nullptr, "a diagonal off by one rounding");
        expect(rate_exp_matrix(q.data(), S, m) == nullptr, "the valid rate matrix again");
        // -- the refusals of edge lengths and rates
        const int K = 4, count = 3;
        const double rates[K] = {0.0, 0.3, 1.1, 2.0};
        std::vector<RateExpArg> args((size_t) count * K);
        const double cap = 0x1p20 / (m.mu * 2.0);
        double t[count] = {0.0, 0.1, cap};
        while (m.mu * (2.0 * t[2]) > 0x1p20) t[2] = std::nextafter(t[2], 0.0);
        expect(rate_exp_args(m.mu, rates, K, t, count, args.data()) == nullptr, "valid edge lengths");
        for (int u = 0; u < count; ++u)
            for (int k = 0; k < K; ++k) {
                const RateExpArg& a = args[(size_t) u * K + k];
                expect(a.s >= 0 && a.s <= MBAMD_RATE_EXP_MAX_SQUARINGS && a.y >= 0.0 && a.y <= 1.0 && (a.s == 0 || a.y > 0.5), "0 <= s <= 20 and y in (1/2, 1]");
                expect(std::ldexp(a.y, a.s) == m.mu * (rates[k] * t[u]) && a.ey == std::exp(-a.y) && a.rate == rates[k], "y 2^s is the argument");
            }
        expect(args[(size_t) 2 * K + 3].s == MBAMD_RATE_EXP_MAX_SQUARINGS || args[(size_t) 2 * K + 3].s == MBAMD_RATE_EXP_MAX_SQUARINGS - 1, "the cap");
        double tb[count] = {0.1, 0.2, -1e-9};
        expect(rate_exp_args(m.mu, rates, K, tb, count, args.data()) != nullptr, "a negative t");
        tb[2] = inf;
        expect(rate_exp_args(m.mu, rates, K, tb, count, args.data()) != nullptr, "an infinite t");
        tb[2] = nan;
        expect(rate_exp_args(m.mu, rates, K, tb, count, args.data()) != nullptr, "a NaN t");
        tb[2] = std::nextafter(t[2], inf);
        while (!(m.mu * (2.0 * tb[2]) > 0x1p20)) tb[2] = std::nextafter(tb[2], inf);
        expect(rate_exp_args(m.mu, rates, K, tb, count, args.data()) != nullptr, "mu r t just above 2^20");
        const double rb[K] = {0.0, -0.5, 1.0, 2.0};
        expect(rate_exp_args(m.mu, rb, K, t, count, args.data()) != nullptr, "a negative rate");
        // -- the refusals of the index lists
        const int p[3] = {0, 1, 2}, d1[3] = {3, 4, 5}, d2[3] = {6, 7, 8};
        expect(rate_exp_indices(9, p, d1, d2, 3) == nullptr, "valid lists");
        expect(rate_exp_indices(9, p, nullptr, d2, 3) == nullptr && rate_exp_indices(9, p, d1, nullptr, 3) == nullptr, "either derivative list alone");
        expect(rate_exp_indices(9, nullptr, d1, d2, 3) != nullptr, "a NULL list");
        expect(rate_exp_indices(8, p, d1, d2, 3) != nullptr, "an index out of range");
        const int neg[3] = {3, 4, -1}, twice[3] = {0, 1, 1}, across[3] = {6, 7, 2};
        expect(rate_exp_indices(9, p, neg, d2, 3) != nullptr, "a negative index");
        expect(rate_exp_indices(9, twice, d1, d2, 3) != nullptr, "an index twice in one list");
        expect(rate_exp_indices(9, p, d1, across, 3) != nullptr, "an index twice among the lists");
        expect(rate_exp_indices(0, p, nullptr, nullptr, 0) == nullptr, "no entries, no buffers");
    }
    // -- a Q of all zeros: the identity; the reduction at its edges
    {
        const std::vector<double> zero(16, 0.0);
        RateExpMatrix m;
        expect(rate_exp_matrix(zero.data(), 4, m) == nullptr && m.mu == 0.0 && m.R[0] == 1.0 && m.R[1] == 0.0 && m.R[5] == 1.0, "a Q of all zeros");
        int s = -1;
        double y = -1.0;
        rate_exp_reduce(0.0, &s, &y);             expect(s == 0 && y == 0.0, "x = 0");
        rate_exp_reduce(1.0, &s, &y);             expect(s == 0 && y == 1.0, "x = 1");
        rate_exp_reduce(std::nextafter(1.0, 2.0), &s, &y); expect(s == 1 && y > 0.5 && y < 0.51, "x just over 1");
        rate_exp_reduce(37.0, &s, &y);            expect(s == 6 && y == 37.0 / 64.0, "x = 37");
        rate_exp_reduce(0x1p20, &s, &y);          expect(s == 20 && y == 1.0, "x = 2^20");
        rate_exp_reduce(0x1p-1060, &s, &y);       expect(s == 0 && y == 0x1p-1060, "a subnormal x");
    }
    std::printf("%s: %d wrong answers\n", wrong ? "FAILED" : "ok", wrong);
    return wrong;
}
