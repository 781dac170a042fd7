// unstored_host_check.cpp -- the host side of the 4-state walk's unstored subtrees (mrbayes_amd/csrc/mbamd_walk4_unstored.h) and of the
// launch timer (mbamd_launch_timer.h), driven through the C ABI as a stand-alone program, made to be run under the host sanitizers with
// the host-emulation build of the engine (tests/hostemu/: the kernels run on the CPU).  No GPU, no Python, nothing preloaded; from the
// repository root, with the ROCm toolchain's clang++ (the flags of tests/hostemu/build_emu.py plus the sanitizers):
//     clang++ -O2 -std=c++17 -w -g -fsanitize=address,undefined -fno-sanitize-recover=all -I tests/hostemu -I include -I mrbayes_amd/csrc \
//         mrbayes_amd/csrc/mbamd_engine.cpp tools/unstored_host_check.cpp -o unstored_check && ./unstored_check
// One instance of 4 states x 2 categories x 130 patterns on 9 taxa, the tree (((1,2),3),((4,5),(6,7))),(8,9): four tip pairs, a subtree
// of three tips and one of four.  After every step the log-likelihood is compared with the first evaluation's; the exit status is the
// number of wrong answers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "libhmsbeagle/beagle.h"

static int wrong = 0;
static void expect(bool ok, const char* what)
{
    std::printf("%s %s\n", ok ? "ok   " : "WRONG", what);
    if (!ok) ++wrong;
}
#define OK(call) do { const int rc_ = (call); if (rc_ != BEAGLE_SUCCESS) { std::printf("WRONG: %s returned %d\n", #call, rc_); ++wrong; } } while (0)

enum { NTAX = 9, NPAT = 130, NCAT = 2, NOP = 8, TOP = 16, EXTRA = 100 };
static int inst = -1;
static const double rates[NCAT] = {0.5, 1.5};
static double length_of(int node) { return 0.02 + 0.013 * (node % 9); }
// tips 0 .. 8; A = 9 (0,1)  B = 10 (A,2)  C = 11 (3,4)  D = 12 (5,6)  E = 13 (C,D)  F = 14 (7,8)  G = 15 (B,E)  H = 16 (G,F); the matrix
// of a branch has its child's number
static const BeagleOperation tree[NOP] = {
    {9, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 0, 0, 1, 1},    {10, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 9, 9, 2, 2},
    {11, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 3, 3, 4, 4},   {12, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 5, 5, 6, 6},
    {13, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 11, 11, 12, 12}, {14, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 7, 7, 8, 8},
    {15, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 10, 10, 13, 13}, {16, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 15, 15, 14, 14},
};

static void counts(long pairs[3], long subtrees[3])
{
    std::memset(pairs, 0, 3 * sizeof(long));
    std::memset(subtrees, 0, 3 * sizeof(long));
    OK(mbamdGetRecomputeCounts(inst, pairs));
    OK(mbamdGetSubtreeRecomputeCounts(inst, subtrees));
}
static void expect_counts(long p0, long p1, long p2, long s0, long s1, long s2, const char* what)
{
    long p[3], s[3];
    counts(p, s);
    std::printf("      tip pairs (left unstored, materialised, launches) %ld %ld %ld, subtrees %ld %ld %ld\n", p[0], p[1], p[2], s[0], s[1], s[2]);
    expect(p[0] == p0 && p[1] == p1 && p[2] == p2 && s[0] == s0 && s[1] == s1 && s[2] == s2, what);
}
static void matrices_of_the_tree()
{
    int idx[TOP + 1];
    double t[TOP + 1];
    for (int i = 0; i < TOP; ++i) { idx[i] = i; t[i] = length_of(i); }
    idx[TOP] = 17; t[TOP] = length_of(15) + length_of(14);       // the branch between G and F, for the edge call
    OK(beagleUpdateTransitionMatrices(inst, 0, idx, nullptr, nullptr, t, TOP + 1));
}
static void run_list() { OK(beagleUpdatePartials(inst, tree, NOP, BEAGLE_OP_NONE)); }
static double root_lnl()
{
    const int top = TOP, zero = 0, none = BEAGLE_OP_NONE;
    double lnl = 0.0;
    OK(beagleCalculateRootLogLikelihoods(inst, &top, &zero, &zero, &none, 1, &lnl));
    return lnl;
}
static std::vector<double> partials_of(int buffer)
{
    std::vector<double> out((size_t) NCAT * NPAT * 4);
    OK(beagleGetPartials(inst, buffer, BEAGLE_OP_NONE, out.data()));
    return out;
}

int main()
{
    // small lists reach the plain walk through a device buffer -- the launches that leave subtrees unstored -- only without the
    // programs in the kernel arguments; one wave per workgroup whatever the list's length
    setenv("MBAMD_NO_INLINE_PROGRAMS", "1", 1);
    setenv("MBAMD_WALK_WAVES", "1", 1);
    int resource = 0;
    BeagleInstanceDetails details;
    inst = beagleCreateInstance(NTAX, 30 + EXTRA + EXTRA / 2 - NTAX, NTAX, 4, NPAT, 1, 20, NCAT, 4, &resource, 1, BEAGLE_FLAG_PRECISION_SINGLE, 0, &details);
    if (inst < 0) { std::printf("WRONG: beagleCreateInstance returned %d\n", inst); return 1; }
    std::printf("%s\n", details.implName);
    // Jukes-Cantor: Q = H diag(0, -4/3, -4/3, -4/3) H / 4 with the Hadamard matrix H
    const double U[16] = {1, 1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1};
    double Ui[16];
    for (int i = 0; i < 16; ++i) Ui[i] = U[i] / 4.0;
    const double lambda[4] = {0.0, -4.0 / 3.0, -4.0 / 3.0, -4.0 / 3.0}, pi[4] = {0.25, 0.25, 0.25, 0.25}, w[NCAT] = {0.5, 0.5};
    OK(beagleSetEigenDecomposition(inst, 0, U, Ui, lambda));
    OK(beagleSetStateFrequencies(inst, 0, pi));
    OK(beagleSetCategoryWeights(inst, 0, w));
    OK(beagleSetCategoryRates(inst, rates));
    std::vector<double> pw(NPAT, 1.0);
    OK(beagleSetPatternWeights(inst, pw.data()));
    std::vector<std::vector<int>> states(NTAX, std::vector<int>(NPAT));
    unsigned x = 12345u;
    for (int c = 0; c < NPAT; ++c) {
        x = x * 1664525u + 1013904223u;
        const int base = (int) (x >> 24) % 4;
        for (int t = 0; t < NTAX; ++t) {
            x = x * 1664525u + 1013904223u;
            const unsigned r = x >> 24;
            states[t][c] = r < 40 ? (int) (r % 4) : r < 52 ? 4 : base;       // mostly the column's state, some others, some gaps
        }
    }
    for (int t = 0; t < NTAX; ++t) OK(beagleSetTipStates(inst, t, states[t].data()));

    // 1. a whole-tree list: four tip pairs, the subtree of three tips and the one of four stay unstored
    matrices_of_the_tree();
    run_list();
    const double first = root_lnl();
    std::printf("      lnL %.10f\n", first);
    expect(std::isfinite(first) && first < 0.0, "1. the first evaluation");
    expect_counts(4, 0, 0, 2, 0, 0, "1. four tip pairs and two subtrees left unstored");

    // 2. a recipe buffer is read: the subtree of four tips is made by a launch of its own, the tip pairs inside it are not
    const std::vector<double> four = partials_of(13);
    expect_counts(4, 0, 0, 2, 1, 1, "2. the subtree of four tips materialised by the read");
    expect(root_lnl() == first, "2. lnL");

    // 3. a tip that a recipe uses gets new states: the subtree of three tips is made first, from the old ones
    std::vector<int> other(NPAT);
    for (int c = 0; c < NPAT; ++c) other[c] = (states[2][c] + 1) % 4;
    OK(beagleSetTipStates(inst, 2, other.data()));
    expect_counts(4, 0, 0, 2, 2, 2, "3. the subtree of three tips materialised before its tip changed");
    expect(root_lnl() == first, "3. lnL");
    OK(beagleSetTipStates(inst, 2, states[2].data()));

    // 4. a matrix is overwritten between the launch and the snapshot: the recipes read what the launch read
    run_list();
    expect_counts(8, 0, 0, 4, 2, 2, "4. the same list again leaves the same buffers unstored");
    std::vector<double> junk((size_t) NCAT * 16, 0.25);
    OK(beagleSetTransitionMatrix(inst, 3, junk.data(), 0.0));
    expect(partials_of(13) == four, "4. the subtree of four tips, made after its matrix was overwritten, is what it was");
    expect_counts(8, 0, 0, 4, 3, 3, "4. ... by one launch");
    expect(root_lnl() == first, "4. lnL");
    matrices_of_the_tree();

    // 5. an edge log-likelihood whose child end is an unstored tip pair (the pulley principle: the same likelihood, other roundings)
    {
        const int parent = 15, child = 14, matrix = 17, zero = 0, none = BEAGLE_OP_NONE;
        double lnl = 0.0;
        OK(beagleCalculateEdgeLogLikelihoods(inst, &parent, &child, &matrix, nullptr, nullptr, &zero, &zero, &none, 1, &lnl, nullptr, nullptr));
        std::printf("      edge lnL %.10f\n", lnl);
        expect(std::fabs(lnl - first) <= 1e-5 * std::fabs(first), "5. lnL over the edge");
        expect_counts(8, 1, 1, 4, 3, 3, "5. the tip pair materialised by the edge call");
    }

    // 6. the same list again
    run_list();
    expect(root_lnl() == first, "6. lnL");
    expect_counts(12, 1, 1, 6, 3, 3, "6. left unstored once more");

    // 7. more unstored buffers than a program in the kernel arguments holds: a list of EXTRA tip pairs, then a list that reads them all
    {
        std::vector<BeagleOperation> pairs(EXTRA), readers(EXTRA / 2);
        for (int i = 0; i < EXTRA; ++i) pairs[i] = {30 + i, BEAGLE_OP_NONE, BEAGLE_OP_NONE, i % NTAX, i % NTAX, (i + 4) % NTAX, (i + 4) % NTAX};
        for (int i = 0; i < EXTRA / 2; ++i) readers[i] = {30 + EXTRA + i, BEAGLE_OP_NONE, BEAGLE_OP_NONE, 30 + 2 * i, 9, 30 + 2 * i + 1, 10};
        OK(beagleUpdatePartials(inst, pairs.data(), EXTRA, BEAGLE_OP_NONE));
        expect_counts(12 + EXTRA, 1, 1, 6, 3, 3, "7. a hundred tip pairs left unstored");
        OK(beagleUpdatePartials(inst, readers.data(), EXTRA / 2, BEAGLE_OP_NONE));
        expect_counts(12 + EXTRA, 1 + EXTRA, 2, 6, 3, 3, "7. ... and materialised by one launch, its program in a device buffer");
        const std::vector<double> last = partials_of(30 + EXTRA + EXTRA / 2 - 1);
        bool finite = true;
        for (double v : last) finite = finite && std::isfinite(v) && v >= 0.0;
        expect(finite, "7. a result made from them");
        run_list();
        expect(root_lnl() == first, "7. lnL");
    }

    // 8. timing on: an evaluation is one step; both read-outs
    {
        OK(mbamdKernelTiming(inst, 1));
        double ms = 0.0, stepMs = 0.0;
        long launches = 0, steps = 0;
        OK(mbamdGetKernelTiming(inst, &ms, &launches, 1));
        matrices_of_the_tree();
        run_list();
        expect(root_lnl() == first, "8. lnL");
        OK(mbamdGetKernelTiming(inst, &ms, &launches, 1));
        OK(mbamdGetStepTiming(inst, &stepMs, &steps, 1));
        std::printf("      %ld launch(es) in %.4f ms, %ld step(s) in %.4f ms\n", launches, ms, steps, stepMs);
        expect(launches == 1 && ms >= 0.0 && steps == 1 && stepMs >= 0.0, "8. one list launch, one step");
        OK(mbamdGetStepTiming(inst, &stepMs, &steps, 1));
        expect(steps == 0, "8. nothing after the reset");
    }

    // 9. the instance goes with unstored buffers, a waiting snapshot and timing on
    run_list();
    OK(beagleFinalizeInstance(inst));
    OK(beagleFinalize());
    std::printf("%s: %d wrong answers\n", wrong ? "FAILED" : "ok", wrong);
    return wrong;
}
