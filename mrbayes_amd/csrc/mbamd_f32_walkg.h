// mbamd_f32_walkg.h -- the single-precision engine (mbamd_f32.h): the 20/61-state tree walk on the matrix cores (kernels:
// mbamd_walkg.h, mbamd_pathg_kernel.h).  In front of the engine: wg_compiled, MBAMD_WG_DISPATCH, raise_walkg_lds (which state counts
// the walk is instantiated for).  Defines Instance::wgGeometry, updatePartialsG, scaleOpsIndependentOfPending, flushWalkG, buildPathG,
// launch_walkg_t, launch_pathg_t, walkGArgs, runWalkG.
#ifndef MBAMD_F32_WALKG_H_
#define MBAMD_F32_WALKG_H_

#include "mbamd_host.h"          // the HIP runtime
#include "mbamd_kernels.h"       // k_walkg, WgShape (mbamd_walkg.h)

namespace mbamd {

// state counts the 20/61-state tree walk (mbamd_walkg.h) is instantiated for: amino acids, doublets, and the sense codons of
// every genetic code MrBayes knows (60 vertebrate mitochondrial ... 63; reference src/model.c SetCode)
// state counts MrBayes sends: restriction sites 2, covarion nucleotides 8, doublets 16, amino acids 20, covarion amino acids 40, the
// sense codons of every genetic code 60..63 (4 has its own kernel; anything else runs on the level kernels)
// (round 5: 3, 5, 6, 7, 9, 10 as well -- the state counts of standard (morphology) characters, whose transition-matrix classes are
//  engine instances of a few hundred patterns: a launch per dependency level of the level kernels was ten launches where this is one)
static inline bool wg_compiled(int S) { return (S >= 2 && S <= 10 && S != 4) || S == 16 || S == 20 || S == 40 || (S >= 60 && S <= 63); }
// FN<SC, WMAX, CH, DEPTH>: one row tile -> whole jobs two ahead; two row tiles -> half jobs one ahead (see k_walkg)
#if !defined(MBAMD_WG_DEPTH61)
#define MBAMD_WG_DEPTH61 1       // chunks the operand fetch of the 60..63-state kernels runs ahead (experiments: 2)
#endif
#define MBAMD_WG_DISPATCH(S, FN, ...)                                   \
    switch (S) {                                                        \
        case 2: FN<2, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 3: FN<3, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 5: FN<5, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 6: FN<6, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 7: FN<7, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 8: FN<8, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 9: FN<9, 8, 1, 2>(__VA_ARGS__); break;                     \
        case 10: FN<10, 8, 1, 2>(__VA_ARGS__); break;                   \
        case 16: FN<16, 8, 1, 2>(__VA_ARGS__); break;                   \
        case 20: FN<20, 8, 1, 2>(__VA_ARGS__); break;                   \
        case 40: FN<40, 4, 1, 1>(__VA_ARGS__); break;                   \
        case 60: FN<60, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
        case 61: FN<61, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
        case 62: FN<62, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
        default: FN<63, 4, 2, MBAMD_WG_DEPTH61>(__VA_ARGS__); break;    \
    }

template <int SC_, int WMAX_, int CH_, int DEPTH_>
static void raise_walkg_lds(int maxLds)
{
    if (hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
        hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgsInline>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess)
        (void) hipGetLastError();
    if constexpr (WgShape<SC_>::BF) {            // (the range-safe instantiations exist where the pieces are bf16: wg_contract_bf16)
        if (hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgs, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
            hipFuncSetAttribute((const void*) k_walkg<SC_, WMAX_, CH_, DEPTH_, WalkGArgsInline, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess)
            (void) hipGetLastError();
    }
}

}  // namespace mbamd

#include "mbamd_f32.h"           // Instance

namespace mbamd {

// 20/61-state walk: waves per workgroup and LDS slots per wave for (tiles x categories x lists) workgroups.  Waves per
// workgroup are a power of two (two-wave workgroups are launched as four, see k_walkg; three or five leave SIMDs idle).
inline void Instance::wgGeometry(int lists, int& W, int& slots) const
{
    int numCU = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) numCU = prop.multiProcessorCount;
    // registers bound the residency: 4 (20 states) / 2 (61 states) waves per SIMD
    const int maxW = S > 32 ? 4 : 8, wavesPerCU = S > 32 ? 6 : 12;
    const int slotBytes = (int) wg_block_bytes(S);
    const long wgs = (long) (Ppad / MBAMD_WG_TW) * K * lists;
    const int perCU = (int) std::max(1L, (wgs + numCU - 1) / numCU);
    const int ldsPerWG = (160 * 1024) / std::min(perCU, 32) - 64;
    auto slotsFor = [&](int w) { return (ldsPerWG / w - MBAMD_WG_STAGE) / slotBytes; };
    long want = std::max(1L, std::min((long) maxW, ((long) wavesPerCU * numCU + wgs / 2) / wgs));
    W = 1;
    while (W * 2 <= want) W *= 2;
    while (W > 1 && slotsFor(W) < 4) W /= 2;
    if (sw.walkWaves) W = std::max(1, std::min(maxW, *sw.walkWaves));
    slots = std::max(3, std::min(24, slotsFor(W)));
    if (sw.maxLdsSlots) slots = std::max(1, std::min((160 * 1024 / W - MBAMD_WG_STAGE) / slotBytes, *sw.maxLdsSlots));
}

// ---------------------------------------------------------------------------------------------
// 20/61-state tree walk (mbamd_walkg.h).  beagleUpdatePartials only queues: MrBayes submits one list per eigen-system
// part of a codon model (reference src/mbbeagle.c:1095-1104), and a forest of three trees fills the chip where one tree
// cannot.  The queue runs -- as ONE program per wave, hazards cut into segments like any list -- when the next call
// arrives that depends on it.
// ---------------------------------------------------------------------------------------------
inline int Instance::updatePartialsG(const BeagleOperation* ops, int n, int cumIdx)
{
    bool clash = (int) wgListCum.size() >= MBAMD_WG_MAXLISTS;
    if (cumIdx != BEAGLE_OP_NONE)
        for (int c : wgListCum) clash |= c == cumIdx;            // one list per cumulative buffer and launch
    if (clash) {
        int rc = flushPending();
        if (rc) return rc;
    }
    wgListStart.push_back((int) wgOps.size());
    wgListCum.push_back(cumIdx);
    wgOps.insert(wgOps.end(), ops, ops + n);
    if (sw.noDefer) return flushPending();
    return BEAGLE_SUCCESS;
}

// does a beagle{Accumulate,Remove}ScaleFactors call commute with the queued lists?  (MrBayes removes the old node factors
// of part j+1 between the lists of parts j and j+1, reference src/mbbeagle.c:1086-1104)
inline bool Instance::scaleOpsIndependentOfPending(const int* idx, int n, int cumIdx) const
{
    for (int c : wgListCum) if (c == cumIdx) return false;
    for (const BeagleOperation& b : wgOps) {
        if (b.destinationScaleWrite == cumIdx || b.destinationScaleRead == cumIdx) return false;
        for (int i = 0; i < n; ++i)
            if (b.destinationScaleWrite == idx[i]) return false;
    }
    for (int i = 0; i < n; ++i)
        for (int c : wgListCum) if (c == idx[i]) return false;
    return true;
}

inline int Instance::flushWalkG()
{
    if (wgListCum.empty()) return BEAGLE_SUCCESS;
    std::vector<BeagleOperation> ops;
    std::vector<int> starts, cums;
    ops.swap(wgOps); starts.swap(wgListStart); cums.swap(wgListCum);
    const int n = (int) ops.size();
    int nl = (int) cums.size();
    std::vector<int> listOf(n, 0);
    for (int q = 0; q < nl; ++q)
        for (int o = starts[q]; o < (q + 1 < nl ? starts[q + 1] : n); ++o) listOf[o] = q;
    // ---- plan cache key: the operations as submitted and the list boundaries ---------------------------------------------
    std::vector<int> key(reinterpret_cast<const int*>(ops.data()), reinterpret_cast<const int*>(ops.data()) + (size_t) n * 7);
    for (int q = 0; q < nl; ++q) key.push_back(starts[q]);
    // One list that does not rescale may hold several independent trees: without a cumulative buffer MrBayes submits the
    // operations of all eigen-system parts as ONE list (reference src/mbbeagle.c:1029-1104, No_Rescale), and a move dirties
    // the same root-ward path in each part.  Its connected components are treated like lists of their own.
    if (nl == 1 && cums[0] == BEAGLE_OP_NONE && n >= 2) {
        std::vector<int> comp(n);
        for (int o = 0; o < n; ++o) comp[o] = o;
        auto find = [&](int x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
        std::unordered_map<int, int> writer, scaleUser;
        bool ok = true;
        for (int o = 0; o < n && ok; ++o) {
            const BeagleOperation& b = ops[o];
            for (int c : {b.child1Partials, b.child2Partials}) {
                auto it = writer.find(c);
                if (it != writer.end()) comp[find(o)] = find(it->second);
            }
            if (writer.count(b.destinationPartials)) ok = false;            // (written twice: leave it to the hazard segments)
            writer[b.destinationPartials] = o;
            for (int sc : {b.destinationScaleWrite, b.destinationScaleRead})
                if (sc != BEAGLE_OP_NONE) {
                    auto it = scaleUser.find(sc);
                    if (it != scaleUser.end()) comp[find(o)] = find(it->second); else scaleUser[sc] = o;
                }
        }
        for (int o = 0; o < n && ok; ++o)                                    // a buffer read before a later operation writes it
            for (int c : {ops[o].child1Partials, ops[o].child2Partials}) {
                auto it = writer.find(c);
                if (it != writer.end() && it->second > o) ok = false;
            }
        std::vector<int> roots;
        for (int o = 0; o < n && ok; ++o) if (find(o) == o) roots.push_back(o);
        if (ok && roots.size() >= 2 && roots.size() <= (size_t) MBAMD_WG_MAXLISTS) {
            std::vector<BeagleOperation> sorted;
            sorted.reserve(n);
            starts.clear();
            for (size_t q = 0; q < roots.size(); ++q) {
                starts.push_back((int) sorted.size());
                for (int o = 0; o < n; ++o) if (find(o) == roots[q]) sorted.push_back(ops[o]);
            }
            ops.swap(sorted);
            nl = (int) roots.size();
            cums.assign(nl, BEAGLE_OP_NONE);
            for (int q = 0; q < nl; ++q)
                for (int o = starts[q]; o < (q + 1 < nl ? starts[q + 1] : n); ++o) listOf[o] = q;
        }
    }
    wgFresh = 0;
    for (int q = 0; q < MBAMD_WG_MAXLISTS; ++q) wgCum[q] = nullptr;
    for (int q = 0; q < nl; ++q) {
        const int ci = cums[q];
        if (ci == BEAGLE_OP_NONE) continue;
        bool fresh;
        int rc = scales.cumulativeForAdd(ci, wgCum[q], fresh);
        if (rc) return rc;
        if (fresh) wgFresh |= 1 << q;
    }
    bool build;
    Plan* plan = cachedPlan(key.data(), key.size(), build);
    if (build) {
        // Mutually independent lists (the eigen-system parts of a codon model) run as separate workgroups of ONE launch --
        // three times the workgroups for a grid that does not fill the chip otherwise -- if they compile to the same geometry;
        // anything else is one merged forest.
        bool independent = nl > 1;
        if (independent) {
            std::vector<int> wr(nBuffers, -1), rd(nBuffers, -1);
            std::vector<int> sc(scales.count(), -1);
            for (int o = 0; o < n && independent; ++o) {
                const BeagleOperation& b = ops[o];
                const int q = listOf[o];
                auto clash = [&](std::vector<int>& v, int i) { if (i < 0 || i >= (int) v.size()) return false; if (v[i] >= 0 && v[i] != q) return true; v[i] = q; return false; };
                if (clash(wr, b.destinationPartials) || (b.destinationPartials >= 0 && b.destinationPartials < nBuffers && rd[b.destinationPartials] >= 0 && rd[b.destinationPartials] != q)) independent = false;
                for (int c : {b.child1Partials, b.child2Partials})
                    if (c >= 0 && c < nBuffers && !(tipStates[c] && wr[c] < 0)) {
                        if (wr[c] >= 0 && wr[c] != q) independent = false;
                        if (rd[c] < 0) rd[c] = q; else if (rd[c] != q) rd[c] = 1 << 20;      // (read by several lists: fine unless one writes it)
                    }
                if (b.destinationScaleWrite != BEAGLE_OP_NONE && clash(sc, b.destinationScaleWrite)) independent = false;
                if (b.destinationScaleRead != BEAGLE_OP_NONE && b.destinationScaleRead >= 0 && b.destinationScaleRead < (int) sc.size() &&
                    sc[b.destinationScaleRead] >= 0 && sc[b.destinationScaleRead] != q) independent = false;
            }
            for (int o = 0; o < n && independent; ++o)                  // a buffer one list writes must not be read by another
                for (int c : {ops[o].child1Partials, ops[o].child2Partials})
                    if (c >= 0 && c < nBuffers && wr[c] >= 0 && wr[c] != listOf[o]) independent = false;
            if (sw.verbose) std::fprintf(stderr, "[mbamd] %d queued lists, %d operations: %s\n", nl, n, independent ? "independent" : "one forest");
        }
        int rc;
        {
            StatTimer st_(ST_PLAN);
            plan->lists = 1;
            plan->pathG = plan->forked = false;
            rc = BEAGLE_SUCCESS;
            bool done = (nl == 1 || independent) && buildPathG(*plan, ops.data(), n, starts, nl);
            if (!done) { plan->inlineProg.clear(); plan->pathG = plan->forked = false; }
            if (!done && independent) {
                const int keepW = w4.maxW, keepS = w4.maxSlots, keepS1 = w4.maxSlots1;
                wgGeometry(nl, w4.maxW, w4.maxSlots);
                w4.maxSlots1 = w4.maxSlots;
                rc = buildWalk(*plan, ops.data(), n, listOf.data(), true);
                w4.maxW = keepW; w4.maxSlots = keepS; w4.maxSlots1 = keepS1;
                bool same = rc == BEAGLE_SUCCESS && (int) plan->segments.size() == nl;
                for (size_t i = 1; same && i < plan->segments.size(); ++i)
                    same = plan->segments[i].W == plan->segments[0].W && plan->segments[i].entries == plan->segments[0].entries &&
                           plan->segments[i].first == plan->segments[0].first + i * (size_t) plan->segments[0].W * plan->segments[0].entries;
                if (same) {
                    int ns = 0;
                    for (const Plan::Segment& sg : plan->segments) ns = std::max(ns, sg.nslots);
                    for (Plan::Segment& sg : plan->segments) sg.nslots = ns;
                    plan->lists = nl;
                    done = true;
                    // (several independent lists = several segments, one launch: short enough, they travel in its arguments too)
                    if (!sw.noInlinePrograms && w4table.size() <= (size_t) MBAMD_W4_INLINE) plan->inlineProg = w4table;
                }
            }
            if (!done) rc = buildWalk(*plan, ops.data(), n, listOf.data(), false);
        }
        if (planBuilt(*plan, rc)) return rc;
    }
    // one flush = one list event, however many eigen-system parts it carries
    listLaunched(ops.data(), n, plan->pathG, plan->forked);
    // Which instantiation of the bf16-piece contraction (wgRescaled).  Here, not earlier: the plan exists, so every index of every
    // operation has been checked (checkOperation, when this list or an identical one was compiled).  The operations in the order
    // they run: a child an earlier operation of the flush writes is what that operation leaves (wgWrote: -1 not written, else
    // whether it rescales), whatever the buffer held before -- compact states included.  The buffers' own marks change only once
    // the launch has been accepted; a launch that failed leaves results nobody knows.
    const bool pieces = S >= MBAMD_WG_BF_MIN;
    wgRangeSafe = false;
    if (pieces) {
        if (wgRescaled.size() != (size_t) nBuffers) wgRescaled.assign((size_t) nBuffers, 0);
        wgWrote.assign((size_t) nBuffers, -1);
        for (const BeagleOperation& b : ops) {
            for (int c : {b.child1Partials, b.child2Partials}) {
                const int8_t w = wgWrote[(size_t) c];
                if (w >= 0 ? w == 0 : (!tipStates[c] && !wgRescaled[(size_t) c])) wgRangeSafe = true;
            }
            wgWrote[(size_t) b.destinationPartials] = b.destinationScaleWrite != BEAGLE_OP_NONE ? 1 : 0;
        }
        ++(wgRangeSafe ? wgFlushesRangeSafe : wgFlushesPlain);
    }
    const int rrc = timedRun(*plan, nullptr);
    if (pieces)
        for (const BeagleOperation& b : ops) wgRescaled[(size_t) b.destinationPartials] = rrc == BEAGLE_SUCCESS && wgWrote[(size_t) b.destinationPartials] == 1 ? 1 : 0;
    return rrc;
}

// The same for the 20/61-state walk (k_pathg, mbamd_pathg_kernel.h): `nl` mutually independent lists (the eigen-system parts of a
// codon model; one for a protein model), each a root-ward path -- or root-ward paths that join, at the same positions in every
// list --, all of the same length.  Entries [list][operation] in the tile arena's units (byte offsets of a buffer inside a tile,
// tip states at 32 bytes per buffer, matrix buffers in bytes); an entry carries its list's index.
static inline bool pathg_compiled(int S) { return S == 20 || (S >= 60 && S <= 63); }
inline bool Instance::buildPathG(Plan& plan, const BeagleOperation* ops, int n, const std::vector<int>& starts, int nl)
{
    if (sw.noPathG || !pathg_compiled(S) || nl < 1 || nl > MBAMD_WG_MAXLISTS || n < nl || n % nl != 0) return false;
    const int L = n / nl;
    if (L < 2 || (size_t) n > (size_t) MBAMD_W4_INLINE) return false;      // (a single operation gains nothing; the program travels in the kernel arguments)
    for (int q = 0; q < nl; ++q) if (starts[(size_t) q] != q * L) return false;
    bool forked;
    if (!recognisePath(ops, n, L, forked) || (forked && sw.noForkPath)) return false;
    // every list the same arms: the workgroups of one launch run the same program shape
    for (int o = L; o < n; ++o)
        if (pathSteps[(size_t) o].start != pathSteps[(size_t) (o % L)].start || pathSteps[(size_t) o].join != pathSteps[(size_t) (o % L)].join) return false;
    const uint32_t pbuf = (uint32_t) K * wg_block_bytes(S), mbuf = (uint32_t) (matrixFloats * 4);
    plan.inlineProg.resize((size_t) n);
    for (int o = 0; o < n; ++o) {
        // (a different scratch row for neighbouring entries, see the arena)
        plan.inlineProg[(size_t) o] = pathEntry(pathSteps[(size_t) o], pbuf, (uint32_t) MBAMD_WG_TW, mbuf, (int) scales.count() + (o % L) % MBAMD_WG_SCRATCH_ROWS);
        plan.inlineProg[(size_t) o].ctl |= (uint32_t) (o / L) << 10;
    }
    if (sw.verbose) std::fprintf(stderr, "[mbamd] walk plan: %d list(s) of %d operations each: root-ward paths%s (k_pathg)\n", nl, L, forked ? " that join" : "");
    plan.pathG = true;
    plan.lists = nl;
    pathPlan(plan, L, forked);
    return true;
}

// the launch of k_walkg's instantiation for A, the form of the arguments (WalkGArgs: the program in a device buffer; WalkGArgsInline: in
// the arguments themselves), and RS_, the range-safe contraction (instantiated where the pieces are bf16 only)
template <int SC_, int WMAX_, int CH_, int DEPTH_, class A, bool RS_>
static void launch_walkg_as(hipStream_t stream, const A& args, const WalkGArgs& a, int W, int nslots)
{
    auto kern = k_walkg<SC_, WMAX_, CH_, DEPTH_, A, RS_>;
    MBAMD_LAUNCH_BARRIER(kern, walkg_grid(a.Ppad / MBAMD_WG_TW, a.K * a.lists), 64 * W * (a.spread ? 2 : 1), wg_lds_bytes(W, nslots, a.S), stream, args);
}
template <int SC_, int WMAX_, int CH_, int DEPTH_>
inline void Instance::launch_walkg_t(Instance& in, const WalkGArgs& a, int W, int nslots, const std::vector<Walk4Entry>* inlineProg)
{
    auto launch = [&](const auto& args) {
        typedef std::decay_t<decltype(args)> A;
        if constexpr (WgShape<SC_>::BF) {
            if (in.wgRangeSafe) { launch_walkg_as<SC_, WMAX_, CH_, DEPTH_, A, true>(in.stream, args, a, W, nslots); return; }
        }
        launch_walkg_as<SC_, WMAX_, CH_, DEPTH_, A, false>(in.stream, args, a, W, nslots);
    };
    if (inlineProg && !inlineProg->empty()) {
        WalkGArgsInline ai;
        ai.a = a;
        ai.a.prog = nullptr;
        std::memcpy(ai.inl, inlineProg->data(), inlineProg->size() * sizeof(Walk4Entry));
        launch(ai);
    } else {
        launch(a);
    }
}

// ... and of k_pathg's: the program always travels in the arguments; FORK_: arms that join
template <int SC_, bool FORK_, bool RS_>
static void launch_pathg_as(hipStream_t stream, const WalkGArgsInline& ai)
{
    auto kern = k_pathg<SC_, WalkGArgsInline, FORK_, RS_>;
    MBAMD_LAUNCH_BARRIER(kern, walkg_grid(ai.a.Ppad / MBAMD_WG_TW, ai.a.K * ai.a.lists), 128, pathg_lds_bytes(ai.a.S, FORK_), stream, ai);
}
template <int SC_>
inline void Instance::launch_pathg_t(Instance& in, const WalkGArgs& a, const std::vector<Walk4Entry>& prog, bool forked)
{
    WalkGArgsInline ai;
    ai.a = a;
    ai.a.prog = nullptr;
    std::memcpy(ai.inl, prog.data(), prog.size() * sizeof(Walk4Entry));
    if constexpr (WgShape<SC_>::BF) {
        if (in.wgRangeSafe) {
            if (forked) launch_pathg_as<SC_, true, true>(in.stream, ai);
            else launch_pathg_as<SC_, false, true>(in.stream, ai);
            return;
        }
    }
    if (forked) launch_pathg_as<SC_, true, false>(in.stream, ai);
    else launch_pathg_as<SC_, false, false>(in.stream, ai);
}

// the instance's side of a general-state walk's arguments, with the cumulative buffers of the lists being flushed; the call
// site adds program, geometry and which of those buffers are fresh
inline WalkGArgs Instance::walkGArgs() const
{
    WalkGArgs a;
    std::memset(&a, 0, sizeof a);
    a.partials = arenaPartials;
    a.tileBytes = wgTileBytes;
    a.tips = arenaTipStates;
    a.tipTileBytes = wgTipTileBytes;
    a.exps = scales.nodeExponents();
    a.estride = scales.blockStride();
    a.matrices = matrices;
    a.tabOff = (unsigned) (wgTabFloats * 4);
    a.tabBytes = (unsigned) (wg_table_floats(S) * 4);
    for (int q = 0; q < MBAMD_WG_MAXLISTS; ++q) a.cum[q] = wgCum[q];
    a.K = K; a.Ppad = Ppad; a.ntiles = Ppad / MBAMD_WG_TW; a.S = S; a.SP = SP;
    return a;
}

inline int Instance::runWalkG(const Plan& plan)
{
    WalkGArgs a = walkGArgs();
    a.lists = plan.lists;
    if (plan.pathG) {
        a.entries = plan.segments.front().entries;
        a.cumFresh = wgFresh;
        switch (S) {
            case 20: launch_pathg_t<20>(*this, a, plan.inlineProg, plan.forked); break;
            case 60: launch_pathg_t<60>(*this, a, plan.inlineProg, plan.forked); break;
            case 61: launch_pathg_t<61>(*this, a, plan.inlineProg, plan.forked); break;
            case 62: launch_pathg_t<62>(*this, a, plan.inlineProg, plan.forked); break;
            default: launch_pathg_t<63>(*this, a, plan.inlineProg, plan.forked); break;
        }
        HIP_TRY(hipGetLastError());
        timer.count();
        return BEAGLE_SUCCESS;
    }
    for (const Plan::Segment& sg : plan.segments) {
        if (plan.lists > 1 && &sg != &plan.segments.front()) break;     // (independent lists: one launch covers all segments)
        a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
        a.entries = sg.entries;
        a.nslots = sg.nslots;
        a.cumFresh = (&sg == &plan.segments.front()) ? wgFresh : 0;
        a.spread = sg.W == 2 ? 1 : 0;     // two-wave workgroups are launched as four (see k_walkg)
        MBAMD_WG_DISPATCH(S, launch_walkg_t, *this, a, sg.W, sg.nslots, &plan.inlineProg);
        HIP_TRY(hipGetLastError());
        timer.count();
    }
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd

#endif  // MBAMD_F32_WALKG_H_
