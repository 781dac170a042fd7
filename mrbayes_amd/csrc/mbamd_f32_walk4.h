// mbamd_f32_walk4.h -- the single-precision engine (mbamd_f32.h): the 4-state tree walk (kernels: mbamd_walk4.h; scheduler:
// mbamd_walk4_host.h; unstored subtrees: mbamd_walk4_unstored.h).  Defines Instance::configureWalk (the walk geometry of both arena
// layouts), updatePartials4, listLaunched, buildPath4, walk4Args, runWalk, and the held path: runHeldPath, integratePath4.
#ifndef MBAMD_F32_WALK4_H_
#define MBAMD_F32_WALK4_H_

#include "mbamd_f32.h"           // Instance
#include "mbamd_f32_walkg.h"     // MBAMD_WG_DISPATCH, raise_walkg_lds (configureWalk)

namespace mbamd {

// ---------------------------------------------------------------------------------------------
// Tree-walk geometry.  The grid is (pattern blocks) x (categories) workgroups of W waves; each wave owns `slots` LDS
// slots of 1 KiB.  W and the slot count are chosen so that the whole grid is resident at once when the chip allows it:
// few blocks -> more tree parallelism per block, many blocks -> single-wave workgroups with deep slot stacks.
#define MBAMD_W4_PLAIN_WAVES_PER_CU 32    // eight waves per SIMD: beyond that the grid is not resident
#define MBAMD_W4_PLAIN_MAXW 4            // (the sweep's largest)
// microseconds per entry and wave of the plain 4-state loop against the waves resident on a CU: measured on the MI355X at DNA 500 x
// 20 000 and 1000 x 50 000, W = 1 ... 4 (profiles/walk4_plain_waves.txt section 3), linear between the points and beyond the last
static inline double walk4_entry_us(double wavesPerCU)
{
    static const double x[] = {4.9, 9.8, 12.2, 14.7, 19.6, 24.4}, y[] = {0.354, 0.395, 0.428, 0.485, 0.542, 0.747};
    if (wavesPerCU <= x[0]) return y[0];
    int i = 1;
    while (i < 5 && wavesPerCU > x[i]) ++i;
    return y[i - 1] + (y[i] - y[i - 1]) * (wavesPerCU - x[i - 1]) / (x[i] - x[i - 1]);
}
inline int Instance::configureWalk()
{
    int numCU = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) numCU = prop.multiProcessorCount;
    const int maxLds = 160 * 1024;
    if (s4 && (hipFuncSetAttribute((const void*) k_walk4_t<Walk4Args>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
               hipFuncSetAttribute((const void*) k_walk4_t<Walk4Args, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
               hipFuncSetAttribute((const void*) k_walk4_t<Walk4Args, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess ||
               hipFuncSetAttribute((const void*) k_walk4_t<Walk4ArgsInline>, hipFuncAttributeMaxDynamicSharedMemorySize, maxLds) != hipSuccess))
        (void) hipGetLastError();
    if (wg) {
        // one wave = (32-pattern tile, category); registers bound the residency: 20 states 4 waves per SIMD, 61 states 2
        const unsigned slotBytes = wg_block_bytes(S);
        MBAMD_WG_DISPATCH(S, raise_walkg_lds, maxLds);
        wgGeometry(1, w4.maxW, w4.maxSlots);
        w4.maxSlots1 = w4.maxSlots;
        if (!sw.walkWaves && !sw.maxLdsSlots) {   // a single-wave program may use the LDS of the whole workgroup
            const long wgsG = (long) (Ppad / MBAMD_WG_TW) * K;
            const int perCUG = (int) std::max(1L, (wgsG + numCU - 1) / numCU);
            w4.maxSlots1 = std::max(w4.maxSlots, std::min(24, (int) (((160 * 1024) / std::min(perCUG, 32) - 64 - MBAMD_WG_STAGE) / (int) slotBytes)));
        }
        w4.memSlots = false;
        w4.leadNops = MBAMD_WG_LEAD; w4.unroll = 3; w4.tailNops = MBAMD_WG_TAIL;
        w4.prefetchDistance = 0;
        if (sw.walkSmallPhase) w4.smallPhase = std::max(1, *sw.walkSmallPhase);
        if (sw.verbose) std::fprintf(stderr, "[mbamd] tree walk (%d states): %ld workgroups, up to %d waves x %d slots of %u bytes\n",
                                     S, (long) (Ppad / MBAMD_WG_TW) * K, w4.maxW, w4.maxSlots, slotBytes);
        return BEAGLE_SUCCESS;
    }
    const long wgs = (long) (Ppad / 64) * K;
    const int perCU = (int) std::max(1L, (wgs + numCU - 1) / numCU);          // workgroups a CU must host for full residency
    const int ldsPerWG = (160 * 1024) / std::min(perCU, 32) - 64;
    auto slotsFor = [&](int W) { return (ldsPerWG / W - MBAMD_W4_STAGE) / 1024; };
    // measured (profiles/): about 12-15 waves per CU (3-4 per SIMD) is the sweet spot -- fewer leave the scalar-load
    // latency uncovered, more cost LDS (slots) and tree-partition efficiency (phases, padding) without buying anything.
    // (Round 6, profiles/r06_walk4_waves.txt: DNA 500 x 20 000 = 4.9 workgroups per CU ran two waves each until then; with three
    //  -- 15 waves per CU, 190 entries per wave instead of 264 -- the evaluation takes 0.158-0.164 ms instead of 0.181; four: 0.192.)
    int W = (int) std::max(1L, std::min((long) MBAMD_W4_MAXW, (14L * numCU + wgs / 2) / wgs));
    while (W > 1 && slotsFor(W) < 7) --W;
    if (sw.walkWaves) W = std::max(1, std::min(MBAMD_W4_MAXW, *sw.walkWaves));
    int slots = std::max(3, std::min(48, slotsFor(W)));
    if (sw.maxLdsSlots) slots = std::max(3, std::min(150 / W, *sw.maxLdsSlots));
    w4.maxW = W;
    w4.maxSlots = slots;
    w4.maxSlots1 = sw.maxLdsSlots ? slots : std::max(slots, std::min(40, slotsFor(1)));
    if (sw.walkPrefetch) w4.prefetchDistance = std::max(0, *sw.walkPrefetch);
    w4.forward = true;
    w4.safeWaits = sw.walkSafe;
    if (sw.walkSmallPhase) w4.smallPhase = std::max(1, *sw.walkSmallPhase);
    // Whole-tree lists on the plain loop (Walk4Builder::plainWaves) have a geometry of their own.  Their time is one wave's serial chain
    // of entries, each with an exposed scalar-load round trip: more waves per workgroup shorten the chain, but every wave more on a CU
    // makes an entry slower (at 24 waves per CU 1.7 times what it is at 12), and the whole grid must stay resident.  The LDS of a
    // workgroup's share of the CU is ONE pool of slots, nothing in front of them; a list that does not fit it without an eviction, or
    // whose cut does not win against one wave, is tried on fewer waves and then gets the geometry above.
    // How many: the measured time per entry and wave against the waves on a CU (profiles/walk4_plain_waves.txt section 3) says what W
    // waves of n / W entries would take; the W with the least, and per W the longest wave that still beats one wave by 5 %.
    {
        const double wpc = (double) wgs / numCU;
        double bestTime = walk4_entry_us(wpc);
        w4.plainWaves = 1;
        for (int w = 2; w <= MBAMD_W4_PLAIN_MAXW; ++w) {
            w4.plainShare[w] = (int) (1024.0 * 0.95 * walk4_entry_us(wpc) / walk4_entry_us(wpc * w));
            if (perCU * w > MBAMD_W4_PLAIN_WAVES_PER_CU) continue;                 // (the whole grid resident)
            const double tw = walk4_entry_us(wpc * w) / w;
            if (tw < bestTime) { bestTime = tw; w4.plainWaves = w; }
        }
        w4.plainDescend = !sw.walkWaves;
    }
    if (sw.walkWaves) w4.plainWaves = W;
    if (sw.noPlainWalk) w4.plainWaves = 0;
    // (a sixteenth of the share kept back: 12 slots of the 12.2 KiB that 13 workgroups per CU leave each ran as 12 workgroups per CU and
    //  a second round, profiles/walk4_plain_waves.txt; forced: the pool is that many)
    w4.plainSlots = std::min(250, sw.maxLdsSlots ? slots : (ldsPerWG - ldsPerWG / 16) / 1024);
    if (sw.walkPlainMinOps) w4.plainMinOps = std::max(1, *sw.walkPlainMinOps);
    if (sw.verbose) std::fprintf(stderr, "[mbamd] tree walk: %ld workgroups (%d per CU), up to %d waves x %d slots\n", wgs, perCU, W, slots);
    return BEAGLE_SUCCESS;
}

// ---------------------------------------------------------------------------------------------
// 4-state path: beagleUpdatePartials -> per-wave programs of the tree-walk kernel (mbamd_walk4.h).
// ---------------------------------------------------------------------------------------------
// A compiled list of an arena layout was launched (or is held), compiled now or before: its destinations are valid and hold no recipe (overwritten;
// the launch leaves its own small subtrees unstored afresh, runWalk), the exponent buffers it writes hold node exponents; the list counters
inline void Instance::listLaunched(const BeagleOperation* ops, int n, bool path, bool forked)
{
    for (int o = 0; o < n; ++o) {
        valid[ops[o].destinationPartials] = 1;
        unstored4.forget(ops[o].destinationPartials);
        if (ops[o].destinationScaleWrite != BEAGLE_OP_NONE) scales.nodeWritten(ops[o].destinationScaleWrite);
    }
    listsTotal++;
    if (path) { listsPath++; if (forked) forkedPaths++; }
    else { listsWalked++; opsWalked += n; }
}

inline int Instance::updatePartials4(const BeagleOperation* ops, int n, int cumIdx)
{
    if (heldPath) { int prc = runHeldPath(); if (prc) return prc; }      // (a list behind a held path: the path runs first)
    { int src = snapshotNow(); if (src) return src; }                    // (no integration followed the launch; this call may recompile the plan)
    if (unstored4.any()) {
        // children from outside the list that an earlier launch left unstored: made now, before a path is held -- the launch runs
        // while the host compiles or looks up the list
        std::vector<int>& ext = w4segList;
        std::vector<char>& written = w4written;
        ext.clear();
        written.assign((size_t) nBuffers, 0);
        for (int o = 0; o < n; ++o) {
            for (const int c : {ops[o].child1Partials, ops[o].child2Partials})
                if (unstored4.holds(c) && !written[(size_t) c]) ext.push_back(c);
            if (ops[o].destinationPartials >= 0 && ops[o].destinationPartials < nBuffers) written[(size_t) ops[o].destinationPartials] = 1;
        }
        if (!ext.empty()) { int src = ensureStored(ext.data(), (int) ext.size()); if (src) return src; }
    }
    int32_t* cumPtr = nullptr;
    walkCumFresh = false;
    if (cumIdx != BEAGLE_OP_NONE) { int rc = scales.cumulativeForAdd(cumIdx, cumPtr, walkCumFresh); if (rc) return rc; }
    bool build;
    Plan* plan = cachedPlan(reinterpret_cast<const int*>(ops), (size_t) n * 7, build);
    if (build) {
        int rc = flushMatrices();                // the matrix kernel runs while the host compiles the list
        if (rc == BEAGLE_SUCCESS) {
            StatTimer st_(ST_PLAN);
            plan->path = plan->forked = false;
            plan->unstoredSubtrees.clear();
            rc = buildPath4(*plan, ops, n) ? BEAGLE_SUCCESS : buildWalk(*plan, ops, n);
        }
        if (planBuilt(*plan, rc)) return rc;
    }
    listLaunched(ops, n, plan->path, plan->forked);
    int mrc = flushMatrices();
    if (mrc) return mrc;
    if (plan->path && !sw.noFusePath && K <= 8 && plan->inlineProg.size() <= MBAMD_W4_INLINE) {
        // hold it: the next call decides (runHeldPath / integratePath4)
        heldPath = plan;
        heldPaths++;
        heldPathCum = cumPtr;
        heldPathFresh = walkCumFresh;
        heldPathDst = ops[n - 1].destinationPartials;
        return BEAGLE_SUCCESS;
    }
    return timedRun(*plan, cumPtr);
}

// One list as k_path4's entries (mbamd_walk4.h): partials buffers in KiB of the buffer-major arena, 32 bytes of state bitplanes
// per tip, matrices [K][4][4]; the first entry of an arm carries the arm's length.
inline bool Instance::buildPath4(Plan& plan, const BeagleOperation* ops, int n)
{
    if (sw.noPath4 || n < 1 || n > MBAMD_W4_INLINE) return false;
    bool forked;
    if (!recognisePath(ops, n, n, forked) || (forked && sw.noForkPath)) return false;
    const uint32_t pbuf = (uint32_t) ((size_t) (Ppad / 64) * K), mbuf = (uint32_t) K * 64u;
    plan.inlineProg.resize((size_t) n);
    for (int i = 0; i < n; ++i) {
        const PathStep& p = pathSteps[(size_t) i];
        plan.inlineProg[(size_t) i] = pathEntry(p, pbuf, 32u, mbuf, (int) scales.count());
        plan.inlineProg[(size_t) i].ctl |= (uint32_t) p.arm << 16;
    }
    plan.path = true;
    pathPlan(plan, n, forked);
    return true;
}

// the instance's side of a 4-state kernel's arguments; the call site adds program, geometry and cumulative buffer
inline Walk4Args Instance::walk4Args() const
{
    Walk4Args a{};
    a.partials = reinterpret_cast<f4*>(arenaPartials);
    a.pstride = geom.pstride;
    a.tips = arenaTips;
    a.tstride = geom.tstride;
    a.exps = scales.nodeExponents();
    a.estride = scales.blockStride();
    a.matrices = matrices;
    a.K = K;
    a.Ppad = Ppad;
    a.nblocks = Ppad / 64;
    return a;
}

inline int Instance::runWalk(const Plan& plan, int32_t* cum)
{
    Walk4ArgsInline ai;
    Walk4Args& a = ai.a;
    a = walk4Args();
    a.cum = cum;
    if (!plan.inlineProg.empty()) std::memcpy(ai.inl, plan.inlineProg.data(), plan.inlineProg.size() * sizeof(Walk4Entry));
    if (plan.path) {
        a.entries = (int) plan.inlineProg.size();
        a.cumFresh = walkCumFresh ? 1 : 0;
        auto kernel = k_path4<Walk4ArgsInline>;
        MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, path4_lds_bytes((int) plan.inlineProg.size()), stream, ai);    // (lanes exchange through LDS: the emulation runs them as fibers)
        HIP_TRY(hipGetLastError());
        timer.count();
        return BEAGLE_SUCCESS;
    }
    for (const Plan::Segment& sg : plan.segments) {
        a.entries = sg.entries;
        a.nslots = sg.nslots;
        a.cumFresh = (walkCumFresh && &sg == &plan.segments.front()) ? 1 : 0;
        a.tail = sg.tail;
        bool plainHere = false;
        if (!plan.inlineProg.empty()) {
            auto kernel = k_walk4_t<Walk4ArgsInline>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64 * sg.W, walk4_lds_bytes(sg.W, sg.nslots), stream, ai);
        } else if (sg.waves) {
            // a whole-tree list cut over several waves, each on the plain loop: the program's own layout, no other kernel reads it
            a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
            auto kernel = k_walk4_t<Walk4Args, true, true>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64 * sg.W, walk4_waves_lds_bytes(sg.W, sg.nslots), stream, a);
            plainHere = true;
            if (!plan.unstoredSubtrees.empty()) { const int urc = unstored4.launched(plan, a); if (urc) return urc; }
        } else if (sg.plain && !sw.noPlainWalk) {
            // nothing rare in the program (a whole-tree list): the instantiation without that code; an odd operation count's padding entry joins the tail
            a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
            a.tail = sg.tail + (sg.peel ? 1 : 0);
            auto kernel = k_walk4_t<Walk4Args, true>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, sg.nslots), stream, a);
            plainHere = true;
            if (!plan.unstoredSubtrees.empty()) { const int urc = unstored4.launched(plan, a); if (urc) return urc; }
        } else {
            a.prog = reinterpret_cast<const Walk4Entry*>(plan.d_table) + sg.first;
            auto kernel = k_walk4_t<Walk4Args>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64 * sg.W, walk4_lds_bytes(sg.W, sg.nslots), stream, a);
        }
        HIP_TRY(hipGetLastError());
        ++(plainHere ? walksPlain : walksGeneric);
        if (plainHere) ++walksPlainByW[(sg.waves ? sg.W : 1) - 1];
        timer.count();
    }
    return BEAGLE_SUCCESS;
}

inline int Instance::runHeldPath()
{
    Plan* plan = heldPath;
    heldPath = nullptr;
    if (!plan) return BEAGLE_SUCCESS;
    walkCumFresh = heldPathFresh;
    return timedRun(*plan, heldPathCum);
}

// the held root-ward path (k_path4 plan) and the log-likelihood over its last result as ONE launch (k_path4_lnl, mbamd_walk4.h;
// arguments checked by integrate).  The path stays held until that launch is in the stream: whatever fails before, the path
// still runs on its own and the error is returned.
inline int Instance::integratePath4(const int* child, const int* prob, const int* wIdx, const int* fIdx, const int* cumIdx)
{
    Plan* plan = heldPath;
    PathLnl4 t;
    std::memset(&t, 0, sizeof t);
    if (child) {
        const Operand c = operand(child[0]);
        t.child = c.ptr; t.child_kind = c.kind;
        t.matrix = matrixPtr(prob[0]);
    }
    t.weights = d_weights + (size_t) wIdx[0] * K;
    t.freqs = d_freqs + (size_t) fIdx[0] * S;
    int rc = BEAGLE_SUCCESS;
    if (cumIdx && cumIdx[0] != BEAGLE_OP_NONE) rc = scales.cumulativeForRead(cumIdx[0], t.cum);
    t.pattern_weights = d_pweights;
    t.site = siteTarget();
    t.wsite = h_sums_dev;
    t.P = P;
    hipEvent_t ev0{}, ev1{};
    if (rc == BEAGLE_SUCCESS) rc = timer.launchesBegin(ev0, ev1);
    if (rc == BEAGLE_SUCCESS) {
        plan->lastLaunch = ++launchClock;
        Walk4ArgsInline ai;
        ai.a = walk4Args();
        ai.a.entries = (int) plan->inlineProg.size();
        ai.a.cum = heldPathCum;
        ai.a.cumFresh = heldPathFresh ? 1 : 0;
        std::memcpy(ai.inl, plan->inlineProg.data(), plan->inlineProg.size() * sizeof(Walk4Entry));
        auto kernel = k_path4_lnl<Walk4ArgsInline>;
        MBAMD_LAUNCH_BARRIER(kernel, 8u * (unsigned) ((Ppad / 64 + 7) / 8), 64 * K, path4_lnl_lds_bytes(ai.a.entries, K), stream, ai, t);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = hip_fail(le, "k_path4_lnl");
    }
    if (rc) {
        (void) runHeldPath();
        return rc;
    }
    heldPath = nullptr;
    fusedPaths++;
    timer.count();
    return timer.launchesEnd(ev0, ev1);
}

}  // namespace mbamd

#endif  // MBAMD_F32_WALK4_H_
