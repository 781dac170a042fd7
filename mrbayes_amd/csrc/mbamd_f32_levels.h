// mbamd_f32_levels.h -- the single-precision engine (mbamd_f32.h): the level kernels (mbamd_kernels.h) and their matrix-core forms
// (mbamd_kernels_mfma.h), one launch per dependency level, with the deferral queue's merged launches.  Defines MBAMD_MFMA_DISPATCH[_SC]
// and mfma_shape_compiled (which shapes the split / serial kernels are instantiated for), Instance::launch_mfma*, launch_tips*,
// launch_gen, ensureTrace, buildGeneric, runGeneric, flushMerged (the merged-launch half of flushPending), integrateLevels.
#ifndef MBAMD_F32_LEVELS_H_
#define MBAMD_F32_LEVELS_H_

namespace mbamd {

// The shapes (NT, S, K) -- row tiles of 32 states, state count, rate categories -- the split and serial kernels are instantiated for,
// the first that fits: the 20- and 61-state specialisations (_SC: those alone -- the spine kernels have no others), then any state
// count, S = 0, at these tile and category counts.  Calls FN<NT, S, K>(...) of it; `served`: there was one.
#define MBAMD_MFMA_DISPATCH_SC(NT, S, K, served, FN, ...)                                       \
    do {                                                                                        \
        served = true;                                                                          \
        if ((NT) == 1 && (S) == 20 && (K) == 4) FN<1, 20, 4>(__VA_ARGS__);                      \
        else if ((NT) == 1 && (S) == 20 && (K) == 1) FN<1, 20, 1>(__VA_ARGS__);                 \
        else if ((NT) == 2 && (S) == 61 && (K) == 1) FN<2, 61, 1>(__VA_ARGS__);                 \
        else served = false;                                                                    \
    } while (0)
#define MBAMD_MFMA_DISPATCH(NT, S, K, served, FN, ...)                                          \
    do {                                                                                        \
        MBAMD_MFMA_DISPATCH_SC(NT, S, K, served, FN, __VA_ARGS__);                              \
        if (served) break;                                                                      \
        served = true;                                                                          \
        if ((NT) == 1 && (K) == 1) FN<1, 0, 1>(__VA_ARGS__);                                    \
        else if ((NT) == 1 && (K) == 2) FN<1, 0, 2>(__VA_ARGS__);                               \
        else if ((NT) == 1 && (K) == 4) FN<1, 0, 4>(__VA_ARGS__);                               \
        else if ((NT) == 2 && (K) == 1) FN<2, 0, 1>(__VA_ARGS__);                               \
        else if ((NT) == 2 && (K) == 2) FN<2, 0, 2>(__VA_ARGS__);                               \
        else served = false;                                                                    \
    } while (0)
template <int NT_, int SC_, int KC_> static inline void mfma_shape_none(int) {}
// ... whether that list serves these tile and category counts at any state count: lists of other shapes (three rate categories,
// say) are neither merged nor run as one serial launch
static inline bool mfma_shape_compiled(int NT, int K)
{
    bool served;
    MBAMD_MFMA_DISPATCH(NT, 0, K, served, mfma_shape_none, 0);
    return served;
}

}  // namespace mbamd

#include "mbamd_f32.h"           // Instance

namespace mbamd {

template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_t(Instance& in, const PartialsOp* ops, int count, int32_t* cum)
{
    const int gx = (in.Ppad + 127) / 128;
    const unsigned grid = (unsigned) (8 * ((gx + 7) / 8) * count);
    auto kern = k_partials_mfma<NT_, SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, grid, 256, 0, in.stream, ops, in.S, in.SP, in.Ppad, gx, cum);
}
template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_split_t(Instance& in, const OpTables& tabs, int count)
{
    constexpr int NP = 2 * KC_ * NT_;
    const int gx = in.Ppad / 32;
    auto kern = k_partials_mfma_split<NT_, SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx * count), 64 * NP, (size_t) NP * (8 * 64 + 32 + 16 * 32) * sizeof(float), in.stream, tabs, in.S,
                 in.SP, in.Ppad, gx);
}
// one launch over up to four operation tables (false: no split kernel for this shape)
inline bool Instance::launch_mfma_split(Instance& in, const OpTables& tabs, int count)
{
    bool served;
    MBAMD_MFMA_DISPATCH(in.NT, in.S, in.K, served, launch_mfma_split_t, in, tabs, count);
    return served;
}
template <int SC_, int KC_>
inline void Instance::launch_tips_t(Instance& in, const OpTables& tabs, int count)
{
    const int gx4 = (in.Ppad + 127) / 128;
    auto kern = k_partials_tips<SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx4 * count), 256, (size_t) 4 * in.S * 32 * sizeof(float), in.stream, tabs, in.S, in.SP, in.Ppad, gx4);
}
// operations on two compact tips, up to four tables (false: no kernel for this shape)
inline bool Instance::launch_tips(Instance& in, const OpTables& tabs, int count)
{
    const int S = in.S, K = in.K;
    if (S > 64) return false;
    if (S == 20 && K == 4) { launch_tips_t<20, 4>(in, tabs, count); return true; }
    if (S == 20 && K == 1) { launch_tips_t<20, 1>(in, tabs, count); return true; }
    if (S == 61 && K == 1) { launch_tips_t<61, 1>(in, tabs, count); return true; }
    if (K == 1) { launch_tips_t<0, 1>(in, tabs, count); return true; }
    if (K == 2 && S <= 32) { launch_tips_t<0, 2>(in, tabs, count); return true; }
    return false;
}
// MBAMD_WALK_TRACE: the buffer the serial MFMA kernels stamp their steps into, allocated when the first of them is launched
inline void Instance::ensureTrace()
{
    if (d_trace || !sw.walkTrace) return;
    if (hipMalloc(&d_trace, (size_t) 4096 * 8 * 3 * sizeof(long long)) != hipSuccess) d_trace = nullptr;
    else (void) hipMemset(d_trace, 0, (size_t) 4096 * 8 * 3 * sizeof(long long));
}
template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_serial_t(Instance& in, const OpTables& tabs, int ntables)
{
    constexpr int NP = 2 * KC_ * NT_;
    const int gx = in.Ppad / 32;
    auto kern = k_partials_mfma_serial<NT_, SC_, KC_>;
    in.ensureTrace();
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx * ntables), 64 * NP, (size_t) NP * (8 * 64 + 32 + 16 * 32) * sizeof(float), in.stream, tabs, in.S,
                 in.SP, in.Ppad, gx, in.d_trace);
    if (in.d_trace) { in.lastWalkSteps = tabs.start[0]; in.walkWaves = NP - 1; }
}
template <int NT_, int SC_, int KC_>
inline void Instance::launch_mfma_spine_t(Instance& in, const OpTables& tabs, int ntables)
{
    constexpr int NP = 2 * KC_ * NT_;
    const int gx = in.Ppad / 32;
    in.ensureTrace();
    auto kern = k_partials_mfma_spine<NT_, SC_, KC_>;
    MBAMD_LAUNCH_BARRIER(kern, (unsigned) (gx * ntables), 64 * (NP + 1), ((size_t) NP * (8 * 64 + 32) + (size_t) 2 * KC_ * SC_ * 32) * sizeof(float),
                 in.stream, tabs, in.SP, gx, in.d_trace);
    if (in.d_trace) { in.lastWalkSteps = tabs.start[0]; in.walkWaves = NP - 1; }
}
// one launch that walks up to four whole (narrow) operation lists; tabs.start[t] = operations of list t
inline bool Instance::launch_mfma_serial(Instance& in, const OpTables& tabs, int ntables)
{
    bool served = false;
    // the software-pipelined variant where there is one (MBAMD_NO_SPINE=1: the plain serial kernel)
    if (!in.sw.noSpine) MBAMD_MFMA_DISPATCH_SC(in.NT, in.S, in.K, served, launch_mfma_spine_t, in, tabs, ntables);
    if (!served) MBAMD_MFMA_DISPATCH(in.NT, in.S, in.K, served, launch_mfma_serial_t, in, tabs, ntables);
    return served;
}
inline bool Instance::launch_mfma(Instance& in, const PartialsOp* ops, int count, int32_t* cum)
{
    const int S = in.S, K = in.K;
    if (!in.sw.mfmaWhole) {                 // default: one wave per factor tile (MBAMD_MFMA_WHOLE=1 selects the wave-per-tile-column kernel)
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        tabs.ops[0] = ops;
        tabs.cum[0] = cum;
        for (int t = 1; t <= MBAMD_MAX_TABLES; ++t) tabs.start[t] = 1 << 30;
        if (launch_mfma_split(in, tabs, count)) return true;
    }
    if (in.NT == 1) {
        if (S == 20 && K == 4) launch_mfma_t<1, 20, 4>(in, ops, count, cum);
        else if (S == 20 && K == 1) launch_mfma_t<1, 20, 1>(in, ops, count, cum);
        else if (K == 1) launch_mfma_t<1, 0, 1>(in, ops, count, cum);
        else if (K == 2) launch_mfma_t<1, 0, 2>(in, ops, count, cum);
        else if (K == 3) launch_mfma_t<1, 0, 3>(in, ops, count, cum);
        else if (K == 4) launch_mfma_t<1, 0, 4>(in, ops, count, cum);
        else return false;
    } else {
        if (S == 61 && K == 1) launch_mfma_t<2, 61, 1>(in, ops, count, cum);
        else if (K == 1) launch_mfma_t<2, 0, 1>(in, ops, count, cum);
        else if (K == 2) launch_mfma_t<2, 0, 2>(in, ops, count, cum);
        else return false;
    }
    return true;
}

template <int SP_, int FK_>
inline void Instance::launch_gen(Instance& in, const PartialsOp* ops, int count, int32_t* cum)
{
    auto kern = k_partials_gen<SP_, FK_>;
    MBAMD_LAUNCH(kern, dim3(in.Ppad / 64, count), 64, 0, in.stream, ops, in.S, in.K, in.Ppad, cum);
}

// General path: order the operations by dependency level (RAW, WAR and WAW on buffer indices) and
// launch one grid per level.
inline int Instance::buildGeneric(Plan& plan, std::vector<PartialsOp>& dev, const std::vector<int>& dstIdx,
                           const std::vector<int>& c1Idx, const std::vector<int>& c2Idx)
{
    const int n = (int) dev.size();
    std::vector<int> lastWrite(nBuffers, -1), lastRead(nBuffers, -1), level(n, 0);
    // scale buffers are dependencies too: an operation that divides by the factors of a buffer (SCALE_READ) must run after
    // the operation of this list that writes them, a second writer after the first writer and all its readers
    std::unordered_map<const void*, std::pair<int, int>> scaleLevels;     // scale buffer -> (last write level, last read level)
    int nLevels = 0;
    // The serial kernels (k_partials_mfma_serial / _spine) fetch an operation's operands -- the exponents a SCALE_READ divides by
    // among them -- while the operation before it computes and the writer wave still stores the one before that: partials of
    // the last two results are forwarded through LDS, exponents are not.  A list in which an operation reads the exponents an
    // earlier operation of the list writes (MrBayes never sends one) therefore runs level by level: a launch boundary orders them.
    bool scaleForward = false;
    for (int o = 0; o < n; ++o) {
        int l = 0;
        l = std::max(l, lastWrite[c1Idx[o]] + 1);
        l = std::max(l, lastWrite[c2Idx[o]] + 1);
        l = std::max(l, lastWrite[dstIdx[o]] + 1);
        l = std::max(l, lastRead[dstIdx[o]] + 1);
        if (dev[o].scale_mode != SCALE_NONE) {
            auto it = scaleLevels.find(dev[o].scale);
            if (it != scaleLevels.end()) {
                if (dev[o].scale_mode == SCALE_READ && it->second.first >= 0) scaleForward = true;
                l = std::max(l, it->second.first + 1);
                if (dev[o].scale_mode == SCALE_WRITE) l = std::max(l, it->second.second + 1);
            }
        }
        level[o] = l;
        if (dev[o].scale_mode != SCALE_NONE) {
            auto& sl = scaleLevels.emplace(dev[o].scale, std::make_pair(-1, -1)).first->second;
            if (dev[o].scale_mode == SCALE_WRITE) sl.first = l; else sl.second = std::max(sl.second, l);
        }
        lastWrite[dstIdx[o]] = l;
        lastRead[c1Idx[o]] = std::max(lastRead[c1Idx[o]], l);
        lastRead[c2Idx[o]] = std::max(lastRead[c2Idx[o]], l);
        nLevels = std::max(nLevels, l + 1);
    }
    std::vector<int> start(nLevels + 1, 0);
    for (int o = 0; o < n; ++o) start[level[o] + 1]++;
    for (int l = 0; l < nLevels; ++l) start[l + 1] += start[l];
    std::vector<PartialsOp> sorted(n);
    {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int o = 0; o < n; ++o) sorted[fill[level[o]]++] = dev[o];
    }
    // level 0: operations on two compact tips first (they get their own kernel)
    auto tipPair = [](const PartialsOp& d) { return d.c1_kind == CHILD_STATES && d.c2_kind == CHILD_STATES; };
    plan.tipTip = nLevels > 0 ? (int) (std::stable_partition(sorted.begin(), sorted.begin() + start[1], tipPair) - sorted.begin()) : 0;
    plan.anyScale = false;
    for (const PartialsOp& d : sorted) plan.anyScale |= d.scale_mode != SCALE_NONE;
    plan.start = start;
    plan.narrow = serialRatio > 0 && !scaleForward && n <= serialRatio * nLevels;
    // Independent sub-lists.  A list often is several root-ward paths interleaved (MrBayes puts the operations of all
    // eigen-system parts of a codon model into one list, reference src/mbbeagle.c:1029-1100).  chainsOf() splits a
    // subset of the list (original indices, list order) into connected components of the "touches a buffer a member
    // writes" relation and packs them into at most MBAMD_MAX_TABLES bins; the serial kernel walks the bins side by side.
    auto chainsOf = [&](const std::vector<int>& sub) {
        const int m = (int) sub.size();
        std::vector<int> comp(m);
        for (int x = 0; x < m; ++x) comp[x] = x;
        auto find = [&](int x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
        auto unite = [&](int a, int b) { a = find(a); b = find(b); if (a != b) comp[std::max(a, b)] = std::min(a, b); };
        std::vector<int> owner(nBuffers, -1);                    // a member that writes the buffer
        for (int x = 0; x < m; ++x) {
            const int o = sub[x];
            if (owner[dstIdx[o]] >= 0) unite(x, owner[dstIdx[o]]);
            owner[dstIdx[o]] = x;
        }
        for (int x = 0; x < m; ++x) {
            const int o = sub[x];
            if (owner[c1Idx[o]] >= 0) unite(x, owner[c1Idx[o]]);
            if (owner[c2Idx[o]] >= 0) unite(x, owner[c2Idx[o]]);
        }
        for (int x = 0; x < m; ++x)                              // node scale buffers written by one, used by another
            for (int y = x + 1; y < m; ++y) {
                const PartialsOp &dx = dev[sub[x]], &dy = dev[sub[y]];
                if (dx.scale == dy.scale && dx.scale_mode != SCALE_NONE && dy.scale_mode != SCALE_NONE &&
                    (dx.scale_mode == SCALE_WRITE || dy.scale_mode == SCALE_WRITE))
                    unite(x, y);
            }
        std::vector<int> roots, size(m, 0);
        for (int x = 0; x < m; ++x) { size[find(x)]++; if (find(x) == x) roots.push_back(x); }
        std::sort(roots.begin(), roots.end(), [&](int a, int b) { return size[a] > size[b]; });
        const int nb = std::min<int>(MBAMD_MAX_TABLES, (int) roots.size());
        std::vector<int> binLen(nb, 0), binOf(m, 0);
        for (int r : roots) {                                    // largest first, each into the currently shortest bin
            const int bsel = (int) (std::min_element(binLen.begin(), binLen.end()) - binLen.begin());
            binOf[r] = bsel;
            binLen[bsel] += size[r];
        }
        std::vector<std::vector<int>> bins(nb);
        for (int x = 0; x < m; ++x) bins[binOf[find(x)]].push_back(sub[x]);
        return bins;
    };
    auto appendBins = [&](const std::vector<std::vector<int>>& bins, std::vector<std::pair<int, int>>& out) {
        for (const auto& bin : bins) {
            if (bin.empty()) continue;
            out.emplace_back((int) sorted.size(), (int) bin.size());
            for (int o : bin) sorted.push_back(dev[o]);          // (list order inside a bin = dependency order)
        }
    };
    plan.chains.clear();
    plan.spineChains.clear();
    plan.serialFrom = nLevels;
    if (plan.narrow) {
        std::vector<int> all(n);
        for (int o = 0; o < n; ++o) all[o] = o;
        const auto bins = chainsOf(all);
        if (bins.size() > 1) appendBins(bins, plan.chains);
        else plan.chains.emplace_back(0, n);
    } else if (serialRatio > 0 && !scaleForward) {
        // the tail of a level-launched list: trailing levels of a few operations each.  If they fall apart into parallel
        // chains (three codon parts -> three chains) one serial launch walks them side by side; otherwise only the
        // strictly single-operation levels (the spine towards the root) go serial.
        int from = nLevels;
        while (from > 0 && start[from] - start[from - 1] <= MBAMD_MAX_TABLES) from--;
        if (nLevels - from >= 2) {
            std::vector<int> sub;
            for (int o = 0; o < n; ++o) if (level[o] >= from) sub.push_back(o);
            const auto bins = chainsOf(sub);
            size_t longest = 0;
            for (const auto& bin : bins) longest = std::max(longest, bin.size());
            if (bins.size() >= 2 && 4 * longest <= 5 * (size_t) (nLevels - from)) {
                plan.serialFrom = from;
                appendBins(bins, plan.spineChains);
            }
        }
        if (plan.spineChains.empty()) {
            from = nLevels;
            const int spineWidth = std::max(1, sw.spineWidth.value_or(1));   // trailing levels of at most this many operations join
            while (from > 0 && start[from] - start[from - 1] <= spineWidth) from--;
            if (nLevels - from >= 2) {
                plan.serialFrom = from;
                plan.spineChains.emplace_back(start[from], n - start[from]);
            }
        }
    }
    return planTable(plan, sorted.data(), sorted.size() * sizeof(PartialsOp));
}

inline int Instance::runGeneric(const Plan& plan, int32_t* cum)
{
    const std::vector<int>& start = plan.start;
    const int nLevels = (int) start.size() - 1;
    const bool anyScale = plan.anyScale;
    if (plan.narrow && mfma && !sw.mfmaWhole) {
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int nt = 0;
        for (auto& ch : plan.chains) {
            tabs.ops[nt] = plan.d_table + ch.first;
            tabs.cum[nt] = cum;
            tabs.start[nt] = ch.second;
            ++nt;
        }
        if (launch_mfma_serial(*this, tabs, nt)) {
            timer.count();
            HIP_TRY(hipGetLastError());
            return BEAGLE_SUCCESS;
        }
    }
    int levelEnd = nLevels;
    if (mfma && !sw.mfmaWhole) levelEnd = plan.serialFrom;
    for (int l = 0; l < levelEnd; ++l) {
        int off = start[l];
        int remaining = start[l + 1] - start[l];
        if (l == 0 && mfma && !sw.mfmaWhole && plan.tipTip > 0 && plan.tipTip <= 8192) {
            OpTables tabs;
            std::memset(&tabs, 0, sizeof tabs);
            tabs.ops[0] = plan.d_table;
            tabs.cum[0] = cum;
            for (int t = 1; t <= MBAMD_MAX_TABLES; ++t) tabs.start[t] = 1 << 30;
            if (launch_tips(*this, tabs, plan.tipTip)) {
                timer.count();
                off += plan.tipTip;
                remaining -= plan.tipTip;
            }
        }
        while (remaining > 0) {
            const int count = std::min(remaining, 32768);
            const PartialsOp* ops = plan.d_table + off;
            bool fused = true;
            if (mfma && launch_mfma(*this, ops, std::min(count, 8192), cum)) {
                const int done = std::min(count, 8192);
                timer.count();
                off += done;
                remaining -= done;
                continue;
            }
            if (SP == 20 && K == 4) launch_gen<20, 4>(*this, ops, count, cum);
            else if (SP == 20 && K == 1) launch_gen<20, 1>(*this, ops, count, cum);
            else if (SP == 64 && K == 1) launch_gen<64, 1>(*this, ops, count, cum);
            else if (SP == 4 && K == 4) launch_gen<4, 4>(*this, ops, count, cum);
            else if (SP == 4 && K == 1) launch_gen<4, 1>(*this, ops, count, cum);
            else {
                fused = false;
                switch (SP) {
                    case 4: launch_gen<4, 0>(*this, ops, count, cum); break;
                    case 8: launch_gen<8, 0>(*this, ops, count, cum); break;
                    case 16: launch_gen<16, 0>(*this, ops, count, cum); break;
                    case 20: launch_gen<20, 0>(*this, ops, count, cum); break;
                    case 32: launch_gen<32, 0>(*this, ops, count, cum); break;
                    default: launch_gen<64, 0>(*this, ops, count, cum); break;
                }
            }
            timer.count();
            if (!fused && anyScale) {
                MBAMD_LAUNCH(k_rescale_gen, dim3(Ppad / 64, count), 64, 0, stream, ops, S, K, Ppad, cum);
                timer.count();
            }
            off += count;
            remaining -= count;
        }
    }
    if (levelEnd < nLevels) {                    // the spine: one launch walks it
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int nt = 0;
        for (auto& ch : plan.spineChains) {
            tabs.ops[nt] = plan.d_table + ch.first;
            tabs.cum[nt] = cum;
            tabs.start[nt] = ch.second;
            ++nt;
        }
        if (!launch_mfma_serial(*this, tabs, nt)) return fail(BEAGLE_ERROR_GENERAL, "no serial MFMA kernel for this shape");
        timer.count();
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// The merged-launch half of flushPending: `work`, two or more deferred lists of a shape the split kernels serve
// (mfma_shape_compiled), mutually independent, run together -- one launch per dependency level over all of them.
inline int Instance::flushMerged(std::vector<std::pair<Plan*, int>>& work)
{
    hipEvent_t ev0{}, ev1{};
    { int brc = timer.launchesBegin(ev0, ev1); if (brc) return brc; }
    size_t maxLevels = 0;
    bool allNarrow = true;
    for (auto& w : work) {
        maxLevels = std::max(maxLevels, w.first->start.size() - 1);
        allNarrow = allNarrow && w.first->narrow;
    }
    if (allNarrow) {                             // every list is a set of root-ward paths: one launch walks them all
        size_t nchains = 0;
        for (auto& w : work) nchains += w.first->chains.size();
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int t = 0;
        for (auto& w : work) {
            if (nchains <= MBAMD_MAX_TABLES) {
                for (auto& ch : w.first->chains) {
                    tabs.ops[t] = w.first->d_table + ch.first;
                    tabs.cum[t] = cumulativeOf(w.second);
                    tabs.start[t] = ch.second;
                    ++t;
                }
            } else {                             // too many sub-lists: each list in its own order
                tabs.ops[t] = w.first->d_table;
                tabs.cum[t] = cumulativeOf(w.second);
                tabs.start[t] = w.first->start.back();
                ++t;
            }
        }
        if (launch_mfma_serial(*this, tabs, t)) {
            timer.count();
            maxLevels = 0;
        }
    }
    // levels every list runs as level launches; from spineFrom on each list is a spine of single operations
    size_t spineFrom = 0;
    for (auto& w : work) spineFrom = std::max(spineFrom, (size_t) w.first->serialFrom);
    if (maxLevels > 0) {
        int spineOps = 0;
        for (auto& w : work) spineOps += std::max(0, w.first->start.back() - w.first->start[std::min(spineFrom, w.first->start.size() - 1)]);
        if (spineOps < 2) spineFrom = maxLevels;
    }
    for (size_t l = 0; l < std::min(maxLevels, spineFrom); ++l) {
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int t = 0, total = 0;
        bool tipsDone = false;
        if (l == 0) {                            // operations on two compact tips: their own kernel
            for (auto& w : work) {
                if (w.first->tipTip == 0) continue;
                tabs.ops[t] = w.first->d_table;
                tabs.cum[t] = cumulativeOf(w.second);
                tabs.start[t] = total;
                total += w.first->tipTip;
                ++t;
            }
            for (int u = t; u <= MBAMD_MAX_TABLES; ++u) tabs.start[u] = 1 << 30;
            if (total > 0 && launch_tips(*this, tabs, total)) {
                timer.count();
                tipsDone = true;
            }
            std::memset(&tabs, 0, sizeof tabs);
            t = 0;
            total = 0;
        }
        for (auto& w : work) {
            const std::vector<int>& st = w.first->start;
            if (l + 1 >= st.size() || st[l + 1] == st[l]) continue;
            const int skip = (l == 0 && tipsDone) ? w.first->tipTip : 0;
            if (st[l + 1] - st[l] - skip == 0) continue;
            tabs.ops[t] = w.first->d_table + st[l] + skip;
            tabs.cum[t] = cumulativeOf(w.second);
            tabs.start[t] = total;
            total += st[l + 1] - st[l] - skip;
            ++t;
        }
        for (int u = t; u <= MBAMD_MAX_TABLES; ++u) tabs.start[u] = 1 << 30;
        if (total == 0) continue;
        if (!launch_mfma_split(*this, tabs, total)) return fail(BEAGLE_ERROR_GENERAL, "no MFMA kernel for a deferred list");
        timer.count();
    }
    if (spineFrom < maxLevels) {
        OpTables tabs;
        std::memset(&tabs, 0, sizeof tabs);
        int t = 0;
        for (auto& w : work) {
            const std::vector<int>& st = w.first->start;
            if (spineFrom + 1 >= st.size()) continue;
            tabs.ops[t] = w.first->d_table + st[spineFrom];
            tabs.cum[t] = cumulativeOf(w.second);
            tabs.start[t] = st.back() - st[spineFrom];
            ++t;
        }
        if (t > 0) {
            if (!launch_mfma_serial(*this, tabs, t)) return fail(BEAGLE_ERROR_GENERAL, "no serial MFMA kernel for a deferred list");
            timer.count();
        }
    }
    HIP_TRY(hipGetLastError());
    return timer.launchesEnd(ev0, ev1);
}

// the level kernels' integration (arguments checked by integrate)
inline int Instance::integrateLevels(const int* parent, const int* child, const int* prob, const int* wIdx, const int* fIdx,
                              const int* cumIdx, int count)
{
    IntegrateArgs a;
    { int rc = integrateOperands(a, parent, child, prob, wIdx, fIdx, cumIdx, count); if (rc) return rc; }
    double* const siteOut = siteTarget();
    if (S >= 8) MBAMD_LAUNCH_BARRIER(k_integrate_lnl_wide, (unsigned) nblocks, 256, 0, stream, a, S, SP, K, P, Ppad, (const double*) d_pweights, siteOut, h_sums_dev);
    else
        MBAMD_LAUNCH(k_integrate_lnl, (unsigned) nblocks, 64, 0, stream, a, S, SP, K, P, Ppad, (const double*) d_pweights, siteOut, h_sums_dev);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

}  // namespace mbamd

#endif  // MBAMD_F32_LEVELS_H_
