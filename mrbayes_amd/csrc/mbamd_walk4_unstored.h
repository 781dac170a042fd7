// mbamd_walk4_unstored.h -- the small subtrees a whole-tree launch of the plain 4-state walk did not store (MBAMD_W4_NOSTORE,
// mbamd_walk4.h): `Walk4Unstored` knows which partials buffers hold a recipe instead of values, owns the matrix snapshots the recipes
// read and the programs that make such buffers again.  The engine reports what its launches left unstored and what is about to be read
// or overwritten, and never sees a recipe.
// Such a buffer stays valid for the engine: it carries a RECIPE -- its compact tips, its one to three operations with their scale modes
// (Walk4Recipe: a closure, no inner buffer is named) -- and its slot (its own index) in a device table of MATRIX SNAPSHOTS
// float [buffer][MBAMD_W4_SNAP][K][16], copied by k_walk4_snapshot behind the integration launch (off the critical path) or, at the
// latest, before anything overwrites a matrix or reads a recipe (flushSnapshot) -- so a recipe never depends on a matrix buffer the client
// may overwrite.  Every reader of partials calls ensureStored first: the unstored buffers among those it names are recomputed into
// their arena slices by ONE launch of the generic k_walk4_t (same source, same bits; exponent bytes go to the scratch rows, the real scale
// buffers were written by the original launch).  A subtree of three or four tips runs its two or three operations on the plain
// instantiation instead, the inner ones with MBAMD_W4_NOSTORE: only the named buffer is written.  Any write to a buffer drops its recipe
// (forget); overwriting a tip materialises the recipes that use it first (tipChanging).
// Per call the engine hands over `base`, its side of a 4-state kernel's arguments (arenas, strides, the matrices a snapshot copies),
// and `scratchRow`, the first exponent row behind the scale buffers.
#ifndef MBAMD_WALK4_UNSTORED_H_
#define MBAMD_WALK4_UNSTORED_H_

#include <functional>
#include <optional>

#include "mbamd_host.h"          // the HIP runtime, HIP_TRY, grow_device
#include "mbamd_kernels.h"       // k_walk4_t, k_walk4_snapshot, Walk4Args, Walk4Entry and its codes (mbamd_walk4.h)
#include "mbamd_plan.h"          // Plan, Walk4Recipe

namespace mbamd {

struct Walk4Unstored {
    typedef std::function<int(void* dst, const void* src, size_t bytes)> Upload;     // the engine's small asynchronous copy to the device
    Walk4Unstored() = default;
    Walk4Unstored(const Walk4Unstored&) = delete; Walk4Unstored& operator=(const Walk4Unstored&) = delete;
    ~Walk4Unstored()
    {
        if (d_snap) (void) hipFree(d_snap);
        if (d_storeProg) (void) hipFree(d_storeProg);
    }
    // launchClock_: the engine's count of launches, which every launch here advances; tips: MBAMD_UNSTORED_TIPS
    void create(hipStream_t stream_, int nBuffers_, int K_, int Ppad_, uint64_t* launchClock_, Upload upload_, std::optional<int> tips)
    {
        stream = stream_; nBuffers = nBuffers_; K = K_; Ppad = Ppad_; launchClock = launchClock_; upload = std::move(upload_);
        tipsMax = std::max(2, std::min(MBAMD_W4_UNSTORED_TIPS_MAX, tips.value_or(MBAMD_W4_UNSTORED_TIPS_DEFAULT)));
        unstored.assign((size_t) nBuffers, 0);
        recipes.assign((size_t) nBuffers, Walk4Recipe());
    }
    bool any() const { return nUnstored != 0; }                    // every hook of the engine is one comparison while nothing is
    bool holds(int b) const { return nUnstored && b >= 0 && b < nBuffers && unstored[(size_t) b]; }
    void forget(int b) { if (nUnstored && unstored[(size_t) b]) { unstored[(size_t) b] = 0; --nUnstored; } }     // b is being overwritten
    int maxTips() const { return tipsMax; }                        // the largest subtree a list may leave unstored
    bool snapshotWaiting() const { return snapPlan != nullptr; }   // the matrices of the latest such launch are still to be copied
    // tip-pair buffers launches left unstored / buffers materialised since / launches that materialised them (mbamdGetRecomputeCounts);
    // the same for the subtrees of three and four tips (mbamdGetSubtreeRecomputeCounts): added to out3
    void pairCounts(long out3[3]) const { out3[0] += leftUnstored; out3[1] += materialised; out3[2] += materialiseLaunches; }
    void subtreeCounts(long out3[3]) const { out3[0] += leftUnstoredSub; out3[1] += materialisedSub; out3[2] += materialiseLaunchesSub; }

    // behind a launch of the plain kernel whose program carries MBAMD_W4_NOSTORE entries: their destinations hold recipes from now on
    int launched(const Plan& plan, const Walk4Args& base)
    {
        if (!d_snap) HIP_TRY(hipMalloc(&d_snap, (size_t) nBuffers * MBAMD_W4_SNAP * K * 16 * sizeof(float)));
        if (snapPlan && snapPlan != &plan) { int rc = flushSnapshot(base); if (rc) return rc; }     // (the matrices are what they were at that launch: nothing overwrote one since)
        for (const Plan::Unstored& u : plan.unstoredSubtrees) {
            if (!unstored[(size_t) u.dst]) ++nUnstored;
            unstored[(size_t) u.dst] = 1;
            recipes[(size_t) u.dst] = u.r;
            ++(u.r.nops > 1 ? leftUnstoredSub : leftUnstored);
        }
        snapPlan = const_cast<Plan*>(&plan);
        return BEAGLE_SUCCESS;
    }

    // the waiting copy of the matrices of a launch's unstored subtrees into the snapshot table, now (k_walk4_snapshot reads the plan's own
    // program): before a matrix changes, before the plan may be recompiled, and behind the integration that followed the launch
    int flushSnapshot(const Walk4Args& base)
    {
        Plan* const plan = snapPlan;
        snapPlan = nullptr;
        if (!plan || plan->segments.size() != 1 || !plan->d_table) return BEAGLE_SUCCESS;
        const Plan::Segment& sg = plan->segments[0];
        plan->lastLaunch = ++*launchClock;           // (the program must stay what it is until this launch has run: the engine re-uploads a table only behind lastLaunch)
        const unsigned nprog = sg.waves ? (unsigned) (sg.W * sg.entries) : (unsigned) (sg.entries - sg.tail);   // (several waves: [W][entries], the padding carries no flag)
        MBAMD_LAUNCH(k_walk4_snapshot, nprog + (unsigned) plan->sideCount, 64, 0, stream, reinterpret_cast<const Walk4Entry*>(plan->d_table) + sg.first,
                     nprog, reinterpret_cast<const Walk4Entry*>(plan->d_table) + plan->sideFirst, (unsigned) ((size_t) (Ppad / 64) * K), (const float*) base.matrices, d_snap, K);
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }

    // Every reader of partials, before its launch: the unstored buffers among `bufs` (indices out of range, tips and stored buffers are
    // passed over) are recomputed into the arena by one launch of the generic k_walk4_t -- entries with both children tips, matrices from
    // the snapshot table, no cumulative buffer, the exponent byte to the scratch rows -- and drop their recipes.  With a subtree of three or
    // four tips among them the one launch is of the plain instantiation, through a device buffer (subtreeProgram).
    int ensureStored(const int* bufs, int n, const Walk4Args& base, int scratchRow)
    {
        if (nUnstored == 0) return BEAGLE_SUCCESS;
        std::vector<int>& list = storeList;
        list.clear();
        for (int i = 0; i < n; ++i) {
            const int b = bufs[i];
            if (b < 0 || b >= nBuffers || unstored[(size_t) b] != 1) continue;
            unstored[(size_t) b] = 2;                // (named twice: listed once)
            list.push_back(b);
        }
        for (int b : list) unstored[(size_t) b] = 1;
        if (list.empty()) return BEAGLE_SUCCESS;
        int rc = flushSnapshot(base);
        if (rc) return rc;
        bool plain = false;
        for (int b : list) plain = plain || recipes[(size_t) b].nops > 1;
        return plain ? subtreeProgram(base, scratchRow) : pairProgram(base, scratchRow);
    }

    // a compact tip is about to change (new states, or partials in its place): the unstored buffers made from it are stored first;
    // whatever the tip's own buffer held is gone
    int tipChanging(int tip, const Walk4Args& base, int scratchRow)
    {
        if (nUnstored == 0) return BEAGLE_SUCCESS;
        std::vector<int> users;
        for (int b = 0; b < nBuffers; ++b)
            if (unstored[(size_t) b] && recipes[(size_t) b].usesTip(tip)) users.push_back(b);
        const int rc = users.empty() ? BEAGLE_SUCCESS : ensureStored(users.data(), (int) users.size(), base, scratchRow);
        if (rc) return rc;
        forget(tip);
        return BEAGLE_SUCCESS;
    }

private:
    hipStream_t stream{};
    int nBuffers = 0, K = 0, Ppad = 0, tipsMax = 2;
    uint64_t* launchClock = nullptr;
    Upload upload;
    std::vector<char> unstored;      // per partials buffer: 1 = valid, not in the arena, recipes[idx] says how to make it
    std::vector<Walk4Recipe> recipes;
    int nUnstored = 0;
    float* d_snap = nullptr;         // the matrix snapshots, allocated with the first unstored buffer
    Plan* snapPlan = nullptr;        // the plan whose tip-pair matrices are still to be copied there
    void* d_storeProg = nullptr;     size_t storeProgCap = 0;       // a materialising program too long for the kernel arguments
    std::vector<int> storeList;      // scratch: the buffers ensureStored is making
    std::vector<Walk4Entry> storeProg;
    long leftUnstored = 0, materialised = 0, materialiseLaunches = 0;                 // tip pairs
    long leftUnstoredSub = 0, materialisedSub = 0, materialiseLaunchesSub = 0;        // subtrees of three and four tips

    // storeList holds tip pairs alone: the generic kernel, every entry on two tips
    int pairProgram(const Walk4Args& base, int scratchRow)
    {
        const std::vector<int>& list = storeList;
        const int m = (int) list.size(), entries = (m + 1) / 2 * 2 + 2;              // the kernel's loop runs two entries a turn and reads two ahead
        const uint32_t pbuf = (uint32_t) ((size_t) (Ppad / 64) * K), ebuf = (uint32_t) K * 64u, mbuf = (uint32_t) K * 64u;
        const uint32_t scratch = (uint32_t) scratchRow;
        storeProg.resize((size_t) entries);
        for (int i = 0; i < entries; ++i) {
            Walk4Entry& e = storeProg[(size_t) i];
            std::memset(&e, 0, sizeof e);
            e.ctl = MBAMD_W4_NOP;
            e.ewrite = (scratch + (uint32_t) (i % MBAMD_W4_SCRATCH_ROWS)) * ebuf;
            e.eread = scratch * ebuf;
            if (i >= m) continue;
            const uint32_t b = (uint32_t) list[(size_t) i];
            const Walk4Recipe& r = recipes[b];
            e.ctl = MBAMD_W4_TIP1 | MBAMD_W4_TIP2 | ((uint32_t) r.op[0].mode << 8);
            e.dst = b * pbuf;
            e.c1 = (uint32_t) r.op[0].c1 * 32u;
            e.c2 = (uint32_t) r.op[0].c2 * 32u;
            e.m1 = ((uint32_t) MBAMD_W4_SNAP * b) * mbuf;
            e.m2 = ((uint32_t) MBAMD_W4_SNAP * b + 1u) * mbuf;
        }
        return runProgram(base, entries, 2, false, m, 0);
    }

    // storeList (every buffer in it unstored, the matrices snapshot) holds a subtree of three or four tips: ONE launch of the plain
    // instantiation k_walk4_t<Walk4Args, true> -- the kernel and the entry kinds of the original launch: the same bits -- over the recipes'
    // operations in post-order.  An inner operation carries MBAMD_W4_NOSTORE: its result reaches its parent through the forwarding
    // registers or LDS slot 0 (the first tip pair of a balanced four) and lands nowhere else -- the arena slice of the inner buffer may
    // hold something else by now.  Matrices from the buffer's snapshot slots, exponent bytes to the scratch rows, no cumulative buffer.
    int subtreeProgram(const Walk4Args& base, int scratchRow)
    {
        const std::vector<int>& list = storeList;
        const uint32_t pbuf = (uint32_t) ((size_t) (Ppad / 64) * K), ebuf = (uint32_t) K * 64u, mbuf = (uint32_t) K * 64u;
        const uint32_t scratch = (uint32_t) scratchRow;
        storeProg.clear();
        int pairs = 0, subtrees = 0;
        for (int b : list) {
            const Walk4Recipe& r = recipes[(size_t) b];
            ++(r.nops > 1 ? subtrees : pairs);
            for (int j = 0; j < r.nops; ++j) {
                const Walk4Recipe::Op& o = r.op[j];
                Walk4Entry e;
                std::memset(&e, 0, sizeof e);
                const bool last = j == r.nops - 1;
                // matrices: the buffer's own operation in snapshot slots 0 and 1, inner operation j in 2 + 2 j and 3 + 2 j
                const uint32_t mslot = (uint32_t) MBAMD_W4_SNAP * (uint32_t) b + (last ? 0u : 2u + 2u * (uint32_t) j);
                uint32_t flags = 0;
                // a child made by the operation in front is forwarded; one made two in front (the first tip pair of a balanced four) waits in slot 0
                if (!o.in1) { flags |= MBAMD_W4_TIP1; e.c1 = (uint32_t) o.c1 * 32u; }
                else if (o.c1 == j - 1) flags |= MBAMD_W4_FWD1;
                if (!o.in2) { flags |= MBAMD_W4_TIP2; e.c2 = (uint32_t) o.c2 * 32u; }
                else if (o.c2 == j - 1) flags |= MBAMD_W4_FWD2;
                for (int q = j + 2; q < r.nops; ++q)
                    if ((r.op[q].in1 && r.op[q].c1 == j) || (r.op[q].in2 && r.op[q].c2 == j)) flags |= MBAMD_W4_KEEP;   // (slot 0: [23:16] stays zero)
                e.ctl = flags | ((uint32_t) o.mode << 8) | walk4_kind_of(flags) | (last ? 0u : MBAMD_W4_NOSTORE);
                e.dst = last ? (uint32_t) b * pbuf : 0u;
                e.m1 = mslot * mbuf;
                e.m2 = (mslot + 1u) * mbuf;
                e.ewrite = (scratch + (uint32_t) (storeProg.size() % MBAMD_W4_SCRATCH_ROWS)) * ebuf;
                e.eread = (flags & MBAMD_W4_TIP1) ? e.c1 : 0u;                   // (a plain program: child 1's plane offset or 0, as the list compiler fills it)
                storeProg.push_back(e);
            }
        }
        const int nops = (int) storeProg.size(), entries = (nops + 1) / 2 * 2 + 2;   // the read-ahead tail: valid offsets, nothing executed
        for (int i = nops; i < entries; ++i) {
            Walk4Entry e;
            std::memset(&e, 0, sizeof e);
            e.ctl = MBAMD_W4_NOP;
            e.ewrite = (scratch + (uint32_t) (i % MBAMD_W4_SCRATCH_ROWS)) * ebuf;
            storeProg.push_back(e);
        }
        return runProgram(base, entries, entries - nops, true, pairs, subtrees);
    }

    // storeProg, one wave and one LDS slot per workgroup, makes the buffers of storeList: matrices from the snapshots, no cumulative buffer.
    // A generic program short enough travels in the kernel arguments; a plain one has no such form and goes through d_storeProg, however
    // short.  Then the buffers are stored, and counted (launches: one for the tip pairs if there were any, one for the subtrees likewise).
    int runProgram(const Walk4Args& base, int entries, int tail, bool plain, int pairs, int subtrees)
    {
        Walk4ArgsInline ai;
        Walk4Args& a = ai.a;
        a = base;
        a.matrices = d_snap;
        a.cum = nullptr;
        a.cumFresh = 0;
        a.entries = entries;
        a.nslots = 1;
        a.tail = tail;
        ++*launchClock;
        if (!plain && entries <= MBAMD_W4_INLINE) {
            std::memcpy(ai.inl, storeProg.data(), (size_t) entries * sizeof(Walk4Entry));
            auto kernel = k_walk4_t<Walk4ArgsInline>;
            MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, 1), stream, ai);
        } else {
            const size_t bytes = (size_t) entries * sizeof(Walk4Entry);
            int rc = grow_device(stream, &d_storeProg, &storeProgCap, bytes, std::max(bytes, storeProgCap * 2));
            if (rc) return rc;
            rc = upload(d_storeProg, storeProg.data(), bytes);
            if (rc) return rc;
            a.prog = static_cast<const Walk4Entry*>(d_storeProg);
            if (plain) {
                auto kernel = k_walk4_t<Walk4Args, true>;
                MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, 1), stream, a);
            } else {
                auto kernel = k_walk4_t<Walk4Args>;
                MBAMD_LAUNCH_BARRIER(kernel, walk4_grid(Ppad / 64, K), 64, walk4_lds_bytes(1, 1), stream, a);
            }
        }
        HIP_TRY(hipGetLastError());
        for (int b : storeList) unstored[(size_t) b] = 0;
        nUnstored -= (int) storeList.size();
        materialised += pairs;
        materialiseLaunches += pairs ? 1 : 0;
        materialisedSub += subtrees;
        materialiseLaunchesSub += subtrees ? 1 : 0;
        return BEAGLE_SUCCESS;
    }
};

}  // namespace mbamd

#endif  // MBAMD_WALK4_UNSTORED_H_
