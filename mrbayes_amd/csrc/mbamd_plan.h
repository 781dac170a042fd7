// mbamd_plan.h -- the plain data the single-precision engine's schedulers hand to one another: `Plan`, a compiled operation list as the
// plan cache holds it; `Walk4Recipe`, how an unstored result of the 4-state walk is made again; `PathStep`, one operation of a
// root-ward path.  No engine state: the owner of the unstored subtrees (mbamd_walk4_unstored.h) reads a Plan without seeing the engine.
#ifndef MBAMD_PLAN_H_
#define MBAMD_PLAN_H_

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "mbamd_kernels.h"       // PartialsOp; Walk4Entry and MBAMD_W4_UNSTORED_TIPS_MAX (mbamd_walk4.h)

namespace mbamd {

// 4-state walk: how an unstored result is made again from compact tips alone (Walk4Unstored::ensureStored) -- the one to three operations of
// its subtree in post-order, the last one its own.  A child is a compact tip (its buffer index) or, `in` set, the result of an earlier
// operation of the same recipe (that operation's number): no buffer of an inner node is named.  Matrices, in the buffer's slot of the
// snapshot table: places 0 and 1 for its own operation (as a tip pair's), 2 + 2 j and 3 + 2 j for inner operation j (k_walk4_snapshot).
// (MBAMD_W4_UNSTORED_TIPS_MAX and MBAMD_W4_SNAP, the matrices of a slot: mbamd_walk4.h, beside k_walk4_snapshot)
#define MBAMD_W4_UNSTORED_TIPS_DEFAULT 4
struct Walk4Recipe {
    int nops = 0;
    struct Op { int c1, c2, mode; bool in1, in2; } op[MBAMD_W4_UNSTORED_TIPS_MAX - 1];
    bool usesTip(int tip) const
    {
        for (int j = 0; j < nops; ++j) if ((!op[j].in1 && op[j].c1 == tip) || (!op[j].in2 && op[j].c2 == tip)) return true;
        return false;
    }
};

// A compiled operation list: the device-resident table a partials kernel walks, cached under the exact
// BeagleOperation array it was built from.  MrBayes re-issues the same lists all the time (every move
// that dirties the whole tree alternates between the two buffer-flip states), so the host-side
// scheduling and the table upload happen once per distinct list, not once per generation.
struct Plan {
    std::vector<int> key;            // the BeagleOperation ints + cumulative index + layout epoch
    uint64_t hash = 0, lastUse = 0;
    uint64_t lastLaunch = 0;         // Instance::launchClock value of the latest launch that reads d_table
    PartialsOp* d_table = nullptr;
    size_t cap = 0;                  // bytes allocated for d_table
    struct Segment {                             // tree-walk path: one launch per hazard-free segment
        size_t first; int W, entries, nslots, tail = 2;
        bool plain = false, peel = false;        // 4-state walk: nothing rare in it (Walk4Template::plain / peel) -- k_walk4_t<Walk4Args, true>
        bool waves = false;                      // ... cut over W > 1 waves (Walk4Template::waves) -- k_walk4_t<Walk4Args, true, true>; nslots: of the workgroup
    };
    std::vector<Segment> segments;               // (Walk4Entry index of its program in d_table, geometry)
    std::vector<Walk4Entry> inlineProg;          // 4-state walk: a short single-segment program travels in the kernel arguments instead
    // 4-state walk: the SMALL SUBTREES (compact tips and operations of the list alone, at most MBAMD_UNSTORED_TIPS tips: tip pairs, and
    // subtrees of three and four tips) of a list that is ONE plain segment in a device buffer -- their entries carry MBAMD_W4_NOSTORE,
    // their destinations are left unstored with a recipe (Walk4Unstored::launched); empty for every other plan.  `inner`: the program
    // entries of the recipe's inner operations, which k_walk4_snapshot copies the matrices of (the side table behind the program)
    struct Unstored { int entry, dst; Walk4Recipe r; int inner[MBAMD_W4_UNSTORED_TIPS_MAX - 2]; };
    std::vector<Unstored> unstoredSubtrees;
    size_t sideFirst = 0; int sideCount = 0;     // the side table: Walk4Entry index in d_table, records (one per subtree of more than two tips)
    bool path = false;                           // 4-state walk: the list is a root-ward path -- inlineProg holds k_path4's entries
    bool forked = false;                         // ... of several arms that join (the list of a topology move)
    bool pathG = false;                          // 20/61-state walk: every list is a root-ward path of the same length -- inlineProg holds k_pathg's entries
    int lists = 1;                               // 20/61-state walk: > 1 = the segments are that many independent lists, ONE launch
    std::vector<int> start;                      // general path: first table entry of each dependency level
    bool anyScale = false;
    bool narrow = false;                         // general path: few operations per level -> one serial launch
    std::vector<std::pair<int, int>> chains;     // narrow general-state lists: (first table entry, operations) of up to four
                                                 // mutually independent sub-lists (they walk in parallel workgroups)
    std::vector<std::pair<int, int>> spineChains;   // the same for the serial tail of a level-launched list (levels >= serialFrom)
    int tipTip = 0;                              // general path: the first tipTip operations of level 0 have two compact tip children
    int serialFrom = 0;                          // general path: levels >= serialFrom are narrow (the spine towards the
                                                 // root): they run as one serial launch after the level launches
    std::vector<int> bufsRead, bufsWritten, scalesUsed;   // buffer / scale indices the list touches (deferral hazards)
};

// One operation of a root-ward path as Instance::recognisePath sees it, in buffer / matrix / scale INDICES: the path kernels'
// entries are filled from it in their own units (Instance::pathEntry).
struct PathStep {
    bool start, join;                // begins an arm (both children come from outside) / its other child is the saved result of the arm before
    bool chainTip, sibTip;           // the child is a compact tip
    int arm;                         // start: the number of operations of the arm it begins
    int dst, chain, sib;             // partials buffers: result; the child on the path (an operand only where an arm starts); the other child
    int mchain, msib;                // their transition matrices
    int scaleMode, scaleIdx;         // SCALE_NONE / SCALE_WRITE / SCALE_READ and its exponent buffer
};

}  // namespace mbamd

#endif  // MBAMD_PLAN_H_
