// mbamd_f32_walk.h -- the single-precision engine (mbamd_f32.h): the front of the program compiler that both tree walks use.
// Defines Instance::buildWalk (an operation list -> hazard-free segments -> per-wave programs of k_walk4_t / k_walkg), and the
// root-ward paths of the path kernels: recognisePath, pathEntry, pathPlan.
#ifndef MBAMD_F32_WALK_H_
#define MBAMD_F32_WALK_H_

#include "mbamd_f32.h"           // Instance

namespace mbamd {

// Compile one operation list: validate, cut into hazard-free segments, build (or re-use) the structural template of
// each segment and fill it with this list's buffer / matrix / scale indices.
inline int Instance::buildWalk(Plan& plan, const BeagleOperation* ops, int n, const int* listOf, bool perList)
{
    const int scratchScale = (int) scales.count();              // sink / source of entries that do not rescale
    std::vector<int>& segList = w4segList;                     // (20/61-state walk) merged-list index of each operation of the segment
    segList.clear();
    std::vector<char>& written = w4written;
    written.assign((size_t) nBuffers, 0);
    w4table.clear();
    plan.segments.clear();
    plan.unstoredSubtrees.clear();
    std::vector<Walk4Op>& seg = w4ops;
    seg.clear();
    // segment state: buffers / exponent buffers the current segment has read or written
    std::vector<char>&segRead = w4segRead, &segWritten = w4segWritten, &segScale = w4segScale;
    segRead.assign((size_t) nBuffers, 0); segWritten.assign((size_t) nBuffers, 0); segScale.assign(scales.count() + 1, 0);
    if (w4writer.size() < (size_t) nBuffers) w4writer.assign((size_t) nBuffers, -1);
    int reloads = 0, externals = 0, phases = 0;
    auto flushSegment = [&]() -> int {
        if (seg.empty()) return BEAGLE_SUCCESS;
        // structural key
        std::vector<int>& key = w4key;
        key.clear();
        key.reserve(seg.size() * 3 + 4);
        key.push_back((int) seg.size()); key.push_back(w4.maxW); key.push_back(w4.maxSlots + 256 * w4.maxSlots1);
        key.push_back(w4.prefetchDistance * 2 + (w4.safeWaits ? 1 : 0));
        key.push_back(w4.plainWaves + 16 * w4.plainSlots); key.push_back(w4.plainMinOps + 64 * w4.plainShare[std::max(2, std::min(8, w4.plainWaves))] + (w4.plainDescend ? 1 << 20 : 0));
        {
            std::vector<int>& writer = w4writer;          // buffer -> operation of this segment that writes it (-1 outside this block)
            // (4-state walk) per operation: the tips of its subtree if that is compact tips and operations of this segment alone and has at
            // most MBAMD_W4_UNSTORED_TIPS_MAX of them, else 0; and the subtree's operations in list order, its own last
            constexpr int RO = MBAMD_W4_UNSTORED_TIPS_MAX - 1;
            w4subTips.assign(wg ? 0 : seg.size(), 0);
            w4subOps.assign(wg ? 0 : seg.size() * RO, -1);
            for (size_t o = 0; o < seg.size() && !wg; ++o) {
                const Walk4Op& op = seg[o];
                const int w1 = op.tip1 ? -1 : writer[op.c1], w2 = op.tip2 ? -1 : writer[op.c2];
                const int t1 = op.tip1 ? 1 : (w1 >= 0 ? w4subTips[(size_t) w1] : 0), t2 = op.tip2 ? 1 : (w2 >= 0 ? w4subTips[(size_t) w2] : 0);
                if (t1 && t2 && t1 + t2 <= MBAMD_W4_UNSTORED_TIPS_MAX && (op.tip1 || op.tip2 || op.c1 != op.c2)) {
                    w4subTips[o] = t1 + t2;
                    int below = 0, *mine = &w4subOps[o * RO];
                    for (const int w : {std::min(w1, w2), std::max(w1, w2)})          // (two inner children: two tip pairs, list order)
                        for (int j = 0; w >= 0 && j < RO && w4subOps[(size_t) w * RO + j] >= 0; ++j) mine[below++] = w4subOps[(size_t) w * RO + j];
                    mine[below] = (int) o;
                }
                writer[op.dst] = (int) o;
            }
            for (size_t o = 0; o < seg.size() && !wg; ++o) writer[seg[o].dst] = -1;
            for (size_t o = 0; o < seg.size(); ++o) {
                key.push_back(seg[o].tip1 ? -1 : writer[seg[o].c1]);
                key.push_back(seg[o].tip2 ? -1 : writer[seg[o].c2]);
                key.push_back((int) seg[o].tip1 | ((int) seg[o].tip2 << 1) | ((!seg[o].tip1 && !seg[o].tip2 && seg[o].c1 == seg[o].c2) ? 4 : 0) |
                              ((seg[o].scaleWrite < 0 && seg[o].scaleRead >= 0) ? 8 : 0));   // (SCALE_READ entries wait for an exponent DMA)
                writer[seg[o].dst] = (int) o;
            }
            for (size_t o = 0; o < seg.size(); ++o) writer[seg[o].dst] = -1;
        }
        const uint64_t kh = fnv1a(key.data(), key.size());
        auto it = w4templates.find(kh);
        if (it == w4templates.end() || it->second.key != key) {
            scheduleMisses++;
            if (w4templates.size() >= 8192) w4templates.clear();
            Walk4Template& t = w4templates[kh];
            bool ok = w4.build(seg, t);
            if (!ok) {                           // out of slots with look-ahead prefetches: retry without, then on one wave
                Walk4Builder plain = w4;
                plain.prefetchDistance = 0;
                ok = plain.build(seg, t);
                if (!ok) { plain.maxW = 1; ok = plain.build(seg, t); }
            }
            if (!ok) { w4templates.erase(kh); return fail(BEAGLE_ERROR_GENERAL, "tree-walk scheduler: cannot place this list"); }
            t.key = key;
            it = w4templates.find(kh);
        } else {
            scheduleHits++;
        }
        const Walk4Template& t = it->second;
        reloads += t.reloads; externals += t.externals; phases = std::max(phases, t.phases);
        Plan::Segment sg;
        sg.first = w4table.size();
        sg.W = t.W; sg.entries = t.entries; sg.nslots = t.nslots; sg.tail = t.tail;
        sg.plain = t.plain && !wg; sg.peel = t.peel; sg.waves = sg.plain && t.waves;
        plan.segments.push_back(sg);
        w4table.resize(sg.first + t.prog.size());
        // bytes per buffer inside a block / tile, bytes per LDS slot
        const uint32_t slotb = wg ? wg_block_bytes(S) : 1024u;
        // a partials buffer inside a tile (20/61-state walk: bytes) / in the buffer-major 4-state arena (KiB: P_pad/64 x K of them)
        const uint32_t pbuf = wg ? (uint32_t) K * slotb : (uint32_t) ((size_t) (Ppad / 64) * K);
        const uint32_t ebuf = (uint32_t) K * 64u, mbuf = wg ? (uint32_t) (matrixFloats * 4) : (uint32_t) K * 64u;
        int prevKept = -1;                           // (20/61-state walk) slot the previous operation of the same program kept its result in
        w4entryOf.assign(seg.size(), -1);            // (4-state walk) operation -> its entry, for the recipes of a plain program (entries are filled wave by wave: a subtree with an inner operation on a LATER wave than its own finds -1 there and is stored, `placed` below)
        for (size_t i = 0; i < t.prog.size(); ++i) {
            const Walk4Template::Entry& te = t.prog[i];
            Walk4Entry& e = w4table[sg.first + i];
            std::memset(&e, 0, sizeof e);
            if (i % (size_t) t.entries == 0) prevKept = -1;
            uint32_t flags = te.flags, mode = SCALE_NONE, keep = 0;
            e.ewrite = (uint32_t) scratchScale * ebuf;
            e.eread = (uint32_t) scratchScale * ebuf;
            e.ewrite = (uint32_t) (scratchScale + (int) (i % (size_t) (wg ? MBAMD_WG_SCRATCH_ROWS : MBAMD_W4_SCRATCH_ROWS))) * ebuf;   // (neighbouring entries: different scratch rows)
            if (wg) {
                // k_walkg (mbamd_walkg.h): no prefetch entries; a child that is neither a tip nor in a slot is read from
                // HBM by the operand pipeline; NOP entries store zeros to the extra buffer of the tile
                e.dst = (uint32_t) nBuffers * pbuf;
                if (te.op >= 0) {
                    const Walk4Op& op = seg[te.op];
                    e.dst = (uint32_t) op.dst * pbuf;
                    if (op.tip1) { e.c1 = (uint32_t) op.c1 * (uint32_t) MBAMD_WG_TW; flags |= MBAMD_W4_TIP1; }
                    else if (te.c1slot == 0xFF) { e.c1 = (uint32_t) op.c1 * pbuf; flags |= MBAMD_WG_MEM1; }
                    else e.c1 = (uint32_t) te.c1slot * slotb;
                    if (op.tip2) { e.c2 = (uint32_t) op.c2 * (uint32_t) MBAMD_WG_TW; flags |= MBAMD_W4_TIP2; }
                    else if (te.c2slot == 0xFF) { e.c2 = (uint32_t) op.c2 * pbuf; flags |= MBAMD_WG_MEM2; }
                    else e.c2 = (uint32_t) te.c2slot * slotb;
                    e.m1 = (uint32_t) op.m1 * mbuf;
                    e.m2 = (uint32_t) op.m2 * mbuf;
                    if (te.dslot != 0xFF) { keep = te.dslot; flags |= MBAMD_W4_KEEP; }
                    if (!op.tip1 && te.c1slot != 0xFF && (int) te.c1slot == prevKept) flags |= MBAMD_WG_PREV1;
                    if (!op.tip2 && te.c2slot != 0xFF && (int) te.c2slot == prevKept) flags |= MBAMD_WG_PREV2;
                    prevKept = te.dslot != 0xFF ? (int) te.dslot : -1;
                    mode = op.scaleWrite >= 0 ? SCALE_WRITE : (op.scaleRead >= 0 ? SCALE_READ : SCALE_NONE);
                    if (op.scaleWrite >= 0) e.ewrite = (uint32_t) op.scaleWrite * ebuf;
                    if (op.scaleRead >= 0) e.eread = (uint32_t) op.scaleRead * ebuf;
                    e.ctl = flags | (mode << 8) | ((uint32_t) segList[te.op] << 10) | (keep << 16);
                } else {
                    e.ctl = (flags & (MBAMD_W4_NOP | MBAMD_W4_BARRIER)) | MBAMD_W4_NOP;
                }
                continue;
            }
            if (te.pfOp[0] >= 0) {                          // PF entry
                const Walk4Op& p0 = seg[te.pfOp[0]];
                e.dst = (uint32_t) (te.pfChild[0] == 0 ? p0.c1 : p0.c2) * pbuf;
                e.c1 = (uint32_t) te.pfSlot[0] * 1024u;
                flags |= MBAMD_W4_PF0 | MBAMD_W4_NOP;
                if (te.pfOp[1] >= 0) {
                    const Walk4Op& p1 = seg[te.pfOp[1]];
                    e.c2 = (uint32_t) (te.pfChild[1] == 0 ? p1.c1 : p1.c2) * pbuf;
                    e.m1 = (uint32_t) te.pfSlot[1] * 1024u;
                    flags |= MBAMD_W4_PF1;
                }
            } else if (te.op >= 0) {
                const Walk4Op& op = seg[te.op];
                e.dst = (uint32_t) op.dst * pbuf;
                if (op.tip1) { e.c1 = (uint32_t) op.c1 * 32u; flags |= MBAMD_W4_TIP1; }
                else if (te.c1slot == 0xFE) flags |= MBAMD_W4_FWD1;
                else e.c1 = (uint32_t) te.c1slot * 1024u;
                if (op.tip2) { e.c2 = (uint32_t) op.c2 * 32u; flags |= MBAMD_W4_TIP2; }
                else if (te.c2slot == 0xFE) flags |= MBAMD_W4_FWD2;
                else e.c2 = (uint32_t) te.c2slot * 1024u;
                e.m1 = (uint32_t) op.m1 * mbuf;
                e.m2 = (uint32_t) op.m2 * mbuf;
                if (te.dslot != 0xFF) { keep = te.dslot; flags |= MBAMD_W4_KEEP; }
                mode = op.scaleWrite >= 0 ? SCALE_WRITE : (op.scaleRead >= 0 ? SCALE_READ : SCALE_NONE);
                if (op.scaleWrite >= 0) e.ewrite = (uint32_t) op.scaleWrite * ebuf;
                if (op.scaleRead >= 0) e.eread = (uint32_t) op.scaleRead * ebuf;
                w4entryOf[(size_t) te.op] = (int) (sg.first + i);
                const int subTips = w4subTips[(size_t) te.op];
                if (sg.plain && subTips >= 2 && subTips <= unstored4.maxTips()) {     // (kept or dropped below)
                    // the recipe: the subtree's operations with their children as tips or as operations of the recipe; every one of them
                    // ran earlier in this program (a child runs before its parent), so its entry is known
                    constexpr int RO = MBAMD_W4_UNSTORED_TIPS_MAX - 1;
                    const int* const sub = &w4subOps[(size_t) te.op * RO];
                    Plan::Unstored u;
                    u.entry = (int) (sg.first + i); u.dst = op.dst;
                    for (int& x : u.inner) x = -1;
                    bool placed = true;
                    for (int j = 0; j < RO && sub[j] >= 0; ++j) {
                        const Walk4Op& so = seg[(size_t) sub[j]];
                        Walk4Recipe::Op& ro = u.r.op[u.r.nops++];
                        ro.mode = so.scaleWrite >= 0 ? SCALE_WRITE : (so.scaleRead >= 0 ? SCALE_READ : SCALE_NONE);
                        ro.in1 = !so.tip1; ro.in2 = !so.tip2;
                        ro.c1 = so.c1; ro.c2 = so.c2;
                        for (int q = 0; q < j; ++q) {
                            if (ro.in1 && seg[(size_t) sub[q]].dst == so.c1) ro.c1 = q;
                            if (ro.in2 && seg[(size_t) sub[q]].dst == so.c2) ro.c2 = q;
                        }
                        if (sub[j] != te.op) { u.inner[j] = w4entryOf[(size_t) sub[j]]; placed = placed && u.inner[j] >= 0; }
                    }
                    if (placed) plan.unstoredSubtrees.push_back(u);
                }
            }
            if (te.vmwait != 0xFF) flags |= MBAMD_W4_VMWAIT;
            // the entry in front of a SCALE_READ entry of the same wave fetches that entry's stored exponents (mbamd_walk4.h)
            if ((i + 1) % (size_t) t.entries != 0) {
                const Walk4Template::Entry& tn = t.prog[i + 1];
                if (tn.op >= 0 && seg[tn.op].scaleWrite < 0 && seg[tn.op].scaleRead >= 0) flags |= MBAMD_W4_NEXT_READS;
            }
            e.ctl = flags | (mode << 8) | ((uint32_t) (te.vmwait == 0xFF ? 0 : te.vmwait) << 10) | (keep << 16);
            // a segment for the plain kernel: every operation says once what pair of child kinds it is (MBAMD_W4_KIND_*: the loop body it
            // runs in), and every entry -- the read-ahead tail included -- carries child 1's "plane offset or 0" ready-made in `eread`,
            // which nothing else reads in such a program (no entry divides by stored exponents)
            if (sg.plain) {
                if (te.op >= 0) e.ctl |= walk4_kind_of(flags);
                e.eread = (flags & MBAMD_W4_TIP1) ? e.c1 : 0u;
            }
        }
        if (sg.waves) {
            // the phase table behind the program (walk4_waves_table_entries)
            const size_t at = w4table.size();
            w4table.resize(at + walk4_waves_table_entries(t.W, t.phases));
            std::memset(&w4table[at], 0, (w4table.size() - at) * sizeof(Walk4Entry));
            uint32_t* const tab = reinterpret_cast<uint32_t*>(&w4table[at]);
            tab[0] = (uint32_t) t.phases;
            for (size_t q = 0; q < t.phaseCount.size(); ++q) tab[1 + q] = (uint32_t) t.phaseCount[q];
        }
        lastWalkW = t.W; lastWalkSlots = t.nslots; lastWalkEntries = t.entries; lastWalkPhases = t.phases; lastWalkCrossing = t.crossing;
        seg.clear();
        segList.clear();
        std::fill(segRead.begin(), segRead.end(), 0);
        std::fill(segWritten.begin(), segWritten.end(), 0);
        std::fill(segScale.begin(), segScale.end(), 0);
        return BEAGLE_SUCCESS;
    };
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        const char* what;
        if (const int crc = checkOperation(b, written, what)) return fail(crc, what);
        Walk4Op w;
        w.dst = b.destinationPartials;
        w.c1 = b.child1Partials; w.c2 = b.child2Partials;
        w.m1 = b.child1TransitionMatrix; w.m2 = b.child2TransitionMatrix;
        const uint8_t tip[2] = {(uint8_t) (tipStates[w.c1] && !written[w.c1]), (uint8_t) (tipStates[w.c2] && !written[w.c2])};
        w.tip1 = tip[0]; w.tip2 = tip[1];
        w.scaleWrite = w.scaleRead = -1;
        if (b.destinationScaleWrite != BEAGLE_OP_NONE) {
            w.scaleWrite = b.destinationScaleWrite;
        } else if (b.destinationScaleRead != BEAGLE_OP_NONE) {
            if (scales.isCumulative(b.destinationScaleRead) && !segScale[b.destinationScaleRead])
                return fail(BEAGLE_ERROR_NO_IMPLEMENTATION, "beagleUpdatePartials: destinationScaleRead names a cumulative buffer");
            w.scaleRead = b.destinationScaleRead;
        }
        // hazards that the in-launch dependency analysis does not cover end the segment (MrBayes never produces them):
        // a buffer written twice or written after it was read, an exponent buffer touched twice unless only read
        bool hazard = segWritten[w.dst] || segRead[w.dst];
        if (perList && o > 0 && listOf[o] != listOf[o - 1]) hazard = true;       // (independent lists: one program set each)
        if (w.scaleWrite >= 0 && segScale[w.scaleWrite]) hazard = true;
        if (w.scaleRead >= 0 && segScale[w.scaleRead] == 2) hazard = true;
        if (hazard) {
            int rc = flushSegment();
            if (rc) return rc;
        }
        segWritten[w.dst] = 1;
        if (!tip[0]) segRead[w.c1] = 1;
        if (!tip[1]) segRead[w.c2] = 1;
        if (w.scaleWrite >= 0) segScale[w.scaleWrite] = 2;
        if (w.scaleRead >= 0 && !segScale[w.scaleRead]) segScale[w.scaleRead] = 1;
        written[w.dst] = 1;
        seg.push_back(w);
        segList.push_back(listOf ? listOf[o] : 0);
    }
    int rc = flushSegment();
    if (rc) return rc;
    if (sw.verbose)
        std::fprintf(stderr, "[mbamd] walk plan: %d ops, %zu segment(s), W=%d, %d entries/wave, %d slots/%s, %d phases, %d reloads, %d external children, %d values cross waves in LDS%s\n",
                     n, plan.segments.size(), lastWalkW, lastWalkEntries, lastWalkSlots, plan.segments.back().waves ? "workgroup" : "wave", phases, reloads, externals,
                     lastWalkCrossing, plan.segments.back().plain ? " (plain)" : "");
    // a short program goes out with the launch itself (k_walk4_t<Walk4ArgsInline>, k_walkg<..., WalkGArgsInline>)
    plan.inlineProg.clear();
    // (a plain program of several waves has no generic reading: the slots of its entries are the workgroup's)
    const bool inlineForm = !sw.noInlinePrograms && plan.segments.size() == 1 && w4table.size() <= (size_t) MBAMD_W4_INLINE && !plan.segments[0].waves;
    // Small subtrees are not stored where nothing can read the HBM copy in the launch that makes them: the list is ONE segment and that
    // segment runs on the plain kernel, on one wave or several (no prefetch: every child is a tip, a slot -- also of a value from another
    // wave -- or the forwarded result).  Lists cut over several segments, programs in the kernel arguments and the generic / path
    // kernels store everything.
    plan.sideFirst = 0; plan.sideCount = 0;
    if (s4 && !sw.storeTipPairs && !sw.noPlainWalk && !inlineForm && plan.segments.size() == 1 && plan.segments[0].plain) {
        for (const Plan::Unstored& u : plan.unstoredSubtrees) w4table[(size_t) u.entry].ctl |= MBAMD_W4_NOSTORE;
        // the side table k_walk4_snapshot reads, behind the program: per subtree of more than two tips its own entry and its inner ones
        plan.sideFirst = w4table.size();
        for (const Plan::Unstored& u : plan.unstoredSubtrees) {
            if (u.r.nops < 2) continue;
            Walk4Entry side;
            std::memset(&side, 0, sizeof side);
            side.ctl = (uint32_t) u.entry; side.dst = (uint32_t) (u.r.nops - 1);
            side.c1 = (uint32_t) u.inner[0]; side.c2 = (uint32_t) (u.r.nops > 2 ? u.inner[1] : u.inner[0]);
            w4table.push_back(side);
            plan.sideCount++;
        }
    } else {
        plan.unstoredSubtrees.clear();
    }
    if (inlineForm) {
        plan.inlineProg = w4table;
        return BEAGLE_SUCCESS;
    }
    return planTable(plan, w4table.data(), w4table.size() * sizeof(Walk4Entry));
}

// A root-ward path (the list of a move that dirtied one branch): operation i has the result of operation i - 1 as one child; its
// other child -- and both children of operation 0 -- are compact tips or buffers the list does not write; no buffer or exponent
// buffer is written twice or read after it is written.  Round 6: also FORKED paths (the list of a topology move: root-ward paths
// that join, in post-order) -- an operation that does not read its predecessor's result begins a new ARM (the predecessor's
// result is saved), an operation whose other child is the saved result JOINS the arms; one saved result at a time.
// ops[0, n) are n / L lists of L operations (one list; or the mutually independent lists of the eigen-system parts of a codon
// model), every one such a path, and the hazard rules hold over all of them.  true: pathSteps describes the operations.  Anything
// else (false) is compiled by buildWalk, which also reports what is wrong with an operation.
inline bool Instance::recognisePath(const BeagleOperation* ops, int n, int L, bool& forked)
{
    std::vector<char>& written = w4written;          // buffers earlier operations write; after this loop: any operation
    written.assign((size_t) nBuffers, 0);
    std::vector<char>& named = w4segScale;           // how many scale fields of the operations name an exponent buffer (3 = more)
    named.assign(scales.count() + 1, 0);
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        const char* what;
        if (checkOperation(b, written, what) != BEAGLE_SUCCESS) return false;
        if (tipStates[b.destinationPartials] || written[b.destinationPartials]) return false;
        written[b.destinationPartials] = 1;
        for (int f : {b.destinationScaleWrite, b.destinationScaleRead})
            if (f >= 0 && f < nScale && named[f] < 3) ++named[f];
    }
    pathSteps.resize((size_t) n);
    forked = false;
    int saved = -1;                              // buffer of the saved result (an arm that waits for its join), or -1
    int armStart = 0, arms = 0;
    for (int o = 0; o < n; ++o) {
        const BeagleOperation& b = ops[o];
        PathStep& p = pathSteps[(size_t) o];
        const bool first = o % L == 0;
        const int prev = first ? -1 : ops[o - 1].destinationPartials;
        const bool one = !first && b.child1Partials == prev, two = !first && b.child2Partials == prev;
        if (one && two) return false;
        p.start = !one && !two;
        p.join = false;
        p.arm = 0;
        p.dst = b.destinationPartials;
        p.chain = two ? b.child2Partials : b.child1Partials; p.sib = two ? b.child1Partials : b.child2Partials;
        p.mchain = two ? b.child2TransitionMatrix : b.child1TransitionMatrix; p.msib = two ? b.child1TransitionMatrix : b.child2TransitionMatrix;
        if (p.start) {
            if (!first) {
                if (saved >= 0) return false;                                 // (two results waiting: not the path kernels' shape)
                saved = prev;
                pathSteps[(size_t) armStart].arm = o - armStart;
            }
            armStart = o;
            ++arms;
        } else if (saved >= 0 && p.sib == saved) {
            p.join = true;
            saved = -1;
        }
        // what comes from outside must not be written anywhere in the lists (before: a second dependency; after: a hazard)
        if ((!p.join && written[p.sib]) || (p.start && written[p.chain])) return false;
        p.chainTip = p.start && tipStates[p.chain] != nullptr;
        p.sibTip = !p.join && tipStates[p.sib] != nullptr;
        p.scaleMode = SCALE_NONE;
        p.scaleIdx = -1;
        if (b.destinationScaleWrite != BEAGLE_OP_NONE) {
            // the operation's own: nobody else's scale fields name it
            if (named[b.destinationScaleWrite] != 1 + (b.destinationScaleRead == b.destinationScaleWrite ? 1 : 0)) return false;
            p.scaleMode = SCALE_WRITE;
            p.scaleIdx = b.destinationScaleWrite;
        } else if (b.destinationScaleRead != BEAGLE_OP_NONE) {
            if (scales.isCumulative(b.destinationScaleRead)) return false;
            p.scaleMode = SCALE_READ;
            p.scaleIdx = b.destinationScaleRead;
        }
        if (o % L == L - 1) {                    // the end of a list
            if (saved >= 0) return false;        // (an arm nobody joins: two trees in one list)
            pathSteps[(size_t) armStart].arm = o + 1 - armStart;
            forked = forked || arms > 1;
            arms = 0;
        }
    }
    return true;
}

// A step as an entry of k_path4 / k_pathg, offsets in the caller's units: a partials buffer, a compact tip, a matrix buffer, and
// the scratch exponent row an operation that records no exponents stores to.
inline Walk4Entry Instance::pathEntry(const PathStep& p, uint32_t pbuf, uint32_t tipb, uint32_t mbuf, int scratchRow) const
{
    const uint32_t ebuf = (uint32_t) K * 64u;
    Walk4Entry e;
    std::memset(&e, 0, sizeof e);
    uint32_t flags = 0;
    e.dst = (uint32_t) p.dst * pbuf;
    if (p.start) {
        flags |= MBAMD_P4_START;
        if (p.chainTip) { e.c1 = (uint32_t) p.chain * tipb; flags |= MBAMD_W4_TIP1; }
        else e.c1 = (uint32_t) p.chain * pbuf;
    }
    if (p.join) flags |= MBAMD_P4_JOIN;
    else if (p.sibTip) { e.c2 = (uint32_t) p.sib * tipb; flags |= MBAMD_W4_TIP2; }
    else e.c2 = (uint32_t) p.sib * pbuf;
    e.m1 = (uint32_t) p.mchain * mbuf;
    e.m2 = (uint32_t) p.msib * mbuf;
    e.ewrite = (uint32_t) scratchRow * ebuf;
    e.eread = (uint32_t) scales.count() * ebuf;
    if (p.scaleMode == SCALE_WRITE) e.ewrite = (uint32_t) p.scaleIdx * ebuf;
    else if (p.scaleMode == SCALE_READ) e.eread = (uint32_t) p.scaleIdx * ebuf;
    e.ctl = flags | ((uint32_t) p.scaleMode << 8);
    return e;
}

// a path plan's geometry: one single-wave program of `entries` per list, no LDS slots, no read-ahead tail
inline void Instance::pathPlan(Plan& plan, int entries, bool forked)
{
    plan.forked = forked;
    plan.segments.clear();
    Plan::Segment sg;
    sg.first = 0; sg.W = 1; sg.entries = entries; sg.nslots = 0; sg.tail = 0;
    plan.segments.push_back(sg);
    lastWalkW = 1; lastWalkSlots = 0; lastWalkEntries = entries; lastWalkPhases = 1;
}

}  // namespace mbamd

#endif  // MBAMD_F32_WALK_H_
