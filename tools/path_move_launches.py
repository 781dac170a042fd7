#!/usr/bin/env python3
"""Count what a path move pays for the small subtrees a whole-tree launch left unstored (profiles/walk4_small_subtrees.txt section 6,
profiles/walk4_plain_waves.txt section 6): a fixed-topology chain on a golden case -- branch-length moves (one branch, new length =
old x exp(0.2 (u - 0.5)), each one fused path launch) and every fifth generation a whole-tree evaluation, Metropolis accept / reject --
then the recompute exports, the walk counts and the wall time per generation of the calling process.

    python tools/path_move_launches.py [--case bench_c2] [--generations 300] [--seed 7]

Environment switches (MBAMD_STORE_TIP_PAIRS, MBAMD_UNSTORED_TIPS, MBAMD_WALK_WAVES, MBAMD_LIBRARY) select what is compared.  Prints one
JSON line.  Run from the repository root of the tree whose package and library are meant."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np  # noqa: E402

from mrbayes_amd import beagle as bg  # noqa: E402
from mrbayes_amd import likelihood as lk  # noqa: E402
from mrbayes_amd.division import division_from_golden  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="bench_c2")
    ap.add_argument("--generations", type=int, default=300)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    div = division_from_golden(os.path.join(os.getcwd(), "tests", "golden"), args.case)
    t = div.tree
    bd = lk.BeagleDivision(div, bg.library())
    rng = np.random.default_rng(args.seed)
    branches = [p for p in t.all_down_pass if p != t.root and t.anc[p] != -1]
    lnl = bd.LogLike(0)
    bd.AcceptMove(0)
    moves = accepted = whole = 0
    t0 = time.perf_counter()
    for g in range(1, args.generations + 1):
        if g % 5 == 0:
            bd.TouchAllTreeNodes(0)
            new = bd.LogLike(0)
            whole += 1
            assert abs(new - lnl) <= 1e-6 * abs(lnl), (new, lnl)           # (the same state, every node again)
            bd.AcceptMove(0)
            continue
        i = branches[int(rng.integers(len(branches)))]
        old = t.length[i]
        t.length[i] = old * math.exp(0.2 * (rng.random() - 0.5))
        bd.TouchBranch(0, i)
        new = bd.LogLike(0)
        moves += 1
        if math.log(rng.random()) < new - lnl:
            lnl = new
            accepted += 1
            bd.AcceptMove(0)
        else:
            t.length[i] = old
            bd.ResetFlips(0)
    wall = time.perf_counter() - t0
    inst = bd.inst
    out = {"case": args.case, "generations": args.generations, "path_moves": moves, "accepted": accepted, "whole_tree": whole + 1,
           "lnL": lnl, "ms_per_generation": 1e3 * wall / args.generations,
           "tip_pairs_left_made_launches": inst.get_recompute_counts(), "subtrees_left_made_launches": inst.get_subtree_recompute_counts(),
           "walk_counts": inst.get_walk_counts(), "list_counts": inst.get_list_counts()}
    if hasattr(inst, "get_plain_wave_counts"):
        out["plain_launches_by_waves"] = inst.get_plain_wave_counts()
    bd.finalize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
