"""Host side of the hot path above the C ABI: the Python twin of MrBayes' BEAGLE adapter.

Function-for-function mirror of the reference's src/mbbeagle.c (same names, same argument meaning, same
call protocol), so that the parity tests read like the reference and so that bench.py drives the
engine exactly the way an unmodified MrBayes does:

    InitBeagleInstance                       src/mbbeagle.c:60    (+ index tables of InitChainCondLikes,
                                                                   src/mcmc.c:5907-6253)
    TreeTiProbs_Beagle                       src/mbbeagle.c:1368
    TreeCondLikes_Beagle_No_Rescale          src/mbbeagle.c:783
    TreeCondLikes_Beagle_Rescale_All         src/mbbeagle.c:884
    TreeCondLikes_Beagle_Always_Rescale      src/mbbeagle.c:995
    TreeLikelihood_Beagle                    src/mbbeagle.c:1117
    LaunchBEAGLELogLikeForDivision           src/mbbeagle.c:400
    Flip*Space / ResetFlips                  src/likelihood.c:5614-5683, src/mcmc.c:15695-15766

The real MrBayes needs none of this -- it links libhmsbeagle.so directly; this module
exists for tests, the benchmark and the multi-GPU chain driver.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np

from . import beagle as bg
from .division import Division
from .model import eigen_blocks

MB_BEAGLE_SCALE_ALWAYS = 0
MB_BEAGLE_SCALE_DYNAMIC = 1
BRLENS_MIN = 1e-8      # src/bayes.h
BRLENS_MAX = 100.0
BEAGLE_RESCALE_FREQ = 160   # src/bayes.h:77


class BeagleDivision:
    """ModelInfo-like state of one division driven through the BEAGLE ABI for `nchains` local chains."""

    def __init__(self, div: Division, lib: Optional[bg.BeagleLibrary] = None, nchains: int = 1,
                 scaling: int = MB_BEAGLE_SCALE_ALWAYS, resource: Optional[int] = None, device_eigen: bool = False,
                 double_precision: bool = False, pre_order: bool = False, second_order: bool = False, spare: int = 0):
        self.div = div
        pre_order = pre_order or second_order
        self.pre_order = pre_order                      # reserve the buffers of BranchGradient (behind every existing one)
        self.second_order = second_order                # ... and the second differential matrix of BranchCurvature (behind those)
        self.spare = int(spare)
        self.double_precision = double_precision        # `set beagleprecision=double` (src/command.c:6765-6766): a preference flag
        self.device_eigen = device_eigen and div.rate_matrices is not None and bool(np.all(np.asarray(div.pi) > 0))
        self.lib = lib or bg.library()
        self.nchains = nchains
        self.scaling = scaling
        t = div.tree
        self.N = N = t.ntaxa
        self.nInt = nInt = t.n_int_nodes
        self.nNodes = nNodes = t.n_nodes
        self.step = step = div.n_cijk_parts            # indexStep = nCijkParts, src/mcmc.c:5907-5910
        # --- index tables (InitChainCondLikes) -------------------------------------------------
        self.condLikeIndex = [[0] * nNodes for _ in range(nchains)]
        for c in range(nchains):
            for i in range(N):
                self.condLikeIndex[c][i] = i * step                      # tips shared by all chains
            for j in range(nInt):
                self.condLikeIndex[c][N + j] = (N + c * nInt + j) * step
        self.condLikeScratchIndex = [0] * nNodes
        for j in range(nInt):
            self.condLikeScratchIndex[N + j] = (N + nchains * nInt + j) * step
        self.numCondLikes = N + (nchains + 1) * nInt
        self.tiProbsIndex = [[(c * nNodes + i) * step for i in range(nNodes)] for c in range(nchains)]
        self.tiProbsScratchIndex = [(nchains * nNodes + i) * step for i in range(nNodes)]
        self.numTiProbs = (nchains + 1) * nNodes
        self.nodeScalerIndex = [[0] * nNodes for _ in range(nchains)]
        for c in range(nchains):
            for j in range(nInt):
                self.nodeScalerIndex[c][N + j] = (c * nInt + j) * step
        self.nodeScalerScratchIndex = [0] * nNodes
        for j in range(nInt):
            self.nodeScalerScratchIndex[N + j] = (nchains * nInt + j) * step
        base = (nchains + 1) * nInt
        self.siteScalerIndex = [(base + c) * step for c in range(nchains)]
        self.siteScalerScratchIndex = (base + nchains) * step
        self.numScalers = (nchains + 1) * (nInt + 1)
        self.cijkIndex = [c * step for c in range(nchains)]
        self.cijkScratchIndex = nchains * step
        # --- pre-order buffers (BranchGradient): one partials buffer per node and one for the start vector, one matrix for D
        self.numPreOrder = self.numDiffMatrices = 0
        if pre_order:
            self.preOrderIndex = [(self.numCondLikes + i) * step for i in range(nNodes)]
            self.preOrderStartIndex = (self.numCondLikes + nNodes) * step
            self.numPreOrder = nNodes + 1
            self.diffMatrixIndex = self.numTiProbs * step
            self.numDiffMatrices = 1
            if div.complex_eigen:
                # a non-reversible model cannot turn the root branch round: the process starts at the top interior node, and the
                # root tip is its third child -- one more pre-order buffer (the root tip's) and an identity matrix (PreOrderOperations)
                self.preOrderRootIndex = (self.numCondLikes + nNodes + 1) * step
                self.numPreOrder = nNodes + 2
                self.identityMatrixIndex = (self.numTiProbs + 1) * step
                self.numDiffMatrices = 2
            if second_order:
                self.diffMatrix2Index = (self.numTiProbs + self.numDiffMatrices) * step
                self.numDiffMatrices += 1
        # --- dirty flags ("touch" state), per chain ----------------------------------------------
        self.upDateCl = [[True] * nNodes for _ in range(nchains)]
        self.upDateTi = [[True] * nNodes for _ in range(nchains)]
        self.upDateAll = [True] * nchains
        self.upDateCijk = [True] * nchains
        self.flips: List[List[tuple]] = [[] for _ in range(nchains)]
        # dynamic rescaling state (src/mcmc.c:6220-6240)
        self.rescaleFreq = [max(1, BEAGLE_RESCALE_FREQ // div.nstates)] * nchains
        self.isScalerNode = [[False] * nNodes for _ in range(nchains)]
        self.successCount = [0] * nchains
        self.rescaleBeagleAll = False
        self.InitBeagleInstance(resource)

    # ------------------------------------------------------------------------------------------
    def InitBeagleInstance(self, resource=None):
        d = self.div
        part_ambig = [d.tip_states[i] is None for i in range(self.N)]
        num_part_ambig = sum(part_ambig)
        req = bg.BEAGLE_FLAG_SCALERS_LOG if self.scaling == MB_BEAGLE_SCALE_ALWAYS else 0   # src/mbbeagle.c:191-194
        if d.complex_eigen:                                               # a non-reversible model: eigenvalues in conjugate pairs
            req |= bg.BEAGLE_FLAG_EIGEN_COMPLEX
        # `spare` partials, matrix and scale buffers of each kind behind every other one (spareBufferIndex, spareMatrixIndex,
        # spareScalerIndex: scratch for a client's own operations, as InsertionLogLikelihoods' subtree); 0: none
        self.spareBufferIndex = (self.numCondLikes + self.numPreOrder) * self.step
        self.spareMatrixIndex = (self.numTiProbs + self.numDiffMatrices) * self.step
        self.spareScalerIndex = self.numScalers * self.step
        self.inst = bg.BeagleInstance(
            self.lib, self.N, (self.numCondLikes + self.numPreOrder) * self.step + self.spare, self.N - num_part_ambig, d.nstates, d.npatterns,
            (self.nchains + 1) * self.step, (self.numTiProbs + self.numDiffMatrices) * self.step + self.spare, d.ncat,
            self.numScalers * self.step + self.spare,
            resource=resource, requirement_flags=req,
            preference_flags=bg.BEAGLE_FLAG_PRECISION_DOUBLE if self.double_precision else bg.BEAGLE_FLAG_PRECISION_SINGLE)
        for i in range(self.N):                                           # src/mbbeagle.c:123-167
            if not part_ambig[i]:
                self.inst.set_tip_states(i * self.step, d.tip_states[i])
            else:
                self.inst.set_tip_partials(i * self.step, d.tip_partials[i])
        self.inst.set_pattern_weights(d.weights)                          # src/mcmc.c:6264
        for i in range(self.numScalers * self.step):                      # src/mcmc.c:6268-6271
            self.inst.reset_scale_factors(i)

    def finalize(self):
        self.inst.finalize()

    # ---- buffer flips (MH accept/reject for free) ---------------------------------------------
    def _flip(self, table, scratch, chain, node, tag):
        table[chain][node], scratch[node] = scratch[node], table[chain][node]
        self.flips[chain].append((tag, node))

    def FlipCondLikeSpace(self, chain, node):
        self._flip(self.condLikeIndex, self.condLikeScratchIndex, chain, node, "cl")

    def FlipNodeScalerSpace(self, chain, node):
        self._flip(self.nodeScalerIndex, self.nodeScalerScratchIndex, chain, node, "ns")

    def FlipTiProbsSpace(self, chain, node):
        self._flip(self.tiProbsIndex, self.tiProbsScratchIndex, chain, node, "ti")

    def FlipSiteScalerSpace(self, chain):
        self.siteScalerIndex[chain], self.siteScalerScratchIndex = self.siteScalerScratchIndex, self.siteScalerIndex[chain]
        self.flips[chain].append(("ss", -1))

    def FlipCijkSpace(self, chain):
        self.cijkIndex[chain], self.cijkScratchIndex = self.cijkScratchIndex, self.cijkIndex[chain]
        self.flips[chain].append(("cijk", -1))

    def ResetFlips(self, chain):
        """Undo every flip since the last accept (move rejected), src/mcmc.c:15695-15766."""
        for tag, node in reversed(self.flips[chain]):
            if tag == "cl":
                self.condLikeIndex[chain][node], self.condLikeScratchIndex[node] = self.condLikeScratchIndex[node], self.condLikeIndex[chain][node]
            elif tag == "ns":
                self.nodeScalerIndex[chain][node], self.nodeScalerScratchIndex[node] = self.nodeScalerScratchIndex[node], self.nodeScalerIndex[chain][node]
            elif tag == "ti":
                self.tiProbsIndex[chain][node], self.tiProbsScratchIndex[node] = self.tiProbsScratchIndex[node], self.tiProbsIndex[chain][node]
            elif tag == "ss":
                self.siteScalerIndex[chain], self.siteScalerScratchIndex = self.siteScalerScratchIndex, self.siteScalerIndex[chain]
            elif tag == "cijk":
                self.cijkIndex[chain], self.cijkScratchIndex = self.cijkScratchIndex, self.cijkIndex[chain]
        self.flips[chain] = []

    def AcceptMove(self, chain):
        self.flips[chain] = []

    # ---- touching --------------------------------------------------------------------------------
    def TouchAllTreeNodes(self, chain):
        """src/proposal.c:17682: everything dirty."""
        self.upDateCl[chain] = [True] * self.nNodes
        self.upDateTi[chain] = [True] * self.nNodes
        self.upDateAll[chain] = True

    def ClearTouches(self, chain):
        self.upDateCl[chain] = [False] * self.nNodes
        self.upDateTi[chain] = [False] * self.nNodes
        self.upDateAll[chain] = False
        self.upDateCijk[chain] = False

    def TouchBranch(self, chain, node):
        """A branch-length change on `node`: new Ti for the branch, new CLs on the path to the root."""
        t = self.div.tree
        self.upDateTi[chain][node] = True
        p = t.anc[node]
        while p >= self.N and p != -1:
            self.upDateCl[chain][p] = True
            if p == t.root_left:
                break
            p = t.anc[p]

    # ---- UpDateCijk (BEAGLE branch, src/likelihood.c:10636-10660, 10736-10757) ----------------------
    def UpDateCijk(self, chain):
        self.FlipCijkSpace(chain)
        if self.device_eigen:
            # extension: the eigen-systems are computed on the device from the rate matrices -- an
            # unmodified MrBayes has no call for this, it sends finished eigen-systems like the branch below
            self.inst.set_rate_matrices(self.cijkIndex[chain], np.stack(self.div.rate_matrices), self.div.pi)
        else:
            d_complex = self.div.complex_eigen          # (a complex instance reads 2 S eigenvalues: zero imaginary parts for a real part)
            for i, es in enumerate(self.div.eigen):
                self.inst.set_eigen_decomposition(self.cijkIndex[chain] + i, es.evec, es.ivec, es.values if d_complex else es.eval)
        self.upDateAll[chain] = True

    # ---- TreeTiProbs_Beagle ------------------------------------------------------------------------
    def TreeTiProbs_Beagle(self, chain):
        d, t = self.div, self.div.tree
        self.inst.set_category_rates(d.cat_rates)                          # src/mbbeagle.c:1404-1409
        idx, lens = [], []
        for p in t.all_down_pass:
            if self.upDateTi[chain][p]:
                self.FlipTiProbsSpace(chain, p)
                length = min(max(t.length[p], BRLENS_MIN), BRLENS_MAX)     # src/mbbeagle.c:1453-1456
                lens.append(length)
                idx.append(self.tiProbsIndex[chain][p])
        if idx:
            idx = np.asarray(idx, dtype=np.int32)
            for i in range(self.step):                                     # src/mbbeagle.c:1475-1486
                self.inst.update_transition_matrices(self.cijkIndex[chain] + i, idx + i, lens)

    # ---- operation builders ------------------------------------------------------------------------
    def _op(self, chain, p):
        t = self.div.tree
        l, r = t.left[p], t.right[p]
        return [self.condLikeIndex[chain][p], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE,
                self.condLikeIndex[chain][l], self.tiProbsIndex[chain][l],
                self.condLikeIndex[chain][r], self.tiProbsIndex[chain][r]]

    def _expand_parts(self, op, chil1Step, chil2Step, j):
        """The j-th cijk-part twin of an operation (src/mbbeagle.c:845-863, 951-971, 1062-1075)."""
        o = list(op)
        o[0] += j
        if o[1] != bg.BEAGLE_OP_NONE:
            o[1] += j
        if o[2] != bg.BEAGLE_OP_NONE:
            o[2] += j
        o[3] += j * chil1Step
        o[4] += j
        o[5] += j * chil2Step
        o[6] += j
        return o

    def TreeCondLikes_Beagle_No_Rescale(self, chain):
        t = self.div.tree
        ops = []
        for p in t.int_down_pass:
            if not self.upDateCl[chain][p]:
                continue
            self.FlipCondLikeSpace(chain, p)
            op = self._op(chain, p)
            if self.isScalerNode[chain][p]:
                op[2] = self.nodeScalerIndex[chain][p]
            s1 = 0 if t.left[p] < self.N else 1
            s2 = 0 if t.right[p] < self.N else 1
            for j in range(self.step):
                ops.append(self._expand_parts(op, s1, s2, j))
        if ops:
            self.inst.update_partials(np.asarray(ops, dtype=np.int32), bg.BEAGLE_OP_NONE)

    def TreeCondLikes_Beagle_Rescale_All(self, chain):
        t = self.div.tree
        per_part: List[List[list]] = [[] for _ in range(self.step)]
        for p in t.int_down_pass:
            if not self.upDateCl[chain][p]:
                self.FlipCondLikeSpace(chain, p)
            op = self._op(chain, p)
            if self.isScalerNode[chain][p]:
                self.FlipNodeScalerSpace(chain, p)
                op[1] = self.nodeScalerIndex[chain][p]
            s1 = 0 if t.left[p] < self.N else 1
            s2 = 0 if t.right[p] < self.N else 1
            for j in range(self.step):
                per_part[j].append(self._expand_parts(op, s1, s2, j))
        for j in range(self.step):
            self.inst.update_partials(np.asarray(per_part[j], dtype=np.int32), self.siteScalerIndex[chain] + j)

    def TreeCondLikes_Beagle_Always_Rescale(self, chain):
        t = self.div.tree
        per_part: List[List[list]] = [[] for _ in range(self.step)]
        remove: List[List[int]] = [[] for _ in range(self.step)]
        for p in t.int_down_pass:
            if not self.upDateCl[chain][p]:
                continue
            if not self.upDateAll[chain]:                                  # remove old scalers
                for j in range(self.step):
                    remove[j].append(self.nodeScalerIndex[chain][p] + j)
            self.FlipCondLikeSpace(chain, p)
            self.FlipNodeScalerSpace(chain, p)
            op = self._op(chain, p)
            op[1] = self.nodeScalerIndex[chain][p]
            s1 = 0 if t.left[p] < self.N else 1
            s2 = 0 if t.right[p] < self.N else 1
            for j in range(self.step):
                per_part[j].append(self._expand_parts(op, s1, s2, j))
        for j in range(self.step):
            cum = self.siteScalerIndex[chain] + j
            if not self.upDateAll[chain] and remove[j]:
                self.inst.remove_scale_factors(remove[j], cum)
            if per_part[j]:
                self.inst.update_partials(np.asarray(per_part[j], dtype=np.int32), cum)

    # ---- TreeLikelihood_Beagle -----------------------------------------------------------------------
    def TreeLikelihood_Beagle(self, chain):
        """Returns (beagle return code, lnL)."""
        d, t = self.div, self.div.tree
        p = t.root_left
        if self.upDateCijk[chain]:
            for i in range(self.step):
                self.inst.set_state_frequencies(self.cijkIndex[chain] + i, d.pi)
        if d.n_cijk_parts > 1 or d.pinvar > 0.0 or self.upDateCijk[chain]:
            for i in range(self.step):
                self.inst.set_category_weights(self.cijkIndex[chain] + i, d.category_weights(i))
        buf = [self.condLikeIndex[chain][p] + i for i in range(self.step)]
        eig = [self.cijkIndex[chain] + i for i in range(self.step)]
        cum = [self.siteScalerIndex[chain] + i for i in range(self.step)]
        child = [self.condLikeIndex[chain][t.root]] * self.step
        prob = [self.tiProbsIndex[chain][p] + i for i in range(self.step)]
        rc, lnl = self.inst.calculate_edge_log_likelihoods(buf, child, prob, eig, eig, cum)
        if not math.isfinite(lnl):
            rc = bg.BEAGLE_ERROR_FLOATING_POINT
        if rc == bg.BEAGLE_ERROR_FLOATING_POINT:
            return rc, lnl
        self.successCount[chain] += 1
        if d.pinvar > 0.0:                                                 # src/mbbeagle.c:1326-1356
            site = self.inst.get_site_log_likelihoods()
            like_i = (d.inv_condlikes.astype(np.float64) * d.pi[None, :]).sum(axis=1)
            with np.errstate(divide="ignore"):
                ln_like_i = np.log(like_i * d.pinvar)
            diff = np.where(like_i != 0.0, ln_like_i - site, -1000.0)
            contrib = np.where(diff < -200.0, site,
                               np.where(diff > 200.0, ln_like_i, site + np.log1p(np.exp(np.clip(diff, -745, 700)))))
            lnl = float((contrib * d.weights).sum())
        return rc, lnl

    # ---- ResetScalersPartition (src/mcmc.c:15780) --------------------------------------------------
    def ResetScalersPartition(self, chain, rescaleFreq):
        t = self.div.tree
        unscaled = [0] * self.nNodes
        for p in t.int_down_pass:
            l, r = t.left[p], t.right[p]
            n = 1 + (unscaled[l] if l >= self.N else 0) + (unscaled[r] if r >= self.N else 0)
            if n >= rescaleFreq:
                self.isScalerNode[chain][p] = True
                unscaled[p] = 0
            else:
                self.isScalerNode[chain][p] = False
                unscaled[p] = n

    # ---- LaunchBEAGLELogLikeForDivision --------------------------------------------------------------
    def LaunchBEAGLELogLikeForDivision(self, chain):
        if self.upDateCijk[chain]:
            self.UpDateCijk(chain)                                         # src/likelihood.c:7864-7872
        if self.scaling == MB_BEAGLE_SCALE_ALWAYS:
            self.FlipSiteScalerSpace(chain)
            if self.upDateAll[chain]:
                for i in range(self.step):
                    self.inst.reset_scale_factors(self.siteScalerIndex[chain] + i)
            else:                                                          # CopySiteScalers, src/likelihood.c:8071-8107
                for i in range(self.step):
                    self.inst.copy_scale_factors(self.siteScalerIndex[chain] + i, self.siteScalerScratchIndex + i)
            self.TreeTiProbs_Beagle(chain)
            self.TreeCondLikes_Beagle_Always_Rescale(chain)
            rc, lnl = self.TreeLikelihood_Beagle(chain)
            return lnl
        # MB_BEAGLE_SCALE_DYNAMIC (src/mbbeagle.c:429-534), without the success-count heuristics
        self.rescaleBeagleAll = False
        self.TreeTiProbs_Beagle(chain)
        self.TreeCondLikes_Beagle_No_Rescale(chain)
        rc, lnl = self.TreeLikelihood_Beagle(chain)
        if rc == bg.BEAGLE_ERROR_FLOATING_POINT:
            rescaleFreqNew = self.rescaleFreq[chain]
            self.successCount[chain] = 0
            self.rescaleBeagleAll = True
            self.FlipSiteScalerSpace(chain)
            while True:
                self.ResetScalersPartition(chain, rescaleFreqNew)
                for i in range(self.step):
                    self.inst.reset_scale_factors(self.siteScalerIndex[chain] + i)
                self.TreeCondLikes_Beagle_Rescale_All(chain)
                rc, lnl = self.TreeLikelihood_Beagle(chain)
                if rc == bg.BEAGLE_ERROR_FLOATING_POINT and rescaleFreqNew > 1:
                    for p in self.div.tree.int_down_pass:
                        if self.isScalerNode[chain][p]:
                            self.FlipNodeScalerSpace(chain, p)
                    rescaleFreqNew -= rescaleFreqNew >> 3
                    rescaleFreqNew -= 1
                    rescaleFreqNew = max(rescaleFreqNew, 1)
                    continue
                break
            self.rescaleFreq[chain] = rescaleFreqNew
        return lnl

    # ---- the gradient in all branch lengths (no counterpart in src/mbbeagle.c) ------------------------------------------
    def PreOrderOperations(self, chain):
        """The pre-order list of the whole tree, top-down and level by level (the engine runs operations that do not depend on one
        another in one launch, and cuts the list where they do): the top interior node hangs from the start vector without a
        sibling factor, every other node from its parent's pre-order buffer with its sibling's post-order buffer.  (A division with
        complex eigen-systems: the root tip is the top node's third child, see below.)"""
        t = self.div.tree
        top = t.root_left
        if self.div.complex_eigen:
            # the start vector is pi at the top node; its buffer gets pi_i (P_top tip_root)[i] (the root tip as a sibling, through the
            # identity), the root tip's own buffer sum_i P_top[i,j] pi_i post_top[i]: the pair BranchGradient reads for the root branch
            ops = [[self.preOrderIndex[top], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, self.preOrderStartIndex, self.identityMatrixIndex,
                    self.condLikeIndex[chain][t.root], self.tiProbsIndex[chain][top]],
                   [self.preOrderRootIndex, bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, self.preOrderStartIndex, self.tiProbsIndex[chain][top],
                    self.condLikeIndex[chain][top], self.identityMatrixIndex]]
        else:
            ops = [[self.preOrderIndex[top], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, self.preOrderStartIndex, self.tiProbsIndex[chain][top],
                    bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE]]
        level = [top]
        while level:
            below = []
            for p in level:
                for n, sib in ((t.left[p], t.right[p]), (t.right[p], t.left[p])):
                    ops.append([self.preOrderIndex[n], bg.BEAGLE_OP_NONE, bg.BEAGLE_OP_NONE, self.preOrderIndex[p], self.tiProbsIndex[chain][n],
                                self.condLikeIndex[chain][sib], self.tiProbsIndex[chain][sib]])
                    if t.left[n] >= 0:
                        below.append(n)
            level = below
        return np.asarray(ops, dtype=np.int32)

    def _PreOrderPass(self, chain, who):
        """the start vector pi_i tip_root[c,i], then the pre-order list of the whole tree"""
        if not self.pre_order:
            raise ValueError(who + " needs BeagleDivision(..., pre_order=True)")
        if self.step != 1:
            raise NotImplementedError(who + ": one eigen-system part per division")
        d, t = self.div, self.div.tree
        S, K, P = d.nstates, d.ncat, d.npatterns
        tip = np.ones((P, S))
        if d.tip_states[t.root] is not None:
            st = np.asarray(d.tip_states[t.root])
            ok = (st >= 0) & (st < S)
            tip[ok] = 0.0
            tip[np.arange(P)[ok], st[ok]] = 1.0
        else:
            tip = np.asarray(d.tip_partials[t.root], dtype=np.float64).reshape(P, S)
        start = tip * np.asarray(d.pi, dtype=np.float64)[None, :]
        if d.complex_eigen:                  # (the root tip enters through the operations: PreOrderOperations)
            start = np.broadcast_to(np.asarray(d.pi, dtype=np.float64)[None, :], (P, S))
            self.inst.set_transition_matrix(self.identityMatrixIndex, np.broadcast_to(np.eye(S), (K, S, S)))
        self.inst.set_partials(self.preOrderStartIndex, np.broadcast_to(start, (K, P, S)))
        self.inst.update_pre_partials(self.PreOrderOperations(chain))

    # the (post-order, pre-order) buffer pair at the lower end of every branch; a non-reversible model reads the root branch at
    # the root tip (PreOrderOperations)
    def _EdgePosts(self, chain, nodes):
        t = self.div.tree
        return [self.condLikeIndex[chain][t.root if self.div.complex_eigen and n == t.root_left else n] for n in nodes]

    def _EdgePres(self, nodes):
        t = self.div.tree
        return [self.preOrderRootIndex if self.div.complex_eigen and n == t.root_left else self.preOrderIndex[n] for n in nodes]

    def _RateMatrix(self):
        es = self.div.eigen[0]
        if es.imag is None:
            return (np.asarray(es.evec, dtype=np.float64) * np.asarray(es.eval, dtype=np.float64)[None, :]) @ np.asarray(es.ivec, dtype=np.float64)
        # Q = U D U^-1 with D in block form
        return np.asarray(es.evec, dtype=np.float64) @ eigen_blocks(es, es.eval + 1j * es.imag) @ np.asarray(es.ivec, dtype=np.float64)

    def BranchGradient(self, chain=0, sites=False):
        """{node: d lnL / d t_node} for all 2N-3 branches of the chain's current tree, after LogLike: the start vector
        pi_i tip_root[c,i] and D_k = r_k Q are set, the pre-order list of the whole tree is issued and ONE
        calculate_edge_gradient call reads every branch.  sites=True: (that, {node: per-site derivatives})."""
        self._PreOrderPass(chain, "BranchGradient")
        d, t = self.div, self.div.tree
        q = self._RateMatrix()
        self.inst.set_differential_matrix(self.diffMatrixIndex, np.asarray(d.cat_rates, dtype=np.float64)[:, None, None] * q[None, :, :])
        nodes = list(t.all_down_pass)
        rc, per, sums, _ = self.inst.calculate_edge_gradient(self._EdgePosts(chain, nodes), self._EdgePres(nodes),
                                                             [self.diffMatrixIndex] * len(nodes), [self.cijkIndex[chain]] * len(nodes), sites=sites)
        grad = {n: float(sums[i]) for i, n in enumerate(nodes)}
        return (grad, {n: per[i] for i, n in enumerate(nodes)}) if sites else grad

    def BranchCurvature(self, chain=0, sites=False):
        """{node: (d lnL / d t_node, d2 lnL / d t_node^2)} for all 2N-3 branches of the chain's current tree, after LogLike: as
        BranchGradient with D1_k = r_k Q and D2_k = r_k^2 Q^2, and ONE calculate_edge_second_derivatives call reads every branch
        once.  sites=True: (that, {node: (per-site d1, per-site d2)}).  Needs BeagleDivision(..., second_order=True)."""
        if not self.second_order:
            raise ValueError("BranchCurvature needs BeagleDivision(..., second_order=True)")
        self._PreOrderPass(chain, "BranchCurvature")
        d, t = self.div, self.div.tree
        q, r = self._RateMatrix(), np.asarray(d.cat_rates, dtype=np.float64)
        self.inst.set_differential_matrix(self.diffMatrixIndex, r[:, None, None] * q[None, :, :])
        self.inst.set_differential_matrix(self.diffMatrix2Index, (r * r)[:, None, None] * (q @ q)[None, :, :])
        nodes = list(t.all_down_pass)
        rc, per1, per2, sums1, sums2 = self.inst.calculate_edge_second_derivatives(
            self._EdgePosts(chain, nodes), self._EdgePres(nodes), [self.diffMatrixIndex] * len(nodes), [self.diffMatrix2Index] * len(nodes),
            [self.cijkIndex[chain]] * len(nodes), sites=sites)
        curv = {n: (float(sums1[i]), float(sums2[i])) for i, n in enumerate(nodes)}
        return (curv, {n: (per1[i], per2[i]) for i, n in enumerate(nodes)}) if sites else curv

    def SiteModelGradient(self, chain=0):
        """(d lnL / d r_k [categories], expected sites per category [categories], d lnL / d pi_i at fixed Q [states]) of the
        chain's current tree, after LogLike and BranchGradient (whose pre-order buffers it reads): the UNIT-rate differential
        matrix D_k = Q goes where BranchGradient keeps r_k Q (BranchGradient sets its own again), and ONE
        calculate_site_model_derivatives call reads every branch.  d lnL / d w_k is the count divided by the category weight; the
        chain rule to a gamma shape or a constrained parameterisation is the client's."""
        if not self.pre_order:
            raise ValueError("SiteModelGradient needs BeagleDivision(..., pre_order=True)")
        d, t = self.div, self.div.tree
        self.inst.set_differential_matrix(self.diffMatrixIndex, np.broadcast_to(self._RateMatrix(), (d.ncat, d.nstates, d.nstates)))
        nodes = list(t.all_down_pass)
        lengths = [min(max(t.length[n], BRLENS_MIN), BRLENS_MAX) for n in nodes]
        rc, _, rates, counts, root = self.inst.calculate_site_model_derivatives(
            self._EdgePosts(chain, nodes), self._EdgePres(nodes), [self.diffMatrixIndex] * len(nodes), [self.cijkIndex[chain]] * len(nodes),
            lengths, edges=False)
        return rates, counts, root

    def NodePosteriors(self, chain=0, sites=False, best=False):
        """{node: expected number of sites in every state [states]} for the lower end of all 2N-3 branches of the chain's current
        tree (every interior node and every tip but the root tip), after LogLike: the pre-order pass of BranchGradient, then ONE
        calculate_node_posteriors call.  sites=True adds {node: posteriors [patterns][states]}, best=True {node: (best states
        [patterns], their posteriors [patterns])}: the return value is the tuple of the dictionaries asked for, the sums first."""
        self._PreOrderPass(chain, "NodePosteriors")
        nodes = list(self.div.tree.all_down_pass)
        rc, per, states, values, sums = self.inst.calculate_node_posteriors(
            [self.condLikeIndex[chain][n] for n in nodes], [self.preOrderIndex[n] for n in nodes], [self.cijkIndex[chain]] * len(nodes),
            sites=sites, best=best)
        out = [{n: sums[i] for i, n in enumerate(nodes)}]
        if sites:
            out.append({n: per[i] for i, n in enumerate(nodes)})
        if best:
            out.append({n: (states[i], values[i]) for i, n in enumerate(nodes)})
        return out[0] if len(out) == 1 else tuple(out)

    def InsertionLogLikelihoods(self, chain=0, subtree=None, subtree_matrix=None, subtree_scale=None, sites=False):
        """{node: lnL(the chain's current tree with the subtree attached at the child end of node's branch) - lnL(the tree)} for all
        2N-3 branches, after LogLike: the pre-order pass of BranchGradient, then ONE calculate_insertion_log_likelihoods call.
        subtree: a partials buffer (or a buffer of compact tip states) that holds the clade or the query, subtree_matrix the matrix
        buffer of the pendant branch, subtree_scale the subtree's cumulative scale buffer (None: unscaled).  sites=True: (that,
        {node: per-site log ratios [patterns]})."""
        if subtree is None or subtree_matrix is None:
            raise ValueError("InsertionLogLikelihoods: subtree and subtree_matrix are required")
        self._PreOrderPass(chain, "InsertionLogLikelihoods")
        nodes = list(self.div.tree.all_down_pass)
        n = len(nodes)
        rc, per, sums = self.inst.calculate_insertion_log_likelihoods(
            self._EdgePres(nodes), self._EdgePosts(chain, nodes), [bg.BEAGLE_OP_NONE] * n, [subtree] * n, [subtree_matrix] * n,
            [bg.BEAGLE_OP_NONE if subtree_scale is None else subtree_scale] * n, [self.cijkIndex[chain]] * n, sites=sites)
        score = {node: float(sums[i]) for i, node in enumerate(nodes)}
        return (score, {node: per[i] for i, node in enumerate(nodes)}) if sites else score

    def CategoryPosteriors(self, chain=0):
        """q [categories][patterns], the posterior category probabilities of the chain's latest LogLike: site rates are
        (q * cat_rates[:, None]).sum(0)."""
        return self.inst.get_category_posteriors(self.cijkIndex[chain])

    def AutocorrelatedLogLikelihood(self, chain=0, site_patterns=None, transitions=None, jumps=None, posteriors=False):
        """ln H of the listed sites under autocorrelated rates after the chain's latest LogLike: a Markov chain with the matrix
        transitions [categories][categories] over the rate categories along the sequence, site_patterns[s] the pattern of site s,
        jumps[s] the distance between sites s - 1 and s (None: 1).  posteriors=True: (ln H, gamma [categories][sites]), the
        per-site category posteriors under the chain -- site rates are (gamma * cat_rates[:, None]).sum(0)."""
        if site_patterns is None or transitions is None:
            raise ValueError("AutocorrelatedLogLikelihood: site_patterns and transitions are required")
        rc, lnh, gamma = self.inst.autocorrelated_log_likelihood(self.cijkIndex[chain], site_patterns, transitions, jumps=jumps, posteriors=posteriors)
        return (lnh, gamma) if posteriors else lnh

    def AncestralSamplingEdges(self, chain=0):
        """The breadth-first edge list of the chain's current tree as sample_ancestral_states takes it -- (nodes, parent slots,
        post-order buffers, matrices): nodes[0] = the top interior node is slot 0, nodes[i + 1] the lower end of edge i.  The root
        tip hangs from the top across the top's own matrix (the branch the log-likelihood call integrates); level by level, so
        that the engine needs one launch per level."""
        t = self.div.tree
        top = t.root_left
        nodes, parents = [top, t.root], [0]
        mats = [self.tiProbsIndex[chain][top]]
        level = [(top, 0)]
        while level:
            below = []
            for p, slot in level:
                for n in (t.left[p], t.right[p]):
                    parents.append(slot)
                    mats.append(self.tiProbsIndex[chain][n])
                    nodes.append(n)
                    if t.left[n] >= 0:
                        below.append((n, len(nodes) - 1))
            level = below
        return nodes, parents, [self.condLikeIndex[chain][n] for n in nodes[1:]], mats

    def SampleAncestralStates(self, chain=0, seed=0, categories=False, changes=False):
        """{node: sampled states [patterns]} for every node of the chain's current tree (the root tip included), ONE draw from the
        joint posterior of all ancestral states after LogLike; no pre-order pass.  categories=True adds the sampled categories
        [patterns], changes=True {node: sampled number of substitutions on the branch above it} (the root tip: on the root branch):
        the return value is the tuple of what was asked for, the states first."""
        if self.step != 1:
            raise NotImplementedError("SampleAncestralStates: one eigen-system part per division")
        nodes, parents, posts, mats = self.AncestralSamplingEdges(chain)
        rc, states, cats, counts = self.inst.sample_ancestral_states(parents, posts, mats, self.cijkIndex[chain], seed,
                                                                     categories=categories, changes=changes)
        out = [{n: states[i] for i, n in enumerate(nodes)}]
        if categories:
            out.append(cats)
        if changes:
            out.append({n: float(counts[i]) for i, n in enumerate(nodes[1:])})
        return out[0] if len(out) == 1 else tuple(out)

    def RateMatrixCrossProducts(self, chain=0):
        """X [S][S], the cross-product matrix of the gradient in the rate matrix, for the chain's current tree after LogLike: the same
        steps as BranchGradient (start vector, pre-order list of the whole tree), then ONE calculate_cross_products call over all
        2N-3 branches with their current lengths.  sum_ij X[i,j] dQ[i,j] / d theta is the gradient in a rate-matrix parameter."""
        t = self.div.tree
        self._PreOrderPass(chain, "RateMatrixCrossProducts")
        nodes = list(t.all_down_pass)
        lengths = [min(max(t.length[n], BRLENS_MIN), BRLENS_MAX) for n in nodes]
        _, x = self.inst.calculate_cross_products(self._EdgePosts(chain, nodes), self._EdgePres(nodes),
                                                  [0] * len(nodes), [self.cijkIndex[chain]] * len(nodes), lengths)
        return x

    def LogLike(self, chain=0):
        """One full evaluation of a chain from its current dirty flags; clears them afterwards."""
        lnl = self.LaunchBEAGLELogLikeForDivision(chain)
        self.ClearTouches(chain)
        return lnl


# ------------------------------------------------------------------------------------------------
# Call recording / replay.  MrBayes' host side is C: the handful of BEAGLE calls of one generation
# cost it microseconds.  The Python twin above spends milliseconds building the same arguments, so
# throughput measurements record the exact C-ABI call sequence of an evaluation once (function
# pointer + already marshalled ctypes arguments) and replay it: the engine sees byte-for-byte the
# calls an unmodified MrBayes makes, without the interpreter in the timed path.
# ------------------------------------------------------------------------------------------------
class _RecordingLib:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self._log.append((fn, args))
            return fn(*args)
        return call


class RecordedEvaluation:
    """The C-ABI calls of one LogLike(chain), replayable with `run()` -> (return code, lnL)."""

    def __init__(self, calls):
        self.calls = calls
        self._out = None
        for fn, args in calls:
            if fn.__name__ in ("beagleCalculateEdgeLogLikelihoods", "beagleCalculateRootLogLikelihoods"):
                ref = args[-3] if fn.__name__ == "beagleCalculateEdgeLogLikelihoods" else args[-1]
                self._out = ref._obj
        if self._out is None:
            raise ValueError("the recorded evaluation contains no log-likelihood call")

    def run(self):
        rc = 0
        for fn, args in self.calls:
            r = fn(*args)
            if r != 0:
                rc = r
        return rc, self._out.value


def record_evaluation(bd: BeagleDivision, chain: int = 0, touch_all: bool = True) -> RecordedEvaluation:
    """Run bd.LogLike(chain) once while logging every C-ABI call it makes."""
    log = []
    real = bd.inst.lib
    bd.inst.lib = _RecordingLib(real, log)
    try:
        if touch_all:
            bd.TouchAllTreeNodes(chain)
        bd.LogLike(chain)
        bd.AcceptMove(chain)
    finally:
        bd.inst.lib = real
    return RecordedEvaluation(log)
