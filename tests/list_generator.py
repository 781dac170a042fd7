"""Seeded random operation lists for tests/test_operation_lists.py.  Pure numpy: no engine, no reference arithmetic beyond float64.

    case = make_case(family, seed, S, K, P, double_precision, per_category, missing_is_one)

A *case* is everything one run needs: the instance dimensions, the source data (compact tips, one tip given as partials, dense
source buffers, transition matrices), a sequence of *calls* and the buffers / exponent buffers to read at the end.  A call is an
int32 [n][7] operation array in BeagleOperation field order (destination, scale write, scale read, child 1, matrix 1, child 2,
matrix 2) with its cumulative index, the setter calls that come in front of it (`pre`: a transition matrix or a tip replaced between two
lists), whether the caller reads a result before issuing it (`flush`: what lets a queueing engine see this list on its own), and what
a path recogniser must make of it (`expect`: "path", "forked", "not_path" or None).

Buffer layout, the same at every shape (LAYOUT below): compact tips 0 ... 4, the tip given as partials 5, dense sources 6, 7, 8, results
9 ... 48; 12 matrices; node exponent buffers 0 ... 47, cumulative buffers 48 and 49.

Families (FAMILIES; every case records its family and its variant, so that a failure says which):
  tree            a random binary tree over 3 ... 12 leaves drawn with repetition from all nine sources (one buffer may be both children
                  of an operation), its operations in a random topological order
  forest          two to four such trees, their operations interleaved
  path            a small tree (the prologue: it leaves results and written exponent buffers to read), a read, then a root-ward chain
                  of 2 ... 20 operations: every operation reads its predecessor and one operand from outside the list.  Variants that
                  a path recogniser must refuse: "outside_written_later" (an outside operand is the destination of a later operation
                  of the chain) and "scale_twice" (an exponent buffer named by two operations of the list)
  forked          the same with two or three arms that join, one saved result at a time, arms that read exponent buffers
                  included; the variant "two_saved" starts a third arm while the first still waits
  dag             results read by several later operations
  hazard          few result and exponent buffers for many operations: destinations written twice, written after they were read,
                  exponent buffers written twice, written then read, read then written (case.hazards says which occurred)
  small_subtrees  a tree (or two) over compact tips alone, with no operation that divides by stored exponents, then WITHOUT a read a
                  second call that reads the result of a subtree of two to four tips as a child ("read_child"), after one of that subtree's
                  matrices ("matrix") or tips ("tip") was replaced, or that overwrites the result itself and reads it ("overwrite")
  relabelled      a prologue, then one structural list issued two to four times with result buffers, sources, matrices and exponent
                  buffers permuted, once more unchanged, and once more unchanged but for the cumulative index
  queued          two to four calls, no read between them: later calls are independent of the earlier ones, read their results,
                  overwrite their operands and results, or reuse their exponent buffers

Scale modes per operation are none, SCALE_WRITE and SCALE_READ (of a buffer written earlier in the case); calls come with and without
a cumulative buffer.  Matrices are row-stochastic, a third of them times 0.02; dense sources are (0.05 ... 0.95) x 2^(-20 ... 0) per
column, rounded to the storage type first, one pattern of one of them all zero (a dead column travels up every list that reads it);
tips carry the missing code S.

Keeping values in range is a CONDITION of a case, not a measurement: while it draws, the generator runs every operation in float64 on
the values as an engine stores them (divided by the exponents written or read -- per (category, pattern) column with `per_category`, per
pattern otherwise) and draws the operation's matrices and scale mode again when a live column maximum of its result leaves
[2^-100, 2^60] (single precision) / [2^-900, 2^900] (double), or no column is live -- the result as stored, and the product in front of
the exponents too: a SCALE_WRITE of two operands at 2^-80 stores a column in [0.5, 1) that the single-precision kernels have formed at
2^-160, below every float.  Without the condition a SCALE_READ of unrelated exponents overflows and both sides of a comparison hold
NaN.  After six failed draws the operation becomes a SCALE_WRITE into an unused buffer; if that is out of range too (the operands'
doing: no draw helps), the whole case is drawn again and every draw of the abandoned attempt counts as re-drawn.  case.draws /
case.redraws count them.

Re-drawn share over the committed seed set (every family x every shape of tests/test_operation_lists.py x seeds 0 ... 19, counted and
printed per shape by test_redrawn_share there, which asserts it below a tenth): 1 422 of 47 446 draws, 3.0 %; the most at
(4, 1, 64) single precision, 6.3 %; none in double precision.
"""
import numpy as np

from tests.operation_reference import dense_tip

NONE = -1
FAMILIES = ("tree", "forest", "path", "forked", "dag", "hazard", "small_subtrees", "relabelled", "queued")


class LAYOUT:
    COMPACT = (0, 1, 2, 3, 4)
    TIP_PARTIALS = 5
    DENSE = (6, 7, 8)
    FIRST_RESULT, N_RESULTS = 9, 40
    TIPS = 6                            # tip buffers (compact and partials)
    N_BUFFERS = 49
    N_MATRICES = 12
    N_NODE_SCALES = 48
    CUMULATIVE = (48, 49)
    N_SCALES = 50
    DEAD_SOURCE, DEAD_PATTERN = 7, 3     # dense source 7 is zero at pattern 3 in every category


SOURCES = LAYOUT.COMPACT + (LAYOUT.TIP_PARTIALS,) + LAYOUT.DENSE


class Call:
    def __init__(self, ops, cum, flush=False, pre=(), expect=None):
        self.ops = np.asarray(ops, dtype=np.int32).reshape(-1, 7)
        self.cum = int(cum)
        self.flush = bool(flush)
        self.pre = list(pre)            # ("matrix", index, [K][S][S]) / ("tip", index, int32 [P])
        self.expect = expect

    def literal(self):
        pre = ["(%r, %d, ...)" % (a[0], a[1]) for a in self.pre]
        return "Call(%s, cum=%d, flush=%s, pre=[%s], expect=%r)" % (self.ops.tolist(), self.cum, self.flush, ", ".join(pre), self.expect)


class Case:
    """see the module docstring; `tips` [5] int32 [P], `tip_partials` [P][S], `dense` {buffer: [K][P][S]}, `matrices` [12][K][S][S]"""

    def describe(self):
        head = "family %s (%s) seed %d, %d states x %d categories x %d patterns, %s, exponents per %s" % (
            self.family, self.variant, self.seed, self.S, self.K, self.P, "fp64" if self.double_precision else "fp32",
            "(category, pattern)" if self.per_category else "pattern")
        return "\n".join([head] + ["  " + c.literal() for c in self.calls] +
                         ["  read buffers %s, exponent buffers %s" % (self.read_buffers, self.read_scales)])

    def total_operations(self):
        return sum(len(c.ops) for c in self.calls)

    def shortened(self):
        """the same case without the last operation of its last call (an emptied call goes), or None; what is read at the end
        is what the remaining calls write"""
        calls = [Call(c.ops.copy(), c.cum, c.flush, c.pre, c.expect) for c in self.calls]
        while calls and len(calls[-1].ops) == 0:
            calls.pop()
        if not calls or sum(len(c.ops) for c in calls) <= 1:
            return None
        calls[-1].ops = calls[-1].ops[:-1]
        calls[-1].expect = None
        if len(calls[-1].ops) == 0:
            calls.pop()
        out = Case.__new__(Case)
        out.__dict__.update(self.__dict__)
        out.calls = calls
        out.read_buffers = sorted({int(o[0]) for c in calls for o in c.ops})
        out.read_scales = sorted({int(o[1]) for c in calls for o in c.ops if o[1] != NONE})
        return out


def _stored(a, double_precision):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float64 if double_precision else np.float32).astype(np.float64))


class Infeasible(Exception):
    """no draw of matrices and scale mode brings this operation into range: its operands are too small or too large"""


class _Builder:
    def __init__(self, family, seed, S, K, P, double_precision, per_category, missing_is_one, attempt=0):
        self.rng = np.random.default_rng([FAMILIES.index(family), seed, S, K, P, int(double_precision), attempt])
        self.S, self.K, self.P, self.dbl, self.per_category, self.seed = S, K, P, double_precision, per_category, seed
        rng = self.rng
        c = Case()
        c.family, c.seed, c.S, c.K, c.P, c.double_precision, c.per_category = family, seed, S, K, P, double_precision, per_category
        c.missing_is_one = self.missing_is_one = missing_is_one
        c.variant = "-"
        c.tips = [rng.integers(0, S + 1, size=P).astype(np.int32) for _ in LAYOUT.COMPACT]
        c.tip_partials = _stored(rng.random((P, S)) * 0.9 + 0.05, double_precision)
        c.dense = {}
        for b in LAYOUT.DENSE:
            # (a column is what the layout rescales as one: with an exponent per pattern, a spread between the categories of a pattern
            #  stays in every result above it and multiplies from operation to operation until the smallest category leaves the range)
            ex = rng.integers(-20, 1, size=(K if per_category else 1, P, 1)).astype(np.float64)
            d = (rng.random((K, P, S)) * 0.9 + 0.05) * np.exp2(ex)
            if b == LAYOUT.DEAD_SOURCE:
                d[:, LAYOUT.DEAD_PATTERN, :] = 0.0
            c.dense[b] = _stored(d, double_precision)
        c.matrices = [self.matrix(0.02 if m % 3 == 2 else 1.0) for m in range(LAYOUT.N_MATRICES)]
        c.calls, c.hazards = [], set()
        c.draws = c.redraws = 0
        self.case = c
        self.lo, self.hi = (2.0 ** -900, 2.0 ** 900) if double_precision else (2.0 ** -100, 2.0 ** 60)
        # the float64 interpreter's state: values as stored, exponent buffers, matrices
        self.states = {b: c.tips[b] for b in LAYOUT.COMPACT}
        self.V = {b: dense_tip(c.tips[b], S, K) for b in LAYOUT.COMPACT}
        self.V[LAYOUT.TIP_PARTIALS] = np.broadcast_to(c.tip_partials, (K, P, S)).copy()
        self.V.update({b: c.dense[b].copy() for b in LAYOUT.DENSE})
        self.far = {b: self.is_far(v) for b, v in self.V.items()}
        self.M = [m.copy() for m in c.matrices]
        self.X = {}
        self.free_results = list(range(LAYOUT.FIRST_RESULT, LAYOUT.FIRST_RESULT + LAYOUT.N_RESULTS))
        self.free_scales = list(range(LAYOUT.N_NODE_SCALES))
        self.written_scales = []
        self.results = []               # result buffers that hold a value, in the order they were first written
        self.rows = []                  # the call being built

    def is_far(self, v):
        """a live column maximum beyond the fourth root of the range's ends: the product of two such operands may leave it"""
        col = v.max(axis=2)
        col = col[col > 0]
        return bool(col.size and (col.min() < self.lo ** 0.25 or col.max() > self.hi ** 0.25))

    # ---- sources -----------------------------------------------------------------------------------------------------------------
    def matrix(self, factor):
        m = self.rng.random((self.K, self.S, self.S)) + 0.05
        return _stored(m / m.sum(axis=2, keepdims=True) * factor, self.dbl)

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def leaf(self):
        return self.pick(SOURCES)

    def new_result(self):
        return self.free_results.pop(int(self.rng.integers(len(self.free_results))))

    def new_scale(self):
        return self.free_scales.pop(int(self.rng.integers(len(self.free_scales))))

    # ---- one operation -------------------------------------------------------------------------------------------------------------
    def factor(self, m, c):
        f = np.einsum("kij,kcj->kci", self.M[m], self.V[c])
        if self.missing_is_one and c in self.states:
            f[:, self.states[c] >= self.S, :] = 1.0
        return f

    def compute(self, c1, m1, c2, m2, mode, sidx):
        """-> (stored result, exponents or None) in float64, or None when out of range"""
        raw = self.factor(m1, c1) * self.factor(m2, c2)
        e = None
        if mode == "write":
            mx = raw.max(axis=2) if self.per_category else np.broadcast_to(raw.max(axis=(0, 2)), (self.K, self.P))
            e = np.where(mx > 0, np.frexp(mx)[1], 0).astype(np.int64)
        elif mode == "read":
            e = self.X[sidx]
        val = raw if e is None else np.ldexp(raw, -e[:, :, None].astype(np.int32))
        for a in (raw, val):                     # (the product before the exponents are applied, and what is stored)
            col = a.max(axis=2)
            live = col > 0
            if not live.any() or not np.isfinite(a).all() or col[live].min() < self.lo or col[live].max() > self.hi:
                return None
        return val, (e if mode == "write" else None)

    def emit(self, dst, c1, c2, modes=("none", "write", "read"), write_to=None, read_from=None, force=None):
        """Draw matrices and a scale mode for dst = f(c1, c2) until the result is in range; commit it to the interpreter and append
        the row.  write_to / read_from: the exponent buffers to choose from (default: an unused one / every buffer written so far).
        force = (mode, buffer): this mode first; the draw is free again once it failed."""
        rng, c = self.rng, self.case
        assert dst != c1 and dst != c2
        for attempt in range(7):
            c.draws += 1
            m1, m2 = int(rng.integers(LAYOUT.N_MATRICES)), int(rng.integers(LAYOUT.N_MATRICES))
            fresh = None
            if force is not None and attempt < 3 and not (force[0] == "read" and force[1] not in self.X):
                mode, sidx = force
            elif attempt == 6:
                mode, sidx = "write", None
            else:
                readable = self.written_scales if read_from is None else [s for s in read_from if s in self.X]
                allowed = [m for m in modes if m != "read" or readable]
                # (operands far from 1 call for a rescale, as in a client's dynamic scheme: SCALE_WRITE three times in four then)
                far = any(self.far[c] for c in (c1, c2))
                mode = "write" if far and "write" in allowed and rng.random() < 0.75 else self.pick(allowed)
                sidx = None
                if mode == "read":
                    sidx = self.pick(readable)
                elif mode == "write" and write_to:
                    sidx = self.pick(write_to)
            if mode == "write" and sidx is None:
                sidx = fresh = self.free_scales[int(rng.integers(len(self.free_scales)))]
            got = self.compute(c1, m1, c2, m2, mode, sidx)
            if got is None:
                c.redraws += 1
                continue
            val, e = got
            if fresh is not None:
                self.free_scales.remove(fresh)
            self.V[dst] = val
            self.far[dst] = self.is_far(val)
            if mode == "write":
                self.X[sidx] = e
                if sidx not in self.written_scales:
                    self.written_scales.append(sidx)
            if dst not in self.results:
                self.results.append(dst)
            row = [dst, sidx if mode == "write" else NONE, sidx if mode == "read" else NONE, c1, m1, c2, m2]
            self.rows.append(row)
            return row
        raise Infeasible()

    def end_call(self, cum=None, **kw):
        if cum is None:
            cum = self.pick((NONE, NONE) + LAYOUT.CUMULATIVE)
        self.case.calls.append(Call(self.rows, cum, **kw))
        self.rows = []

    def finish(self):
        c = self.case
        c.read_buffers = sorted({int(o[0]) for call in c.calls for o in call.ops})
        c.read_scales = sorted({int(o[1]) for call in c.calls for o in call.ops if o[1] != NONE})
        c.hazards = hazards_of(c)
        return c

    # ---- shapes ------------------------------------------------------------------------------------------------------------------
    def tree_shape(self, leaves, first=0):
        """join two roots until one is left -> [(node, child, child)], a child ("L", buffer) or ("N", node); nodes first, first + 1 ..."""
        roots = [("L", b) for b in leaves]
        nodes = []
        while len(roots) > 1:
            i, j = sorted(self.rng.choice(len(roots), size=2, replace=False).tolist())
            node = first + len(nodes)
            nodes.append((node, roots[i], roots[j]))
            del roots[j]
            roots[i] = ("N", node)
        return nodes

    def topological(self, nodes, post_order=False):
        """a random order in which every node follows its children"""
        if post_order:
            return list(nodes)
        left, done, out = list(nodes), set(), []
        while left:
            ready = [n for n in left if all(ch[0] == "L" or ch[1] in done for ch in n[1:])]
            n = self.pick(ready)
            left.remove(n)
            done.add(n[0])
            out.append(n)
        return out

    def emit_nodes(self, nodes, have=None, **kw):
        dst = dict(have or {})
        for node, a, b in nodes:
            dst[node] = self.new_result()
            self.emit(dst[node], *(ch[1] if ch[0] == "L" else dst[ch[1]] for ch in (a, b)), **kw)
        return dst

    def random_leaves(self, n, pool=SOURCES):
        leaves = [self.pick(pool) for _ in range(n)]
        if self.rng.random() < 0.3:
            leaves[1] = leaves[0]
        return leaves

    def prologue(self):
        """a small tree that leaves results and written exponent buffers for the lists behind it to read"""
        nodes = self.tree_shape(self.random_leaves(int(self.rng.integers(3, 6))))
        first = self.emit_nodes(nodes[:1], modes=("write",))
        self.emit_nodes(nodes[1:], modes=("write", "write", "none"), have=first)
        self.end_call()

    # ---- families ----------------------------------------------------------------------------------------------------------------
    def tree(self):
        nodes = self.tree_shape(self.random_leaves(int(self.rng.integers(3, 13))))
        self.emit_nodes(self.topological(nodes, post_order=self.rng.random() < 0.25))
        self.end_call()

    def forest(self):
        ntrees = int(self.rng.integers(2, 5))
        nodes = []
        for _ in range(ntrees):
            nodes += self.tree_shape(self.random_leaves(int(self.rng.integers(3, 8))), first=len(nodes))
        self.emit_nodes(self.topological(nodes))
        self.end_call()

    def chain(self, length, outside, start=None, **kw):
        """`length` operations, each reading its predecessor (the first one `start`, or two outside operands) and an outside operand"""
        prev = start
        for _ in range(length):
            dst = self.new_result()
            sib = self.pick(outside)
            first = self.pick(outside) if prev is None else prev
            pair = (first, sib) if self.rng.random() < 0.5 else (sib, first)
            self.emit(dst, *pair, **kw)
            prev = dst
        return prev

    def path(self):
        self.prologue()
        outside = list(SOURCES) + list(self.results)
        readable = list(self.written_scales)
        variant = ("ok", "outside_written_later", "ok", "scale_twice")[self.seed % 4]         # (by seed: any eight seeds hold them all)
        n = int(self.rng.integers(2, 21))
        kw = dict(read_from=readable)
        if variant == "ok":
            self.chain(n, outside, **kw)
        elif variant == "outside_written_later":
            n = max(n, 3)
            i = int(self.rng.integers(1, n - 1))
            j = int(self.rng.integers(i + 1, n))
            victim = self.pick(self.results)
            prev = self.chain(i, outside, **kw)
            dst = self.new_result()
            self.emit(dst, prev, victim, **kw)
            prev = self.chain(j - i - 1, [b for b in outside if b != victim], start=dst, **kw)
            self.emit(victim, prev, self.pick([b for b in outside if b != victim]), **kw)
            self.chain(n - j - 1, outside, start=victim, **kw)
        else:
            i = int(self.rng.integers(0, n - 1))
            j = int(self.rng.integers(i + 1, n))
            prev = self.chain(i, outside, **kw) if i else None
            s = self.new_scale()
            prev = self.chain(1, outside, start=prev, force=("write", s), **kw)
            ok = self.rows[-1][1] == s
            prev = self.chain(j - i - 1, outside, start=prev, **kw)
            prev = self.chain(1, outside, start=prev, force=(self.pick(("write", "read")), s), **kw)
            ok = ok and s in self.rows[-1][1:3]
            self.chain(n - j - 1, outside, start=prev, **kw)
            if not ok:
                variant = "ok"               # (the forced modes were out of range: what was drawn instead is a plain path)
        self.case.variant = variant
        self.end_call(flush=True, expect="path" if variant == "ok" else "not_path")

    def forked(self):
        self.prologue()
        outside = list(SOURCES) + list(self.results)
        kw = dict(read_from=list(self.written_scales))
        variant = ("two_arms", "three_arms", "two_saved")[self.seed % 3]
        L = lambda hi: int(self.rng.integers(1, hi + 1))
        if variant == "two_saved":
            a, b, c = self.chain(L(4), outside, **kw), self.chain(L(4), outside, **kw), self.chain(L(4), outside, **kw)
            d = self.new_result()
            self.emit(d, c, b, **kw)
            prev = self.chain(L(2) - 1, outside, start=d, **kw)
            d = self.new_result()
            self.emit(d, prev, a, **kw)
            self.chain(L(3) - 1, outside, start=d, **kw)
        else:
            saved = self.chain(L(5), outside, **kw)
            for arm in range(2 if variant == "two_arms" else 3)[1:]:
                prev = self.chain(L(5), outside, **kw)
                d = self.new_result()
                self.emit(d, *((prev, saved) if self.rng.random() < 0.5 else (saved, prev)), **kw)
                saved = self.chain(L(4) - 1, outside, start=d, **kw)
        self.case.variant = variant
        self.end_call(flush=True, expect="not_path" if variant == "two_saved" else "forked")

    def dag(self):
        mine = []
        for _ in range(int(self.rng.integers(2, 25))):
            ch = [self.pick(mine) if mine and self.rng.random() < 0.6 else self.leaf() for _ in (0, 1)]
            dst = self.new_result()
            self.emit(dst, *ch)
            mine.append(dst)
        self.end_call()

    def hazard(self):
        pool = [self.new_result() for _ in range(4)]
        spool = [self.new_scale() for _ in range(3)]
        for _ in range(int(self.rng.integers(4, 25))):
            have = [b for b in pool if b in self.V]
            ch = [self.pick(have) if have and self.rng.random() < 0.6 else self.leaf() for _ in (0, 1)]
            dst = self.pick([b for b in pool if b not in ch])
            self.emit(dst, *ch, write_to=spool, read_from=spool)
        self.end_call()

    def small_subtrees(self):
        ntrees = 1 if self.rng.random() < 0.7 else 2
        nodes = []
        for _ in range(ntrees):
            nodes += self.tree_shape([self.pick(LAYOUT.COMPACT) for _ in range(int(self.rng.integers(5, 12)))], first=len(nodes))
        order = self.topological(nodes, post_order=self.rng.random() < 0.5)
        dst = self.emit_nodes(order, modes=("none", "write"))
        self.end_call()
        # the tips below every node; a small subtree: two to four of them
        ntips, below = {}, {}
        for node, a, b in nodes:
            ntips[node] = sum(1 if ch[0] == "L" else ntips[ch[1]] for ch in (a, b))
            below[node] = [node] + [x for ch in (a, b) if ch[0] == "N" for x in below[ch[1]]]
        small = [n for n in ntips if 2 <= ntips[n] <= 4]
        target = self.pick(small)
        rows = {int(r[0]): r for r in self.case.calls[0].ops}
        inside = [rows[dst[n]] for n in below[target]]
        variant = ("read_child", "matrix", "tip", "overwrite")[self.seed % 4]
        pre = []
        if variant == "matrix":
            m = int(self.pick([int(r[q]) for r in inside for q in (4, 6)]))
            self.M[m] = self.matrix(1.0)
            pre.append(("matrix", m, self.M[m].copy()))
        elif variant == "tip":
            t = int(self.pick([int(r[q]) for r in inside for q in (3, 5) if int(r[q]) in LAYOUT.COMPACT]))
            states = self.rng.integers(0, self.S + 1, size=self.P).astype(np.int32)
            self.V[t] = dense_tip(states, self.S, self.K)
            self.far[t] = False
            self.states[t] = states
            pre.append(("tip", t, states))
        elif variant == "overwrite":
            self.emit(dst[target], self.leaf(), self.leaf())
        d = self.new_result()
        self.emit(d, dst[target], self.leaf())
        self.chain(int(self.rng.integers(0, 3)), list(SOURCES), start=d)
        self.case.variant = variant
        self.end_call(pre=pre)

    def relabelled(self):
        self.prologue()
        results = [self.new_result() for _ in range(8)]
        # the structure: symbolic results 0 ..., symbolic sources by kind, the scale mode of every operation
        n = int(self.rng.integers(3, 9))
        struct = []
        for o in range(n):
            ch = [("R", int(self.rng.integers(o))) if o and self.rng.random() < 0.6 else self.pick((("C", 0), ("C", 1), ("C", 2), ("D", 0), ("D", 1), ("T", 0)))
                  for _ in (0, 1)]
            struct.append((ch[0], ch[1], self.pick(("none", "write", "read"))))
        dense_like = list(LAYOUT.DENSE) + [b for b in self.results if b not in results]
        ncalls = int(self.rng.integers(2, 5))
        for issue in range(ncalls):
            rmap = self.rng.permutation(results).tolist()
            cmap = self.rng.permutation(LAYOUT.COMPACT).tolist()
            dmap = self.rng.permutation(dense_like).tolist()
            name = {"R": lambda i: rmap[i], "C": lambda i: cmap[i], "D": lambda i: dmap[i], "T": lambda i: LAYOUT.TIP_PARTIALS}
            for o, (a, b, mode) in enumerate(struct):
                force = (mode, None if mode != "read" else self.pick(self.written_scales))
                self.emit(rmap[o], name[a[0]](a[1]), name[b[0]](b[1]), modes=(mode, "write"), force=force)
            self.end_call()
        last = self.case.calls[-1]
        self.replay(last, last.cum)                                  # unchanged: the exact plan again
        self.replay(last, self.pick([c for c in (NONE,) + LAYOUT.CUMULATIVE if c != last.cum]))      # ... but for the cumulative index
        self.case.variant = "%d issues" % ncalls

    def replay(self, call, cum):
        """the rows of `call` once more, as they are (redrawn like any other operation if the values have moved out of range)"""
        for r in call.ops.tolist():
            mode = "write" if r[1] != NONE else ("read" if r[2] != NONE else "none")
            c = self.case
            c.draws += 1
            got = self.compute(r[3], r[4], r[5], r[6], mode, r[1] if mode == "write" else r[2])
            if got is None:
                c.redraws += 1
                self.emit(r[0], r[3], r[5])
                continue
            self.V[r[0]] = got[0]
            self.far[r[0]] = self.is_far(got[0])
            if mode == "write":
                self.X[r[1]] = got[1]
            self.rows.append(r)
        self.end_call(cum=cum)

    def queued(self):
        ncalls = int(self.rng.integers(2, 5))
        read_by, wrote, scales = [], [], []          # what earlier calls read (results only), wrote, and their exponent buffers
        for q in range(ncalls):
            kind = "independent" if q == 0 else self.pick(("independent", "reads", "overwrites", "reuses_scales"))
            mine = []
            for o in range(int(self.rng.integers(2, 8))):
                pool = mine + (wrote if kind == "reads" else [])
                ch = [self.pick(pool) if pool and self.rng.random() < 0.6 else self.leaf() for _ in (0, 1)]
                victims = [b for b in read_by + wrote if b not in ch]
                dst = self.pick(victims) if kind == "overwrites" and victims and self.rng.random() < 0.6 else self.new_result()
                kw = dict(write_to=scales, read_from=scales) if kind == "reuses_scales" and scales else {}
                row = self.emit(dst, *ch, **kw)
                mine.append(dst)
                read_by += [b for b in ch if b >= LAYOUT.FIRST_RESULT]
                if row[1] != NONE and row[1] not in scales:
                    scales.append(row[1])
            wrote += [b for b in mine if b not in wrote]
            self.case.variant = (self.case.variant + "," + kind).lstrip("-,")
            self.end_call()


def hazards_of(case):
    """which of the five in-list hazards the calls of a case hold: {"waw", "war", "scale_ww", "scale_wr", "scale_rw"}"""
    out = set()
    for call in case.calls:
        written, read, sw, sr = set(), set(), set(), set()
        for d, w, r, c1, _, c2, _ in call.ops.tolist():
            if d in written:
                out.add("waw")
            if d in read:
                out.add("war")
            if w != NONE:
                out |= ({"scale_ww"} if w in sw else set()) | ({"scale_rw"} if w in sr else set())
                sw.add(w)
            if r != NONE:
                if r in sw:
                    out.add("scale_wr")
                sr.add(r)
            written.add(d)
            read |= {c1, c2}
    return out


def make_case(family, seed, S, K, P, double_precision=False, per_category=False, missing_is_one=True):
    """The case of (family, seed) at this shape: deterministic -- the same arguments give the same case.  per_category and missing_is_one
    say how the values an engine stores are to be followed (the range condition): an exponent per (category, pattern) column or per
    pattern; a missing tip state as the factor 1 (BEAGLE's padded matrix column) or as the sum of the matrix row (the tip as the dense
    vector of ones) -- one and the same only where rows sum to one."""
    wasted = 0
    for attempt in range(100):
        b = _Builder(family, int(seed), S, K, P, bool(double_precision), bool(per_category), bool(missing_is_one), attempt)
        try:
            getattr(b, family)()
        except Infeasible:
            wasted += b.case.draws               # (the whole attempt counts as re-drawn)
            continue
        case = b.finish()
        case.draws += wasted
        case.redraws += wasted
        return case
    raise AssertionError("no case in range in 100 attempts")
