"""Reference for the prefix tree under the batched LAS search (emoasr_lm_tree_advance_beam, csrc/lm_tree.hip).
TEST INFRASTRUCTURE ONLY.

    BeamTree(S, W, Lcap, node_cap)         tests/lm_tree_ref.Tree with 2 S W slots in two halves and advance_beam(ids, parent, state,
                                           src_base, dst_base) -> (row_node, row_pos, lab, dst): the kernel restated row by row.
                                           Nodes are handed out in row order, as the kernel hands them out: everything compares exactly
    BookWalk(seed, S, W, V, ...)           a random lockstep walk in emoasr_beam_update_batch's style: per step ids / parent / state
                                           (global parent rows inside the search, a shrinking n_alive, finished searches, junk in the
                                           dead rows, planted parents outside the search), with every slot's label sequence kept on
                                           the host
"""
import numpy as np

from tests import lm_tree_ref as T

OVERLEN, POOL_FULL = T.OVERLEN, T.POOL_FULL


def halves(step, nb):
    """(src_base, dst_base) of a step: (0, S W) on even steps, (S W, 0) on odd ones"""
    return (0, nb) if step % 2 == 0 else (nb, 0)


class BeamTree(T.Tree):
    def __init__(self, S, W, Lcap, node_cap):
        super().__init__(S, W, 2 * S * W, Lcap, node_cap)

    def advance_beam(self, ids, parent, state, src_base, dst_base):
        """ids / parent int [S W], state int [S, 4] (pos, n_alive, n_results, done) -> (row_node, row_pos int32 [S W], lab, dst
        int64 [S W])"""
        S, W, Lcap = self.S, self.W, self.Lcap
        nb = S * W
        assert 0 <= src_base and 0 <= dst_base and max(src_base, dst_base) + nb <= self.nslots and abs(src_base - dst_base) >= nb
        row_node, row_pos = np.full(nb, -1, np.int32), np.zeros(nb, np.int32)
        lab, dst = np.zeros(nb, np.int64), np.full(nb, -1, np.int64)
        copies = []
        for s in range(S):
            R = s * W
            na = 0 if state[s][3] else min(max(int(state[s][1]), 0), W)
            base = int(min(max(self.nnodes[s], 0), self.node_cap))
            taken = 0
            for w in range(na):
                r = R + w
                pr = int(parent[r])
                sl, dl = src_base + (pr if R <= pr < R + W else R), dst_base + r
                p = int(self.llen[sl])
                if p < 0:
                    continue
                if p >= Lcap:
                    self.status[s] |= OVERLEN
                    continue
                if base + taken >= self.node_cap:
                    self.status[s] |= POOL_FULL
                    continue
                node = s * self.node_cap + base + taken
                taken += 1
                row_node[r], row_pos[r], lab[r], dst[r] = node, p, int(ids[r]), dl
                copies.append((dl, self.lanc[sl, :p].copy(), node))          # (every source is read before any list is written)
            self.nnodes[s] = base + taken
        for dl, head, node in copies:
            p = len(head)
            self.lanc[dl, :p] = head
            self.lanc[dl, p] = node
            self.llen[dl] = p + 1
        return row_node, row_pos, lab, dst


class BookWalk:
    """per step next_step() -> (ids int32 [S W], parent int32 [S W], state int32 [S, 4]); commit(row_node) records which rows took a
    node.  n_alive of search s starts at 1 (step 0: one hypothesis, parent = the search's row 0) and is drawn anew every step from
    alive (a callable (step, search) -> count, which may lie outside 0 .. W, or None: random in 0 .. W, shrinking towards the end); `done` searches are finished from
    the start; bad: {step: [(row, parent value)]} plants parents outside the search; dead rows carry junk."""

    def __init__(self, seed, S, W, V, done=(), alive=None, bad=None, shrink_from=None):
        self.rs = np.random.RandomState(seed)
        self.S, self.W, self.V, self.done, self.alive, self.bad = S, W, V, set(done), alive, bad or {}
        self.shrink_from = shrink_from
        self.step = 0
        self.seq = [dict() for _ in range(2)]          # half -> {row: labels}: the prefixes the slots of a half hold

    def next_step(self):
        S, W, rs, i = self.S, self.W, self.rs, self.step
        nb = S * W
        ids = rs.randint(-5, 1 << 20, nb).astype(np.int32)                # junk everywhere, overwritten for the live rows
        parent = rs.randint(-3, 1 << 20, nb).astype(np.int32)
        state = np.zeros((S, 4), np.int32)
        for s in range(S):
            R = s * W
            if i == 0:
                na = 1
            elif self.alive is not None:
                na = int(self.alive(i, s))
            else:
                hi = W if self.shrink_from is None or i < self.shrink_from else max(0, W - (i - self.shrink_from + 1))
                na = int(rs.randint(0, hi + 1))
            prev = [r for r in range(R, R + W) if r in self.seq[i % 2]]      # slots of the source half that hold a prefix
            if i > 0 and not prev:
                na = 0                                  # nothing to descend from: the search has no live row
            state[s] = (i, na, int(rs.randint(0, W + 1)), 1 if s in self.done else 0)
            for w in range(min(max(na, 0), W)):         # (a count outside 0 .. W is clamped by the kernel)
                ids[R + w] = rs.randint(0, self.V)
                parent[R + w] = R if i == 0 else prev[rs.randint(len(prev))]
        for r, value in self.bad.get(i, ()):
            parent[r] = value
        self.last = (ids, parent, state)
        return self.last

    def commit(self, row_node):
        ids, parent, state = self.last
        S, W, i = self.S, self.W, self.step
        src, dst = self.seq[i % 2], self.seq[1 - i % 2]
        for s in range(S):
            R = s * W
            for w in range(W):
                r = R + w
                if row_node[r] >= 0:
                    pr = int(parent[r])
                    pr = pr if R <= pr < R + W else R
                    dst[r] = src.get(pr, []) + [int(ids[r])]
        self.step += 1


def labels(tree, slot, node_label):
    return T.labels_of(tree, slot, node_label)
