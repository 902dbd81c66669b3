"""Reference for the prefix tree of the Transformer-LM fusion in the transducer beam search (csrc/lm_tree.hip).
TEST INFRASTRUCTURE ONLY.

    Tree(S, W, nslots, Lcap, node_cap)     the state in numpy (llen, lanc, nnodes, status) and advance(src, dst, act) ->
                                           (row_node, row_pos): emoasr_lm_tree_advance restated row by row
    labels_of(tree, slot, node_label)      the label sequence a slot holds, read back through its list
    gathered_attn_ref(...)                 the gathered single-query attention in f64 / f32: decode_step_ref.attn_step_ref over the
                                           rows gathered through a slot's list
    Walk(...)                              a random walk of control words in the book kernel's style: per search a region of slots,
                                           sources drawn from the live slots, destinations from the free ones (never a slot a live
                                           row reads: the mark-and-sweep guarantee), slots recycled; the label sequence of every
                                           slot is kept on the host
    oracle_tlm_scorers / gap_cases         the end-to-end cases of tests/test_rnnt_tlm_fusion_gpu.py and their cut gaps
"""
import numpy as np

from tests.decode_step_ref import attn_step_ref

OVERLEN, POOL_FULL = 1, 2


class Tree:
    def __init__(self, S, W, nslots, Lcap, node_cap):
        self.S, self.W, self.nslots, self.Lcap, self.node_cap = S, W, nslots, Lcap, node_cap
        self.llen = np.zeros(nslots, np.int32)
        self.lanc = np.zeros((nslots, Lcap), np.int32)
        self.nnodes = np.zeros(S, np.int32)
        self.status = np.zeros(S, np.int32)

    def advance(self, src, dst, act):
        """src / dst / act: int64 [S W] -> (row_node, row_pos) int32 [S W]"""
        S, W, Lcap = self.S, self.W, self.Lcap
        row_node, row_pos = np.full(S * W, -1, np.int32), np.zeros(S * W, np.int32)
        copies = []
        for s in range(S):
            base = int(min(max(self.nnodes[s], 0), self.node_cap))
            taken = 0
            for w in range(W):
                r = s * W + w
                sl, dl = int(src[r]), int(dst[r])
                if not (act[r] != 0 and 0 <= sl < self.nslots and 0 <= dl < self.nslots):
                    continue
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
                row_node[r], row_pos[r] = node, p
                copies.append((dl, self.lanc[sl, :p].copy(), node))          # (every source is read before any list is written)
            self.nnodes[s] = base + taken
        for dl, head, node in copies:
            p = len(head)
            self.lanc[dl, :p] = head
            self.lanc[dl, p] = node
            self.llen[dl] = p + 1
        return row_node, row_pos


def labels_of(tree, slot, node_label):
    """the labels at the nodes of the slot's list, oldest first"""
    return [int(node_label[int(n)]) for n in tree.lanc[slot, :int(tree.llen[slot])]]


def gathered_attn_ref(qkv, kpool, vpool, lanc, llen, row_node, dst, H, dtype=np.float64):
    """qkv [R, 3d], kpool / vpool [nodes, d] (ONE layer), the lists AFTER advance -> (out [R, d], kpool', vpool'): row r with
    row_node[r] >= 0 writes its k / v at its node and attends over the nodes of lanc[dst[r]][:llen[dst[r]]] (its own node last);
    the other rows of out are NaN (never compared) and write nothing"""
    qkv = np.asarray(qkv, np.float64)
    kpool, vpool = np.asarray(kpool, np.float64).copy(), np.asarray(vpool, np.float64).copy()
    R, d = qkv.shape[0], qkv.shape[1] // 3
    out = np.full((R, d), np.nan, dtype)
    for r in range(R):
        if row_node[r] >= 0:
            kpool[row_node[r]], vpool[row_node[r]] = qkv[r, d:2 * d], qkv[r, 2 * d:]
    for r in range(R):
        if row_node[r] < 0:
            continue
        n = int(llen[dst[r]])
        ids = lanc[dst[r], :n]
        assert ids[-1] == row_node[r]
        out[r] = attn_step_ref(qkv[r:r + 1], kpool[ids][None], vpool[ids][None], n - 1, H, dtype=dtype)[0][0]
    return out, kpool, vpool


class Walk:
    """control words of random rounds over S searches of W rows, `per` slots each (slot s * per is the search's zero state and is
    never a destination); off: rows that are always inactive; bad: {round: [(row, "src" | "dst", value)]} plants slot numbers outside
    the pool.  next_round() -> (lab, src, dst, act) int64 [S W]; commit(row_node) tells the walk which rows really took effect."""

    def __init__(self, seed, S, W, per, V, off=(), rows=None, keep=None, bad=None):
        self.rs = np.random.RandomState(seed)
        self.S, self.W, self.per, self.V, self.off = S, W, per, V, set(off)
        self.rows = S * W if rows is None else rows          # rows >= self.rows are inactive too (a partial last search)
        self.keep = W if keep is None else keep              # live hypotheses a search keeps after a round
        self.bad = bad or {}
        self.live = [[s * per] for s in range(S)]
        self.seq = {s * per: [] for s in range(S)}            # slot -> the labels it holds
        self.round = 0

    def next_round(self):
        S, W, per, rs = self.S, self.W, self.per, self.rs
        R = S * W
        lab, src, dst, act = (np.zeros(R, np.int64) for _ in range(4))
        for s in range(S):
            free = [x for x in range(s * per + 1, (s + 1) * per) if x not in self.live[s]]
            rs.shuffle(free)
            for w in range(W):
                r = s * W + w
                lab[r] = rs.randint(0, self.V)
                if r in self.off or r >= self.rows or not free or rs.rand() < 0.15:
                    lab[r], src[r], dst[r] = rs.randint(-5, 1 << 20), rs.randint(-3, 1 << 20), rs.randint(-3, 1 << 20)   # (anything)
                    continue
                act[r], src[r], dst[r] = 1, self.live[s][rs.randint(len(self.live[s]))], free.pop()
        for r, what, value in self.bad.get(self.round, ()):
            if act[r]:
                (src if what == "src" else dst)[r] = value
        self.last = (lab, src, dst, act)
        return self.last

    def commit(self, row_node):
        lab, src, dst, act = self.last
        for s in range(self.S):
            grown = []
            for r in range(s * self.W, (s + 1) * self.W):
                if row_node[r] >= 0:
                    self.seq[int(dst[r])] = self.seq[int(src[r])] + [int(lab[r])]
                    grown.append(int(dst[r]))
            pool = self.live[s] + grown
            self.rs.shuffle(pool)
            self.live[s] = sorted(set(pool[:self.keep])) or [s * self.per]
        self.round += 1


# ---- the end-to-end cases --------------------------------------------------------------------------------------------------------
ELENS = (12, 5, 0)
WIDTHS, MUS = (2, 4), (0.3, 1.0)


def oracle_tlm_scorers(sd, cfg, lm_sd, lm_cfg, eouts):
    """(scorer, lm_scorer) of tests/rnnt_fusion_ref.search: the oracle transducer on eouts [1, T, d] and oracle.decoder.lm_predict"""
    import torch

    from oracle import decoder as od
    from tests import rnnt_fusion_ref as F
    scorer = F.oracle_scorers(sd, cfg, None, eouts)[0]

    def lm_scorer(seq):
        return od.lm_predict(lm_sd, lm_cfg, torch.tensor([list(seq)]), torch.tensor([len(seq)]))[0].numpy().astype(np.float32)
    return scorer, lm_scorer


def gap_cases(sd, cfg, lm_sd, lm_cfg, eouts):
    """eouts [>= 2, >= 12, d] f32 on the host -> {(b, W, mu): (min_gap, fused hyps, plain hyps)} of the eight cases"""
    import torch

    from tests import rnnt_fusion_ref as F
    out = {}
    with torch.no_grad():
        for b in (0, 1):
            sc, lm = oracle_tlm_scorers(sd, cfg, lm_sd, lm_cfg, eouts[b:b + 1, :ELENS[b]])
            for W in WIDTHS:
                plain = F.search(sc, lm, 0.0, ELENS[b], W)[0]
                for mu in MUS:
                    hyps, _, ev = F.search(sc, lm, mu, ELENS[b], W)
                    out[(b, W, mu)] = (float(ev.min_gap), hyps, plain)
    return out
