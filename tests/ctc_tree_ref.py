"""Reference for the prefix tree under the fused CTC search (emoasr_lm_tree_advance_rec, csrc/lm_tree.hip).
TEST INFRASTRUCTURE ONLY.

    RecTree(S, W, slots, Lcap, node_cap)   tests/lm_tree_ref.Tree whose slots are the rows of the LM pool (search s owns the slots
                                           s * slots ..) with advance_rec(rec, n, lm_weight=None) -> (row_node, row_pos, lab, dst):
                                           the kernel restated record by record.  Nodes are handed out in record order here; the
                                           kernel hands them out in any order, so a comparison goes through the label lists
    record_frames(lp, top, W, ...)         tests/ctc_beam_lm_ref.search_by_slots as a generator: the same loop, yielding after the
                                           root and after every frame the records (node, parent, token, src slot, dst slot) and the
                                           tokens of every node; its last item is the search's result
    pack(frames, S, W, slots)              the records of S searches' frames as the kernel's rec int32 [6, S W] and their count
    label_lists(tree, node_label)          slot -> labels for every slot that holds a prefix
"""
import numpy as np

from tests import lm_tree_ref as T
from tests.ctc_beam_lm_ref import Counters, SlotsExhausted
from tests.ctc_beam_ref import BLANK, EOS, Trie, device_frame, root

OVERLEN, POOL_FULL = T.OVERLEN, T.POOL_FULL


class RecTree(T.Tree):
    def __init__(self, S, W, slots, Lcap, node_cap):
        super().__init__(S, W, S * slots, Lcap, node_cap)
        self.per = slots

    def advance_rec(self, rec, n, lm_weight=None):
        """rec int [6, cap], n = the record count as it stands on the device -> (row_node, row_pos int32 [cap], lab, dst int64 [cap])"""
        rec = np.asarray(rec)
        cap, per = rec.shape[1], self.per
        n = min(max(int(n), 0), cap)
        row_node, row_pos = np.full(cap, -1, np.int32), np.zeros(cap, np.int32)
        lab, dst = np.zeros(cap, np.int64), np.full(cap, -1, np.int64)
        copies = []
        for r in range(n):
            s, tok, sl, dl = (int(rec[i, r]) for i in (0, 3, 4, 5))
            if not (0 <= s < self.S and s * per <= dl < (s + 1) * per and (sl < 0 or s * per <= sl < (s + 1) * per)):
                continue
            if lm_weight is not None and not lm_weight[s] > 0:
                continue
            p = 0 if sl < 0 else int(self.llen[sl])
            if p < 0:
                continue
            if p >= self.Lcap:
                self.status[s] |= OVERLEN
                continue
            if self.nnodes[s] >= self.node_cap:
                self.status[s] |= POOL_FULL
                continue
            node = s * self.node_cap + int(self.nnodes[s])
            self.nnodes[s] += 1
            row_node[r], row_pos[r], lab[r], dst[r] = node, p, tok, dl
            copies.append((dl, self.lanc[sl, :p].copy() if sl >= 0 else np.zeros(0, np.int32), node))   # (read before any write)
        for dl, head, node in copies:
            p = len(head)
            self.lanc[dl, :p] = head
            self.lanc[dl, p] = node
            self.llen[dl] = p + 1
        return row_node, row_pos, lab, dst


def record_frames(lp, top, W, len_weight, lm_weight, row, nslot=None, blank=BLANK, eos=EOS):
    """search_by_slots, yielding (records, toks_of) after the root and after every frame, then ("result", hyps, scores, ev)"""
    k = top.shape[1] if top.size else min(W, lp.shape[1])
    nslot = 2 * W + 2 if nslot is None else nslot
    ev = Counters()
    trie, toks_of = Trie(), {0: (eos,)}
    free, dying, pool = list(range(nslot - 1, 0, -1)), [], {}
    records = [(0, -1, eos, -1, 0)]

    def run_lm():
        for node, parent, v, src, dst in records:
            toks_of[node] = toks_of[parent] + (v,) if parent >= 0 else (eos,)
            pool[dst] = row(toks_of[node])
        ev.records += len(records)

    run_lm()
    yield list(records), toks_of
    lm_term = (lambda p, v: lm_weight * float(pool[p["slot"]][v])) if lm_weight > 0 else None
    live = [root()]
    for t in range(lp.shape[0]):
        new = device_frame(live, lp[t], top[t], k, W, len_weight, blank, eos, lm_term, ev)
        free += [s for s, _ in dying]
        records = []
        for c in new:
            if c["id"] is None:
                c["id"] = trie.id_of(c["parent"], c["last"])
                if not free:
                    raise SlotsExhausted(t)
                c["slot"] = free.pop()
                records.append((c["id"], c["parent"], c["last"], c["src"], c["slot"]))
        now = {c["id"] for c in new}
        dying = [(p["slot"], p["id"]) for p in live if p["id"] not in now]
        run_lm()
        yield list(records), toks_of
        live = new
    yield "result", [trie.tokens(p["id"], eos) for p in live], [p["total"] for p in live], ev


def pack(frames, S, W, slots, order=None):
    """frames[s]: the records of search s in one frame -> (rec int32 [6, max(S W, 1)], n); order: a permutation of the n records"""
    rows = [(s, node, parent, tok, (s * slots + src) if src >= 0 else -1, s * slots + dst)
            for s in range(S) for node, parent, tok, src, dst in frames[s]]
    if order is not None:
        rows = [rows[i] for i in order]
    rec = np.zeros((6, max(S * W, 1)), np.int32)
    assert len(rows) <= rec.shape[1]
    if rows:
        rec[:, :len(rows)] = np.asarray(rows, np.int32).T
    return rec, len(rows)


def label_lists(tree, node_label):
    return {slot: T.labels_of(tree, slot, node_label) for slot in range(tree.nslots) if tree.llen[slot] > 0}


# ---- the end-to-end cases of tests/test_ctc_tlm_fusion_gpu.py and their gaps --------------------------------------------------------
GAP_TOL = 1e-3
_GAPS = {}


def golden_gap_cases():
    """-> {(setting, utterance): (smallest gap, ties, hyps)} over the LM settings of tests/util.CTC_BEAM_SETTINGS and the golden
    utterances of ctcbeam_tiny, encoded as one batch: tests/ctc_beam_lm_ref.search_by_slots over the oracle model's log-probabilities
    with oracle.decoder.lm_predict as the LM.  The gap is the smallest non-zero distance between adjacent totals of a frame's ranking
    up to the prune boundary -- every pruning decision and every pair of adjacent results --, an exact tie counts as a gap of 0.
    Computed once."""
    if _GAPS:
        return _GAPS
    from types import SimpleNamespace

    import torch

    from oracle import decoder as od
    from oracle import model as om
    from tests.ctc_beam_lm_ref import search_by_slots
    from tests.util import CTC_BEAM_SETTINGS, LM_CFG, load_ctc_beam_golden
    cfg, sd, lm_sd, g2, _ = load_ctc_beam_golden()
    lm_cfg = SimpleNamespace(**LM_CFG)
    rows = {}

    def row(prefix):
        if prefix not in rows:
            rows[prefix] = od.lm_predict(lm_sd, lm_cfg, torch.tensor([list(prefix)]), torch.tensor([len(prefix)]))[0].numpy().astype(np.float32)
        return rows[prefix]

    with torch.no_grad():
        eouts, elens = om.encoder_forward(sd, cfg, g2["xs"], g2["xlens"])
        lp_all = torch.log_softmax(om.ctc_decoder_forward(sd, cfg, eouts, elens).float(), -1).numpy()
        for si, st in enumerate(CTC_BEAM_SETTINGS):
            if not st["lm_weight"] > 0:
                continue
            for b in range(lp_all.shape[0]):
                lp = np.ascontiguousarray(lp_all[b, :int(elens[b])])
                W = st["beam_width"]
                top = np.argsort(-lp, axis=1, kind="stable")[:, :min(W, lp.shape[1])].astype(np.int32)
                hyps, _, ev = search_by_slots(lp, top, W, st["len_weight"], st["lm_weight"], row, blank=cfg.blank_id, eos=cfg.eos_id)
                _GAPS[(si, b)] = (0.0 if ev.ties else float(ev.min_gap), ev.ties, hyps)
    return _GAPS


def kept_cases():
    """the (setting, utterance) cases whose smallest gap is at least GAP_TOL: those a score difference of 1e-4 cannot reorder"""
    return sorted(k for k, v in golden_gap_cases().items() if v[0] >= GAP_TOL)
