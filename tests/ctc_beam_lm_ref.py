"""Shared references for the fused (LM) batched CTC prefix beam search tests (no GPU, no library); rows and case tables come from
tests/ctc_beam_ref.py.

    table_lm(V, scale)                 -> row(prefix) f32 [V] = log_softmax(scale * N(0, 1)) seeded by zlib.crc32 of the prefix's int32
                                          bytes: a next-token "LM" that is a pure function of the prefix; row.batch(batch, lens) is the
                                          same LM in the shape of oracle.ctc_beam's lm_predict argument
    search_by_slots(lp, top, W, len_weight, lm_weight, row, nslot=None)
                                       the fused search as csrc/ctc_beam_lm.hip organises it, a loop around the frame of
                                       tests/ctc_beam_ref.py::device_frame: node ids from the (parent id, label) trie, LM rows
                                       in numbered slots handed out from a free list and given back one frame after their
                                       prefix left the beam, one record per new prefix, the LM term as a running sum along a
                                       live prefix's candidates -> (hyps, scores, Counters)
"""
import math
import zlib

import numpy as np

from tests.ctc_beam_ref import BLANK, EOS, Trie, device_frame, root


def table_lm(V, scale=2.0):
    def row(prefix):
        seed = zlib.crc32(np.asarray(list(prefix), dtype=np.int32).tobytes())
        x = np.random.RandomState(seed).randn(V) * scale
        return (x - np.log(np.sum(np.exp(x)))).astype(np.float32)

    def batch(hyps, lens):
        return np.stack([row(tuple(int(v) for v in h[:n])) for h, n in zip(np.asarray(hyps), np.asarray(lens))])

    row.batch = batch
    return row


class Counters:
    def __init__(self):
        self.folds_stay_first = 0     # a stay and its extension twin folded, the stay seen first
        self.folds_ext_first = 0      # ... the extension seen first
        self.folds_lm_differ = 0      # folds whose two sides carried different LM terms (the first one's is kept)
        self.reformed_waiting = 0     # new prefixes whose earlier slot was still waiting to be freed
        self.slot_high = 0            # most slots held at once
        self.records = 0              # new prefixes over the whole search, the root included
        self.ties = 0                 # exact ties of adjacent totals, up to the prune boundary
        self.min_gap = math.inf       # smallest non-zero gap between adjacent totals, up to the prune boundary


class SlotsExhausted(Exception):
    pass


def search_by_slots(lp, top, W, len_weight, lm_weight, row, nslot=None, blank=BLANK, eos=EOS):
    k = top.shape[1] if top.size else min(W, lp.shape[1])
    nslot = 2 * W + 2 if nslot is None else nslot
    ev = Counters()
    trie, toks_of = Trie(), {0: (eos,)}
    free, dying, pool = list(range(nslot - 1, 0, -1)), [], {}        # (taken from the end: 1, 2, ...)
    records = [(0, -1, eos, -1, 0)]                                 # (node, parent node, token, src slot, dst slot)

    def run_lm():
        for node, parent, v, src, dst in records:
            toks_of[node] = toks_of[parent] + (v,) if parent >= 0 else (eos,)
            pool[dst] = row(toks_of[node])
        ev.records += len(records)

    run_lm()
    ev.slot_high = 1
    lm_term = (lambda p, v: lm_weight * float(pool[p["slot"]][v])) if lm_weight > 0 else None
    live = [root()]
    for t in range(lp.shape[0]):
        new = device_frame(live, lp[t], top[t], k, W, len_weight, blank, eos, lm_term, ev)
        # slots that waited one frame are free again; then ids, slots and records of the new prefixes
        waiting = {s: n for s, n in dying}
        free += [s for s, _ in dying]
        records = []
        for c in new:
            if c["id"] is None:
                c["id"] = trie.id_of(c["parent"], c["last"])
                ev.reformed_waiting += c["id"] in waiting.values()
                if not free:
                    raise SlotsExhausted(t)
                c["slot"] = free.pop()
                records.append((c["id"], c["parent"], c["last"], c["src"], c["slot"]))
        ev.slot_high = max(ev.slot_high, nslot - len(free))
        now = {c["id"] for c in new}
        dying = [(p["slot"], p["id"]) for p in live if p["id"] not in now]
        run_lm()
        live = new
    hyps = [trie.tokens(p["id"], eos) for p in live]
    assert all(len(h) == p["len"] and tuple(h) == toks_of[p["id"]] for h, p in zip(hyps, live))
    return hyps, [p["total"] for p in live], ev
