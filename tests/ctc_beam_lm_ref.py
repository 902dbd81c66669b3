"""Shared references for the fused (LM) batched CTC prefix beam search tests (no GPU, no library); rows and case tables come from
tests/ctc_beam_ref.py.

    table_lm(V, scale)                 -> row(prefix) f32 [V] = log_softmax(scale * N(0, 1)) seeded by zlib.crc32 of the prefix's int32
                                          bytes: a next-token "LM" that is a pure function of the prefix; row.batch(batch, lens) is the
                                          same LM in the shape of oracle.ctc_beam's lm_predict argument
    search_by_slots(lp, top, W, len_weight, lm_weight, row, nslot=None)
                                       the fused search as csrc/ctc_beam_lm.hip organises it: node ids from the (parent id, label)
                                       trie, LM rows in numbered slots handed out from a free list and given back one frame after
                                       their prefix left the beam, one record per new prefix, the LM term as a running sum along a
                                       live prefix's candidates -> (hyps, scores, Counters)
"""
import math
import zlib

import numpy as np

from tests.ctc_beam_ref import BLANK, EOS, NEG, _lse2


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
    use_lm = lm_weight > 0
    trie, nodes, toks_of = {}, [(-1, -1)], {0: (eos,)}
    free, dying, pool = list(range(nslot - 1, 0, -1)), [], {}        # (taken from the end: 1, 2, ...)
    records = [(0, -1, eos, -1, 0)]                                 # (node, parent node, token, src slot, dst slot)

    def run_lm():
        for node, parent, v, src, dst in records:
            toks_of[node] = toks_of[parent] + (v,) if parent >= 0 else (eos,)
            pool[dst] = row(toks_of[node])
        ev.records += len(records)

    run_lm()
    ev.slot_high = 1
    live = [dict(id=0, parent=-1, last=-1, n_plain=0, len=1, p_b=0.0, p_nb=NEG, lm=0.0, bonus=0.0, total=0.0, slot=0)]
    for t in range(lp.shape[0]):
        fr = lp[t]
        lp_blank = float(fr[blank])
        cand = {}
        for i, p in enumerate(live):
            has_last = p["last"] >= 0
            stay_b = _lse2(p["p_b"] + lp_blank, p["p_nb"] + lp_blank)
            stay_nb = p["p_nb"] + float(fr[p["last"]]) if has_last else NEG
            cand[i * (k + 1)] = dict(p, p_b=stay_b, p_nb=stay_nb, asr=_lse2(stay_b, stay_nb), match=None)
            lm_run = p["lm"]
            for j in range(1, k + 1):
                v = int(top[t, j - 1])
                if v == blank:
                    continue
                if use_lm:
                    lm_run = lm_run + lm_weight * float(pool[p["slot"]][v])
                lp_v = float(fr[v])
                ext_nb = p["p_b"] + lp_v if (has_last and v == p["last"]) else _lse2(p["p_b"] + lp_v, p["p_nb"] + lp_v)
                c = dict(id=None, parent=p["id"], last=v, n_plain=p["n_plain"] + (0 if v == eos else 1), len=p["len"] + 1,
                         p_b=NEG, p_nb=ext_nb, asr=_lse2(NEG, ext_nb), lm=lm_run, bonus=len_weight * (p["n_plain"] + 1), slot=None,
                         src=p["slot"])
                c["match"] = [q for q, lq in enumerate(live) if lq["parent"] == p["id"] and lq["last"] == v]
                cand[i * (k + 1) + j] = c
        for pos in sorted(cand):
            c = cand.get(pos)
            if c is None or not c.get("match"):
                continue
            (q,) = c["match"]
            z = q * (k + 1)
            first, second = (z, pos) if z < pos else (pos, z)
            a, b = cand[first], cand[second]
            ev.folds_stay_first += z < pos
            ev.folds_ext_first += pos < z
            ev.folds_lm_differ += a["lm"] != b["lm"]
            for f in ("p_b", "p_nb", "asr"):
                a[f] = _lse2(a[f], b[f])
            a["id"], a["slot"] = live[q]["id"], live[q]["slot"]
            del cand[second]
        for c in cand.values():
            c["total"] = (c["asr"] + c["lm"]) + c["bonus"]
        ranked = sorted(cand.values(), key=lambda c: c["total"], reverse=True)    # (stable; the positions are already rising)
        for a, b in zip(ranked[:W], ranked[1:W + 1]):
            gap = a["total"] - b["total"]
            if gap == 0.0:
                ev.ties += 1
            else:
                ev.min_gap = min(ev.min_gap, gap)
        new = []
        for _ in range(W):
            best = None
            for pos in sorted(cand):
                if best is None or cand[pos]["total"] > cand[best]["total"]:
                    best = pos
            if best is None:
                break
            new.append(cand.pop(best))
        # slots that waited one frame are free again; then ids, slots and records of the new prefixes
        waiting = {s: n for s, n in dying}
        free += [s for s, _ in dying]
        records = []
        for c in new:
            if c["id"] is None:
                key = (c["parent"], c["last"])
                if key not in trie:
                    trie[key] = len(nodes)
                    nodes.append(key)
                c["id"] = trie[key]
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
    hyps = []
    for p in live:
        toks, i = [], p["id"]
        while i > 0:
            toks.append(nodes[i][1])
            i = nodes[i][0]
        hyps.append([eos] + toks[::-1])
        assert len(hyps[-1]) == p["len"] and tuple(hyps[-1]) == toks_of[p["id"]]
    return hyps, [p["total"] for p in live], ev
