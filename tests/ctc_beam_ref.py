"""Shared rows and pure-Python references for the batched CTC prefix beam search tests (no GPU, no library).

    make_rows(seed, T, V, scale, W, tie_cols=None) -> (lp f32 [T, V], top int32 [T, k]), k = min(W, V); blank 0, <eos> 2
    search(lp, top, W, len_weight)      the host search restated over label tuples, instrumented -> (hyps, scores, events)
    device_frame(live, row, top_t, ...)  ONE frame as the device kernels organise it (csrc/ctc_beam_step.h): no table over label
                                        sequences, the merge test q.parent == p.id and q.last == v on canonical node ids, the
                                        total (asr + lm) + bonus, W rounds of arg-max; the LM term and the counters are optional
    search_by_ids(lp, top, W, len_weight)  the loop around it without an LM: node ids from a Trie keyed by (parent id, label)
                                        -> (hyps, scores); tests/ctc_beam_lm_ref.py::search_by_slots is the loop with one
"""
import math

import numpy as np

BLANK, EOS = 0, 2
NEG = -1e10


def _lse2(a, b):
    m = a if a > b else b
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def make_rows(seed, T, V, scale, W, tie_cols=None):
    r = np.random.RandomState(seed)
    x = (r.randn(T, V) * scale).astype(np.float32)
    if tie_cols is not None:
        x[:, tie_cols[1]] = x[:, tie_cols[0]]
    lp = (x - np.log(np.sum(np.exp(x.astype(np.float64)), axis=1, keepdims=True))).astype(np.float32)
    k = min(W, V)
    top = np.argsort(-lp, axis=1, kind="stable")[:, :k].astype(np.int32)
    return np.ascontiguousarray(lp), np.ascontiguousarray(top)


class Events:
    def __init__(self):
        self.folds = 0             # two candidates of a frame denoted the same label sequence
        self.folds_ext_first = 0   # ... and the extension was the one seen first
        self.reformed = 0          # a prefix that had dropped out came back while a child of it is live
        self.ties = 0              # exact ties of the total at adjacent ranks, up to the prune boundary
        self.eos_new = 0           # new prefixes that end in <eos>
        self.min_gap = math.inf    # smallest non-zero gap between adjacent totals, up to the prune boundary


def search(lp, top, W, len_weight=0.0, blank=BLANK, eos=EOS):
    """csrc/ctc_beam_host.hip without an LM, over label tuples: -> (hyps, scores, Events)"""
    ev = Events()
    live = [dict(toks=(eos,), p_b=0.0, p_nb=NEG, asr=0.0, bonus=0.0, n_plain=0)]
    ever = {(eos,)}
    for t in range(lp.shape[0]):
        row = lp[t]
        lp_blank = float(row[blank])
        table, order = {}, []

        def put(q, is_ext):
            old = table.get(q["toks"])
            if old is None:
                table[q["toks"]] = q
                order.append(q)
            else:
                ev.folds += 1
                ev.folds_ext_first += 0 if is_ext else 1
                old["p_b"], old["p_nb"], old["asr"] = _lse2(old["p_b"], q["p_b"]), _lse2(old["p_nb"], q["p_nb"]), \
                    _lse2(old["asr"], q["asr"])

        for p in live:
            last = p["toks"][-1] if len(p["toks"]) > 1 else None
            stay_b = _lse2(p["p_b"] + lp_blank, p["p_nb"] + lp_blank)
            stay_nb = p["p_nb"] + float(row[last]) if last is not None else NEG
            put(dict(toks=p["toks"], p_b=stay_b, p_nb=stay_nb, asr=_lse2(stay_b, stay_nb), bonus=p["bonus"],
                     n_plain=p["n_plain"]), False)
            bonus = len_weight * (p["n_plain"] + 1)
            for v in top[t]:
                v = int(v)
                if v == blank:
                    continue
                lp_v = float(row[v])
                ext_nb = p["p_b"] + lp_v if v == last else _lse2(p["p_b"] + lp_v, p["p_nb"] + lp_v)
                put(dict(toks=p["toks"] + (v,), p_b=NEG, p_nb=ext_nb, asr=_lse2(NEG, ext_nb), bonus=bonus,
                         n_plain=p["n_plain"] + (0 if v == eos else 1)), True)
        for q in order:
            q["total"] = (q["asr"] + 0.0) + q["bonus"]
        order.sort(key=lambda q: q["total"], reverse=True)      # stable, like std::stable_sort and sorted()
        for a, b in zip(order[:W], order[1:W + 1]):
            gap = a["total"] - b["total"]
            if gap == 0.0:
                ev.ties += 1
            else:
                ev.min_gap = min(ev.min_gap, gap)
        before = {p["toks"] for p in live}
        live = order[:W]
        now = {p["toks"] for p in live}
        for p in live:
            if p["toks"] not in before:
                ev.eos_new += p["toks"][-1] == eos
                if p["toks"] in ever and any(len(c) == len(p["toks"]) + 1 and c[:-1] == p["toks"] for c in now):
                    ev.reformed += 1
        ever |= now
    return [list(p["toks"]) for p in live], [p["total"] if "total" in p else 0.0 for p in live], ev


class Trie:
    """canonical node ids: (parent id, label) -> id, the root (<eos>) being 0; tokens(id) walks the keys back to the root"""

    def __init__(self):
        self.ids, self.nodes = {}, [(-1, -1)]

    def id_of(self, parent, label):
        key = (parent, label)
        if key not in self.ids:
            self.ids[key] = len(self.nodes)
            self.nodes.append(key)
        return self.ids[key]

    def tokens(self, i, eos):
        toks = []
        while i > 0:
            toks.append(self.nodes[i][1])
            i = self.nodes[i][0]
        return [eos] + toks[::-1]


def root():
    """the live set before the first frame: (<eos>), holding slot 0"""
    return dict(id=0, parent=-1, last=-1, n_plain=0, len=1, p_b=0.0, p_nb=NEG, lm=0.0, bonus=0.0, total=0.0, slot=0)


def device_frame(live, row, top_t, k, W, len_weight, blank=BLANK, eos=EOS, lm_term=None, ev=None):
    """one frame as csrc/ctc_beam_step.h organises it: candidates by position i (k + 1) + j, the merge test q.parent == p.id and
    q.last == v, the fold into the one seen first (which keeps its LM term, bonus, and position), the total (asr + lm) + bonus,
    W rounds of arg-max over rising positions -> the survivors, best first.  A survivor with id None is an extension without a
    live twin: the caller names it (and src is its parent's slot); one that folded has its twin's id and slot.
    lm_term(p, v): what label v adds to the running LM sum along live prefix p's candidates (None: no LM, the term stays p's).
    ev: a Counters-like object whose fold and tie counts are kept."""
    lp_blank = float(row[blank])
    cand = {}                                        # position i (k + 1) + j -> candidate
    for i, p in enumerate(live):
        has_last = p["last"] >= 0
        stay_b = _lse2(p["p_b"] + lp_blank, p["p_nb"] + lp_blank)
        stay_nb = p["p_nb"] + float(row[p["last"]]) if has_last else NEG
        cand[i * (k + 1)] = dict(p, p_b=stay_b, p_nb=stay_nb, asr=_lse2(stay_b, stay_nb), match=None)
        lm_run = p["lm"]
        for j in range(1, k + 1):
            v = int(top_t[j - 1])
            if v == blank:
                continue
            if lm_term is not None:
                lm_run = lm_run + lm_term(p, v)
            lp_v = float(row[v])
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
        if ev is not None:
            ev.folds_stay_first += z < pos
            ev.folds_ext_first += pos < z
            ev.folds_lm_differ += a["lm"] != b["lm"]
        for f in ("p_b", "p_nb", "asr"):
            a[f] = _lse2(a[f], b[f])
        a["id"], a["slot"] = live[q]["id"], live[q]["slot"]
        del cand[second]
    for c in cand.values():
        c["total"] = (c["asr"] + c["lm"]) + c["bonus"]
    if ev is not None:
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
    return new


def search_by_ids(lp, top, W, len_weight=0.0, blank=BLANK, eos=EOS):
    """the search as csrc/ctc_beam.hip organises it -> (hyps, scores)"""
    k = top.shape[1] if top.size else min(W, lp.shape[1])
    trie, live = Trie(), [root()]
    for t in range(lp.shape[0]):
        live = device_frame(live, lp[t], top[t], k, W, len_weight, blank, eos)
        for c in live:
            if c["id"] is None:
                c["id"] = trie.id_of(c["parent"], c["last"])
    hyps = [trie.tokens(p["id"], eos) for p in live]
    assert all(len(h) == p["len"] for h, p in zip(hyps, live))
    return hyps, [p["total"] for p in live]


# the cases of tests/test_ctc_beam_batch_{cpu,gpu}.py: (V, W, T, scale, len_weight, seeds, tie_cols)
FOLD_CASES = [(5, 3, 32, 1.0, 0.0, (19, 103, 138), None), (6, 8, 32, 1.0, 0.0, (8, 49, 58), None)]
LEN_CASES = [(5, 4, 32, 1.5, 0.3, (0, 1, 2, 3), None), (8, 4, 48, 2.0, 0.5, (0, 1, 2, 3), None)]
TIE_CASES = [(6, 4, 32, 1.0, 0.1, (0, 1, 2), (1, 3))]
SIZE_CASES = [(1000, 10, 48, 3.0, 0.0, (0,), None), (40, 32, 16, 3.0, 0.0, (0,), None), (5, 8, 1, 1.0, 0.0, (0,), None)]
ALL_CASES = FOLD_CASES + LEN_CASES + TIE_CASES + SIZE_CASES


def expand(cases):
    return [(V, W, T, scale, lw, seed, tie) for V, W, T, scale, lw, seeds, tie in cases for seed in seeds]
