"""References for the transducer beam search with the bookkeeping on the device (csrc/rnnt_beam_book.hip).  TEST INFRASTRUCTURE ONLY.

    search(scorer, T, W, E)          the bookkeeping of oracle.rnnt.rnnt_beam_search over label tuples (stable sort by double score,
                                     merge of equal label sequences into the first by np.logaddexp, cut to W), with the network
                                     replaced by scorer(label_sequence, t) -> (blank, vals[W], ids[W]) and an event counter
    search_by_ids(scorer, T, W, E)   the kernel's organisation of the same search: canonical node ids from a trie keyed by
                                     (parent id, label), W rounds of arg-max instead of the sort, LSTM state slots recycled by
                                     mark and sweep inside (E + 1) W slots; it records every round's control words
    hash_scorer(seed, V, W, tie)     synthetic scorers: a hash of (seed, label sequence, t) seeds the row, values rounded to f32;
                                     the tie mode puts them on a grid of 0.5 so that sums tie exactly

A scorer's ids are relative to column 1 (label = id + 1), its values descend with ties to the lower id: the record of
emoasr_rnnt_beam_pick.  Hypotheses keep the leading <sos> (= EOS)."""
import zlib
from types import SimpleNamespace

import numpy as np

from oracle.rnnt import _merge_same_hyp

BLANK, EOS = 0, 2


def hash_scorer(seed, V, W, tie=False, scale=3.0):
    def scorer(seq, t):
        h = zlib.crc32(np.asarray([seed, t, len(seq)] + list(seq), dtype=np.int64).tobytes())
        x = np.random.default_rng(h).normal(size=V) * scale
        lp = x - np.logaddexp.reduce(x)
        if tie:
            lp = np.round(lp * 2.0) / 2.0
        lp = lp.astype(np.float32)
        ids = np.argsort(-lp[1:], kind="stable")[:W]
        return np.float32(lp[BLANK]), lp[1:][ids].copy(), ids.astype(np.int64)
    return scorer


def _events():
    return SimpleNamespace(merges=0, reformed=0, ties=0, min_gap=float("inf"))


def _note_order(ev, cands, W):
    """cands sorted best first: exact ties between neighbours, and the smallest gap between neighbours down to the cut"""
    for j in range(len(cands) - 1):
        gap = cands[j]["score"] - cands[j + 1]["score"]
        if gap == 0.0:
            ev.ties += 1
        if j < W:
            ev.min_gap = min(ev.min_gap, gap)


def search(scorer, T, W, E=3):
    """-> (hyps, scores, events): oracle.rnnt.rnnt_beam_search with the network replaced by the scorer"""
    ev = _events()
    beams = [dict(hyp=[EOS], score=0.0)]
    ever = {(EOS,)}
    for t in range(T):
        frame_out, live = [], beams
        for v in range(E):
            recs = [scorer(tuple(b["hyp"]), t) for b in live]
            for b, (blank, _, _) in zip(live, recs):
                frame_out.append(dict(hyp=b["hyp"], score=b["score"] + float(np.float64(blank))))
            grown = []
            if v < E - 1:
                for b, (_, vals, ids) in zip(live, recs):
                    for k in range(W):
                        grown.append(dict(hyp=b["hyp"] + [int(ids[k]) + 1], score=b["score"] + float(np.float64(vals[k]))))
            grown.sort(key=lambda c: -c["score"])
            _note_order(ev, grown, W)
            n0 = len(grown)
            live = _merge_same_hyp(grown)
            assert len(live) == n0          # distinct parents, distinct labels per parent: nothing to fold among the grown
            live = live[:W]
            held = {tuple(c["hyp"]) for c in frame_out} | {tuple(b["hyp"]) for b in beams}
            for c in live:
                key = tuple(c["hyp"])
                if key in ever and key not in held:
                    ev.reformed += 1
                ever.add(key)
            if not live:
                break
        frame_out.sort(key=lambda c: -c["score"])
        _note_order(ev, frame_out, W)
        n0 = len(frame_out)
        frame_out = [dict(c) for c in frame_out]
        merged = _merge_same_hyp(frame_out)
        ev.merges += n0 - len(merged)
        beams = merged[:W]
    return [b["hyp"] for b in beams], [b["score"] for b in beams], ev


def search_by_ids(scorer, T, W, E=3):
    """-> (hyps, scores, rounds): the organisation of csrc/rnnt_beam_book.hip.  rounds[n] = dict(t, v, ctl, refs): ctl the W rows
    (label, source slot, destination slot, active, t) the n-th launch of the round kernels runs under, refs the slots that live
    rows, frame list and beams reference at that moment"""
    NS = (E + 1) * W
    trie, keys = {}, {0: None}       # (parent id, label) -> id;  id -> (parent id, label)

    def find_or_add(parent, label):
        if (parent, label) not in trie:
            trie[(parent, label)] = len(trie) + 1
            keys[trie[(parent, label)]] = (parent, label)
        return trie[(parent, label)]

    def labels(hid):
        out = []
        while keys[hid] is not None:
            hid, lab = keys[hid]
            out.append(lab)
        return [EOS] + out[::-1]

    def best_first(cands, n):
        """n rounds of arg-max over (score descending, position ascending)"""
        left, out = list(range(len(cands))), []
        while left and len(out) < n:
            b = left[0]
            for p in left[1:]:
                if cands[p]["score"] > cands[b]["score"]:
                    b = p
            left.remove(b)
            out.append(cands[b])
        return out

    rounds = []

    def next_round(t, v, live, frame, beams):
        refs = {c["slot"] for c in live} | {c["slot"] for c in frame} | {c["slot"] for c in beams}
        free = [s for s in range(NS) if s not in refs]
        assert len(free) >= len(live)
        ctl = []
        for i in range(W):
            if i < len(live):
                live[i]["dst"] = free[i]
                ctl.append((live[i]["last"], live[i]["slot"], free[i], 1, t))
            else:
                ctl.append((0, 0, 0, 0, 0))
        rounds.append(dict(t=t, v=v, ctl=ctl, refs=refs))

    beams = [dict(id=0, score=0.0, last=EOS, slot=0, len=1)]
    for t in range(T):
        frame, live = [], [dict(b) for b in beams]
        for v in range(E):
            next_round(t, v, live, frame, beams)
            recs = [scorer(tuple(labels(c["id"])), t) for c in live]
            for c, (blank, _, _) in zip(live, recs):
                frame.append(dict(c, score=c["score"] + float(np.float64(blank))))
            if v == E - 1:
                break
            grown = []
            for c, (_, vals, ids) in zip(live, recs):
                for k in range(W):
                    grown.append(dict(parent=c["id"], last=int(ids[k]) + 1, score=c["score"] + float(np.float64(vals[k])),
                                      slot=c["dst"], len=c["len"] + 1))
            live = best_first(grown, W)
            for c in live:
                c["id"] = find_or_add(c.pop("parent"), c["last"])
        out = []
        for c in best_first(frame, len(frame)):
            hit = [o for o in out if o["id"] == c["id"]]
            if hit:
                hit[0]["score"] = float(np.logaddexp(hit[0]["score"], c["score"]))
            elif len(out) < W:
                out.append(dict(c))
        beams = out
    return [labels(b["id"]) for b in beams], [b["score"] for b in beams], rounds


# (seed, V, W, T, E, tie): W in {1, 2, 4, 16}, T in {0, 1, 2, 12}, V - 1 == W and V - 1 > W, a tie mode
CASES = [(s, W + 1, W, T, 3, False) for s, W in enumerate((1, 2, 4, 16)) for T in (0, 1, 2, 12)]
CASES += [(20 + s, V, W, T, 3, False) for s, (V, W) in enumerate(((5, 2), (9, 4), (40, 4), (40, 16))) for T in (1, 2, 12)]
CASES += [(40, 3, 2, 12, 2, False), (41, 5, 4, 12, 4, False), (42, 5, 2, 12, 1, False)]
TIE_CASES = [(60 + s, V, W, 12, 3, True) for s, (V, W) in enumerate(((3, 2), (5, 4), (9, 4), (40, 16)))]
ALL_CASES = CASES + TIE_CASES


def case_id(c):
    return "s%d-V%d-W%d-T%d-E%d%s" % (c[0], c[1], c[2], c[3], c[4], "-tie" if c[5] else "")


def scorer_of(case):
    seed, V, W, T, E, tie = case
    return hash_scorer(seed, V, W, tie)
