"""Word / character error rate (asr/metrics.py:20-175): Levenshtein alignment with the reference's
backtrace preference (correct, then insertion, then substitution, then deletion), so the reported
D / S / I split is the same as the reference's, not just the distance."""
import numpy as np


def compute_wer(hyp, ref, cer=False):
    """-> (wer in %, dict(wer, n_sub, n_ins, n_del, n_ref, error_list)); an empty hypothesis is scored as
    one dummy word that matches nothing (metrics.py:21-23)."""
    hyp = list(hyp) if len(hyp) else ["<dummy>"]
    ref = list(ref)
    if cer:
        hyp, ref = list("".join(hyp)), list("".join(ref))
    R, H = len(ref), len(hyp)
    d = np.zeros((R + 1, H + 1), dtype=np.int64)
    d[0, :] = np.arange(H + 1)
    d[:, 0] = np.arange(R + 1)
    for i in range(1, R + 1):
        ri = ref[i - 1]
        for j in range(1, H + 1):
            d[i, j] = d[i - 1, j - 1] if ri == hyp[j - 1] else 1 + min(d[i - 1, j - 1], d[i, j - 1], d[i - 1, j])
    ops, x, y = [], R, H
    while x or y:
        if x and y and d[x, y] == d[x - 1, y - 1] and ref[x - 1] == hyp[y - 1]:
            ops.append("C"); x -= 1; y -= 1
        elif y and d[x, y] == d[x, y - 1] + 1:
            ops.append("I"); y -= 1
        elif x and y and d[x, y] == d[x - 1, y - 1] + 1:
            ops.append("S"); x -= 1; y -= 1
        else:
            ops.append("D"); x -= 1
    ops.reverse()
    n_sub, n_ins, n_del = ops.count("S"), ops.count("I"), ops.count("D")
    assert int(d[R, H]) == n_sub + n_ins + n_del
    wer = 100.0 * int(d[R, H]) / R
    return wer, {"wer": wer, "n_sub": n_sub, "n_ins": n_ins, "n_del": n_del, "n_ref": R, "error_list": ops}


def _total(pairs, cer):
    tot = {"n_sub": 0, "n_ins": 0, "n_del": 0, "n_ref": 0}
    for hyp, ref in pairs:
        _, w = compute_wer(hyp, ref, cer=cer)
        for k in tot:
            tot[k] += w[k]
    wer = 100.0 * (tot["n_sub"] + tot["n_ins"] + tot["n_del"]) / tot["n_ref"]
    return wer, dict(tot, wer=wer)


def _total_device(pairs, cer, device):
    """_total with every pair aligned in one ops.edit_align call (csrc/rescore.hip); the same integers, so the same WER"""
    from . import ops
    vocab = {}
    intern = lambda seq: [vocab.setdefault(w, len(vocab)) for w in seq]
    hyps, refs = [], []
    for hyp, ref in pairs:
        hyp, ref = list(hyp) or ["<dummy>"], list(ref)      # (the empty hypothesis BEFORE the join to characters, as compute_wer)
        if cer:
            hyp, ref = list("".join(hyp)), list("".join(ref))
        hyps.append(intern(hyp))
        refs.append(intern(ref))
    counts = ops.edit_align(hyps, refs, device=device)["counts"].astype(np.int64).sum(axis=0)
    tot = {"n_sub": int(counts[0]), "n_ins": int(counts[1]), "n_del": int(counts[2]), "n_ref": sum(len(r) for r in refs)}
    wer = 100.0 * (tot["n_sub"] + tot["n_ins"] + tot["n_del"]) / tot["n_ref"]
    return wer, dict(tot, wer=wer)


def compute_wers(hyps, refs, vocab=None, cer=False, device=None):
    """corpus-level WER over id (with vocab: subword -> word) or word sequences (metrics.py:108-130).  With a `device` the pairs are
    aligned there in one call (sides of at most 4096 tokens); the default is the host loop."""
    if vocab is not None:
        hyps, refs = [vocab.ids2words(h) for h in hyps], [vocab.ids2words(r) for r in refs]
    return _total(zip(hyps, refs), cer) if device is None else _total_device(zip(hyps, refs), cer, device)


def compute_wers_cells(cells, refs, device=None):
    """cells[c][u]: the word hypothesis of utterance u in cell c of a grid; refs[u] its reference -> [(wer, dict)] per cell, what
    compute_wers(cells[c], refs, device=device) gives.  Cells of a grid share most hypotheses: every distinct (utterance, hypothesis)
    pair is aligned ONCE (with a `device` all of them in one ops.edit_align call, the alignment compute_wers runs there; an
    utterance's hypotheses share its reference) and a cell's totals are the sums over its pairs."""
    n_ref = sum(len(r) for r in refs)
    index = [{} for _ in refs]       # per utterance: hypothesis -> its number among the utterance's distinct hypotheses
    for cell in cells:
        assert len(cell) == len(refs)
        for u, hyp in enumerate(cell):
            index[u].setdefault(tuple(hyp), len(index[u]))
    pairs = [(u, hyp) for u, seen in enumerate(index) for hyp in seen]
    counts = {}
    if device is None:
        for u, hyp in pairs:
            w = compute_wer(hyp, refs[u])[1]
            counts[u, hyp] = (w["n_sub"], w["n_ins"], w["n_del"])
    elif pairs:
        from . import ops
        vocab = {}
        intern = lambda seq: [vocab.setdefault(w, len(vocab)) for w in seq]
        got = ops.edit_align([intern(list(hyp) or ["<dummy>"]) for _, hyp in pairs], [intern(r) for r in refs],
                             ref_idx=[u for u, _ in pairs], device=device)["counts"]
        counts = {p: tuple(int(v) for v in got[i, :3]) for i, p in enumerate(pairs)}
    out = []
    for cell in cells:
        s = np.sum([counts[u, tuple(hyp)] for u, hyp in enumerate(cell)], axis=0) if len(cell) else np.zeros(3)
        tot = {"n_sub": int(s[0]), "n_ins": int(s[1]), "n_del": int(s[2]), "n_ref": n_ref}
        wer = 100.0 * (tot["n_sub"] + tot["n_ins"] + tot["n_del"]) / n_ref
        out.append((wer, dict(tot, wer=wer)))
    return out


def compute_wers_df(dfhyp, dfref=None, cer=False, device=None):
    """result TSV (columns text, reftext) or hypothesis + reference tables joined on utt_id
    (metrics.py:133-175); missing / NaN hypotheses count as empty.  `device`: as compute_wers."""
    def words(v):
        return v.split() if isinstance(v, str) else []
    total = _total if device is None else (lambda pairs, cer: _total_device(pairs, cer, device))
    if dfref is None:
        return total(((words(r.text), words(r.reftext)) for r in dfhyp.itertuples()), cer)
    id2hyp = {r.utt_id: words(r.text) for r in dfhyp.itertuples()}
    return total(((id2hyp.get(r.utt_id, []), words(r.text)) for r in dfref.itertuples()), cer)


def wer_summary(wer, w, cer=False):
    return f"{'CER' if cer else 'WER'}: {wer:.2f} [D={w['n_del']:d}, S={w['n_sub']:d}, I={w['n_ins']:d}, N={w['n_ref']:d}]"
