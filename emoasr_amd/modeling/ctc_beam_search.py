"""CTC prefix beam search with LM shallow fusion for CTC-only models -- the decode path of
asr/modeling/decoders/ctc.py:203-344 (`CTCDecoder._beam_search`) and :372-397 (`_merge_ctc_paths`).

Split of work: the acoustic side runs once per utterance on the GPU (output projection, log-softmax
and the per-frame top-k, all frames in one launch each: emoasr_gemm_nt / emoasr_log_softmax /
emoasr_topk) and comes to the host in one copy; the Transformer LM scores the NEW prefixes of a frame
in one batched device call (LM.predict, as the reference batches them with pad_sequence, ctc.py:241-260),
its rows stay on the device while their prefix is live and a frame brings only its k candidate columns to
the host; the prefix bookkeeping itself -- ~110 candidates per frame: extend, merge, stable sort, prune --
is native host code in IEEE doubles, like the reference's python floats (csrc/ctc_beam_host.hip:
emoasr_ctc_beam_step, 20 us per frame).  EMOASR_CTC_BEAM_NATIVE=0 runs the same bookkeeping as the Python
loop below (bit-identical results; tests/test_ctc_beam_gpu.py compares the two).

A stateful LM (the RNN LM, modeling/rnnlm.py: `lm.stateful`) is never re-run over a prefix: its state after a prefix is a function
of the prefix alone (the reference's `lm_states` of a beam is the LSTM run over hyp[:-1], whichever path reached it), so the "score
each distinct prefix once" scheme carries over with the state next to the row.  A live prefix's slot holds its log-probability row
and the state after the whole prefix; a new prefix p + (v) is ONE step (token v, from p's slot, into a fresh slot), the root (<eos>,)
a step from the zero state.  The slot of a prefix that died is freed only after the next frame's new prefixes were scored from it.

Reference behaviour kept on purpose (it decides which prefixes survive):
  * the LM score of the k-th candidate extension of a prefix also contains the LM scores of the
    candidates tried before it (`score_lm +=` inside the candidate loop, ctc.py:309-310);
  * length bonus = len_weight * (number of non-<eos> tokens of the PARENT prefix + 1) (ctc.py:308);
  * when two paths reach the same prefix, probabilities are merged but the LM / length scores of the
    first path are kept (ctc.py:388-393);
  * hypotheses start with <eos> (the LM's BOS) and scores are returned best first.

Without an LM (the N-best lists of `test_asr.py --nbest --beam_width N`) the search depends on nothing outside the utterance's own
rows: ctc_prefix_beam_search_batch runs it for any number of utterances in ONE launch on the device (csrc/ctc_beam.hip:
emoasr_ctc_beam_batch; beam_width <= 32), with the same hypotheses in the same order as the host loop.

With an LM, ctc_prefix_beam_search_batch_lm runs the searches of a whole batch -- and of all (lm_weight, len_weight) cells of a
fusion grid over that batch -- frame by frame on the device (csrc/ctc_beam_lm.hip: one launch moves every search one frame and lists
the prefixes that are new; one batched LM call scores them into a pool of rows the next launch reads).  Nothing but the record
count (and, for a stateless LM, the records) comes to the host per frame.  decoder.ctc_tlm_fusion = "device" steps the Transformer LM
over a prefix tree instead (_TreePass; csrc/lm_tree.hip): the records stay on the device and no prefix is re-run.
"""
import math
import os

import numpy as np
import torch

from .. import ops
from .functions import _engine_of
from .lm import require_next_token_lm

NEG = -1e10  # LOG_0 of decoders/ctc.py:23


def _lse2(a, b):
    m = a if a > b else b
    return m + math.log(math.exp(a - m) + math.exp(b - m))


class _Prefix:
    __slots__ = ("toks", "p_b", "p_nb", "asr", "lm", "len_bonus", "n_plain", "lm_states")

    def __init__(self, toks, p_b, p_nb, asr, lm, len_bonus, n_plain):
        self.toks, self.p_b, self.p_nb, self.asr, self.lm, self.len_bonus = toks, p_b, p_nb, asr, lm, len_bonus
        self.n_plain = n_plain  # tokens that are not <eos>
        self.lm_states = None   # stateful LM without the prefix cache: (h, c) after toks[:-1], as the reference's beams carry it

    @property
    def total(self):
        return self.asr + self.lm + self.len_bonus


class _LMSlots:
    """slot bookkeeping of a stateful LM for the prefix searches: prefix -> slot of lm.new_pools (state after the prefix + its
    log-probability row).  score(live) steps the prefixes that have no slot yet from their parents' slots; release(live) frees
    what the PREVIOUS release found dead (its slots were still parents of this frame's new prefixes).  live <= beam_width prefixes,
    as many dying ones: 2 * beam_width slots (+ 2 spare)."""

    def __init__(self, lm, beam_width):
        self.lm, self.n = lm, 2 * beam_width + 2
        self.pools = lm.new_pools(self.n)
        self.slot_of, self.free, self.dying = {}, list(range(self.n)), []
        self.dev = self.pools.logp.device

    def score(self, live):
        """-> the prefixes that were new (now scored), in live order"""
        need = [p for p in live if p not in self.slot_of]
        if need:
            from ..engine import h2d_i32
            src = [self.slot_of[p[:-1]] if len(p) > 1 else -1 for p in need]     # (the root starts from the zero state)
            dst = [self.free.pop() for _ in need]
            ctl = h2d_i32([p[-1] for p in need] + src + dst, self.dev)
            n = len(need)
            self.lm.step(self.pools, n, ctl[:n], ctl[n:2 * n], ctl[2 * n:], ctl[2 * n:])
            self.slot_of.update(zip(need, dst))
        return need

    def release(self, live):
        keep = set(live)
        for key in self.dying:
            if key not in keep:     # (a prefix that died can be formed again one frame later: it keeps its slot)
                self.free.append(self.slot_of.pop(key))
        self.dying = [q for q in self.slot_of if q not in keep]


def _search_native(logp_dev, top_dev, T, V, k, blank, eos, beam_width, len_weight, lm, lm_weight):
    """the frame loop over csrc/ctc_beam_host.hip: per frame one C call (bookkeeping), and -- with an LM -- one batched LM call for
    the prefixes that are new plus one [live, k] gather of their cached rows (the frame's only device-to-host copy)"""
    import ctypes
    from .. import lib
    L = lib.load()
    L.emoasr_ctc_beam_new.restype = ctypes.c_void_p
    L.emoasr_ctc_beam_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    L.emoasr_ctc_beam_free.argtypes = [ctypes.c_void_p]
    L.emoasr_ctc_beam_free.restype = None
    L.emoasr_ctc_beam_step.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    L.emoasr_ctc_beam_scores.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    use_lm = lm is not None and lm_weight > 0
    logp = logp_dev.cpu().numpy()                      # f32 [T, V]: one D2H for the whole utterance (rows read as doubles in C)
    top = np.ascontiguousarray(top_dev.cpu().numpy().astype(np.int32))
    h = L.emoasr_ctc_beam_new(int(beam_width), int(blank), int(eos), float(len_weight), float(lm_weight if use_lm else 0.0))
    assert h, "emoasr_ctc_beam_new failed"
    try:
        parent = np.zeros(beam_width, dtype=np.int32)
        tok = np.zeros(beam_width, dtype=np.int32)
        live = [(eos,)]
        dev = logp_dev.device
        stateful = use_lm and getattr(lm, "stateful", False)
        if stateful:
            slots = _LMSlots(lm, beam_width)
            cache, slot_of = slots.pools.logp, slots.slot_of
            top_long = top_dev.long()
        elif use_lm:
            nslot = 2 * beam_width + 2
            cache = torch.empty(nslot, V, device=dev, dtype=torch.float32)   # LM rows of the live prefixes
            slot_of, free = {}, list(range(nslot))
            top_long = top_dev.long()
        for t in range(T):
            lm_ptr = None
            if use_lm:
                if stateful:
                    slots.score(live)     # one step per new prefix, rows and states stay in the slot pools
                need = [p for p in live if p not in slot_of]
                if need:
                    n = max(len(p) for p in need)
                    batch = torch.zeros(len(need), n, dtype=torch.int64)   # 0-padded like pad_sequence (ctc.py:243-246)
                    for i, p in enumerate(need):
                        batch[i, : len(p)] = torch.tensor(p)
                    rows, _ = lm.predict(batch, [len(p) for p in need])
                    ids = []
                    for p in need:
                        slot_of[p] = free.pop()
                        ids.append(slot_of[p])
                    cache.index_copy_(0, torch.tensor(ids, device=dev), rows.float())
                sl = torch.tensor([slot_of[p] for p in live], device=dev)
                vals = cache.index_select(0, sl).index_select(1, top_long[t]).cpu().numpy().astype(np.float64)   # [live, k]
                vals = np.ascontiguousarray(vals)
                lm_ptr = vals.ctypes.data
            n = L.emoasr_ctc_beam_step(h, logp[t].ctypes.data, top[t].ctypes.data, int(k), lm_ptr, parent.ctypes.data, tok.ctypes.data)
            if n < 0:
                raise lib.EmoasrHipError("emoasr_ctc_beam_step failed: " + L.emoasr_last_error().decode())
            live = [live[parent[i]] + ((int(tok[i]),) if tok[i] >= 0 else ()) for i in range(n)]
            if stateful:
                slots.release(live)
            elif use_lm:
                keep = set(live)
                for key in [q for q in slot_of if q not in keep]:
                    free.append(slot_of.pop(key))
        scores = np.zeros(len(live), dtype=np.float64)
        L.emoasr_ctc_beam_scores(h, scores.ctypes.data)
        return [list(p) for p in live], [float(v) for v in scores]
    finally:
        L.emoasr_ctc_beam_free(h)


def _stateless_rows(lm, live, lm_rows, lm_cache):
    """LM rows (float64 numpy) of the live prefixes from a stateless LM, which re-runs a prefix to score it.
    The reference scores EVERY live prefix with the LM at every frame (ctc.py:241-260) -- the same prefix again and again
    while it survives.  The LM's next-token row is a function of the prefix alone, so each distinct prefix is scored
    ONCE (the frame it first survives) and its row kept while it is live: a frame costs an LM call only for prefixes
    that are new, in one batch (rows of a batched call do not depend on their neighbours).  EMOASR_CTC_LM_CACHE=0:
    the reference's recomputation."""
    need = [p for p in live if p.toks not in lm_rows] if lm_cache else list(live)
    if need:
        n = max(len(p.toks) for p in need)
        batch = torch.zeros(len(need), n, dtype=torch.int64)  # 0-padded like pad_sequence (ctc.py:243-246)
        for i, p in enumerate(need):
            batch[i, : len(p.toks)] = torch.tensor(p.toks)
        rows, _ = lm.predict(batch, [len(p.toks) for p in need])
        rows = rows.cpu().numpy().astype(np.float64)
        for i, p in enumerate(need):
            lm_rows[p.toks] = rows[i]
    lm_lp = [lm_rows[p.toks] for p in live]
    if lm_cache:
        keep = {p.toks for p in live}
        for key in [k for k in lm_rows if k not in keep]:
            del lm_rows[key]
    else:
        lm_rows.clear()
    return lm_lp


def ctc_prefix_beam_search(dec, eouts, elens, beam_width, len_weight=0.0, lm=None, lm_weight=0.0):
    """-> (hyps, scores, logits) for ONE utterance (the reference asserts batch size 1, ctc.py:212)."""
    require_next_token_lm(lm, lm_weight)
    assert eouts.shape[0] == 1, "CTC beam search decodes one utterance at a time (ctc.py:212)"
    eng = _engine_of(dec)
    blank, eos, V = dec.blank_id, dec.eos_id, dec.vocab_size
    with torch.no_grad():
        logits = eng.head_logits(eouts, getattr(dec, "_prefix", "decoder") + ".output")                      # [1, T, V]
        T = logits.shape[1]
        logp_dev = ops.log_softmax(logits.view(T, V))        # f32 [T, V]
        k = min(beam_width, V)
        _, top_dev, _ = ops.topk(logp_dev, k)                # ids sorted by descending score, per frame
        if os.environ.get("EMOASR_CTC_BEAM_NATIVE", "1") != "0":
            hyps, scores = _search_native(logp_dev, top_dev, T, V, k, blank, eos, beam_width, len_weight, lm, lm_weight)
            return hyps, scores, logits
        logp = logp_dev.cpu().numpy().astype(np.float64)     # one D2H for the whole utterance
        top = top_dev.cpu().numpy()
    use_lm = lm is not None and lm_weight > 0
    lm_cache, lm_rows = os.environ.get("EMOASR_CTC_LM_CACHE", "1") != "0", {}
    stateful, slots, new_states = use_lm and getattr(lm, "stateful", False), None, None
    live = [_Prefix((eos,), 0.0, NEG, 0.0, 0.0, 0.0, 0)]
    if stateful and not lm_cache:
        live[0].lm_states = lm.zero_states(1, logp_dev.device)     # (ctc.py:226)
    for t in range(T):
        row = logp[t]
        lp_blank = float(row[blank])
        cands = [(int(v), float(row[v])) for v in top[t] if int(v) != blank]
        if use_lm:
            if stateful and not lm_cache:
                # the reference literally (ctc.py:251-260, 312-331): every live beam carries (h, c) after hyp[:-1]; one batched step
                # from the concatenated states, the extensions below take their slice of the new states
                n = max(len(p.toks) for p in live)
                batch = torch.zeros(len(live), n, dtype=torch.int64)
                for i, p in enumerate(live):
                    batch[i, : len(p.toks)] = torch.tensor(p.toks)
                states = tuple(torch.cat([p.lm_states[j] for p in live], dim=1) for j in (0, 1))
                rows, new_states = lm.predict(batch, [len(p.toks) for p in live], states=states)
                lm_lp = list(rows.cpu().numpy().astype(np.float64))
            elif stateful:
                if slots is None:
                    slots = _LMSlots(lm, beam_width)
                toks = [p.toks for p in live]
                fresh = slots.score(toks)
                if fresh:
                    sl = torch.tensor([slots.slot_of[q] for q in fresh], device=slots.dev)
                    got = slots.pools.logp.index_select(0, sl).cpu().numpy().astype(np.float64)
                    lm_rows.update(zip(fresh, got))
                lm_lp = [lm_rows[q] for q in toks]
            else:
                lm_lp = _stateless_rows(lm, live, lm_rows, lm_cache)
        table, order = {}, []  # prefix -> _Prefix, in first-seen order (dict merge of ctc.py:374-395)

        def put(q):
            old = table.get(q.toks)
            if old is None:
                table[q.toks] = q
                order.append(q)
            else:  # same label sequence reached twice: fold the path probabilities only
                old.p_b, old.p_nb, old.asr = _lse2(old.p_b, q.p_b), _lse2(old.p_nb, q.p_nb), _lse2(old.asr, q.asr)

        for i, p in enumerate(live):
            last = p.toks[-1] if len(p.toks) > 1 else None
            # stay on the same prefix: blank, or a repeat of its last label
            stay_b = _lse2(p.p_b + lp_blank, p.p_nb + lp_blank)
            stay_nb = p.p_nb + float(row[last]) if last is not None else NEG
            stay = _Prefix(p.toks, stay_b, stay_nb, _lse2(stay_b, stay_nb), p.lm, p.len_bonus, p.n_plain)
            stay.lm_states = p.lm_states     # (ctc.py:291: not updated)
            put(stay)
            # extend by each of the frame's top-k labels
            lm_run = p.lm
            bonus = len_weight * (p.n_plain + 1)
            for v, lp_v in cands:
                ext_nb = p.p_b + lp_v if v == last else _lse2(p.p_b + lp_v, p.p_nb + lp_v)
                if use_lm:
                    lm_run += lm_weight * float(lm_lp[i][v])
                q = _Prefix(p.toks + (v,), NEG, ext_nb, _lse2(NEG, ext_nb), lm_run, bonus, p.n_plain + (0 if v == eos else 1))
                if new_states is not None:
                    q.lm_states = (new_states[0][:, i:i + 1], new_states[1][:, i:i + 1])
                put(q)
        order.sort(key=lambda q: q.total, reverse=True)  # stable, like sorted() in ctc.py:338
        live = order[:beam_width]
        if slots is not None:
            slots.release([p.toks for p in live])
            for key in [q for q in lm_rows if q not in slots.slot_of]:
                del lm_rows[key]
    return [list(p.toks) for p in live], [p.total for p in live], logits


CTC_BEAM_BATCH_BUDGET = 1 << 27   # rows x V elements of one chunk: 512 MiB of f32 log-probabilities next to the logits
CTC_BEAM_LM_POOL_BUDGET = 1 << 30   # searches x rows per search x V elements of one chunk's LM pool: 4 GiB of f32 rows


def _check_width(beam_width):
    if not 1 <= beam_width <= ops.CTC_BEAM_MAX_WIDTH:
        raise ValueError(f"device CTC beam search: beam width {beam_width} is outside 1..{ops.CTC_BEAM_MAX_WIDTH}")


def _chunks(dec, eouts, elens, k, admits=lambda n, longest: True):
    """the acoustic side of the device searches, chunk by chunk -> (b0, b1, row_off, logits, logp, top) per chunk of utterances
    b0 .. b1: row_off the host list of their row offsets, logits [rows, V] of the head over their valid frames only (the rows of
    all of them stacked), logp its log-soft-max, top int32 [rows, k] its top-k: one launch each.  The next utterance joins the
    chunk while the chunk's rows x V stay within CTC_BEAM_BATCH_BUDGET and admits(utterances the chunk would then hold, its longest); an
    utterance that breaks either bound on its own goes alone."""
    eng = _engine_of(dec)
    V = dec.vocab_size
    B, Tmax = eouts.shape[0], eouts.shape[1]
    lens = [min(int(n), Tmax) for n in elens]
    assert len(lens) == B
    b0 = 0
    while b0 < B:
        b1, rows, longest = b0 + 1, lens[b0], lens[b0]
        while b1 < B and (rows + lens[b1]) * V <= CTC_BEAM_BATCH_BUDGET and admits(b1 + 1 - b0, max(longest, lens[b1])):
            rows += lens[b1]
            longest = max(longest, lens[b1])
            b1 += 1
        row_off = [0]
        for n in lens[b0:b1]:
            row_off.append(row_off[-1] + n)
        if rows:
            x = eouts[b0, :lens[b0]] if b1 == b0 + 1 else torch.cat([eouts[b, :lens[b]] for b in range(b0, b1)])
            logits = eng.head_logits(x.unsqueeze(0), getattr(dec, "_prefix", "decoder") + ".output")[0]      # [rows, V]
            logp = ops.log_softmax(logits)
            _, top, _ = ops.topk(logp, k)
        else:
            logits = torch.empty(0, V, device=eouts.device, dtype=eouts.dtype)
            logp = torch.empty(0, V, device=eouts.device, dtype=torch.float32)
            top = torch.empty(0, k, device=eouts.device, dtype=torch.int32)
        yield b0, b1, row_off, logits, logp, top
        b0 = b1


def _search_chunks(chunks, search):
    """-> (hyps, scores, logits) over all chunks: search(logp, top, row_off) gives a chunk's per-utterance hyps and scores.
    Nothing here records a gradient: the chunk walk and the searches run under torch.no_grad()."""
    hyps, scores, logits_out = [], [], []
    with torch.no_grad():
        for _, _, row_off, logits, logp, top in chunks:
            h, s = search(logp, top, row_off)
            hyps += h
            scores += s
            logits_out += [logits[a:b].unsqueeze(0) for a, b in zip(row_off[:-1], row_off[1:])]
    return hyps, scores, logits_out


def _max_frames(row_off_host):
    return max([b - a for a, b in zip(row_off_host[:-1], row_off_host[1:])] + [0])


def _download(out_tok, out_len, out_score, out_n, status, refused):
    """ONE download of the results of n searches (tokens, lengths, scores, counts and the status word packed into one int32 array)
    -> (hyps, scores), each a list per search, best first; a status bit raises EmoasrHipError(`refused`: what the bits say)"""
    n, W, L = out_tok.shape
    host = torch.cat([out_tok.view(-1), out_len.view(-1), out_score.view(torch.int32).view(-1), out_n, status]).cpu().numpy()
    o1, o2, o3 = n * W * L, n * W * L + n * W, n * W * L + 3 * n * W
    tok, ln = host[:o1].reshape(n, W, L), host[o1:o2].reshape(n, W)
    score, cnt, st = host[o2:o3].copy().view(np.float64).reshape(n, W), host[o3:o3 + n], int(host[o3 + n])
    if st:
        from .. import lib
        raise lib.EmoasrHipError(f"{refused}: {ops.ctc_beam_status_text(st)} (status {st})")
    hyps = [[tok[s, i, :ln[s, i]].tolist() for i in range(cnt[s])] for s in range(n)]
    return hyps, [[float(v) for v in score[s, :cnt[s]]] for s in range(n)]


def _search_device(logp, top, row_off_host, beam_width, blank, eos, len_weight):
    """one launch over the utterances of row_off, ONE download -> (hyps, scores) per utterance"""
    row_off = torch.tensor(row_off_host, dtype=torch.int32).to(logp.device)
    outs = ops.ctc_beam_batch(logp, row_off, top, beam_width, blank, eos, len_weight, max_frames=_max_frames(row_off_host))
    return _download(*outs, "emoasr_ctc_beam_batch refused an utterance")


def ctc_prefix_beam_search_batch(dec, eouts, elens, beam_width, len_weight=0.0):
    """-> (hyps, scores, logits) for ALL utterances of the batch, no LM: hyps[b] / scores[b] are what ctc_prefix_beam_search returns
    for utterance b alone (best first, every hypothesis starting with <eos>), logits[b] is [1, elens[b], V].

    The head runs over the valid frames only (the rows of all utterances stacked), then one log-soft-max and one top-k over all
    rows, one search launch and one download.  Utterances are taken in chunks of at most CTC_BEAM_BATCH_BUDGET = 2^27 rows x V
    elements (an utterance larger than that goes alone), so the f32 log-probabilities of a chunk stay within 512 MiB."""
    _check_width(beam_width)
    blank, eos = dec.blank_id, dec.eos_id
    return _search_chunks(_chunks(dec, eouts, elens, min(beam_width, dec.vocab_size)),
                          lambda logp, top, row_off: _search_device(logp, top, row_off, beam_width, blank, eos, len_weight))


class _StatefulPass:
    """LM pass of a stateful LM (the RNN LM): the token, source-row and destination-row columns of the record list go to lm.step as
    they lie on the device (lm.step chunks them by RNNLM_STEP_MAX); no per-prefix host work, no prefix is ever re-run"""

    def __init__(self, lm, rows, V):
        self.lm, self.pools = lm, lm.new_pools(rows)
        self.logp = self.pools.logp
        assert self.logp.shape[1] >= V, "the LM's vocabulary is smaller than the CTC head's"

    def __call__(self, st, n):
        if n:
            self.lm.step(self.pools, n, st.rec[3], st.rec[4], st.rec[5], row_dst=st.rec[5])


class _StatelessPass:
    """LM pass of a stateless LM (the Transformer LM): the host keeps (search, node) -> tokens from the records (the parent's tokens
    + the token), runs ONE lm.predict over the new prefixes of all searches, 0-padded like pad_sequence (ctc.py:243-246), and
    copies the rows into the pool with one index_copy_"""

    def __init__(self, lm, rows, V, device):
        self.lm, self.toks = lm, {}
        self.logp = torch.empty(rows, V, device=device, dtype=torch.float32)

    def __call__(self, st, n):
        if not n:
            return
        rec = st.rec[:, :n].cpu().numpy()
        need = []
        for s, node, parent, tok, _, _ in rec.T.tolist():
            p = (self.toks[(s, parent)] + (tok,)) if parent >= 0 else (tok,)
            self.toks[(s, node)] = p
            need.append(p)
        width = max(len(p) for p in need)
        batch = torch.zeros(n, width, dtype=torch.int64)
        for i, p in enumerate(need):
            batch[i, : len(p)] = torch.tensor(p)
        rows, _ = self.lm.predict(batch, [len(p) for p in need])
        self.logp.index_copy_(0, st.rec[5, :n].long(), rows[:, : self.logp.shape[1]].float())


tree_stats = None              # of the last chunk searched over the prefix tree: nodes taken per search, the capacities, the longest list
_TLM_POOL_BUDGET = 8 << 30     # bytes of K / V node pools and lists one chunk of tree-fused searches may hold (as engine/rnnt_search.py)


def _tree_bytes(lm, W, max_frames):
    """bytes of one search's share of the tree: its K / V nodes over all layers and the lists of its 2 W + 2 slots"""
    from .. import lm_tree
    P = lm.params
    esz = 2 if lm.compute_dtype == torch.bfloat16 else 4
    return (2 * P.num_layers * lm_tree.ctc_node_cap(W, max_frames) * P.hidden_size * esz
            + ops.ctc_beam_lm_slots(W) * (lm_tree.ctc_list_cap(max_frames, P.max_seq_len) + 1) * 4)


class _TreePass:
    """LM pass of the Transformer LM under decoder.ctc_tlm_fusion = "device" (DESIGN.md section 32): the pool rows are the slots of a
    prefix tree (lm_tree.TreeState), a record is one new node.  Per call emoasr_lm_tree_advance_rec reads the record list where the
    frame kernel left it, emoasr_lm_tree_step_rows steps the n new prefixes by ONE token against their parents' keys / values, and
    emoasr_log_softmax_rows_to puts the normalised rows into the pool.  No host work beyond the count the caller read, no record
    comes to the host, no prefix is re-run.  A search with lm_weight <= 0 takes no node (its rows are never read)."""

    def __init__(self, lm, S, W, slots, V, max_frames, lm_weight, device):
        from .. import lm_tree
        lm._prepare()
        P = lm.params
        self.V, self.lm_weight, self.split = V, lm_weight, lm._split()
        self.tree = lm_tree.TreeState(S, W, S * slots, lm_tree.ctc_list_cap(max_frames, P.max_seq_len),
                                      lm_tree.ctc_node_cap(W, max_frames), device, rows=max(S * W, 1))
        self.tree.reset()
        with ops.stream_scope(self.split):
            self.step = lm_tree.TreeStep(lm, self.tree)
        self.logp = torch.zeros(S * slots, V, device=device, dtype=torch.float32)

    def __call__(self, st, n):
        n = min(n, self.tree.rows)
        if not n:
            return
        with ops.stream_scope(self.split):
            self.tree.advance_records(st.rec, st.rec_count, self.lm_weight)
            logits = self.step(n)
            ops.log_softmax_rows_to(logits, n, st.rec[5], self.logp, self.V, row_ok=self.tree.row_node)

    def finish(self, names):
        global tree_stats
        tree_stats = {"nodes": self.tree.nnodes.tolist(), "node_cap": self.tree.node_cap, "lcap": self.tree.Lcap,
                      "longest_prefix": int(self.tree.llen.max())}
        self.tree.raise_for_status("ctc_prefix_beam_search_batch_lm (ctc_tlm_fusion = 'device')", names, tags=True)


def _search_device_lm(logp, top, row_off_host, beam_width, blank, eos, lm, weights, tree=False, first=0):
    """the frame loop over csrc/ctc_beam_lm.hip for the utterances of row_off x the weight pairs -> (hyps, scores), each
    [utterance][pair].  init, an LM pass over the root records, then per frame one launch, one small download (the record count;
    the stateless pass also takes the records) and one LM pass; finish and ONE download of the results.  tree: the Transformer LM
    over the prefix tree (_TreePass; a limit it met is a RuntimeError naming the search, `first` the chunk's first utterance)."""
    dev = logp.device
    B, C, W = len(row_off_host) - 1, len(weights), beam_width
    S, V = B * C, logp.shape[1]
    max_frames = _max_frames(row_off_host)
    row_off = torch.tensor(row_off_host, dtype=torch.int32).to(dev)
    utt = torch.arange(B, dtype=torch.int32).repeat_interleave(C).to(dev)                  # search s = utterance s // C, pair s % C
    wt = torch.tensor([[float(a) for a, _ in weights] * B, [float(b) for _, b in weights] * B], dtype=torch.float64).to(dev)
    st = ops.ctc_beam_lm_init(row_off, utt, W, eos, max_frames)
    rows = S * st.slots
    if tree:
        lm_pass = _TreePass(lm, S, W, st.slots, V, max_frames, wt[0], dev)
    else:
        lm_pass = _StatefulPass(lm, rows, V) if getattr(lm, "stateful", False) else _StatelessPass(lm, rows, V, dev)
    lm_pass(st, int(st.rec_count.item()))
    for t in range(max_frames):
        ops.ctc_beam_lm_frame(st, t, logp, top, wt[0], wt[1], blank, lm_pass.logp)
        lm_pass(st, int(st.rec_count.item()))
    hyps, scores = _download(*ops.ctc_beam_lm_finish(st), st.status, "emoasr_ctc_beam_lm refused a search")
    if tree:
        lm_pass.finish([f"search {s} (utterance {first + s // C}, weights {weights[s % C]})" for s in range(S)])
    return [hyps[b * C:(b + 1) * C] for b in range(B)], [scores[b * C:(b + 1) * C] for b in range(B)]


def ctc_prefix_beam_search_batch_lm(dec, eouts, elens, beam_width, lm, weights):
    """CTC prefix beam search WITH LM shallow fusion for all utterances of the batch and all (lm_weight, len_weight) pairs of
    `weights` at once, on the device (csrc/ctc_beam_lm.hip).  One pair is plain batched fusion; several pairs are the cells of a
    fusion grid, which share everything the weights do not touch.  -> (hyps, scores, logits): hyps[b][c] / scores[b][c] are what
    ctc_prefix_beam_search returns for utterance b alone with pair c (best first, every hypothesis starting with <eos>), logits[b]
    is [1, elens[b], V].

    The acoustic side is ctc_prefix_beam_search_batch's, once per utterance whatever the number of pairs: the head over the valid
    frames, one log-soft-max, one top-k.  Utterances are taken in chunks: the next utterance joins the chunk while (a) the chunk's
    rows x V stay within CTC_BEAM_BATCH_BUDGET = 2^27 elements (512 MiB of f32 log-probabilities) and (b) its searches' LM pool,
    utterances x pairs x (2 beam_width + 2) rows x V, stays within CTC_BEAM_LM_POOL_BUDGET = 2^30 elements (4 GiB); an utterance
    that breaks either bound on its own goes alone.

    decoder.ctc_tlm_fusion = "device" with a causal Transformer LM (functions.ctc_tlm_why_not passes it; otherwise a ValueError
    carrying the reason): the LM is stepped over a prefix tree on the device (_TreePass), and (c) the searches' node pools and
    lists, sized for the chunk's longest utterance, stay within _TLM_POOL_BUDGET = 8 GiB.  An RNN LM ignores the switch."""
    from .functions import ctc_tlm_fusion_of, ctc_tlm_why_not
    require_next_token_lm(lm, max([float(a) for a, _ in weights] + [0.0]))
    if lm is None:
        raise ValueError("ctc_prefix_beam_search_batch_lm needs an LM (without one: ctc_prefix_beam_search_batch)")
    _check_width(beam_width)
    weights = [(float(a), float(b)) for a, b in weights]
    assert weights, "at least one (lm_weight, len_weight) pair"
    blank, eos, V = dec.blank_id, dec.eos_id, dec.vocab_size
    per_utt = len(weights) * ops.ctc_beam_lm_slots(beam_width) * V          # pool elements one utterance's searches need
    tree = ctc_tlm_fusion_of(dec) == "device" and getattr(lm, "lm_type", None) == "transformer" and any(a > 0 for a, _ in weights)
    if not tree:
        return _search_chunks(_chunks(dec, eouts, elens, min(beam_width, V), lambda n, longest: n * per_utt <= CTC_BEAM_LM_POOL_BUDGET),
                              lambda logp, top, row_off: _search_device_lm(logp, top, row_off, beam_width, blank, eos, lm, weights))
    why = ctc_tlm_why_not(dec, lm)
    if why is not None:
        raise ValueError(f"emoasr_amd: ctc_tlm_fusion = 'device' cannot fuse this LM: {why}")
    admits = lambda n, longest: (n * per_utt <= CTC_BEAM_LM_POOL_BUDGET
                                 and n * len(weights) * _tree_bytes(lm, beam_width, longest) <= _TLM_POOL_BUDGET)
    first = [0]

    def search(logp, top, row_off):
        out = _search_device_lm(logp, top, row_off, beam_width, blank, eos, lm, weights, tree=True, first=first[0])
        first[0] += len(row_off) - 1
        return out

    return _search_chunks(_chunks(dec, eouts, elens, min(beam_width, V), admits), search)
