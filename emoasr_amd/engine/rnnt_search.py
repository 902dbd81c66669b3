"""The RNN-Transducer's searches: greedy (launch chain, one cooperative launch, the batch in lockstep) and
alignment-length synchronous beam search (launch chain, replayed round, the batch on the device with its two LM fusions).
  reference: asr/modeling/decoders/rnn_transducer.py:194-359
Shared here and written once: the limits of the rows / round kernels (the functions below), the host loop of the two beam searches
that keep their books on the host (beam_host_loop), the rows step of the two lockstep forms (RowsStep).  RNNTSearch is a base of
engine/rnnt.py's RNNTDecoder, which keeps the network, the loss and the backward."""
import os
from ctypes import c_void_p

import torch

from .. import lockstep, ops
from .arena import _Stash, h2d_i32


# ---- the kernels' size limits, each condition once (csrc/rnnt_beam.hip; the table and what composes what: DESIGN.md section 31) -----
def lstm_rows_fits(dtype, nins, H):
    """emoasr_rnnt_beam_lstm_rows on layers of input widths nins: 8 (bf16) / 4 (f32) elements per vector access, nin + H columns
    inside the plan of 1904 (bf16, the MFMA plan) / 2368 (f32)"""
    vec, wide = (8, 1904) if dtype == torch.bfloat16 else (4, 2368)
    return not (H % 8 or H % vec or any(n % vec for n in nins) or max(nins) + H > wide)


def joint_rows_fits(H):
    """emoasr_rnnt_beam_joint / _joint_rows: 16 rows of H floats in 64 KiB of LDS"""
    return 16 * H * 4 <= 64 * 1024


def pick_row_fits(V):
    """emoasr_rnnt_beam_pick / _pick_lm: a vocabulary row of f32 in 60 KiB of LDS"""
    return V * 4 <= 60 * 1024


def round_fits(dtype, V, nin_max, H):
    """the fused round (emoasr_rnnt_beam_lstm, _joint, _pick): pick and joint as above, nin + H <= 2368 columns in f32; the bf16
    plan is left to the kernel (_rnnt_beam_round_graph's warm-up falls back to the chain body when an entry point refuses)"""
    return pick_row_fits(V) and joint_rows_fits(H) and (dtype == torch.bfloat16 or nin_max + H <= 2368)


def beam_host_loop(round, T, W, E, eos, start, return_scores=False, len_weight=None):
    """the bookkeeping of the alignment-length synchronous beam search (rnn_transducer.py:242-325,348-359) over T frames of up to E
    rounds at width W, on the host like the reference and without torch: stable sort by float64 score, merge of equal label
    sequences by log-add in encounter order, cut to the beam.  A hypothesis is (labels with the leading <sos>, score, token of the
    LSTM state from BEFORE its last label); start: the zero state's token.
    round(live, t, v, last) -> (host, state_of): host the float64 [nb, 1 + 2 W] record (blank log-prob | top-k log-probs | top-k
    ids relative to column 1) of the live hypotheses at frame t -- on a frame's last round only column 0 is read -- and state_of(i)
    the token of the state that row i's step left.  len_weight (a fused search): rnnt_len_expand at the end.
    -> hyps best first, with return_scores (hyps, scores)"""
    import numpy as np

    def merge(cands):
        seen = {}
        for hyp, score, state in cands:
            key = tuple(hyp)
            if key in seen:
                seen[key][1] = float(np.logaddexp(seen[key][1], score))
            else:
                seen[key] = [hyp, score, state]
        return [tuple(c) for c in seen.values()]

    beams = [([eos], 0.0, start)]
    for t in range(T):
        frame_out, live = [], beams
        for v in range(E):
            if not live:
                break
            last = v == E - 1
            host, state_of = round(live, t, v, last)
            for i, (hyp, score, state) in enumerate(live):
                frame_out.append((hyp, score + float(host[i, 0]), state))
            grown = []
            if not last:
                for i, (hyp, score, _) in enumerate(live):
                    state = state_of(i)      # (once per row: the loop below is the host form's hot path)
                    for k in range(W):
                        grown.append((hyp + [int(host[i, 1 + W + k]) + 1], score + float(host[i, 1 + k]), state))
            grown.sort(key=lambda c: -c[1])
            live = merge(grown)[:W]
        frame_out.sort(key=lambda c: -c[1])
        beams = merge(frame_out)[:W]
    hyps, scores = [hyp for hyp, _, _ in beams], [score for _, score, _ in beams]
    if len_weight is not None:
        hyps, scores = lockstep.expand_len_weights(hyps, scores, [len_weight], 0)[0]
    return (hyps, scores) if return_scores else hyps


class RowsStep(_Stash):
    """what the two lockstep forms (greedy, beam) share, and the record they cache.  The buffers of S searches: per layer nslots
    state slots (ph in the compute dtype, pc in f32), e = the stacked w_enc . eouts + b of <= rows frames (doubling from 1024), hj =
    the R joint rows of a step, row_off, the LSTM bias sums; the launches of a step over them; the staging of a chunk.  The form
    adds its control words (its book kernel defines their layout), its books, its LM branch, its graph and its tmax."""

    def __init__(self, eng, S, R, nslots, total):
        J, H, nl, dev = eng.r_J, eng.r_H, eng.r_nl, eng.arena.flat.device
        self.S, self.R, self.nslots, self.rows = S, R, nslots, max(1024, 1 << (total - 1).bit_length())
        self.ph = [torch.zeros(nslots, H, device=dev, dtype=eng.dtype) for _ in range(nl)]
        self.pc = [torch.zeros(nslots, H, device=dev, dtype=torch.float32) for _ in range(nl)]
        self.e = torch.zeros(self.rows, J, device=dev, dtype=eng.dtype)
        self.hj = torch.zeros(R, J, device=dev, dtype=eng.dtype)
        self.row_off = torch.zeros(S + 1, device=dev, dtype=torch.int32)
        self.bias = [eng._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(nl)]   # (refreshed per search: stage)

    def lstm_layers(self, n, emb, weights, bias, ph, pc, Hl, p_lab, p_src, p_dst, p_act):
        """a stack of LSTM layers (the prediction network's, a fused RNN LM's) on n rows through emoasr_rnnt_beam_lstm_rows: layer 0
        embeds the labels at p_lab, every layer reads its state from the slots at p_src and leaves it in those at p_dst"""
        from .. import lib
        dtc = ops.dt(self.ph[0])
        xtab, ldx, nx, xidx = emb, emb.shape[1], emb.shape[0], p_lab
        for l, (w_ih, w_hh) in enumerate(weights):
            lib.call("emoasr_rnnt_beam_lstm_rows", dtc, n, w_ih.shape[1], Hl, ops._p(xtab), ldx, nx, xidx, ops._p(w_ih), ops._p(w_hh),
                     ops._p(bias[l]), ops._p(ph[l]), ops._p(pc[l]), self.nslots, p_src, p_dst, p_act, ops._stream())
            xtab, ldx, nx, xidx = ph[l], Hl, self.nslots, p_dst

    def prediction(self, eng, n, p_lab, p_src, p_dst, p_act):
        """the first half of a step: the prediction network's layers on n rows (a fused form's LM branch comes behind it)"""
        A = eng.arena
        weights = [(A.w(f"decoder.rnns.{l}.weight_ih_l0"), A.w(f"decoder.rnns.{l}.weight_hh_l0")) for l in range(eng.r_nl)]
        self.lstm_layers(n, A.w("decoder.embed.weight"), weights, self.bias, self.ph, self.pc, eng.r_H, p_lab, p_src, p_dst, p_act)

    def joint_logits(self, eng, j_dst, j_act, j_row):
        """the second half: the joint rows (the top layer's h of slot j_dst against frame j_row of e, R rows) and the output product
        -> logits [R, V]"""
        from .. import lib
        A = eng.arena
        lib.call("emoasr_rnnt_beam_joint_rows", ops.dt(self.ph[0]), self.R, eng.r_H, eng.r_J, self.rows, ops._p(self.ph[eng.r_nl - 1]),
                 self.nslots, j_dst, j_act, ops._p(A.w("decoder.w_dec.weight")), ops._p(A.p("decoder.w_dec.bias")), ops._p(self.e),
                 j_row, ops._p(self.hj), ops._stream())
        return ops.gemm_nt(self.hj, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))

    def stage(self, eng, eouts, elens, sutt):
        """a chunk ready for its book kernel's start; search s runs over utterance sutt[s] (the same utterance several times in a row:
        its rows are replicated per search, so the frame offsets keep rising).  w_enc . eouts + b per utterance, as the single-
        utterance forms compute it (a row's bits then do not depend on the batch), formed once for the consecutive searches of an
        utterance; row_off; the current bias_ih + bias_hh, in place; slot 0 of every search's region, its zero state"""
        A = eng.arena
        offs, rows_of = [0], {}
        for b in sutt:
            if elens[b]:
                if b not in rows_of:
                    rows_of = {b: ops.gemm_nt(eouts[b, :elens[b]], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))}
                self.e[offs[-1]:offs[-1] + elens[b]].copy_(rows_of[b])
            offs.append(offs[-1] + elens[b])
        self.row_off.copy_(torch.tensor(offs, dtype=torch.int32))
        for l in range(eng.r_nl):
            self.bias[l].copy_(eng._lstm_bias(f"decoder.rnns.{l}"))
            self.ph[l].view(self.S, -1, eng.r_H)[:, 0].zero_()
            self.pc[l].view(self.S, -1, eng.r_H)[:, 0].zero_()


class RNNTSearch:
    def rnnt_greedy(self, eouts, elens_host, blank, eos, max_seq_len=256, window=64):
        """time-synchronous greedy search (rnn_transducer.py:194-240).  While the arg-max is blank the
        prediction network does not move, so the frames t, t+1, ... can be scored against the SAME decoder
        state in one batched joint + output GEMM: each round scores up to `window` frames, finds the first
        non-blank one on the device and brings (index, token) back with one 8-byte copy -- one host round
        trip per emitted label (plus one per all-blank window) instead of one per frame.  The sequence of
        (frame, token) decisions is exactly the reference's."""
        with self._scope(), torch.no_grad():
            A, J = self.arena, self.r_J
            A.refresh_shadow()
            hyps, aligns = [], []
            V = A.w("decoder.output.weight").shape[0]
            # the one-launch search per utterance that fits it (model shape, LDS image, step-tag range); the launch chain otherwise
            fits = [bool(ops.lib.size_query("emoasr_rnnt_greedy_fits", ops.dt(eouts), self.r_emb, self.r_H, J, V, self.r_nl,
                                            int(elens_host[b]), max_seq_len)) for b in range(eouts.shape[0])]
            if all(fits):
                return self._rnnt_greedy_device(eouts, elens_host, blank, eos, max_seq_len)
            for b in range(eouts.shape[0]):
                if fits[b]:
                    (hyp,), (align,) = self._rnnt_greedy_device(eouts[b:b + 1], [int(elens_host[b])], blank, eos, max_seq_len)
                else:
                    hyp, align = self._rnnt_greedy_chain(eouts[b], int(elens_host[b]), blank, eos, max_seq_len, window)
                hyps.append(hyp)
                aligns.append(align)
            return hyps, aligns

    def _rnnt_greedy_chain(self, eouts_b, T, blank, eos, max_seq_len, window):
        """one utterance through the launch chain: windows of frames scored against the same decoder state, the first non-blank
        frame found on the device, one host round trip per emitted label"""
        A, J = self.arena, self.r_J
        dev = eouts_b.device
        e_all = ops.gemm_nt(eouts_b[:max(T, 1)], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))
        dout, state, _ = self.rnnt_recurrency(h2d_i32([[eos]], dev), None, False, False)
        g = ops.gemm_nt(dout.view(1, self.r_H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
        hyp, align, t = [], [], 0
        while t < T:
            n = min(window, T - t)
            h = ops.joint_tanh(e_all[t:t + n].view(1, n, J), g.view(1, 1, J))
            logits = ops.gemm_nt(h.view(n, J), A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
            k, tok = ops.first_not_equal(ops.argmax_rows(logits), blank).tolist()
            if k < 0:  # every frame of the window is blank
                align += [blank] * n
                t += n
                continue
            align += [blank] * k + [tok]
            t += k  # the label is emitted AT frame t+k: the search stays on that frame
            hyp.append(tok)
            dout, state, _ = self.rnnt_recurrency(h2d_i32([[tok]], dev), state, False, False)
            g = ops.gemm_nt(dout.view(1, self.r_H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
            if len(hyp) > max_seq_len:
                break
        return hyp, align

    def _rnnt_greedy_device(self, eouts, elens_host, blank, eos, max_seq_len):
        """the whole search of an utterance as ONE cooperative launch (csrc/rnnt_greedy.hip): no host round trip per label; the
        utterances of a batch are enqueued one after the other and read back with a single synchronisation"""
        from .. import lib
        A, J, H, E = self.arena, self.r_J, self.r_H, self.r_emb
        dev = eouts.device
        w_out = A.w("decoder.output.weight")
        V = w_out.shape[0]
        nbytes = lib.size_query("emoasr_rnnt_greedy_ws_bytes", H, J)
        b_l = [self._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(2)]
        outs = []
        for b in range(eouts.shape[0]):
            T = int(elens_host[b])
            e_all = ops.gemm_nt(eouts[b, :max(T, 1)], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            hyp = torch.empty(max_seq_len + 1, device=dev, dtype=torch.int32)
            align = torch.empty(T + max_seq_len + 1, device=dev, dtype=torch.int32)
            lens = torch.zeros(2, device=dev, dtype=torch.int32)
            lib.call("emoasr_rnnt_greedy", ops.dt(eouts), T, E, H, J, V, blank, eos, max_seq_len, ops._p(e_all),
                     ops._p(A.w("decoder.embed.weight")), ops._p(A.w("decoder.rnns.0.weight_ih_l0")),
                     ops._p(A.w("decoder.rnns.0.weight_hh_l0")), ops._p(b_l[0]), ops._p(A.w("decoder.rnns.1.weight_ih_l0")),
                     ops._p(A.w("decoder.rnns.1.weight_hh_l0")), ops._p(b_l[1]), ops._p(A.w("decoder.w_dec.weight")),
                     ops._p(A.p("decoder.w_dec.bias")), ops._p(w_out), ops._p(A.p("decoder.output.bias")), ops._p(ws), nbytes,
                     ops._p(hyp), ops._p(align), ops._p(lens), ops._stream())
            outs.append((e_all, ws, hyp, align, lens))
        hyps, aligns = [], []
        for e_all, ws, hyp, align, lens in outs:
            nh, na = lens.tolist()    # (the first read synchronises)
            err = int(ws[64:68].view(torch.int32).item())
            if err:
                raise RuntimeError("rnnt_greedy: a grid barrier gave up waiting (csrc/rnnt_greedy.hip); "
                                   "emoasr_set_option('rnnt_greedy_coop', 0) selects the launch chain")
            hyps.append(hyp[:nh].tolist())
            aligns.append(align[:na].tolist())
        return hyps, aligns

    # ---- the batched greedy search in lockstep (csrc/rnnt_greedy_batch.hip) -------------------------------
    # joint rows per step: S K <= 1024, so a chunk holds 1024 // K searches (128 at K = 8).  What the cap implies at the L4 sizes
    # (J = 512, V = 1000, bf16): 1 MB of joint rows, 2 MB of logits, 2 S state slots per layer (0.8 MB for two layers), and the
    # stacked w_enc . eouts + b of the chunk, 1 KB per frame (39 MB for 128 utterances of 300 frames); twice that in f32.
    _GREEDY_BATCH_ROWS = 1024
    # frames_per_step and the steps between two reads of the live counter (once ceil(max(elens) / K) steps have run): the fastest
    # of K = 1 / 2 / 4 / 8 at every batch size and dtype measured, and of blocks of 4 / 8 / 16 / 32
    _GREEDY_BATCH_K = 8
    _GREEDY_BATCH_POLL = 32

    def rnnt_greedy_batch_why_not(self):
        """why the batched greedy search cannot take this model (None: it can): nl >= 1 and the limits of
        emoasr_rnnt_beam_lstm_rows / _joint_rows (lstm_rows_fits, joint_rows_fits).  rnnt_beam_device_ok's bound on the vocabulary
        belongs to the pick kernel, which keeps a row in LDS; the greedy book kernel reads its rows from global memory, so any
        vocabulary of two labels or more is taken."""
        A, H, nl = self.arena, self.r_H, self.r_nl
        if self.dtype not in (torch.float32, torch.bfloat16):
            return f"the compute dtype {self.dtype} is neither float32 nor bfloat16"
        if nl < 1:
            return "the prediction network has no LSTM layer"
        V_ = A.w("decoder.output.weight").shape[0]
        if V_ < 2:
            return f"the vocabulary ({V_}) has no label beside blank"
        nins = [A.w(f"decoder.rnns.{l}.weight_ih_l0").shape[1] for l in range(nl)]
        if not (lstm_rows_fits(self.dtype, nins, H) and joint_rows_fits(H)):
            return (f"the prediction network's sizes (embedding {self.r_emb}, hidden {H}, layers {nl}) are outside "
                    f"emoasr_rnnt_beam_lstm_rows' limits")
        return None

    def _rnnt_greedy_batch_graph(self, S, K, blank, eos, max_seq_len, total, longest):
        """static buffers of S searches of K frames per step over <= st.rows frames in all, none longer than st.tmax (doubling from
        512), and ONE STEP of all of them (LSTM layers on S rows, joint on S K rows, output product, book) captured as a HIP graph.
        The warm-up runs the body with every search finished (no frames): every row is inactive, no state is touched.  Two state
        slots per search; the control words are 4 S LSTM words, then 3 S K joint words (csrc/rnnt_greedy_batch.hip)."""
        tab = self.__dict__.setdefault("_greedy_batch_static", {})
        key = (S, K, blank, eos, max_seq_len)
        st = tab.get(key)
        if st is not None and st.rows >= total and st.tmax >= longest:
            return st
        R = S * K
        st = RowsStep(self, S, R, 2 * S, total)
        st.tmax = max(512, 1 << (longest - 1).bit_length())
        st.ctl, st.state, st.hyp, st.align, st.lens, st.live = ops.rnnt_greedy_batch_buffers(S, K, max_seq_len, st.tmax, st.e.device)

        def launches():
            """the step without its bookkeeping -> the logits [S K, V] of the rows of st.ctl"""
            with self._scope():
                st.prediction(self, S, *(c_void_p(st.ctl.data_ptr() + 8 * S * i) for i in range(4)))
                return st.joint_logits(self, *(c_void_p(st.ctl.data_ptr() + 8 * (4 * S + R * i)) for i in range(3)))

        def body():
            with self._scope():    # (the scope pins the stream the calls go to: the book kernel belongs to the capture as well)
                logits = launches()
                ops.rnnt_greedy_batch_book(st.row_off, K, blank, max_seq_len, logits, st.ctl, st.state, st.hyp, st.align, st.lens,
                                           st.live)

        st.launches = launches     # (tests run the same launches step by step and keep the books on the host)
        ops.rnnt_greedy_batch_start(st.row_off, K, eos, max_seq_len, st.ctl, st.state, st.lens, st.live)   # (row_off all zero)
        st.graph, _ = lockstep.capture_after_warmup(body, st.e.device)
        tab[key] = st
        return st

    def _rnnt_greedy_batch_load(self, eouts, elens, K, blank, eos, max_seq_len):
        """one chunk's searches ready for their first step: the buffers and graph, the staging (RowsStep.stage), the control words
        of step 0"""
        st = self._rnnt_greedy_batch_graph(len(elens), K, blank, eos, max_seq_len, sum(elens), max(elens))
        st.stage(self, eouts, elens, range(len(elens)))
        ops.rnnt_greedy_batch_start(st.row_off, K, eos, max_seq_len, st.ctl, st.state, st.lens, st.live)
        return st

    def rnnt_greedy_batch(self, eouts, elens, blank, eos, max_seq_len=256, frames_per_step=None, poll_block=None):
        """time-synchronous greedy search (rnn_transducer.py:194-240) of a BATCH in lockstep, the bookkeeping on the device
        (csrc/rnnt_greedy_batch.hip): eouts [B, Tmax, d], utterance b is searched over its own elens[b] frames -> (hyps, aligns)
        as rnnt_greedy returns them.  One step -- LSTM layers on S rows, joint and output product on S K rows (K =
        frames_per_step consecutive frames of every live search against its current state), book -- is captured once per (S, K)
        and replayed: ceil(max(elens) / K) times (no search can finish sooner), then in blocks of poll_block steps with one
        4-byte read of the live counter after each, until it is zero; never more than max(elens) + max_seq_len + 1 steps.
        Batches are searched in chunks of _GREEDY_BATCH_ROWS // K utterances.  A model outside the rows kernels' limits is a
        ValueError naming the reason (rnnt_greedy_batch_why_not); rnnt_greedy takes any model.  self.rnnt_greedy_batch_stats:
        the replays and counter reads of the last call."""
        K = self._GREEDY_BATCH_K if frames_per_step is None else int(frames_per_step)
        block = self._GREEDY_BATCH_POLL if poll_block is None else int(poll_block)
        if not 1 <= K <= ops.RNNT_GREEDY_BATCH_MAX_FRAMES:
            raise ValueError(f"rnnt_greedy_batch: frames_per_step {K} is outside 1..{ops.RNNT_GREEDY_BATCH_MAX_FRAMES}")
        if block < 1:
            raise ValueError(f"rnnt_greedy_batch: poll_block {block} is below 1")
        elens = [int(v) for v in elens]
        B = eouts.shape[0]
        assert len(elens) == B and all(0 <= n <= eouts.shape[1] for n in elens), (elens, tuple(eouts.shape))
        why = self.rnnt_greedy_batch_why_not()
        if why is not None:
            raise ValueError(f"rnnt_greedy_batch: {why}")
        stats = self.rnnt_greedy_batch_stats = dict(steps=0, polls=0, bound=0)
        hyps, aligns = [], []
        cap = max(1, self._GREEDY_BATCH_ROWS // K)
        with self._scope(), torch.no_grad():
            self.arena.refresh_shadow()
            for b0 in range(0, B, cap):
                lens = elens[b0:b0 + cap]
                st = self._rnnt_greedy_batch_load(eouts[b0:b0 + cap], lens, K, blank, eos, max_seq_len)
                bound = max(lens) + max_seq_len + 1
                steps, todo = 0, -(-max(lens) // K)
                while True:
                    for _ in range(todo):
                        st.graph.replay()
                    steps += todo
                    live = int(st.live.item())
                    stats["polls"] += 1
                    if live == 0:
                        break
                    todo = min(block, bound - steps)
                    if todo <= 0:
                        raise RuntimeError(f"rnnt_greedy_batch: {live} searches still live after {steps} steps (bound {bound})")
                stats["steps"] += steps
                stats["bound"] += bound
                n, hyp, align = st.lens.tolist(), st.hyp.cpu(), st.align.cpu()
                hyps += [hyp[s, :n[s][0]].tolist() for s in range(len(lens))]
                aligns += [align[s, :n[s][1]].tolist() for s in range(len(lens))]
        return hyps, aligns

    # ---- beam search, the books on the host: one utterance (beam_host_loop with the launch chain's or the replayed round) ---------
    def rnnt_beam_search(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False, lm=None, lm_weight=0,
                         len_weight=0):
        """alignment-length synchronous beam search for ONE utterance (rnn_transducer.py:242-325,348-359): the expansion round as a
        replayed HIP graph (_rnnt_beam_search_graph) unless EMOASR_RNNT_BEAM_GRAPH=0 or the utterance does not fit its static
        buffers; then the launch chain below.  return_scores: (hyps, float64 scores) instead of hyps (tests compare the two forms).
        lm with lm_weight > 0: shallow fusion through the launch chain, the only host form that fuses;
        without it lm_weight and len_weight are not read."""
        if lm is not None and lm_weight > 0:
            return self._rnnt_beam_search_chain(eouts, beam_width, blank, eos, num_expands, return_scores, lm, lm_weight, len_weight)
        T = eouts.shape[1]
        if (os.environ.get("EMOASR_RNNT_BEAM_GRAPH", "1") != "0" and beam_width <= 16
                and (T * num_expands + 2) * beam_width + 1 <= self._BEAM_POOL - 16 and T <= self._BEAM_TMAX):
            return self._rnnt_beam_search_graph(eouts, beam_width, blank, eos, num_expands, return_scores)
        return self._rnnt_beam_search_chain(eouts, beam_width, blank, eos, num_expands, return_scores)

    _BEAM_POOL, _BEAM_TMAX = 32768, 4096   # (the pool's last 16 slots are the warm-up's scratch, never a hypothesis's)

    def _rnnt_beam_round_graph(self, beam_width, nb, blank):
        """the device work of ONE expansion round over nb live hypotheses, captured once as a HIP graph over static buffers:
        control words (last labels, source / destination slots of the LSTM states in the pool, frame index) come in through
        `ctl`, (blank log-prob, top-k log-probs, top-k ids) per hypothesis go out through `out`.  The host loop pays one replay
        per round instead of ~12 C-ABI calls, ~16 allocations and the torch glue (246 us per round, host-bound:
        tools/l4_beam_prof.py).  Round 5: the captured body is five launches (csrc/rnnt_beam.hip) that read the control words from
        the PINNED host record and write the result record into pinned host memory -- no upload / download launches: 124 -> 66 us
        per round; EMOASR_RNNT_BEAM_FUSED=0 captures the launch chain with explicit copies as before."""
        from .. import lib
        st = self.__dict__.setdefault("_beam_static", None)
        A, J, H, nl = self.arena, self.r_J, self.r_H, self.r_nl
        dev = A.flat.device
        if st is None:
            st = self._beam_static = _Stash()
            st.ph = [torch.zeros(self._BEAM_POOL, H, device=dev, dtype=self.dtype) for _ in range(nl)]
            st.pc = [torch.zeros(self._BEAM_POOL, H, device=dev, dtype=torch.float32) for _ in range(nl)]
            st.e = torch.zeros(self._BEAM_TMAX, J, device=dev, dtype=self.dtype)
            st.ctl = torch.zeros(3 * 16 + 1, device=dev, dtype=torch.int64)
            st.ctl_host = torch.zeros(3 * 16 + 1, dtype=torch.int64).pin_memory()
            st.out = torch.zeros(16, 1 + 2 * 16, device=dev, dtype=torch.float32)
            st.out_host = torch.zeros(16, 1 + 2 * 16, dtype=torch.float32).pin_memory()
            st.hj = torch.zeros(16, J, device=dev, dtype=self.dtype)
            st.bias = [self._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(nl)]   # (refreshed per search, below)
            st.graphs = {}
        key = (beam_width, nb, blank)
        if key in st.graphs:
            return st, st.graphs[key]

        # a model outside the fused kernels' LDS plans decodes through the launch chain as before round 5 -- decided here from the
        # limits, and once more by the warm-up below (an entry point that still refuses turns the round into the chain body
        # instead of failing the search)
        nin_max = max(A.w(f"decoder.rnns.{l}.weight_ih_l0").shape[1] for l in range(nl)) if nl else 0
        st.zero_copy = (os.environ.get("EMOASR_RNNT_BEAM_FUSED", "1") != "0" and nl >= 1
                        and round_fits(self.dtype, A.w("decoder.output.weight").shape[0], nin_max, H))

        def body_fused():
            # csrc/rnnt_beam.hip: five launches -- one per LSTM layer (gather, both products, cell, scatter), the joint input, the
            # output layer, the pick (log-softmax + blank + top-k into the result record)
            with self._scope():
                # zero-copy hand-off: the kernels read the control words straight from the PINNED host record (each word once,
                # through LDS) and the pick kernel writes the result record into pinned host memory -- no upload / download
                # launches (two ~5 us copy kernels + their enqueue per round)
                dtc = ops.dt(st.ph[0])
                words = lambda base: tuple(c_void_p(base.data_ptr() + 8 * o) for o in (0, 16, 32, 48))
                h_ids, h_src, h_dst, _ = words(st.ctl_host)       # the first launch reads the host record (and copies it over) ...
                p_ids, p_src, p_dst, p_t = words(st.ctl)          # ... the later ones its device twin
                emb = A.w("decoder.embed.weight")
                xtab, ldx, xidx = emb, emb.shape[1], h_ids
                for l in range(nl):
                    name = f"decoder.rnns.{l}"
                    w_ih, w_hh = A.w(name + ".weight_ih_l0"), A.w(name + ".weight_hh_l0")
                    first = l == 0
                    lib.call("emoasr_rnnt_beam_lstm", dtc, nb, w_ih.shape[1], H, ops._p(xtab), ldx, xidx, ops._p(w_ih), ops._p(w_hh),
                             ops._p(st.bias[l]), ops._p(st.ph[l]), ops._p(st.pc[l]), h_src if first else p_src,
                             h_dst if first else p_dst, ops._p(st.ctl_host) if first else None, ops._p(st.ctl) if first else None,
                             st.ctl.numel() if first else 0, ops._stream())
                    xtab, ldx, xidx = st.ph[l], H, p_dst
                hj = st.hj[:nb]
                lib.call("emoasr_rnnt_beam_joint", dtc, nb, H, J, self._BEAM_TMAX, ops._p(st.ph[nl - 1]), p_dst,
                         ops._p(A.w("decoder.w_dec.weight")), ops._p(A.p("decoder.w_dec.bias")), ops._p(st.e), p_t, ops._p(hj),
                         ops._stream())
                logits = ops.gemm_nt(hj, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
                lib.call("emoasr_rnnt_beam_pick", dtc, nb, logits.shape[1], beam_width, blank, ops._p(logits), logits.stride(0),
                         ops._p(st.out_host), st.out_host.stride(0), ops._stream())

        def body():
            if st.zero_copy:      # (the fused body: it hands its records over without copies)
                return body_fused()
            with self._scope():
                ids = st.ctl[:nb].to(torch.int32).view(1, nb)
                src, dst, t = st.ctl[16:16 + nb], st.ctl[32:32 + nb], st.ctl[48:49]
                prev = ([p.index_select(0, src) for p in st.ph], [p.index_select(0, src) for p in st.pc])
                dout, (nh, nc), _ = self.rnnt_recurrency(ids, prev, False, False)
                for l in range(nl):
                    st.ph[l].index_copy_(0, dst, nh[l])
                    st.pc[l].index_copy_(0, dst, nc[l])
                g = ops.gemm_nt(dout.view(nb, H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
                h = ops.joint_tanh(st.e.index_select(0, t).view(1, 1, J), g.view(1, nb, J))
                logits = ops.gemm_nt(h.view(nb, J), A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
                lp = ops.log_softmax(logits)
                vals, idx, _ = ops.topk(lp[:, 1:], beam_width)
                st.out[:nb, 0:1].copy_(lp[:, blank:blank + 1])
                st.out[:nb, 1:1 + beam_width].copy_(vals)
                st.out[:nb, 1 + beam_width:1 + 2 * beam_width].copy_(idx)

        def warm():
            try:
                body()
            except lib.EmoasrHipError:
                if not st.zero_copy:
                    raise
                st.zero_copy = False   # outside a fused kernel's limits: the launch chain's body
                st.ctl.copy_(st.ctl_host)
                body()

        # the warm-up runs the body for real: give it control words of its own -- label 0, the zero state of slot 0 as source and
        # the pool's reserved scratch slots as destination -- so that it never writes a slot a live hypothesis reads (the
        # caller uploads the round's words after this call, before the replay)
        st.ctl_host.zero_()
        st.ctl_host[32:32 + 16] = torch.arange(self._BEAM_POOL - 16, self._BEAM_POOL)
        st.ctl.copy_(st.ctl_host)
        st.graphs[key], _ = lockstep.capture_after_warmup(body, dev, warm)
        return st, st.graphs[key]

    def _rnnt_beam_search_graph(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False):
        """the search of rnnt_beam_search with every expansion round's device work replayed from a HIP graph; the bookkeeping stays
        on the host (beam_host_loop), as in the reference and in _rnnt_beam_search_chain, whose arithmetic and launch order the
        captured body repeats.  A hypothesis' state token is its slot in the pool."""
        import numpy as np
        with self._scope(), torch.no_grad():
            A = self.arena
            A.refresh_shadow()
            T = eouts.shape[1]
            e_all = ops.gemm_nt(eouts[0], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))  # [T,J]
            st, _ = self._rnnt_beam_round_graph(beam_width, 1, blank)
            st.e[:T].copy_(e_all)
            for l in range(self.r_nl):   # bias_ih + bias_hh of the current weights, into the buffers the captured launches read
                st.bias[l].copy_(self._lstm_bias(f"decoder.rnns.{l}"))
            for l in range(self.r_nl):   # slot 0: the zero state every search starts from
                st.ph[l][0].zero_()
                st.pc[l][0].zero_()
            ctl, out = st.ctl_host.numpy(), st.out_host.numpy()
            stream = torch.cuda.current_stream()
            free = [1]      # the first slot no hypothesis has been given

            def round(live, t, v, last):
                nb, base = len(live), free[0]
                _, graph = self._rnnt_beam_round_graph(beam_width, nb, blank)
                for i, (hyp, _, slot) in enumerate(live):
                    ctl[i], ctl[16 + i], ctl[32 + i] = hyp[-1], slot, base + i
                ctl[48] = t
                if not st.zero_copy:
                    st.ctl.copy_(st.ctl_host, non_blocking=True)
                graph.replay()
                if not st.zero_copy:
                    st.out_host.copy_(st.out, non_blocking=True)
                stream.synchronize()
                free[0] += nb
                return out[:nb].astype(np.float64), lambda i: base + i

            return beam_host_loop(round, T, beam_width, num_expands, eos, 0, return_scores)

    def _rnnt_lm_rows(self, lm, live, rows, states, V):
        """shallow fusion, host form: the LM's log-probability row (f32 [V] on the device: log_softmax over the LM's vocabulary,
        cut to the model's) of every live hypothesis, from lm.predict -- the stateful one-step call for the RNN LM (the state
        after a label sequence is kept per label tuple; a hypothesis' parent was live one round earlier), the whole prefix for
        the Transformer LM -- cached per label tuple in rows / states -> [nb, V]"""
        todo = []
        for hyp, _, _ in live:
            key = tuple(hyp)
            if key not in rows and key not in todo:
                todo.append(key)
        if todo:
            if getattr(lm, "stateful", False):
                prev = None
                if any(len(k) > 1 for k in todo):
                    zero = lm.zero_states(1, self.arena.flat.device)
                    parts = [states[k[:-1]] if len(k) > 1 else zero for k in todo]
                    prev = (torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1))
                logp, (h, c) = lm.predict(torch.tensor([[k[-1]] for k in todo]), [1] * len(todo), prev)
                for i, k in enumerate(todo):
                    states[k] = (h[:, i:i + 1].clone(), c[:, i:i + 1].clone())
            else:
                n = max(len(k) for k in todo)
                ys = torch.zeros(len(todo), n, dtype=torch.int64)
                for i, k in enumerate(todo):
                    ys[i, :len(k)] = torch.tensor(k)
                logp, _ = lm.predict(ys, [len(k) for k in todo], None)
            assert logp.shape[1] >= V, f"the LM's vocabulary ({logp.shape[1]}) is smaller than the model's ({V})"
            for i, k in enumerate(todo):
                rows[k] = logp[i, :V].to(torch.float32).clone()
        return torch.stack([rows[tuple(hyp)] for hyp, _, _ in live])

    def _rnnt_beam_search_chain(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False, lm=None, lm_weight=0,
                                len_weight=0):
        """alignment-length synchronous beam search for ONE utterance (rnn_transducer.py:242-325,348-359).

        lm with lm_weight > 0: shallow fusion (the reference's search takes the arguments and never reads
        them).  The non-blank candidates of a live hypothesis are the beam_width best v >= 1 of f = lp + mu * lq in torch f32 (mu
        rounded to f32, product and sum rounded separately), lq the LM's row for the hypothesis' label sequence (_rnnt_lm_rows); the
        blank extension takes no LM term; at the end score + len_weight * len(hyp) and a stable re-sort (rnnt_len_expand).  A
        masked LM is refused.  Without an LM (or lm_weight <= 0) neither weight is read.

        eouts [1,T,d].  Per frame up to `num_expands` rounds; each round is one batched prediction-network
        step over the live hypotheses (every hypothesis keeps the LSTM state from before its last label, as
        the reference does: its state token is (the state tensors of a round, its row in them)), one joint + output GEMM,
        log-softmax and top-k on the device, and ONE D2H of (blank score, k scores, k ids) per live hypothesis; the bookkeeping
        stays on the host like the reference (beam_host_loop).
        Returns the surviving label sequences best-first, including the leading <sos>."""
        with self._scope(), torch.no_grad():
            A, J, H, nl = self.arena, self.r_J, self.r_H, self.r_nl
            A.refresh_shadow()
            dev = eouts.device
            T = eouts.shape[1]
            e_all = ops.gemm_nt(eouts[0], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))  # [T,J]
            cdt = e_all.dtype
            zero = ([torch.zeros(1, H, device=dev, dtype=cdt) for _ in range(nl)],
                    [torch.zeros(1, H, device=dev, dtype=torch.float32) for _ in range(nl)])
            fuse = lm is not None and lm_weight > 0
            if fuse:
                from ..modeling.lm import require_next_token_lm
                require_next_token_lm(lm, lm_weight)
                mu = torch.tensor(float(lm_weight), device=dev, dtype=torch.float32)
                lm_rows, lm_states = {}, {}

            def gather(live):
                srcs = {id(st[0]): st[0] for _, _, st in live}
                if len(srcs) == 1:
                    (hs, cs), = srcs.values()
                    rows = [st[1] for _, _, st in live]
                    if rows == list(range(hs[0].shape[0])):
                        return hs, cs
                    ix = torch.tensor(rows, device=dev)
                    return [h.index_select(0, ix) for h in hs], [c.index_select(0, ix) for c in cs]
                hs = [torch.cat([st[0][0][l][st[1]:st[1] + 1] for _, _, st in live]) for l in range(nl)]
                cs = [torch.cat([st[0][1][l][st[1]:st[1] + 1] for _, _, st in live]) for l in range(nl)]
                return hs, cs

            def round(live, t, v, last):
                nb = len(live)
                prev = gather(live)
                ids = h2d_i32([[hyp[-1] for hyp, _, _ in live]], dev)  # [1,nb]
                dout, after, _ = self.rnnt_recurrency(ids, prev, False, False)
                g = ops.gemm_nt(dout.view(nb, H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
                h = ops.joint_tanh(e_all[t].view(1, 1, J), g.view(1, nb, J))
                logits = ops.gemm_nt(h.view(nb, J), A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
                lp = ops.log_softmax(logits)
                if last:
                    return lp[:, blank].cpu().double().numpy().reshape(nb, 1), None
                cand = lp
                if fuse:   # two f32 roundings: the product, then the sum (csrc/rnnt_beam_lm.hip does the same)
                    cand = lp + mu * self._rnnt_lm_rows(lm, live, lm_rows, lm_states, lp.shape[1])
                vals, idx, _ = ops.topk(cand[:, 1:], beam_width)
                host = torch.cat([lp[:, blank:blank + 1], vals, idx.to(torch.float32)], 1).cpu().double().numpy()
                return host, lambda i: (after, i)

            return beam_host_loop(round, T, beam_width, num_expands, eos, (zero, 0), return_scores, len_weight if fuse else None)

    # ---- beam search, the books on the device: the batch in lockstep (csrc/rnnt_beam_book.hip, DESIGN.md sections 22, 25, 30) -----
    _BEAM_BATCH_CAP = 64   # searches per launch chain: S W <= 1024 rows, S (E + 1) W state slots per layer (25 MB at H = 512, W = 16)

    _BEAM_POOL_BUDGET = 256 << 20   # bytes of state pools (prediction network + LM) one chunk of fused searches may hold

    def rnnt_beam_lm_why_not(self, lm):
        """why the batched device search cannot fuse this LM (None: it can).  The LM's LSTM layers run through
        emoasr_rnnt_beam_lstm_rows beside the prediction network's and csrc/rnnt_beam_lm.hip ranks the candidates: an RNN LM
        (lm_type == "rnn") of the engine's compute dtype and product mode, its layer sizes inside that kernel's LDS plans, its
        vocabulary at least the model's"""
        why = lockstep.lm_type_why_not(lm, "rnn") or lockstep.lm_compute_why_not(self, lm, (torch.float32, torch.bfloat16))
        if why is not None:
            return why
        V_ = self.arena.w("decoder.output.weight").shape[0]
        if lm.L < 1 or not (lstm_rows_fits(self.dtype, [lm.E, lm.H], lm.H) and joint_rows_fits(lm.H)):
            return f"the LM's sizes (embedding {lm.E}, hidden {lm.H}, layers {lm.L}) are outside emoasr_rnnt_beam_lstm_rows' limits"
        if lm.V < V_:
            return f"the LM's vocabulary ({lm.V}) is smaller than the model's ({V_})"
        return None

    _TLM_POOL_BUDGET = 8 << 30     # bytes of K / V node pools one chunk of Transformer-LM fused searches may hold (the joint search's
                                   # cache budget, not the 256 MB of the LSTM pools: a node is layers x d x 2 values)

    def rnnt_beam_tlm_why_not(self, lm):
        """why the batched device search cannot fuse this LM over the prefix tree (None: it can).  The LM's step
        is emoasr_lm_tree_step (csrc/lm_tree.hip) beside the prediction network's launches: a causal Transformer LM (lm_type ==
        "transformer") of the engine's compute dtype and product mode, its vocabulary at least the model's, its heads and its longest
        prefix inside emoasr_lm_tree_attn's plan.  rnnt_beam_lm_why_not keeps answering for the RNN form."""
        from .. import lm_tree
        why = lockstep.lm_type_why_not(lm, "transformer")
        if why is None and not getattr(lm, "causal", False):
            why = "there is no causal LM (the prefix tree steps p(next token | prefix))"
        why = why or lockstep.lm_compute_why_not(self, lm, (torch.float32, torch.bfloat16))
        if why is not None:
            return why
        P = lm.params
        V_ = self.arena.w("decoder.output.weight").shape[0]
        if P.vocab_size < V_:
            return f"the LM's vocabulary ({P.vocab_size}) is smaller than the model's ({V_})"
        if not lm_tree.head_ok(P.hidden_size, P.num_attention_heads):
            return (f"the LM's heads ({P.hidden_size} over {P.num_attention_heads}) are outside emoasr_lm_tree_attn's plan "
                    f"(8 .. 128 wide, a multiple of 8)")
        if lm_tree.attn_lds_bytes(P.max_seq_len) > lm_tree.LDS_BYTES:
            return (f"max_seq_len {P.max_seq_len} needs {lm_tree.attn_lds_bytes(P.max_seq_len)} bytes of LDS in emoasr_lm_tree_attn "
                    f"({lm_tree.LDS_BYTES} at most)")
        return None

    @staticmethod
    def _tlm_frames(longest):
        """the frame capacity the tree's buffers are sized for: the longest utterance, rounded up to 64 frames"""
        return max(64, -(-int(longest) // 64) * 64)

    def rnnt_beam_tlm_chunk_capacity(self, W, E, lm, longest):
        """searches per launch chain with the Transformer LM: _BEAM_BATCH_CAP, and no more than hold their tree -- W (E - 1) frames + 1
        nodes per search (the worst case: every fused round steps W rows) of (K, V) x layers x d values, the lists of its (E + 1) W
        slots and the prediction network's pools -- inside _TLM_POOL_BUDGET; never below one"""
        from .. import lm_tree
        P = lm.params
        esz = 2 if self.dtype == torch.bfloat16 else 4
        frames = self._tlm_frames(longest)
        nodes, Lcap = lm_tree.node_cap(W, E, frames), lm_tree.list_cap(E, frames, P.max_seq_len)
        per_search = (2 * P.num_layers * nodes * P.hidden_size * esz + (E + 1) * W * (Lcap + 1) * 4
                      + (E + 1) * W * (esz + 4) * self.r_nl * self.r_H)
        return max(1, min(self._BEAM_BATCH_CAP, self._TLM_POOL_BUDGET // per_search))

    def rnnt_beam_device_ok(self, beam_width, num_expands=3, lm=None):
        """does the model fit the batched search's round kernels?  (the limits of the fused round, round_fits, and of the
        bookkeeping kernel: beam_width <= 16, beam_width <= V - 1; with an LM to fuse, rnnt_beam_lm_why_not as well)"""
        A, H, nl = self.arena, self.r_H, self.r_nl
        V_ = A.w("decoder.output.weight").shape[0]
        nin_max = max(A.w(f"decoder.rnns.{l}.weight_ih_l0").shape[1] for l in range(nl)) if nl else 0
        if lm is not None and self.rnnt_beam_lm_why_not(lm) is not None:
            return False
        return (nl >= 1 and round_fits(self.dtype, V_, nin_max, H) and 1 <= beam_width <= min(ops.RNNT_BEAM_MAX_WIDTH, V_ - 1)
                and 1 <= num_expands <= ops.RNNT_BEAM_MAX_EXPANDS)

    def rnnt_beam_chunk_capacity(self, W, E, lm=None):
        """searches per launch chain: _BEAM_BATCH_CAP, and with an LM no more than hold their state pools -- (E + 1) W slots per
        search of (h in the compute dtype, c in f32) per layer of both networks -- inside _BEAM_POOL_BUDGET; never below one"""
        if lm is None:
            return self._BEAM_BATCH_CAP
        esz = 2 if self.dtype == torch.bfloat16 else 4
        per_search = (E + 1) * W * (esz + 4) * (self.r_nl * self.r_H + lm.L * lm.H)
        return max(1, min(self._BEAM_BATCH_CAP, self._BEAM_POOL_BUDGET // per_search))

    @staticmethod
    def rnnt_len_expand(hyps, scores, len_weight):
        """the finish of a fused search: final = score + len_weight * len(hyp) in doubles (the hypothesis with its leading <sos>,
        decoders/transformer.py:274), then a stable descending re-sort"""
        return lockstep.expand_len_weights(hyps, scores, [len_weight], 0)[0]

    def rnnt_beam_search_batch(self, eouts, elens, beam_width, blank, eos, num_expands=3, lm=None, lm_weights=None, len_weights=None,
                               tlm_fusion="host"):
        """alignment-length synchronous beam search for a BATCH (rnn_transducer.py:242-325 per utterance; the reference asserts a
        batch of one): eouts [B, Tmax, d], utterance b is searched over its own elens[b] frames -> (hyps[b][n], scores[b][n]),
        best first, hypotheses with the leading <sos>, float64 scores.  The bookkeeping runs on the device
        (csrc/rnnt_beam_book.hip): one frame -- num_expands rounds of (LSTM layers, joint, output product, pick, book) over all
        S W rows -- is captured once per (S, W) and replayed max(elens) times without a synchronisation in between.  Batches above
        _BEAM_BATCH_CAP are searched in chunks.  A model outside the round kernels' limits is searched utterance by utterance
        through rnnt_beam_search.

        lm_weights (a list; None: the call above, unchanged): the shallow-fusion GRID ->
        (hyps[b][cell][n], scores[b][cell][n]), cells in lm_weight-outer, len_weight-inner order (len_weights None: [0]).  A search
        is an (utterance, lm_weight) pair: every distinct positive lm_weight of an utterance is searched once with the LM's LSTM
        stepped beside the prediction network's, all weights <= 0 (or no LM) are ONE search on the chain above.  The len_weights
        are a host expansion of a fused search's results (rnnt_len_expand); the search without the LM does not read them.  An LM
        or a width the device form cannot take is searched utterance by utterance through the host form.

        tlm_fusion ("host", the default: everything above, unchanged; or "device"; decoder.rnnt_tlm_fusion): with "device" a
        Transformer LM is fused on the device too, stepped over a prefix tree of K / V nodes in chunks of
        rnnt_beam_tlm_chunk_capacity searches; an LM or a width that form cannot take is then a ValueError naming the reason, and a
        search that outgrows the LM's positions or its node pool a RuntimeError naming the search.  self.rnnt_tlm_stats: the nodes
        every search of the last such call took, and their bound."""
        if tlm_fusion not in ("host", "device"):
            raise ValueError(f"emoasr_amd: rnnt_tlm_fusion is 'host' or 'device', not {tlm_fusion!r}")
        elens = [int(v) for v in elens]
        B = eouts.shape[0]
        assert len(elens) == B and all(0 <= n <= eouts.shape[1] for n in elens), (elens, tuple(eouts.shape))
        with self._scope():
            self.arena.refresh_shadow()
        if lm_weights is not None:
            return self._rnnt_beam_search_grid(eouts, elens, beam_width, blank, eos, num_expands, lm, lm_weights, len_weights,
                                               tlm_fusion)
        hyps, scores = [], []
        if not self.rnnt_beam_device_ok(beam_width, num_expands):
            for b in range(B):
                if elens[b] == 0:
                    h, s = [[eos]], [0.0]
                else:
                    h, s = self.rnnt_beam_search(eouts[b:b + 1, :elens[b]], beam_width, blank, eos, num_expands, return_scores=True)
                hyps.append(h)
                scores.append([float(v) for v in s])
            return hyps, scores
        for b0 in range(0, B, self._BEAM_BATCH_CAP):
            h, s = self._rnnt_beam_search_device(eouts[b0:b0 + self._BEAM_BATCH_CAP], elens[b0:b0 + self._BEAM_BATCH_CAP], beam_width,
                                                 blank, eos, num_expands)
            hyps += h
            scores += s
        return hyps, scores

    def _rnnt_beam_search_grid(self, eouts, elens, W, blank, eos, E, lm, lm_weights, len_weights, tlm_fusion="host"):
        """rnnt_beam_search_batch with lm_weights: lockstep.run_fusion_grid over (utterance, weight) pairs in chunks; the fused
        searches' results are expanded by rnnt_len_expand, the search without the LM does not read the len_weights.  tlm_fusion ==
        "device" sends a Transformer LM through the same chunks over the prefix tree instead of the host chain."""
        from ..modeling.lm import require_next_token_lm
        lm_weights = [float(a) for a in lm_weights]
        len_weights = [0.0] if len_weights is None else [float(v) for v in len_weights]
        require_next_token_lm(lm, max(lockstep.grid_cell_plan(lm_weights, len_weights, lm is not None)[0]))
        B = len(elens)

        tlm = tlm_fusion == "device" and getattr(lm, "lm_type", None) == "transformer"
        if tlm and any(a > 0 for a in lm_weights):      # asked for by name: no quiet detour through the host chain
            why = self.rnnt_beam_tlm_why_not(lm)
            if why is None and not self.rnnt_beam_device_ok(W, E):
                why = f"the model, beam_width {W} or num_expands {E} is outside the batched device search's limits"
            if why is not None:
                raise ValueError(f"emoasr_amd: rnnt_tlm_fusion = 'device' cannot fuse this LM: {why}")

        def search_fused(positive, weights, found):
            if not tlm and not self.rnnt_beam_device_ok(W, E, lm):      # the host chain, utterance by utterance
                for b in range(B):
                    for k in positive:
                        if elens[b] == 0:
                            found[b][k] = ([[eos]], [0.0])
                        else:
                            h, s = self._rnnt_beam_search_chain(eouts[b:b + 1, :elens[b]], W, blank, eos, E, True, lm, weights[k], 0)
                            found[b][k] = (h, [float(v) for v in s])
                return
            pairs = [(b, k) for b in range(B) for k in positive]
            if tlm:
                cap = self.rnnt_beam_tlm_chunk_capacity(W, E, lm, max(elens, default=0))
                self.rnnt_tlm_stats = dict(nodes=[], node_cap=0, lcap=0)
            else:
                cap = self.rnnt_beam_chunk_capacity(W, E, lm)
            for p0 in range(0, len(pairs), cap):
                chunk = pairs[p0:p0 + cap]
                h, s = self._rnnt_beam_search_device(eouts, elens, W, blank, eos, E, lm, [weights[k] for _, k in chunk],
                                                     [b for b, _ in chunk])
                for i, (b, k) in enumerate(chunk):
                    found[b][k] = (h[i], s[i])

        return lockstep.run_fusion_grid(B, lm_weights, len_weights, lm is not None,
                                        lambda: self.rnnt_beam_search_batch(eouts, elens, W, blank, eos, E), search_fused,
                                        lambda f, a: [self.rnnt_len_expand(*f, w) if a > 0 else f for w in len_weights])

    def _rnnt_beam_frame_graph(self, S, W, blank, eos, E, total, lm=None, longest=0):
        """static buffers of S searches of width W over <= st.rows frames in all (a RowsStep of (E + 1) W state slots per search,
        five control words per row: csrc/rnnt_beam_book.hip), and ONE FRAME of all of them (E rounds of LSTM layers, joint, output
        product, pick, book) captured as a HIP graph.  The warm-up runs the body with every search finished (no frames): every row
        is inactive, no state is touched.
        lm (an RNN LM that rnnt_beam_lm_why_not passes, _prepare()d by the caller): the fused frame -- every round but the last runs
        the LM's LSTM layers under the same control words on pools lh / lc beside ph / pc, gathers the top layer's h, forms the LM's
        logits and ranks the candidates with emoasr_rnnt_beam_pick_lm under the per-search weights st.mu; the last round of a frame
        grows no candidate and stays the chain without the LM.  Keyed by the LM's identity, sizes and parameter addresses.
        lm a Transformer LM that rnnt_beam_tlm_why_not passes, longest = the chunk's longest utterance: the
        same fused rounds with emoasr_lm_tree_advance + emoasr_lm_tree_step (csrc/lm_tree.hip) in place of the LSTM layers, gather and
        head product: the tree state st.tree and the node pools of st.tstep beside ph / pc under the same slot numbers, sized for
        st.tmax >= longest frames."""
        from .. import lib
        tab = self.__dict__.setdefault("_beam_batch_static", {})
        key = (S, W, blank, eos, E)
        tlm = lm is not None and getattr(lm, "lm_type", None) == "transformer"
        if tlm:
            LA, P = lm._arena, lm.params
            key += ("tlm", id(lm), P.vocab_size, P.hidden_size, P.num_attention_heads, P.intermediate_size, P.num_layers,
                    P.max_seq_len, LA.flat.data_ptr(), LA.shadow.data_ptr(), lm._pe.data_ptr())
        elif lm is not None:
            LA = lm._arena
            key += (id(lm), lm.V, lm.E, lm.H, lm.L, LA.flat.data_ptr(), LA.shadow.data_ptr(), lm._bias[0].data_ptr())
        st = tab.get(key)
        if st is not None and st.rows >= total and (not tlm or st.tmax >= longest):
            return st
        if st is not None:
            del tab[key], st       # (the pools of the outgrown record are released before the larger ones are taken)
        dev = self.arena.flat.device
        V_ = self.arena.w("decoder.output.weight").shape[0]
        R = S * W
        st = RowsStep(self, S, R, S * (E + 1) * W, total)
        st.ctl = torch.zeros(5, R, device=dev, dtype=torch.int64)
        st.rec = torch.zeros(R, 1 + 2 * W, device=dev, dtype=torch.float32)
        st.ws = torch.empty(lib.size_query("emoasr_rnnt_beam_ws_bytes", S, st.rows, W, E), device=dev, dtype=torch.uint8)
        st.status = torch.zeros(1, device=dev, dtype=torch.int32)
        if tlm:
            from .. import lm_tree
            st.tmax = self._tlm_frames(longest)
            # the node pools of ALL kept records stay inside the budget: the oldest records go first (a chunk of another size,
            # another width or another LM left them behind)
            st.tbytes = (2 * P.num_layers * S * lm_tree.node_cap(W, E, st.tmax) * P.hidden_size
                         * (2 if self.dtype == torch.bfloat16 else 4))
            held = [k for k, v in tab.items() if getattr(v, "tbytes", 0)]
            while held and sum(tab[k].tbytes for k in held) + st.tbytes > self._TLM_POOL_BUDGET:
                del tab[held.pop(0)]
            st.tree = lm_tree.TreeState(S, W, st.nslots, lm_tree.list_cap(E, st.tmax, lm.params.max_seq_len),
                                        lm_tree.node_cap(W, E, st.tmax), dev)
            st.tstep = lm_tree.TreeStep(lm, st.tree, c_void_p(st.ctl.data_ptr()), c_void_p(st.ctl.data_ptr() + 8 * R * 2))
            st.mu = torch.zeros(S, device=dev, dtype=torch.float32)
        elif lm is not None:
            st.lh = [torch.zeros(st.nslots, lm.H, device=dev, dtype=self.dtype) for _ in range(lm.L)]
            st.lc = [torch.zeros(st.nslots, lm.H, device=dev, dtype=torch.float32) for _ in range(lm.L)]
            st.lmh = torch.zeros(R, lm.H, device=dev, dtype=self.dtype)
            st.mu = torch.zeros(S, device=dev, dtype=torch.float32)

        def body():
            with self._scope():
                dtc = ops.dt(st.ph[0])
                p_lab, p_src, p_dst, p_act, p_row = (c_void_p(st.ctl.data_ptr() + 8 * R * i) for i in range(5))
                for v in range(E):
                    fuse = lm is not None and v < E - 1
                    st.prediction(self, R, p_lab, p_src, p_dst, p_act)
                    if fuse and tlm:
                        # the lists of the destination slots, a node per live row; like the LSTM rows kernel this relies on the book
                        # kernel's mark and sweep: no live row's source slot is a destination slot of the same round
                        st.tree.advance(p_src, p_dst, p_act)
                        lm_logits = st.tstep()
                    elif fuse:
                        LA = lm._arena
                        st.lstm_layers(R, LA.w("lm.embed.weight"), [lm._w(l) for l in range(lm.L)], lm._bias, st.lh, st.lc, lm.H,
                                       p_lab, p_src, p_dst, p_act)
                    logits = st.joint_logits(self, p_dst, p_act, p_row)
                    if fuse:
                        if not tlm:
                            lib.call("emoasr_rnnt_beam_gather_rows", dtc, R, lm.H, ops._p(st.lh[lm.L - 1]), st.nslots, p_dst, p_act,
                                     ops._p(st.lmh), ops._stream())
                            lm_logits = ops.gemm_nt(st.lmh, LA.w("lm.output.weight"), bias=LA.p("lm.output.bias"))
                        lib.call("emoasr_rnnt_beam_pick_lm", dtc, R, V_, lm_logits.shape[1], W, blank, W, ops._p(logits), logits.stride(0),
                                 ops._p(lm_logits), lm_logits.stride(0), ops._p(st.mu), p_act, ops._p(st.rec), st.rec.stride(0),
                                 ops._stream())
                    else:
                        lib.call("emoasr_rnnt_beam_pick", dtc, R, V_, W, blank, ops._p(logits), logits.stride(0), ops._p(st.rec),
                                 st.rec.stride(0), ops._stream())
                    ops.rnnt_beam_book(st.row_off, W, E, V_, eos, st.rec, st.ctl, st.ws, st.status)

        ops.rnnt_beam_start(st.row_off, W, E, V_, eos, st.ctl, st.ws, st.status)   # (row_off all zero: every search finished)
        st.graph, _ = lockstep.capture_after_warmup(body, dev)
        tab[key] = st
        return st

    def _rnnt_beam_search_device(self, eouts, elens, W, blank, eos, E, lm=None, mus=None, sutt=None):
        """one chunk of rnnt_beam_search_batch: S <= _BEAM_BATCH_CAP searches, one per utterance -- or, with sutt, search s over
        utterance sutt[s] (RowsStep.stage).  lm, mus: the fused chain with the LM weight mus[s] of search s (f32-rounded on the
        device; 0 ranks by the model alone, through the same launches)."""
        with self._scope(), torch.no_grad():
            sutt = list(range(len(elens))) if sutt is None else list(sutt)
            lens = [elens[b] for b in sutt]
            S, total, longest = len(lens), sum(lens), max(lens)
            V_ = self.arena.w("decoder.output.weight").shape[0]
            tlm = lm is not None and getattr(lm, "lm_type", None) == "transformer"
            if lm is not None:
                assert len(mus) == S and (self.rnnt_beam_tlm_why_not(lm) if tlm else self.rnnt_beam_lm_why_not(lm)) is None
                lm._prepare()      # (compute-dtype weights current, bias_ih + bias_hh / the position table rebuilt in place)
            st = self._rnnt_beam_frame_graph(S, W, blank, eos, E, total, lm, longest)
            st.stage(self, eouts, elens, sutt)
            if lm is not None:
                st.mu.copy_(torch.tensor([float(m) for m in mus], dtype=torch.float32))
            if tlm:
                st.tree.reset()    # llen = 0 in every slot (a search's first slot is its zero state), no node taken, no bit raised
            elif lm is not None:
                for l in range(lm.L):
                    st.lh[l].view(S, -1, lm.H)[:, 0].zero_()
                    st.lc[l].view(S, -1, lm.H)[:, 0].zero_()
            st.status.zero_()
            ops.rnnt_beam_start(st.row_off, W, E, V_, eos, st.ctl, st.ws, st.status)
            for _ in range(longest):
                st.graph.replay()
            if tlm:    # a raised bit is an error naming the search and the limit, as the host form's max_seq_len assertion is
                st.tree.raise_for_status("rnnt_beam_search_batch (Transformer-LM fusion)",
                                         [f"search {s} (utterance {b}, lm_weight {float(mus[s]):g})" for s, b in enumerate(sutt)])
                stats = self.rnnt_tlm_stats = getattr(self, "rnnt_tlm_stats", None) or dict(nodes=[], node_cap=0, lcap=0)
                stats["nodes"] += st.tree.nnodes.tolist()
                stats["node_cap"], stats["lcap"] = st.tree.node_cap, st.tree.Lcap
            hyps, scores, _ = ops.rnnt_beam_finish(st.row_off, W, E, V_, eos, longest * (E - 1), st.ws, st.status)
            return hyps, scores
