"""Joint CTC / attention beam search (+ Transformer-LM shallow fusion) with the WHOLE output step on the device.

Same behaviour as modeling/beam_search.py:joint_beam_search (the reference's decoders/transformer.py:161-294 with its
quirks), but per output step the host makes ONE C-ABI call (csrc/decode_rt.hip:emoasr_joint_beam_step) and reads ONE
flag back:
  * the decoder and the LM process one position per hypothesis against self-attention K / V caches, re-ordered on the
    device by parent beam (no prefix recomputation);
  * candidate selection, CTC prefix re-scoring, the per-beam and global prunes, <eos> handling and the result list are
    device kernels (emoasr_beam_update: numpy-float32 candidate scores, double hypothesis scores, stable orders);
  * the token sequences are rebuilt once, at the end, from the per-step (parent, token) history.

joint_beam_search_device_batch (second half of this file) runs the same search for S utterances in lockstep: rows s * W ..
s * W + W - 1 belong to utterance s, one captured step serves them all.
"""
import ctypes
import gc
import math
import os
import time

import numpy as np
import torch

from .. import lib, lockstep, ops
from ..decode_rt import DecoderStepRuntime, LMStepRuntime, _lin, _ln
from ..engine import h2d_i32
from ..lockstep import (_STEP_DEADLINE_S, _yield, batch_nbest_from_pack, batch_pack_sizes, batch_step_reported,  # noqa: F401
                        expand_len_weights, grid_cell_plan, grid_chunk_plan)
from .functions import _engine_of
from .lm import require_next_token_lm

CTC_BEAM_WIDTH_RATIO = 1.5


class _Buffers:
    """device buffers of one search configuration (beam, candidates, Lmax, model sizes), reused across utterances"""

    def __init__(self, dev, dtype, bw, cw, Lmax, V, dnl, dd, lnl, ld):
        i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.state = i32(4)                       # pos, n_alive, n_results, done
        self.ids, self.parent, self.pcand = i32(bw), i32(bw), i32(bw)
        self.last, self.outlen, self.klens = i32(bw), i32(bw), i32(bw)
        self.score = torch.zeros(bw, device=dev, dtype=torch.float64)
        self.score_ctc = f32(bw)
        self.hist_parent, self.hist_token = i32(Lmax, bw), i32(Lmax, bw)
        self.res_score = torch.zeros(bw, device=dev, dtype=torch.float64)
        self.res_step, self.res_parent = i32(bw), i32(bw)
        self.vals, self.cands, self.lm_at, self.psi = f32(bw, cw), i32(bw, cw), f32(bw, cw), f32(bw, cw)
        self.scores_pre = f32(bw, V)
        self.logits = torch.zeros(bw, V, device=dev, dtype=dtype)
        self.lm_logp = f32(bw, V)
        self.dec_k = torch.zeros(2, dnl, bw, Lmax, dd, device=dev, dtype=dtype)
        self.dec_v = torch.zeros_like(self.dec_k)
        self.lm_k = torch.zeros(2, max(lnl, 1), bw, Lmax, ld, device=dev, dtype=dtype)
        self.lm_v = torch.zeros_like(self.lm_k)
        # the flag the host polls: a pinned copy of `state`
        self.state_host = torch.zeros(4, dtype=torch.int32).pin_memory()


def joint_beam_search_device(dec, eouts, elens, beam_width, len_weight=0, lm=None, lm_weight=0, decode_ctc_weight=0):
    require_next_token_lm(lm, lm_weight)
    eng = _engine_of(dec)
    assert eouts.shape[0] == 1, "beam search decodes one utterance at a time (decoders/transformer.py:181)"
    V, eos, blank = dec.vocab_size, dec.eos_id, dec.blank_id
    dev = eouts.device
    T = eouts.shape[1]
    use_ctc = decode_ctc_weight > 0
    use_lm = lm is not None and lm_weight > 0 and hasattr(lm, "predict_device")
    bw = beam_width
    cw = min(V, int(bw * CTC_BEAM_WIDTH_RATIO)) if use_ctc else bw
    assert bw <= 32 and cw <= 32, "device beam bookkeeping handles up to 32 beams x 32 candidates"
    max_steps = dec.max_decode_ylen
    Lmax = max_steps + 1
    A = eng.arena
    timing = os.environ.get("EMOASR_BEAM_TIMING") == "1"
    if timing:
        torch.cuda.synchronize()
        t_start = time.perf_counter()
    # the search runs on its own stream: the legacy default stream cannot be captured into a graph
    bstream = getattr(eng, "_beam_stream", None)
    if bstream is None:
        bstream = eng._beam_stream = torch.cuda.Stream(device=dev)
    caller = torch.cuda.current_stream()
    bstream.wait_stream(caller)
    with torch.no_grad(), torch.cuda.stream(bstream), ops.stream_scope():
        rt = getattr(eng, "_dec_rt", None)
        if rt is None:
            rt = eng._dec_rt = DecoderStepRuntime(eng)
        dec_layers = rt._params()
        rt.begin(eouts, bw)                     # cross-attention K / V of the memory, once per utterance
        dtype = A.shadow.dtype
        dd, dh = eng.dd, eng.dh
        lnl = ld = lH = lF = 0
        if use_lm:
            lmrt = getattr(lm, "_step_rt", None)
            if lmrt is None:
                lmrt = lm._step_rt = LMStepRuntime(lm)
            LA, lm_layers = lmrt._params()
            P = lm.params
            lnl, ld, lH, lF = P.num_layers, P.hidden_size, P.num_attention_heads, P.intermediate_size
            assert P.vocab_size == V and LA.shadow.dtype == dtype
            assert lm._pe.shape[0] >= Lmax, "LM position table shorter than max_decode_ylen + 1"
        key = (str(dev), dtype, bw, cw, Lmax, V, eng.dnl, dd, lnl, ld)
        cache = getattr(eng, "_beam_bufs", None)
        if cache is None or cache[0] != key:
            cache = eng._beam_bufs = (key, _Buffers(dev, dtype, bw, cw, Lmax, V, eng.dnl, dd, lnl, ld))
        Bf = cache[1]
        if use_ctc:
            ctc_logits = eng.head_logits(eouts, "decoder.ctc.output")
            x = ops.log_softmax(ctc_logits.view(T, V))
            init_state = ops.ctc_prefix_init(x, blank)
            states = torch.empty(2, bw, cw, T, 2, device=dev, dtype=torch.float32)
            states[1, 0, 0].copy_(init_state)    # step 0 reads "previous" = index 1 at (parent 0, candidate 0)
        # ---- initial beams: one hypothesis [<sos> = eos] ----
        Bf.state.copy_(torch.tensor([0, 1, 0, 0], dtype=torch.int32), non_blocking=True)
        Bf.ids.fill_(eos); Bf.last.fill_(eos)
        Bf.parent.zero_(); Bf.pcand.zero_(); Bf.outlen.zero_(); Bf.klens.fill_(1)
        Bf.score.zero_(); Bf.score_ctc.zero_()
        esz = A.shadow.element_size()
        F = rt._F
        ws_dec = torch.empty(lib.size_query("emoasr_decode_step_ws_bytes", ops.dt(Bf.logits), bw, dd, dh, F, V), device=dev,
                             dtype=torch.uint8)
        ws_lm = torch.empty(lib.size_query("emoasr_decode_step_ws_bytes", ops.dt(Bf.logits), bw, max(ld, 8), max(lH, 1),
                                           max(lF, 8), V), device=dev, dtype=torch.uint8) if use_lm else None
        pe_dec = eng._abs_table(Lmax, dev, dd)
        steps = []
        for cur in (0, 1):
            prev = cur ^ 1
            js = lib.JointStep()
            js.dec_nl, js.dec_layers = eng.dnl, dec_layers
            d = js.dec
            d.nb, d.Lmax, d.T, d.dd, d.H, d.F, d.V = bw, Lmax, T, dd, dh, F, V
            d.ids, d.pos, d.klens = Bf.ids.data_ptr(), Bf.state.data_ptr(), Bf.klens.data_ptr()
            d.embed, d.pe, d.emb_scale = A.w("decoder.embed.weight").data_ptr(), pe_dec.data_ptr(), math.sqrt(dd)
            d.kmem, d.kv = rt.kmem.data_ptr(), ctypes.cast(rt.kv_ptrs, ctypes.POINTER(ctypes.c_void_p))
            d.kcache, d.vcache = Bf.dec_k[cur].data_ptr(), Bf.dec_v[cur].data_ptr()
            _ln(d.ln_out, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"))
            _lin(d.out, A.w("decoder.output.weight"), A.p("decoder.output.bias"))
            d.logits_last, d.ws, d.ws_bytes = Bf.logits.data_ptr(), ws_dec.data_ptr(), ws_dec.numel()
            js.dec_k_prev, js.dec_v_prev = Bf.dec_k[prev].data_ptr(), Bf.dec_v[prev].data_ptr()
            js.lm_nl = lnl if use_lm else 0
            if use_lm:
                js.lm_layers = lm_layers
                l = js.lm
                pre, cp = "lm.transformer.bert.", "lm.transformer.cls.predictions."
                l.nb, l.Lmax, l.d, l.H, l.F, l.V = bw, Lmax, ld, lH, lF, V
                l.ids, l.pos, l.klens = Bf.ids.data_ptr(), Bf.state.data_ptr(), Bf.klens.data_ptr()
                l.word_emb, l.pe = LA.w(pre + "embeddings.word_embeddings.weight").data_ptr(), lm._pe.data_ptr()
                _ln(l.ln_emb, LA.p(pre + "embeddings.LayerNorm.weight"), LA.p(pre + "embeddings.LayerNorm.bias"))
                l.kcache, l.vcache = Bf.lm_k[cur].data_ptr(), Bf.lm_v[cur].data_ptr()
                _lin(l.transform, LA.w(cp + "transform.dense.weight"), LA.p(cp + "transform.dense.bias"))
                _ln(l.ln_transform, LA.p(cp + "transform.LayerNorm.weight"), LA.p(cp + "transform.LayerNorm.bias"))
                l.out_bias, l.logp = LA.p(cp + "bias").data_ptr(), Bf.lm_logp.data_ptr()
                l.raw_logits = 1   # the scoring kernel does both log-softmaxes (emoasr_beam_scores_topk)
                l.ws, l.ws_bytes = ws_lm.data_ptr(), ws_lm.numel()
                js.lm_k_prev, js.lm_v_prev = Bf.lm_k[prev].data_ptr(), Bf.lm_v[prev].data_ptr()
            js.parent, js.scores_pre = Bf.parent.data_ptr(), Bf.scores_pre.data_ptr()
            js.T, js.blank = T, blank
            if use_ctc:
                js.ctc_x = x.data_ptr()
                js.states_prev, js.states_cur = states[prev].data_ptr(), states[cur].data_ptr()
            u = js.upd
            u.bw, u.cw, u.eos = bw, cw, eos
            lam, mu = float(decode_ctc_weight), float(lm_weight)
            u.one_minus_lam, u.lam, u.mu = float(np.float32(1 - lam)), float(np.float32(lam)), float(np.float32(mu)) if use_lm else 0.0
            u.len_weight = float(len_weight)
            u.vals, u.cands = Bf.vals.data_ptr(), Bf.cands.data_ptr()
            u.lm_at = Bf.lm_at.data_ptr() if (use_lm and use_ctc) else None
            u.psi = Bf.psi.data_ptr() if use_ctc else None
            u.score, u.score_ctc = Bf.score.data_ptr(), Bf.score_ctc.data_ptr()
            u.n_ids, u.n_parent, u.n_pcand = Bf.ids.data_ptr(), Bf.parent.data_ptr(), Bf.pcand.data_ptr()
            u.n_last, u.n_outlen, u.n_klens = Bf.last.data_ptr(), Bf.outlen.data_ptr(), Bf.klens.data_ptr()
            u.hist_parent, u.hist_token = Bf.hist_parent.data_ptr(), Bf.hist_token.data_ptr()
            u.res_score, u.res_step, u.res_parent = Bf.res_score.data_ptr(), Bf.res_step.data_ptr(), Bf.res_parent.data_ptr()
            u.state = Bf.state.data_ptr()
            u.host_mirror = Bf.state_host.data_ptr()   # pinned: the kernel writes it, the host polls it (no copy engine)
            steps.append(js)
        side = None
        if use_lm:
            side = getattr(eng, "_lm_stream", None)
            if side is None:
                side = eng._lm_stream = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream()
        dt_code = ops.dt(Bf.logits)
        if timing:
            torch.cuda.synchronize()
            t_loop = time.perf_counter()
        main_p, side_p = main.cuda_stream, (side.cuda_stream if side is not None else None)
        t_loop0 = time.perf_counter()
        # HIP graphs pay off for the launch chains (~185 kernels per step); with the cooperative step kernels a step is ~25 launches
        # and plain launches are ~3 % faster (no graph boundaries: 0.476-0.607 against 0.494-0.625 ms per step over T' 190-600)
        g_env = os.environ.get("EMOASR_BEAM_GRAPH", "auto")
        use_graph = (lib.get_option("decode_coop") == 0) if g_env == "auto" else g_env != "0"
        if use_graph:
            if not getattr(eng, "_beam_graph_warm", False):
                # first use in this process: one eager pass with the search marked finished, so that every kernel's lazy
                # one-time setup (function attributes, device queries) happens outside stream capture
                Bf.state.copy_(torch.tensor([0, 1, 0, 1], dtype=torch.int32))
                lib.call("emoasr_joint_beam_step", dt_code, ctypes.byref(steps[0]), main_p, side_p)
                main.synchronize()
                Bf.state.copy_(torch.tensor([0, 1, 0, 0], dtype=torch.int32))
                eng._beam_graph_warm = True
            for k in (0, 1):
                for part in ((0, 1, 2) if use_lm else (0, 2)):
                    lib.call("emoasr_joint_beam_graph_build", dt_code, ctypes.byref(steps[k]), k, part, main_p)
            if timing:
                print(f"[beam timing] graph build / update {1e3 * (time.perf_counter() - t_loop0):.2f} ms", flush=True)
        # Steps are issued one ahead of the flag they depend on: a step launched after the search has finished changes
        # nothing (emoasr_beam_update returns at once), and the GPU never waits for the host's round trip.
        ev_tail, ev_lm = torch.cuda.Event(), torch.cuda.Event()
        # device time of the search loop for the running totals (bench.py: search_loop_ms_per_step): events on the search stream, so
        # that the encoder pass / cross-attention K, V / CTC prefix setup still queued AHEAD of the first step are not charged to
        # the loop (host wall time from here charged ~4 ms of them per utterance: 0.94 ms per step on ten-step searches, 0.53 on
        # forced 36-step ones, for the same 0.55 ms steps)
        ev_loop0, ev_loop1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev_loop0.record(main)
        two_streams = os.environ.get("EMOASR_BEAM_TWO_STREAMS", "1") != "0"
        mirror = Bf.state_host.numpy()               # [pos, n_alive, n_results, done], written by emoasr_beam_update
        mirror[:] = (0, 1, 0, 0)
        # a generation-2 garbage collection in the middle of the loop stalls a 0.65 ms step for 10-15 ms; the loop allocates
        # next to nothing, so collection simply waits until it is over
        gc_was_on = gc.isenabled()
        gc.disable()
        dbg = os.environ.get("EMOASR_BEAM_STEP_TIMING") == "1"
        t_l = t_s = 0.0
        worst = (0.0, -1, "")
        try:
            for i in range(max_steps):
                if dbg:
                    _t0 = time.perf_counter()
                if use_graph:
                    k = i & 1
                    if use_lm and two_streams:   # the LM chain on the side stream, concurrent with the decoder chain
                        ev_tail.record(main)             # the previous step's tail (ids / parent / pos) is complete
                        side.wait_event(ev_tail)
                        lib.call("emoasr_joint_beam_graph_launch", k, 1, side_p)
                        ev_lm.record(side)
                    elif use_lm:
                        lib.call("emoasr_joint_beam_graph_launch", k, 1, main_p)
                    lib.call("emoasr_joint_beam_graph_launch", k, 0, main_p)
                    if use_lm and two_streams:
                        main.wait_event(ev_lm)
                    lib.call("emoasr_joint_beam_graph_launch", k, 2, main_p)
                else:
                    lib.call("emoasr_joint_beam_step", dt_code, ctypes.byref(steps[i & 1]), main_p, side_p)
                if dbg:
                    _t1 = time.perf_counter()
                # Steps are issued one ahead of the flag they depend on (a step launched after the search has finished changes
                # nothing: emoasr_beam_update returns at once), so the GPU never waits for the host.  The state of step i - 1
                # arrives in pinned memory by the kernel's own store; polling it involves no copy engine and no event.
                if i >= 1:
                    spins, t_wait = 0, None
                    while mirror[0] < i and not mirror[3]:
                        _yield()   # the runtime's own threads (signal handling, graph bookkeeping) may share this core
                        spins += 1
                        if spins & 0xFFF == 0:   # a lost launch / a faulted device must surface, not spin forever
                            now = time.perf_counter()
                            t_wait = now if t_wait is None else t_wait
                            if now - t_wait > _STEP_DEADLINE_S:
                                raise RuntimeError(f"beam search: step {i - 1} did not report within {_STEP_DEADLINE_S:.0f} s "
                                                   f"(stream idle: {main.query()}; last library error: {lib.load().emoasr_last_error().decode()!r})")
                    if mirror[3]:
                        break
                if dbg:
                    _t2 = time.perf_counter()
                    t_l += _t1 - _t0; t_s += _t2 - _t1
                    if _t1 - _t0 > worst[0]:
                        worst = (_t1 - _t0, i, "launch")
                    if _t2 - _t1 > worst[0]:
                        worst = (_t2 - _t1, i, "sync")
            ev_loop1.record(main)
            main.synchronize()
            if lib.size_query("emoasr_decode_coop_status") > 0:
                raise RuntimeError("decode_coop: a grid barrier gave up waiting (csrc/decode_coop.hip); emoasr_set_option('decode_coop', 0) "
                                   "selects the launch chain")
        finally:
            if gc_was_on:   # (also on an exception: the collector must not stay off for the rest of the process)
                gc.enable()
        if dbg:
            print(f"   host: launches {1e3 * t_l:.2f} ms, waits {1e3 * t_s:.2f} ms, worst {1e3 * worst[0]:.2f} ms at step {worst[1]} ({worst[2]})", flush=True)
        n_done = int(mirror[0])                      # effective steps (pos advances only while the search is live)
        stats = getattr(eng, "_beam_stats", None)    # running totals for bench.py: steps and wall time of the search loops
        if stats is None:
            stats = eng._beam_stats = {"steps": 0, "loop_s": 0.0, "utts": 0}
        # (the loop issues one step beyond the last effective one: its device time is part of the figure)
        stats["steps"] += n_done; stats["loop_s"] += 1e-3 * ev_loop0.elapsed_time(ev_loop1); stats["utts"] += 1
        if side is not None:
            main.wait_stream(side)
        if timing:
            torch.cuda.synchronize()
            t_end = time.perf_counter()
            print(f"[beam timing] T' {T}: setup {1e3 * (t_loop - t_start):.2f} ms, {n_done} steps {1e3 * (t_end - t_loop):.2f} ms "
                  f"({1e3 * (t_end - t_loop) / max(n_done, 1):.3f} ms/step)", flush=True)
        # ---- results: token sequences from the (parent, token) history ----
        n_res = int(mirror[2])
        hp, ht = Bf.hist_parent[:n_done].cpu().numpy(), Bf.hist_token[:n_done].cpu().numpy()
        rs, rstep, rpar = Bf.res_score[:n_res].cpu().numpy(), Bf.res_step[:n_res].cpu().numpy(), Bf.res_parent[:n_res].cpu().numpy()
    caller.wait_stream(bstream)
    results = []
    for k in range(n_res):
        toks, slot = [], int(rpar[k])
        for p in range(int(rstep[k]) - 1, -1, -1):
            toks.append(int(ht[p, slot]))
            slot = int(hp[p, slot])
        results.append(dict(hyp=toks[::-1], score=float(rs[k])))
    results = sorted(results, key=lambda r: r["score"], reverse=True)
    return [r["hyp"] for r in results], [r["score"] for r in results], None, None


# ---------------------------------------------------------------------------------------------------------------------------
# The same search for S utterances at once.  A search is one utterance; S searches of width W occupy
# rows s * W .. s * W + W - 1 of every per-hypothesis array and step in lockstep: one captured step serves all of them, a
# finished search keeps its rows (computed and ignored).  Kernels: csrc/decode_batch.hip (grouped cross-attention over the
# unreplicated memories, one bookkeeping workgroup per search), the ragged CTC prefix scorer (csrc/decoder.hip) and the
# chain emoasr_joint_beam_batch_step (csrc/decode_rt.hip).  A stateful LM (the RNN LM) under decoder.joint_rnnlm_impl = "device" is
# stepped inside the same chain: emoasr_rnnlm_step_rows over all S * W rows, its state in a double-buffered
# slot pool addressed by the chain's own parent array, through emoasr_joint_beam_batch_step_rnnlm / _grid_step_rnnlm.
# ---------------------------------------------------------------------------------------------------------------------------
MAX_ROWS = 1024                     # S * W rows of one chunk
GRID_BUFFER_SETS = 3                # buffer sets the fusion grid keeps (one per chunk shape)
CACHE_BUDGET_BYTES = 8 << 30        # the self-attention cache pools of one chunk (decoder + LM, both halves of the ping-pong)


def batch_cache_bytes(nb, Lmax, dnl, dd, lnl, ld, esz):
    """bytes of the cache pools of nb rows: K and V, two halves (previous / current step), every layer, Lmax positions"""
    return 2 * 2 * nb * Lmax * (dnl * dd + lnl * ld) * esz


def batch_chunk_capacity(W, Lmax, dnl, dd, lnl, ld, esz, budget=None, max_rows=None):
    """S_max: the most searches of width W one chunk holds -- S_max * W <= MAX_ROWS rows and batch_cache_bytes(S_max * W, ...)
    <= CACHE_BUDGET_BYTES; never below one search"""
    budget = CACHE_BUDGET_BYTES if budget is None else budget
    max_rows = MAX_ROWS if max_rows is None else max_rows
    per_search = batch_cache_bytes(W, Lmax, dnl, dd, lnl, ld, esz)
    return max(1, min(max_rows // W, budget // per_search))


def joint_rnnlm_impl(dec):
    """the decoder's switch for a stateful LM in the batched searches: "host" (default) or "device"; anything else is refused"""
    impl = getattr(dec, "joint_rnnlm_impl", "host")
    if impl not in ("host", "device"):
        raise ValueError(f"emoasr_amd: joint_rnnlm_impl is 'host' or 'device', not {impl!r}")
    return impl


def batch_rnnlm_why_not(dec, beam_width, lm, decode_ctc_weight):
    """why the batched device search cannot fuse this LM through emoasr_rnnlm_step_rows (None: it can)"""
    V = dec.vocab_size
    why = lockstep.rnnlm_rows_why_not(_engine_of(dec), V, lm)
    if why is not None:
        return why
    cw = min(V, int(beam_width * CTC_BEAM_WIDTH_RATIO)) if decode_ctc_weight > 0 else beam_width
    if not (1 <= beam_width <= 32 and 1 <= cw <= 32 and beam_width <= V):
        return f"beam_width {beam_width} (candidate width {cw}, vocabulary {V}) is outside the device bookkeeping's 32 beams x 32 candidates"
    for env in ("EMOASR_DEVICE_BEAM", "EMOASR_CPP_DECODE"):
        if os.environ.get(env, "1") == "0":
            return f"{env}=0 forces the host bookkeeping"
    return None


def rnnlm_on_device(dec, beam_width, lm, lm_weight, decode_ctc_weight):
    """does a stateful LM go through the batched device search?  Exactly when the decoder's joint_rnnlm_impl says "device" -- then a
    configuration the device form cannot take is a ValueError naming the reason, never a quiet detour through the host form.  False
    without an LM to fuse and for an LM without state (the Transformer LM: the switch does not touch it)."""
    impl = joint_rnnlm_impl(dec)
    if lm is None or lm_weight <= 0 or not getattr(lm, "stateful", False) or impl != "device":
        return False
    why = batch_rnnlm_why_not(dec, beam_width, lm, decode_ctc_weight)
    if why is not None:
        raise ValueError(f"emoasr_amd: joint_rnnlm_impl = 'device' cannot fuse this LM: {why}")
    return True


def batch_device_ok(dec, beam_width, lm, lm_weight, decode_ctc_weight):
    """whether the batched device search takes this configuration (else: utterance by utterance through joint_beam_search)"""
    if rnnlm_on_device(dec, beam_width, lm, lm_weight, decode_ctc_weight):
        return True
    use_ctc = decode_ctc_weight > 0
    cw = min(dec.vocab_size, int(beam_width * CTC_BEAM_WIDTH_RATIO)) if use_ctc else beam_width
    if os.environ.get("EMOASR_DEVICE_BEAM", "1") == "0" or os.environ.get("EMOASR_CPP_DECODE", "1") == "0":
        return False   # the switches that force the host bookkeeping
    if not (1 <= beam_width <= 32 and 1 <= cw <= 32 and beam_width <= dec.vocab_size):
        return False
    return lm is None or lm_weight <= 0 or hasattr(lm, "predict_device")


class _BatchBuffers(lockstep.BookBuffers):
    """lockstep.BookBuffers of one (S, W, cw, Lmax, model sizes, frame capacities) configuration, with the joint search's own pools:
    the decoder's (and a Transformer LM's) self-attention caches of two halves, the CTC scorer's frames and states"""

    def __init__(self, dev, dtype, S, W, cw, Lmax, V, dnl, dd, lnl, ld, rows_cap, Tcap, use_ctc, grid=False, rnn=None):
        super().__init__(dev, dtype, S, W, cw, Lmax, V, rnn, grid)     # (rnn = (L, H): a stateful LM has slot pools, no K / V pools)
        nb = S * W
        self.rows_cap, self.Tcap = rows_cap, Tcap
        i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.lm_at, self.psi = f32(nb, cw), f32(nb, cw)
        self.logits = torch.zeros(nb, V, device=dev, dtype=dtype)
        self.lm_logp = self.lm_logits if rnn else (f32(nb, V) if lnl else None)    # (what either LM's step writes)
        self.dec_k = torch.zeros(2, dnl, nb, Lmax, dd, device=dev, dtype=dtype)
        self.dec_v = torch.zeros_like(self.dec_k)
        self.lm_k = torch.zeros(2, max(lnl, 1), nb, Lmax, max(ld, 1), device=dev, dtype=dtype) if lnl else None
        self.lm_v = torch.zeros_like(self.lm_k) if lnl else None
        self.ctc_x = f32(rows_cap, V) if use_ctc else None
        self.states = f32(2, nb, cw, Tcap, 2) if use_ctc else None
        if grid:   # the LM weight of every search, the attention's row groups [<= S, 3]
            self.groups, self.mu = i32(3 * S), f32(S)


def _batch_search_chunk(dec, eng, eouts, elens, bw, len_weight, lm, lm_weight, decode_ctc_weight, grid=None, sort=True):
    """S = len(elens) searches in lockstep -> (hyps[s], scores[s]): each search's results sorted by score (stable; sort=False: in
    the order the search found them).
    grid = (sutt, mus, cells_per_group): the fusion grid's chunk (section 24) -- the U = len(elens) utterances are encoded,
    projected and soft-maxed once, search s runs over utterance sutt[s] (consecutive per utterance) with the LM weight mus[s] > 0
    through emoasr_joint_beam_grid_step; lm_weight is not read and len_weight must be 0."""
    V, eos, blank = dec.vocab_size, dec.eos_id, dec.blank_id
    dev = eouts.device
    U, W = len(elens), bw
    S = len(grid[0]) if grid else U
    nb = S * W
    use_ctc = decode_ctc_weight > 0
    use_lm = lm is not None and (lm_weight > 0 or grid is not None)
    if grid:
        sutt, mus, cells_per_group = grid
        assert lm is not None and len(mus) == S and all(m > 0 for m in mus) and len_weight == 0
        assert all(0 <= u < U for u in sutt) and all(a <= b for a, b in zip(sutt, sutt[1:])), sutt
        groups, group_rows = ops.cell_groups(sutt, W, cells_per_group)
        flat_groups = [v for g in groups for v in g]
        lib.call("emoasr_cell_groups_check", len(groups), (ctypes.c_int * len(flat_groups))(*flat_groups), group_rows, nb, U)
    cw = min(V, int(bw * CTC_BEAM_WIDTH_RATIO)) if use_ctc else bw
    max_steps = dec.max_decode_ylen
    Lmax = max_steps + 1
    A = eng.arena
    bstream = getattr(eng, "_beam_stream", None)
    if bstream is None:
        bstream = eng._beam_stream = torch.cuda.Stream(device=dev)
    caller = torch.cuda.current_stream()
    bstream.wait_stream(caller)
    # the launch chains only: the cooperative step kernels (csrc/decode_coop.hip, <= 16 rows) are not part of the batched step
    with torch.no_grad(), torch.cuda.stream(bstream), ops.stream_scope(), lib.options(decode_coop=0):
        rt = getattr(eng, "_dec_rt", None)
        if rt is None:
            rt = eng._dec_rt = DecoderStepRuntime(eng)
        dec_layers = rt._params()
        total, longest = sum(elens), max(elens)
        rows_cap = (total + 1023) // 1024 * 1024
        Tcap = (longest + 63) // 64 * 64
        mem = rt.begin_batch(eouts, elens, rows_cap)   # (raises ValueError for an utterance without frames)
        dtype = A.shadow.dtype
        dd, dh, F = eng.dd, eng.dh, rt._F
        lnl = ld = lH = lF = 0
        lm_guard = None
        rnn = None      # a stateful LM: (L, H) of its slot pools
        if use_lm and getattr(lm, "stateful", False):
            LA = lm._prepare()       # (arena bound, compute-dtype weights and the summed biases current: before the capture)
            assert lm.V == V and LA.shadow.dtype == dtype
            rnn = (lm.L, lm.H)
            lm_guard = (LA.flat.data_ptr(), LA.shadow.data_ptr()) + tuple(b.data_ptr() for b in lm._bias)
        elif use_lm:
            lmrt = getattr(lm, "_step_rt", None)
            if lmrt is None:
                lmrt = lm._step_rt = LMStepRuntime(lm)
            LA, lm_layers = lmrt._params()
            P = lm.params
            lnl, ld, lH, lF = P.num_layers, P.hidden_size, P.num_attention_heads, P.intermediate_size
            assert P.vocab_size == V and LA.shadow.dtype == dtype
            assert lm._pe.shape[0] >= Lmax, "LM position table shorter than max_decode_ylen + 1"
            lm_guard = (LA.flat.data_ptr(), LA.shadow.data_ptr(), lm._pe.data_ptr())
        # one set of buffers is kept: reused while the sizes match and the frame capacities suffice
        key = (str(dev), dtype, S, W, cw, Lmax, V, eng.dnl, dd, lnl, ld, use_ctc, grid is not None, rnn)
        cache = getattr(eng, "_beam_batch_bufs", None)
        if grid:      # the grid alternates between a few chunk shapes (and the search without the LM): one set of buffers each
            sets = getattr(eng, "_beam_grid_bufs", None)
            if sets is None:
                sets = eng._beam_grid_bufs = {}
            cache = (key, sets[key]) if key in sets else None
        if cache is not None and cache[0] == key and cache[1].rows_cap >= rows_cap and cache[1].Tcap >= Tcap:
            Bf = cache[1]
            rows_cap, Tcap = Bf.rows_cap, Bf.Tcap
        elif grid:
            Bf = _BatchBuffers(dev, dtype, S, W, cw, Lmax, V, eng.dnl, dd, lnl, ld, rows_cap, Tcap, use_ctc, True, rnn)
            sets.pop(key, None)
            while len(sets) >= GRID_BUFFER_SETS:
                sets.pop(next(iter(sets)))
            sets[key] = Bf
        else:
            Bf = _BatchBuffers(dev, dtype, S, W, cw, Lmax, V, eng.dnl, dd, lnl, ld, rows_cap, Tcap, use_ctc, grid is not None, rnn)
            eng._beam_batch_bufs = (key, Bf)
        # ---- this call's inputs, into the buffers the captured steps read ----
        Bf.moff[:U + 1].copy_(h2d_i32(rt.moff_host, dev))
        if grid:
            Bf.sutt.copy_(h2d_i32(list(sutt), dev))
            Bf.groups[:len(flat_groups)].copy_(h2d_i32(flat_groups, dev))
            mu32 = np.asarray(mus, dtype=np.float32)        # rounded as emoasr_beam_update_t.mu is
            Bf.mu.copy_(torch.from_numpy(mu32).to(dev))
            Bf.mu_row.copy_(torch.from_numpy(np.repeat(mu32, W)).to(dev))
        if use_ctc:
            ctc_logits = eng.head_logits(mem.unsqueeze(0), "decoder.ctc.output")
            Bf.ctc_x[:total].copy_(ops.log_softmax(ctc_logits.view(total, V)))

        reset = lambda done: lockstep.reset_book(Bf, S, W, eos, done)
        lam, mu = float(decode_ctc_weight), float(lm_weight)
        if grid:    # the weights are device data; the groups' count and width are part of the captured launches
            mu = 0.0
        gkey = (A.flat.data_ptr(), A.shadow.data_ptr(), lm_guard, tuple(k.data_ptr() for k in rt.kv_group), lam, mu if use_lm else 0.0,
                float(len_weight), eos, blank, id(Bf), (U, len(groups), group_rows) if grid else None)
        step_fn = ("emoasr_joint_beam_grid_step" if grid else "emoasr_joint_beam_batch_step") + ("_rnnlm" if rnn else "")
        if Bf.graphs is None or Bf.graphs[0] != gkey:
            dt_code = ops.dt(Bf.logits)
            ws_dec = torch.empty(lib.size_query("emoasr_decode_step_group_ws_bytes", dt_code, nb, dd, dh, F, V), device=dev, dtype=torch.uint8)
            ws_lm = torch.empty(lib.size_query("emoasr_decode_step_ws_bytes", dt_code, nb, max(ld, 8), max(lH, 1), max(lF, 8), V),
                                device=dev, dtype=torch.uint8) if (use_lm and not rnn) else None
            rows, lm_tabs = [], None
            if rnn:      # the stateful LM's step over the chain's rows: the even step reads half 1 of the pools and writes half 0
                rows, lm_tabs, ws_lm = lockstep.rnnlm_rows_pair(lm, LA, Bf, nb, V, dt_code, even_src=1)
            pe_dec = eng._abs_table(Lmax, dev, dd)
            steps = []
            for cur in (0, 1):
                prev = cur ^ 1
                if grid:
                    gs = lib.JointGridStep()
                    js = gs.js
                    gs.U, gs.n_groups, gs.group_rows = U, len(groups), group_rows
                    gs.sutt, gs.groups = Bf.sutt.data_ptr(), Bf.groups.data_ptr()
                    gs.mu, gs.mu_row = Bf.mu.data_ptr(), Bf.mu_row.data_ptr()
                else:
                    js = lib.JointBatchStep()
                js.dec_nl, js.dec_layers = eng.dnl, dec_layers
                js.dec.S, js.dec.W, js.dec.moff = S, W, Bf.moff.data_ptr()
                d = js.dec.d
                d.nb, d.Lmax, d.T, d.dd, d.H, d.F, d.V = nb, Lmax, Tcap, dd, dh, F, V
                d.ids, d.pos, d.klens = Bf.ids.data_ptr(), Bf.pos.data_ptr(), Bf.klens.data_ptr()
                d.embed, d.pe, d.emb_scale = A.w("decoder.embed.weight").data_ptr(), pe_dec.data_ptr(), math.sqrt(dd)
                d.kmem, d.kv = None, ctypes.cast(rt.kv_group_ptrs, ctypes.POINTER(ctypes.c_void_p))
                d.kcache, d.vcache = Bf.dec_k[cur].data_ptr(), Bf.dec_v[cur].data_ptr()
                _ln(d.ln_out, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"))
                _lin(d.out, A.w("decoder.output.weight"), A.p("decoder.output.bias"))
                d.logits_last, d.ws, d.ws_bytes = Bf.logits.data_ptr(), ws_dec.data_ptr(), ws_dec.numel()
                js.dec_k_prev, js.dec_v_prev = Bf.dec_k[prev].data_ptr(), Bf.dec_v[prev].data_ptr()
                js.lm_nl = lnl if use_lm else 0
                if use_lm and not rnn:
                    js.lm_layers = lm_layers
                    l = js.lm
                    pre, cp = "lm.transformer.bert.", "lm.transformer.cls.predictions."
                    l.nb, l.Lmax, l.d, l.H, l.F, l.V = nb, Lmax, ld, lH, lF, V
                    l.ids, l.pos, l.klens = Bf.ids.data_ptr(), Bf.pos.data_ptr(), Bf.klens.data_ptr()
                    l.word_emb, l.pe = LA.w(pre + "embeddings.word_embeddings.weight").data_ptr(), lm._pe.data_ptr()
                    _ln(l.ln_emb, LA.p(pre + "embeddings.LayerNorm.weight"), LA.p(pre + "embeddings.LayerNorm.bias"))
                    l.kcache, l.vcache = Bf.lm_k[cur].data_ptr(), Bf.lm_v[cur].data_ptr()
                    _lin(l.transform, LA.w(cp + "transform.dense.weight"), LA.p(cp + "transform.dense.bias"))
                    _ln(l.ln_transform, LA.p(cp + "transform.LayerNorm.weight"), LA.p(cp + "transform.LayerNorm.bias"))
                    l.out_bias, l.logp = LA.p(cp + "bias").data_ptr(), Bf.lm_logp.data_ptr()
                    l.raw_logits = 1   # emoasr_beam_scores_topk does both log-softmaxes
                    l.ws, l.ws_bytes = ws_lm.data_ptr(), ws_lm.numel()
                    js.lm_k_prev, js.lm_v_prev = Bf.lm_k[prev].data_ptr(), Bf.lm_v[prev].data_ptr()
                js.parent = Bf.parent.data_ptr()
                js.Tmax, js.blank = Tcap, blank
                if use_ctc:
                    js.ctc_x = Bf.ctc_x.data_ptr()
                    js.states_prev, js.states_cur = Bf.states[prev].data_ptr(), Bf.states[cur].data_ptr()
                lockstep.fill_beam_update(js.upd, Bf, S, W, cw, eos, max_steps, len_weight)
                u = js.upd.u
                u.one_minus_lam, u.lam = float(np.float32(1 - lam)), float(np.float32(lam))
                u.mu = float(np.float32(mu)) if use_lm else 0.0      # (the grid: mu[s] on the device)
                u.lm_at = Bf.lm_at.data_ptr() if (use_lm and use_ctc) else None
                u.psi = Bf.psi.data_ptr() if use_ctc else None
                steps.append(gs if grid else js)
            step_args = lambda k: (dt_code, ctypes.byref(steps[k])) + ((ctypes.byref(rows[k]),) if rnn else ()) + (ops._stream(),)
            graphs = lockstep.capture_two_steps(lambda k: lib.call(step_fn, *step_args(k)), reset)
            Bf.graphs = (gkey, graphs, (steps, ws_dec, ws_lm, pe_dec, dec_layers, rt.kv_group, rows, lm_tabs))
        reset(0)
        if rnn:       # (after the warm-up, whose steps write both halves) step 0 reads "previous" = half 1 at the search's row 0: zeros
            Bf.lm_h[:, nb:].zero_()
            Bf.lm_c[:, nb:].zero_()
        if use_ctc:   # (after the warm-up, whose steps write both halves of the scorer states)
            # step 0 reads "previous" = half 1 at (the search's row 0, candidate 0)
            if grid:
                ops.ctc_prefix_init_cells(Bf.ctc_x, Bf.moff[:U + 1], Bf.sutt, blank, Bf.states[1], W * cw * Tcap * 2)
            else:
                ops.ctc_prefix_init_ragged(Bf.ctc_x, Bf.moff, blank, Bf.states[1], W * cw * Tcap * 2)
        host = lockstep.replay_until_done(Bf.graphs[1], Bf, max_steps, S, eng, "_beam_batch_stats")   # (totals: tools/joint_beam_bench.py)
    caller.wait_stream(bstream)
    return batch_nbest_from_pack(host, Bf.pack_off, S, W, Lmax, sort)


def joint_beam_search_device_batch(dec, eouts, elens, beam_width, len_weight=0, lm=None, lm_weight=0, decode_ctc_weight=0):
    """joint_beam_search_device for every utterance of the batch: eouts [B, Tmax, d], utterance b over its own elens[b] >= 1
    frames -> (hyps, scores, None, None) with hyps[b] / scores[b] what the single search returns for eouts[b:b+1, :elens[b]]
    (hypotheses best first).  The batch is searched in chunks of at most batch_chunk_capacity searches."""
    require_next_token_lm(lm, lm_weight)
    eng = _engine_of(dec)
    elens = [int(n) for n in elens]
    B = eouts.shape[0]
    if len(elens) != B or any(n < 1 for n in elens):
        raise ValueError(f"joint_beam_search_device_batch: every utterance needs at least one frame, got elens {elens}")
    use_ctc = decode_ctc_weight > 0
    use_lm = lm is not None and lm_weight > 0
    cw = min(dec.vocab_size, int(beam_width * CTC_BEAM_WIDTH_RATIO)) if use_ctc else beam_width
    assert 1 <= beam_width <= 32 and 1 <= cw <= 32, "device beam bookkeeping handles up to 32 beams x 32 candidates"
    stateful = use_lm and rnnlm_on_device(dec, beam_width, lm, lm_weight, decode_ctc_weight)
    assert not use_lm or stateful or hasattr(lm, "predict_device"), "the batched search fuses the Transformer LM, or the RNN LM by its switch"
    esz = 2 if eouts.dtype == torch.bfloat16 else 4
    lnl, ld = (lm.params.num_layers, lm.params.hidden_size) if (use_lm and not stateful) else (0, 0)    # (a stateful LM: no K / V pools)
    cap = batch_chunk_capacity(beam_width, dec.max_decode_ylen + 1, eng.dnl, eng.dd, lnl, ld, esz)
    hyps, scores = [], []
    for b0 in range(0, B, cap):
        n = elens[b0:b0 + cap]
        h, s = _batch_search_chunk(dec, eng, eouts[b0:b0 + cap, :max(n)], n, beam_width, len_weight, lm, lm_weight, decode_ctc_weight)
        hyps += h
        scores += s
    return hyps, scores, None, None


# ---------------------------------------------------------------------------------------------------------------------------
# The shallow-fusion grid of the joint search: every (lm_weight, len_weight) cell of every utterance
# from ONE call.  len_weight never touches the search (it is added to a finished hypothesis' score only), so a cell's N-best
# list is the result set of its lm_weight's search, rescored and stably re-sorted on the host; the searches of the distinct
# positive lm_weights of an utterance share its frames (csrc/decode_grid.hip).
# ---------------------------------------------------------------------------------------------------------------------------
# searches of one utterance per cross-attention workgroup (None: ops.cell_groups' 32 // W).  Packing wins for the kernel alone only
# where it saves a round of workgroups, and does not beat 1 inside the grid call: the default is 1
GRID_CELLS_PER_GROUP = 1


def joint_beam_search_device_grid(dec, eouts, elens, beam_width, lm, lm_weights, len_weights, decode_ctc_weight=0):
    """the joint search of every utterance for every (lm_weight, len_weight) cell -> (hyps, scores): hyps[b][c] / scores[b][c] what
    joint_beam_search_device_batch returns for utterance b with cell c's weights (cells in lm_weight-outer, len_weight-inner
    order).  Distinct lm_weights are searched once, at len_weight 0; weights <= 0 are one search without the LM
    (lockstep.run_fusion_grid)."""
    lm_weights, len_weights = [float(a) for a in lm_weights], [float(b) for b in len_weights]
    top = max(grid_cell_plan(lm_weights, len_weights, lm is not None)[0])
    require_next_token_lm(lm, top)
    elens = [int(n) for n in elens]
    B = eouts.shape[0]
    if len(elens) != B or any(n < 1 for n in elens):
        raise ValueError(f"joint_beam_search_device_grid: every utterance needs at least one frame, got elens {elens}")
    expand = lambda f, a: expand_len_weights(*f, len_weights)
    if not batch_device_ok(dec, beam_width, lm, top, decode_ctc_weight):
        from .beam_search import joint_beam_search_batch
        host = lambda a: joint_beam_search_batch(dec, eouts, elens, beam_width, 0, lm, a, decode_ctc_weight)[:2]

        def host_fused(positive, weights, found):
            for k in positive:
                h, s = host(weights[k])
                for b in range(B):
                    found[b][k] = (h[b], s[b])

        return lockstep.run_fusion_grid(B, lm_weights, len_weights, lm is not None, lambda: host(0.0), host_fused, expand)
    eng = _engine_of(dec)
    esz = 2 if eouts.dtype == torch.bfloat16 else 4
    Lmax = dec.max_decode_ylen + 1

    def search_plain():      # the search without the LM: the batched search as it is, no LM launches
        cap = batch_chunk_capacity(beam_width, Lmax, eng.dnl, eng.dd, 0, 0, esz)
        hyps, scores = [], []
        for b0 in range(0, B, cap):
            n = elens[b0:b0 + cap]
            h, s = _batch_search_chunk(dec, eng, eouts[b0:b0 + cap, :max(n)], n, beam_width, 0, None, 0, decode_ctc_weight, sort=False)
            hyps += h
            scores += s
        return hyps, scores

    def search_fused(positive, weights, found):
        lnl, ld = (0, 0) if getattr(lm, "stateful", False) else (lm.params.num_layers, lm.params.hidden_size)
        cap = batch_chunk_capacity(beam_width, Lmax, eng.dnl, eng.dd, lnl, ld, esz)
        for utts, n, sutt, k_local in lockstep.grid_chunks(B, len(positive), cap, elens):
            ks = [positive[j] for j in k_local]
            sub = eouts[utts[0]:utts[-1] + 1, :max(n)]      # (a chunk's utterances are consecutive)
            h, s = _batch_search_chunk(dec, eng, sub, n, beam_width, 0, lm, 0, decode_ctc_weight,
                                       grid=(sutt, [weights[k] for k in ks], GRID_CELLS_PER_GROUP), sort=False)
            for i, (u, k) in enumerate(zip(sutt, ks)):
                found[utts[u]][k] = (h[i], s[i])

    return lockstep.run_fusion_grid(B, lm_weights, len_weights, lm is not None, search_plain, search_fused, expand)
