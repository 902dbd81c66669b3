"""The host scaffold the lockstep beam searches share: S searches of width W occupy rows s * W .. s * W + W - 1
of every per-hypothesis array and step together, one captured step serving them all (emoasr_beam_update_batch keeps their books).
Here: the bookkeeping buffers and their reset, the fillers of the update and RNN-LM structs, the capture of the two steps, the replay
loop with its one download, the admission checks of emoasr_rnnlm_step_rows, and the driver of the (lm_weight, len_weight) grids.
What belongs to one decoder -- the staging of its inputs, its step, its cache key and its buffer-cache policy -- stays with it:
modeling/beam_search_device.py (joint CTC / attention), engine/las.py (LAS), engine/rnnt_search.py (the transducer, whose books are
rnnt_beam_book / rnnt_greedy_batch_book: of this module it takes the grid driver, the capture after a warm-up, the LM admission checks
and the length expansion)."""
import ctypes
import gc
import os
import time

import numpy as np
import torch

from . import lib, ops

_STEP_DEADLINE_S = 30.0   # a search step takes ~0.5 ms; this only bounds the wait for a launch that will never report
_yield = os.sched_yield if os.environ.get("EMOASR_BEAM_YIELD", "1") != "0" else (lambda: None)
_LOGGED = set()           # messages log_once has emitted


def log_once(logger, message):
    """logger.info(message), the first time this message comes"""
    if message not in _LOGGED:
        _LOGGED.add(message)
        logger.info(message)


# ------------------------------------------------------------------------------------------------ the books of a chunk
def batch_pack_sizes(S, W, Lmax):
    """int32 words of the parts of the ONE allocation the host reads back after a batched search: res_score (double [nb]) |
    state [S, 4] | res_step [nb] | res_parent [nb] | hist_parent [Lmax, nb] | hist_token [Lmax, nb]"""
    nb = S * W
    return [2 * nb, 4 * S, nb, nb, Lmax * nb, Lmax * nb]


class BookBuffers:
    """the bookkeeping buffers of S searches of width W (cw candidates per row, Lmax positions), reused across calls: the captured
    steps point into them.  Everything the host reads back at the end lives in ONE int32 allocation (`pack`, batch_pack_sizes).
    rnn = (L, H, ...): a fused RNN LM's slot pools of two halves (source / destination of a step) and its raw f32 logits [nb, V];
    grid: the fusion grid's search -> utterance map and the LM weight of every row.  A decoder's class adds its own pools."""

    def __init__(self, dev, dtype, S, W, cw, Lmax, V=0, rnn=None, grid=False):
        nb = S * W
        i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        n = batch_pack_sizes(S, W, Lmax)
        self.pack = i32(sum(n))
        o = [0]
        for v in n:
            o.append(o[-1] + v)
        self.pack_off = o
        part = lambda k: self.pack[o[k]:o[k + 1]]
        self.res_score = part(0).view(torch.float64)
        self.state, self.res_step, self.res_parent = part(1).view(S, 4), part(2), part(3)
        self.hist_parent, self.hist_token = part(4).view(Lmax, nb), part(5).view(Lmax, nb)
        self.pos, self.ctl = i32(1), i32(1)
        self.ids, self.parent, self.pcand = i32(nb), i32(nb), i32(nb)
        self.last, self.outlen, self.klens = i32(nb), i32(nb), i32(nb)
        self.score = torch.zeros(nb, device=dev, dtype=torch.float64)
        self.score_ctc = f32(nb)
        self.vals, self.cands = f32(nb, cw), i32(nb, cw)
        self.moff = i32(S + 1)
        self.mirror_host = torch.zeros(2, dtype=torch.int32).pin_memory()   # {position, finished searches}
        self.lm_h = torch.zeros(rnn[0], 2 * nb, rnn[1], device=dev, dtype=dtype) if rnn else None
        self.lm_c = f32(rnn[0], 2 * nb, rnn[1]) if rnn else None
        self.lm_logits = f32(nb, V) if rnn else None
        if grid:
            self.sutt, self.mu_row = i32(S), f32(nb)
        self.graphs = None    # (key, [graph of the even steps, graph of the odd steps], what the captured launches point at)


def reset_book(Bf, S, W, eos, done):
    """every search back to one hypothesis [<sos> = eos] at position 0; done = 1: marked finished (the warm-up, whose bookkeeping
    then returns at once).  The caller zeroes its own pools after this."""
    from .engine.arena import h2d_i32      # (the engine imports this module: resolved at call time)
    dev = Bf.state.device
    Bf.state.copy_(h2d_i32([[0, 1, 0, done]] * S, dev))
    Bf.pos.zero_(); Bf.ctl.fill_(done)
    Bf.ids.fill_(eos); Bf.last.fill_(eos)
    Bf.parent.copy_(torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(W) * W)
    Bf.pcand.zero_(); Bf.outlen.zero_(); Bf.klens.fill_(1)
    Bf.score.zero_(); Bf.score_ctc.zero_()


def fill_beam_update(ub, Bf, S, W, cw, eos, max_pos, len_weight):
    """lib.BeamUpdateBatch over Bf's books, as an attention-only search needs it: one_minus_lam 1, lam and mu 0, psi and lm_at NULL
    (the joint search sets its weights and those two on top)"""
    ub.S, ub.max_pos, ub.pos, ub.ctl = S, max_pos, Bf.pos.data_ptr(), Bf.ctl.data_ptr()
    u = ub.u
    u.bw, u.cw, u.eos = W, cw, eos
    u.one_minus_lam, u.lam, u.mu, u.len_weight = 1.0, 0.0, 0.0, float(len_weight)
    u.vals, u.cands = Bf.vals.data_ptr(), Bf.cands.data_ptr()
    u.score, u.score_ctc = Bf.score.data_ptr(), Bf.score_ctc.data_ptr()
    u.n_ids, u.n_parent, u.n_pcand = Bf.ids.data_ptr(), Bf.parent.data_ptr(), Bf.pcand.data_ptr()
    u.n_last, u.n_outlen, u.n_klens = Bf.last.data_ptr(), Bf.outlen.data_ptr(), Bf.klens.data_ptr()
    u.hist_parent, u.hist_token = Bf.hist_parent.data_ptr(), Bf.hist_token.data_ptr()
    u.res_score, u.res_step, u.res_parent = Bf.res_score.data_ptr(), Bf.res_step.data_ptr(), Bf.res_parent.data_ptr()
    u.state = Bf.state.data_ptr()
    u.host_mirror = Bf.mirror_host.data_ptr()      # pinned: the tail kernel writes it, the host polls it (no copy engine)


def rnnlm_rows_pair(lm, LA, Bf, nb, V, dt_code, even_src):
    """the lib.RnnlmRows of the even and the odd step of a captured pair -> (rows, tabs, ws): emoasr_rnnlm_step_rows over the nb rows
    of the chain, its state in the two halves of Bf.lm_h / lm_c, its raw logits in Bf.lm_logits; tabs the weight pointer tables (host
    arrays of device pointers) and ws the workspace, ONE set for both structs -- the caller keeps all three alive with the graphs.
    LA = lm._prepare().  even_src: the half the EVEN step reads; it writes the other one, the odd step does the reverse.
      1 -- the joint search: its K / V caches and scorer states call index 1 "previous" on step 0, the LM's pools follow them; it
           zeroes half 1 before every run;
      0 -- the LAS search: pool k is the source of step k, as with its own state pools; its reset zeroes half 0.
    On step 0 every row's parent is its search's row 0, so the zeroed half makes the step start from the LM's zero state (the
    warm-up steps write both halves: the zeroing comes after them)."""
    ws = torch.empty(lib.size_query("emoasr_rnnlm_step_rows_ws_bytes", dt_code, nb, lm.H), device=Bf.lm_h.device, dtype=torch.uint8)
    ptrs = ctypes.c_void_p * lm.L
    lm_w = [lm._w(l) for l in range(lm.L)]
    tabs = (ptrs(*[w[0].data_ptr() for w in lm_w]), ptrs(*[w[1].data_ptr() for w in lm_w]), ptrs(*[b.data_ptr() for b in lm._bias]))
    rows = [ops.rnnlm_rows_fill(nb, V, LA.w("lm.embed.weight"), tabs, LA.w("lm.output.weight"), LA.p("lm.output.bias"), Bf.lm_h,
                                Bf.lm_c, (even_src ^ k) * nb, (even_src ^ k ^ 1) * nb, Bf.lm_logits, ws) for k in (0, 1)]
    return rows, tabs, ws


def capture_two_steps(step, reset):
    """step(k): the launches of an even (k = 0) / odd (k = 1) step on the current stream -> [graph of the even steps, graph of the odd
    steps].  Warm-up with every search marked finished (the bookkeeping returns at once, the networks run on valid rows): every
    kernel's lazy one-time setup happens outside the capture.  Then each step is captured once: a linear chain on one stream.
    The graphs hold raw addresses: the caller stores them with everything the launches point at."""
    reset(1)
    for k in (0, 1):
        step(k)
    torch.cuda.current_stream().synchronize()
    graphs = []
    for k in (0, 1):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"), ops.stream_scope():
            step(k)
        graphs.append(g)
    return graphs


def capture_after_warmup(body, device, warm=None):
    """-> (graph, what the captured body() returned): body's launches captured as a HIP graph with the DEFAULT capture mode (not
    capture_two_steps' relaxed one), after a warm-up outside the capture (allocator, lazy initialisation, per-stream scratch) on a
    fresh side stream.  warm: the warm-up, when it is more than one run of body."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (warm or body)()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    return graph, out


def batch_step_reported(mirror, i, S, main):
    """wait until emoasr_beam_update_batch's pinned mirror {position, finished searches} shows step i - 1 -> whether every search
    has finished"""
    spins, t_wait = 0, None
    while mirror[0] < i and mirror[1] < S:
        _yield()   # the runtime's own threads (signal handling, graph bookkeeping) may share this core
        spins += 1
        if spins & 0xFFF == 0:   # a lost launch / a faulted device must surface, not spin forever
            now = time.perf_counter()
            t_wait = now if t_wait is None else t_wait
            if now - t_wait > _STEP_DEADLINE_S:
                raise RuntimeError(f"batched beam search: step {i - 1} did not report within {_STEP_DEADLINE_S:.0f} s "
                                   f"(stream idle: {main.query()}; last library error: {lib.load().emoasr_last_error().decode()!r})")
    return mirror[1] >= S


def replay_until_done(graphs, Bf, max_steps, S, stats_owner, stats_name):
    """the search loop over the reset books -> the downloaded pack (numpy int32; batch_nbest_from_pack reads it).  Steps are issued
    one ahead of the mirror they depend on: a step replayed after the end changes nothing, and the GPU never waits for the host.
    stats_owner.<stats_name>: the running totals {steps, loop_s, utts, calls} the bench tools read."""
    mirror = Bf.mirror_host.numpy()
    mirror[:] = (0, 0)
    main = torch.cuda.current_stream()
    main.synchronize()     # (the mirror is host memory: the caller's reset must not race the first step's store)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(main)
    gc_was_on = gc.isenabled()
    gc.disable()           # (a collection in the middle of the loop stalls a step for milliseconds)
    try:
        for i in range(max_steps):
            graphs[i & 1].replay()
            if i >= 1 and batch_step_reported(mirror, i, S, main):
                break
        ev1.record(main)
        main.synchronize()
    finally:
        if gc_was_on:      # (also on an exception: the collector must not stay off for the rest of the process)
            gc.enable()
    stats = getattr(stats_owner, stats_name, None)
    if stats is None:
        stats = {"steps": 0, "loop_s": 0.0, "utts": 0, "calls": 0}
        setattr(stats_owner, stats_name, stats)
    stats["steps"] += int(mirror[0]); stats["loop_s"] += 1e-3 * ev0.elapsed_time(ev1); stats["utts"] += S; stats["calls"] += 1
    return Bf.pack.cpu().numpy()      # the one download


def batch_nbest_from_pack(host, o, S, W, Lmax, sort=True):
    """the downloaded pack (batch_pack_sizes; o: the parts' offsets) -> (hyps[s], scores[s]): the token sequences rebuilt from
    the (parent, token) history, each search's results sorted by score (stable); sort=False: in the order they were found"""
    rs = host[o[0]:o[1]].view(np.float64)
    state = host[o[1]:o[2]].reshape(S, 4)
    rstep, rpar = host[o[2]:o[3]], host[o[3]:o[4]]
    hp, ht = host[o[4]:o[5]].reshape(Lmax, S, W), host[o[5]:o[6]].reshape(Lmax, S, W)
    hyps, scores = [], []
    for s in range(S):
        results = []
        for k in range(int(state[s, 2])):
            toks, slot = [], int(rpar[s * W + k])
            for p in range(int(rstep[s * W + k]) - 1, -1, -1):
                toks.append(int(ht[p, s, slot]))
                slot = int(hp[p, s, slot])
            results.append((toks[::-1], float(rs[s * W + k])))
        if sort:
            results = sorted(results, key=lambda r: r[1], reverse=True)
        hyps.append([r[0] for r in results])
        scores.append([r[1] for r in results])
    return hyps, scores


def lm_type_why_not(lm, lm_type):
    """the first admission check of every fused device search: the LM is of the type whose state the search can hold"""
    if getattr(lm, "lm_type", None) != lm_type:
        note = " (no per-hypothesis state the slot pools could hold)" if lm_type == "rnn" else ""
        return f"lm_type {getattr(lm, 'lm_type', None)!r} is not {lm_type!r}{note}"
    return None


def lm_compute_why_not(eng, lm, dtypes=None):
    """the LM computes as the engine does: the same dtype (one of dtypes, when the kernels take no other), the same product mode"""
    if lm.compute_dtype != eng.dtype or (dtypes is not None and lm.compute_dtype not in dtypes) or bool(lm.f32_split) != bool(eng.split):
        return f"the LM computes in {lm.compute_dtype} (split products: {bool(lm.f32_split)}), the model in {eng.dtype} ({bool(eng.split)})"
    return None


def rnnlm_rows_why_not(eng, V, lm):
    """why emoasr_rnnlm_step_rows cannot step this LM inside a lockstep chain of an engine with vocabulary V (None: it can): the
    reasons the searches share; each adds its own (beam and candidate widths, environment switches)"""
    why = lm_type_why_not(lm, "rnn")
    if why is None and lm.V != V:   # the scores kernel soft-maxes the first V columns; the reference soft-maxes all of the LM's, then slices
        why = f"the LM's vocabulary ({lm.V}) is not the model's ({V})"
    why = why or lm_compute_why_not(eng, lm)
    if why is not None:
        return why
    code = lib.F32X3 if lm.f32_split else {torch.float32: lib.F32, torch.bfloat16: lib.BF16}.get(lm.compute_dtype)
    if code is None or lib.size_query("emoasr_rnnlm_step_rows_supported", code, lm.L, lm.E, lm.H) != 1:
        return f"the LM's sizes (embedding {lm.E}, hidden {lm.H}, layers {lm.L}) are outside emoasr_rnnlm_step_rows' shape plan"
    return None


# ------------------------------------------------------------------------------------------------ the fusion grids
# len_weight never touches a search (it is added to a finished hypothesis' score only), so a cell's N-best list is the result set of
# its lm_weight's search, rescored and stably re-sorted on the host; every distinct positive lm_weight is searched once.
def grid_cell_plan(lm_weights, len_weights, has_lm=True):
    """-> (search_weights, cells): search_weights the distinct lm_weights to search in order of first appearance, every weight
    <= 0 (and every weight without an LM) folded into ONE entry 0.0, the search without the LM; cells[c] = (index into
    search_weights, index into len_weights) for the cells in lm_weight-outer, len_weight-inner order.  Weights are compared as
    doubles, unrounded: 0.30000000000000004 and 0.3 are two searches."""
    search_weights, index, cells = [], {}, []
    for a in lm_weights:
        a = float(a)
        a = a if (has_lm and a > 0) else 0.0
        if a not in index:
            index[a] = len(search_weights)
            search_weights.append(a)
        cells += [(index[a], j) for j in range(len(len_weights))]
    return search_weights, cells


def grid_chunk_plan(n_utts, n_weights, cap):
    """chunks of at most cap searches for n_utts utterances of n_weights searches each -> [[(utterance, first weight, count)]]:
    whole utterances per chunk while an utterance fits a chunk; an utterance with more searches than a chunk is cut into
    pieces of cap (each piece forms that utterance's memory projection again)"""
    assert n_weights >= 1 and cap >= 1
    chunks, cur, room = [], [], cap
    for b in range(n_utts):
        k0 = 0
        while k0 < n_weights:
            left = n_weights - k0
            if left > room and (cur and (left <= cap or k0 == 0)):   # does not fit behind what the chunk holds: a new chunk
                chunks.append(cur)
                cur, room = [], cap
            n = min(left, room)
            cur.append((b, k0, n))
            k0 += n
            room -= n
            if room == 0:
                chunks.append(cur)
                cur, room = [], cap
    if cur:
        chunks.append(cur)
    return chunks


def grid_chunks(B, n_positive, cap, elens):
    """grid_chunk_plan, unpacked per chunk -> (utts, n, sutt, k_local): utts the chunk's utterances (consecutive), n their frame
    counts, and per search of the chunk the index of its utterance INSIDE the chunk (sutt) and of its weight among the n_positive
    positive ones (k_local)"""
    for chunk in grid_chunk_plan(B, n_positive, cap):
        utts = sorted({b for b, _, _ in chunk})
        local = {b: i for i, b in enumerate(utts)}
        yield (utts, [elens[b] for b in utts], [local[b] for b, _, cnt in chunk for _ in range(cnt)],
               [k0 + j for _, k0, cnt in chunk for j in range(cnt)])


def expand_len_weights(hyps, scores, len_weights, offset=2):
    """the results of ONE search at len_weight 0 in the order the search found them -> per len_weight w (hyps, scores): every score
    + w * (len(hyp) + offset) in double -- what emoasr_beam_update_batch writes as cscore + len_weight * (double)(pos + 2), the
    library being compiled without contraction of the multiply-add; the transducer, whose hypotheses keep their leading <sos>, passes
    offset 0 -- sorted by score with the stable order of batch_nbest_from_pack"""
    out = []
    for w in len_weights:
        w = float(w)
        sc = [float(s) + w * float(len(h) + offset) for h, s in zip(hyps, scores)]
        order = sorted(range(len(sc)), key=lambda i: sc[i], reverse=True)
        out.append(([hyps[i] for i in order], [sc[i] for i in order]))
    return out


def run_fusion_grid(B, lm_weights, len_weights, has_lm, search_plain, search_fused, expand):
    """every (lm_weight, len_weight) cell of B utterances -> (hyps[b][c], scores[b][c]), cells in lm_weight-outer, len_weight-inner
    order.  found[b][k] = (hyps, scores) of utterance b under search weight k (grid_cell_plan):
      search_plain() -> (hyps[b], scores[b]) of all B: the search without the LM, called if some weight is <= 0 (or has_lm is false);
      search_fused(positive, weights, found): fills found[b][k] for every k in positive, called if some weight is positive;
      expand(found[b][k], weights[k]) -> one (hyps, scores) per len_weight."""
    weights, cells = grid_cell_plan(lm_weights, len_weights, has_lm)
    found = [[None] * len(weights) for _ in range(B)]
    positive = [k for k, a in enumerate(weights) if a > 0]
    if len(positive) < len(weights):
        k = weights.index(0.0)
        h, s = search_plain()
        for b in range(B):
            found[b][k] = (h[b], s[b])
    if positive:
        search_fused(positive, weights, found)
    hyps, scores = [], []
    for b in range(B):
        per_search = [expand(f, a) for f, a in zip(found[b], weights)]
        hyps.append([per_search[k][j][0] for k, j in cells])
        scores.append([per_search[k][j][1] for k, j in cells])
    return hyps, scores
