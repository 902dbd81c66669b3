"""RNN-LM shallow fusion in the LAS beam search on the device: emoasr_las_attend_cells bit for bit against
emoasr_las_attend_group on replicated frames, the fused step's first position against the host form, LASDecoder.decode under
las_lm_fusion = "fuse" against the reference's modules (tests/golden/las_fusion_tiny.npz, written by
tests/golden/make_golden_las_fusion.py), the forms against each other, the (lm_weight, len_weight) grid, bf16, and the refusals."""
import logging
from types import SimpleNamespace

import pytest
import torch

from tests import las_beam_util as UB
from tests import las_fusion_util as U
from tests import las_ref
from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state

pytestmark = pytest.mark.gpu

D = 128
SENTINEL = -768.0   # (exact in bf16)


# =========================================================================================== 1. the attention of the grid
PER_UTT = (1, 3, 2)                      # searches of the three utterances
SUTT = [0, 1, 1, 1, 2, 2]
DONE, SHORT = 2, 4                       # one finished search (inside utterance 1's run), one with a live count below W


def _cells_case(Ts, W, A, dtype, dev):
    """three utterances with 1, 3 and 2 searches: parents permuted inside each search, junk parents on the dead rows, one search
    finished, NaN in the source pool past each utterance's frames"""
    from emoasr_amd import ops
    S, nb, Tmax = len(SUTT), len(SUTT) * W, (max(Ts) + 63) // 64 * 64
    gen = torch.Generator().manual_seed(W * 1000 + A + sum(Ts))
    rn = lambda *s: torch.randn(*s, generator=gen)
    offs = [0, Ts[0], Ts[0] + Ts[1], sum(Ts)]
    c = SimpleNamespace(S=S, W=W, Ts=Ts, Tmax=Tmax, offs=offs)
    c.pk, c.eo, c.pq = rn(offs[-1], A).to(dtype).to(dev), rn(offs[-1], D).to(dtype).to(dev), rn(nb, A).to(dtype).to(dev)
    c.Wt = ops.LasWeights((0.3 * rn(10, 1, 201)).to(dev), (0.5 * rn(A, 10)).to(dev), (0.1 * rn(A)).to(dev), rn(1, A).to(dev))
    c.alive = [W - 1 if s == SHORT else W for s in range(S)]
    c.live = [0 if s == DONE else c.alive[s] for s in range(S)]     # rows the kernels must compute
    c.state = torch.tensor([[3, c.alive[s], 0, 1 if s == DONE else 0] for s in range(S)], dtype=torch.int32, device=dev)
    aw = torch.full((nb, Tmax), float("nan"))
    parent = torch.zeros(nb, dtype=torch.int32)
    for s in range(S):
        T = Ts[SUTT[s]]
        aw[s * W:(s + 1) * W, :T] = torch.softmax(2.0 * rn(W, T), dim=1)
        parent[s * W:(s + 1) * W] = s * W + torch.randperm(W, generator=gen).to(torch.int32)
        if s != DONE:
            parent[s * W + c.live[s]:(s + 1) * W] = torch.tensor([10 ** 9, -5] * W, dtype=torch.int32)[:W - c.live[s]]
    c.aw_src, c.parent = aw.to(dev), parent.to(dev)
    c.moff = torch.tensor(offs, dtype=torch.int32, device=dev)
    # the same searches for the group form: every search with its own copy of its utterance's frames
    rep = lambda x: torch.cat([x[offs[u]:offs[u + 1]] for u in SUTT]).contiguous()
    c.pk_rep, c.eo_rep = rep(c.pk), rep(c.eo)
    roffs = [0]
    for u in SUTT:
        roffs.append(roffs[-1] + Ts[u])
    c.moff_rep = torch.tensor(roffs, dtype=torch.int32, device=dev)
    return c


def _outputs(c, dev, dtype):
    nb = c.S * c.W
    return (torch.full((nb, c.Tmax), SENTINEL, device=dev), torch.full((nb, D), SENTINEL, device=dev, dtype=dtype),
            torch.full((nb, c.Tmax), SENTINEL, device=dev))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("A", [80, 512])
@pytest.mark.parametrize("W", [1, 3, 9])
@pytest.mark.parametrize("Ts", [(50, 33, 1), (70, 64, 65)], ids=["T50_33_1", "T70_64_65"])
def test_cells_attention_equals_the_group_form_on_replicated_frames(dev, Ts, W, A, dtype):
    """weights and context bit for bit, sentinels wherever the group form writes nothing; then one search's map entry out of range:
    that search writes nothing, every other row is unchanged"""
    from emoasr_amd import ops
    c = _cells_case(Ts, W, A, dtype, dev)
    sutt = ops.las_cells_map(SUTT, 3, dev)
    aw_g, ctx_g, sc_g = _outputs(c, dev, dtype)
    aw_c, ctx_c, sc_c = _outputs(c, dev, dtype)
    with ops.stream_scope(False):
        ops.las_attend_group(c.Wt, c.pk_rep, c.eo_rep, c.moff_rep, c.pq, c.aw_src, c.parent, c.state, W, aw_g, ctx_g, sc_g)
        ops.las_attend_cells(c.Wt, c.pk, c.eo, c.moff, sutt, c.pq, c.aw_src, c.parent, c.state, W, aw_c, ctx_c, sc_c)
    torch.cuda.synchronize()
    assert torch.equal(aw_c, aw_g) and torch.equal(ctx_c, ctx_g) and torch.equal(sc_c, sc_g)
    for s in range(c.S):      # (the comparison is not between two empty results)
        r0, n, T = s * W, c.live[s], Ts[SUTT[s]]
        assert (aw_c[r0 + n:r0 + W] == SENTINEL).all() and (ctx_c[r0 + n:r0 + W].float() == SENTINEL).all(), s
        assert (aw_c[r0:r0 + n, T:] == SENTINEL).all()
        if n:
            assert torch.isfinite(aw_c[r0:r0 + n, :T]).all() and torch.isfinite(ctx_c[r0:r0 + n].float()).all()
            assert torch.allclose(aw_c[r0:r0 + n, :T].sum(1), torch.ones(n, device=dev), atol=1e-3)
    for bad_s, bad_u in ((0, 3), (3, -1), (5, 10 ** 9)):
        m = list(SUTT)
        m[bad_s] = bad_u
        bad = torch.tensor(m, dtype=torch.int32, device=dev)     # (not through las_cells_map: the host check refuses it)
        aw_b, ctx_b, sc_b = _outputs(c, dev, dtype)
        with ops.stream_scope(False):
            ops.las_attend_cells(c.Wt, c.pk, c.eo, c.moff, bad, c.pq, c.aw_src, c.parent, c.state, W, aw_b, ctx_b, sc_b)
        torch.cuda.synchronize()
        rows = slice(bad_s * W, (bad_s + 1) * W)
        assert (aw_b[rows] == SENTINEL).all() and (ctx_b[rows].float() == SENTINEL).all() and (sc_b[rows] == SENTINEL).all()
        keep = torch.ones(c.S * W, dtype=torch.bool, device=dev)
        keep[rows] = False
        assert torch.equal(aw_b[keep], aw_g[keep]) and torch.equal(ctx_b[keep], ctx_g[keep])


def test_cells_refusals(dev):
    from ctypes import byref
    from emoasr_amd import lib, ops
    for sutt, n, what in (([0, 2, 2], 3, "after utterance 0"), ([1, 1], 2, "starts at utterance 0"), ([0, 1, 1], 3, "ends at utterance 1 of 3"),
                          ([0, 1, 0], 2, "after utterance 1"), ([0], 2, "2 utterances for 1 searches")):
        with pytest.raises(lib.EmoasrHipError, match=what):
            ops.las_cells_map(sutt, n, dev)
    assert ops.las_cells_map(SUTT, 3, dev).tolist() == SUTT
    z = lambda *s, d=torch.float32: torch.zeros(*s, device=dev, dtype=d)
    A, T, nb = 80, 4, 2
    Wt = ops.LasWeights(z(10, 1, 201), z(A, 10), z(A), z(1, A))
    state = torch.tensor([[0, 1, 0, 0]] * 2, dtype=torch.int32, device=dev)
    moff = torch.tensor([0, T], dtype=torch.int32, device=dev)
    c = lib.LasAttendCells()
    ops._las_group_args(Wt, z(T, A), z(T, D), moff, z(nb, A), z(nb, 64), z(nb, d=torch.int32), state, 1, z(nb, 64), z(nb, D), z(nb, 64),
                        a=c.g, S=2)
    sutt = z(2, d=torch.int32)
    for U_, ptr, what in ((1, None, "missing arguments"), (0, sutt.data_ptr(), "0 utterances for 2 searches"),
                          (3, sutt.data_ptr(), "3 utterances for 2 searches")):
        c.U, c.sutt = U_, ptr
        with pytest.raises(lib.EmoasrHipError, match="las_attend_cells: " + what):
            lib.call("emoasr_las_attend_cells", lib.F32, byref(c), ops._stream())
    c.U, c.sutt, c.g.W = 1, sutt.data_ptr(), 33
    with pytest.raises(lib.EmoasrHipError, match="las_attend_cells: group size 33 outside 1..32"):
        lib.call("emoasr_las_attend_cells", lib.F32, byref(c), ops._stream())


# =========================================================================================== 2. the searches
_CACHE = {}


def _las():
    if "las" not in _CACHE:
        _CACHE["las"] = las_ref.load_las_golden()
    return _CACHE["las"]


def _model(dev, mode):
    """the las_tiny model (eval mode) and the rnnlm_tiny LM in the same compute dtype, one pair per dtype for the module"""
    if mode not in _CACHE:
        from emoasr_amd.modeling.lm import LM
        model = _asr(dev, mode)
        lm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=mode)
        lm.load_state_dict(rnnlm_state(rnnlm_golden()))
        _CACHE[mode] = (model, lm.to(dev).eval())
    return _CACHE[mode]


def _asr(dev, mode):
    """a las_tiny model of its own (eval mode): its engine has captured nothing yet"""
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, _ = _las()
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**las_ref.las_asr_config(cfg)), compute_dtype=mode)
    model.load_state_dict(sd, strict=False)
    model.decoder.score.dropout_attn_rate = 0.0
    return model.to(dev).eval()


@pytest.fixture
def fused(dev):
    """(f32 model with las_lm_fusion = "fuse" for the test, the LM)"""
    model, lm = _model(dev, torch.float32)
    model.decoder.las_lm_fusion = "fuse"
    yield model, lm
    model.decoder.las_lm_fusion = "ignore"
    model.decoder.las_beam_impl = "single"


@pytest.fixture(scope="module")
def gold():
    return U.load_las_fusion_golden()[1]


@pytest.fixture(scope="module")
def gold_unfused():
    return UB.load_las_beam_golden()[1]


def _padded(searches, dev, seed=3):
    """the searches' frames as ONE padded batch; the padding past elens is 50 * randn"""
    g = _las()[2]
    elens = [t for _, t in searches]
    gen = torch.Generator().manual_seed(seed)
    eouts = 50.0 * torch.randn(len(searches), max(elens), D, generator=gen)
    for b, (u, t) in enumerate(searches):
        eouts[b, :t] = g[f"decode/{u}/eouts"][:t]
    return eouts.to(dev), elens


def _count(monkeypatch, model, lm):
    """-> (calls of the engine's batched search, host LM steps) from here on"""
    from emoasr_amd.modeling.functions import _engine_of
    eng = _engine_of(model.decoder)
    calls, steps = [], []
    orig, orig_step = eng.las_beam_search_batch, lm.step
    monkeypatch.setattr(eng, "las_beam_search_batch", lambda *a, **k: (calls.append(len(a[1])), orig(*a, **k))[1])
    monkeypatch.setattr(lm, "step", lambda *a, **k: (steps.append(1), orig_step(*a, **k))[1])
    return calls, steps


def _same(a, b, tol):
    return len(a) == len(b) and all(abs(x - y) < tol for x, y in zip(a, b))


def test_first_position_of_the_fused_step(dev, fused, monkeypatch):
    """the device chain's first step (one live row per search) against las_step(first=True) with the host fused row, on the three
    uncut utterances: the top-W tokens equal, the values within 1e-4"""
    from emoasr_amd.modeling.functions import _engine_of
    model, lm = fused
    eng = _engine_of(model.decoder)
    W, mu = 4, 0.5
    searches = U.SEARCHES[:3]
    eouts, elens = _padded(searches, dev)
    dec = model.decoder
    eng._las_beam_chunk(eouts, elens, W, 0.0, dec.eos_id, 1, lm, mu)          # max_len = 1: exactly the first step
    Bf = eng._las_beam_bufs[1]
    torch.cuda.synchronize()
    vals, cands = Bf.vals.view(3, W, W)[:, 0].cpu(), Bf.cands.view(3, W, W)[:, 0].cpu()
    seen, orig = [], eng.las_step

    def spy(S, ids, parents, first, *a):
        out = orig(S, ids, parents, first, *a)
        if first:
            assert len(a) == 2 and a[1] == mu, "the host form hands the LM's rows to the step"
            seen.append((out[0].cpu(), out[1].cpu()))
        return out

    monkeypatch.setattr(eng, "las_step", spy)
    for b, n in enumerate(elens):
        eng.las_beam_search(eouts[b:b + 1, :n].contiguous(), W, 0.0, dec.eos_id, 1, lm=lm, lm_weight=mu)
        hv, hi = seen[-1]
        assert hi[0].tolist() == cands[b].tolist(), (b, hi, cands[b])
        assert (hv[0] - vals[b]).abs().max().item() < 1e-4, (b, hv, vals[b])
    assert len(seen) == 3


def test_replayed_graphs_outlive_a_collection(dev, fused):
    """the fused chunk of B = 3, elens (9, 4, 2), W = 4 is captured on one set of frames; after gc.collect() the same graphs are
    replayed on other frames of the same shape and return exactly what a fresh engine, which captures anew, returns for them:
    everything the captured launches point at (structs, pointer tables, workspace) is still alive"""
    import gc
    from emoasr_amd.modeling.functions import _engine_of
    model, lm = fused
    first, elens = _padded([(0, 9), (1, 4), (2, 2)], dev)
    second, _ = _padded([(1, 9), (2, 4), (0, 2)], dev)
    assert elens == [9, 4, 2]
    dec = model.decoder
    run = lambda eng, frames: eng._las_beam_chunk(frames, elens, 4, 0.0, dec.eos_id, dec.max_decode_ylen, lm, 0.3)
    eng = _engine_of(dec)
    run(eng, first)
    graphs = eng._las_beam_bufs[1].graphs[1]
    gc.collect()
    got = run(eng, second)
    assert eng._las_beam_bufs[1].graphs[1] is graphs, "the second call replays the first call's graphs"
    want = run(_engine_of(_asr(dev, torch.float32).decoder), second)
    assert got == want, (got, want)
    assert all(len(h) >= 1 for h in got[0]) and got != run(eng, first)


_E2E = [(a, W, lw) for a, W in U.CASES for lw in U.LEN_WEIGHTS]


@pytest.mark.parametrize("a,W,lw", _E2E, ids=[f"lm{a}-W{W}-lw{lw}" for a, W, lw in _E2E])
def test_fused_sets_against_the_reference_f32(dev, fused, gold, gold_unfused, a, W, lw, monkeypatch):
    """set A as ONE decode call on the padded batch under "fuse": the fixture's hypotheses in order, scores within 1e-3 |score|
    (test_sets_against_the_reference_f32's bar), exactly one batched search and no host LM step; the same call under the default
    "ignore" returns the unfused lists of las_beam_tiny"""
    model, lm = fused
    eouts, elens = _padded(U.SEARCHES, dev)
    calls, steps = _count(monkeypatch, model, lm)
    hyps, scores, logits, aligns = model.decoder.decode(eouts, torch.tensor(elens), None, W, lw, lm=lm, lm_weight=a, decode_ctc_weight=0.3)
    assert calls == [len(U.SEARCHES)] and steps == [] and logits is None and aligns is None
    assert len(hyps) == len(scores) == len(U.SEARCHES)
    for b, (u, t) in enumerate(U.SEARCHES):
        want, wscores = U.fused_nbest(gold, u, t, W, lw, a)
        assert hyps[b] == want, (b, hyps[b], want)
        assert len(scores[b]) == len(wscores)
        assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores[b], wscores)), (b, scores[b], wscores)
    model.decoder.las_lm_fusion = "ignore"
    hyps, scores, _, _ = model.decoder.decode(eouts, torch.tensor(elens), None, W, lw, lm=lm, lm_weight=a, decode_ctc_weight=0.3)
    assert calls == [len(U.SEARCHES)] * 2 and steps == []
    for b, (u, t) in enumerate(U.SEARCHES):
        want, wscores = UB.golden_nbest(gold_unfused, u, t, W, lw)
        assert hyps[b] == want, (b, hyps[b], want)
        assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores[b], wscores)), (b, scores[b], wscores)


@pytest.mark.parametrize("lw", U.LEN_WEIGHTS)
def test_forms_against_each_other(dev, fused, gold, lw, monkeypatch):
    """W = 3, lm_weight = 0.5, set A: every utterance alone through the host form, one utterance through las_beam_impl = "batch", and
    chunks [2, 2, 1] -- equal hypotheses, scores within 1e-4 (test_batch_equals_the_single_search's bar)"""
    from emoasr_amd.engine import las as eng_las
    from emoasr_amd.modeling.functions import _engine_of
    model, lm = fused
    dec = model.decoder
    W, a = 3, 0.5
    eouts, elens = _padded(U.SEARCHES, dev)
    hyps, scores, _, _ = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
    assert hyps == [U.fused_nbest(gold, u, t, W, lw, a)[0] for u, t in U.SEARCHES]
    calls, steps = _count(monkeypatch, model, lm)
    for b, n in enumerate(elens):
        one = eouts[b:b + 1, :n].contiguous()
        h, s, _, _ = dec.decode(one, [n], None, W, lw, lm=lm, lm_weight=a)
        assert calls == [] and len(steps) >= 1, "one utterance under 'single' is the host form, which steps the LM itself"
        assert h == hyps[b] and _same(s, scores[b], 1e-4), (b, h, hyps[b], s, scores[b])
        steps.clear()
        dec.las_beam_impl = "batch"
        h2, s2, l2, a2 = dec.decode(eouts[b:b + 1], [n], None, W, lw, lm=lm, lm_weight=a)     # (its padding still attached)
        dec.las_beam_impl = "single"
        assert calls == [1] and steps == [] and l2 is None and a2 is None
        calls.clear()
        assert h2 == hyps[b] and isinstance(s2, list) and _same(s2, scores[b], 1e-4)
    eng = _engine_of(dec)
    chunks, orig = [], eng._las_beam_chunk
    monkeypatch.setattr(eng_las, "las_beam_chunk_capacity", lambda *a_, **k: 2)
    monkeypatch.setattr(eng, "_las_beam_chunk", lambda *a_, **k: (chunks.append((len(a_[1]), a_[6] is lm, a_[7])), orig(*a_, **k))[1])
    parts = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
    assert chunks == [(2, True, a), (2, True, a), (1, True, a)]
    assert parts[0] == hyps and all(_same(x, y, 1e-4) for x, y in zip(parts[1], scores))


@pytest.mark.parametrize("W", [3, 10])
def test_grid(dev, fused, gold, gold_unfused, W, monkeypatch):
    """lm_weights [0, 0.3, 0.5] x len_weights [0, 0.1] on set A in ONE call: every cell against the fixtures at the end-to-end bar and
    against one batched decode per cell (hypotheses equal, scores within 1e-4); the cells of one lm_weight come from one search
    (two chunks: the unfused searches, and ten fused ones over five utterances' frames); the lm_weight = 0 cells are bit-equal to
    the unfused batched search"""
    from emoasr_amd.modeling.functions import _engine_of, las_fusion_grid_apply
    model, lm = fused
    dec = model.decoder
    eng = _engine_of(dec)
    lm_weights, len_weights = [0.0, 0.3, 0.5], [0.0, 0.1]
    eouts, elens = _padded(U.SEARCHES, dev)
    chunks, orig = [], eng._las_beam_chunk

    def spy(*a, **k):
        grid = k.get("grid")
        chunks.append((len(a[1]), None if grid is None else (list(grid[0]), list(grid[1]))))
        return orig(*a, **k)

    monkeypatch.setattr(eng, "_las_beam_chunk", spy)
    _, steps = _count(monkeypatch, model, lm)
    hyps, scores = las_fusion_grid_apply(dec, eouts, elens, W, lm, lm_weights, len_weights)
    assert chunks == [(5, None), (5, ([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], [0.3, 0.5] * 5))] and steps == []
    monkeypatch.setattr(eng, "_las_beam_chunk", orig)
    assert len(hyps) == len(scores) == 5 and all(len(h) == 6 for h in hyps)
    cells = [(a, lw) for a in lm_weights for lw in len_weights]
    for c, (a, lw) in enumerate(cells):
        dec.las_lm_fusion = "fuse" if a > 0 else "ignore"
        h1, s1, _, _ = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
        for b, (u, t) in enumerate(U.SEARCHES):
            want, wscores = U.fused_nbest(gold, u, t, W, lw, a) if a > 0 else UB.golden_nbest(gold_unfused, u, t, W, lw)
            assert hyps[b][c] == want, (a, lw, b, hyps[b][c], want)
            assert len(scores[b][c]) == len(wscores)
            assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores[b][c], wscores)), (a, lw, b)
            assert h1[b] == hyps[b][c] and _same(s1[b], scores[b][c], 1e-4), (a, lw, b, s1[b], scores[b][c])
            if a == 0:
                assert s1[b] == scores[b][c], (lw, b, s1[b], scores[b][c])       # bit-equal


@pytest.mark.parametrize("a,W,lw", [(0.5, 1, 0.0), (0.5, 1, 0.1), (1.0, 1, 0.0), (1.0, 1, 0.1), (0.5, 4, 0.0), (0.5, 4, 0.1)])
def test_fused_bf16(dev, gold, a, W, lw):
    """test_batch_bf16's rule on the three uncut utterances: width 1 (margins 3.5e-2 and up) gives the fixture's hypothesis, its score
    within 2e-2 |w| + 2e-2; at width 4 the margins are narrower than bf16's rounding and only the best score is held to that bar"""
    model, lm = _model(dev, torch.bfloat16)
    model.decoder.las_lm_fusion = "fuse"
    try:
        searches = U.SEARCHES[:3]
        eouts, elens = _padded(searches, dev)
        hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
    finally:
        model.decoder.las_lm_fusion = "ignore"
    for b, (u, t) in enumerate(searches):
        want, wscores = U.fused_nbest(gold, u, t, W, lw, a)
        assert hyps[b] and scores[b]
        if W == 1:
            assert hyps[b] == want, (b, hyps[b], want)
        assert abs(scores[b][0] - wscores[0]) <= 2e-2 * abs(wscores[0]) + 2e-2, (b, scores[b], wscores)


def test_refusals_and_fall_backs(dev, fused, monkeypatch, caplog):
    """width 33, an LM with another vocabulary and a Transformer LM on a batch: the host form per utterance with the batch's return
    shape (the reason logged); a masked LM and an utterance without frames are refused"""
    from emoasr_amd.modeling import functions as F
    from emoasr_amd.modeling.lm import LM, _NO_PREDICT
    from tests.util import LM_CFG, load_ctc_beam_golden
    model, lm = fused
    dec = model.decoder
    F._LAS_FUSION_LOGGED.clear()
    searches = U.SEARCHES[:3]
    eouts, elens = _padded(searches, dev)
    calls, steps = _count(monkeypatch, model, lm)
    fused3, fused3_scores, _, _ = dec.decode(eouts, elens, None, 3, 0.1, lm=lm, lm_weight=0.5)
    assert calls == [3]
    calls.clear()
    # beams wider than the device bookkeeping
    hyps, scores, _, _ = dec.decode(eouts, elens, None, 33, 0.1, lm=lm, lm_weight=0.5)
    assert calls == [] and len(steps) >= 3 and len(hyps) == len(scores) == 3
    for b, n in enumerate(elens):
        h, s, _, _ = dec.decode(eouts[b:b + 1, :n].contiguous(), [n], None, 33, 0.1, lm=lm, lm_weight=0.5)
        assert hyps[b] == h and _same(scores[b], s, 1e-4) and len(h) >= 1, b
    # the LM's vocabulary is wider than the model's: the host form soft-maxes all of it and slices, as the reference does
    torch.manual_seed(1)
    wide = LM(SimpleNamespace(**dict(RNNLM_CFG, vocab_size=RNNLM_CFG["vocab_size"] + 8)), compute_dtype=torch.float32).to(dev).eval()
    with caplog.at_level(logging.INFO):
        hyps, scores, _, _ = dec.decode(eouts, elens, None, 3, 0.1, lm=wide, lm_weight=0.5)
    assert calls == [] and len(hyps) == len(scores) == 3 and all(1 <= len(h) <= 3 for h in hyps)
    assert any("vocabulary (48)" in r.getMessage() for r in caplog.records)
    # a Transformer LM: the host form per utterance, the batch's return shape, the single call's results
    tlm = LM(SimpleNamespace(**LM_CFG), compute_dtype=torch.float32)
    tlm.load_state_dict(load_ctc_beam_golden()[2])
    tlm = tlm.to(dev).eval()
    with caplog.at_level(logging.INFO):
        hyps, scores, logits, aligns = dec.decode(eouts, elens, None, 3, 0.1, lm=tlm, lm_weight=0.5)
    assert calls == [] and logits is None and aligns is None and len(hyps) == len(scores) == 3
    assert any("lm_type 'transformer'" in r.getMessage() for r in caplog.records)
    for b, n in enumerate(elens):
        h, s, _, _ = dec.decode(eouts[b:b + 1, :n].contiguous(), [n], None, 3, 0.1, lm=tlm, lm_weight=0.5)
        assert hyps[b] == h and _same(scores[b], s, 1e-4) and len(h) >= 1, b
    unfused = dec.decode(eouts, elens, None, 3, 0.1)
    calls.clear()
    assert hyps != unfused[0] or not all(_same(x, y, 1e-6) for x, y in zip(scores, unfused[1])), "the Transformer LM was not fused"
    # refused
    with pytest.raises(NotImplementedError) as info:
        dec.decode(eouts, elens, None, 3, 0.1, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.5)
    assert str(info.value) == _NO_PREDICT
    with pytest.raises(ValueError, match="1 <= elens"):
        dec.decode(eouts, [elens[0], 0, elens[2]], None, 3, 0.1, lm=lm, lm_weight=0.5)
    dec.las_lm_fusion = "both"
    with pytest.raises(ValueError, match="las_lm_fusion"):
        dec.decode(eouts, elens, None, 3, 0.1, lm=lm, lm_weight=0.5)
    dec.las_lm_fusion = "fuse"
    # and the device form is still what a batch gets
    again = dec.decode(eouts, elens, None, 3, 0.1, lm=lm, lm_weight=0.5)
    assert calls == [3] and again[0] == fused3 and again[1] == fused3_scores
