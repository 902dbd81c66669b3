"""The batched LAS beam search on the device: the kernels of csrc/las_beam.hip against float64 and against
torch, the search (engine/las.py:las_beam_search_batch) through LASDecoder.decode against the reference's N-best lists
(tests/golden/las_beam_tiny.npz, written by tests/golden/make_golden_las_beam.py) and against today's single search, and the
N-best rows of decode.test over a batch."""
from types import SimpleNamespace

import pytest
import torch

from tests import las_beam_util as U
from tests import las_ref

pytestmark = pytest.mark.gpu

D = 128
SENTINEL = -768.0   # (exact in bf16)


# =========================================================================================== 1. grouped attention
def _group_case(Ts, W, A, dtype, dev, rot):
    """three searches: one fully live, one with a live count below W, one finished (roles rotated by `rot`); parents permuted
    inside each search, junk parents on the dead rows, NaN in the source pool past every search's frames"""
    from emoasr_amd import ops
    S, nb, Tmax = 3, 3 * W, (max(Ts) + 63) // 64 * 64
    gen = torch.Generator().manual_seed(W * 1000 + A + sum(Ts) + 7 * rot)
    rn = lambda *s: torch.randn(*s, generator=gen)
    offs = [0, Ts[0], Ts[0] + Ts[1], sum(Ts)]
    c = SimpleNamespace(S=S, W=W, Ts=Ts, Tmax=Tmax, offs=offs)
    c.pk, c.eo, c.pq = rn(offs[-1], A).to(dtype).to(dev), rn(offs[-1], D).to(dtype).to(dev), rn(nb, A).to(dtype).to(dev)
    c.Wt = ops.LasWeights((0.3 * rn(10, 1, 201)).to(dev), (0.5 * rn(A, 10)).to(dev), (0.1 * rn(A)).to(dev), rn(1, A).to(dev))
    roles = [("live", "short", "done")[(s + rot) % 3] for s in range(S)]
    c.alive = [W if r != "short" else W - 1 for r in roles]
    c.live = [0 if r == "done" else n for r, n in zip(roles, c.alive)]     # rows the kernels must compute
    c.state = torch.tensor([[3, c.alive[s], 0, 1 if roles[s] == "done" else 0] for s in range(S)], dtype=torch.int32, device=dev)
    aw = torch.full((nb, Tmax), float("nan"))
    parent = torch.zeros(nb, dtype=torch.int32)
    for s in range(S):
        aw[s * W:(s + 1) * W, :Ts[s]] = torch.softmax(2.0 * rn(W, Ts[s]), dim=1)
        parent[s * W:(s + 1) * W] = s * W + torch.randperm(W, generator=gen).to(torch.int32)
        if roles[s] != "done":
            parent[s * W + c.live[s]:(s + 1) * W] = torch.tensor([10 ** 9, -5] * W, dtype=torch.int32)[:W - c.live[s]]
    c.aw_src, c.parent = aw.to(dev), parent.to(dev)
    c.moff = torch.tensor(offs, dtype=torch.int32, device=dev)
    return c


def _run_group(c, dev, dtype, s=None):
    """the grouped step on the case (s: that search alone, as a batch of one) -> (aw_dst, ctx), sentinel where nothing is written"""
    from emoasr_amd import ops
    W = c.W
    if s is None:
        pk, eo, moff, pq, aw_src, parent, state = c.pk, c.eo, c.moff, c.pq, c.aw_src, c.parent, c.state
    else:
        r = slice(s * W, (s + 1) * W)
        pk, eo = c.pk[c.offs[s]:c.offs[s + 1]].contiguous(), c.eo[c.offs[s]:c.offs[s + 1]].contiguous()
        moff = torch.tensor([0, c.Ts[s]], dtype=torch.int32, device=dev)
        pq, aw_src, state = c.pq[r].contiguous(), c.aw_src[r].contiguous(), c.state[s:s + 1].contiguous()
        parent = c.parent[r].clone()
        parent[:c.live[s]] -= s * W
    nb = pq.shape[0]
    aw_dst = torch.full((nb, c.Tmax), SENTINEL, device=dev)
    scores = torch.full((nb, c.Tmax), SENTINEL, device=dev)
    ctx = torch.full((nb, D), SENTINEL, device=dev, dtype=dtype)
    with ops.stream_scope(False):
        ops.las_attend_group(c.Wt, pk, eo, moff, pq, aw_src, parent, state, W, aw_dst, ctx, scores)
    torch.cuda.synchronize()
    return aw_dst, ctx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("A", [80, 512])
@pytest.mark.parametrize("W", [1, 3, 8, 9, 32])
@pytest.mark.parametrize("Ts", [(1, 37, 211), (32, 33, 64)], ids=["T1_37_211", "T32_33_64"])
def test_grouped_attention_against_f64(dev, Ts, W, A, dtype):
    """three searches of different lengths in one launch against las_ref.attend_step in float64 from the rounded inputs.  The
    bar is measured in the same test: ops.las_attend_fwd on the same rows, the memory replicated and padded per row, against
    the same reference -- the grouped kernel stays within twice that error plus 1e-7 (another order of the soft-max sums).
    Dead rows keep the sentinel, a search's rows are bit-identical alone and inside the batch."""
    from emoasr_amd import ops
    for rot in range(3):   # every search takes every role, so every T_s is computed with all W rows
        c = _group_case(Ts, W, A, dtype, dev, rot)
        aw_dst, ctx = _run_group(c, dev, dtype)
        assert torch.isfinite(ctx.float()).all()
        f64 = lambda t: t.double().cpu()
        for s in range(c.S):
            r0, n, T = s * W, c.live[s], Ts[s]
            dead = slice(r0 + n, r0 + W)
            assert (aw_dst[dead] == SENTINEL).all() and (ctx[dead].float() == SENTINEL).all(), (rot, s)
            assert (aw_dst[r0:r0 + n, T:] == SENTINEL).all()
            if n == 0:
                continue
            rows = slice(r0, r0 + n)
            par = c.parent[rows].long()
            pk, eo = c.pk[c.offs[s]:c.offs[s + 1]], c.eo[c.offs[s]:c.offs[s + 1]]
            awp = c.aw_src[par][:, :T]
            want_aw, want_ctx = las_ref.attend_step(f64(pk)[None].expand(n, T, A), f64(c.pq[rows]), f64(awp), f64(eo)[None], None,
                                                    f64(c.Wt.filt), f64(c.Wt.w_conv), f64(c.Wt.b_conv), f64(c.Wt.w_score))
            # the comparator: today's step, every row with its own padded copy of the memory
            Tm = max(Ts)
            pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, Tm - T))[None].expand(n, Tm, t.shape[1]).contiguous()
            with ops.stream_scope(False):
                old_aw, old_ctx, _ = ops.las_attend_fwd(c.Wt, pad(pk), c.pq[rows].contiguous(),
                                                        torch.nn.functional.pad(awp, (0, Tm - T)).contiguous(), pad(eo),
                                                        torch.full((n,), T, dtype=torch.int32, device=dev))
            got_aw, got_ctx = aw_dst[rows, :T], ctx[rows]
            assert torch.isfinite(got_aw).all()
            for name, got, old, want in (("aw", got_aw, old_aw[:, :T], want_aw), ("ctx", got_ctx, old_ctx, want_ctx)):
                e_new, e_old = (f64(got) - want).abs().max().item(), (f64(old) - want).abs().max().item()
                print(f"las_attend_group {str(dtype)[6:]} W={W} A={A} T={T} rot={rot} {name}: max error {e_new:.3e}, "
                      f"las_attend_fwd {e_old:.3e}")
                assert e_new <= 2 * e_old + 1e-7, (name, rot, s, e_new, e_old)
            alone_aw, alone_ctx = _run_group(c, dev, dtype, s)
            assert torch.equal(alone_aw[:n, :T], got_aw) and torch.equal(alone_ctx[:n], got_ctx), (rot, s)


# =========================================================================================== 2. state gather
@pytest.mark.parametrize("W", [1, 5, 32])
def test_state_gather_equals_index_select(dev, W):
    from emoasr_amd import ops
    S, nb = 3, 3 * W
    gen = torch.Generator().manual_seed(W)
    shapes = [((224,), torch.bfloat16), ((96,), torch.float32), ((96,), torch.bfloat16), ((96,), torch.float32), ((8,), torch.bfloat16)]
    src = [torch.randn(nb, *s, generator=gen).to(d).to(dev) for s, d in shapes]
    dst = [torch.full((nb, *s), SENTINEL, dtype=d, device=dev) for s, d in shapes]
    alive = [W, W - 1, W]
    state = torch.tensor([[2, alive[0], 0, 0], [2, alive[1], 1, 0], [2, alive[2], 0, 1]], dtype=torch.int32, device=dev)
    live = [alive[0], alive[1], 0]
    parent = torch.cat([s * W + torch.randperm(W, generator=gen) for s in range(S)]).to(torch.int32)
    for s in range(S):
        parent[s * W + live[s]:(s + 1) * W] = -(10 ** 9)   # junk on the dead rows: never read
    parent = parent.to(dev)
    with ops.stream_scope(False):
        ops.las_state_gather(list(zip(src, dst)), parent, state, W)
    torch.cuda.synchronize()
    for a, b in zip(src, dst):
        for s in range(S):
            rows = slice(s * W, s * W + live[s])
            assert torch.equal(b[rows], a.index_select(0, parent[rows].long())), (s, a.dtype)
            assert (b[s * W + live[s]:(s + 1) * W].float() == SENTINEL).all(), (s, a.dtype)


# =========================================================================================== 3. refusals
def test_refusals(dev):
    from emoasr_amd import ops
    from emoasr_amd.lib import EmoasrHipError

    def attend(W, A, dtype=torch.float32):
        nb, T = max(W, 1), 4
        z = lambda *s, d=torch.float32: torch.zeros(*s, device=dev, dtype=d)
        Wt = ops.LasWeights(z(10, 1, 201), z(A, 10), z(A), z(1, A))
        state = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device=dev)
        moff = torch.tensor([0, T], dtype=torch.int32, device=dev)
        # (the Python wrapper holds S * W rows to the tensors; a width of 0 is given one row)
        a = ops._las_group_args(Wt, z(T, A, d=dtype), z(T, D, d=dtype), moff, z(nb, A, d=dtype), z(nb, 64), z(nb, d=torch.int32),
                                state, nb, z(nb, 64), z(nb, D, d=dtype), z(nb, 64))
        a.W = W
        from ctypes import byref
        from emoasr_amd import lib
        lib.call("emoasr_las_attend_group", ops.dt(z(1, d=dtype)), byref(a), ops._stream())

    for W in (0, 33):
        with pytest.raises(EmoasrHipError, match=f"group size {W} outside 1..32"):
            attend(W, 80)
    with pytest.raises(EmoasrHipError, match="A=520 must be a multiple of 8, at most 512"):
        attend(4, 520)
    with pytest.raises(EmoasrHipError, match="A=84 must be a multiple of 8"):
        attend(4, 84)
    for elens in ([5, 0, 3], [4, -1]):
        with pytest.raises(EmoasrHipError, match="offsets must rise"):
            ops.las_group_offsets(elens, dev)
    moff, offs = ops.las_group_offsets([5, 1, 3], dev)
    assert offs == [0, 5, 6, 9] and moff.tolist() == offs
    x = torch.zeros(33, 8, device=dev)
    state = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device=dev)
    with pytest.raises(EmoasrHipError, match="group size 33 outside 1..32"):
        ops.las_state_gather([(x, x.clone())], torch.zeros(33, dtype=torch.int32, device=dev), state, 33)
    y = torch.zeros(4, 6, device=dev)    # rows of 24 bytes
    with pytest.raises(EmoasrHipError, match="multiple of 16 bytes"):
        ops.las_state_gather([(y, y.clone())], torch.zeros(4, dtype=torch.int32, device=dev), state, 4)
    with pytest.raises(EmoasrHipError, match=r"17 arrays"):
        ops.las_state_gather([(x[:4], x[4:8].clone())] * 17, torch.zeros(4, dtype=torch.int32, device=dev), state, 4)


# =========================================================================================== 4. the search, end to end
_CACHE = {}


def _build(fx, dev, mode, encoder=False):
    from emoasr_amd.modeling.asr import ASR
    from tests.util import load_golden
    cfg, sd, _ = fx
    torch.manual_seed(0)
    model = ASR(SimpleNamespace(**las_ref.las_asr_config(cfg)), compute_dtype=mode)
    model.load_state_dict(sd, strict=False)
    if encoder:   # the l3_tiny encoder's weights live in that fixture
        _, sd3, _ = load_golden("l3_tiny")
        model.load_state_dict({k: v for k, v in sd3.items() if k.startswith("encoder.")}, strict=False)
    model.decoder.score.dropout_attn_rate = 0.0
    return model.to(dev).eval()


def _model(dev, mode, encoder=False):
    """the las_tiny model as tests/test_las_gpu.py builds it (eval mode), one per (dtype, encoder) for the module"""
    key = (str(mode), encoder)
    if key not in _CACHE:
        _CACHE[key] = _build(_las(), dev, mode, encoder)
    return _CACHE[key]


def _las():
    if "las" not in _CACHE:
        _CACHE["las"] = las_ref.load_las_golden()
    return _CACHE["las"]


@pytest.fixture(scope="module")
def gold():
    return U.load_las_beam_golden()[1]


def _padded(searches, dev, seed=3):
    """the searches' frames as ONE padded batch; the padding past elens is 50 * randn"""
    g = _las()[2]
    elens = [t for _, t in searches]
    gen = torch.Generator().manual_seed(seed)
    eouts = 50.0 * torch.randn(len(searches), max(elens), D, generator=gen)
    for b, (u, t) in enumerate(searches):
        eouts[b, :t] = g[f"decode/{u}/eouts"][:t]
    return eouts.to(dev), elens


def _count_batched(monkeypatch, model):
    """calls of the engine's batched search from here on"""
    from emoasr_amd.modeling.functions import _engine_of
    eng = _engine_of(model.decoder)
    calls, orig = [], eng.las_beam_search_batch
    monkeypatch.setattr(eng, "las_beam_search_batch", lambda *a, **k: (calls.append(len(a[1])), orig(*a, **k))[1])
    return calls


_SET_CASES = [(name, W) for name, spec in U.SETS.items() for W in spec["widths"]]


@pytest.mark.parametrize("lw", U.LEN_WEIGHTS)
@pytest.mark.parametrize("name,W", _SET_CASES, ids=[f"{n}-W{w}" for n, w in _SET_CASES])
def test_sets_against_the_reference_f32(dev, gold, name, W, lw, monkeypatch):
    """a whole set as ONE decode call on the padded batch: the reference's hypotheses in order, scores within 1e-3 |score| (the
    bar of test_beam_search_f32); `lm`, `lm_weight` and an intermediate decode_ctc_weight are accepted and ignored"""
    model = _model(dev, torch.float32)
    searches = U.SETS[name]["searches"]
    eouts, elens = _padded(searches, dev)
    calls = _count_batched(monkeypatch, model)
    hyps, scores, logits, aligns = model.decoder.decode(eouts, torch.tensor(elens), None, W, lw, lm=None, lm_weight=0.3,
                                                        decode_ctc_weight=0.3)
    assert calls == [len(searches)] and logits is None and aligns is None
    assert len(hyps) == len(scores) == len(searches)
    for b, (u, t) in enumerate(searches):
        want, wscores = U.golden_nbest(gold, u, t, W, lw)
        assert hyps[b] == want, (b, hyps[b], want)
        assert len(scores[b]) == len(wscores)
        assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores[b], wscores)), (b, scores[b], wscores)


@pytest.mark.parametrize("lw", U.LEN_WEIGHTS)
def test_batch_equals_the_single_search(dev, lw, monkeypatch):
    """set A at W = 4: every search also alone through today's single search -- equal hypotheses, scores within 1e-4 (the bar
    between the two f32 forms of the joint search); one utterance through las_beam_impl = "batch" has the single search's
    return shape and results"""
    model = _model(dev, torch.float32)
    searches = U.SETS["A"]["searches"]
    eouts, elens = _padded(searches, dev)
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, 4, lw)
    calls = _count_batched(monkeypatch, model)
    for b, n in enumerate(elens):
        one = eouts[b:b + 1, :n].contiguous()
        h, s, _, _ = model.decoder.decode(one, [n], None, 4, lw)
        assert calls == [], "one utterance stays with the single search"
        assert h == hyps[b] and len(s) == len(scores[b]) and all(abs(x - y) < 1e-4 for x, y in zip(s, scores[b])), (b, h, hyps[b])
        monkeypatch.setattr(model.decoder, "las_beam_impl", "batch")
        h2, s2, l2, a2 = model.decoder.decode(eouts[b:b + 1], [n], None, 4, lw)     # (its padding still attached)
        monkeypatch.setattr(model.decoder, "las_beam_impl", "single")
        assert calls == [1] and l2 is None and a2 is None
        calls.clear()
        assert h2 == h and isinstance(s2, list) and len(s2) == len(s) and all(abs(x - y) < 1e-4 for x, y in zip(s2, s))
    monkeypatch.setattr(model.decoder, "las_beam_impl", "neither")
    with pytest.raises(ValueError, match="las_beam_impl"):
        model.decoder.decode(eouts, elens, None, 4, lw)


@pytest.mark.parametrize("W,lw", [(1, 0.0), (1, 0.1), (4, 0.0), (4, 0.1)])
def test_batch_bf16(dev, W, lw):
    """the rule of test_beam_search_bf16, on the utterances it decodes (the uncut three, here as one batch): bf16 moves every
    log-probability by more than the recorded margins, so width 1 must give the reference's hypothesis, wider beams its BEST
    hypothesis first, the best score within 2e-2 |w| + 2e-2"""
    model = _model(dev, torch.bfloat16)
    searches = U.SETS["A"]["searches"][:3]
    eouts, elens = _padded(searches, dev)
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, W, lw)
    gold = U.load_las_beam_golden()[1]
    for b, (u, t) in enumerate(searches):
        want, wscores = U.golden_nbest(gold, u, t, W, lw)
        assert hyps[b] and hyps[b][0] == want[0], (b, hyps[b], want)
        assert abs(scores[b][0] - wscores[0]) <= 2e-2 * abs(wscores[0]) + 2e-2, (scores[b], wscores)


def test_chunking(dev, monkeypatch):
    """with a chunk capacity of two searches set A runs as chunks [2, 2, 1] and returns what it returns in one chunk (products
    over another number of rows may take another tile: scores within 1e-4, hypotheses equal)"""
    from emoasr_amd.engine import las as eng_las
    from emoasr_amd.modeling.functions import _engine_of
    model = _model(dev, torch.float32)
    eouts, elens = _padded(U.SETS["A"]["searches"], dev)
    whole = model.decoder.decode(eouts, elens, None, 4, 0.1)
    eng = _engine_of(model.decoder)
    chunks, orig = [], eng._las_beam_chunk
    monkeypatch.setattr(eng_las, "las_beam_chunk_capacity", lambda *a, **k: 2)
    monkeypatch.setattr(eng, "_las_beam_chunk", lambda *a, **k: (chunks.append(len(a[1])), orig(*a, **k))[1])
    parts = model.decoder.decode(eouts, elens, None, 4, 0.1)
    assert chunks == [2, 2, 1]
    assert parts[0] == whole[0]
    for a, c in zip(parts[1], whole[1]):
        assert len(a) == len(c) and all(abs(x - y) < 1e-4 for x, y in zip(a, c)), (a, c)


def test_endless_search(dev, monkeypatch):
    """<eos> never wins: every search runs out of steps at max_decode_ylen and returns no hypothesis"""
    from emoasr_amd.modeling.functions import _engine_of
    model = _build(_las(), dev, torch.float32)     # (its weights are changed: not the module's shared model)
    with torch.no_grad():
        model.decoder.output.bias[_las()[0]["eos_id"]] = -1e4
    model.engine().arena.refresh_shadow()
    eouts, elens = _padded(U.SETS["A"]["searches"], dev)
    for W in (1, 4):
        hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, W, 0.0)
        assert hyps == [[]] * 5 and scores == [[]] * 5
        stats = _engine_of(model.decoder)._las_beam_stats
        assert stats["steps"] == model.decoder.max_decode_ylen and stats["calls"] == 1
        stats.update(steps=0, calls=0)


def test_other_routes(dev, monkeypatch):
    """beam_width 33 takes the search per utterance with equal results and the batch's return shape; an utterance without frames is
    refused; decode_ctc_weight == 1 stays CTC greedy"""
    model = _model(dev, torch.float32)
    searches = U.SETS["A"]["searches"][:3]
    eouts, elens = _padded(searches, dev)
    calls = _count_batched(monkeypatch, model)
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, 33, 0.1)
    assert calls == [] and len(hyps) == 3
    for b, n in enumerate(elens):
        h, s, _, _ = model.decoder.decode(eouts[b:b + 1, :n].contiguous(), [n], None, 33, 0.1)
        assert hyps[b] == h and scores[b] == s and len(h) >= 1, b
    with pytest.raises(ValueError, match="1 <= elens"):
        model.decoder.decode(eouts, [elens[0], 0, elens[2]], None, 4, 0.0)
    a = model.decoder.decode(eouts, torch.tensor(elens), None, 4, 0.0, decode_ctc_weight=1)
    model.decoder.ctc._owner = model.decoder._owner
    b = model.decoder.ctc.decode(eouts, torch.tensor(elens), beam_width=1)
    assert a[0] == b[0] and len(a[0]) == 3 and calls == []


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_nbest_rows_of_a_three_utterance_loader(dev, tmp_path, monkeypatch):
    """decode.test(nbest=True) over one batch of three utterances gives the rows of three one-utterance loaders (scores within
    1e-4) and the five-column TSV.  A one-utterance loader hands its utterance over with the padding it has in the batch --
    padding leaks through the encoder's convolution layers, so a shorter utterance encoded alone is another input to the search,
    not another search (tests/test_ctc_beam_batch_gpu.py) -- and decodes its valid frames through las_beam_impl = "batch"; the
    longest utterance has no padding and is also compared with the default single search.  Beam width 1 gives one row per
    utterance through the same route."""
    from emoasr_amd import decode as dec
    from tests.util import load_golden
    model = _model(dev, torch.float32, encoder=True)
    _, _, g = load_golden("l3_tiny")
    xs, xlens = g["xs"], g["xlens"]
    n0 = int(xlens[0])
    assert n0 == int(xlens[:3].max())
    x3 = xs[:3, :n0].clone()
    l3 = xlens[:3].clone()
    ids = ["utt0", "utt1", "utt2"]
    batch = [{"utt_ids": ids, "texts": ["r0", "r1", "r2"], "xs": x3, "xlens": l3}]
    ones = [{"utt_ids": ids[b:b + 1], "texts": [f"r{b}"], "xs": x3[b:b + 1], "xlens": l3[b:b + 1]} for b in range(3)]
    calls = _count_batched(monkeypatch, model)
    for bw in (4, 1):
        args = (_Vocab(), bw, 0.1, 0.0, False, None, 0.0, dev)
        calls.clear()
        rows = dec.test(model, batch, *args, nbest=True)
        assert calls == [3]
        monkeypatch.setattr(model.decoder, "las_beam_impl", "batch")
        want = dec.test(model, ones, *args, nbest=True)
        assert calls == [3, 1, 1, 1]
        monkeypatch.setattr(model.decoder, "las_beam_impl", "single")
        first = dec.test(model, ones[:1], *args, nbest=True)
        assert calls == [3, 1, 1, 1]
        assert len(rows) == len(want) and len(rows) >= 3 and [r[0] for r in rows] == sorted(r[0] for r in rows)
        assert bw > 1 or len(rows) == 3
        for r, w in list(zip(rows, want)) + list(zip(rows, first)):
            assert r[0] == w[0] and r[2:] == w[2:], (r, w)
            assert isinstance(r[1], float) and abs(r[1] - w[1]) < 1e-4, (r, w)
        assert len(first) >= 1
        plain = dec.test(model, batch, *args)      # the four-column rows: every utterance's best hypothesis
        assert [p[0] for p in plain] == ids and all(p[1] == next(r[2] for r in rows if r[0] == p[0]) for p in plain)
    path = tmp_path / "nbest.tsv"
    dec.save_results(rows, str(path), nbest=True)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["utt_id", "score_asr", "token_id", "text", "reftext"] and len(lines) == 1 + len(rows)
