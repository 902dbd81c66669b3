"""The batched CTC prefix beam search on the device (csrc/ctc_beam.hip) against the host search (csrc/ctc_beam_host.hip) over
the same log-probabilities and top-k labels: the same hypotheses in the same order, scores within 1e-9 * max(1, |score|).

The bar: device and host exp / log are each good to a couple of ulp, a value passes at most three lse2 per frame, |score| <~ 12 T;
at T <= 48 that bounds the drift near 1e-11, and the bar leaves two orders over it.  Exact order is demanded because every case has
a smallest non-zero gap between adjacent totals above 1e-7 (tests/test_ctc_beam_batch_cpu.py checks that, and that the cases hold
the folds, re-formed prefixes and exact ties they are here for).  Largest difference seen on an MI355X: 0.0 -- every score of
every case came out bit-identical to the host's."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ctc_beam_ref as R
from tests.util import CONFIGS, LM_CFG, load_ctc_beam_golden

pytestmark = pytest.mark.gpu

_HOST = {}


def host_search(lp, top, W, lw):
    """emoasr_ctc_beam_new / _step / _scores over the rows -> (hyps, scores)"""
    from emoasr_amd import lib
    L = lib.load()
    L.emoasr_ctc_beam_new.restype = ctypes.c_void_p
    L.emoasr_ctc_beam_new.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 2
    L.emoasr_ctc_beam_free.argtypes = [ctypes.c_void_p]
    L.emoasr_ctc_beam_free.restype = None
    L.emoasr_ctc_beam_step.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    L.emoasr_ctc_beam_scores.argtypes = [ctypes.c_void_p] * 2
    h = L.emoasr_ctc_beam_new(W, R.BLANK, R.EOS, lw, 0.0)
    parent, tok = np.zeros(W, np.int32), np.zeros(W, np.int32)
    live = [(R.EOS,)]
    for t in range(lp.shape[0]):
        n = L.emoasr_ctc_beam_step(h, lp[t].ctypes.data, top[t].ctypes.data, top.shape[1], None, parent.ctypes.data,
                                   tok.ctypes.data)
        assert n > 0
        live = [live[parent[i]] + ((int(tok[i]),) if tok[i] >= 0 else ()) for i in range(n)]
    scores = np.zeros(len(live))
    assert L.emoasr_ctc_beam_scores(h, scores.ctypes.data) == len(live)
    L.emoasr_ctc_beam_free(h)
    return [list(p) for p in live], scores.tolist()


def host_of(case):
    """the host result of a case, computed once and shared"""
    if case not in _HOST:
        V, W, T, scale, lw, seed, tie = case
        lp, top = R.make_rows(seed, T, V, scale, W, tie)
        _HOST[case] = (lp, top) + host_search(lp, top, W, lw)
    return _HOST[case]


def device_search(dev, utts, W, lw, V):
    """one launch over the utterances [(lp, top)] -> [(hyps, scores)] and the raw out_n"""
    from emoasr_amd import ops
    k = min(W, V)
    lens = [lp.shape[0] for lp, _ in utts]
    lp = torch.from_numpy(np.concatenate([u[0].reshape(-1, V) for u in utts])).to(dev)
    top = torch.from_numpy(np.concatenate([u[1].reshape(-1, k) for u in utts])).to(dev)
    row_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(dev)
    out_tok, out_len, out_score, out_n, status = ops.ctc_beam_batch(lp, row_off, top, W, R.BLANK, R.EOS, lw)
    assert int(status.item()) == 0
    tok, ln, sc, n = out_tok.cpu().numpy(), out_len.cpu().numpy(), out_score.cpu().numpy(), out_n.cpu().numpy()
    assert tok.shape == (len(utts), W, max(lens) + 1)
    return [([tok[b, i, :ln[b, i]].tolist() for i in range(n[b])], sc[b, :n[b]].tolist()) for b in range(len(utts))], n


def check_against_host(dev, case):
    V, W, T, scale, lw, seed, tie = case
    lp, top, want_h, want_s = host_of(case)
    (got_h, got_s), = device_search(dev, [(lp, top)], W, lw, V)[0]
    worst = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(got_s, want_s)) if len(got_s) == len(want_s) else None
    print(f"V={V} W={W} T={T} seed={seed}: {len(got_h)} hypotheses, largest score difference {worst}")
    assert got_h == want_h
    for a, b in zip(got_s, want_s):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (a, b)
    return got_h


_ID = lambda c: "V%d-W%d-T%d-s%d" % (c[0], c[1], c[2], c[5])


@pytest.mark.parametrize("case", R.expand(R.FOLD_CASES), ids=_ID)
def test_folds_and_the_reformed_prefix(dev, case):
    """random 5- and 6-label rows: folds of both kinds in the hundreds, a prefix that drops out and comes back while its child is
    live on every seed, <eos> as an ordinary column; W > V makes k = V, so the blank is always among the top-k"""
    check_against_host(dev, case)


@pytest.mark.parametrize("case", R.expand(R.LEN_CASES), ids=_ID)
def test_length_bonus(dev, case):
    check_against_host(dev, case)


@pytest.mark.parametrize("case", R.expand(R.TIE_CASES), ids=_ID)
def test_stable_order_under_exact_ties(dev, case):
    """column 3 equals column 1 before the soft-max: dozens of exact ties per seed between prefixes that went through identical
    operations, so a disagreement is the tie-break and not rounding"""
    check_against_host(dev, case)


@pytest.mark.parametrize("case", R.expand(R.SIZE_CASES), ids=_ID)
def test_sizes(dev, case):
    V, W = case[0], case[1]
    hyps = check_against_host(dev, case)
    assert len(hyps) == (5 if V == 5 else W)         # V = 5, one frame: out_n < W


def test_a_beam_over_the_limit_is_an_error(dev):
    from emoasr_amd import lib, ops
    lp, top = R.make_rows(0, 4, 40, 3.0, 33)
    d_lp, d_top = torch.from_numpy(lp).to(dev), torch.from_numpy(top).to(dev)
    row_off = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.ctc_beam_batch(d_lp, row_off, d_top, 33, R.BLANK, R.EOS, 0.0)
    out = torch.zeros(33 * 5 + 33 * 4 + 1, dtype=torch.int32, device=dev)
    ws = torch.zeros(4096, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for W in (33, 0):
        with pytest.raises(lib.EmoasrHipError):
            lib.call("emoasr_ctc_beam_batch", 1, 40, W, min(max(W, 1), 40), p(d_lp), 40, p(row_off), p(d_top), R.BLANK, R.EOS, 0.0, 4,
                     p(out), p(out), p(ws), p(out), p(ws), 8 * ws.numel(), p(status), None)
    torch.cuda.synchronize()
    assert int(out.abs().sum().item()) == 0 and int(status.item()) == 0


def test_ragged_batch(dev):
    """utterances of 0, 1, 7, 32 and 33 frames in one launch: each gets exactly what it gets alone -- device alone against device
    batched is bit-equal, scores included -- and what the host search gives; the empty one is the single prefix (<eos>), 0.0"""
    V, W, lw = 5, 3, 0.0
    lp, top = R.make_rows(19, 33, V, 1.0, W)
    utts = [(lp[:n], top[:n]) for n in (0, 1, 7, 32, 33)]
    batched, n = device_search(dev, utts, W, lw, V)
    assert batched[0] == ([[R.EOS]], [0.0]) and n.tolist() == [1, 3, 3, 3, 3]
    for u, got in zip(utts, batched):
        (alone,), _ = device_search(dev, [u], W, lw, V)
        assert got == alone                                  # (lists of ints and of doubles: bit-equal)
        want_h, want_s = host_search(u[0], u[1], W, lw)
        assert got[0] == want_h
        assert all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(got[1], want_s))


def _guarded(dev, n, dtype, fill):
    """n elements between two guard zones of 64"""
    buf = torch.full((n + 128,), fill, dtype=dtype, device=dev)
    return buf, buf[64:64 + n]


def test_bounds(dev):
    """a label >= V in the top-k of the second of three utterances: that utterance is refused (out_n = -1, status bit 0), the other
    two are as in the clean run, and nothing is written outside the outputs; a frame count over max_frames and a short workspace
    are refused the same way (bits 2 and 3)"""
    from emoasr_amd import lib
    V, W, lw, T = 6, 8, 0.0, 32
    k = min(W, V)
    rows = [R.make_rows(s, T, V, 1.0, W) for s in (8, 49, 58)]
    clean, _ = device_search(dev, rows, W, lw, V)
    lp = torch.from_numpy(np.concatenate([r[0] for r in rows])).to(dev)
    top_h = np.concatenate([r[1] for r in rows])
    bad = top_h.copy()
    bad[T + 11, 2] = V
    row_off = torch.tensor([0, T, 2 * T, 3 * T], dtype=torch.int32, device=dev)
    ws_bytes = lib.size_query("emoasr_ctc_beam_batch_ws_bytes", 3, 3 * T, W)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def launch(top_np, max_frames, ws_given):
        g_tok, tok = _guarded(dev, 3 * W * (max_frames + 1), torch.int32, -7)
        g_len, ln = _guarded(dev, 3 * W, torch.int32, -7)
        g_sc, sc = _guarded(dev, 3 * W, torch.float64, -7.0)
        g_n, n = _guarded(dev, 3, torch.int32, -7)
        g_ws, ws = _guarded(dev, ws_bytes // 8, torch.int64, -7)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        top = torch.from_numpy(top_np).to(dev)
        lib.call("emoasr_ctc_beam_batch", 3, V, W, k, p(lp), V, p(row_off), p(top), R.BLANK, R.EOS, lw, max_frames, p(tok), p(ln),
                 p(sc), p(n), p(ws), ws_given, p(status), None)
        torch.cuda.synchronize()
        for g in (g_tok, g_len, g_sc, g_n, g_ws):
            assert bool((g[:64] == -7).all()) and bool((g[-64:] == -7).all())
        tok, ln = tok.view(3, W, max_frames + 1).cpu().numpy(), ln.view(3, W).cpu().numpy()
        return tok, ln, sc.view(3, W).cpu().numpy(), n.cpu().numpy(), int(status.item())

    tok, ln, sc, n, status = launch(bad, T, ws_bytes)
    assert status == 1 and n.tolist() == [W, -1, W]
    assert bool((tok[1] == -7).all()) and bool((ln[1] == -7).all()) and bool((sc[1] == -7.0).all())
    for b in (0, 2):
        assert [tok[b, i, :ln[b, i]].tolist() for i in range(W)] == clean[b][0] and sc[b].tolist() == clean[b][1]
    tok, ln, sc, n, status = launch(top_h, T - 1, ws_bytes)
    assert status == 4 and n.tolist() == [-1, -1, -1] and bool((tok == -7).all())
    tok, ln, sc, n, status = launch(top_h, T, ws_bytes - 32)
    assert status == 8 and n.tolist() == [W, W, -1]
    assert [tok[0, i, :ln[0, i]].tolist() for i in range(W)] == clean[0][0]


# ---- module level, on the ctcbeam_tiny fixture -----------------------------------------------------------------------------
def _build(dev):
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    cfg, sd, lmsd, g2, gb = load_ctc_beam_golden()
    model = ASR(SimpleNamespace(**CONFIGS["l2_tiny"]), compute_dtype=torch.float32)
    model.load_state_dict(sd)
    lm = LM(SimpleNamespace(**LM_CFG), compute_dtype=torch.float32)
    lm.load_state_dict(lmsd)
    return model.to(dev).eval(), lm.to(dev).eval(), g2


def _same(got, want):
    assert got[0] == want[0], (got[0], want[0])
    np.testing.assert_allclose(got[1], want[1], rtol=1e-3, atol=1e-3)


def test_decode_of_a_batch_equals_each_utterance_alone(dev, monkeypatch):
    """model.decode on the fixture's whole batch against each utterance alone through the default host path: hypotheses equal in
    order, scores within 1e-3 (the bar of tests/test_ctc_beam_gpu.py for this fixture).  The utterance alone is decoded from ITS
    rows of the batch's encoder output: padding leaks through the convolution layers when utterances are batched (see
    tests/test_model_gpu.py::test_decode_driver_and_rtf), so a shorter utterance encoded alone is another input to the search,
    not another search (measured on this fixture: decoded alone and trimmed, utterances 1-3 give other hypotheses, with scores
    0.23-0.82 away from their rows of the batch; utterance 0 gives the same hypotheses and bit-identical scores).  Utterance 0
    is the longest and has no padding: it is also compared with model.decode of it alone."""
    from emoasr_amd import lib
    model, lm, g2 = _build(dev)
    xs, xlens = g2["xs"].to(dev), g2["xlens"]
    B = xs.shape[0]
    assert B > 1 and model.decoder.ctc_beam_impl == "host"
    calls = {"step": 0, "batch": 0}
    handle = lib.load()
    step = handle.emoasr_ctc_beam_step
    step.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3      # (the search sets them on the wrapper)

    def counting_step(*a):
        calls["step"] += 1
        return step(*a)

    real_call = lib.call

    def counting_call(name, *a):
        calls["batch"] += name == "emoasr_ctc_beam_batch"
        return real_call(name, *a)

    monkeypatch.setattr(handle, "emoasr_ctc_beam_step", counting_step)
    monkeypatch.setattr(lib, "call", counting_call)
    with torch.no_grad():
        eouts, elens, _ = model.encoder(xs, xlens)
    for lw in (0.0, 0.1):
        calls.update(step=0, batch=0)
        hyps, scores, logits, aligns = model.decode(xs, xlens, beam_width=4, len_weight=lw)
        assert calls == {"step": 0, "batch": 1} and aligns is None and len(hyps) == len(scores) == len(logits) == B
        for b in range(B):
            n = int(elens[b])
            assert logits[b].shape == (1, n, model.decoder.vocab_size)
            calls.update(step=0, batch=0)
            want = model.decoder.decode(eouts[b:b + 1, :n], [n], None, 4, lw)
            assert calls == {"step": n, "batch": 0}      # one utterance, "host": still emoasr_ctc_beam_step, once per frame
            _same((hyps[b], scores[b]), want)
            # one utterance through the device search meets the host at the same bar
            model.decoder.ctc_beam_impl = "device"
            got = model.decoder.decode(eouts[b:b + 1, :n], [n], None, 4, lw)
            model.decoder.ctc_beam_impl = "host"
            assert calls == {"step": n, "batch": 1} and got[2].shape == want[2].shape
            _same(got, want)
        n0 = int(xlens[0])
        assert n0 == xs.shape[1]
        _same((hyps[0], scores[0]), model.decode(xs[0:1, :n0], xlens[0:1], beam_width=4, len_weight=lw))
    with pytest.raises(NotImplementedError):
        model.decode(xs, xlens, beam_width=4, len_weight=0.1, lm=lm, lm_weight=0.3)
    with pytest.raises(NotImplementedError):
        model.decode(xs, xlens, beam_width=4, decode_phone=True)


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_driver_takes_batches_of_several_utterances(dev):
    """decode.test with a two-utterances-per-batch loader gives the rows of the batch-of-one loader, n-best and 1-best: token ids
    and texts equal, score_asr within 1e-3.  The batch-of-one loader hands each utterance over with the padding it has in its pair
    (see above) and decodes its valid frames on the device; the longer utterance of a pair has no padding and is also compared
    with the default host path."""
    from emoasr_amd import decode as dec
    model, _, g2 = _build(dev)
    xs, xlens = g2["xs"], g2["xlens"]
    B = xs.shape[0]
    assert B == 4
    ids = [f"utt{b}" for b in range(B)]
    pairs, ones, unpadded = [], [], []
    for a in range(0, B, 2):
        T = int(xlens[a:a + 2].max())
        pairs.append({"utt_ids": ids[a:a + 2], "texts": [f"ref{a}", f"ref{a + 1}"], "xs": xs[a:a + 2, :T], "xlens": xlens[a:a + 2]})
        for b in (a, a + 1):
            ones.append({"utt_ids": [ids[b]], "texts": [f"ref{b}"], "xs": xs[b:b + 1, :T], "xlens": xlens[b:b + 1]})
            if int(xlens[b]) == T:
                unpadded.append(b)
    vocab = _Vocab()
    for nbest in (True, False):
        args = (vocab, 4, 0.1, 0.0, False, None, 0.0, dev)
        got = dec.test(model, pairs, *args, nbest=nbest)
        model.decoder.ctc_beam_impl = "device"
        want = dec.test(model, ones, *args, nbest=nbest)
        model.decoder.ctc_beam_impl = "host"
        host = dec.test(model, [ones[b] for b in unpadded], *args, nbest=nbest)
        assert [r[0] for r in got] == [i for i in ids for _ in range(4 if nbest else 1)]
        for rows_got, rows_want in ((got, want), ([r for r in got if int(r[0][3:]) in unpadded], host)):
            assert len(rows_got) == len(rows_want) > 0
            for r, w in zip(rows_got, rows_want):
                if nbest:
                    assert [r[0]] + r[2:] == [w[0]] + w[2:] and abs(r[1] - w[1]) < 1e-3
                else:
                    assert r == w
    # greedy decoding takes the same loaders
    assert dec.test(model, pairs, vocab, 1, 0.0, 0.0, False, None, 0.0, dev) == dec.test(model, ones, vocab, 1, 0.0, 0.0, False, None,
                                                                                       0.0, dev)
    # num_samples counts utterances, whatever the batching
    assert [r[0] for r in dec.test(model, pairs, vocab, 4, 0.1, 0.0, False, None, 0.0, dev, num_samples=3)] == ids[:3]
