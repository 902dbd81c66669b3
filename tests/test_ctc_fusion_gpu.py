"""The batched fused CTC search at module level (ctc_prefix_beam_search_batch_lm, CTCDecoder.decode with ctc_beam_impl = "device",
emoasr_amd.fusion_grid) on the ctcbeam_tiny model with the rnnlm_tiny LM and with the Transformer LM of tests/util.LM_CFG, f32.

The comparison of a batch with the host search is the one tests/test_ctc_beam_batch_gpu.py explains: the host search is run over
each utterance's OWN ROWS of the batch's encoder output, so both searches see the same log-probabilities.  They also see the same LM
rows bit for bit when an LM row does not depend on where in a call (and in how large a call) it is computed; the first test checks
that for the RNN LM's step kernel, which the fused search calls with up to 32 rows per launch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state
from tests.util import CONFIGS, CTC_BEAM_SETTINGS, LM_CFG, load_ctc_beam_golden, split_ragged

pytestmark = pytest.mark.gpu

LM_SETTINGS = [si for si, st in enumerate(CTC_BEAM_SETTINGS) if st["lm_weight"] > 0]


def _build(dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    cfg, sd, lmsd, g2, gb = load_ctc_beam_golden()
    model = ASR(SimpleNamespace(**CONFIGS["l2_tiny"]), compute_dtype=dtype)
    model.load_state_dict(sd)
    tlm = LM(SimpleNamespace(**LM_CFG), compute_dtype=dtype)
    tlm.load_state_dict(lmsd)
    rlm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=dtype)
    rlm.load_state_dict(rnnlm_state(rnnlm_golden()))
    return model.to(dev).eval(), {"rnn": rlm.to(dev).eval(), "transformer": tlm.to(dev).eval()}, g2, gb


def test_an_lm_step_does_not_depend_on_its_place_in_the_call(dev):
    """one step of a row alone, the same row at another position of a 32-row call, and in a call of 33 rows (two chunks): bit-equal
    log-probability rows and states"""
    from emoasr_amd import ops
    _, lms, _, _ = _build(torch.float32, dev)
    lm = lms["rnn"]
    pools = lm.new_pools(128)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    lm.step(pools, 2, i32([2, 7]), i32([-1, -1]), i32([0, 1]), row_dst=i32([0, 1]))       # two parent states: after (<eos>) and (7)
    assert lm.last_step == "kernel" and ops.RNNLM_STEP_MAX == 32
    r = np.random.RandomState(3)

    def call(n, at, base):
        ids, src = r.randint(3, 40, n).tolist(), r.randint(-1, 2, n).tolist()
        ids[at], src[at] = 11, 1
        dst = list(range(base, base + n))
        lm.step(pools, n, i32(ids), i32(src), i32(dst), row_dst=i32(dst))
        return base + at

    rows = [call(1, 0, 2), call(32, 17, 3), call(33, 32, 40), call(33, 5, 80)]
    torch.cuda.synchronize()
    for a in rows[1:]:
        d_row = (pools.logp[a] - pools.logp[rows[0]]).abs().max().item()
        d_h = (pools.ph[:, a].float() - pools.ph[:, rows[0]].float()).abs().max().item()
        d_c = (pools.pc[:, a] - pools.pc[:, rows[0]]).abs().max().item()
        print(f"row {a} against the row alone: log-probabilities {d_row} h {d_h} c {d_c}")
        assert torch.equal(pools.logp[a], pools.logp[rows[0]]) and torch.equal(pools.ph[:, a], pools.ph[:, rows[0]])
        assert torch.equal(pools.pc[:, a], pools.pc[:, rows[0]])


def test_single_utterances_give_the_golden_hypotheses(dev):
    """ctc_beam_impl = "device", one utterance at a time: the reference's hypotheses exactly, scores within 1e-3 (the bars and cases
    of tests/test_rnnlm_beam_gpu.py::test_ctc_beam_search_f32 and tests/test_ctc_beam_gpu.py)"""
    model, lms, g2, gb = _build(torch.float32, dev)
    gr = rnnlm_golden()
    model.decoder.ctc_beam_impl = "device"
    for si in LM_SETTINGS:
        st = CTC_BEAM_SETTINGS[si]
        for b in (1, 2, 3):
            n = int(g2["xlens"][b])
            x, xl = g2["xs"][b:b + 1, :n].to(dev), g2["xlens"][b:b + 1]
            for kind, want_h, want_s in (("rnn", split_ragged(gr[f"ctc/{si}/{b}/hyps"], gr[f"ctc/{si}/{b}/lens"]), gr[f"ctc/{si}/{b}/scores"]),
                                         ("transformer", split_ragged(gb[f"decode/{si}/{b}/hyps"], gb[f"decode/{si}/{b}/lens"]),
                                          gb[f"decode/{si}/{b}/scores"])):
                hyps, scores, logits, aligns = model.decode(x, xl, lm=lms[kind], **st)
                assert aligns is None and logits.shape[0] == 1 and logits.shape[2] == model.decoder.vocab_size
                assert hyps == want_h, (kind, si, b, hyps, want_h)
                np.testing.assert_allclose(scores, want_s.numpy(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("kind", ["rnn", "transformer"])
def test_a_batch_equals_the_host_search_over_its_rows(dev, kind):
    """all golden utterances in one call against the host ctc_prefix_beam_search over each utterance's own rows of the batch's
    encoder output: the same hypotheses, scores within 1e-9 * max(1, |score|)"""
    model, lms, g2, _ = _build(torch.float32, dev)
    lm = lms[kind]
    xs, xlens = g2["xs"].to(dev), g2["xlens"]
    B = xs.shape[0]
    assert B > 1
    with torch.no_grad():
        eouts, elens, _ = model.encoder(xs, xlens)
    for si in LM_SETTINGS:
        st = CTC_BEAM_SETTINGS[si]
        model.decoder.ctc_beam_impl = "device"
        hyps, scores, logits, aligns = model.decoder.decode(eouts, elens, None, st["beam_width"], st["len_weight"], lm, st["lm_weight"])
        model.decoder.ctc_beam_impl = "host"
        assert aligns is None and len(hyps) == len(scores) == len(logits) == B
        for b in range(B):
            n = int(elens[b])
            assert logits[b].shape == (1, n, model.decoder.vocab_size)
            want_h, want_s, _, _ = model.decoder.decode(eouts[b:b + 1, :n], [n], None, st["beam_width"], st["len_weight"], lm,
                                                        st["lm_weight"])
            worst = max(abs(a - w) / max(1.0, abs(w)) for a, w in zip(scores[b], want_s))
            print(f"{kind} setting {si} utterance {b}: largest score difference {worst}")
            assert hyps[b] == want_h, (si, b, hyps[b], want_h)
            for a, w in zip(scores[b], want_s):
                assert abs(a - w) <= 1e-9 * max(1.0, abs(w)), (si, b, a, w)


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_fusion_grid_equals_one_decode_per_cell(dev, monkeypatch):
    """the 2 x 2 grid lm_weight in {0, 0.3} x len_weight in {0, 0.5} over a two-batch loader: every cell's 1-best texts and WER
    counts are those of decode.test with that cell's weights alone, and the head ran once per batch, not once per cell"""
    from emoasr_amd import decode as dec
    from emoasr_amd import fusion_grid as fg
    from emoasr_amd.metrics import compute_wers, wer_summary
    from emoasr_amd.modeling.functions import _engine_of
    model, lms, g2, _ = _build(torch.float32, dev)
    lm = lms["rnn"]
    xs, xlens = g2["xs"], g2["xlens"]
    assert xs.shape[0] == 4
    refs = ["w5 w9 w11 w3", "w7 w7 w12", "w4 w30 w8 w21 w6", "w9"]
    loader = []
    for a in (0, 2):
        T = int(xlens[a:a + 2].max())
        loader.append({"utt_ids": [f"utt{a}", f"utt{a + 1}"], "texts": refs[a:a + 2], "xs": xs[a:a + 2, :T], "xlens": xlens[a:a + 2]})
    eng = _engine_of(model.decoder)
    calls = []
    real = eng.head_logits
    monkeypatch.setattr(eng, "head_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    lm_w, len_w = [0.0, 0.3], [0.0, 0.5]
    texts = []
    results, best = fg.ctc_fusion_grid(model, loader, _Vocab(), 4, lm, lm_w, len_w, dev, texts_out=texts)
    assert len(calls) == len(loader)
    assert [(r[0], r[1]) for r in results] == [(0.0, 0.0), (0.0, 0.5), (0.3, 0.0), (0.3, 0.5)] and len(texts) == 4
    model.decoder.ctc_beam_impl = "device"
    want_best = (0, 0, 100, "")
    for c, (a, b, wer, info) in enumerate(results):
        rows = dec.test(model, loader, _Vocab(), 4, b, 0.0, False, lm, a, dev)
        assert [r[0] for r in rows] == ["utt0", "utt1", "utt2", "utt3"]
        assert [r[2] for r in rows] == texts[c], (a, b)
        w_wer, w_dict = compute_wers([r[2].split() for r in rows], [r[3].split() for r in rows])
        assert info == wer_summary(w_wer, w_dict) and abs(wer - w_wer) < 1e-9, (a, b, info)
        if w_wer < want_best[2]:
            want_best = (a, b, w_wer, info)
    assert tuple(best) == want_best
    with pytest.raises(NotImplementedError, match="CTC models only"):
        fg.ctc_fusion_grid(model, loader, _Vocab(), 4, lm, lm_w, len_w, dev, decode_ctc_weight=0.3)


def test_bf16_runs(dev):
    """throughput mode: the same code path end to end; W finite, sorted scores per utterance"""
    model, lms, g2, _ = _build(torch.bfloat16, dev)
    model.decoder.ctc_beam_impl = "device"
    xs, xlens = g2["xs"].to(dev), g2["xlens"]
    for kind in ("rnn", "transformer"):
        hyps, scores, _, _ = model.decode(xs, xlens, beam_width=4, len_weight=0.1, lm=lms[kind], lm_weight=0.3)
        assert len(hyps) == len(scores) == xs.shape[0]
        for h, s in zip(hyps, scores):
            assert len(h) == len(s) == 4 and all(np.isfinite(s)) and s == sorted(s, reverse=True)
            assert all(p[0] == 2 and all(0 <= v < 40 for v in p) for p in h)
