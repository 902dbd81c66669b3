"""Shallow fusion with the RNN LM in the two beam searches against the reference's outputs (tests/golden/rnnlm_tiny.npz: the
reference's CTC prefix search on the ctcbeam_tiny model and its joint CTC / attention search on l3_tiny, both with the rnnlm_tiny
LM): same hypotheses in the same order, scores within 1e-3.  The LM's state is threaded through slot pools, one step per new
prefix / per output step -- never a re-run of the prefix."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state
from tests.util import CONFIGS, CTC_BEAM_SETTINGS, DECODE_SETTINGS, LM_CFG, load_ctc_beam_golden, load_golden, lm_state, split_ragged

pytestmark = pytest.mark.gpu
CTC_CASES = [(si, b) for si in range(1, len(CTC_BEAM_SETTINGS)) for b in (1, 2, 3)]
JOINT_SETTINGS = [si for si, st in enumerate(DECODE_SETTINGS) if st["lm_weight"] > 0]


def _rnnlm(dtype, dev):
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=dtype)
    lm.load_state_dict(rnnlm_state(rnnlm_golden()))
    return lm.to(dev).eval()


def _ctc_model(dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, _, g2, _ = load_ctc_beam_golden()
    model = ASR(SimpleNamespace(**CONFIGS["l2_tiny"]), compute_dtype=dtype)
    model.load_state_dict(sd)
    return model.to(dev).eval(), g2


def _l3_model(dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, g = load_golden("l3_tiny")
    model = ASR(SimpleNamespace(**CONFIGS["l3_tiny"]), compute_dtype=dtype)
    model.load_state_dict(sd)
    return model.to(dev).eval(), g


def _utt(g, b, dev):
    n = int(g["xlens"][b])
    return g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1]


def test_ctc_beam_search_f32(dev, monkeypatch):
    """the golden's hypotheses and scores; the native bookkeeping against the Python loop (bit-identical float64 scores); the
    reference's literal state threading (EMOASR_CTC_LM_CACHE=0); the step kernel against the chain form"""
    g = rnnlm_golden()
    model, g2 = _ctc_model(torch.float32, dev)
    lm = _rnnlm(torch.float32, dev)
    for si, b in CTC_CASES:
        st = CTC_BEAM_SETTINGS[si]
        x, xl = _utt(g2, b, dev)
        want = split_ragged(g[f"ctc/{si}/{b}/hyps"], g[f"ctc/{si}/{b}/lens"])
        monkeypatch.setenv("EMOASR_CTC_BEAM_NATIVE", "1")
        lm.step_kernel = True
        hyps, scores, _, aligns = model.decode(x, xl, lm=lm, **st)
        assert aligns is None and lm.last_step == "kernel"
        assert hyps == want, (si, b, hyps, want)
        np.testing.assert_allclose(scores, g[f"ctc/{si}/{b}/scores"].numpy(), rtol=1e-3, atol=1e-3)
        lm.step_kernel = False
        hyps_c, scores_c, _, _ = model.decode(x, xl, lm=lm, **st)
        assert lm.last_step == "chain" and hyps_c == want, (si, b)
        np.testing.assert_allclose(scores_c, g[f"ctc/{si}/{b}/scores"].numpy(), rtol=1e-3, atol=1e-3)
        lm.step_kernel = True
        monkeypatch.setenv("EMOASR_CTC_BEAM_NATIVE", "0")
        hyps_p, scores_p, _, _ = model.decode(x, xl, lm=lm, **st)
        assert hyps_p == hyps and list(scores_p) == list(scores), (si, b, scores_p, scores)
        monkeypatch.setenv("EMOASR_CTC_LM_CACHE", "0")
        hyps_l, scores_l, _, _ = model.decode(x, xl, lm=lm, **st)
        monkeypatch.delenv("EMOASR_CTC_LM_CACHE")
        assert hyps_l == want, (si, b)
        np.testing.assert_allclose(scores_l, g[f"ctc/{si}/{b}/scores"].numpy(), rtol=1e-3, atol=1e-3)


def test_joint_beam_search_f32(dev):
    g = rnnlm_golden()
    model, g3 = _l3_model(torch.float32, dev)
    lm = _rnnlm(torch.float32, dev)
    for si in JOINT_SETTINGS:
        for b in range(2):
            x, xl = _utt(g3, b, dev)
            want = split_ragged(g[f"joint/{si}/{b}/hyps"], g[f"joint/{si}/{b}/lens"])
            for kernel in (True, False):
                lm.step_kernel = kernel
                hyps, scores, _, _ = model.decode(x, xl, lm=lm, **DECODE_SETTINGS[si])
                assert lm.last_step == ("kernel" if kernel else "chain")
                assert hyps == want, (si, b, kernel, hyps, want)
                np.testing.assert_allclose(scores, g[f"joint/{si}/{b}/scores"].numpy(), rtol=1e-3, atol=1e-3)


def test_bf16_runs(dev):
    """throughput mode: same code paths end to end; finite, sorted, well-formed (as test_ctc_beam_search_bf16_runs checks)"""
    lm = _rnnlm(torch.bfloat16, dev)
    model, g2 = _ctc_model(torch.bfloat16, dev)
    x, xl = _utt(g2, 3, dev)
    hyps, scores, _, _ = model.decode(x, xl, beam_width=4, len_weight=0.1, lm=lm, lm_weight=0.3)
    assert lm.last_step == "kernel"
    assert len(hyps) == 4 and hyps[0][0] == 2 and all(0 < v < 40 for v in hyps[0])
    assert scores == sorted(scores, reverse=True) and all(np.isfinite(scores))
    model, g3 = _l3_model(torch.bfloat16, dev)
    x, xl = _utt(g3, 0, dev)
    hyps, scores, _, _ = model.decode(x, xl, lm=lm, **DECODE_SETTINGS[2])
    assert len(hyps) >= 1 and all(0 < v < 40 for h in hyps for v in h)
    assert scores == sorted(scores, reverse=True) and all(np.isfinite(scores))


def test_dispatch_of_the_joint_search(dev, monkeypatch):
    """a Transformer LM still takes the device-resident joint search; the stateful RNN LM the host bookkeeping"""
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling.lm import LM
    model, g3 = _l3_model(torch.float32, dev)
    tlm = LM(SimpleNamespace(**LM_CFG), compute_dtype=torch.float32)
    tlm.load_state_dict(lm_state(g3))
    tlm = tlm.to(dev).eval()
    calls = []
    orig = bsd.joint_beam_search_device
    monkeypatch.setattr(bsd, "joint_beam_search_device", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    x, xl = _utt(g3, 0, dev)
    assert tlm.stateful is False
    hyps, _, _, _ = model.decode(x, xl, lm=tlm, **DECODE_SETTINGS[2])
    assert len(calls) == 1 and hyps == split_ragged(g3["decode/2/0/hyps"], g3["decode/2/0/lens"])
    model.decode(x, xl, lm=_rnnlm(torch.float32, dev), **DECODE_SETTINGS[2])
    assert len(calls) == 1, "a stateful LM must not take the device-resident search"
