"""The batched transducer greedy search in lockstep (csrc/rnnt_greedy_batch.hip, engine.rnnt_greedy_batch,
decoder.rnnt_greedy_impl = "batch"): the book kernel alone against tests/rnnt_greedy_ref.Lockstep step by step, the search end to end
on the l4_tiny golden model against the reference's hypotheses and alignments and against the per-utterance form, every dtype
against a host loop that issues the same launches and keeps the books in Python, and the public interface."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnnt_greedy_ref as G
from tests.util import CONFIGS, load_golden, split_ragged

pytestmark = pytest.mark.gpu


def _build(dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, g = load_golden("l4_tiny")
    model = ASR(SimpleNamespace(**CONFIGS["l4_tiny"]), compute_dtype=dtype)
    model.load_state_dict(sd)
    return model.to(dev).eval(), g


def _encode_alone(model, g, dev):
    """every utterance encoded alone, stacked and padded (tests/test_rnnt_beam_device_gpu.py)"""
    outs = []
    with torch.no_grad():
        for b in range(g["xs"].shape[0]):
            n = int(g["xlens"][b])
            eouts, elens, _ = model.encoder(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1])
            outs.append(eouts[0, :int(elens[0])])
    elens = [int(e.shape[0]) for e in outs]
    eouts = torch.zeros(len(outs), max(elens), outs[0].shape[1], device=dev, dtype=outs[0].dtype)
    for b, e in enumerate(outs):
        eouts[b, :elens[b]] = e
    return eouts, elens


# ---- 1. the book kernel alone ---------------------------------------------------------------------------------------------------------
TS = (0, 1, 5, 12)


def _book_steps(dev, K, V, blank, dtype, rows, max_seq_len):
    """start, then one book call per step on logits made by rows(search, label sequence, frame); before every call the control
    words and the live counter equal the reference's; inactive rows hold a row whose arg-max is a label, so reading one shows"""
    from emoasr_amd import ops
    S = len(TS)
    want_h, want_a, steps = G.search(G.argmax_scorer(rows), TS, K, blank, G.EOS, max_seq_len)
    offs = np.concatenate([[0], np.cumsum(TS)]).astype(np.int32)
    row_off = torch.tensor(offs, device=dev)
    ctl, state, hyp, align, lens, live = ops.rnnt_greedy_batch_buffers(S, K, max_seq_len, max(TS), dev)
    ops.rnnt_greedy_batch_start(row_off, K, G.EOS, max_seq_len, ctl, state, lens, live)
    L = G.Lockstep(TS, K, blank, G.EOS, max_seq_len)
    decoy = np.full(V, -5.0, dtype=np.float32)
    decoy[(blank + 1) % V] = 5.0
    for n, step in enumerate(steps):
        assert np.array_equal(ctl.cpu().numpy(), step["ctl"]), (n, ctl.tolist(), step["ctl"].tolist())
        assert int(live.item()) == step["live"] == L.live, (n, int(live.item()), step["live"])
        if step["live"] == 0:
            break
        host = np.tile(decoy, (S * K, 1))
        for s in range(S):
            for i, (_, on, t) in enumerate(step["joint"][s]):
                if on:
                    host[s * K + i] = rows(s, tuple([G.EOS] + L.hyps[s]), t)
        logits = torch.from_numpy(host).to(dev).to(dtype)
        assert torch.equal(logits.float().cpu(), torch.from_numpy(host))          # the values are exact in the compute dtype
        ops.rnnt_greedy_batch_book(row_off, K, blank, max_seq_len, logits, ctl, state, hyp, align, lens, live)
        L.advance(lambda s, i: int(np.argmax(host[s * K + i])))
    assert n == len(steps) - 1 and (L.hyps, L.aligns) == (want_h, want_a)
    got_l = lens.tolist()
    assert got_l == [[len(h), len(a)] for h, a in zip(want_h, want_a)]
    assert [hyp[s, :got_l[s][0]].tolist() for s in range(S)] == want_h
    assert [align[s, :got_l[s][1]].tolist() for s in range(S)] == want_a
    assert want_h[0] == [] and want_a[0] == [] and int(live.item()) == 0
    # after the end two more book calls change nothing
    before = [x.clone() for x in (ctl, state, hyp, align, lens, live)]
    for _ in range(2):
        ops.rnnt_greedy_batch_book(row_off, K, blank, max_seq_len, logits, ctl, state, hyp, align, lens, live)
    assert all(torch.equal(a, b) for a, b in zip(before, (ctl, state, hyp, align, lens, live)))
    return want_h, want_a


@pytest.mark.parametrize("blank", [0, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16-ties"])
@pytest.mark.parametrize("V", [9, 70, 1030])
@pytest.mark.parametrize("K", [1, 3, 4])
def test_book_kernel_step_by_step(dev, K, V, dtype, blank):
    """Ts = (0, 1, 5, 12): a search without frames, K > T, a window that crosses an utterance's end; V below a wave, not a multiple
    of 64, several loads per lane.  bf16: the rows lie on the integers -3 .. 3, so the maximum is tied many times over and the
    lowest index must win -- with blank = 3 a tie between blank and a lower label is an emission, one with a higher label is not"""
    tie = dtype == torch.bfloat16
    hyps, aligns = _book_steps(dev, K, V, blank, dtype, G.hash_rows(17 * V + K, V, blank, tie=tie), 256)
    assert all(len(a) >= T for a, T in zip(aligns, TS)) and any(hyps)
    if tie:
        assert any(tok < blank for h in hyps for tok in h) or blank == 0


@pytest.mark.parametrize("K", [1, 3, 4])
def test_book_kernel_cuts_after_max_seq_len(dev, K):
    """a scorer that never emits blank, max_seq_len = 2: three labels on frame 0, then the search is finished"""
    hyps, aligns = _book_steps(dev, K, 70, 0, torch.float32, G.hash_rows(5, 70, 0, never_blank=True), 2)
    assert [len(h) for h in hyps] == [0, 3, 3, 3] and aligns == hyps


# ---- 2. end to end, f32 ---------------------------------------------------------------------------------------------------------------
def _oracle_alone(g):
    """the oracle's greedy search of every utterance encoded alone (CPU)"""
    from oracle import model as om
    from oracle import rnnt as orn
    cfg, sd, _ = load_golden("l4_tiny")
    hyps, aligns = [], []
    with torch.no_grad():
        for b in range(g["xs"].shape[0]):
            n = int(g["xlens"][b])
            eouts, elens = om.encoder_forward(sd, cfg, g["xs"][b:b + 1, :n], g["xlens"][b:b + 1])
            h, a = orn.rnnt_greedy(sd, cfg, eouts, elens)
            hyps += h
            aligns += a
    return hyps, aligns


def test_batch_f32_returns_the_golden_search(dev):
    """The golden eval/hyps and eval/aligns were recorded on the encoder outputs of the PADDED batch (the encoder's output depends
    on padding: encoded alone, two of the four utterances end in one more label -- in the oracle too), so they are asked for on
    those, as tests/test_l4_gpu.py does; on the utterances encoded alone and stacked, the search must return the oracle's search
    of the same utterances encoded alone.  On either, it equals decoder._greedy under "utterance"."""
    model, g = _build(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    assert dec.rnnt_greedy_impl == "utterance"
    golden = (split_ragged(g["eval/hyps"], g["eval/hyp_lens"]), split_ragged(g["eval/aligns"], g["eval/align_lens"]))
    with torch.no_grad():
        e_b, l_b, _ = model.encoder(g["xs"].to(dev), g["xlens"])
    l_b = [int(n) for n in l_b]
    e_a, l_a = _encode_alone(model, g, dev)
    assert l_a == l_b and len(l_a) > 1 and len(set(l_a)) > 1
    alone = _oracle_alone(g)
    assert alone != golden and all(len(h) > 0 for h in golden[0] + alone[0])   # every utterance emits labels: more steps than max(elens)
    with torch.no_grad():
        for eouts, elens, (want_h, want_a) in ((e_b, l_b, golden), (e_a, l_a, alone)):
            h_u, _, _, a_u = dec._greedy(eouts, elens)
            for K in (1, 4):
                hyps, aligns = eng.rnnt_greedy_batch(eouts, elens, dec.blank_id, dec.eos_id, dec.max_seq_len, frames_per_step=K,
                                                     poll_block=2)
                stats = dict(eng.rnnt_greedy_batch_stats)
                print(f"K={K}: {stats}")
                assert hyps == want_h and aligns == want_a, (K, hyps, want_h)
                assert hyps == h_u and aligns == a_u
                # the polling loop ran past its first block, and within the bound
                assert stats["polls"] >= 2
                assert -(-max(elens) // K) < stats["steps"] <= stats["bound"] == max(elens) + dec.max_seq_len + 1
        eouts, elens, (want_h, want_a) = e_a, l_a, alone
        # an utterance without frames in the middle of the batch: [] and [], its neighbours unchanged
        e0 = torch.cat([eouts[:1], torch.zeros_like(eouts[:1]), eouts[1:]])
        hyps, aligns = eng.rnnt_greedy_batch(e0, elens[:1] + [0] + elens[1:], dec.blank_id, dec.eos_id, dec.max_seq_len)
        assert hyps == want_h[:1] + [[]] + want_h[1:] and aligns == want_a[:1] + [[]] + want_a[1:]
        # chunks: a cap of two searches per launch chain gives the same lists
        eng._GREEDY_BATCH_ROWS = 2 * eng._GREEDY_BATCH_K
        try:
            assert eng.rnnt_greedy_batch(eouts, elens, dec.blank_id, dec.eos_id, dec.max_seq_len) == (want_h, want_a)
        finally:
            del eng._GREEDY_BATCH_ROWS


# ---- 3. every dtype -------------------------------------------------------------------------------------------------------------------
def _host_lockstep(eng, eouts, elens, K, blank, eos, max_seq_len):
    """the search with the SAME launches on the same S K rows each step (st.launches: LSTM rows, joint rows, output product) and the
    bookkeeping in Python: the arg-max of every row comes back to the host, tests/rnnt_greedy_ref.Lockstep writes the next words"""
    from emoasr_amd import ops
    offs = np.concatenate([[0], np.cumsum(elens)])
    with eng._scope(), torch.no_grad():
        st = eng._rnnt_greedy_batch_load(eouts, elens, K, blank, eos, max_seq_len)
        L = G.Lockstep(elens, K, blank, eos, max_seq_len)
        assert np.array_equal(st.ctl.cpu().numpy(), L.ctl(offs))
        while L.live:
            st.ctl.copy_(torch.from_numpy(L.ctl(offs)))
            am = ops.argmax_rows(st.launches()).tolist()
            L.advance(lambda s, i: am[s * K + i])
    return L.hyps, L.aligns


@pytest.mark.parametrize("dtype,mfma", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1)], ids=["f32-valu", "bf16-valu", "bf16-mfma"])
def test_batch_equals_the_host_loop(dev, dtype, mfma):
    """token for token, no tolerance: the two differ only in where the integer logic runs.  Against the per-utterance form (another
    summation order: a near-tie may flip) the token agreement is printed and held to the 0.8 of
    tests/test_l4_gpu.py::test_greedy_on_the_device_equals_the_launch_chain"""
    from emoasr_amd import lib
    model, g = _build(dtype, dev)
    eouts, elens = _encode_alone(model, g, dev)
    eng, dec = model.engine(), model.decoder
    with lib.options(rnnt_beam_mfma=mfma), torch.no_grad():
        for K in (1, 4):
            got = eng.rnnt_greedy_batch(eouts, elens, dec.blank_id, dec.eos_id, dec.max_seq_len, frames_per_step=K)
            want = _host_lockstep(eng, eouts, elens, K, dec.blank_id, dec.eos_id, dec.max_seq_len)
            assert got == want, (K, got, want)
        h_u, _, _, _ = dec._greedy(eouts, elens)
    agree = sum(int(a == b) for h1, h0 in zip(got[0], h_u) for a, b in zip(h1, h0)) / max(1, sum(len(h) for h in h_u))
    print(f"{dtype} mfma={mfma}: token agreement with the per-utterance form {agree:.3f}")
    assert agree > 0.8, (agree, got[0], h_u)


# ---- 4. the interface -----------------------------------------------------------------------------------------------------------------
class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_interface(dev, monkeypatch):
    from emoasr_amd import decode as D
    from emoasr_amd.modeling.asr import ASR
    model, g = _build(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    xs, xlens = g["xs"], g["xlens"]
    B = xs.shape[0]
    loader = []
    for a in range(0, B, 3):
        T = int(xlens[a:a + 3].max())
        loader.append({"utt_ids": [f"utt{b}" for b in range(a, min(a + 3, B))], "texts": [f"ref{b}" for b in range(a, min(a + 3, B))],
                       "xs": xs[a:a + 3, :T], "xlens": xlens[a:a + 3]})
    args = (_Vocab(), 1, 0.0, 0.0, False, None, 0.0, dev)

    # the default: "utterance", and the cooperative launch per utterance is still what runs
    assert dec.rnnt_greedy_impl == "utterance" and "rnnt_greedy_impl" not in dec.state_dict()
    ran = []
    device_form, batch_form = eng._rnnt_greedy_device, eng.rnnt_greedy_batch
    monkeypatch.setattr(eng, "_rnnt_greedy_device", lambda *a, **k: ran.append("device") or device_form(*a, **k))
    monkeypatch.setattr(eng, "rnnt_greedy_batch", lambda *a, **k: ran.append("batch") or batch_form(*a, **k))
    rows_u = D.test(model, loader, *args)
    plain_u = model.decode(xs[:3, :int(xlens[:3].max())].to(dev), xlens[:3])
    assert ran and set(ran) == {"device"}
    del ran[:]

    dec.rnnt_greedy_impl = "batch"
    rows_b = D.test(model, loader, *args)
    plain_b = model.decode(xs[:3, :int(xlens[:3].max())].to(dev), xlens[:3])
    assert ran and set(ran) == {"batch"}
    assert rows_b == rows_u and len(rows_b) == B and plain_b == plain_u and plain_b[1:] == (None, None, None)
    n0 = int(xlens[0])
    one = model.decode(xs[:1, :n0].to(dev), xlens[:1])                      # B = 1
    dec.rnnt_greedy_impl = "utterance"
    assert one == model.decode(xs[:1, :n0].to(dev), xlens[:1]) and len(one[0]) == 1
    with torch.no_grad():
        eouts, elens, _ = model.encoder(xs[:2, :int(xlens[:2].max())].to(dev), xlens[:2])
        g_u = dec._greedy(eouts, elens)
        dec.rnnt_greedy_impl = "batch"
        assert dec._greedy(eouts, elens) == g_u and g_u[3] is not None

    # refusals: an unknown value; a model the form cannot take (asked for by name: no quiet detour, no kernel error)
    dec.rnnt_greedy_impl = "lockstep"
    with pytest.raises(ValueError, match="rnnt_greedy_impl"):
        model.decode(xs[:1, :n0].to(dev), xlens[:1])
    dec.rnnt_greedy_impl = "batch"
    monkeypatch.setattr(eng, "rnnt_greedy_batch_why_not", lambda: "the sizes do not fit")
    loaded = []
    monkeypatch.setattr(eng, "_rnnt_greedy_batch_load", lambda *a, **k: loaded.append(a))
    del ran[:]
    with pytest.raises(ValueError, match="the sizes do not fit"):
        model.decode(xs[:1, :n0].to(dev), xlens[:1])
    assert ran == ["batch"] and loaded == []          # refused by the engine before any launch, and no detour to the utterance form
    wide = ASR(SimpleNamespace(**dict(CONFIGS["l4_tiny"], dec_hidden_size=1032)), compute_dtype=torch.float32).to(dev).eval()
    why = wide.engine().rnnt_greedy_batch_why_not()
    assert why is not None and "1032" in why and eng.__class__.rnnt_greedy_batch_why_not(eng) is None
    wide.decoder.rnnt_greedy_impl = "batch"
    with pytest.raises(ValueError, match="1032"):
        wide.decode(xs[:1, :n0].to(dev), xlens[:1])
