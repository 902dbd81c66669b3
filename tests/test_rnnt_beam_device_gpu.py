"""The batched transducer beam search with the bookkeeping on the device (csrc/rnnt_beam_book.hip, the rows forms of
csrc/rnnt_beam.hip, engine.rnnt_beam_search_batch, RNNTDecoder.decode): the bookkeeping kernel alone against
tests/rnnt_beam_ref.search_by_ids round by round, the rows kernels bit for bit against the 16-row entry points, and the search end
to end on the l4_tiny golden model against the reference's hypotheses and the host-bookkeeping forms."""
from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnnt_beam_ref as R
from tests.util import CONFIGS, RNNT_BEAM_WIDTHS, load_golden, load_rnnt_beam_golden

pytestmark = pytest.mark.gpu


def _build(dtype, dev):
    from emoasr_amd.modeling.asr import ASR
    cfg, sd, g = load_golden("l4_tiny")
    model = ASR(SimpleNamespace(**CONFIGS["l4_tiny"]), compute_dtype=dtype)
    model.load_state_dict(sd)
    return model.to(dev).eval(), g


def _encode_alone(model, g, dev):
    """every utterance encoded alone (as the golden was made: the encoder's output depends on padding), stacked and padded"""
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


# ---- 1. the bookkeeping kernel alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ts,W,V", [((0, 5, 12), 4, 9), ((6,), 16, 17)], ids=["S3-W4", "S1-W16"])
def test_book_kernel_round_by_round(dev, Ts, W, V):
    """the control words of every round, the final hypotheses, their order and (within 1e-9: the last bits of exp / log in double
    over at most a few thousand log-adds of values below 1e4) their scores equal search_by_ids; the records come from synthetic
    scorers, which learn each row's label sequence from a host map slot -> label sequence"""
    from emoasr_amd import lib, ops
    E, S = 3, len(Ts)
    scorers = [R.hash_scorer(100 + 7 * s + W, V, W) for s in range(S)]
    want = [R.search_by_ids(scorers[s], Ts[s], W, E) for s in range(S)]
    NS, Rr = (E + 1) * W, S * W
    offs = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int32)
    row_off = torch.tensor(offs, device=dev)
    ws = torch.empty(lib.size_query("emoasr_rnnt_beam_ws_bytes", S, int(offs[-1]), W, E), device=dev, dtype=torch.uint8)
    ctl = torch.zeros(5, Rr, device=dev, dtype=torch.int64)
    rec = torch.zeros(Rr, 1 + 2 * W, device=dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    ops.rnnt_beam_start(row_off, W, E, V, R.EOS, ctl, ws, status)
    seq_of = [{0: ()} for _ in range(S)]
    done_rounds = [0] * S
    for _ in range(max(Ts) * E):
        c = ctl.cpu().numpy()
        host = np.zeros((Rr, 1 + 2 * W), dtype=np.float32)
        for s in range(S):
            rows = [tuple(int(c[j, s * W + i]) for j in range(5)) for i in range(W)]
            if done_rounds[s] >= Ts[s] * E:
                assert all(r[3] == 0 for r in rows), (s, rows)
                continue
            rd = want[s][2][done_rounds[s]]
            local = [(r[0], r[1] - s * NS, r[2] - s * NS, r[3], r[4] - int(offs[s]) if r[3] else r[4]) for r in rows]
            assert local == rd["ctl"], (s, done_rounds[s], local, rd["ctl"])
            for i, (lab, src, dst, on, t) in enumerate(local):
                if on:
                    seq = seq_of[s][src] + (lab,)
                    seq_of[s][dst] = seq
                    blank, vals, ids = scorers[s](seq, t)
                    host[s * W + i, 0], host[s * W + i, 1:1 + W], host[s * W + i, 1 + W:] = blank, vals, ids
            done_rounds[s] += 1
        rec.copy_(torch.from_numpy(host))
        ops.rnnt_beam_book(row_off, W, E, V, R.EOS, rec, ctl, ws, status)
    assert int((ctl[3] != 0).sum()) == 0                       # every search is finished: no active row is left
    hyps, scores, n = ops.rnnt_beam_finish(row_off, W, E, V, R.EOS, max(Ts) * (E - 1), ws, status)
    for s in range(S):
        assert hyps[s] == want[s][0], (s, hyps[s], want[s][0])
        assert max(abs(a - b) for a, b in zip(scores[s], want[s][1])) <= 1e-9, (s, scores[s], want[s][1])
    assert hyps[0] == [[R.EOS]] or Ts[0] > 0


# ---- 2. the rows kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mfma", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1)], ids=["f32-valu", "bf16-valu", "bf16-mfma"])
def test_rows_kernels_equal_the_16_row_entry_points(dev, dtype, mfma):
    """37 rows (three tiles, the last one partial) with inactive rows scattered: every active row's new h, c and joint row is
    bit-identical to what emoasr_rnnt_beam_lstm / _joint write for it when called on the active rows of its tile, and nothing
    but the active rows' destination slots and joint rows moves"""
    from emoasr_amd import lib, ops
    with lib.options(rnnt_beam_mfma=mfma):
        torch.manual_seed(37)
        Rr, E, H, J, V, POOL, Tm = 37, 64, 96, 48, 200, 160, 7
        r = lambda *s, sc=1.0: (torch.randn(*s, device=dev) * sc).to(dtype)
        emb, w_ih, w_hh = r(V, E), r(4 * H, E, sc=E ** -0.5), r(4 * H, H, sc=H ** -0.5)
        bias = torch.randn(4 * H, device=dev) * 0.1
        ph, pc = r(POOL, H, sc=0.5), torch.randn(POOL, H, device=dev) * 0.5
        w_dec, b_dec, e_all = r(J, H, sc=H ** -0.5), torch.randn(J, device=dev) * 0.1, r(Tm, J)
        ids = torch.randint(0, V, (Rr,), device=dev)
        src = torch.randint(0, 60, (Rr,), device=dev)
        dst = 60 + torch.randperm(100, device=dev)[:Rr]
        act = torch.ones(Rr, dtype=torch.int64, device=dev)
        act[torch.tensor([0, 3, 4, 15, 16, 21, 30, 33, 36], device=dev)] = 0
        trow = torch.randint(0, Tm, (Rr,), device=dev)
        ptr = lambda tt: c_void_p(tt.data_ptr())
        ph_r, pc_r = ph.clone(), pc.clone()
        hj_r = torch.full((Rr, J), 7.0, device=dev, dtype=dtype)
        lib.call("emoasr_rnnt_beam_lstm_rows", ops.dt(emb), Rr, E, H, ptr(emb), E, V, ptr(ids), ptr(w_ih), ptr(w_hh), ptr(bias),
                 ptr(ph_r), ptr(pc_r), POOL, ptr(src), ptr(dst), ptr(act), ops._stream())
        lib.call("emoasr_rnnt_beam_joint_rows", ops.dt(emb), Rr, H, J, Tm, ptr(ph_r), POOL, ptr(dst), ptr(act), ptr(w_dec),
                 ptr(b_dec), ptr(e_all), ptr(trow), ptr(hj_r), ops._stream())
        ph_w, pc_w = ph.clone(), pc.clone()
        hj_w = torch.full((Rr, J), 7.0, device=dev, dtype=dtype)
        for r0 in range(0, Rr, 16):
            rows = [i for i in range(r0, min(r0 + 16, Rr)) if int(act[i])]
            ix = torch.tensor(rows, device=dev)
            g_ids, g_src, g_dst = ids[ix].contiguous(), src[ix].contiguous(), dst[ix].contiguous()
            lib.call("emoasr_rnnt_beam_lstm", ops.dt(emb), len(rows), E, H, ptr(emb), E, ptr(g_ids), ptr(w_ih), ptr(w_hh), ptr(bias),
                     ptr(ph_w), ptr(pc_w), ptr(g_src), ptr(g_dst), None, None, 0, ops._stream())
            for t in sorted(set(trow[ix].tolist())):
                hj = torch.zeros(16, J, device=dev, dtype=dtype)
                tt = torch.tensor([t], device=dev)
                lib.call("emoasr_rnnt_beam_joint", ops.dt(emb), len(rows), H, J, Tm, ptr(ph_w), ptr(g_dst), ptr(w_dec), ptr(b_dec),
                         ptr(e_all), ptr(tt), ptr(hj), ops._stream())
                for k, i in enumerate(rows):
                    if int(trow[i]) == t:
                        hj_w[i] = hj[k]
        assert torch.equal(ph_r, ph_w) and torch.equal(pc_r, pc_w) and torch.equal(hj_r, hj_w)
        on = act.bool()
        keep = torch.ones(POOL, dtype=torch.bool, device=dev)
        keep[dst[on]] = False
        assert torch.equal(ph_r[keep], ph[keep]) and torch.equal(pc_r[keep], pc[keep])
        assert not torch.equal(ph_r[dst[on]], ph[dst[on]])
        assert bool((hj_r[~on].float() == 7.0).all()) and bool((hj_r[on].float().abs() <= 1.0).all())


# ---- 3. - 6. the search end to end ---------------------------------------------------------------------------------------------------
def test_batch_f32_returns_the_golden_hypotheses(dev):
    """model.decoder.decode on the stacked batch: the reference's hypotheses for widths 2 and 4, scores within 1e-4 of the graph
    form (the bar tests/test_l4_gpu.py sets between two forms of the round), and utterance b's result identical, hypotheses and
    doubles, to the same search of it alone"""
    model, g = _build(torch.float32, dev)
    want = load_rnnt_beam_golden()
    eouts, elens = _encode_alone(model, g, dev)
    assert len(elens) > 1 and len(set(elens)) > 1
    eng, dec = model.engine(), model.decoder
    with torch.no_grad():
        for bw in RNNT_BEAM_WIDTHS:
            hyps, scores, logits, aligns = dec.decode(eouts, elens, beam_width=bw)
            assert logits is None and aligns is None and len(hyps) == len(scores) == len(elens)
            for b, n in enumerate(elens):
                assert hyps[b] == want[bw][b], (b, bw, hyps[b], want[bw][b])
                h_g, s_g = eng._rnnt_beam_search_graph(eouts[b:b + 1, :n], bw, dec.blank_id, dec.eos_id, return_scores=True)
                assert h_g == hyps[b] and max(abs(a - c) for a, c in zip(scores[b], s_g)) < 1e-4, (b, bw, scores[b], s_g)
                assert dec.rnnt_beam_impl == "host"
                assert dec.decode(eouts[b:b + 1, :n], [n], beam_width=bw) == (want[bw][b], None, None, None)
                dec.rnnt_beam_impl = "device"
                try:
                    h1, s1, _, _ = dec.decode(eouts[b:b + 1, :n], [n], beam_width=bw)
                finally:
                    dec.rnnt_beam_impl = "host"
                assert h1 == hyps[b] and s1 == scores[b], (b, bw, s1, scores[b])
        # an utterance without frames
        hyps, scores, _, _ = dec.decode(eouts, [0] + elens[1:], beam_width=2)
        assert hyps[0] == [[dec.eos_id]] and scores[0] == [0.0] and hyps[1] == want[2][1]


def test_round_graph_with_the_unfused_body(dev, monkeypatch):
    """EMOASR_RNNT_BEAM_FUSED=0, set before a fresh model's engine builds its record: the replayed round captures the launch chain
    with explicit copies (also the fall-back when a fused kernel refuses in the warm-up) -- the reference's hypotheses for every
    golden utterance, scores within 1e-4 of the chain form's (the bar tests/test_l4_gpu.py sets between two forms of the round)"""
    monkeypatch.setenv("EMOASR_RNNT_BEAM_FUSED", "0")
    model, g = _build(torch.float32, dev)
    want = load_rnnt_beam_golden()
    eouts, elens = _encode_alone(model, g, dev)
    eng, dec = model.engine(), model.decoder
    assert getattr(eng, "_beam_static", None) is None
    with torch.no_grad():
        for bw in RNNT_BEAM_WIDTHS:
            for b, n in enumerate(elens):
                h_g, s_g = eng._rnnt_beam_search_graph(eouts[b:b + 1, :n], bw, dec.blank_id, dec.eos_id, return_scores=True)
                h_c, s_c = eng._rnnt_beam_search_chain(eouts[b:b + 1, :n], bw, dec.blank_id, dec.eos_id, return_scores=True)
                print(bw, b, max(abs(a - c) for a, c in zip(s_g, s_c)))
                assert h_g == want[bw][b] and h_c == h_g, (b, bw, h_g, want[bw][b])
                assert max(abs(a - c) for a, c in zip(s_g, s_c)) < 1e-4, (b, bw, s_g, s_c)
                assert eng._beam_static.zero_copy is False


def test_batch_bf16_agrees_with_the_graph_form(dev):
    """bf16 at width 4 against the graph form: token agreement above 0.9 (the bar of
    tests/test_l4_gpu.py::test_beam_search_bf16_fused_round_agrees_with_the_chain)"""
    model, g = _build(torch.bfloat16, dev)
    eouts, elens = _encode_alone(model, g, dev)
    eng, dec = model.engine(), model.decoder
    with torch.no_grad():
        hyps, scores, _, _ = dec.decode(eouts, elens, beam_width=4)
        ref = [eng._rnnt_beam_search_graph(eouts[b:b + 1, :n], 4, dec.blank_id, dec.eos_id)[0] for b, n in enumerate(elens)]
    got = [h[0] for h in hyps]
    same = sum(int(a == c) for ha, hc in zip(got, ref) for a, c in zip(ha, hc))
    tot = sum(max(len(ha), len(hc)) for ha, hc in zip(got, ref))
    assert same / max(tot, 1) > 0.9, (got, ref)
    assert all(isinstance(v, float) for s in scores for v in s)


def test_batch_outside_the_fused_round_limits(dev):
    """vocab_size = 16001 (tests/test_l4_gpu.py::test_beam_search_outside_the_fused_round_limits): two copies of the first
    utterance are answered utterance by utterance through the existing forms -- the chain form's hypotheses, scores within 1e-4"""
    from emoasr_amd.modeling.asr import ASR
    torch.manual_seed(5)
    m = ASR(SimpleNamespace(**dict(CONFIGS["l4_tiny"], vocab_size=16001)), compute_dtype=torch.float32).to(dev).eval()
    _, _, g = load_golden("l4_tiny")
    with torch.no_grad():
        n = int(g["xlens"][0])
        eouts, elens, _ = m.encoder(g["xs"][:1, :n].to(dev), g["xlens"][:1])
        T = int(elens[0])
        assert not m.engine().rnnt_beam_device_ok(3)
        h_c, s_c = m.engine()._rnnt_beam_search_chain(eouts[:, :T], 3, m.decoder.blank_id, m.decoder.eos_id, return_scores=True)
        hyps, scores, _, _ = m.decoder.decode(torch.cat([eouts, eouts]), [T, T], beam_width=3)
    for b in range(2):
        assert hyps[b] == h_c, (b, hyps[b], h_c)
        assert max(abs(a - c) for a, c in zip(scores[b], s_c)) < 1e-4, (scores[b], s_c)


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_nbest_rows_from_batches_of_two(dev, tmp_path):
    """decode.test(nbest=True) on a transducer model with a two-utterances-per-batch loader: one row per hypothesis, float scores
    that do not rise within an utterance, the first hypothesis equal to the plain decode, and the five-column TSV"""
    from emoasr_amd import decode as dec
    model, g = _build(torch.float32, dev)
    xs, xlens = g["xs"], g["xlens"]
    B = xs.shape[0] // 2 * 2
    ids = [f"utt{b}" for b in range(B)]
    pairs = []
    for a in range(0, B, 2):
        T = int(xlens[a:a + 2].max())
        pairs.append({"utt_ids": ids[a:a + 2], "texts": [f"ref{a}", f"ref{a + 1}"], "xs": xs[a:a + 2, :T], "xlens": xlens[a:a + 2]})
    args = (_Vocab(), 4, 0.0, 0.0, False, None, 0.0, dev)
    rows = dec.test(model, pairs, *args, nbest=True)
    plain = dec.test(model, pairs, *args, nbest=False)
    assert [r[0] for r in plain] == ids and len(rows) > len(ids)
    for utt, first in zip(ids, plain):
        mine = [r for r in rows if r[0] == utt]
        assert 1 <= len(mine) <= 4 and all(isinstance(r[1], float) for r in mine)
        assert all(a[1] >= b[1] for a, b in zip(mine, mine[1:])), mine
        assert mine[0][2:] == first[1:], (mine[0], first)
        assert len({r[2] for r in mine}) == len(mine)
    path = tmp_path / "nbest.tsv"
    dec.save_results(rows, str(path), nbest=True)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["utt_id", "score_asr", "token_id", "text", "reftext"] and len(lines) == 1 + len(rows)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, monkeypatch):
    from emoasr_amd import lib, ops
    from emoasr_amd.modeling.decoders.rnn_transducer import RNNTDecoder
    S, W, E, V, T = 1, 4, 3, 9, 5
    row_off = torch.tensor([0, T], device=dev, dtype=torch.int32)
    nbytes = lib.size_query("emoasr_rnnt_beam_ws_bytes", S, T, W, E)
    ws = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    ctl = torch.full((5, S * W), 9, device=dev, dtype=torch.int64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    ops.rnnt_beam_start(row_off, W, E, V, R.EOS, ctl, ws, status, ws_bytes=nbytes - 32)      # one node short
    assert int(status.item()) == 8 and int((ctl[3] != 0).sum()) == 0
    with pytest.raises(RuntimeError, match="workspace") as info:
        ops.rnnt_beam_finish(row_off, W, E, V, R.EOS, T * (E - 1), ws, status, ws_bytes=nbytes - 32)
    assert info.value.out_n == [-1]
    status.zero_()
    ops.rnnt_beam_start(row_off, W, E, V, R.EOS, ctl, ws, status)                            # the full size is taken
    assert int(status.item()) == 0 and ctl[3].tolist() == [1, 0, 0, 0]

    dec = RNNTDecoder(SimpleNamespace(**CONFIGS["l4_tiny"]))
    dec.rnnt_beam_impl = "device"
    calls = []
    monkeypatch.setattr(lib, "call", lambda name, *a: calls.append(name))
    with pytest.raises(ValueError, match="beam_width"):
        dec.decode(torch.zeros(1, 3, 8, device=dev), [3], beam_width=17)
    assert calls == []
