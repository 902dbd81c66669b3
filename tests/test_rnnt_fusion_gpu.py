"""RNN-LM shallow fusion in the transducer beam search on the device (csrc/rnnt_beam_lm.hip, engine.rnnt_beam_search_batch with an LM,
RNNTDecoder.decode, fusion_grid.rnnt_fusion_grid): the fused pick kernel alone against an f64 reference and,
at mu = 0, bit for bit against emoasr_rnnt_beam_pick; the gather kernel; and the search end to end on the l4_tiny golden model with
the rnnlm_tiny LM against the host-bookkeeping form."""
from types import SimpleNamespace

import pytest
import torch

from tests import rnnt_fusion_ref as F
from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state
from tests.util import CONFIGS, LM_CFG, load_ctc_beam_golden, load_golden

pytestmark = pytest.mark.gpu

VS = (5, 64, 65, 257, 1000, 1025)          # both kernel forms (<= 1024: registers), the lane and the 64-column edges
R_ROWS, W_ROWS = 37, 4                     # 37 rows of 10 searches (the last one partial)
OFF = (0, 3, 4, 15, 16, 21, 30, 33, 36)    # the inactive rows


def _inputs(V, V_lm, dtype, dev, grid=False):
    g = torch.Generator().manual_seed(1000 * V + V_lm)
    x, y = torch.randn(R_ROWS, V, generator=g) * 3.0, torch.randn(R_ROWS, V_lm, generator=g) * 2.0
    if grid:      # a 0.5 grid, and every candidate column c of the first half has a twin c + half with the same two logits
        x, y = torch.round(x * 2) / 2, torch.round(y * 2) / 2
        half = (V - 1) // 2
        x[:, 1 + half:1 + 2 * half] = x[:, 1:1 + half]
        y[:, 1 + half:1 + 2 * half] = y[:, 1:1 + half]
    act = torch.ones(R_ROWS, dtype=torch.int64)
    act[list(OFF)] = 0
    mu = torch.tensor([(0.0, 0.3, 1.0)[s % 3] for s in range((R_ROWS + W_ROWS - 1) // W_ROWS)], dtype=torch.float32)
    return x.to(dev, dtype), y.to(dev, dtype), mu.to(dev), act.to(dev)


def _f64(x, y, mu):
    """-> (lp, f) in doubles from the (already rounded) inputs; column 0 of f is no candidate"""
    lp, lq = torch.log_softmax(x.double(), -1), torch.log_softmax(y.double(), -1)
    f = lp + mu.double().repeat_interleave(W_ROWS)[:x.shape[0], None] * lq[:, :x.shape[1]]
    f[:, 0] = float("-inf")
    return lp, f


def _distance(out, k, lp, f, blank):
    """largest distance of a record's values from the doubles at the columns it names"""
    idx = out[:, 1 + k:1 + 2 * k].long() + 1
    d = (out[:, 1:1 + k].double() - f.gather(1, idx)).abs().max()
    return max(float(d), float((out[:, 0].double() - lp[:, blank]).abs().max()))


_PICK_ERR = {}


def _pick_error(dtype, dev):
    """emoasr_rnnt_beam_pick's largest distance from the f64 reference over the rows of this file, per dtype"""
    from emoasr_amd import ops
    if dtype not in _PICK_ERR:
        worst = 0.0
        for V in VS:
            x, _, mu, _ = _inputs(V, V, dtype, dev)
            k = min(16, V - 1)
            out = ops.rnnt_beam_pick(x, k, 0, torch.zeros(R_ROWS, 1 + 2 * k, device=dev))
            lp = torch.log_softmax(x.double(), -1)
            f = lp.clone()
            f[:, 0] = float("-inf")
            worst = max(worst, _distance(out, k, lp, f, 0))
        _PICK_ERR[dtype] = worst
    return _PICK_ERR[dtype]


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pick_lm_against_f64_and_the_unfused_pick(dev, dtype, V):
    """values within twice emoasr_rnnt_beam_pick's own largest distance from the f64 reference (one margin for the second
    soft-max, one for the multiply-add), indices equal the f64 order wherever its gaps exceed that tolerance, inactive rows
    untouched, and with mu = 0 the records of emoasr_rnnt_beam_pick bit for bit"""
    from emoasr_amd import ops
    e_pick = _pick_error(dtype, dev)
    tol = 2.0 * e_pick
    worst = 0.0
    for V_lm in (V, V + 3):
        x, y, mu, act = _inputs(V, V_lm, dtype, dev)
        on = act.bool()
        lp, f = _f64(x, y, mu)
        for k in (k for k in (1, 4, 16) if k < V):
            blank = 0 if k != 4 else V - 1
            out = torch.full((R_ROWS, 3 + 2 * k), 7.0, device=dev)
            ops.rnnt_beam_pick_lm(x, y, mu, W_ROWS, k, blank, out, act)
            assert bool((out[~on] == 7.0).all()) and bool((out[:, 1 + 2 * k:] == 7.0).all())
            got = out[on]
            worst = max(worst, _distance(got, k, lp[on], f[on], blank))
            top, order = torch.sort(f[on], dim=1, descending=True, stable=True)
            idx = got[:, 1 + k:1 + 2 * k].long() + 1
            gap_up = torch.cat([torch.full_like(top[:, :1], float("inf")), top[:, :k - 1] - top[:, 1:k]], 1)
            gap_down = top[:, :k] - top[:, 1:k + 1]          # (column 0 sorts last at -inf: there is always a next one)
            clear = (gap_up > tol) & (gap_down > tol)
            assert bool((idx[clear] == order[:, :k][clear]).all()), (V, V_lm, k)
            assert int(clear.sum()) >= clear.numel() // 2          # (the comparison is not empty)
            # mu = 0 through the fused kernel: the unfused record, bit for bit
            zero = torch.full((R_ROWS, 1 + 2 * k), 7.0, device=dev)
            ops.rnnt_beam_pick_lm(x, y, torch.zeros_like(mu), W_ROWS, k, blank, zero, act)
            plain = ops.rnnt_beam_pick(x, k, blank, torch.zeros(R_ROWS, 1 + 2 * k, device=dev))
            assert torch.equal(zero[on], plain[on]), (V, V_lm, k)
    print(f"V={V} {dtype}: pick {e_pick:.3g} (all rows of the file), pick_lm {worst:.3g}, allowed {tol:.3g}")
    assert worst <= tol, (worst, tol)


@pytest.mark.parametrize("V,k", [(65, 64), (1025, 40)], ids=["registers", "lds"])
def test_pick_lm_exact_ties_go_to_the_lowest_index(dev, V, k):
    """0.5-grid logits in which candidate column c and its twin c + (V - 1) / 2 hold the same two values: their fused values are
    the same floats, the record's values never rise, equal neighbours come in ascending column order, a twin never precedes its
    lower column"""
    from emoasr_amd import ops
    x, y, mu, act = _inputs(V, V + 3, torch.float32, dev, grid=True)
    out = torch.zeros(R_ROWS, 1 + 2 * k, device=dev)
    ops.rnnt_beam_pick_lm(x, y, mu, W_ROWS, k, 0, out, None)
    vals, idx = out[:, 1:1 + k].cpu(), out[:, 1 + k:].long().cpu() + 1
    half = (V - 1) // 2
    assert bool((vals[:, :-1] >= vals[:, 1:]).all())
    same = vals[:, :-1] == vals[:, 1:]
    assert int(same.sum()) >= R_ROWS * (k // 4) and bool((idx[:, :-1][same] < idx[:, 1:][same]).all())
    for r in range(R_ROWS):
        seen = set()
        for c in idx[r].tolist():
            assert 1 <= c < V and c not in seen and (c <= half or c - half in seen), (r, c)
            seen.add(c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gather_rows(dev, dtype):
    from emoasr_amd import ops
    torch.manual_seed(3)
    pool = torch.randn(50, 72, device=dev).to(dtype)
    dst = torch.randint(0, 50, (R_ROWS,), device=dev)
    dst[5], dst[6], dst[7] = -1, 50, 1 << 40
    act = torch.ones(R_ROWS, dtype=torch.int64, device=dev)
    act[list(OFF)] = 0
    out = ops.rnnt_beam_gather_rows(pool, dst, act, torch.full((R_ROWS, 72), 7.0, device=dev, dtype=dtype))
    live = act.bool() & (dst >= 0) & (dst < 50)
    assert int(live.sum()) == R_ROWS - len(OFF) - 3
    assert torch.equal(out[live], pool[dst[live]]) and bool((out[~live] == 0).all())
    assert torch.equal(ops.rnnt_beam_gather_rows(pool, dst.clamp(0, 49)), pool[dst.clamp(0, 49)])


# ---- the search end to end ---------------------------------------------------------------------------------------------------------
ELENS = (12, 5, 0)
MUS = (0.3, 1.0)
_MODELS = {}


def _models(dtype, dev):
    """(model, rnn lm, transformer lm, eouts [3, 12, d], oracle state) -- built once per dtype"""
    if dtype not in _MODELS:
        from emoasr_amd.modeling.asr import ASR
        from emoasr_amd.modeling.lm import LM
        cfg, sd, g = load_golden("l4_tiny")
        model = ASR(SimpleNamespace(**CONFIGS["l4_tiny"]), compute_dtype=dtype)
        model.load_state_dict(sd)
        model = model.to(dev).eval()
        rlm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=dtype)
        rlm.load_state_dict(rnnlm_state(rnnlm_golden()))
        tlm = LM(SimpleNamespace(**LM_CFG), compute_dtype=dtype)
        tlm.load_state_dict(load_ctc_beam_golden()[2])
        outs = []
        with torch.no_grad():
            for b in range(3):
                n = int(g["xlens"][b])
                e, el, _ = model.encoder(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1])
                assert int(el[0]) >= ELENS[b]
                outs.append(e[0, :ELENS[0]])
        _MODELS[dtype] = (model, rlm.to(dev).eval(), tlm.to(dev).eval(), torch.stack(outs), (cfg, sd))
    return _MODELS[dtype]


_REF = {}


def _gap_checked(dev):
    """[(b, W, mu)] of the end-to-end cases whose host restatement (oracle network, f32, over the f32 model's encoder outputs)
    keeps every cut further apart than GAP_TOL; at most 10 % may be left out"""
    if "cases" not in _REF:
        _, _, _, eouts, (cfg, sd) = _models(torch.float32, dev)
        lm_sd = {k: v.float() for k, v in rnnlm_state(rnnlm_golden()).items()}
        cases, every = [], 0
        with torch.no_grad():
            for b in (0, 1):
                sc, lm = F.oracle_scorers(sd, cfg, lm_sd, eouts[b:b + 1, :ELENS[b]].float().cpu())
                for W in (2, 4):
                    for mu in MUS:
                        every += 1
                        if F.search(sc, lm, mu, ELENS[b], W)[2].min_gap > F.GAP_TOL:
                            cases.append((b, W, mu))
        assert len(cases) >= every - every // 10, cases
        _REF["cases"] = cases
    return _REF["cases"]


def _host(eng, dec, lm, eouts, b, W, mu, lw=0.0):
    return eng._rnnt_beam_search_chain(eouts[b:b + 1, :ELENS[b]], W, dec.blank_id, dec.eos_id, 3, True, lm, mu, lw)


def _close(a, b, tol=1e-4):
    return len(a) == len(b) and all(abs(p - q) < tol for p, q in zip(a, b))


def test_device_search_equals_the_host_form_f32(dev):
    """hypotheses and order equal, scores within 1e-4 (the bar between two forms of the search, section 20) on the gap-checked
    cases; utterance b in the batch returns the doubles it returns alone; fusion really changes results"""
    model, lm, _, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    moved = 0
    with torch.no_grad():
        for W in (2, 4):
            plain, _, _, _ = dec.decode(eouts, list(ELENS), beam_width=W)
            for mu in MUS:
                hyps, scores, logits, aligns = dec.decode(eouts, list(ELENS), beam_width=W, lm=lm, lm_weight=mu, len_weight=0.7)
                assert logits is None and aligns is None and hyps[2] == [[dec.eos_id]] and scores[2] == [0.7]
                for b in (0, 1):
                    moved += int(hyps[b] != plain[b])
                    if (b, W, mu) in _gap_checked(dev):
                        h, s = _host(eng, dec, lm, eouts, b, W, mu, 0.7)
                        assert hyps[b] == h and _close(scores[b], s), (b, W, mu, hyps[b], h, scores[b], s)
                    dec.rnnt_beam_impl = "device"
                    try:
                        h1, s1, _, _ = dec.decode(eouts[b:b + 1, :ELENS[b]], [ELENS[b]], beam_width=W, lm=lm, lm_weight=mu, len_weight=0.7)
                    finally:
                        dec.rnnt_beam_impl = "host"
                    assert h1 == hyps[b] and s1 == scores[b], (b, W, mu)
                    # one utterance on the default "host" implementation: the host form, no scores
                    h2 = dec.decode(eouts[b:b + 1, :ELENS[b]], [ELENS[b]], beam_width=W, lm=lm, lm_weight=mu, len_weight=0.7)
                    assert h2 == (_host(eng, dec, lm, eouts, b, W, mu, 0.7)[0], None, None, None)
    assert moved >= 2


def test_mu_zero_through_the_fused_chain_is_the_unfused_search(dev):
    """the LM's launches run, weighted 0: hypotheses and doubles of the search without the LM, bit for bit"""
    model, lm, _, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    with torch.no_grad():
        for W in (2, 4):
            want = eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id)
            got = eng._rnnt_beam_search_device(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, 3, lm, [0.0] * 3)
            assert got[0] == want[0] and got[1] == want[1]
            # weights <= 0 in a grid call are the search without the LM, and do not read the length weight
            grid = eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, lm=lm, lm_weights=[0.0, -1.0], len_weights=[2.0])
            assert [h[0] for h in grid[0]] == want[0] == [h[1] for h in grid[0]] and [s[0] for s in grid[1]] == want[1]


def test_grid_call_equals_single_cell_calls(dev):
    """a 3 x 2 grid (one weight <= 0) against six decode calls of one cell each: hypotheses and doubles"""
    model, lm, _, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    lm_weights, len_weights = [0.0, 0.3, 1.0], [0.0, 1.5]
    with torch.no_grad():
        hyps, scores = eng.rnnt_beam_search_batch(eouts, list(ELENS), 4, dec.blank_id, dec.eos_id, lm=lm, lm_weights=lm_weights,
                                                  len_weights=len_weights)
        c = 0
        for a in lm_weights:
            for w in len_weights:
                h1, s1, _, _ = dec.decode(eouts, list(ELENS), beam_width=4, lm=lm, lm_weight=a, len_weight=w)
                assert [h[c] for h in hyps] == h1 and [s[c] for s in scores] == s1, (a, w)
                c += 1
    assert len(hyps[0]) == 6


def test_bf16_agrees_with_f32_on_the_best_hypothesis(dev):
    model, lm, _, eouts, _ = _models(torch.bfloat16, dev)
    m32, lm32, _, e32, _ = _models(torch.float32, dev)
    with torch.no_grad():
        for W in (2, 4):
            for mu in MUS:
                got = model.decoder.decode(eouts, list(ELENS), beam_width=W, lm=lm, lm_weight=mu)[0]
                want = m32.decoder.decode(e32, list(ELENS), beam_width=W, lm=lm32, lm_weight=mu)[0]
                for b in (0, 1):
                    if (b, W, mu) in _gap_checked(dev):
                        assert got[b][0] == want[b][0], (b, W, mu, got[b], want[b])


def test_transformer_lm_takes_the_host_form(dev):
    model, _, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    with torch.no_grad():
        assert eng.rnnt_beam_lm_why_not(tlm) is not None and not eng.rnnt_beam_device_ok(4, lm=tlm)
        hyps, scores, _, _ = dec.decode(eouts, list(ELENS), beam_width=4, lm=tlm, lm_weight=0.5, len_weight=0.2)
        for b in (0, 1):
            h, s = _host(eng, dec, tlm, eouts, b, 4, 0.5, 0.2)
            assert hyps[b] == h and scores[b] == [float(v) for v in s]
        assert hyps[2] == [[dec.eos_id]] and scores[2] == [0.2]


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_fused_nbest_tsv_and_grid_driver(dev, tmp_path):
    """decode.test(nbest=True) with an LM on batches of two writes the five-column TSV of the FUSED N-best lists, and
    rnnt_fusion_grid's cells hold the decode calls' best hypotheses"""
    from emoasr_amd import decode as dc
    from emoasr_amd import fusion_grid as fg
    model, lm, _, _, _ = _models(torch.float32, dev)
    g = load_golden("l4_tiny")[2]
    xs, xlens = g["xs"], g["xlens"]
    ids = [f"utt{b}" for b in range(4)]
    pairs = []
    for a in (0, 2):
        T = int(xlens[a:a + 2].max())
        pairs.append({"utt_ids": ids[a:a + 2], "texts": [f"w12 w{a}", "w35"], "xs": xs[a:a + 2, :T], "xlens": xlens[a:a + 2]})
    rows = dc.test(model, pairs, _Vocab(), 4, 0.5, 0.0, False, lm, 1.0, dev, nbest=True)
    plain = dc.test(model, pairs, _Vocab(), 4, 0.0, 0.0, False, None, 0.0, dev, nbest=True)
    assert {r[0] for r in rows} == set(ids) and all(isinstance(r[1], float) for r in rows)
    assert [r[1:3] for r in rows] != [r[1:3] for r in plain]
    for utt in ids:
        mine = [r for r in rows if r[0] == utt]
        assert 1 <= len(mine) <= 4 and all(p[1] >= q[1] for p, q in zip(mine, mine[1:]))
    path = tmp_path / "nbest.tsv"
    dc.save_results(rows, str(path), nbest=True)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["utt_id", "score_asr", "token_id", "text", "reftext"] and len(lines) == 1 + len(rows)
    assert all(len(line.split("\t")) == 5 for line in lines)
    texts = []
    results, best = fg.grid_of("rnn_transducer")(model, pairs, _Vocab(), 4, lm, [0.0, 1.0], [0.0, 0.5], dev, texts_out=texts)
    assert [(r[0], r[1]) for r in results] == [(0.0, 0.0), (0.0, 0.5), (1.0, 0.0), (1.0, 0.5)]
    assert best in results or best == (0, 0, 100, "")          # (the rule for best starts from WER 100, as the reference's does)
    first = lambda rr: [next(r[3] for r in rr if r[0] == u) for u in ids]
    assert texts[3] == first(rows) and texts[0] == texts[1] == first(plain)


def test_refusals(dev):
    from emoasr_amd import lib, ops
    from emoasr_amd.modeling.lm import _NO_PREDICT
    x, y = torch.zeros(4, 9, device=dev), torch.zeros(4, 8, device=dev)
    mu, out = torch.zeros(1, device=dev), torch.zeros(4, 9, device=dev)
    with pytest.raises(lib.EmoasrHipError, match="smaller than the model's"):
        ops.rnnt_beam_pick_lm(x, y, mu, 4, 4, 0, out)                                   # V_lm < V
    with pytest.raises(lib.EmoasrHipError, match="bad arguments"):
        ops.rnnt_beam_pick_lm(x, x, mu, 4, 9, 0, torch.zeros(4, 19, device=dev))        # k >= V
    with pytest.raises(lib.EmoasrHipError, match="bad arguments"):
        ops.rnnt_beam_pick_lm(x, x, mu, 4, 4, 0, torch.zeros(4, 8, device=dev))         # ldo < 1 + 2 k
    model, lm, tlm, eouts, _ = _models(torch.float32, dev)
    dec = model.decoder
    dec.rnnt_beam_impl = "device"
    try:
        with pytest.raises(ValueError, match="lm_type 'transformer'"):
            dec.decode(eouts, list(ELENS), beam_width=4, lm=tlm, lm_weight=0.5)
        wide = SimpleNamespace(lm_type="rnn", compute_dtype=torch.float32, f32_split=False, L=2, H=4096, E=64, V=40)
        with pytest.raises(ValueError, match="cannot fuse this LM"):
            dec.decode(eouts, list(ELENS), beam_width=4, lm=wide, lm_weight=0.5)
        small = SimpleNamespace(lm_type="rnn", compute_dtype=torch.float32, f32_split=False, L=2, H=64, E=48, V=39)
        with pytest.raises(ValueError, match="vocabulary"):
            dec.decode(eouts, list(ELENS), beam_width=4, lm=small, lm_weight=0.5)
    finally:
        dec.rnnt_beam_impl = "host"
    with pytest.raises(NotImplementedError) as info:
        model.engine()._rnnt_beam_search_chain(eouts[:1], 4, dec.blank_id, dec.eos_id, 3, True, SimpleNamespace(lm_type="bert"), 0.5, 0)
    assert str(info.value) == _NO_PREDICT
