"""The CTC error-correction kernels (csrc/correct.hip) against float64 restatements (tests/correct_ref.py).

  ctc_token_conf   frame and ntok exact, conf within 1e-6 relative (f32 logits; the reference is float64 from the logits alone, so the
                   bar also holds the rounding of the log-sum-exp input to f32: at most 2^-22 absolute for lse < 8, 2.4e-7 relative on
                   the probability) / 1e-5 (bf16 logits, float64 on the same rounded inputs).  Every run's best frame is at least 1e-4
                   (relative) ahead of its second-best in float64 -- asserted, so no token is left out -- except where a tie is
                   planted by copying a whole frame row: there the earliest frame must win.
  correct_fuse     ids exact, the winning value within 1e-6 relative.  Every row's float64 top-2 margin is at least 1e-6 absolute
                   (asserted); planted ties (two columns equal in both inputs) go to the lowest column.
  end to end       correct_step in f32 on the three utterances, two LMs and two weights of tests/golden/p2w_tiny_correct.npz: the word
                   and phone hypotheses, the masked positions and hyp_cor equal the reference's test_step, token_probs_v within 1e-4;
                   decode_word_and_phone equals two separate decode calls exactly."""
import numpy as np
import pytest
import torch

from tests.correct_ref import collapse_runs, fuse_ref, softmax64, token_conf_ref

pytestmark = pytest.mark.gpu

_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]
BLANK = 0


# ---- ctc_token_conf ------------------------------------------------------------------------------------------------------------------
def _elens(T):
    return [T, (T + 1) // 2, max(T - 2, 0)]


def _paths(T, V, rng):
    """three frame-level paths [3, T] for _elens(T), ids past the lengths are garbage:
    0: a token only at frame 0, equal tokens separated by one blank, adjacent different tokens, random runs, a run ending at the
       last valid frame;  1: all blank;  2: one long run from frame 1 to the last valid frame (it crosses every 64-frame pass)"""
    el = _elens(T)
    tok = lambda: int(rng.integers(1, V))

    def other(a):
        b = tok()
        return b if b != a else (a % (V - 1)) + 1

    a = tok()
    p0 = [a, BLANK, a, BLANK, a, a, other(a)]
    while len(p0) < el[0]:
        v = int(rng.integers(0, V))
        p0 += [v] * int(rng.integers(1, 6))
    p0 = p0[:el[0]]
    if el[0] >= 2:
        p0[-1] = other(p0[-2]) if el[0] > 7 else (p0[-1] or a)   # the last run ends at elens - 1
    paths = np.full((3, T), 10 ** 6, np.int64)
    paths[0, :el[0]] = p0
    paths[1, :el[1]] = BLANK
    paths[1, el[1]:] = -7
    paths[2, :el[2]] = tok()
    if el[2] >= 1:
        paths[2, 0] = BLANK
    paths[2, el[2]:] = 1     # a valid token id past the length: must not extend the run
    return paths, el


def _conf_case(T, V, dtype):
    """-> logits [3,T,V] (rounded to dtype, as float64), paths, elens, and per utterance the float64 reference with planted ties.
    The first seed of ten whose every run has its best frame 1e-4 (relative) ahead of the second-best is the case."""
    for seed in range(10):
        case = _conf_case_of(T, V, dtype, seed)
        if case is not None:
            return case
    raise AssertionError(f"no seed gives T={T} V={V} {dtype} a best-two gap of 1e-4 in every run")


def _conf_case_of(T, V, dtype, seed):
    rng = np.random.default_rng(1000 * T + V + 7919 * seed)
    paths, el = _paths(T, V, rng)
    z = rng.standard_normal((3, T, V)) * 2.0
    for b in range(3):
        for t in range(el[b]):
            if paths[b, t] != BLANK:
                z[b, t, paths[b, t]] += rng.uniform(1.0, 5.0)     # the path's id is the likely one, with a spread of confidences
    z = torch.from_numpy(z).to(dtype).double().numpy()
    want = []
    for b in range(3):
        ids, frames, confs, gaps = token_conf_ref(softmax64(z[b]), paths[b], el[b], BLANK)
        if not all(g >= 1e-4 for g in gaps):
            return None
        want.append([ids, frames, confs])
    # plant exact ties: copy the best frame's row onto another frame of its run (every run of two frames or more)
    for b in range(3):
        ids, frames, confs = want[b]
        for j, (v, ts) in enumerate(collapse_runs(paths[b], el[b], BLANK)):
            if len(ts) >= 2 and j % 2 == 0:
                k = frames[j]
                o = ts[-1] if k != ts[-1] else ts[0]      # the far end of the run: across a 64-frame pass where the run is long
                z[b, o] = z[b, k]
                frames[j] = min(k, o)
    return z, paths, el, want


@pytest.mark.parametrize("V", [5, 40, 1003])
@pytest.mark.parametrize("T", [1, 7, 64, 65, 130])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_ctc_token_conf(dev, dtype, T, V):
    from emoasr_amd import ops
    z, paths, el, want = _conf_case(T, V, dtype)
    lse = torch.logsumexp(torch.from_numpy(z), dim=-1).float()       # float64, rounded once
    pad = 3                                                          # rows of V + 3 elements: most are not 16-byte aligned
    wide = torch.full((3, T, V + pad), float("nan"), dtype=dtype)
    wide[..., :V] = torch.from_numpy(z).to(dtype)
    zd = wide.to(dev)[..., :V]
    frame, conf, ntok = ops.ctc_token_conf(zd, lse.reshape(-1).to(dev), torch.from_numpy(paths).to(torch.int32).to(dev),
                                           torch.tensor(el, dtype=torch.int32, device=dev), BLANK)
    frame, conf, ntok = frame.cpu().numpy(), conf.cpu().numpy().astype(np.float64), ntok.cpu().numpy()
    bar = 1e-6 if dtype == torch.float32 else 1e-5
    worst = 0.0
    for b in range(3):
        ids, frames, confs = want[b]
        assert ntok[b] == len(ids), (b, ntok[b], len(ids))
        assert frame[b, :len(ids)].tolist() == frames, (b, frame[b, :len(ids)].tolist(), frames)
        if ids:
            rel = np.abs(conf[b, :len(ids)] - np.asarray(confs)) / np.asarray(confs)
            worst = max(worst, float(rel.max()))
    print(f"[measured] ctc_token_conf T={T} V={V} {dtype}: conf rel err {worst:.2e} (bar {bar:.0e})")
    assert worst <= bar
    assert ntok[1] == 0


def test_ctc_token_conf_matches_the_collapse(dev):
    """token j of ctc_token_conf is hyp[b, j] of ctc_greedy on the same logits (the recogniser's own path, no planted ids)"""
    from emoasr_amd import ops
    g = torch.Generator().manual_seed(5)
    B, T, V = 4, 150, 12
    z = torch.randn(B, T, V, generator=g)
    z[..., BLANK] += 1.5
    z = z.repeat_interleave(2, dim=1)[:, :T].contiguous()            # runs of two equal frames
    el = [150, 149, 64, 1]
    zd, eld = z.to(dev), torch.tensor(el, dtype=torch.int32, device=dev)
    best, hyp, hyplen = ops.ctc_greedy(zd, eld, BLANK)
    frame, conf, ntok = ops.ctc_token_conf(zd, ops.row_lse(zd.view(B * T, V)), best.contiguous(), eld, BLANK)
    assert torch.equal(ntok, hyplen)
    probs = softmax64(z.double().numpy())
    for b in range(B):
        n = int(ntok[b])
        assert n > 0 or el[b] == 1
        fr = frame[b, :n].cpu().numpy()
        assert (np.diff(fr) > 0).all() and (fr < el[b]).all()
        want = probs[b, fr, hyp[b, :n].cpu().numpy()]
        np.testing.assert_allclose(conf[b, :n].cpu().numpy(), want, rtol=2e-6)   # (row_lse's own f32 error is inside this bar)


# ---- correct_fuse --------------------------------------------------------------------------------------------------------------------
def _fuse_case(n, V, w, dt_a, dt_l, seed=0):
    rng = np.random.default_rng(100 * n + V + int(10 * w) + seed)
    R = n + 2
    asr = rng.standard_normal((R, V)) * 2.0
    lm = rng.standard_normal((n, V + 1)) * 2.0
    for x in (asr, lm):      # the leading column of every row leads by 0.5 at least: bf16 rounding cannot make the top two equal
        x[np.arange(len(x)), x.argmax(axis=1)] += rng.uniform(0.5, 1.5, len(x))
    asr[:, rng.integers(0, V)] = -np.inf
    lm[:, rng.integers(0, V + 1)] = -np.inf
    rows = rng.permutation(R)[:n]
    asr = torch.from_numpy(asr).to(dt_a).double().numpy()
    lm = torch.from_numpy(lm).to(dt_l).double().numpy()
    ids, val, margin = fuse_ref(asr[rows], lm, w, V)
    assert (margin >= 1e-6).all(), (n, V, w, margin.min())
    return asr, lm, rows, ids, val


def _dev_rows(x, dtype, dev, ld=None):
    """x [M, V] on the device, as the [:, :V] view of a NaN-filled [M, ld] buffer when a row stride is given"""
    t = torch.from_numpy(x).to(dtype)
    if ld is None:
        return t.to(dev)
    wide = torch.full((x.shape[0], ld), float("nan"), dtype=dtype)
    wide[:, :x.shape[1]] = t
    return wide.to(dev)[:, :x.shape[1]]


@pytest.mark.parametrize("w", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("V", [5, 40, 1003])
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("dts", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)],
                         ids=["f32", "bf16", "f32+bf16"])
def test_correct_fuse(dev, dts, n, V, w):
    from emoasr_amd import ops
    asr, lm, rows, ids, val = _fuse_case(n, V, w, *dts)
    lse = torch.logsumexp(torch.from_numpy(asr), dim=-1).float().to(dev)
    rows_d = torch.from_numpy(rows).to(torch.int32).to(dev)
    worst = 0.0
    # contiguous rows (odd V: most rows are not 16-byte aligned), then rows padded to a multiple of 8 elements (all aligned: the
    # 16-byte loads with the ragged end by element)
    for ld_a, ld_l in ((None, None), ((V + 7) // 8 * 8 + 8, (V + 8) // 8 * 8)):
        got_id, got_val = ops.correct_fuse(_dev_rows(asr, dts[0], dev, ld_a), lse, _dev_rows(lm, dts[1], dev, ld_l), w, V,
                                           asr_rows=rows_d)
        assert got_id.dtype == torch.int32 and got_id.cpu().numpy().tolist() == ids.tolist(), (got_id.cpu().numpy(), ids)
        worst = max(worst, float((np.abs(got_val.cpu().numpy().astype(np.float64) - val) / val).max()))
    print(f"[measured] correct_fuse n={n} V={V} w={w} {dts}: value rel err {worst:.2e} (bar 1e-06)")
    assert worst <= 1e-6


@pytest.mark.parametrize("V", [5, 40, 1003])
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_correct_fuse_ties_go_to_the_lowest_column(dev, dtype, V):
    from emoasr_amd import ops
    rng = np.random.default_rng(V)
    n = 6
    asr = torch.from_numpy(rng.standard_normal((n, V))).to(dtype)
    lm = torch.from_numpy(rng.standard_normal((n, V + 1))).to(dtype)
    lo = [0, 1, V // 2 - 1, V - 2, 0, 2]
    hi = [V - 1, 2, V // 2 + 1, V - 1, 1, V - 1]
    for i in range(n):                     # two columns equal in both inputs and above the rest: equal mixed values, bit for bit
        asr[i, lo[i]] = asr[i, hi[i]] = 6.0
        lm[i, lo[i]] = lm[i, hi[i]] = 5.0
    lse = torch.logsumexp(asr.double(), dim=-1).float()
    for w in (0.0, 0.3, 1.0):
        got_id, got_val = ops.correct_fuse(asr.to(dev), lse.to(dev), lm.to(dev), w, V)
        assert got_id.cpu().tolist() == lo, (w, got_id.cpu().tolist(), lo)
    # a column only the LM likes, outside n_cols, is not a candidate
    lm[:, V] = 30.0
    got_id, _ = ops.correct_fuse(asr.to(dev), lse.to(dev), lm.to(dev), 1.0, V)
    assert got_id.cpu().tolist() == lo


# ---- end to end: correct_step against the reference's test_step (tests/golden/p2w_tiny_correct.npz) ------------------------------------
PHONE = dict(mtl_phone_ctc_weight=0.3, hie_mtl_phone=True, phone_vocab_size=12, inter_ctc_layer_id=1)


# the largest |change| of a soft-max entry of each LM at a masked position of the fixture when the CPU restatement (tests/bert_ref.py,
# tests/p2w_ref.py) runs with weights and stored activations rounded to bf16 instead of f32; tests/golden/make_golden_p2w.py measures
# them (lm_bf16_sim), asserts them to 2 % and asserts that the rule below leaves out at most a quarter of the masked positions.
# With the LM in bf16 a masked position is compared when its recorded absolute top-2 margin of the mixed probabilities exceeds
# 2 * lm_weight * 4 * that error: either leader may move by lm_weight * error, and 4 x the simulation is the bf16 bar used elsewhere.
LM_BF16_SIM = {"bert": 1.517e-4, "pbert": 8.425e-3}


@pytest.fixture(scope="module")
def world(dev):
    return _world(dev, torch.float32, torch.float32)


@pytest.fixture(scope="module")
def world_bf16_lm(dev):
    return _world(dev, torch.float32, torch.bfloat16)


@pytest.fixture(scope="module")
def world_bf16(dev):
    return _world(dev, torch.bfloat16, torch.bfloat16)


def _world(dev, asr_dtype, lm_dtype):
    """the fixture's recogniser (l2_tiny's weights, a sharpened word head, a seeded hierarchical phone head), both LMs, the data"""
    from types import SimpleNamespace
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.lm import LM
    from emoasr_amd.modeling.p2w import P2W
    from tests.test_p2w_gpu import P2W_CFG
    from tests.util import CONFIGS, LM_CFG, golden_npz
    c = golden_npz("p2w_tiny_correct")
    l2, bg, pg = golden_npz("l2_tiny"), golden_npz("bert_tiny"), golden_npz("p2w_tiny")
    cfg = dict(CONFIGS["l2_tiny"], **PHONE)
    sd = {k[3:]: torch.from_numpy(v) for k, v in l2.items() if k.startswith("sd/")}
    sd.update({k[4:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("asr/")})
    asr = ASR(SimpleNamespace(**cfg), phase="test", compute_dtype=asr_dtype)
    asr.load_state_dict(sd)
    asr = asr.to(dev).eval()
    bert = LM(SimpleNamespace(**dict(LM_CFG, lm_type="bert", mask_id=39)), compute_dtype=lm_dtype)
    bert.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in bg.items() if k.startswith("sd/")})
    lms = {"bert": bert.to(dev).eval()}
    for kind in ("pbert", "pctc"):
        lm = P2W(SimpleNamespace(**dict(P2W_CFG, lm_type=kind)), compute_dtype=lm_dtype)
        psd = {k[len(kind) + 4:]: torch.from_numpy(v) for k, v in pg.items() if k.startswith(kind + "/sd/")}
        if kind == "pbert":      # (the fixture sharpens the pbert head: a freshly initialised LM is near-uniform)
            psd["decoder.output.weight"] = torch.from_numpy(c["pbert/decoder.output.weight"])
        lm.load_state_dict(psd)
        lms[kind] = lm.to(dev).eval()
    xs, xlens = torch.from_numpy(l2["xs"]), torch.from_numpy(l2["xlens"])
    data = [{"utt_ids": [f"utt-{u}"], "xs": xs[u:u + 1, :int(xlens[u])], "xlens": xlens[u:u + 1], "texts": ["ref"]} for u in range(3)]
    return SimpleNamespace(c=c, cfg=cfg, asr=asr, lms=lms, data=data)


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_step_f32(dev, world, kind):
    from emoasr_amd.correct import correct_step
    c, cfg = world.c, world.cfg
    th = float(c["mask_th"])
    for u, data in enumerate(world.data):
        for w in c["lm_weights"].tolist():
            det = {}
            utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens = correct_step(
                world.asr, world.lms[kind], data, cfg["blank_id"], 39, th, w, dev, cfg["vocab_size"], details=det)
            assert utt_id == f"utt-{u}" and reftext == "ref"
            assert list(hyp) == c[f"u{u}/hyp"].tolist()
            if kind == "pbert":
                assert det["hyp_phone"].tolist() == c[f"u{u}/hyp_phone"].tolist()
            err = np.abs(det["token_probs_v"].astype(np.float64) - c[f"u{u}/token_probs_v"]).max()
            assert err <= 1e-4, err
            assert det["hyp_masked"].tolist() == c[f"u{u}/hyp_masked"].tolist()
            assert num_tokens == len(hyp) and num_masked == int((c[f"u{u}/hyp_masked"] == 39).sum()) and num_masked > 0
            assert hyp_cor == c[f"u{u}/{kind}/w{w}/hyp_cor"].tolist(), (u, kind, w)
    print(f"correct_step {kind}: token_probs_v within {err:.2e} on the last utterance")


def test_correct_step_cascade(dev, world):
    """lm_type "pctc": the phone hypothesis goes through P2W.decode; nothing is masked"""
    from emoasr_amd.correct import correct_step
    c, cfg = world.c, world.cfg
    lm = world.lms["pctc"]
    for u, data in enumerate(world.data):
        _, hyp, hyp_cor, _, num_masked, num_tokens = correct_step(world.asr, lm, data, cfg["blank_id"], 39, 0.8, 1.0, dev,
                                                                  cfg["vocab_size"], cascade_ctc=True)
        assert list(hyp) == c[f"u{u}/hyp"].tolist() and (num_masked, num_tokens) == (0, 0)
        assert hyp_cor == lm.decode(torch.from_numpy(c[f"u{u}/hyp_phone"]).unsqueeze(0))[0]


def test_empty_hypothesis_returns_the_empty_result(dev, world):
    from emoasr_amd.correct import correct_step
    data = dict(world.data[0])
    out = correct_step(world.asr, world.lms["bert"], data, world.cfg["blank_id"], 39, 0.8, 0.5, dev, 40)
    assert len(out[1]) > 0
    w = world.asr.decoder.output
    keep = w.bias.detach().clone()
    try:
        with torch.no_grad():
            w.bias[world.cfg["blank_id"]] += 1e4       # every frame is blank
        out = correct_step(world.asr, world.lms["bert"], data, world.cfg["blank_id"], 39, 0.8, 0.5, dev, 40)
        assert out == ("utt-0", [], [], "ref", 0, 0)
    finally:
        with torch.no_grad():
            w.bias.copy_(keep)


def test_decode_word_and_phone_equals_two_decodes(dev, world):
    c = world.c
    for u, data in enumerate(world.data):
        xs = data["xs"].to(dev)
        word, phone = world.asr.decode_word_and_phone(xs, data["xlens"])
        w2 = world.asr.decode(xs, data["xlens"])
        p2 = world.asr.decode(xs, data["xlens"], decode_phone=True)
        assert word[0] == w2[0] and word[3] == w2[3] and torch.equal(word[2], w2[2])
        assert phone[0] == p2[0] and phone[3] == p2[3] and torch.equal(phone[2], p2[2])
        assert phone[0][0] == c[f"u{u}/hyp_phone"].tolist() and word[0][0] == c[f"u{u}/hyp"].tolist()
        assert phone[2].shape[-1] == 12
    with pytest.raises(NotImplementedError):
        world.asr.decode(xs, data["xlens"], beam_width=4, decode_phone=True)


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_step_bf16_lm(dev, world_bf16_lm, kind):
    """the LM in bf16 (its logits reach correct_fuse as f32 for "bert", as bf16 for "pbert"), the recogniser in f32 so that the
    hypothesis and the masked positions are the fixture's: hyp_cor at the masked positions whose recorded margin is above the
    simulated bf16 error (LM_BF16_SIM above); the fixture maker asserts that at most a quarter of them are left out"""
    from emoasr_amd.correct import correct_step
    world = world_bf16_lm
    c, cfg = world.c, world.cfg
    compared = left_out = 0
    for u, data in enumerate(world.data):
        for w in c["lm_weights"].tolist():
            det = {}
            _, hyp, hyp_cor, _, num_masked, _ = correct_step(world.asr, world.lms[kind], data, cfg["blank_id"], 39, float(c["mask_th"]),
                                                            w, dev, cfg["vocab_size"], details=det)
            assert list(hyp) == c[f"u{u}/hyp"].tolist() and det["hyp_masked"].tolist() == c[f"u{u}/hyp_masked"].tolist()
            assert det["lm_logits"].dtype == (torch.float32 if kind == "bert" else torch.bfloat16)
            mask = c[f"u{u}/hyp_masked"] == 39
            sure = mask & (c[f"u{u}/{kind}/w{w}/margin_abs"] > 2 * w * 4 * LM_BF16_SIM[kind])
            want = c[f"u{u}/{kind}/w{w}/hyp_cor_full"]      # (the reference's hyp_cor before its pad ids are dropped)
            assert len(want) == len(mask)
            got = np.where(mask, det["y_gen"], c[f"u{u}/hyp"])
            assert (got[sure] == want[sure]).all(), (u, kind, w, got[sure], want[sure])
            assert (got[~mask] == want[~mask]).all()
            compared, left_out = compared + int(sure.sum()), left_out + int((mask & ~sure).sum())
    print(f"correct_step {kind}, LM in bf16: {compared} masked positions compared, {left_out} left out")
    assert 4 * left_out <= compared + left_out


@pytest.mark.parametrize("f32_head", [True, False], ids=["f32-head", "bf16-head"])
@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_step_bf16_is_its_kernels(dev, world_bf16, kind, f32_head):
    """recogniser and LM in bf16 (the recogniser's logits f32 or bf16): its hypothesis may differ from the f32 reference's, so the
    step is held to its own inputs -- confidences, frames, masked positions and fused ids restated in float64 from the logits the
    step's kernels read (ids only where the float64 top-2 margin is above 1e-6, the kernels' tested resolution)"""
    from emoasr_amd.correct import correct_step
    world = world_bf16
    c, cfg = world.c, world.cfg
    eng = world.asr.engine()
    keep = eng.f32_head
    eng.f32_head = f32_head
    try:
        for u, data in enumerate(world.data):
            det = {}
            _, hyp, hyp_cor, _, num_masked, num_tokens = correct_step(world.asr, world.lms[kind], data, cfg["blank_id"], 39,
                                                                       float(c["mask_th"]), 0.5, dev, cfg["vocab_size"], details=det)
            z = det["asr_logits"]
            assert z.dtype == (torch.float32 if f32_head else torch.bfloat16)
            z = z.double().cpu().numpy()
            best = det["best"].cpu().numpy()
            ids, frames, confs, gaps = token_conf_ref(softmax64(z), best, len(best), cfg["blank_id"])
            assert ids == list(hyp) and num_tokens == len(ids)
            np.testing.assert_allclose(det["token_probs_v"], confs, rtol=2e-6)      # (row_lse's own f32 error is inside this bar)
            fr = det["frames"].cpu().numpy()
            clear = np.asarray(gaps) > 1e-4
            assert (fr[clear] == np.asarray(frames)[clear]).all()
            mask = det["mask_indices"]
            assert num_masked == int(mask.sum()) and (det["hyp_masked"] == np.where(mask, 39, ids)).all()
            fid, fval, margin = fuse_ref(z[fr], det["lm_logits"].double().cpu().numpy(), 0.5, cfg["vocab_size"])
            ok = margin > 1e-6
            assert (det["y_gen"][ok] == fid[ok]).all()
            np.testing.assert_allclose(det["mix_values"], fval, rtol=2e-6)
            assert hyp_cor == [int(x) for x in np.where(mask, det["y_gen"], ids) if x != 0]
    finally:
        eng.f32_head = keep


def test_token_confidences_entry_point(dev, world):
    """correct.token_confidences on decode()'s own outputs: the lists of aligns, a tensor of frame ids, and strided logits"""
    from emoasr_amd.correct import token_confidences
    c, cfg = world.c, world.cfg
    for u, data in enumerate(world.data):
        hyps, _, logits, aligns = world.asr.decode(data["xs"].to(dev), data["xlens"])
        T = logits.shape[1]
        want = c[f"u{u}/token_probs_v"]
        wide = torch.zeros(1, T, 48, device=dev, dtype=logits.dtype)
        wide[..., :40] = logits
        best = torch.tensor([aligns[0]], device=dev)
        for lg, al in ((logits, aligns), (logits, best), (wide[..., :40], aligns)):
            frame, conf, ntok = token_confidences(lg, al, [len(aligns[0])], cfg["blank_id"])
            assert int(ntok[0]) == len(hyps[0]) == len(want)
            np.testing.assert_allclose(conf[0, :len(want)].cpu().numpy(), want, atol=1e-4)
            assert [aligns[0][t] for t in frame[0, :len(want)].tolist()] == hyps[0]


def test_correct_test_rows(dev, world):
    """correct.test: the result rows of decode.test's shape, one per utterance, from correct_step"""
    from emoasr_amd import correct
    c, cfg = world.c, world.cfg
    vocab = SimpleNamespaceVocab()
    rows = correct.test(world.asr, world.lms["bert"], world.data, vocab, cfg["vocab_size"], dev, cfg["blank_id"], 39,
                        float(c["mask_th"]), 0.5)
    assert [r[0] for r in rows] == ["utt-0", "utt-1", "utt-2"] and all(len(r) == 4 and r[3] == "ref" for r in rows)
    for u, r in enumerate(rows):
        want = c[f"u{u}/bert/w0.5/hyp_cor"].tolist()
        assert r[1] == " ".join(str(i) for i in want) and r[2] == vocab.ids2text(want)
    assert len(correct.test(world.asr, world.lms["bert"], world.data, vocab, cfg["vocab_size"], dev, cfg["blank_id"], 39,
                            float(c["mask_th"]), 0.5, num_samples=2)) == 2


class SimpleNamespaceVocab:
    def ids2text(self, ids):
        return "".join(chr(97 + i % 26) for i in ids)
