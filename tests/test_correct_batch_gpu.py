"""correct.correct_batch end to end on the three utterances of tests/golden/p2w_tiny_correct.npz over the 16 cells of
tests/golden/correct_grid_tiny.npz (the reference's test_step, cell by cell, one utterance at a time).

  f32          hyp, hyp_phone, hyp_masked, num_masked and hyp_cor against the fixture in every cell (its maker asserts a top-2 margin
               above 1e-5 at every masked position and thresholds 1e-4 away from every confidence, so nothing is left out); one LM
               pass per threshold that masks something; the th = 0.8 cells against correct_step looped over the utterances.
  bf16 / f32   the batch held to its own inputs, as test_correct_step_bf16_is_its_kernels does: confidences, frames, masks, row lists
               and fused ids restated in float64 from the tensors in `details`, ids where the float64 margin exceeds 1e-6.

PADDING.  The Conformer's convolution module never masks padded frames by default (csrc/convmodule.hip, as the reference's does
not), so an utterance padded inside a batch would not have the hypothesis it has alone: with the three utterances (203, 167 and 131
input frames) as ONE zero-padded batch the CPU oracle (oracle/model.py: asr_ctc_greedy) gives utterance 1 another word hypothesis,
and without masking 69 entries of the grid differed from the fixture on an MI355X, all on utterances 1 and 2.  correct_batch
therefore runs its one encoder pass with engine.mask_padding (the GLU writes zeros past every utterance's end:
ops.glu_fwd_masked), and the padded batch of three is held to the batch-of-one fixture and to correct_step looped."""
import numpy as np
import pytest
import torch

from tests.correct_grid_ref import fuse_grid_ref, mask_grid_ref
from tests.correct_ref import softmax64, token_conf_ref
from tests.test_correct_gpu import SimpleNamespaceVocab, _world
from tests.util import golden_npz

pytestmark = pytest.mark.gpu

MASK_ID = 39


@pytest.fixture(scope="module")
def world(dev):
    return _world(dev, torch.float32, torch.float32)


@pytest.fixture(scope="module")
def world_bf16(dev):
    return _world(dev, torch.bfloat16, torch.bfloat16)


@pytest.fixture(scope="module")
def grid():
    return golden_npz("correct_grid_tiny")


def _batch(world, utts=(0, 1, 2)):
    """the utterances collated: zero-padded features, their lengths, ids and references"""
    data = [world.data[u] for u in utts]
    xs = torch.nn.utils.rnn.pad_sequence([d["xs"][0] for d in data], batch_first=True)
    return {"utt_ids": [d["utt_ids"][0] for d in data], "xs": xs, "xlens": torch.cat([d["xlens"] for d in data]),
            "texts": [d["texts"][0] for d in data]}


def _same(a, b):
    """two lists of correct_step tuples, hyp compared as a list"""
    return len(a) == len(b) and all(x[0] == y[0] and list(x[1]) == list(y[1]) and list(x[2]) == list(y[2]) and x[3:] == y[3:]
                                    for x, y in zip(a, b))


def _grid_cells(world, grid, kind, dev, utts=(0, 1, 2)):
    cfg = world.cfg
    det = {}
    cells = correct_batch_of(world, kind, dev, _batch(world, utts), grid["mask_ths"].tolist(), grid["lm_weights"].tolist(), det)
    return cells, det


def correct_batch_of(world, kind, dev, data, ths, ws, det=None, **kw):
    from emoasr_amd.correct import correct_batch
    cfg = world.cfg
    return correct_batch(world.asr, world.lms[kind], data, cfg["blank_id"], MASK_ID, ths, ws, dev, cfg["vocab_size"], details=det, **kw)


def _against_fixture(cells, det, g, kind, utts):
    """-> the (field, mask_th, lm_weight, utterance) entries of the grid that differ from the fixture"""
    bad = []
    for k, th in enumerate(g["mask_ths"].tolist()):
        for m, w in enumerate(g["lm_weights"].tolist()):
            for b, u in enumerate(utts):
                utt_id, hyp, hyp_cor, reftext, num_masked, num_tokens = cells[k][m][b]
                assert utt_id == f"utt-{u}" and reftext == "ref" and num_tokens == len(hyp)
                got = dict(hyp=list(hyp), hyp_masked=det["hyp_masked"][k][b].tolist(), num_masked=num_masked, hyp_cor=hyp_cor)
                want = dict(hyp=g[f"u{u}/hyp"].tolist(), hyp_masked=g[f"th{th}/u{u}/hyp_masked"].tolist(),
                            num_masked=int(g[f"th{th}/u{u}/num_masked"]), hyp_cor=g[f"th{th}/w{w}/{kind}/u{u}/hyp_cor"].tolist())
                if kind == "pbert":
                    got["hyp_phone"], want["hyp_phone"] = det["hyp_phone"][b].tolist(), g[f"u{u}/hyp_phone"].tolist()
                bad += [(f, th, w, u) for f in want if got[f] != want[f]]
    return bad


# ---- the padded batch against the batch-of-one fixture (see PADDING above) -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_batch_f32_is_the_reference_in_every_cell(dev, world, grid, kind):
    """the three utterances as ONE padded batch, the 16 cells, every field against the fixture"""
    cells, det = _grid_cells(world, grid, kind, dev)
    assert len(cells) == 4 and all(len(row) == 4 for row in cells)
    bad = _against_fixture(cells, det, grid, kind, (0, 1, 2))
    print(f"[measured] padded batch, {kind}: {len(bad)} grid entries differ from the batch-of-one fixture, utterances "
          f"{sorted({e[3] for e in bad})}, fields {sorted({e[0] for e in bad})}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_batch_is_correct_step_looped(dev, world, grid, kind):
    """the th = 0.8 cells of the padded batch against correct_step looped over the utterances"""
    from emoasr_amd.correct import correct_step
    cfg = world.cfg
    ws = grid["lm_weights"].tolist()
    cells = correct_batch_of(world, kind, dev, _batch(world), [0.8], ws)
    differ = []
    for m, w in enumerate(ws):
        loop = [correct_step(world.asr, world.lms[kind], d, cfg["blank_id"], MASK_ID, 0.8, w, dev, cfg["vocab_size"]) for d in world.data]
        differ += [(w, u) for u in range(3) if not _same(cells[0][m][u:u + 1], loop[u:u + 1])]
    print(f"[measured] padded batch, {kind}, th 0.8: (lm_weight, utterance) that differ from correct_step looped: {differ}")
    assert not differ


def test_correct_batch_cascade(dev, world):
    """lm_type "pctc": one batched P2W.decode over the padded phone hypotheses against correct_step(cascade_ctc=True) per utterance.
    On batches without padding (one utterance, two copies of it) and on the padded batch of three."""
    from emoasr_amd.correct import correct_step
    cfg, lm = world.cfg, world.lms["pctc"]
    loop = [correct_step(world.asr, lm, d, cfg["blank_id"], MASK_ID, 0.8, 1.0, dev, cfg["vocab_size"], cascade_ctc=True)
            for d in world.data]
    assert all(len(t[2]) > 0 and t[4:] == (0, 0) for t in loop)
    for u in range(3):                     # no padding: one utterance, and two copies of it
        for utts in ((u,), (u, u)):
            det = {}
            cells = correct_batch_of(world, "pctc", dev, _batch(world, utts), [0.6, 0.8], [0.5, 1.0], det, cascade_ctc=True)
            assert len(cells) == 1 and len(cells[0]) == 1 and det["lm_calls"] == 0      # no grid: one cell
            assert _same(cells[0][0], [loop[u]] * len(utts)), utts
    cells = correct_batch_of(world, "pctc", dev, _batch(world), 0.8, 1.0, cascade_ctc=True)
    differ = [u for u in range(3) if not _same(cells[0][0][u:u + 1], loop[u:u + 1])]
    print(f"[measured] padded batch, pctc cascade: utterances that differ from correct_step: {differ}")
    assert not differ


def test_correct_test_takes_a_batched_loader(dev, world):
    """correct.test: a loader of batch size 3 gives the rows that the batch-1 loader gives; impl="batch" sends single utterances
    through correct_batch with the same rows"""
    from emoasr_amd import correct
    cfg = world.cfg
    vocab = SimpleNamespaceVocab()
    args = (vocab, cfg["vocab_size"], dev, cfg["blank_id"], MASK_ID, 0.8, 0.5)
    one = correct.test(world.asr, world.lms["bert"], world.data, *args)
    assert len(one) == 3 and correct.test(world.asr, world.lms["bert"], world.data, *args, impl="batch") == one
    with pytest.raises(ValueError):
        correct.test(world.asr, world.lms["bert"], world.data, *args, impl="grid")
    rows = correct.test(world.asr, world.lms["bert"], [_batch(world)], *args)
    assert len(rows) == 3 and [r[0] for r in rows] == [r[0] for r in one] and rows[0] == one[0]      # (utterance 0 has no padding)
    differ = [u for u in range(3) if rows[u] != one[u]]
    print(f"[measured] correct.test, loader of batch size 3: rows that differ from the batch-1 loader's: {differ}")
    assert rows == one


def test_mask_padding_gives_every_utterance_its_own_encoder_output(dev, world):
    """engine.mask_padding: the valid frames of every utterance of the zero-padded batch equal the utterance's batch-of-one encoder
    output to 1e-4 of the largest output (f32: the same kernels on other row counts, rounding of ~6e-8 sqrt(256) per product through
    two layers); without it (the default, the reference's behaviour) a padded utterance misses that bar"""
    asr, data = world.asr, _batch(world)
    eng = asr.engine()
    with torch.no_grad():
        alone = [asr.encoder(d["xs"].to(dev), d["xlens"])[0][0] for d in world.data]
        plain = asr.encoder(data["xs"].to(dev), data["xlens"])[0]
        eng.mask_padding = True
        try:
            masked = asr.encoder(data["xs"].to(dev), data["xlens"])[0]
        finally:
            eng.mask_padding = False
    scale = max(float(a.abs().max()) for a in alone)
    err = [float((masked[u, :len(a)] - a).abs().max()) / scale for u, a in enumerate(alone)]
    leak = [float((plain[u, :len(a)] - a).abs().max()) / scale for u, a in enumerate(alone)]
    print(f"[measured] padded batch against batch of one, relative to the largest output: masked {err}, unmasked {leak}")
    assert max(err) <= 1e-4
    assert leak[0] <= 1e-4 and min(leak[1:]) > 1e-4      # (utterance 0 is the longest: no padded frame; the others miss the bar)


# ---- what correct_batch adds, held exactly -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_batch_without_padding_is_the_reference_in_every_cell(dev, world, grid, kind):
    """every utterance as a batch of one and as a batch of two copies of itself (no padded frame): every field of the 16 cells equals
    the fixture, and the th = 0.8 cells equal correct_step"""
    from emoasr_amd.correct import correct_step
    cfg = world.cfg
    ths, ws = grid["mask_ths"].tolist(), grid["lm_weights"].tolist()
    for u in range(3):
        for utts in ((u,), (u, u)):
            cells, det = _grid_cells(world, grid, kind, dev, utts)
            assert det["lm_calls"] == 3                       # th = 0.2 masks nothing: it adds no LM pass
            assert not _against_fixture(cells, det, grid, kind, utts)
        for m, w in enumerate(ws):
            step = correct_step(world.asr, world.lms[kind], world.data[u], cfg["blank_id"], MASK_ID, 0.8, w, dev, cfg["vocab_size"])
            assert _same(cells[ths.index(0.8)][m], [step, step])


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_batch_padded_utterance_0_is_the_reference(dev, world, grid, kind):
    """the padded batch of three: utterance 0 (the longest: no padded frame in its row) equals the fixture in every cell, next to
    two other utterances with other lengths, counts and masks; th = 0.2 masks nothing anywhere and adds no LM pass"""
    cells, det = _grid_cells(world, grid, kind, dev)
    bad = [e for e in _against_fixture(cells, det, grid, kind, (0, 1, 2)) if e[3] == 0]
    assert not bad, bad[:8]
    assert det["lm_calls"] == 3 and int(det["num_masked"][0].sum()) == 0 and all(det["valid"])


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_batch_scalars_are_the_one_cell_grid(dev, world, grid, kind):
    ths, ws = grid["mask_ths"].tolist(), grid["lm_weights"].tolist()
    cells, _ = _grid_cells(world, grid, kind, dev)
    one = correct_batch_of(world, kind, dev, _batch(world), 0.8, 0.5)
    assert len(one) == 1 and len(one[0]) == 1 and _same(one[0][0], cells[ths.index(0.8)][ws.index(0.5)])
    assert _same(one[0][0], correct_batch_of(world, kind, dev, _batch(world), [0.8], [0.5])[0][0])


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_correct_batch_everything_blank(dev, world, kind):
    cfg = world.cfg
    w = world.asr.decoder.output
    keep = w.bias.detach().clone()
    try:
        with torch.no_grad():
            w.bias[cfg["blank_id"]] += 1e4       # every frame is blank
        det = {}
        cells = correct_batch_of(world, kind, dev, _batch(world), [0.2, 0.9], [0.0, 0.5, 1.0], det)
        assert det["lm_calls"] == 0 and det["lm_logits"] is None
        for row in cells:
            for cell in row:
                assert cell == [(f"utt-{u}", [], [], "ref", 0, 0) for u in range(3)]
    finally:
        with torch.no_grad():
            w.bias.copy_(keep)


@pytest.mark.parametrize("kind", ["bert", "pbert"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_correct_batch_is_its_kernels(dev, world, world_bf16, dtype, kind):
    """the padded batch held to its own inputs (bf16: recogniser and LM in bf16)"""
    world = world if dtype == "f32" else world_bf16
    cfg = world.cfg
    V, blank = cfg["vocab_size"], cfg["blank_id"]
    ths, ws = [0.2, 0.6, 0.8, 0.9], [0.0, 0.25, 0.5, 1.0]
    det = {}
    data = _batch(world)
    cells = correct_batch_of(world, kind, dev, data, ths, ws, det)
    z = det["asr_logits"].double().cpu().numpy()
    B, T, _ = z.shape
    best, hyp_d = det["best"].cpu().numpy(), det["hyp"].cpu().numpy()
    ntok, conf, frames = det["ntok"].cpu().numpy(), det["conf"].cpu().numpy(), det["frames"].cpu().numpy()
    elens = [((int(n) - 1) // 2 - 1) // 2 for n in data["xlens"]]
    for b in range(B):
        ids, fr, confs, gaps = token_conf_ref(softmax64(z[b]), best[b], elens[b], blank)
        n = len(ids)
        assert n > 0 and ntok[b] == n and hyp_d[b, :n].tolist() == ids and list(cells[0][0][b][1]) == ids
        np.testing.assert_allclose(conf[b, :n], confs, rtol=2e-6)      # (row_lse's own f32 error is inside this bar)
        clear = np.asarray(gaps) > 1e-4
        assert (frames[b, :n][clear] == np.asarray(fr)[clear]).all()
    # masks and row lists from the kernel's own f32 confidences and frames: exact
    w_ys, w_num, w_lm, w_asr = mask_grid_ref(hyp_d, ntok, conf, frames, ths, MASK_ID, 0)
    assert (det["ys"].cpu().numpy() == w_ys).all() and (det["num_masked"].cpu().numpy() == w_num).all()
    assert det["lm_rows"].cpu().tolist() == w_lm.tolist() and det["asr_rows"].cpu().tolist() == w_asr.tolist()
    assert det["lm_calls"] == int((w_num.sum(axis=1) > 0).sum()) and len(w_lm) > 0
    # fused ids and maxima from the logits the fuse kernel read
    lm = det["lm_logits"].double().cpu().numpy()
    assert lm.shape[0] == len(w_lm)
    fid, fval, margin = fuse_grid_ref(z.reshape(B * T, -1)[w_asr], lm, ws, V)
    first = np.concatenate([[0], np.cumsum(w_num.reshape(-1))])
    for k in range(len(ths)):
        for m in range(len(ws)):
            for b in range(B):
                lo, hi = first[k * B + b], first[k * B + b + 1]
                ok = margin[m, lo:hi] > 1e-6
                y_gen = det["y_gen"][k][m][b]
                assert (y_gen[ok] == fid[m, lo:hi][ok]).all()
                np.testing.assert_allclose(det["mix_values"][k][m][b], fval[m, lo:hi], rtol=2e-6)
                pos = w_lm[lo:hi] % T
                assert det["mask_positions"][k][b].tolist() == pos.tolist()
                cor = hyp_d[b, :ntok[b]].astype(np.int64)
                cor[pos] = y_gen
                utt_id, hyp, hyp_cor, _, num_masked, num_tokens = cells[k][m][b]
                assert hyp_cor == [int(x) for x in cor if x != 0] and (num_masked, num_tokens) == (hi - lo, ntok[b])


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_logits_at_is_forward_at_the_rows(dev, world, kind):
    """LM.logits_at / P2W.logits_at on device inputs against the all-rows forward on the same ids, at rows of two stacked copies of a
    ragged batch; a MAX_TOKEN_ROWS that splits the stack into three runs gives the same logits.  f32: 1e-5 of the largest logit
    (the two paths run the same kernels on other row counts)"""
    from emoasr_amd.modeling.lm import LM
    lm = world.lms[kind]
    g = torch.Generator().manual_seed(3)
    ylens, plens, Lw = [9, 1, 5], [7, 2, 11], 12
    ys = torch.randint(3, 39, (3, Lw), generator=g)
    ps = torch.randint(3, 11, (3, 11), generator=g)
    for b, n in enumerate(ylens):
        ys[b, n:] = 0
    ys[0, 2] = ys[2, 4] = MASK_ID
    want = (lm(ys[:, :9], ylens) if kind == "bert" else lm(ys[:, :9], ylens, ps=ps, plens=plens)).float()
    pairs = [(0, 2), (0, 8), (1, 0), (2, 4), (3, 2), (5, 0), (5, 4)]          # (sequence of the stack of two copies, position)
    rows = torch.tensor([s * Lw + j for s, j in pairs], dtype=torch.int32, device=dev)
    stack = torch.cat([ys, ys]).to(dev)
    extra = () if kind == "bert" else (ps.to(dev), plens)
    got = lm.logits_at(stack, ylens * 2, rows, *extra)
    assert got.shape == (len(pairs), 40)
    ref = torch.stack([want[s % 3, j] for s, j in pairs])
    bar = 1e-5 * float(ref.abs().max())
    assert float((got.float() - ref).abs().max()) <= bar
    keep = LM.MAX_TOKEN_ROWS
    try:
        LM.MAX_TOKEN_ROWS = 2 * 16      # two sequences per run
        split = lm.logits_at(stack, ylens * 2, rows, *extra)
    finally:
        LM.MAX_TOKEN_ROWS = keep
    assert float((split.float() - ref).abs().max()) <= bar
    assert lm.logits_at(stack, ylens * 2, rows[:0], *extra).shape == (0, 40)
