"""The correction grid on the CPU: tests/correct_grid_ref.py (the numpy restatement of emoasr_correct_mask_grid /
emoasr_correct_fuse_grid and of correct_batch's assembly, the oracle of the GPU tests) held to tests/golden/correct_grid_tiny.npz, which
the reference's test_step wrote cell by cell; the argument parsing of emoasr_amd.correct_grid; metrics.compute_wers_cells.

The fixture's maker asserts that every masked position's top-2 margin of the mixed probabilities exceeds 1e-5 and that every threshold
is 1e-4 away from every confidence, so the float64 restatement below (LM soft-max error ~1e-7) decides every id and every mask."""
import numpy as np
import pytest
import torch

from tests import bert_ref, p2w_ref
from tests.correct_grid_ref import assemble_ref, fuse_grid_ref, mask_grid_ref
from tests.correct_ref import softmax64, token_conf_ref
from tests.util import golden_npz

MASK_ID, V = 39, 40


@pytest.fixture(scope="module")
def grid():
    """the fixture, the three utterances as one padded batch (hyp, ntok, conf, frame from the recorded recogniser logits), and the
    restated mask grid over the fixture's thresholds"""
    g, c = golden_npz("correct_grid_tiny"), golden_npz("p2w_tiny_correct")
    hyps = [g[f"u{u}/hyp"] for u in range(3)]
    T = max(len(c[f"u{u}/aligns"]) for u in range(3))
    hyp, conf, frame = np.full((3, T), -5, np.int64), np.full((3, T), np.nan, np.float32), np.zeros((3, T), np.int64)
    for u in range(3):
        aligns = c[f"u{u}/aligns"]
        ids, frames, confs, _ = token_conf_ref(softmax64(c[f"u{u}/logits"]), aligns, len(aligns), 0)
        assert ids == hyps[u].tolist()
        hyp[u, :len(ids)], conf[u, :len(ids)], frame[u, :len(ids)] = ids, confs, frames
    ntok = [len(h) for h in hyps]
    ths = g["mask_ths"].tolist()
    return dict(g=g, c=c, hyp=hyp, conf=conf, frame=frame, ntok=ntok, T=T, ths=ths, ws=g["lm_weights"].tolist(),
                grid=mask_grid_ref(hyp, ntok, conf, frame, ths, MASK_ID, 0))


def test_the_fixture_is_the_issue_s(grid):
    g = grid["g"]
    assert grid["ths"] == [0.2, 0.6, 0.8, 0.9] and grid["ws"] == [0.0, 0.25, 0.5, 1.0]
    per_th = [sum(int(g[f"th{th}/u{u}/num_masked"]) for u in range(3)) for th in grid["ths"]]
    assert per_th == [0, 14, 33, 44]
    least = min(g[f"th{th}/w{w}/{kind}/u{u}/margin_abs"][g[f"th{th}/u{u}/hyp_masked"] == MASK_ID].min()
                for th in grid["ths"][1:] for w in grid["ws"] for kind in ("bert", "pbert") for u in range(3)
                if (g[f"th{th}/u{u}/hyp_masked"] == MASK_ID).any())
    assert least > 1e-5
    assert min(np.abs(g[f"u{u}/token_probs_v"] - th).min() for u in range(3) for th in grid["ths"]) > 1e-4


def test_mask_grid_restatement_gives_the_reference_s_masks_counts_and_order(grid):
    g, T = grid["g"], grid["T"]
    ys, num, lm_rows, asr_rows = grid["grid"]
    for k, th in enumerate(grid["ths"]):
        for u in range(3):
            n = grid["ntok"][u]
            assert ys[k, u, :n].tolist() == g[f"th{th}/u{u}/hyp_masked"].tolist() and (ys[k, u, n:] == 0).all()
            assert num[k, u] == int(g[f"th{th}/u{u}/num_masked"])
    assert len(lm_rows) == num.sum() == 91 and (np.diff(lm_rows) > 0).all()      # (threshold, utterance, token): ascending flat rows
    want = [(k * 3 + u) * T + j for k, th in enumerate(grid["ths"]) for u in range(3)
            for j in np.flatnonzero(g[f"th{th}/u{u}/hyp_masked"] == MASK_ID)]
    assert lm_rows.tolist() == want
    b, j = (lm_rows // T) % 3, lm_rows % T
    assert (asr_rows == b * T + grid["frame"][b, j]).all()


def test_mask_grid_restatement_edges():
    hyp = np.array([[5, 6, 7], [8, 9, 1], [2, 3, 4]])
    conf = np.array([[0.5, 0.25, 0.75], [0.1, 0.2, 0.3], [0.9, 0.9, 0.9]], np.float32)
    frame = np.array([[0, 2, 5], [1, 3, 4], [0, 1, 2]])
    ys, num, lm_rows, asr_rows = mask_grid_ref(hyp, [3, 0, 2], conf, frame, [0.0, 0.5, 2.0], 39, 0)
    assert ys[0].tolist() == [[5, 6, 7], [0, 0, 0], [2, 3, 0]] and num[0].tolist() == [0, 0, 0]      # masks nothing
    assert ys[1].tolist() == [[5, 39, 7], [0, 0, 0], [2, 3, 0]] and num[1].tolist() == [1, 0, 0]     # 0.5 == th: not masked
    assert ys[2].tolist() == [[39, 39, 39], [0, 0, 0], [39, 39, 0]] and num[2].tolist() == [3, 0, 2]  # masks everything
    assert lm_rows.tolist() == [10, 18, 19, 20, 24, 25] and asr_rows.tolist() == [2, 0, 2, 5, 6, 7]


def _sd64(arrays, prefix):
    return {k[len(prefix):]: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v)
            for k, v in arrays.items() if k.startswith(prefix)}


@pytest.mark.parametrize("kind", ["bert", "pbert"])
def test_grid_restatement_gives_the_reference_s_hyp_cor_in_every_cell(grid, kind):
    """masked inputs of the restated mask grid -> the LM's float64 restatement -> the multi-weight fuse -> the assembly"""
    g, c, T = grid["g"], grid["c"], grid["T"]
    ys, num, lm_rows, asr_rows = grid["grid"]
    if kind == "bert":
        sd = _sd64(golden_npz("bert_tiny"), "sd/")
    else:
        sd = _sd64(golden_npz("p2w_tiny"), "pbert/sd/")
        sd["decoder.output.weight"] = torch.from_numpy(c["pbert/decoder.output.weight"]).double()
    asr = np.zeros((3 * T, V))
    for u in range(3):
        asr[u * T:u * T + len(c[f"u{u}/logits"])] = c[f"u{u}/logits"]
    first = np.concatenate([[0], np.cumsum(num.reshape(-1))])
    for k, th in enumerate(grid["ths"]):
        lm = np.zeros((3 * T, V))
        for u in range(3):
            n = grid["ntok"][u]
            y = torch.from_numpy(ys[k, u:u + 1, :n])
            if kind == "bert":
                lg = bert_ref.logits(sd, y, [n])
            else:
                ps = torch.from_numpy(g[f"u{u}/hyp_phone"]).unsqueeze(0)
                lg = p2w_ref.pbert_logits(sd, y, [n], ps, [ps.shape[1]])
            lm[u * T:u * T + n] = lg[0, :, :V].numpy()
        lo, hi = first[k * 3], first[(k + 1) * 3]
        rows = lm_rows[lo:hi] - k * 3 * T
        ids, _, margin = fuse_grid_ref(asr[asr_rows[lo:hi]], lm[rows], grid["ws"], V)
        assert hi == lo or margin.min() > 1e-5
        for m, w in enumerate(grid["ws"]):
            for u in range(3):
                a, b = first[k * 3 + u] - lo, first[k * 3 + u + 1] - lo
                got = assemble_ref(g[f"u{u}/hyp"], lm_rows[lo + a:lo + b] % T, ids[m, a:b])
                assert got == g[f"th{th}/w{w}/{kind}/u{u}/hyp_cor"].tolist(), (kind, th, w, u)


def test_fuse_grid_restatement_is_fuse_ref_per_weight():
    from tests.correct_ref import fuse_ref
    rng = np.random.default_rng(3)
    asr, lm = rng.standard_normal((4, 9)), rng.standard_normal((4, 11))
    ids, val, margin = fuse_grid_ref(asr, lm, [0.0, 0.3, 1.0], 9)
    assert ids.shape == (3, 4)
    for m, w in enumerate([0.0, 0.3, 1.0]):
        i1, v1, m1 = fuse_ref(asr, lm, w, 9)
        assert (ids[m] == i1).all() and (val[m] == v1).all() and (margin[m] == m1).all()
    assert (ids[0] == asr.argmax(axis=1)).all() and (ids[2] == lm[:, :9].argmax(axis=1)).all()


def test_correct_grid_arguments():
    from emoasr_amd import correct_grid
    p = correct_grid.build_parser()
    a = p.parse_args("-conf a.yaml -ep 40 -lm_conf l.yaml -lm_ep 20 --lm_weight 0,0.25,1 --mask_th 0.8".split())
    assert a.lm_weight == [0.0, 0.25, 1.0] and a.mask_th == [0.8] and a.conf == "a.yaml" and a.lm_ep == "20"
    d = p.parse_args("-conf a.yaml -ep 40 -lm_conf l.yaml -lm_ep 20".split())
    assert d.lm_weight == [1.0] and d.mask_th == [0.9] and d.data_tag == "test" and not d.runtime      # the reference's defaults
    assert correct_grid.float_list(" 0.5 , 1 ") == [0.5, 1.0]
    with pytest.raises(SystemExit):
        p.parse_args("-conf a.yaml -ep 40 -lm_conf l.yaml -lm_ep 20 --mask_th ,".split())
    with pytest.raises(SystemExit):
        p.parse_args("-conf a.yaml -ep 40 --mask_th 0.5".split())


def test_write_results_names_the_cells_as_the_reference_does(tmp_path):
    from emoasr_amd import correct_grid
    wd = dict(n_sub=1, n_ins=0, n_del=2, n_ref=10, wer=30.0)
    rows = [["utt-0", "3 4", "c d", "c e"], ["utt-1", None, "", "f"]]
    path = correct_grid.write_results([(0.9, 0.5, rows, 30.0, wd, 4, 7), (0.9, 1.0, rows, 30.0, wd, 4, 7)], str(tmp_path), "test",
                                      "bert", "40")
    lines = open(tmp_path / "result_test_bert_corr0.5_maskth0.9_ep40.tsv").read().splitlines()
    assert lines[0] == "# WER: 30.00 [D=2, S=1, I=0, N=10]" and lines[1] == "#" and lines[2] == "utt_id\ttoken_id\ttext\treftext"
    assert lines[3] == "utt-0\t3 4\tc d\tc e" and (tmp_path / "result_test_bert_corr1.0_maskth0.9_ep40.tsv").exists()
    summary = open(path).read().splitlines()
    assert summary[0].split("\t")[:3] == ["mask_th", "lm_weight", "wer"] and len(summary) == 3
    assert summary[1].split("\t") == ["0.9", "0.5", "30.0", "1", "0", "2", "10", "4", "7"]


def test_compute_wers_cells_is_compute_wers_per_cell():
    from emoasr_amd.metrics import compute_wers, compute_wers_cells
    refs = ["a b c d".split(), "e f".split(), "g".split()]
    cells = [["a b c d".split(), "e".split(), []], ["a x c".split(), "e".split(), "g h".split()], ["a b c d".split(), "f e".split(), []]]
    got = compute_wers_cells(cells, refs)
    for cell, (wer, wd) in zip(cells, got):
        want_wer, want = compute_wers(cell, refs)
        assert wer == want_wer and all(wd[k] == want[k] for k in ("n_sub", "n_ins", "n_del", "n_ref"))
