"""N-best rescoring and error-label alignment on the device (csrc/rescore.hip, emoasr_amd/rescore.py, emoasr_amd/align_hyps.py) against
the host alignment emoasr_amd.metrics.compute_wer, the restatements of tests/rescore_ref.py and the reference's own outputs
(tests/golden/rescore.npz) -- all three are held to each other by tests/test_rescore_cpu.py.  Everything is integers, strings or
bit-specified float64, so every comparison is exact.

The host alignments of the length sweep are computed once per alphabet (module-scoped) and shared."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rescore_ref
from tests.test_rescore_cpu import tables
from tests.util import golden_npz

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257]      # the strip width of the kernel is 64; align_hyps' default len_max is 256
# (R, H) on each side of the size at which the direction codes leave LDS (2 * ceil(H / 64) * (R + 63) words against 4096):
# one strip of columns and three
THRESHOLD = [(1985, 1), (1986, 1), (619, 130), (620, 130)]


@pytest.fixture(scope="module")
def g():
    return golden_npz("rescore")


def _host(hyps, refs, ref_idx):
    from emoasr_amd.metrics import compute_wer
    out = []
    for h, r in zip(hyps, ref_idx):
        _, w = compute_wer(h, refs[r])
        out.append(((w["n_sub"], w["n_ins"], w["n_del"], w["n_sub"] + w["n_ins"] + w["n_del"]), "".join(w["error_list"])))
    return out


def _sweep(alphabet):
    """every (R, H) of LENGTHS x ({0} + LENGTHS), the R references shared by index; half of the hypotheses are edited copies of
    their reference (long runs of C with ties around the edits), half are random; the 257 x 257 pairs first and last"""
    rng = np.random.default_rng(100 + alphabet)
    refs = [rng.integers(0, alphabet, R).tolist() for R in LENGTHS]
    hyps, ref_idx = [], []
    pairs = [(r, H) for r in range(len(LENGTHS)) for H in [0] + LENGTHS]
    big = (len(LENGTHS) - 1, 257)
    pairs.remove(big)
    pairs = [big] + pairs + [big]
    for k, (r, H) in enumerate(pairs):
        if k % 2 == 0 and H:
            src = [t for t in refs[r] if rng.random() > 0.15] or [0]
            hyp = [(int(rng.integers(0, alphabet)) if rng.random() < 0.1 else src[j % len(src)]) for j in range(H)]
        else:
            hyp = rng.integers(0, alphabet, H).tolist()
        hyps.append(hyp)
        ref_idx.append(r)
    return hyps, refs, ref_idx, _host(hyps, refs, ref_idx)


@pytest.fixture(scope="module", params=[2, 5], ids=["alphabet2", "alphabet5"])
def sweep(request):
    return _sweep(request.param)


def _check(out, want, hyps, mode):
    assert out["counts"].tolist() == [list(c) for c, _ in want]
    assert out["ops"] == [o for _, o in want]
    labels = ["".join(rescore_ref.fold_labels(o, mode)) if h else "" for (_, o), h in zip(want, hyps)]
    assert out["labels"] == labels


@pytest.mark.parametrize("mode", ["SI", "SID"])
def test_edit_align_length_sweep(dev, sweep, mode):
    from emoasr_amd import ops
    hyps, refs, ref_idx, want = sweep
    out = ops.edit_align(hyps, refs, ref_idx=ref_idx, device=dev, want_ops=True, label_mode=mode)
    _check(out, want, hyps, mode)
    assert len(hyps) == 73 and len(hyps[0]) == len(hyps[-1]) == 257 and len(refs[ref_idx[0]]) == len(refs[ref_idx[-1]]) == 257


def test_edit_align_counts_alone(dev, sweep):
    """no op list and no labels asked for (the rescoring path), references by position"""
    from emoasr_amd import ops
    hyps, refs, ref_idx, want = sweep
    out = ops.edit_align(hyps[:9], [refs[r] for r in ref_idx[:9]], device=dev)
    assert out["counts"].tolist() == [list(c) for c, _ in want[:9]] and "ops" not in out and "labels" not in out


def test_edit_align_lds_and_workspace_sides(dev):
    """one pair on each side of the LDS capacity, for one strip and for three, in one batch with small pairs between them"""
    from emoasr_amd import lib, ops
    rng = np.random.default_rng(7)
    refs, hyps = [], []
    for R, H in THRESHOLD:
        ref = rng.integers(0, 3, R).tolist()
        refs += [ref, rng.integers(0, 3, 5).tolist()]
        hyps += [[ref[(j * R) // H] if rng.random() > 0.2 else int(rng.integers(0, 3)) for j in range(H)], rng.integers(0, 3, 4).tolist()]
        words = lib.size_query("emoasr_edit_align_ws_words", R, H)
        assert (words == 0) == ((R, H) in THRESHOLD[0::2])
    want = _host(hyps, refs, range(len(hyps)))
    out = ops.edit_align(hyps, refs, device=dev, want_ops=True, label_mode="SID")
    _check(out, want, hyps, "SID")


def test_edit_align_longest_pair_and_the_limit(dev):
    """4096 tokens a side run (identical sequences: all C; against the empty hypothesis: R - 1 deletions and one substitution, what
    compute_wer gives for any R); 4097 on either side is an error, not a truncation"""
    from emoasr_amd import lib, ops
    from emoasr_amd.metrics import compute_wer
    ref = (np.arange(4096) % 7).tolist()
    out = ops.edit_align([ref, [], ref[:4095]], [ref], ref_idx=[0, 0, 0], device=dev, want_ops=True, label_mode="SID")
    assert out["counts"].tolist() == [[0, 0, 0, 0], [1, 0, 4095, 4096], [0, 0, 1, 1]]
    assert out["ops"] == ["C" * 4096, "D" * 4095 + "S", "C" * 4095 + "D"]
    assert out["labels"] == ["C" * 4096, "", "C" * 4095]
    _, w = compute_wer([], ref[:9])
    assert "".join(w["error_list"]) == "D" * 8 + "S"
    long = [0] * 4097
    with pytest.raises(lib.EmoasrHipError, match="over the limit"):
        ops.edit_align([long], [ref], device=dev)
    with pytest.raises(lib.EmoasrHipError, match="over the limit"):
        ops.edit_align([ref], [long], device=dev)


def _grid_case(rng, U, single=()):
    n_rows = rng.integers(1, 6, U)
    n_rows[list(single)] = 1
    utt_off = np.concatenate([[0], np.cumsum(n_rows)])
    N = int(utt_off[-1])
    sa, sl = -rng.random(N) * 30, -rng.random(N) * 50
    ylen = rng.integers(1, 30, N)
    for u in range(0, U, 3):          # tied rows: equal scores and length, so every cell ties and the first row must win
        a, b = utt_off[u], utt_off[u + 1]
        if b - a >= 2:
            sa[b - 1], sl[b - 1], ylen[b - 1] = sa[a], sl[a], ylen[a]
    counts = rng.integers(0, 9, (N, 4)).astype(np.int32)
    return sa, sl, ylen.astype(np.int32), utt_off.astype(np.int32), counts


@pytest.mark.parametrize("U", [1, 63, 65, 300])
def test_rescore_grid(dev, U):
    from emoasr_amd import ops
    rng = np.random.default_rng(U)
    sa, sl, ylen, utt_off, counts = _grid_case(rng, U, single=(0, U // 2))
    lm_w, len_w = np.array([0.0, 0.1, 0.7, 1.0]), np.array([0.0, 1.0, 2.5])
    d = lambda a: torch.from_numpy(a).to(dev)
    best, totals = ops.rescore_grid(d(sa), d(sl), d(ylen), d(utt_off), d(counts), d(lm_w), d(len_w))
    want_best, want_totals = rescore_ref.grid_ref(sa, sl, ylen, utt_off, counts, lm_w, len_w)
    assert best.dtype == torch.int32 and totals.dtype == torch.int64
    assert np.array_equal(best.cpu().numpy(), want_best) and np.array_equal(totals.cpu().numpy(), want_totals)
    tied = [u for u in range(0, U, 3) if utt_off[u + 1] - utt_off[u] >= 2]
    assert tied or U == 1
    # the totals are cleared by the call itself (integer atomics: repeatable to the bit)
    best2, totals2 = ops.rescore_grid(d(sa), d(sl), d(ylen), d(utt_off), d(counts), d(lm_w), d(len_w))
    assert torch.equal(best, best2) and torch.equal(totals, totals2)


def test_rescore_grid_rounds_each_operation_once(dev):
    """scores chosen so that a fused multiply-add picks the other row: a = 1 + 2^-30, b = 1 - 2^-30, a * b = 1 - 2^-60 rounds to 1,
    so -1 + a * b is 0 when the product is rounded first and -2^-60 when it is fused; the rival row scores -2^-61"""
    from emoasr_amd import ops
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    sa, sl = np.array([-1.0, -2.0 ** -61]), np.array([b, 0.0])
    ylen, utt_off, counts = np.array([1, 1], np.int32), np.array([0, 2], np.int32), np.array([[1, 0, 0, 1], [0, 1, 0, 1]], np.int32)
    d = lambda x: torch.from_numpy(x).to(dev)
    best, totals = ops.rescore_grid(d(sa), d(sl), d(ylen), d(utt_off), d(counts), d(np.array([a])), d(np.array([0.0])))
    assert (np.float64(-1.0) + np.float64(a) * np.float64(b)) == 0.0
    assert best.tolist() == [[0]] and totals.tolist() == [[1, 0, 0]]
    want_best, _ = rescore_ref.grid_ref(sa, sl, ylen, utt_off, counts, [a], [0.0])
    assert want_best.tolist() == [[0]]


def test_rescore_grid_utterance_without_rows(dev):
    from emoasr_amd import ops
    d = lambda x: torch.from_numpy(x).to(dev)
    best, totals = ops.rescore_grid(d(np.array([-1.0])), d(np.array([-2.0])), d(np.array([3], np.int32)), d(np.array([0, 0, 1, 1], np.int32)),
                                    d(np.array([[2, 3, 4, 9]], np.int32)), d(np.array([0.5])), d(np.array([0.0, 1.0])))
    assert best.tolist() == [[-1, 0, -1]] * 2 and totals.tolist() == [[2, 3, 4]] * 2


# ---------------------------------------------------------------- end to end on the golden table
def test_grid_search_matches_the_reference(dev, g):
    from emoasr_amd import rescore
    df, dfref = tables(g)
    before = df.copy()
    table, best = rescore.grid_search(df, dfref, g["grid/lm_weights"], g["grid/len_weights"], device=dev)
    cells = [c for row in table for c in row]
    assert [wer for wer, _ in cells] == g["grid/wer"].tolist()
    assert [[w["n_sub"], w["n_ins"], w["n_del"], w["n_ref"]] for _, w in cells] == g["grid/totals"].tolist()
    assert all(w["wer"] == wer for wer, w in cells)
    assert [best["lm_weight"], best["len_weight"], best["wer"]] == g["grid/best"].tolist()
    k = int(np.argmax((g["grid/lm_weights"][:, None] == g["grid/best"][0]) & (g["grid/len_weights"][None, :] == g["grid/best"][1])))
    assert list(best["df_best"].index) == g["grid/winners"][k].tolist()
    assert list(best["df_best"].columns) == ["utt_id", "text", "token_id", "score_asr"]
    assert df.equals(before)
    # one cell at a time
    for cell, (a, b) in enumerate([(a, b) for a in range(3) for b in range(3)]):
        wer, w, df_best = rescore.rescore(df.copy(), dfref, g["grid/lm_weights"][a], g["grid/len_weights"][b], device=dev)
        assert wer == g["grid/wer"][cell] and list(df_best.index) == g["grid/winners"][cell].tolist()


def test_rescore_of_a_shuffled_table(dev, g):
    """an utterance's rows are no longer contiguous and a tie goes to another row (the first of the table AS GIVEN): the winners
    are those of the reference's expression (groupby / idxmax) on the host, the counts those of the host compute_wers_df"""
    from emoasr_amd import rescore
    from emoasr_amd.metrics import compute_wers_df
    df, dfref = tables(g)
    shuffled = df.sample(frac=1.0, random_state=3)
    wl, wn = np.float64(0.3), np.float64(0.5)
    wer, w, df_best = rescore.rescore(shuffled, dfref, wl, wn, device=dev)
    host = shuffled.loc[shuffled.groupby("utt_id")["score"].idxmax(), :]       # (rescore left the score column, as the reference does)
    _, hw = compute_wers_df(host, dfref)
    assert list(df_best.index) == list(host.index)
    assert [w[k] for k in ("n_sub", "n_ins", "n_del", "n_ref")] == [hw[k] for k in ("n_sub", "n_ins", "n_del", "n_ref")]


def test_rescore_keeps_utterances_the_reference_does_not_list(dev, g):
    """rows of df whose utt_id is not in dfref get a winner in df_best (the reference's groupby keeps them) and count nothing"""
    import pandas as pd
    from emoasr_amd import rescore
    df, dfref = tables(g)
    extra = pd.DataFrame({"utt_id": ["zzz-b", "aaa-a", "zzz-b", "aaa-a"], "score_asr": [-3.0, -1.0, -2.0, -1.0], "score_lm": [-1.0, -5.0, -9.0, -5.0],
                          "token_id": ["3 4", "5", "6 7 3", "4"], "text": ["w0 w1", "w2", "w3 w4 w0", "w1"], "reftext": ["w0"] * 4})
    both = pd.concat([df.iloc[:70], extra, df.iloc[70:]], ignore_index=True)
    table, best = rescore.grid_search(both, dfref, g["grid/lm_weights"], g["grid/len_weights"], device=dev)
    cells = [c for row in table for c in row]
    assert [wer for wer, _ in cells] == g["grid/wer"].tolist()
    assert [[w["n_sub"], w["n_ins"], w["n_del"], w["n_ref"]] for _, w in cells] == g["grid/totals"].tolist()
    wl, wn = np.float64(0.3), np.float64(0.5)
    wer, w, df_best = rescore.rescore(both, dfref, wl, wn, device=dev)
    host = both.loc[both.groupby("utt_id")["score"].idxmax(), :]
    assert list(df_best.index) == list(host.index) and {"aaa-a", "zzz-b"} <= set(df_best["utt_id"])
    assert df_best["utt_id"].tolist() == sorted(df_best["utt_id"]) and wer == g["grid/wer"][4]


def test_bad_inputs_are_refused_on_the_host(dev):
    """an empty reference (compute_wer divides by its length) and offsets that do not cover the rows never reach a kernel"""
    from emoasr_amd import ops
    with pytest.raises(ValueError, match="empty reference"):
        ops.edit_align([[1, 2], [3]], [[1], []], device=dev)
    d = lambda x: torch.from_numpy(x).to(dev)
    args = [d(np.array([-1.0, -2.0])), d(np.array([-2.0, -1.0])), d(np.array([3, 1], np.int32))]
    tail = [d(np.array([[2, 3, 4, 9], [0, 0, 0, 0]], np.int32)), d(np.array([0.5])), d(np.array([0.0]))]
    for off in ([0, 3], [1, 2], [0, 2, 1, 2]):
        with pytest.raises(ValueError, match="utt_off"):
            ops.rescore_grid(*args, d(np.array(off, np.int32)), *tail)
    best, _ = ops.rescore_grid(*args, d(np.array([0, 2], np.int32)), *tail)
    assert best.tolist() == [[0]]


def test_alignment_matches_the_reference(dev, g):
    from emoasr_amd import align_hyps
    df, dfref = tables(g)
    for mode in ("SI", "SID"):
        out = align_hyps.alignment(df, dfref, align_type=mode, device=dev)
        assert list(out.columns) == ["utt_id", "score_asr", "token_id", "text", "reftext", "error_label"]
        assert out["error_label"].tolist() == g["align/" + mode].tolist()
        assert out["token_id"].tolist() == df["token_id"].tolist() and out["score_asr"].tolist() == df["score_asr"].tolist()
    rows = g["align/SID_len3to6_rows"]
    out = align_hyps.alignment(df, dfref, len_min=3, len_max=6, device=dev)
    assert out["error_label"].tolist() == g["align/SID"][rows].tolist() and out["utt_id"].tolist() == df["utt_id"][rows].tolist()


def test_compute_wers_on_the_device(dev, g):
    from emoasr_amd.metrics import compute_wers, compute_wers_df
    df, dfref = tables(g)
    best = df.iloc[g["grid/winners"][4]]
    assert compute_wers_df(best, dfref, device=dev) == compute_wers_df(best, dfref)
    assert compute_wers_df(df, device=dev) == compute_wers_df(df)
    assert compute_wers_df(df, cer=True, device=dev) == compute_wers_df(df, cer=True)
    hyps, refs = [t.split() for t in df["text"]], [t.split() for t in df["reftext"]]
    assert compute_wers(hyps, refs, device=dev) == compute_wers(hyps, refs)


def test_compute_wers_on_the_device_with_empty_hypotheses(dev, g):
    """an empty hypothesis is the WORD "<dummy>": with cer=True its seven characters are aligned (and can match), and as a word it
    matches a reference word spelt that way -- on the device as on the host"""
    from emoasr_amd.metrics import compute_wers, compute_wers_df
    df, dfref = tables(g)
    best = df.iloc[g["grid/winners"][4]]
    short = best[~best["utt_id"].isin(["utt-003", "utt-020"])]              # two more utterances without a hypothesis (utt-007 has none)
    for cer in (False, True):
        assert compute_wers_df(short, dfref, cer=cer, device=dev) == compute_wers_df(short, dfref, cer=cer)
    nan = df.copy()
    nan.loc[[2, 50], "text"] = np.nan                                        # a NaN text counts as empty
    assert compute_wers_df(nan, cer=True, device=dev) == compute_wers_df(nan, cer=True)
    hyps = [[], ["ab"], [], [], ["x", "y"]]
    refs = [["ab"], ["ab", "c"], ["dummy", "x"], ["<dummy>", "m"], ["x"]]
    for cer in (False, True):
        assert compute_wers(hyps, refs, cer=cer, device=dev) == compute_wers(hyps, refs, cer=cer)
    assert compute_wers(hyps[:1], refs[:1], cer=True)[1]["n_ins"] == 5 and compute_wers(hyps[3:4], refs[3:4])[1]["n_sub"] == 0


def _lm(name, cfg, dev):
    from emoasr_amd.modeling.lm import LM
    z = golden_npz(name)
    lm = LM(SimpleNamespace(**cfg), compute_dtype=torch.float32)
    lm.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd/")})
    return lm.to(dev).eval()


@pytest.mark.parametrize("kind", ["electra", "bert"])
def test_score_lm_batches_like_direct_calls(dev, g, kind, monkeypatch):
    """41 rows in batches of 8: five full calls and a last call of ONE row, which is where ELECTRA's score changes sign
    (LM.score); the column equals direct LM.score calls over the same row groups"""
    from emoasr_amd import rescore
    from tests.test_bert_cpu import BERT_CFG
    from tests.test_electra_cpu import ELECTRA_CFG
    lm = _lm("electra_tiny", ELECTRA_CFG, dev) if kind == "electra" else _lm("bert_tiny", BERT_CFG, dev)
    df, _ = tables(g)
    df = df.iloc[:41].drop(columns="score_lm")
    monkeypatch.setattr(rescore, "BATCH_SIZE", 8)
    out = rescore.score_lm(df, lm, dev, mask_id=39)
    want = []
    for b0 in range(0, len(df), 8):
        ys = [torch.tensor([int(t) for t in s.split()]) for s in df["token_id"][b0:b0 + 8]]
        pad = torch.nn.utils.rnn.pad_sequence(ys, batch_first=True).to(dev)
        want += lm.score(pad, torch.tensor([len(y) for y in ys]).to(dev), batch_size=8)
    assert out is df and out["score_lm"].tolist() == want and len(want) == 41
    if kind == "electra":
        assert all(v < 0 for v in want[:40]) and want[40] > 0
