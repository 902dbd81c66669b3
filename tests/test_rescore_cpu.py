"""N-best rescoring and error-label alignment without a GPU: the restatements the GPU tests compare against (tests/rescore_ref.py,
emoasr_amd.metrics.compute_wer) are held to the reference's own outputs (tests/golden/rescore.npz: tests/golden/
make_golden_rescore.py), exactly -- everything here is integers, strings and bit-specified float64 -- and the new entry points are
declared, exported, bound and importable."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import rescore_ref
from tests.util import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("emoasr_edit_align", "emoasr_rescore_grid", "emoasr_edit_align_ws_words", "emoasr_edit_align_lds_words")


@pytest.fixture(scope="module")
def g():
    return golden_npz("rescore")


def tables(g):
    import pandas as pd
    df = pd.DataFrame({k: g["hyp/" + k] for k in ("utt_id", "score_asr", "score_lm", "token_id", "text", "reftext")})
    dfref = pd.DataFrame({k: g["ref/" + k] for k in ("utt_id", "token_id", "text")})
    return df, dfref


def host_alignments(g):
    """metrics.compute_wer of every row of the golden table against its reference (token ids) -> [(counts, ops)]"""
    from emoasr_amd.metrics import compute_wer
    id2ref = {u: t.split() for u, t in zip(g["ref/utt_id"], g["ref/token_id"])}
    out = []
    for u, t in zip(g["hyp/utt_id"], g["hyp/token_id"]):
        _, w = compute_wer(t.split(), id2ref[u])
        out.append(((w["n_sub"], w["n_ins"], w["n_del"], w["n_sub"] + w["n_ins"] + w["n_del"]), "".join(w["error_list"])))
    return out


def test_compute_wer_reproduces_the_reference(g):
    from emoasr_amd.metrics import compute_wer
    got = host_alignments(g)
    assert [o for _, o in got] == g["wer/ops"].tolist()
    assert np.array_equal(np.array([c for c, _ in got], np.int32), g["wer/counts"])
    _, w = compute_wer([], g["ref/token_id"][7].split())
    assert "".join(w["error_list"]) == str(g["wer/empty_ops"])
    assert [w["n_sub"], w["n_ins"], w["n_del"]] == g["wer/empty_counts"].tolist()


@pytest.mark.parametrize("mode", ["SI", "SID"])
def test_label_fold_reproduces_the_reference(g, mode):
    got = [" ".join(rescore_ref.fold_labels(o, mode)) for o in g["wer/ops"]]
    assert got == g["align/" + mode].tolist()
    assert all(len(lab.split()) == len(t.split()) for lab, t in zip(got, g["hyp/token_id"]))


def test_sid_quirk_is_kept(g):
    """a deletion after a C vanishes; only a deletion with no C before it marks the next C"""
    fold = lambda o: "".join(rescore_ref.fold_labels(o, "SID"))
    assert [fold(o) for o in ("CDC", "DC", "SDC", "CDSDC", "DDCC", "CDD", "IDC", "DCDC")] == ["CC", "D", "SD", "CSD", "DC", "C", "ID", "DD"]
    # the fixture holds both kinds, and the reference's own labels show them
    vanish = [i for i, o in enumerate(g["wer/ops"]) if re.fullmatch(r"C+D+C*", o)]
    marked = [i for i, o in enumerate(g["wer/ops"]) if re.match(r"D+C", o)]
    assert len(vanish) >= 3 and len(marked) >= 3
    assert all("D" not in g["align/SID"][i] for i in vanish) and all(g["align/SID"][i].startswith("D") for i in marked)


def test_grid_restatement_reproduces_the_reference(g):
    """grid_ref over the golden table (word-level counts from metrics.compute_wer, one empty hypothesis for the utterance without
    rows) gives the reference's winners, totals and WER in every cell"""
    from emoasr_amd.metrics import compute_wer
    df, dfref = tables(g)
    utt_of = {u: k for k, u in enumerate(dfref["utt_id"])}
    rows = [[] for _ in utt_of]
    for k, u in enumerate(df["utt_id"]):
        rows[utt_of[u]].append(k)
    src, utt_off = [], [0]
    for r in rows:
        src += r or [-1]
        utt_off.append(len(src))
    counts, sa, sl, yl = [], [], [], []
    for k, u in zip(src, np.repeat(np.arange(len(rows)), np.diff(utt_off))):
        hyp = df["text"][k].split() if k >= 0 else []
        _, w = compute_wer(hyp, dfref["text"][u].split())
        counts.append((w["n_sub"], w["n_ins"], w["n_del"]))
        sa.append(df["score_asr"][k] if k >= 0 else 0.0)
        sl.append(df["score_lm"][k] if k >= 0 else 0.0)
        yl.append(len(df["token_id"][k].split()) if k >= 0 else 0)
    best, totals = rescore_ref.grid_ref(sa, sl, yl, utt_off, counts, g["grid/lm_weights"], g["grid/len_weights"])
    n_ref = sum(len(t.split()) for t in dfref["text"])
    assert np.array_equal(totals, g["grid/totals"][:, :3]) and (g["grid/totals"][:, 3] == n_ref).all()
    assert ((totals.sum(axis=1) / n_ref) * 100).tolist() == g["grid/wer"].tolist()
    src = np.array(src)
    for cell in range(len(best)):
        winners = src[best[cell]]
        assert np.array_equal(winners[winners >= 0], g["grid/winners"][cell])
    assert len(np.unique(best, axis=0)) > 3      # the weights move the winners


def test_new_symbols_are_declared_exported_and_bound():
    from emoasr_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "emoasr_hip.h")).read()
    handle = lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(handle, name), name
    assert len(lib.SIGNATURES["emoasr_edit_align"]) == 18 and len(lib.SIGNATURES["emoasr_rescore_grid"]) == 14
    assert callable(ops.edit_align) and callable(ops.rescore_grid)
    assert "rescore.hip" in __import__("emoasr_amd.build", fromlist=["SOURCES"]).SOURCES
    # the workspace rule: nothing up to the LDS capacity, the code words past it, -1 over the limit
    cap = lib.size_query("emoasr_edit_align_lds_words")
    assert lib.size_query("emoasr_edit_align_ws_words", 1985, 1) == 0 and 2 * (1985 + 63) == cap
    assert lib.size_query("emoasr_edit_align_ws_words", 1986, 1) == 2 * (1986 + 63)
    assert lib.size_query("emoasr_edit_align_ws_words", 257, 257) == 0
    assert lib.size_query("emoasr_edit_align_ws_words", 620, 130) == 2 * 3 * (620 + 63)
    assert lib.size_query("emoasr_edit_align_ws_words", 4096, 0) == 2 * (4096 + 63)
    assert lib.size_query("emoasr_edit_align_ws_words", 4097, 1) == -1 and lib.size_query("emoasr_edit_align_ws_words", 1, 4097) == -1


def test_modules_keep_the_reference_signatures():
    from emoasr_amd import align_hyps, metrics, rescore
    assert list(inspect.signature(rescore.score_lm).parameters) == ["df", "model", "device", "mask_id", "vocab", "num_samples"]
    assert list(inspect.signature(rescore.rescore).parameters)[:4] == ["df", "dfref", "lm_weight", "len_weight"]
    assert list(inspect.signature(rescore.grid_search).parameters)[:4] == ["df", "dfref", "lm_weights", "len_weights"]
    sig = inspect.signature(align_hyps.alignment)
    assert list(sig.parameters)[:5] == ["dfhyp", "dfref", "align_type", "len_min", "len_max"]
    assert [sig.parameters[k].default for k in ("align_type", "len_min", "len_max")] == ["SID", 1, 256]
    assert rescore.BATCH_SIZE == 100
    for fn in (metrics.compute_wers, metrics.compute_wers_df):
        assert inspect.signature(fn).parameters["device"].default is None


def test_host_wer_is_unchanged_by_the_device_argument(g):
    """device=None is the host loop: the totals of the reference's first cell's winners"""
    from emoasr_amd.metrics import compute_wers_df
    df, dfref = tables(g)
    wer, w = compute_wers_df(df.iloc[g["grid/winners"][0]], dfref)
    assert [w["n_sub"], w["n_ins"], w["n_del"], w["n_ref"]] == g["grid/totals"][0].tolist()
    assert wer == pytest.approx(g["grid/wer"][0], rel=1e-15)


def test_command_lines_take_the_reference_arguments():
    from emoasr_amd import align_hyps, rescore
    a = rescore.build_parser().parse_args(
        ["nbest.tsv", "-ref", "ref.tsv", "-lm_conf", "lm.yaml", "-lm_ep", "30-40", "--lm_tag", "bert", "--lm_min", "0.1", "--lm_max",
         "0.9", "--lm_step", "0.2", "--len_min", "1", "--len_max", "3", "--len_step", "0.5", "--runtime", "--runtime_num_samples",
         "5", "--runtime_num_repeats", "2", "--wavtime_factor", "100", "--debug", "--cpu"])
    assert (a.tsv_path, a.ref, a.lm_conf, a.lm_ep, a.lm_tag) == ("nbest.tsv", "ref.tsv", "lm.yaml", "30-40", "bert")
    assert (a.lm_min, a.lm_max, a.lm_step, a.len_min, a.len_max, a.len_step) == (0.1, 0.9, 0.2, 1.0, 3.0, 0.5)
    assert a.runtime and a.debug and a.cpu and (a.runtime_num_samples, a.runtime_num_repeats, a.wavtime_factor) == (5, 2, 100.0)
    d = rescore.build_parser().parse_args(["n.tsv", "-ref", "r.tsv", "-lm_conf", "c.yaml", "-lm_ep", "3"])
    assert (d.lm_min, d.lm_max, d.lm_step, d.len_min, d.len_max, d.len_step) == (0, 1, 0.1, 0, 5, 1)
    assert (d.runtime_num_samples, d.runtime_num_repeats, d.wavtime_factor, d.lm_tag) == (20, 5, 1000, None)
    assert rescore.model_path("exp/lm/bert.yaml", "30-40") == os.path.join("exp/lm/bert", "checkpoints", "model.ep30-40")
    b = align_hyps.build_parser().parse_args(["nbest.tsv", "-ref", "ref.tsv", "--align_type", "SI", "--len_min", "2", "--len_max", "99"])
    assert (b.tsv_path, b.ref, b.align_type, b.len_min, b.len_max) == ("nbest.tsv", "ref.tsv", "SI", 2, 99)
    c = align_hyps.build_parser().parse_args(["nbest.tsv", "-ref", "ref.tsv"])
    assert (c.align_type, c.len_min, c.len_max) == ("SID", 1, 256)
    with pytest.raises(SystemExit):
        align_hyps.build_parser().parse_args(["nbest.tsv", "-ref", "ref.tsv", "--align_type", "DIS"])


def test_score_lm_early_return_lists_the_utterances(g):
    """num_samples > 0 (the --runtime mode): the ids of the utterances seen before the count is reached, no model call after it"""
    from emoasr_amd import rescore
    df, _ = tables(g)

    class Counting:
        calls = 0

        def score(self, ys, ylens, batch_size=None):
            Counting.calls += 1
            return [0.0] * len(ylens)

    prev, rescore.BATCH_SIZE = rescore.BATCH_SIZE, 1
    try:
        utt_ids = rescore.score_lm(df, Counting(), "cpu", num_samples=3)
    finally:
        rescore.BATCH_SIZE = prev
    assert utt_ids == ["utt-000", "utt-001", "utt-002"] and Counting.calls == 8      # (the reference's off-by-one: 2 utterances scored)
    assert "score_lm" in df and len(rescore.score_lm(df.drop(columns="score_lm"), Counting(), "cpu")) == len(df)
