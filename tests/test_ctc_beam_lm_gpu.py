"""The fused (LM) batched CTC prefix beam search on the device (csrc/ctc_beam_lm.hip) against the host search
(csrc/ctc_beam_host.hip: emoasr_ctc_beam_new / _step / _scores) over the same log-probabilities, top-k labels and LM rows: the same
hypotheses in the same order, scores within 1e-9 * max(1, |score|).

The test drives init / frame / finish itself.  After each launch it reads the records and writes table_lm(prefix) (tests/
ctc_beam_lm_ref.py) into the pool row each record names, so the device reads exactly the f32 rows the host search is fed as lm_lp.

The bar is that of tests/test_ctc_beam_batch_gpu.py: device and host exp / log are each good to a couple of ulp, a value passes at
most three lse2 per frame, the LM term is built from exactly rounded products and sums on both sides, |score| <~ 12 T + the LM
term; at T <= 48 that bounds the drift near 1e-11.  Exact order is demanded because every case has a smallest non-zero gap between
adjacent totals above 1e-4 (tests/test_ctc_beam_lm_cpu.py).  Every output, the record list, the workspace and the pool lie between
guard words in every run here."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ctc_beam_lm_ref as M
from tests import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
_ROWS = {}


def table_row(V, prefix):
    """table_lm(V)(prefix), computed once per prefix and shared by the device side and the host side"""
    key = (V, tuple(prefix))
    if key not in _ROWS:
        _ROWS[key] = M.table_lm(V)(prefix)
    return _ROWS[key]


def host_search(lp, top, W, lw, lmw):
    """emoasr_ctc_beam_new / _step / _scores over the rows, lm_lp from the table LM's f32 rows -> (hyps, scores)"""
    from emoasr_amd import lib
    L = lib.load()
    L.emoasr_ctc_beam_new.restype = ctypes.c_void_p
    L.emoasr_ctc_beam_new.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 2
    L.emoasr_ctc_beam_free.argtypes = [ctypes.c_void_p]
    L.emoasr_ctc_beam_free.restype = None
    L.emoasr_ctc_beam_step.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    L.emoasr_ctc_beam_scores.argtypes = [ctypes.c_void_p] * 2
    V = lp.shape[1] if lp.ndim == 2 else 0
    h = L.emoasr_ctc_beam_new(W, R.BLANK, R.EOS, lw, lmw)
    parent, tok = np.zeros(W, np.int32), np.zeros(W, np.int32)
    live = [(R.EOS,)]
    for t in range(lp.shape[0]):
        lm_lp = np.ascontiguousarray(np.stack([table_row(V, p)[top[t]] for p in live]).astype(np.float64)) if lmw > 0 else None
        n = L.emoasr_ctc_beam_step(h, lp[t].ctypes.data, top[t].ctypes.data, top.shape[1], None if lm_lp is None else lm_lp.ctypes.data,
                                   parent.ctypes.data, tok.ctypes.data)
        assert n > 0
        live = [live[parent[i]] + ((int(tok[i]),) if tok[i] >= 0 else ()) for i in range(n)]
    scores = np.zeros(len(live))
    assert L.emoasr_ctc_beam_scores(h, scores.ctypes.data) == len(live)
    L.emoasr_ctc_beam_free(h)
    return [list(p) for p in live], scores.tolist()


def _guarded(dev, n, dtype, fill):
    """n elements between two guard zones"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def drive(dev, utts, searches, W, V, slots=None, top_edit=None, utt_edit=None, W_call=None):
    """init, then per frame one launch and the table LM over its records, then finish.  utts = [(lp, top)], searches = [(utterance,
    lm_weight, len_weight)].  -> ([(hyps, scores) | None (out_n = -1)] per search, status, raw outputs).  top_edit / utt_edit change
    what the device is given (a bad label, a bad utterance index), W_call the beam width of the calls."""
    from emoasr_amd import lib, ops
    k, S, B = min(W, V), len(searches), len(utts)
    lens = [u[0].shape[0] for u in utts]
    T = max(lens + [0])
    slots = ops.ctc_beam_lm_slots(W) if slots is None else slots
    Wc = W if W_call is None else W_call
    top_h = np.concatenate([u[1].reshape(-1, k) for u in utts])
    if top_edit is not None:
        top_h = top_h.copy()
        top_h[top_edit[0], top_edit[1]] = top_edit[2]
    lp = torch.from_numpy(np.concatenate([u[0].reshape(-1, V) for u in utts])).to(dev)
    top = torch.from_numpy(top_h).to(dev)
    row_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(dev)
    utt_h = [s[0] for s in searches]
    if utt_edit is not None:
        utt_h[utt_edit[0]] = utt_edit[1]
    utt = torch.tensor(utt_h, dtype=torch.int32).to(dev)
    lmw = torch.tensor([s[1] for s in searches], dtype=torch.float64).to(dev)
    lenw = torch.tensor([s[2] for s in searches], dtype=torch.float64).to(dev)
    ws_bytes = lib.size_query("emoasr_ctc_beam_lm_ws_bytes", S, T, W)
    cap = S * W
    g_ws, ws = _guarded(dev, ws_bytes // 8, torch.int64, -7)
    g_rec, rec = _guarded(dev, 6 * cap, torch.int32, -7)
    g_cnt, cnt = _guarded(dev, 1, torch.int32, -7)
    g_pool, pool = _guarded(dev, S * slots * V, torch.float32, -7.0)
    g_tok, tok = _guarded(dev, S * W * (T + 1), torch.int32, -7)
    g_len, ln = _guarded(dev, S * W, torch.int32, -7)
    g_sc, sc = _guarded(dev, S * W, torch.float64, -7.0)
    g_n, n_out = _guarded(dev, S, torch.int32, -7)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    guards = (g_ws, g_rec, g_cnt, g_pool, g_tok, g_len, g_sc, g_n)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pool2 = pool.view(S * slots, V)
    toks = {}

    def lm_pass():
        n = int(cnt.item())
        assert 0 <= n <= cap
        if n == 0:
            return
        r = rec.view(6, cap)[:, :n].cpu().numpy()
        rows = []
        for s, node, parent, v, src, dst in r.T.tolist():
            assert s * slots <= dst < (s + 1) * slots and (src == -1 if parent < 0 else s * slots <= src < (s + 1) * slots)
            toks[(s, node)] = toks[(s, parent)] + (v,) if parent >= 0 else (v,)
            rows.append(table_row(V, toks[(s, node)]))
        assert len(set(r[5].tolist())) == n                      # no two new prefixes share a row
        pool2.index_copy_(0, torch.from_numpy(r[5].astype(np.int64)).to(dev), torch.from_numpy(np.stack(rows)).to(dev))

    with torch.cuda.device(dev):
        lib.call("emoasr_ctc_beam_lm_init", S, B, Wc, p(row_off), p(utt), R.EOS, T, slots, p(ws), ws_bytes, p(rec), cap, p(cnt),
                 p(status), None)
        lm_pass()
        for t in range(T):
            lib.call("emoasr_ctc_beam_lm_frame", S, B, V, Wc, k, t, p(lp), V, p(row_off), p(top), p(utt), p(lmw), p(lenw), R.BLANK,
                     R.EOS, T, p(pool), V, p(ws), ws_bytes, p(rec), cap, p(cnt), p(status), None)
            lm_pass()
        lib.call("emoasr_ctc_beam_lm_finish", S, Wc, T, R.EOS, p(tok), p(ln), p(sc), p(n_out), p(ws), ws_bytes, None)
    torch.cuda.synchronize()
    for g in guards:
        assert bool((g[:GUARD] == -7).all()) and bool((g[-GUARD:] == -7).all())
    tok_h, ln_h = tok.view(S, W, T + 1).cpu().numpy(), ln.view(S, W).cpu().numpy()
    sc_h, n_h = sc.view(S, W).cpu().numpy(), n_out.cpu().numpy()
    out = [None if n_h[s] < 0 else ([tok_h[s, i, :ln_h[s, i]].tolist() for i in range(n_h[s])], sc_h[s, :n_h[s]].tolist())
           for s in range(S)]
    return out, int(status.item()), (tok_h, ln_h, sc_h, n_h)


def same_as_host(got, want):
    assert got is not None and got[0] == want[0], (got, want)
    worst = 0.0
    for a, b in zip(got[1], want[1]):
        worst = max(worst, abs(a - b) / max(1.0, abs(b)))
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (a, b)
    return worst


_ID = lambda c: "V%d-W%d-T%d-s%d" % (c[0], c[1], c[2], c[5])


@pytest.mark.parametrize("case", R.expand(R.ALL_CASES), ids=_ID)
def test_every_case_equals_the_host_search(dev, case):
    """the case tables of the search without an LM (folds of both kinds, a length bonus, exact ties of the acoustic rows, V = 1 000,
    W = 32, a single frame), each with lm_weight 0.3 and 1.0 as two searches of one launch sequence"""
    V, W, T, scale, lw, seed, tie = case
    lp, top = R.make_rows(seed, T, V, scale, W, tie)
    out, status, _ = drive(dev, [(lp, top)], [(0, 0.3, lw), (0, 1.0, lw)], W, V)
    assert status == 0
    for got, lmw in zip(out, (0.3, 1.0)):
        worst = same_as_host(got, host_search(lp, top, W, lw, lmw))
        print(f"V={V} W={W} T={T} seed={seed} lm_weight={lmw}: {len(got[0])} hypotheses, largest score difference {worst}")
        assert len(got[0]) == (5 if (V, T) == (5, 1) else W)


@pytest.mark.parametrize("case", R.expand(R.ALL_CASES), ids=_ID)
def test_lm_weight_zero_is_the_search_without_an_lm_bit_for_bit(dev, case):
    """one fused search with lm_weight = 0.0 (its pool holds finite rows, which it must not read into a score) against
    emoasr_ctc_beam_batch over the same rows: tokens, lengths, counts and scores are equal as bits, and so is everything neither
    wrote.  Both kernels run the frame of csrc/ctc_beam_step.h; this is what keeps them doing so."""
    from emoasr_amd import lib
    V, W, T, scale, lw, seed, tie = case
    lp, top = R.make_rows(seed, T, V, scale, W, tie)
    out, status, (f_tok, f_len, f_sc, f_n) = drive(dev, [(lp, top)], [(0, 0.0, lw)], W, V)
    assert status == 0 and out[0] is not None
    d_lp, d_top = torch.from_numpy(lp).to(dev), torch.from_numpy(top).to(dev)
    row_off = torch.tensor([0, T], dtype=torch.int32, device=dev)
    ws_bytes = lib.size_query("emoasr_ctc_beam_batch_ws_bytes", 1, T, W)
    g_ws, ws = _guarded(dev, ws_bytes // 8, torch.int64, -7)
    g_tok, tok = _guarded(dev, W * (T + 1), torch.int32, -7)
    g_len, ln = _guarded(dev, W, torch.int32, -7)
    g_sc, sc = _guarded(dev, W, torch.float64, -7.0)
    g_n, n_out = _guarded(dev, 1, torch.int32, -7)
    b_status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        lib.call("emoasr_ctc_beam_batch", 1, V, W, min(W, V), p(d_lp), V, p(row_off), p(d_top), R.BLANK, R.EOS, lw, T, p(tok), p(ln),
                 p(sc), p(n_out), p(ws), ws_bytes, p(b_status), None)
    torch.cuda.synchronize()
    for g in (g_ws, g_tok, g_len, g_sc, g_n):
        assert bool((g[:GUARD] == -7).all()) and bool((g[-GUARD:] == -7).all())
    assert int(b_status.item()) == 0
    assert n_out.cpu().numpy().tolist() == f_n.tolist() == [5 if (V, T) == (5, 1) else W]
    assert np.array_equal(ln.view(1, W).cpu().numpy(), f_len)
    assert np.array_equal(tok.view(1, W, T + 1).cpu().numpy(), f_tok)
    assert np.array_equal(sc.view(torch.int64).view(1, W).cpu().numpy(), f_sc.view(np.int64))


def test_mixed_cells_of_two_utterances(dev):
    """six searches over two utterances (32 and 20 frames) with mixed weights in one launch sequence: each equals the host search;
    the lm_weight = 0 cells are bit-equal to emoasr_ctc_beam_batch; every search is bit-equal to itself run alone"""
    from emoasr_amd import ops
    V, W = 6, 8
    utts = [R.make_rows(8, 32, V, 1.0, W), tuple(a[:20] for a in R.make_rows(49, 32, V, 1.0, W))]
    searches = [(0, 0.0, 0.0), (0, 0.3, 0.0), (1, 1.0, 0.5), (0, 0.3, 0.3), (1, 0.0, 0.5), (1, 0.3, 0.0)]
    out, status, _ = drive(dev, utts, searches, W, V)
    assert status == 0
    lp = torch.from_numpy(np.concatenate([u[0] for u in utts])).to(dev)
    top = torch.from_numpy(np.concatenate([u[1] for u in utts])).to(dev)
    row_off = torch.tensor([0, 32, 52], dtype=torch.int32, device=dev)
    for s, (u, lmw, lw) in enumerate(searches):
        same_as_host(out[s], host_search(utts[u][0], utts[u][1], W, lw, lmw))
        (alone,), st1, _ = drive(dev, [utts[u]], [(0, lmw, lw)], W, V)
        assert st1 == 0 and alone == out[s]                           # (lists of ints and of doubles: bit-equal)
        if lmw == 0.0:
            b_tok, b_len, b_sc, b_n, b_st = ops.ctc_beam_batch(lp, row_off, top, W, R.BLANK, R.EOS, lw)
            assert int(b_st.item()) == 0 and int(b_n[u]) == len(out[s][0])
            b_tok, b_len = b_tok.cpu().numpy(), b_len.cpu().numpy()
            assert [b_tok[u, i, :b_len[u, i]].tolist() for i in range(len(out[s][0]))] == out[s][0]
            assert b_sc[u, :len(out[s][1])].cpu().tolist() == out[s][1]


def test_ragged_batch(dev):
    """utterances of 0, 1, 7, 32 and 33 frames, two cells each, in one launch sequence: every search gets what the host search
    gives; the empty utterance is the single prefix (<eos>), 0.0"""
    V, W = 5, 3
    lp, top = R.make_rows(19, 33, V, 1.0, W)
    utts = [(lp[:n], top[:n]) for n in (0, 1, 7, 32, 33)]
    searches = [(u, lmw, lw) for u in range(5) for lmw, lw in ((0.3, 0.0), (1.0, 0.2))]
    out, status, (_, _, _, n) = drive(dev, utts, searches, W, V)
    assert status == 0 and n.tolist() == [1, 1, 3, 3, 3, 3, 3, 3, 3, 3]
    assert out[0] == ([[R.EOS]], [0.0]) and out[1] == ([[R.EOS]], [0.0])
    for got, (u, lmw, lw) in zip(out, searches):
        same_as_host(got, host_search(utts[u][0], utts[u][1], W, lw, lmw))


def test_a_beam_over_the_limit_is_an_error(dev):
    from emoasr_amd import lib
    lp, top = R.make_rows(0, 4, 40, 3.0, 32)
    with pytest.raises(lib.EmoasrHipError, match="outside 1..32"):
        drive(dev, [(lp, top)], [(0, 0.3, 0.0)], 32, 40, W_call=33)
    # (drive checks nothing after the error; the calls one by one, every buffer between guards and untouched)
    S, T, V, W = 1, 4, 40, 33
    bufs = [torch.full((4096,), -7, dtype=torch.int32, device=dev) for _ in range(4)]
    out, ws, rec, pool = bufs
    wts = torch.zeros(2, dtype=torch.float64, device=dev)
    ids = torch.zeros(8, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    d_lp, d_top = torch.from_numpy(lp).to(dev), torch.from_numpy(top).to(dev)
    for Wb in (33, 0):
        with pytest.raises(lib.EmoasrHipError):
            lib.call("emoasr_ctc_beam_lm_init", S, 1, Wb, p(ids), p(ids), R.EOS, T, 66, p(ws), 4 * ws.numel(), p(rec), 64, p(rec), p(ids),
                     None)
        with pytest.raises(lib.EmoasrHipError):
            lib.call("emoasr_ctc_beam_lm_frame", S, 1, V, Wb, 32, 0, p(d_lp), V, p(ids), p(d_top), p(ids), p(wts), p(wts), R.BLANK, R.EOS,
                     T, p(pool), V, p(ws), 4 * ws.numel(), p(rec), 64, p(rec), p(ids), None)
        with pytest.raises(lib.EmoasrHipError):
            lib.call("emoasr_ctc_beam_lm_finish", S, Wb, T, R.EOS, p(out), p(out), p(out), p(out), p(ws), 4 * ws.numel(), None)
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs) and int(ids.abs().sum().item()) == 0


def test_refusals(dev):
    """a search that names utterance B, a label outside [0, V) and a pool share of 2 rows: the searches concerned are retired
    (out_n = -1, their status bit), their output rows stay untouched, the others are as in the clean run, the guards hold"""
    V, W, T = 6, 8, 32
    utts = [R.make_rows(s, T, V, 1.0, W) for s in (8, 49)]
    searches = [(0, 0.3, 0.0), (1, 0.3, 0.0), (0, 1.0, 0.1), (1, 0.0, 0.0)]
    clean, status, _ = drive(dev, utts, searches, W, V)
    assert status == 0 and all(c is not None for c in clean)
    # utt[2] = B
    out, status, (tok, ln, sc, n) = drive(dev, utts, searches, W, V, utt_edit=(2, 2))
    assert status == 16 and n.tolist() == [W, W, -1, W]
    assert bool((tok[2] == -7).all()) and bool((ln[2] == -7).all()) and bool((sc[2] == -7.0).all())
    assert [out[s] for s in (0, 1, 3)] == [clean[s] for s in (0, 1, 3)]
    out, status, (_, _, _, n) = drive(dev, utts, searches, W, V, utt_edit=(0, -1))
    assert status == 16 and n.tolist() == [-1, W, W, W] and out[1:] == clean[1:]
    # a label >= V in the top-k of utterance 1 at frame 11: its two searches are retired there
    out, status, (tok, ln, sc, n) = drive(dev, utts, searches, W, V, top_edit=(T + 11, 2, V))
    assert status == 1 and n.tolist() == [W, -1, W, -1]
    assert bool((tok[[1, 3]] == -7).all()) and bool((ln[[1, 3]] == -7).all()) and bool((sc[[1, 3]] == -7.0).all())
    assert [out[s] for s in (0, 2)] == [clean[s] for s in (0, 2)]
    out, status, (_, _, _, n) = drive(dev, utts, searches, W, V, top_edit=(3, 0, -1))
    assert status == 1 and n.tolist() == [-1, W, -1, W]
    # two rows per search: the root holds one, the first frame with two new prefixes finds the free list empty
    out, status, (tok, ln, sc, n) = drive(dev, utts, searches, W, V, slots=2)
    assert status == 32 and n.tolist() == [-1] * 4 and out == [None] * 4
    assert bool((tok == -7).all()) and bool((ln == -7).all()) and bool((sc == -7.0).all())
    # 2 W rows are enough (the bound of the design), the result does not depend on the share
    out, status, _ = drive(dev, utts, searches, W, V, slots=2 * W)
    assert status == 0 and out == clean
