"""The joint CTC / attention fusion grid on the GPU: every cell kernel bit for bit against its scalar twin
(the EXISTING entry points), the len_weight expansion against the update kernel, and the grid end to end on l3_tiny against
the batched search run cell by cell."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import joint_beam_ref as ref
from tests.test_joint_beam_batch_gpu import _DeviceUpdate, _count_ties
from tests.util import CONFIGS, LM_CFG, load_golden, lm_state

pytestmark = pytest.mark.gpu

CUT_FRAC = (0.6, 0.6)      # as tests/test_joint_beam_batch_gpu.py cuts its utterances


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# =========================================================================================== 1. cross-attention over cells
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,dk", [(2, 64), (4, 32), (1, 128)])
@pytest.mark.parametrize("W", [1, 3, 10, 17, 32])
def test_attn_step_cells_equals_the_grouped_kernel(dev, W, H, dk, dtype):
    """three utterances with 1 / 2 / 5 searches, frame counts around the tile: every row bit-equal to emoasr_attn_step_group run
    with one offset entry per search over replicated memory, with the default grouping (a last group is partial) and with one
    search per group; rows outside the launch keep their sentinel"""
    from emoasr_amd import ops
    dd, TK = H * dk, (32 if dk == 128 else 64)
    per_utt = (1, 2, 5)
    sutt = [u for u, n in enumerate(per_utt) for _ in range(n)]
    S, nb = len(sutt), len(sutt) * W
    for Ts in ((1, TK - 1, 2 * TK + 2), (TK + 1, 2 * TK + 2, 1)):
        gen = torch.Generator().manual_seed(W * 1000 + H * 10 + sum(Ts))
        offs = [0, Ts[0], Ts[0] + Ts[1], sum(Ts)]
        q = torch.randn(nb, dd, generator=gen).to(dtype).to(dev)
        kv = torch.randn(sum(Ts), 2 * dd, generator=gen).to(dtype).to(dev)
        moff = torch.tensor(offs, dtype=torch.int32, device=dev)
        # the twin: the memory of every search's utterance once per search
        rep = torch.cat([kv[offs[u]:offs[u + 1]] for u in sutt], 0).contiguous()
        roffs = [0]
        for u in sutt:
            roffs.append(roffs[-1] + Ts[u])
        want = ops.attn_step_group(q, rep, torch.tensor(roffs, dtype=torch.int32, device=dev), W, H)
        assert torch.isfinite(want.float()).all()
        for cpg in (None, 1):
            groups, most = ops.cell_groups(sutt, W, cpg)
            if cpg is None and W == 10:
                assert [n for _, n, _ in groups] == [10, 20, 30, 20]                    # a full group and partial ones
            out = torch.full((nb + 5, dd), 777.0, dtype=dtype, device=dev)
            ops.attn_step_cells(q, kv, moff, groups, most, H, out=out)
            assert torch.equal(out[:nb], want), (W, H, dk, Ts, cpg)
            assert (out[nb:] == 777.0).all()
            # a launch over the first two utterances' rows only: nothing beyond them is written
            sub = 3 * W
            g2, m2 = ops.cell_groups(sutt[:3], W, cpg)
            out2 = torch.full((nb, dd), 777.0, dtype=dtype, device=dev)
            ops.attn_step_cells(q[:sub], kv, moff, g2, m2, H, out=out2)
            assert torch.equal(out2[:sub], want[:sub]) and (out2[sub:] == 777.0).all()


def test_cell_group_refusals(dev):
    from emoasr_amd import lib, ops
    q = torch.zeros(8, 64, device=dev)
    moff = torch.tensor([0, 4, 8], dtype=torch.int32, device=dev)
    for bad in ([(0, 4, 0), (4, 4, 2)], [(0, 4, 0), (5, 3, 1)], [(0, 4, 0)], [(0, 4, 0), (4, 5, 1)]):
        with pytest.raises(lib.EmoasrHipError, match="cell groups"):
            ops.attn_step_cells(q, q.repeat(1, 2).contiguous(), moff, bad, 4, 2)
    with pytest.raises(lib.EmoasrHipError, match="1..32"):
        lib.call("emoasr_attn_step_cells", lib.F32, 1, 33, 8, 2, 64, 2, q.data_ptr(), q.data_ptr(), moff.data_ptr(), moff.data_ptr(),
                 q.data_ptr(), _stream())


# =========================================================================================== 2. scores + top-k, a weight per row
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [1, 6, 32])
@pytest.mark.parametrize("V", [40, 1031])
def test_beam_scores_topk_rows_equals_the_scalar_kernel(dev, V, k, dtype):
    from emoasr_amd import lib, ops
    M = 7
    gen = torch.Generator().manual_seed(V + k)
    dec = (3 * torch.randn(M, V, generator=gen)).to(dtype).to(dev)
    lm = (3 * torch.randn(M, V, generator=gen)).to(dev)
    dec[2, 5] = dec[2, 9]                                     # an exact tie inside a row (no LM: it survives)
    mus = np.array([0.0, 0.3, 1.0, 0.3, 0.0, 1.0, 0.3], dtype=np.float32)
    mu_row = torch.from_numpy(mus).to(dev)

    def scalar(lm_t, mu):
        vals = torch.empty(M, k, device=dev)
        idx = torch.empty(M, k, dtype=torch.int32, device=dev)
        at = torch.empty(M, k, device=dev)
        lib.call("emoasr_beam_scores_topk", ops.dt(dec), M, V, k, dec.data_ptr(), V, lm_t.data_ptr() if lm_t is not None else None,
                 V if lm_t is not None else 0, float(mu), vals.data_ptr(), idx.data_ptr(), at.data_ptr(), _stream())
        return vals, idx, at

    vals, idx, at = ops.beam_scores_topk_rows(dec, lm, mu_row, k)
    for mu in (0.0, 0.3, 1.0):
        w_vals, w_idx, w_at = scalar(lm, np.float32(mu))
        rows = torch.from_numpy(mus == np.float32(mu)).to(dev)
        assert rows.any()
        assert torch.equal(vals[rows], w_vals[rows]) and torch.equal(idx[rows], w_idx[rows]) and torch.equal(at[rows], w_at[rows]), mu
    assert torch.isfinite(vals).all()
    # the LM operand absent
    vals, idx, at = ops.beam_scores_topk_rows(dec, None, None, k)
    w_vals, w_idx, w_at = scalar(None, 0.0)
    assert torch.equal(vals, w_vals) and torch.equal(idx, w_idx) and torch.equal(at, w_at)
    if k > 1:
        assert 5 in idx[2].tolist() or 9 not in idx[2].tolist()      # ties keep the lower index first


# =========================================================================================== 3. the CTC scorer pair over cells
def test_ctc_prefix_cells_equals_the_ragged_pair_on_replicated_emissions(dev):
    from emoasr_amd import ops
    rs = np.random.RandomState(0)
    V, blank, eos, W, cw = 40, 0, 2, 3, 4
    Ts, per_utt = [1, 37], [3, 2]
    sutt = [u for u, n in enumerate(per_utt) for _ in range(n)]
    S, Tmax, nb = len(sutt), 64, len(sutt) * W
    offs = [0, 1, 38]
    x = torch.from_numpy(np.log(rs.dirichlet(np.ones(V) * 0.5, size=offs[-1])).astype(np.float32)).to(dev)
    xoff = torch.tensor(offs, dtype=torch.int32, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    sutt_d = i32(sutt)
    xrep = torch.cat([x[offs[u]:offs[u + 1]] for u in sutt], 0).contiguous()
    roffs = [0]
    for u in sutt:
        roffs.append(roffs[-1] + Ts[u])
    xroff = i32(roffs)
    stride = W * cw * Tmax * 2
    prev = torch.full((nb, cw, Tmax, 2), 123.0, device=dev)
    prev_w = torch.full((nb, cw, Tmax, 2), 123.0, device=dev)
    ops.ctc_prefix_init_cells(x, xoff, sutt_d, blank, prev, stride)
    ops.ctc_prefix_init_ragged(xrep, xroff, blank, prev_w, stride)
    assert torch.equal(prev, prev_w)                  # (the sentinel past every search's frames included)
    c0 = i32(rs.randint(0, V, (nb, cw)))
    c0[:, 1] = eos
    c0[0, 2] = blank
    last0, olen0 = i32([eos] * nb), i32([0] * nb)
    par0, pc0 = i32([s * W for s in range(S) for _ in range(W)]), i32([0] * nb)
    psi0, st0 = ops.ctc_prefix_score_cells(x, xoff, sutt_d, W, Tmax, c0, last0, olen0, blank, eos, prev, par0, pc0)
    wpsi0, wst0 = ops.ctc_prefix_score_ragged(xrep, xroff, W, Tmax, c0, last0, olen0, blank, eos, prev_w, par0, pc0)
    assert torch.equal(psi0, wpsi0) and torch.equal(st0, wst0)
    # step 1: parents and candidates mixed inside every search; one candidate repeats the last token
    c1 = i32(rs.randint(0, V, (nb, cw)))
    lpar = [int(v) for v in rs.randint(0, W, nb)]
    pc1 = [int(v) for v in rs.randint(0, cw, nb)]
    assert len(set(lpar)) > 1 and len(set(pc1)) > 1
    last1 = i32([int(c0[(m // W) * W + lpar[m], pc1[m]]) for m in range(nb)])
    c1[:, 0] = last1
    c1[:, 2] = eos
    olen1 = i32([1] * nb)
    par1 = i32([(m // W) * W + lpar[m] for m in range(nb)])
    psi1, st1 = ops.ctc_prefix_score_cells(x, xoff, sutt_d, W, Tmax, c1, last1, olen1, blank, eos, st0, par1, i32(pc1))
    wpsi1, wst1 = ops.ctc_prefix_score_ragged(xrep, xroff, W, Tmax, c1, last1, olen1, blank, eos, wst0, par1, i32(pc1))
    assert torch.equal(psi1, wpsi1) and torch.equal(st1, wst1)
    assert torch.isfinite(psi1).all()


# =========================================================================================== 4. the update kernel over cells
def _sub_state(st, s):
    """search s of the state as a one-search state made of views: joint_beam_ref.update writes through them"""
    W = st["W"]
    rows = slice(s * W, s * W + W)
    sub = dict(S=1, W=W, max_pos=st["max_pos"], pos=st["pos"], all_done=0, mirror=[0, 0], state=st["state"][s:s + 1],
               hist_parent=st["hist_parent"][:, rows], hist_token=st["hist_token"][:, rows])
    for k in ("ids", "last", "parent", "pcand", "outlen", "klens", "score", "score_ctc", "res_score", "res_step", "res_parent"):
        sub[k] = st[k][rows]
    return sub, rows


def _update_cells_ref(st, vals, cands, psi, lm_at, cw, eos, lam, mus):
    """joint_beam_ref.update search by search with that search's mu and len_weight 0; parents made global; the tail once"""
    if st["all_done"] or st["pos"] >= st["max_pos"]:
        return
    pos = st["pos"]
    for s in range(st["S"]):
        if st["state"][s, 3]:
            continue
        sub, rows = _sub_state(st, s)
        cut = lambda a: None if a is None else a[rows]
        ref.update(sub, vals[rows], cands[rows], cut(psi), cut(lm_at), cw, eos, lam, float(mus[s]), 0.0)
        st["parent"][rows] += s * st["W"]
    nd = int(st["state"][:, 3].sum())
    st["pos"] = pos + 1
    if nd == st["S"]:
        st["all_done"] = 1
    st["mirror"] = [pos + 1, nd]


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("W,cw", [(1, 1), (3, 4), (4, 6), (32, 32)])
def test_update_cells_equals_the_reference_search_by_search(dev, S, W, cw):
    """every output array equal (ints exactly, doubles bit for bit) after every step, inputs drawn as
    test_update_kernel_equals_the_reference draws them (tables on a grid of 0.5: exact ties), a weight per search"""
    from emoasr_amd import lib
    eos, V, max_pos = 2, 11, 9
    lam = 0.5
    mus = np.array([0.5, 1.0, 0.25, 0.5, 2.0], dtype=np.float32)[:S]      # exact in float32: the grid stays a grid
    mu_d = torch.from_numpy(mus).to(dev)
    for mode in ("att", "ctc", "ctc+lm"):
        use_psi, use_lm = mode != "att", mode == "ctc+lm"
        rng = np.random.default_rng(1000 * S + 10 * W + cw)
        st = ref.new_state(S, W, max_pos, eos)
        D = _DeviceUpdate(dev, S, W, cw, max_pos, eos, use_psi, use_lm, lam, 123.0, 0.0)    # (u.mu is not read)
        ties, finished_at = 0, {}
        nb = S * W
        for i in range(max_pos + 2):
            vals = (-0.5 * rng.integers(0, 6, (nb, cw))).astype(np.float32)
            psi = (-0.5 * rng.integers(0, 6, (nb, cw))).astype(np.float32)
            lm_at = (-0.5 * rng.integers(0, 6, (nb, cw))).astype(np.float32)
            cands = rng.integers(3, V, (nb, cw)).astype(np.int32)
            for s in range(S):
                rows = slice(s * W, s * W + W)
                cands[rows] = np.where(rng.random((W, cw)) < 0.08 + 0.12 * s, eos, cands[rows])
            if i == 0:
                first = slice(0, nb, W) if cw > 1 else slice(0, 1)
                cands[first, 0], vals[first, 0] = eos, 0.5
            if i >= 5:
                cands[:] = eos
            before, live = int(st["pos"]), not st["all_done"]
            for s in range(S):
                if not st["all_done"] and not st["state"][s, 3]:
                    sub, rows = _sub_state(st, s)
                    ties += _count_ties(sub, vals[rows], cands[rows], psi[rows] if use_psi else None, lm_at[rows] if use_lm else None,
                                        cw, lam, float(mus[s]))
            _update_cells_ref(st, vals, cands, psi if use_psi else None, lm_at if use_lm else None, cw, eos, lam, mus)
            D.vals.copy_(torch.from_numpy(vals)); D.cands.copy_(torch.from_numpy(cands))
            if D.psi is not None:
                D.psi.copy_(torch.from_numpy(psi))
            if D.lm_at is not None:
                D.lm_at.copy_(torch.from_numpy(lm_at))
            lib.call("emoasr_beam_update_cells", ctypes.byref(D.b), mu_d.data_ptr(), _stream())
            torch.cuda.synchronize()
            D.compare(st, (mode, i))
            assert int(D.pos.item()) == before + (1 if live else 0), (mode, i)
            for s in range(S):
                if st["state"][s, 3] and s not in finished_at:
                    finished_at[s] = i
        assert st["all_done"] == 1 and st["pos"] < max_pos + 2, "the replayed steps came after the end"
        if S >= 3:
            assert len(set(finished_at.values())) >= 2, finished_at
        if W > 1:
            assert ties >= 10, (mode, ties)


def test_update_cells_weights_matter(dev):
    """two searches with the same inputs and different weights end differently: mu[s] is read per search"""
    from emoasr_amd import lib
    D = _DeviceUpdate(dev, 2, 2, 3, 4, 2, True, True, 0.5, 0.0, 0.0)
    vals = np.array([[-1.0, -2.0, -3.0]] * 4, dtype=np.float32)
    lm_at = np.array([[-9.0, -1.0, -1.0]] * 4, dtype=np.float32)
    cands = np.array([[3, 4, 5]] * 4, dtype=np.int32)
    D.vals.copy_(torch.from_numpy(vals)); D.cands.copy_(torch.from_numpy(cands)); D.lm_at.copy_(torch.from_numpy(lm_at))
    D.psi.zero_()
    mu = torch.tensor([0.0, 1.0], device=dev)
    lib.call("emoasr_beam_update_cells", ctypes.byref(D.b), mu.data_ptr(), _stream())
    torch.cuda.synchronize()
    ids = D.arr["ids"].cpu().tolist()
    assert ids[0] == 3 and ids[2] == 4, ids
    with pytest.raises(lib.EmoasrHipError, match="missing arguments"):
        lib.call("emoasr_beam_update_cells", ctypes.byref(D.b), None, _stream())


# =========================================================================================== 5. the len_weight expansion
def test_expansion_equals_the_update_kernels_result_score(dev):
    """positions 1..63 x len_weight {0.1, 0.3, 1.0, 5.0}: expand_len_weights on what the kernel writes at len_weight 0 gives,
    bit for bit, what emoasr_beam_update_batch writes with that len_weight for the same hypothesis score"""
    from emoasr_amd import lib
    from emoasr_amd.modeling.beam_search_device import expand_len_weights
    eos, S = 2, 63                      # search s finishes its one hypothesis at position s + 1
    rng = np.random.default_rng(5)
    base = rng.standard_normal(S) * 7 - 20

    def run(len_weight):
        out = np.zeros(S)
        for p in range(1, S + 1):
            D = _DeviceUpdate(dev, 1, 1, 1, 64, eos, False, False, 0.0, 0.0, len_weight)
            D.pos.fill_(p)
            D.arr["state"].copy_(torch.tensor([[p, 1, 0, 0]], dtype=torch.int32))
            D.arr["score"].copy_(torch.tensor([base[p - 1]], dtype=torch.float64))
            D.vals.copy_(torch.tensor([[np.float32(-0.1 * p)]])); D.cands.fill_(eos)
            lib.call("emoasr_beam_update_batch", ctypes.byref(D.b), _stream())
            torch.cuda.synchronize()
            assert D.arr["state"].cpu().tolist() == [[p + 1, 0, 1, 1]] and int(D.arr["res_step"].item()) == p
            out[p - 1] = D.arr["res_score"].cpu().numpy()[0]
        return out

    plain = run(0.0)
    assert np.array_equal(plain, base + np.array([float(np.float32(-0.1 * p)) for p in range(1, S + 1)]))
    hyps = [[7] * p for p in range(1, S + 1)]             # len(hyp) = the position the hypothesis ended at
    for w in (0.1, 0.3, 1.0, 5.0):
        want = run(w)
        got = expand_len_weights(hyps, list(plain), [w])[0]
        by_hyp = {len(h): s for h, s in zip(*got)}
        assert all(np.float64(by_hyp[p]).tobytes() == np.float64(want[p - 1]).tobytes() for p in range(1, S + 1)), w
        assert got[1] == sorted(got[1], reverse=True)


# =========================================================================================== 6-10. end to end on l3_tiny
_CACHE = {}
GRID_A = dict(decode_ctc_weight=0.3, W=4, lm_weights=[0.0, 0.3], len_weights=[0.0, 0.1, 0.3])
GRID_B = dict(decode_ctc_weight=0.0, W=3, lm_weights=[0.5], len_weights=[0.0, 0.2, 0.3])


def _l3(dtype, dev):
    key = ("model", dtype, str(dev))
    if key not in _CACHE:
        from emoasr_amd.modeling.asr import ASR
        from emoasr_amd.modeling.lm import LM
        cfg, sd, g = load_golden("l3_tiny")
        model = ASR(SimpleNamespace(**CONFIGS["l3_tiny"]), compute_dtype=dtype)
        model.load_state_dict(sd)
        lm = LM(SimpleNamespace(**LM_CFG), compute_dtype=dtype)
        lm.load_state_dict(lm_state(g))
        _CACHE[key] = (model.to(dev).eval(), lm.to(dev).eval(), g)
    return _CACHE[key]


def _five(dtype, dev):
    """-> (eouts [5, Tmax, d], elens): utterance 0, utterance 1, both cut to CUT_FRAC of their frames, utterance 1 cut to one"""
    key = ("five", dtype, str(dev))
    if key not in _CACHE:
        model, _, g = _l3(dtype, dev)
        enc = []
        with torch.no_grad():
            for b in range(2):
                n = int(g["xlens"][b])
                e, el, _ = model.encoder(g["xs"][b:b + 1, :n].to(dev), g["xlens"][b:b + 1])
                enc.append(e[0, :int(el[0])])
        parts = [enc[0], enc[1], enc[0][:max(2, round(CUT_FRAC[0] * enc[0].shape[0]))],
                 enc[1][:max(2, round(CUT_FRAC[1] * enc[1].shape[0]))], enc[1][:1]]
        elens = [p.shape[0] for p in parts]
        eouts = torch.zeros(5, max(elens), parts[0].shape[1], device=dev, dtype=parts[0].dtype)
        for b, p in enumerate(parts):
            eouts[b, :elens[b]] = p
        _CACHE[key] = (eouts, elens)
    return _CACHE[key]


def _per_cell(dtype, dev, grid):
    """joint_beam_search_device_batch cell by cell -> [cell][(hyps[b], scores[b])], once per grid"""
    key = ("cells", dtype, str(dev), str(grid))
    if key not in _CACHE:
        from emoasr_amd.modeling.beam_search_device import joint_beam_search_device_batch
        model, lm, _ = _l3(dtype, dev)
        eouts, elens = _five(dtype, dev)
        out = []
        for a in grid["lm_weights"]:
            for w in grid["len_weights"]:
                out.append(joint_beam_search_device_batch(model.decoder, eouts, elens, grid["W"], w, lm, a, grid["decode_ctc_weight"])[:2])
        _CACHE[key] = out
    return _CACHE[key]


def _run_grid(dtype, dev, grid):
    from emoasr_amd.modeling.beam_search_device import joint_beam_search_device_grid
    model, lm, _ = _l3(dtype, dev)
    eouts, elens = _five(dtype, dev)
    return joint_beam_search_device_grid(model.decoder, eouts, elens, grid["W"], lm, grid["lm_weights"], grid["len_weights"],
                                         grid["decode_ctc_weight"])


def _compare_f32(got, want, n_cells, what):
    hyps, scores = got
    assert len(hyps) == 5 and all(len(h) == n_cells for h in hyps)
    for c in range(n_cells):
        w_h, w_s = want[c]
        for b in range(5):
            assert hyps[b][c] == w_h[b], (what, c, b, hyps[b][c], w_h[b])
            assert len(scores[b][c]) == len(w_s[b])
            assert all(abs(x - y) < 1e-4 for x, y in zip(scores[b][c], w_s[b])), (what, c, b, scores[b][c], w_s[b])


@pytest.mark.parametrize("name", ["A", "B"])
def test_grid_equals_the_batched_search_cell_by_cell_f32(dev, name, monkeypatch):
    """every cell: hypotheses in order exactly, scores within 1e-4 (the bar between two f32 forms of this search); the per-cell
    reference's neighbouring scores differ by more than 1e-3 (asserted); grid A searches 2 weights per utterance, not 6 cells,
    and forms the memory projection and the CTC head's output once per chunk"""
    from emoasr_amd.decode_rt import DecoderStepRuntime
    from emoasr_amd.modeling import beam_search_device as bsd
    grid = GRID_A if name == "A" else GRID_B
    want = _per_cell(torch.float32, dev, grid)
    n_cells = len(grid["lm_weights"]) * len(grid["len_weights"])
    for c, (w_h, w_s) in enumerate(want):
        for b, s in enumerate(w_s):
            gaps = [x - y for x, y in zip(s, s[1:])]
            print(f"grid {name} cell {c} search {b}: {len(s)} results, smallest score gap {min(gaps) if gaps else float('nan'):.4g}")
            assert all(d > 1e-3 for d in gaps), (name, c, b, s)
    model, _, _ = _l3(torch.float32, dev)
    eng = bsd._engine_of(model.decoder)
    chunks, begins, heads = [], [], []
    orig_chunk, orig_begin, orig_head = bsd._batch_search_chunk, DecoderStepRuntime.begin_batch, eng.head_logits
    monkeypatch.setattr(bsd, "_batch_search_chunk",
                        lambda *a, **k: (chunks.append(len(k["grid"][0]) if k.get("grid") else len(a[3])), orig_chunk(*a, **k))[1])
    monkeypatch.setattr(DecoderStepRuntime, "begin_batch", lambda self, *a, **k: (begins.append(1), orig_begin(self, *a, **k))[1])
    monkeypatch.setattr(eng, "head_logits", lambda *a, **k: (heads.append(1), orig_head(*a, **k))[1])
    got = _run_grid(torch.float32, dev, grid)
    _compare_f32(got, want, n_cells, name)
    if name == "A":
        assert chunks == [5, 5], chunks                 # 2 distinct weights x 5 utterances: 10 searches, not 30
        assert len(begins) == 2 and len(heads) == 2     # once per chunk
    else:
        assert chunks == [5] and len(begins) == 1 and len(heads) == 0


@pytest.mark.parametrize("cap", [3, 1])
def test_grid_chunking(dev, cap, monkeypatch):
    """a chunk capacity of 3 searches (5 utterances x 2 weights; capacity 1 also cuts every utterance across chunks): hypotheses
    equal the unforced call, scores within 1e-4"""
    from emoasr_amd.modeling import beam_search_device as bsd
    grid = dict(GRID_A, lm_weights=[0.3, 0.5], len_weights=[0.0, 0.3])
    whole = _run_grid(torch.float32, dev, grid)
    chunks = []
    orig = bsd._batch_search_chunk
    monkeypatch.setattr(bsd, "batch_chunk_capacity", lambda *a, **k: cap)
    monkeypatch.setattr(bsd, "_batch_search_chunk", lambda *a, **k: (chunks.append((len(a[3]), len(k["grid"][0]))), orig(*a, **k))[1])
    parts = _run_grid(torch.float32, dev, grid)
    assert chunks == ([(1, 2)] * 5 if cap == 3 else [(1, 1)] * 10), chunks
    assert parts[0] == whole[0]
    for b in range(5):
        for x, y in zip(parts[1][b], whole[1][b]):
            assert len(x) == len(y) and all(abs(p - q) < 1e-4 for p, q in zip(x, y)), (b, x, y)


def test_grid_cells_per_group(dev, monkeypatch):
    """one search per attention workgroup or several: the kernels give a row the same bits, so the grid returns the same lists"""
    from emoasr_amd.modeling import beam_search_device as bsd
    grid = dict(GRID_A, lm_weights=[0.3, 0.5, 0.1], len_weights=[0.0, 0.3])
    monkeypatch.setattr(bsd, "GRID_CELLS_PER_GROUP", 1)
    one = _run_grid(torch.float32, dev, grid)
    monkeypatch.setattr(bsd, "GRID_CELLS_PER_GROUP", 3)
    three = _run_grid(torch.float32, dev, grid)
    assert one == three


def test_grid_bf16(dev):
    """grid A in bf16: every cell's best hypothesis is the per-cell batched search's, its score within test_batch_bf16's bar"""
    want = _per_cell(torch.bfloat16, dev, GRID_A)
    hyps, scores = _run_grid(torch.bfloat16, dev, GRID_A)
    for c, (w_h, w_s) in enumerate(want):
        for b in range(5):
            if not w_h[b]:
                assert not hyps[b][c]
                continue
            print(f"bf16 cell {c} search {b}: best score {scores[b][c][0]:.5f}, per cell {w_s[b][0]:.5f}")
            assert hyps[b][c][0] == w_h[b][0], (c, b, hyps[b][c], w_h[b])
            assert abs(scores[b][c][0] - w_s[b][0]) < 2e-2 * abs(w_s[b][0]) + 1e-3, (c, b, scores[b][c][0], w_s[b][0])


@pytest.mark.parametrize("how", ["rnnlm", "host_bookkeeping"])
def test_grid_fallback(dev, how, monkeypatch):
    """outside the batched device search (the RNN LM; EMOASR_DEVICE_BEAM=0) the grid returns decoder.decode looped over the cells:
    hypotheses exact, scores within 1e-4"""
    from emoasr_amd.modeling import beam_search_device as bsd
    model, lm, _ = _l3(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    e3, l3 = eouts[:3], elens[:3]
    if how == "rnnlm":
        from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state
        from emoasr_amd.modeling.lm import LM
        lm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=torch.float32)
        lm.load_state_dict(rnnlm_state(rnnlm_golden()))
        lm = lm.to(dev).eval()
    else:
        monkeypatch.setenv("EMOASR_DEVICE_BEAM", "0")
    grid_calls = []
    orig = bsd._batch_search_chunk
    monkeypatch.setattr(bsd, "_batch_search_chunk", lambda *a, **k: (grid_calls.append(k.get("grid")), orig(*a, **k))[1])
    lm_w, len_w, W, ctc_w = [0.0, 0.3], [0.0, 0.3], 4, 0.3
    hyps, scores = bsd.joint_beam_search_device_grid(model.decoder, e3, l3, W, lm, lm_w, len_w, ctc_w)
    assert not any(grid_calls), "the fallback does not run the grid chain"
    c = 0
    for a in lm_w:
        for w in len_w:
            w_h, w_s, _, _ = model.decoder.decode(e3, l3, None, W, w, lm, a, ctc_w)
            for b in range(3):
                assert hyps[b][c] == w_h[b], (how, a, w, b, hyps[b][c], w_h[b])
                assert len(scores[b][c]) == len(w_s[b]) and all(abs(x - y) < 1e-4 for x, y in zip(scores[b][c], w_s[b])), (how, a, w, b)
            c += 1


def test_grid_guards(dev):
    from emoasr_amd.modeling import beam_search_device as bsd
    model, lm, _ = _l3(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    with pytest.raises(ValueError, match="at least one frame"):
        bsd.joint_beam_search_device_grid(model.decoder, eouts[:3], [elens[0], 0, elens[2]], 4, lm, [0.3], [0.0], 0.3)
    with pytest.raises(NotImplementedError):
        bsd.joint_beam_search_device_grid(model.decoder, eouts[:1], elens[:1], 4, SimpleNamespace(lm_type="bert"), [0.3], [0.0], 0.3)


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_joint_fusion_grid_equals_one_decode_per_cell(dev, monkeypatch):
    """a 2 x 2 grid over a two-batch loader: every cell's 1-best texts, WER and summary are decode.test's with that cell's weights
    (joint_beam_impl = "batch"); best follows the reference's rule; the encoder ran once per batch; decode_ctc_weight = 1 gives
    identical cells"""
    from emoasr_amd import decode as dec
    from emoasr_amd import fusion_grid as fg
    from emoasr_amd.metrics import compute_wers, wer_summary
    model, lm, g = _l3(torch.float32, dev)
    xs, xlens = g["xs"], g["xlens"]
    n0 = int(xlens[0])
    cut = n0 * 3 // 5 // 4 * 4
    T = int(xlens[:2].max())
    loader = [{"utt_ids": ["utt0", "utt1"], "texts": ["w5 w9 w11", "w7 w7 w12 w3"], "xs": xs[:2, :T], "xlens": xlens[:2]},
              {"utt_ids": ["utt2"], "texts": ["w4 w30"], "xs": xs[:1, :cut], "xlens": torch.tensor([cut])}]
    enc_calls = []
    real = model.encoder.forward
    monkeypatch.setattr(model.encoder, "forward", lambda *a, **k: (enc_calls.append(1), real(*a, **k))[1])
    lm_w, len_w, W, ctc_w = [0.0, 0.3], [0.0, 0.3], 4, 0.3
    # references that some cell can reach: the last cell's own 1-best texts with one word changed (WERs below 100, so that the
    # rule for `best` has something to choose from)
    first = []
    fg.joint_fusion_grid(model, loader, _Vocab(), W, lm, lm_w, len_w, dev, decode_ctc_weight=ctc_w, texts_out=first)
    flat = first[-1]
    assert len(flat) == 3 and flat[0]
    loader[0]["texts"] = [" ".join(flat[0].split()[:-1] + ["w39"]), flat[1]]
    loader[1]["texts"] = [flat[2]]
    del enc_calls[:]
    texts = []
    results, best = fg.joint_fusion_grid(model, loader, _Vocab(), W, lm, lm_w, len_w, dev, decode_ctc_weight=ctc_w, texts_out=texts)
    assert len(enc_calls) == len(loader) and texts == first
    assert [(r[0], r[1]) for r in results] == [(0.0, 0.0), (0.0, 0.3), (0.3, 0.0), (0.3, 0.3)] and len(texts) == 4
    monkeypatch.setattr(model.decoder, "joint_beam_impl", "batch")
    want_best = (0, 0, 100, "")
    for c, (a, b, wer, info) in enumerate(results):
        rows = dec.test(model, loader, _Vocab(), W, b, ctc_w, False, lm, a, dev)
        assert [r[0] for r in rows] == ["utt0", "utt1", "utt2"]
        assert [r[2] for r in rows] == texts[c], (a, b)
        w_wer, w_dict = compute_wers([r[2].split() for r in rows], [r[3].split() for r in rows])
        assert info == wer_summary(w_wer, w_dict) and abs(wer - w_wer) < 1e-9, (a, b, info)
        if w_wer < want_best[2]:
            want_best = (a, b, w_wer, info)
    assert tuple(best) == want_best and best[2] < 100
    # greedy CTC: the weights do not matter
    texts1 = []
    results1, best1 = fg.joint_fusion_grid(model, loader, _Vocab(), W, lm, lm_w, len_w, dev, decode_ctc_weight=1, texts_out=texts1)
    rows = dec.test(model, loader, _Vocab(), 1, 0.0, 1, False, None, 0.0, dev)       # (greedy: one hypothesis per utterance)
    assert all(t == [r[2] for r in rows] for t in texts1) and len(texts1) == 4
    assert len({(r[2], r[3]) for r in results1}) == 1
    assert tuple(best1) == (tuple(results1[0]) if results1[0][2] < 100 else (0, 0, 100, ""))      # the first strictly smaller WER
    with pytest.raises(NotImplementedError, match="CTC models only"):
        fg.ctc_fusion_grid(model, loader, _Vocab(), W, lm, lm_w, len_w, dev)
