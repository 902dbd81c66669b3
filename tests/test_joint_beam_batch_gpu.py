"""The batched joint CTC / attention beam search on the GPU: its three kernels alone against their
references, and the search end to end against the single search on l3_tiny."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import joint_beam_ref as ref
from tests.util import CONFIGS, DECODE_SETTINGS, LM_CFG, load_golden, lm_state, split_ragged

pytestmark = pytest.mark.gpu

# the five searches of the end-to-end tests: utterance 0, utterance 1, each cut to about 60 % of its encoder frames, and
# utterance 1 cut to one frame.  The cut lengths are chosen so that the SINGLE search's neighbouring result scores differ by more
# than 1e-3 in every setting (asserted below): hypotheses can then be compared in order.
CUT_FRAC = (0.6, 0.6)


# =========================================================================================== 1. the update kernel alone
class _DeviceUpdate:
    """device arrays of emoasr_beam_update_batch for S searches, initialised like the search does"""

    def __init__(self, dev, S, W, cw, max_pos, eos, use_psi, use_lm, lam, mu, len_weight):
        from emoasr_amd import lib
        nb = S * W
        st0 = ref.new_state(S, W, max_pos, eos)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.arr = {k: t(st0[k]) for k in ("state", "ids", "last", "parent", "pcand", "outlen", "klens", "score", "score_ctc",
                                           "hist_parent", "hist_token", "res_score", "res_step", "res_parent")}
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ctl = torch.zeros(1, dtype=torch.int32, device=dev)
        self.vals = torch.zeros(nb, cw, device=dev)
        self.cands = torch.zeros(nb, cw, dtype=torch.int32, device=dev)
        self.psi = torch.zeros(nb, cw, device=dev) if use_psi else None
        self.lm_at = torch.zeros(nb, cw, device=dev) if (use_psi and use_lm) else None
        self.mirror = torch.zeros(2, dtype=torch.int32).pin_memory()
        b = self.b = lib.BeamUpdateBatch()
        b.S, b.max_pos, b.pos, b.ctl = S, max_pos, self.pos.data_ptr(), self.ctl.data_ptr()
        u, a = b.u, self.arr
        u.bw, u.cw, u.eos = W, cw, eos
        u.one_minus_lam, u.lam, u.mu = float(np.float32(1 - lam)), float(np.float32(lam)), float(np.float32(mu))
        u.len_weight = float(len_weight)
        u.vals, u.cands = self.vals.data_ptr(), self.cands.data_ptr()
        u.psi = self.psi.data_ptr() if self.psi is not None else None
        u.lm_at = self.lm_at.data_ptr() if self.lm_at is not None else None
        u.score, u.score_ctc = a["score"].data_ptr(), a["score_ctc"].data_ptr()
        u.n_ids, u.n_parent, u.n_pcand = a["ids"].data_ptr(), a["parent"].data_ptr(), a["pcand"].data_ptr()
        u.n_last, u.n_outlen, u.n_klens = a["last"].data_ptr(), a["outlen"].data_ptr(), a["klens"].data_ptr()
        u.hist_parent, u.hist_token = a["hist_parent"].data_ptr(), a["hist_token"].data_ptr()
        u.res_score, u.res_step, u.res_parent = a["res_score"].data_ptr(), a["res_step"].data_ptr(), a["res_parent"].data_ptr()
        u.state, u.host_mirror = a["state"].data_ptr(), self.mirror.data_ptr()

    def step(self, vals, cands, psi, lm_at):
        from emoasr_amd import lib
        self.vals.copy_(torch.from_numpy(vals)); self.cands.copy_(torch.from_numpy(cands))
        if self.psi is not None:
            self.psi.copy_(torch.from_numpy(psi))
        if self.lm_at is not None:
            self.lm_at.copy_(torch.from_numpy(lm_at))
        lib.call("emoasr_beam_update_batch", ctypes.byref(self.b), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def compare(self, st, where):
        for k, v in self.arr.items():
            got = v.cpu().numpy()
            # ints exactly, doubles and floats bit for bit
            assert got.dtype == st[k].dtype and got.tobytes() == st[k].tobytes(), (where, k, got, st[k])
        assert int(self.pos.item()) == st["pos"] and int(self.ctl.item()) == st["all_done"], (where, self.pos.item(), st["pos"])
        assert self.mirror.tolist() == st["mirror"], (where, self.mirror.tolist(), st["mirror"])


def _count_ties(st, vals, cands, psi, lm_at, cw, lam, mu):
    """exact ties the update has to break in this step, counted on the reference's arithmetic: equal candidate scores inside a
    beam and equal hypothesis scores among a search's kept candidates"""
    S, W = st["S"], st["W"]
    f1, fl, fm = np.float32(1 - lam), np.float32(lam), np.float32(mu)
    ties = 0
    for s in range(S):
        if st["state"][s, 3]:
            continue
        tot = []
        for m in range(int(st["state"][s, 1])):
            r = s * W + m
            sc = vals[r].copy() if psi is None else f1 * vals[r] + fl * (psi[r] - st["score_ctc"][r])
            if psi is not None and lm_at is not None:
                sc = sc + fm * lm_at[r]
            ties += len(sc) - len(np.unique(sc))
            tot += [float(st["score"][r]) + float(v) for v in np.sort(sc)[::-1][:min(W, cw)]]
        ties += len(tot) - len(set(tot))
    return ties


@pytest.mark.parametrize("len_weight", [0.0, 0.3])
@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("W,cw", [(1, 1), (3, 4), (4, 6), (32, 32)])
def test_update_kernel_equals_the_reference(dev, S, W, cw, len_weight):
    """every output array equal (ints exactly, doubles bit for bit) after every step, for tables on a grid of 0.5 (exact ties),
    searches that finish at different steps, n_alive < W, <eos> at position 0 (dropped); the shared position advances exactly
    once per live step; a replay after the end changes nothing"""
    eos, V, max_pos = 2, 11, 9
    lam, mu = 0.5, 0.5       # exact in float32: the grid stays a grid
    for mode in ("att", "ctc", "ctc+lm"):
        use_psi, use_lm = mode != "att", mode == "ctc+lm"
        rng = np.random.default_rng(1000 * S + 10 * W + cw + (7 if len_weight else 0))
        st = ref.new_state(S, W, max_pos, eos)
        D = _DeviceUpdate(dev, S, W, cw, max_pos, eos, use_psi, use_lm, lam, mu if use_lm else 0.0, len_weight)
        D.compare(st, (mode, "start"))
        ties, finished_at, saw_short = 0, {}, False
        nb = S * W
        for i in range(max_pos + 2):
            vals = (-0.5 * rng.integers(0, 6, (nb, cw))).astype(np.float32)
            psi = (-0.5 * rng.integers(0, 6, (nb, cw))).astype(np.float32)
            lm_at = (-0.5 * rng.integers(0, 6, (nb, cw))).astype(np.float32)
            cands = rng.integers(3, V, (nb, cw)).astype(np.int32)
            for s in range(S):     # <eos> more often in the later searches: they finish at different steps
                rows = slice(s * W, s * W + W)
                cands[rows] = np.where(rng.random((W, cw)) < 0.08 + 0.12 * s, eos, cands[rows])
            if i == 0:             # <eos> as the best candidate at position 0: an empty hypothesis, dropped
                first = slice(0, nb, W) if cw > 1 else slice(0, 1)      # (one candidate only: that search ends there, empty)
                cands[first, 0], vals[first, 0] = eos, 0.5
            if i >= 5:             # the end: everything proposes <eos>
                cands[:] = eos
            before = int(st["pos"])
            live = not st["all_done"]
            ties += _count_ties(st, vals, cands, psi if use_psi else None, lm_at if use_lm else None, cw, lam, mu)
            ref.update(st, vals, cands, psi if use_psi else None, lm_at if use_lm else None, cw, eos, lam, mu if use_lm else 0.0,
                       len_weight)
            D.step(vals, cands, psi, lm_at)
            D.compare(st, (mode, i))
            assert int(D.pos.item()) == before + (1 if live else 0), (mode, i)
            for s in range(S):
                saw_short |= bool(not st["state"][s, 3] and 0 < st["state"][s, 1] < W)
                if st["state"][s, 3] and s not in finished_at:
                    finished_at[s] = i
        assert st["all_done"] == 1 and st["pos"] < max_pos + 2, "the replayed steps came after the end"
        assert int(st["state"][0, 2]) == 0 or st["res_step"][0] >= 1          # nothing finished at position 0
        if W > 1:
            assert ties >= 10, (mode, ties)
            assert saw_short or S == 1, "no live search with n_alive < W"
        if S >= 3:
            assert len(set(finished_at.values())) >= 2, finished_at           # mixed states: not all at the same step


def test_update_refusals(dev):
    from emoasr_amd import lib
    D = _DeviceUpdate(dev, 1, 4, 6, 4, 2, True, False, 0.5, 0.0, 0.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for field, value in (("bw", 33), ("bw", 0), ("cw", 33), ("cw", 0)):
        old = getattr(D.b.u, field)
        setattr(D.b.u, field, value)
        with pytest.raises(lib.EmoasrHipError, match="outside 1..32"):
            lib.call("emoasr_beam_update_batch", ctypes.byref(D.b), stream)
        setattr(D.b.u, field, old)
    with pytest.raises(lib.EmoasrHipError, match="offsets must rise"):
        lib.call("emoasr_group_offsets_check", 3, (ctypes.c_int * 4)(0, 5, 5, 9))
    with pytest.raises(lib.EmoasrHipError, match="offsets must rise"):
        lib.call("emoasr_group_offsets_check", 2, (ctypes.c_int * 3)(0, 7, 3))
    lib.call("emoasr_group_offsets_check", 3, (ctypes.c_int * 4)(0, 1, 8, 9))
    q = torch.zeros(33, 64, device=dev)
    with pytest.raises(lib.EmoasrHipError, match="outside 1..32"):
        lib.call("emoasr_attn_step_group", lib.F32, 1, 33, 64, 2, q.data_ptr(), q.data_ptr(), q.data_ptr(), q.data_ptr(), stream)
    ws = torch.zeros(1024, device=dev, dtype=torch.uint8)
    g = lib.DecoderStepGroup()
    g.S, g.W, g.moff = 2, 2, q.data_ptr()
    d = g.d
    d.nb, d.Lmax, d.dd, d.H, d.F, d.V = 4, 8, 64, 2, 128, 40
    kvp = (ctypes.c_void_p * 1)(q.data_ptr())
    d.kv = ctypes.cast(kvp, ctypes.POINTER(ctypes.c_void_p))
    for f in ("ids", "pos", "klens", "kcache", "vcache", "logits_last", "ws"):
        setattr(d, f, ws.data_ptr())
    d.ws_bytes = ws.numel()
    assert lib.size_query("emoasr_decode_step_group_ws_bytes", lib.F32, 4, 64, 2, 128, 40) > ws.numel()
    layers = (lib.DecoderLayer * 1)()
    with pytest.raises(lib.EmoasrHipError, match="scratch too small"):
        lib.call("emoasr_transformer_decoder_step_group", lib.F32, 1, layers, ctypes.byref(g), stream)
    g.W = 3
    with pytest.raises(lib.EmoasrHipError, match="rows for"):
        lib.call("emoasr_transformer_decoder_step_group", lib.F32, 1, layers, ctypes.byref(g), stream)


# =========================================================================================== 2. grouped cross-attention
def _attn_f64(q, kv, offs, W, H):
    """softmax(q k^T / sqrt(dk)) v per search and head in float64, from the (rounded) inputs"""
    nb, dd = q.shape
    dk = dd // H
    q, kv = q.double().cpu(), kv.double().cpu()
    out = torch.zeros(nb, dd, dtype=torch.float64)
    for s in range(len(offs) - 1):
        k, v = kv[offs[s]:offs[s + 1], :dd], kv[offs[s]:offs[s + 1], dd:]
        for h in range(H):
            c = slice(h * dk, h * dk + dk)
            p = torch.softmax(q[s * W:(s + 1) * W, c] @ k[:, c].T / dk ** 0.5, -1)
            out[s * W:(s + 1) * W, c] = p @ v[:, c]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,dk", [(2, 64), (4, 32)])
@pytest.mark.parametrize("W", [1, 3, 16, 17, 32])
def test_grouped_cross_attention(dev, W, H, dk, dtype):
    """three searches of different lengths in one launch against float64; the bar is measured in the same test: emoasr_attn_fwd
    (Tq = 1, the memory replicated per beam) on the same inputs against the same reference -- the grouped kernel stays within
    twice that error plus 1e-7 (a different order of sums of the same length).  A search's rows are bit-identical alone and
    inside the batch."""
    from emoasr_amd import ops
    dd, S = H * dk, 3
    for Ts in ((1, 64, 200), (63, 65, 1)):
        gen = torch.Generator().manual_seed(W * 1000 + H * 10 + sum(Ts))
        offs = [0, Ts[0], Ts[0] + Ts[1], sum(Ts)]
        q = torch.randn(S * W, dd, generator=gen).to(dtype).to(dev)
        kv = torch.randn(sum(Ts), 2 * dd, generator=gen).to(dtype).to(dev)
        moff = torch.tensor(offs, dtype=torch.int32, device=dev)
        out = ops.attn_step_group(q, kv, moff, W, H)
        want = _attn_f64(q, kv, offs, W, H)
        # the comparator: today's step form, every beam with its own copy of the (padded) memory
        Tm = max(Ts)
        rep = torch.zeros(S * W, Tm, 2 * dd, dtype=dtype, device=dev)
        for s in range(S):
            rep[s * W:(s + 1) * W, :Ts[s]] = kv[offs[s]:offs[s + 1]]
        klens = torch.tensor([Ts[s] for s in range(S) for _ in range(W)], dtype=torch.int32, device=dev)
        if dk == 64:
            old, _ = ops.attn_fwd(q.view(S * W, 1, dd), rep[..., :dd], rep[..., dd:], H, 1.0 / dk ** 0.5, klens=klens)
            old = old.view(S * W, dd)
        else:
            # emoasr_attn_fwd takes heads of 64 columns only: the same inputs with every head zero-filled to 64 columns (the
            # scores and the first dk output columns of a head are the same sums plus zeros) and the scale of dk columns
            wide = lambda t: torch.nn.functional.pad(t.reshape(*t.shape[:-1], H, dk), (0, 64 - dk)).reshape(*t.shape[:-1], H * 64)
            old, _ = ops.attn_fwd(wide(q).view(S * W, 1, H * 64), wide(rep[..., :dd]), wide(rep[..., dd:]), H, 1.0 / dk ** 0.5,
                                  klens=klens)
            old = old.view(S * W, H, 64)[..., :dk].reshape(S * W, dd)
        err_new = (out.double().cpu() - want).abs().max().item()
        err_old = (old.double().cpu() - want).abs().max().item()
        print(f"grouped attention {str(dtype)[6:]} W={W} H={H} dk={dk} T={Ts}: max error {err_new:.3e}, emoasr_attn_fwd {err_old:.3e}")
        assert torch.isfinite(out.float()).all()
        assert err_new <= 2 * err_old + 1e-7, (err_new, err_old)
        for s in range(S):     # row invariance
            alone = ops.attn_step_group(q[s * W:(s + 1) * W].contiguous(), kv[offs[s]:offs[s + 1]].contiguous(),
                                        torch.tensor([0, Ts[s]], dtype=torch.int32, device=dev), W, H)
            assert torch.equal(alone, out[s * W:(s + 1) * W]), (s, Ts)


# =========================================================================================== 3. ragged CTC prefix scorer
def test_ragged_ctc_prefix_scorer_equals_the_scorer_per_search(dev):
    from emoasr_amd import ops
    rs = np.random.RandomState(0)
    V, blank, eos, W, cw = 40, 0, 2, 2, 3
    Ts = [1, 7, 37]
    S, Tmax = len(Ts), 64
    offs = [0, 1, 8, 45]
    x = torch.from_numpy(np.log(rs.dirichlet(np.ones(V) * 0.5, size=offs[-1])).astype(np.float32)).to(dev)
    xoff = torch.tensor(offs, dtype=torch.int32, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    nb = S * W
    # step 0: every row reads its search's initial state at (row s * W, candidate 0) of the "previous" half
    prev = torch.full((nb, cw, Tmax, 2), 123.0, device=dev)
    ops.ctc_prefix_init_ragged(x, xoff, blank, prev, W * cw * Tmax * 2)
    c0 = i32(rs.randint(0, V, (nb, cw)))
    c0[:, 1] = eos
    c0[0, 2] = blank
    last0, olen0 = i32([eos] * nb), i32([0] * nb)
    par0, pc0 = i32([s * W for s in range(S) for _ in range(W)]), i32([0] * nb)
    psi0, st0 = ops.ctc_prefix_score_ragged(x, xoff, W, Tmax, c0, last0, olen0, blank, eos, prev, par0, pc0)
    # step 1: parents and candidates mixed inside every search; one candidate repeats the last token
    c1 = i32(rs.randint(0, V, (nb, cw)))
    lpar, pc1 = [1, 0, 0, 0, 1, 1], [2, 0, 1, 2, 0, 2]
    last1 = i32([int(c0[s * W + lpar[s * W + m], pc1[s * W + m]]) for s in range(S) for m in range(W)])
    c1[:, 0] = last1
    c1[:, 2] = eos
    olen1 = i32([1] * nb)
    par1 = i32([s * W + lpar[s * W + m] for s in range(S) for m in range(W)])
    psi1, st1 = ops.ctc_prefix_score_ragged(x, xoff, W, Tmax, c1, last1, olen1, blank, eos, st0, par1, i32(pc1))
    for s in range(S):
        rows = slice(s * W, s * W + W)
        xs = x[offs[s]:offs[s + 1]].contiguous()
        r0 = ops.ctc_prefix_init(xs, blank)
        assert torch.equal(prev[s * W, 0, :Ts[s]], r0), s
        p0, s0 = ops.ctc_prefix_score(xs, c0[rows].contiguous(), last0[rows], olen0[rows], blank, eos, init_state=r0)
        assert torch.equal(psi0[rows], p0) and torch.equal(st0[rows, :, :Ts[s]], s0), s
        p1, s1 = ops.ctc_prefix_score(xs, c1[rows].contiguous(), last1[rows], olen1[rows], blank, eos, prev_states=s0,
                                      parent=i32(lpar[s * W:(s + 1) * W]), pcand=i32(pc1[s * W:(s + 1) * W]))
        assert torch.equal(psi1[rows], p1) and torch.equal(st1[rows, :, :Ts[s]], s1), s
    assert torch.isfinite(psi1).all()


# =========================================================================================== 4-8. end to end on l3_tiny
_CACHE = {}


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


def _single(dtype, dev, kw):
    """the single search on every one of the five, once per setting"""
    key = ("single", dtype, str(dev), tuple(sorted(kw.items())))
    if key not in _CACHE:
        model, lm, _ = _l3(dtype, dev)
        eouts, elens = _five(dtype, dev)
        assert model.decoder.joint_beam_impl == "single"
        _CACHE[key] = [model.decoder.decode(eouts[b:b + 1, :elens[b]], [elens[b]], None, lm=lm, **kw)[:2] for b in range(5)]
    return _CACHE[key]


def _count_batched(monkeypatch):
    from emoasr_amd.modeling import beam_search_device as bsd
    calls = []
    orig = bsd.joint_beam_search_device_batch
    monkeypatch.setattr(bsd, "joint_beam_search_device_batch", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


@pytest.mark.parametrize("len_weight", [0.0, 0.3])
@pytest.mark.parametrize("si", range(len(DECODE_SETTINGS)))
def test_batch_equals_the_single_search_f32(dev, si, len_weight, monkeypatch):
    """decoder.decode on the batch of five equals the single search on eouts[b:b+1, :elens[b]]: hypotheses in order, scores within
    1e-4 (the bar test_device_beam_search_equals_host_bookkeeping holds between the two f32 forms of today); the single
    search's neighbouring scores differ by more than 1e-3; the uncut utterances also equal the fixture"""
    model, lm, g = _l3(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    kw = dict(DECODE_SETTINGS[si], len_weight=len_weight)
    want = _single(torch.float32, dev, kw)
    for b, (h, s) in enumerate(want):
        gaps = [a - c for a, c in zip(s, s[1:])]
        print(f"setting {si} len_weight {len_weight} search {b} (T {elens[b]}): {len(h)} results, smallest score gap "
              f"{min(gaps) if gaps else float('nan'):.4g}")
        assert all(d > 1e-3 for d in gaps), (si, len_weight, b, s)
    calls = _count_batched(monkeypatch)
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    assert len(calls) == 1, "the batched search was not the one called"
    assert len(hyps) == 5 and len(scores) == 5
    for b in range(5):
        assert hyps[b] == want[b][0], (si, len_weight, b, hyps[b], want[b][0])
        assert len(scores[b]) == len(want[b][1])
        assert all(abs(a - c) < 1e-4 for a, c in zip(scores[b], want[b][1])), (si, len_weight, b, scores[b], want[b][1])
    if len_weight == DECODE_SETTINGS[si]["len_weight"]:
        for b in range(2):
            assert hyps[b] == split_ragged(g[f"decode/{si}/{b}/hyps"], g[f"decode/{si}/{b}/lens"]), (si, b)


def test_one_utterance_through_the_batched_search(dev, monkeypatch):
    """joint_beam_impl = "batch": one utterance takes the batched search and returns the single search's shape and results"""
    model, lm, _ = _l3(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    kw = dict(DECODE_SETTINGS[2])
    want = _single(torch.float32, dev, kw)
    calls = _count_batched(monkeypatch)
    monkeypatch.setattr(model.decoder, "joint_beam_impl", "batch")
    for b in (0, 4):
        hyps, scores, _, _ = model.decoder.decode(eouts[b:b + 1, :elens[b]], [elens[b]], None, lm=lm, **kw)
        assert hyps == want[b][0] and all(abs(a - c) < 1e-4 for a, c in zip(scores, want[b][1])), (b, hyps, want[b])
    assert len(calls) == 2


def test_batch_bf16(dev, monkeypatch):
    """bf16 runs; the best hypothesis equals the single search's and its score is within the existing bf16 bar"""
    model, lm, _ = _l3(torch.bfloat16, dev)
    eouts, elens = _five(torch.bfloat16, dev)
    kw = dict(DECODE_SETTINGS[2])
    want = _single(torch.bfloat16, dev, kw)
    calls = _count_batched(monkeypatch)
    hyps, scores, _, _ = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    assert len(calls) == 1
    for b in range(5):
        if not want[b][0]:
            continue
        print(f"bf16 search {b}: best score {scores[b][0]:.5f}, single {want[b][1][0]:.5f}")
        assert hyps[b][0] == want[b][0][0], (b, hyps[b], want[b][0])
        assert abs(scores[b][0] - want[b][1][0]) < 2e-2 * abs(want[b][1][0]) + 1e-3, (b, scores[b][0], want[b][1][0])


def test_chunking(dev, monkeypatch):
    """with a chunk capacity of two searches the batch of five returns what it returns in one chunk (products over another
    number of rows may take another tile: scores within the f32 bar of 1e-4, hypotheses equal)"""
    from emoasr_amd.modeling import beam_search_device as bsd
    model, lm, _ = _l3(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    kw = dict(DECODE_SETTINGS[2])
    whole = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    chunks = []
    orig = bsd._batch_search_chunk
    monkeypatch.setattr(bsd, "batch_chunk_capacity", lambda *a, **k: 2)
    monkeypatch.setattr(bsd, "_batch_search_chunk", lambda *a, **k: (chunks.append(len(a[3])), orig(*a, **k))[1])
    parts = model.decoder.decode(eouts, elens, None, lm=lm, **kw)
    assert chunks == [2, 2, 1]
    assert parts[0] == whole[0]
    for a, c in zip(parts[1], whole[1]):
        assert len(a) == len(c) and all(abs(x - y) < 1e-4 for x, y in zip(a, c)), (a, c)


def test_beam_width_one_and_the_fallbacks(dev, monkeypatch):
    """beam_width == 1 on three utterances: one hypothesis (or none) per utterance; width 33 and the RNN LM fall back to the
    search per utterance with the same hypotheses"""
    from tests.rnnlm_util import RNNLM_CFG, rnnlm_golden, rnnlm_state
    from emoasr_amd.modeling.lm import LM
    model, lm, _ = _l3(torch.float32, dev)
    eouts, elens = _five(torch.float32, dev)
    e3, l3 = eouts[:3], elens[:3]
    dec = model.decoder
    calls = _count_batched(monkeypatch)
    kw = dict(DECODE_SETTINGS[1], beam_width=1)
    hyps, scores, _, _ = dec.decode(e3, l3, None, lm=lm, **kw)
    assert len(calls) == 1 and len(hyps) == 3
    for b in range(3):
        h, s, _, _ = dec.decode(e3[b:b + 1, :l3[b]], [l3[b]], None, lm=lm, **kw)
        assert (hyps[b], scores[b]) == ((h[0], pytest.approx(s[0], abs=1e-4)) if h else ([], None)), (b, hyps[b], h)
    rnnlm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=torch.float32)
    rnnlm.load_state_dict(rnnlm_state(rnnlm_golden()))
    rnnlm = rnnlm.to(dev).eval()
    for kw, the_lm in ((dict(DECODE_SETTINGS[1], beam_width=33), lm), (dict(DECODE_SETTINGS[2]), rnnlm)):
        hyps, scores, _, _ = dec.decode(e3, l3, None, lm=the_lm, **kw)
        assert len(calls) == 1, "the fallback goes through joint_beam_search"
        for b in range(3):
            h, s, _, _ = dec.decode(e3[b:b + 1, :l3[b]], [l3[b]], None, lm=the_lm, **kw)
            assert hyps[b] == h and scores[b] == pytest.approx(s, abs=1e-4), (kw, b)
    with pytest.raises(ValueError, match="at least one"):
        dec.decode(e3, [l3[0], 0, l3[2]], None, lm=lm, **DECODE_SETTINGS[2])


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_nbest_rows_of_a_three_utterance_loader(dev, tmp_path, monkeypatch):
    """decode.test(nbest=True) over one batch of three utterances gives the rows of three one-utterance loaders (scores within
    1e-4) and the five-column TSV.  A one-utterance loader hands its utterance over with the padding it has in the batch --
    padding leaks through the encoder's convolution layers, so a shorter utterance encoded alone is another input to the search,
    not another search (tests/test_ctc_beam_batch_gpu.py) -- and decodes its valid frames through joint_beam_impl = "batch"; the
    longest utterance has no padding and is also compared with the default single search."""
    from emoasr_amd import decode as dec
    model, lm, g = _l3(torch.float32, dev)
    xs, xlens = g["xs"], g["xlens"]
    n0 = int(xlens[0])
    assert n0 == int(xlens[:2].max())
    cut = n0 * 3 // 5 // 4 * 4
    x3 = torch.zeros(3, n0, xs.shape[2])
    x3[:2] = xs[:2, :n0]
    x3[2, :cut] = xs[0, :cut]
    l3 = torch.tensor([n0, int(xlens[1]), cut])
    ids = ["utt0", "utt1", "utt2"]
    batch = [{"utt_ids": ids, "texts": ["r0", "r1", "r2"], "xs": x3, "xlens": l3}]
    ones = [{"utt_ids": ids[b:b + 1], "texts": [f"r{b}"], "xs": x3[b:b + 1], "xlens": l3[b:b + 1]} for b in range(3)]
    st = DECODE_SETTINGS[2]
    args = (_Vocab(), st["beam_width"], st["len_weight"], st["decode_ctc_weight"], False, lm, st["lm_weight"], dev)
    calls = _count_batched(monkeypatch)
    rows = dec.test(model, batch, *args, nbest=True)
    assert len(calls) == 1
    monkeypatch.setattr(model.decoder, "joint_beam_impl", "batch")
    want = dec.test(model, ones, *args, nbest=True)
    assert len(calls) == 4
    monkeypatch.setattr(model.decoder, "joint_beam_impl", "single")
    first = dec.test(model, ones[:1], *args, nbest=True)
    assert len(calls) == 4
    assert len(rows) == len(want) and len(rows) >= 3 and [r[0] for r in rows] == sorted(r[0] for r in rows)
    for r, w in list(zip(rows, want)) + list(zip(rows, first)):
        assert r[0] == w[0] and r[2:] == w[2:], (r, w)
        assert isinstance(r[1], float) and abs(r[1] - w[1]) < 1e-4, (r, w)
    assert len(first) >= 1
    path = tmp_path / "nbest.tsv"
    dec.save_results(rows, str(path), nbest=True)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["utt_id", "score_asr", "token_id", "text", "reftext"] and len(lines) == 1 + len(rows)
