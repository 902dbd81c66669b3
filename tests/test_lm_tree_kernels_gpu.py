"""The kernels of the Transformer-LM fusion over a prefix tree (csrc/lm_tree.hip) on the device: advance against
its numpy restatement (tests/lm_tree_ref.py) over a random walk with slot reuse and at both capacity limits, the gathered single-query
attention against the float64 attention over the gathered rows (the bound of test_attn_step_against_f64: one output ulp + 4 x the f32
numpy model's own error), and the whole step, driven by a random tree walk, against oracle.decoder.lm_logits in double on the full
prefix of every row -- within twice the distance emoasr_bert_lm_step's chain form on dense caches shows on the same prefixes."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import lm_tree_ref as T
from tests.test_rnnt_fusion_gpu import OFF
from tests.util import LM_CFG, load_ctc_beam_golden

pytestmark = pytest.mark.gpu

S, W, PER, ROWS = 10, 4, 16, 37          # 37 rows of 10 searches (the last one partial), 16 slots per search
SENT = -7


def _i64(a, dev):
    return torch.as_tensor(np.asarray(a, np.int64)).to(dev)


def _same(state, ref):
    """the device tree equals the restatement, entry for entry"""
    return (np.array_equal(state.llen.cpu().numpy(), ref.llen) and np.array_equal(state.lanc.cpu().numpy(), ref.lanc)
            and np.array_equal(state.nnodes.cpu().numpy(), ref.nnodes) and np.array_equal(state.status.cpu().numpy(), ref.status))


# ---- advance ------------------------------------------------------------------------------------------------------------------------
def test_advance_equals_the_restatement_over_a_random_walk(dev):
    """40 rounds with slot reuse, inactive rows, slot numbers outside the pool (such a row is inactive) and prefixes that reach Lcap =
    16: lists, lengths, node counts, status and the per-row (node, position) equal the restatement exactly after every round"""
    from emoasr_amd import lm_tree
    Lcap, cap = 16, 170
    state, ref = lm_tree.TreeState(S, W, S * PER, Lcap, cap, dev), T.Tree(S, W, S * PER, Lcap, cap)
    walk = T.Walk(5, S, W, PER, 40, off=OFF, rows=ROWS, keep=3,
                  bad={2: [(1, "src", -1), (2, "dst", S * PER)], 3: [(5, "dst", 1 << 40)], 4: [(6, "src", S * PER), (9, "dst", -1)]})
    planted = 0
    for rnd in range(40):
        lab, src, dst, act = walk.next_round()
        planted += sum(int(act[r] != 0 and not (0 <= src[r] < S * PER and 0 <= dst[r] < S * PER)) for r in range(S * W))
        node, pos = ref.advance(src, dst, act)
        state.advance(_i64(src, dev), _i64(dst, dev), _i64(act, dev))
        assert np.array_equal(state.row_node.cpu().numpy(), node) and np.array_equal(state.row_pos.cpu().numpy(), pos), rnd
        assert _same(state, ref), rnd
        walk.commit(node)
    assert planted >= 3 and bool((ref.status & T.OVERLEN).any()) and int(ref.llen.max()) == Lcap and int(ref.nnodes.sum()) > 400


def test_advance_at_the_capacity_limits_writes_nothing(dev):
    """a full pool raises POOL_FULL for the rows past the last node, a prefix at Lcap raises OVERLEN: the refused rows' destination
    lists and lengths keep their sentinel fill, nothing else moves but the bit"""
    from emoasr_amd import lm_tree
    state, ref = lm_tree.TreeState(2, 4, 16, 3, 5, dev), T.Tree(2, 4, 16, 3, 5)
    act = [1, 1, 0, 1, 1, 1, 1, 1]

    def both(src, dst, active, refused=()):
        for slot in refused:          # sentinel fills where a refused row would have written
            ref.lanc[slot], ref.llen[slot] = SENT, SENT
            state.lanc[slot], state.llen[slot] = SENT, SENT
        node, pos = ref.advance(np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(active, np.int64))
        state.advance(_i64(src, dev), _i64(dst, dev), _i64(active, dev))
        assert np.array_equal(state.row_node.cpu().numpy(), node) and np.array_equal(state.row_pos.cpu().numpy(), pos)
        assert _same(state, ref)
        for slot in refused:
            assert bool((state.lanc[slot] == SENT).all()) and int(state.llen[slot]) == SENT
        return node.tolist()

    assert both([0, 0, 0, 0, 8, 8, 8, 8], [1, 2, 3, 4, 9, 10, 11, 12], act) == [0, 1, -1, 2, 5, 6, 7, 8]
    assert both([1, 2, 0, 4, 9, 9, 10, 11], [5, 6, 7, 3, 13, 14, 15, 8], act, refused=(7, 3, 14, 15)) == [3, 4, -1, -1, 9, -1, -1, -1]
    assert state.status.tolist() == [T.POOL_FULL, T.POOL_FULL] and state.nnodes.tolist() == [5, 5]
    assert both([1, 9, 0, 0, 8, 8, 8, 8], [7, 3, 7, 3, 14, 15, 14, 15], [1, 0, 0, 0, 0, 0, 0, 1], refused=(7, 15)) == [-1] * 8      # still full
    # a prefix at Lcap = 3
    state, ref = lm_tree.TreeState(1, 2, 8, 3, 50, dev), T.Tree(1, 2, 8, 3, 50)
    for k in range(3):
        assert min(both([k, k], [k + 1, 7], [1, 1])) >= 0
    assert both([3, 0], [4, 5], [1, 1], refused=(4,)) == [-1, 6] and state.status.tolist() == [T.OVERLEN]
    # slot numbers outside the pool: the row is inactive, no node is taken, no bit is raised
    state, ref = lm_tree.TreeState(1, 4, 8, 3, 50, dev), T.Tree(1, 4, 8, 3, 50)
    assert both([-1, 0, 8, 0], [1, 8, 2, 1 << 40], [1, 1, 1, 1], refused=(1, 2)) == [-1] * 4
    assert state.status.tolist() == [0] and state.nnodes.tolist() == [0]


def test_entry_points_refuse_what_is_outside_the_plan(dev):
    from emoasr_amd import lib, lm_tree
    state = lm_tree.TreeState(1, 4, 8, 8129, 4, dev)
    qkv = torch.zeros(4, 3 * 64, device=dev)
    pool, dst = torch.zeros(4, 64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(lib.EmoasrHipError, match="bytes of LDS"):
        state.attn(qkv, pool, pool.clone(), dst, 8)
    state = lm_tree.TreeState(1, 4, 8, 16, 4, dev)
    with pytest.raises(lib.EmoasrHipError, match="unsupported"):
        state.attn(qkv, pool, pool.clone(), dst, 16)          # heads 4 wide
    with pytest.raises(lib.EmoasrHipError, match="unsupported"):
        lm_tree.TreeState(1, 65, 8, 16, 1, dev).advance(dst, dst, dst)


# ---- gathered attention -----------------------------------------------------------------------------------------------------------------
LCAP = 200
LENGTHS = (1, 2, 63, 64, 65, 128, 129, LCAP, 0, 17, 0, 100)          # mixed within one launch; 0: a row without a node


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d,H", [(256, 4), (256, 2), (64, 8), (128, 4)])
def test_gathered_attention_against_f64(dev, d, H, dtype):
    """dk = 64, 128, 8, 32; the lists are a random permutation inside a pool larger than needed (a dense read cannot pass).  The new
    k / v land at the row's node bit for bit and nowhere else, rows without a node write nothing, the output is within one output
    ulp + 4 e32 of the float64 attention over the rounded inputs"""
    from emoasr_amd import lm_tree
    Ss, Ws = 3, 4
    R, nslots, cap = Ss * Ws, 20, 400
    rs = np.random.RandomState(d + 7 * H)
    g = torch.Generator().manual_seed(d + 7 * H)
    state = lm_tree.TreeState(Ss, Ws, nslots, LCAP, cap, dev)
    nodes = Ss * cap
    assert sum(LENGTHS) < nodes
    perm = rs.permutation(nodes)
    slots = rs.permutation(nslots)[:R]
    llen, lanc = np.zeros(nslots, np.int32), np.full((nslots, LCAP), SENT, np.int32)
    row_node, k = np.full(R, -1, np.int32), 0
    for r, n in enumerate(LENGTHS):
        if n:
            llen[slots[r]], lanc[slots[r], :n] = n, perm[k:k + n]
            row_node[r], k = perm[k + n - 1], k + n
        else:
            llen[slots[r]] = rs.randint(1, LCAP)          # a slot with a list, but the row has no node: nothing happens
            lanc[slots[r], :llen[slots[r]]] = perm[-LCAP:][:llen[slots[r]]]
    state.llen.copy_(torch.from_numpy(llen))
    state.lanc.copy_(torch.from_numpy(lanc))
    state.row_node.copy_(torch.from_numpy(row_node))
    qkv = torch.randn(R, 3 * d, generator=g).to(dtype)
    kp, vp = torch.randn(nodes, d, generator=g).to(dtype), torch.randn(nodes, d, generator=g).to(dtype)
    f64 = lambda t: t.double().cpu().numpy()
    ref, k_ref, v_ref = T.gathered_attn_ref(f64(qkv), f64(kp), f64(vp), lanc, llen, row_node, slots, H)
    m32, _, _ = T.gathered_attn_ref(f64(qkv), f64(kp), f64(vp), lanc, llen, row_node, slots, H, dtype=np.float32)
    kd, vd = kp.to(dev), vp.to(dev)
    out = state.attn(qkv.to(dev), kd, vd, _i64(slots, dev), H, out=torch.full((R, d), 7.0, device=dev, dtype=dtype))
    assert np.array_equal(f64(kd), k_ref) and np.array_equal(f64(vd), v_ref)          # the new rows at their nodes, the rest untouched
    on = row_node >= 0
    got = f64(out)
    assert bool((got[~on] == 7.0).all()) and int(on.sum()) == R - 2
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    e32 = float(np.abs(m32[on].astype(np.float64) - ref[on]).max())
    err = np.abs(got[on] - ref[on])
    share = float((err / (ulp * np.abs(ref[on]) + 4 * e32)).max())
    print(f"[measured] lm_tree_attn d={d} H={H} {dtype}: err {err.max():.2e} (f32 model {e32:.2e}) {share:.2f} of bound")
    assert np.isfinite(got[on]).all() and share <= 1.0, (float(err.max()), e32, share)


# ---- the whole step, by a random tree walk ----------------------------------------------------------------------------------------------
ROUNDS = 30
_WALK = {}


def _lm(dtype, dev):
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**LM_CFG), compute_dtype=dtype)
    lm.load_state_dict(load_ctc_beam_golden()[2])
    lm = lm.to(dev).eval()
    lm._prepare()
    return lm


def _dense_chain(lm, seqs, dev):
    """emoasr_bert_lm_step (its launch chain: more than 16 rows) on dense caches, every sequence of seqs one row, stepped position by
    position -> f32 log-probabilities after each row's last token [len(seqs), V]"""
    from emoasr_amd import lib, ops
    from emoasr_amd.decode_rt import LMStepRuntime, _lin, _ln
    P = lm.params
    A, layers = LMStepRuntime(lm)._params()
    d, H, F, V, nl = P.hidden_size, P.num_attention_heads, P.intermediate_size, P.vocab_size, P.num_layers
    nb, Lmax = max(len(seqs), 17), max(map(len, seqs))
    dtype = A.shadow.dtype
    code = lib.BF16 if dtype == torch.bfloat16 else lib.F32
    fn = lib.load().emoasr_decode_step_ws_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * 6
    ws = torch.zeros(int(fn(code, nb, d, H, F, V)), device=dev, dtype=torch.uint8)
    kc, vc = (torch.zeros(nl, nb, Lmax, d, device=dev, dtype=dtype) for _ in range(2))
    ids, pos, klens = (torch.zeros(n, device=dev, dtype=torch.int32) for n in (nb, 1, nb))
    logp, out = torch.zeros(nb, V, device=dev), torch.zeros(len(seqs), V)
    pre, cp = "lm.transformer.bert.", "lm.transformer.cls.predictions."
    io = lib.BertStep()
    io.nb, io.Lmax, io.d, io.H, io.F, io.V = nb, Lmax, d, H, F, V
    io.ids, io.pos, io.klens = ids.data_ptr(), pos.data_ptr(), klens.data_ptr()
    io.word_emb, io.pe = A.w(pre + "embeddings.word_embeddings.weight").data_ptr(), lm._pe.data_ptr()
    _ln(io.ln_emb, A.p(pre + "embeddings.LayerNorm.weight"), A.p(pre + "embeddings.LayerNorm.bias"))
    io.kcache, io.vcache = kc.data_ptr(), vc.data_ptr()
    _lin(io.transform, A.w(cp + "transform.dense.weight"), A.p(cp + "transform.dense.bias"))
    _ln(io.ln_transform, A.p(cp + "transform.LayerNorm.weight"), A.p(cp + "transform.LayerNorm.bias"))
    io.out_bias, io.logp, io.raw_logits = A.p(cp + "bias").data_ptr(), logp.data_ptr(), 0
    io.ws, io.ws_bytes = ws.data_ptr(), ws.numel()
    for p in range(Lmax):
        ids.copy_(torch.tensor([s[p] if p < len(s) else 0 for s in seqs] + [0] * (nb - len(seqs)), dtype=torch.int32))
        pos.fill_(p)
        klens.fill_(p + 1)
        lib.call("emoasr_bert_lm_step", code, nl, layers, ctypes.byref(io), ops._stream())
        host = logp.cpu()
        for i, s in enumerate(seqs):
            if len(s) == p + 1:
                out[i] = host[i]
    return out


def tree_walk_distance(dtype, dev):
    """-> (tree, dense): the largest distance of the tree step's log-softmaxed logits, and of emoasr_bert_lm_step's chain form on
    dense caches, from oracle.decoder.lm_logits in double over the prefixes of a 30-round random walk at R = 37 (once per dtype)"""
    if dtype in _WALK:
        return _WALK[dtype]
    from emoasr_amd import lm_tree
    from oracle import decoder as od
    lm = _lm(dtype, dev)
    P = lm.params
    state = lm_tree.TreeState(S, W, S * PER, P.max_seq_len, W * ROUNDS + 1, dev)
    walk = T.Walk(11, S, W, PER, P.vocab_size, off=OFF, rows=ROWS, keep=3)
    ctl = torch.zeros(4, S * W, dtype=torch.int64, device=dev)
    step = lm_tree.TreeStep(lm, state, ctl[0], ctl[2])
    seqs, got = [], []
    for _ in range(ROUNDS):
        words = walk.next_round()
        ctl.copy_(torch.from_numpy(np.stack(words)))
        state.advance(ctl[1], ctl[2], ctl[3])
        logits = step().double().cpu()
        node = state.row_node.cpu().numpy()
        walk.commit(node)
        for r in np.nonzero(node >= 0)[0]:
            seqs.append(tuple(walk.seq[int(words[2][r])]))
            got.append(torch.log_softmax(logits[r], -1))
    assert not state.status.any() and len(seqs) > 15 * ROUNDS and max(map(len, seqs)) >= 10
    sd64 = {k: v.double() for k, v in load_ctc_beam_golden()[2].items()}
    n = max(map(len, seqs))
    ys = torch.zeros(len(seqs), n, dtype=torch.int64)
    for i, s in enumerate(seqs):
        ys[i, :len(s)] = torch.tensor(s)
    lens = torch.tensor([len(s) for s in seqs])
    with torch.no_grad():
        ref = torch.log_softmax(od.lm_logits(sd64, P, ys, lens), -1)[torch.arange(len(seqs)), lens - 1]
    uniq = sorted(set(seqs))
    dense = _dense_chain(lm, uniq, dev).double()
    at = {s: i for i, s in enumerate(uniq)}
    e_tree = float((torch.stack(got) - ref).abs().max())
    e_dense = float((dense[[at[s] for s in seqs]] - ref).abs().max())
    _WALK[dtype] = (e_tree, e_dense)
    return _WALK[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_tree_step_against_the_oracle_on_full_prefixes(dev, dtype):
    """advance + emoasr_lm_tree_step over 30 rounds of synthetic control words at R = 37: every row's log-softmaxed logits against the
    oracle LM in double on the row's full prefix, within twice the distance of emoasr_bert_lm_step's chain form on dense caches from
    the same reference on the same prefixes (one margin for the gathered summation order, one for products over 37 rows)"""
    e_tree, e_dense = tree_walk_distance(dtype, dev)
    print(f"[measured] tree step {dtype}: {e_tree:.3e} from the f64 oracle; emoasr_bert_lm_step (chain, dense caches) {e_dense:.3e}; "
          f"allowed {2 * e_dense:.3e}")
    assert e_tree <= 2.0 * e_dense, (e_tree, e_dense)
