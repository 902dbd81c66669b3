"""The kernels of the Transformer-LM fusion over a prefix tree inside the fused CTC search (csrc/lm_tree.hip) on
the device, every buffer between guard words: emoasr_lm_tree_advance_rec against its numpy model (tests/ctc_tree_ref.py) over walks of
shuffled record lists -- node names are the kernel's own, so the comparison goes through the label lists --, at both capacity limits
and on malformed records; emoasr_log_softmax_rows_to bit for bit against ops.log_softmax; emoasr_lm_tree_attn_rows against the float64
attention over the gathered rows and emoasr_lm_tree_step_rows against the oracle LM in double, with the comparisons and bars of
tests/test_lm_tree_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from tests import ctc_tree_ref as C
from tests import lm_tree_ref as T
from tests.util import load_ctc_beam_golden

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -7


class Guarded:
    """tensors cut out of buffers with GUARD sentinel elements on either side; intact(): no guard word has changed"""

    def __init__(self, dev):
        self.dev, self.held = dev, []

    def __call__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        mark = 93
        buf = torch.full((n + 2 * GUARD,), mark, device=self.dev, dtype=dtype)
        buf[GUARD:GUARD + n] = fill
        self.held.append((buf, n, mark))
        return buf[GUARD:GUARD + n].view(*shape)

    def intact(self):
        return all(bool((b[:GUARD] == m).all()) and bool((b[GUARD + n:] == m).all()) for b, n, m in self.held)


def guarded_tree(g, S, W, slots, Lcap, cap, dev, rows=None):
    """a TreeState whose every array (and control words) lies between guard words"""
    from emoasr_amd import lm_tree
    st = lm_tree.TreeState(S, W, S * slots, Lcap, cap, dev, rows=rows)
    i32 = torch.int32
    st.llen, st.lanc = g((S * slots,), i32, 0), g((S * slots, Lcap), i32, SENT)
    st.nnodes, st.status = g((S,), i32, 0), g((S,), i32, 0)
    st.row_node, st.row_pos = g((st.rows,), i32, SENT), g((st.rows,), i32, SENT)
    st.ctl = g((2, st.rows), torch.int64, SENT)
    c = st.c
    c.llen, c.lanc, c.nnodes = st.llen.data_ptr(), st.lanc.data_ptr(), st.nnodes.data_ptr()
    c.row_node, c.row_pos, c.status = st.row_node.data_ptr(), st.row_pos.data_ptr(), st.status.data_ptr()
    return st


class RecordWalk:
    """record lists in the frame kernel's style for S searches of width W with `slots` pool rows each: the first list holds the roots
    (src = -1), afterwards a search's records take their sources from its live rows and their destinations from rows that are not
    live (never a row a record of the same list reads), at most W per search; the deepest live prefix always survives and is the
    likeliest parent, so lists reach any Lcap.  frame(total) -> the records per search, (node, parent, token, src, dst) with the
    slots counted inside the search as tests/ctc_tree_ref.pack takes them (node and parent ids are not the tree's business: 0)"""

    def __init__(self, seed, S, W, slots, V):
        self.rs, self.S, self.W, self.slots, self.V = np.random.RandomState(seed), S, W, slots, V
        self.live = [[] for _ in range(S)]
        self.started = False

    def frame(self, total):
        S, W, rs = self.S, self.W, self.rs
        if not self.started:
            self.started = True
            for s in range(S):
                self.live[s] = [0]
            return [[(0, -1, C.EOS, -1, 0)] for _ in range(S)]
        counts = [1] * S if total >= S else [0] * S          # (every search grows whenever the list has room for all of them)
        for _ in range(total - sum(counts)):
            open_ = [s for s in range(S) if counts[s] < W]
            counts[open_[rs.randint(len(open_))]] += 1
        out = []
        for s in range(S):
            free = [x for x in range(self.slots) if x not in self.live[s]]
            rs.shuffle(free)
            recs = []
            for i in range(counts[s]):
                src = self.live[s][-1] if (i == 0 or rs.rand() < 0.5) else self.live[s][rs.randint(len(self.live[s]))]
                recs.append((0, 0, int(rs.randint(0, self.V)), src, free.pop()))
            out.append(recs)
            if recs:      # the child of the deepest prefix is the deepest now: it stays, last; W live rows at most
                rest = self.live[s] + [r[4] for r in recs[1:]]
                rs.shuffle(rest)
                self.live[s] = rest[:W - 1] + [recs[0][4]]
        return out


def _run_frame(state, ref, frames, S, W, slots, rs, dev, label_dev, label_ref, lm_weight=None):
    """one list of records, shuffled, with garbage behind it, through the kernel and the model; the comparison through label lists"""
    n = sum(map(len, frames))
    rec, _ = C.pack(frames, S, W, slots, rs.permutation(n))
    rec[:, n:] = rs.randint(-5, 1 << 20, size=(6, rec.shape[1] - n))
    node_r, pos_r, lab_r, dst_r = ref.advance_rec(rec, n, lm_weight)
    rec_dev = torch.from_numpy(rec).to(dev)
    state.advance_records(rec_dev, torch.tensor([n], dtype=torch.int32, device=dev),
                          None if lm_weight is None else torch.tensor(lm_weight, dtype=torch.float64, device=dev))
    node = state.row_node.cpu().numpy()
    assert np.array_equal(node >= 0, node_r >= 0) and (node[n:] == -1).all()
    assert np.array_equal(state.row_pos.cpu().numpy(), pos_r)
    ctl = state.ctl.cpu().numpy()
    assert np.array_equal(ctl[0], lab_r) and np.array_equal(ctl[1], dst_r)
    assert np.array_equal(state.llen.cpu().numpy(), ref.llen) and np.array_equal(state.nnodes.cpu().numpy(), ref.nnodes)
    assert np.array_equal(state.status.cpu().numpy(), ref.status)
    got = node[node >= 0]
    assert len(set(got.tolist())) == len(got)
    for r in np.nonzero(node >= 0)[0]:
        s = int(rec[0, r])
        assert s * ref.node_cap <= node[r] < s * ref.node_cap + ref.nnodes[s]          # inside the search's share, below its count
        assert int(node[r]) not in label_dev
        label_dev[int(node[r])], label_ref[int(node_r[r])] = int(rec[3, r]), int(rec[3, r])
    dev_tree = T.Tree(S, W, S * slots, ref.Lcap, ref.node_cap)
    dev_tree.llen, dev_tree.lanc = state.llen.cpu().numpy(), state.lanc.cpu().numpy()
    assert C.label_lists(dev_tree, label_dev) == C.label_lists(ref, label_ref)
    return node


@pytest.mark.parametrize("Lcap", [1, 2, 64, 65])
@pytest.mark.parametrize("W", [1, 4, 32])
@pytest.mark.parametrize("S", [1, 3])
def test_advance_rec_against_the_numpy_model(dev, S, W, Lcap):
    """record counts 0, 1, 64, 65 and S W (those the list can hold) among random ones, records in shuffled order, garbage behind the
    count; prefixes run into Lcap (OVERLEN, the row without effect) either side of one wave's copy stride"""
    g = Guarded(dev)
    slots, frames_n = 2 * W + 2, (70 if Lcap >= 64 else 8)
    cap = W * frames_n + 1
    state, ref = guarded_tree(g, S, W, slots, Lcap, cap, dev, rows=S * W), C.RecTree(S, W, slots, Lcap, cap)
    walk, rs = RecordWalk(S * 100 + W * 10 + Lcap, S, W, slots, 50), np.random.RandomState(Lcap)
    counts = [S] + [n for n in (0, 1, 64, 65, S * W) if n <= S * W]
    label_dev, label_ref, deepest = {}, {}, 0
    for f in range(frames_n):
        total = counts[f] if f < len(counts) else int(rs.randint(S, S * W + 1))
        before = (state.llen.clone(), state.lanc.clone(), state.nnodes.clone())
        _run_frame(state, ref, walk.frame(total), S, W, slots, rs, dev, label_dev, label_ref)
        if f and total == 0:          # n = 0: nothing changes
            assert all(torch.equal(a, b) for a, b in zip(before, (state.llen, state.lanc, state.nnodes)))
        assert g.intact(), f
        deepest = max(deepest, int(ref.llen.max()))
    assert deepest == Lcap and bool((ref.status & C.OVERLEN).all()) and not (ref.status & C.POOL_FULL).any()


def test_advance_rec_limits_raise_bits_for_their_search_alone(dev):
    """OVERLEN at p = Lcap and POOL_FULL with node_cap = 2: the bit for that search only, the refused row without effect (its
    destination keeps the sentinel fill), the other rows proceed; a search with lm_weight <= 0 takes no node"""
    g = Guarded(dev)
    S, W, slots = 2, 4, 10
    rs = np.random.RandomState(0)
    state, ref = guarded_tree(g, S, W, slots, 2, 50, dev, rows=S * W), C.RecTree(S, W, slots, 2, 50)
    ld, lr = {}, {}
    _run_frame(state, ref, [[(0, -1, 2, -1, 0)], [(0, -1, 2, -1, 0)]], S, W, slots, rs, dev, ld, lr)
    _run_frame(state, ref, [[(0, 0, 5, 0, 1)], [(0, 0, 6, 0, 1)]], S, W, slots, rs, dev, ld, lr)
    node = _run_frame(state, ref, [[(0, 0, 7, 0, 2)], [(0, 0, 8, 1, 2), (0, 0, 9, 0, 3)]], S, W, slots, rs, dev, ld, lr)   # search 1: p = 2
    assert state.status.tolist() == [0, C.OVERLEN] and node.tolist().count(-1) == 6
    assert int(state.llen[slots + 2]) == 0 and bool((state.lanc[slots + 2] == SENT).all()) and int(state.llen[slots + 3]) == 2
    # node_cap = 2: the root, then three records of search 0 for one node (which of them gets it is the kernel's business)
    state = guarded_tree(g, S, W, slots, 8, 2, dev, rows=S * W)
    rec, n = C.pack([[(0, -1, 2, -1, 0)], [(0, -1, 2, -1, 0)]], S, W, slots)
    count = lambda k: torch.tensor([k], dtype=torch.int32, device=dev)
    state.advance_records(torch.from_numpy(rec).to(dev), count(n))
    rec, n = C.pack([[(0, 0, 5, 0, 1), (0, 0, 6, 0, 2), (0, 0, 7, 0, 3)], [(0, 0, 8, 0, 1)]], S, W, slots, [2, 3, 0, 1])
    state.advance_records(torch.from_numpy(rec).to(dev), count(n))
    node = state.row_node.tolist()
    assert state.status.tolist() == [C.POOL_FULL, 0] and state.nnodes.tolist() == [2, 2]
    assert node[1] == 3 and sorted(node[i] for i in (0, 2, 3)) == [-1, -1, 1] and node[4:] == [-1] * 4
    taken = [int(rec[5, i]) for i in (0, 2, 3) if node[i] >= 0]
    for slot in (1, 2, 3):
        if slot in taken:
            assert int(state.llen[slot]) == 2 and state.lanc[slot, :2].tolist() == [0, 1]
        else:
            assert int(state.llen[slot]) == 0 and bool((state.lanc[slot] == SENT).all())
    assert int(state.llen[slots + 1]) == 2 and state.lanc[slots + 1, :2].tolist() == [2, 3]
    # lm_weight <= 0: no node, no bit
    state, ref = guarded_tree(g, S, W, slots, 8, 2, dev, rows=S * W), C.RecTree(S, W, slots, 8, 2)
    _run_frame(state, ref, [[(0, -1, 2, -1, 0)], [(0, -1, 2, -1, 0)]], S, W, slots, rs, dev, {}, {}, lm_weight=[0.5, 0.0])
    assert state.nnodes.tolist() == [1, 0] and state.status.tolist() == [0, 0] and state.row_node.tolist()[:2].count(-1) == 1
    assert g.intact()


def test_advance_rec_malformed_records_write_nothing(dev):
    """a search of -1 or S, a slot in another search's share, negative and huge slots: row_node = -1, nothing else moves, guards intact"""
    g = Guarded(dev)
    S, W, slots = 2, 4, 10
    state, ref = guarded_tree(g, S, W, slots, 8, 50, dev, rows=S * W), C.RecTree(S, W, slots, 8, 50)
    _run_frame(state, ref, [[(0, -1, 2, -1, 0)], [(0, -1, 2, -1, 0)]], S, W, slots, np.random.RandomState(1), dev, {}, {})
    before = (state.llen.clone(), state.lanc.clone(), state.nnodes.clone(), state.status.clone())
    big = (1 << 31) - 1
    bad = [(-1, 0, 0, 5, 0, 3), (S, 0, 0, 5, 0, 3), (0, 0, 0, 5, 0, slots + 1), (0, 0, 0, 5, slots, 3), (1, 0, 0, 5, slots, 3),
           (1, 0, 0, 5, slots, -1), (0, 0, 0, 5, 0, big), (big, 0, 0, big, big, big)]
    rec = torch.tensor(bad, dtype=torch.int32).t().contiguous().to(dev)
    for n in (len(bad), big, -1):
        state.advance_records(rec, torch.tensor([n], dtype=torch.int32, device=dev))
        assert state.row_node.tolist() == [-1] * 8 and state.ctl[1].tolist() == [-1] * 8
        assert all(torch.equal(a, b) for a, b in zip(before, (state.llen, state.lanc, state.nnodes, state.status)))
    assert g.intact()


# ---- log_softmax_rows_to ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V_lm,V", [(40, 40), (41, 40), (1000, 1000), (1025, 1000)])
def test_log_softmax_rows_to_is_log_softmax_bit_for_bit(dev, V_lm, V, dtype):
    """normalised over all V_lm columns, the first V go to the destination row of the pool (ld_lm > V); n < R; rows and columns the
    call does not own keep their fill; a row that row_ok refuses or that names no pool row is dropped"""
    from emoasr_amd import ops
    g = Guarded(dev)
    R, n, rows, ld = 9, 7, 12, V + 5
    x = g((R, V_lm), dtype, 0)
    x.copy_((torch.randn(R, V_lm, generator=torch.Generator().manual_seed(V_lm)) * 4).to(dtype))
    pool = g((rows, ld), torch.float32, 7.0)
    dst = g((R,), torch.int32, 0)
    dst.copy_(torch.tensor([3, 0, 11, 5, 12, 8, -1, 1, 2], dtype=torch.int32))          # row 4: past the pool, row 6: negative
    ok = g((R,), torch.int32, 0)
    ok[5] = -1
    ops.log_softmax_rows_to(x, n, dst, pool, V, row_ok=ok)
    want = ops.log_softmax(x)[:, :V]
    written = {3: 0, 0: 1, 11: 2, 5: 3}
    for o in range(rows):
        if o in written:
            assert torch.equal(pool[o, :V], want[written[o]]) and bool((pool[o, V:] == 7.0).all()), o
        else:
            assert bool((pool[o] == 7.0).all()), o
    ops.log_softmax_rows_to(x, n, dst, pool, V)          # without row_ok row 5 goes to pool row 8
    assert torch.equal(pool[8, :V], want[5]) and bool((pool[8, V:] == 7.0).all()) and bool((pool[1] == 7.0).all())
    ops.log_softmax_rows_to(x, 0, dst, pool, V)
    assert g.intact()


# ---- attn_rows ----------------------------------------------------------------------------------------------------------------------
CAP_ROWS, LCAP = 64, 200


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", [1, 16, 17, 33])
def test_attn_rows_against_f64(dev, R, dtype):
    """R rows out of a capacity of 64, lists of mixed lengths through a permuted pool: the bound of
    tests/test_lm_tree_kernels_gpu.py (one output ulp + 4 x the f32 numpy model's own error); rows >= R write neither their output
    nor their key / value; R = S W is the old entry point bit for bit"""
    g = Guarded(dev)
    d, H, S, W, nslots, cap = 128, 4, 16, 4, 80, 300
    rs, gen = np.random.RandomState(R), torch.Generator().manual_seed(R)
    state = guarded_tree(g, S, W, nslots // S, LCAP, cap, dev, rows=CAP_ROWS)
    nodes = S * cap
    lengths = [(1, 2, 63, 64, 65, 128, 129, LCAP, 0, 17)[r % 10] for r in range(CAP_ROWS)]
    perm, slots = rs.permutation(nodes), rs.permutation(nslots)[:CAP_ROWS]
    llen, lanc = np.zeros(nslots, np.int32), np.full((nslots, LCAP), SENT, np.int32)
    row_node, k = np.full(CAP_ROWS, -1, np.int32), 0
    for r, n in enumerate(lengths):
        if n:
            llen[slots[r]], lanc[slots[r], :n] = n, perm[k:k + n]
            row_node[r], k = perm[k + n - 1], k + n
    assert k <= nodes
    state.llen.copy_(torch.from_numpy(llen))
    state.lanc.copy_(torch.from_numpy(lanc))
    state.row_node.copy_(torch.from_numpy(row_node))
    qkv = g((CAP_ROWS, 3 * d), dtype, 0)
    qkv.copy_(torch.randn(CAP_ROWS, 3 * d, generator=gen).to(dtype))
    kp, vp = torch.randn(nodes, d, generator=gen).to(dtype), torch.randn(nodes, d, generator=gen).to(dtype)
    f64 = lambda t: t.double().cpu().numpy()
    masked = np.where(np.arange(CAP_ROWS) < R, row_node, -1)
    ref, k_ref, v_ref = T.gathered_attn_ref(f64(qkv), f64(kp), f64(vp), lanc, llen, masked, slots, H)
    m32 = T.gathered_attn_ref(f64(qkv), f64(kp), f64(vp), lanc, llen, masked, slots, H, dtype=np.float32)[0]
    kd, vd = g((nodes, d), dtype, 0), g((nodes, d), dtype, 0)
    kd.copy_(kp)
    vd.copy_(vp)
    dst = g((CAP_ROWS,), torch.int64, 0)
    dst.copy_(torch.from_numpy(slots.astype(np.int64)))
    out = state.attn(qkv, kd, vd, dst, H, out=g((CAP_ROWS, d), dtype, 7.0), n=R)
    assert np.array_equal(f64(kd), k_ref) and np.array_equal(f64(vd), v_ref)          # keys / values of the first R rows only
    on = masked >= 0
    got = f64(out)
    assert bool((got[~on] == 7.0).all())
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    e32 = float(np.abs(m32[on].astype(np.float64) - ref[on]).max())
    err = np.abs(got[on] - ref[on])
    share = float((err / (ulp * np.abs(ref[on]) + 4 * e32)).max())
    print(f"[measured] lm_tree_attn_rows R={R} {dtype}: err {err.max():.2e} (f32 model {e32:.2e}) {share:.2f} of bound")
    assert np.isfinite(got[on]).all() and share <= 1.0, (float(err.max()), e32, share)
    if R == 33:          # the whole capacity: the old entry point, bit for bit
        a = state.attn(qkv, kd, vd, dst, H, out=g((CAP_ROWS, d), dtype, 7.0), n=CAP_ROWS)
        b = state.attn(qkv, kd, vd, dst, H, out=g((CAP_ROWS, d), dtype, 7.0))
        assert torch.equal(a, b) and int((row_node >= 0).sum()) == int((a[:, 0] != 7.0).sum())
    assert g.intact()


# ---- step_rows, driven by advance_rec -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_step_rows_against_the_oracle_on_full_prefixes(dev, dtype):
    """advance_rec + emoasr_lm_tree_step_rows over record lists of 1, 16, 17 and 33 rows out of a capacity of 64: every row's
    log-softmaxed logits against the oracle LM in double on the row's full prefix, within twice the distance of
    emoasr_bert_lm_step's chain form on dense caches from the same reference on the same prefixes (the bar of
    test_tree_step_against_the_oracle_on_full_prefixes); the logits of rows >= R keep their fill; R = the capacity is
    emoasr_lm_tree_step bit for bit"""
    from emoasr_amd import lm_tree
    from oracle import decoder as od
    from tests.test_lm_tree_kernels_gpu import _dense_chain, _lm
    g = Guarded(dev)
    lm = _lm(dtype, dev)
    P = lm.params
    S, W = 8, 8
    slots, frames_n = 2 * W + 2, 14
    state = guarded_tree(g, S, W, slots, P.max_seq_len, W * frames_n + 1, dev, rows=CAP_ROWS)
    step = lm_tree.TreeStep(lm, state)
    V = P.vocab_size
    step.logits = g((CAP_ROWS, V), step.logits.dtype, 0)
    step.io.logits = step.logits.data_ptr()
    walk, rs = RecordWalk(3, S, W, slots, V), np.random.RandomState(4)
    seq_of, seqs, got = {}, [], []
    for f in range(frames_n):
        total = S if f == 0 else (1, 16, 17, 33, 64)[f % 5]
        frames = walk.frame(total)
        n = sum(map(len, frames))
        rec, _ = C.pack(frames, S, W, slots, rs.permutation(n))
        step.logits.fill_(77.0)
        state.advance_records(torch.from_numpy(rec).to(dev), torch.tensor([n], dtype=torch.int32, device=dev))
        logits = step(n)
        assert bool((logits[n:] == 77.0).all()) and bool((state.row_node[:n] >= 0).all())
        if n == CAP_ROWS:
            first = logits.clone()
            assert torch.equal(step(), first)          # (the keys / values it writes again are the same values)
        host = logits[:n].double().cpu()
        new = {}
        for r in range(n):
            src, dst = int(rec[4, r]), int(rec[5, r])
            new[dst] = (seq_of[src] if src >= 0 else ()) + (int(rec[3, r]),)
            seqs.append(new[dst])
            got.append(torch.log_softmax(host[r], -1))
        seq_of.update(new)
    assert not state.status.any() and g.intact() and max(map(len, seqs)) >= 10
    sd64 = {k: v.double() for k, v in load_ctc_beam_golden()[2].items()}
    ys = torch.zeros(len(seqs), max(map(len, seqs)), dtype=torch.int64)
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
    print(f"[measured] tree step_rows {dtype}: {e_tree:.3e} from the f64 oracle over {len(seqs)} rows; emoasr_bert_lm_step (chain, "
          f"dense caches) {e_dense:.3e}; allowed {2 * e_dense:.3e}")
    assert e_tree <= 2.0 * e_dense, (e_tree, e_dense)
