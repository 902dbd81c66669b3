"""The kernels of the Transformer-LM fusion inside the batched LAS beam search (csrc/lm_tree.hip) on the device,
every buffer between guard words: emoasr_lm_tree_advance_beam exactly against its numpy restatement (tests/las_tree_ref.py) -- node
names are deterministic, so every array compares --, and the LM part of the chain (advance, emoasr_lm_tree_step,
emoasr_log_softmax_rows_to) against the oracle LM in double, with the bar of tests/test_lm_tree_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from tests import las_tree_ref as R
from tests.test_ctc_tree_kernels_gpu import SENT, Guarded, guarded_tree
from tests.util import load_ctc_beam_golden

pytestmark = pytest.mark.gpu

S5, LCAP, STEPS = 5, 16, 18
DONE = 3                     # the finished search


def _book(g, ids, parent, state, dev):
    """the book's arrays between guard words"""
    i32 = torch.int32
    out = []
    for a in (ids, parent, state):
        t = g(tuple(a.shape), i32, 0)
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        out.append(t)
    return out


def _alive(W):
    """search 0: counts from -2 to W + 7 (clamped), zeros among them; 1: always W (it reaches Lcap and uses up a small share);
    2: W, shrinking to 0 over the last steps; 3: finished; 4: random"""
    rs = np.random.RandomState(W)
    odd = [W + 7, 0, -2, W, 1]

    def alive(i, s):
        if s == 0:
            return odd[i % len(odd)]
        if s == 2:
            return max(0, min(W, STEPS - 2 - i))
        if s == 4:
            return int(rs.randint(0, W + 1))
        return W
    return alive


@pytest.mark.parametrize("tight", [False, True], ids=["roomy", "tight"])
@pytest.mark.parametrize("W", [1, 3, 10, 32])
def test_advance_beam_equals_the_restatement(dev, W, tight):
    """S = 5, Lcap = 16, 18 steps alternating the halves: lanc, llen, nnodes, status, row_node, row_pos, lab and dst equal the numpy
    restatement after every step.  Random parents inside the search, planted parents outside it (they read the search's row 0),
    n_alive from below 0 to above W, one finished search, junk in the dead rows' ids / parent; roomy: the always-full search runs
    into Lcap at step 16 (OVERLEN), tight: node_cap = 3 W + 2 is used up in the middle of a wave (POOL_FULL).  The lists of refused
    and dead rows keep their sentinel fill."""
    g = Guarded(dev)
    S, nb = S5, S5 * W
    cap = 3 * W + 2 if tight else W * STEPS + 1
    tree, ref = guarded_tree(g, S, W, 2 * W, LCAP, cap, dev), R.BeamTree(S, W, LCAP, cap)
    assert tree.nslots == 2 * nb
    ref.lanc[:] = SENT
    far = W + (W - 1)        # a row of the next search
    bad = {3: [(1 * W, 1 * W + far)], 5: [(4 * W, -1)], 7: [(1 * W + W - 1, 1 << 30)], 9: [(1 * W, 0)], 10: [(2 * W, 3 * W)]}
    walk = R.BookWalk(100 + W, S, W, 50, done=(DONE,), alive=_alive(W), bad=bad)
    node_label = {}
    for i in range(STEPS):
        ids, parent, state = walk.next_step()
        d_ids, d_parent, d_state = _book(g, ids, parent, state, dev)
        src_base, dst_base = R.halves(i, nb)
        want = ref.advance_beam(ids, parent, state, src_base, dst_base)
        tree.advance_beam(d_ids, d_parent, d_state, src_base, dst_base)
        got = (tree.row_node.cpu().numpy(), tree.row_pos.cpu().numpy(), tree.ctl[0].cpu().numpy(), tree.ctl[1].cpu().numpy())
        for name, a, b in zip(("row_node", "row_pos", "lab", "dst"), got, want):
            assert np.array_equal(a, b), (i, name, a, b)
        for name in ("llen", "lanc", "nnodes", "status"):
            assert np.array_equal(getattr(tree, name).cpu().numpy(), getattr(ref, name)), (i, name)
        assert g.intact(), i
        for r in np.nonzero(want[0] >= 0)[0]:
            node_label[int(want[0][r])] = int(ids[r])
        walk.commit(want[0])
        for half in (0, 1):
            for r, seq in walk.seq[half].items():
                assert R.labels(ref, half * nb + r, node_label) == seq, (i, half, r)
    status = ref.status.tolist()
    assert status[DONE] == 0 and ref.nnodes[DONE] == 0
    dead = ref.lanc[[DONE * W + w for w in range(W)] + [nb + DONE * W + w for w in range(W)]]
    assert (dead == SENT).all()                                   # nothing of the finished search was written
    if tight:
        assert status[1] == R.POOL_FULL and ref.nnodes[1] == cap and not any(b & R.OVERLEN for b in status)
    else:
        assert status[1] == R.OVERLEN and int(ref.llen.max()) == LCAP and not any(b & R.POOL_FULL for b in status)


def test_advance_beam_refuses_halves_that_do_not_lie_apart(dev):
    from emoasr_amd import lib
    g = Guarded(dev)
    S, W = 2, 3
    tree = guarded_tree(g, S, W, 2 * W, 4, 9, dev)
    ids, parent, state = _book(g, np.zeros(6, np.int32), np.zeros(6, np.int32), np.zeros((2, 4), np.int32), dev)
    for src_base, dst_base in ((0, 0), (0, 5), (6, 7), (-1, 6), (0, 7)):
        with pytest.raises(lib.EmoasrHipError, match="lm_tree_advance_beam: halves"):
            tree.advance_beam(ids, parent, state, src_base, dst_base)
    assert g.intact() and not tree.nnodes.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_chain_lm_part_against_the_oracle_on_full_prefixes(dev, dtype):
    """advance_beam + emoasr_lm_tree_step + emoasr_log_softmax_rows_to (identity row map, row_ok = row_node) on a 12-step walk at
    S = 4, W = 3: the f32 row of every live row against the oracle LM in double on the row's full prefix, within twice the distance
    of emoasr_bert_lm_step's chain form on dense caches from the same reference on the same prefixes (section 30's bar: measured
    against existing code, the factor 2 covers another summation order); rows without a node keep the buffer's fill"""
    from emoasr_amd import lm_tree, ops
    from oracle import decoder as od
    from tests.test_lm_tree_kernels_gpu import _dense_chain, _lm
    g = Guarded(dev)
    lm = _lm(dtype, dev)
    P = lm.params
    S, W, steps, V = 4, 3, 12, lm.params.vocab_size
    nb = S * W
    tree = guarded_tree(g, S, W, 2 * W, lm_tree.las_list_cap(steps, P.max_seq_len), lm_tree.las_node_cap(W, steps), dev)
    step = lm_tree.TreeStep(lm, tree)
    buf = g((nb, V), torch.float32, 77.0)
    row_id = torch.arange(nb, device=dev, dtype=torch.int32)
    walk = R.BookWalk(11, S, W, V, done=(2,), alive=lambda i, s: (W, W, W, max(1, W - i % 3))[s])
    seqs, got = [], []
    for i in range(steps):
        ids, parent, state = walk.next_step()
        d_ids, d_parent, d_state = _book(g, ids, parent, state, dev)
        src_base, dst_base = R.halves(i, nb)
        buf.fill_(77.0)
        tree.advance_beam(d_ids, d_parent, d_state, src_base, dst_base)
        ops.log_softmax_rows_to(step(), nb, row_id, buf, V, row_ok=tree.row_node)
        node = tree.row_node.cpu().numpy()
        walk.commit(node)
        host = buf.double().cpu()
        for r in range(nb):
            if node[r] >= 0:
                seqs.append(tuple(walk.seq[1 - i % 2][r]))
                got.append(host[r])
            else:
                assert bool((host[r] == 77.0).all()), (i, r)
        assert (node[2 * W:3 * W] == -1).all() and (node >= 0).sum() >= (1 if i else 3)
    assert not tree.status.any() and g.intact() and max(map(len, seqs)) == steps and len(seqs) > 80
    sd64 = {k: v.double() for k, v in load_ctc_beam_golden()[2].items()}
    ys = torch.zeros(len(seqs), steps, dtype=torch.int64)
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
    print(f"[measured] LAS chain LM part {dtype}: {e_tree:.3e} from the f64 oracle over {len(seqs)} rows; emoasr_bert_lm_step (chain, "
          f"dense caches) {e_dense:.3e}; allowed {2 * e_dense:.3e}")
    assert e_tree <= 2.0 * e_dense, (e_tree, e_dense)


def test_nan_in_rows_without_a_node_changes_nothing(dev):
    """the batched search on set A at W = 10, lm_weight 0.05, twice.  Cut to ONE step, rows 1 .. W - 1 of every search never get a
    node: with NaN in their rows of the f32 buffer the score kernel reads, the step's candidates and the search's results are bit for
    bit what they were, and the NaNs are still there.  At full length, with the WHOLE buffer NaN before the search (a row keeps it
    through every step until it first gets a node, rows 1 .. W - 1 at least through step 0), the replayed graphs return exactly
    the first run's lists: emoasr_beam_update_batch never reads a row without a node"""
    from emoasr_amd.modeling.functions import _engine_of
    from tests import las_tlm_fusion_util as U
    from tests.test_las_fusion_gpu import _asr, _padded
    from tests.test_lm_tree_kernels_gpu import _lm
    model, lm = _asr(dev, torch.float32), _lm(torch.float32, dev)
    dec, eng = model.decoder, _engine_of(model.decoder)
    eouts, elens = _padded(U.SEARCHES, dev)
    S, W = len(U.SEARCHES), 10
    for max_len in (1, dec.max_decode_ylen):
        run = lambda: eng._las_beam_chunk(eouts, elens, W, 0.1, dec.eos_id, max_len, lm, 0.05)
        first = run()
        Bf = eng._las_beam_bufs[1]
        graphs = Bf.graphs[1]
        book = [x.clone() for x in (Bf.vals, Bf.cands, Bf.ids, Bf.parent, Bf.score, Bf.pack)]
        assert bool(torch.isfinite(Bf.lm_logits).all())
        if max_len == 1:
            rows = Bf.lm_logits.view(S, W, -1)
            rows[:, 1:] = float("nan")
        else:
            assert all(len(h) >= 1 for h in first[0])
            Bf.lm_logits.fill_(float("nan"))
        again = run()
        assert eng._las_beam_bufs[1] is Bf and Bf.graphs[1] is graphs and again == first
        if max_len == 1:
            rows = Bf.lm_logits.view(S, W, -1)
            assert bool(torch.isnan(rows[:, 1:]).all()) and bool(torch.isfinite(rows[:, 0]).all())
            assert Bf.tree.nnodes.tolist() == [1] * S
            live = lambda x: x.view(S, W, -1)[:, 0]
            assert torch.equal(live(Bf.vals), live(book[0])) and torch.equal(live(Bf.cands), live(book[1]))
            for now, was in zip((Bf.ids, Bf.parent, Bf.score, Bf.pack), book[2:]):
                assert torch.equal(now, was)
        else:
            assert bool(torch.isfinite(Bf.lm_logits.view(S, W, -1)[:, 0]).all())
