"""The host side of the joint CTC / attention fusion grid: the cell plan, the cross-attention's group
table, the len_weight expansion, chunk planning and the command-line tool's dispatch.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest


def test_cell_plan():
    from emoasr_amd.modeling.beam_search_device import grid_cell_plan
    lm_w = [0.0, 0.3, -0.1, 0.5, 0.3]
    len_w = [0.0, 0.1, 0.3]
    weights, cells = grid_cell_plan(lm_w, len_w)
    assert weights == [0.0, 0.3, 0.5]                       # distinct; 0.0 and -0.1 are the one search without the LM
    assert len(cells) == len(lm_w) * len(len_w)
    want_search = [0, 1, 0, 2, 1]
    for i in range(len(lm_w)):                              # lm_weight outer, len_weight inner
        assert cells[3 * i:3 * i + 3] == [(want_search[i], 0), (want_search[i], 1), (want_search[i], 2)]
    # the reference's unrounded candidates stay distinct from their rounded neighbours
    from emoasr_amd.fusion_grid import weight_lists
    grid_w, _ = weight_lists(0, 1, 0.1, 0, 5, 1)
    assert float(grid_w[3]) != 0.3 and len(grid_w) == 11
    weights, cells = grid_cell_plan(list(grid_w) + [0.3], [0.0])
    assert len(weights) == 12 and weights[3] == float(grid_w[3]) and weights[-1] == 0.3
    assert cells[3] == (3, 0) and cells[-1] == (11, 0)
    # without an LM no weight means anything: one search
    assert grid_cell_plan([0.0, 0.3, 0.5], [0.0, 1.0], has_lm=False) == ([0.0], [(0, 0), (0, 1)] * 3)
    assert grid_cell_plan([0.2], []) == ([0.2], [])


@pytest.mark.parametrize("W", [1, 3, 10, 16, 17, 32])
def test_group_table(W):
    from emoasr_amd.ops import cell_groups
    for per_utt in range(1, 8):
        for cpg in (None, 1):
            counts = [per_utt, 1, per_utt, (per_utt % 3) + 1]
            sutt = [u for u, n in enumerate(counts) for _ in range(n)]
            groups, most = cell_groups(sutt, W, cpg)
            assert most == max(n for _, n, _ in groups) and most <= 32
            covered = []
            for row0, n, u in groups:
                assert 1 <= n <= 32 and n % W == 0 and row0 % W == 0
                searches = range(row0 // W, (row0 + n) // W)
                assert {sutt[s] for s in searches} == {u}          # never straddles utterances
                covered += list(range(row0, row0 + n))
            assert covered == list(range(len(sutt) * W))               # every row once, in order
            want_cpg = max(1, 32 // W) if cpg is None else 1
            assert all(n <= want_cpg * W for _, n, _ in groups)
            # packed as far as the utterance allows: a group is short only at the end of its utterance
            for (row0, n, u), nxt in zip(groups, groups[1:]):
                if n < want_cpg * W:
                    assert nxt[2] != u
    with pytest.raises(AssertionError):
        cell_groups([0, 0], W, 32 // W + 1 if W > 1 else 33)


def _expand_direct(hyps, scores, w):
    """the reference's list handling restated: results in the order found, score + w * len (sos / eos included), stable sort"""
    res = [dict(hyp=h, score=s + w * (len(h) + 2)) for h, s in zip(hyps, scores)]
    res = sorted(res, key=lambda r: r["score"], reverse=True)
    return [r["hyp"] for r in res], [r["score"] for r in res]


def test_host_expansion_and_ties():
    from emoasr_amd.modeling.beam_search_device import expand_len_weights
    hyps = [[5, 6], [7], [8, 9, 10], [11], [12, 13]]
    scores = [-2.0, -1.5, -2.5, -1.5, -2.0]            # ties at len_weight 0 (equal lengths) ...
    len_w = [0.0, 0.5, 0.25, 1.0]                      # ... all five at 0.5: -2 + 0.5 * 4 = -1.5 + 0.5 * 3 = -2.5 + 0.5 * 5 = 0
    got = expand_len_weights(hyps, scores, len_w)
    assert len(got) == len(len_w)
    for (h, s), w in zip(got, len_w):
        assert (h, s) == _expand_direct(hyps, scores, w)
    assert got[0][0] == [[7], [11], [5, 6], [12, 13], [8, 9, 10]]          # equal scores keep the order found
    assert got[1] == (hyps, [0.0] * 5)
    assert got[3][0] == [[8, 9, 10], [5, 6], [12, 13], [7], [11]]
    assert expand_len_weights([], [], len_w) == [([], [])] * 4
    # double arithmetic, multiply then add
    rng = np.random.default_rng(0)
    sc = [float(x) for x in -10 * rng.random(40)]
    hy = [[1] * int(n) for n in rng.integers(1, 64, 40)]
    for w in (0.1, 0.3, 5.0):
        _, s = expand_len_weights(hy, sc, [w])[0]
        assert sorted(s, reverse=True) == s
        assert set(s) == {a + w * float(len(h) + 2) for a, h in zip(sc, hy)}


def test_chunk_planning():
    from emoasr_amd.modeling.beam_search_device import batch_chunk_capacity, grid_chunk_plan

    def check(plan, n_utts, nw, cap):
        seen = []
        for chunk in plan:
            assert 1 <= sum(n for _, _, n in chunk) <= cap
            utts = [b for b, _, _ in chunk]
            assert utts == sorted(utts) and utts == list(range(utts[0], utts[-1] + 1)) or len(set(utts)) == len(utts)
            seen += [(b, k) for b, k0, n in chunk for k in range(k0, k0 + n)]
        assert seen == [(b, k) for b in range(n_utts) for k in range(nw)]

    assert grid_chunk_plan(5, 2, 100) == [[(b, 0, 2) for b in range(5)]]
    # whole utterances while they fit: 2 searches each into chunks of 3 -> one utterance per chunk, none split
    assert grid_chunk_plan(5, 2, 3) == [[(b, 0, 2)] for b in range(5)]
    assert grid_chunk_plan(5, 2, 4) == [[(0, 0, 2), (1, 0, 2)], [(2, 0, 2), (3, 0, 2)], [(4, 0, 2)]]
    # an utterance larger than a chunk is cut; what is left of its last chunk takes whole utterances only
    assert grid_chunk_plan(2, 5, 2) == [[(0, 0, 2)], [(0, 2, 2)], [(0, 4, 1)], [(1, 0, 2)], [(1, 2, 2)], [(1, 4, 1)]]
    assert grid_chunk_plan(3, 3, 2) == [[(0, 0, 2)], [(0, 2, 1)], [(1, 0, 2)], [(1, 2, 1)], [(2, 0, 2)], [(2, 2, 1)]]
    assert grid_chunk_plan(3, 1, 1) == [[(0, 0, 1)], [(1, 0, 1)], [(2, 0, 1)]]
    assert grid_chunk_plan(2, 5, 4) == [[(0, 0, 4)], [(0, 4, 1)], [(1, 0, 4)], [(1, 4, 1)]]
    assert grid_chunk_plan(0, 3, 4) == []
    for n_utts, nw, cap in ((7, 3, 5), (4, 11, 3), (16, 11, 102), (3, 4, 4), (5, 1, 2)):
        check(grid_chunk_plan(n_utts, nw, cap), n_utts, nw, cap)
    # the budget in searches is batch_chunk_capacity's: rows and cache bytes
    assert batch_chunk_capacity(10, 37, 6, 256, 12, 768, 2, max_rows=1024, budget=1 << 40) == 102
    per_search = 2 * 2 * 10 * 37 * (6 * 256 + 12 * 768) * 2
    assert batch_chunk_capacity(10, 37, 6, 256, 12, 768, 2, budget=7 * per_search + 1) == 7
    assert grid_chunk_plan(2, 11, 7) == [[(0, 0, 7)], [(0, 7, 4)], [(1, 0, 7)], [(1, 7, 4)]]


def test_refusals_and_dispatch():
    from emoasr_amd import fusion_grid as fg
    assert fg.grid_of("ctc") is fg.ctc_fusion_grid
    assert fg.grid_of("transformer") is fg.joint_fusion_grid
    for kind in ("rnnt", "las", None):
        with pytest.raises(NotImplementedError, match="'ctc' and 'transformer'"):
            fg.grid_of(kind)
    for kind in ("ctc", "rnnt", "las"):
        with pytest.raises(NotImplementedError, match="decoder_type == 'transformer'"):
            fg.joint_fusion_grid(SimpleNamespace(decoder_type=kind), [], None, 4, object(), [0.1], [0.0], "cpu")
    # the CTC grid keeps its refusals, with their messages
    with pytest.raises(NotImplementedError, match="CTC models only"):
        fg.ctc_fusion_grid(SimpleNamespace(decoder_type="transformer"), [], None, 4, object(), [0.1], [0.0], "cpu")
    with pytest.raises(NotImplementedError, match="decode_ctc_weight > 0"):
        fg.ctc_fusion_grid(SimpleNamespace(decoder_type="ctc"), [], None, 4, object(), [0.1], [0.0], "cpu", decode_ctc_weight=0.3)
    # an empty loader: every cell at WER 0 would need references; the cells come back in order either way
    args = fg.build_parser().parse_args(["-conf", "x.yaml", "-ep", "1", "--decode_ctc_weight", "0.3"])
    assert args.decode_ctc_weight == 0.3


def test_grid_refuses_a_masked_lm_and_empty_utterances():
    import torch
    from emoasr_amd.modeling.beam_search_device import joint_beam_search_device_grid
    masked = SimpleNamespace(lm_type="bert")
    dec = SimpleNamespace(vocab_size=40)
    with pytest.raises(Exception):
        joint_beam_search_device_grid(dec, torch.zeros(1, 4, 8), [4], 4, masked, [0.3], [0.0])
    with pytest.raises(ValueError, match="at least one frame"):
        joint_beam_search_device_grid(dec, torch.zeros(2, 4, 8), [4, 0], 4, None, [0.0], [0.0])
