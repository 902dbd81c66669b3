"""Split-K plan of the grouped weight-gradient launch (host only: emoasr_gemm_tn_grouped_plan), 128x128-tile kernel.

The per-problem cap on k slices is the rule of the plain launch (csrc/gemm.hip: tn_split_cap): about 8 MB of f32 atomic traffic,
or more where the reduction is long enough that the atomics stay a small share of the product's time.  What that must and must
not change: the vocabulary head alone in its launch (10 000 x 256 f32 = 10.2 MB of output, one slice under the 8 MB term alone)
is split; one encoder layer's nine products keep the 8 slices each, 768 blocks, that the 8 MB term alone gave them."""
import torch

K = 35145
LAYER = [(256, 1024, K), (1024, 256, K), (256, 256, K), (512, 256, K), (256, 256, K), (256, 256, 4400), (768, 256, K),
         (256, 1024, K), (1024, 256, K)]


def _old_rule(shapes, slots=768, bt=128, bk=32):
    """the plan with the 8 MB term alone"""
    tiles = sum(-(-n1 // bt) * -(-n2 // bt) for n1, n2, _ in shapes)
    want = max(1, slots // tiles)
    out = []
    for n1, n2, k in shapes:
        nk = -(-k // bk)
        sp = max(1, min(want, max(1, (8 << 20) // (n1 * n2 * 4)), max(1, nk // 4)))
        out.append(-(-nk // -(-nk // sp)))
    return out


def test_layer_group_plan_unchanged():
    from emoasr_amd import ops
    splits, tile, blocks = ops.gemm_tn_grouped_plan(LAYER)
    assert tile == 128
    assert splits == _old_rule(LAYER) == [8] * 9
    assert blocks == 768
    short = [(n1, n2, 3001 if k == K else 411) for n1, n2, k in LAYER]   # the shapes of tests/test_ops_gpu.py
    assert ops.gemm_tn_grouped_plan(short)[0] == _old_rule(short)


def test_head_alone_is_split():
    from emoasr_amd import ops
    assert _old_rule([(10000, 256, K)]) == [1]
    splits, tile, blocks = ops.gemm_tn_grouped_plan([(10000, 256, K)])
    assert tile == 128 and splits == [4] and blocks == 4 * 79 * 2   # one round of 768 resident blocks holds four slices of 158 tiles
    assert ops.gemm_tn_grouped_plan([(10000, 256, 777)])[0] == [1]   # a short reduction: the atomics would dominate


def test_f32_groups_follow_the_same_cap():
    from emoasr_amd import ops
    shapes = [(256, 256, 3001), (1024, 256, 3001)]
    assert ops.gemm_tn_grouped_plan(shapes, dtype=torch.float32)[0] == _old_rule(shapes, bk=16)
