"""Weight-gradient (TN) products of one encoder layer at the stacked row count, one grouped launch, under a few launch policies
(256 x 256 eight-wave tile with its block budgets, the 128 x 128 tile's older variants), the vocabulary head alone, the plain
launches, and the Conv2d weight gradient of five micro-batches as five launches / one segmented launch.
Prints the time per launch; run under `rocprofv3 --pmc FETCH_SIZE` to get the bytes each variant pulls through L2 (dispatch order =
the order printed here).  usage: python tools/tn_probe.py [rows]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from emoasr_amd import ops, lib

dev = torch.device("cuda:0")
K = int(sys.argv[1]) if len(sys.argv) > 1 else 35145
REP = int(os.environ.get("REP", 5))
dt = torch.bfloat16
def rnd(*s): return torch.randn(*s, device=dev).to(dt)
# the nine products of csrc/layer.hip's backward, in its order: (N1, N2, rows, bias gradient)
R = int(os.environ.get("POS_ROWS", 4400))
shapes = [(256, 1024, K, 1), (1024, 256, K, 1), (256, 256, K, 1), (512, 256, K, 1), (256, 256, K, 1), (256, 256, R, 0), (768, 256, K, 1),
          (256, 1024, K, 1), (1024, 256, K, 1)]
if os.environ.get("UNIFORM"):
    shapes = [(n1, n2, K, 1) for n1, n2, _, _ in shapes]
probs = []
for n1, n2, k, cs in shapes:
    probs.append((rnd(k, n1), rnd(k, n2), torch.zeros(n1, n2, device=dev), 1.0, torch.zeros(n1, device=dev) if cs and not os.environ.get("NO_COLSUM") else None, 1.0))
alg = sum(k * (n1 + n2) * 2 for n1, n2, k, _ in shapes)
print(f"rows {K}: algorithmic input bytes per grouped launch {alg/1e6:.1f} MB")

def timeit(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REP * 1e3

OLD = {"tn_big": 0}                        # the 128x128 tile of gemm_tn_grouped_kernel: what the older variants below tune
variants = [("default (256 tile)", {}), ("256 tile, 160 blocks", {"tn_big_blocks": 160}), ("256 tile, 192 blocks", {"tn_big_blocks": 192}),
            ("256 tile, 256 blocks", {"tn_big_blocks": 256}), ("256 tile, 320 blocks", {"tn_big_blocks": 320}),
            ("128 tile", OLD), ("slices placed per XCD", {**OLD, "tn_place": 1}), ("hw block order", {**OLD, "gemm_xcd": 0}),
            ("BK=64, 512 blocks", {**OLD, "gemm_kb": 2, "tn_group_blocks": 512}), ("BK=64, 256 blocks", {**OLD, "gemm_kb": 2, "tn_group_blocks": 256}),
            ("BK=32, 512 blocks", {**OLD, "tn_group_blocks": 512}), ("BK=32, 896 blocks", {**OLD, "tn_group_blocks": 896}),
            ("64x64 tiles", {**OLD, "gemm_tile": 3})]
for name, opts in variants:
    with lib.options(**opts):
        us = timeit(lambda: ops.gemm_tn_grouped(probs))
    print(f"group  {name:22s} {us:8.1f} us  {alg/us/1e3:7.1f} GB/s algorithmic   ({REP + 1} launches)")
# the vocabulary head alone in a grouped launch (N1 = 10 000 under lda = 10 048), as the training step issues it
ha, hb = rnd(K, 10048)[:, :10000], rnd(K, 256)
hout, hcs = torch.zeros(10000, 256, device=dev), torch.zeros(10000, device=dev)
for name, opts in [("default (256 tile)", {}), ("256 tile, 192 blocks", {"tn_big_blocks": 192}), ("256 tile, 256 blocks", {"tn_big_blocks": 256}),
                   ("256 tile, 320 blocks", {"tn_big_blocks": 320}), ("128 tile", OLD)]:
    with lib.options(**opts):
        us = timeit(lambda: ops.gemm_tn_grouped([(ha, hb, hout, 1.0, hcs, 1.0)]))
    print(f"head   {name:22s} {us:8.1f} us   ({REP + 1} launches)")
for i in (0, 1, 2, 3):
    us = timeit(lambda: ops.gemm_tn_grouped(probs[i:i + 1]))
    n1, n2 = shapes[i][:2]
    print(f"single {n1}x{n2}        {us:8.1f} us  {K*(n1+n2)*2/us/1e3:7.1f} GB/s algorithmic   ({REP + 1} launches)")

# plain launches, 128 tile (the Conv2d weight gradient is an implicit GEMM, K = B*T2*F2, and has no 256-tile form)
a, b = rnd(K, 10000), rnd(K, 256)
out, cs = torch.zeros(10000, 256, device=dev), torch.zeros(10000, device=dev)
B_, T1, F1, C = 16, 4 * (K // 5 // 16) // 2, 39, 256
y1 = rnd(B_, T1, F1, C); T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
dy2 = rnd(B_, T2, F2, C); dw = torch.zeros(C, 3, 3, C, device=dev); db = torch.zeros(C, device=dev)
print(f"conv2 wgrad: K = {B_ * T2 * F2}")
for name, opts in [("default", {}), ("BK=64, 512", {"gemm_kb": 2, "tn_group_blocks": 512}), ("288 blocks", {"tn_group_blocks": 288}),
                   ("576 blocks", {"tn_group_blocks": 576}), ("864 blocks", {"tn_group_blocks": 864})]:
    with lib.options(tn_big=0, **opts):
        u1 = timeit(lambda: ops.gemm_tn(a, b, out=out, accumulate=True, colsum=cs))
        u2 = timeit(lambda: ops.conv2_wgrad(dy2, y1, dw, db, accumulate=True))
    print(f"plain  {name:16s} head wgrad {u1:8.1f} us   conv2 wgrad {u2:8.1f} us")
# the Conv2d weight gradient of five micro-batches: five launches (gemm_tn_kernel) against ONE segmented launch of the 256 tile
segs = [(rnd(B_ * T2 * F2, C), rnd(B_, T1, F1, C)) for _ in range(5)]
def five():
    for d, y in segs: ops.conv2_wgrad(d, y, dw, db, accumulate=True)
print(f"conv2 wgrad x 5: five launches {timeit(five):8.1f} us")
for blocks in (0, 189, 252, 315):
    with lib.options(tn_big_blocks=blocks):
        print(f"conv2 wgrad x 5: one segmented launch, {blocks or 'default'} blocks {timeit(lambda: ops.conv2_wgrad_seg(segs, dw, dbias=db)):8.1f} us")
