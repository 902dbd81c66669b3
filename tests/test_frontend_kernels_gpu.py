"""The Conv2d front-end kernels -- csrc/subsample.hip, the gathered modes of csrc/gemm.hip, the conv entries of csrc/gemm_big.hip
and BigTnConv of csrc/gemm_big_tn.hip -- against the float64 restatement of tests/frontend_ref.py (pinned on the CPU by
tests/test_frontend_ref_cpu.py), through the C ABI with the test's own buffers: every output is NaN-filled with a 64-element NaN
guard behind it, every scratch is NaN-filled at exactly the size its query returns, accumulators start from non-zero values (random
integers in the integer cases; the expectation is start + reference), options are set by lib.options scopes only.  After each launch
the guards are untouched and the result is (a) EQUAL to the float64 reference (integer cases: every float32 order is exact, a NaN
left in the buffer is unequal) or (b) inside the bound of tests/frontend_ref.py (randn cases; every element, finite).

PATH COVERAGE, from the dispatch conditions (ids of frontend_ref's tables; "int" = equality, "randn" = bounded):
  emoasr_conv1_fwd: bf16 && C == 256 && option conv1_pair -> conv1_fwd2_kernel, else conv1_fwd_kernel<T>
    conv1_fwd_kernel<float>     c1f-int-* as "f32" (C = 8 .. 512: the c += 256 loop at 264 and 512), c1f-randn-* f32
    conv1_fwd_kernel<bf16>      c1f-int-* as "bf16" (C = 256 under conv1_pair = 0), c1f-randn-* bf16
    conv1_fwd2_kernel           c1f-int-*-256 as "pair": T = 3 .. 11 gives T1 = 1 .. 5, odd T1 = a last block without a second row,
                                T = 3, 4 stage nrow = 3, 4 < 5 rows; equal to the reference AND to the one-row kernel; c1f-randn-3-11-80-256
  emoasr_conv1_wgrad: conv1_wgrad_kernel<T> + conv1_wgrad_reduce_kernel, always
    <float>, <bf16>             c1w-int-* (T1 on both sides of the 8 staged rows and the 32-row chunk, F1 on both sides of the lanes'
                                8 and 64 positions, C = 8 .. 512 = the channel guard and a second channel block), accumulate 0 | 1;
                                c1w-randn-*
  emoasr_conv2_fwd: bf16 && C % 256 == 0 && conv_big && a plain epilogue (alpha = 1, bf16 out, bias / ReLU only) -> big_nt_kernel
  with the gathered A (tile height big_bm: 128 | 192 | 256 | 0 = by rule; big_waves 4 | 8); else gemm_nt_kernel<T, BM, BN, 1>,
  tile by gemm_tile (1 = 128x128, 2 = 128x64, 3 = 64x64), BK by gemm_kb; f32x3 -> the SP instantiations by split_tile / split_kb
    big_nt_kernel (conv)        c2f-int-*-{256,512} "big": conv_big = 1 x big_bm x big_waves, bias + ReLU | no bias | no activation;
                                c2f-randn-{3-9-8-256,1-5-7-512}
    gemm_nt_kernel<bf16,..,1>   every c2f-int-* under conv_big = 0 x gemm_tile 1 | 2 | 3 x gemm_kb 1 | 2 (C = 32 .. 512), tr_read 0;
                                out_f32 and alpha = 0.5 under conv_big = 1 (both must leave the large-tile kernel); c2f-randn-* bf16
    gemm_nt_kernel<float,..,1>  c2f-int-* f32 x gemm_tile 0 .. 3; c2f-randn-* f32
    gemm_nt_kernel<..,SP>       c2f-int-* f32x3 x split_tile 0 .. 3 x split_kb 1 | 2; c2f-randn-* f32x3
  emoasr_conv2_dgrad: four launches of gemm_nt_kernel<T, BM, BN, 2, true, TR> (TR = option tr_read; f32x3: SP)
                                c2d-int-* f32 | bf16 x tr_read 0 | 1 x gemm_tile 0 .. 3 (bf16: x gemm_kb 0 | 1 | 2); f32x3 x
                                split_tile 0 .. 3 x split_kb 1 | 2 (the 128x128 and BK = 64 SP instantiations only by option:
                                the rule's own switch at 512 tiles of 128x128 is beyond a quick shape); c2d-randn-*
  emoasr_conv2_col2im: col2im_kernel<T>   c2d-int-* f32 | bf16 (f32x3 is f32 here); c2d-randn-*
  emoasr_conv2_dgrad_kc (bf16, C % 256 == 0): big_nt_kernel with the parity-class tile table (dgrad_plan)
                                c2d-int-*-{256,512} x big_bm x big_waves: class sizes 2 / 1 at T1 = 3, rows of the one-tap and
                                of the heaviest class on both sides of 128 / 192 / 256; c2d-randn-{3-8-7-256,2-7-4-512}
  emoasr_conv2_wgrad: gemm_tn_kernel<T, BN, BN, 1, TR, KB> (or <.., SP> for f32x3), BN = 128 when cdiv(C, 128) cdiv(9C, 128) >= 32
  (C = 256, 512), else 64 (C = 128); TR = option tr_read; KB by gemm_kb (bf16); split-K slices by the rule of launch_tn
                                c2w-int-* f32 | bf16 | f32x3, accumulate 0 | 1 x dbias NULL | given, tr_read 0 | 1, gemm_kb 0 | 2;
                                several slices: c2w-int-3x20x-75-256 (999 rows), c2w-int-7x25x5x31-41-256; c2w-randn-*
  emoasr_conv2_wgrad_seg: bf16 && C % 256 == 0 && tn_big && tr_read -> big_tn_kernel<1, BigTnConv> in ONE launch, slices by
  tn_big_blocks; else one emoasr_conv2_wgrad per segment
    big_tn_kernel<1, BigTnConv> c2w-int-*-{256,512} bf16 under tn_big = 1 x tn_big_blocks (one slice | the default budget: up to 3
                                slices at C = 256 from 256 rows on, one at C = 512: tn_split_cap), nseg 1 | 2 | 8
                                (segments of different B and T1 whose rows are no multiples of 32), F2 = 1 .. 37; c2w-randn-*-256
    per segment                 the same under tn_big = 0, and every f32 / f32x3 / C = 128 case
  emoasr_conv2_dgrad_w1 (bf16, C % 256 == 0): big_nt_kernel<.., 6> (the fold epilogue) + w1_fold_kernel (64 slices) + the reduce
                                w1-int-* x big_bm 0 | 128 | 192 | 256 x accumulate 0 | 1, also EQUAL to _kc followed by
                                emoasr_conv1_wgrad; tile rows 4 (every small shape), 63, 64, 65, 130 at big_bm = 128 (W1_TILES);
                                w1-randn-*
  NOT covered: the 4 GiB refusals (no small call reaches them); tile rows 1 of the fold (four classes exist whenever
  T1, F1 >= 3).

MEASURED on an MI355X, worst share of the bound per family (the `[measured] frontend <family>` lines this module prints when it
is done; f32 | bf16 | f32x3).  Wall time of the module's 431 tests: 12 s.
  conv1_fwd       y1 0.120 | 0.995 (one-row and pair kernel alike)
  conv1_wgrad     dw1 0.001, db1 0.001 | dw1 0.001, db1 0.000 (accumulate 0 and 1 alike)
  conv2_fwd       bias + ReLU 0.002, no bias 0.003, no activation 0.004, out_f32 0.002, alpha 0.002
                  | large tile: 0.703, 0.707, 0.785; 128x64 / 64x64: 0.847, 0.856, 0.893, out_f32 0.001, alpha 0.885
                  | f32x3 0.013, 0.014, 0.013, 0.013, 0.012
  conv2_dgrad     dgrad 0.026, col2im 0.076 | dgrad 0.967, col2im 0.996, _kc 0.956 at every tile height | f32x3 dgrad 0.076
                  (tr_read 0 and 1 alike)
  conv2_wgrad     segmented dw 0.037, db 0.013, plain dw 0.011, db 0.003 | segmented dw 0.022, db 0.006, 256 tile dw 0.028, db 0.006,
                  plain dw 0.009, db 0.001 | f32x3 segmented dw 0.158, db 0.028, plain dw 0.054, db 0.016
  conv2_dgrad_w1  dw1 0.223, db1 0.155 at every tile height, accumulate 0 and 1
Every share near 1 is a bf16 ELEMENT output: the term of its bound that is reached is 2^-8 |ref|, bf16's worst rounding, which is
the bound by construction; the f32 column beside it shows the arithmetic before that rounding.  The f32x3 shares are a sixth of
their bound at most: the 3.03 2^-16 sum |term| term is a worst case over signs that random operands do not meet.

What the sweep exposed: no wrong result on the device -- every kernel on every path above is EQUAL to the reference on every
integer case (written zeros at even T1 / F1 included), holds every bound, every NaN guard and every refusal -- and ONE host error:
the conv2 entries had no B == 0 branch.  emoasr_conv2_fwd, _dgrad and _dgrad_kc asked for an empty grid (a launch error, status 2)
and emoasr_conv2_wgrad divided by its zero k-tiles in launch_tn (an integer division by zero on the host: the process dies).  They
now return early after their argument checks, as emoasr_conv1_fwd does (conv2_wgrad after zeroing dw / dbias when it does not
accumulate); test_empty_batch holds that and include/emoasr_hip.h says it.  Tile rows 1 of the fold, which the issue lists, cannot
be reached: four parity classes exist whenever T1, F1 >= 3.

That the module can fail was tried on scratch builds with three errors planted, each a wrong answer inside every buffer; none of
them is in the tree.  "Present" = the front-end tests the suite had (tests/test_tn_big_gpu.py, tests/test_conv1_fold_gpu.py,
tests/test_split_gpu.py and the conv1 / conv2 / frontend tests of tests/test_ops_gpu.py: 57 tests).
  (1) BigTnConv: cv_f2 advanced without the carry into cv_t2.  Present: 4 fail (the three test_conv2_wgrad shapes and
      test_conv2_wgrad_five_segments of test_tn_big_gpu.py), 53 pass.  Here 16 fail: test_conv2_wgrad_integer (15: every
      C % 256 == 0 id with more than one (t2) row in a 32-row tile -- F2 = 1 from 23 rows per utterance on, F2 = 19 .. 37, all three
      segment tables) and test_conv2_wgrad_bounded[c2w-randn-3x9x2x11-7-256-bf16]; the ids of 32 rows or fewer in one (b, t2) walk,
      C = 128 and f32 pass, as they must.
  (2) dgrad_plan: tile0 of the third class one tile late.  Present: 32 fail (test_conv2_large_tile_kernels 16,
      test_conv1_wgrad_folded_into_conv2_dgrad 15, test_conv1_fold_matches_torch_autograd), 25 pass.  Here 135 fail:
      test_conv2_dgrad_integer (61: every C % 256 == 0 id), test_conv2_dgrad_w1_integer (66: all), test_conv2_dgrad_w1_fold_slices
      (4), test_conv2_dgrad_bounded (2) and test_conv2_dgrad_w1_bounded (2).
  (3) the last of the 64 fold slices left out of the reduce.  Present: all 57 pass (no shape has 64 k tile rows, and at
      B 5, T 97, F 80 the 64th slice is empty).  Here exactly one fails: test_conv2_dgrad_w1_fold_slices[64].  A first version of
      that case (B 8, T 45, F 89: even T1) passed too -- the last tile row of the plan is the one-tap class's last rows, which at an
      even T1 are the rows without a tap: zeros; the case now has odd T1 and F1 (tests/test_frontend_ref_cpu.py asserts the rows
      are non-zero).  63, 65 and 130 tile rows leave the 64th slice empty and pass, as they must."""
import ctypes

import pytest
import torch

from tests import frontend_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
BIG_BM = (0, 128, 192, 256)


def _nan_out(dev, shape, dtype):
    """a NaN-filled tensor of this shape with 64 NaN guard elements behind it -> (tensor, guard)"""
    n = 1
    for v in shape:
        n *= v
    flat = torch.full((n + 64,), NAN, device=dev, dtype=dtype)
    return flat[:n].view(*shape), flat[n:]


def _start_out(dev, start):
    t, g = _nan_out(dev, tuple(start.shape), F32)
    t.copy_(start)
    return t, g


def _untouched(*guards):
    return all(bool(torch.isnan(g).all()) for g in guards)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _code(dname):
    from emoasr_amd import lib
    return {"f32": lib.F32, "bf16": lib.BF16, "f32x3": lib.F32X3}[dname]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(dev, t, dtype=F32):
    return None if t is None else t.to(dtype).to(dev).contiguous()


def _eq(got, ref64):
    """every element equal to the float64 reference (a NaN is unequal)"""
    return torch.equal(got.double().reshape(ref64.shape), ref64.to(got.device))


_WORST = {}


def _report(family, dname, case, res):
    w = _WORST.setdefault(family, {}).setdefault(dname, {})
    for k, v in res.items():
        w[k] = max(v, w.get(k, 0.0))
    assert max(res.values()) <= 1.0, (family, dname, case, res)


@pytest.fixture(scope="module", autouse=True)
def _measured():
    yield
    for family, by in _WORST.items():
        print(f"\n[measured] frontend {family}: " + " | ".join(d + " " + ", ".join(f"{k} {v:.3f}" for k, v in w.items())
                                                                for d, w in by.items()), end="")
    print()


_INPUTS = {}


def _inputs(make, case, dname):
    if (case, dname) not in _INPUTS:
        _INPUTS[(case, dname)] = make(case, dname)
    return _INPUTS[(case, dname)]


# ---- launches -------------------------------------------------------------------------------------------------------------------------
def _conv1_fwd(dev, inp, x, w1, b1):
    from emoasr_amd import lib
    y, g = _nan_out(dev, (inp.B, inp.T1, inp.F1, inp.C), inp.dtype)
    lib.call("emoasr_conv1_fwd", _code(inp.dname), inp.B, inp.T, inp.F, inp.C, _p(x), _p(w1), _p(b1), _p(y), _stream())
    return y, g


def _conv1_wgrad(dev, dname, B, T, F, C, x, dy1, dw, db, accumulate):
    """-> the guard of the NaN-filled scratch"""
    from emoasr_amd import lib
    scratch, g = _nan_out(dev, (lib.size_query("emoasr_conv1_wgrad_scratch_floats", B, T, C),), F32)
    lib.call("emoasr_conv1_wgrad", _code(dname), B, T, F, C, _p(x), _p(dy1), _p(dw), _p(db), int(accumulate), _p(scratch), _stream())
    return g


def _conv2_fwd(dev, inp, y1, w, bias, act=R.ACT_RELU, alpha=1.0, out_f32=False):
    from emoasr_amd import lib
    y, g = _nan_out(dev, (inp.M, inp.C), F32 if out_f32 else inp.dtype)
    ep = lib.Epilogue(bias=bias.data_ptr() if bias is not None else None, alpha=alpha, res_scale=1.0, act=act, out_f32=int(out_f32))
    lib.call("emoasr_conv2_fwd", _code(inp.dname), inp.B, inp.T1, inp.F1, inp.C, _p(y1), _p(w), _p(y), ctypes.byref(ep), _stream())
    return y, g


def _dgrad(dev, entry, inp, src, w, y1):
    """entry: emoasr_conv2_dgrad | _dgrad_kc (src = dy2, w) | _col2im (src = dcol, w = None)"""
    from emoasr_amd import lib
    dy1, g = _nan_out(dev, (inp.B, inp.T1, inp.F1, inp.C), inp.dtype)
    args = (_p(src),) + ((_p(w),) if w is not None else ()) + (_p(y1), _p(dy1), _stream())
    lib.call(entry, _code(inp.dname), inp.B, inp.T1, inp.F1, inp.C, *args)
    return dy1, g


def _seg_array(inp, dev_data, nseg):
    from emoasr_amd import lib
    arr = (lib.Conv2WgradSeg * max(nseg, 1))()
    for i in range(min(nseg, len(dev_data))):
        arr[i].dy2, arr[i].y1, arr[i].B, arr[i].T1 = dev_data[i][0].data_ptr(), dev_data[i][1].data_ptr(), inp.segs[i][0], inp.segs[i][1]
    return arr


def _fold(dev, inp, dy2, wt, y1, x, dw, db, accumulate):
    from emoasr_amd import lib
    n = lib.size_query("emoasr_conv2_dgrad_w1_scratch_floats", inp.B, inp.T, inp.F, inp.C)
    scratch, g = _nan_out(dev, (n,), F32)
    lib.call("emoasr_conv2_dgrad_w1", lib.BF16, inp.B, inp.T, inp.F, inp.C, _p(dy2), _p(wt), _p(y1), _p(x), _p(dw), _p(db),
             int(accumulate), _p(scratch), _stream())
    return g, n // (10 * inp.C) - 64


# ---- conv1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.C1F_INT, ids=R.case_id)
def test_conv1_fwd_integer(dev, case):
    from emoasr_amd import lib
    outs = {}
    for path, dname, pair in (("f32", "f32", 1), ("bf16", "bf16", 0), ("pair", "bf16", 1)):
        inp = _inputs(R.conv1_inputs, case, dname)
        ref = R.assert_exact(inp, "c1f")[0]
        with lib.options(conv1_pair=pair):
            y, g = _conv1_fwd(dev, inp, _up(dev, inp.x), _up(dev, inp.w1), _up(dev, inp.b1))
        torch.cuda.synchronize()
        assert _untouched(g) and _eq(y, ref), (case, path)
        outs[path] = y
    assert torch.equal(outs["bf16"], outs["pair"])


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.C1F_RANDN, ids=R.case_id)
def test_conv1_fwd_bounded(dev, case, dname):
    from emoasr_amd import lib
    inp = _inputs(R.conv1_inputs, case, dname)
    res, ys = {}, []
    for pair in (0, 1):
        with lib.options(conv1_pair=pair):
            y, g = _conv1_fwd(dev, inp, _up(dev, inp.x), _up(dev, inp.w1), _up(dev, inp.b1))
        torch.cuda.synchronize()
        assert _untouched(g)
        res[f"y1(pair={pair})"] = R.check(inp, "c1f", 0, y.float().cpu())
        ys.append(y)
    assert torch.equal(ys[0], ys[1])      # bf16, C = 256: conv1_fwd2_kernel bit for bit the one-row kernel; else the same kernel twice
    _report("conv1_fwd", dname, case, res)


@pytest.mark.parametrize("case", R.C1W_INT, ids=R.case_id)
def test_conv1_wgrad_integer(dev, case):
    for dname in ("f32", "bf16"):
        inp = _inputs(R.conv1_inputs, case, dname)
        dw_r, db_r = R.assert_exact(inp, "c1w")[:2]
        x, dy1 = _up(dev, inp.x), _up(dev, inp.dy1, inp.dtype)
        for acc in (0, 1):
            (dw, g0), (db, g1) = (_start_out(dev, inp.dw0), _start_out(dev, inp.db0)) if acc else (_nan_out(dev, (inp.C, 9), F32), _nan_out(dev, (inp.C,), F32))
            g2 = _conv1_wgrad(dev, dname, inp.B, inp.T, inp.F, inp.C, x, dy1, dw, db, acc)
            torch.cuda.synchronize()
            assert _untouched(g0, g1, g2), (case, dname, acc)
            assert _eq(dw, dw_r + (inp.dw0.double() if acc else 0)) and _eq(db, db_r + (inp.db0.double() if acc else 0)), (case, dname, acc)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.C1W_RANDN, ids=R.case_id)
def test_conv1_wgrad_bounded(dev, case, dname):
    inp = _inputs(R.conv1_inputs, case, dname)
    x, dy1 = _up(dev, inp.x), _up(dev, inp.dy1, inp.dtype)
    for acc in (0, 1):
        (dw, g0), (db, g1) = (_start_out(dev, inp.dw0), _start_out(dev, inp.db0)) if acc else (_nan_out(dev, (inp.C, 9), F32), _nan_out(dev, (inp.C,), F32))
        g2 = _conv1_wgrad(dev, dname, inp.B, inp.T, inp.F, inp.C, x, dy1, dw, db, acc)
        torch.cuda.synchronize()
        assert _untouched(g0, g1, g2)
        _report(f"conv1_wgrad acc={acc}", dname, case, {"dw1": R.check(inp, "c1w", 0, dw.cpu(), start=inp.dw0 if acc else None),
                                                         "db1": R.check(inp, "c1w", 1, db.cpu(), start=inp.db0 if acc else None)})


# ---- conv2 forward --------------------------------------------------------------------------------------------------------------------
# (name, reference kwargs, launch kwargs)
EPILOGUES = (("bias+relu", {}, {}), ("nobias", {"bias": False}, {"bias": False}), ("noact", {"act": R.ACT_NONE}, {"act": R.ACT_NONE}))
EPILOGUES_64 = (("out_f32", {}, {"out_f32": True}), ("alpha", {"alpha": 0.5}, {"alpha": 0.5}))      # these leave the large-tile kernel
ALL_EPILOGUES = EPILOGUES + EPILOGUES_64
RELU_ONLY = EPILOGUES[:1]


def _c2f_runs(dname, C):
    """[(options, epilogues)] of an integer case, written out: every tile / BK option with bias + ReLU, every epilogue on the
    rule's own choice, on the 128x64 tile and on every large-tile variant"""
    if dname == "f32":
        return [(dict(gemm_tile=0), ALL_EPILOGUES), (dict(gemm_tile=1), RELU_ONLY), (dict(gemm_tile=2), ALL_EPILOGUES),
                (dict(gemm_tile=3), RELU_ONLY)]
    if dname == "f32x3":
        return ([(dict(split_tile=0, split_kb=1), ALL_EPILOGUES), (dict(split_tile=2, split_kb=2), ALL_EPILOGUES)]
                + [(dict(split_tile=t, split_kb=kb), RELU_ONLY) for t, kb in ((0, 2), (1, 1), (1, 2), (2, 1), (3, 1), (3, 2))])
    runs = [(dict(conv_big=0), ALL_EPILOGUES), (dict(conv_big=0, tr_read=0), RELU_ONLY),
            (dict(conv_big=0, gemm_tile=2, gemm_kb=2), ALL_EPILOGUES)]
    runs += [(dict(conv_big=0, gemm_tile=t, gemm_kb=kb), RELU_ONLY) for t, kb in ((1, 1), (1, 2), (2, 1), (3, 1), (3, 2))]
    if C % 256 == 0:
        runs += [(dict(conv_big=1, big_bm=bm, big_waves=wv), EPILOGUES) for bm in BIG_BM for wv in (4, 8)]
        runs += [(dict(conv_big=1), EPILOGUES_64), (dict(conv_big=1, tr_read=0), RELU_ONLY)]      # EPILOGUES_64 leave the large tile
    return runs


def _c2f_launch(dev, inp, ops, lkw):
    bias = None if lkw.get("bias") is False else ops["bias"]
    return _conv2_fwd(dev, inp, ops["y1"], ops["w"], bias, **{k: v for k, v in lkw.items() if k != "bias"})


@pytest.mark.parametrize("case", R.C2F_INT, ids=R.case_id)
def test_conv2_fwd_integer(dev, case):
    from emoasr_amd import lib
    for dname in ("f32", "bf16", "f32x3"):
        inp = _inputs(R.conv2_inputs, case, dname)
        ops = dict(y1=_up(dev, inp.y1, inp.dtype), w=_up(dev, inp.w, inp.dtype), bias=_up(dev, inp.bias))
        for opts, epilogues in _c2f_runs(dname, inp.C):
            for name, rkw, lkw in epilogues:
                ref = R.assert_exact(inp, "c2f", **rkw)[0]
                with lib.options(**opts):
                    y, g = _c2f_launch(dev, inp, ops, lkw)
                torch.cuda.synchronize()
                assert _untouched(g) and _eq(y, ref), (case, dname, opts, name)


@pytest.mark.parametrize("dname", ["f32", "bf16", "f32x3"])
@pytest.mark.parametrize("case", R.C2F_RANDN, ids=R.case_id)
def test_conv2_fwd_bounded(dev, case, dname):
    from emoasr_amd import lib
    inp = _inputs(R.conv2_inputs, case, dname)
    ops = dict(y1=_up(dev, inp.y1, inp.dtype), w=_up(dev, inp.w, inp.dtype), bias=_up(dev, inp.bias))
    res = {}
    for opts in ((dict(conv_big=1), dict(conv_big=0)) if dname == "bf16" else ({},)):
        for name, rkw, lkw in ALL_EPILOGUES:
            with lib.options(**opts):
                y, g = _c2f_launch(dev, inp, ops, lkw)
            torch.cuda.synchronize()
            assert _untouched(g)
            res[f"{name}{'/big' if opts.get('conv_big') and inp.C % 256 == 0 and lkw == rkw and 'alpha' not in lkw else ''}"] = \
                R.check(inp, "c2f", 0, y.float().cpu(), out_f32=lkw.get("out_f32", False), **rkw)
    _report("conv2_fwd", dname, case, res)


# ---- conv2 data gradient --------------------------------------------------------------------------------------------------------------
def _dgrad_option_sets(dname):
    """emoasr_conv2_dgrad: the tile (0 = the rule, which picks 64x64 at these sizes; 1 = 128x128, 2 = 128x64, 3 = 64x64) x BK x the
    tr_read form of the k-major operand; f32x3 has one operand form (the SP kernels ignore tr_read)"""
    if dname == "f32x3":
        return [dict(split_tile=t, split_kb=kb) for t in (0, 1, 2, 3) for kb in (1, 2)]
    kbs = (0, 1, 2) if dname == "bf16" else (0,)      # gemm_kb: 0 = BK 64 from K = 512 on (the one-tap class of C = 256 takes 32)
    return [dict(tr_read=tr, gemm_tile=t, gemm_kb=kb) for tr in (0, 1) for t in (0, 1, 2, 3) for kb in kbs]


@pytest.mark.parametrize("case", R.C2D_INT, ids=R.case_id)
def test_conv2_dgrad_integer(dev, case):
    """dgrad, dgrad_kc and col2im: equal to the reference, rows / columns without a tap (even T1 / F1) come back as written zeros"""
    from emoasr_amd import lib
    for dname in ("f32", "bf16", "f32x3"):
        inp = _inputs(R.conv2_inputs, case, dname)
        ref = R.assert_exact(inp, "c2d")[0]
        assert torch.equal(ref, R.assert_exact(inp, "c2d", layout="wt")[0])
        y1, dy2, w = _up(dev, inp.y1, inp.dtype), _up(dev, inp.dy2, inp.dtype), _up(dev, inp.w, inp.dtype)
        for opts in _dgrad_option_sets(dname):
            with lib.options(**opts):
                dy1, g = _dgrad(dev, "emoasr_conv2_dgrad", inp, dy2, w, y1)
            torch.cuda.synchronize()
            assert _untouched(g) and _eq(dy1, ref), (case, dname, "dgrad", opts)
        if dname != "f32x3":
            dy1, g = _dgrad(dev, "emoasr_conv2_col2im", inp, _up(dev, inp.dcol, inp.dtype), None, y1)
            torch.cuda.synchronize()
            assert _untouched(g) and _eq(dy1, R.assert_exact(inp, "col2im")[0]), (case, dname, "col2im")
        if dname == "bf16" and inp.C % 256 == 0:
            wt = _up(dev, inp.wt, BF)
            for bm in BIG_BM:
                for wv in (4, 8):
                    with lib.options(big_bm=bm, big_waves=wv):
                        dy1, g = _dgrad(dev, "emoasr_conv2_dgrad_kc", inp, dy2, wt, y1)
                    torch.cuda.synchronize()
                    assert _untouched(g) and _eq(dy1, ref), (case, "kc", bm, wv)


@pytest.mark.parametrize("dname", ["f32", "bf16", "f32x3"])
@pytest.mark.parametrize("case", R.C2D_RANDN, ids=R.case_id)
def test_conv2_dgrad_bounded(dev, case, dname):
    from emoasr_amd import lib
    inp = _inputs(R.conv2_inputs, case, dname)
    y1, dy2, w = _up(dev, inp.y1, inp.dtype), _up(dev, inp.dy2, inp.dtype), _up(dev, inp.w, inp.dtype)
    res, guards = {}, []
    for tr in (0, 1):
        with lib.options(tr_read=tr):
            dy1, g = _dgrad(dev, "emoasr_conv2_dgrad", inp, dy2, w, y1)
        guards.append(g)
        res[f"dgrad(tr={tr})"] = R.check(inp, "c2d", 0, dy1.float().cpu())
    if dname != "f32x3":
        dy1, g = _dgrad(dev, "emoasr_conv2_col2im", inp, _up(dev, inp.dcol, inp.dtype), None, y1)
        guards.append(g)
        res["col2im"] = R.check(inp, "col2im", 0, dy1.float().cpu())
    if dname == "bf16" and inp.C % 256 == 0:
        for bm in BIG_BM:
            with lib.options(big_bm=bm):
                dy1, g = _dgrad(dev, "emoasr_conv2_dgrad_kc", inp, dy2, _up(dev, inp.wt, BF), y1)
            guards.append(g)
            res[f"kc(bm={bm})"] = R.check(inp, "c2d", 0, dy1.float().cpu(), layout="wt")
    assert _untouched(*guards)
    _report("conv2_dgrad", dname, case, res)


# ---- conv2 weight gradient ------------------------------------------------------------------------------------------------------------
def _tn_option_sets(dname, C):
    """tn_big_blocks = the 9 (C / 256)^2 output tiles -> one slice; 0 = the default budget of 256 blocks -> as many slices as
    tn_split_cap(C, 9C, K) and the k tiles allow: up to 3 at C = 256 (8 MB of atomics over a 2.4 MB output) from eight 32-row
    tiles on, always 1 at C = 512 (9.4 MB) -- several slices of big_tn_kernel are reached at C = 256 only"""
    sets = [dict(tn_big=0), dict(tn_big=0, tr_read=0)] + ([dict(tn_big=0, gemm_kb=2)] if dname == "bf16" else [])
    if dname == "bf16" and C % 256 == 0:
        sets += [dict(tn_big=1, tn_big_blocks=9 * (C // 256) ** 2), dict(tn_big=1, tn_big_blocks=0)]
    return sets


def _wgrad_outs(dev, inp, acc, with_db):
    dw, g0 = _start_out(dev, inp.dw0) if acc else _nan_out(dev, (inp.C, 9 * inp.C), F32)
    db, g1 = (_start_out(dev, inp.db0) if acc else _nan_out(dev, (inp.C,), F32)) if with_db else (None, torch.full((1,), NAN, device=dev))
    return dw, db, g0, g1


def _wgrad_calls(dev, inp, data, nseg):
    """every (name, options, accumulate, with_db, launch) of this input set over its first nseg segments"""
    from emoasr_amd import lib
    calls = []
    for opts in _tn_option_sets(inp.dname, inp.C):
        for with_db in (True, False):
            arr = _seg_array(inp, data, nseg)
            calls.append(("seg", opts, 1, with_db, lambda dw, db, arr=arr: lib.call(
                "emoasr_conv2_wgrad_seg", _code(inp.dname), nseg, arr, inp.F1, inp.C, _p(dw), _p(db), _stream())))
        if nseg == 1 and "tn_big_blocks" not in opts:
            for acc, with_db in ((0, True), (0, False), (1, True), (1, False)):
                calls.append(("plain", opts, acc, with_db, lambda dw, db, acc=acc: lib.call(
                    "emoasr_conv2_wgrad", _code(inp.dname), inp.segs[0][0], inp.segs[0][1], inp.F1, inp.C, _p(data[0][0]), _p(data[0][1]),
                    _p(dw), _p(db), acc, _stream())))
    return calls


def _nsegs(inp):
    return sorted({1, min(2, len(inp.segs)), len(inp.segs)})


@pytest.mark.parametrize("case", R.C2W_INT + R.C2W_SEG_INT, ids=R.case_id)
def test_conv2_wgrad_integer(dev, case):
    from emoasr_amd import lib
    for dname in ("f32", "bf16", "f32x3"):
        inp = _inputs(R.wgrad_inputs, case, dname)
        data = [(_up(dev, d, inp.dtype), _up(dev, y, inp.dtype)) for d, y in inp.data]
        for nseg in _nsegs(inp):
            dw_r, db_r = R.assert_exact(inp, "c2w", nseg=nseg)[:2]
            for name, opts, acc, with_db, launch in _wgrad_calls(dev, inp, data, nseg):
                dw, db, g0, g1 = _wgrad_outs(dev, inp, acc, with_db)
                with lib.options(**opts):
                    launch(dw, db)
                torch.cuda.synchronize()
                assert _untouched(g0, g1), (case, dname, nseg, name, opts)
                assert _eq(dw, dw_r + (inp.dw0.double() if acc else 0)), (case, dname, nseg, name, opts, acc, "dw")
                assert db is None or _eq(db, db_r + (inp.db0.double() if acc else 0)), (case, dname, nseg, name, opts, acc, "dbias")


@pytest.mark.parametrize("dname", ["f32", "bf16", "f32x3"])
@pytest.mark.parametrize("case", R.C2W_RANDN, ids=R.case_id)
def test_conv2_wgrad_bounded(dev, case, dname):
    from emoasr_amd import lib
    inp = _inputs(R.wgrad_inputs, case, dname)
    data = [(_up(dev, d, inp.dtype), _up(dev, y, inp.dtype)) for d, y in inp.data]
    nseg = len(inp.segs)
    res = {}
    for name, opts, acc, with_db, launch in _wgrad_calls(dev, inp, data, nseg):
        dw, db, g0, g1 = _wgrad_outs(dev, inp, acc, with_db)
        with lib.options(**opts):
            launch(dw, db)
        torch.cuda.synchronize()
        assert _untouched(g0, g1)
        tag = f"{name}{'/big' if opts.get('tn_big') and dname == 'bf16' and inp.C % 256 == 0 else ''}"
        res[f"dw {tag}"] = max(res.get(f"dw {tag}", 0.0), R.check(inp, "c2w", 0, dw.cpu(), start=inp.dw0 if acc else None))
        if db is not None:
            res[f"db {tag}"] = max(res.get(f"db {tag}", 0.0), R.check(inp, "c2w", 1, db.cpu(), start=inp.db0 if acc else None))
    _report("conv2_wgrad", dname, case, res)


# ---- the fold -------------------------------------------------------------------------------------------------------------------------
def _fold_ops(dev, inp):
    return _up(dev, inp.dy2, BF), _up(dev, inp.wt, BF), _up(dev, inp.y1, BF), _up(dev, inp.x)


def _fold_integer(dev, inp, bms, tiles=None):
    from emoasr_amd import lib
    res = R.assert_exact(inp, "w1")
    dy2, wt, y1, x = _fold_ops(dev, inp)
    for bm in bms:
        with lib.options(big_bm=bm):
            # the two kernels the fold replaces, on the same operands
            dy1, g = _dgrad(dev, "emoasr_conv2_dgrad_kc", inp, dy2, wt, y1)
            (dw2, g0), (db2, g1) = _nan_out(dev, (inp.C, 9), F32), _nan_out(dev, (inp.C,), F32)
            g2 = _conv1_wgrad(dev, "bf16", inp.B, inp.T, inp.F, inp.C, x, dy1, dw2, db2, 0)
            assert _untouched(g, g0, g1, g2) and _eq(dy1, res[4])
            for acc in (0, 1):
                (dw, g0), (db, g1) = (_start_out(dev, inp.dw0), _start_out(dev, inp.db0)) if acc else (_nan_out(dev, (inp.C, 9), F32), _nan_out(dev, (inp.C,), F32))
                g2, tiles_m = _fold(dev, inp, dy2, wt, y1, x, dw, db, acc)
                torch.cuda.synchronize()
                assert _untouched(g0, g1, g2), (inp.case, bm, acc)
                if bm:
                    assert tiles_m == R.class_tiles(inp.B, inp.T1, inp.F1, bm) and (tiles is None or tiles_m == tiles), (inp.case, bm, tiles_m)
                assert _eq(dw, res[0] + (inp.dw0.double() if acc else 0)) and _eq(db, res[1] + (inp.db0.double() if acc else 0)), (inp.case, bm, acc)
                if not acc:
                    assert torch.equal(dw, dw2) and torch.equal(db, db2), (inp.case, bm)


@pytest.mark.parametrize("case", R.W1_INT, ids=R.case_id)
def test_conv2_dgrad_w1_integer(dev, case):
    _fold_integer(dev, _inputs(R.fold_inputs, case, "bf16"), BIG_BM)


@pytest.mark.parametrize("tiles", sorted(R.W1_TILES))
def test_conv2_dgrad_w1_fold_slices(dev, tiles):
    """tile rows on both sides of the 64 slices of the first fold stage: empty, one-row and multi-row slices"""
    _fold_integer(dev, _inputs(R.fold_inputs, R.W1_TILES[tiles], "bf16"), (128,), tiles)


@pytest.mark.parametrize("case", R.W1_RANDN, ids=R.case_id)
def test_conv2_dgrad_w1_bounded(dev, case):
    from emoasr_amd import lib
    inp = _inputs(R.fold_inputs, case, "bf16")
    dy2, wt, y1, x = _fold_ops(dev, inp)
    res = {}
    for bm in BIG_BM:
        for acc in (0, 1):
            (dw, g0), (db, g1) = (_start_out(dev, inp.dw0), _start_out(dev, inp.db0)) if acc else (_nan_out(dev, (inp.C, 9), F32), _nan_out(dev, (inp.C,), F32))
            with lib.options(big_bm=bm):
                g2, _ = _fold(dev, inp, dy2, wt, y1, x, dw, db, acc)
            torch.cuda.synchronize()
            assert _untouched(g0, g1, g2)
            res[f"dw1(bm={bm},acc={acc})"] = R.check(inp, "w1", 0, dw.cpu(), start=inp.dw0 if acc else None)
            res[f"db1(bm={bm},acc={acc})"] = R.check(inp, "w1", 1, db.cpu(), start=inp.db0 if acc else None)
    _report("conv2_dgrad_w1", "bf16", case, res)


# ---- refusals and empties -------------------------------------------------------------------------------------------------------------
def _refused(name, *args):
    from emoasr_amd import lib
    with pytest.raises(lib.EmoasrHipError):
        lib.call(name, *args)


def test_refusals_leave_every_buffer_alone(dev):
    """every EMO_CHECK of these entries that a small call reaches returns non-zero before anything is launched"""
    from emoasr_amd import lib
    f, b = lib.F32, lib.BF16
    big = torch.zeros(1 << 16, device=dev)            # readable operands of any dtype
    out, g = _nan_out(dev, (1 << 16,), F32)
    out2, g2 = _nan_out(dev, (1 << 12,), F32)
    scr, g3 = _nan_out(dev, (1 << 16,), F32)
    s, P = _stream(), _p
    ep = lib.Epilogue(alpha=1.0, res_scale=1.0, act=1)
    for T, F in ((2, 7), (7, 2)):
        _refused("emoasr_conv1_fwd", f, 1, T, F, 8, P(big), P(big), P(big), P(out), s)
        _refused("emoasr_conv1_wgrad", f, 1, T, F, 8, P(big), P(big), P(out), P(out2), 0, P(scr), s)
        _refused("emoasr_conv2_dgrad_w1", b, 1, T, F, 256, P(big), P(big), P(big), P(big), P(out), P(out2), 0, P(scr), s)
    for T, F in ((6, 7), (7, 6)):                      # T1 or F1 = 2
        _refused("emoasr_conv2_dgrad_w1", b, 1, T, F, 256, P(big), P(big), P(big), P(big), P(out), P(out2), 0, P(scr), s)
    for T1, F1 in ((2, 3), (3, 2)):
        _refused("emoasr_conv2_fwd", f, 1, T1, F1, 32, P(big), P(big), P(out), ctypes.byref(ep), s)
        _refused("emoasr_conv2_dgrad", f, 1, T1, F1, 64, P(big), P(big), P(big), P(out), s)
        _refused("emoasr_conv2_dgrad_kc", b, 1, T1, F1, 256, P(big), P(big), P(big), P(out), s)
        _refused("emoasr_conv2_col2im", f, 1, T1, F1, 8, P(big), P(big), P(out), s)
        _refused("emoasr_conv2_wgrad", f, 1, T1, F1, 128, P(big), P(big), P(out), P(out2), 0, s)
    # channel divisibility
    _refused("emoasr_conv1_wgrad", f, 1, 7, 7, 12, P(big), P(big), P(out), P(out2), 0, P(scr), s)
    _refused("emoasr_conv1_wgrad", f, 1, 7, 7, 1032, P(big), P(big), P(out), P(out2), 0, P(scr), s)
    _refused("emoasr_conv2_fwd", f, 1, 3, 3, 48, P(big), P(big), P(out), ctypes.byref(ep), s)
    _refused("emoasr_conv2_dgrad", f, 1, 3, 3, 96, P(big), P(big), P(big), P(out), s)
    _refused("emoasr_conv2_dgrad_kc", b, 1, 3, 3, 128, P(big), P(big), P(big), P(out), s)
    _refused("emoasr_conv2_col2im", f, 1, 3, 3, 12, P(big), P(big), P(out), s)
    _refused("emoasr_conv2_wgrad", f, 1, 3, 3, 64, P(big), P(big), P(out), P(out2), 0, s)
    _refused("emoasr_conv2_dgrad_w1", b, 1, 7, 7, 128, P(big), P(big), P(big), P(big), P(out), P(out2), 0, P(scr), s)
    # F1 = 65 on conv1_wgrad (F = 131)
    _refused("emoasr_conv1_wgrad", f, 1, 7, 131, 8, P(big), P(big), P(out), P(out2), 0, P(scr), s)
    # a non-bf16 dtype on _kc and _w1
    for code in (lib.F32, lib.F32X3):
        _refused("emoasr_conv2_dgrad_kc", code, 1, 3, 3, 256, P(big), P(big), P(big), P(out), s)
        _refused("emoasr_conv2_dgrad_w1", code, 1, 7, 7, 256, P(big), P(big), P(big), P(big), P(out), P(out2), 0, P(scr), s)
    _refused("emoasr_conv1_fwd", 7, 1, 7, 7, 8, P(big), P(big), P(big), P(out), s)      # an unknown dtype code
    # missing scratch
    _refused("emoasr_conv1_wgrad", f, 1, 7, 7, 8, P(big), P(big), P(out), P(out2), 0, None, s)
    _refused("emoasr_conv2_dgrad_w1", b, 1, 7, 7, 256, P(big), P(big), P(big), P(big), P(out), P(out2), 0, None, s)
    # nseg out of range, an empty segment, a short one, F1 and C of the segmented entry
    seg = (lib.Conv2WgradSeg * 9)()
    for i in range(9):
        seg[i].dy2, seg[i].y1, seg[i].B, seg[i].T1 = big.data_ptr(), big.data_ptr(), 1, 3
    for nseg in (0, -1, lib.CONV2_WGRAD_SEGMENTS + 1):
        _refused("emoasr_conv2_wgrad_seg", b, nseg, seg, 3, 256, P(out), P(out2), s)
    for B_, T1_ in ((0, 3), (1, 2)):
        seg[1].B, seg[1].T1 = B_, T1_
        for code in (f, b):
            _refused("emoasr_conv2_wgrad_seg", code, 2, seg, 3, 256, P(out), P(out2), s)
    seg[1].B, seg[1].T1 = 1, 3
    _refused("emoasr_conv2_wgrad_seg", b, 2, seg, 2, 256, P(out), P(out2), s)
    _refused("emoasr_conv2_wgrad_seg", b, 2, seg, 3, 192, P(out), P(out2), s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out2).all()) and bool(torch.isnan(scr).all()) and _untouched(g, g2, g3)


@pytest.mark.parametrize("acc", [0, 1])
def test_empty_batch(dev, acc):
    """B == 0: the weight-gradient entries zero dw / db when not accumulating and leave them alone when accumulating; nothing else
    is touched; the element entries return without a launch.  (Before this module the conv2 entries had no such branch: the
    forward and the data gradients asked for an empty grid -- a launch error --, emoasr_conv2_wgrad divided by its zero k-tiles on
    the host.  They now return early, as emoasr_conv1_fwd does.)"""
    from emoasr_amd import lib
    f, b = lib.F32, lib.BF16
    big = torch.zeros(1 << 12, device=dev)
    s, P = _stream(), _p
    ep = lib.Epilogue(alpha=1.0, res_scale=1.0, act=1)
    out, g = _nan_out(dev, (1 << 12,), F32)
    scr, gs = _nan_out(dev, (1 << 12,), F32)
    for code in (f, b, lib.F32X3):
        lib.call("emoasr_conv1_fwd", code, 0, 7, 7, 8, P(big), P(big), P(big), P(out), s)
        lib.call("emoasr_conv2_fwd", code, 0, 3, 3, 256, P(big), P(big), P(out), ctypes.byref(ep), s)
        lib.call("emoasr_conv2_dgrad", code, 0, 3, 3, 256, P(big), P(big), P(big), P(out), s)
        lib.call("emoasr_conv2_col2im", code, 0, 3, 3, 256, P(big), P(big), P(out), s)
    lib.call("emoasr_conv2_dgrad_kc", b, 0, 3, 3, 256, P(big), P(big), P(big), P(out), s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and _untouched(g)

    def outs(shape_w, shape_b):
        start = torch.arange(1, shape_w[0] * shape_w[1] + 1, dtype=F32).reshape(shape_w)
        (dw, g0), (db, g1) = _start_out(dev, start), _start_out(dev, start[:, 0].clone())
        return start, dw, db, g0, g1

    def settled(start, dw, db, g0, g1):
        torch.cuda.synchronize()
        assert _untouched(g0, g1, gs) and bool(torch.isnan(scr).all())
        if acc:
            assert torch.equal(dw.cpu(), start) and torch.equal(db.cpu(), start[:, 0])
        else:
            assert bool((dw == 0).all()) and bool((db == 0).all())

    for code in (f, b):
        o = outs((8, 9), (8,))
        lib.call("emoasr_conv1_wgrad", code, 0, 7, 7, 8, P(big), P(big), P(o[1]), P(o[2]), acc, P(scr), s)
        settled(*o)
    for code in (f, b, lib.F32X3):
        o = outs((128, 9 * 128), (128,))
        lib.call("emoasr_conv2_wgrad", code, 0, 3, 3, 128, P(big), P(big), P(o[1]), P(o[2]), acc, s)
        settled(*o)
    o = outs((256, 9), (256,))
    lib.call("emoasr_conv2_dgrad_w1", b, 0, 7, 7, 256, P(big), P(big), P(big), P(big), P(o[1]), P(o[2]), acc, P(scr), s)
    settled(*o)
