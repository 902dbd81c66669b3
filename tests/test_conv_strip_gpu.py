"""The frame-strip form of the fused convolution-module kernels (csrc/convfused.hip, bf16): a workgroup walks `conv_strip`
consecutive 32-frame tiles of one utterance and keeps the halo rows in an LDS ring.

Dense entry points: for every strip length all outputs are EQUAL to the unfused launch sequence (the construction of
test_ops_gpu.py::test_fused_conv_module_kernels_are_bit_identical); for the depthwise weight / bias gradient that holds below
1024 tiles (B cdiv(T, 32) < 1024, every shape here) -- from 1024 on the fused entry folds its partials in four slices that meet in
float atomics (tests/test_conv_kernels_gpu.py::test_weight_gradient_fold_at_1024_tiles).  Stacked entry points (several segments of unequal length
in one launch): everything but the depthwise weight / bias gradient is EQUAL to the dense entry points called once per
segment; those two are f32 sums in another order (one partial row per strip) and are held to an f64 reference with the unfused
kernels' own error as the yardstick."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_long, c_void_p

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

STRIPS = [1, 2, 3, 4, 8, 0]   # tiles per strip; 0 = the library chooses
EPS = 1e-5

# (B, T, C, K): the smallest shapes at which each mechanism can fail
SHAPES = [(2, 20, 144, 31),    # one partial tile, partial channel block
          (2, 33, 256, 15),    # second tile of one frame, pad 7
          (3, 70, 256, 31),    # three tiles
          (1, 100, 512, 7),    # two channel blocks
          (2, 130, 256, 31),   # five tiles: the ring wraps; S = 4 leaves a second strip of one tile (left halo from memory)
          (2, 128, 256, 31)]   # strips end exactly on a tile edge

# stacked launches: ([(B, T), ...], C, K)
SEGSETS = [([(3, 70), (2, 130), (4, 20)], 256, 31),
           ([(1, 200), (5, 33)], 144, 15)]


def _rnd(gen, dev, *shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, device=dev, generator=gen) * scale).to(dtype)


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


# ---------------------------------------------------------------- dense entry points
_DENSE = {}


def _dense_case(dev, shape):
    """inputs of a shape and the outputs of the round-1 (unfused, not LDS-staged) kernels, computed once"""
    if shape not in _DENSE:
        from emoasr_amd import lib
        B, T, C, K = shape
        gen = _gen(dev, 1234 + 7 * T + C + K)
        bf = torch.bfloat16
        inp = dict(g=_rnd(gen, dev, B * T, 2 * C, dtype=bf), w=_rnd(gen, dev, C, K, scale=K ** -0.5),
                   bias=_rnd(gen, dev, C, scale=0.1), gamma=1 + 0.1 * _rnd(gen, dev, C), beta=0.1 * _rnd(gen, dev, C),
                   ds=_rnd(gen, dev, B * T, C, dtype=bf), nbt=torch.zeros((), device=dev, dtype=torch.int64))
        with lib.options(dwconv_lds=0):
            ref = _unfused(dev, shape, inp)
        _DENSE[shape] = (inp, ref)
    return _DENSE[shape]


def _unfused(dev, shape, i):
    from emoasr_amd import ops
    B, T, C, K = shape
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    gl = ops.glu_fwd(i["g"])
    c, mean, var = ops.dwconv_bn_stats_fwd(gl.view(B, T, C), i["w"], i["bias"], rm, rv, 0.1, i["nbt"].clone())
    c_eval = ops.dwconv_fwd(gl.view(B, T, C), i["w"], i["bias"])
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dc = ops.bn_swish_bwd(i["ds"], c.view(B * T, C), mean, var, i["gamma"], i["beta"], EPS, dgam, dbet)
    dgl = ops.dwconv_bwd_x(dc.view(B, T, C), i["w"])
    dw, db = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
    ops.dwconv_bwd_w(dc.view(B, T, C), gl.view(B, T, C), dw, db, accumulate=True)
    dg = ops.glu_bwd(i["g"], dgl.view(B * T, C))
    return dict(c=c, mean=mean, var=var, rm=rm, rv=rv, c_eval=c_eval, dgam=dgam, dbet=dbet, dw=dw, db=db, dg=dg, dgl=dgl)


def _fused(dev, shape, i):
    from emoasr_amd import ops
    B, T, C, K = shape
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    c, mean, var = ops.glu_dwconv_fwd(i["g"], B, T, i["w"], i["bias"], rm, rv, 0.1, i["nbt"].clone(), True)
    c_eval = ops.glu_dwconv_fwd(i["g"], B, T, i["w"], i["bias"], rm, rv, training=False)[0]
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dw, db = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
    dg = ops.conv_bwd_fused(i["ds"], c.view(B * T, C), mean, var, i["gamma"], i["beta"], EPS, dgam, dbet, i["g"], i["w"], dw,
                            db, B, T)
    return dict(c=c, mean=mean, var=var, rm=rm, rv=rv, c_eval=c_eval, dgam=dgam, dbet=dbet, dw=dw, db=db, dg=dg)


@pytest.mark.parametrize("S", STRIPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_entries_bit_identical_for_every_strip_length(dev, shape, S):
    """glu_dwconv_fwd / conv_bwd_fused (and the plain LDS-staged depthwise convolution and its data gradient, which walk the
    same strips) against the unfused round-1 kernels: EQUAL, weight gradients included -- the dense entry flushes its
    weight-gradient sums once per tile."""
    from emoasr_amd import lib
    inp, ref = _dense_case(dev, shape)
    with lib.options(conv_strip=S):
        lds = _unfused(dev, shape, inp)
        got = _fused(dev, shape, inp)
    for k, v in ref.items():
        assert torch.equal(lds[k], v), f"S={S}: LDS-staged dwconv: {k} differs"
        if k in got:
            assert torch.equal(got[k], v), f"S={S}: fused: {k} differs (max {(got[k].float() - v.float()).abs().max().item():.3e})"


# ---------------------------------------------------------------- stacked entry points
def _seg_api():
    from emoasr_amd import lib
    l = lib.load()
    P, I, Fl, PS = c_void_p, c_int, c_float, POINTER(lib.Segments)
    l.emoasr_conv_module_fwd_seg.argtypes = [I, PS, I, I, P, P, P, P, P, P, P, P, P, Fl, P, P, P, Fl, P, I, P]
    l.emoasr_conv_module_fwd_seg.restype = c_int
    l.emoasr_conv_module_bwd_seg.argtypes = [I, PS, I, I, P, P, P, P, P, P, Fl] + [P] * 10
    l.emoasr_conv_module_bwd_seg.restype = c_int
    q = l.emoasr_conv_module_bwd_seg_scratch_floats
    q.argtypes, q.restype = [PS, I, I, I], c_long
    return q


def _segments(segs):
    from emoasr_amd import lib
    s = lib.Segments()
    s.n = len(segs)
    for i, (B, T) in enumerate(segs):
        s.B[i], s.T[i] = B, T
    return s


def _stacked_fwd(dev, segs, C, K, i):
    from emoasr_amd import lib
    from emoasr_amd.ops import _p, _stream, dt
    _seg_api()
    seg, n, M = _segments(segs), len(segs), sum(B * T for B, T in segs)
    bf = torch.bfloat16
    c, z = torch.empty(M, C, device=dev, dtype=bf), torch.empty(M, C, device=dev, dtype=bf)
    part = torch.empty(sum(lib.size_query("emoasr_dwconv_stats_floats", B, T, C) for B, T in segs), device=dev)
    bmean, bvar = torch.empty(n, C, device=dev), torch.empty(n, C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros((), device=dev, dtype=torch.int64)
    lib.call("emoasr_conv_module_fwd_seg", dt(i["g"]), ctypes.byref(seg), C, K, _p(i["g"]), _p(i["w"]), _p(i["bias"]), _p(c),
             _p(part), _p(bmean), _p(bvar), _p(rm), _p(rv), 0.1, _p(nbt), _p(i["gamma"]), _p(i["beta"]), EPS, _p(z), 1, _stream())
    return dict(c=c, z=z, bmean=bmean, bvar=bvar, rm=rm, rv=rv, nbt=nbt)


def _stacked_bwd(dev, segs, C, K, i, dz, c, bmean, bvar):
    """-> dg, dw, db; the weight-gradient scratch is NaN-filled first: a row outside the live strips must not be read"""
    from emoasr_amd import lib
    from emoasr_amd.ops import _p, _stream, dt
    q = _seg_api()
    seg = _segments(segs)
    bn_scr = torch.empty(q(ctypes.byref(seg), C, K, 0), device=dev)
    dw_scr = torch.full((q(ctypes.byref(seg), C, K, 1),), float("nan"), device=dev)
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dw, db = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
    dg = torch.empty_like(i["g"])
    lib.call("emoasr_conv_module_bwd_seg", dt(i["g"]), ctypes.byref(seg), C, K, _p(dz), _p(c), _p(bmean), _p(bvar), _p(i["gamma"]),
             _p(i["beta"]), EPS, _p(dgam), _p(dbet), _p(i["g"]), _p(i["w"]), _p(dg), _p(dw), _p(db), _p(bn_scr), _p(dw_scr),
             _stream())
    return dg, dw, db


_STACKED = {}


def _stacked_case(dev, idx):
    """inputs of a segment set; the dense entry points called once per segment, in order; the unfused weight gradient and
    its f64 reference from the unfused intermediates -- computed once (at one tile per strip)"""
    if idx in _STACKED:
        return _STACKED[idx]
    from emoasr_amd import lib, ops
    segs, C, K = SEGSETS[idx]
    pad = (K - 1) // 2
    gen = _gen(dev, 4321 + idx)
    bf = torch.bfloat16
    M = sum(B * T for B, T in segs)
    i = dict(g=_rnd(gen, dev, M, 2 * C, dtype=bf), w=_rnd(gen, dev, C, K, scale=K ** -0.5), bias=_rnd(gen, dev, C, scale=0.1),
             gamma=1 + 0.1 * _rnd(gen, dev, C), beta=0.1 * _rnd(gen, dev, C))
    dz = _rnd(gen, dev, M, C, dtype=bf)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros((), device=dev, dtype=torch.int64)
    cs, zs, means, vars_, dgs = [], [], [], [], []
    dw_u, db_u = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
    dw_ref = torch.zeros(C, K, device=dev, dtype=torch.float64)
    db_ref = torch.zeros(C, device=dev, dtype=torch.float64)
    with lib.options(conv_strip=1):
        r0 = 0
        for B, T in segs:
            gi, dzi = i["g"][r0:r0 + B * T], dz[r0:r0 + B * T]
            c, mean, var = ops.glu_dwconv_fwd(gi, B, T, i["w"], i["bias"], rm, rv, 0.1, nbt, True)
            c2 = c.view(B * T, C)
            zs.append(ops.bn_swish_fwd(c2, mean, var, i["gamma"], i["beta"], EPS))
            dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            dwd, dbd = torch.zeros(C, K, device=dev), torch.zeros(C, device=dev)
            dgs.append(ops.conv_bwd_fused(dzi, c2, mean, var, i["gamma"], i["beta"], EPS, dgam, dbet, gi, i["w"], dwd, dbd, B, T))
            # the unfused intermediates (test_ops_gpu.py pins both to the fused kernel's internals)
            dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            dc = ops.bn_swish_bwd(dzi, c2, mean, var, i["gamma"], i["beta"], EPS, dgam, dbet).view(B, T, C)
            gl = ops.glu_fwd(gi).view(B, T, C)
            ops.dwconv_bwd_w(dc, gl, dw_u, db_u, accumulate=True)
            dcd, zp = dc.double(), F.pad(gl.double(), (0, 0, pad, pad))
            for j in range(K):   # dw_ref[c, j] = sum_t dc[t] * z[t + j - pad]
                dw_ref[:, j] += (dcd * zp[:, j:j + T]).sum(dim=(0, 1))
            db_ref += dcd.sum(dim=(0, 1))
            cs.append(c2), means.append(mean), vars_.append(var)
            r0 += B * T
    ref = dict(c=torch.cat(cs), z=torch.cat(zs), bmean=torch.stack(means), bvar=torch.stack(vars_), rm=rm, rv=rv, nbt=nbt)
    _STACKED[idx] = (i, dz, ref, torch.cat(dgs), dw_u, db_u, dw_ref, db_ref)
    return _STACKED[idx]


@pytest.mark.parametrize("S", STRIPS)
@pytest.mark.parametrize("idx", range(len(SEGSETS)), ids=["70-130-20", "200-33"])
def test_stacked_entries_against_dense_per_segment(dev, idx, S):
    """emoasr_conv_module_fwd_seg / _bwd_seg over segments of unequal length in ONE call.  c, z, the batch and running
    statistics, num_batches_tracked and dg are EQUAL to the dense entry points per segment.  dw / db are f32 sums in another
    order: their distance to an f64 reference stays within 4 x the unfused kernels' own distance e0 (a strip's sequential
    chain is up to 8 times longer, typical rounding error grows like sqrt(8) = 2.9; a dropped tile is far outside).  The
    weight-gradient scratch is NaN-filled before the call: dw / db finite proves that only live rows are read."""
    from emoasr_amd import lib
    segs, C, K = SEGSETS[idx]
    i, dz, ref, dg_ref, dw_u, db_u, dw_ref, db_ref = _stacked_case(dev, idx)
    with lib.options(conv_strip=S):
        got = _stacked_fwd(dev, segs, C, K, i)
        dg, dw, db = _stacked_bwd(dev, segs, C, K, i, dz, got["c"], got["bmean"], got["bvar"])
    for k, v in ref.items():
        assert torch.equal(got[k], v), f"S={S}: {k} differs (max {(got[k].double() - v.double()).abs().max().item():.3e})"
    assert torch.equal(dg, dg_ref), f"S={S}: dg differs (max {(dg.float() - dg_ref.float()).abs().max().item():.3e})"
    assert torch.isfinite(dw).all() and torch.isfinite(db).all(), f"S={S}: a partial row outside the live strips was read"
    for name, g_, u_, r_ in (("dw", dw, dw_u, dw_ref), ("db", db, db_u, db_ref)):
        e0 = (u_.double() - r_).abs().max().item()
        e = (g_.double() - r_).abs().max().item()
        print(f"S={S} {name}: unfused e0 {e0:.3e}, strips {e:.3e}, scale {r_.abs().max().item():.3e}")
        assert e <= 4 * e0, f"S={S}: {name} error {e:.3e} against the f64 reference, unfused kernels e0 {e0:.3e} (bound 4 e0)"


@pytest.mark.parametrize("S", STRIPS)
def test_stacked_backward_drops_no_tile(dev, S):
    """dc == 1 on every row of one segment (five tiles, a strip boundary inside it for S = 2, 3, 4) and 0 on the others:
    the bias gradient must be that segment's row count exactly.  With c = 1, mean 0, invstd 1, gamma -1, beta 1 and dz = 2:
    xhat = 1, dbn = 2 swish'(0) = 1, both BatchNorm means are 1, dc = -1 (1 - 1 - 1) = 1."""
    from emoasr_amd import ops
    segs, C, K = [(3, 70), (2, 130), (4, 20)], 256, 31
    one = 1
    gen = _gen(dev, 99)
    bf = torch.bfloat16
    M = sum(B * T for B, T in segs)
    r0 = sum(B * T for B, T in segs[:one])
    n1 = segs[one][0] * segs[one][1]
    i = dict(g=_rnd(gen, dev, M, 2 * C, dtype=bf), w=_rnd(gen, dev, C, K, scale=K ** -0.5), bias=None,
             gamma=-torch.ones(C, device=dev), beta=torch.ones(C, device=dev))
    c = torch.ones(M, C, device=dev, dtype=bf)
    dz = torch.zeros(M, C, device=dev, dtype=bf)
    dz[r0:r0 + n1] = 2
    bmean, bvar = torch.zeros(len(segs), C, device=dev), torch.full((len(segs), C), 1 - EPS, device=dev)
    dgam, dbet = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dc = ops.bn_swish_bwd(dz[r0:r0 + n1], c[r0:r0 + n1], bmean[one], bvar[one], i["gamma"], i["beta"], EPS, dgam, dbet)
    assert torch.equal(dc, torch.ones_like(dc)), "the construction does not give dc == 1"
    from emoasr_amd import lib
    with lib.options(conv_strip=S):
        _, dw, db = _stacked_bwd(dev, segs, C, K, i, dz, c, bmean, bvar)
    assert torch.isfinite(dw).all()
    assert torch.equal(db, torch.full_like(db, float(n1))), f"S={S}: db {db.min().item()} .. {db.max().item()}, rows {n1}"
