"""Tensor-level wrappers over the C ABI (emoasr_amd/lib.py).

torch is used only as the owner of device memory and of the current HIP stream; every
function here enqueues hand-written HIP kernels from libemoasr_hip.so.  Nothing in this
module has autograd: forward and backward ops are separate entry points and the model
code (emoasr_amd/engine/) sequences them explicitly.
"""
import ctypes
from ctypes import byref, c_void_p

import os
import threading
from types import SimpleNamespace

import torch

from . import lib
from .lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SWISH, BF16, F32, F32X3, AttnArgs, Epilogue  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt(t):
    """dtype code of a call on tensor t: F32 / BF16, or F32X3 for an f32 tensor while the calling thread's engine runs split products"""
    if t.dtype == torch.float32 and split_products():
        return F32X3
    return _DT[t.dtype]


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


_STREAM_CACHE = None


def _stream():
    if _STREAM_CACHE is not None:
        return _STREAM_CACHE
    return c_void_p(torch.cuda.current_stream().cuda_stream)


# "f32x3" (lib.F32X3): f32 tensors whose matrix products run as three bf16 MFMAs over (hi, lo) operand pairs.  The mode is an
# argument of every C call (the dtype code dt() returns); on this side it is a property of the calling engine, held per THREAD for
# the duration of the engine's entry point (an autograd thread or a second engine never sees another's mode; there is no library
# state to go stale -- rounds 4-5 had a process-wide option).
# EMOASR_FORCE_SPLIT=1: EVERY f32 product of the process runs split, whatever an engine asks for (test aid: the whole GPU suite's f32
# cases under the split arithmetic, profiles/r05_forced_split_suite.txt)
_FORCE_SPLIT = os.environ.get("EMOASR_FORCE_SPLIT", "0") == "1"
_mode = threading.local()


def split_products(on=None):
    """the calling thread's f32 product mode: split_products(True / False) sets it, split_products() reads it"""
    if on is not None:
        _mode.split = bool(on)
    return bool(getattr(_mode, "split", False)) or _FORCE_SPLIT


class stream_scope:
    """Resolve torch's current stream once for a whole forward/backward sequence (the lookup costs
    more than a kernel launch when done per op).  f32_split: also assert that mode of the f32 products (None: leave it)."""

    def __init__(self, f32_split=None):
        self.f32_split = f32_split

    def __enter__(self):
        global _STREAM_CACHE
        self.prev = _STREAM_CACHE
        _STREAM_CACHE = c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.f32_split is not None:
            split_products(self.f32_split)
        return self

    def __exit__(self, *exc):
        global _STREAM_CACHE
        _STREAM_CACHE = self.prev
        return False


def _chk(t, dtype=None):
    assert t.is_cuda, "emoasr_amd ops need device tensors (no CPU fallback)"
    if dtype is not None:
        assert t.dtype == dtype, f"expected {dtype}, got {t.dtype}"
    return t


def _rows(t):
    """(rows, cols, ld) of a 2-D view whose last dim is contiguous."""
    assert t.stride(-1) == 1
    if t.dim() == 1:
        return 1, t.shape[0], t.shape[0]
    assert t.dim() == 2
    return t.shape[0], t.shape[1], t.stride(0)


def make_epilogue(bias=None, act=ACT_NONE, alpha=1.0, residual=None, res_scale=1.0, pre_out=None,
                  dact_pre=None, dact=ACT_NONE, drop_p=0.0, seed=0, out_f32=False):
    return Epilogue(None if bias is None else bias.data_ptr(),
                    None if residual is None else residual.data_ptr(),
                    None if pre_out is None else pre_out.data_ptr(),
                    None if dact_pre is None else dact_pre.data_ptr(),
                    alpha, res_scale, act, dact, 0 if residual is None else residual.stride(0),
                    1 if out_f32 else 0, drop_p, seed)


def gemm_nt(a, b, out=None, **epi):
    """out[M,N] = epilogue(a[M,K] @ b[N,K]^T)"""
    M, K, lda = _rows(_chk(a))
    N, Kb, ldb = _rows(_chk(b, a.dtype))
    assert K == Kb, (a.shape, b.shape)
    out_f32 = epi.get("out_f32", False)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    ep = make_epilogue(**epi)
    lib.call("emoasr_gemm_nt", dt(a), M, N, K, _p(a), lda, _p(b), ldb, _p(out), out.stride(0), byref(ep),
             _stream())
    return out


def gemm_nn(a, b, out=None, **epi):
    """out[M,N] = epilogue(a[M,K] @ b[K,N])   (b row-major [K,N]: dgrad with b = weight [out,in])"""
    M, K, lda = _rows(_chk(a))
    Kb, N, ldb = _rows(_chk(b, a.dtype))
    assert K == Kb, (a.shape, b.shape)
    out_f32 = epi.get("out_f32", False)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    ep = make_epilogue(**epi)
    lib.call("emoasr_gemm_nn", dt(a), M, N, K, _p(a), lda, _p(b), ldb, _p(out), out.stride(0), byref(ep),
             _stream())
    return out


def gemm_tn(a, b, out=None, alpha=1.0, accumulate=False, colsum=None, colsum_scale=1.0):
    """out[N1,N2] (+)= alpha * a[K,N1]^T @ b[K,N2]  (f32 out);
    colsum[N1] (+)= colsum_scale * a.sum(0) (fused bias gradient)"""
    K, N1, lda = _rows(_chk(a))
    Kb, N2, ldb = _rows(_chk(b, a.dtype))
    assert K == Kb
    if out is None:
        assert not accumulate
        out = torch.empty(N1, N2, device=a.device, dtype=torch.float32)
    _chk(out, torch.float32)
    lib.call("emoasr_gemm_tn", dt(a), N1, N2, K, _p(a), lda, _p(b), ldb, _p(out), out.stride(0), alpha,
             int(accumulate), _p(colsum), colsum_scale, _stream())
    return out


def gemm_tn_grouped(problems, stream=None):
    """problems: list of (a[K,N1], b[K,N2], out[N1,N2] f32, alpha, colsum or None, colsum_scale); every
    out (and colsum) is accumulated into, all in one launch per lib.TN_GROUP_MAX problems.
    stream: raw HIP stream handle (int) to enqueue on instead of torch's current stream."""
    sptr = _stream() if stream is None else c_void_p(stream)
    for i0 in range(0, len(problems), lib.TN_GROUP_MAX):
        chunk = problems[i0:i0 + lib.TN_GROUP_MAX]
        arr = (lib.TnProblem * len(chunk))()
        for q, (a, b, out, alpha, colsum, colsum_scale) in zip(arr, chunk):
            K, N1, lda = _rows(_chk(a))
            Kb, N2, ldb = _rows(_chk(b, a.dtype))
            assert K == Kb and out.shape == (N1, N2) and a.dtype == chunk[0][0].dtype
            _chk(out, torch.float32)
            q.N1, q.N2, q.K, q.A, q.lda, q.B, q.ldb = N1, N2, K, a.data_ptr(), lda, b.data_ptr(), ldb
            q.C, q.ldc, q.alpha = out.data_ptr(), out.stride(0), alpha
            q.colsum = None if colsum is None else colsum.data_ptr()
            q.colsum_scale = colsum_scale
        lib.call("emoasr_gemm_tn_grouped", dt(chunk[0][0]), len(chunk), arr, sptr)


def gemm_tn_grouped_plan(shapes, dtype=torch.bfloat16):
    """Launch plan of one grouped call for shapes = [(N1, N2, K), ...] (at most lib.TN_GROUP_MAX), host only:
    -> (split-K slices per problem, tile edge, workgroups of the launch)"""
    arr = (lib.TnProblem * len(shapes))()
    for q, (N1, N2, K) in zip(arr, shapes):
        q.N1, q.N2, q.K, q.lda, q.ldb, q.ldc, q.alpha = N1, N2, K, (N1 + 7) // 8 * 8, N2, N2, 1.0
    splits, tile, blocks = (ctypes.c_int * len(shapes))(), ctypes.c_int(), ctypes.c_int()
    lib.call("emoasr_gemm_tn_grouped_plan", _DT[dtype], len(shapes), arr, splits, byref(tile), byref(blocks))
    return list(splits), tile.value, blocks.value


def gemm_nn_batched(a, b, out, M, N, K, lda, sa, ldb, sb, ldc, sc, nb, nh, alpha=1.0, accumulate=False):
    """out[b,h] (+)= alpha * a[b,h] (M x K, k-contiguous) @ b[b,h] (K x N, k-major); s* = (outer, inner)
    batch strides in elements; base pointers are the tensors' data pointers."""
    lib.call("emoasr_gemm_nn_batched", dt(a), M, N, K, _p(a), lda, sa[0], sa[1], _p(b), ldb, sb[0], sb[1],
             _p(out), ldc, sc[0], sc[1], nb, nh, alpha, int(accumulate), _stream())
    return out


def colsum(x, out=None, scale=1.0, accumulate=False):
    M, N, ld = _rows(_chk(x))
    if out is None:
        out = torch.empty(N, device=x.device, dtype=torch.float32)
    lib.call("emoasr_colsum", dt(x), M, N, _p(x), ld, _p(_chk(out, torch.float32)), scale, int(accumulate),
             _stream())
    return out


# ---- front-end -----------------------------------------------------------------------
def conv1_fwd(x, w1, b1, dtype):
    B, T, F = x.shape
    C = w1.shape[0]
    T1, F1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    y1 = torch.empty(B, T1, F1, C, device=x.device, dtype=dtype)
    lib.call("emoasr_conv1_fwd", _DT[dtype], B, T, F, C, _p(_chk(x, torch.float32)), _p(w1), _p(b1), _p(y1),
             _stream())
    return y1


def conv1_wgrad(x, dy1, dw1, db1, accumulate=False):
    B, T, F = x.shape
    C = dy1.shape[-1]
    scratch = torch.empty(lib.size_query("emoasr_conv1_wgrad_scratch_floats", B, T, C), device=x.device, dtype=torch.float32)
    lib.call("emoasr_conv1_wgrad", dt(dy1), B, T, F, C, _p(x), _p(dy1), _p(dw1), _p(db1), int(accumulate),
             _p(scratch), _stream())


def conv2_fwd(y1, w, out=None, **epi):
    B, T1, F1, C = y1.shape
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    if out is None:
        y2 = torch.empty(B, T2, F2, C, device=y1.device, dtype=y1.dtype)
    else:  # (a contiguous slice of a larger buffer: the stacked micro-batches of engine.ctc_train_stacked)
        assert out.is_contiguous() and out.numel() == B * T2 * F2 * C and out.dtype == y1.dtype
        y2 = out.view(B, T2, F2, C)
    ep = make_epilogue(**epi)
    lib.call("emoasr_conv2_fwd", dt(y1), B, T1, F1, C, _p(y1), _p(_chk(w, y1.dtype)), _p(y2), byref(ep),
             _stream())
    return y2


def conv2_wgrad(dy2, y1, dw, dbias=None, accumulate=False):
    B, T1, F1, C = y1.shape
    lib.call("emoasr_conv2_wgrad", dt(y1), B, T1, F1, C, _p(dy2), _p(y1), _p(_chk(dw, torch.float32)),
             _p(dbias), int(accumulate), _stream())


def conv2_wgrad_seg(segs, dw, dbias=None):
    """segs: up to lib.CONV2_WGRAD_SEGMENTS pairs (dy2 [B,T2,F2,C] or [B*T2*F2, C], y1 [B,T1,F1,C]) sharing F1 and C; dw (and
    dbias) accumulate the weight gradient of all of them as ONE reduction -- one launch where the 256-tile kernel applies"""
    assert 1 <= len(segs) <= lib.CONV2_WGRAD_SEGMENTS
    _, _, F1, C = segs[0][1].shape
    arr = (lib.Conv2WgradSeg * len(segs))()
    for q, (dy2, y1) in zip(arr, segs):
        B, T1, f1, c = y1.shape
        assert (f1, c) == (F1, C) and y1.dtype == segs[0][1].dtype
        _chk(dy2, y1.dtype)
        q.dy2, q.y1, q.B, q.T1 = dy2.data_ptr(), _chk(y1).data_ptr(), B, T1
    lib.call("emoasr_conv2_wgrad_seg", dt(segs[0][1]), len(segs), arr, F1, C, _p(_chk(dw, torch.float32)), _p(dbias), _stream())


def conv2_dgrad(dy2, w, y1):
    """dy2 [B,T2,F2,C] (or [B*T2*F2, C]), w [C, 9C] (conv2_fwd's layout), y1 [B,T1,F1,C] -> dy1 = relu'(y1) * conv2^T(dy2)"""
    B, T1, F1, C = y1.shape
    dy1 = torch.empty_like(y1)
    lib.call("emoasr_conv2_dgrad", dt(y1), B, T1, F1, C, _p(_chk(dy2, y1.dtype)), _p(_chk(w, y1.dtype)), _p(y1), _p(dy1),
             _stream())
    return dy1


def conv2_dgrad_kc(dy2, wt, y1):
    """as conv2_dgrad on the large-tile kernel: wt [C, 9C] = conv.2.weight.permute(1, 2, 3, 0) (c, kh, kw, n); bf16, C % 256 == 0"""
    B, T1, F1, C = y1.shape
    dy1 = torch.empty_like(y1)
    lib.call("emoasr_conv2_dgrad_kc", dt(y1), B, T1, F1, C, _p(_chk(dy2, y1.dtype)), _p(_chk(wt, y1.dtype)), _p(y1), _p(dy1),
             _stream())
    return dy1


def conv2_dgrad_w1(dy2, wt, y1, x, dw1, db1, accumulate=False):
    """conv2_dgrad_kc with conv1_wgrad(x, dy1, dw1, db1) folded into its epilogue: dy1 is never materialised.
    x [B,T,F] f32 (conv1's input), dw1 [C,9], db1 [C] f32"""
    B, T1, F1, C = y1.shape
    Bx, T, Fd = x.shape
    assert Bx == B and (T - 3) // 2 + 1 == T1 and (Fd - 3) // 2 + 1 == F1, (x.shape, y1.shape)
    scratch = torch.empty(lib.size_query("emoasr_conv2_dgrad_w1_scratch_floats", B, T, Fd, C), device=x.device,
                          dtype=torch.float32)
    lib.call("emoasr_conv2_dgrad_w1", dt(y1), B, T, Fd, C, _p(_chk(dy2, y1.dtype)), _p(_chk(wt, y1.dtype)), _p(y1),
             _p(_chk(x, torch.float32)), _p(_chk(dw1, torch.float32)), _p(_chk(db1, torch.float32)), int(accumulate),
             _p(scratch), _stream())


def gemm_nt_big(a, b, out=None, bias=None, relu=False):
    """out[M,N] = relu?(a[M,K] @ b[N,K]^T + bias) on the large-tile kernel (bf16, N % 8 == 0, K % 64 == 0)"""
    M, K, lda = _rows(_chk(a, torch.bfloat16))
    N, Kb, ldb = _rows(_chk(b, a.dtype))
    assert K == Kb, (a.shape, b.shape)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    lib.call("emoasr_gemm_nt_big", dt(a), M, N, K, _p(a), lda, _p(b), ldb, _p(out), out.stride(0), _p(bias), int(relu),
             _stream())
    return out


def conv2_col2im(dcol, y1):
    B, T1, F1, C = y1.shape
    dy1 = torch.empty_like(y1)
    lib.call("emoasr_conv2_col2im", dt(y1), B, T1, F1, C, _p(dcol), _p(y1), _p(dy1), _stream())
    return dy1


# ---- LayerNorm -------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, want_stats=True):
    M, N, ld = _rows(_chk(x))
    assert ld == N
    y = torch.empty_like(x)
    mean = torch.empty(M, device=x.device, dtype=torch.float32) if want_stats else None
    rstd = torch.empty(M, device=x.device, dtype=torch.float32) if want_stats else None
    lib.call("emoasr_layernorm_fwd", dt(x), M, N, _p(x), _p(gamma), _p(beta), eps, _p(y), _p(mean), _p(rstd),
             _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, branch=None, deferred=None):
    """dx = dres + LN'(dy); dgamma / dbeta accumulated.
    branch=(scale, p, seed): also return dropout(dx * scale) -- the gradient entering the next residual
    branch of the backward sweep (replaces a scale_dropout pass); returns (dx, dy_branch).
    deferred: a list; the dgamma/dbeta fold is postponed and recorded there for layernorm_bwd_finalize."""
    M, N, ld = _rows(_chk(x))
    dx = torch.empty_like(x)
    scratch = None
    if dgamma is not None or dbeta is not None:
        scratch = torch.empty(lib.size_query("emoasr_layernorm_bwd_scratch_floats", N), device=x.device, dtype=torch.float32)
    if branch is None and deferred is None:
        lib.call("emoasr_layernorm_bwd", dt(x), M, N, _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx),
                 _p(dgamma), _p(dbeta), _p(scratch), _stream())
        return dx
    o = lib.LnBwdOpts()
    dy2 = None
    if branch is not None:
        dy2 = torch.empty_like(x)
        o.dy2, o.scale2, o.drop_p2, o.seed2 = dy2.data_ptr(), branch[0], branch[1], branch[2]
    if deferred is not None and scratch is not None:
        o.defer_finalize = 1
        deferred.append((M, N, scratch, dgamma, dbeta))
    lib.call("emoasr_layernorm_bwd_ex", dt(x), M, N, _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx),
             _p(dgamma), _p(dbeta), _p(scratch), byref(o), _stream())
    return dx if branch is None else (dx, dy2)


def layernorm_bwd_finalize(deferred):
    """fold the dgamma / dbeta partials of deferred layernorm_bwd calls (one launch per 64 of them)"""
    for i0 in range(0, len(deferred), lib.LN_FINALIZE_MAX):
        chunk = deferred[i0:i0 + lib.LN_FINALIZE_MAX]
        arr = (lib.LnFinalizeItem * len(chunk))()
        for it, (M, N, scratch, dgamma, dbeta) in zip(arr, chunk):
            it.M, it.N, it.part = M, N, scratch.data_ptr()
            it.dgamma = None if dgamma is None else dgamma.data_ptr()
            it.dbeta = None if dbeta is None else dbeta.data_ptr()
        lib.call("emoasr_layernorm_bwd_finalize", len(chunk), arr, _stream())
    del deferred[:]


# ---- attention -------------------------------------------------------------------------
def _attn_args(q, k, v, H, pos, bias_u, bias_v, klens, causal, scale, drop_p, seed):
    B, Tq, D = q.shape
    Tk = k.shape[1]
    a = AttnArgs()
    a.B, a.H, a.DK, a.Tq, a.Tk = B, H, D // H, Tq, Tk
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    assert q.stride(0) == Tq * q.stride(1) and k.stride(0) == Tk * k.stride(1) and v.stride(0) == Tk * v.stride(1)
    a.ldq, a.ldk, a.ldv = q.stride(1), k.stride(1), v.stride(1)
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    if pos is not None:
        a.pos, a.ldp = pos.data_ptr(), pos.stride(0)
    a.bias_u = None if bias_u is None else bias_u.data_ptr()
    a.bias_v = None if bias_v is None else bias_v.data_ptr()
    a.klens = None if klens is None else klens.data_ptr()
    a.causal = int(causal)
    a.scale, a.drop_p, a.seed = scale, drop_p, seed
    return a


def attn_dropmask(q, k, H, klens=None, drop_p=0.0, seed=0):
    """the attention-dropout keep mask of an attn_fwd / attn_bwd call with these arguments as bits: uint32 [B * Tq, H, ceil(Tk / 32)]
    (emoasr_attn_t::keep_mask: hashed once, tested by the forward and both passes of the fused backward)"""
    B, Tq, _ = q.shape
    nw = lib.size_query("emoasr_attn_dropmask_words", k.shape[1])
    a = _attn_args(q, k, k, H, None, None, None, klens, False, 1.0, drop_p, seed)
    mask = torch.zeros(B * Tq, H, nw, device=q.device, dtype=torch.int32)
    lib.call("emoasr_attn_dropmask", dt(q), byref(a), mask.data_ptr(), nw, _stream())
    return mask


def attn_fwd(q, k, v, H, scale, pos=None, bias_u=None, bias_v=None, klens=None, causal=False, drop_p=0.0,
             seed=0, store_scores=False, keep_mask=None):
    """q [B,Tq,D], k/v [B,Tk,D] (views with a row stride are fine) -> out [B,Tq,D], lse [B,H,Tq]
    (+ st f32 [B,H,Tk,ldst], the scaled scores S^T kept for the backward, if store_scores)"""
    B, Tq, D = q.shape
    a = _attn_args(q, k, v, H, pos, bias_u, bias_v, klens, causal, scale, drop_p, seed)
    out = torch.empty(B, Tq, D, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
    a.out, a.ldo, a.lse = out.data_ptr(), D, lse.data_ptr()
    if keep_mask is not None:
        a.keep_mask, a.keep_nw = keep_mask.data_ptr(), keep_mask.shape[-1]
    st = None
    if store_scores:
        st = torch.empty(B, H, k.shape[1], (Tq + 7) // 8 * 8, device=q.device, dtype=torch.float32)
        a.st, a.ldst = st.data_ptr(), st.shape[-1]
    lib.call("emoasr_attn_fwd", dt(q), byref(a), _stream())
    return (out, lse, st) if store_scores else (out, lse)


class AttnScratch:
    """Zero-initialised HBM scratch of the materialised attention backward (P^T, dS^T, dBD band).
    Reusable across calls that share (B, H, Tq, Tk, klens) -- e.g. all layers of one step."""

    def __init__(self, B, H, Tq, Tk, dtype, device, rel):
        self.key = (B, H, Tq, Tk, dtype, rel)
        self.ldpd = (Tq + 7) // 8 * 8
        self.ldbd = (2 * Tq - 1 + 7) // 8 * 8
        self.pdT = torch.zeros(B, H, Tk, self.ldpd, device=device, dtype=dtype)
        self.dsT = torch.zeros(B, H, Tk, self.ldpd, device=device, dtype=dtype)
        self.dbd = torch.zeros(H, B, Tq, self.ldbd, device=device, dtype=dtype) if rel else None
        self.cs = torch.empty(H, self.ldbd, device=device, dtype=torch.float32) if rel else None
        # Q + pos_bias_u / Q + pos_bias_v and the per-query-tile dbias partial sums (emoasr_attn_t.qu/qv/dbias_part)
        self.qu = torch.empty(B, Tq, H * 64, device=device, dtype=dtype) if rel else None
        self.qv = torch.empty(B, Tq, H * 64, device=device, dtype=dtype) if rel else None
        self.dbias_part = torch.empty(B * ((Tq + 31) // 32), H, 2, 64, device=device, dtype=torch.float32)


_FUSED_WS = {}


def fused_attn_bwd_ok(q, pos, bias_u, bias_v, causal):
    """can emoasr_attn_bwd_fused take this call? (bf16, no causal mask, relative positions with both biases or none)"""
    return (q.dtype == torch.bfloat16 and not causal and (pos is None or (bias_u is not None and bias_v is not None))
            and (pos is not None or (bias_u is None and bias_v is None)))


def _fused_ws(device, nbytes):
    """scratch of the single-pass attention backward: one buffer per device, grown on demand (no initialisation needed;
    every call runs on the current stream, so calls never overlap)"""
    w = _FUSED_WS.get(device)
    if w is None or w.numel() < nbytes:
        w = _FUSED_WS[device] = torch.empty(int(nbytes * 1.25) + 256, device=device, dtype=torch.uint8)
    return w


def attn_bwd(dout, out, lse, q, k, v, H, scale, dq, dk, dv, pos=None, bias_u=None, bias_v=None, klens=None,
             causal=False, drop_p=0.0, seed=0, dpos=None, dbias_u=None, dbias_v=None, scratch=None,
             materialise=True, st=None, keep_mask=None):
    """dq/dk/dv are written (same strides as q/k/v); dpos/dbias_* are accumulated into.
    materialise="fused": the single-pass kernel (bf16, no causal mask; see fused_attn_bwd_ok);
    materialise=True: dV/dK/dpos through batched GEMMs over stored P^T/dS^T (scratch is allocated
    here unless an AttnScratch for this shape/mask is passed); False: score-recompute kernels."""
    B, Tq, D = q.shape
    if materialise == "fused":
        assert fused_attn_bwd_ok(q, pos, bias_u, bias_v, causal)
        a = _attn_args(q, k, v, H, pos, bias_u, bias_v, klens, causal, scale, drop_p, seed)
        if keep_mask is not None:
            a.keep_mask, a.keep_nw = keep_mask.data_ptr(), keep_mask.shape[-1]
        assert dq.stride() == q.stride() and dk.stride() == k.stride() and dv.stride() == v.stride()
        assert dout.is_contiguous() and out.is_contiguous()
        delta = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
        a.out, a.ldo, a.lse = out.data_ptr(), D, lse.data_ptr()
        a.dout, a.delta = dout.data_ptr(), delta.data_ptr()
        a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
        a.dpos = None if dpos is None else dpos.data_ptr()
        a.dbias_u = None if dbias_u is None else dbias_u.data_ptr()
        a.dbias_v = None if dbias_v is None else dbias_v.data_ptr()
        nb = lib.size_query("emoasr_attn_bwd_fused_ws_bytes", dt(q), B, H, Tq, k.shape[1], int(pos is not None))
        ws = _fused_ws(q.device, nb)
        lib.call("emoasr_attn_bwd_fused", dt(q), byref(a), ws.data_ptr(), ws.numel(), _stream())
        return
    a = _attn_args(q, k, v, H, pos, bias_u, bias_v, klens, causal, scale, drop_p, seed)
    assert dq.stride() == q.stride() and dk.stride() == k.stride() and dv.stride() == v.stride()
    assert dout.is_contiguous() and out.is_contiguous()
    delta = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
    a.out, a.ldo, a.lse = out.data_ptr(), D, lse.data_ptr()
    a.dout, a.delta = dout.data_ptr(), delta.data_ptr()
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.dpos = None if dpos is None else dpos.data_ptr()
    a.dbias_u = None if dbias_u is None else dbias_u.data_ptr()
    a.dbias_v = None if dbias_v is None else dbias_v.data_ptr()
    if materialise:
        rel = pos is not None
        if scratch is None:
            scratch = AttnScratch(B, H, Tq, k.shape[1], q.dtype, q.device, rel)
        assert scratch.key == (B, H, Tq, k.shape[1], q.dtype, rel), "AttnScratch built for another shape"
        a.pdT, a.dsT, a.ldpd = scratch.pdT.data_ptr(), scratch.dsT.data_ptr(), scratch.ldpd
        if rel:
            a.dbd, a.ldbd, a.cs = scratch.dbd.data_ptr(), scratch.ldbd, scratch.cs.data_ptr()
            if bias_u is not None and bias_v is not None and q.shape[2] == H * 64:
                a.qu, a.qv = scratch.qu.data_ptr(), scratch.qv.data_ptr()
        a.dbias_part = scratch.dbias_part.data_ptr()
        if st is not None:  # scores stored by attn_fwd(store_scores=True): no recomputation
            a.st, a.ldst = st.data_ptr(), st.shape[-1]
    lib.call("emoasr_attn_bwd", dt(q), byref(a), _stream())


# ---- conv module -----------------------------------------------------------------------
def glu_fwd(x):
    M, C2, ld = _rows(_chk(x))
    out = torch.empty(M, C2 // 2, device=x.device, dtype=x.dtype)
    lib.call("emoasr_glu_fwd", dt(x), M, C2 // 2, _p(x), _p(out), _stream())
    return out


def glu_fwd_masked(x, B, T, lens):
    """glu_fwd of x [B*T, 2C] with zeros at the frames t >= lens[b] (lens int32 [B] on the device) -> [B*T, C]"""
    M, C2, ld = _rows(_chk(x))
    assert M == B * T and ld == C2 and _chk(lens, torch.int32).numel() == B and lens.is_contiguous()
    out = torch.empty(M, C2 // 2, device=x.device, dtype=x.dtype)
    lib.call("emoasr_glu_fwd_masked", dt(x), B, T, C2 // 2, _p(x), _p(lens), _p(out), _stream())
    return out


def glu_bwd(x, dout):
    M, C2, ld = _rows(_chk(x))
    din = torch.empty_like(x)
    lib.call("emoasr_glu_bwd", dt(x), M, C2 // 2, _p(x), _p(dout), _p(din), _stream())
    return din


def dwconv_fwd(x, w, bias):
    B, T, C = x.shape
    y = torch.empty_like(x)
    lib.call("emoasr_dwconv_fwd", dt(x), B, T, C, w.shape[-1], _p(_chk(x)), _p(w), _p(bias), _p(y), _stream())
    return y


def dwconv_bn_stats_fwd(x, w, bias, running_mean=None, running_var=None, momentum=0.1, num_batches_tracked=None):
    """depthwise conv + training-mode BatchNorm statistics of its output in two launches:
    -> (y, batch mean [C], biased batch var [C]); running stats / counter updated in place."""
    B, T, C = x.shape
    y = torch.empty_like(x)
    part = torch.empty(lib.size_query("emoasr_dwconv_stats_floats", B, T, C), device=x.device, dtype=torch.float32)
    lib.call("emoasr_dwconv_fwd_stats", dt(x), B, T, C, w.shape[-1], _p(_chk(x)), _p(w), _p(bias), _p(y), _p(part),
             _stream())
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    var = torch.empty(C, device=x.device, dtype=torch.float32)
    if num_batches_tracked is not None:
        _chk(num_batches_tracked, torch.int64)
    lib.call("emoasr_bn_stats_finalize", B, T, C, _p(part), _p(mean), _p(var), _p(running_mean), _p(running_var),
             momentum, _p(num_batches_tracked), _stream())
    return y, mean, var


def glu_dwconv_fwd(g, B, T, w, bias, running_mean=None, running_var=None, momentum=0.1, num_batches_tracked=None,
                   training=True):
    """c = depthwise_conv(GLU(g)) in one launch (bf16; g [B*T, 2C]); training: + the BatchNorm batch statistics of c
    -> (c [B,T,C], mean, var) like dwconv_bn_stats_fwd, else (c, running_mean, running_var)."""
    C = g.shape[-1] // 2
    c = torch.empty(B, T, C, device=g.device, dtype=g.dtype)
    if not training:
        lib.call("emoasr_glu_dwconv_fwd", dt(g), B, T, C, w.shape[-1], _p(_chk(g)), _p(w), _p(bias), _p(c), None, _stream())
        return c, running_mean, running_var
    part = torch.empty(lib.size_query("emoasr_dwconv_stats_floats", B, T, C), device=g.device, dtype=torch.float32)
    lib.call("emoasr_glu_dwconv_fwd", dt(g), B, T, C, w.shape[-1], _p(_chk(g)), _p(w), _p(bias), _p(c), _p(part), _stream())
    mean = torch.empty(C, device=g.device, dtype=torch.float32)
    var = torch.empty(C, device=g.device, dtype=torch.float32)
    if num_batches_tracked is not None:
        _chk(num_batches_tracked, torch.int64)
    lib.call("emoasr_bn_stats_finalize", B, T, C, _p(part), _p(mean), _p(var), _p(running_mean), _p(running_var),
             momentum, _p(num_batches_tracked), _stream())
    return c, mean, var


def conv_bwd_fused(ds, c, mean, var, gamma, beta, eps, dgamma, dbeta, g, w, dw, dbias, B, T):
    """backward of GLU -> depthwise conv -> BatchNorm(training) -> Swish in three launches (bf16): BatchNorm sums + fold,
    then apply / depthwise data gradient / GLU backward / depthwise weight-gradient partials fused, then their fold.
    ds: gradient w.r.t. the Swish output [B*T, C]; c: the convolution's output; g: the GLU input [B*T, 2C] -> dg."""
    import ctypes
    M, C, _ = _rows(_chk(c))
    K = w.shape[-1]
    scr = torch.empty(lib.size_query("emoasr_bn_swish_bwd_scratch_floats", M, C), device=c.device, dtype=torch.float32)
    tot = ctypes.c_void_p()
    lib.call("emoasr_bn_swish_bwd_sums", dt(c), M, C, _p(_chk(ds, c.dtype)), _p(c), _p(mean), _p(var), _p(gamma), _p(beta),
             eps, _p(dgamma), _p(dbeta), _p(scr), ctypes.byref(tot), _stream())
    dg = torch.empty_like(g)
    wscr = torch.empty(lib.size_query("emoasr_dwconv_bwd_w_scratch_floats", B, T, C, K), device=c.device, dtype=torch.float32)
    lib.call("emoasr_conv_bwd_fused", dt(c), B, T, C, K, _p(ds), _p(c), _p(mean), _p(var), _p(gamma), _p(beta), eps, tot,
             _p(_chk(g, c.dtype)), _p(w), _p(dg), _p(dw), _p(dbias), _p(wscr), _stream())
    return dg


def dwconv_bwd_x(dy, w):
    B, T, C = dy.shape
    dx = torch.empty_like(dy)
    lib.call("emoasr_dwconv_bwd_x", dt(dy), B, T, C, w.shape[-1], _p(dy), _p(w), _p(dx), _stream())
    return dx


def dwconv_bwd_w(dy, x, dw, dbias, accumulate=False):
    B, T, C = dy.shape
    K = dw.shape[-1]
    scratch = torch.empty(lib.size_query("emoasr_dwconv_bwd_w_scratch_floats", B, T, C, K), device=dy.device,
                          dtype=torch.float32)
    lib.call("emoasr_dwconv_bwd_w", dt(dy), B, T, C, K, _p(dy), _p(x), _p(dw), _p(dbias),
             int(accumulate), _p(scratch), _stream())


def bn_stats(y, running_mean=None, running_var=None, momentum=0.1):
    M, C, ld = _rows(_chk(y))
    mean = torch.empty(C, device=y.device, dtype=torch.float32)
    var = torch.empty(C, device=y.device, dtype=torch.float32)
    lib.call("emoasr_bn_stats", dt(y), M, C, _p(y), _p(mean), _p(var), _p(running_mean), _p(running_var),
             momentum, _stream())
    return mean, var


def bn_swish_fwd(y, mean, var, gamma, beta, eps):
    M, C, ld = _rows(_chk(y))
    z = torch.empty_like(y)
    lib.call("emoasr_bn_swish_fwd", dt(y), M, C, _p(y), _p(mean), _p(var), _p(gamma), _p(beta), eps, _p(z),
             _stream())
    return z


def bn_swish_bwd(dz, y, mean, var, gamma, beta, eps, dgamma, dbeta):
    M, C, ld = _rows(_chk(y))
    dy = torch.empty_like(y)
    scratch = torch.empty(lib.size_query("emoasr_bn_swish_bwd_scratch_floats", M, C), device=y.device, dtype=torch.float32)
    lib.call("emoasr_bn_swish_bwd", dt(y), M, C, _p(dz), _p(y), _p(mean), _p(var), _p(gamma), _p(beta), eps,
             _p(dy), _p(dgamma), _p(dbeta), _p(scratch), _stream())
    return dy


# ---- element-wise ----------------------------------------------------------------------
def strided_copy(src, out=None, out_dtype=None, accumulate=False):
    """out (contiguous, src.shape) (+)= src (any strides, <= 4 dims); casts f32 <-> bf16."""
    assert src.dim() <= 4
    shape = [1] * (4 - src.dim()) + list(src.shape)
    strides = [0] * (4 - src.dim()) + list(src.stride())
    if out is None:
        out = torch.empty(src.shape, device=src.device, dtype=out_dtype or src.dtype)
    assert out.is_contiguous()
    lib.call("emoasr_strided_copy", dt(src), dt(out), _p(src), _p(out), *shape, *strides, int(accumulate),
             _stream())
    return out


def transpose_cast_batched(pairs):
    """pairs: [(src f32 [rows, cols] contiguous, dst [cols, rows] compute dtype, last dim contiguous)] -> every dst = src^T, one
    launch per lib.TC_MAX pairs (the transposed weight copies of the layer runtime, refreshed with the parameter shadow)"""
    for i0 in range(0, len(pairs), lib.TC_MAX):
        chunk = pairs[i0:i0 + lib.TC_MAX]
        arr = (lib.TcItem * len(chunk))()
        for q, (src, dst) in zip(arr, chunk):
            rows, cols = src.shape
            assert src.is_contiguous() and src.dtype == torch.float32 and tuple(dst.shape) == (cols, rows) and dst.stride(1) == 1
            assert dst.dtype == chunk[0][1].dtype
            q.src, q.dst, q.rows, q.cols, q.ld_dst = src.data_ptr(), dst.data_ptr(), rows, cols, dst.stride(0)
        lib.call("emoasr_transpose_cast_batched", dt(chunk[0][1]), len(chunk), arr, _stream())


def scale_dropout(x, scale=1.0, drop_p=0.0, seed=0, out=None):
    """out: where to write (contiguous, x's shape and dtype; x itself: in place)"""
    assert out is None or (out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype)
    y = torch.empty_like(x) if out is None else out
    lib.call("emoasr_scale_dropout", dt(x), x.numel(), _p(_chk(x)), _p(y), scale, drop_p, seed, _stream())
    return y


def posenc(x, pe, scale, drop_p=0.0, seed=0):
    B, T, N = x.shape
    y = torch.empty_like(x)
    lib.call("emoasr_posenc", dt(x), B, T, N, _p(_chk(x)), _p(pe), scale, drop_p, seed, _p(y), _stream())
    return y


def act_bwd(dy, pre, act):
    """dy * act'(pre), elementwise (same shape and dtype)"""
    assert dy.shape == pre.shape and dy.dtype == pre.dtype and dy.is_contiguous() and pre.is_contiguous()
    dx = torch.empty_like(dy)
    lib.call("emoasr_act_bwd", dt(dy), dy.numel(), act, _p(_chk(dy)), _p(pre), _p(dx), _stream())
    return dx


def add(a, b):
    y = torch.empty_like(a)
    lib.call("emoasr_add", dt(a), a.numel(), _p(a), _p(b), _p(y), _stream())
    return y


# ---- CTC -------------------------------------------------------------------------------
def gemm_nt_lse(a, b, bias):
    """logits = a @ b^T + bias and their row log-sum-exp in ONE pass over the logits (the CTC head: emoasr_gemm_nt_lse) when the
    large-tile kernel takes the shape (bf16, N % 8 == 0, K % 64 == 0, operands below 4 GiB); else the product + a row pass"""
    M, K, lda = _rows(_chk(a))
    N, Kb, ldb = _rows(_chk(b, a.dtype))
    assert K == Kb
    if (a.dtype == torch.bfloat16 and N % 8 == 0 and N >= 256 and K % 64 == 0 and lda % 8 == 0 and ldb % 8 == 0
            and M * lda * 2 < (1 << 32) and N * ldb * 2 < (1 << 32) and M >= 2048):
        # rows padded to a multiple of 64 columns (V = 10 000: 20 000-byte rows put every 128-byte store of a tile astride two lines)
        Np = (N + 63) // 64 * 64
        out = torch.empty(M, Np, device=a.device, dtype=a.dtype)[:, :N]
        part = torch.empty((N + 63) // 64, M, 2, device=a.device, dtype=torch.float32)
        lse = torch.empty(M, device=a.device, dtype=torch.float32)
        lib.call("emoasr_gemm_nt_lse", dt(a), M, N, K, _p(a), lda, _p(b), ldb, _p(out), Np, _p(bias), _p(part), _p(lse), _stream())
        return out, lse
    out = gemm_nt(a, b, bias=bias)
    return out, row_lse(out)


def row_lse(logits):
    M, V, ld = _rows(_chk(logits))
    lse = torch.empty(M, device=logits.device, dtype=torch.float32)
    lib.call("emoasr_row_lse", dt(logits), M, V, _p(logits), ld, _p(lse), _stream())
    return lse


def ctc_forward(logits, lse, labels, elens, ylens, blank):
    """logits [B,T,V]; labels int32 [B,Lmax]; elens/ylens int32 [B] -> (lp, alpha, beta, nll)"""
    B, T, V = logits.shape
    Lmax = labels.shape[1]
    S = 2 * Lmax + 1
    dev = logits.device
    lp = torch.empty(B, T, S, device=dev, dtype=torch.float32)
    alpha = torch.empty(B, T, S, device=dev, dtype=torch.float32)
    beta = torch.empty(B, T, S, device=dev, dtype=torch.float32)
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    lib.call("emoasr_ctc_forward", dt(logits), B, T, V, Lmax, _p(logits), logits.stride(1), _p(lse), _p(labels),
             _p(elens), _p(ylens), blank, _p(lp), _p(alpha), _p(beta), _p(nll), _stream())
    return lp, alpha, beta, nll


def ctc_grad(logits, lse, labels, elens, ylens, blank, lp, alpha, beta, nll, gscale, gscale_dev=None, out=None):
    B, T, V = logits.shape
    ld = logits.stride(1)  # rows of a ragged vocabulary are padded (engine.head_logits): keep that layout
    if out is not None:
        assert out.shape == logits.shape and out.dtype == logits.dtype and out.stride(2) == 1
        grad = out
    else:
        grad = torch.empty_like(logits) if ld == V else torch.empty(B, T, ld, device=logits.device, dtype=logits.dtype)[..., :V]
    lib.call("emoasr_ctc_grad", dt(logits), B, T, V, labels.shape[1], _p(logits), logits.stride(1), _p(lse),
             _p(labels), _p(elens), _p(ylens), blank, _p(lp), _p(alpha), _p(beta), _p(nll), gscale, _p(gscale_dev),
             _p(grad),
             grad.stride(1), _stream())
    return grad


def ctc_forward_rows(logits2, lse, labels, elens, ylens, blank, row0, Tmax):
    """CTC lattices of utterances whose logits rows are row0[b] + t in the stacked [M, V] `logits2` (several micro-batches in
    one set of launches); the lattice tables are [B, Tmax, S].  -> (lp, alpha, beta, nll)"""
    M, V = logits2.shape
    B, Lmax = labels.shape
    S = 2 * Lmax + 1
    dev = logits2.device
    lp = torch.empty(B, Tmax, S, device=dev, dtype=torch.float32)
    alpha = torch.empty(B, Tmax, S, device=dev, dtype=torch.float32)
    beta = torch.empty(B, Tmax, S, device=dev, dtype=torch.float32)
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    assert row0.dtype == torch.int64
    lib.call("emoasr_ctc_forward_rows", dt(logits2), B, Tmax, V, Lmax, _p(logits2), logits2.stride(0), _p(lse), _p(labels),
             _p(elens), _p(ylens), blank, _p(row0), _p(lp), _p(alpha), _p(beta), _p(nll), _stream())
    return lp, alpha, beta, nll


def ctc_grad_rows(logits2, lse, labels, elens, ylens, blank, lp, alpha, beta, nll, gscale, row0, tpad, uscale, out):
    """gradient rows of ctc_forward_rows' utterances written into `out` [M, V] (every row of every utterance, zeros on padding)"""
    M, V = logits2.shape
    B, Tmax, _ = lp.shape
    assert out.shape == logits2.shape and out.dtype == logits2.dtype and tpad.dtype == torch.int32 and uscale.dtype == torch.float32
    lib.call("emoasr_ctc_grad_rows", dt(logits2), B, Tmax, V, labels.shape[1], _p(logits2), logits2.stride(0), _p(lse), _p(labels),
             _p(elens), _p(ylens), blank, _p(lp), _p(alpha), _p(beta), _p(nll), gscale, None, _p(row0), _p(tpad), _p(uscale),
             _p(out), out.stride(0), _stream())
    return out


def ctc_greedy(logits, elens, blank):
    B, T, V = logits.shape
    dev = logits.device
    # one buffer, three views: the caller reads all of them back with ONE device-to-host copy (ctc_greedy_apply)
    buf = torch.empty(2 * B * T + B, device=dev, dtype=torch.int32)
    best, hyp, hyplen = buf[:B * T].view(B, T), buf[B * T:2 * B * T].view(B, T), buf[2 * B * T:]
    lib.call("emoasr_ctc_greedy", dt(logits), B, T, V, _p(logits), logits.stride(1), _p(elens), blank, _p(best),
             _p(hyp), _p(hyplen), _stream())
    return best, hyp, hyplen


# ---- Transformer decoder side ------------------------------------------------------------
def embed_fwd(ids, table, pe, scale, drop_p=0.0, seed=0):
    """ids int32 [B,L]; table [V,d] (compute dtype); pe f32 [>=L,d] or None -> [B,L,d]"""
    B, L = ids.shape
    d = table.shape[1]
    out = torch.empty(B, L, d, device=table.device, dtype=table.dtype)
    lib.call("emoasr_embed_fwd", dt(table), B * L, L, d, _p(ids), _p(table), _p(pe), scale, drop_p, seed, _p(out),
             _stream())
    return out


def embed_bwd(ids, dout, scale, dtable, drop_p=0.0, seed=0):
    B, L = ids.shape
    lib.call("emoasr_embed_bwd", dt(dout), B * L, dout.shape[-1], _p(ids), _p(dout), scale, drop_p, seed,
             _p(_chk(dtable, torch.float32)), _stream())


def lsm_loss(logits, labels, w, lsm_prob, want_grad=False, gscale=1.0, gscale_dev=None, grad=None):
    """logits [M,V]; labels int32 [M]; w f32 [M] row weights (0 = padded) -> (loss_rows f32 [M], grad | None).
    grad: a [M,V] buffer of the logits' dtype to write the gradient into (rows may be padded: last dim contiguous)"""
    M, V, ld = _rows(_chk(logits))
    loss = torch.empty(M, device=logits.device, dtype=torch.float32)
    if grad is not None:
        assert want_grad and _chk(grad, logits.dtype).shape == logits.shape and grad.stride(1) == 1
    else:
        grad = torch.empty_like(logits) if want_grad else None
    lib.call("emoasr_lsm_loss", dt(logits), M, V, _p(logits), ld, _p(labels), _p(w), lsm_prob, _p(loss), gscale,
             _p(gscale_dev), _p(grad), 0 if grad is None else grad.stride(0), _stream())
    return loss, grad


# ---- masked LM -----------------------------------------------------------------------------
def mlm_expand(ys, ylens, row0, r_begin, r_count, Np, mask_id, pad_id=0, total=None, out=None):
    """the masked copies r_begin .. r_begin + r_count - 1 of ys int32 [B,N] (lengths ylens int32 [B], row0 int32 [B+1] their prefix
    sums, all on the device; `total` = sum(ylens) where the caller knows it on the host)
    -> (ids int32 [r_count,Np], klens [r_count], idx [r_count] = flat row of each copy's masked position, labels [r_count]).
    out: that tuple of int32 buffers to write into (at least r_count rows each; the rest is left alone)"""
    B, N = _chk(ys, torch.int32).shape
    assert ys.is_contiguous() and ylens.numel() == B and row0.numel() == B + 1
    _chk(ylens, torch.int32), _chk(row0, torch.int32)
    assert r_begin >= 0 and r_count >= 1 and (total is None or r_begin + r_count <= total), (r_begin, r_count, total)
    if out is None:
        dev = ys.device
        out = (torch.empty(r_count, Np, device=dev, dtype=torch.int32),) + tuple(
            torch.empty(r_count, device=dev, dtype=torch.int32) for _ in range(3))
    ids, klens, idx, labels = out
    for t in out:
        assert _chk(t, torch.int32).is_contiguous() and t.shape[0] >= r_count
    assert ids.shape[1] == Np
    lib.call("emoasr_mlm_expand", B, N, Np, _p(ys), _p(ylens), _p(row0), r_begin, r_count, mask_id, pad_id, _p(ids), _p(klens),
             _p(idx), _p(labels), _stream())
    return ids[:r_count], klens[:r_count], idx[:r_count], labels[:r_count]


# ---- ELECTRA ---------------------------------------------------------------------------------
def sample_rows(logits, labels, w, seed, row0=0, want_lse=False):
    """logits [M,V] (f32 / bf16, last dim contiguous); labels int32 [M]; w f32 [M] -> (loss rows f32 [M] = -w * log p(label),
    samples int32 [M] ~ softmax(logits[m]), lse f32 [M] | None).  sample[m] = argmax_v (logits[m,v].float() + gumbel_noise(...)[m,v])
    with ties to the lowest column: a function of (seed, row0 + m, v) only, so chunks of rows (row0) draw what one call draws."""
    M, V, ld = _rows(_chk(logits))
    assert logits.dim() == 2 and V >= 2 and labels.numel() == M and w.numel() == M and row0 >= 0
    _chk(labels, torch.int32), _chk(w, torch.float32)
    loss = torch.empty(M, device=logits.device, dtype=torch.float32)
    sample = torch.empty(M, device=logits.device, dtype=torch.int32)
    lse = torch.empty(M, device=logits.device, dtype=torch.float32) if want_lse else None
    lib.call("emoasr_sample_rows", _DT[logits.dtype], M, V, _p(logits), ld, _p(labels), _p(w), int(seed) & (2 ** 64 - 1), int(row0),
             _p(loss), _p(lse), _p(sample), _stream())
    return loss, sample, lse


def gumbel_noise(M, V, seed, row0=0, device="cuda"):
    """the Gumbel(0, 1) variates sample_rows adds to an [M, V] block of logits -> f32 [M, V]"""
    out = torch.empty(M, V, device=device, dtype=torch.float32)
    lib.call("emoasr_gumbel_noise", M, V, int(seed) & (2 ** 64 - 1), int(row0), _p(out), V, _stream())
    return out


def electra_corrupt(ids, sel, labels, samples, out=None):
    """ids int32 [B*N] (any shape, contiguous); sel / labels / samples int32 [M]: the flat masked rows, the tokens the masks hide and
    the generator's samples -> (generated int32 like ids, replaced f32 0/1 like ids, counters int32 [2] = (replaced, masked)).
    out: that tuple of buffers to write into (only their first B*N / 2 entries are written)"""
    BN, M = ids.numel(), sel.numel()
    assert _chk(ids, torch.int32).is_contiguous() and labels.numel() == M and samples.numel() == M and M <= BN
    for t in (sel, labels, samples):
        assert _chk(t, torch.int32).is_contiguous()
    if out is None:
        out = (torch.empty_like(ids), torch.empty(ids.shape, device=ids.device, dtype=torch.float32),
               torch.empty(2, device=ids.device, dtype=torch.int32))
    generated, replaced, counters = out
    assert _chk(generated, torch.int32).is_contiguous() and _chk(replaced, torch.float32).is_contiguous()
    assert generated.numel() >= BN and replaced.numel() >= BN and _chk(counters, torch.int32).numel() >= 2
    lib.call("emoasr_electra_corrupt", BN, M, _p(ids), _p(sel), _p(labels), _p(samples), _p(generated), _p(replaced), _p(counters),
             _stream())
    return generated, replaced, counters


def bce_head_fwd(h, wp, bp, y=None, w=None, want_sigmoid=False):
    """h [M,H]; wp [H] or [1,H] (h's dtype); bp f32 [1]; y, w f32 [M] (both or neither)
    -> (z f32 [M] = h . wp + bp, loss rows f32 [M] = w * BCEWithLogits(z, y) | None, sigmoid(z) f32 [M] | None)"""
    M, H, ldh = _rows(_chk(h))
    assert h.dim() == 2 and _chk(wp, h.dtype).numel() == H and wp.is_contiguous() and _chk(bp, torch.float32).numel() == 1
    assert (y is None) == (w is None)
    z = torch.empty(M, device=h.device, dtype=torch.float32)
    loss = sig = None
    if y is not None:
        assert _chk(y, torch.float32).numel() == M and _chk(w, torch.float32).numel() == M and y.is_contiguous() and w.is_contiguous()
        loss = torch.empty(M, device=h.device, dtype=torch.float32)
    if want_sigmoid:
        sig = torch.empty(M, device=h.device, dtype=torch.float32)
    lib.call("emoasr_bce_head_fwd", _DT[h.dtype], M, H, _p(h), ldh, _p(wp), _p(bp), _p(y), _p(w), _p(z), _p(loss), _p(sig), _stream())
    return z, loss, sig


def bce_head_bwd(h, wp, z, y, w, dwp, dbp, gscale=1.0, gscale_dev=None):
    """-> dh [M,H] = dz wp with dz = w * (sigmoid(z) - y) * gscale * [gscale_dev]; dwp f32 [H] += sum_m dz h, dbp f32 [1] += sum_m dz"""
    M, H, ldh = _rows(_chk(h))
    assert _chk(wp, h.dtype).numel() == H and _chk(dwp, torch.float32).numel() == H and _chk(dbp, torch.float32).numel() == 1
    assert dwp.is_contiguous() and wp.is_contiguous()
    for t in (z, y, w):
        assert _chk(t, torch.float32).numel() == M and t.is_contiguous()
    dh = torch.empty(M, H, device=h.device, dtype=h.dtype)
    lib.call("emoasr_bce_head_bwd", _DT[h.dtype], M, H, _p(h), ldh, _p(wp), _p(z), _p(y), _p(w), gscale, _p(gscale_dev), _p(dh), H,
             _p(dwp), _p(dbp), _stream())
    return dh


# ---- CTC error correction ----------------------------------------------------------------------
def ctc_token_conf(logits, lse, best, elens, blank):
    """logits [B,T,V] (f32 / bf16, last dim contiguous, utterance stride T * row stride); lse f32 [B*T]; best int32 [B,T] the greedy
    frame ids; elens int32 [B] -> (frame int32 [B,T], conf f32 [B,T], ntok int32 [B]): for token j of the collapsed path, the frame
    of its run where softmax(logits)[id] is largest (earliest on ties) and that probability.  Entries from ntok[b] on are unset."""
    B, T, V = _chk(logits).shape
    assert logits.dtype in _DT and logits.stride(2) == 1 and (B == 1 or logits.stride(0) == T * logits.stride(1))
    assert _chk(lse, torch.float32).numel() == B * T and lse.is_contiguous()
    assert _chk(best, torch.int32).shape == (B, T) and best.is_contiguous() and _chk(elens, torch.int32).numel() == B
    dev = logits.device
    frame = torch.empty(B, T, device=dev, dtype=torch.int32)
    conf = torch.empty(B, T, device=dev, dtype=torch.float32)
    ntok = torch.empty(B, device=dev, dtype=torch.int32)
    lib.call("emoasr_ctc_token_conf", _DT[logits.dtype], B, T, V, _p(logits), logits.stride(1), _p(lse), _p(best), _p(elens),
             int(blank), _p(frame), _p(conf), _p(ntok), _stream())
    return frame, conf, ntok


def correct_fuse(asr_logits, asr_lse, lm_logits, w, n_cols, asr_rows=None):
    """asr_logits [R,V_asr] with asr_lse f32 [R]; lm_logits [n,V_lm] (f32 / bf16 each, last dim contiguous); asr_rows int32 [n]: the
    recogniser row of each LM row (None: row i) -> (ids int32 [n], values f32 [n]) = arg-max and maximum over v < n_cols of
    (1 - w) softmax(asr row)[v] + w softmax(lm row)[v], the lowest column on ties.  The LM's log-sum-exp is formed in the kernel."""
    R, Va, lda = _rows(_chk(asr_logits))
    n, Vl, ldl = _rows(_chk(lm_logits))
    assert asr_logits.dim() == 2 and lm_logits.dim() == 2 and asr_logits.dtype in _DT and lm_logits.dtype in _DT
    assert _chk(asr_lse, torch.float32).numel() == R and asr_lse.is_contiguous()
    if asr_rows is not None:
        assert _chk(asr_rows, torch.int32).numel() == n and asr_rows.is_contiguous()
    else:
        assert R >= n
    ids = torch.empty(n, device=lm_logits.device, dtype=torch.int32)
    val = torch.empty(n, device=lm_logits.device, dtype=torch.float32)
    lib.call("emoasr_correct_fuse", _DT[asr_logits.dtype], _DT[lm_logits.dtype], n, Va, Vl, int(n_cols), _p(asr_logits), lda,
             _p(asr_lse), _p(asr_rows), R, _p(lm_logits), ldl, float(w), _p(ids), _p(val), _stream())
    return ids, val


CORRECT_MAX_WEIGHTS = 16     # EMO_CORRECT_MAX_WEIGHTS: weights per emoasr_correct_fuse_grid launch


def correct_mask_grid(hyp, ntok, conf, frame, ths, mask_id, pad_id=0):
    """hyp int32 [B,T] the collapsed greedy ids; ntok int32 [B], conf f32 [B,T], frame int32 [B,T] as ctc_token_conf leaves them; ths
    f32 [NT] (device) -> (ys int32 [NT,B,T], num_masked int32 [NT,B], lm_rows int32 [NT*B*T], asr_rows int32 [NT*B*T]): ys[k,b,j] =
    mask_id where conf[b,j] < ths[k] (strictly), hyp[b,j] otherwise, pad_id from ntok[b] on.  The first num_masked.sum() entries of
    the two lists are the masked positions in (threshold, utterance, token) order: lm_rows = (k * B + b) * T + j, the row of
    ys.view(-1), and asr_rows = b * T + frame[b,j], the recogniser's row; the rest is unset.  The order comes from a scan over the
    counts, so it is a fixed function of the inputs."""
    B, T = _chk(hyp, torch.int32).shape
    NT = _chk(ths, torch.float32).numel()
    assert hyp.is_contiguous() and ths.is_contiguous() and _chk(ntok, torch.int32).numel() == B and ntok.is_contiguous()
    assert _chk(conf, torch.float32).shape == (B, T) and conf.is_contiguous()
    assert _chk(frame, torch.int32).shape == (B, T) and frame.is_contiguous()
    assert T >= 1 and NT * B * T < 2 ** 31
    dev = hyp.device
    ys = torch.empty(NT, B, T, device=dev, dtype=torch.int32)
    num_masked = torch.empty(NT, B, device=dev, dtype=torch.int32)
    lm_rows = torch.empty(NT * B * T, device=dev, dtype=torch.int32)
    asr_rows = torch.empty(NT * B * T, device=dev, dtype=torch.int32)
    lib.call("emoasr_correct_mask_grid", B, T, NT, _p(hyp), _p(ntok), _p(conf), _p(frame), _p(ths), int(mask_id), int(pad_id),
             _p(ys), _p(num_masked), _p(lm_rows), _p(asr_rows), _stream())
    return ys, num_masked, lm_rows, asr_rows


def correct_fuse_grid(asr_logits, asr_lse, lm_logits, weights, n_cols, asr_rows=None):
    """correct_fuse for every weight of `weights` (host floats in [0, 1]) in one read of the two rows -> (ids int32 [NW,n], values f32
    [NW,n]); row k is correct_fuse(..., weights[k], ...) bit for bit.  One launch per CORRECT_MAX_WEIGHTS weights."""
    R, Va, lda = _rows(_chk(asr_logits))
    n, Vl, ldl = _rows(_chk(lm_logits))
    assert asr_logits.dim() == 2 and lm_logits.dim() == 2 and asr_logits.dtype in _DT and lm_logits.dtype in _DT
    assert _chk(asr_lse, torch.float32).numel() == R and asr_lse.is_contiguous()
    if asr_rows is not None:
        assert _chk(asr_rows, torch.int32).numel() == n and asr_rows.is_contiguous()
    else:
        assert R >= n
    w = torch.as_tensor([float(v) for v in weights], dtype=torch.float32)
    NW = w.numel()
    ids = torch.empty(NW, n, device=lm_logits.device, dtype=torch.int32)
    val = torch.empty(NW, n, device=lm_logits.device, dtype=torch.float32)
    for k0 in range(0, NW, CORRECT_MAX_WEIGHTS):
        k1 = min(k0 + CORRECT_MAX_WEIGHTS, NW)
        lib.call("emoasr_correct_fuse_grid", _DT[asr_logits.dtype], _DT[lm_logits.dtype], n, Va, Vl, int(n_cols), _p(asr_logits),
                 lda, _p(asr_lse), _p(asr_rows), R, _p(lm_logits), ldl, _p(w[k0:k1]), k1 - k0, _p(ids[k0:k1]), _p(val[k0:k1]),
                 _stream())
    return ids, val


# ---- N-best rescoring and error-label alignment -------------------------------------------------
ALIGN_MODES = {None: 0, "SI": 1, "SID": 2}
EDIT_MAX_LEN = 4096


def edit_align(hyps, refs, ref_idx=None, device="cuda", want_ops=False, label_mode=None):
    """hyps: P int sequences; refs: int sequences; ref_idx [P]: the reference of each hypothesis (None: refs[p]) -> dict of host
    arrays: counts int32 [P,4] = (n_sub, n_ins, n_del, dist), exactly metrics.compute_wer's; with want_ops `ops`, a list of P
    strings over C / S / I / D; with label_mode "SI" / "SID" `labels`, a list of P strings, one letter per hypothesis token
    (align_hyps' fold).  One upload, one emoasr_edit_align call over all pairs, one download.  An empty hypothesis is one token
    that matches nothing.  A side of more than EDIT_MAX_LEN tokens raises; so does a pair with an empty reference (compute_wer
    divides by its length; the kernel would count the hypothesis' tokens as insertions)."""
    import numpy as np
    P = len(hyps)
    ref_idx = np.arange(P, dtype=np.int32) if ref_idx is None else np.asarray(ref_idx, dtype=np.int32)
    assert ref_idx.shape == (P,) and (P == 0 or (ref_idx.min() >= 0 and ref_idx.max() < len(refs)))
    mode = ALIGN_MODES[label_mode]
    if P == 0:
        return {"counts": np.zeros((0, 4), np.int32), "ops": [], "labels": []}
    hlen = np.fromiter((len(h) for h in hyps), np.int64, P)
    rlen = np.fromiter((len(r) for r in refs), np.int64, len(refs))
    assert hlen.sum() < 2 ** 31 and rlen.sum() < 2 ** 31
    hyp_off = np.concatenate([[0], np.cumsum(hlen)])
    ref_off = np.concatenate([[0], np.cumsum(rlen)])
    heff, rp = np.maximum(hlen, 1), rlen[ref_idx]
    ops_off = np.concatenate([[0], np.cumsum(heff + rp)])
    max_h, max_r = int(hlen.max()), int(rp.max())
    if int(rp.min()) == 0:
        raise ValueError(f"edit_align: pair {int(np.argmin(rp))} has an empty reference")
    ws_need = np.zeros(P, np.int64)
    if max_h <= EDIT_MAX_LEN and max_r <= EDIT_MAX_LEN:       # (over the limit: the call below returns the error)
        words = 2 * ((heff + 63) // 64) * (rp + 63)             # emoasr_edit_align_ws_words, vectorised; checked against it below
        ws_need = np.where(words > lib.size_query("emoasr_edit_align_lds_words"), words, 0)
        k = int(np.argmax(words))
        assert int(ws_need[k]) == lib.size_query("emoasr_edit_align_ws_words", int(rp[k]), int(hlen[k]))
    ws_off = np.concatenate([[0], np.cumsum(ws_need)])

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)

    flat = lambda seqs, n: np.fromiter((t for s in seqs for t in s), np.int32, n)
    d_hyp, d_ref = up(flat(hyps, int(hyp_off[-1])), np.int32), up(flat(refs, int(ref_off[-1])), np.int32)
    d_hoff, d_roff, d_ridx = up(hyp_off, np.int32), up(ref_off, np.int32), up(ref_idx, np.int32)
    d_ooff, d_woff = up(ops_off[:-1], np.int64), up(ws_off, np.int64)
    counts = torch.empty(P, 4, device=device, dtype=torch.int32)
    status = torch.zeros(1, device=device, dtype=torch.int32)
    d_ops = torch.empty(int(ops_off[-1]), device=device, dtype=torch.uint8) if want_ops else None
    d_lab = torch.empty(max(int(hyp_off[-1]), 1), device=device, dtype=torch.uint8) if mode else None
    d_ws = torch.empty(int(ws_off[-1]), device=device, dtype=torch.int64) if ws_off[-1] else None
    with torch.cuda.device(counts.device):
        lib.call("emoasr_edit_align", P, len(refs), max_h, max_r, _p(d_hyp), _p(d_hoff), _p(d_ref), _p(d_roff), _p(d_ridx), mode,
                 _p(counts), _p(d_ops), _p(d_ooff), _p(d_lab), _p(d_ws), _p(d_woff), _p(status), _stream())
    out = {"counts": counts.cpu().numpy()}
    if int(status.item()):
        raise lib.EmoasrHipError("emoasr_edit_align: a pair broke its declared bounds (status %d)" % int(status.item()))
    if want_ops:
        raw = d_ops.cpu().numpy().tobytes()
        n_ops = heff + out["counts"][:, 2]
        out["ops"] = [raw[int(o):int(o + n)].decode("ascii") for o, n in zip(ops_off[:-1], n_ops)]
    if mode:
        raw = d_lab.cpu().numpy().tobytes()
        out["labels"] = [raw[int(a):int(b)].decode("ascii") for a, b in zip(hyp_off[:-1], hyp_off[1:])]
    return out


def rescore_grid(score_asr, score_lm, ylen, utt_off, counts, lm_w, len_w):
    """score_asr / score_lm f64 [N], ylen int32 [N], utt_off int32 [U+1] (an utterance's rows are contiguous), counts int32 [N,4],
    lm_w f64 [G1], len_w f64 [G2], all on the device -> (best int32 [G1*G2, U], totals int64 [G1*G2, 3]): per grid cell the first
    row of each utterance with the largest (score_asr + lm_w * score_lm) + len_w * ylen (f64, each operation rounded once), and
    the (n_sub, n_ins, n_del) of the winners summed."""
    N, U, G1, G2 = score_asr.numel(), utt_off.numel() - 1, lm_w.numel(), len_w.numel()
    for t in (score_asr, score_lm, lm_w, len_w):
        assert _chk(t, torch.float64).is_contiguous() and t.dim() == 1
    assert score_lm.numel() == N and _chk(ylen, torch.int32).numel() == N and ylen.is_contiguous()
    assert _chk(utt_off, torch.int32).is_contiguous() and _chk(counts, torch.int32).shape == (N, 4) and counts.is_contiguous()
    # (one synchronisation: the kernel trusts the offsets)
    if not bool((utt_off[0] == 0) & (utt_off[-1] == N) & (utt_off[1:] >= utt_off[:-1]).all()):
        raise ValueError(f"rescore_grid: utt_off must rise from 0 to the {N} rows")
    best = torch.empty(G1 * G2, U, device=score_asr.device, dtype=torch.int32)
    totals = torch.empty(G1 * G2, 3, device=score_asr.device, dtype=torch.int64)
    with torch.cuda.device(score_asr.device):
        lib.call("emoasr_rescore_grid", N, U, G1, G2, _p(score_asr), _p(score_lm), _p(ylen), _p(utt_off), _p(counts), _p(lm_w),
                 _p(len_w), _p(best), _p(totals), _stream())
    return best, totals


# ---- knowledge distillation ---------------------------------------------------------------
def soft_ce(logits, soft=None, src=None, hard=None, w_soft=None, w_hard=None, lsm_prob=0.0, lrow=None, want_grad=False,
            gscale=1.0, gscale_dev=None, grad=None):
    """logits [M,V]; soft f32 [N,V]; src/hard/lrow int32 [R]; w_* f32 [R] -> (loss rows f32 [R], grad [M,V] | None).
    With `lrow` only the listed logits rows are touched: pass a zero-filled `grad`."""
    M, V, ld = _rows(_chk(logits))
    R = M if lrow is None else lrow.numel()
    loss = torch.empty(R, device=logits.device, dtype=torch.float32)
    if want_grad and grad is None:
        grad = torch.zeros_like(logits) if lrow is not None else torch.empty_like(logits)
    if soft is not None:
        _chk(soft, torch.float32)
        assert soft.shape[-1] == V and soft.is_contiguous()
    lib.call("emoasr_soft_ce", dt(logits), R, V, _p(logits), ld, _p(lrow), _p(soft), V, _p(src), _p(hard), _p(w_soft),
             _p(w_hard), lsm_prob, _p(loss), gscale, _p(gscale_dev), _p(grad) if want_grad else None,
             grad.stride(-2) if want_grad else 0, _stream())
    return loss, grad if want_grad else None


def ctc_best_path(lp, alpha, beta, labels, elens, ylens, blank):
    """lattices of ctc_forward [B,T,S] -> aligns int32 [B,T] (ctc_aligner.py:139-221)"""
    B, T, S = lp.shape
    aligns = torch.empty(B, T, device=lp.device, dtype=torch.int32)
    lib.call("emoasr_ctc_best_path", B, T, labels.shape[1], _p(lp), _p(alpha), _p(beta), _p(labels), _p(elens),
             _p(ylens), blank, _p(aligns), _stream())
    return aligns


def rnnt_best_path(alpha, beta, elens, ylens):
    """lattices of rnnt_forward f32 [B,T,U] -> aligns int32 [B,U-1] (rnnt_aligner.py:186-196)"""
    B, T, U = alpha.shape
    aligns = torch.zeros(B, max(U - 1, 0), device=alpha.device, dtype=torch.int32)
    lib.call("emoasr_rnnt_best_path", B, T, U, _p(alpha), _p(beta), _p(elens), _p(ylens), _p(aligns), _stream())
    return aligns


LABEL_POSITIONS = {"all": 0, "left": 1, "mid": 2, "right": 3}


def ctc_label_map(aligns, xlens, blank, position="all"):
    """aligns int32 [B,T], xlens int32 [B] -> (label_map int32 [B,T] (-1: none), count int32 [B])"""
    B, T = aligns.shape
    lmap = torch.empty(B, T, device=aligns.device, dtype=torch.int32)
    count = torch.empty(B, device=aligns.device, dtype=torch.int32)
    lib.call("emoasr_ctc_label_map", B, T, _p(aligns), _p(xlens), blank, LABEL_POSITIONS[position], _p(lmap), _p(count),
             _stream())
    return lmap, count


# ---- beam search -----------------------------------------------------------------------------
def log_softmax(x, add=None, mu=0.0):
    """x [M,V] (row stride allowed) -> f32 [M,V] = log_softmax(x) + mu*add[:, :V]"""
    M, V, ld = _rows(_chk(x))
    out = torch.empty(M, V, device=x.device, dtype=torch.float32)
    lib.call("emoasr_log_softmax", dt(x), M, V, _p(x), ld, _p(add), 0 if add is None else add.stride(0), mu, _p(out),
             V, _stream())
    return out


def log_softmax_rows_to(x, n, row_dst, pool, V, row_ok=None):
    """emoasr_log_softmax_rows_to: row r < n of the raw logits x [R, V_lm] (f32 or bf16; row stride allowed) is normalised over all
    V_lm columns, its first V columns go to row row_dst[r] (int32 [>= n]) of the f32 pool [rows, >= V]; a row with row_ok[r] < 0
    (int32, optional) or a destination outside the pool is dropped.  Bit-equal to log_softmax(x)[r, :V]."""
    R, V_lm, ld = _rows(_chk(x))
    n, V = int(n), int(V)
    assert 0 <= n <= R and 1 <= V <= V_lm and _chk(pool, torch.float32).dim() == 2 and pool.stride(1) == 1 and pool.shape[1] >= V
    assert _chk(row_dst, torch.int32).dim() == 1 and row_dst.is_contiguous() and row_dst.numel() >= n
    assert row_ok is None or (_chk(row_ok, torch.int32).is_contiguous() and row_ok.numel() >= n)
    if n:
        lib.call("emoasr_log_softmax_rows_to", dt(x), n, V_lm, V, _p(x), ld, _p(row_dst), _p(row_ok), _p(pool),
                 pool.stride(0) if pool.shape[0] > 1 else pool.shape[1], pool.shape[0], _stream())
    return pool


def topk(x, k, aux=None):
    """x f32 [M,V] -> (vals [M,k], idx int32 [M,k], aux gathered [M,k] | None)"""
    M, V, ld = _rows(_chk(x, torch.float32))
    vals = torch.empty(M, k, device=x.device, dtype=torch.float32)
    idx = torch.empty(M, k, device=x.device, dtype=torch.int32)
    aux_out = torch.empty(M, k, device=x.device, dtype=torch.float32) if aux is not None else None
    lib.call("emoasr_topk", M, V, k, _p(x), ld, _p(aux), 0 if aux is None else aux.stride(0), _p(vals), _p(idx),
             _p(aux_out), _stream())
    return vals, idx, aux_out


CTC_BEAM_MAX_WIDTH = 32
CTC_BEAM_STATUS = {1: "a top-k label outside the vocabulary", 2: "row_off not rising", 4: "more frames than max_frames",
                   8: "workspace share short", 16: "a search names an utterance outside the batch",
                   32: "no free row left in a search's share of the LM pool"}


def ctc_beam_status_text(status):
    return ", ".join(text for bit, text in CTC_BEAM_STATUS.items() if status & bit) or "ok"


def _ctc_beam_outputs(n, W, max_frames, dev):
    """-> (out_tok int32 [n, W, max_frames + 1], out_len int32 [n, W], out_score f64 [n, W], out_n int32 [n]), uninitialised"""
    return (torch.empty(n, W, max_frames + 1, device=dev, dtype=torch.int32), torch.empty(n, W, device=dev, dtype=torch.int32),
            torch.empty(n, W, device=dev, dtype=torch.float64), torch.empty(n, device=dev, dtype=torch.int32))


def ctc_beam_batch(logp, row_off, top, W, blank, eos, len_weight=0.0, max_frames=None):
    """CTC prefix beam search without an LM for B utterances in one launch (csrc/ctc_beam.hip).  logp f32 [rows, V] (row stride
    allowed): log_softmax over all frames of all utterances; row_off int32 [B+1]: utterance b owns rows row_off[b] .. row_off[b+1];
    top int32 [rows, k], k = min(W, V): topk of logp -> device tensors (out_tok int32 [B, W, max_frames + 1], out_len int32 [B, W],
    out_score f64 [B, W] best first, out_n int32 [B], status int32 [1]).  Only the first out_n[b] rows of an utterance and the first
    out_len tokens of a row are defined; out_n[b] = -1 and a bit of status: that utterance was refused (CTC_BEAM_STATUS).  One
    synchronisation here, the check of row_off (which also gives max_frames when it is not passed); the caller reads status with
    the outputs."""
    assert _chk(logp, torch.float32).dim() == 2 and (logp.shape[0] == 0 or logp.stride(1) == 1)
    rows, V = logp.shape
    ld = logp.stride(0) if rows > 1 else V
    B = row_off.numel() - 1
    W = int(W)
    if not 1 <= W <= CTC_BEAM_MAX_WIDTH:
        raise ValueError(f"ctc_beam_batch: beam width {W} is outside 1..{CTC_BEAM_MAX_WIDTH}")
    k = min(W, V)
    assert B >= 0 and _chk(row_off, torch.int32).is_contiguous() and row_off.dim() == 1
    assert _chk(top, torch.int32).shape == (rows, k) and top.is_contiguous()
    dev = logp.device
    if B == 0:
        return _ctc_beam_outputs(0, W, 0, dev) + (torch.zeros(1, device=dev, dtype=torch.int32),)
    # (one synchronisation: the kernel checks each utterance's own offsets, not that they cover the rows)
    n = row_off[1:] - row_off[:-1]
    ok, longest = torch.stack([((row_off[0] == 0) & (row_off[-1] == rows) & (n >= 0).all()).int(), n.max()]).tolist()
    if not ok:
        raise ValueError(f"ctc_beam_batch: row_off must rise from 0 to the {rows} rows")
    max_frames = int(longest) if max_frames is None else int(max_frames)
    out_tok, out_len, out_score, out_n = _ctc_beam_outputs(B, W, max_frames, dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    ws_bytes = lib.size_query("emoasr_ctc_beam_batch_ws_bytes", B, rows, W)
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        lib.call("emoasr_ctc_beam_batch", B, V, W, k, _p(logp), ld, _p(row_off), _p(top), int(blank), int(eos), float(len_weight),
                 max_frames, _p(out_tok), _p(out_len), _p(out_score), _p(out_n), _p(ws), ws_bytes, _p(status), _stream())
    return out_tok, out_len, out_score, out_n, status


def ctc_beam_lm_slots(W):
    """rows of the LM pool one search of beam width W needs (2 W + 2)"""
    return lib.size_query("emoasr_ctc_beam_lm_slots", W)


def ctc_beam_lm_init(row_off, utt, W, eos, max_frames, slots=None):
    """start S = len(utt) fused searches (csrc/ctc_beam_lm.hip) over the B utterances of row_off (int32 [B+1], device): utt int32
    [S] names each search's utterance.  -> the state that ctc_beam_lm_frame / _finish take: .rec int32 [6, S W] (search, node,
    parent node, token, src row, dst row) and .rec_count int32 [1] hold the records of the last call -- here the S roots, src = -1
    -- whose pool rows dst the caller fills before the next call; .status int32 [1] collects the refusals (CTC_BEAM_STATUS)."""
    W = int(W)
    if not 1 <= W <= CTC_BEAM_MAX_WIDTH:
        raise ValueError(f"ctc_beam_lm: beam width {W} is outside 1..{CTC_BEAM_MAX_WIDTH}")
    assert _chk(row_off, torch.int32).is_contiguous() and row_off.dim() == 1 and _chk(utt, torch.int32).is_contiguous() and utt.dim() == 1
    S, B, dev = utt.numel(), row_off.numel() - 1, utt.device
    slots = ctc_beam_lm_slots(W) if slots is None else int(slots)
    max_frames = int(max_frames)
    ws_bytes = lib.size_query("emoasr_ctc_beam_lm_ws_bytes", S, max_frames, W)
    st = SimpleNamespace(S=S, B=B, W=W, eos=int(eos), max_frames=max_frames, slots=slots, row_off=row_off, utt=utt, ws_bytes=ws_bytes,
                         ws=torch.empty(max(ws_bytes // 8, 1), device=dev, dtype=torch.int64), rec_cap=max(S * W, 1),
                         status=torch.zeros(1, device=dev, dtype=torch.int32))
    buf = torch.zeros(1 + 6 * st.rec_cap, device=dev, dtype=torch.int32)
    st.rec_count, st.rec = buf[:1], buf[1:].view(6, st.rec_cap)
    if S:
        with torch.cuda.device(dev):
            lib.call("emoasr_ctc_beam_lm_init", S, B, W, _p(row_off), _p(utt), st.eos, max_frames, slots, _p(st.ws), ws_bytes,
                     _p(st.rec), st.rec_cap, _p(st.rec_count), _p(st.status), _stream())
    return st


def ctc_beam_lm_frame(st, t, logp, top, lm_weight, len_weight, blank, lm_logp):
    """advance every search whose utterance has a frame t by that frame.  logp f32 [rows, V], top int32 [rows, k]: as for
    ctc_beam_batch; lm_weight / len_weight f64 [S]; lm_logp f32 [S * st.slots, >= V]: the pool whose rows the records name.  The new
    prefixes of the frame are in st.rec[:, :st.rec_count]."""
    assert _chk(logp, torch.float32).dim() == 2 and logp.stride(1) == 1 and _chk(lm_logp, torch.float32).dim() == 2 and lm_logp.stride(1) == 1
    rows, V = logp.shape
    k = min(st.W, V)
    assert _chk(top, torch.int32).shape == (rows, k) and top.is_contiguous()
    assert _chk(lm_weight, torch.float64).shape == (st.S,) and _chk(len_weight, torch.float64).shape == (st.S,)
    assert lm_weight.is_contiguous() and len_weight.is_contiguous()
    assert lm_logp.shape[0] >= st.S * st.slots and lm_logp.shape[1] >= V
    if st.S:
        with torch.cuda.device(logp.device):
            lib.call("emoasr_ctc_beam_lm_frame", st.S, st.B, V, st.W, k, int(t), _p(logp), logp.stride(0) if rows > 1 else V,
                     _p(st.row_off), _p(top), _p(st.utt), _p(lm_weight), _p(len_weight), int(blank), st.eos, st.max_frames, _p(lm_logp),
                     lm_logp.stride(0), _p(st.ws), st.ws_bytes, _p(st.rec), st.rec_cap, _p(st.rec_count), _p(st.status), _stream())


def ctc_beam_lm_finish(st):
    """-> (out_tok int32 [S, W, max_frames + 1], out_len int32 [S, W], out_score f64 [S, W] best first, out_n int32 [S]; -1: the
    search was refused, see st.status) as ctc_beam_batch returns them per utterance"""
    dev = st.utt.device
    out_tok, out_len, out_score, out_n = _ctc_beam_outputs(st.S, st.W, st.max_frames, dev)
    if st.S:
        with torch.cuda.device(dev):
            lib.call("emoasr_ctc_beam_lm_finish", st.S, st.W, st.max_frames, st.eos, _p(out_tok), _p(out_len), _p(out_score), _p(out_n),
                     _p(st.ws), st.ws_bytes, _stream())
    return out_tok, out_len, out_score, out_n


def ctc_prefix_init(x, blank):
    T, V = x.shape
    r = torch.empty(T, 2, device=x.device, dtype=torch.float32)
    lib.call("emoasr_ctc_prefix_init", T, V, _p(_chk(x, torch.float32)), blank, _p(r), _stream())
    return r


def ctc_prefix_score(x, cands, last, out_len, blank, eos, prev_states=None, parent=None, pcand=None, init_state=None):
    """x f32 [T,V]; cands int32 [nb,cw]; last/out_len int32 [nb] -> (log_psi [nb,cw], states [nb,cw,T,2])"""
    T, V = x.shape
    nb, cw = cands.shape
    log_psi = torch.empty(nb, cw, device=x.device, dtype=torch.float32)
    states = torch.empty(nb, cw, T, 2, device=x.device, dtype=torch.float32)
    cw_prev = 0 if prev_states is None else prev_states.shape[1]
    lib.call("emoasr_ctc_prefix_score", nb, T, V, cw, _p(x), _p(prev_states), cw_prev, _p(parent), _p(pcand),
             _p(init_state), _p(last), _p(out_len), _p(cands), blank, eos, _p(log_psi), _p(states), _stream())
    return log_psi, states


def ctc_prefix_init_ragged(x, xoff, blank, out, stride):
    """x f32 [sum T_s, V], xoff int32 [S + 1] (device): search s's initial state into out.view(-1)[s * stride:][: 2 T_s]"""
    S = xoff.numel() - 1
    lib.call("emoasr_ctc_prefix_init_ragged", S, x.shape[1], _p(_chk(x, torch.float32)), _p(xoff), blank, _p(out), stride, _stream())


def ctc_prefix_score_ragged(x, xoff, W, Tmax, cands, last, out_len, blank, eos, prev_states, parent, pcand, log_psi=None, states=None):
    """the ragged twin of ctc_prefix_score: row m of cands [nb, cw] belongs to search m // W, which runs over the rows
    xoff[s] .. xoff[s + 1] - 1 of x; prev_states / states [nb, cw, Tmax, 2], parent the GLOBAL row -> (log_psi, states)"""
    nb, cw = cands.shape
    V = x.shape[1]
    if log_psi is None:
        log_psi = torch.empty(nb, cw, device=x.device, dtype=torch.float32)
    if states is None:
        states = torch.zeros(nb, cw, Tmax, 2, device=x.device, dtype=torch.float32)
    lib.call("emoasr_ctc_prefix_score_ragged", nb, W, Tmax, V, cw, _p(_chk(x, torch.float32)), _p(xoff), _p(prev_states),
             prev_states.shape[1], _p(parent), _p(pcand), _p(last), _p(out_len), _p(cands), blank, eos, _p(log_psi), _p(states),
             _stream())
    return log_psi, states


def attn_step_group(q, kv, moff, W, H):
    """single-query cross-attention of S searches of W hypotheses: q [S * W, dd], kv [sum T_s, 2 dd] (K | V) the searches' stacked
    memories, moff int32 [S + 1] (device) -> out [S * W, dd]"""
    nb, dd = q.shape
    S = moff.numel() - 1
    assert nb == S * W and kv.shape[1] == 2 * dd and kv.dtype == q.dtype and q.is_contiguous() and kv.is_contiguous()
    out = torch.empty_like(q)
    lib.call("emoasr_attn_step_group", dt(q), S, W, dd, H, _p(_chk(q)), _p(_chk(kv)), _p(moff), _p(out), _stream())
    return out


# ---- the fusion grid of the joint search (csrc/decode_grid.hip): a search is an (utterance, lm_weight) pair ----
def cell_groups(sutt, W, cells_per_group=None):
    """the row groups of emoasr_attn_step_cells for searches of width W over the utterances sutt[s] (searches of one utterance
    consecutive): up to cells_per_group (default 32 // W, at least 1) consecutive searches of ONE utterance per group
    -> ([(first row, rows, utterance)], the most rows of a group)"""
    cpg = max(1, 32 // W) if cells_per_group is None else int(cells_per_group)
    assert 1 <= W <= 32 and 1 <= cpg and cpg * W <= max(32, W), (W, cpg)
    groups, s, S = [], 0, len(sutt)
    while s < S:
        n = 1
        while n < cpg and s + n < S and sutt[s + n] == sutt[s]:
            n += 1
        groups.append((s * W, n * W, int(sutt[s])))
        s += n
    return groups, max(g[1] for g in groups)


def attn_step_cells(q, kv, moff, groups, group_rows, H, out=None):
    """emoasr_attn_step_group for searches that share utterances: q [nb, dd], kv [sum T_u, 2 dd], moff int32 [U + 1] (device),
    groups a HOST list of (first row, rows, utterance) covering the nb rows (cell_groups) -> out [nb, dd]"""
    import ctypes
    nb, dd = q.shape
    U, G = moff.numel() - 1, len(groups)
    assert kv.shape[1] == 2 * dd and kv.dtype == q.dtype and q.is_contiguous() and kv.is_contiguous()
    flat = [int(v) for g in groups for v in g]
    lib.call("emoasr_cell_groups_check", G, (ctypes.c_int * (3 * G))(*flat), group_rows, nb, U)
    table = torch.tensor(flat, dtype=torch.int32).to(q.device)
    out = torch.empty_like(q) if out is None else out
    lib.call("emoasr_attn_step_cells", dt(q), G, group_rows, nb, U, dd, H, _p(_chk(q)), _p(_chk(kv)), _p(moff), _p(table), _p(out),
             _stream())
    return out


def beam_scores_topk_rows(dec, lm, mu_row, k):
    """emoasr_beam_scores_topk with one weight per row: dec [M, V] (compute dtype), lm f32 [M, V] or None, mu_row f32 [M]
    -> (vals f32 [M, k], idx int32 [M, k], lm_at f32 [M, k])"""
    M, V = dec.shape
    vals = torch.empty(M, k, device=dec.device, dtype=torch.float32)
    idx = torch.empty(M, k, device=dec.device, dtype=torch.int32)
    lm_at = torch.empty(M, k, device=dec.device, dtype=torch.float32)
    lib.call("emoasr_beam_scores_topk_rows", dt(dec), M, V, k, _p(_chk(dec)), V, _p(lm), V if lm is not None else 0,
             _p(_chk(mu_row, torch.float32)) if mu_row is not None else None, _p(vals), _p(idx), _p(lm_at), _stream())
    return vals, idx, lm_at


def ctc_prefix_init_cells(x, xoff, sutt, blank, out, stride):
    """x f32 [sum T_u, V], xoff int32 [U + 1], sutt int32 [S] (device): the initial state of utterance sutt[s] into
    out.view(-1)[s * stride:][: 2 T_u] for every search s (computed once per utterance)"""
    lib.call("emoasr_ctc_prefix_init_cells", sutt.numel(), xoff.numel() - 1, x.shape[1], _p(_chk(x, torch.float32)), _p(xoff), _p(sutt),
             blank, _p(out), stride, _stream())


def ctc_prefix_score_cells(x, xoff, sutt, W, Tmax, cands, last, out_len, blank, eos, prev_states, parent, pcand, log_psi=None,
                           states=None):
    """ctc_prefix_score_ragged with search m // W over the frames of utterance sutt[m // W] -> (log_psi, states)"""
    nb, cw = cands.shape
    V = x.shape[1]
    assert sutt.numel() * W == nb
    if log_psi is None:
        log_psi = torch.empty(nb, cw, device=x.device, dtype=torch.float32)
    if states is None:
        states = torch.zeros(nb, cw, Tmax, 2, device=x.device, dtype=torch.float32)
    lib.call("emoasr_ctc_prefix_score_cells", nb, W, Tmax, V, cw, _p(_chk(x, torch.float32)), _p(xoff), _p(sutt), _p(prev_states),
             prev_states.shape[1], _p(parent), _p(pcand), _p(last), _p(out_len), _p(cands), blank, eos, _p(log_psi), _p(states),
             _stream())
    return log_psi, states


# ---- RNN-T -------------------------------------------------------------------------------------
DACT_TANH_OUT = 5
DACT_MUL = 6            # epilogue dact: multiply by the saved factor (ACT_SAVE_DACT forward)
ACT_SAVE_DACT = 0x100   # epilogue act flag: pre_out <- act'(pre) * dropout_scale


def lstm_cell_fwd(gates_pre, c_prev, h_out, c_out, gates_act):
    """gates_pre [B,4H]; c_prev f32 [B,H] | None; h_out: [B,H] view (row stride allowed)"""
    B, H4 = gates_pre.shape
    lib.call("emoasr_lstm_cell_fwd", dt(gates_pre), B, H4 // 4, _p(gates_pre), _p(c_prev), _p(h_out), h_out.stride(0),
             _p(c_out), _p(gates_act), _stream())


def lstm_seq_supported(x, B, H):
    """does the cooperative whole-sequence recurrence (csrc/lstm_coop.hip) take this layer?"""
    return lib.size_query("emoasr_lstm_seq_supported", dt(x), B, H) == 1


def lstm_seq_fwd(pre, w_hh, h0, c0, hseq, cseq, gact):
    """pre [U,B,4H] (input projection + biases) -> hseq [U,B,H], cseq f32 [U,B,H], gact [U,B,4H] in one launch"""
    U, B, H4 = pre.shape
    for t in (pre, w_hh, hseq, cseq, gact) + tuple(t for t in (h0, c0) if t is not None):
        assert t.is_contiguous()
    for t in (w_hh, hseq, gact) + ((h0,) if h0 is not None else ()):
        assert t.dtype == pre.dtype, (t.dtype, pre.dtype)
    assert cseq.dtype == torch.float32 and (c0 is None or c0.dtype == torch.float32)
    lib.call("emoasr_lstm_seq_fwd", dt(pre), U, B, H4 // 4, _p(pre), _p(w_hh), _p(h0), _p(c0), _p(hseq), _p(cseq), _p(gact), _stream())


_lstm_ws = {}


def lstm_seq_bwd(dh_seq, gact, cseq, c0, w_hh, dgp):
    """dh_seq [U,B,H] (gradient w.r.t. the layer outputs) -> dgp [U,B,4H] (w.r.t. the gate pre-activations) in one launch"""
    U, B, H = dh_seq.shape
    for t in (dh_seq, gact, cseq, w_hh, dgp) + ((c0,) if c0 is not None else ()):
        assert t.is_contiguous()
    for t in (gact, w_hh, dgp):
        assert t.dtype == dh_seq.dtype, (t.dtype, dh_seq.dtype)
    assert cseq.dtype == torch.float32 and (c0 is None or c0.dtype == torch.float32)
    need = lib.size_query("emoasr_lstm_seq_bwd_ws_bytes", B, H)
    key = (dh_seq.device, need)
    ws = _lstm_ws.get(key)
    if ws is None:
        ws = _lstm_ws[key] = torch.empty(need, device=dh_seq.device, dtype=torch.uint8)
    lib.call("emoasr_lstm_seq_bwd", dt(dh_seq), U, B, H, _p(dh_seq), _p(gact), _p(cseq), _p(c0), _p(w_hh), _p(dgp), _p(ws), need,
             _stream())


def lstm_cell_bwd(dh_out, dh_rec, dc, gates_act, c_prev, c, dgates_pre):
    B, H4 = gates_act.shape
    lib.call("emoasr_lstm_cell_bwd", dt(gates_act), B, H4 // 4, _p(dh_out), dh_out.stride(0), _p(dh_rec), _p(dc),
             _p(gates_act), _p(c_prev), _p(c), _p(dgates_pre), _stream())


def bilstm_cell_fwd(s, elens, pre, rec, hstate, cstate, hseq, hprev, cseq, gact):
    """step s of both directions of a length-aware bidirectional LSTM layer (csrc/bilstm.hip): pre [B,T,8H] (row stride allowed),
    rec [2,B,4H] | None (s = 0), hstate [2,B,H] / cstate f32 [2,B,H] in-out, outputs hseq / hprev [2,B,T,H], cseq f32, gact [2,B,T,4H]"""
    _, B, T, H = hseq.shape
    assert pre.stride(-1) == 1 and pre.stride(0) == T * pre.stride(1) and elens.dtype == torch.int32
    for t in (hstate, cstate, hseq, hprev, cseq, gact) + ((rec,) if rec is not None else ()):
        assert t.is_contiguous()
    for t in (pre, hstate, hprev, gact) + ((rec,) if rec is not None else ()):
        assert t.dtype == hseq.dtype, (t.dtype, hseq.dtype)
    assert cseq.dtype == cstate.dtype == torch.float32
    lib.call("emoasr_bilstm_cell_fwd", dt(hseq), B, T, H, s, _p(elens), _p(pre), pre.stride(1), _p(rec), _p(hstate), _p(cstate),
             _p(hseq), _p(hprev), _p(cseq), _p(gact), _stream())


def bilstm_cell_bwd(s, elens, dy, dh_rec, dcstate, gact, cseq, dg, dgc):
    """backward step s (T - 1 .. 0): dy [B,T,H], dh_rec [2,B,H] | None (s = T - 1), dcstate f32 [2,B,H] in-out ->
    dg [2,B,T,4H] at this step's frames, dgc [2,B,4H]"""
    _, B, T, H4 = dg.shape
    for t in (dy, dcstate, gact, cseq, dg, dgc) + ((dh_rec,) if dh_rec is not None else ()):
        assert t.is_contiguous()
    for t in (dy, gact, dgc) + ((dh_rec,) if dh_rec is not None else ()):
        assert t.dtype == dg.dtype, (t.dtype, dg.dtype)
    assert cseq.dtype == dcstate.dtype == torch.float32 and elens.dtype == torch.int32
    lib.call("emoasr_bilstm_cell_bwd", dt(dg), B, T, H4 // 4, s, _p(elens), _p(dy), _p(dh_rec), _p(dcstate), _p(gact), _p(cseq),
             _p(dg), _p(dgc), _stream())


def bilstm_out(elens, x0, x1=None, drop_p=0.0, seed=0):
    """y [B,T,H] = dropout(x0 + x1) at t < elens[b], exact zeros beyond (x1 None: masked dropout of x0)"""
    B, T, H = x0.shape
    assert x0.is_contiguous() and (x1 is None or (x1.is_contiguous() and x1.shape == x0.shape and x1.dtype == x0.dtype))
    assert elens.dtype == torch.int32
    y = torch.empty_like(x0)
    lib.call("emoasr_bilstm_out", dt(x0), B, T, H, _p(elens), _p(x0), _p(x1), _p(y), drop_p, seed, _stream())
    return y


def bilstm_seq_supported(x, B, H):
    """does the cooperative bidirectional recurrence (csrc/lstm_coop.hip) take this layer?"""
    return lib.size_query("emoasr_bilstm_seq_supported", dt(x), B, H) == 1


def bilstm_seq_fwd(elens, pre, w_hh_f, w_hh_r, hseq, hprev, cseq, gact):
    """the whole recurrence of both directions in one cooperative launch: same operands as bilstm_cell_fwd over all steps"""
    _, B, T, H = hseq.shape
    assert pre.stride(-1) == 1 and pre.stride(0) == T * pre.stride(1) and elens.dtype == torch.int32
    for t in (pre, w_hh_f, w_hh_r, hprev, gact):
        assert t.dtype == hseq.dtype, (t.dtype, hseq.dtype)
    for t in (w_hh_f, w_hh_r, hseq, hprev, cseq, gact):
        assert t.is_contiguous()
    assert cseq.dtype == torch.float32
    lib.call("emoasr_bilstm_seq_fwd", dt(hseq), B, T, H, _p(elens), _p(pre), pre.stride(1), _p(w_hh_f), _p(w_hh_r), _p(hseq),
             _p(hprev), _p(cseq), _p(gact), _stream())


def bilstm_seq_bwd(elens, dy, gact, cseq, w_hh_f, w_hh_r, dg):
    """dy [B,T,H] -> dg [2,B,T,4H] over all steps in one cooperative launch"""
    _, B, T, H4 = dg.shape
    H = H4 // 4
    for t in (dy, gact, w_hh_f, w_hh_r):
        assert t.dtype == dg.dtype, (t.dtype, dg.dtype)
    for t in (dy, gact, cseq, w_hh_f, w_hh_r, dg):
        assert t.is_contiguous()
    assert cseq.dtype == torch.float32 and elens.dtype == torch.int32
    need = lib.size_query("emoasr_bilstm_seq_bwd_ws_bytes", B, H)
    key = ("bilstm", dg.device, need)
    ws = _lstm_ws.get(key)
    if ws is None:
        ws = _lstm_ws[key] = torch.empty(need, device=dg.device, dtype=torch.uint8)
    lib.call("emoasr_bilstm_seq_bwd", dt(dg), B, T, H, _p(elens), _p(dy), _p(gact), _p(cseq), _p(w_hh_f), _p(w_hh_r), _p(dg), _p(ws),
             need, _stream())


def joint_tanh(e, g):
    """e [B,T,J], g [B,U,J] -> tanh(e[:, :, None] + g[:, None]) [B,T,U,J]"""
    B, T, J = e.shape
    U = g.shape[1]
    h = torch.empty(B, T, U, J, device=e.device, dtype=e.dtype)
    lib.call("emoasr_joint_tanh", dt(e), B, T, U, J, _p(e), _p(g), _p(h), _stream())
    return h


def joint_reduce(d):
    B, T, U, J = d.shape
    de = torch.empty(B, T, J, device=d.device, dtype=d.dtype)
    dg = torch.empty(B, U, J, device=d.device, dtype=d.dtype)
    lib.call("emoasr_joint_reduce", dt(d), B, T, U, J, _p(d), _p(de), _p(dg), _stream())
    return de, dg


def rnnt_forward(logits, labels, elens, ylens, blank):
    """logits [B,T,U,V]; labels int32 [B,Lmax] (U = Lmax+1) -> ctx tuple, nll f32 [B]"""
    B, T, U, V = logits.shape
    dev = logits.device
    f = lambda: torch.empty(B, T, U, device=dev, dtype=torch.float32)
    lse, lpb, lpy, alpha, beta = f(), f(), f(), f(), f()
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    lib.call("emoasr_rnnt_forward", dt(logits), B, T, U, V, labels.shape[1], _p(logits), _p(labels), _p(elens), _p(ylens),
             blank, _p(lse), _p(lpb), _p(lpy), _p(alpha), _p(beta), _p(nll), _stream())
    return (lse, lpb, lpy, alpha, beta), nll


def rnnt_head_forward(h, w, bias, B, T, U, labels, elens, ylens, blank, lattice_stream=None, rows_per_launch=None):
    """the transducer's output layer + loss lattice WITHOUT the [B,T,U,V] logits: h [B*T*U, J] (bf16), w [V, J]
    -> ctx tuple (lse, lpb, lpy, alpha, beta) f32 [B,T,U], nll f32 [B]   (as rnnt_forward)
    lattice_stream: a torch side stream for the fold + lattice launches (2 B blocks of one wave row each: ~190 us of a mostly
    idle chip); -> (ctx, nll, event, keep) then -- the caller waits for `event` on its own stream before it reads ctx / nll and
    holds `keep` (scratch the side stream still reads) until then
    rows_per_launch: a multiple of 256 that replaces the 4 GiB row step (tests: the launches with row0 > 0 at small sizes)"""
    N, J = h.shape
    V = w.shape[0]
    dev = h.device
    nchunk = (V + 63) // 64
    part = torch.empty(nchunk, N, 2, device=dev, dtype=torch.float32)   # chunk-major: every launch fills its rows
    f = lambda: torch.empty(B, T, U, device=dev, dtype=torch.float32)
    lse, zb, zy, alpha, beta = f(), f(), f(), f(), f()
    zy.fill_(0.0)   # (cells beyond ylens never get a label logit)
    ycol = torch.empty(N, device=dev, dtype=torch.int32)
    lib.call("emoasr_rnnt_ycol", B, T, U, labels.shape[1], _p(labels), _p(ylens), _p(ycol), _stream())
    step = max(1, min(N, ((1 << 31) // (J * 2)) // 256 * 256))   # rows per launch: the operand stays below 4 GiB
    if rows_per_launch is not None:
        assert rows_per_launch > 0 and rows_per_launch % 256 == 0 and rows_per_launch * J * 2 < (1 << 32), rows_per_launch
        step = rows_per_launch
    for r0 in range(0, N, step):
        n = min(step, N - r0)
        lib.call("emoasr_rnnt_head_fwd", dt(h), r0, n, T, U, V, J, labels.shape[1], _p(h[r0:r0 + n]), _p(w), _p(bias), _p(labels),
                 _p(ylens), blank, _p(part), N, _p(zb.view(-1)[r0:r0 + n]), _p(zy.view(-1)[r0:r0 + n]), _p(ycol[r0:r0 + n]), _stream())
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    if lattice_stream is not None:
        main = torch.cuda.current_stream()
        ev0 = torch.cuda.Event()
        ev0.record(main)
        lattice_stream.wait_event(ev0)
        lib.call("emoasr_rnnt_forward_parts", B, T, U, V, _p(part), _p(elens), _p(ylens), _p(lse), _p(zb), _p(zy), _p(alpha),
                 _p(beta), _p(nll), c_void_p(lattice_stream.cuda_stream))
        ev1 = torch.cuda.Event()
        ev1.record(lattice_stream)
        return (lse, zb, zy, alpha, beta), nll, ev1, (part, ycol)
    lib.call("emoasr_rnnt_forward_parts", B, T, U, V, _p(part), _p(elens), _p(ylens), _p(lse), _p(zb), _p(zy), _p(alpha),
             _p(beta), _p(nll), _stream())
    return (lse, zb, zy, alpha, beta), nll


def rnnt_coef(ctx, nll, labels, elens, ylens, gscale, gscale_dev=None):
    """per-cell constants of the output layer's gradient -> coef f32 [cells, 4], ycol int32 [cells]"""
    lse, lpb, lpy, alpha, beta = ctx
    B, T, U = lse.shape
    coef = torch.empty(B * T * U, 4, device=lse.device, dtype=torch.float32)
    ycol = torch.empty(B * T * U, device=lse.device, dtype=torch.int32)
    lib.call("emoasr_rnnt_coef", B, T, U, labels.shape[1], _p(lse), _p(lpb), _p(lpy), _p(alpha), _p(beta), _p(labels), _p(elens),
             _p(ylens), _p(nll), gscale, _p(gscale_dev), _p(coef), _p(ycol), _stream())
    return coef, ycol


def rnnt_head_grad(h, w, bias, coef, ycol, blank, out):
    """out [n, V] (bf16) = gradient rows of the output layer for the cells of h [n, J], logits recomputed"""
    n, J = h.shape
    V = w.shape[0]
    lib.call("emoasr_rnnt_head_grad", dt(h), n, V, J, _p(h), _p(w), _p(bias), _p(coef), _p(ycol), blank, _p(out), out.stride(0),
             _stream())
    return out


def rnnt_grad(logits, ctx, nll, labels, elens, ylens, blank, gscale, gscale_dev=None, out=None):
    B, T, U, V = logits.shape
    lse, lpb, lpy, alpha, beta = ctx
    dz = torch.empty_like(logits) if out is None else out
    lib.call("emoasr_rnnt_grad", dt(logits), B, T, U, V, labels.shape[1], _p(logits), _p(lse), _p(lpb), _p(lpy), _p(alpha),
             _p(beta), _p(labels), _p(elens), _p(ylens), _p(nll), blank, gscale, _p(gscale_dev), _p(dz), _stream())
    return dz


# ---- cross-entropy vocabulary head without the logits (Transformer LM) -------------------------------------------------------
CE_HEAD_MIN_ROWS = 1024    # below this the large-tile product leaves most CUs idle: the materialised path is taken
CE_HEAD_CHUNK = 1024       # rows of dz alive at a time in the backward


def ce_head_ok(x, w):
    """does the logit-free head take this shape?  bf16, V % 8 == 0, K % 64 == 0, enough rows, operands below 4 GiB"""
    M, K, lda = _rows(x)
    V = w.shape[0]
    return (x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and V % 8 == 0 and V >= 256 and K % 64 == 0 and lda == K
            and w.stride(0) == K and M >= CE_HEAD_MIN_ROWS and M * K * 2 < (1 << 32) and V * K * 2 < (1 << 32))


def ce_head_fwd(x, w, bias, labels, wrow=None):
    """x [M, K] bf16, w [V, K] bf16, bias f32 [V], labels int32 [M] (-100 = ignored), wrow f32 [M] | None
    -> (loss rows f32 [M] = -wrow * logp, logp f32 [M] = log p(label | row), ctx for ce_head_bwd).  No [M, V] buffer."""
    assert ce_head_ok(x, w), "ce_head_fwd: shape outside the fused head's gates (ops.ce_head_ok)"
    M, K, _ = _rows(_chk(x))
    V = w.shape[0]
    dev = x.device
    part = torch.empty((V + 63) // 64, M, 2, device=dev, dtype=torch.float32)
    zscr = torch.empty(2 * M, device=dev, dtype=torch.float32)
    ycol = torch.empty(M, device=dev, dtype=torch.int32)
    out = torch.empty(3, M, device=dev, dtype=torch.float32)
    lse, logp, loss = out[0], out[1], out[2]
    lib.call("emoasr_ce_head_fwd", dt(x), M, V, K, _p(x), _p(w), _p(bias), _p(_chk(labels, torch.int32)), _p(wrow), _p(part),
             _p(zscr), _p(ycol), _p(lse), _p(logp), _p(loss), _stream())
    return loss, logp, (lse, ycol, wrow)


def ce_head_sample_ok(x, w, min_rows=None):
    """does the sampling head (ce_head_sample_fwd) take this shape?  ce_head_ok's gates with the kernel's own V >= 64 and at least
    min_rows rows (default CE_HEAD_MIN_ROWS)"""
    M, K, lda = _rows(x)
    V = w.shape[0]
    min_rows = CE_HEAD_MIN_ROWS if min_rows is None else min_rows
    return (x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and V % 8 == 0 and V >= 64 and K % 64 == 0 and lda == K
            and w.stride(0) == K and M >= max(1, min_rows) and M * K * 2 < (1 << 32) and V * K * 2 < (1 << 32))


def ce_head_sample_fwd(x, w, bias, labels, wrow, seed, row0=0, min_rows=None):
    """ce_head_fwd that also draws one sample per row in the product's epilogue -> (loss rows f32 [M], logp f32 [M], samples int32 [M],
    ctx for ce_head_bwd).  samples[m] = argmax_v (z32[m, v] + gumbel_noise(M, V, seed, row0)[m, v]), z32 the f32 accumulator + bias,
    ties to the lowest column: a draw from softmax(z[m]) and a function of (seed, row0 + m, v) only.  No [M, V] buffer."""
    assert ce_head_sample_ok(x, w, min_rows), "ce_head_sample_fwd: shape outside the sampling head's gates (ops.ce_head_sample_ok)"
    assert row0 >= 0
    M, K, _ = _rows(_chk(x))
    V = w.shape[0]
    dev = x.device
    part = torch.empty((V + 63) // 64, M, 4, device=dev, dtype=torch.float32)
    zscr = torch.empty(M, device=dev, dtype=torch.float32)
    ycol = torch.empty(M, device=dev, dtype=torch.int32)
    sample = torch.empty(M, device=dev, dtype=torch.int32)
    out = torch.empty(3, M, device=dev, dtype=torch.float32)
    lse, logp, loss = out[0], out[1], out[2]
    lib.call("emoasr_ce_head_sample_fwd", dt(x), M, V, K, _p(x), _p(w), _p(bias), _p(_chk(labels, torch.int32)), _p(wrow), _p(part),
             _p(zscr), _p(ycol), _p(lse), _p(logp), _p(loss), int(seed) & (2 ** 64 - 1), int(row0), _p(sample), _stream())
    return loss, logp, sample, (lse, ycol, wrow)


def ce_head_bwd(x, w, bias, ctx, dw, dbias, gscale=1.0, gscale_dev=None, chunk=None, want_dx=True):
    """gradients of sum(loss rows) * gscale [* gscale_dev]: dw f32 [V, K] and dbias f32 [V] are ACCUMULATED into, -> dx [M, K] bf16.
    dz = w_row (softmax - onehot) is recomputed `chunk` rows at a time and fed to gemm_nn / gemm_tn."""
    lse, ycol, wrow = ctx
    M, K, _ = _rows(_chk(x))
    V = w.shape[0]
    chunk = min(M, chunk or CE_HEAD_CHUNK)
    dz = torch.empty(chunk, V, device=x.device, dtype=x.dtype)
    coef = torch.empty(chunk, 4, device=x.device, dtype=torch.float32)
    dx = torch.empty(M, K, device=x.device, dtype=x.dtype) if want_dx else None
    for r0 in range(0, M, chunk):
        n = min(chunk, M - r0)
        lib.call("emoasr_ce_head_grad", dt(x), n, V, K, _p(x[r0:r0 + n]), _p(w), _p(bias), _p(lse[r0:r0 + n]), _p(ycol[r0:r0 + n]),
                 None if wrow is None else _p(wrow[r0:r0 + n]), gscale, _p(gscale_dev), _p(coef), _p(dz), V, _stream())
        if want_dx:
            gemm_nn(dz[:n], w, out=dx[r0:r0 + n])
        gemm_tn(dz[:n], x[r0:r0 + n], out=dw, accumulate=True, colsum=dbias)
    return dx


def lm_head_fwd(fused_wanted, x, w, bias, labels, wrow):
    """the LMs' output projection + soft-max reduced per row (logit-free where wanted and ce_head_ok); labels int32 [M] (clamped), wrow
    f32 [M] -> (rows f32 [M] = -wrow[m] * log p(labels[m] | row m), head stash for lm_head_bwd: ("fused" | "materialised", ...))"""
    if fused_wanted and ce_head_ok(x, w):
        rows, _, ctx = ce_head_fwd(x, w, bias, labels, wrow)
        return rows, ("fused", ctx)
    logits = gemm_nt(x, w, bias=bias)
    rows, _ = lsm_loss(logits, labels, wrow, 0.0)
    return rows, ("materialised", logits)


def lm_head_bwd(head, x, w, bias, labels, wrow, dw, dbias, gscale_dev):
    """gradients of sum(rows) * gscale_dev of lm_head_fwd: dw f32 [V, K] and dbias f32 [V] are ACCUMULATED into, -> dx [M, K]"""
    if head[0] == "fused":
        return ce_head_bwd(x, w, bias, head[1], dw, dbias, 1.0, gscale_dev)
    _, dz = lsm_loss(head[1], labels, wrow, 0.0, True, 1.0, gscale_dev)
    gemm_tn(dz, x, out=dw, accumulate=True, colsum=dbias)
    return gemm_nn(dz, w)


# ---- RNN LM: one shallow-fusion step for up to 32 hypotheses (csrc/rnnlm.hip) ------------------------------------------------------
RNNLM_STEP_MAX = 32


def rnnlm_step_supported(x, nb, L, E, H):
    """does the step kernel's shape plan take nb rows of an L-layer LSTM LM (embedding E, hidden H) in x's dtype?"""
    return lib.size_query("emoasr_rnnlm_step_supported", dt(x), nb, L, E, H) == 1


class RnnlmStepWeights:
    """the operands of emoasr_rnnlm_step that do not change between steps: per-layer pointer tables (host arrays of device
    pointers) and the workspace.  Holds the tensors, so the addresses stay valid."""

    def __init__(self, emb, w_ih, w_hh, bias, w_out, b_out):
        self.tensors = (emb, list(w_ih), list(w_hh), list(bias), w_out, b_out)
        self.L, self.E, self.H, self.V = len(w_ih), emb.shape[1], w_hh[0].shape[1], w_out.shape[0]
        arr = c_void_p * self.L
        self.p_ih = arr(*[t.data_ptr() for t in w_ih])
        self.p_hh = arr(*[t.data_ptr() for t in w_hh])
        self.p_b = arr(*[_chk(t, torch.float32).data_ptr() for t in bias])
        self.ws_bytes = lib.size_query("emoasr_rnnlm_step_ws_bytes", _DT[emb.dtype], self.H, self.V)
        self.ws = torch.empty(self.ws_bytes, device=emb.device, dtype=torch.uint8)


def rnnlm_step(W, nb, ids, ph, pc, src, dst, logp, row_dst=None):
    """ids / src / dst / row_dst int32 [>= nb] on the device; ph [L, slots, H] (compute dtype), pc f32 [L, slots, H]: the state pools,
    read at src (< 0: zeros), written at dst; logp f32 [rows, >= V] (row stride allowed): row i -> logp[row_dst[i]] (None: i)"""
    emb, _, _, _, w_out, b_out = W.tensors
    L, slots, H = ph.shape
    assert L == W.L and H == W.H and pc.shape == ph.shape and ph.is_contiguous() and pc.is_contiguous()
    assert ph.dtype == emb.dtype and logp.stride(1) == 1 and logp.shape[1] >= W.V
    for t in (ids, src, dst) + (() if row_dst is None else (row_dst,)):
        assert t.dtype == torch.int32 and t.numel() >= nb and t.is_cuda
    lib.call("emoasr_rnnlm_step", dt(emb), nb, L, W.E, H, W.V, slots, _p(ids), _p(emb), W.p_ih, W.p_hh, W.p_b, _p(ph),
             _p(_chk(pc, torch.float32)), _p(src), _p(dst), _p(w_out), _p(b_out), _p(_chk(logp, torch.float32)), logp.stride(0),
             logp.shape[0], _p(row_dst), _p(W.ws), W.ws_bytes, _stream())


def rnnlm_step_rows_supported(x, L, E, H):
    """does emoasr_rnnlm_step_rows take an L-layer LSTM LM (embedding E, hidden H) in x's dtype?  (the step kernel's plan at 32 rows)"""
    return lib.size_query("emoasr_rnnlm_step_rows_supported", dt(x), L, E, H) == 1


def rnnlm_step_rows(W, R, ids, parent, ph, pc, src_base, dst_base, logits):
    """the step for any R >= 1 rows in one call (csrc/rnnlm.hip): row r consumes ids[r] from the state in slot
    src_base + parent[r] (a parent outside 0 .. R - 1: the zero state) and writes its new state to slot dst_base + r; ids / parent int32
    [>= R] on the device; the two slot ranges lie inside ph / pc [L, slots, H] and do not overlap.  The RAW f32 logits of row r go to
    logits[r] (f32 [>= R, >= V], row stride allowed).  W: RnnlmStepWeights"""
    emb, _, _, _, w_out, b_out = W.tensors
    L, slots, H = ph.shape
    assert L == W.L and H == W.H and pc.shape == ph.shape and ph.is_contiguous() and pc.is_contiguous()
    assert ph.dtype == emb.dtype and logits.stride(1) == 1 and logits.shape[1] >= W.V and logits.shape[0] >= R
    for t in (ids, parent):
        assert t.dtype == torch.int32 and t.numel() >= R and t.is_cuda
    ws = getattr(W, "ws_rows", None)
    need = lib.size_query("emoasr_rnnlm_step_rows_ws_bytes", _DT[emb.dtype], R, H)
    if ws is None or ws.numel() < need:
        ws = W.ws_rows = torch.empty(need, device=emb.device, dtype=torch.uint8)
    rl = rnnlm_rows_fill(R, W.V, emb, (W.p_ih, W.p_hh, W.p_b), w_out, b_out, ph, _chk(pc, torch.float32), src_base, dst_base,
                         _chk(logits, torch.float32), ws)
    lib.call("emoasr_rnnlm_step_rows", dt(emb), ctypes.byref(rl), _p(ids), _p(parent), _stream())


def rnnlm_rows_fill(R, V, emb, tabs, w_out, b_out, ph, pc, src_base, dst_base, logits, ws):
    """-> lib.RnnlmRows for R rows: tabs = (w_ih, w_hh, bias) per-layer pointer tables (host arrays of device pointers, which the
    caller keeps alive), ph / pc [L, slots, H] the state pools, logits f32 [>= R, >= V] (row stride allowed), ws the workspace"""
    rl = lib.RnnlmRows()
    L, slots, H = ph.shape
    rl.L, rl.E, rl.H, rl.V, rl.R = L, emb.shape[1], H, V, R
    rl.emb = emb.data_ptr()
    rl.w_ih, rl.w_hh, rl.bias = (ctypes.cast(t, c_void_p) for t in tabs)
    rl.w_out, rl.b_out = w_out.data_ptr(), b_out.data_ptr()
    rl.ph, rl.pc, rl.slots = ph.data_ptr(), pc.data_ptr(), slots
    rl.src_base, rl.dst_base = src_base, dst_base
    rl.logits, rl.ldl = logits.data_ptr(), logits.stride(0)
    rl.ws, rl.ws_bytes = ws.data_ptr(), ws.numel()
    return rl


# ---- LAS decoder: location-aware attention, one position (csrc/las.hip) -------------------------------------------
LAS_MAX_ATTN_DIM = 512


class LasWeights:
    """the f32 operands of the attention step that do not change between positions: score.conv.weight [10,1,201], score.w_conv
    weight [A,10] + bias [A], score.w_score.weight [1,A]"""

    def __init__(self, filt, w_conv, b_conv, w_score):
        for t in (filt, w_conv, b_conv, w_score):
            assert _chk(t, torch.float32).is_contiguous()
        A = w_conv.shape[0]
        assert tuple(filt.shape[-1:]) == (201,) and filt.numel() == 2010 and tuple(w_conv.shape) == (A, 10)
        assert b_conv.numel() == A and w_score.numel() == A
        self.filt, self.w_conv, self.b_conv, self.w_score, self.A = filt, w_conv, b_conv, w_score, A


def _las_args(W, pk, pq, aw_prev, eouts, elens, drop_p, seed, step):
    B, A = pq.shape
    T, D = eouts.shape[-2], eouts.shape[-1]
    assert A == W.A and pk.shape[-2:] == (T, A) and pk.dtype == pq.dtype == eouts.dtype
    assert pq.is_contiguous() and pk.stride(-1) == 1 and pk.stride(-2) == A and eouts.stride(-1) == 1 and eouts.stride(-2) == D
    a = lib.LasAttend()
    a.B, a.T, a.A, a.D = B, T, A, D
    a.pk, a.pq, a.eouts = _chk(pk).data_ptr(), _chk(pq).data_ptr(), _chk(eouts).data_ptr()
    # a [T,A] / [T,D] operand is one utterance read by every row (the beam's hypotheses); [B,T,*] gives each row its own
    a.pk_bstride = pk.stride(0) if pk.dim() == 3 else 0
    a.eo_bstride = eouts.stride(0) if eouts.dim() == 3 else 0
    assert (pk.dim() == 2 or pk.shape[0] == B) and (eouts.dim() == 2 or eouts.shape[0] == B)
    if aw_prev is not None:
        assert _chk(aw_prev, torch.float32).shape == (B, T) and aw_prev.is_contiguous()
        a.aw_prev = aw_prev.data_ptr()
    a.filt, a.w_conv, a.b_conv, a.w_score = W.filt.data_ptr(), W.w_conv.data_ptr(), W.b_conv.data_ptr(), W.w_score.data_ptr()
    if elens is not None:
        assert _chk(elens, torch.int32).numel() >= B
        a.elens = elens.data_ptr()
    a.drop_p, a.seed, a.step = float(drop_p), int(seed), int(step)
    return a


def las_attend_fwd(W, pk, pq, aw_prev, eouts, elens=None, drop_p=0.0, seed=0, step=0, aw=None, ctx=None, lse=None, scores=None):
    """one position of the location-aware attention for all rows (include/emoasr_hip.h: emoasr_las_attend_t).
    pk [B,T,A] | [T,A] key projection (+ bias), pq [B,A] query projection (+ bias), aw_prev f32 [B,T] | None (position 0),
    eouts [B,T,D] | [T,D], elens int32 [B] | None -> (aw f32 [B,T] the DROPPED weights, ctx [B,D] (a view with a row stride is
    written in place), lse f32 [B])"""
    a = _las_args(W, pk, pq, aw_prev, eouts, elens, drop_p, seed, step)
    dev = pq.device
    aw = torch.empty(a.B, a.T, device=dev, dtype=torch.float32) if aw is None else aw
    ctx = torch.empty(a.B, a.D, device=dev, dtype=pq.dtype) if ctx is None else ctx
    lse = torch.empty(a.B, device=dev, dtype=torch.float32) if lse is None else lse
    scores = torch.empty(a.B, a.T, device=dev, dtype=torch.float32) if scores is None else scores
    assert aw.is_contiguous() and aw.shape == (a.B, a.T) and ctx.shape == (a.B, a.D) and ctx.stride(1) == 1 and ctx.dtype == pq.dtype
    assert scores.numel() >= a.B * a.T and lse.numel() >= a.B
    a.aw, a.ctx, a.ctx_ld, a.lse, a.scores = aw.data_ptr(), ctx.data_ptr(), ctx.stride(0), lse.data_ptr(), scores.data_ptr()
    lib.call("emoasr_las_attend_fwd", dt(pq), byref(a), _stream())
    return aw, ctx, lse


def las_attend_bwd(W, pk, pq, aw_prev, eouts, elens, drop_p, seed, step, aw, ctx, lse, dctx, daw, dpq, daw_prev, dpk, deouts,
                   dw_score, dw_conv, db_conv, dfilt):
    """the reverse of las_attend_fwd at one position: aw / ctx / lse as the forward left them, dctx [B,D] (row stride allowed), daw
    f32 [B,T] | None the gradient arriving at aw from the next position's convolution.  ACCUMULATES (all f32) into dpq [B,A],
    daw_prev [B,T] | None, dpk [B,T,A], deouts [B,T,D] | None and the parameter gradients dw_score [A], dw_conv [A,10], db_conv [A],
    dfilt [10,201]"""
    a = _las_args(W, pk, pq, aw_prev, eouts, elens, drop_p, seed, step)
    B, T, A, D = a.B, a.T, a.A, a.D
    assert pk.dim() == 3 and eouts.dim() == 3
    assert _chk(aw, torch.float32).shape == (B, T) and aw.is_contiguous() and ctx.stride(1) == 1 and dctx.stride(1) == 1
    assert ctx.dtype == pq.dtype and dctx.dtype == pq.dtype and ctx.shape == (B, D) and dctx.shape == (B, D)
    a.aw, a.ctx, a.ctx_ld, a.lse = aw.data_ptr(), ctx.data_ptr(), ctx.stride(0), _chk(lse, torch.float32).data_ptr()
    a.dctx, a.dctx_ld = dctx.data_ptr(), dctx.stride(0)
    for t, shape in ((daw, (B, T)), (daw_prev, (B, T)), (dpq, (B, A)), (dpk, (B, T, A)), (deouts, (B, T, D)), (dw_score, None),
                     (dw_conv, (A, 10)), (db_conv, (A,)), (dfilt, None)):
        if t is not None:
            assert _chk(t, torch.float32).is_contiguous() and (shape is None or tuple(t.shape) == shape), (t.shape, shape)
    assert dw_score.numel() == A and dfilt.numel() == 2010
    a.daw = None if daw is None else daw.data_ptr()
    a.daw_prev = None if daw_prev is None else daw_prev.data_ptr()
    a.deouts = None if deouts is None else deouts.data_ptr()
    a.dpq, a.dpk = dpq.data_ptr(), dpk.data_ptr()
    a.dw_score, a.dw_conv, a.db_conv, a.dfilt = dw_score.data_ptr(), dw_conv.data_ptr(), db_conv.data_ptr(), dfilt.data_ptr()
    lib.call("emoasr_las_attend_bwd", dt(pq), byref(a), _stream())


def las_group_offsets(elens, device):
    """frame counts of S searches -> (moff int32 [S + 1] on the device, the host list): the row offsets of their stacked frames,
    checked on the host (rising, T_s >= 1: emoasr_group_offsets_check) before the upload"""
    offs = [0]
    for n in elens:
        offs.append(offs[-1] + int(n))
    S = len(offs) - 1
    lib.call("emoasr_group_offsets_check", S, (ctypes.c_int * (S + 1))(*offs))
    t = torch.tensor(offs, dtype=torch.int32)
    return t.pin_memory().to(device, non_blocking=True), offs


def _las_group_args(W, pk, eouts, moff, pq, aw_src, parent, state, width, aw_dst, ctx, scores, a=None, S=None):
    """a / S: the struct to fill and the number of searches where moff counts utterances (las_attend_cells)"""
    nb, A = pq.shape
    S = moff.numel() - 1 if S is None else S
    rows, D = eouts.shape
    Tmax = aw_src.shape[1]
    assert nb == S * width and A == W.A and pk.shape == (rows, A) and pk.dtype == pq.dtype == eouts.dtype == ctx.dtype
    assert pq.is_contiguous() and pk.is_contiguous() and eouts.is_contiguous()
    for t in (aw_src, aw_dst, scores):
        assert _chk(t, torch.float32).is_contiguous() and t.shape == (nb, Tmax)
    assert _chk(parent, torch.int32).numel() == nb and _chk(moff, torch.int32).is_contiguous()
    assert _chk(state, torch.int32).is_contiguous() and state.numel() == 4 * S
    assert ctx.shape == (nb, D) and ctx.stride(1) == 1
    a = lib.LasAttendGroup() if a is None else a
    a.S, a.W, a.A, a.D, a.Tmax, a.rows = S, width, A, D, Tmax, rows
    a.pk, a.eouts, a.moff, a.pq = _chk(pk).data_ptr(), _chk(eouts).data_ptr(), moff.data_ptr(), _chk(pq).data_ptr()
    a.aw_src, a.parent, a.state = aw_src.data_ptr(), parent.data_ptr(), state.data_ptr()
    a.filt, a.w_conv, a.b_conv, a.w_score = W.filt.data_ptr(), W.w_conv.data_ptr(), W.b_conv.data_ptr(), W.w_score.data_ptr()
    a.scores, a.aw_dst, a.ctx, a.ctx_ld = scores.data_ptr(), aw_dst.data_ptr(), ctx.data_ptr(), ctx.stride(0)
    return a


def las_attend_group(W, pk, eouts, moff, pq, aw_src, parent, state, width, aw_dst, ctx, scores):
    """one position of the location-aware attention for S searches of `width` rows (include/emoasr_hip.h:
    emoasr_las_attend_group_t): pk [sum T_s, A] / eouts [sum T_s, D] stacked over the searches, moff int32 [S + 1] (device,
    las_group_offsets), pq [S * width, A], aw_src f32 [S * width, Tmax] read at the PARENT's row (parent int32, global rows),
    state int32 [S, 4] of emoasr_beam_update_batch; writes aw_dst, ctx (a view with a row stride is written in place) and the
    scratch `scores` -- for the live rows only"""
    a = _las_group_args(W, pk, eouts, moff, pq, aw_src, parent, state, width, aw_dst, ctx, scores)
    lib.call("emoasr_las_attend_group", dt(pq), byref(a), _stream())


def las_cells_map(sutt, U, device):
    """the search -> utterance map of las_attend_cells, checked on the host (emoasr_las_cells_check) -> int32 [S] on the device"""
    sutt = [int(u) for u in sutt]
    lib.call("emoasr_las_cells_check", len(sutt), (ctypes.c_int * len(sutt))(*sutt), int(U))
    return torch.tensor(sutt, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def las_attend_cells(W, pk, eouts, moff, sutt, pq, aw_src, parent, state, width, aw_dst, ctx, scores):
    """las_attend_group for searches that share utterances (emoasr_las_attend_cells_t): pk / eouts stacked over the U UTTERANCES,
    moff int32 [U + 1], sutt int32 [S] (device, las_cells_map): search s runs over the frames of utterance sutt[s]; everything
    else as las_attend_group, row for row the same bits"""
    S = _chk(sutt, torch.int32).numel()
    assert sutt.is_contiguous()
    c = lib.LasAttendCells()
    _las_group_args(W, pk, eouts, moff, pq, aw_src, parent, state, width, aw_dst, ctx, scores, a=c.g, S=S)
    c.U, c.sutt = moff.numel() - 1, sutt.data_ptr()
    lib.call("emoasr_las_attend_cells", dt(pq), byref(c), _stream())


def las_state_gather_args(pairs, parent, state, width):
    """the pointer table of las_state_gather: pairs of (src, dst) arrays [S * width, ...] with contiguous rows"""
    S = state.numel() // 4
    g = lib.LasStateGather()
    g.S, g.W, g.n = S, width, len(pairs)
    assert _chk(parent, torch.int32).numel() == S * width and _chk(state, torch.int32).is_contiguous()
    g.parent, g.state = parent.data_ptr(), state.data_ptr()
    if len(pairs) > lib.LAS_GATHER_MAX:
        raise lib.EmoasrHipError(f"las_state_gather: {len(pairs)} arrays (1..{lib.LAS_GATHER_MAX})")
    for k, (src, dst) in enumerate(pairs):
        assert _chk(src).shape == _chk(dst).shape and src.dtype == dst.dtype and src.shape[0] == S * width
        assert src.is_contiguous() and dst.is_contiguous()
        g.item[k].src, g.item[k].dst = src.data_ptr(), dst.data_ptr()
        g.item[k].row_bytes = src[0].numel() * src.element_size()
    return g


def las_state_gather(pairs, parent, state, width):
    """dst[r] = src[parent[r]] for every live row r of every (src, dst) pair, ONE launch (exact copies; dead rows untouched)"""
    g = las_state_gather_args(pairs, parent, state, width)
    lib.call("emoasr_las_state_gather", byref(g), _stream())


def las_dropmask(B, T, drop_p, seed, step, device="cuda"):
    """the keep mask las_attend_fwd / _bwd derive at (seed, step): uint8 [B,T], 1 = kept (for tests)"""
    a = lib.LasAttend()
    a.B, a.T, a.drop_p, a.seed, a.step = B, T, float(drop_p), int(seed), int(step)
    mask = torch.empty(B, T, device=device, dtype=torch.uint8)
    lib.call("emoasr_las_dropmask", byref(a), _p(mask), _stream())
    return mask


def argmax_rows(x):
    M, V, ld = _rows(_chk(x))
    out = torch.empty(M, device=x.device, dtype=torch.int32)
    lib.call("emoasr_argmax_rows", dt(x), M, V, _p(x), ld, _p(out), _stream())
    return out


def first_not_equal(x, value):
    """x int32 [n] -> int32 [2] = (first index with x != value or -1, x there or value)"""
    out = torch.empty(2, device=x.device, dtype=torch.int32)
    lib.call("emoasr_first_not_equal", x.numel(), _p(_chk(x, torch.int32)), int(value), _p(out), _stream())
    return out


# ---- optimizer -------------------------------------------------------------------------
def sqnorm(x, out):
    lib.call("emoasr_sqnorm", x.numel(), _p(_chk(x, torch.float32)), _p(out), _stream())


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, gnorm_sq=None, clip=0.0, grad_mult=1.0, skipped=None):
    lib.call("emoasr_adam_step_ex", p.numel(), _p(p), _p(g), _p(m), _p(v), lr, beta1, beta2, eps, weight_decay,
             step, _p(gnorm_sq), clip, grad_mult, _p(skipped), _stream())


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, step, span_end, span_wd, gnorm_sq=None, clip=0.0, grad_mult=1.0, skipped=None):
    """span_end int64 [S] / span_wd f32 [S] on the device: see emoasr_adamw_step (a negative span_wd leaves the span untouched)"""
    assert span_end.dtype == torch.int64 and span_wd.dtype == torch.float32 and span_end.numel() == span_wd.numel()
    lib.call("emoasr_adamw_step", p.numel(), _p(p), _p(g), _p(m), _p(v), lr, beta1, beta2, eps, step, _p(gnorm_sq), clip,
             grad_mult, _p(skipped), _p(_chk(span_end)), _p(_chk(span_wd)), span_end.numel(), _stream())


# ---- features --------------------------------------------------------------------------
def specaug_apply(x, spans, nf, nt, xlens=None, fill=None):
    B, T, F = x.shape
    lib.call("emoasr_specaug_apply", B, T, F, _p(_chk(x, torch.float32)), _p(spans), nf, nt, _p(xlens), _p(fill),
             _stream())
    return x


def cmvn(x, mean, std):
    M = x.numel() // x.shape[-1]
    lib.call("emoasr_cmvn", M, x.shape[-1], _p(x), _p(mean), _p(std), _stream())
    return x


def fbank(wav, frame_len, frame_shift, n_fft, n_mel, preemph, window, mel_fb):
    n = wav.numel()
    T = 1 + (n - frame_len) // frame_shift if n >= frame_len else 0
    feats = torch.empty(T, n_mel, device=wav.device, dtype=torch.float32)
    lib.call("emoasr_fbank", _p(wav), n, frame_len, frame_shift, n_fft, n_mel, preemph, _p(window), _p(mel_fb),
             _p(feats), T, _stream())
    return feats


# ---- small-M decode-step kernels (csrc/rowlin.hip) -------------------------------------------------------------------
def rowlin(x, w, bias=None, act=ACT_NONE, ln_a=None, res=None, ln_r=None, out_f32=False, eps=1e-12):
    """y[M <= 16, N] = act(LN_a?(x) @ w^T + bias) (+ res | LN_r(res)); bf16; ln_a / ln_r = (gamma, beta)"""
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    ga, ba = ln_a if ln_a is not None else (None, None)
    gr, br = ln_r if ln_r is not None else (None, None)
    lib.call("emoasr_rowlin", M, N, K, _p(_chk(x, torch.bfloat16)), x.stride(0), _p(ga), _p(ba), eps, _p(_chk(w, torch.bfloat16)),
             _p(bias), act, _p(res), 0 if res is None else res.stride(0), _p(gr), _p(br), eps, _p(y), int(out_f32), N, _stream())
    return y


def attn_step(qkv, kcache, vcache, pos, H):
    """single-query attention of every row of qkv [nb, 3d] against its cache [nb, Lmax, d]; appends k, v at *pos (device int)"""
    nb, d3 = qkv.shape
    d = d3 // 3
    out = torch.empty(nb, d, device=qkv.device, dtype=qkv.dtype)
    lib.call("emoasr_attn_step", nb, d, H, kcache.shape[1], _p(_chk(qkv, torch.bfloat16)), _p(kcache), _p(vcache), _p(pos), _p(out),
             _stream())
    return out


# ---- batched transducer beam search with the bookkeeping on the device (csrc/rnnt_beam_book.hip) --------------------------------
RNNT_BEAM_MAX_WIDTH, RNNT_BEAM_MAX_EXPANDS = 16, 15
RNNT_BEAM_STATUS = {1: "a picked label outside 1 .. V - 1", 2: "row_off not rising", 4: "a hypothesis longer than the output row",
                    8: "workspace too short for the searches' states and tries", 32: "no free state slot in a search's region"}


def rnnt_beam_start(row_off, W, num_expands, V, eos, ctl, ws, status, ws_bytes=None):
    """every search of row_off (int32 [S + 1], device) at [(<sos>)], score 0, slot 0; writes the control words ctl (int64 [5, S W])
    of round 0.  ws: uint8 workspace of emoasr_rnnt_beam_ws_bytes(S, row_off[-1], W, num_expands) bytes (ws_bytes: what to tell
    the kernels instead of its size)."""
    S = row_off.numel() - 1
    if not 1 <= int(W) <= RNNT_BEAM_MAX_WIDTH:
        raise ValueError(f"rnnt_beam: beam width {W} is outside 1..{RNNT_BEAM_MAX_WIDTH}")
    assert _chk(row_off, torch.int32).is_contiguous() and _chk(ctl, torch.int64).is_contiguous() and ctl.numel() == 5 * S * W
    with torch.cuda.device(ws.device):
        lib.call("emoasr_rnnt_beam_start", S, int(W), int(num_expands), int(V), int(eos), _p(row_off), _p(ctl), _p(ws),
                 ws.numel() if ws_bytes is None else int(ws_bytes), _p(status), _stream())


def rnnt_beam_book(row_off, W, num_expands, V, eos, rec, ctl, ws, status, ws_bytes=None):
    """one round's bookkeeping from the records rec (f32 [S W, >= 1 + 2 W]: what emoasr_rnnt_beam_pick wrote for the rows of ctl)
    and the next round's control words into ctl"""
    S = row_off.numel() - 1
    assert _chk(rec, torch.float32).shape[0] == S * W and rec.stride(1) == 1 and ctl.numel() == 5 * S * W
    with torch.cuda.device(ws.device):
        lib.call("emoasr_rnnt_beam_book", S, int(W), int(num_expands), int(V), int(eos), _p(row_off), _p(rec), rec.stride(0), _p(ctl),
                 _p(ws), ws.numel() if ws_bytes is None else int(ws_bytes), _p(status), _stream())


def rnnt_beam_finish(row_off, W, num_expands, V, eos, Lmax, ws, status, ws_bytes=None):
    """-> (hyps[s][n] with the leading <sos>, float64 scores[s][n], out_n list) best first; one download.  RuntimeError naming the
    cause when a search was refused (RNNT_BEAM_STATUS; its out_n is -1)."""
    S, dev = row_off.numel() - 1, ws.device
    out_tok, out_len, out_score, out_n = _ctc_beam_outputs(S, int(W), int(Lmax), dev)
    with torch.cuda.device(dev):
        lib.call("emoasr_rnnt_beam_finish", S, int(W), int(num_expands), int(V), int(eos), _p(row_off), int(Lmax), _p(out_tok),
                 _p(out_len), _p(out_score), _p(out_n), _p(ws), ws.numel() if ws_bytes is None else int(ws_bytes), _p(status),
                 _stream())
    n, st = out_n.tolist(), int(status.item())
    if st or min(n, default=0) < 0:
        why = ", ".join(text for bit, text in RNNT_BEAM_STATUS.items() if st & bit) or f"status {st}"
        err = RuntimeError(f"rnnt_beam: refused {sum(1 for v in n if v < 0)} of {S} searches: {why}")
        err.out_n = n
        raise err
    tok, lens, score = out_tok.cpu().numpy(), out_len.cpu().numpy(), out_score.cpu().numpy()
    hyps = [[tok[s, i, :lens[s, i]].tolist() for i in range(n[s])] for s in range(S)]
    scores = [[float(score[s, i]) for i in range(n[s])] for s in range(S)]
    return hyps, scores, n


# ---- batched transducer greedy search in lockstep (csrc/rnnt_greedy_batch.hip) ------------------------------------------------------
RNNT_GREEDY_BATCH_MAX_FRAMES = 16


def rnnt_greedy_batch_buffers(S, K, max_seq_len, longest, device):
    """the bookkeeping's buffers for S searches of K frames per step over utterances of at most `longest` frames ->
    (ctl int64 [4 S + 3 S K], state int32 [S, 4], hyp int32 [S, max_seq_len + 1], align int32 [S, longest + max_seq_len + 1],
    lens int32 [S, 2], live int32 [1])"""
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, device=device, dtype=dtype)
    return (z(4 * S + 3 * S * K, dtype=torch.int64), z(S, 4), z(S, max_seq_len + 1), z(S, longest + max_seq_len + 1), z(S, 2), z(1))


def _rnnt_greedy_batch_chk(row_off, K, ctl, state, lens, live):
    S = row_off.numel() - 1
    if not 1 <= int(K) <= RNNT_GREEDY_BATCH_MAX_FRAMES:
        raise ValueError(f"rnnt_greedy_batch: frames_per_step {K} is outside 1..{RNNT_GREEDY_BATCH_MAX_FRAMES}")
    assert _chk(row_off, torch.int32).is_contiguous() and _chk(ctl, torch.int64).is_contiguous() and ctl.numel() == 4 * S + 3 * S * K
    assert _chk(state, torch.int32).is_contiguous() and state.numel() == 4 * S and _chk(lens, torch.int32).is_contiguous()
    assert lens.numel() == 2 * S and _chk(live, torch.int32).numel() == 1
    return S


def rnnt_greedy_batch_start(row_off, K, eos, max_seq_len, ctl, state, lens, live):
    """every search of row_off (int32 [S + 1], device) before its first step: the control words of step 0 (<eos> from slot 2 s into
    slot 2 s + 1, the rows at frames 0 .. K - 1), empty outputs, live = the searches with frames"""
    S = _rnnt_greedy_batch_chk(row_off, K, ctl, state, lens, live)
    with torch.cuda.device(ctl.device):
        lib.call("emoasr_rnnt_greedy_batch_start", S, int(K), int(eos), int(max_seq_len), _p(row_off), _p(ctl), _p(state), _p(lens),
                 _p(live), _stream())


def rnnt_greedy_batch_book(row_off, K, blank, max_seq_len, logits, ctl, state, hyp, align, lens, live):
    """one step's bookkeeping from the logits [S K, V] of the rows of ctl (compute dtype, as the output product stored them): the
    reference's rule per search, the outputs, the next step's control words"""
    S = _rnnt_greedy_batch_chk(row_off, K, ctl, state, lens, live)
    assert logits.dim() == 2 and logits.shape[0] == S * K and logits.stride(1) == 1 and logits.dtype in _DT
    assert _chk(hyp, torch.int32).shape[0] == S and hyp.stride(1) == 1 and _chk(align, torch.int32).shape[0] == S and align.stride(1) == 1
    with torch.cuda.device(ctl.device):
        lib.call("emoasr_rnnt_greedy_batch_book", dt(logits), S, int(K), logits.shape[1], int(blank), int(max_seq_len), _p(row_off),
                 _p(logits), logits.stride(0), _p(ctl), _p(state), _p(hyp), hyp.stride(0), _p(align), align.stride(0), _p(lens),
                 _p(live), _stream())


# ---- RNN-LM shallow fusion inside the batched transducer search (csrc/rnnt_beam_lm.hip) -------------------------------------------
def rnnt_beam_pick(logits, k, blank, out):
    """out[r] (f32, row stride >= 1 + 2 k) = { log_softmax(logits[r])[blank], the k best of log_softmax(logits[r])[1:], their indices
    relative to column 1 as floats } (emoasr_rnnt_beam_pick)"""
    R, V, ldl = _rows(_chk(logits))
    assert _chk(out, torch.float32).shape[0] == R and out.stride(1) == 1
    lib.call("emoasr_rnnt_beam_pick", dt(logits), R, V, int(k), int(blank), _p(logits), ldl, _p(out), out.stride(0), _stream())
    return out


def rnnt_beam_pick_lm(logits, lm_logits, mu, W, k, blank, out, active=None):
    """the fused record of emoasr_rnnt_beam_pick_lm: candidates ranked by log_softmax(logits[r])[v] + mu[r // W] *
    log_softmax(lm_logits[r])[v]; logits [R, V] and lm_logits [R, V_lm >= V] of one dtype (row strides allowed), mu f32 [>= ceil(R / W)],
    active int64 [R] or None; rows with active == 0 leave out untouched"""
    R, V, ldl = _rows(_chk(logits))
    Rl, V_lm, ldlm = _rows(_chk(lm_logits, logits.dtype))
    assert Rl == R and _chk(out, torch.float32).shape[0] == R and out.stride(1) == 1
    assert _chk(mu, torch.float32).is_contiguous() and mu.numel() * int(W) >= R, (mu.shape, W, R)
    assert active is None or (_chk(active, torch.int64).is_contiguous() and active.numel() == R)
    lib.call("emoasr_rnnt_beam_pick_lm", dt(logits), R, V, V_lm, int(k), int(blank), int(W), _p(logits), ldl, _p(lm_logits), ldlm,
             _p(mu), _p(active), _p(out), out.stride(0), _stream())
    return out


def rnnt_beam_gather_rows(pool, dst, active=None, out=None):
    """out[r] = pool[dst[r]] for an active row whose slot lies inside the pool, a zero row otherwise (emoasr_rnnt_beam_gather_rows);
    pool [nslots, H] contiguous, dst / active int64 [R]"""
    nslots, H = pool.shape
    R = dst.numel()
    assert _chk(pool).is_contiguous() and _chk(dst, torch.int64).is_contiguous()
    assert active is None or (_chk(active, torch.int64).is_contiguous() and active.numel() == R)
    if out is None:
        out = torch.empty(R, H, device=pool.device, dtype=pool.dtype)
    assert _chk(out, pool.dtype).is_contiguous() and tuple(out.shape) == (R, H)
    lib.call("emoasr_rnnt_beam_gather_rows", dt(pool), R, H, _p(pool), nslots, _p(dst), _p(active), _p(out), _stream())
    return out
