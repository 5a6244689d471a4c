"""Thin Python wrappers + autograd plumbing over the C ABI (include/yt8m_hip.h).

torch is used for device memory, streams and the autograd tape only; every FLOP of the hot path is a
HIP kernel in libyt8m_hip.so.  No op has a CPU / eager fallback: host tensors raise.  (Documented exceptions: ens_combine /
ens_moments / ens_tensor_moe / ens_mix of the ensemble stage, scale_mix, distill_input, distill_blend, softmax_moe and split_softmax_loss have a composed form that
inputs outside the kernels' layout take by rule, not by failure; so has frame_subset, whose draw is also restated on the host for CPU
tensors; linear_group multiplies CPU tensors with torch, for the host tests.)

Gradient routing: parameters are NOT autograd leaves.  Each op's backward writes dW directly into the
variable's slice of the gradient arena (GEMM beta = 0 on first write, 1 afterwards) and returns None for
it.  A dummy requires-grad scalar (``graph.token``) is threaded through every op so that backward runs
even when the op's data input is plain data (first layer).
"""
import collections
import ctypes
import os

import torch

from . import _lib
from . import wimg as _wimg
from .flags import FLAGS, DEFINE_string
from .variables import get_default_graph

# new: compute dtype of the large GEMMs (BASELINE config 5 is bf16; configs 1-4 are fp32)
DEFINE_string("compute_dtype", "float32", "float32 (exact fp32 MFMA) or bfloat16 (bf16 MFMA operands, fp32 accumulate, fp32 "
              "master weights / gradients / optimiser) for the fully-connected and MoE-head GEMMs; the fused NetVLAD pooling "
              "uses single-f16 operands instead of the f16 hi+lo split.")

_C = _lib.CONSTANTS            # the enumerators and #defines of include/yt8m_hip.h
ACT = {k: _C["YT8M_ACT_" + k.upper()] for k in ("sigmoid", "relu", "relu6", "tanh", "elu")}     # enum yt8m_act
XENT_EPS = 10e-6  # W/losses.py:115


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.Yt8mHipError("yt8m_amd ops run on the MI355X only (got a %s tensor); there is no CPU fallback"
                                    % t.device.type)


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    return t if t.is_contiguous() else t.contiguous()


def _rowmajor2d(t):
    """Accepts 2-D tensors whose inner stride is 1 (row-major with an arbitrary leading dimension)."""
    if t.dim() != 2:
        raise ValueError("expected a 2-D tensor")
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    if t.stride(1) != 1 and t.shape[1] != 1:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    if ld < t.shape[1]:
        t = t.contiguous()
        ld = t.shape[1]
    return t, ld


# ------------------------------------------------------------------------------------------ raw kernels
_WS = {}


def _workspace(device):
    """Split-K workspace of the persistent GEMM: one per (device, stream) -- 256 MiB each of the 288 GB -- so that GEMMs
    running concurrently on different streams (the pipelined LSTM stack) never share scratch."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(_lib.lib().yt8m_gemm_workspace_bytes() // 4, dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


_F32, _F32_BF16 = (torch.float32,), (torch.float32, torch.bfloat16)


def _marshal(pre, M, N, K, a, lda, b, ldb, out, bias, beta, out_dtypes=_F32, new_dtype=torch.float32):
    """One product of a grouped launch -> (yt8m_gemm_problem, its output, the temporaries the launch reads).  a / b: the tensors the
    operand pointers come from (lda = ldb = 0 for operand images); a missing `out` is allocated as [M, N] of new_dtype.  The caller
    keeps the temporaries (contiguous copies, the converted bias) referenced until its launch has returned.  pre: the family's name in
    its error messages."""
    if out is None:
        if beta != 0.0:
            raise ValueError("beta != 0 needs an output tensor")
        out = torch.empty((M, N), dtype=new_dtype, device=a.device)
    if out.dtype not in out_dtypes or tuple(out.shape) != (M, N) or (out.stride(1) != 1 and N != 1):
        raise ValueError(pre + ": bad output tensor")
    ldc = out.stride(0) if M > 1 else max(N, 1)
    if bias is not None:
        bias = _f32c(bias)
        if bias.numel() != N:
            raise ValueError("bias size mismatch")
    pr = _lib.GemmProblem(M, N, K, a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(), ldc,
                          bias.data_ptr() if bias is not None else None, float(beta))
    return pr, out, (a, b, bias)


def _chunks(per, probs, *side):
    """Cuts a group into launches of at most `per` problems: yields (n, yt8m_gemm_problem[n], the same slice of every per-problem
    side list)."""
    for lo in range(0, len(probs), per):
        part = probs[lo:lo + per]
        yield (len(part), (_lib.GemmProblem * len(part))(*part)) + tuple(s[lo:lo + per] for s in side)


def _problem(A, B, out, transA, transB, bias, beta):
    A, lda = _rowmajor2d(A)
    B, ldb = _rowmajor2d(B)
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
    if K != K2:
        raise ValueError("gemm: inner dimensions differ (%d vs %d)" % (K, K2))
    return _marshal("gemm", M, N, K, A, lda, B, ldb, out, bias, beta)


X3 = os.environ.get("YT8M_GEMM_X3", "1") != "0"        # large fp32 products on the bf16 pipe (three-plane split, csrc/gemm_x3.hip)


def _x3_wins(shapes, transA=False, transB=False):
    """The library's cost estimate (csrc/gemm_auto.hip: six bf16 products of split operands on 256 x 256 tiles plus the split passes
    against the fp32-MFMA kernel on 128 x 128 tiles) for every (M, N, K) of a group; the dispatch itself is per product."""
    shapes = [s_ for s_ in shapes if s_[0] * s_[1] * s_[2] != 0]
    return bool(shapes) and all(_lib.lib().yt8m_gemm_x3_pays(int(M), int(N), int(K)) for M, N, K in shapes)


GEMM_ROLE_DW = _C["YT8M_GEMM_ROLE_DW"]
GEMM_ROLE_H2 = _C["YT8M_GEMM_ROLE_H2"]


def gemm_grouped(items, transA=False, transB=False, role=None):
    """items: list of dicts(A=, B=, out=None, bias=None, beta=0.0) sharing transA/transB -> list of outputs.
    role="dw" DECLARES the products weight gradients x^T . dz (transA, neither operand a weight): the library may then run them as
    three f16 products under one device-measured scale per operand (the "h2" contract of include/yt8m_hip.h); without it a
    product keeps the six-product / fp32 forms whatever its transposition flags.
    fp32 operands either way; the library picks the kernel per product (yt8m_gemm_auto_grouped: large products run as six bf16
    MFMA products of three-plane split operands -- fp32-grade error at twice the rate --, the rest on the fp32 MFMA kernel) and
    groups the launches; the operand images live in a scratch tensor sized by the library's own query."""
    probs, outs, keep = [], [], []
    for it in items:
        _dev(it["A"], it["B"], it.get("out"), it.get("bias"))
        pr, out, k = _problem(it["A"], it["B"], it.get("out"), transA, transB, it.get("bias"), it.get("beta", 0.0))
        probs.append(pr)
        outs.append(out)
        keep.append(k)
    if role not in (None, "dw", "h2"):
        raise ValueError("role must be None, 'dw' or 'h2'")
    ta = int(bool(transA)) | (GEMM_ROLE_DW if (role == "dw" and transA and not transB) else 0) | (GEMM_ROLE_H2 if role == "h2" else 0)
    ws = _workspace(outs[0].device)
    lib = _lib.lib()
    if not X3:
        for n, arr in _chunks(4, probs):
            _lib.check(lib.yt8m_gemm_f32_grouped(int(transA), int(transB), n, arr, _p(ws), ws.numel() * 4, _stream()))
        return outs
    # absmaxA / absmaxB: operands whose maximum the caller already has on the device (a [1] float tensor holding it as float bits:
    # yt8m_h2_absmax's form) skip their absmax pass when they take the h2 form
    for n, arr, wa, wb in _chunks(64, probs, [it.get("absmaxA") for it in items], [it.get("absmaxB") for it in items]):
        nb = lib.yt8m_gemm_auto_scratch_bytes(ta, int(transB), n, arr)
        img = torch.empty(nb, dtype=torch.uint8, device=outs[0].device) if nb else None
        if any(w is not None for w in wa) or any(w is not None for w in wb):
            pa = (ctypes.c_void_p * n)(*[w.data_ptr() if w is not None else None for w in wa])
            pb = (ctypes.c_void_p * n)(*[w.data_ptr() if w is not None else None for w in wb])
            _lib.check(lib.yt8m_gemm_auto_grouped_ex(ta, int(transB), n, arr, pa, pb, _p(ws), ws.numel() * 4, _p(img), nb, None, _stream()))
        else:
            _lib.check(lib.yt8m_gemm_auto_grouped(ta, int(transB), n, arr, _p(ws), ws.numel() * 4, _p(img), nb, None, _stream()))
    return outs


def gemm(A, B, out=None, transA=False, transB=False, bias=None, beta=0.0, role=None):
    """out[M,N] = op(A) . op(B) (+ bias) (+ out if beta == 1), through the persistent scheduler (role: see gemm_grouped)."""
    return gemm_grouped([dict(A=A, B=B, out=out, bias=bias, beta=beta)], transA, transB, role=role)[0]


def gemm_simple(A, B, out=None, transA=False, transB=False, bias=None, beta=0.0):
    """Same contract through the plain one-tile-per-workgroup launch (yt8m_gemm_f32)."""
    _dev(A, B, out, bias)
    pr, out, keep = _problem(A, B, out, transA, transB, bias, beta)
    _lib.check(_lib.lib().yt8m_gemm_f32(int(transA), int(transB), pr.M, pr.N, pr.K, pr.A, pr.lda, pr.B, pr.ldb, pr.C, pr.ldc,
                                        pr.bias, float(beta), _stream()))
    return out


def _bf16_empty(rows, cols, device):
    """bf16 [rows, cols] whose rows start 16-byte aligned (row pitch padded to a multiple of 8 elements): the bf16 GEMMs then
    stay on their LDS-DMA path for any reduction length (V*(M+1) = 14148 is not a multiple of 8)."""
    pitch = (cols + 7) // 8 * 8
    return torch.empty((rows, pitch), dtype=torch.bfloat16, device=device)[:, :cols]


def cast_bf16(x, transpose=False):
    """fp32 [R,C] (inner stride 1) -> bf16 [R,C] or, transposed, [C,R] (yt8m_cast_f32_bf16, round to nearest even); the result
    is a view with a 16-byte aligned row pitch."""
    _dev(x)
    x, ld = _rowmajor2d(x)
    R, C = x.shape
    out = _bf16_empty(C, R, x.device) if transpose else _bf16_empty(R, C, x.device)
    _lib.check(_lib.lib().yt8m_cast_f32_bf16(_p(x), R, C, ld, _p(out), out.stride(0), int(transpose), _stream()))
    return out


def gemm_any(A, B, out=None, transA=False, transB=False, bias=None, beta=0.0, bf16=False, role=None):
    """C = op(A) . op(B) (+ bias) (+ C); bf16=True takes bf16 copies of both operands when the product is large enough to pay for the
    two cast passes (_dense_plan's answer for a plain product; its h2 answer is not read: the role is the caller's to state)."""
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    N = B.shape[0] if transB else B.shape[1]
    casts = _dense_plan(M, N, K, bf16, layer=False, need_dx=False).fwd == "bf16_nt"
    return _product("bf16_nt" if casts else "auto", A, B, out=out, transA=transA, transB=transB, bias=bias, beta=beta, role=role)


def cast_bf16_both(x):
    """fp32 [R,C] -> (bf16 [R,C], bf16 [C,R]) from one pass over the source (yt8m_cast_f32_bf16_dual)."""
    _dev(x)
    x, ld = _rowmajor2d(x)
    R, C = x.shape
    plain = _bf16_empty(R, C, x.device)
    trans = _bf16_empty(C, R, x.device)
    _lib.check(_lib.lib().yt8m_cast_f32_bf16_dual(_p(x), R, C, ld, _p(plain), plain.stride(0), _p(trans), trans.stride(0), _stream()))
    return plain, trans


def gemm_bf16_nt_grouped(items):
    """items: dicts(A=bf16 [M,K], B=bf16 [N,K], out=None fp32 [M,N], bias=None, beta=0.0) -> fp32 outputs.
    C = A . B^T on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (yt8m_gemm_bf16_nt_grouped)."""
    probs, outs, keep = [], [], []
    for it in items:
        A, B = it["A"], it["B"]
        _dev(A, B, it.get("out"), it.get("bias"))
        if A.dtype != torch.bfloat16 or B.dtype != torch.bfloat16 or A.dim() != 2 or B.dim() != 2:
            raise TypeError("gemm_bf16_nt: operands must be 2-D bfloat16")
        A = A if A.stride(1) == 1 else A.contiguous()
        B = B if B.stride(1) == 1 else B.contiguous()
        M, K = A.shape
        N, K2 = B.shape
        if K != K2:
            raise ValueError("gemm_bf16_nt: inner dimensions differ (%d vs %d)" % (K, K2))
        pr, out, k = _marshal("gemm_bf16_nt", M, N, K, A, A.stride(0) if M > 1 else max(K, 1), B, B.stride(0) if N > 1 else max(K, 1),
                              it.get("out"), it.get("bias"), it.get("beta", 0.0))
        probs.append(pr)
        outs.append(out)
        keep.append(k)
    ws = _workspace(outs[0].device)
    for n, arr in _chunks(4, probs):                                # the library takes 1..4 problems per launch
        _lib.check(_lib.lib().yt8m_gemm_bf16_nt_grouped(n, arr, _p(ws), ws.numel() * 4, _stream()))
    return outs


# ---- operand images (csrc/gemm_x3.hip, csrc/x3_image.h): [32-row group][16-column K block][plane] of 2-byte elements -----------------
def image_bytes(rows, K, planes):
    """Bytes of a `planes`-plane operand image of a `rows` x `K` operand (a third of the library's three-plane size per plane)."""
    return _lib.lib().yt8m_x3_image_bytes(rows, K) // 3 * planes


def image_buffer(rows, K, planes, device, header=0, alloc=torch.empty):
    """uint8 buffer for that image (at least 16 bytes: an empty operand still hands the kernels a pointer), `header` bytes in front."""
    return alloc(header + max(image_bytes(rows, K, planes), 16), dtype=torch.uint8, device=device)


class X3Image:
    """Operand image of an fp32 matrix: `rows` x `K` logical shape, `planes` planes per K block -- 3: the three-plane bf16 split
    [row][ceil(K/16)][3][16] (x3_split), 1: its first plane alone (bf16_image); 2: see H2Image.  Each image family's product takes
    its own plane count only."""
    __slots__ = ("buf", "rows", "K", "planes")

    def __init__(self, buf, rows, K, planes=3):
        self.buf, self.rows, self.K, self.planes = buf, rows, K, planes


def _image_empty(rows, K, planes, device):
    return X3Image(image_buffer(rows, K, planes, device), rows, K, planes)


def _weight_or_fresh_images(x, want_p, want_t, planes, scale, split):
    """(image of x as an [R rows, K = C] operand, image of x^T as a [C rows, K = R] operand), None where not wanted: the resident image
    of a weight matrix where the optimiser pass keeps one current (wimg.py), else a fresh buffer; `split` (yt8m_x3_split /
    yt8m_bf16_image) fills the fresh ones in one pass over x."""
    _dev(x)
    x, ld = _rowmajor2d(x)
    R, C = x.shape
    imgs, fresh = [None, None], [None, None]
    for trans, want, rows, K in ((0, want_p, R, C), (1, want_t, C, R)):
        if want:
            r = _wimg.resident_image(x, R, C, ld, trans, planes, scale)
            imgs[trans] = X3Image(r[0], rows, K, planes) if r else _image_empty(rows, K, planes, x.device)
            fresh[trans] = None if r else imgs[trans].buf
    if fresh[0] is not None or fresh[1] is not None:
        _lib.check(split(_p(x), R, C, ld, float(scale), _p(fresh[0]), _p(fresh[1]), _stream()))
    return tuple(imgs)


def x3_split(x, plain=True, trans=False, scale=1.0):
    """fp32 [R, C] -> (X3Image of x as an [R rows, K = C] operand or None, X3Image of x^T as a [C rows, K = R] operand or None),
    both from one pass over x (yt8m_x3_split)."""
    return _weight_or_fresh_images(x, plain, trans, 3, scale, _lib.lib().yt8m_x3_split)


def _image_problems(pre, what, planes, items, bf16_out=False):
    """The items of an image family's group -> (problems, outputs, temporaries).  Operands are images of `planes` planes ([M rows, K]
    and [N rows, K]); bf16_out: the family also writes bf16 outputs (an item's out_dtype picks what a missing `out` is made as)."""
    probs, outs, keep = [], [], []
    out_dtypes = _F32_BF16 if bf16_out else _F32
    for it in items:
        A, B = it["A"], it["B"]
        if getattr(A, "planes", None) != planes or getattr(B, "planes", None) != planes:
            raise TypeError("%s: operands must be %s" % (pre, what))
        if A.K != B.K:
            raise ValueError("%s: inner dimensions differ (%d vs %d)" % (pre, A.K, B.K))
        out, bias = it.get("out"), it.get("bias")
        _dev(A.buf, B.buf, out, bias)
        pr, out, k = _marshal(pre, A.rows, B.rows, A.K, A.buf, 0, B.buf, 0, out, bias, it.get("beta", 0.0), out_dtypes,
                              it.get("out_dtype", torch.float32) if bf16_out else torch.float32)
        probs.append(pr)
        outs.append(out)
        keep.append(k)
    return probs, outs, keep


def gemm_x3_grouped(items):
    """items: dicts(A=X3Image [M rows, K], B=X3Image [N rows, K], out=None fp32 [M,N], bias=None, beta=0.0) -> fp32 outputs
    C = A . B^T from six bf16 MFMA products of the split operands (yt8m_gemm_x3_nt_grouped): fp32-grade accuracy."""
    probs, outs, keep = _image_problems("gemm_x3", "X3Image", 3, items)
    ws = _workspace(outs[0].device)
    for n, arr in _chunks(4, probs):                                # the library takes 1..4 problems per launch
        _lib.check(_lib.lib().yt8m_gemm_x3_nt_grouped(n, arr, _p(ws), ws.numel() * 4, _stream()))
    return outs


# ---- h2: fp32 products as three f16 MFMA products of two-plane half images (csrc/gemm_x3.hip gemm_h2q_kernel, round 5) -------------
class H2Image(X3Image):
    """Two IEEE-half planes of S x (csrc/x3_image.h); `scale` = the host-side S (the caller's alpha carries 1 / S), `dinv` = the device
    word with max |x| (yt8m_h2_absmax) when the rest of the scale was chosen on the device, else None."""
    __slots__ = ("scale", "dinv")

    def __init__(self, buf, rows, K, scale=1.0, dinv=None):
        X3Image.__init__(self, buf, rows, K, 2)
        self.scale, self.dinv = float(scale), dinv


def h2_absmax(x):
    """Device int32 word holding max |x| as float bits (yt8m_h2_absmax): the handle of a device-chosen h2 scale."""
    _dev(x)
    x, ld = _rowmajor2d(x)
    word = torch.zeros(1, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().yt8m_h2_absmax(_p(x), x.shape[0], x.shape[1], ld, _p(word), _stream()))
    return word


def h2_split(x, plain=True, trans=False, scale=1.0, dynamic=False):
    """fp32 [R, C] -> (H2Image of x as an [R rows, K = C] operand or None, H2Image of x^T or None).  scale: host power of two with
    |scale x| < 65504; dynamic=True: the scale is measured on the device instead (one more pass over x)."""
    _dev(x)
    x, ld = _rowmajor2d(x)
    R, C = x.shape
    ds = h2_absmax(x) if dynamic else None
    bp = image_buffer(R, C, 2, x.device) if plain else None
    bt = image_buffer(C, R, 2, x.device) if trans else None
    _lib.check(_lib.lib().yt8m_h2_split(_p(x), R, C, ld, float(scale), _p(ds), _p(bp), _p(bt), None, _stream()))
    return (H2Image(bp, R, C, scale, ds) if plain else None, H2Image(bt, C, R, scale, ds) if trans else None)


def gemm_h2_grouped(items):
    """items: dicts(A=H2Image [M rows, K], B=H2Image [N rows, K], out=None fp32 [M,N], bias=None, beta=0.0) -> fp32 outputs
    C = A . B^T from three f16 MFMA products of the two-plane operands (yt8m_gemm_h2_nt_grouped); the images' scales are undone in
    the epilogue (host part as alpha, device part through pointers)."""
    probs, outs, keep = _image_problems("gemm_h2", "H2Image", 2, items)
    alphas = [1.0 / (it["A"].scale * it["B"].scale) for it in items]
    dsa = [it["A"].dinv.data_ptr() if it["A"].dinv is not None else None for it in items]
    dsb = [it["B"].dinv.data_ptr() if it["B"].dinv is not None else None for it in items]
    ws = _workspace(outs[0].device)
    for n, arr, al, pa, pb in _chunks(4, probs, alphas, dsa, dsb):
        _lib.check(_lib.lib().yt8m_gemm_h2_nt_grouped(n, arr, (ctypes.c_float * n)(*al), (ctypes.c_void_p * n)(*pa), (ctypes.c_void_p * n)(*pb),
                                                      _p(ws), ws.numel() * 4, _stream()))
    return outs


B1_IMAGES = os.environ.get("YT8M_BF16_IMAGES", "1") != "0"   # bf16 configuration: large products on one-plane operand images (gemm_b1_kernel)


def _b1_ok(M, N, K):
    """Large enough for the 256 x 256 image kernel to pay (at least half a round of tiles, a few K steps)."""
    return B1_IMAGES and ((M + 255) // 256) * ((N + 255) // 256) >= 64 and K >= 256


def bf16_image(x, transpose=False, both=False):
    """fp32 [R, C] -> one-plane bf16 operand image(s) of csrc/gemm_x3.hip (yt8m_bf16_image): the matrix as an [R rows, K = C]
    operand, its transpose as a [C rows, K = R] operand (transpose=True), or both from one pass (both=True -> (plain, trans))."""
    ip, it = _weight_or_fresh_images(x, both or not transpose, both or transpose, 1, 1.0, _lib.lib().yt8m_bf16_image)
    return (ip, it) if both else (it if transpose else ip)


def gemm_b1_grouped(items):
    """items: dicts(A=image [M rows, K], B=image [N rows, K], out=None fp32 [M,N], bias=None, beta=0.0) -> fp32 outputs;
    C = A . B^T on v_mfma_f32_32x32x16_bf16 from ONE-plane bf16 operand images (yt8m_gemm_b1_nt_grouped)."""
    probs, outs, keep = _image_problems("gemm_b1", "one-plane images", 1, items, bf16_out=True)
    for pr, out in zip(probs, outs):
        if out.dtype == torch.bfloat16 and (pr.beta != 0.0 or out.stride(0) % 4 != 0):
            raise ValueError("gemm_b1: a bf16 output takes beta = 0 and a row pitch that is a multiple of 4")
    ws = _workspace(outs[0].device)
    for n, arr, part in _chunks(4, probs, outs):
        mask = sum(1 << j for j, o in enumerate(part) if o.dtype == torch.bfloat16)
        if mask:                                  # bf16 outputs (round 6: the MoE logits of the bf16 configuration)
            _lib.check(_lib.lib().yt8m_gemm_b1_nt_grouped_bf16c(n, arr, mask, _p(ws), ws.numel() * 4, _stream()))
        else:
            _lib.check(_lib.lib().yt8m_gemm_b1_nt_grouped(n, arr, _p(ws), ws.numel() * 4, _stream()))
    return outs


def gemm_batched(A, B, out=None, transA=False, transB=False, beta=0.0):
    """Batched over dim 0 of 3-D contiguous tensors.  yt8m_gemm_f32_batched."""
    _dev(A, B, out)
    A, B = _f32c(A), _f32c(B)
    nb = A.shape[0]
    M, K = (A.shape[2], A.shape[1]) if transA else (A.shape[1], A.shape[2])
    K2, N = (B.shape[2], B.shape[1]) if transB else (B.shape[1], B.shape[2])
    if K != K2 or B.shape[0] != nb:
        raise ValueError("gemm_batched: shape mismatch")
    if out is None:
        out = torch.empty((nb, M, N), dtype=torch.float32, device=A.device)
    if not out.is_contiguous() or tuple(out.shape) != (nb, M, N):
        raise ValueError("gemm_batched: bad output tensor")
    _lib.check(_lib.lib().yt8m_gemm_f32_batched(int(transA), int(transB), M, N, K, _p(A), A.shape[2], A.shape[1] * A.shape[2],
                                                _p(B), B.shape[2], B.shape[1] * B.shape[2], _p(out), N, M * N,
                                                float(beta), nb, _stream()))
    return out


def colsum(X, out, beta=0.0):
    _dev(X, out)
    X, ld = _rowmajor2d(X)
    ws = _workspace(X.device)       # stream-ordered scratch shared with the GEMM's split-K partials
    _lib.check(_lib.lib().yt8m_colsum_f32(_p(X), X.shape[0], X.shape[1], ld, _p(out), float(beta), _p(ws),
                                          min(ws.numel() * 4, 1 << 22), _stream()))
    return out


def act_fwd(kind, x):
    _dev(x)
    x = _f32c(x)
    y = torch.empty_like(x)
    _lib.check(_lib.lib().yt8m_act_fwd_f32(ACT[kind], _p(x), _p(y), x.numel(), _stream()))
    return y


def act_bwd(kind, y, dy):
    _dev(y, dy)
    y, dy = _f32c(y), _f32c(dy)
    dx = torch.empty_like(y)
    _lib.check(_lib.lib().yt8m_act_bwd_f32(ACT[kind], _p(y), _p(dy), _p(dx), y.numel(), _stream()))
    return dx


def l2norm_fwd(x, eps=1e-12):
    _dev(x)
    x = _f32c(x)
    cols = x.shape[-1]
    y = torch.empty_like(x)
    _lib.check(_lib.lib().yt8m_l2norm_fwd_f32(_p(x), _p(y), x.numel() // max(cols, 1), cols, eps, _stream()))
    return y


def l2norm_bwd(x, dy, eps=1e-12):
    _dev(x, dy)
    x, dy = _f32c(x), _f32c(dy)
    cols = x.shape[-1]
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().yt8m_l2norm_bwd_f32(_p(x), _p(dy), _p(dx), x.numel() // max(cols, 1), cols, eps, _stream()))
    return dx


def dequant_l2norm(q, num_frames=None, eps=1e-12):
    """uint8 [B,F,D] -> float32 [B,F,D]: dequantise, zero the padding rows, L2-normalise each frame."""
    _dev(q, num_frames)
    if q.dtype != torch.uint8 or q.dim() != 3:
        raise TypeError("expected uint8 [B,F,D]")
    q = q.contiguous()
    B, F, D = q.shape
    x = torch.empty((B, F, D), dtype=torch.float32, device=q.device)
    nf = None if num_frames is None else num_frames.to(torch.int32).contiguous()
    _lib.check(_lib.lib().yt8m_dequant_l2norm_u8(_p(q), _p(nf), _p(x), B, F, D, eps, _stream()))
    return x


def dequant_mean_l2norm(q, num_frames=None, eps=1e-12):
    """uint8 [B,F,D] -> float32 [B,D]: mean of the dequantised valid frames, L2-normalised."""
    _dev(q, num_frames)
    if q.dtype != torch.uint8 or q.dim() != 3:
        raise TypeError("expected uint8 [B,F,D]")
    q = q.contiguous()
    B, F, D = q.shape
    x = torch.empty((B, D), dtype=torch.float32, device=q.device)
    nf = None if num_frames is None else num_frames.to(torch.int32).contiguous()
    _lib.check(_lib.lib().yt8m_dequant_mean_l2norm_u8(_p(q), _p(nf), _p(x), B, F, D, eps, _stream()))
    return x


# ---- training-time data augmenters (csrc/augment.hip; data_augmentation.py) --------------------------------------------------------
def _frames_nf(x, num_frames):
    """num_frames may be on the host (as the reader hands it over): it is copied to the frames' device."""
    _dev(x)
    if x.dim() != 3:
        raise ValueError("expected frames [B,F,D], got %d dimensions" % x.dim())
    if num_frames is None:
        raise ValueError("the frame augmenters need num_frames")
    return x.contiguous(), num_frames.to(device=x.device, dtype=torch.int32).contiguous()


def half_segments(x, num_frames):
    """HalfAugmenter's gather (W/all_data_augmentation/half_augmenter.py:8-45): uint8 or float32 frames [B,F,D] -> ([3B,F,D] of the
    same dtype, num_frames [3B] int32 on the device) = [originals; first halves; second halves], zeros past each half's
    s = max(n // 2, 1) frames.  Frames are data: no gradient."""
    x, nf = _frames_nf(x, num_frames)
    B, F, D = x.shape
    y = torch.empty((3 * B, F, D), dtype=x.dtype, device=x.device)
    nf_out = torch.empty((3 * B,), dtype=torch.int32, device=x.device)
    if x.dtype == torch.uint8:
        fn = _lib.lib().yt8m_half_segments_u8
    elif x.dtype == torch.float32:
        fn = _lib.lib().yt8m_half_segments_f32
    else:
        raise TypeError("expected uint8 or float32 frames, got %s" % x.dtype)
    _lib.check(fn(_p(x), _p(nf), _p(y), _p(nf_out), B, F, D, _stream()))
    return y, nf_out


# ---- random half-frame inference (csrc/frame_subset.hip; FrameRandomEvalModel, FrameAttentionEvalModel, LstmRandomModel) ------------
# anything but 0 (the default): frame_subset gathers with the kernel of csrc/frame_subset.hip; 0: with index_select, a comparison and a
# sum (A/B runs, tests).  The draw has one form per device either way.  The kernel is the default because tools/frame_subset_step.py's op
# leg showed its median below the composed form's at every shape in both runs (3.8 - 8.3 x: DESIGN_LOG.md section 44).
FRAME_SUBSET_FUSED = os.environ.get("YT8M_FRAME_SUBSET_FUSED", "1") != "0"
FRAME_SUBSET_CALLS = {"kernels": 0, "composed": 0}      # which form gathered (tests)
FRAME_SUBSET_MAX_F = 1024                               # csrc/frame_subset.hip DRAW_MAX_F


def _philox_words_host(n, seed):
    """The uint32 Philox4x32-10 word of logical elements 0..n-1 under key = seed (csrc/philox.h: counter (element >> 2, 0), word
    element & 3), in numpy integer arithmetic: the host form of the draw, for CPU tensors."""
    import numpy as np
    u, mask = np.uint64, np.uint64(0xFFFFFFFF)
    ctr = np.arange((n + 3) // 4, dtype=np.uint64)
    c0, c1, c2, c3 = ctr & mask, ctr >> u(32), np.zeros_like(ctr), np.zeros_like(ctr)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c0 * u(0xD2511F53), c2 * u(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ u(k0), p1 & mask, (p0 >> u(32)) ^ c3 ^ u(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).reshape(-1)[:n]


def frame_subset_index(E, F, K, seed=None, device=None):
    """index [E,K] int32: per replica one uniformly random K-subset of the frame indices 0..F-1 in ascending order -- what the first K
    entries of tf.random_shuffle's permutation are after Z/frame_level_models.py:6195-6199 has sorted them -- shared by every video of
    the batch.  Frame f of replica e takes the Philox word of logical element e F4 + f (F4 = F rounded up to a multiple of 4) under
    key = seed; the subset is the K frames with the smallest (word, f) pairs.  seed None: the graph's next random-op key; device None:
    the graph's.  A CPU device restates the draw on the host: for one seed, CPU and device hold the same index."""
    E, F, K = int(E), int(F), int(K)
    if seed is None:
        seed = get_default_graph().next_random_seed()
    device = torch.device(device) if device is not None else get_default_graph().device
    if E < 0 or not 2 <= F <= FRAME_SUBSET_MAX_F or not 1 <= K <= F:
        raise ValueError("frame_subset_index: E >= 0, 2 <= F <= %d and 1 <= K <= F, got E = %d, F = %d, K = %d" % (FRAME_SUBSET_MAX_F, E, F, K))
    if device.type != "cuda":
        import numpy as np
        F4 = (F + 3) // 4 * 4
        w = _philox_words_host(E * F4, seed).reshape(E, F4)[:, :F]
        order = np.argsort(w, axis=1, kind="stable")                            # stable: ties go to the smaller f
        return torch.from_numpy(np.sort(order[:, :K], axis=1).astype(np.int32)).to(device)
    index = torch.empty((E, K), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().yt8m_frame_subset_draw(_p(index), E, F, K, int(seed), _stream()))
    return index


def frame_subset_composed(x, num_frames, index):
    """frame_subset's gather in torch ops: index_select, the count from a comparison and a sum, padding rows multiplied to zero."""
    B, F, D = x.shape
    E, K = index.shape
    idx = index.to(torch.int64)
    inside = (idx >= 0) & (idx < F)
    live = inside[None] & (idx[None] < num_frames.clamp(0, F).to(torch.int64).view(B, 1, 1))        # [B,E,K]
    y = x.index_select(1, idx.clamp(0, F - 1).flatten()).view(B * E, K, D)
    return y * live.view(B * E, K, 1).to(x.dtype), live.sum(dim=2).view(B * E).to(torch.int32)


def frame_subset(x, num_frames, E, K=None, seed=None, index=None):
    """E replicas of every video on a random, order-preserving K-subset of its frames (Z/frame_level_models.py:6189-6217; K None: F // 2):
    uint8 or float32 frames [B,F,D] -> (y [B E,K,D] of the same dtype, num_frames_out [B E] int32, index [E,K] int32), row b E + e =
    replica e of video b.  y[b E + e, j] = x[b, index[e,j]] where index[e,j] < num_frames[b] (clamped to [0, F]), else a zero row;
    num_frames_out counts the former.  The indices ascend, so a replica is a padded video: its real frames first, then zeros.  index
    None: frame_subset_index(E, F, K, seed) on the frames' device.  An index outside [0, F) is padding.  Frames are data: no gradient.
    The gather runs csrc/frame_subset.hip where FRAME_SUBSET_FUSED is on; CPU tensors, other dtypes and the switch's 0 take
    frame_subset_composed."""
    if x.dim() != 3:
        raise ValueError("expected frames [B,F,D], got %d dimensions" % x.dim())
    if num_frames is None:
        raise ValueError("frame_subset needs num_frames")
    B, F, D = x.shape
    E = int(E)
    if index is None:
        index = frame_subset_index(E, F, F // 2 if K is None else K, seed=seed, device=x.device)
    index = index.to(device=x.device, dtype=torch.int32).contiguous()
    if index.dim() != 2 or index.shape[0] != E or (K is not None and index.shape[1] != int(K)):
        raise ValueError("frame_subset: index must be [E = %d, K], got %s" % (E, tuple(index.shape)))
    K = index.shape[1]
    x, nf = x.contiguous(), num_frames.to(device=x.device, dtype=torch.int32).contiguous()
    fused = FRAME_SUBSET_FUSED and x.is_cuda and x.dtype in (torch.uint8, torch.float32)
    FRAME_SUBSET_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return frame_subset_composed(x, nf, index) + (index,)
    y = torch.empty((B * E, K, D), dtype=x.dtype, device=x.device)
    nf_out = torch.empty((B * E,), dtype=torch.int32, device=x.device)
    fn = _lib.lib().yt8m_frame_subset_gather_u8 if x.dtype == torch.uint8 else _lib.lib().yt8m_frame_subset_gather_f32
    _lib.check(fn(_p(x), _p(nf), _p(index), _p(y), _p(nf_out), B, F, D, E, K, _stream()))
    return y, nf_out, index


def half_segment_means(q, num_frames, l2norm=False, eps=1e-12):
    """HalfVideoAugmenter (W/all_data_augmentation/half_video_augmenter.py:8-16) in one pass over the bytes: uint8 [B,F,D] -> float32
    [3B,D], the means of the dequantised frames of the whole video and of its two halves (0 where there is no real frame).  l2norm:
    also L2-normalise every row (the DefaultTransformer, folded)."""
    q, nf = _frames_nf(q, num_frames)
    if q.dtype != torch.uint8:
        raise TypeError("expected the reader's uint8 frames, got %s" % q.dtype)
    B, F, D = q.shape
    x = torch.empty((3 * B, D), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().yt8m_half_segment_means_u8(_p(q), _p(nf), _p(x), B, F, D, 1 if l2norm else 0, eps, _stream()))
    return x


def dequant_noise(q, num_frames, stddev, seed):
    """uint8 [B,F,D] -> float32 [B,F,D]: utils.Dequantize with the padding frames 0, plus N(0, stddev^2) over every element (the
    frame-level NoiseAugmenter); bit for bit the dequantisation followed by add_noise(stddev, seed).  stddev = 0: dequantise only."""
    q, nf = _frames_nf(q, num_frames)
    if q.dtype != torch.uint8:
        raise TypeError("expected the reader's uint8 frames, got %s" % q.dtype)
    B, F, D = q.shape
    y = torch.empty((B, F, D), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().yt8m_dequant_noise_u8(_p(q), _p(nf), _p(y), B, F, D, float(stddev), int(seed), _stream()))
    return y


def dequantize_frames(q, num_frames):
    """uint8 [B,F,D] -> float32 [B,F,D]: what the reference's reader hands over (utils.Dequantize, zero padding frames)."""
    return dequant_noise(q, num_frames, 0.0, 0)


# ---- input transformers beyond the default (csrc/transform.hip; feature_transform.py) -----------------------------------------------
def resolution_mean(x, num_frames, resolution, l2norm=True, eps=1e-12):
    """ResolutionTransformer (W/all_feature_transform/resolution_transformer.py:7-29) in one pass: uint8 or float32 frames [B,F,D] ->
    (float32 [B, F // r, D], num_frames // r [B] int32 on the device).  Row g of a video is the mean of its frames [g r, (g + 1) r),
    l2-normalised when l2norm; frames from (F // r) r on are dropped.  uint8: dequantised with the padding frames 0, the divisor
    always r.  float32: the plain mean of the rows as they are.  num_frames may be on the host.  Frames are data: no gradient."""
    x, nf = _frames_nf(x, num_frames)
    B, F, D = x.shape
    r = int(resolution)
    if r < 1 or r > F:
        raise ValueError("resolution must be in [1, F = %d], got %d" % (F, r))
    if x.dtype == torch.uint8:
        fn = _lib.lib().yt8m_resolution_mean_u8
    elif x.dtype == torch.float32:
        fn = _lib.lib().yt8m_resolution_mean_f32
    else:
        raise TypeError("expected uint8 or float32 frames, got %s" % x.dtype)
    y = torch.empty((B, F // r, D), dtype=torch.float32, device=x.device)
    nf_out = torch.empty((B,), dtype=torch.int32, device=x.device)
    _lib.check(fn(_p(x), _p(nf), _p(y), _p(nf_out), B, F, D, r, 1 if l2norm else 0, eps, _stream()))
    return y, nf_out


# anything but 0 (the default): frame_pyramid runs csrc/frame_pyramid.hip on the reader's bytes where it covers the shape; 0: every level
# is composed from resolution_mean, slices, l2_normalize and a transpose copy (A/B runs, tests).  The rule for the default and the
# measurements behind it: DESIGN_LOG.md section 24.
FRAME_PYRAMID_FUSED = os.environ.get("YT8M_FRAME_PYRAMID_FUSED", "1") != "0"


def frame_pyramid_supported(D, widths, levels):
    widths = [int(w) for w in widths]
    return bool(_lib.lib().yt8m_frame_pyramid_supported(int(D), len(widths), (ctypes.c_int64 * len(widths))(*widths), int(levels)))


def frame_pyramid(x, num_frames, levels, widths, eps=1e-12):
    """The coarse inputs of the multi-resolution LSTM plugin (W/all_frame_models/multires_lstm_memory_deep_combine_chain_model.py:149-165,
    :21): uint8 or float32 frames [B,F,D] -> (parts, num_frames_out) with parts[l][s] float32 [F // r, B, widths[s]] TIME-major for
    r = 2^(l+1), l < levels -- the mean over every r frames (resolution_mean's: dequantised bytes with the padding frames 0, floats as
    they are; the divisor always r), split by widths and every part l2-normalised -- and num_frames_out[l] = num_frames // r [B] int32 on
    the device.  uint8: one pass over the bytes writes every level (csrc/frame_pyramid.hip) where yt8m_frame_pyramid_supported holds and
    FRAME_PYRAMID_FUSED is on; everything else composes resolution_mean(l2norm=False) -> slice -> l2_normalize -> transpose copy per
    level.  Frames are data: no gradient."""
    x, nf = _frames_nf(x, num_frames)
    B, F, D = x.shape
    levels, widths = int(levels), [int(w) for w in widths]
    if levels < 1 or (1 << levels) > F:
        raise ValueError("frame_pyramid: levels must be >= 1 with 2^levels <= F = %d, got %d" % (F, levels))
    if not widths or min(widths) <= 0 or sum(widths) != D:
        raise ValueError("frame_pyramid: widths %s do not partition the %d columns" % (widths, D))
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError("expected uint8 or float32 frames, got %s" % x.dtype)
    if x.dtype == torch.uint8 and FRAME_PYRAMID_FUSED and x.data_ptr() % 16 == 0 and frame_pyramid_supported(D, widths, levels):
        n = len(widths)
        parts = [[torch.empty((F >> (l + 1), B, w), dtype=torch.float32, device=x.device) for w in widths] for l in range(levels)]
        nf_out = [torch.empty((B,), dtype=torch.int32, device=x.device) for _ in range(levels)]
        _lib.check(_lib.lib().yt8m_frame_pyramid_u8(_p(x), _p(nf), B, F, D, levels, n, (ctypes.c_int64 * n)(*widths),
                                                    (ctypes.c_void_p * (levels * n))(*[t.data_ptr() for row in parts for t in row]),
                                                    (ctypes.c_void_p * levels)(*[t.data_ptr() for t in nf_out]), eps, _stream()))
        return parts, nf_out
    parts, nf_out = [], []
    with torch.no_grad():
        for l in range(levels):
            y, n_l = resolution_mean(x, nf, 2 << l, l2norm=False, eps=eps)
            row, off = [], 0
            for w in widths:
                row.append(l2_normalize(y[:, :, off:off + w].contiguous(), eps).transpose(0, 1).contiguous())
                off += w
            parts.append(row)
            nf_out.append(n_l)
    return parts, nf_out


def moe_mix_fwd(Zg, Ze, V, M):
    _dev(Zg, Ze)
    B = Zg.shape[0]
    p = torch.empty((B, V), dtype=torch.float32, device=Zg.device)
    if Zg.dtype == torch.bfloat16:                # logits written as bf16 by the b1 product (Z16_LOGITS)
        _lib.check(_lib.lib().yt8m_moe_mix_fwd_bf16z(_p(Zg), _p(Ze), _p(p), B, V, M, _stream()))
    else:
        _lib.check(_lib.lib().yt8m_moe_mix_fwd(_p(Zg), _p(Ze), _p(p), B, V, M, _stream()))
    return p


def moe_mix_bwd_(Zg, Ze, dp, V, M):
    _dev(Zg, Ze, dp)
    dp = _f32c(dp)
    _lib.check(_lib.lib().yt8m_moe_mix_bwd(_p(Zg), _p(Ze), _p(dp), Zg.shape[0], V, M, _stream()))
    return Zg, Ze


def _labels_arg(labels):
    if labels.dtype == torch.bool:
        labels = labels.view(torch.uint8)
    if labels.dtype == torch.uint8:
        return labels.contiguous(), 0
    if labels.dtype == torch.float32:
        return labels.contiguous(), 1
    raise TypeError("labels must be bool / uint8 / float32, got %s" % labels.dtype)


def xent_fwd(p, labels, weights=None, want_dp=False, eps=XENT_EPS, upstream=1.0):
    _dev(p, labels, weights)
    p = _f32c(p)
    B, V = p.shape
    lab, ldt = _labels_arg(labels)
    if tuple(lab.shape) != (B, V):
        raise ValueError("labels shape %s != predictions shape %s" % (tuple(lab.shape), (B, V)))
    L = _lib.lib()
    ws = torch.empty((L.yt8m_xent_workspace_bytes(B, V) + 3) // 4, dtype=torch.float32, device=p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    dp = torch.empty_like(p) if want_dp else None
    w = None if weights is None else _f32c(weights)
    _lib.check(L.yt8m_xent_fwd_bwd(_p(p), _p(lab), ldt, _p(w), _p(loss), _p(dp), B, V, eps, upstream, _p(ws), _stream()))
    return loss, dp


def xent_bwd(p, labels, weights, upstream_dev, eps=XENT_EPS, upstream=1.0):
    _dev(p, labels, weights, upstream_dev)
    p = _f32c(p)
    B, V = p.shape
    lab, ldt = _labels_arg(labels)
    dp = torch.empty_like(p)
    w = None if weights is None else _f32c(weights)
    up = None if upstream_dev is None else _f32c(upstream_dev)
    _lib.check(_lib.lib().yt8m_xent_bwd(_p(p), _p(lab), ldt, _p(w), _p(up), _p(dp), B, V, eps, upstream, _stream()))
    return dp


def topk_rows(p, k=20):
    _dev(p)
    p = _f32c(p)
    B, V = p.shape
    k = min(k, V)
    vals = torch.empty((B, k), dtype=torch.float32, device=p.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=p.device)
    _lib.check(_lib.lib().yt8m_topk_rows(_p(p), B, V, k, _p(vals), _p(idx), _stream()))
    return vals, idx


def sample_frames(x, num_frames, num_samples, mode, seed, return_index=False):
    """SampleRandomFrames (mode 0) / SampleRandomSequence (mode 1) of W/model_utils.py:23-70 on the device: x [B,F,D] uint8 or
    float32 -> [B,S,D] of the same dtype (the frames are data: no gradient)."""
    _dev(x)
    x = x.contiguous()
    B, F, D = x.shape
    nf = None if num_frames is None else num_frames.to(torch.int32).contiguous().view(-1)
    out = torch.empty((B, num_samples, D), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, num_samples), dtype=torch.int32, device=x.device) if return_index else None
    fn = {torch.uint8: "yt8m_sample_frames_u8", torch.float32: "yt8m_sample_frames_f32"}[x.dtype]
    _lib.check(getattr(_lib.lib(), fn)(_p(x), _p(nf), B, F, D, int(num_samples), int(mode), int(seed), _p(out), _p(idx), _stream()))
    return (out, idx) if return_index else out


class _FramePool(torch.autograd.Function):
    """FramePooling max / average over the sampled frames (W/model_utils.py:72-95); the max gradient is split equally between
    tied maxima like tf.reduce_max's."""

    @staticmethod
    def forward(ctx, x, mode):
        x = _f32c(x)
        _dev(x)
        B, S, C = x.shape
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().yt8m_frame_pool_fwd(_p(x), B, S, C, mode, _p(out), _stream()))
        ctx.save_for_backward(x, out)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, dy):
        x, out = ctx.saved_tensors
        B, S, C = x.shape
        dy = _f32c(dy)
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().yt8m_frame_pool_bwd(_p(x), _p(out), _p(dy), B, S, C, ctx.mode, _p(dx), _stream()))
        return dx, None


def frame_pool(x, method):
    return _FramePool.apply(x, {"max": 0, "average": 1}[method])


class _BatchNorm(torch.autograd.Function):
    """slim.batch_norm(center=True, scale=True) (W/all_frame_models/dbof_model.py:66-71,79-84,103-108) on the
    rows of x [N,C]: yt8m_batchnorm_fwd / _bwd.  Couples the examples of the local batch, like the reference."""

    @staticmethod
    def forward(ctx, x, token, gamma, beta, mm, mv, is_training, eps, decay):
        x = _f32c(x)
        _dev(x)
        N, C = x.shape
        y = torch.empty_like(x)
        mean = torch.empty((C,), dtype=torch.float32, device=x.device)
        rstd = torch.empty((C,), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().yt8m_batchnorm_fwd(_p(x), N, C, _p(gamma.data), _p(beta.data), _p(mm.data), _p(mv.data),
                                                 int(bool(is_training)), float(eps), float(decay), _p(y), _p(mean), _p(rstd), _stream()))
        ctx.save_for_backward(x, mean, rstd)
        ctx.vars = (gamma, beta, bool(is_training))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        gamma, beta, is_training = ctx.vars
        N, C = x.shape
        dy = _f32c(dy)
        L = _lib.lib()
        ws = torch.empty(L.yt8m_batchnorm_workspace_bytes(C) // 4, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gg, gb = gamma.grad, beta.grad
        bg = gamma.grad_beta() if gg is not None else 0.0
        bb = beta.grad_beta() if gb is not None else 0.0
        _lib.check(L.yt8m_batchnorm_bwd(_p(x), _p(dy), N, C, _p(gamma.data), _p(mean), _p(rstd), int(is_training), _p(dx), _p(gg),
                                        float(bg), _p(gb), float(bb), _p(ws), ws.numel() * 4, _stream()))
        if gg is not None:
            gamma.grad_done()
        if gb is not None:
            beta.grad_done()
        return dx, None, None, None, None, None, None, None, None


def batch_norm(x, gamma, beta, moving_mean, moving_variance, is_training, eps=1e-3, decay=0.999):
    return _BatchNorm.apply(x, _token(gamma._graph), gamma, beta, moving_mean, moving_variance, is_training, eps, decay)


def perr_rows(p, labels):
    """Per-video precision at equal recall rate on the device (W/eval_util.py:74-99); labels bool / uint8 [B,V]."""
    _dev(p)
    p = _f32c(p)
    lab = labels.contiguous()
    if lab.dtype == torch.bool:
        lab = lab.view(torch.uint8)
    assert lab.dtype == torch.uint8 and lab.shape == p.shape
    B, V = p.shape
    out = torch.empty((B,), dtype=torch.float32, device=p.device)
    _lib.check(_lib.lib().yt8m_perr_rows(_p(p), _p(lab), B, V, _p(out), _stream()))
    return out


def sqnorm_and_adam(graph, lr_t, gscale=1.0, clip=1.0, beta1=0.9, beta2=0.999, eps=1e-8, tensors=None):
    """Per-tensor clip + TF-Adam over the arena (two multi-tensor passes).  tensors = (lo, hi) restricts the update
    to trainable variables lo..hi-1 (a contiguous slice of the chunk table)."""
    _dev(graph.params)
    L = _lib.lib()
    s = _stream()
    nt = len(graph.trainable_variables())
    lo, hi = (0, nt) if tensors is None else tensors
    if hi <= lo:
        return
    c0, c1 = graph.chunk_start[lo], graph.chunk_start[hi]
    chunks = ctypes.c_void_p(graph.chunks.data_ptr() + 16 * c0)
    partial = ctypes.c_void_p(graph.partial.data_ptr() + 4 * c0)
    if clip > 0:
        _lib.check(L.yt8m_sqnorm_multi(_p(graph.params), _p(graph.grads), chunks, c1 - c0, _p(graph.l2), gscale, partial,
                                       _p(graph.norms), lo, hi - lo, _p(graph.chunk_start_dev), c0, s))
    wi = getattr(graph, "wimg", None)
    tiles = wi is not None and wi.active
    # tensors that own operand images are updated by the tile pass, which rewrites the images where it rewrites the weight
    # (csrc/optim.hip adam_tile_kernel: bitwise the chunk kernel's arithmetic); the chunk pass leaves them alone
    _lib.check(L.yt8m_adam_multi_ex(_p(graph.params), _p(graph.adam_m), _p(graph.adam_v), _p(graph.grads), chunks, c1 - c0,
                                    _p(graph.l2), gscale, _p(graph.norms), clip, lr_t, beta1, beta2, eps,
                                    _p(wi.skip_dev) if tiles else None, s))
    if tiles:
        wi.adam(lo, hi, (gscale, clip, lr_t, beta1, beta2, eps), s)


# ------------------------------------------------------------------------------------------ autograd ops
def _token(graph=None):
    g = graph or get_default_graph()
    if g.token is None:
        g.begin_step()
    return g.token


class _Dropout(torch.autograd.Function):
    """tf.nn.dropout(x, keep_prob) (W/all_video_models/deep_combine_chain_model.py:57-58): x / keep_prob where the Philox
    stream of (seed, offset + element) keeps the element, else 0.  The mask is never stored: backward replays it."""

    @staticmethod
    def forward(ctx, x, keep_prob, seed, offset):
        x = _f32c(x)
        _dev(x)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().yt8m_dropout_f32(_p(x), _p(y), x.numel(), float(keep_prob), int(seed), int(offset), _stream()))
        ctx.args = (float(keep_prob), int(seed), int(offset))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _f32c(dy)
        dx = torch.empty_like(dy)
        keep_prob, seed, offset = ctx.args
        _lib.check(_lib.lib().yt8m_dropout_f32(_p(dy), _p(dx), dy.numel(), keep_prob, seed, offset, _stream()))
        return dx, None, None, None


def dropout(x, keep_prob, seed=None, offset=0, graph=None):
    """seed None: the next key of the graph's random stream (variables.random_seed)."""
    if seed is None:
        seed = (graph or get_default_graph()).next_random_seed()
    return _Dropout.apply(x, keep_prob, seed, offset)


def dropout_(x, keep_prob, seed, offset=0):
    """In place, no autograd (used inside the fused recurrent-stack op)."""
    _dev(x)
    assert x.is_contiguous() and x.dtype == torch.float32
    _lib.check(_lib.lib().yt8m_dropout_f32(_p(x), _p(x), x.numel(), float(keep_prob), int(seed), int(offset), _stream()))
    return x


class _AddNoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stddev, seed, offset):
        x = _f32c(x)
        _dev(x)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().yt8m_add_noise_f32(_p(x), _p(y), x.numel(), float(stddev), int(seed), int(offset), _stream()))
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None, None


def add_noise(x, stddev, seed=None, offset=0, graph=None):
    """x + N(0, stddev^2) (W/all_frame_models/lstm_memory_model.py:62-63); the gradient passes through unchanged."""
    if seed is None:
        seed = (graph or get_default_graph()).next_random_seed()
    return _AddNoise.apply(x, stddev, seed, offset)


BF16_MIN_MACS = 1 << 27      # below this the cast passes cost more than the bf16 MFMAs save
BF16_MIN_ROWS = 512          # a weight matrix is re-cast every step (6 B/element): that only pays when >= ~100 activation
                             # rows share it; 512 keeps a margin (measured: B = 128 NetVLAD hidden FC loses, 1024-row chain wins)


_DensePlan = collections.namedtuple("_DensePlan", "fwd dw dy_dual dx xmax")


def _dense_plan(M, N, K, bf16, layer=True, weight_cast=None, need_dx=True, w_grad=True, w_contiguous=True, dy_contiguous=True):
    """The forms of the three products of a dense layer y [M,N] = x [M,K] . W [K,N] -- forward, dW [K,N] = x^T dy (reduction over the M
    rows), dx [M,K] = dy W^T (reduction over N): the ONE place where they are chosen, in the forward pass; the backward passes dispatch on
    the fields alone (the table is pinned by tests/test_dense_plan_host.py).  Plain integers and booleans only; the knobs are read when
    it is called.  layer: a fully-connected layer (ops.linear, the time-major CNN's products) -- else a hoisted input projection of a
    recurrent layer or a plain product (gemm_any).  weight_cast (default: layer): W is cast to bf16 for each product that reads it.
    need_dx: the input takes a gradient; w_grad: W takes one; w_contiguous, dy_contiguous: what the h2 dx needs of W and dy.
    bf16 operands (bf16 = True, compute_dtype=bfloat16; K-contiguous copies on both sides, fp32 accumulation, fp32 master weights and
    gradients) need an even reduction length (bf16 pairs) and BF16_MIN_MACS of work to pay for the two cast passes; a product that casts
    a weight matrix for itself (weight_cast: the forward and the dx product) also BF16_MIN_ROWS rows to amortise that cast; a hoisted /
    plain product a reduction length >= 32.
    The h2 forms follow one size rule: from LINEAR_H2_MIN_ROWS rows on, or when the product is large whatever the row count
    (LINEAR_H2_MIN_MNK: the NetVLAD / DBoF hidden layers at B = 128 -- K = 73 728 / 8 192 -- gain 12-14 % of their step; small layers do
    not pay the per-call passes over their activations back: cnn_chain +3 % with every layer on it).  A layer takes them wherever its
    bf16 size rule refuses, in the bf16 configuration too; a hoisted product never under bf16 (there the choice is bf16 casts or the
    generic product).
    fwd: "bf16_nt"; "h2" (round 6: the declared h2 role for the FORWARD product, N % 4 == 0 -- the scaled epilogue stores float4 --
         and K >= 512, a shorter reduction is not worth the operand passes: activation x weight, one scale per operand matrix serves
         and the weight's half-plane image is resident, wimg.py; a hoisted projection's input is the l2-normalised frames or a bounded
         recurrent output, three f16 products instead of six bf16 ones); or "auto" (the persistent scheduler's own choice).
    dw:  "bf16_nt" or "auto" (the "dw" role); dy_dual: a layer's dy feeds dW (transposed) and dx (plain) as bf16, so ONE pass casts it
         to both layouts -- exactly when both products are "bf16_nt" and W takes a gradient; hoisted products cast per product.
    dx:  None (need_dx off); "bf16_nt"; "h2_rows" (three f16 products with dy split ROW BY ROW, _linear_dx_h2_rows: one scale per
         matrix does not serve dx, whose dy rows -- time steps -- may differ by decades; N >= 512, K % 4 == 0, W contiguous, and for a
         hoisted product, whose dy may be a column window, dy contiguous); or "auto".
    xmax: a layer on "h2" measures max |x| ONCE: the forward product's split and the weight gradient's split of x^T both take the word.
    Two asymmetries are known and kept as they are: _Linear.backward never calls grad_done(), while _LinearCat, _LinearGroup and the
    recurrent layers do; _LinearGroup has no form choice and does not ask this plan."""
    macs = M * N * K                                       # of each of the three products
    casts = bool(bf16) and macs >= BF16_MIN_MACS           # ... each then asks for its own reduction length: even, >= 32 outside a layer
    shortest = 2 if layer else 32
    rows = M >= BF16_MIN_ROWS or not (layer if weight_cast is None else weight_cast)          # for the products that cast W: forward, dx
    h2_size = (M >= LINEAR_H2_MIN_ROWS or macs >= LINEAR_H2_MIN_MNK) and (layer or not bf16)
    if casts and rows and K % 2 == 0 and K >= shortest:
        fwd = "bf16_nt"
    else:
        fwd = "h2" if (LINEAR_FWD_H2 and h2_size and N % 4 == 0 and K >= 512) else "auto"
    dw = "bf16_nt" if (casts and M % 2 == 0 and M >= shortest) else "auto"
    if not need_dx:
        dx = None
    elif casts and rows and N % 2 == 0 and N >= shortest:
        dx = "bf16_nt"
    else:
        h2_rows = LINEAR_DX_H2 and h2_size and N >= 512 and K % 4 == 0 and w_contiguous and (layer or dy_contiguous)
        dx = "h2_rows" if h2_rows else "auto"
    return _DensePlan(fwd, dw, layer and w_grad and dw == "bf16_nt" and dx == "bf16_nt", dx, layer and fwd == "h2")


def _skinny_plan(M, N, K=None):
    """_dense_plan's sibling for layers with <= 16 outputs over many rows (attention logits).  Without K: ops.linear hands the layer to
    linear_cat; with the K of one full part: that part takes the vector-ALU streaming kernels (csrc/gemm_skinny.hip, float4 rows:
    K % 4 == 0) where the library also has room for its weight image and the operands are aligned (skinny_ok), else the GEMM."""
    return N <= 16 and M >= SKINNY_MIN_ROWS and (K is None or K % 4 == 0)


def _product(form, A, B, out=None, transA=False, transB=False, bias=None, beta=0.0, role=None):
    """C = op(A) . op(B) (+ bias) (+ C) in a form of _dense_plan: "bf16_nt" takes bf16 copies of both operands (each cast into the
    K-contiguous layout the NT kernel wants), "h2" declares that role, "auto" the caller's (None or "dw"); fp32 accumulate / output."""
    if form != "bf16_nt":
        return gemm(A, B, out=out, transA=transA, transB=transB, bias=bias, beta=beta, role="h2" if form == "h2" else role)
    Ab = cast_bf16(A, transpose=transA)                # op(A)   [M, K]
    Bb = cast_bf16(B, transpose=not transB)            # op(B)^T [N, K]
    return gemm_bf16_nt_grouped([dict(A=Ab, B=Bb, out=out, bias=bias, beta=beta)])[0]


class _Linear(torch.autograd.Function):
    """y = x.W (+ b) for a 2-D x.  slim.fully_connected without activation.  The forms of its three GEMMs: _dense_plan."""

    @staticmethod
    def forward(ctx, x, token, W, b, bf16):
        x2 = _f32c(x)
        M, K = x2.shape
        N = W.data.shape[1]
        # (w_grad: a graph makes the gradient slots after its first forward pass, so only `trainable` is known here; backward looks)
        plan = _dense_plan(M, N, K, bf16, need_dx=ctx.needs_input_grad[0], w_grad=W.trainable, w_contiguous=W.data.is_contiguous())
        ctx.xmax = h2_absmax(x2).view(torch.float32) if plan.xmax else None
        if plan.fwd == "bf16_nt":
            y = _product("bf16_nt", x2, W.data, bias=None if b is None else b.data)
        else:
            y = gemm_grouped([dict(A=x2, B=W.data, bias=None if b is None else b.data, absmaxA=ctx.xmax)],
                             role="h2" if plan.fwd == "h2" else None)[0]
        ctx.save_for_backward(x2)
        ctx.W, ctx.b, ctx.plan = W, b, plan
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        W, b, plan = ctx.W, ctx.b, ctx.plan
        dy = _f32c(dy)
        dyb = None
        if W.trainable and W.grad is not None:
            if plan.dw == "bf16_nt":
                if plan.dy_dual:
                    dyb, dyT = cast_bf16_both(dy)
                else:
                    dyT = cast_bf16(dy, transpose=True)
                gemm_bf16_nt_grouped([dict(A=cast_bf16(x, transpose=True), B=dyT, out=W.grad, beta=W.grad_beta())])
                del dyT
            else:
                gemm_grouped([dict(A=x, B=dy, out=W.grad, beta=W.grad_beta(), absmaxA=ctx.xmax)], transA=True, role="dw")
        if b is not None and b.trainable and b.grad is not None:
            colsum(dy, b.grad.view(-1), beta=b.grad_beta())
        dx = None
        if plan.dx == "bf16_nt":
            dx, = gemm_bf16_nt_grouped([dict(A=dyb if dyb is not None else cast_bf16(dy), B=cast_bf16(W.data))])
        elif plan.dx == "h2_rows":
            dx = _linear_dx_h2_rows(dy, W)
        elif plan.dx == "auto":
            dx = gemm(dy, W.data, transB=True)
        return dx, None, None, None, None


class _RowWindow(object):
    """The first rows of a weight matrix as the `W` of _linear_dx_h2_rows (a recurrent layer's input half W[:in] of its [in + H, .] weights)."""
    __slots__ = ("data",)

    def __init__(self, data):
        self.data = data


def hoisted_fwd(x, Wrows, out=None, bias=None, beta=0.0, bf16=False):
    """out [M, N] (+)= x [M, K] . Wrows [K, N] (+ bias): a recurrent layer's hoisted input projection over all time steps (GRU /
    LayerNorm-LSTM / scalar-gate layers outside the native stack), in its plan's forward form."""
    form = _dense_plan(x.shape[0], Wrows.shape[1], x.shape[1], bf16, layer=False, need_dx=False).fwd
    return _product(form, x, Wrows, out=out, bias=bias, beta=beta)


def hoisted_dw(x, dy, out, beta=0.0, bf16=False):
    """out [K, N] (+)= x [M, K]^T . dy [M, N]: that projection's weight gradient."""
    form = _dense_plan(x.shape[0], dy.shape[1], x.shape[1], bf16, layer=False, need_dx=False).dw
    return _product(form, x, dy, out=out, transA=True, beta=beta, role="dw")


def hoisted_dx(dy, Wrows, out=None, beta=0.0, bf16=False):
    """dx [M, K] (+)= dy [M, N] . Wrows [K, N]^T: that projection's input gradient (h2_rows: time steps whose gradients differ by decades
    keep their own precision)."""
    form = _dense_plan(dy.shape[0], dy.shape[1], Wrows.shape[0], bf16, layer=False, w_contiguous=Wrows.is_contiguous(),
                       dy_contiguous=dy.is_contiguous()).dx
    if form == "h2_rows":
        return _linear_dx_h2_rows(dy, _RowWindow(Wrows), out=out, beta=beta)
    return _product(form, dy, Wrows, out=out, transB=True, beta=beta)


def _linear_dx_h2_rows(dy, W, out=None, beta=0.0, row0=0):
    """dx [M, K] = dy [M, N] . W [K, N]^T as three f16 products with dy split ROW BY ROW -- one power of two per row (yt8m_h2_rowscales /
    _split_rows, undone by the product's rowscale): a row of dy whose gradient is decades below the largest keeps its own 22 bits, which
    one scale per matrix would not give it (the form the recurrent stack's dx takes, csrc/lstm_stack.hip).  W as an [K rows, K' = N]
    half-plane image: resident (wimg.py) or made here under its measured maximum.  row0 (a multiple of 32): only the columns [row0, K) of
    dx are computed -- rows [row0, K) of W are whole 32-row groups of its image --, a fresh dx holds zeros in front of them."""
    L = _lib.lib()
    M, N = dy.shape
    K = W.data.shape[0]
    assert row0 % 32 == 0 and 0 <= row0 < K
    dev = dy.device
    S = torch.empty(M, dtype=torch.float32, device=dev)
    inv = torch.empty(M, dtype=torch.float32, device=dev)
    _lib.check(L.yt8m_h2_rowscales(_p(dy), M, N, N, _p(S), _p(inv), _stream()))
    dyi = image_buffer(M, N, 2, dev)
    _lib.check(L.yt8m_h2_split_rows(_p(dy), M, N, N, _p(S), _p(dyi), _stream()))
    wp = ctypes.c_void_p(W.data.data_ptr())
    ptr = L.yt8m_wimg_lookup(wp, K, N, N, 0, 2, 0.0)
    keep = None
    if ptr:
        wimg_p, word_p = ctypes.c_void_p(ptr), ctypes.c_void_p(ptr - 256)          # (the scale word sits in front of a resident image)
    else:
        L.yt8m_wimg_note_demand(wp, K, N, N, 0, 2, 0.0)                            # its owner may keep it resident from the next step on
        word = h2_absmax(W.data)
        wi = image_buffer(K, N, 2, dev)
        _lib.check(L.yt8m_h2_split(wp, K, N, N, 1.0, _p(word), _p(wi), None, None, _stream()))
        keep = (word, wi)
        wimg_p, word_p = _p(wi), _p(word)
    if out is not None:
        dx = out
    else:
        dx = (torch.zeros if row0 else torch.empty)((M, K), dtype=torch.float32, device=dev)
    ws = _workspace(dev)
    if row0:                                                     # (a K block of an h2 image: two 1 KiB half planes)
        wimg_p = ctypes.c_void_p(wimg_p.value + (row0 // 32) * ((N + 15) // 16) * 2048)
    _lib.check(L.yt8m_gemm_h2_nt_ex(M, K - row0, N, _p(dyi), 0, wimg_p, 0, ctypes.c_void_p(dx.data_ptr() + row0 * 4), K, None, 1.0, None,
                                    word_p, _p(inv), float(beta), _p(ws), ws.numel() * 4, _stream()))
    del keep
    return dx


SKINNY_MIN_ROWS = 2048       # below this the padded MFMA tiles are cheap enough


def skinny_ok(M, K, N, *tensors):
    """_skinny_plan's answer for one part, with what the plan does not see: the library's room and the operands' alignment."""
    return bool(_skinny_plan(M, N, K) and _lib.lib().yt8m_skinny_supported(M, K, N)
                and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tensors))


def skinny_fwd(x, W, bias, y, beta=0.0):
    """y[M,N] (+)= x[M,K] . W[K,N] (+ bias); W may be a row slice of a wider-K weight (ld = N)."""
    M, K = x.shape
    N = W.shape[1]
    _lib.check(_lib.lib().yt8m_skinny_fwd_f32(_p(x), x.stride(0), _p(W), W.stride(0), _p(bias), _p(y), y.stride(0), M, K, N,
                                              float(beta), _stream()))
    return y


def skinny_dw(x, dy, dW, beta=0.0):
    M, K = x.shape
    N = dy.shape[1]
    ws = _workspace(x.device)
    _lib.check(_lib.lib().yt8m_skinny_dw_f32(_p(x), x.stride(0), _p(dy), dy.stride(0), _p(dW), dW.stride(0), M, K, N, float(beta),
                                             _p(ws), ws.numel() * 4, _stream()))
    return dW


def skinny_dx(dy, W, dx=None, beta=0.0):
    M, N = dy.shape
    K = W.shape[0]
    if dx is None:
        dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().yt8m_skinny_dx_f32(_p(dy), dy.stride(0), _p(W), W.stride(0), _p(dx), dx.stride(0), M, K, N, float(beta),
                                             _stream()))
    return dx


class _LinearCat(torch.autograd.Function):
    """slim.fully_connected on tf.concat(parts, axis=-1) without materialising the concatenation
    (W/all_frame_models/lstm_attention_max_pooling_model.py:51-56): y = sum_i parts_i . W[rows_i] + b.  W rows are taken in
    part order.  The first `nfull` parts are [M, K_i]; the others are PER-GROUP parts [M / rep, K_i] whose rows stand for
    `rep` consecutive rows of the concatenation each (a per-video vector tiled over the frames, e.g. the mean frame of
    lstm_positional_attention_max_pooling_model.py:77-84): their product is computed once per group and broadcast.
    Narrow outputs (<= 16) over many rows take the streaming kernels (csrc/gemm_skinny.hip)."""

    @staticmethod
    def forward(ctx, token, W, b, rep, nfull, *parts):
        parts = [_f32c(p) for p in parts]
        _dev(*parts)
        M = parts[0].shape[0]
        N = W.data.shape[1]
        assert nfull >= 1 and sum(p.shape[1] for p in parts) == W.data.shape[0], "parts do not add up to the weight's input width"
        y = torch.empty((M, N), dtype=torch.float32, device=parts[0].device)
        _cat_parts_fwd(y, W, 0, parts, [i >= nfull for i in range(len(parts))], rep, written=False, bias=None if b is None else b.data)
        ctx.save_for_backward(*parts)
        ctx.W, ctx.b, ctx.rep, ctx.nfull = W, b, rep, nfull
        return y

    @staticmethod
    def backward(ctx, dy):
        parts = ctx.saved_tensors
        W, b, rep, nfull = ctx.W, ctx.b, ctx.rep, ctx.nfull
        wbeta = W.grad_beta() if (W.trainable and W.grad is not None) else None
        dxs = _cat_parts_bwd(_f32c(dy), W, b, wbeta, 0, parts, [i >= nfull for i in range(len(parts))], rep, ctx.needs_input_grad[5:])
        return (None, None, None, None, None) + tuple(dxs)


def _cat_parts_fwd(y, W, k0, parts, grouped, rep, written=True, bias=None):
    """y [M, N] (+)= sum_i parts_i . W[rows_i], the rows taken from k0 on in part order.  grouped[i]: part i is a per-group part
    [M / rep, K_i], its product computed once per group and broadcast; a full part takes the streaming kernels or the GEMM
    (skinny_ok).  written False: the first part, a full one, starts y and carries the bias; True: every part accumulates."""
    M, N = y.shape
    first = not written
    for p, group in zip(parts, grouped):
        K = p.shape[1]
        Wi = W.data[k0:k0 + K]
        if group:
            assert p.shape[0] * rep == M
            t = gemm(p, Wi)                                           # [M / rep, N]: tiny
            y.view(-1, rep, N).add_(t.view(-1, 1, N))                 # broadcast over the group (layout glue on [M, N])
        elif skinny_ok(M, K, N, p):
            skinny_fwd(p, Wi, bias if first else None, y, beta=0.0 if first else 1.0)
        else:
            gemm(p, Wi, out=y, bias=bias if first else None, beta=0.0 if first else 1.0)
        first = False
        k0 += K


def _cat_parts_bwd(dy, W, b, wbeta, k0, parts, grouped, rep, need_dx):
    """The backward of _cat_parts_fwd from dy [M, N]: per part its rows of W.grad (wbeta: their beta, None: W takes no gradient) and
    its dx (None where need_dx[i] is off), then grad_done() for W and the bias gradient.  -> the dx list."""
    M, N = dy.shape
    dxs = []
    dyg = None
    for p, group, need in zip(parts, grouped, need_dx):
        K = p.shape[1]
        Wi = W.data[k0:k0 + K]
        if group:
            if dyg is None:
                dyg = dy.view(-1, rep, N).sum(dim=1)                  # [M / rep, N]
            if wbeta is not None:
                gemm(p, dyg, out=W.grad[k0:k0 + K], transA=True, beta=wbeta, role="dw")
            dxs.append(gemm(dyg, Wi, transB=True) if need else None)
        else:
            sk = skinny_ok(M, K, N, p, dy)
            if wbeta is not None:
                if sk:
                    skinny_dw(p, dy, W.grad[k0:k0 + K], beta=wbeta)
                else:
                    gemm(p, dy, out=W.grad[k0:k0 + K], transA=True, beta=wbeta, role="dw")
            dxs.append((skinny_dx(dy, Wi) if sk else gemm(dy, Wi, transB=True)) if need else None)
        k0 += K
    if wbeta is not None:
        W.grad_done()
    if b is not None and b.trainable and b.grad is not None:
        colsum(dy, b.grad.view(-1), beta=b.grad_beta())
        b.grad_done()
    return dxs


def linear_cat(parts, W, b=None, group_parts=()):
    """parts: tensors [..., K_i] with equal leading dims; group_parts: tensors [G, K_j] with G * rep = number of rows, each row
    standing for `rep` consecutive rows (appended after `parts` in the concatenation order)."""
    lead = parts[0].shape[:-1]
    flat = [p.reshape(-1, p.shape[-1]) for p in parts]
    rep = 1
    if group_parts:
        rep = flat[0].shape[0] // group_parts[0].shape[0]
    y = _LinearCat.apply(_token(W._graph), W, b, rep, len(flat), *flat, *group_parts)
    return y.view(*lead, y.shape[-1])


def linear(x, W, b=None, bf16=None):
    """Rank-N input is flattened on the leading dims like slim.fully_connected."""
    if _skinny_plan(x.numel() // x.shape[-1], W.data.shape[1]):
        return linear_cat([x], W, b)
    lead = x.shape[:-1]
    if bf16 is None:
        bf16 = FLAGS.compute_dtype == "bfloat16"
    y = _Linear.apply(x.reshape(-1, x.shape[-1]), _token(W._graph), W, b, bool(bf16))
    return y.view(*lead, y.shape[-1])


class _VarTensor(torch.autograd.Function):
    """A Variable used as a plain tensor in layout glue (tile / concat), e.g. the positional embedding of
    W/all_frame_models/lstm_positional_attention_max_pooling_model.py:68-76: forward hands out the parameter, backward
    lands the gradient in the arena slice (beta 0/1 like every other op)."""

    @staticmethod
    def forward(ctx, token, var):
        ctx.var = var
        return var.data.view_as(var.data)

    @staticmethod
    def backward(ctx, g):
        var = ctx.var
        if var.grad is not None and g is not None:
            if var.grad_beta() == 0.0:
                var.grad.copy_(g.view_as(var.grad))
            else:
                var.grad.add_(g.view_as(var.grad))
            var.grad_done()
        return None, None


def as_tensor(var):
    return _VarTensor.apply(_token(var._graph), var)


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        y = act_fwd(kind, x)
        ctx.kind = kind
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return act_bwd(ctx.kind, y, dy), None


def activation(x, kind):
    return _Act.apply(x, kind)


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = _f32c(x)
        ctx.save_for_backward(x)
        ctx.eps = eps
        return l2norm_fwd(x, eps)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return l2norm_bwd(x, dy, ctx.eps), None


def l2_normalize(x, eps=1e-12):
    """tf.nn.l2_normalize on the last axis (differentiable)."""
    return _L2Norm.apply(x, eps)


CHAIN_LINK_FUSED = os.environ.get("YT8M_CHAIN_LINK_FUSED", "1") != "0"   # 0: chain_link composes the three existing ops (A/B runs, tests)


class _ChainLink(torch.autograd.Function):
    """csrc/chain_link.hip: relu / elu, optional noise and l2_normalize of a pre-activation in one pass each way.  Saved for backward:
    z (the linear's output), y (the next stage's input) and rinv [rows]."""

    @staticmethod
    def forward(ctx, z, kind, stddev, seed, offset, eps):
        z = _f32c(z)
        _dev(z)
        cols = z.shape[-1]
        rows = z.numel() // max(cols, 1)
        y = torch.empty_like(z)
        rinv = torch.empty(rows, dtype=torch.float32, device=z.device)
        _lib.check(_lib.lib().yt8m_chain_link_fwd(ACT[kind], _p(z), _p(y), _p(rinv), rows, cols, float(eps), float(stddev), int(seed),
                                                  int(offset), _stream()))
        ctx.kind, ctx.eps = kind, float(eps)
        ctx.save_for_backward(z, y, rinv)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, y, rinv = ctx.saved_tensors
        dy = _f32c(dy)
        dz = torch.empty_like(z)
        _lib.check(_lib.lib().yt8m_chain_link_bwd(ACT[ctx.kind], _p(z), _p(y), _p(rinv), _p(dy), _p(dz), rinv.numel(), z.shape[-1],
                                                  ctx.eps, _stream()))
        return dz, None, None, None, None, None


def chain_link(z, kind="relu", noise_level=None, seed=None, offset=0, eps=1e-12, graph=None):
    """l2_normalize(add_noise(activation(z, kind), noise_level)) on the last axis: one "link" of the chain / distillchain plugins
    (W/all_video_models/distillchain_deep_combine_chain_model.py:27-56).  kind: "relu" or "elu".  noise_level None or 0: no noise and
    no seed is taken; otherwise seed None takes the next key of the graph's random stream, as add_noise does.
    YT8M_CHAIN_LINK_FUSED=0 (read at import): the three existing ops instead of the fused kernel."""
    if kind not in ("relu", "elu"):
        raise ValueError("chain_link: kind must be relu or elu, got %r" % (kind,))
    noisy = noise_level is not None and float(noise_level) != 0.0
    if noisy and seed is None:
        seed = (graph or get_default_graph()).next_random_seed()
    if not CHAIN_LINK_FUSED:
        a = activation(z, kind)
        if noisy:
            a = add_noise(a, noise_level, seed, offset)
        return l2_normalize(a, eps)
    return _ChainLink.apply(z, kind, float(noise_level) if noisy else 0.0, seed if noisy else 0, offset, eps)


# 0 (the default): memory_link composes torch.cat and l2_normalize; anything else: the fused kernel.  Composed is the default because
# tools/multilstm_step.py measured it faster on the host without normalize (a cat and slice views against two launches through a Python
# autograd Function), and whole steps do not move either way (DESIGN_LOG.md section 23).
MEMORY_LINK_FUSED = os.environ.get("YT8M_MEMORY_LINK_FUSED", "0") != "0"


class _MemoryLink(torch.autograd.Function):
    """csrc/memory_link.hip: the concatenation of [B, w_s] tensors along the columns and, with normalize, l2_normalize of the result, in
    one pass each way.  Saved for backward with normalize: y (the next stage's input) and rinv [rows]; without: nothing."""

    @staticmethod
    def forward(ctx, normalize, eps, *tensors):
        srcs = [_f32c(t) for t in tensors]
        _dev(*srcs)
        rows = srcs[0].shape[0]
        for t in srcs:
            if t.dim() != 2 or t.shape[0] != rows:
                raise ValueError("memory_link: every tensor must be [%d, width], got %s" % (rows, tuple(t.shape)))
        n = len(srcs)
        widths = (ctypes.c_int64 * n)(*[t.shape[1] for t in srcs])
        y = torch.empty((rows, sum(t.shape[1] for t in srcs)), dtype=torch.float32, device=srcs[0].device)
        rinv = torch.empty(rows, dtype=torch.float32, device=y.device) if normalize else None
        _lib.check(_lib.lib().yt8m_memory_link_fwd(n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs]), widths, int(normalize), _p(y),
                                                   _p(rinv), rows, float(eps), _stream()))
        ctx.normalize, ctx.eps, ctx.widths = bool(normalize), float(eps), widths
        if normalize:
            ctx.save_for_backward(y, rinv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, rinv = ctx.saved_tensors if ctx.normalize else (None, None)
        dy = _f32c(dy)
        n = len(ctx.widths)
        grads = [torch.empty((dy.shape[0], ctx.widths[s]), dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[2 + s] else None
                 for s in range(n)]
        _lib.check(_lib.lib().yt8m_memory_link_bwd(n, ctx.widths, int(ctx.normalize), _p(y), _p(rinv), _p(dy),
                                                   (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in grads]),
                                                   dy.shape[0], ctx.eps, _stream()))
        return (None, None) + tuple(grads)


def memory_link(tensors, normalize, eps=1e-12):
    """[B, sum w_s]: the [B, w_s] tensors side by side and, with normalize, l2-normalised along the row -- what turns the final memories of
    the multi-LSTM chain plugins' stacks into a stage's classifier input (W/all_frame_models/lstm_memory_deep_chain_model.py:72,
    distillchain_lstm_memory_deep_combine_chain_model.py:57,74).  1 to 16 tensors.  The backward pass hands every input one contiguous
    gradient of its own (the stack's dc_final operands).
    YT8M_MEMORY_LINK_FUSED (read at import): 0, the default, is torch.cat and ops.l2_normalize; 1 is the fused kernel."""
    tensors = list(tensors)
    if not 1 <= len(tensors) <= 16:
        raise ValueError("memory_link: 1 to 16 tensors, got %d" % len(tensors))
    if not MEMORY_LINK_FUSED:
        cat = torch.cat(tensors, dim=1)
        return l2_normalize(cat, eps) if normalize else cat
    return _MemoryLink.apply(bool(normalize), eps, *tensors)


# 0 (the default): scale_mix composes torch.stack, softmax, multiply and sum; anything else: the fused kernels of csrc/scale_mix.hip.
# Composed is the default until tools/scale_mix_step.py's op leg has shown the kernels' median below the composed form's at every shape in
# both runs: nobody has measured it on an MI355X yet (DESIGN_LOG.md section 35).
SCALE_MIX_FUSED = os.environ.get("YT8M_SCALE_MIX_FUSED", "0") != "0"
SCALE_MIX_MAX = 8                                    # csrc/scale_mix.hip MAX_L
SCALE_MIX_CALLS = {"kernels": 0, "composed": 0}      # which form ran (tests)


def scale_mix_composed(ps, zs):
    """sum_l softmax_l(z_l) p_l in torch ops, in the dtype of the inputs."""
    return (torch.softmax(torch.stack(list(zs), dim=0), dim=0) * torch.stack(list(ps), dim=0)).sum(dim=0)


def _ptr_table(tensors):
    """A host array of device pointers (NULL for None), as the C ABI's `float* const*` arguments take it."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class _ScaleMix(torch.autograd.Function):
    """csrc/scale_mix.hip: the per-label softmax over the scales and the weighted sum of the sub-predictions in one pass each way.  Saved
    for backward: the 2 L planes and out."""

    @staticmethod
    def forward(ctx, L, *planes):
        planes = [_f32c(t) for t in planes]
        _dev(*planes)
        rows, cols = planes[0].shape
        out = torch.empty((rows, cols), dtype=torch.float32, device=planes[0].device)
        ctx.L = L
        ctx.save_for_backward(out, *planes)
        _lib.check(_lib.lib().yt8m_scale_mix_fwd(L, _ptr_table(planes[:L]), _ptr_table(planes[L:]), _p(out), rows, cols, _stream()))
        return out

    @staticmethod
    def backward(ctx, g):
        out, *planes = ctx.saved_tensors
        L = ctx.L
        g = _f32c(g)
        want = [k for k in range(2 * L) if ctx.needs_input_grad[1 + k]]
        slab = torch.empty((len(want),) + tuple(out.shape), dtype=torch.float32, device=out.device)       # one allocation for every gradient
        grads = [None] * (2 * L)
        for i, k in enumerate(want):
            grads[k] = slab[i]
        _lib.check(_lib.lib().yt8m_scale_mix_bwd(L, _ptr_table(planes[:L]), _ptr_table(planes[L:]), _p(out), _p(g), _ptr_table(grads[:L]),
                                                 _ptr_table(grads[L:]), out.shape[0], out.shape[1], _stream()))
        return (None,) + tuple(grads)


def scale_mix(ps, zs):
    """out [B,V] = sum_l softmax over l of z_l [B,V] times p_l [B,V]: the LstmMultiscale plugins' per-label mix of their scales' sub-
    predictions (Z/frame_level_models.py:2982-2985: tf.stack, tf.nn.softmax(dim=1), multiply, reduce_sum).  ps: L tensors [B,V]; zs: L
    tensors [B,V] or one [L,B,V] tensor (taken apart into its L planes, no copy).  Differentiable in every plane.
    YT8M_SCALE_MIX_FUSED (read at import): 0, the default, is the composed torch form; 1 is the fused kernel pair, which CPU tensors,
    non-float32 tensors, L > 8 and shapes yt8m_scale_mix_supported refuses never take."""
    ps = list(ps)
    zs = list(zs.unbind(0)) if torch.is_tensor(zs) else list(zs)
    L = len(ps)
    if L < 1 or len(zs) != L:
        raise ValueError("scale_mix: L >= 1 sub-predictions and as many mix logits, got %d and %d" % (L, len(zs)))
    shape = tuple(ps[0].shape)
    if len(shape) != 2 or any(tuple(t.shape) != shape for t in ps + zs):
        raise ValueError("scale_mix: every plane must be [B, V] = %s" % (shape,))
    fused = (SCALE_MIX_FUSED and L <= SCALE_MIX_MAX and all(t.is_cuda and t.dtype == torch.float32 for t in ps + zs)
             and bool(_lib.lib().yt8m_scale_mix_supported(L, shape[0], shape[1])))
    SCALE_MIX_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return scale_mix_composed(ps, zs)
    return _ScaleMix.apply(L, *ps, *zs)


# 0 (the default): distill_input / distill_blend compose the existing ops and torch glue; anything else: the kernels of
# csrc/distill_head.hip.  A kernel is the default only where tools/distill_head_step.py's `kernels` leg has shown its median below the
# composed form's at every shape in both runs; neither did: distill_input in 13 rows of 14 (2.6-2.8x in the Norm2 mode, level with a relu
# and a cat in the Chain mode), distill_blend in 2 of 8 (two multiplies and an add beat a Python autograd Function on the host).  Whole
# steps move by at most 0.06 ms either way (DESIGN_LOG.md section 39).
DISTILL_INPUT_FUSED = os.environ.get("YT8M_DISTILL_INPUT_FUSED", "0") != "0"
DISTILL_BLEND_FUSED = os.environ.get("YT8M_DISTILL_BLEND_FUSED", "0") != "0"
DISTILL_CALLS = {"input_kernels": 0, "input_composed": 0, "blend_kernels": 0, "blend_composed": 0}      # which form ran (tests)
# mode -> (l2-normalise x, relu, divide by the row sum of t[:, v0:], l2-normalise the class part): the heads of Z/video_level_models.py
DISTILL_MODES = {"chain": (False, True, False, False), "norm": (True, False, True, True), "norm2": (True, True, True, True),
                 "split": (False, True, False, False)}


def _distill_mode_bits(mode):
    norm_x, relu, div, norm_c = DISTILL_MODES[mode]
    return int(norm_x) | int(relu) << 1 | int(div) << 2 | int(norm_c) << 3       # enum yt8m_distill_mode


def distill_input_composed(x, z, t, mode, v0=0, eps=1e-12):
    """distill_input as activation, a torch sum and divide, l2_normalize and torch.cat."""
    norm_x, relu, div, norm_c = DISTILL_MODES[mode]
    a = activation(z, "relu") if relu else z
    if div:
        s = t[:, v0:].sum(dim=1, keepdim=True).to(a.dtype)
        live = s != 0                                                     # a zero-sum row: zeros, and a zero gradient for its z
        a = a / torch.where(live, s, torch.ones_like(s)) * live.to(a.dtype)
    return torch.cat([l2_normalize(x, eps) if norm_x else x, l2_normalize(a, eps) if norm_c else a], dim=1)


class _DistillInput(torch.autograd.Function):
    """csrc/distill_head.hip: the head input [x' | class part] in one pass each way.  Saved for backward: z (the linear's output), y (the
    MoE block's input) and the three per-row scalars."""

    @staticmethod
    def forward(ctx, x, z, t, bits, v0, eps):
        x, z = _f32c(x), _f32c(z)
        t, ldt = _rowmajor2d(t)
        _dev(x, z, t)
        rows, D = x.shape
        C = z.shape[1]
        y = torch.empty((rows, D + C), dtype=torch.float32, device=x.device)
        stats = torch.empty((3, rows), dtype=torch.float32, device=x.device)             # rx, rc, 1 / s
        _lib.check(_lib.lib().yt8m_distill_input_fwd(bits, _p(x), _p(z), _p(t), ldt, int(v0), t.shape[1], _p(y), _p(stats[0]), _p(stats[1]),
                                                     _p(stats[2]), rows, D, C, float(eps), _stream()))
        ctx.bits, ctx.D = bits, D
        ctx.save_for_backward(z, y, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, y, stats = ctx.saved_tensors
        dy = _f32c(dy)
        rows, C = z.shape
        dx = torch.empty((rows, ctx.D), dtype=torch.float32, device=z.device) if ctx.needs_input_grad[0] else None
        dz = torch.empty_like(z)
        _lib.check(_lib.lib().yt8m_distill_input_bwd(ctx.bits, _p(z), _p(y), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(dy), _p(dx), _p(dz),
                                                     rows, ctx.D, C, _stream()))
        return dx, dz, None, None, None, None


def distill_input(x, z, t, mode, v0=0, eps=1e-12):
    """[B, D + C]: the input of the MoeDistillChain* / MoeDistillSplit heads' MoE block (Z/video_level_models.py:316-324, :389-399,
    :464-474, :541-550) from the head's features x [B, D], z = t_window W + b [B, C] (ops.linear under "class_inputs") and another
    model's predictions t [B, V], which are data.  mode (DISTILL_MODES): "chain" and "split" [x | relu(z)]; "norm"
    [l2norm(x) | l2norm(z / sum_v t[:, v0:])]; "norm2" the same with relu before the division.  A row whose t sums to exactly 0 (0 / 0 in
    the reference) gets a class part of zeros and a zero gradient for its z.  Differentiable in x and z.
    YT8M_DISTILL_INPUT_FUSED (read at import): 0, the default, is the composed form (distill_input_composed); 1 is the fused kernel
    pair, which CPU tensors, non-float32 tensors and shapes yt8m_distill_input_supported refuses never take."""
    if mode not in DISTILL_MODES:
        raise ValueError("distill_input: mode must be one of %s, got %r" % (sorted(DISTILL_MODES), mode))
    if x.dim() != 2 or z.dim() != 2 or t.dim() != 2 or not (x.shape[0] == z.shape[0] == t.shape[0]) or not 0 <= v0 < t.shape[1]:
        raise ValueError("distill_input: x [B, D], z [B, C], t [B, V] and 0 <= v0 < V, got %s, %s, %s, v0 = %d"
                         % (tuple(x.shape), tuple(z.shape), tuple(t.shape), v0))
    t = t.detach()
    fused = (DISTILL_INPUT_FUSED and x.shape[0] > 0 and all(a.is_cuda and a.dtype == torch.float32 for a in (x, z, t))
             and bool(_lib.lib().yt8m_distill_input_supported(x.shape[1], z.shape[1], t.shape[1])))
    DISTILL_CALLS["input_kernels" if fused else "input_composed"] += 1
    if not fused:
        return distill_input_composed(x, z, t, mode, v0, eps)
    return _DistillInput.apply(x, z, t, _distill_mode_bits(mode), v0, eps)


def distill_blend_composed(p1, t, w):
    """distill_blend as torch.cat, two multiplies and an add, 1 - w formed in fp32."""
    w32 = torch.tensor(w, dtype=torch.float32)
    V1 = p1.shape[1]
    both = p1 if V1 == t.shape[1] else torch.cat([p1, t[:, V1:]], dim=1)
    return both * float(w32) + t * float(1.0 - w32)


class _DistillBlend(torch.autograd.Function):
    """csrc/distill_head.hip: concat(p1, t[:, V1:]) * w + t * (1 - w) in one pass each way.  Nothing is saved for backward."""

    @staticmethod
    def forward(ctx, p1, t, w):
        p1 = _f32c(p1)
        t, ldt = _rowmajor2d(t)
        _dev(p1, t)
        rows, V = t.shape
        out = torch.empty((rows, V), dtype=torch.float32, device=t.device)
        _lib.check(_lib.lib().yt8m_distill_blend_fwd(_p(p1), _p(t), ldt, _p(out), rows, V, p1.shape[1], float(w), _stream()))
        ctx.w, ctx.V1 = float(w), p1.shape[1]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _f32c(dout)
        rows, V = dout.shape
        dp1 = torch.empty((rows, ctx.V1), dtype=torch.float32, device=dout.device)
        _lib.check(_lib.lib().yt8m_distill_blend_bwd(_p(dout), _p(dp1), rows, V, ctx.V1, ctx.w, _stream()))
        return dp1, None, None


def distill_blend(p1, t, w, bound):
    """[B, V] = concat(p1 [B, bound], t[:, bound:]) * w + t * (1 - w): the last line of the MoeDistillChain* / MoeDistillSplit heads
    (Z/video_level_models.py:355, :578-580), w = --ensemble_w, bound = the number of labels the head predicts itself (V for the Chain
    heads).  t is data; 1 - w is formed in fp32.  With w == 1.0 and bound == V -- the Chain heads' training setting -- the op returns p1
    ITSELF: the reference's p * 1.0 + t * 0.0 equals p bit for bit for finite t.
    YT8M_DISTILL_BLEND_FUSED (read at import): 0, the default, is the composed form (distill_blend_composed); 1 is the fused kernel pair,
    which CPU tensors, non-float32 tensors and shapes yt8m_distill_blend_supported refuses never take."""
    if p1.dim() != 2 or t.dim() != 2 or p1.shape[0] != t.shape[0] or p1.shape[1] != bound or not 0 < bound <= t.shape[1]:
        raise ValueError("distill_blend: p1 [B, bound], t [B, V] and 0 < bound <= V, got %s, %s, bound = %d"
                         % (tuple(p1.shape), tuple(t.shape), bound))
    if float(w) == 1.0 and bound == t.shape[1]:
        return p1
    t = t.detach()
    fused = (DISTILL_BLEND_FUSED and p1.shape[0] > 0 and p1.is_cuda and t.is_cuda and p1.dtype == t.dtype == torch.float32
             and bool(_lib.lib().yt8m_distill_blend_supported(t.shape[0], t.shape[1], bound)))
    DISTILL_CALLS["blend_kernels" if fused else "blend_composed"] += 1
    if not fused:
        return distill_blend_composed(p1, t, w)
    return _DistillBlend.apply(p1, t, w)


# YT8M_MIX_LINK_FUSED, 0: mix_link composes the existing ops in the reference's order; anything else (the default): one product and the
# kernels of csrc/mix_link.hip.  Fused is the default because tools/mix_chain_step.py's op leg measured its median below the composed
# form's at every one of the four shapes in both runs of the leg, 1.4 - 1.9 x (DESIGN_LOG.md section 40).  The form with a given q
# (MoeKnowledgeModel) has a switch of its own, YT8M_MIX_LINK_FUSED_Q, and stays composed by default: its row was below the composed form's
# in one run of two (320 against 375 us, then 451 against 433 on a noisy machine), and its whole step is level.
MIX_LINK_FUSED = os.environ.get("YT8M_MIX_LINK_FUSED", "1") != "0"
MIX_LINK_FUSED_Q = os.environ.get("YT8M_MIX_LINK_FUSED_Q", "0") != "0"
MIX_LINK_CALLS = {"kernels": 0, "composed": 0}       # which form ran (tests)
MIX_LINK_PLAIN, MIX_LINK_NONE = _C["YT8M_MIX_LINK_PLAIN"], _C["YT8M_MIX_LINK_NONE"]      # enum yt8m_mix_link_mode


def mix_link_composed(prev, p, W1, b1, W2, b2, q=None, norm=True, scale=1.0, eps=1e-12):
    """mix_link as the reference writes it: two products on p and on a materialised 1 - p (or on q), two elu passes, two
    l2-normalisations with a scale and torch.cat."""
    c1 = activation(linear(p, W1, b1), "elu")
    c2 = activation(linear((1.0 - p) if q is None else q, W2, b2), "elu")
    if norm:
        c1, c2 = l2_normalize(c1, eps) * scale, l2_normalize(c2, eps) * scale
    return torch.cat([prev, c1, c2], dim=1)


class _MixProduct(torch.autograd.Function):
    """The host's half of a fused mix_link in the complement mode: z [rows, 2 C] = x . [W1 | W2], ONE product without biases, and
    u [2 C] = [b1 | colsum(W2) + b2], the column sum taken in float64 and rounded once, so that the kernel's u2 - z2 is
    (1 - x) . W2 + b2.  Backward: the weight gradients x^T . dz as one grouped launch into the Variables' arena slots, the biases' from
    du, colsum(W2)'s share du2 broadcast onto W2's gradient, and dx as ONE product dz . [W1 | W2]^T (the complement's sign is already
    in dz)."""

    @staticmethod
    def forward(ctx, token, W1, b1, W2, b2, x):
        x = _f32c(x)
        Wcat = torch.cat([W1.data, W2.data], dim=1)
        z = gemm(x, Wcat)
        u2 = (W2.data.sum(dim=0, dtype=torch.float64) + b2.data.double()).float()
        ctx.save_for_backward(x, Wcat)
        ctx.vars = (W1, b1, W2, b2)
        return z, torch.cat([b1.data.view(-1), u2.view(-1)])

    @staticmethod
    def backward(ctx, dz, du):
        W1, b1, W2, b2 = ctx.vars
        x, Wcat = ctx.saved_tensors
        dz, du = _f32c(dz), _f32c(du)
        C = W1.data.shape[1]
        dx = gemm(dz, Wcat, transB=True) if ctx.needs_input_grad[5] else None
        items = [dict(A=x, B=dz[:, k * C:(k + 1) * C], out=W.grad, beta=W.grad_beta())
                 for k, W in enumerate((W1, W2)) if W.trainable and W.grad is not None]
        if items:
            gemm_grouped(items, transA=True, role="dw")
        if W2.trainable and W2.grad is not None:
            W2.grad.add_(du[C:])                                          # colsum(W2) reaches every row of W2 alike
        for b, g in ((b1, du[:C]), (b2, du[C:])):
            if b.trainable and b.grad is not None:
                if b.grad_beta() == 0.0:
                    b.grad.view(-1).copy_(g)
                else:
                    b.grad.view(-1).add_(g)
        return None, None, None, None, None, dx


class _MixLink(torch.autograd.Function):
    """csrc/mix_link.hip: [prev | y1 | y2] from z and u in one pass each way.  Saved for backward: z, u and stats [2, rows]."""

    @staticmethod
    def forward(ctx, prev, z, u, bits, scale, dx_from, eps):
        prev, z, u = _f32c(prev), _f32c(z), _f32c(u)
        _dev(prev, z, u)
        rows, Wprev = prev.shape
        C = z.shape[1] // 2
        out = torch.empty((rows, Wprev + 2 * C), dtype=torch.float32, device=prev.device)
        stats = torch.empty((2, rows), dtype=torch.float32, device=prev.device)
        _lib.check(_lib.lib().yt8m_mix_link_fwd(bits, _p(prev), _p(z), _p(u), _p(out), _p(stats), rows, Wprev, C, float(scale), float(eps),
                                                _stream()))
        ctx.bits, ctx.scale, ctx.Wprev, ctx.dx_from = bits, float(scale), Wprev, int(dx_from)
        ctx.save_for_backward(z, u, stats)
        return out

    @staticmethod
    def backward(ctx, dy):
        z, u, stats = ctx.saved_tensors
        dy = _f32c(dy)
        rows, C = z.shape[0], z.shape[1] // 2
        dprev = None
        if ctx.needs_input_grad[0]:                                       # the data columns in front hold zeros
            dprev = (torch.zeros if ctx.dx_from else torch.empty)((rows, ctx.Wprev), dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        _lib.check(_lib.lib().yt8m_mix_link_bwd(ctx.bits, _p(z), _p(u), _p(stats), _p(dy), _p(dprev), _p(dz), rows, ctx.Wprev, C, ctx.dx_from,
                                                ctx.scale, _stream()))
        du = colsum(dz, torch.empty(2 * C, dtype=torch.float32, device=z.device))
        if not ctx.bits & MIX_LINK_PLAIN:
            du[C:].neg_()                                                 # dz2 carries the complement's sign, u2's gradient does not
        return dprev, dz, du, None, None, None, None


def mix_link(prev, p, W1, b1, W2, b2, q=None, norm=True, scale=1.0, dx_from=0, eps=1e-12):
    """[rows, Wprev + 2 C]: the input of the next MoE stage of the MoeMix4 / MoeKnowledge heads (Z/video_level_models.py:1997-2013,
    :1391-1407) from the previous stage's input prev [rows, Wprev] and its prediction p [rows, V]:
        c1 = elu(p . W1 + b1);  c2 = elu((1 - p) . W2 + b2), or elu(q . W2 + b2) for a given q [rows, K] (MoeKnowledge: q = p . seq);
        norm: c_k = l2_normalize(c_k) * scale;  out = [prev | c1 | c2].
    W1, b1, W2, b2 are Variables (class_inputs1-<i>, class_inputs2-<i>).  dx_from: the leading columns of prev that are data (no
    gradient is computed for them; the returned gradient holds zeros there).
    YT8M_MIX_LINK_FUSED (read at import): 1, the default, is one product z = p . [W1 | W2] and the fused kernel pair, where the
    complement is u2 - z2 with u2 = colsum(W2) + b2 and no 1 - p tensor exists; 0 is the composed form (mix_link_composed).  With q
    the switch is YT8M_MIX_LINK_FUSED_Q, 0 by default: the composed form, 1: the two products, then the kernel pair.  CPU tensors,
    non-float32 tensors and shapes yt8m_mix_link_supported refuses (C > 1024) always take the composed form."""
    C = W1.data.shape[1]
    if prev.dim() != 2 or p.dim() != 2 or prev.shape[0] != p.shape[0] or (q is not None and (q.dim() != 2 or q.shape[0] != p.shape[0])) \
            or tuple(W2.data.shape) != ((p if q is None else q).shape[1], C) or W1.data.shape[0] != p.shape[1] or not 0 <= dx_from <= prev.shape[1]:
        raise ValueError("mix_link: prev [rows, Wprev], p [rows, V], q [rows, K] or None, W1 [V, C], W2 [V or K, C] and 0 <= dx_from <= Wprev, "
                         "got %s, %s, %s, %s, %s, dx_from = %d" % (tuple(prev.shape), tuple(p.shape), None if q is None else tuple(q.shape),
                                                                  tuple(W1.data.shape), tuple(W2.data.shape), dx_from))
    fused = ((MIX_LINK_FUSED if q is None else MIX_LINK_FUSED_Q) and prev.shape[0] > 0 and all(t.is_cuda and t.dtype == torch.float32 for t in (prev, p) + (() if q is None else (q,)))
             and bool(_lib.lib().yt8m_mix_link_supported(prev.shape[1], C)))
    MIX_LINK_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return mix_link_composed(prev, p, W1, b1, W2, b2, q, norm, scale, eps)
    if q is None:
        z, u = _MixProduct.apply(_token(W1._graph), W1, b1, W2, b2, p)
    else:                                                                 # two inputs: the composed form's own two products
        z, u = torch.cat([linear(p, W1), linear(q, W2)], dim=1), torch.cat([as_tensor(b1), as_tensor(b2)])
    bits = (0 if q is None else MIX_LINK_PLAIN) | (0 if norm else MIX_LINK_NONE)
    return _MixLink.apply(prev, z, u, bits, scale, dx_from, eps)


# YT8M_SOFTMAX_MOE_FUSED, 0: softmax_moe composes torch ops in the reference's order; anything else: the kernels of csrc/softmax_moe.hip.
# YT8M_SPLIT_SOFTMAX_LOSS_FUSED: the same for split_softmax_loss.  Each default follows the project's rule on its own -- the kernels only
# where tools/softmax_moe_step.py measured their median below the composed form's at every shape in both runs.  Both did: the block
# 1.4 - 4.1 x at its four shapes, the loss 3.4 - 5.6 x at its two (DESIGN_LOG.md section 42), so both defaults are 1.
SOFTMAX_MOE_FUSED = os.environ.get("YT8M_SOFTMAX_MOE_FUSED", "1") != "0"
SPLIT_SOFTMAX_LOSS_FUSED = os.environ.get("YT8M_SPLIT_SOFTMAX_LOSS_FUSED", "1") != "0"
SOFTMAX_MOE_CALLS = {"kernels": 0, "composed": 0}                # which form ran (tests)
SPLIT_SOFTMAX_LOSS_CALLS = {"kernels": 0, "composed": 0}
SOFTMAX_LOSS_EPS = 10e-8  # Z/losses.py:428


def softmax_moe_composed(Zg, Ze, S, M, head=None):
    """softmax_moe as the reference writes it (Z/video_level_models.py:941-957): two softmaxes -- over the M + 1 gates and, per mixture,
    over the S labels --, the product's sum over the mixtures, the division by the row sum, the last label dropped and torch.cat."""
    rows = Zg.shape[0]
    g = torch.softmax(Zg.reshape(rows, S, M + 1), dim=2)
    e = torch.softmax(Ze.reshape(rows, S, M), dim=1)
    p = (g[:, :, :M] * e).sum(dim=2)
    q = (p / p.sum(dim=1, keepdim=True))[:, :-1]
    return q if head is None else torch.cat([head, q], dim=1)


class _SoftmaxMoe(torch.autograd.Function):
    """csrc/softmax_moe.hip: the whole prediction row [head | q] from the two logit matrices in one launch each way.  Saved for backward:
    Zg, Ze and stats [rows, 2 M + 1].  overwrite: the backward pass writes dZg / dZe over the logits (the model's own, which nothing else
    reads); otherwise into fresh tensors."""

    @staticmethod
    def forward(ctx, Zg, Ze, head, S, M, overwrite):
        Zg, Ze = _f32c(Zg), _f32c(Ze)
        head = None if head is None else _f32c(head)
        _dev(Zg, Ze, head)
        rows = Zg.shape[0]
        V1 = 0 if head is None else head.shape[1]
        out = torch.empty((rows, V1 + S - 1), dtype=torch.float32, device=Zg.device)
        stats = torch.empty((rows, 2 * M + 1), dtype=torch.float32, device=Zg.device)
        _lib.check(_lib.lib().yt8m_softmax_moe_fwd(_p(Zg), _p(Ze), _p(head), _p(out), _p(stats), rows, S, M, V1, _stream()))
        ctx.S, ctx.M, ctx.V1, ctx.overwrite = S, M, V1, bool(overwrite)
        ctx.save_for_backward(Zg, Ze, stats)
        return out

    @staticmethod
    def backward(ctx, dout):
        Zg, Ze, stats = ctx.saved_tensors
        dout, ldd = _rowmajor2d(dout)
        dZg, dZe = (Zg, Ze) if ctx.overwrite else (torch.empty_like(Zg), torch.empty_like(Ze))
        _lib.check(_lib.lib().yt8m_softmax_moe_bwd(_p(Zg), _p(Ze), _p(stats), _p(dout), ldd, ctx.V1, _p(dZg), _p(dZe), Zg.shape[0], ctx.S,
                                                   ctx.M, _stream()))
        dhead = dout[:, :ctx.V1] if (ctx.V1 and ctx.needs_input_grad[2]) else None       # the head's gradient: dout's leading columns
        return dZg, dZe, dhead, None, None, None


def softmax_moe(Zg, Ze, S, M, head=None, overwrite_logits=False):
    """[rows, V1 + S - 1] = [head | q[:, :S - 1]]: the label-softmax mixture block of MoeSoftmaxModel (Z/video_level_models.py:927-959)
    from its gate logits Zg [rows, S (M + 1)] (column s (M + 1) + m), its expert logits Ze [rows, S M] (column s M + m) and, where
    given, the sigmoid part head [rows, V1]:  g = softmax over the M + 1 gates, e = softmax over the S LABELS per mixture,
    p = sum_{m < M} g e, q = p / sum_s p; the last label ("none of the infrequent labels") is dropped.  Differentiable in all three.
    overwrite_logits: the fused backward may write the gradients over Zg and Ze (for logits nothing else reads).
    YT8M_SOFTMAX_MOE_FUSED (read at import): 0 is the composed form (softmax_moe_composed), anything else the kernel pair; CPU tensors,
    non-float32 tensors and shapes yt8m_softmax_moe_supported refuses (S < 2, S > 65536, M > 8) always take the composed form."""
    S, M = int(S), int(M)
    if Zg.dim() != 2 or Ze.dim() != 2 or S < 2 or M < 1 or tuple(Zg.shape) != (Ze.shape[0], S * (M + 1)) or Ze.shape[1] != S * M \
            or (head is not None and (head.dim() != 2 or head.shape[0] != Zg.shape[0])):
        raise ValueError("softmax_moe: Zg [rows, S (M + 1)], Ze [rows, S M], head [rows, V1] or None with S >= 2 and M >= 1, got %s, %s, %s, "
                         "S = %d, M = %d" % (tuple(Zg.shape), tuple(Ze.shape), None if head is None else tuple(head.shape), S, M))
    if head is not None and head.shape[1] == 0:
        head = None
    ts = (Zg, Ze) + (() if head is None else (head,))
    fused = (SOFTMAX_MOE_FUSED and Zg.shape[0] > 0 and all(t.is_cuda and t.dtype == torch.float32 for t in ts)
             and bool(_lib.lib().yt8m_softmax_moe_supported(S, M)))
    SOFTMAX_MOE_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return softmax_moe_composed(Zg, Ze, S, M, head)
    return _SoftmaxMoe.apply(Zg, Ze, head, S, M, bool(overwrite_logits))


def split_softmax_loss_composed(p, labels, bound, scale=1.0):
    """split_softmax_loss as the reference writes it (Z/losses.py:424-446), in torch: cross entropy on the first `bound` columns; on the
    others the labels divided by their row sum with 1 - max appended, the predictions with max(1 - sum, 0) appended (the clamp is this
    repository's; its gradient is taken as if unclamped), and the two-sided log loss with eps = 10e-8."""
    y = labels.to(p.dtype)
    y1, p1, y2, p2 = y[:, :bound], p[:, :bound], y[:, bound:], p[:, bound:]
    cross_entropy_loss = -(y1 * torch.log(p1 + XENT_EPS) + (1 - y1) * torch.log(1 - p1 + XENT_EPS)).sum(dim=1).mean()
    label_rowsum = torch.clamp(y2.sum(dim=1, keepdim=True), min=SOFTMAX_LOSS_EPS)
    norm_float_labels = torch.cat((y2 / label_rowsum, 1.0 - y2.max(dim=1, keepdim=True)[0]), dim=1)
    predictions_append = 1.0 - p2.sum(dim=1, keepdim=True)
    predictions_append = predictions_append + (torch.clamp(predictions_append, min=0.0) - predictions_append).detach()
    softmax_outputs = torch.cat((p2, predictions_append), dim=1)
    softmax_loss = -(norm_float_labels * torch.log(softmax_outputs + SOFTMAX_LOSS_EPS)
                     + (1 - norm_float_labels) * torch.log(1 - softmax_outputs + SOFTMAX_LOSS_EPS)).sum(dim=1)
    loss = softmax_loss.mean() + cross_entropy_loss
    return loss * scale if scale != 1.0 else loss


def _split_softmax_loss_args(p, labels):
    p, ldp = _rowmajor2d(p)
    lab, ldt = _labels_arg(labels)
    return p, ldp, lab, ldt


class _SplitSoftmaxLoss(torch.autograd.Function):
    """csrc/softmax_moe.hip: p is read in place through its row pitch (a piece of predictions_class goes in without a copy); backward
    recomputes dL/dp from (p, y) with the upstream scalar read on the device, as _Xent."""

    @staticmethod
    def forward(ctx, p, labels, bound, scale):
        _dev(p, labels)
        pp, ldp, lab, ldt = _split_softmax_loss_args(p, labels)
        B, V = pp.shape
        L = _lib.lib()
        ws = _loss_workspace(L.yt8m_split_softmax_loss_workspace_bytes(B), pp.device)
        loss = torch.empty((), dtype=torch.float32, device=pp.device)
        _lib.check(L.yt8m_split_softmax_loss_fwd_bwd(_p(pp), ldp, 0, _p(lab), ldt, _p(loss), None, B, V, bound, XENT_EPS, SOFTMAX_LOSS_EPS, 1.0,
                                                     _p(ws), _stream()))
        ctx.save_for_backward(p)
        ctx.labels, ctx.bound, ctx.scale = labels, bound, scale
        return loss * scale if scale != 1.0 else loss

    @staticmethod
    def backward(ctx, dloss):
        (p,) = ctx.saved_tensors
        pp, ldp, lab, ldt = _split_softmax_loss_args(p, ctx.labels)
        B, V = pp.shape
        dp = torch.empty((B, V), dtype=torch.float32, device=pp.device)
        _lib.check(_lib.lib().yt8m_split_softmax_loss_bwd(_p(pp), ldp, 0, _p(lab), ldt, _p(_f32c(dloss.reshape(1))), _p(dp), B, V, ctx.bound,
                                                          XENT_EPS, SOFTMAX_LOSS_EPS, ctx.scale, _stream()))
        return dp, None, None, None


def split_softmax_loss(p, labels, bound, scale=1.0):
    """Z's SoftmaxLoss (Z/losses.py:412-446; losses.SplitSoftmaxLoss) times `scale`: cross entropy (eps 10e-6) on the columns [0, bound)
    of p [B, V] plus, on the others, -sum (n log(o + 10e-8) + (1 - n) log(1 - o + 10e-8)) with n = [y2 / max(sum y2, 10e-8) | 1 - max y2]
    and o = [p2 | max(1 - sum p2, 0)], mean over the batch.  The clamp is this repository's (the reference's 1 - sum falls below -10e-8 in
    float32 and gives NaN); its gradient is taken as if unclamped.  p may be a column window of a wider tensor.
    YT8M_SPLIT_SOFTMAX_LOSS_FUSED (read at import): 0 is the composed form (split_softmax_loss_composed), anything else the kernel; CPU
    tensors, non-float32 predictions and labels that are not bool / uint8 / float32 always take the composed form."""
    bound = int(bound)
    if p.dim() != 2 or tuple(labels.shape) != tuple(p.shape) or not 0 < bound < p.shape[1]:
        raise ValueError("split_softmax_loss: p and labels [B, V] and 0 < bound < V, got %s, %s, bound = %d"
                         % (tuple(p.shape), tuple(labels.shape), bound))
    fused = (SPLIT_SOFTMAX_LOSS_FUSED and p.shape[0] > 0 and p.is_cuda and labels.is_cuda and p.dtype == torch.float32
             and labels.dtype in (torch.bool, torch.uint8, torch.float32))
    SPLIT_SOFTMAX_LOSS_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return split_softmax_loss_composed(p, labels, bound, scale)
    return _SplitSoftmaxLoss.apply(p, labels, bound, float(scale))


class _MatConst(torch.autograd.Function):
    """x . S for a constant matrix S [V, K] (MoeKnowledgeModel's class matrix): dx = dy . S^T."""

    @staticmethod
    def forward(ctx, x, S):
        ctx.S = S
        return gemm(_f32c(x), S)

    @staticmethod
    def backward(ctx, dy):
        return gemm(_f32c(dy), ctx.S, transB=True), None


def matmul_const(x, S):
    """x [rows, V] . S [V, K], S a constant of the model (no gradient).  CPU tensors take torch.matmul (host tests)."""
    return _MatConst.apply(x, S) if x.is_cuda else x @ S


class _LinearGroup(torch.autograd.Function):
    """y_k = x_k . W_k (+ b_k) for n products of one shape family, each direction one grouped launch (gemm_grouped): the forward
    products, the weight gradients x_k^T . dy_k (role "dw") into the Variables' arena slots, and dx_k = dy_k . W_k^T for the inputs that
    want one.  spec[k] = (W, index, b): W_k is W.data (index None) or the plane W.data[index] of a stacked Variable."""

    @staticmethod
    def forward(ctx, token, spec, *xs):
        xs = [_f32c(x) for x in xs]
        planes = [W.data if i is None else W.data[i] for W, i, _ in spec]
        ys = gemm_grouped([dict(A=x, B=Wk, bias=None if b is None else b.data) for x, Wk, (_, _, b) in zip(xs, planes, spec)])
        ctx.spec = spec
        ctx.save_for_backward(*xs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        xs, spec = ctx.saved_tensors, ctx.spec
        dys = [_f32c(dy) for dy in dys]
        betas, items = {}, []
        for x, dy, (W, i, b) in zip(xs, dys, spec):
            if W.trainable and W.grad is not None:
                if id(W) not in betas:                                   # the planes of one stacked Variable: one first write each
                    betas[id(W)] = (W, W.grad_beta())
                items.append(dict(A=x, B=dy, out=W.grad if i is None else W.grad[i], beta=betas[id(W)][1]))
            if b is not None and b.trainable and b.grad is not None:
                colsum(dy, b.grad.view(-1), beta=b.grad_beta())
                b.grad_done()
        if items:
            gemm_grouped(items, transA=True, role="dw")
        for W, _ in betas.values():
            W.grad_done()
        dxs = [None] * len(xs)
        want = [k for k in range(len(xs)) if ctx.needs_input_grad[2 + k]]
        if want:
            outs = gemm_grouped([dict(A=dys[k], B=spec[k][0].data if spec[k][1] is None else spec[k][0].data[spec[k][1]]) for k in want],
                                transB=True)
            for k, dx in zip(want, outs):
                dxs[k] = dx
        return (None, None) + tuple(dxs)


def linear_group(xs, spec):
    """[x_k . W_k (+ b_k)] for spec[k] = (W, index, b) (see _LinearGroup): n fully-connected products as one grouped launch per
    direction.  CPU tensors take torch.matmul on the Variables as tensors (host tests; the device never does)."""
    xs = list(xs)
    if not xs[0].is_cuda:
        ys = []
        for x, (W, i, b) in zip(xs, spec):
            Wt = as_tensor(W)
            y = x @ (Wt if i is None else Wt[i])
            ys.append(y if b is None else y + as_tensor(b))
        return ys
    return list(_LinearGroup.apply(_token(spec[0][0]._graph), tuple(spec), *xs))


# 0: ens_combine / ens_moments compose torch ops; anything else (the default): the fused kernels of csrc/ensemble.hip where the input is a
# method-major device tensor.  Fused is the default because tools/ensemble_step.py's op leg measured its median below the composed form's
# at every shape in both runs of the leg, 3.6 - 13 x (DESIGN_LOG.md section 30).
ENSEMBLE_FUSED = os.environ.get("YT8M_ENSEMBLE_FUSED", "1") != "0"
ENS_XFORM = {None: 0, "logit": 1}
ENS_LOGIT_EPS = 1e-5                  # E/all_ensemble_models/nonunit_matrix_regression_model.py:27


def ens_method_major(x):
    """x [B, V, M] is a view of a contiguous [M, B, V] buffer (strides (V, 1, B V)): ensemble.EnsembleInput's layout."""
    return x.dim() == 3 and x.permute(2, 0, 1).is_contiguous()


def _ens_fused(x, J=1):
    return (ENSEMBLE_FUSED and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and ens_method_major(x)
            and J <= _lib.lib().yt8m_ens_max_gates())


def ens_xform(x, xform=None):
    if xform not in ENS_XFORM:
        raise ValueError("ens_combine: xform must be None or 'logit', got %r" % (xform,))
    return x if xform is None else torch.log((ENS_LOGIT_EPS + x) / (1.0 + ENS_LOGIT_EPS - x))


def ens_combine_composed(x, W, gate=None, xform=None):
    """The reference's formulation in torch ops: logits, their softmax over the methods and the weighted sum."""
    t = ens_xform(x, xform)
    if gate is None:
        return torch.einsum("bvk,vk->bv", t, torch.softmax(W[0], dim=-1))
    return (torch.softmax(torch.einsum("bj,jvk->bvk", gate, W), dim=-1) * t).sum(dim=-1)


class _EnsCombine(torch.autograd.Function):
    """csrc/ensemble.hip: one pass over the method-major predictions each way.  Saved for backward: x (data), the [J, M, V] re-layout of
    the tables, gate, out [B, V] and the softmax statistics [2, B, V] -- nothing of size [B, V, M]."""

    @staticmethod
    def forward(ctx, x, W, gate, xform):
        B, V, M = x.shape
        J = W.shape[0]
        Wt = W.detach().permute(0, 2, 1).contiguous()                    # v innermost: 5.6 MB at J = 4, V = 4716, M = 74
        g = None if gate is None else _f32c(gate.detach())
        need = ctx.needs_input_grad[1] or (gate is not None and ctx.needs_input_grad[2])
        out = torch.empty((B, V), dtype=torch.float32, device=x.device)
        stat = torch.empty((2, B, V), dtype=torch.float32, device=x.device) if need else None
        _lib.check(_lib.lib().yt8m_ens_combine_fwd(_p(x), _p(Wt), _p(g), ENS_XFORM[xform], _p(out), _p(stat), B, V, M, J, _stream()))
        ctx.xform = xform
        if need:
            ctx.has_gate = g is not None
            ctx.save_for_backward(*([x, Wt, out, stat] + ([g] if g is not None else [])))
        return out

    @staticmethod
    def backward(ctx, dout):
        x, Wt, out, stat = ctx.saved_tensors[:4]
        g = ctx.saved_tensors[4] if ctx.has_gate else None
        B, V, M = x.shape
        J = Wt.shape[0]
        dout = _f32c(dout)
        dWt = torch.empty_like(Wt)
        dgate = torch.empty_like(g) if g is not None else None
        nbytes = _lib.lib().yt8m_ens_combine_bwd_workspace_bytes(B, V, M, J)
        ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().yt8m_ens_combine_bwd(_p(x), _p(Wt), _p(g), ENS_XFORM[ctx.xform], _p(out), _p(stat), _p(dout), _p(dWt), _p(dgate),
                                                   _p(ws), nbytes, B, V, M, J, _stream()))
        return None, dWt.permute(0, 2, 1), dgate, None


def ens_combine(x, W, gate=None, xform=None):
    """out [B, V] = sum_k softmax_k(sum_j gate[b, j] W[j, v, k]) t(x[b, v, k]): the combine every plugin of ensemble_level_models.py
    ends in.  x [B, V, M]: stacked predictions, data.  W [J, V, M]: logit tables; gate [B, J], or None with J = 1 (gate = 1).  xform:
    None (t = identity) or "logit" (t = log((1e-5 + x) / (1 + 1e-5 - x))).  Gradients reach W and gate.
    The fused kernels take device tensors in ensemble.EnsembleInput's method-major layout with up to 4 tables unless YT8M_ENSEMBLE_FUSED
    (read at import) is 0; CPU tensors, contiguous [B, V, M] inputs, an x that requires a gradient and more tables take the composed
    torch form, which computes the same thing."""
    if xform not in ENS_XFORM:
        raise ValueError("ens_combine: xform must be None or 'logit', got %r" % (xform,))
    if x.dim() != 3 or W.dim() != 3 or tuple(W.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError("ens_combine: x [B, V, M] and W [J, V, M], got %s and %s" % (tuple(x.shape), tuple(W.shape)))
    if gate is None and W.shape[0] != 1:
        raise ValueError("ens_combine: no gate means one table, got %d" % W.shape[0])
    if gate is not None and tuple(gate.shape) != (x.shape[0], W.shape[0]):
        raise ValueError("ens_combine: gate must be [%d, %d], got %s" % (x.shape[0], W.shape[0], tuple(gate.shape)))
    if not _ens_fused(x, W.shape[0]):
        return ens_combine_composed(x, W, gate, xform)
    return _EnsCombine.apply(x, W, gate, xform)


def ens_moments(x, variance=False):
    """(mean over the methods [B, V], unbiased variance [B, V] or None) of stacked predictions x [B, V, M]; x is data, no gradient.
    One kernel pass under the conditions of ens_combine, torch ops otherwise."""
    M = x.shape[2]
    if variance and M < 2:
        raise ValueError("ens_moments: the unbiased variance needs at least 2 methods")
    with torch.no_grad():
        if not _ens_fused(x):
            mean = x.mean(dim=2)
            return mean, ((x - mean.unsqueeze(2)) ** 2).sum(dim=2) / (M - 1) if variance else None
        B, V, _ = x.shape
        mean = torch.empty((B, V), dtype=torch.float32, device=x.device)
        var = torch.empty_like(mean) if variance else None
        _lib.check(_lib.lib().yt8m_ens_moments(_p(x), _p(mean), _p(var), B, V, M, _stream()))
        return mean, var


# The per-class matrix mix and the per-video mix of the ensemble stage (csrc/ensemble_tensor.hip).  Each switch is read at import; 0 takes
# the composed torch form everywhere.  The defaults follow tools/ensemble_moe_step.py's op legs (profiles/ensemble_moe_step.jsonl,
# DESIGN_LOG.md section 43): fused is the default of an op only if its median was below the composed form's at every shape in both
# runs of the leg.  ens_tensor_moe: it was, 1.5 - 2.7 x: fused.  ens_mix: 25 - 92 x below at B = 1024, but at [128, 4716, 74] the first
# run measured 168 us against 156 us (the second 76 against 136; both forms are bound by the host there): composed stays the default and
# YT8M_ENS_MIX_FUSED=1 opts in -- which a run at the training scripts' B = 1024 should do (InputMoeModel's step: 0.85 ms against 18.4 ms).
ENS_TENSOR_FUSED = os.environ.get("YT8M_ENS_TENSOR_FUSED", "1") != "0"
ENS_MIX_FUSED = os.environ.get("YT8M_ENS_MIX_FUSED", "0") != "0"
ENS_TENSOR_CALLS = {"kernels": 0, "composed": 0}
ENS_MIX_CALLS = {"kernels": 0, "composed": 0}


def _ens_layout_ok(x):
    return x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and ens_method_major(x)


def _ens_tensor_fused(x):
    return ENS_TENSOR_FUSED and _ens_layout_ok(x) and x.shape[2] <= _lib.lib().yt8m_ens_tensor_max_methods()


def _ens_mix_fused(x):
    return ENS_MIX_FUSED and _ens_layout_ok(x)


def ens_tensor_moe_composed(x, W, b):
    """moe_model.py:51-54 in torch ops: the einsum, its softmax over the methods and the sum."""
    gate_activations = torch.einsum("ijk,jkl->ijl", x, W) + b.unsqueeze(0)
    return (x * torch.softmax(gate_activations, dim=-1)).sum(dim=2)


class _EnsTensorMoe(torch.autograd.Function):
    """csrc/ensemble_tensor.hip.  Saved for backward: x (data), the [M, M, V] and [M, V] re-layouts of W and b, out [B, V] and the softmax
    statistics [2, B, V] -- nothing of size [B, V, M]."""

    @staticmethod
    def forward(ctx, x, W, b):
        B, V, M = x.shape
        Wt = W.detach().permute(1, 2, 0).contiguous()                    # [k, l, V], v innermost: 103 MB at V = 4716, M = 74
        bt = b.detach().t().contiguous()
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        out = torch.empty((B, V), dtype=torch.float32, device=x.device)
        stat = torch.empty((2, B, V), dtype=torch.float32, device=x.device) if need else None
        _lib.check(_lib.lib().yt8m_ens_tensor_fwd(_p(x), _p(Wt), _p(bt), _p(out), _p(stat), B, V, M, _stream()))
        if need:
            ctx.save_for_backward(x, Wt, bt, out, stat)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, Wt, bt, out, stat = ctx.saved_tensors
        B, V, M = x.shape
        dout = _f32c(dout)
        dWt, dbt = torch.empty_like(Wt), torch.empty_like(bt)
        nbytes = _lib.lib().yt8m_ens_tensor_bwd_workspace_bytes(B, V, M)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes > 0 else None
        _lib.check(_lib.lib().yt8m_ens_tensor_bwd(_p(x), _p(Wt), _p(bt), _p(out), _p(stat), _p(dout), _p(dWt), _p(dbt), _p(ws), nbytes,
                                                  B, V, M, _stream()))
        return None, dWt.permute(2, 0, 1), dbt.t()


def ens_tensor_moe(x, W, b):
    """out [B, V] = sum_l softmax_l(sum_k x[b, v, k] W[v, k, l] + b[v, l]) x[b, v, l]: the ensemble MoeModel's per-class matrix over the
    methods.  x [B, V, M]: stacked predictions, data.  W [V, M, M], b [V, M]: gradients reach both.
    The fused kernels take device tensors in ensemble.EnsembleInput's method-major layout with up to yt8m_ens_tensor_max_methods() = 80
    methods unless YT8M_ENS_TENSOR_FUSED (read at import) is 0; CPU tensors, contiguous [B, V, M] inputs, other dtypes, an x that requires
    a gradient and more methods take ens_tensor_moe_composed, which computes the same thing."""
    if x.dim() != 3 or tuple(W.shape) != (x.shape[1], x.shape[2], x.shape[2]) or tuple(b.shape) != tuple(x.shape[1:]):
        raise ValueError("ens_tensor_moe: x [B, V, M], W [V, M, M] and b [V, M], got %s, %s and %s"
                         % (tuple(x.shape), tuple(W.shape), tuple(b.shape)))
    fused = _ens_tensor_fused(x)
    ENS_TENSOR_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return ens_tensor_moe_composed(x, W, b)
    return _EnsTensorMoe.apply(x, W, b)


def ens_mix_composed(x, a):
    return torch.einsum("ijk,ik->ij", x, a)


class _EnsMix(torch.autograd.Function):
    """csrc/ensemble_tensor.hip: one pass over the method-major predictions each way; saved for backward: x (data) alone."""

    @staticmethod
    def forward(ctx, x, a):
        B, V, M = x.shape
        a32 = _f32c(a.detach())
        out = torch.empty((B, V), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().yt8m_ens_mix_fwd(_p(x), _p(a32), _p(out), B, V, M, _stream()))
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        B, V, M = x.shape
        dout = _f32c(dout)
        da = torch.empty((B, M), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().yt8m_ens_mix_bwd(_p(x), _p(dout), _p(da), B, V, M, _stream()))
        return None, da


def ens_mix(x, a):
    """out [B, V] = sum_k a[b, k] x[b, v, k]: one mixing row per video (InputMoeModel, AttentionMoeModel).  x [B, V, M]: stacked
    predictions, data; the gradient reaches a [B, M].  Kernels under the conditions of ens_tensor_moe (any M) unless YT8M_ENS_MIX_FUSED
    (read at import) is 0, ens_mix_composed otherwise."""
    if x.dim() != 3 or tuple(a.shape) != (x.shape[0], x.shape[2]):
        raise ValueError("ens_mix: x [B, V, M] and a [B, M], got %s and %s" % (tuple(x.shape), tuple(a.shape)))
    fused = _ens_mix_fused(x)
    ENS_MIX_CALLS["kernels" if fused else "composed"] += 1
    if not fused:
        return ens_mix_composed(x, a)
    return _EnsMix.apply(x, a)


class _HeadPlan(collections.namedtuple("_HeadPlan", "logits z16 backward dx_bf16 dx k0 absmax need_dx")):
    """The forms one call of the MoE head runs its three products in -- logits, dx, dW --, chosen once, in the forward pass
    (_moe_head_plan), from shapes, dtypes, flags and the module's knobs; the backward passes dispatch on these fields alone.
    logits: "b1_keep" (one-plane bf16 operand images whose pass writes the OTHER orientation of x / Wg / We too -- what the backward
            products read (x^T for dW, W for dx) --, so each tensor is read once per step), "b1" (those images, one orientation),
            "bf16_nt" (bf16 casts, both sides K-contiguous), "h2" (fp32 operands under the declared h2 role: three f16 products under one
            scale per operand matrix, max |x| measured once -- the weight gradient's split of x^T takes the same word) or "fp32".
    z16:    the logits leave the b1 product as bf16 -- the bf16 configuration's own precision -- because everything behind them reads
            bf16: the bf16-logit mixing pass (M == 2, V % 4 == 0) and, when a backward pass follows, the image form of the fused mixing
            backward writing into both gradient slots.  Halves the 773 MB a [8192, 5 x 4716] stage of configs[4] writes and the two
            passes behind it read.  Opt-in: see Z16_LOGITS.
    backward: None (no backward pass follows), "fused_images" (bf16, M == 2: ONE pass over the logits writes dL/dZ straight into the
            one-plane images of both orientations; three image products), "fused_rows" (the same pass onto row-major bf16; three bf16
            products), "casts" (mixing backward in place, then bf16 casts of dZ; dx_bf16: dx as a bf16 product too -- not with an odd
            V (M + 1) or V M, a reduction length that cannot be packed in bf16 pairs) or "fp32" (in place, then fp32 products).
    dx:     of the "fp32" backward when the input takes a gradient (need_dx), else None: "h2_rows" (row-scaled three-f16-product form
            from column k0 on), "window" (the columns [k0:) on the generic product) or "plain"; k0: moe_head's dx_from where it is a
            whole 32-row group of the weights' images inside D, else 0.
    absmax: moe_head_xent's in-place mixing backward measures max |dZ| for the dW products' h2 split (MIX_BWD_ABSMAX)."""
    __slots__ = ()

    def __new__(cls, **fields):
        plan = super(_HeadPlan, cls).__new__(cls, **fields)
        assert not plan.z16 or plan.backward in (None, "fused_images"), "bf16 logits: only the image form of the fused mixing backward reads them"
        return plan


def _moe_head_plan(B, D, Ng, Ne, V, M, bf16, training, need_dx, dx_from=0, z16_allowed=False, w_contiguous=True, grad_slots=True):
    """The _HeadPlan of x [B, D] against Wg [D, Ng] and We [D, Ne]: the ONE place where the head's forms are chosen (the table is pinned
    by tests/test_moe_head_plan_host.py).  Plain integers and booleans only; the knobs are read when it is called.  training: a backward
    pass may follow; z16_allowed: the op's mixing pass reads bf16 logits; w_contiguous: both weight matrices are; grad_slots: both have a
    gradient slot."""
    # bf16 GEMMs need even reduction lengths (D for the forward, the batch for dW) and enough rows to amortise the per-step cast of the weights
    b16 = bf16 and B % 2 == 0 and D % 2 == 0 and B >= BF16_MIN_ROWS
    b1_fwd, b1_bwd = b16 and _b1_ok(B, Ng, D), _b1_ok(D, Ng, B)
    pairs = Ng % 2 == 0 and Ne % 2 == 0                 # dZ's reduction lengths pack in bf16 pairs
    if not training:
        backward = None
    elif b16 and M == 2 and pairs:
        backward = "fused_images" if (b1_fwd and b1_bwd) else "fused_rows"
    else:
        backward = "casts" if b16 else "fp32"
    if b1_fwd:
        logits = "b1_keep" if (M == 2 and training and b1_bwd) else "b1"
    elif b16:
        logits = "bf16_nt"
    else:
        # from MOE_LOGITS_H2_MIN_ROWS rows on: the weights' half-plane images are made per call (absmax + split of [D, 5V]), which a
        # B = 128 product does not pay back (NetVLADModel at B = 128: 2.57 -> 2.88 ms/step with it; break-even by the split / product rates
        # ~1 000 rows while the images were made per call; with them resident (wimg.py) 512 rows gain too: DeepCombineChain at B = 512
        # 12.95 -> 12.03 ms/step; measured -6 % at 1 024, -7 % at 8 192)
        logits = "h2" if (MOE_LOGITS_H2 and B >= MOE_LOGITS_H2_MIN_ROWS) else "fp32"
    z16 = (z16_allowed and Z16_LOGITS and b1_fwd and M == 2 and V % 4 == 0 and Ng == 3 * V and Ne == 2 * V
           and (backward is None or (backward == "fused_images" and grad_slots)))
    dx, k0 = None, 0
    if backward == "fp32" and need_dx:
        k0 = dx_from if (MOE_DX_FROM and 0 < dx_from < D and dx_from % 32 == 0) else 0
        # round 6: from 1 024 rows on, three f16 products with dZ split row by row against the weights' half-plane images (the form of
        # ops._linear_dx_h2_rows) instead of the fp32-MFMA kernel these 16-tile, K ~ 14 000 products fell back to
        h2_rows = MOE_DX_H2 and B >= MOE_LOGITS_H2_MIN_ROWS and D % 4 == 0 and w_contiguous
        dx = "h2_rows" if h2_rows else "window" if k0 else "plain"
    return _HeadPlan(logits=logits, z16=z16, backward=backward, dx_bf16=backward == "casts" and need_dx and pairs, dx=dx, k0=k0,
                     absmax=MIX_BWD_ABSMAX and backward in ("casts", "fp32"), need_dx=need_dx)


class _MoeHead(torch.autograd.Function):
    """MoE block of W/all_video_models/moe_model.py:40-64: two GEMMs + mixing kernel; backward per Appendix G."""

    @staticmethod
    def forward(ctx, x, token, Wg, We, be, V, M, bf16, dx_from=0):
        x2, Zg, Ze = _moe_head_fwd(ctx, x, Wg, We, be, V, M, bf16, dx_from=dx_from, z16=True)
        return moe_mix_fwd(Zg, Ze, V, M)

    @staticmethod
    def backward(ctx, dp):
        plan, kept, x, Zg, Ze, Wg, We, be, V, M = _moe_head_saved(ctx)
        if plan.backward in ("fused_images", "fused_rows"):
            dx = _moe_head_bwd_bf16_fused(plan, kept, x, Zg, Ze, Wg, We, be, V, M, dp=_f32c(dp))
            return dx, None, None, None, None, None, None, None, None
        moe_mix_bwd_(Zg, Ze, dp, V, M)            # in place: Zg <- dL/dZg, Ze <- dL/dZe
        dx = _moe_head_param_grads(plan, x, Zg, Ze, Wg, We, be, xmax=kept.get("xmax"))
        return dx, None, None, None, None, None, None, None, None


def _moe_head_fwd(ctx, x, Wg, We, be, V, M, bf16, dx_from=0, z16=False):
    """What the two head ops' forward passes share: the plan, the logits (x2, Zg, Ze) and everything the backward forms read from ctx.
    z16: the op's mixing pass reads bf16 logits."""
    x2 = _f32c(x)
    ctx.plan = _moe_head_plan(x2.shape[0], x2.shape[1], Wg.data.shape[1], We.data.shape[1], V, M, bf16,
                              training=ctx.needs_input_grad[0] or ctx.needs_input_grad[1], need_dx=ctx.needs_input_grad[0], dx_from=dx_from,
                              z16_allowed=z16, w_contiguous=Wg.data.is_contiguous() and We.data.is_contiguous(),
                              grad_slots=Wg.grad is not None and We.grad is not None)
    ctx.kept = {}                # what the logits' form hands the backward: the images "xT" / "Wg" / "We" (b1_keep), the word "xmax" (h2)
    Zg, Ze = _moe_logits(x2, Wg, We, be, ctx.plan, ctx.kept)
    ctx.save_for_backward(x2)
    ctx.Z = (Zg, Ze)
    ctx.vars = (Wg, We, be)
    ctx.VM = (V, M)
    return x2, Zg, Ze


def _moe_head_saved(ctx):
    """(plan, kept, x, Zg, Ze, Wg, We, be, V, M) of _moe_head_fwd; the logits and what was kept are released with the backward pass."""
    saved = (ctx.plan, ctx.kept) + ctx.saved_tensors + ctx.Z + ctx.vars + ctx.VM
    ctx.Z = ctx.kept = None
    return saved


def _moe_head_dw(product, pg, pe, Wg, We, be, bsrc, **kw):
    """The tail of every backward form of the head: the weight-gradient products pg -> Wg.grad, pe -> We.grad through `product` (None,
    None: a gradient slot is missing, no product) and the experts' bias gradient, the column sums of bsrc."""
    if pg is not None:
        if Wg._graph is not None and Wg._graph.grad_ready_hook is not None:
            # data-parallel: finish the big gate gradient first so its all-reduce rides under the expert GEMM
            product([pg], **kw)
            Wg.grad_done()
            product([pe], **kw)
            We.grad_done()
        else:
            product([pg, pe], **kw)
            Wg.grad_done()
            We.grad_done()
    if be.grad is not None:
        colsum(bsrc, be.grad.view(-1), beta=be.grad_beta())
        be.grad_done()


def _moe_head_bwd_bf16_fused(plan, kept, x, Zg, Ze, Wg, We, be, V, M, dp=None, labels=None, ldt=0, dscale=1.0, up=None):
    """bf16 configuration: ONE pass over the fp32 logits produces dL/dZ as bf16 in both layouts + the bias partial sums, then
    the same three bf16 products as _moe_head_param_grads_bf16 (no fp32 dZ, no cast passes, no colsum over dZ_e)."""
    L = _lib.lib()
    B = Zg.shape[0]
    dev = Zg.device
    if plan.backward == "fused_images":
        return _moe_head_bwd_bf16_images(plan, kept, x, Zg, Ze, Wg, We, be, V, M, dp, labels, ldt, dscale, up)
    Zgb, ZgT = _bf16_empty(B, Zg.shape[1], dev), _bf16_empty(Zg.shape[1], B, dev)
    Zeb, ZeT = _bf16_empty(B, Ze.shape[1], dev), _bf16_empty(Ze.shape[1], B, dev)
    part = torch.empty((L.yt8m_moe_mix_bwd_bf16_partial_rows(B), Ze.shape[1]), dtype=torch.float32, device=dev) \
        if be.grad is not None else None
    _lib.check(L.yt8m_moe_mix_bwd_bf16(_p(Zg), _p(Ze), _p(dp), _p(labels), ldt, B, V, M, XENT_EPS, float(dscale), _p(up),
                                       _p(Zgb), Zgb.stride(0), _p(ZgT), ZgT.stride(0), _p(Zeb), Zeb.stride(0), _p(ZeT),
                                       ZeT.stride(0), _p(part), _stream()))
    dx = None
    if plan.need_dx:
        dx, = gemm_bf16_nt_grouped([dict(A=Zgb, B=cast_bf16(Wg.data))])
        gemm_bf16_nt_grouped([dict(A=Zeb, B=cast_bf16(We.data), out=dx, beta=1.0)])
    del Zgb, Zeb
    pg = pe = None
    if Wg.grad is not None and We.grad is not None:
        xT = cast_bf16(x, transpose=True)
        pg = dict(A=xT, B=ZgT, out=Wg.grad, beta=Wg.grad_beta())
        pe = dict(A=xT, B=ZeT, out=We.grad, beta=We.grad_beta())
    _moe_head_dw(gemm_bf16_nt_grouped, pg, pe, Wg, We, be, part)
    return dx


def _moe_head_bwd_bf16_images(plan, kept, x, Zg, Ze, Wg, We, be, V, M, dp, labels, ldt, dscale, up):
    """_moe_head_bwd_bf16_fused on operand images: the mixing backward writes dL/dZ straight into the one-plane images the b1
    kernel reads (both orientations), the weights and x^T are rounded into images by one pass each unless the forward's image
    passes kept them (`kept`); three image products."""
    L = _lib.lib()
    B, Ng, Ne = Zg.shape[0], Zg.shape[1], Ze.shape[1]
    dev = Zg.device
    Zgi, ZgTi, Zei, ZeTi = _image_empty(B, Ng, 1, dev), _image_empty(Ng, B, 1, dev), _image_empty(B, Ne, 1, dev), _image_empty(Ne, B, 1, dev)
    part = torch.empty((L.yt8m_moe_mix_bwd_bf16_partial_rows(B), Ne), dtype=torch.float32, device=dev) if be.grad is not None else None
    kb = lambda K: (K + 15) // 16
    mix = L.yt8m_moe_mix_bwd_bf16_images_z16 if Zg.dtype == torch.bfloat16 else L.yt8m_moe_mix_bwd_bf16_images
    _lib.check(mix(_p(Zg), _p(Ze), _p(dp), _p(labels), ldt, B, V, M, XENT_EPS, float(dscale), _p(up),
                   _p(Zgi.buf), kb(Ng), _p(ZgTi.buf), kb(B), _p(Zei.buf), kb(Ne), _p(ZeTi.buf), kb(B), _p(part), _stream()))
    dx = None
    if plan.need_dx:
        dx, = gemm_b1_grouped([dict(A=Zgi, B=kept.get("Wg") or bf16_image(Wg.data))])           # W [D, N] as [D rows, K = N]
        gemm_b1_grouped([dict(A=Zei, B=kept.get("We") or bf16_image(We.data), out=dx, beta=1.0)])
    del Zgi, Zei
    pg = pe = None
    if Wg.grad is not None and We.grad is not None:
        xT = kept.get("xT") or bf16_image(x, transpose=True)                    # [D rows, K = B]
        pg = dict(A=xT, B=ZgTi, out=Wg.grad, beta=Wg.grad_beta())
        pe = dict(A=xT, B=ZeTi, out=We.grad, beta=We.grad_beta())
    _moe_head_dw(gemm_b1_grouped, pg, pe, Wg, We, be, part)
    return dx


# OPT-IN (YT8M_Z16_LOGITS=1): configs[4] at B = 1024 19.88 / 19.71 -> 19.25 / 19.19 ms/step (-3 %), but the full-size golden replay of the same
# configuration (tests/test_gpu_fullsize_golden.py[c4_composite_bf16]) then sees the attention weights' gradient at 0.67 of its fp64
# magnitude (abs-sum 2.61 against 3.89; tolerance 0.2 of the scale, met with fp32 logits): rounding the logits themselves -- not just the
# products' operands -- to 8 significant bits is more than that gradient takes.  The kernels are exact in kind (bit for bit the fp32-logit
# passes on rounded logits: tests/test_gpu_round6.py::test_bf16_logits_*).
Z16_LOGITS = os.environ.get("YT8M_Z16_LOGITS", "0") != "0"
MOE_LOGITS_H2 = os.environ.get("YT8M_MOE_LOGITS_H2", "1") != "0"
MOE_LOGITS_H2_MIN_ROWS = int(os.environ.get("YT8M_MOE_LOGITS_H2_MIN_ROWS", "512"))   # 512: DeepCombineChain at B = 512 12.95 -> 12.03 ms/step (tools/r6_moe_rows.sh); B = 128 heads stay on the fp32 kernel (+0.3 ms on the headline with them)
LINEAR_FWD_H2 = os.environ.get("YT8M_LINEAR_FWD_H2", "1") != "0"
LINEAR_H2_MIN_ROWS = int(os.environ.get("YT8M_LINEAR_H2_MIN_ROWS", "512"))
LINEAR_DX_H2 = os.environ.get("YT8M_LINEAR_DX_H2", "1") != "0"
LINEAR_H2_MIN_MNK = float(os.environ.get("YT8M_LINEAR_H2_MIN_MNK", "1e9"))
MOE_DX_H2 = os.environ.get("YT8M_MOE_DX_H2", "1") != "0"
MOE_DX_FROM = os.environ.get("YT8M_MOE_DX_FROM", "1") != "0"           # chain models: no dx for the data columns in front of a head's input
MIX_BWD_ABSMAX = os.environ.get("YT8M_MIX_BWD_ABSMAX", "1") != "0"     # the mixing backward measures max |dZ| for the dW products' h2 split


def _moe_logits(x2, Wg, We, be, plan, kept):
    """Zg = x.Wg, Ze = x.We + be as ONE persistent launch in the plan's form (_HeadPlan.logits); bf16 forms: accumulation stays fp32 and
    so do the outputs unless plan.z16.  kept: receives what the form hands the backward pass."""
    if plan.logits in ("b1_keep", "b1"):
        odt = torch.bfloat16 if plan.z16 else torch.float32
        if plan.logits == "b1_keep":
            xi, kept["xT"] = bf16_image(x2, both=True)
            kept["Wg"], WgT = bf16_image(Wg.data, both=True)
            kept["We"], WeT = bf16_image(We.data, both=True)
        else:                                                # [B rows, K = D]; W^T as [N rows, K = D]: the transposing image pass
            xi, WgT, WeT = bf16_image(x2), bf16_image(Wg.data, transpose=True), bf16_image(We.data, transpose=True)
        return gemm_b1_grouped([dict(A=xi, B=WgT, out_dtype=odt), dict(A=xi, B=WeT, bias=be.data, out_dtype=odt)])
    if plan.logits == "bf16_nt":
        xb = cast_bf16(x2)
        return gemm_bf16_nt_grouped([dict(A=xb, B=cast_bf16(Wg.data, transpose=True)),
                                     dict(A=xb, B=cast_bf16(We.data, transpose=True), bias=be.data)])
    # fp32 configuration: the logits product declares the h2 role -- its input is l2-normalised or a bounded hidden activation, each operand
    # one weight matrix (MOE_LOGITS_H2 / YT8M_MOE_LOGITS_H2=0: six-product form)
    h2 = plan.logits == "h2"
    if h2:
        kept["xmax"] = h2_absmax(x2).view(torch.float32)
    xmax = kept.get("xmax")
    return gemm_grouped([dict(A=x2, B=Wg.data, absmaxA=xmax), dict(A=x2, B=We.data, bias=be.data, absmaxA=xmax)], role="h2" if h2 else None)


class _MoeHeadXent(torch.autograd.Function):
    """MoE block + CrossEntropyLoss in one op: returns (p, loss).  The head's GEMMs are the same grouped launches as
    _MoeHead; mixing+loss and (dL/dp -> dL/dZ) are single fused passes (yt8m_moe_mix_xent_fwd/bwd)."""

    @staticmethod
    def forward(ctx, x, token, Wg, We, be, labels, V, M, bf16):
        x2, Zg, Ze = _moe_head_fwd(ctx, x, Wg, We, be, V, M, bf16)
        B = x2.shape[0]
        lab, ldt = _labels_arg(labels)
        if tuple(lab.shape) != (B, V):
            raise ValueError("labels shape %s != predictions shape %s" % (tuple(lab.shape), (B, V)))
        L = _lib.lib()
        ws = torch.empty((L.yt8m_moe_mix_xent_workspace_bytes(B, V) + 3) // 4, dtype=torch.float32, device=x2.device)
        p = torch.empty((B, V), dtype=torch.float32, device=x2.device)
        loss = torch.empty((), dtype=torch.float32, device=x2.device)
        _lib.check(L.yt8m_moe_mix_xent_fwd(_p(Zg), _p(Ze), _p(lab), ldt, _p(p), _p(loss), B, V, M, XENT_EPS, _p(ws), _stream()))
        ctx.lab = (lab, ldt)
        ctx.mark_non_differentiable(p)          # predictions leave through the loss only on this path
        ctx.set_materialize_grads(False)        # no [B,V] zero-fill for the unused dL/dp slot
        return p, loss

    @staticmethod
    def backward(ctx, dp_unused, dloss):
        plan, kept, x, Zg, Ze, Wg, We, be, V, M = _moe_head_saved(ctx)
        lab, ldt = ctx.lab
        if dloss is None:
            return (None,) * 9
        if plan.backward in ("fused_images", "fused_rows"):
            dx = _moe_head_bwd_bf16_fused(plan, kept, x, Zg, Ze, Wg, We, be, V, M, labels=lab, ldt=ldt, dscale=1.0 / x.shape[0],
                                          up=_f32c(dloss.reshape(1)))
            return dx, None, None, None, None, None, None, None, None
        zmax = None
        if plan.absmax:
            zmax = torch.empty(2, dtype=torch.float32, device=Zg.device)  # max |dZg|, max |dZe| as float bits, written by the same pass
            _lib.check(_lib.lib().yt8m_moe_mix_xent_bwd_absmax(_p(Zg), _p(Ze), _p(lab), ldt, _p(_f32c(dloss.reshape(1))), x.shape[0], V, M,
                                                               XENT_EPS, 1.0, _p(zmax), _stream()))
        else:
            _lib.check(_lib.lib().yt8m_moe_mix_xent_bwd(_p(Zg), _p(Ze), _p(lab), ldt, _p(_f32c(dloss.reshape(1))), x.shape[0], V, M,
                                                        XENT_EPS, 1.0, _stream()))
        dx = _moe_head_param_grads(plan, x, Zg, Ze, Wg, We, be, zmax=zmax, xmax=kept.get("xmax"))
        return dx, None, None, None, None, None, None, None, None


def _moe_head_param_grads_bf16(plan, x, Zg, Ze, Wg, We, be):
    """Same gradients on bf16 MFMAs: every product is written as A.B^T with K-contiguous bf16 copies
    (dW = x^T.dZ = (x^T) . (dZ^T)^T, dx = dZ . (W)^T with W [D,N] itself K-contiguous over N)."""
    dx = None
    need_dw = Wg.grad is not None and We.grad is not None
    ZgT = ZeT = None
    if plan.need_dx:
        if plan.dx_bf16:
            # dZ is needed K-contiguous for dx and row-transposed for dW: both layouts from one pass over the fp32 logits
            Zgb, ZgT = cast_bf16_both(Zg) if need_dw else (cast_bf16(Zg), None)
            Zeb, ZeT = cast_bf16_both(Ze) if need_dw else (cast_bf16(Ze), None)
            dx, = gemm_bf16_nt_grouped([dict(A=Zgb, B=cast_bf16(Wg.data))])
            gemm_bf16_nt_grouped([dict(A=Zeb, B=cast_bf16(We.data), out=dx, beta=1.0)])
            del Zgb, Zeb
        else:                                      # odd V*(M+1): the reduction length cannot be packed in bf16 pairs
            dx = gemm(Zg, Wg.data, transB=True)
            gemm(Ze, We.data, out=dx, transB=True, beta=1.0)
    pg = pe = None
    if need_dw:
        xT = cast_bf16(x, transpose=True)
        pg = dict(A=xT, B=ZgT if ZgT is not None else cast_bf16(Zg, transpose=True), out=Wg.grad, beta=Wg.grad_beta())
        pe = dict(A=xT, B=ZeT if ZeT is not None else cast_bf16(Ze, transpose=True), out=We.grad, beta=We.grad_beta())
    _moe_head_dw(gemm_bf16_nt_grouped, pg, pe, Wg, We, be, Ze)
    return dx


_SIDE = {}
DEFER_HEAD_DW = os.environ.get("YT8M_DEFER_HEAD_DW", "0") != "0"   # measured: no gain (the backward pass is work-bound), opt-in


def side_stream(graph):
    """The side stream on which an op may leave weight-gradient work that nothing later in the backward pass reads (round 5): the
    classifier head's dW products when a recurrent stack's backward pass follows -- its first recurrence holds half the chip for a
    millisecond and waits only for dx.  None when the step must not defer (no stack follows, data parallel: the reducer starts a
    gradient's all-reduce from the current stream)."""
    if not DEFER_HEAD_DW or graph is None or not getattr(graph, "defer_head_dw", False) or graph.grad_ready_hook is not None:
        return None
    st = _SIDE.get(graph.device)
    if st is None:
        st = torch.cuda.Stream(device=graph.device)
        _SIDE[graph.device] = st
    return st


def join_side_work(graph):
    """Makes the current stream wait for everything ops left on side streams in this backward pass (called by the recurrent
    stack's backward and by TrainGraph.step before the optimiser pass)."""
    if graph is None:
        return
    for st in getattr(graph, "side_pending", None) or ():
        torch.cuda.current_stream(graph.device).wait_stream(st)
    graph.side_pending = []


def _moe_head_param_grads(plan, x, Zg, Ze, Wg, We, be, zmax=None, xmax=None):
    """dW_g = x^T dZ_g, dW_e = x^T dZ_e, db_e = colsum(dZ_e), dx = dZ_g W_g^T + dZ_e W_e^T.
    zmax (a [2] float tensor, optional): max |dZ_g|, max |dZ_e| as float bits, already measured by the pass that wrote them."""
    mg = zmax[0:1] if zmax is not None else None
    me = zmax[1:2] if zmax is not None else None
    if plan.backward == "casts":
        return _moe_head_param_grads_bf16(plan, x, Zg, Ze, Wg, We, be)
    # dx before the weights' gradient slots are released to an optimiser.  Columns [0, k0) of x are data (moe_head's dx_from): no gradient is
    # computed for them
    k0, dx = plan.k0, None
    if plan.dx == "h2_rows":
        dx = _linear_dx_h2_rows(Zg, Wg, row0=k0)
        _linear_dx_h2_rows(Ze, We, out=dx, beta=1.0, row0=k0)
    elif plan.dx == "window":
        dx = torch.zeros((Zg.shape[0], Wg.data.shape[0]), dtype=torch.float32, device=Zg.device)
        gemm(Zg, Wg.data[k0:], transB=True, out=dx[:, k0:])
        gemm(Ze, We.data[k0:], out=dx[:, k0:], transB=True, beta=1.0)
    elif plan.dx == "plain":
        dx = gemm(Zg, Wg.data, transB=True)
        gemm(Ze, We.data, out=dx, transB=True, beta=1.0)
    side = side_stream(Wg._graph) if (dx is not None and Wg.grad is not None and We.grad is not None and be.grad is not None) else None
    if side is not None:
        # dx is on its way to the recurrent stack; the parameter gradients are read by the optimiser only: off the critical chain
        g = Wg._graph
        side.wait_stream(torch.cuda.current_stream(g.device))
        for t in (x, Zg, Ze):
            t.record_stream(side)                  # (their memory must not be handed out again before the side stream is done)
        bw, bwe, bbe = Wg.grad_beta(), We.grad_beta(), be.grad_beta()
        with torch.cuda.stream(side):
            gemm_grouped([dict(A=x, B=Zg, out=Wg.grad, beta=bw, absmaxA=xmax, absmaxB=mg), dict(A=x, B=Ze, out=We.grad, beta=bwe, absmaxA=xmax, absmaxB=me)],
                         transA=True, role="dw")
            colsum(Ze, be.grad.view(-1), beta=bbe)
        if not hasattr(g, "side_pending") or g.side_pending is None:
            g.side_pending = []
        g.side_pending.append(side)
        Wg.grad_done()
        We.grad_done()
        be.grad_done()
        return dx
    pg = pe = None
    if Wg.grad is not None and We.grad is not None:
        pg = dict(A=x, B=Zg, out=Wg.grad, beta=Wg.grad_beta(), absmaxA=xmax, absmaxB=mg)
        pe = dict(A=x, B=Ze, out=We.grad, beta=We.grad_beta(), absmaxA=xmax, absmaxB=me)
    _moe_head_dw(gemm_grouped, pg, pe, Wg, We, be, Ze, transA=True, role="dw")
    return dx


def moe_head_xent(x, Wg, We, be, labels, vocab_size, num_mixtures, bf16=False):
    return _MoeHeadXent.apply(x, _token(Wg._graph), Wg, We, be, labels, vocab_size, num_mixtures, bool(bf16))


def moe_head(x, Wg, We, be, vocab_size, num_mixtures, bf16=False, dx_from=0):
    """dx_from: the first `dx_from` columns of x are DATA (the chain models concatenate the model input in front of what they learned:
    deep_combine_chain_model.py:66-70) -- their gradient is not computed (fp32 configuration; the returned dx holds zeros there)."""
    return _MoeHead.apply(x, _token(Wg._graph), Wg, We, be, vocab_size, num_mixtures, bool(bf16), int(dx_from))


class _Xent(torch.autograd.Function):
    """CrossEntropyLoss (W/losses.py:110-130); backward recomputes dL/dp from (p, y) with the upstream scalar read
    on the device, so no host sync and no extra elementwise pass."""

    @staticmethod
    def forward(ctx, p, labels, weights, scale):
        loss, _ = xent_fwd(p, labels, weights, want_dp=False, upstream=1.0)
        ctx.save_for_backward(p)
        ctx.labels, ctx.weights, ctx.scale = labels, weights, scale
        return loss * scale if scale != 1.0 else loss

    @staticmethod
    def backward(ctx, dloss):
        (p,) = ctx.saved_tensors
        dp = xent_bwd(p, ctx.labels, ctx.weights, dloss.reshape(1), upstream=ctx.scale)
        return dp, None, None, None


def cross_entropy(p, labels, weights=None, scale=1.0):
    return _Xent.apply(p, labels, weights, float(scale))


BA_STATS_FLOATS = _C["YT8M_BA_STATS_FLOATS"]
BA_STATS = {"min_pp": 0, "max_np": 1, "c_fn": 2, "c_fp": 3, "n_fn": 14, "n_fp": 15, "ties_max_np": 16, "ties_min_pp": 17}
BA_TOPK = 20                          # W/losses.py:331
POINTWISE_LOSSES = {k: _C["YT8M_LOSS_" + k.upper()] for k in ("weighted_xent", "mse", "hinge")}      # enum yt8m_pointwise_loss


def _loss_args(p, labels, min_classes=1):
    """(p, labels, label dtype code, B, V) of a [B, V] loss; shape errors come before the device check (they need no device)."""
    if p.dim() != 2:
        raise ValueError("expected [batch, classes] predictions, got %s" % (tuple(p.shape),))
    B, V = p.shape
    if tuple(labels.shape) != (B, V):
        raise ValueError("labels shape %s != predictions shape %s" % (tuple(labels.shape), (B, V)))
    if V < min_classes:
        raise ValueError("%d classes: top_k(k = %d) needs at least %d" % (V, min_classes, min_classes))
    _dev(p, labels)
    lab, ldt = _labels_arg(labels)
    return _f32c(p), lab, ldt, B, V


def _loss_workspace(nbytes, device):
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def batch_agreement_fwd(p, labels, agreement, batch_size, eps=XENT_EPS):
    """BatchAgreementCrossEntropyLoss (W/losses.py:281-320): (loss, stats).  stats: the batch statistics, BA_STATS_FLOATS device
    floats (BA_STATS names the readable ones) that batch_agreement_bwd takes."""
    p, lab, ldt, B, V = _loss_args(p, labels)
    L = _lib.lib()
    ws = _loss_workspace(L.yt8m_batch_agreement_workspace_bytes(B, V), p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    stats = torch.empty(BA_STATS_FLOATS, dtype=torch.float32, device=p.device)
    _lib.check(L.yt8m_batch_agreement_fwd(_p(p), _p(lab), ldt, _p(loss), _p(stats), B, V, eps, agreement, batch_size, _p(ws), _stream()))
    return loss, stats


def batch_agreement_bwd(p, labels, stats, upstream_dev, eps=XENT_EPS, upstream=1.0):
    p, lab, ldt, B, V = _loss_args(p, labels)
    _dev(stats, upstream_dev)
    dp = torch.empty_like(p)
    up = None if upstream_dev is None else _f32c(upstream_dev)
    _lib.check(_lib.lib().yt8m_batch_agreement_bwd(_p(p), _p(lab), ldt, _p(_f32c(stats)), _p(up), _p(dp), B, V, eps, upstream, _stream()))
    return dp


def topk_batch_agreement_fwd(p, labels, agreement, eps=XENT_EPS):
    """TopKBatchAgreementCrossEntropyLoss (W/losses.py:322-356): (loss, stats); stats = min_pp, then the rows' thresholds (1 + B)."""
    p, lab, ldt, B, V = _loss_args(p, labels, min_classes=BA_TOPK)
    L = _lib.lib()
    ws = _loss_workspace(L.yt8m_batch_agreement_workspace_bytes(B, V), p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    stats = torch.empty(1 + B, dtype=torch.float32, device=p.device)
    _lib.check(L.yt8m_topk_batch_agreement_fwd(_p(p), _p(lab), ldt, _p(loss), _p(stats), B, V, eps, agreement, _p(ws), _stream()))
    return loss, stats


def topk_batch_agreement_bwd(p, labels, stats, upstream_dev, agreement, eps=XENT_EPS, upstream=1.0):
    p, lab, ldt, B, V = _loss_args(p, labels, min_classes=BA_TOPK)
    _dev(stats, upstream_dev)
    dp = torch.empty_like(p)
    up = None if upstream_dev is None else _f32c(upstream_dev)
    _lib.check(_lib.lib().yt8m_topk_batch_agreement_bwd(_p(p), _p(lab), ldt, _p(_f32c(stats)), _p(up), _p(dp), B, V, eps, agreement,
                                                        upstream, _stream()))
    return dp


def pointwise_loss_fwd(p, labels, kind, c0=1.0, c1=1.0, want_dp=False, eps=XENT_EPS, upstream=1.0):
    p, lab, ldt, B, V = _loss_args(p, labels)
    L = _lib.lib()
    ws = _loss_workspace(L.yt8m_pointwise_loss_workspace_bytes(B, V), p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    dp = torch.empty_like(p) if want_dp else None
    _lib.check(L.yt8m_pointwise_loss_fwd_bwd(POINTWISE_LOSSES[kind], _p(p), _p(lab), ldt, _p(loss), _p(dp), B, V, c0, c1, eps, upstream,
                                             _p(ws), _stream()))
    return loss, dp


def pointwise_loss_bwd(p, labels, kind, upstream_dev, c0=1.0, c1=1.0, eps=XENT_EPS, upstream=1.0):
    p, lab, ldt, B, V = _loss_args(p, labels)
    _dev(upstream_dev)
    dp = torch.empty_like(p)
    up = None if upstream_dev is None else _f32c(upstream_dev)
    _lib.check(_lib.lib().yt8m_pointwise_loss_bwd(POINTWISE_LOSSES[kind], _p(p), _p(lab), ldt, _p(up), _p(dp), B, V, c0, c1, eps, upstream,
                                                  _stream()))
    return dp


class _BatchAgreementXent(torch.autograd.Function):
    """Saves p and the 20 floats of batch statistics; the backward pass recomputes dL/dp from (p, y) and them, with the upstream
    scalar read on the device: no host sync, nothing of size [B, V] kept beyond p."""

    @staticmethod
    def forward(ctx, p, labels, agreement, batch_size):
        loss, stats = batch_agreement_fwd(p, labels, agreement, batch_size)
        ctx.save_for_backward(p, stats)
        ctx.labels = labels
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, stats = ctx.saved_tensors
        return batch_agreement_bwd(p, ctx.labels, stats, dloss.reshape(1)), None, None, None


class _TopKBatchAgreementXent(torch.autograd.Function):
    """Saves p, min_pp and the rows' thresholds (1 + B floats)."""

    @staticmethod
    def forward(ctx, p, labels, agreement):
        loss, stats = topk_batch_agreement_fwd(p, labels, agreement)
        ctx.save_for_backward(p, stats)
        ctx.labels, ctx.agreement = labels, agreement
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, stats = ctx.saved_tensors
        return topk_batch_agreement_bwd(p, ctx.labels, stats, dloss.reshape(1), ctx.agreement), None, None


class _PointwiseLoss(torch.autograd.Function):
    """WeightedCrossEntropyLoss / MeanSquareErrorLoss / HingeLoss (W/losses.py:76-108, 132-148): mean_b sum_v f(p, y); the backward
    pass recomputes f' from (p, y)."""

    @staticmethod
    def forward(ctx, p, labels, kind, c0, c1):
        loss, _ = pointwise_loss_fwd(p, labels, kind, c0, c1)
        ctx.save_for_backward(p)
        ctx.args = labels, kind, c0, c1
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (p,) = ctx.saved_tensors
        labels, kind, c0, c1 = ctx.args
        return pointwise_loss_bwd(p, labels, kind, dloss.reshape(1), c0, c1), None, None, None, None


def batch_agreement_cross_entropy(p, labels, agreement, batch_size):
    """batch_size: --batch_size as the reference takes it (float(FLAGS.batch_size)), whatever the number of rows of p."""
    return _BatchAgreementXent.apply(p, labels, float(agreement), float(batch_size))


def topk_batch_agreement_cross_entropy(p, labels, agreement):
    return _TopKBatchAgreementXent.apply(p, labels, float(agreement))


def pointwise_loss(p, labels, kind, c0=1.0, c1=1.0):
    """kind: "weighted_xent" (c0 / c1 = false negative / false positive punishment), "mse" or "hinge" (c0 = b)."""
    return _PointwiseLoss.apply(p, labels, kind, float(c0), float(c1))


# ---- the --loss_function branches of Z's CrossEntropyLoss (Z/losses.py:64-168); csrc/xent_variants.hip --------------------------
XENT_VARIANTS = {"loss_" + k: _C["YT8M_XV_" + k.upper()] for k in ("square", "sqrt", "jsd", "mix", "weight", "margin", "relabel")}   # enum yt8m_xent_variant
XV_STATS_FLOATS = _C["YT8M_XV_STATS_FLOATS"]
XV_STATS = {k: _C["YT8M_XV_STAT_" + k.upper()] for k in ("loss", "pre", "flag", "pos", "neg")}


def xent_variant_fwd(p, labels, kind, c0=0.5, eps=XENT_EPS):
    """(loss, stats, argmax) of one --loss_function kind, unscaled.  stats: XV_STATS_FLOATS device floats (XV_STATS names the readable
    ones); argmax: the rows' argmax of p as [B] int32 for "loss_relabel", None for the other kinds.  c0: --jsd_pi ("loss_jsd" alone)."""
    code = XENT_VARIANTS[kind]
    p, lab, ldt, B, V = _loss_args(p, labels)
    L = _lib.lib()
    ws = _loss_workspace(L.yt8m_xent_variant_workspace_bytes(B, V), p.device)
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    stats = torch.empty(XV_STATS_FLOATS, dtype=torch.float32, device=p.device)
    argmax = torch.empty(B, dtype=torch.int32, device=p.device) if kind == "loss_relabel" else None
    _lib.check(L.yt8m_xent_variant_fwd(code, _p(p), _p(lab), ldt, _p(loss), _p(stats), _p(argmax), B, V, c0, eps, _p(ws), _stream()))
    return loss, stats, argmax


def xent_variant_bwd(p, labels, kind, stats, argmax, upstream_dev, c0=0.5, eps=XENT_EPS, upstream=1.0):
    code = XENT_VARIANTS[kind]
    p, lab, ldt, B, V = _loss_args(p, labels)
    _dev(stats, argmax, upstream_dev)
    dp = torch.empty_like(p)
    up = None if upstream_dev is None else _f32c(upstream_dev)
    _lib.check(_lib.lib().yt8m_xent_variant_bwd(code, _p(p), _p(lab), ldt, _p(None if stats is None else _f32c(stats)), _p(argmax), _p(up),
                                                _p(dp), B, V, c0, eps, upstream, _stream()))
    return dp


class _XentVariant(torch.autograd.Function):
    """Saves p, the 16 floats of stats and (loss_relabel) the rows' argmax; the backward pass recomputes dL/dp from (p, y) and them, with
    the upstream scalar read on the device: no host sync, nothing of size [B, V] kept beyond p."""

    @staticmethod
    def forward(ctx, p, labels, kind, c0, scale):
        loss, stats, argmax = xent_variant_fwd(p, labels, kind, c0)
        ctx.save_for_backward(p, stats)
        ctx.args = labels, kind, c0, scale, argmax
        return loss * scale if scale != 1.0 else loss

    @staticmethod
    def backward(ctx, dloss):
        p, stats = ctx.saved_tensors
        labels, kind, c0, scale, argmax = ctx.args
        return xent_variant_bwd(p, labels, kind, stats, argmax, dloss.reshape(1), c0, upstream=scale), None, None, None, None


def xent_variant(p, labels, kind, c0=0.5, scale=1.0):
    """kind: a key of XENT_VARIANTS (the reference's --loss_function names); c0: --jsd_pi; scale multiplies the whole loss."""
    if kind not in XENT_VARIANTS:
        raise ValueError("unknown loss kind %r: one of %s" % (kind, ", ".join(XENT_VARIANTS)))
    return _XentVariant.apply(p, labels, kind, float(c0), float(scale))
