"""Host tests (no GPU) of the Python layer in front of the grouped GEMM kernels (yt8m_amd/ops.py): what each wrapper hands to the
library -- the yt8m_gemm_problem fields, the launches a group is cut into and the per-problem side arrays that travel with them --,
every error it raises, the image buffers' sizes and the launch / grad_done() order of the MoE head's weight-gradient tail.

The library is replaced by a recorder: every call is noted with its arguments and returns 0; only the pure host queries
(yt8m_x3_image_bytes, yt8m_moe_mix_bwd_bf16_partial_rows) answer with the real library's value.  Operands are CPU tensors.

Everything here holds for the wrappers as they were before they shared one marshaller (same names, same recorded calls) -- the proof
that the marshalling did not change -- except the tests whose docstrings say how they differ: the two new rejections (`*_new_rejection`),
bf16-NT groups of more than four, and the allocator's own test (a new name)."""
import pytest
import torch

import yt8m_amd._lib as _lib
import yt8m_amd.ops as ops
from library_recorder import install

REAL_DEV = ops._dev


@pytest.fixture()
def rec(monkeypatch):
    return install(monkeypatch)


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def bf16(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


AUTO = ("yt8m_gemm_auto_grouped", "yt8m_gemm_auto_grouped_ex")


def _one_auto(rec):
    (name, args), = rec.calls(*AUTO)
    assert name == "yt8m_gemm_auto_grouped" and args[2] == 1
    return args[0], args[1], args[3][0]


# ---- the strided families: gemm / gemm_grouped / gemm_simple ------------------------------------------------------------------------
def test_gemm_contiguous_operands(rec):
    A, B = f32(5, 7), f32(7, 3)
    out = ops.gemm(A, B)
    ta, tb, p = _one_auto(rec)
    assert (ta, tb) == (0, 0)
    assert p == dict(M=5, N=3, K=7, A=A.data_ptr(), lda=7, B=B.data_ptr(), ldb=3, C=out.data_ptr(), ldc=3, bias=None, beta=0.0)
    assert out.dtype == torch.float32 and tuple(out.shape) == (5, 3)
    # the workspace and its size in bytes travel with every launch
    args = rec.calls(*AUTO)[0][1]
    assert args[4] == rec.ws.data_ptr() and args[5] == rec.ws.numel() * 4


def test_gemm_column_window_keeps_the_parents_row_stride(rec):
    wide, Bw = f32(5, 20), f32(7, 12)
    A, B = wide[:, 4:11], Bw[:, 2:5]
    into = f32(5, 9)
    out = ops.gemm(A, B, out=into[:, 3:6])
    _, _, p = _one_auto(rec)
    assert (p["A"], p["lda"]) == (A.data_ptr(), 20) and (p["B"], p["ldb"]) == (B.data_ptr(), 12)
    assert (p["C"], p["ldc"]) == (into.data_ptr() + 12, 9) and out.data_ptr() == p["C"]


def test_gemm_inner_stride_not_one_passes_a_contiguous_copy(rec):
    A = f32(7, 5).t()                                    # [5, 7], strides (1, 5)
    B = f32(7, 3)
    ops.gemm(A, B)
    _, _, p = _one_auto(rec)
    assert p["A"] != A.data_ptr() and p["lda"] == 7 and (p["M"], p["K"]) == (5, 7)
    assert (p["B"], p["ldb"]) == (B.data_ptr(), 3)


def test_gemm_single_row_and_single_column(rec):
    A, B = f32(1, 7), f32(7, 1)
    out = ops.gemm(A, B)
    _, _, p = _one_auto(rec)
    assert (p["M"], p["N"], p["K"]) == (1, 1, 7) and (p["lda"], p["ldb"], p["ldc"]) == (7, 1, 1) and tuple(out.shape) == (1, 1)
    rec.log.clear()
    wide = f32(1, 20)[:, 3:10]                           # one row of a wider matrix: ld = max(cols, 1), not the parent's stride
    ops.gemm(wide, f32(7, 4))
    _, _, p = _one_auto(rec)
    assert (p["A"], p["lda"], p["ldc"]) == (wide.data_ptr(), 7, 4)
    rec.log.clear()
    col = f32(1, 5).t()                                  # out [5, 1] with stride(1) = 5: accepted when N == 1
    assert col.stride(1) != 1
    got = ops.gemm(f32(5, 7), B, out=col)
    _, _, p = _one_auto(rec)
    assert got is col and (p["C"], p["ldc"]) == (col.data_ptr(), col.stride(0))
    rec.log.clear()
    ops.gemm(f32(5, 0), f32(0, 3))                       # K = 0: the leading dimensions keep the max(., 1) floor on one-row operands
    _, _, p = _one_auto(rec)
    assert (p["M"], p["N"], p["K"]) == (5, 3, 0)


@pytest.mark.parametrize("transA,transB", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_grouped_transpositions(rec, transA, transB):
    M, N, K = 5, 3, 7
    A = f32(K, M) if transA else f32(M, K)
    B = f32(N, K) if transB else f32(K, N)
    out, = ops.gemm_grouped([dict(A=A, B=B)], transA=transA, transB=transB)
    ta, tb, p = _one_auto(rec)
    assert (ta, tb) == (int(transA), int(transB))
    assert (p["M"], p["N"], p["K"]) == (M, N, K) and (p["lda"], p["ldb"], p["ldc"]) == (A.shape[1], B.shape[1], N)
    assert tuple(out.shape) == (M, N)


@pytest.mark.parametrize("role,transA,transB,want", [
    (None, False, False, 0), (None, True, False, 1),
    ("dw", True, False, 1 | ops.GEMM_ROLE_DW), ("dw", False, False, 0), ("dw", True, True, 1),
    ("h2", False, False, ops.GEMM_ROLE_H2), ("h2", True, False, 1 | ops.GEMM_ROLE_H2)])
def test_gemm_grouped_role_flags(rec, role, transA, transB, want):
    A = f32(7, 5) if transA else f32(5, 7)
    B = f32(3, 7) if transB else f32(7, 3)
    ops.gemm_grouped([dict(A=A, B=B)], transA=transA, transB=transB, role=role)
    ta, tb, _ = _one_auto(rec)
    assert (ta, tb) == (want, int(transB))
    (_, sargs), = rec.calls("yt8m_gemm_auto_scratch_bytes")          # the scratch query sees the same flags
    assert sargs[0] == want and sargs[1] == int(transB) and sargs[2] == 1


def test_gemm_grouped_bias_on_one_item_and_beta_into_out(rec):
    bias = f32(3)
    into = f32(5, 3)
    outs = ops.gemm_grouped([dict(A=f32(5, 7), B=f32(7, 3)), dict(A=f32(5, 7), B=f32(7, 3), bias=bias),
                             dict(A=f32(5, 7), B=f32(7, 3), out=into, beta=1.0)])
    (name, args), = rec.calls(*AUTO)
    assert name == "yt8m_gemm_auto_grouped" and args[2] == 3
    p0, p1, p2 = args[3]
    assert (p0["bias"], p1["bias"], p2["bias"]) == (None, bias.data_ptr(), None)
    assert (p0["beta"], p1["beta"], p2["beta"]) == (0.0, 0.0, 1.0)
    assert outs[2] is into and [p["C"] for p in args[3]] == [o.data_ptr() for o in outs]


def test_gemm_simple_goes_through_the_same_problem(rec):
    A, B, bias = f32(5, 20)[:, 2:9], f32(7, 3), f32(3)
    out = ops.gemm_simple(A, B, bias=bias)
    (_, a), = rec.calls("yt8m_gemm_f32")
    assert a[:12] == [0, 0, 5, 3, 7, A.data_ptr(), 20, B.data_ptr(), 3, out.data_ptr(), 3, bias.data_ptr()] and a[12] == 0.0
    pr, o, keep = ops._problem(A, B, None, False, False, bias, 0.0)
    assert (pr.M, pr.N, pr.K, pr.lda, pr.ldb, pr.ldc) == (5, 3, 7, 20, 3, 3) and pr.C == o.data_ptr() and len(keep) == 3


def test_gemm_errors(rec):
    A, B = f32(5, 7), f32(7, 3)
    with pytest.raises(ValueError, match=r"^gemm: inner dimensions differ \(7 vs 6\)"):
        ops.gemm(A, f32(6, 3))
    with pytest.raises(ValueError, match=r"^beta != 0 needs an output tensor"):
        ops.gemm(A, B, beta=1.0)
    for bad in (f32(5, 4), f32(3, 5).t(), torch.zeros((5, 3), dtype=torch.float64), f32(15)):
        with pytest.raises(ValueError, match=r"^gemm: bad output tensor"):
            ops.gemm(A, B, out=bad)
    with pytest.raises(ValueError, match=r"^bias size mismatch"):
        ops.gemm(A, B, bias=f32(4))
    with pytest.raises(TypeError, match=r"^expected float32"):
        ops.gemm(A, B, bias=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError, match=r"^expected float32"):
        ops.gemm(A.double(), B)
    with pytest.raises(ValueError, match=r"^expected a 2-D tensor"):
        ops.gemm(f32(2, 5, 7), B)
    with pytest.raises(ValueError, match=r"^role must be None, 'dw' or 'h2'"):
        ops.gemm(A, B, role="dx")
    with pytest.raises(ValueError, match=r"^gemm: inner dimensions differ"):
        ops.gemm_simple(A, f32(6, 3))
    assert not rec.calls(*AUTO) and not rec.calls("yt8m_gemm_f32")


def test_every_family_refuses_host_tensors(rec, monkeypatch):
    x3, h2, b1 = ops.x3_split(f32(5, 8))[0], ops.h2_split(f32(5, 8))[0], ops.bf16_image(f32(5, 8))
    rec.log.clear()
    monkeypatch.setattr(ops, "_dev", REAL_DEV)
    for call in (lambda: ops.gemm(f32(5, 7), f32(7, 3)), lambda: ops.gemm_simple(f32(5, 7), f32(7, 3)),
                 lambda: ops.gemm_bf16_nt_grouped([dict(A=bf16(5, 8), B=bf16(3, 8))]),
                 lambda: ops.gemm_x3_grouped([dict(A=x3, B=x3)]), lambda: ops.gemm_h2_grouped([dict(A=h2, B=h2)]),
                 lambda: ops.gemm_b1_grouped([dict(A=b1, B=b1)])):
        with pytest.raises(_lib.Yt8mHipError, match="there is no CPU fallback"):
            call()
    assert not rec.log


# ---- bf16 NT ------------------------------------------------------------------------------------------------------------------------
def test_bf16_nt_marshalling(rec):
    A, B = bf16(5, 8), bf16(3, 8)
    wide = bf16(5, 24)[:, 8:16]
    At = bf16(8, 5).t()                                  # inner stride 5: a contiguous copy is passed
    bias = f32(3)
    into = f32(5, 9)
    outs = ops.gemm_bf16_nt_grouped([dict(A=A, B=B), dict(A=wide, B=B, bias=bias), dict(A=At, B=B, out=into[:, 3:6], beta=1.0),
                                     dict(A=bf16(1, 8), B=bf16(1, 8))])
    (_, args), = rec.calls("yt8m_gemm_bf16_nt_grouped")              # up to four problems: one launch
    assert args[0] == 4 and args[2] == rec.ws.data_ptr() and args[3] == rec.ws.numel() * 4
    p = args[1]
    assert p[0] == dict(M=5, N=3, K=8, A=A.data_ptr(), lda=8, B=B.data_ptr(), ldb=8, C=outs[0].data_ptr(), ldc=3, bias=None, beta=0.0)
    assert (p[1]["A"], p[1]["lda"], p[1]["bias"]) == (wide.data_ptr(), 24, bias.data_ptr())
    assert p[2]["A"] != At.data_ptr() and p[2]["lda"] == 8 and (p[2]["C"], p[2]["ldc"], p[2]["beta"]) == (into.data_ptr() + 12, 9, 1.0)
    assert (p[3]["M"], p[3]["N"], p[3]["lda"], p[3]["ldb"], p[3]["ldc"]) == (1, 1, 8, 8, 1)
    assert [q["C"] for q in p] == [o.data_ptr() for o in outs]


def test_bf16_nt_groups_of_five_launch_as_four_and_one(rec):
    """Differs from the parent, which handed the library all five at once: yt8m_gemm_bf16_nt_grouped takes 1..4 problems and refused
    them (YT8M_E_BADARG).  Groups of up to four -- every caller's -- launch as before."""
    outs = ops.gemm_bf16_nt_grouped([dict(A=bf16(5 + i, 8), B=bf16(3, 8)) for i in range(5)])
    c = rec.calls("yt8m_gemm_bf16_nt_grouped")
    assert [(a[0], len(a[1])) for _, a in c] == [(4, 4), (1, 1)]
    assert [p["C"] for _, a in c for p in a[1]] == [o.data_ptr() for o in outs] and [p["M"] for _, a in c for p in a[1]] == [5, 6, 7, 8, 9]


def test_bf16_nt_errors(rec):
    A, B = bf16(5, 8), bf16(3, 8)
    for a, b in ((f32(5, 8), B), (A, f32(3, 8)), (bf16(2, 5, 8), B)):
        with pytest.raises(TypeError, match=r"^gemm_bf16_nt: operands must be 2-D bfloat16"):
            ops.gemm_bf16_nt_grouped([dict(A=a, B=b)])
    with pytest.raises(ValueError, match=r"^gemm_bf16_nt: inner dimensions differ \(8 vs 6\)"):
        ops.gemm_bf16_nt_grouped([dict(A=A, B=bf16(3, 6))])
    with pytest.raises(ValueError, match=r"^beta != 0 needs an output tensor"):
        ops.gemm_bf16_nt_grouped([dict(A=A, B=B, beta=1.0)])
    for bad in (f32(5, 4), f32(3, 5).t(), torch.zeros((5, 3), dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match=r"^gemm_bf16_nt: bad output tensor"):
            ops.gemm_bf16_nt_grouped([dict(A=A, B=B, out=bad)])
    with pytest.raises(TypeError, match=r"^expected float32"):
        ops.gemm_bf16_nt_grouped([dict(A=A, B=B, bias=torch.zeros(3, dtype=torch.float64))])
    assert not rec.calls("yt8m_gemm_bf16_nt_grouped")


# ---- the image families -------------------------------------------------------------------------------------------------------------
def _images(kind, rows, K, **kw):
    x = f32(rows, K)
    if kind == "x3":
        return ops.x3_split(x)[0]
    if kind == "h2":
        return ops.h2_split(x, **kw)[0]
    return ops.bf16_image(x)


IMAGE_FAMILIES = {"x3": ("gemm_x3_grouped", ("yt8m_gemm_x3_nt_grouped",)), "h2": ("gemm_h2_grouped", ("yt8m_gemm_h2_nt_grouped",)),
                  "b1": ("gemm_b1_grouped", ("yt8m_gemm_b1_nt_grouped", "yt8m_gemm_b1_nt_grouped_bf16c"))}


@pytest.mark.parametrize("kind", ["x3", "h2", "b1"])
def test_image_family_marshalling(rec, kind):
    wrapper, launches = IMAGE_FAMILIES[kind]
    A, B, a1, b1 = _images(kind, 5, 8), _images(kind, 3, 8), _images(kind, 1, 8), _images(kind, 1, 8)
    bias = f32(3)
    into = f32(5, 9)
    col = f32(1, 5).t()
    rec.log.clear()
    outs = getattr(ops, wrapper)([dict(A=A, B=B), dict(A=A, B=B, bias=bias), dict(A=A, B=B, out=into[:, 3:6], beta=1.0),
                                  dict(A=a1, B=b1)])
    (_, args), = rec.calls(*launches)
    assert args[0] == 4 and args[-3:] == [rec.ws.data_ptr(), rec.ws.numel() * 4, None]
    p = args[1]
    assert p[0] == dict(M=5, N=3, K=8, A=A.buf.data_ptr(), lda=0, B=B.buf.data_ptr(), ldb=0, C=outs[0].data_ptr(), ldc=3, bias=None,
                        beta=0.0)
    assert (p[1]["bias"], p[1]["beta"]) == (bias.data_ptr(), 0.0)
    assert (p[2]["C"], p[2]["ldc"], p[2]["beta"]) == (into.data_ptr() + 12, 9, 1.0) and outs[2].data_ptr() == p[2]["C"]
    assert (p[3]["M"], p[3]["N"], p[3]["ldc"]) == (1, 1, 1)
    assert all(o.dtype == torch.float32 for o in outs)
    rec.log.clear()
    got, = getattr(ops, wrapper)([dict(A=A, B=b1, out=col)])         # out [5, 1] with stride(1) != 1
    (_, args), = rec.calls(*launches)
    assert got is col and (args[1][0]["C"], args[1][0]["ldc"]) == (col.data_ptr(), col.stride(0))


@pytest.mark.parametrize("kind", ["x3", "h2", "b1"])
def test_image_family_errors(rec, kind):
    wrapper, launches = IMAGE_FAMILIES[kind]
    fn = getattr(ops, wrapper)
    prefix = "gemm_" + kind
    A, B = _images(kind, 5, 8), _images(kind, 3, 8)
    rec.log.clear()
    with pytest.raises(ValueError, match=r"^%s: inner dimensions differ \(8 vs 6\)" % prefix):
        fn([dict(A=A, B=_images(kind, 3, 6))])
    with pytest.raises(ValueError, match=r"^beta != 0 needs an output tensor"):
        fn([dict(A=A, B=B, beta=1.0)])
    for bad in (f32(5, 4), f32(3, 5).t(), torch.zeros((5, 3), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"^%s: bad output tensor" % prefix):
            fn([dict(A=A, B=B, out=bad)])
    with pytest.raises(TypeError, match=r"^expected float32"):
        fn([dict(A=A, B=B, bias=torch.zeros(3, dtype=torch.float64))])
    if kind == "x3":
        with pytest.raises(ValueError, match=r"^bias size mismatch"):
            fn([dict(A=A, B=B, bias=f32(4))])
        for a, b in ((f32(5, 8), B), (A, f32(3, 8))):
            with pytest.raises(TypeError, match=r"^gemm_x3: operands must be X3Image"):
                fn([dict(A=a, B=b)])
    if kind == "h2":
        x3 = _images("x3", 5, 8)
        for a, b in ((x3, B), (A, x3), (f32(5, 8), B)):
            with pytest.raises(TypeError, match=r"^gemm_h2: operands must be H2Image"):
                fn([dict(A=a, B=b)])
    if kind == "b1":
        with pytest.raises(ValueError, match=r"^gemm_b1: bad output tensor"):
            fn([dict(A=A, B=B, out=torch.zeros((5, 3), dtype=torch.float16))])
        for bad in (dict(out=torch.zeros((5, 4), dtype=torch.bfloat16)[:, :3], beta=1.0), dict(out=torch.zeros((5, 3), dtype=torch.bfloat16))):
            with pytest.raises(ValueError, match=r"^gemm_b1: a bf16 output takes beta = 0 and a row pitch that is a multiple of 4"):
                fn([dict(A=A, B=B, **bad)])
    assert not rec.calls(*launches)


@pytest.mark.parametrize("wrapper,make", [("gemm_bf16_nt_grouped", lambda r: bf16(r, 8)), ("gemm_h2_grouped", lambda r: _images("h2", r, 8)),
                                          ("gemm_b1_grouped", lambda r: _images("b1", r, 8))])
def test_missized_bias_new_rejection(rec, wrapper, make):
    """Differs from the parent, which handed a bias of any length to the kernel (read out of bounds when shorter than N)."""
    rec.log.clear()
    with pytest.raises(ValueError, match=r"^bias size mismatch"):
        getattr(ops, wrapper)([dict(A=make(5), B=make(3), bias=f32(2))])
    getattr(ops, wrapper)([dict(A=make(5), B=make(3), bias=f32(1, 3))])      # N elements of any shape, as gemm takes them


def test_wrong_plane_count_new_rejection(rec):
    """Differs from the parent, where a two-plane image passed gemm_x3's isinstance check (H2Image subclasses X3Image), a one-plane image
    was a plain X3Image over a buffer a third of the size, and gemm_b1 checked nothing."""
    img = {k: (_images(k, 5, 8), _images(k, 3, 8)) for k in ("x3", "h2", "b1")}
    assert [img[k][0].planes for k in ("x3", "h2", "b1")] == [3, 2, 1]
    assert ops.X3Image(torch.empty(16, dtype=torch.uint8), 1, 1).planes == 3
    assert ops.H2Image(torch.empty(16, dtype=torch.uint8), 1, 1, 2.0, None).planes == 2
    rec.log.clear()
    for kind, message in (("x3", "gemm_x3: operands must be X3Image"), ("h2", "gemm_h2: operands must be H2Image"),
                          ("b1", "gemm_b1: operands must be one-plane images")):
        fn = getattr(ops, IMAGE_FAMILIES[kind][0])
        for other in ("x3", "h2", "b1"):
            if other == kind:
                continue
            for a, b in ((img[other][0], img[kind][1]), (img[kind][0], img[other][1])):
                with pytest.raises(TypeError, match="^" + message):
                    fn([dict(A=a, B=b)])
    with pytest.raises(TypeError, match="^gemm_b1: operands must be one-plane images"):
        ops.gemm_b1_grouped([dict(A=f32(5, 8), B=img["b1"][1])])
    assert not rec.log


# ---- chunking: the problem array and every side array are cut by the same indices ---------------------------------------------------
def test_x3_groups_of_five_launch_as_four_and_one(rec):
    items = [dict(A=_images("x3", 5 + i, 8), B=_images("x3", 3, 8)) for i in range(5)]
    rec.log.clear()
    outs = ops.gemm_x3_grouped(items)
    c = rec.calls("yt8m_gemm_x3_nt_grouped")
    assert [a[0] for _, a in c] == [4, 1] and [len(a[1]) for _, a in c] == [4, 1]
    assert [p["C"] for _, a in c for p in a[1]] == [o.data_ptr() for o in outs]
    assert [p["M"] for _, a in c for p in a[1]] == [5, 6, 7, 8, 9]
    assert [p["A"] for _, a in c for p in a[1]] == [it["A"].buf.data_ptr() for it in items]


def test_h2_groups_of_five_carry_alpha_and_scale_words_with_their_problem(rec):
    word = torch.zeros(1, dtype=torch.int32)
    wordb = torch.zeros(1, dtype=torch.int32)
    buf = torch.empty(4096, dtype=torch.uint8)
    items = [dict(A=_images("h2", 5 + i, 8, scale=2.0), B=_images("h2", 3, 8)) for i in range(4)]
    items.append(dict(A=ops.H2Image(buf, 9, 8, 8.0, word), B=ops.H2Image(buf, 3, 8, 1.0, None)))
    items[1]["B"] = ops.H2Image(buf, 3, 8, 4.0, wordb)
    rec.log.clear()
    outs = ops.gemm_h2_grouped(items)
    c = rec.calls("yt8m_gemm_h2_nt_grouped")
    assert [a[0] for _, a in c] == [4, 1]
    (_, first), (_, last) = c
    assert [p["C"] for p in first[1]] == [o.data_ptr() for o in outs[:4]] and last[1][0]["C"] == outs[4].data_ptr()
    assert first[2] == [0.5, 0.125, 0.5, 0.5] and first[3] == [None] * 4 and first[4] == [None, wordb.data_ptr(), None, None]
    assert last[2] == [0.125] and last[3] == [word.data_ptr()] and last[4] == [None] and last[1][0]["M"] == 9
    assert first[5:] == [rec.ws.data_ptr(), rec.ws.numel() * 4, None]


def test_b1_groups_of_five_carry_the_bf16_output_mask_with_their_problem(rec):
    items = [dict(A=_images("b1", 5 + i, 8), B=_images("b1", 8, 8)) for i in range(5)]
    items[1]["out_dtype"] = torch.bfloat16                           # allocated by the wrapper: pitch N = 8
    given = torch.zeros((9, 12), dtype=torch.bfloat16)[:, :8]        # a window of a wider bf16 matrix, pitch 12
    items[4]["out"] = given
    rec.log.clear()
    outs = ops.gemm_b1_grouped(items)
    c = rec.calls("yt8m_gemm_b1_nt_grouped", "yt8m_gemm_b1_nt_grouped_bf16c")
    assert [(n, a[0], a[2]) for n, a in c] == [("yt8m_gemm_b1_nt_grouped_bf16c", 4, 0b10), ("yt8m_gemm_b1_nt_grouped_bf16c", 1, 0b1)]
    assert [o.dtype for o in outs] == [torch.float32, torch.bfloat16, torch.float32, torch.float32, torch.bfloat16]
    assert outs[4] is given and c[1][1][1][0]["C"] == given.data_ptr() and c[1][1][1][0]["ldc"] == 12
    assert [p["C"] for _, a in c for p in a[1]] == [o.data_ptr() for o in outs]
    rec.log.clear()
    ops.gemm_b1_grouped(items[2:4])                                  # no bf16 output: the plain entry point, no mask argument
    (name, a), = rec.calls("yt8m_gemm_b1_nt_grouped", "yt8m_gemm_b1_nt_grouped_bf16c")
    assert name == "yt8m_gemm_b1_nt_grouped" and a[0] == 2 and a[2] == rec.ws.data_ptr()


def test_auto_groups_of_sixty_five_launch_as_sixty_four_and_one(rec):
    word = torch.zeros(1, dtype=torch.float32)
    items = [dict(A=f32(5, 7), B=f32(7, 3)) for _ in range(65)]
    items[64]["absmaxB"] = word
    outs = ops.gemm_grouped(items, transA=False, role="h2")
    c = rec.calls(*AUTO)
    assert [(n, a[2], len(a[3])) for n, a in c] == [("yt8m_gemm_auto_grouped", 64, 64), ("yt8m_gemm_auto_grouped_ex", 1, 1)]
    assert [p["C"] for _, a in c for p in a[3]] == [o.data_ptr() for o in outs]
    ex = c[1][1]
    assert ex[4] == [None] and ex[5] == [word.data_ptr()] and ex[6] == rec.ws.data_ptr()
    assert [a[2] for _, a in rec.calls("yt8m_gemm_auto_scratch_bytes")] == [64, 1]
    rec.log.clear()
    items[3]["absmaxA"] = word                                       # a word in the first launch only: _ex there, plain for the rest
    del items[64]["absmaxB"]
    ops.gemm_grouped(items)
    c = rec.calls(*AUTO)
    assert [(n, a[2]) for n, a in c] == [("yt8m_gemm_auto_grouped_ex", 64), ("yt8m_gemm_auto_grouped", 1)]
    assert c[0][1][4] == [None] * 3 + [word.data_ptr()] + [None] * 60 and c[0][1][5] == [None] * 64


def test_fp32_groups_of_five_launch_as_four_and_one_without_x3(rec, monkeypatch):
    monkeypatch.setattr(ops, "X3", False)
    outs = ops.gemm_grouped([dict(A=f32(7, 5 + i), B=f32(7, 3)) for i in range(5)], transA=True, role="dw")
    c = rec.calls("yt8m_gemm_f32_grouped")
    assert [(a[0], a[1], a[2], len(a[3])) for _, a in c] == [(1, 0, 4, 4), (1, 0, 1, 1)]          # plain 0 / 1 flags: no role bits
    assert [p["C"] for _, a in c for p in a[3]] == [o.data_ptr() for o in outs] and [p["M"] for _, a in c for p in a[3]] == [5, 6, 7, 8, 9]
    assert not rec.calls(*AUTO) and c[0][1][4:] == [rec.ws.data_ptr(), rec.ws.numel() * 4, None]


# ---- image buffers ------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (32, 16), (33, 17), (4716, 1152)]


def _want_bytes(rows, K, planes):
    return max(_lib.lib().yt8m_x3_image_bytes(rows, K) // 3 * planes, 16)


@pytest.mark.parametrize("rows,K", SIZES)
def test_image_sizes_through_the_split_functions(rec, rows, K):
    x = f32(rows, K)
    for planes, (ip, it) in ((3, ops.x3_split(x, trans=True)), (2, ops.h2_split(x, trans=True)), (1, ops.bf16_image(x, both=True))):
        assert ip.buf.dtype == torch.uint8 and (ip.rows, ip.K, it.rows, it.K) == (rows, K, K, rows)
        assert ip.buf.numel() == _want_bytes(rows, K, planes) and it.buf.numel() == _want_bytes(K, rows, planes)


@pytest.mark.parametrize("rows,K", SIZES)
@pytest.mark.parametrize("planes", [1, 2, 3])
def test_image_buffer_allocator(rec, rows, K, planes):
    """New with the allocator (the sizes it replaces are pinned by test_image_sizes_through_the_split_functions)."""
    buf = ops.image_buffer(rows, K, planes, torch.device("cpu"))
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.numel() == _want_bytes(rows, K, planes)
    assert ops.image_bytes(rows, K, planes) == _lib.lib().yt8m_x3_image_bytes(rows, K) // 3 * planes
    assert ops.image_buffer(0, K, planes, torch.device("cpu")).numel() == 16          # the floor


def test_split_passes_receive_the_buffers_they_made(rec):
    x = f32(5, 20)[:, 2:10]
    ip, it = ops.x3_split(x, trans=True, scale=0.5)
    (_, a), = rec.calls("yt8m_x3_split")
    assert a == [x.data_ptr(), 5, 8, 20, 0.5, ip.buf.data_ptr(), it.buf.data_ptr(), None]
    rec.log.clear()
    only_t = ops.bf16_image(x, transpose=True)
    (_, a), = rec.calls("yt8m_bf16_image")
    assert a == [x.data_ptr(), 5, 8, 20, 1.0, None, only_t.buf.data_ptr(), None] and (only_t.rows, only_t.K) == (8, 5)
    rec.log.clear()
    hp, ht = ops.h2_split(x, plain=False, trans=True, scale=4.0)
    (_, a), = rec.calls("yt8m_h2_split")
    assert hp is None and a == [x.data_ptr(), 5, 8, 20, 4.0, None, None, ht.buf.data_ptr(), None, None] and ht.scale == 4.0 and ht.dinv is None


# ---- the MoE head's weight-gradient tail --------------------------------------------------------------------------------------------
class _Graph(object):
    def __init__(self, hook):
        self.grad_ready_hook = hook
        self.device = torch.device("cpu")


class _Var(object):
    def __init__(self, name, shape, graph, log):
        self.name, self._graph, self._log = name, graph, log
        self.data, self.grad = torch.zeros(shape), torch.zeros(shape)
        self.trainable = True

    def grad_beta(self):
        return 0.0

    def grad_done(self):
        self._log.append(("grad_done", self.name))


B_, D_, NG, NE = 512, 4, 6, 4            # 512 even rows: what the bf16 forms ask of x


def _plan(bf16, M=2):
    """The head's plan at these shapes, no dx: fp32 -> the fp32 backward; bf16 -> the fused mixing backward (M = 2) or the casts (M = 3)."""
    return ops._moe_head_plan(B_, D_, NG, NE, NE // 2, M, bf16, training=True, need_dx=False)


def _head(rec, hook):
    g = _Graph(hook)
    Wg, We, be = _Var("Wg", (D_, NG), g, rec.log), _Var("We", (D_, NE), g, rec.log), _Var("be", (NE,), g, rec.log)
    return f32(B_, D_), f32(B_, NG), f32(B_, NE), Wg, We, be


def _tail(rec, launch, Wg, We):
    """The recorded order from the first weight-gradient launch on: (launch, [which gradient each problem writes]) and grad_done()s."""
    names = {Wg.grad.data_ptr(): "Wg", We.grad.data_ptr(): "We"}
    seq = []
    for name, a in rec.log:
        if name == "grad_done":
            seq.append(("grad_done", a))
        elif name == "yt8m_colsum_f32":
            seq.append(("colsum", a[4]))
        elif name in launch:
            probs = next(v for v in a if isinstance(v, list) and v and isinstance(v[0], dict))
            seq.append(("launch", [names[p["C"]] for p in probs]))
    return seq


FORMS = {
    "fp32": (lambda x, Zg, Ze, Wg, We, be: ops._moe_head_param_grads(_plan(False), x, Zg, Ze, Wg, We, be), AUTO),
    "bf16": (lambda x, Zg, Ze, Wg, We, be: ops._moe_head_param_grads(_plan(True, M=3), x, Zg, Ze, Wg, We, be), ("yt8m_gemm_bf16_nt_grouped",)),
    "bf16_fused": (lambda x, Zg, Ze, Wg, We, be: ops._moe_head_bwd_bf16_fused(_plan(True), {}, x, Zg, Ze, Wg, We, be, NE // 2, 2, dp=f32(B_, NE // 2)),
                   ("yt8m_gemm_bf16_nt_grouped",)),
    "bf16_images": (lambda x, Zg, Ze, Wg, We, be: ops._moe_head_bwd_bf16_images(_plan(True), {}, x, Zg, Ze, Wg, We, be, NE // 2, 2, f32(B_, NE // 2),
                                                                                   None, 0, 1.0, None), ("yt8m_gemm_b1_nt_grouped",)),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_moe_head_weight_gradient_tail_order(rec, form):
    run, launch = FORMS[form]
    x, Zg, Ze, Wg, We, be = _head(rec, None)
    run(x, Zg, Ze, Wg, We, be)
    assert _tail(rec, launch, Wg, We) == [("launch", ["Wg", "We"]), ("grad_done", "Wg"), ("grad_done", "We"),
                                          ("colsum", be.grad.data_ptr()), ("grad_done", "be")]
    rec.log.clear()
    x, Zg, Ze, Wg, We, be = _head(rec, lambda *a: None)             # data parallel: the gate gradient is released before the expert product
    run(x, Zg, Ze, Wg, We, be)
    assert _tail(rec, launch, Wg, We) == [("launch", ["Wg"]), ("grad_done", "Wg"), ("launch", ["We"]), ("grad_done", "We"),
                                          ("colsum", be.grad.data_ptr()), ("grad_done", "be")]


def test_moe_head_tail_without_gradient_slots(rec):
    x, Zg, Ze, Wg, We, be = _head(rec, None)
    Wg.grad = None                                                   # frozen gate weights: no product, no grad_done for either matrix
    ops._moe_head_param_grads(_plan(False), x, Zg, Ze, Wg, We, be)
    assert [e for e in rec.log if e[0] in AUTO + ("grad_done",)] == [("grad_done", "be")]
    rec.log.clear()
    be.grad = None
    ops._moe_head_param_grads(_plan(False), x, Zg, Ze, Wg, We, be)
    assert not [e for e in rec.log if e[0] in AUTO + ("grad_done", "yt8m_colsum_f32")]
