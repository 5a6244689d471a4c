"""Grouped launches of the bf16-NT, x3, h2 and b1 families through their ops wrappers on the device: a group of five problems is cut
into launches of four and one, and every problem must still get its own operands, bias, beta and output.  The kernels' numerics are
pinned elsewhere (test_gpu_gemm_branches.py, test_gpu_x3.py, test_gpu_h2.py); this is the end-to-end check of the marshalling.

Shapes: M = 40, N = 24, K = 80 -- no multiple of the images' 32-row / 16-column blocks in M or N, K even -- accepted by all four
families as they are.  Operands, biases and the prefilled output are integers in [-4, 4]: exact in bf16 and in IEEE half (so every
split plane but the first is zero), every partial sum an integer below 2^24, so any summation order gives the fp64 product exactly."""
import numpy as np
import pytest
import torch

import yt8m_amd.ops as ops

pytestmark = pytest.mark.gpu

M, N, K, GROUP = 40, 24, 80, 5
WIDE, COL0 = 56, 16                  # problem 4 accumulates into columns [16, 40) of a [40, 56] matrix


def _ints(rs, *shape):
    return rs.randint(-4, 5, size=shape).astype(np.float32)


@pytest.fixture(scope="module")
def case():
    """Host operands of the five problems and their fp64 results (computed once, read-only)."""
    rs = np.random.RandomState(35)
    A = [_ints(rs, M, K) for _ in range(GROUP)]
    B = [_ints(rs, N, K) for _ in range(GROUP)]
    bias = _ints(rs, N)
    wide = _ints(rs, M, WIDE)
    ref = [a.astype(np.float64) @ b.astype(np.float64).T for a, b in zip(A, B)]
    ref[2] = ref[2] + bias.astype(np.float64)
    ref[4] = ref[4] + wide[:, COL0:COL0 + N].astype(np.float64)
    for a in A + B + ref + [bias, wide]:
        a.setflags(write=False)
    return dict(A=A, B=B, bias=bias, wide=wide, ref=ref)


def _operand(family, x, dev):
    t = torch.tensor(x, device=dev)
    if family == "bf16_nt":
        out = ops._bf16_empty(x.shape[0], x.shape[1], dev)
        out.copy_(t)
        return out
    if family == "x3":
        return ops.x3_split(t)[0]
    if family == "h2":
        return ops.h2_split(t, scale=1.0)[0]
    return ops.bf16_image(t)


WRAPPER = {"bf16_nt": "gemm_bf16_nt_grouped", "x3": "gemm_x3_grouped", "h2": "gemm_h2_grouped", "b1": "gemm_b1_grouped"}


@pytest.mark.parametrize("family", ["bf16_nt", "x3", "h2", "b1"])
def test_group_of_five_equals_the_exact_product(dev, case, family):
    items = [dict(A=_operand(family, a, dev), B=_operand(family, b, dev)) for a, b in zip(case["A"], case["B"])]
    items[2]["bias"] = torch.tensor(case["bias"], device=dev)
    wide = torch.tensor(case["wide"], device=dev)
    items[4].update(out=wide[:, COL0:COL0 + N], beta=1.0)
    bf16_at = None
    if family == "b1":                                   # one bf16 output in the launch of four: a window of a [40, 28] bf16 matrix
        bf16_at = 1
        pitch = torch.full((M, 28), 7.0, dtype=torch.bfloat16, device=dev)
        items[1]["out"] = pitch[:, :N]
    outs = getattr(ops, WRAPPER[family])(items)
    torch.cuda.synchronize()
    assert len(outs) == GROUP and outs[4].data_ptr() == wide[:, COL0:COL0 + N].data_ptr()
    for i, (got, ref) in enumerate(zip(outs, case["ref"])):
        assert tuple(got.shape) == (M, N)
        if i == bf16_at:
            want = torch.tensor(ref).float().bfloat16()              # the exact result (an fp32 integer) rounded to nearest even once
            assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), want), "problem %d (bf16 output)" % i
            assert bool((pitch[:, N:] == 7.0).all())
        else:
            assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().astype(np.float64), ref), "problem %d" % i
    outside = np.ones(WIDE, dtype=bool)
    outside[COL0:COL0 + N] = False
    assert np.array_equal(wide.cpu().numpy()[:, outside], case["wide"][:, outside])
