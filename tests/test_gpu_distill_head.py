"""-m gpu: the head-input and blend kernels (csrc/distill_head.hip, ops.distill_input, ops.distill_blend) and Z's four cascade heads
(MoeDistillChainModel, -NormModel, -Norm2Model, MoeDistillSplitModel) against the fp64 restatement (tests/distill_head_restatement.py).

Bounds.  The measure is max |got - ref| / max(1, max |ref|) against the fp64 restatement on the same float32 inputs.  For the two ops'
own quantities (y, dx, dz; out, dp1; through the C ABI and through autograd) the bound is ensemble_restatement.bound in that measure:
FOUR times the error of the float32 restatement (plain torch on the CPU, in the reference's form) against the float64 one plus one
float32 ulp of the largest reference magnitude.  It is never derived from the kernels' output.  Every case prints the measured errors
with the float32 restatement's beside them and asserts that the float32 restatement is finite (t = rand in (0, 1) outside the zero_sum
kind).  WIDER names the quantities that get the gate tests' factor 8 and floors (2e-6 outputs, 5e-6 gradients) instead, with the
reason: the plugins' quantities, which sit behind the MoE products.

Measured on an MI355X (largest error per quantity, the float32 restatement's error of the same case in brackets):
  distill_input through the C ABI, the 80 cases: y 5.2e-8 [5.2e-8], dx 1.1e-7 [1.1e-7], dz 1.8e-7 [7.0e-8] on the 4 x bound; the nearest
    approach is that dz at 0.46 of its bound ((2, 1028, 256, 4717, 0), norm, clamped: the 1e6 of the clamped row sets the scale)
  distill_blend through the C ABI, the 30 cases: out 6.2e-8 [6.2e-8], dp1 2.8e-8 [2.8e-8]; out is the float32 restatement bit for bit
  through autograd: distill_input kernels y 3.0e-8 [2.3e-8], dx 3.2e-8 [4.9e-8], dz 4.4e-8 [2.7e-8] (0.31 of its bound); composed y 3.0e-8,
    dx 3.2e-8, dz 2.3e-8; distill_blend out 6.2e-8 [6.2e-8], dp1 2.8e-8 [2.8e-8] in both forms
  the 24 head cases, on the wider rule: predictions 1.0e-7 [8.7e-8] (MoeDistillChainModel, workload shape), loss 1.7e-7 [5.6e-8], gradients
    1.2e-7 [8.3e-8] (experts/weights; gates/weights at the workload shape 1.2e-7 [8.7e-8]): at most 0.09 of the floors
  LstmGateModel + head on bytes, the 6 cases: predictions 6.9e-8 [7.5e-8], loss 3.7e-8 [3.7e-8], gradients 5.1e-8 [4.6e-8] (gates/weights),
    the cell's own 2.3e-8 [1.9e-8] (lstm_forward/bc)
"""
import functools

import numpy as np
import pytest
import torch

import distill_head_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
import yt8m_amd.train  # noqa: F401  (defines the distillation flags the plugin tests set)
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
_PRODUCTS = ("a plugin quantity: behind the class_inputs product, the MoE head's products and (in frame-level use) the recurrence, which the "
             "device runs K-split and, where they are large, as three f16 products with 2^-21 per term under per-operand scales, with "
             "v_exp / v_rcp gate functions -- none of which the float32 restatement on the CPU draws (the reason of tests/test_gpu_gate_lstm.py "
             "and tests/test_gpu_scale_mix.py)")
WIDER = {"predictions": _PRODUCTS, "loss": _PRODUCTS, "gradient": _PRODUCTS}
GUARD = 16            # floats around every buffer
SENTINEL = -1234.5


def _bound(name, r32, r64):
    ref64 = torch.as_tensor(np.asarray(r64, dtype=np.float64))
    ref32 = torch.as_tensor(np.asarray(r32, dtype=np.float64))
    assert bool(torch.isfinite(ref32).all()), name
    big = max(1.0, float(ref64.abs().max()) if ref64.numel() else 0.0)
    if name in WIDER:
        return max(8.0 * R.err(r32, r64), GRAD_FLOOR if name == "gradient" else OUT_FLOOR)
    return R.bound(ref32, ref64) / big


def _report(tag, got, ref64, ref32, kind=None):
    """prints measured / float32-restatement errors and bounds per quantity, then asserts every one of them"""
    rows = [(k, R.err(got[k], ref64[k]), R.err(ref32[k], ref64[k]), _bound(kind or k, ref32[k], ref64[k])) for k in got]
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % r for r in rows))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, (tag, bad)


def _np(d):
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


class _Guarded(object):
    """A device buffer of n floats between GUARD sentinel floats, `off` floats past a 16-byte boundary; everything is sentinel until
    written, and what is not operand must stay so."""

    def __init__(self, dev, n, off=0, data=None):
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD + off:GUARD + off + n]
        assert self.view.data_ptr() % 16 == 4 * off
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).view(-1))
        self.n, self.off = n, off

    def intact(self):
        lo = GUARD + self.off
        return bool((self.buf[:lo] == SENTINEL).all()) and bool((self.buf[lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def written(self):
        return bool((self.view != SENTINEL).all())


# ---- distill_input through the C ABI ------------------------------------------------------------------------------------------------------
# one row; rows per workgroup (4) not dividing B and widths with no factor 4; the widest register-resident x (1024) with the workload's
# t and the Split head's window; the first x past the registers (1028) with a V with no factor 4; a 16-byte-misaligned t window (row
# pitch 37 floats, from column 10) under the video-level D
INPUT_SHAPES = [(1, 4, 37, 37, 0), (3, 37, 256, 260, 1), (5, 1024, 256, 4716, 1000), (2, 1028, 256, 4717, 0), (5, 1152, 64, 37, 10)]
INPUT_KINDS = ["plain", "misaligned", "clamped", "zero_sum"]
MODES = ["chain", "norm", "norm2", "split"]


def _input_case(B, D, C, V, v0, kind, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, D).astype(np.float32)
    z = rs.randn(B, C).astype(np.float32)
    t = rs.rand(B, V).astype(np.float32)
    t = np.maximum(t, np.float32(1e-3))                                   # in (0, 1)
    dy = rs.randn(B, D + C).astype(np.float32)
    if kind == "clamped":
        x[0] = 0.0                                                        # a row of x all zero
        z[1 % B] = -np.abs(z[1 % B]) - np.float32(1e-3)                   # a row of z all <= 0: relu leaves nothing
        x[2 % B] *= np.float32(1e-8)                                      # the sums of squares below eps = 1e-12
        z[2 % B] *= np.float32(1e-8)
    if kind == "zero_sum":
        t[B - 1] = 0.0
    return x, z, t, dy


@functools.lru_cache(maxsize=None)
def _input_refs(B, D, C, V, v0, kind, mode):
    x, z, t, dy = _input_case(B, D, C, V, v0, kind, 1000 * MODES.index(mode) + B + D + len(kind))
    r64 = R.distill_input_with_grads(x, z, t, mode, v0, dy, torch.float64)
    r32 = R.distill_input_with_grads(x, z, t, mode, v0, dy, torch.float32)
    return (x, z, t, dy), _np(r64), _np(r32)


@pytest.mark.parametrize("kind", INPUT_KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,C,V,v0", INPUT_SHAPES)
def test_distill_input_through_the_c_abi(dev, B, D, C, V, v0, mode, kind):
    lib = L.lib()
    assert lib.yt8m_distill_input_supported(D, C, V) == 1
    (x, z, t, dy), r64, r32 = _input_refs(B, D, C, V, v0, kind, mode)
    bits = ops._distill_mode_bits(mode)
    norm_x, relu, div, norm_c = R.MODES[mode]
    off = 1 if kind == "misaligned" else 0                    # every pointer 4 bytes past a 16-byte boundary
    new = lambda n, data=None: _Guarded(dev, n, off, data)
    xb, zb, tb, gb = new(B * D, x), new(B * C, z), new(B * V, t), new(B * (D + C), dy)

    def run(want_dx=True):
        y, rx, rc, sinv = new(B * (D + C)), new(B), new(B), new(B)
        dx, dz = (new(B * D) if want_dx else None), new(B * C)
        L.check(lib.yt8m_distill_input_fwd(bits, _p(xb.view), _p(zb.view), _p(tb.view), V, v0, V, _p(y.view), _p(rx.view), _p(rc.view),
                                           _p(sinv.view), B, D, C, 1e-12, _stream()))
        L.check(lib.yt8m_distill_input_bwd(bits, _p(zb.view), _p(y.view), _p(rx.view), _p(rc.view), _p(sinv.view), _p(gb.view),
                                           _p(dx.view) if want_dx else None, _p(dz.view), B, D, C, _stream()))
        torch.cuda.synchronize()
        return y, rx, rc, sinv, dx, dz

    outs = run()
    y, rx, rc, sinv, dx, dz = outs
    for b in [xb, zb, tb, gb] + list(outs):
        assert b.intact()
    for b in outs:
        assert b.written()                                    # every element of every output was overwritten
    for b, src in ((xb, x), (zb, z), (tb, t), (gb, dy)):
        assert torch.equal(b.view.cpu(), torch.from_numpy(src).view(-1))          # the operands are only read
    got = {"y": y.view.cpu().view(B, D + C), "dx": dx.view.cpu().view(B, D), "dz": dz.view.cpu().view(B, C)}
    _report("distill_input c abi (%d,%d,%d,%d,%d) %s %s:" % (B, D, C, V, v0, mode, kind), got, r64, r32)
    # the saved scalars: 1 where a part is not normalised / nothing is divided, the sign at the clamp, 0 for a zero sum
    rxc, rcc, sc = rx.view.cpu(), rc.view.cpu(), sinv.view.cpu()
    if not norm_x:
        assert bool((rxc == 1).all())
    if not norm_c:
        assert bool((rcc == 1).all())
    if not div:
        assert bool((sc == 1).all())
    else:
        s64 = t[:, v0:].astype(np.float64).sum(axis=1)
        live = s64 != 0
        assert np.allclose(sc.numpy()[live], 1.0 / s64[live], rtol=1e-5) and bool((sc.numpy()[~live] == 0).all())
    if kind == "clamped":
        if norm_x:
            assert float(rxc[0]) == -1e6 and float(rxc[2 % B]) == -1e6 and (B < 4 or float(rxc[3]) > 0)
        if norm_c and relu:
            assert float(rcc[1 % B]) == -1e6
        if relu:                                              # nothing of the row passes the relu: zeros out, zeros back
            assert float(got["y"][1 % B, D:].abs().max()) == 0.0 and float(got["dz"][1 % B].abs().max()) == 0.0
    if kind == "zero_sum" and div:
        assert float(got["y"][B - 1, D:].abs().max()) == 0.0 and float(got["dz"][B - 1].abs().max()) == 0.0
        assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["dz"]).all())
    # a second run gives the same bits
    outs2 = run()
    assert all(torch.equal(a.buf, b.buf) for a, b in zip(outs2, outs))
    # an unrequested dx is untouched, dz unchanged
    spare = new(B * D)
    outs3 = run(want_dx=False)
    assert spare.untouched() and outs3[4] is None and torch.equal(outs3[5].buf, dz.buf) and torch.equal(outs3[0].buf, y.buf)


def test_refused_distill_input_arguments_launch_nothing(dev):
    lib = L.lib()
    b = [_Guarded(dev, 64, 0, np.zeros(64)) for _ in range(3)]
    y, s = _Guarded(dev, 64), _Guarded(dev, 8)
    call = lambda mode=15, v0=0, rows=2, D=8: lib.yt8m_distill_input_fwd(mode, _p(b[0].view), _p(b[1].view), _p(b[2].view), 8, v0, 8,
                                                                         _p(y.view), _p(s.view), _p(s.view), _p(s.view), rows, D, 8, 1e-12, _stream())
    assert call(mode=16) == -1 and call(v0=8) == -1 and call(rows=0) == -2 and call(D=0) == -2
    torch.cuda.synchronize()
    assert y.untouched() and s.untouched()


# ---- distill_blend through the C ABI ------------------------------------------------------------------------------------------------------
BLEND_SHAPES = [(1, 37, 37), (3, 37, 10), (5, 4716, 1000), (2, 4717, 1001), (128, 4716, 4716)]


@functools.lru_cache(maxsize=None)
def _blend_refs(B, V, V1, w):
    rs = np.random.RandomState(B + V + V1)
    p1, t, dout = rs.rand(B, V1).astype(np.float32), rs.rand(B, V).astype(np.float32), rs.randn(B, V).astype(np.float32)
    return (p1, t, dout), _np(R.distill_blend_with_grads(p1, t, w, dout, torch.float64)), _np(R.distill_blend_with_grads(p1, t, w, dout, torch.float32))


@pytest.mark.parametrize("kind", ["plain", "misaligned"])
@pytest.mark.parametrize("w", [1.0, 0.2, 0.0])
@pytest.mark.parametrize("B,V,V1", BLEND_SHAPES)
def test_distill_blend_through_the_c_abi(dev, B, V, V1, w, kind):
    lib = L.lib()
    assert lib.yt8m_distill_blend_supported(B, V, V1) == 1
    (p1, t, dout), r64, r32 = _blend_refs(B, V, V1, w)
    off = 1 if kind == "misaligned" else 0
    new = lambda n, data=None: _Guarded(dev, n, off, data)
    pb, tb, gb = new(B * V1, p1), new(B * V, t), new(B * V, dout)

    def run():
        out, dp1 = new(B * V), new(B * V1)
        L.check(lib.yt8m_distill_blend_fwd(_p(pb.view), _p(tb.view), V, _p(out.view), B, V, V1, w, _stream()))
        L.check(lib.yt8m_distill_blend_bwd(_p(gb.view), _p(dp1.view), B, V, V1, w, _stream()))
        torch.cuda.synchronize()
        return out, dp1

    out, dp1 = run()
    for b in (pb, tb, gb, out, dp1):
        assert b.intact()
    assert out.written() and dp1.written()
    for b, src in ((pb, p1), (tb, t), (gb, dout)):
        assert torch.equal(b.view.cpu(), torch.from_numpy(src).view(-1))
    got = {"out": out.view.cpu().view(B, V), "dp1": dp1.view.cpu().view(B, V1)}
    _report("distill_blend c abi (%d,%d,%d) w=%g %s:" % (B, V, V1, w, kind), got, r64, r32)
    if w == 1.0:                                              # p * 1.0 + t * 0.0 is p bit for bit, and the teacher's own labels stay
        assert torch.equal(got["out"][:, :V1], torch.from_numpy(p1)) and torch.equal(got["out"][:, V1:], torch.from_numpy(t[:, V1:]))
    if w == 0.0:
        assert torch.equal(got["out"], torch.from_numpy(t)) and float(got["dp1"].abs().max()) == 0.0
    assert torch.equal(got["out"], torch.from_numpy(r32["out"]))          # the reference's own roundings: two products, then the sum
    out2, dp2 = run()
    assert torch.equal(out2.buf, out.buf) and torch.equal(dp2.buf, dp1.buf)


# ---- both ops through autograd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,D,C,V,v0", [("norm2", 5, 1024, 256, 4716, 1000), ("norm", 3, 37, 256, 260, 1), ("chain", 2, 1028, 256, 4717, 0),
                                             ("split", 5, 1152, 64, 37, 10)])
def test_distill_input_autograd_fused_and_composed_against_the_restatement(dev, monkeypatch, mode, B, D, C, V, v0):
    (x, z, t, dy), r64, r32 = _input_refs(B, D, C, V, v0, "plain", mode)
    d = lambda a: torch.from_numpy(a).to(dev)
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", fused)
        key = "input_kernels" if fused else "input_composed"
        for rep in range(2):
            xt, zt = d(x).requires_grad_(True), d(z).requires_grad_(True)
            tw = d(t)
            before = dict(ops.DISTILL_CALLS)
            y = ops.distill_input(xt, zt, tw, mode, v0)
            assert ops.DISTILL_CALLS[key] == before[key] + 1 and sum(ops.DISTILL_CALLS.values()) == sum(before.values()) + 1
            y.backward(d(dy))
            got = {"y": y.detach().cpu(), "dx": xt.grad.cpu(), "dz": zt.grad.cpu()}
            if rep:
                assert all(torch.equal(got[k], runs[fused][k]) for k in got)             # two runs: the same bits
            runs[fused] = got
        _report("distill_input autograd (%d,%d,%d,%d,%d) %s %s:" % (B, D, C, V, v0, mode, key), runs[fused], r64, r32)
    # x as data (video-level use): no dx is asked for, dz is the same
    monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", True)
    zt = d(z).requires_grad_(True)
    ops.distill_input(d(x), zt, d(t), mode, v0).backward(d(dy))
    assert torch.equal(zt.grad.cpu(), runs[True]["dz"])
    # t as a column window of a wider tensor (its own row pitch): the same bits
    wide = torch.cat([d(t), d(t)], dim=1)
    zt2 = d(z).requires_grad_(True)
    y2 = ops.distill_input(d(x), zt2, wide[:, :V], mode, v0)
    assert torch.equal(y2.detach().cpu(), runs[True]["y"])


@pytest.mark.parametrize("B,V,V1,w", [(5, 4716, 1000, 0.2), (128, 4716, 4716, 0.2), (3, 37, 10, 1.0)])
def test_distill_blend_autograd_fused_and_composed_against_the_restatement(dev, monkeypatch, B, V, V1, w):
    (p1, t, dout), r64, r32 = _blend_refs(B, V, V1, w)
    d = lambda a: torch.from_numpy(a).to(dev)
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "DISTILL_BLEND_FUSED", fused)
        key = "blend_kernels" if fused else "blend_composed"
        for rep in range(2):
            pt = d(p1).requires_grad_(True)
            before = dict(ops.DISTILL_CALLS)
            out = ops.distill_blend(pt, d(t), w, V1)
            assert ops.DISTILL_CALLS[key] == before[key] + 1 and sum(ops.DISTILL_CALLS.values()) == sum(before.values()) + 1
            out.backward(d(dout))
            got = {"out": out.detach().cpu(), "dp1": pt.grad.cpu()}
            if rep:
                assert all(torch.equal(got[k], runs[fused][k]) for k in got)
            runs[fused] = got
        _report("distill_blend autograd (%d,%d,%d) w=%g %s:" % (B, V, V1, w, key), runs[fused], r64, r32)
    pt = d(p1[:, :V1])
    full = d(np.ascontiguousarray(np.concatenate([p1, t[:, V1:]], axis=1)))
    assert ops.distill_blend(full, d(t), 1.0, V) is full                  # the Chain heads' training setting: p1 itself
    del pt


def test_cpu_and_float64_tensors_take_the_composed_forms_when_the_kernels_are_asked_for(dev, monkeypatch):
    monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", True)
    monkeypatch.setattr(ops, "DISTILL_BLEND_FUSED", True)
    before = dict(ops.DISTILL_CALLS)
    ops.distill_blend(torch.rand(3, 5, device=dev).double(), torch.rand(3, 8, device=dev).double(), 0.5, 5)
    ops.distill_blend(torch.rand(3, 5), torch.rand(3, 8), 0.5, 5)
    assert ops.DISTILL_CALLS["blend_composed"] == before["blend_composed"] + 2 and ops.DISTILL_CALLS["blend_kernels"] == before["blend_kernels"]
    # distill_input's composed form is made of ops.activation and ops.l2_normalize, which are device float32 code: a CPU tensor reaches
    # them, not the fused kernel, and is refused there as by every other op
    with pytest.raises(L.Yt8mHipError):
        ops.distill_input(torch.rand(3, 5), torch.rand(3, 4), torch.rand(3, 8), "split", 2)
    assert ops.DISTILL_CALLS["input_kernels"] == before["input_kernels"] and ops.DISTILL_CALLS["input_composed"] == before["input_composed"] + 1


# ---- the heads as plugins -----------------------------------------------------------------------------------------------------------------
def _train_graph(model, dev, B, identical=True):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=dev, seed=0)
    kw = {"transformer_class": ft.IdenticalTransformer} if identical else {}
    return g, train.TrainGraph(model, label_loss_fn=losses.CrossEntropyLoss(), batch_size=B, graph=g, **kw)


def _load(g, P, dev):
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    torch.cuda.synchronize()


def _grads(g):
    return {k: (v.grad if v.grad_written else torch.zeros_like(v.grad)).detach().cpu() for k, v in g.vars.items() if v.trainable}


HEAD_SHAPES = {"host": (5, 36, 37, 3, 10), "workload": (16, 1152, 4716, 2, 1000)}       # B, D, V, M, --softmax_bound


@functools.lru_cache(maxsize=None)
def _head_refs(name, shape, w):
    B, D, V, M, sb = HEAD_SHAPES[shape]
    rs = np.random.RandomState(50 + R.HEADS.index(name) + B)
    x = rs.randn(B, D).astype(np.float32)
    t = np.maximum(rs.rand(B, V).astype(np.float32), np.float32(1e-3))
    y = rs.rand(B, V) < (0.2 if V < 100 else 3.4 / V)
    P = R.draw(R.variable_shapes(name, D, V, M, sb), rs)
    r64 = R.reference(name, x, t, y, P, M, torch.float64, w, sb)
    r32 = R.reference(name, x, t, y, P, M, torch.float32, w, sb)
    return (x, t, y, P), r64, r32


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("shape,w", [("host", 1.0), ("host", 0.2), ("workload", 0.2)])
@pytest.mark.parametrize("name", R.HEADS)
def test_head_matches_the_fp64_restatement_on_the_device(dev, flags, monkeypatch, name, shape, w, fused):
    """--model=<head> through TrainGraph.forward / loss / backward: predictions, CrossEntropyLoss and every Variable's gradient; the
    features are data, as in video-level use (no head gradient is computed for them)."""
    import yt8m_amd.video_level_models as vlm
    monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", fused)
    monkeypatch.setattr(ops, "DISTILL_BLEND_FUSED", fused)
    B, D, V, M, sb = HEAD_SHAPES[shape]
    flags.moe_num_mixtures, flags.softmax_bound, flags.ensemble_w = M, sb, w
    flags.distillation_features, flags.distillation_as_input = True, True
    (x, t, y, P), r64, r32 = _head_refs(name, shape, w)
    g, tg = _train_graph(getattr(vlm, name)(), dev, B)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    dt = torch.from_numpy(t).to(dev)
    tg.forward(*args, distillation_predictions=dt)
    assert list(g.vars) == list(P)
    _load(g, P, dev)
    before = dict(ops.DISTILL_CALLS)
    res = tg.forward(*args, distillation_predictions=dt)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    blends = 0 if (w == 1.0 and name != "MoeDistillSplitModel") else 1
    form = "kernels" if fused else "composed"
    assert ops.DISTILL_CALLS["input_" + form] == before["input_" + form] + 1 and ops.DISTILL_CALLS["blend_" + form] == before["blend_" + form] + blends
    assert sum(ops.DISTILL_CALLS.values()) == sum(before.values()) + 1 + blends
    tag = "%s %s w=%g %s:" % (name, shape, w, "fused" if fused else "composed")
    got = {"predictions": res["predictions"].detach().cpu(), "loss": loss.detach().cpu()}
    _report(tag, got, {k: r64[k].numpy() for k in got}, {k: r32[k].numpy() for k in got})
    grads = _grads(g)
    assert set(grads) == set(r64["grads"])
    _report(tag + " gradients", grads, _np(r64["grads"]), _np(r32["grads"]), kind="gradient")
    for k in grads:
        assert float(grads[k].abs().max()) > 0, k


GATE = dict(B=16, F=6, D=1152, H=256, V=32, M=2, sb=10)                 # the smallest plugin shape of tests/test_gpu_gate_lstm.py, on bytes


@functools.lru_cache(maxsize=None)
def _gate_refs(name, w):
    from oracle import np_ref
    c = GATE
    rs = np.random.RandomState(70 + R.HEADS.index(name))
    q = rs.randint(0, 256, size=(c["B"], c["F"], c["D"])).astype(np.uint8)
    nf = np.resize(np.array([c["F"], 1, 3, 0, 5, 2], dtype=np.int32), c["B"])
    y = rs.rand(c["B"], c["V"]) < 0.2
    t = np.maximum(rs.rand(c["B"], c["V"]).astype(np.float32), np.float32(1e-3))
    from gate_lstm_restatement import random_unit
    P = {"lstm_forward/" + n: a for n, a in random_unit(rs, c["D"], c["H"]).items()}
    P.update(R.draw(R.variable_shapes(name, c["H"], c["V"], c["M"], c["sb"]), rs))
    x64 = np_ref.dequant_l2norm_folded(q, nf)
    r64 = R.gate_reference(name, x64, nf, t, y, P, c["M"], torch.float64, w, c["sb"])
    r32 = R.gate_reference(name, x64.astype(np.float32), nf, t, y, P, c["M"], torch.float32, w, c["sb"])
    return (q, nf, y, t, P), r64, r32


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name,w", [("MoeDistillChainModel", 1.0), ("MoeDistillChainModel", 0.2), ("MoeDistillSplitModel", 1.0)])
def test_lstm_gate_model_with_a_cascade_head_matches_fp64_on_bytes(dev, flags, monkeypatch, name, w, fused):
    """--model=LstmGateModel --video_level_classifier_model=<head>, 256 cells, B = 16, F = 6, D = 1152 on the reader's bytes, V = 32, 2
    mixtures: the head's input is the cell's memory and hands its gradient to the recurrence (dx of the head-input kernel)."""
    import yt8m_amd.frame_level_models as flm
    monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", fused)
    monkeypatch.setattr(ops, "DISTILL_BLEND_FUSED", fused)
    c = GATE
    flags.lstm_cells, flags.moe_num_mixtures, flags.softmax_bound, flags.ensemble_w = str(c["H"]), c["M"], c["sb"], w
    flags.video_level_classifier_model = name
    (q, nf, y, t, P), r64, r32 = _gate_refs(name, w)
    g, tg = _train_graph(flm.LstmGateModel(), dev, c["B"], identical=False)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    dt = torch.from_numpy(t).to(dev)
    tg.forward(*args, distillation_predictions=dt)
    assert list(g.vars) == list(P)
    _load(g, P, dev)
    before = dict(ops.DISTILL_CALLS)
    res = tg.forward(*args, distillation_predictions=dt)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    form = "kernels" if fused else "composed"
    assert ops.DISTILL_CALLS["input_" + form] == before["input_" + form] + 1
    tag = "LstmGateModel + %s w=%g %s:" % (name, w, "fused" if fused else "composed")
    got = {"predictions": res["predictions"].detach().cpu(), "loss": loss.detach().cpu()}
    _report(tag, got, {k: r64[k].numpy() for k in got}, {k: r32[k].numpy() for k in got})
    grads = {k: v.view(r64["grads"][k].shape) for k, v in _grads(g).items()}
    assert set(grads) == set(r64["grads"])
    _report(tag + " gradients", grads, _np(r64["grads"]), _np(r32["grads"]), kind="gradient")
    assert float(grads["lstm_forward/Wc"].abs().max()) > 0


def test_one_training_step_moves_every_variable(dev, flags, monkeypatch):
    """TrainGraph.step with --distillation_features --distillation_as_input on the device's own clip + Adam pass."""
    import yt8m_amd.video_level_models as vlm
    monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", True)
    monkeypatch.setattr(ops, "DISTILL_BLEND_FUSED", True)
    B, D, V, M, sb = HEAD_SHAPES["host"]
    flags.moe_num_mixtures, flags.softmax_bound, flags.ensemble_w = M, sb, 0.2
    flags.distillation_features, flags.distillation_as_input = True, True
    (x, t, y, P), _, _ = _head_refs("MoeDistillChainNorm2Model", "host", 0.2)
    g, tg = _train_graph(vlm.MoeDistillChainNorm2Model(), dev, B)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    dt = torch.from_numpy(t).to(dev)
    out = tg.step(*args, distill_labels_batch=dt)
    start = {k: v.data.clone() for k, v in g.vars.items()}
    out2 = tg.step(*args, distill_labels_batch=dt)
    torch.cuda.synchronize()
    for k, v in g.vars.items():
        assert bool(torch.isfinite(v.data).all()) and not torch.equal(v.data, start[k]), k
    assert np.isfinite(float(out["loss"])) and float(out2["loss"]) < float(out["loss"])
