"""-m gpu: the scale mix (csrc/scale_mix.hip, ops.scale_mix), the Z training rule with the device's label losses and the three
LstmMultiscale plugins against the fp64 restatement (tests/scale_mix_restatement.py).

Bounds.  The measure is max |got - ref| / max(1, max |ref|) against the fp64 restatement on the same float32 inputs.  For the op's
quantities (out, dp, dz; through the C ABI and through autograd) the bound is ensemble_restatement.bound in that measure: FOUR times the
error of the float32 restatement (plain torch on the CPU, in the reference's form: tf.stack, softmax(dim=1), reduce_sum) against the
float64 one plus one float32 ulp of the largest reference magnitude.  It is never derived from the kernels' output.  Every case prints
the measured errors with the float32 restatement's beside them and asserts that the float32 restatement is finite.  WIDER names the
quantities that get the gate tests' factor 8 and floors (2e-6 outputs, 5e-6 gradients) instead, with the reason: the plugins' quantities,
whose products the device cuts and rounds differently from torch on the CPU.

Measured on an MI355X (largest error per quantity, the float32 restatement's error of the same case in brackets):
  C ABI, the 25 cases: out 2.6e-7 [3.2e-7], dp 1.6e-7 [1.6e-7], dz 5.5e-7 [4.5e-7] on the 4 x bound; the nearest approach is dz at 0.38 of it
    ((8, 3, 260), plain).  dz, the candidate for the wider rule ((p - out) cancels), did not need it: the difference is taken per element from
    the saved out, and its rounding enters dz relative to |p - out|, as the restatement's own does.
  through autograd at (3, 17, 4717) and (4, 128, 4716): kernels out 2.3e-7 [2.4e-7], dp 1.4e-7 [1.4e-7], dz 4.7e-7 [3.8e-7]; composed out 2.4e-7,
    dp 1.4e-7, dz 4.9e-7 [4.1e-7]
  the thirteen plugin cases, on the wider rule: predictions 1.5e-6 [1.2e-6] (B = 16, bytes), prediction_frames 4.2e-7 [4.3e-7], loss 1.1e-7
    [8.9e-8], gradients 5.7e-6 [3.9e-6] (cnn1cnn-filter-len1, LstmMultiscale2Model, generic, floats; bound 3.1e-5); the nearest approach is
    cnn3cnn-filter-len1 of the same model on bytes, 1.9e-6 [6.7e-7] at 0.35 of its bound; ensemble_weight2d exact zeros in every case
  the gradient of predictions (mix kernels' backward, grouped dW and dx): 1.2e-5 [2.2e-5] (cnn3cnn-filter-len1), ensemble_weight2d 1.5e-6 [1.4e-6]
"""
import ctypes

import numpy as np
import pytest
import torch

import scale_mix_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
_PRODUCTS = ("a plugin quantity: behind the CNN, the recurrences, the MoE heads and the logit products, which the device runs K-split and, "
             "where they are large, as three f16 products with 2^-21 per term under per-operand scales, with v_exp / v_rcp gate functions "
             "compounding over the frames -- none of which the float32 restatement on the CPU draws (the reason of tests/test_gpu_gate_lstm.py)")
WIDER = {"predictions": _PRODUCTS, "prediction_frames": _PRODUCTS, "loss": _PRODUCTS, "gradient": _PRODUCTS}
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
    rows = [(k, R.err(got[k], ref64[k]), R.err(ref32[k], ref64[k]), _bound(kind or k.rstrip("0123456789"), ref32[k], ref64[k])) for k in got]
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % r for r in rows))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, (tag, bad)


# ---- the op through the C ABI -----------------------------------------------------------------------------------------------------------
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


def _table(bufs):
    return (ctypes.c_void_p * len(bufs))(*[None if b is None else b.view.data_ptr() for b in bufs])


# odd B, a V with no factor of 4 and the scalar tail, every L parity, the largest L, the workload's own plane once
SHAPES = [(1, 3, 37), (2, 5, 4716), (3, 17, 4717), (4, 128, 4716), (8, 3, 260)]
KINDS = ["plain", "misaligned", "saturated", "equal", "p01"]


def _abi_inputs(Lx, B, V, kind, seed):
    rs = np.random.RandomState(seed)
    ps = rs.rand(Lx, B, V).astype(np.float32)
    zs = (rs.randn(Lx, B, V) * 2).astype(np.float32)
    if kind == "saturated":                                   # logits scaled to +-80: the weights are 0 or 1 to rounding
        zs = (zs * (80.0 / np.abs(zs).max())).astype(np.float32)
    elif kind == "equal":                                     # all z_l equal: every weight 1 / L
        zs[:] = zs[0]
    elif kind == "p01":                                       # p at exactly 0 and 1
        ps = (rs.rand(Lx, B, V) < 0.5).astype(np.float32)
    g = rs.randn(B, V).astype(np.float32)
    return ps, zs, g


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Lx,B,V", SHAPES)
def test_scale_mix_through_the_c_abi(dev, Lx, B, V, kind):
    lib = L.lib()
    assert lib.yt8m_scale_mix_supported(Lx, B, V) == 1
    ps, zs, g = _abi_inputs(Lx, B, V, kind, 100 * Lx + len(kind))
    r64 = R.scale_mix_with_grads(ps, zs, g, torch.float64)
    r32 = R.scale_mix_with_grads(ps, zs, g, torch.float32)
    off = 1 if kind == "misaligned" else 0                    # every pointer 4 bytes past a 16-byte boundary
    n = B * V
    new = lambda data=None: _Guarded(dev, n, off, data)
    pb, zb, gb = [new(p) for p in ps], [new(z) for z in zs], new(g)

    def run(skip_dp=(), skip_dz=()):
        out = new()
        dp = [None if l in skip_dp else new() for l in range(Lx)]
        dz = [None if l in skip_dz else new() for l in range(Lx)]
        L.check(lib.yt8m_scale_mix_fwd(Lx, _table(pb), _table(zb), _p(out.view), B, V, _stream()))
        L.check(lib.yt8m_scale_mix_bwd(Lx, _table(pb), _table(zb), _p(out.view), _p(gb.view), _table(dp), _table(dz), B, V, _stream()))
        torch.cuda.synchronize()
        return out, dp, dz

    out, dp, dz = run()
    for b in [out, gb] + pb + zb + dp + dz:
        assert b.intact()
    for b in [out] + dp + dz:
        assert b.written()                                    # every element of every output was overwritten
    for b, src in zip(pb + zb + [gb], list(ps) + list(zs) + [g]):
        assert torch.equal(b.view.cpu(), torch.from_numpy(src).view(-1))          # the operands are only read
    shp = lambda b: b.view.cpu().view(B, V)
    got = {"out": shp(out)}
    got.update({"dp%d" % l: shp(dp[l]) for l in range(Lx)})
    got.update({"dz%d" % l: shp(dz[l]) for l in range(Lx)})
    ref = lambda r: dict([("out", r[0].numpy())] + [("dp%d" % l, r[1][l].numpy()) for l in range(Lx)] + [("dz%d" % l, r[2][l].numpy()) for l in range(Lx)])
    _report("c abi (%d,%d,%d) %s:" % (Lx, B, V, kind), got, ref(r64), ref(r32))
    if Lx == 1:                                               # one scale: out is the plane itself, its logit gets exact zeros
        assert torch.equal(got["out"], torch.from_numpy(ps[0])) and torch.equal(got["dz0"], torch.zeros(B, V))
    if kind == "equal":
        assert R.err(got["dp0"], g / Lx) < 1e-7
    # a second run gives the same bits
    out2, dp2, dz2 = run()
    assert torch.equal(out2.buf, out.buf) and all(torch.equal(a.buf, b.buf) for a, b in zip(dp2 + dz2, dp + dz))
    # NULL dp[l] / dz[l] are skipped, the others unchanged
    skip_dp, skip_dz = (0,), tuple(range(Lx))[-1:]
    out3, dp3, dz3 = run(skip_dp, skip_dz)
    for l in range(Lx):
        assert dp3[l] is None if l in skip_dp else torch.equal(dp3[l].buf, dp[l].buf)
        assert dz3[l] is None if l in skip_dz else torch.equal(dz3[l].buf, dz[l].buf)
    # nothing wanted: nothing written, nothing launched
    spare = new()
    none = (ctypes.c_void_p * Lx)(*[None] * Lx)
    L.check(lib.yt8m_scale_mix_bwd(Lx, _table(pb), _table(zb), _p(out.view), _p(gb.view), none, none, B, V, _stream()))
    torch.cuda.synchronize()
    assert spare.untouched() and torch.equal(out.buf, out2.buf)


def test_refused_shapes_launch_nothing(dev):
    lib = L.lib()
    t = [_Guarded(dev, 12, 0, np.zeros(12)) for _ in range(9)]
    out = _Guarded(dev, 12)
    tab = (ctypes.c_void_p * 9)(*[b.view.data_ptr() for b in t])
    assert lib.yt8m_scale_mix_fwd(9, tab, tab, _p(out.view), 3, 4, _stream()) == -2
    assert lib.yt8m_scale_mix_fwd(0, tab, tab, _p(out.view), 3, 4, _stream()) == -2
    assert lib.yt8m_scale_mix_fwd(2, tab, tab, _p(out.view), 0, 4, _stream()) == -2
    torch.cuda.synchronize()
    assert out.untouched()


# ---- the op through autograd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lx,B,V,stacked", [(3, 17, 4717, False), (4, 128, 4716, True)])
def test_scale_mix_autograd_fused_against_composed_and_restatement(dev, monkeypatch, Lx, B, V, stacked):
    ps, zs, g = _abi_inputs(Lx, B, V, "plain", 7 + Lx)
    r64 = R.scale_mix_with_grads(ps, zs, g, torch.float64)
    r32 = R.scale_mix_with_grads(ps, zs, g, torch.float32)
    ref = lambda r: dict([("out", r[0].numpy())] + [("dp%d" % l, r[1][l].numpy()) for l in range(Lx)] + [("dz%d" % l, r[2][l].numpy()) for l in range(Lx)])
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "SCALE_MIX_FUSED", fused)
        pt = [torch.from_numpy(p).to(dev).requires_grad_(True) for p in ps]
        if stacked:                                           # z as one [L,B,V] tensor: the wrapper takes it apart into L pointers
            zt = torch.from_numpy(zs).to(dev).requires_grad_(True)
        else:
            zt = [torch.from_numpy(z).to(dev).requires_grad_(True) for z in zs]
        before = dict(ops.SCALE_MIX_CALLS)
        out = ops.scale_mix(pt, zt)
        key = "kernels" if fused else "composed"
        assert ops.SCALE_MIX_CALLS[key] == before[key] + 1 and sum(ops.SCALE_MIX_CALLS.values()) == sum(before.values()) + 1
        out.backward(torch.from_numpy(g).to(dev))
        got = {"out": out.detach().cpu()}
        got.update({"dp%d" % l: pt[l].grad.cpu() for l in range(Lx)})
        got.update({"dz%d" % l: (zt.grad[l] if stacked else zt[l].grad).cpu() for l in range(Lx)})
        _report("autograd (%d,%d,%d) %s:" % (Lx, B, V, key), got, ref(r64), ref(r32))
        runs[fused] = got
    # the two forms against each other: each within its bound of the restatement, so within the sum of the two
    for k in runs[True]:
        assert R.err(runs[True][k], runs[False][k].double().numpy()) <= 2 * _bound(k.rstrip("0123456789"), ref(r32)[k], ref(r64)[k]), k
    # only the logits want a gradient (the sub-predictions are data): the dp pointers are NULL
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", True)
    pt = [torch.from_numpy(p).to(dev) for p in ps]
    zt = [torch.from_numpy(z).to(dev).requires_grad_(True) for z in zs]
    ops.scale_mix(pt, zt).backward(torch.from_numpy(g).to(dev))
    assert all(torch.equal(zt[l].grad.cpu(), runs[True]["dz%d" % l]) for l in range(Lx))


def test_cpu_and_float64_tensors_take_the_composed_form_when_the_kernels_are_asked_for(dev, monkeypatch):
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", True)
    ps, zs, _ = _abi_inputs(9, 3, 8, "plain", 1)
    before = dict(ops.SCALE_MIX_CALLS)
    ops.scale_mix([torch.from_numpy(p).to(dev) for p in ps], torch.from_numpy(zs).to(dev))              # L > 8
    ops.scale_mix([torch.from_numpy(p).to(dev).double() for p in ps[:4]], torch.from_numpy(zs[:4]).to(dev).double())
    assert ops.SCALE_MIX_CALLS["composed"] == before["composed"] + 2 and ops.SCALE_MIX_CALLS["kernels"] == before["kernels"]


# ---- the training rule with the device's label losses -------------------------------------------------------------------------------------
LOSSES = ["CrossEntropyLoss", "WeightedCrossEntropyLoss", "MeanSquareErrorLoss", "HingeLoss", "BatchAgreementCrossEntropyLoss",
          "TopKBatchAgreementCrossEntropyLoss"]


def _train_graph(model, loss_fn, dev, B, identical=True, **kw):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=dev, seed=0)
    if identical:
        kw["transformer_class"] = ft.IdenticalTransformer
    return g, train.TrainGraph(model, label_loss_fn=loss_fn, batch_size=B, graph=g, **kw)


@pytest.mark.parametrize("name", LOSSES)
def test_frames_loss_equals_the_literal_tiled_form_for_every_label_loss(dev, flags, name):
    import yt8m_amd.losses as losses
    import yt8m_amd.train  # noqa: F401  (defines --batch_size)
    B, Lx, V = 6, 4, 37
    flags.batch_size, flags.false_negative_punishment = B, 2.0
    rs = np.random.RandomState(21)
    frames = torch.from_numpy(rs.rand(B * Lx, V).astype(np.float32) * 0.9 + 0.05).to(dev).requires_grad_(True)
    preds = torch.from_numpy(rs.rand(B, V).astype(np.float32)).to(dev).requires_grad_(True)
    labels = torch.from_numpy(rs.rand(B, V) < 0.3).to(dev)
    fn = getattr(losses, name)()
    _, tg = _train_graph(object(), fn, dev, B)
    loss = tg.loss({"predictions": preds, "prediction_frames": frames}, labels)
    loss.backward()
    f2 = frames.detach().clone().requires_grad_(True)
    want = fn.calculate_loss(f2, R.tile_labels(labels, Lx))
    want.backward()
    assert torch.equal(loss.detach(), want.detach()) and torch.equal(frames.grad, f2.grad)
    assert preds.grad is None and float(frames.grad.abs().max()) > 0
    if name == "CrossEntropyLoss":                            # ... and the value is the restatement's, the mean over the scales of the per-scale losses
        ref = R.cross_entropy(frames.detach().cpu().double(), R.tile_labels(labels.cpu(), Lx))
        per = sum(R.cross_entropy(frames.detach().cpu().double().view(B, Lx, V)[:, l], labels.cpu()) for l in range(Lx)) / Lx
        assert abs(float(loss.detach()) - float(ref)) <= OUT_FLOOR * max(1.0, float(ref)) and abs(float(per) - float(ref)) < 1e-12 * float(ref)
        w = torch.from_numpy(rs.rand(B).astype(np.float32) + 0.5).to(dev)
        lw = tg.loss({"predictions": preds, "prediction_frames": frames}, labels, weights=w)
        assert torch.equal(lw.detach(), fn.calculate_loss(frames.detach(), R.tile_labels(labels, Lx), weights=w.repeat_interleave(Lx)))


def test_moe_model_step_loss_is_bit_equal_with_and_without_the_key(dev, flags):
    """A result without the key goes through the code as before; with one row per video under the key the branch computes the same
    loss from the same tensors, and the step moves the parameters alike."""
    import yt8m_amd.losses as losses
    import yt8m_amd.video_level_models as vlm
    flags.moe_num_mixtures, flags.fused_head_loss = 2, False

    class WithFrames(vlm.MoeModel):
        def create_model(self, *a, **k):
            res = super().create_model(*a, **k)
            res["prediction_frames"] = res["predictions"]
            return res

    B, D, V = 16, 64, 37
    rs = np.random.RandomState(22)
    x = torch.from_numpy(rs.randn(B, D).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.rand(B, V) < 0.2).to(dev)
    outs = []
    for model in (vlm.MoeModel(), WithFrames()):
        g, tg = _train_graph(model, losses.CrossEntropyLoss(), dev, B, identical=False)
        out = tg.step(x, y)
        outs.append((out["loss"].clone(), {k: v.data.clone() for k, v in g.vars.items()}))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in outs[0][1])


# ---- the plugins ------------------------------------------------------------------------------------------------------------------------
B_, F_, D_, V_, M_, L_ = 3, 12, 16, 37, 2, 4              # the host test's shape: scales of 12, 6, 3 and 1 frames


def _flags(flags):
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags set below)
    flags.lstm_cells, flags.moe_num_extend, flags.moe_num_mixtures, flags.is_training = "1024", L_, M_, True


def _case(u8, seed, distill, B=B_):
    from oracle import np_ref
    rs = np.random.RandomState(seed)
    nf = np.array([0, 1, 12], dtype=np.int32) if seed % 2 else np.array([7, 12, 5], dtype=np.int32)
    nf = np.resize(nf, B)
    q = rs.randint(0, 256, size=(B, F_, D_)).astype(np.uint8)
    x32 = np_ref.dequant_l2norm_folded(q, nf).astype(np.float32)          # what the bytes mean: dequantised, padding zeroed, l2-normalised
    y = rs.rand(B, V_) < 0.2
    d = rs.rand(B, V_).astype(np.float32) if distill else None
    return rs, (q if u8 else x32), x32, nf, y, d


def _device_run(name, x, nf, y, d, P, dev, step=False):
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    g, tg = _train_graph(getattr(flm, name)(), losses.CrossEntropyLoss(), dev, x.shape[0], identical=x.dtype != np.uint8)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    dt = None if d is None else torch.from_numpy(d).to(dev)
    tg.forward(*args, distillation_predictions=dt)
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    torch.cuda.synchronize()
    return g, tg, args, dt


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "floats"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("name", R.PLUGINS)
def test_plugin_matches_the_fp64_restatement_on_the_device(dev, flags, monkeypatch, name, fused, u8):
    """predictions, prediction_frames, the Z-rule loss and every Variable's gradient; fused: the time-major scale path and the mix
    kernels, generic: the composed scale path and the composed mix."""
    monkeypatch.setattr(seq_ops, "MULTISCALE_FUSED", fused)
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", fused)
    _flags(flags)
    distill = name == "LstmMultiscaleDitillChainModel"
    if distill:
        flags.distillation_features, flags.distillation_as_input = True, True
    rs, x, x32, nf, y, d = _case(u8, 30 + 2 * R.PLUGINS.index(name) + int(u8), distill)
    P = R.draw(R.variable_shapes(name, D_, V_, L_, M_, distill=distill), rs)
    g, tg, args, dt = _device_run(name, x, nf, y, d, P, dev)
    mix, gate = dict(ops.SCALE_MIX_CALLS), dict(seq_ops.GATE_LSTM_CALLS)
    res = tg.forward(*args, distillation_predictions=dt)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    # which form of the mix and of the gate cell ran
    mixes = name != "LstmMultiscale2Model"
    assert ops.SCALE_MIX_CALLS["kernels" if fused else "composed"] - mix["kernels" if fused else "composed"] == (1 if mixes else 0)
    assert sum(ops.SCALE_MIX_CALLS.values()) - sum(mix.values()) == (1 if mixes else 0)
    assert seq_ops.GATE_LSTM_CALLS["kernels"] - gate["kernels"] == (0 if mixes else L_) and seq_ops.GATE_LSTM_CALLS["composed"] == gate["composed"]
    r64 = R.reference(name, x32, nf, y, P, L_, M_, torch.float64, distill=d)
    r32 = R.reference(name, x32, nf, y, P, L_, M_, torch.float32, distill=d)
    got = {"predictions": res["predictions"].detach().cpu(), "prediction_frames": res["prediction_frames"].detach().cpu(), "loss": loss.detach().cpu()}
    pick = lambda r: {k: r[k].numpy() for k in got}
    tag = "%s %s %s:" % (name, "fused" if fused else "generic", "bytes" if u8 else "floats")
    _report(tag, got, pick(r64), pick(r32))
    grads = {}
    for k, v in g.vars.items():
        if v.trainable:
            grads[k] = (v.grad if v.grad_written else torch.zeros_like(v.grad)).detach().cpu()
    assert set(grads) == set(r64["grads"])
    worst = max(((k, R.err(grads[k], r64["grads"][k].numpy()), R.err(r32["grads"][k], r64["grads"][k].numpy())) for k in grads), key=lambda t: t[1])
    print(tag, "worst gradient %s %.2g (fp32 %.2g)" % worst)
    _report(tag + " gradients", grads, {k: t.numpy() for k, t in r64["grads"].items()}, {k: t.numpy() for k, t in r32["grads"].items()}, kind="gradient")
    assert float(grads["ensemble_weight2d"].abs().max()) == 0.0          # label_loss * 0.0: nothing reaches it through predictions


def test_sixteen_videos_of_bytes_take_the_byte_cnn(dev, flags, monkeypatch):
    """B = 16: scale 1 reads the reader's bytes through seq_ops.u8_cnn_tm (B % 16 == 0), as MultiscaleCnnLstmModel."""
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", True)
    _flags(flags)
    name = "LstmMultiscaleModel"
    rs, q, x32, nf, y, _ = _case(True, 61, False, B=16)
    assert seq_ops.u8_cnn_supported(torch.from_numpy(q).to(dev))
    P = R.draw(R.variable_shapes(name, D_, V_, L_, M_), rs)
    g, tg, args, _ = _device_run(name, q, nf, y, None, P, dev)
    seen = []
    inner = seq_ops.u8_cnn_tm
    monkeypatch.setattr(seq_ops, "u8_cnn_tm", lambda *a, **k: seen.append(1) or inner(*a, **k))
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [1]
    r64 = R.reference(name, x32, nf, y, P, L_, M_, torch.float64)
    r32 = R.reference(name, x32, nf, y, P, L_, M_, torch.float32)
    got = {"predictions": res["predictions"].detach().cpu(), "prediction_frames": res["prediction_frames"].detach().cpu(), "loss": loss.detach().cpu()}
    _report("B = 16 bytes:", got, {k: r64[k].numpy() for k in got}, {k: r32[k].numpy() for k in got})
    grads = {k: v.grad.detach().cpu() for k, v in g.vars.items() if v.trainable and v.grad_written}
    _report("B = 16 bytes gradients", grads, {k: r64["grads"][k].numpy() for k in grads}, {k: r32["grads"][k].numpy() for k in grads}, kind="gradient")


def test_predictions_gradient_runs_through_the_mix_and_its_grouped_products(dev, flags, monkeypatch):
    """Outside a training step predictions are differentiable: the mix kernels' backward, the grouped logit products' dW into the planes
    of ensemble_weight2d and their dx into the memories, against the fp64 restatement."""
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", True)
    _flags(flags)
    name = "LstmMultiscaleModel"
    rs, x, x32, nf, y, d = _case(False, 41, False)
    P = R.draw(R.variable_shapes(name, D_, V_, L_, M_), rs)
    g, tg, args, _ = _device_run(name, x, nf, y, None, P, dev)
    res = tg.forward(*args)
    coef = rs.randn(B_, V_).astype(np.float32)
    (res["predictions"] * torch.from_numpy(coef).to(dev)).sum().backward()
    torch.cuda.synchronize()
    refs = {}
    for dtp in (torch.float64, torch.float32):
        tp = R.to_torch(P, dtp)
        r = R.model(name, torch.from_numpy(x32).to(dtp), torch.from_numpy(nf), tp, L_, M_)
        (r["predictions"] * torch.from_numpy(coef).to(dtp)).sum().backward()
        refs[dtp] = {k: t.grad.numpy() for k, t in tp.items() if t.grad is not None}
    grads = {k: g.vars[k].grad.detach().cpu() for k in refs[torch.float64]}
    assert float(np.abs(refs[torch.float64]["ensemble_weight2d"]).max()) > 0
    _report("d predictions:", grads, refs[torch.float64], refs[torch.float32], kind="gradient")


@pytest.mark.parametrize("name", R.PLUGINS)
def test_one_training_step_moves_the_variables_as_the_restatement(dev, flags, monkeypatch, name):
    """TrainGraph.step (forward without a graph for predictions, the Z-rule loss, backward, clip + Adam): every Variable after the step
    against the restatement's first Adam step from the fp64 gradients -- ensemble_weight2d by its l2 term alone (its Adam moment is
    (1 - beta1) l2 w: the label gradient was exact zeros)."""
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", True)
    _flags(flags)
    distill = name == "LstmMultiscaleDitillChainModel"
    if distill:
        flags.distillation_features, flags.distillation_as_input = True, True
    rs, x, x32, nf, y, d = _case(False, 51 + 2 * R.PLUGINS.index(name), distill)
    P = R.draw(R.variable_shapes(name, D_, V_, L_, M_, distill=distill), rs)
    g, tg, args, dt = _device_run(name, x, nf, y, d, P, dev)
    out = tg.step(*args, distill_labels_batch=dt)
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    r64 = R.reference(name, x32, nf, y, P, L_, M_, torch.float64, distill=d)
    assert not out["predictions"].requires_grad
    assert R.err(out["loss"], r64["loss"].numpy()) <= OUT_FLOOR
    LR = 0.01                                                             # TrainGraph's base_learning_rate
    for k, gr in r64["grads"].items():
        v = g.vars[k]
        w0 = torch.from_numpy(P[k]).double()
        w1, m1, _ = R.adam_first_step(w0, gr, v.l2)
        moved = v.data.detach().cpu().double()
        if k == "ensemble_weight2d":
            m = g.adam_m[v.offset:v.offset + v.numel()].view(v.data.shape).cpu().double()
            # (float32 constants: 1 - beta1 is 2.4e-7 off 0.1, l2 6e-8 off 1e-8, two products)
            assert float(gr.abs().max()) == 0.0 and float((m - 0.1 * 1e-8 * w0).abs().max()) <= 2e-6 * 1e-9 * float(w0.abs().max())
            assert float((moved - w1).abs().max()) <= float(np.spacing(np.float32(w0.abs().max())))
            continue
        # Adam's first step is lr sign(g) / (1 + eps / (sqrt(1 - beta2) |g|)), g the clipped gradient: lr = 0.01 where |g| is far above
        # eps / sqrt(1 - beta2) = 3.2e-7.  Elements whose gradient is firm in the fp64 restatement (above four times the gradients' bound,
        # so known to 25 %) must have moved by the restatement's step: a relative error r of g moves the step by at most
        # lr r (3.2e-7 / |g|) < 1e-2 lr there
        firm = gr.abs() > 4 * GRAD_FLOOR * max(1.0, float(gr.abs().max()))
        if bool(firm.any()):
            assert float((moved - w1)[firm].abs().max()) <= 1e-6 + 1e-2 * LR, k
        assert float((moved - w0).abs().max()) <= 1.01 * LR + 1e-7, k    # nobody moves further than one Adam step
