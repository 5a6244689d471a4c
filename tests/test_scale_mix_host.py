"""CPU checks of the LstmMultiscale plugins (Z/frame_level_models.py:2827-3373), of ops.scale_mix's composed form, of the Z training
rule in train.TrainGraph (Z/train.py:359-379) and of the C ABI of csrc/scale_mix.hip: the lookup by name, every Variable's name, shape,
l2 and initial values against a table written from the reference, forward and gradients of each plugin against the float64
restatement (tests/scale_mix_restatement.py), the loss on prediction_frames with tiled labels, the two ValueErrors, and the symbols'
signatures and argument validation without a device.

The plugins run here on the CPU graph with the device-only ops replaced by their torch meaning on the Variables (ops.linear,
ops.batch_norm, ops.activation, ops.moe_head, seq_ops.lstm_stack: _cpu_ops); the scale loop, the gate cell's composed form, the grouped
logit products' host form, ops.scale_mix and the training rule are the product's own code."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scale_mix_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_scale_mix_supported", "yt8m_scale_mix_fwd", "yt8m_scale_mix_bwd")
B_, F_, D_, V_, M_, L_ = 3, 12, 16, 37, 2, 4              # scales of 12, 6, 3 and 1 frames


# ---- lookup, flags --------------------------------------------------------------------------------------------------------------------
def test_find_class_by_name_resolves_the_three_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in R.PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True and cls.trains_on_prediction_frames is True
        assert issubclass(cls, flm.MultiscaleCnnLstmModel)               # the scale loop is shared
    assert not getattr(flm.MultiscaleCnnLstmModel, "trains_on_prediction_frames", False)


def test_flag_defaults_follow_the_reference(flags):
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags)
    assert flags.cnn_cells == 256 and flags.moe_num_extend == 8


def test_not_built_list_names_what_is_left():
    src = open(os.path.join(ROOT, "youtube-8m_amd", "frame_level_models.py")).read()
    assert "LstmMultiscale*:" not in src
    assert "#   LstmMultiscale3Model:" in src and "#   LstmMultiscaleRebuildModel:" in src


# ---- the C ABI on the host ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_scale_mix_symbols():
    src, lib = declared_bound_exported(SYMBOLS)
    assert L.SIGNATURES["yt8m_scale_mix_supported"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64])
    assert L.SIGNATURES["yt8m_scale_mix_fwd"] == (ctypes.c_int, [ctypes.c_int, L.PP, L.PP, L.P, ctypes.c_int64, ctypes.c_int64, L.P])
    assert L.SIGNATURES["yt8m_scale_mix_bwd"] == (ctypes.c_int, [ctypes.c_int, L.PP, L.PP, L.P, L.P, L.PP, L.PP, ctypes.c_int64,
                                                                 ctypes.c_int64, L.P])
    assert "Z/frame_level_models.py:2977-2985" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits_without_a_device():
    lib = L.lib()
    for Lx, rows, cols, ok in ((1, 3, 37, 1), (4, 128, 4716, 1), (8, 1024, 4716, 1), (2, 1, 1, 1), (0, 128, 4716, 0), (9, 128, 4716, 0),
                               (-1, 3, 37, 0), (4, 0, 4716, 0), (4, 128, 0, 0), (4, -5, 37, 0), (4, 1 << 31, 8, 0), (4, 1 << 30, 1 << 20, 0)):
        assert lib.yt8m_scale_mix_supported(Lx, rows, cols) == ok, (Lx, rows, cols)


def test_argument_validation_without_device():
    """Every call here fails validation or has nothing to do: nothing is launched and no device is needed."""
    lib = L.lib()
    OK, BADARG, SHAPE = 0, -1, -2
    table = lambda n, null=(): (ctypes.c_void_p * 8)(*[None if k in null else 256 * (k + 1) for k in range(n)] + [None] * (8 - n))
    out, g = ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def fwd(Lx=4, p=None, z=None, out=out, rows=3, cols=37):
        return lib.yt8m_scale_mix_fwd(Lx, p or table(4), z or table(4), out, rows, cols, None)

    def bwd(Lx=4, p=None, z=None, out=out, g=g, dp=None, dz=None, rows=3, cols=37):
        return lib.yt8m_scale_mix_bwd(Lx, p or table(4), z or table(4), out, g, dp or table(4), dz or table(4), rows, cols, None)

    for call in (fwd, bwd):
        assert call(Lx=0) == SHAPE and call(Lx=9) == SHAPE and call(rows=0) == SHAPE and call(cols=0) == SHAPE and call(rows=-1) == SHAPE
        assert call(out=None) == BADARG
        assert call(p=table(4, null=(2,))) == BADARG and call(z=table(4, null=(0,))) == BADARG          # a null plane
    assert bwd(g=None) == BADARG
    assert b"scale_mix" in lib.yt8m_last_error()
    assert bwd(dp=table(0), dz=table(0)) == OK                            # no gradient wanted: nothing to do


# ---- ops.scale_mix, composed ----------------------------------------------------------------------------------------------------------
def _planes(rs, Lx, B, V, dtype=torch.float64):
    ps = [torch.from_numpy(rs.rand(B, V)).to(dtype).requires_grad_(True) for _ in range(Lx)]
    zs = [torch.from_numpy(rs.randn(B, V) * 2).to(dtype).requires_grad_(True) for _ in range(Lx)]
    return ps, zs


def test_scale_mix_composed_gradcheck_in_float64():
    import yt8m_amd.ops as ops
    rs = np.random.RandomState(3)
    for Lx in (1, 2, 5):
        ps, zs = _planes(rs, Lx, 2, 5)
        before = dict(ops.SCALE_MIX_CALLS)
        assert torch.autograd.gradcheck(lambda *t: ops.scale_mix(t[:Lx], t[Lx:]), ps + zs, eps=1e-6, atol=1e-8)
        assert ops.SCALE_MIX_CALLS["kernels"] == before["kernels"] and ops.SCALE_MIX_CALLS["composed"] > before["composed"]
        out = ops.scale_mix(ps, zs)
        assert R.err(out, R.scale_mix(ps, zs).detach().numpy()) < 1e-15
        assert R.err(ops.scale_mix(ps, torch.stack(zs)), out.detach().numpy()) == 0.0        # z as one [L,B,V] tensor


def test_scale_mix_of_one_plane_is_the_plane_and_its_logit_gets_zeros():
    import yt8m_amd.ops as ops
    rs = np.random.RandomState(4)
    ps, zs = _planes(rs, 1, 3, 7, torch.float32)
    out = ops.scale_mix(ps, zs)
    assert torch.equal(out, ps[0])
    out.backward(torch.from_numpy(rs.randn(3, 7).astype(np.float32)))
    assert torch.equal(zs[0].grad, torch.zeros(3, 7))


def test_scale_mix_beyond_eight_planes_and_other_dtypes_take_the_composed_form(monkeypatch):
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "SCALE_MIX_FUSED", True)                     # even when the kernels are asked for
    rs = np.random.RandomState(5)
    for Lx, dtype in ((9, torch.float32), (4, torch.float64), (4, torch.float32)):      # L > 8; not float32; CPU tensors
        ps, zs = _planes(rs, Lx, 3, 7, dtype)
        before = dict(ops.SCALE_MIX_CALLS)
        out = ops.scale_mix(ps, zs)
        assert ops.SCALE_MIX_CALLS["kernels"] == before["kernels"] and ops.SCALE_MIX_CALLS["composed"] == before["composed"] + 1
        assert R.err(out, R.scale_mix([p.double() for p in ps], [z.double() for z in zs]).detach().numpy()) < 1e-6
    with pytest.raises(ValueError):
        ops.scale_mix(ps, zs[:3])
    with pytest.raises(ValueError):
        ops.scale_mix(ps, [z[:, :5] for z in zs])


def test_the_default_form_follows_the_environment_variable():
    import yt8m_amd.ops as ops
    want = os.environ.get("YT8M_SCALE_MIX_FUSED", "0") != "0"             # composed until the op leg has been measured on the device
    assert ops.SCALE_MIX_FUSED is want


# ---- the plugins on the CPU graph -----------------------------------------------------------------------------------------------------
def _cpu_ops(monkeypatch):
    """The device-only ops as their torch meaning on the Variables (gradients reach the arena through ops.as_tensor)."""
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from oracle import torch_ref
    t = ops.as_tensor

    def batch_norm(x, gamma, beta, mm, mv, is_training, eps=1e-3, decay=0.999):
        if not is_training:
            return t(gamma) * (x - mm.data) * torch.rsqrt(mv.data + eps) + t(beta)
        y, mu, var = torch_ref.batch_norm_train(x, t(gamma), t(beta), eps=eps)
        with torch.no_grad():
            mm.data.mul_(decay).add_((1 - decay) * mu)
            mv.data.mul_(decay).add_((1 - decay) * var)
        return y

    def lstm_stack(x_tm, num_frames, wb, **k):
        outs, c, h = torch_ref.lstm_stack(x_tm.transpose(0, 1), num_frames, [(t(W), t(b)) for W, b in wb], forget_bias=k.get("forget_bias", 1.0))
        return outs.transpose(0, 1), list(zip(c, h))

    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: x @ t(W) if b is None else x @ t(W) + t(b))
    monkeypatch.setattr(ops, "batch_norm", batch_norm)
    monkeypatch.setattr(ops, "activation", lambda x, kind: {"relu": torch.relu}[kind](x))
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V, M, **k: R.moe(x, t(Wg), t(We), t(be), M))
    monkeypatch.setattr(seq_ops, "lstm_stack", lstm_stack)


def _flags(flags, lstm_cells=1024, Lx=L_):
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags set below)
    flags.lstm_cells, flags.moe_num_extend, flags.moe_num_mixtures, flags.is_training = str(lstm_cells), Lx, M_, True


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


def _case(nf, seed, distill):
    rs = np.random.RandomState(seed)
    nf = np.asarray(nf, dtype=np.int32)
    x = rs.randn(B_, F_, D_).astype(np.float32)
    x /= np.sqrt((x * x).sum(axis=2, keepdims=True))
    x *= (np.arange(F_)[None, :] < nf[:, None])[:, :, None]              # the reader's zero padding
    y = rs.rand(B_, V_) < 0.2
    d = rs.rand(B_, V_).astype(np.float32) if distill else None
    return rs, x, nf, y, d


@pytest.mark.parametrize("name,distill", [(n, False) for n in R.PLUGINS] + [("LstmMultiscaleDitillChainModel", True)])
def test_variable_names_shapes_l2_and_initial_values(monkeypatch, flags, name, distill):
    import yt8m_amd.frame_level_models as flm
    _cpu_ops(monkeypatch)
    _flags(flags, lstm_cells=512 if name == "LstmMultiscaleDitillChainModel" else 1024)
    flags.cnn_cells = 128 if name == "LstmMultiscaleDitillChainModel" else 256
    flags.is_training = False                                             # the moving averages stay at their initial values
    g = _graph()
    _, x, nf, y, d = _case([0, 1, 12], 1, distill)
    kw = {"distillation_predictions": torch.from_numpy(d)} if distill else {}
    res = getattr(flm, name)().create_model(torch.from_numpy(x), vocab_size=V_, num_frames=torch.from_numpy(nf), unknown_kwarg=1, **kw)
    assert tuple(res["predictions"].shape) == (B_, V_) and tuple(res["prediction_frames"].shape) == (B_ * L_, V_)
    H = int(flags.lstm_cells)
    want = R.variable_shapes(name, D_, V_, L_, M_, lstm_cells=H, cnn_cells=flags.cnn_cells, distill=distill)
    assert {k: tuple(v.data.shape) for k, v in g.vars.items()} == want
    # ensemble_weight2d's depth per class: sum(filters) = 1024 in the two models that write features_size, lstm_cells in the cascade one
    assert want["ensemble_weight2d"] == ((L_, 512, V_) if name == "LstmMultiscaleDitillChainModel" else (L_, 1024, V_))
    C = sum(R.num_filters(name, flags.cnn_cells))
    for k, v in g.vars.items():
        leaf = k.split("/")[-1]
        assert v.trainable == (not leaf.startswith("moving_")), k
        if "cnn-filter" in k:                                             # truncated_normal(stddev=0.1), l2 1e-8
            assert v.l2 == 1e-8 and float(v.data.abs().max()) <= 0.2 + 1e-7 and abs(float(v.data.std()) - 0.08796) < 0.01, k
        elif leaf in ("gamma", "moving_variance"):
            assert v.l2 == 0.0 and bool((v.data == 1).all()), k
        elif leaf in ("beta", "moving_mean") or leaf == "biases":
            assert v.l2 == 0.0 and bool((v.data == 0).all()), k
        elif "lstm_forward/" in k:                                        # create_recurrent_unit: every one under l2 1e-8
            assert v.l2 == 1e-8, k
            if leaf == "bf":
                assert float(v.data) == 1.0
            elif leaf[0] == "b":
                assert bool((v.data == np.float32(0.1)).all()), k
            else:
                assert float(v.data.abs().max()) <= 0.2 + 1e-7 and float(v.data.std()) > 0.03, k
        elif k == "ensemble_weight2d":                                    # get_variable without initialiser: glorot uniform on [L, d, V]
            lim = np.sqrt(6.0 / (L_ * v.data.shape[1] + L_ * V_))
            assert v.l2 == 1e-8 and float(v.data.abs().max()) <= lim and float(v.data.abs().max()) > 0.95 * lim, k
        elif "basic_lstm_cell/weights" in k:
            lim = np.sqrt(6.0 / (C + H + 4 * H))
            assert v.l2 == 0.0 and float(v.data.abs().max()) <= lim and float(v.data.abs().max()) > 0.95 * lim, k
        else:                                                             # slim.fully_connected weights: xavier, l2 1e-8
            assert leaf == "weights" and v.l2 == 1e-8, k
            lim = np.sqrt(6.0 / (v.data.shape[0] + v.data.shape[1]))
            assert float(v.data.abs().max()) <= lim and float(v.data.abs().max()) > 0.9 * lim, k


def _run(name, x, nf, y, P, d, predictions_no_grad=False):
    """Forward, the Z-rule cross entropy of the restatement on the result, backward: predictions, prediction_frames, loss, gradients."""
    import yt8m_amd.frame_level_models as flm
    g = _graph()
    model = getattr(flm, name)()
    kw = {"distillation_predictions": torch.from_numpy(d)} if d is not None else {}
    args = (torch.from_numpy(x),)
    g.begin_step()
    model.create_model(*args, vocab_size=V_, num_frames=torch.from_numpy(nf), **kw)
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v))
    g.begin_step()
    res = model.create_model(*args, vocab_size=V_, num_frames=torch.from_numpy(nf), predictions_no_grad=predictions_no_grad, **kw)
    loss = R.z_rule_loss(res, torch.from_numpy(y)) if not predictions_no_grad else \
        R.cross_entropy(res["prediction_frames"], R.tile_labels(torch.from_numpy(y), L_))
    loss.backward()
    for v in g.trainable_variables():
        if not v.grad_written:
            v.grad.zero_()                                                # what TrainGraph.step does for variables the step did not touch
    return res, loss.detach(), {k: v.grad.detach().clone() for k, v in g.vars.items() if v.trainable}, g


@pytest.mark.parametrize("name", R.PLUGINS)
@pytest.mark.parametrize("nf", [[0, 1, 12], [7, 12, 5]], ids=["nf-0-1-12", "nf-7-12-5"])
def test_plugin_forward_and_gradients_match_the_float64_restatement(monkeypatch, flags, name, nf):
    """B = 3, F = 12 (scales of 12, 6, 3 and 1 frames), V = 37, 2 mixtures, --lstm_cells=1024.  The rows with 0 and 1 frames exercise
    max(n // 2, 1) and the gate cell's convention for rows without frames.  Bound: ensemble_restatement.bound -- four times the float32
    restatement's own error plus one float32 ulp of the largest reference magnitude."""
    import yt8m_amd.ops as ops
    _cpu_ops(monkeypatch)
    _flags(flags)
    distill = name == "LstmMultiscaleDitillChainModel"
    rs, x, nf, y, d = _case(nf, 7, distill)
    shapes = R.variable_shapes(name, D_, V_, L_, M_, distill=distill)
    P = R.draw(shapes, rs)
    before = dict(ops.SCALE_MIX_CALLS)
    res, loss, grads, _ = _run(name, x, nf, y, P, d)
    mixes = name != "LstmMultiscale2Model"
    assert ops.SCALE_MIX_CALLS["composed"] - before["composed"] == (2 if mixes else 0)       # the graph-building pass and this one
    r64 = R.reference(name, x, nf, y, P, L_, M_, torch.float64, distill=d)
    r32 = R.reference(name, x, nf, y, P, L_, M_, torch.float32, distill=d)
    for key in ("predictions", "prediction_frames", "loss"):
        got = loss if key == "loss" else res[key].detach()
        assert bool(torch.isfinite(r32[key]).all())
        e, b = float((got.double() - r64[key]).abs().max()), R.bound(r32[key], r64[key])
        print("%s %s: error %.3g, float32 restatement %.3g, bound %.3g" % (name, key, e, float((r32[key].double() - r64[key]).abs().max()), b))
        assert e <= b, key
    assert set(grads) == set(r64["grads"])
    for k, ref in r64["grads"].items():
        assert bool(torch.isfinite(r32["grads"][k]).all()), k
        e, b = float((grads[k].double() - ref).abs().max()), R.bound(r32["grads"][k], ref)
        assert e <= b, (k, e, b)
    # ensemble_weight2d: label_loss * 0.0 leaves it without a gradient in all three; the mean model computes nothing from it at all
    assert float(grads["ensemble_weight2d"].abs().max()) == 0.0 and float(r64["grads"]["ensemble_weight2d"].abs().max()) == 0.0
    for k in range(1, L_ + 1):
        assert float(grads["gatesmoe%d/weights" % k].abs().max()) > 0 and float(grads["cnn%dcnn-filter-len3" % k].abs().max()) > 0
    # the rows of prediction_frames: row b L + l is scale l's sub-prediction of video b
    frames = res["prediction_frames"].detach().view(B_, L_, V_)
    if not mixes:
        assert R.err(res["predictions"], frames.double().mean(dim=1).numpy()) < 1e-6


@pytest.mark.parametrize("name", ["LstmMultiscaleModel", "LstmMultiscaleDitillChainModel"])
def test_predictions_carry_the_gradient_of_the_mix_when_they_are_asked_for(monkeypatch, flags, name):
    """Outside a training step predictions are differentiable: ensemble_weight2d and the memories receive the mix's gradient."""
    _cpu_ops(monkeypatch)
    _flags(flags)
    distill = name == "LstmMultiscaleDitillChainModel"
    rs, x, nf, y, d = _case([7, 12, 5], 8, distill)
    P = R.draw(R.variable_shapes(name, D_, V_, L_, M_, distill=distill), rs)
    import yt8m_amd.frame_level_models as flm
    g = _graph()
    model = getattr(flm, name)()
    kw = {"distillation_predictions": torch.from_numpy(d)} if distill else {}
    model.create_model(torch.from_numpy(x), vocab_size=V_, num_frames=torch.from_numpy(nf), **kw)
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v))
    g.begin_step()
    res = model.create_model(torch.from_numpy(x), vocab_size=V_, num_frames=torch.from_numpy(nf), **kw)
    coef = torch.from_numpy(rs.randn(B_, V_).astype(np.float32))
    (res["predictions"] * coef).sum().backward()
    tp = R.to_torch(P, torch.float64)
    t32 = R.to_torch(P, torch.float32)
    outs = {}
    for dt, t in ((torch.float64, tp), (torch.float32, t32)):
        r = R.model(name, torch.from_numpy(x).to(dt), torch.from_numpy(nf), t, L_, M_, distill_labels=None if d is None else torch.from_numpy(d).to(dt))
        (r["predictions"] * coef.to(dt)).sum().backward()
        outs[dt] = r["predictions"].detach()
    for k in ("ensemble_weight2d", "gatesmoe1/weights", "cnn1cnn-filter-len2", "RNN-rnn4/multi_rnn_cell/cell_0/basic_lstm_cell/weights"):
        e = float((g.vars[k].grad.double() - tp[k].grad).abs().max())
        assert float(tp[k].grad.abs().max()) > 0 and e <= R.bound(t32[k].grad, tp[k].grad), (k, e)
    assert float((res["predictions"].detach().double() - outs[torch.float64]).abs().max()) <= R.bound(outs[torch.float32], outs[torch.float64])


def test_the_two_value_errors(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _cpu_ops(monkeypatch)
    _flags(flags, lstm_cells=512)
    _graph()
    _, x, nf, _, _ = _case([0, 1, 12], 2, False)
    with pytest.raises(ValueError, match="--lstm_cells must be 1024"):
        flm.LstmMultiscaleModel().create_model(torch.from_numpy(x), vocab_size=V_, num_frames=torch.from_numpy(nf))
    _flags(flags, lstm_cells=1024, Lx=5)                                  # 12, 6, 3, 1 and then no frame for a fifth scale
    g = _graph()
    with pytest.raises(ValueError, match="moe_num_extend = 5 needs more than 12 frames"):
        flm.LstmMultiscaleModel().create_model(torch.from_numpy(x), vocab_size=V_, num_frames=torch.from_numpy(nf))
    del g                                                                 # (the cascade model at --lstm_cells=512: the Variables test)


# ---- the Z training rule --------------------------------------------------------------------------------------------------------------
class _RecordingLoss(object):
    """Stands for any --label_loss: keeps what it was called with and returns the restatement's cross entropy (weights as
    W/losses.py:124-127 applies them)."""

    def __init__(self):
        self.calls = []

    def calculate_loss(self, predictions, labels, weights=None, **unused_params):
        self.calls.append((predictions, labels, weights))
        y = labels.to(predictions.dtype)
        ce = -(y * torch.log(predictions + 10e-6) + (1 - y) * torch.log(1 - predictions + 10e-6)).sum(1)
        return (ce if weights is None else ce * weights).mean()


def _train_graph(loss_fn, **kw):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.train as train
    return train.TrainGraph(kw.pop("model", object()), label_loss_fn=loss_fn, batch_size=B_, graph=kw.pop("graph", None) or _graph(),
                            transformer_class=ft.IdenticalTransformer, **kw)


def test_loss_on_prediction_frames_is_the_tiled_form(flags):
    import yt8m_amd.train  # noqa: F401
    rs = np.random.RandomState(9)
    frames = torch.from_numpy(rs.rand(B_ * L_, V_)).requires_grad_(True)
    preds = torch.from_numpy(rs.rand(B_, V_)).requires_grad_(True)
    labels = torch.from_numpy(rs.rand(B_, V_) < 0.2)
    distill = torch.from_numpy(rs.rand(B_, V_))
    weights = torch.from_numpy(rs.rand(B_) + 0.5)
    result = {"predictions": preds, "prediction_frames": frames}
    rec = _RecordingLoss()
    tg = _train_graph(rec)
    loss = tg.loss(result, labels)
    assert len(rec.calls) == 1 and rec.calls[0][0] is frames and rec.calls[0][2] is None
    assert torch.equal(rec.calls[0][1], R.tile_labels(labels, L_))
    assert torch.equal(rec.calls[0][1].view(B_, L_, V_)[:, 2], labels)    # row b L + l is video b
    assert float((loss - R.z_rule_loss(result, labels)).detach().abs()) < 1e-14
    # a row-mean loss: the mean over the scales of the per-scale losses
    per_scale = [R.cross_entropy(frames.view(B_, L_, V_)[:, l], labels) for l in range(L_)]
    assert float((loss - sum(per_scale) / L_).detach().abs()) < 1e-13
    loss.backward()
    assert preds.grad is None and float(frames.grad.abs().max()) > 0      # predictions receive no gradient
    # per-video weights are tiled with the labels
    rec.calls.clear()
    lw = tg.loss(result, labels, weights=weights)
    assert torch.equal(rec.calls[0][2], weights.repeat_interleave(L_)) and torch.equal(rec.calls[0][1], R.tile_labels(labels, L_))
    ce = -(R.tile_labels(labels, L_).double() * torch.log(frames + 10e-6) + (1 - R.tile_labels(labels, L_).double()) * torch.log(1 - frames + 10e-6)).sum(1)
    assert float((lw - (ce.view(B_, L_) * weights[:, None]).mean()).detach().abs()) < 1e-13
    # the distillation sources, exactly as loss() picks them for predictions
    flags.distillation_features, flags.distillation_type, flags.distillation_percent = True, 1, 0.25
    rec.calls.clear()
    l1 = tg.loss(result, labels, distill_labels_batch=distill)
    assert [c[0] is frames for c in rec.calls] == [True, True]
    assert torch.equal(rec.calls[0][1], R.tile_labels(labels, L_)) and torch.equal(rec.calls[1][1], R.tile_labels(distill, L_))
    want = 0.75 * R.cross_entropy(frames, R.tile_labels(labels, L_)) + 0.25 * R.cross_entropy(frames, R.tile_labels(distill, L_))
    assert float((l1 - want).detach().abs()) < 1e-13
    flags.distillation_type = 2
    rec.calls.clear()
    tg.loss(result, labels, distill_labels_batch=distill)
    assert len(rec.calls) == 1 and torch.equal(rec.calls[0][1], R.tile_labels(distill, L_))
    flags.distillation_as_boosting = True
    rec.calls.clear()
    tg.loss(result, labels, distill_labels_batch=distill)
    import yt8m_amd.train as train
    assert torch.equal(rec.calls[0][2], train.get_weights_by_predictions(labels, distill).repeat_interleave(L_))


def test_result_without_the_key_goes_through_the_code_as_before(flags):
    rs = np.random.RandomState(10)
    preds = torch.from_numpy(rs.rand(B_, V_))
    labels = torch.from_numpy(rs.rand(B_, V_) < 0.2)
    rec = _RecordingLoss()
    tg = _train_graph(rec)
    a = tg.loss({"predictions": preds}, labels)
    assert rec.calls[0][0] is preds and rec.calls[0][1] is labels         # nothing tiled, nothing copied
    # one row per video: the branch computes the same value from the same tensors, bit for bit
    b = tg.loss({"predictions": preds * 0.5, "prediction_frames": preds}, labels)
    assert torch.equal(a, b) and rec.calls[1][0] is preds and rec.calls[1][1] is labels
    assert tg.loss({"loss": a, "prediction_frames": preds}, labels) is a  # a model-provided loss still wins (W/train.py:384-385)


def test_multitask_with_prediction_frames_raises(flags):
    rs = np.random.RandomState(11)
    preds = torch.from_numpy(rs.rand(B_, V_))
    labels = torch.from_numpy(rs.rand(B_, V_) < 0.2)
    tg = _train_graph(_RecordingLoss(), multitask=True)
    with pytest.raises(ValueError, match="--multitask"):
        tg.loss({"predictions": preds, "support_predictions": preds, "prediction_frames": preds.repeat(L_, 1)}, labels)
    with pytest.raises(ValueError, match="whole number of rows"):
        _train_graph(_RecordingLoss()).loss({"predictions": preds, "prediction_frames": preds.repeat(2, 1)[:-1]}, labels)


@pytest.mark.parametrize("name", R.PLUGINS)
def test_training_step_builds_predictions_without_a_graph_and_leaves_weight2d_to_its_regulariser(monkeypatch, flags, name):
    """TrainGraph.step on the CPU graph up to the optimiser pass (ops.sqnorm_and_adam is device code: recorded here, run in
    tests/test_gpu_scale_mix.py): predictions come back without an autograd graph, every Variable of the scales has a gradient, and
    ensemble_weight2d -- registered, trainable, in the arenas -- reaches the optimiser with a gradient of exact zeros and its l2 term."""
    import yt8m_amd.ops as ops
    _cpu_ops(monkeypatch)
    _flags(flags)
    distill = name == "LstmMultiscaleDitillChainModel"
    if distill:
        flags.distillation_features, flags.distillation_as_input = True, True
    rs, x, nf, y, d = _case([7, 12, 5], 12, distill)
    import yt8m_amd.frame_level_models as flm
    g = _graph()
    seen = {}
    model = getattr(flm, name)()
    create = model.create_model

    def spy(*a, **k):
        seen["kw"] = k
        seen["result"] = create(*a, **k)
        return seen["result"]

    model.create_model = spy
    calls = []
    monkeypatch.setattr(ops, "sqnorm_and_adam", lambda graph, lr_t, **k: calls.append((lr_t, k)))
    tg = _train_graph(_RecordingLoss(), model=model, graph=g)
    out = tg.step(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(nf), distill_labels_batch=None if d is None else torch.from_numpy(d))
    assert seen["kw"].get("predictions_no_grad") is True
    assert not seen["result"]["predictions"].requires_grad and seen["result"]["prediction_frames"].requires_grad
    assert calls and calls[0][1]["tensors"] == (0, len(g.trainable_variables()))
    w2d = g.vars["ensemble_weight2d"]
    assert w2d.trainable and w2d.index >= 0 and w2d.l2 == 1e-8 and float(g.l2[w2d.index]) == np.float32(1e-8)
    assert w2d.grad_written and float(w2d.grad.abs().max()) == 0.0
    assert w2d.data.data_ptr() == g.params[w2d.offset:].data_ptr()       # a view into the parameter arena
    for k, v in g.vars.items():
        # (the last scale has one frame: the head reads c_1 = i g, so of its gate cell only the input gate and the candidate's input
        # side are reached -- the recurrent matrices multiply h_0 = 0, the forget gate c_0 = 0, the output gate an h nobody reads)
        dead = k.startswith("rnn%dlstm_forward/" % L_) and k.split("/")[1] not in ("Wi", "bi", "Wc", "bc")
        if v.trainable and k != "ensemble_weight2d" and not dead:
            assert float(v.grad.abs().max()) > 0, k
    assert tuple(out["predictions"].shape) == (B_, V_)
    # ... and forward() outside a step still hands out differentiable predictions
    res = tg.forward(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(nf),
                     distillation_predictions=None if d is None else torch.from_numpy(d))
    assert res["predictions"].requires_grad
