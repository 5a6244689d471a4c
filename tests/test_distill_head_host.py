"""CPU checks of Z's cascade heads (MoeDistillChainModel, MoeDistillChainNormModel, MoeDistillChainNorm2Model, MoeDistillSplitModel:
Z/video_level_models.py:286-582), of the composed forms of ops.distill_input and ops.distill_blend and of the C ABI of
csrc/distill_head.hip without a device: the lookup by name as --model and as --video_level_classifier_model, every Variable's name, shape,
creation order and l2, predictions, loss and every gradient against the float64 restatement (tests/distill_head_restatement.py) at
--ensemble_w 1.0 and 0.2, the assertions, the w == 1 short cut, a training step, and the symbols' signatures and argument validation.

The heads run here on the CPU graph with the device-only ops replaced by their torch meaning on the Variables (ops.linear,
ops.activation, ops.l2_normalize, ops.moe_head: _cpu_ops); the heads, the composed forms of the two ops (which is what CPU tensors take)
and the training rule are the product's own code.  Shape: B = 5, D = 36, V = 37, 3 mixtures, --softmax_bound=10."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distill_head_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_distill_input_supported", "yt8m_distill_input_fwd", "yt8m_distill_input_bwd", "yt8m_distill_blend_supported",
           "yt8m_distill_blend_fwd", "yt8m_distill_blend_bwd")
B_, D_, V_, M_, BOUND_ = 5, 36, 37, 3, 10


# ---- lookup, flags, documents ---------------------------------------------------------------------------------------------------------
def test_find_class_by_name_resolves_the_four_heads(flags):
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in R.HEADS:
        cls = train.find_class_by_name(name, [flm, vlm])                   # --model
        assert cls is getattr(vlm, name) and not hasattr(flm, name)
        flags.video_level_classifier_model = name                         # --video_level_classifier_model
        assert flm._head() is cls
    assert vlm.MoeDistillChainModel.MODE == "chain" and vlm.MoeDistillSplitModel.SPLIT is True


def test_flag_defaults_follow_the_reference(flags):
    import yt8m_amd.train  # noqa: F401  (defines --distillation_type)
    import yt8m_amd.video_level_models  # noqa: F401  (defines the flags)
    assert flags.ensemble_w == 1.0 and flags.softmax_bound == 1000 and flags.distillation_type == 0


def test_not_built_list_names_what_is_left():
    src = open(os.path.join(ROOT, "youtube-8m_amd", "frame_level_models.py")).read()
    assert "MoeDistillChain* heads" not in src
    for name in ("MoeDistillModel", "MoeDistillSplit2Model", "CnnDCCDistillChainModel", "--distillation_type"):
        assert re.search(r"^#   .*%s" % re.escape(name), src, re.M), name


# ---- the C ABI on the host ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_symbols():
    src, lib = declared_bound_exported(SYMBOLS)
    assert "Z/video_level_models.py:286-582" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits_without_a_device():
    lib = L.lib()
    for D, C, V, ok in ((1, 1, 1, 1), (1152, 256, 4716, 1), (8192, 1024, 1 << 30, 1), (2048, 256, 4716, 1), (37, 37, 37, 1),
                        (0, 256, 4716, 0), (1152, 0, 4716, 0), (1152, 256, 0, 0), (-1, 256, 4716, 0), (1 << 25, 256, 4716, 0), (8, 8, 1 << 31, 0)):
        assert lib.yt8m_distill_input_supported(D, C, V) == ok, (D, C, V)
    for rows, V, V1, ok in ((1, 1, 1, 1), (128, 4716, 4716, 1), (1024, 4716, 1000, 1), (0, 37, 10, 0), (3, 37, 0, 0), (3, 37, 38, 0),
                            (3, 0, 0, 0), (1 << 30, 4716, 1000, 0)):
        assert lib.yt8m_distill_blend_supported(rows, V, V1) == ok, (rows, V, V1)


def test_argument_validation_without_device():
    """Every call here fails validation: nothing is launched and no device is needed."""
    lib = L.lib()
    BADARG, SHAPE = -1, -2
    p = lambda k: ctypes.c_void_p(4096 * k)

    def fwd(mode=15, x=p(1), z=p(2), t=p(3), ldt=37, v0=0, V=37, y=p(4), rx=p(5), rc=p(6), sinv=p(7), rows=3, D=36, C=256, eps=1e-12):
        return lib.yt8m_distill_input_fwd(mode, x, z, t, ldt, v0, V, y, rx, rc, sinv, rows, D, C, eps, None)

    def bwd(mode=15, z=p(1), y=p(2), rx=p(3), rc=p(4), sinv=p(5), dy=p(6), dx=p(7), dz=p(8), rows=3, D=36, C=256):
        return lib.yt8m_distill_input_bwd(mode, z, y, rx, rc, sinv, dy, dx, dz, rows, D, C, None)

    assert fwd(mode=16) == BADARG and fwd(mode=-1) == BADARG and fwd(x=None) == BADARG and fwd(sinv=None) == BADARG
    assert fwd(t=None) == BADARG and fwd(v0=37) == BADARG and fwd(v0=-1) == BADARG and fwd(ldt=36) == BADARG and fwd(eps=0.0) == BADARG
    assert fwd(rows=0) == SHAPE and fwd(D=0) == SHAPE and fwd(C=0) == SHAPE and fwd(V=0) == SHAPE
    assert bwd(mode=16) == BADARG and bwd(dz=None) == BADARG and bwd(dy=None) == BADARG and bwd(rows=0) == SHAPE and bwd(C=0) == SHAPE
    assert b"distill_input" in lib.yt8m_last_error()
    assert lib.yt8m_distill_blend_fwd(None, p(1), 37, p(2), 3, 37, 10, 0.5, None) == BADARG
    assert lib.yt8m_distill_blend_fwd(p(3), p(1), 36, p(2), 3, 37, 10, 0.5, None) == BADARG
    assert lib.yt8m_distill_blend_fwd(p(3), p(1), 37, p(2), 3, 37, 38, 0.5, None) == SHAPE
    assert lib.yt8m_distill_blend_bwd(p(1), None, 3, 37, 10, 0.5, None) == BADARG
    assert lib.yt8m_distill_blend_bwd(p(1), p(2), 0, 37, 10, 0.5, None) == SHAPE
    assert b"distill_blend" in lib.yt8m_last_error()


def test_the_default_forms_follow_the_environment_variables():
    import yt8m_amd.ops as ops
    assert ops.DISTILL_INPUT_FUSED is (os.environ.get("YT8M_DISTILL_INPUT_FUSED", "0") != "0")
    assert ops.DISTILL_BLEND_FUSED is (os.environ.get("YT8M_DISTILL_BLEND_FUSED", "0") != "0")
    assert ops.DISTILL_MODES == R.MODES


# ---- the device-only ops as their torch meaning -------------------------------------------------------------------------------------------
def _cpu_ops(monkeypatch):
    """(gradients reach the arena through ops.as_tensor)"""
    import yt8m_amd.ops as ops
    t = ops.as_tensor
    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: x @ t(W) if b is None else x @ t(W) + t(b))
    monkeypatch.setattr(ops, "activation", lambda x, kind: {"relu": torch.relu}[kind](x))
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: R.l2_normalize(x, eps))
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V, M, **k: R.moe(x, t(Wg), t(We), t(be), M))


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


def _case(seed, B=B_):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, D_).astype(np.float32)
    t = rs.rand(B, V_).astype(np.float32)                                 # in (0, 1): the float32 restatement is finite on its own
    y = rs.rand(B, V_) < 0.2
    return rs, x, t, y


def _set(flags, w, name=None):
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags set below)
    flags.moe_num_mixtures, flags.softmax_bound, flags.ensemble_w = M_, BOUND_, w
    if name:
        flags.video_level_classifier_model = name


# ---- ops.distill_input / ops.distill_blend, composed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(R.MODES))
def test_composed_distill_input_is_the_restatement_in_float64_and_carries_the_zero_sum_rule(monkeypatch, mode):
    import yt8m_amd.ops as ops
    _cpu_ops(monkeypatch)
    monkeypatch.setattr(ops, "DISTILL_INPUT_FUSED", True)                 # CPU and float64 tensors take the composed form even then
    rs = np.random.RandomState(3)
    x, z, t = rs.randn(4, 6), rs.randn(4, 9), rs.rand(4, 11)
    t[2, 3:] = 0.0                                                        # zero from column 3 on
    dy = rs.randn(4, 15)
    for v0 in (0, 3):
        xt, zt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(z).requires_grad_(True)
        tt = torch.from_numpy(t).requires_grad_(True)
        before = dict(ops.DISTILL_CALLS)
        y = ops.distill_input(xt, zt, tt, mode, v0)
        assert ops.DISTILL_CALLS["input_composed"] == before["input_composed"] + 1 and ops.DISTILL_CALLS["input_kernels"] == before["input_kernels"]
        y.backward(torch.from_numpy(dy))
        ref = R.distill_input_with_grads(x.astype(np.float64), z, t, mode, v0, dy, torch.float64)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(zt.grad).all())
        assert R.err(y, ref["y"].numpy()) < 1e-14 and R.err(xt.grad, ref["dx"].numpy()) < 1e-13 and R.err(zt.grad, ref["dz"].numpy()) < 1e-12
        assert tt.grad is None                                            # t is data
        if R.MODES[mode][2] and v0 == 3:                                  # the zero-sum row: zeros, and a zero gradient for its z
            assert float(y.detach()[2, 6:].abs().max()) == 0.0 and float(zt.grad[2].abs().max()) == 0.0
            assert float(zt.grad[1].abs().max()) > 0.0
    with pytest.raises(ValueError):
        ops.distill_input(xt, zt, tt, "norm3")
    with pytest.raises(ValueError):
        ops.distill_input(xt, zt, tt, mode, 11)
    with pytest.raises(ValueError):
        ops.distill_input(xt, zt[:3], tt, mode)


@pytest.mark.parametrize("w", [1.0, 0.2, 0.0])
@pytest.mark.parametrize("v1", [11, 4])
def test_composed_distill_blend_is_the_restatement_in_float64(monkeypatch, w, v1):
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "DISTILL_BLEND_FUSED", True)
    rs = np.random.RandomState(4)
    p1, t, dout = rs.rand(3, v1), rs.rand(3, 11), rs.randn(3, 11)
    pt, tt = torch.from_numpy(p1).requires_grad_(True), torch.from_numpy(t).requires_grad_(True)
    before = dict(ops.DISTILL_CALLS)
    out = ops.distill_blend(pt, tt, w, v1)
    if w == 1.0 and v1 == 11:
        assert out is pt and ops.DISTILL_CALLS == before                  # the Chain heads' training setting: p1 itself
        return
    assert ops.DISTILL_CALLS["blend_composed"] == before["blend_composed"] + 1 and ops.DISTILL_CALLS["blend_kernels"] == before["blend_kernels"]
    out.backward(torch.from_numpy(dout))
    ref = R.distill_blend_with_grads(p1, t, w, dout, torch.float64)
    assert R.err(out, ref["out"].numpy()) < 1e-15 and R.err(pt.grad, ref["dp1"].numpy()) < 1e-15 and tt.grad is None
    assert torch.equal(out[:, v1:], tt[:, v1:].detach() * float(np.float32(w)) + tt[:, v1:].detach() * float(np.float32(1) - np.float32(w)))
    with pytest.raises(ValueError):
        ops.distill_blend(pt, tt, w, v1 + 1)
    with pytest.raises(ValueError):
        ops.distill_blend(pt[:2], tt, w, v1)


# ---- the heads on the CPU graph ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.HEADS)
def test_variable_names_shapes_order_and_l2(monkeypatch, flags, name):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1.0)
    g = _graph()
    _, x, t, _ = _case(1)
    res = getattr(vlm, name)().create_model(torch.from_numpy(x), vocab_size=V_, distillation_predictions=torch.from_numpy(t).double(),
                                            unknown_kwarg=1, labels=None, num_frames=None)
    assert tuple(res["predictions"].shape) == (B_, V_) and res["predictions"].dtype == torch.float32       # t is cast to fp32
    want = R.variable_shapes(name, D_, V_, M_, BOUND_)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(want.items())                     # names, shapes, creation order
    v1 = BOUND_ if name == "MoeDistillSplitModel" else V_
    assert want["class_inputs/weights"] == ((V_ - v1) if name == "MoeDistillSplitModel" else V_, 256)
    assert want["gates/weights"] == (D_ + 256, v1 * (M_ + 1)) and "gates/biases" not in g.vars
    for k, v in g.vars.items():
        assert v.trainable and v.l2 == (1e-8 if k.endswith("/weights") else 0.0), k
        if k.endswith("/biases"):
            assert bool((v.data == 0).all()), k
        else:                                                             # slim.fully_connected weights: xavier
            lim = np.sqrt(6.0 / (v.data.shape[0] + v.data.shape[1]))
            assert float(v.data.abs().max()) <= lim and float(v.data.abs().max()) > 0.9 * lim, k


def _run_head(name, x, t, y, P, x_grad=True):
    import yt8m_amd.train as train
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.video_level_models as vlm
    g = _graph()
    model = train.find_class_by_name(name, [flm, vlm])()
    kw = dict(vocab_size=V_, distillation_predictions=torch.from_numpy(t))
    g.begin_step()
    model.create_model(torch.from_numpy(x), **kw)
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v))
    g.begin_step()
    xt = torch.from_numpy(x).requires_grad_(x_grad)
    res = model.create_model(xt, **kw)
    loss = R.cross_entropy(res["predictions"], torch.from_numpy(y))
    loss.backward()
    return res, loss.detach(), {k: v.grad.detach().clone() for k, v in g.vars.items()}, xt.grad


def _check(tag, got, r64, r32, floor=None):
    """floor None: ensemble_restatement.bound.  Otherwise the rule of tests/test_gpu_gate_lstm.py for what lies behind the recurrence,
    eight times the float32 restatement's error and never below `floor` relative to max(1, max |ref|): the cell's composed form
    multiplies concatenated operands ([Wog|Wc], [Wi|Wf]) and so sums in another order than the restatement's twelve separate products,
    which a scalar gradient such as bf's, a sum over every frame, shows at a few 1e-9."""
    for k in got:
        assert bool(torch.isfinite(r32[k]).all()), k
        e = float((got[k].double() - r64[k]).abs().max())
        b = R.bound(r32[k], r64[k]) if floor is None else max(8.0 * R.err(r32[k], r64[k].numpy()), floor) * max(1.0, float(r64[k].abs().max()))
        print("%s %s: error %.3g, float32 restatement %.3g, bound %.3g" % (tag, k, e, float((r32[k].double() - r64[k]).abs().max()), b))
        assert e <= b, (tag, k, e, b)


@pytest.mark.parametrize("w", [1.0, 0.2])
@pytest.mark.parametrize("name", R.HEADS)
def test_head_as_model_matches_the_float64_restatement(monkeypatch, flags, name, w):
    """--model=<head>: predictions, loss, the gradient of every variable and of x.  Bound: ensemble_restatement.bound -- four times the
    float32 restatement's own error plus one float32 ulp of the largest reference magnitude."""
    import yt8m_amd.ops as ops
    _cpu_ops(monkeypatch)
    _set(flags, w)
    rs, x, t, y = _case(7 + R.HEADS.index(name))
    P = R.draw(R.variable_shapes(name, D_, V_, M_, BOUND_), rs)
    before = dict(ops.DISTILL_CALLS)
    res, loss, grads, dx = _run_head(name, x, t, y, P)
    assert ops.DISTILL_CALLS["input_composed"] == before["input_composed"] + 2 and ops.DISTILL_CALLS["input_kernels"] == before["input_kernels"]
    chain_at_one = w == 1.0 and name != "MoeDistillSplitModel"                # the short cut: no blend at all
    assert ops.DISTILL_CALLS["blend_composed"] == before["blend_composed"] + (0 if chain_at_one else 2)
    r64 = R.reference(name, x, t, y, P, M_, torch.float64, w, BOUND_)
    r32 = R.reference(name, x, t, y, P, M_, torch.float32, w, BOUND_)
    got = {"predictions": res["predictions"].detach(), "loss": loss, "dx": dx}
    _check(name, got, r64, r32)
    assert set(grads) == set(r64["grads"])
    _check(name + " gradient of", grads, r64["grads"], r32["grads"])
    for k in grads:
        assert (float(grads[k].abs().max()) > 0) == (w != 0.0), k
    if name == "MoeDistillSplitModel":                                    # the labels from --softmax_bound on are the teacher's own
        tt = torch.from_numpy(t)
        assert torch.equal(res["predictions"].detach()[:, BOUND_:],
                           tt[:, BOUND_:] * float(np.float32(w)) + tt[:, BOUND_:] * float(np.float32(1) - np.float32(w)))


@pytest.mark.parametrize("w", [1.0, 0.2])
@pytest.mark.parametrize("name", R.HEADS)
def test_head_behind_a_frame_level_model_matches_the_float64_restatement(monkeypatch, flags, name, w):
    """--model=LstmGateModel --video_level_classifier_model=<head>: the head's input is the cell's memory, which needs its gradient:
    every one of the cell's twelve Variables against the restatement.  F = 4 frames of 8 features, 36 cells."""
    import yt8m_amd.train as train
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, w, name)
    F, Din = 4, 8
    flags.lstm_cells = str(D_)
    rs, _, t, y = _case(20 + R.HEADS.index(name))
    frames = rs.randn(B_, F, Din).astype(np.float32)
    nf = np.array([4, 1, 3, 0, 2], dtype=np.int32)
    shapes = {"lstm_forward/" + n: s for n, s in R.gate_shapes(Din, D_).items()}
    shapes.update(R.variable_shapes(name, D_, V_, M_, BOUND_))
    P = R.draw(shapes, rs)
    g = _graph()
    model = train.find_class_by_name("LstmGateModel", [flm, vlm])()
    kw = dict(vocab_size=V_, num_frames=torch.from_numpy(nf), distillation_predictions=torch.from_numpy(t), labels=None, noise_level=None)
    g.begin_step()
    model.create_model(torch.from_numpy(frames), **kw)
    g.finalize()
    assert list(g.vars) == list(shapes)                                   # the cell's Variables, then the head's in its order
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).view(g.vars[k].data.shape))
    g.begin_step()
    res = model.create_model(torch.from_numpy(frames), **kw)
    loss = R.cross_entropy(res["predictions"], torch.from_numpy(y))
    loss.backward()
    r64 = R.gate_reference(name, frames, nf, t, y, P, M_, torch.float64, w, BOUND_)
    r32 = R.gate_reference(name, frames, nf, t, y, P, M_, torch.float32, w, BOUND_)
    _check(name + " behind LstmGateModel", {"predictions": res["predictions"].detach(), "loss": loss.detach()}, r64, r32, floor=2e-6)
    grads = {k: v.grad.detach().view(r64["grads"][k].shape) for k, v in g.vars.items()}
    _check(name + " behind LstmGateModel, gradient of", grads, r64["grads"], r32["grads"], floor=5e-6)
    assert float(grads["lstm_forward/Wc"].abs().max()) > 0


# ---- assertions, the short cut, t as data ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.HEADS)
def test_a_head_without_distillation_predictions_raises_the_assertion_of_distill_link(monkeypatch, flags, name):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1.0)
    _graph()
    _, x, _, _ = _case(2)
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        getattr(vlm, name)().create_model(torch.from_numpy(x), vocab_size=V_)
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        vlm.distill_link(None, 8, 1e-8)


@pytest.mark.parametrize("bad", [0, -3, V_, V_ + 5])
def test_split_head_asserts_its_bound(monkeypatch, flags, bad):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1.0)
    flags.softmax_bound = bad
    g = _graph()
    _, x, t, _ = _case(2)
    with pytest.raises(AssertionError, match="softmax_bound"):
        vlm.MoeDistillSplitModel().create_model(torch.from_numpy(x), vocab_size=V_, distillation_predictions=torch.from_numpy(t))
    assert not g.vars                                                     # before any Variable is created
    flags.softmax_bound = V_ - 1
    assert tuple(vlm.MoeDistillSplitModel().create_model(torch.from_numpy(x), vocab_size=V_, distillation_predictions=torch.from_numpy(t))
                 ["predictions"].shape) == (B_, V_)


def test_chain_heads_at_w_one_return_the_moe_predictions_themselves(monkeypatch, flags):
    import yt8m_amd.ops as ops
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1.0)
    seen = []
    inner = ops.moe_head
    monkeypatch.setattr(ops, "moe_head", lambda *a, **k: seen.append(inner(*a, **k)) or seen[-1])
    _, x, t, _ = _case(5)
    for name in R.HEADS[:3]:
        _graph()
        res = getattr(vlm, name)().create_model(torch.from_numpy(x), vocab_size=V_, distillation_predictions=torch.from_numpy(t))
        assert res["predictions"].data_ptr() == seen[-1].data_ptr() and torch.equal(res["predictions"], seen[-1])
    p1 = torch.rand(3, V_)
    assert ops.distill_blend(p1, torch.rand(3, V_), 1.0, V_) is p1
    assert ops.distill_blend(p1, torch.rand(3, V_), 0.5, V_) is not p1 and ops.distill_blend(p1[:, :5].contiguous(), torch.rand(3, V_), 1.0, 5).shape[1] == V_


@pytest.mark.parametrize("name", R.HEADS)
def test_the_teacher_predictions_get_no_gradient(monkeypatch, flags, name):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 0.2)
    _graph()
    _, x, t, y = _case(6)
    tt = torch.from_numpy(t).requires_grad_(True)
    res = getattr(vlm, name)().create_model(torch.from_numpy(x), vocab_size=V_, distillation_predictions=tt)
    R.cross_entropy(res["predictions"], torch.from_numpy(y)).backward()
    assert tt.grad is None


# ---- a training step -----------------------------------------------------------------------------------------------------------------------
class _Loss(object):
    """Stands for --label_loss=CrossEntropyLoss (device code): the restatement's cross entropy."""

    def calculate_loss(self, predictions, labels, weights=None, **unused_params):
        return R.cross_entropy(predictions, labels)


@pytest.mark.parametrize("name", R.HEADS)
def test_training_step_with_distillation_as_input_moves_the_variables(monkeypatch, flags, name):
    """TrainGraph.step with --distillation_features --distillation_as_input (--distillation_type=0: the plain label loss): the teacher's
    predictions reach the head, every Variable gets a gradient and moves.  ops.sqnorm_and_adam is device code; a plain gradient step on
    the same arenas stands in for it here (the device's own pass runs in tests/test_gpu_distill_head.py)."""
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.ops as ops
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1.0)
    flags.distillation_features, flags.distillation_as_input = True, True
    calls = []

    def sgd(graph, lr_t, tensors=None, **k):
        calls.append(tensors)
        for v in graph.trainable_variables()[tensors[0]:tensors[1]]:
            v.data.sub_(lr_t * v.grad)

    monkeypatch.setattr(ops, "sqnorm_and_adam", sgd)
    _, x, t, y = _case(9)
    g = _graph()
    model = getattr(vlm, name)()
    seen = {}
    create = model.create_model
    model.create_model = lambda *a, **k: seen.update(k) or create(*a, **k)
    tg = train.TrainGraph(model, label_loss_fn=_Loss(), batch_size=B_, graph=g, transformer_class=ft.IdenticalTransformer)
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        tg.step(torch.from_numpy(x), torch.from_numpy(y))                 # no teacher in the batch
    g = _graph()
    tg = train.TrainGraph(model, label_loss_fn=_Loss(), batch_size=B_, graph=g, transformer_class=ft.IdenticalTransformer)
    tt = torch.from_numpy(t)
    out = tg.step(torch.from_numpy(x), torch.from_numpy(y), distill_labels_batch=tt)
    assert seen["distillation_predictions"] is tt and calls == [(0, 5)]
    start = {k: v.data.clone() for k, v in g.vars.items()}
    out2 = tg.step(torch.from_numpy(x), torch.from_numpy(y), distill_labels_batch=tt)
    for k, v in g.vars.items():
        assert v.grad_written and float(v.grad.abs().max()) > 0 and not torch.equal(v.data, start[k]), k
    assert tuple(out["predictions"].shape) == (B_, V_) and float(out2["loss"]) < float(out["loss"])
