"""CPU checks of Z's MoeSoftmaxModel (Z/video_level_models.py:877-1017), of SplitSoftmaxLoss (Z's SoftmaxLoss, Z/losses.py:412-456) and
its calculate_loss_mix, of the composed forms of ops.softmax_moe and ops.split_softmax_loss and of the C ABI of csrc/softmax_moe.hip
without a device: the lookup by name in both roles, every Variable's name, shape, creation order and l2 at --moe_layers 0, 1, 2 and 3,
predictions, predictions_class, both training losses and every gradient against the float64 restatement
(tests/softmax_moe_restatement.py), the training rule's hand-over to calculate_loss_mix, the --softmax_bound assertion, the `weights`
error, the clamp of the appended probability, the symbols' signatures, limits and argument validation, and the two switches.

The model runs here on the CPU graph with the device-only ops replaced by their torch meaning on the Variables (_cpu_ops, as
tests/test_mix_chain_host.py); the model, the chain, the composed forms (which is what CPU tensors take) and the losses are the
product's own code.  Shape: B = 5, D = 36, V = 37, 3 mixtures, --class_size=7, --softmax_bound=10."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import softmax_moe_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_softmax_moe_supported", "yt8m_softmax_moe_resident", "yt8m_softmax_moe_fwd", "yt8m_softmax_moe_bwd",
           "yt8m_split_softmax_loss_workspace_bytes", "yt8m_split_softmax_loss_fwd_bwd", "yt8m_split_softmax_loss_bwd")
B_, D_, V_, M_, C_, V1_ = 5, 36, 37, 3, 7, 10
LAYERS = [0, 1, 2, 3]


# ---- lookup, documents ------------------------------------------------------------------------------------------------------------------
def test_find_class_by_name_resolves_the_model_in_both_roles_and_the_loss(flags):
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    cls = train.find_class_by_name("MoeSoftmaxModel", [flm, vlm])           # --model
    assert cls is vlm.MoeSoftmaxModel and not hasattr(flm, "MoeSoftmaxModel")
    flags.video_level_classifier_model = "MoeSoftmaxModel"                  # --video_level_classifier_model
    assert flm._head() is cls
    loss = train.find_class_by_name("SplitSoftmaxLoss", [losses])           # --label_loss
    assert loss is losses.SplitSoftmaxLoss and issubclass(loss, losses.BaseLoss)
    assert flags.softmax_bound == 1000 and flags.moe_layers == 1 and flags.class_size == 200


def test_documents_say_where_the_model_is_built_and_what_is_left():
    src = open(os.path.join(ROOT, "youtube-8m_amd", "frame_level_models.py")).read()
    line = re.search(r"^#   .*MoeSoftmaxModel.*\n#   .*\n#   .*", src, re.M).group(0)       # the entry and its two continuation lines
    assert "video_level_models" in line and "channels" in line and "W's SoftmaxLoss" in line and "needs Z's SoftmaxLoss" not in src
    doc = __import__("yt8m_amd.losses", fromlist=["x"]).__doc__
    assert "SplitSoftmaxLoss" in doc and "the next step" not in doc and "tf.nn.softmax" in doc


# ---- the C ABI on the host ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_symbols():
    src, lib = declared_bound_exported(SYMBOLS, r"int(?:64_t)?")
    assert "Z/video_level_models.py:877-960" in src and "Z/losses.py:412-456" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved
    P, i64, f, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert L.SIGNATURES["yt8m_softmax_moe_fwd"] == (i, [P, P, P, P, P, i64, i64, i64, i64, P])
    assert L.SIGNATURES["yt8m_softmax_moe_bwd"] == (i, [P, P, P, P, i64, i64, P, P, i64, i64, i64, P])
    assert L.SIGNATURES["yt8m_split_softmax_loss_fwd_bwd"] == (i, [P, i64, i64, P, i, P, P, i64, i64, i64, f, f, f, P, P])
    assert L.SIGNATURES["yt8m_split_softmax_loss_bwd"] == (i, [P, i64, i64, P, i, P, P, i64, i64, i64, f, f, f, P])


def test_supported_states_the_kernels_limits_without_a_device():
    lib = L.lib()
    for S, M, ok in ((2, 1, 1), (1717, 4, 1), (3717, 4, 1), (1717, 8, 1), (65536, 8, 1), (65537, 4, 0), (1, 4, 0), (0, 4, 0), (-3, 4, 0),
                     (1717, 0, 0), (1717, 9, 0), (1717, -1, 0)):
        assert lib.yt8m_softmax_moe_supported(S, M) == ok, (S, M)
    # the register-resident threshold the header documents: S <= 256 * (36 / (M + 1)), integer division
    for M in range(1, 9):
        top = 256 * (36 // (M + 1))
        assert lib.yt8m_softmax_moe_resident(top, M) == 1 and lib.yt8m_softmax_moe_resident(top + 1, M) == 0, M
    assert lib.yt8m_softmax_moe_resident(1717, 4) == 1 and lib.yt8m_softmax_moe_resident(1792, 4) == 1
    assert lib.yt8m_softmax_moe_resident(1793, 4) == 0 and lib.yt8m_softmax_moe_resident(1, 4) == 0
    assert lib.yt8m_split_softmax_loss_workspace_bytes(1024) == 4096 and lib.yt8m_split_softmax_loss_workspace_bytes(0) == 0


def test_argument_validation_without_device():
    """Every call here fails validation: nothing is launched and no device is needed."""
    lib = L.lib()
    BADARG, SHAPE = -1, -2
    p = lambda k: ctypes.c_void_p(4096 * k)

    def fwd(Zg=p(1), Ze=p(2), head=p(3), out=p(4), stats=p(5), rows=3, S=28, M=3, V1=10):
        return lib.yt8m_softmax_moe_fwd(Zg, Ze, head, out, stats, rows, S, M, V1, None)

    def bwd(Zg=p(1), Ze=p(2), stats=p(3), dout=p(4), ldd=37, c0=10, dZg=p(5), dZe=p(6), rows=3, S=28, M=3):
        return lib.yt8m_softmax_moe_bwd(Zg, Ze, stats, dout, ldd, c0, dZg, dZe, rows, S, M, None)

    for name in ("Zg", "Ze", "out", "stats"):
        assert fwd(**{name: None}) == BADARG, name
    assert fwd(head=None) == BADARG and fwd(V1=0) == BADARG                # the head goes with V1 > 0 and only with it
    assert fwd(rows=0) == SHAPE and fwd(rows=-2) == SHAPE and fwd(S=1) == SHAPE and fwd(S=65537) == SHAPE
    assert fwd(M=0) == SHAPE and fwd(M=9) == SHAPE and fwd(V1=-1) == SHAPE and fwd(V1=(1 << 24) + 1) == SHAPE
    for name in ("Zg", "Ze", "stats", "dout", "dZg", "dZe"):
        assert bwd(**{name: None}) == BADARG, name
    assert bwd(c0=-1) == BADARG and bwd(ldd=36) == BADARG and bwd(ldd=26, c0=0) == BADARG
    assert bwd(rows=0) == SHAPE and bwd(S=1) == SHAPE and bwd(M=9) == SHAPE
    assert b"softmax_moe" in lib.yt8m_last_error()

    def loss(pp=p(1), ldp=37, c0=0, labels=p(2), dt=0, out=p(3), dp=p(4), B=3, V=37, bound=10, e1=1e-5, e2=1e-7, ws=p(5)):
        return lib.yt8m_split_softmax_loss_fwd_bwd(pp, ldp, c0, labels, dt, out, dp, B, V, bound, e1, e2, 1.0, ws, None)

    def back(pp=p(1), ldp=37, c0=0, labels=p(2), dt=0, up=p(3), dp=p(4), B=3, V=37, bound=10, e1=1e-5, e2=1e-7):
        return lib.yt8m_split_softmax_loss_bwd(pp, ldp, c0, labels, dt, up, dp, B, V, bound, e1, e2, 1.0, None)

    for name in ("pp", "labels", "out", "ws"):
        assert loss(**{name: None}) == BADARG, name
    assert loss(dt=2) == BADARG and loss(c0=-1) == BADARG and loss(ldp=36) == BADARG and loss(ldp=40, c0=4) == BADARG
    assert loss(e1=0.0) == BADARG and loss(e2=0.0) == BADARG
    assert loss(B=0) == SHAPE and loss(V=1, bound=1) == SHAPE and loss(bound=0) == SHAPE and loss(bound=37) == SHAPE and loss(bound=-1) == SHAPE
    for name in ("pp", "labels", "dp"):
        assert back(**{name: None}) == BADARG, name
    assert back(dt=-1) == BADARG and back(ldp=36) == BADARG and back(B=0) == SHAPE and back(bound=37) == SHAPE
    assert b"split_softmax_loss" in lib.yt8m_last_error()


def test_the_default_forms_follow_the_environment_variables():
    import yt8m_amd.ops as ops
    src = open(os.path.join(ROOT, "youtube-8m_amd", "ops.py")).read()
    for flag, var in ((ops.SOFTMAX_MOE_FUSED, "YT8M_SOFTMAX_MOE_FUSED"), (ops.SPLIT_SOFTMAX_LOSS_FUSED, "YT8M_SPLIT_SOFTMAX_LOSS_FUSED")):
        default = re.search(r'os\.environ\.get\("%s", "([01])"\)' % var, src).group(1)
        assert flag is (os.environ.get(var, default) != "0"), var
    assert ops.SOFTMAX_LOSS_EPS == 10e-8 and ops.XENT_EPS == 10e-6


# ---- the composed forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,S,M,V1", [(1, 2, 1, 0), (3, 7, 2, 1), (4, 28, 3, 10)])
def test_composed_softmax_moe_is_the_restatement_in_float64(monkeypatch, rows, S, M, V1):
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "SOFTMAX_MOE_FUSED", True)                   # CPU and float64 tensors take the composed form even then
    rs = np.random.RandomState(rows + S)
    Zg, Ze = 2 * rs.randn(rows, S * (M + 1)), 2 * rs.randn(rows, S * M)
    head = rs.rand(rows, V1) if V1 else None
    dout = rs.randn(rows, V1 + S - 1)
    zg, ze = torch.from_numpy(Zg).requires_grad_(True), torch.from_numpy(Ze).requires_grad_(True)
    h = torch.from_numpy(head).requires_grad_(True) if V1 else None
    before = dict(ops.SOFTMAX_MOE_CALLS)
    out = ops.softmax_moe(zg, ze, S, M, head=h)
    assert ops.SOFTMAX_MOE_CALLS == dict(before, composed=before["composed"] + 1)
    out.backward(torch.from_numpy(dout))
    ref = R.kernel_with_grads(Zg, Ze, head, S, M, dout, torch.float64)
    got = {"out": out.detach(), "dZg": zg.grad, "dZe": ze.grad}
    if V1:
        got["dhead"] = h.grad
    for k, v in got.items():
        assert R.err(v, ref[k].numpy()) < 1e-14, k
    assert tuple(out.shape) == (rows, V1 + S - 1)
    q = out.detach()[:, V1:]
    assert bool((q.sum(1) < 1).all()) and bool((q > 0).all())            # the dropped label holds the rest
    # the issue's closed forms for the backward pass, in float64
    g = torch.softmax(zg.detach().view(rows, S, M + 1), 2)
    e = torch.softmax(ze.detach().view(rows, S, M), 1)
    w = g[:, :, :M] * e
    p = w.sum(2)
    T = p.sum(1, keepdim=True)
    dq = torch.cat((torch.from_numpy(dout)[:, V1:], torch.zeros(rows, 1, dtype=torch.float64)), 1)
    Dd = (dq * p / T).sum(1, keepdim=True)
    dp = (dq - Dd) / T
    A, Cm = (w * dq[:, :, None]).sum(1), w.sum(1)
    dZe = e * (g[:, :, :M] * dp[:, :, None] - ((A - Dd * Cm) / T)[:, None, :])
    e1 = torch.cat((e, torch.zeros(rows, S, 1, dtype=torch.float64)), 2)
    dZg = g * dp[:, :, None] * (e1 - p[:, :, None])
    assert R.err(dZe.reshape(rows, -1), ref["dZe"].numpy()) < 1e-14 and R.err(dZg.reshape(rows, -1), ref["dZg"].numpy()) < 1e-14
    for bad in (dict(S=S + 1), dict(M=M + 1), dict(S=1)):
        with pytest.raises(ValueError, match="softmax_moe"):
            ops.softmax_moe(zg, ze, **dict(dict(S=S, M=M), **bad))
    with pytest.raises(ValueError, match="softmax_moe"):
        ops.softmax_moe(zg, ze, S, M, head=torch.zeros(rows + 1, 3, dtype=torch.float64))


@pytest.mark.parametrize("dtype", [np.bool_, np.uint8, np.float32, np.float64])
def test_composed_split_softmax_loss_is_the_restatement_in_float64(monkeypatch, dtype):
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "SPLIT_SOFTMAX_LOSS_FUSED", True)
    rs = np.random.RandomState(5)
    p = rs.rand(B_, V_)
    p[:, V1_:] *= 0.9 / p[:, V1_:].sum(1, keepdims=True)
    y = (rs.rand(B_, V_) < 0.2)
    y[0, V1_:] = False                                                     # a row without infrequent labels
    y[1] = False                                                           # a row with no labels at all
    y = y.astype(dtype)
    pt = torch.from_numpy(p).requires_grad_(True)
    before = dict(ops.SPLIT_SOFTMAX_LOSS_CALLS)
    loss = ops.split_softmax_loss(pt, torch.from_numpy(y), V1_, scale=0.1)
    assert ops.SPLIT_SOFTMAX_LOSS_CALLS == dict(before, composed=before["composed"] + 1)
    loss.backward()
    ref = R.loss_with_grads(p, y, V1_, torch.float64, scale=0.1)
    assert abs(float(loss.detach()) - float(ref["loss"])) < 1e-13 * abs(float(ref["loss"])) and R.err(pt.grad, ref["dp"].numpy()) < 1e-13
    clamped = R.loss_with_grads(p, y, V1_, torch.float64, clamp=True, scale=0.1)       # the clamp is idle where 1 - sum >= 0
    assert float(clamped["loss"]) == float(ref["loss"]) and torch.equal(clamped["dp"], ref["dp"])
    for bound in (0, V_, -1):
        with pytest.raises(ValueError, match="bound"):
            ops.split_softmax_loss(pt, torch.from_numpy(y), bound)
    with pytest.raises(ValueError, match="split_softmax_loss"):
        ops.split_softmax_loss(pt, torch.from_numpy(y)[:, :-1], V1_)


def test_the_appended_probability_is_clamped_and_the_loss_stays_finite(flags):
    """A row whose float32 sum over the softmax part is 1 + 2^-23: the reference's 1 - sum + 10e-8 is negative and its log NaN; here
    the appended probability is 0, the loss finite and the gradient that of the unclamped value."""
    import yt8m_amd.losses as losses
    import yt8m_amd.video_level_models  # noqa: F401
    flags.softmax_bound = 3
    p = np.zeros((2, 8), dtype=np.float32)
    p[:, :3] = 0.3
    p[0, 3:5] = np.float32(0.5), np.float32(0.5) + np.float32(2.0 ** -23)
    p[1, 3:] = 0.1
    y = np.zeros((2, 8), dtype=bool)
    y[0, 4] = y[1, 5] = True
    pt = torch.from_numpy(p).requires_grad_(True)
    assert float(pt.detach()[0, 3:].sum()) == 1.0 + 2.0 ** -23 and float(1 - pt.detach()[0, 3:].sum()) < -10e-8
    assert not np.isfinite(float(R.softmax_loss(torch.from_numpy(p), torch.from_numpy(y), 3)))             # the reference's formula
    loss = losses.SplitSoftmaxLoss().calculate_loss(pt, torch.from_numpy(y))
    loss.backward()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pt.grad).all())
    ref = R.loss_with_grads(p, y, 3, torch.float32, clamp=True)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-6 * abs(float(ref["loss"])) and R.err(pt.grad, ref["dp"].numpy()) < 1e-6
    # as if unclamped: every column of the softmax part carries the appended term's d o / d p = -1 at o = 0
    n_app, eps = 0.0, np.float32(10e-8)
    ga = n_app / (0 + eps) - (1 - n_app) / (1 - 0 + eps)
    assert abs(float(pt.grad[0, 7]) - 0.5 * (ga + 1.0 / (1.0 + eps))) < 1e-6                # a zero-probability negative: ga - (-(1 / (1 + eps)))


# ---- the device-only ops as their torch meaning -------------------------------------------------------------------------------------------
def _cpu_ops(monkeypatch):
    """(gradients reach the arena through ops.as_tensor)"""
    import yt8m_amd.ops as ops
    t = ops.as_tensor
    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: x @ t(W) if b is None else x @ t(W) + t(b))
    monkeypatch.setattr(ops, "activation", lambda x, kind: {"elu": R.elu}[kind](x))
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: R.l2_normalize(x, eps))
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V, M, **k: R.moe(x, t(Wg), t(We), t(be), M))


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


def _case(seed):
    rs = np.random.RandomState(seed)
    return rs, rs.randn(B_, D_).astype(np.float32), rs.rand(B_, V_) < 0.2


def _set(flags, layers, bound=V1_):
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags set below)
    import yt8m_amd.train  # noqa: F401
    flags.moe_num_mixtures, flags.class_size, flags.moe_layers, flags.softmax_bound = M_, C_, layers, bound


# ---- the model on the CPU graph ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", LAYERS)
def test_variable_names_shapes_order_and_l2(monkeypatch, flags, layers):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, layers)
    _, x, _ = _case(1)
    g = _graph()
    res = vlm.MoeSoftmaxModel().create_model(torch.from_numpy(x), vocab_size=V_, unknown_kwarg=1, labels=None, num_frames=None)
    assert tuple(res["predictions"].shape) == (B_, V_) and tuple(res["predictions_class"].shape) == (B_, max(layers, 1) * V_)
    if layers == 0:
        assert res["predictions_class"] is res["predictions"]
    want = R.variable_shapes(D_, V_, V1_, M_, C_, layers)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(want.items())                     # names, shapes, creation order
    S = V_ - V1_ + 1
    assert list(want.items())[:6] == [("gatespre/weights", (D_, V1_ * (M_ + 1))), ("expertspre/weights", (D_, V1_ * M_)),
                                      ("expertspre/biases", (V1_ * M_,)), ("class_gates-0pre/weights", (D_, S * (M_ + 1))),
                                      ("class_experts-0pre/weights", (D_, S * M_)), ("class_experts-0pre/biases", (S * M_,))]
    if layers:
        assert list(want)[6:16] == ["class_inputs1-0/weights", "class_inputs1-0/biases", "class_inputs2-0/weights", "class_inputs2-0/biases",
                                    "gates-0/weights", "experts-0/weights", "experts-0/biases", "class_gates-0-0/weights",
                                    "class_experts-0-0/weights", "class_experts-0-0/biases"]
        assert want["class_gates-0-%d/weights" % (layers - 1)] == (D_ + 2 * C_ * layers, S * (M_ + 1))
    assert len(want) == 6 + 10 * layers and not any("gates" in k and k.endswith("/biases") for k in g.vars)
    for k, v in g.vars.items():
        assert v.trainable and v.l2 == (1e-8 if k.endswith("/weights") else 0.0), k
        if k.endswith("/biases"):
            assert bool((v.data == 0).all()), k
        else:                                                             # slim.fully_connected weights: xavier
            lim = np.sqrt(6.0 / (v.data.shape[0] + v.data.shape[1]))
            assert float(v.data.abs().max()) <= lim and float(v.data.abs().max()) > 0.8 * lim, k


def _run_model(x, y, P, layers, loss_name):
    import yt8m_amd.losses as losses
    import yt8m_amd.video_level_models as vlm
    model = vlm.MoeSoftmaxModel()
    g = _graph()
    g.begin_step()
    model.create_model(torch.from_numpy(x), vocab_size=V_)
    g.finalize()
    assert list(g.vars) == list(P)
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v))
    g.begin_step()
    xt = torch.from_numpy(x).requires_grad_(True)
    res = model.create_model(xt, vocab_size=V_)
    if loss_name == "CrossEntropyLoss":                                   # device code: the restatement's rule stands for it
        loss = R.mix_loss(res["predictions"], res["predictions_class"], torch.from_numpy(y), layers)
    else:
        loss = losses.SplitSoftmaxLoss().calculate_loss_mix(res["predictions"], res["predictions_class"], torch.from_numpy(y))
    loss.backward()
    return res, loss.detach(), {k: v.grad.detach().clone() for k, v in g.vars.items()}, xt.grad


def _check(tag, got, r64, r32):
    """ensemble_restatement.bound: four times the float32 restatement's own error plus one float32 ulp of the largest reference
    magnitude."""
    for k in got:
        assert bool(torch.isfinite(r32[k]).all()), k
        e = float((got[k].double() - r64[k]).abs().max())
        b = R.bound(r32[k], r64[k])
        print("%s %s: error %.3g, float32 restatement %.3g, bound %.3g" % (tag, k, e, float((r32[k].double() - r64[k]).abs().max()), b))
        assert e <= b, (tag, k, e, b)


@pytest.mark.parametrize("loss_name", ["CrossEntropyLoss", "SplitSoftmaxLoss"])
@pytest.mark.parametrize("layers", LAYERS)
def test_model_matches_the_float64_restatement(monkeypatch, flags, layers, loss_name):
    """--model=MoeSoftmaxModel: predictions, predictions_class, the training loss under either --label_loss, the gradient of every
    variable and of x."""
    import yt8m_amd.ops as ops
    _cpu_ops(monkeypatch)
    _set(flags, layers)
    rs, x, y = _case(11 + 10 * layers)
    P = R.draw(R.variable_shapes(D_, V_, V1_, M_, C_, layers), rs)
    before = dict(ops.SOFTMAX_MOE_CALLS), dict(ops.SPLIT_SOFTMAX_LOSS_CALLS)
    res, loss, grads, dx = _run_model(x, y, P, layers, loss_name)
    assert ops.SOFTMAX_MOE_CALLS == dict(before[0], composed=before[0]["composed"] + 2 * (layers + 1))
    n_loss = (layers + 1) if loss_name == "SplitSoftmaxLoss" else 0
    assert ops.SPLIT_SOFTMAX_LOSS_CALLS == dict(before[1], composed=before[1]["composed"] + n_loss)
    r64 = R.reference(x, y, P, M_, C_, layers, V1_, torch.float64, loss_name)
    r32 = R.reference(x, y, P, M_, C_, layers, V1_, torch.float32, loss_name)
    got = {"predictions": res["predictions"].detach(), "predictions_class": res["predictions_class"].detach(), "loss": loss, "dx": dx}
    _check(loss_name, got, r64, r32)
    assert set(grads) == set(r64["grads"])
    _check(loss_name + " gradient of", grads, r64["grads"], r32["grads"])
    used = [k for k in grads if float(r64["grads"][k].abs().max()) > 0]
    assert len(used) == len(grads) and all(float(grads[k].abs().max()) > 0 for k in used)
    # the prediction row: the sigmoid part in front, a sub-distribution behind it
    p = r64["predictions"]
    assert bool((p[:, V1_:].sum(1) < 1).all()) and bool((p > 0).all())
    if layers:                                                            # the split loss is not the tiled cross entropy
        other = R.reference(x, y, P, M_, C_, layers, V1_, torch.float64, "SplitSoftmaxLoss" if loss_name == "CrossEntropyLoss" else "CrossEntropyLoss")
        assert abs(float(other["loss"]) - float(r64["loss"])) > 1e-3


def test_softmax_bound_is_asserted(monkeypatch, flags):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _, x, _ = _case(2)
    for bound in (0, V_, V_ + 5, -1):
        _set(flags, 1, bound=bound)
        g = _graph()
        with pytest.raises(AssertionError, match="softmax_bound"):
            vlm.MoeSoftmaxModel().create_model(torch.from_numpy(x), vocab_size=V_)
        assert not g.vars
    _set(flags, 0, bound=V_ - 1)                                          # one infrequent label: S = 2
    _graph()
    assert tuple(vlm.MoeSoftmaxModel().create_model(torch.from_numpy(x), vocab_size=V_)["predictions"].shape) == (B_, V_)


# ---- the loss class and the training rule ---------------------------------------------------------------------------------------------------
def test_split_softmax_loss_refuses_weights_and_ignores_label_smoothing(flags):
    import yt8m_amd.losses as losses
    _set(flags, 1)
    rs = np.random.RandomState(0)
    p, y = torch.from_numpy(rs.rand(B_, V_) / V_), torch.from_numpy(rs.rand(B_, V_) < 0.2)
    fn = losses.SplitSoftmaxLoss()
    with pytest.raises(ValueError, match="weights"):
        fn.calculate_loss(p, y, weights=torch.ones(B_))
    with pytest.raises(ValueError, match="weights"):
        fn.calculate_loss_mix(p, p, y, weights=torch.ones(B_))
    plain = float(fn.calculate_loss(p, y))
    assert plain == float(R.softmax_loss(p, y, V1_))
    flags.label_smoothing = True
    assert float(fn.calculate_loss(p, y)) == plain
    with pytest.raises(ValueError, match="moe_layers"):
        flags.moe_layers = 2
        fn.calculate_loss_mix(p, p, y)


class _CE(object):
    """Stands for --label_loss=CrossEntropyLoss (device code): the restatement's cross entropy; it has no calculate_loss_mix."""

    def calculate_loss(self, predictions, labels, weights=None, **unused_params):
        return R.cross_entropy(predictions, labels)


def _tg(label_loss_fn, **kw):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.train as train
    return train.TrainGraph(None, label_loss_fn=label_loss_fn, batch_size=B_, graph=_graph(), transformer_class=ft.IdenticalTransformer, **kw)


@pytest.mark.parametrize("layers", [1, 3])
def test_mix_loss_hands_over_to_calculate_loss_mix_where_the_loss_has_one(flags, layers):
    import yt8m_amd.losses as losses
    _set(flags, layers)
    rs = np.random.RandomState(layers)
    p, pc = rs.rand(B_, V_) / V_, rs.rand(B_, layers * V_) / V_
    y = torch.from_numpy(rs.rand(B_, V_) < 0.2)
    pt, pct = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(pc).requires_grad_(True)
    fn = losses.SplitSoftmaxLoss()
    calls = []
    real = fn.calculate_loss_mix
    fn.calculate_loss_mix = lambda *a, **k: calls.append((len(a), sorted(k))) or real(*a, **k)
    loss = _tg(fn).loss({"predictions": pt, "predictions_class": pct}, y)
    assert calls == [(3, ["weights"])]
    loss.backward()
    rp, rpc = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(pc).requires_grad_(True)
    ref = R.softmax_loss_mix(rp, rpc, y, V1_, layers)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    assert R.err(pt.grad, rp.grad.numpy()) < 1e-13 and R.err(pct.grad, rpc.grad.numpy()) < 1e-13
    # NOT calculate_loss on the [B, L V] tensor against tiled labels: the bound splits every piece
    tiled = R.softmax_loss(pt.detach(), y, V1_) + 0.1 * R.softmax_loss(pct.detach(), y.repeat(1, layers), V1_)
    same = abs(float(tiled) - float(ref.detach())) <= 1e-3                # (the tiled form's appended probability may be negative: NaN)
    assert same == (layers == 1)                                          # one piece: the two are the same function
    # the rule's own checks come first
    with pytest.raises(ValueError, match="not a whole multiple"):
        _tg(fn).loss({"predictions": pt, "predictions_class": pct[:, :-1]}, y)
    with pytest.raises(ValueError, match="--multitask"):
        _tg(fn, multitask=True).loss({"predictions": pt, "predictions_class": pct, "support_predictions": pt}, y)
    # a loss without calculate_loss_mix keeps the tiled path
    ce = _tg(_CE()).loss({"predictions": pt.detach(), "predictions_class": pct.detach()}, y)
    assert float(ce) == float(R.mix_loss(pt.detach(), pct.detach(), y, layers))
    import yt8m_amd.losses as losses_mod
    assert not hasattr(losses_mod.CrossEntropyLoss, "calculate_loss_mix")


def test_training_step_under_split_softmax_loss_moves_the_variables(monkeypatch, flags):
    """One whole TrainGraph.step; a plain gradient step on the arenas stands for the device's clip + Adam pass, as in
    tests/test_mix_chain_host.py."""
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.ops as ops
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 2)
    calls = []

    def sgd(graph, lr_t, tensors=None, **k):
        calls.append(tensors)
        for v in graph.trainable_variables()[tensors[0]:tensors[1]]:
            v.data.sub_(lr_t * v.grad)

    monkeypatch.setattr(ops, "sqnorm_and_adam", sgd)
    _, x, y = _case(9)
    tg = train.TrainGraph(vlm.MoeSoftmaxModel(), label_loss_fn=losses.SplitSoftmaxLoss(), batch_size=B_, graph=_graph(),
                          transformer_class=ft.IdenticalTransformer)
    out = tg.step(torch.from_numpy(x), torch.from_numpy(y))
    assert calls == [(0, 26)]
    start = {k: v.data.clone() for k, v in tg.graph.vars.items()}
    out2 = tg.step(torch.from_numpy(x), torch.from_numpy(y))
    for k, v in tg.graph.vars.items():
        assert v.grad_written and float(v.grad.abs().max()) > 0 and not torch.equal(v.data, start[k]), k
    assert tuple(out["predictions"].shape) == (B_, V_) and float(out2["loss"]) < float(out["loss"])
