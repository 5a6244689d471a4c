"""CPU checks of Z's combine chain heads (MoeMix4Model, MoeKnowledgeModel: Z/video_level_models.py:1872-2044, :1331-1438), of
LstmExtendCombineModel's tail, of the mix loss rule (Z/train.py:318-349, Z/losses.py:280-313), of the composed form of ops.mix_link and
of the C ABI of csrc/mix_link.hip without a device: the lookup by name, the flags, every Variable's name, shape, creation order and l2,
predictions, predictions_class, loss and every gradient against the float64 restatement (tests/mix_chain_restatement.py) at
--moe_layers 1, 2 and 3, the --frame_features form, the --class_file head, the rule's value, gradients and errors, a training step, and
the symbols' signatures and argument validation.

The heads run here on the CPU graph with the device-only ops replaced by their torch meaning on the Variables (ops.linear,
ops.activation, ops.l2_normalize, ops.moe_head, ops.frame_pool: _cpu_ops); the heads, the composed form of ops.mix_link (which is what CPU
tensors take) and the training rule are the product's own code.  Shape: B = 5, D = 36, V = 37, 3 mixtures, --class_size=7."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mix_chain_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_mix_link_supported", "yt8m_mix_link_fwd", "yt8m_mix_link_bwd")
B_, D_, V_, M_, C_, K_ = 5, 36, 37, 3, 7, 6
LAYERS = [1, 2, 3]


# ---- lookup, flags, documents ---------------------------------------------------------------------------------------------------------
def test_find_class_by_name_resolves_the_three_classes(flags):
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in R.HEADS:
        cls = train.find_class_by_name(name, [flm, vlm])                   # --model
        assert cls is getattr(vlm, name) and not hasattr(flm, name)
        flags.video_level_classifier_model = name                         # --video_level_classifier_model
        assert flm._head() is cls
    cls = train.find_class_by_name("LstmExtendCombineModel", [flm, vlm])
    assert cls is flm.LstmExtendCombineModel and issubclass(cls, flm.LstmExtendModel) and cls.accepts_quantized_input


def test_flag_defaults_follow_the_reference(flags):
    import yt8m_amd.video_level_models  # noqa: F401  (defines the flags)
    assert flags.moe_layers == 1 and flags.class_size == 200 and flags.moe_group is False
    assert flags.class_file == "./resources/labels_knowledge.out"


def test_not_built_list_names_what_is_left():
    src = open(os.path.join(ROOT, "youtube-8m_amd", "frame_level_models.py")).read()
    assert not re.search(r"^#   LstmExtendCombineModel", src, re.M) and "a training rule that\n#   train.py does not have" not in src
    for name in ("CnnDCCDistillChainModel", "MoeSoftmaxModel", "moe_group"):
        assert re.search(r"^#   .*%s" % re.escape(name), src, re.M), name
    losses_src = open(os.path.join(ROOT, "youtube-8m_amd", "losses.py")).read()
    assert "calculate_loss_mix2" in losses_src and "--support_type" in losses_src


# ---- the C ABI on the host ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_symbols():
    src, lib = declared_bound_exported(SYMBOLS)
    assert "Z/video_level_models.py:1872-2044" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits_without_a_device():
    lib = L.lib()
    for Wprev, C, ok in ((1, 1, 1), (1152, 100, 1), (1752, 256, 1), (37, 37, 1), (1 << 24, 1024, 1), (1024, 1024, 1), (1024, 1025, 0),
                         (0, 100, 0), (1152, 0, 0), (-1, 100, 0), (1152, -4, 0), ((1 << 24) + 1, 100, 0)):
        assert lib.yt8m_mix_link_supported(Wprev, C) == ok, (Wprev, C)


def test_argument_validation_without_device():
    """Every call here fails validation: nothing is launched and no device is needed."""
    lib = L.lib()
    BADARG, SHAPE = -1, -2
    p = lambda k: ctypes.c_void_p(4096 * k)

    def fwd(mode=0, prev=p(1), z=p(2), u=p(3), out=p(4), stats=p(5), rows=3, Wprev=36, C=8, scale=0.5, eps=1e-12):
        return lib.yt8m_mix_link_fwd(mode, prev, z, u, out, stats, rows, Wprev, C, scale, eps, None)

    def bwd(mode=0, z=p(1), u=p(2), stats=p(3), dy=p(4), dprev=p(5), dz=p(6), rows=3, Wprev=36, C=8, dx_from=0, scale=0.5):
        return lib.yt8m_mix_link_bwd(mode, z, u, stats, dy, dprev, dz, rows, Wprev, C, dx_from, scale, None)

    assert fwd(mode=4) == BADARG and fwd(mode=-1) == BADARG and fwd(eps=0.0) == BADARG and fwd(scale=0.0) == BADARG
    for name in ("prev", "z", "u", "out", "stats"):
        assert fwd(**{name: None}) == BADARG, name
    assert fwd(rows=0) == SHAPE and fwd(rows=-2) == SHAPE and fwd(Wprev=0) == SHAPE and fwd(C=0) == SHAPE and fwd(C=1025) == SHAPE
    assert bwd(mode=4) == BADARG and bwd(dx_from=-1) == BADARG and bwd(dx_from=37) == BADARG and bwd(scale=-1.0) == BADARG
    for name in ("z", "u", "stats", "dy", "dz"):
        assert bwd(**{name: None}) == BADARG, name
    assert bwd(rows=0) == SHAPE and bwd(Wprev=0) == SHAPE and bwd(C=0) == SHAPE and bwd(C=1025) == SHAPE
    assert b"mix_link" in lib.yt8m_last_error()


def test_the_default_form_follows_the_environment_variable():
    import yt8m_amd.ops as ops
    assert ops.MIX_LINK_FUSED is (os.environ.get("YT8M_MIX_LINK_FUSED", "1") != "0")
    assert ops.MIX_LINK_FUSED_Q is (os.environ.get("YT8M_MIX_LINK_FUSED_Q", "0") != "0")
    assert (ops.MIX_LINK_PLAIN, ops.MIX_LINK_NONE) == (1, 2)
    src = open(os.path.join(ROOT, "include", "yt8m_hip.h")).read()
    assert "YT8M_MIX_LINK_PLAIN = 1, YT8M_MIX_LINK_NONE = 2" in src


# ---- the device-only ops as their torch meaning -------------------------------------------------------------------------------------------
def _cpu_ops(monkeypatch):
    """(gradients reach the arena through ops.as_tensor)"""
    import yt8m_amd.ops as ops
    t = ops.as_tensor
    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: x @ t(W) if b is None else x @ t(W) + t(b))
    monkeypatch.setattr(ops, "activation", lambda x, kind: {"elu": R.elu}[kind](x))
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: R.l2_normalize(x, eps))
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V, M, **k: R.moe(x, t(Wg), t(We), t(be), M))
    monkeypatch.setattr(ops, "frame_pool", lambda x, method: {"max": x.max(dim=1)[0]}[method])


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


def _case(seed, B=B_, D=D_):
    rs = np.random.RandomState(seed)
    x = rs.randn(B, D).astype(np.float32)
    y = rs.rand(B, V_) < 0.2
    return rs, x, y


def _set(flags, layers, frame_features=False):
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags set below)
    import yt8m_amd.train  # noqa: F401  (--frame_features)
    flags.moe_num_mixtures, flags.class_size, flags.moe_layers, flags.frame_features = M_, C_, layers, frame_features


def _class_file(tmp_path, flags, rs):
    seq = (rs.rand(V_, K_) < 0.3).astype(np.float64) + rs.rand(V_, K_) * 0.1
    path = str(tmp_path / "labels_knowledge.out")
    np.savetxt(path, seq)
    flags.class_file = path
    return np.loadtxt(path).astype(np.float32)


# ---- ops.mix_link, composed -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knowledge", [False, True])
@pytest.mark.parametrize("norm", [True, False])
def test_composed_mix_link_is_the_restatement_in_float64(monkeypatch, knowledge, norm):
    import yt8m_amd.ops as ops
    _cpu_ops(monkeypatch)
    monkeypatch.setattr(ops, "MIX_LINK_FUSED", True)                      # CPU and float64 tensors take the composed form even then
    monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", True)
    g = _graph()
    rs = np.random.RandomState(3)
    rows, Wprev, V, C, K = 4, 6, 11, 5, 3
    prev, p, dy = rs.randn(rows, Wprev), rs.rand(rows, V), rs.randn(rows, Wprev + 2 * C)
    q = rs.rand(rows, K) if knowledge else None
    P = {"W1": rs.randn(V, C), "b1": rs.randn(C), "W2": rs.randn(K if knowledge else V, C), "b2": rs.randn(C)}
    from yt8m_amd.variables import zeros
    vs = {k: g.get_variable(k, v.shape, zeros) for k, v in P.items()}
    g.finalize()
    for k, v in P.items():
        vs[k].data = torch.from_numpy(v)                                  # float64 parameters for this check
        vs[k].grad = torch.zeros_like(vs[k].data)
    scale = float(R.link_scale(C, Wprev))
    pt, xt = torch.from_numpy(prev).requires_grad_(True), torch.from_numpy(p).requires_grad_(True)
    qt = None if q is None else torch.from_numpy(q).requires_grad_(True)
    before = dict(ops.MIX_LINK_CALLS)
    out = ops.mix_link(pt, xt, vs["W1"], vs["b1"], vs["W2"], vs["b2"], q=qt, norm=norm, scale=scale)
    assert ops.MIX_LINK_CALLS["composed"] == before["composed"] + 1 and ops.MIX_LINK_CALLS["kernels"] == before["kernels"]
    out.backward(torch.from_numpy(dy))
    ref = R.link_with_grads(prev, p, q, P["W1"], P["b1"], P["W2"], P["b2"], scale if norm else None, dy, torch.float64)
    got = {"out": out, "dprev": pt.grad, "dp": xt.grad, "dW1": vs["W1"].grad, "db1": vs["b1"].grad, "dW2": vs["W2"].grad, "db2": vs["b2"].grad}
    if knowledge:
        got["dq"] = qt.grad
    for k, v in got.items():
        assert R.err(v, ref[k].numpy()) < 1e-12, k
    with pytest.raises(ValueError):
        ops.mix_link(pt, xt[:3], vs["W1"], vs["b1"], vs["W2"], vs["b2"], q=qt)
    with pytest.raises(ValueError):
        ops.mix_link(pt, xt, vs["W1"], vs["b1"], vs["W2"], vs["b2"], q=qt, dx_from=Wprev + 1)
    with pytest.raises(ValueError):
        ops.mix_link(pt, xt[:, :5], vs["W1"], vs["b1"], vs["W2"], vs["b2"], q=qt)


# ---- the heads on the CPU graph ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", LAYERS)
@pytest.mark.parametrize("name", R.HEADS)
def test_variable_names_shapes_order_and_l2(monkeypatch, flags, tmp_path, name, layers):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, layers)
    rs, x, _ = _case(1)
    _class_file(tmp_path, flags, rs)
    g = _graph()
    res = getattr(vlm, name)().create_model(torch.from_numpy(x), vocab_size=V_, unknown_kwarg=1, labels=None, num_frames=None)
    assert tuple(res["predictions"].shape) == (B_, V_) and tuple(res["predictions_class"].shape) == (B_, layers * V_)
    want = R.variable_shapes(name, D_, V_, M_, C_, layers, K_)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(want.items())                     # names, shapes, creation order
    assert list(want)[:3] == ["gates/weights", "experts/weights", "experts/biases"]
    assert list(want)[3:10] == ["class_inputs1-0/weights", "class_inputs1-0/biases", "class_inputs2-0/weights", "class_inputs2-0/biases",
                                "gates-0/weights", "experts-0/weights", "experts-0/biases"]
    assert want["gates-%d/weights" % (layers - 1)] == (D_ + 2 * C_ * layers, V_ * (M_ + 1))
    assert not any(k.startswith("gates") and k.endswith("/biases") for k in g.vars)
    for k, v in g.vars.items():
        assert v.trainable and v.l2 == (1e-8 if k.endswith("/weights") else 0.0), k
        if k.endswith("/biases"):
            assert bool((v.data == 0).all()), k
        else:                                                             # slim.fully_connected weights: xavier
            lim = np.sqrt(6.0 / (v.data.shape[0] + v.data.shape[1]))
            assert float(v.data.abs().max()) <= lim and float(v.data.abs().max()) > 0.8 * lim, k


def _run_head(model, x, y, P, layers, **kw):
    g = _graph()
    kw = dict(vocab_size=V_, **kw)
    g.begin_step()
    model.create_model(torch.from_numpy(x), **kw)
    g.finalize()
    assert list(g.vars) == list(P)
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v))
    g.begin_step()
    xt = torch.from_numpy(x).requires_grad_(True)
    res = model.create_model(xt, **kw)
    loss = R.mix_loss(res["predictions"], res["predictions_class"], torch.from_numpy(y), layers)
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


@pytest.mark.parametrize("frame_features", [False, True], ids=["norm", "frame_features"])
@pytest.mark.parametrize("layers", LAYERS)
@pytest.mark.parametrize("name", R.HEADS)
def test_head_as_model_matches_the_float64_restatement(monkeypatch, flags, tmp_path, name, layers, frame_features):
    """--model=<head>: predictions, predictions_class, the mix loss, the gradient of every variable and of x.  --frame_features leaves
    MoeMix4Model's class inputs unnormalised; MoeKnowledgeModel normalises them either way, as the reference does."""
    import yt8m_amd.ops as ops
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, layers, frame_features)
    rs, x, y = _case(7 + R.HEADS.index(name) + 10 * layers)
    seq = _class_file(tmp_path, flags, rs)
    P = R.draw(R.variable_shapes(name, D_, V_, M_, C_, layers, K_), rs)
    before = dict(ops.MIX_LINK_CALLS)
    res, loss, grads, dx = _run_head(getattr(vlm, name)(), x, y, P, layers)
    assert ops.MIX_LINK_CALLS["composed"] == before["composed"] + 2 * layers and ops.MIX_LINK_CALLS["kernels"] == before["kernels"]
    kw = dict(normalize=not frame_features, seq=seq if name == "MoeKnowledgeModel" else None)
    r64 = R.reference(name, x, y, P, M_, C_, layers, torch.float64, **kw)
    r32 = R.reference(name, x, y, P, M_, C_, layers, torch.float32, **kw)
    got = {"predictions": res["predictions"].detach(), "predictions_class": res["predictions_class"].detach(), "loss": loss, "dx": dx}
    _check(name, got, r64, r32)
    assert set(grads) == set(r64["grads"])
    _check(name + " gradient of", grads, r64["grads"], r32["grads"])
    for k in grads:
        assert float(grads[k].abs().max()) > 0, k
    if name == "MoeMix4Model":                                            # the two forms differ
        other = R.reference(name, x, y, P, M_, C_, layers, torch.float64, normalize=frame_features)
        assert R.err(other["predictions"], r64["predictions"].numpy()) > 1e-4


def test_zero_layers_returns_the_one_prediction_under_both_keys(monkeypatch, flags):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 0)
    g = _graph()
    _, x, _ = _case(2)
    res = vlm.MoeMix4Model().create_model(torch.from_numpy(x), vocab_size=V_)
    assert list(g.vars) == ["gates/weights", "experts/weights", "experts/biases"] and res["predictions_class"] is res["predictions"]


def test_knowledge_head_loads_its_class_file_once_and_checks_its_rows(monkeypatch, flags, tmp_path):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1)
    rs, x, _ = _case(3)
    seq = _class_file(tmp_path, flags, rs)
    loads = []
    real = np.loadtxt
    monkeypatch.setattr(np, "loadtxt", lambda *a, **k: loads.append(a) or real(*a, **k))
    for _ in range(2):
        _graph()
        vlm.MoeKnowledgeModel().create_model(torch.from_numpy(x), vocab_size=V_)
    assert len(loads) == 1
    cached = vlm._class_matrix(torch.device("cpu"))
    assert cached.dtype == torch.float32 and torch.equal(cached, torch.from_numpy(seq))
    _graph()
    with pytest.raises(ValueError, match="class_file"):
        vlm.MoeKnowledgeModel().create_model(torch.from_numpy(x), vocab_size=V_ + 1)


def test_moe_group_raises_not_implemented(monkeypatch, flags):
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 1)
    flags.moe_group = True
    g = _graph()
    _, x, _ = _case(2)
    with pytest.raises(NotImplementedError, match="no script of the final submission's list sets it"):
        vlm.MoeMix4Model().create_model(torch.from_numpy(x), vocab_size=V_)
    assert not g.vars


@pytest.mark.parametrize("layers", [1, 3])
def test_extend_combine_tail_matches_the_float64_restatement(monkeypatch, flags, layers):
    """LstmExtendCombineModel from the pooled rows on: MoeMix4Model under --frame_features on the B E rows, each stage's piece and the
    predictions reduced by the maximum over a video's E rows before the concatenation."""
    import yt8m_amd.ops as ops
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, layers, frame_features=True)
    E = 2
    rs, x, y = _case(40 + layers, B=B_ * E)
    y = y[:B_]
    P = R.draw(R.variable_shapes("MoeMix4Model", D_, V_, M_, C_, layers), rs)
    pool = lambda t: ops.frame_pool(t.view(-1, E, V_), "max")
    res, loss, grads, dx = _run_head(vlm.MoeMix4Model(), x, y, P, layers, support_pool=pool)
    assert tuple(res["predictions"].shape) == (B_, V_) and tuple(res["predictions_class"].shape) == (B_, layers * V_)
    r64 = R.reference("MoeMix4Model", x, y, P, M_, C_, layers, torch.float64, num_extend=E)
    r32 = R.reference("MoeMix4Model", x, y, P, M_, C_, layers, torch.float32, num_extend=E)
    got = {"predictions": res["predictions"].detach(), "predictions_class": res["predictions_class"].detach(), "loss": loss, "dx": dx}
    _check("extend combine tail", got, r64, r32)
    _check("extend combine tail gradient of", grads, r64["grads"], r32["grads"])


# ---- the training rule -----------------------------------------------------------------------------------------------------------------------
class _Loss(object):
    """Stands for --label_loss=CrossEntropyLoss (device code): the restatement's cross entropy."""

    def calculate_loss(self, predictions, labels, weights=None, **unused_params):
        return R.cross_entropy(predictions, labels)


def _tg(model=None, **kw):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.train as train
    return train.TrainGraph(model, label_loss_fn=_Loss(), batch_size=B_, graph=_graph(), transformer_class=ft.IdenticalTransformer, **kw)


@pytest.mark.parametrize("layers", LAYERS)
def test_mix_loss_rule_value_and_gradients(flags, layers):
    _set(flags, layers)
    rs = np.random.RandomState(layers)
    p, pc = rs.rand(B_, V_), rs.rand(B_, layers * V_)
    y = torch.from_numpy(rs.rand(B_, V_) < 0.2)
    pt, pct = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(pc).requires_grad_(True)
    tg = _tg()
    loss = tg.loss({"predictions": pt, "predictions_class": pct}, y)
    loss.backward()
    rp, rpc = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(pc).requires_grad_(True)
    ref = R.mix_loss(rp, rpc, y, layers)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    assert R.err(pt.grad, rp.grad.numpy()) < 1e-14 and R.err(pct.grad, rpc.grad.numpy()) < 1e-14
    # by hand: one sum over all L V columns against the tiled labels, a mean over the batch, a tenth of it
    yt = y.double()
    eps = 10e-6
    by_hand = -(yt.repeat(1, layers) * torch.log(pct.detach() + eps) + (1 - yt.repeat(1, layers)) * torch.log(1 - pct.detach() + eps)).sum(1).mean()
    assert abs(float(loss.detach()) - float(R.cross_entropy(pt.detach(), y) + 0.1 * by_hand)) < 1e-12 * abs(float(ref.detach()))
    # the distillation blends apply to the rule unchanged
    flags.distillation_features, flags.distillation_type, flags.distillation_percent = True, 1, 0.25
    t = torch.from_numpy(rs.rand(B_, V_))
    blended = tg.loss({"predictions": pt.detach(), "predictions_class": pct.detach()}, y, distill_labels_batch=t)
    want = R.mix_loss(pt.detach(), pct.detach(), y, layers) * 0.75 + R.mix_loss(pt.detach(), pct.detach(), t, layers) * 0.25
    assert abs(float(blended) - float(want)) < 1e-12 * abs(float(want))


def test_mix_loss_rule_checks_the_width_and_refuses_multitask(flags):
    _set(flags, 2)
    rs = np.random.RandomState(0)
    p, y = torch.from_numpy(rs.rand(B_, V_)), torch.from_numpy(rs.rand(B_, V_) < 0.2)
    tg = _tg()
    for width in (V_ + 1, 2 * V_ - 1, 0):
        with pytest.raises(ValueError, match="not a whole multiple"):
            tg.loss({"predictions": p, "predictions_class": torch.from_numpy(rs.rand(B_, width))}, y)
    with pytest.raises(ValueError, match="--multitask"):
        _tg(multitask=True).loss({"predictions": p, "predictions_class": p, "support_predictions": p}, y)
    # a result without predictions_class: the loss it had before
    assert float(tg.loss({"predictions": p}, y)) == float(R.cross_entropy(p, y))
    # a model's own "loss" still wins
    assert float(tg.loss({"predictions": p, "predictions_class": p, "loss": torch.tensor(3.0)}, y)) == 3.0


@pytest.mark.parametrize("name", R.HEADS)
def test_training_step_under_the_rule_moves_the_variables(monkeypatch, flags, tmp_path, name):
    """One whole TrainGraph.step.  ops.sqnorm_and_adam is device code; a plain gradient step on the same arenas stands in for it here (the
    device's own pass runs in tests/test_gpu_mix_chain.py)."""
    import yt8m_amd.ops as ops
    import yt8m_amd.video_level_models as vlm
    _cpu_ops(monkeypatch)
    _set(flags, 2)
    calls = []

    def sgd(graph, lr_t, tensors=None, **k):
        calls.append(tensors)
        for v in graph.trainable_variables()[tensors[0]:tensors[1]]:
            v.data.sub_(lr_t * v.grad)

    monkeypatch.setattr(ops, "sqnorm_and_adam", sgd)
    rs, x, y = _case(9)
    _class_file(tmp_path, flags, rs)
    tg = _tg(getattr(vlm, name)())
    g = tg.graph
    out = tg.step(torch.from_numpy(x), torch.from_numpy(y))
    assert calls == [(0, 17)]
    start = {k: v.data.clone() for k, v in g.vars.items()}
    out2 = tg.step(torch.from_numpy(x), torch.from_numpy(y))
    for k, v in g.vars.items():
        assert v.grad_written and float(v.grad.abs().max()) > 0 and not torch.equal(v.data, start[k]), k
    assert tuple(out["predictions"].shape) == (B_, V_) and float(out2["loss"]) < float(out["loss"])
    # the step's loss is the rule's: above the plain label loss of its predictions
    res = tg.forward(torch.from_numpy(x), torch.from_numpy(y))
    assert float(tg.loss(res, torch.from_numpy(y)).detach()) > float(R.cross_entropy(res["predictions"].detach(), torch.from_numpy(y)))
