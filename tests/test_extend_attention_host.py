"""CPU checks of the Extend attention plugins (Z/frame_level_models.py:5169-5234 LstmExtendModel, :5995-6073 InputExtendModel), their
heads (Z/video_level_models.py:2272-2400 MoeExtendModel, MoeExtendDistillChainModel) and their pooling's C ABI
(csrc/softmax_attention.hip): the lookup by name, variable names, shapes, initial values and l2 membership, --moe_num_extend, the head
input widths, the header / signature table / exports, yt8m_smattn_supported at every limit, argument validation without a device, the
composed form of seq_ops.softmax_attention_tm against the restatement, InputExtendModel's windows, and both plugins forward and backward
on the CPU (the LSTM stack and the MoE, which have no CPU form, stubbed by the restatement's)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import extend_attention_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT
from oracle import torch_ref

SYMBOLS = ("yt8m_smattn_supported", "yt8m_smattn_workspace_bytes", "yt8m_smattn_fwd", "yt8m_smattn_bwd")
PLUGINS = ("LstmExtendModel", "InputExtendModel")
HEADS = ("MoeExtendModel", "MoeExtendDistillChainModel")


def test_find_class_by_name_resolves_plugins_and_heads():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True
    for name in HEADS:
        assert train.find_class_by_name(name, [flm, vlm]) is getattr(vlm, name)
    assert "neither receives nor sends a gradient" in flm.LstmExtendModel.__doc__   # the docstring states the empty-video convention
    assert "frames_bool_all" in flm.InputExtendModel.__doc__                        # ... and that the windows reach the padding


def test_moe_num_extend_flag(flags):
    from yt8m_amd.flags import FLAGS
    assert FLAGS.moe_num_extend == 8
    flags.moe_num_extend = 4
    assert FLAGS.moe_num_extend == 4


def test_library_exports_and_header_declares_the_symbols():
    src, lib = declared_bound_exported(SYMBOLS, r"(int|int64_t)")
    assert "csrc/softmax_attention.hip" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits():
    lib = L.lib()
    for B, F, Hs, Hv, E, ok in ((128, 300, 1024, 1024, 8, 1), (128, 300, 1024, 1024, 1, 1), (3, 5, 128, 128, 1, 1), (17, 33, 516, 260, 3, 1),
                                (2, 300, 256, 512, 8, 1), (1, 1, 4, 4, 1, 1), (5, 9, 2048, 2048, 8, 1), (65536, 1, 4, 4, 1, 1),
                                (1, 65536, 4, 4, 1, 1), (65536, 1024, 4, 4, 1, 1),
                                (128, 300, 1024, 1024, 0, 0), (128, 300, 1024, 1024, 9, 0), (128, 300, 1022, 1024, 1, 0),
                                (128, 300, 1024, 1022, 1, 0), (128, 300, 2052, 1024, 1, 0), (128, 300, 1024, 2052, 1, 0),
                                (128, 300, 0, 1024, 1, 0), (128, 300, 1024, 0, 1, 0), (0, 300, 1024, 1024, 1, 0), (128, 0, 1024, 1024, 1, 0),
                                (128, 300, 1024, -4, 1, 0), (65537, 1, 4, 4, 1, 0), (1, 65537, 4, 4, 1, 0), (65536, 1025, 4, 4, 1, 0)):
        assert lib.yt8m_smattn_supported(B, F, Hs, Hv, E) == ok, (B, F, Hs, Hv, E)
        assert (lib.yt8m_smattn_workspace_bytes(B, F, Hs, Hv, E) > 0) == bool(ok), (B, F, Hs, Hv, E)
    # the flagship shape: 5 chunks of 64 frames; forward m_c | l_c | pooled partials, backward 640 partials | their 20 group sums
    fwd = 2 * 5 * 128 * 8 + 5 * 128 * 8 * 1024
    bwd = 640 * 1024 * 8 + 20 * 1024 * 8
    assert lib.yt8m_smattn_workspace_bytes(128, 300, 1024, 1024, 8) == 4 * max(fwd, bwd)


def test_argument_validation_without_device():
    """Every call here fails validation: nothing is launched and no device is needed."""
    lib = L.lib()
    BADARG, SHAPE = -1, -2
    p = [ctypes.c_void_p(256 * k) for k in range(1, 24)]
    B, F, Hs, Hv, E = 3, 5, 128, 64, 2
    need = lib.yt8m_smattn_workspace_bytes(B, F, Hs, Hv, E)
    f_ptrs = dict(src=p[0], vals=p[1], W1=p[2], b1=p[3], extra=p[4], valid=p[5], lo=p[6], hi=p[7], att=p[8], pooled=p[9], ws=p[10])

    def fwd(ld_src=Hs, ld_vals=Hv, ws_bytes=need, B=B, F=F, Hs=Hs, Hv=Hv, E=E, **kw):
        a = dict(f_ptrs, **kw)
        return lib.yt8m_smattn_fwd(a["src"], ld_src, a["vals"], ld_vals, a["W1"], a["b1"], a["extra"], a["valid"], a["lo"], a["hi"], a["att"],
                                   a["pooled"], a["ws"], ws_bytes, B, F, Hs, Hv, E, None)

    b_ptrs = dict(src=p[0], vals=p[1], W1=p[2], valid=p[5], lo=p[6], hi=p[7], att=p[8], pooled=p[9], G=p[11], dsrc=p[12], dvals=p[13],
                  dW1=p[14], db1=p[15], dextra=p[16], ws=p[10])

    def bwd(ld_src=Hs, ld_vals=Hv, ld_dsrc=Hs, ld_dvals=Hv, ws_bytes=need, B=B, F=F, Hs=Hs, Hv=Hv, E=E, **kw):
        a = dict(b_ptrs, **kw)
        return lib.yt8m_smattn_bwd(a["src"], ld_src, a["vals"], ld_vals, a["W1"], a["valid"], a["lo"], a["hi"], a["att"], a["pooled"], a["G"],
                                   a["dsrc"], ld_dsrc, a["dvals"], ld_dvals, a["dW1"], a["db1"], a["dextra"], a["ws"], ws_bytes, B, F, Hs, Hv,
                                   E, None)

    for call in (fwd, bwd):
        assert call(B=0) == SHAPE and call(F=0) == SHAPE and call(E=0) == SHAPE and call(E=9) == SHAPE
        assert call(Hs=130, ld_src=132) == SHAPE and call(Hv=66, ld_vals=68) == SHAPE and call(Hs=2052, ld_src=2052) == SHAPE
        assert call(Hv=0) == SHAPE                                                               # there is no weights-only form
        assert call(ld_src=Hs - 4) == BADARG and call(ld_vals=Hv - 4) == BADARG                  # a leading dimension below its width
        assert call(ws=None) == BADARG and call(ws_bytes=need - 4) == BADARG
        for name in ("src", "vals", "W1", "att", "pooled"):
            assert call(**{name: None}) == BADARG, name
        assert call(vals=p[0]) == BADARG                                                         # shared mode with Hv != Hs
        assert call(vals=p[0], Hv=Hs, ld_vals=Hs + 4, ws_bytes=1 << 30) == BADARG                # ... with another row stride
    assert fwd(b1=None) == BADARG
    assert bwd(G=None) == BADARG and bwd(dsrc=None) == BADARG
    assert bwd(ld_dsrc=Hs - 4) == BADARG and bwd(ld_dvals=Hv - 4) == BADARG
    assert bwd(vals=p[0], Hv=Hs, ld_vals=Hs, ld_dvals=Hs, ws_bytes=1 << 30) == BADARG            # shared mode with a dvals
    assert b"smattn" in lib.yt8m_last_error()


# ---- the plugins on the CPU graph: the stack and the MoE stubbed by the restatement's -------------------------------------------------
def _stub_native(monkeypatch, slots=None):
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops

    def stack(x_tm, nf, wb, slot=0, **kw):
        if slots is not None:
            slots.append(slot)
        out, c, h = torch_ref.lstm_stack(x_tm.transpose(0, 1), nf, [(ops.as_tensor(W), ops.as_tensor(b)) for W, b in wb])
        return out.transpose(0, 1).contiguous(), list(zip(c, h))

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V_, M_, **k: R.moe(x, Wg.data, We.data, be.data, M_))
    monkeypatch.setattr(ops, "frame_pool", lambda x, kind: x.max(dim=1)[0])


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


@pytest.mark.parametrize("name", PLUGINS)
@pytest.mark.parametrize("layers", [1, 2])
def test_variable_names_shapes_initial_values_and_l2(monkeypatch, flags, name, layers):
    import yt8m_amd.frame_level_models as flm
    D, H, E, B, F, V, M = 12, 16, 3, 2, 7, 5, 2
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_extend, flags.moe_num_mixtures = str(H), layers, E, M
    flags.video_level_classifier_model = "MoeExtendModel"
    slots = []
    _stub_native(monkeypatch, slots)
    g = _graph()
    res = getattr(flm, name)().create_model(torch.randn(B, F, D), vocab_size=V, num_frames=torch.tensor([7, 3]), l2_penalty=3e-7)
    want = R.variable_shapes(name, "MoeExtendModel", D, H, layers, E, V, M)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(want.items())               # names, shapes, creation order
    for k in ("W1", "b1", "W2", "b2"):
        assert g.vars[k].l2 == 3e-7 and g.vars[k].trainable, k                                       # all four, biases included
    for k in ("b1", "b2"):
        assert bool((g.vars[k].data == np.float32(0.1)).all()), k
    for k in ("W1", "W2"):
        assert float(g.vars[k].data.abs().max()) <= 0.2 + 1e-7 and float(g.vars[k].data.std()) > 0.03, k   # truncated at two stddev of 0.1
    assert all(v.l2 == 0.0 for k, v in g.vars.items() if "basic_lstm_cell" in k)
    assert g.vars["gates/weights"].l2 == 1e-8                                  # create_model's l2_penalty is not forwarded to the head
    assert tuple(g.vars["gates/weights"].data.shape) == (H, V * (M + 1))       # the head reads the pooled rows, H wide
    assert tuple(res["predictions"].shape) == (B, V)
    if name == "LstmExtendModel":
        assert slots == [0] and tuple(res["attention_weight"].shape) == (B, E * F) and not res["attention_weight"].requires_grad
    else:
        assert slots == [0, 1] and "attention_weight" not in res                                    # slots of their own


def test_distill_chain_head_input_width(monkeypatch, flags):
    import yt8m_amd.ops as ops
    import yt8m_amd.video_level_models as vlm
    E, B, H, V, M = 3, 2, 16, 5, 2
    flags.moe_num_extend, flags.moe_num_mixtures = E, M
    _stub_native(monkeypatch)
    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, **k: x @ W.data + (0 if b is None else b.data))
    monkeypatch.setattr(ops, "activation", lambda x, kind: torch.relu(x))
    x, d = torch.randn(B * E, H), torch.rand(B, V)
    g = _graph()
    res = vlm.MoeExtendDistillChainModel().create_model(x, V, distillation_predictions=d, l2_penalty=2e-7)
    assert list(g.vars) == ["class_inputs/weights", "class_inputs/biases", "gates/weights", "experts/weights", "experts/biases"]
    assert tuple(g.vars["class_inputs/weights"].data.shape) == (V, 256) and g.vars["class_inputs/weights"].l2 == 2e-7
    assert tuple(g.vars["gates/weights"].data.shape) == (H + 256, V * (M + 1))
    P = {k: v.data.double() for k, v in g.vars.items()}
    want = R.moe_extend_distill_chain_model(x.double(), P, M, E, d.double())
    assert R.err(res["predictions"], want.numpy()) < 2e-6
    # without distillation predictions it is MoeExtendModel
    g = _graph()
    res = vlm.MoeExtendDistillChainModel().create_model(x, V)
    assert list(g.vars) == ["gates/weights", "experts/weights", "experts/biases"] and tuple(g.vars["gates/weights"].data.shape) == (H, V * (M + 1))
    P = {k: v.data.double() for k, v in g.vars.items()}
    assert R.err(res["predictions"], R.moe_extend_model(x.double(), P, M, E).numpy()) < 2e-6
    g = _graph()
    res2 = vlm.MoeExtendModel().create_model(x, V)
    assert torch.equal(res2["predictions"], res["predictions"])


# ---- the composed form against the restatement -------------------------------------------------------------------------------------
F_, B_, HS_, HV_, E_ = 7, 5, 12, 8, 3
NF_ = np.array([0, 1, 7, 6, 3], dtype=np.int32)


def _operands(scale=1.0, shared=False):
    rs = np.random.RandomState(7)
    src = rs.randn(F_, B_, HS_).astype(np.float32)
    vals = None if shared else rs.randn(F_, B_, HV_).astype(np.float32)
    W1 = (scale * rs.randn(HS_, E_) / np.sqrt(HS_)).astype(np.float32)
    b1 = (0.1 * rs.randn(E_)).astype(np.float32)
    extra = (scale * 0.5 * rs.randn(B_, F_, E_)).astype(np.float32)
    G = rs.randn(B_, E_, HS_ if shared else HV_).astype(np.float32)
    return src, vals, W1, b1, extra, G


def _masks(kind):
    valid = (np.arange(F_)[None, :] < NF_[:, None]).astype(np.uint8)
    lo, hi = (t.numpy().astype(np.int32) for t in R.windows(NF_, E_))
    return {"frames": (valid, None, None), "window": (None, lo, hi), "both": (valid, lo, hi), "none": (None, None, None)}[kind]


def _composed(src, vals, W1, b1, extra, masks, G, dtype):
    import yt8m_amd.seq_ops as seq_ops
    T = lambda a: None if a is None else torch.from_numpy(a).to(dtype).requires_grad_(True)
    I = lambda a: None if a is None else torch.from_numpy(a)
    ts, tv, tW, tb, tx = T(src), T(vals), T(W1), T(b1), T(extra)
    before = dict(seq_ops.SOFTMAX_ATTENTION_CALLS)
    att, pooled = seq_ops.softmax_attention_tm(ts, tW, tb, ts if tv is None else tv, tx, *(I(m) for m in masks))
    assert seq_ops.SOFTMAX_ATTENTION_CALLS == dict(before, composed=before["composed"] + 1)          # CPU tensors: the composed form
    assert not att.requires_grad                                                                     # att carries no gradient
    (pooled * torch.from_numpy(G).to(dtype)).sum().backward()
    got = {"att": att, "pooled": pooled.detach(), "dsrc": ts.grad, "dW1": tW.grad, "db1": tb.grad}
    if tv is not None:
        got["dvals"] = tv.grad
    if tx is not None:
        got["dextra"] = tx.grad
    return got


@pytest.mark.parametrize("kind", ["frames", "window", "both", "none"])
@pytest.mark.parametrize("shared", [False, True], ids=["two", "shared"])
@pytest.mark.parametrize("scale", [1.0, 20.0])
def test_composed_form_matches_the_restatement(kind, shared, scale):
    src, vals, W1, b1, extra, G = _operands(scale, shared)
    masks = _masks(kind)
    for with_extra in (True, False):
        x = extra if with_extra else None
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-5)):
            ref = R.op_with_grads(src, vals, W1, b1, x, *masks, G, dtype)
            assert all(np.isfinite(v).all() for v in ref.values())
            got = _composed(src, vals, W1, b1, x, masks, G, dtype)
            assert got["att"].dtype == dtype and tuple(got["att"].shape) == (B_, F_, E_)
            assert set(got) == set(ref) - {"den"}
            for k, v in got.items():
                assert R.err(v, ref[k]) <= tol, (k, dtype, R.err(v, ref[k]))


def test_empty_rows_are_exact_zeros_and_rows_sum_to_one():
    src, vals, W1, b1, extra, G = _operands()
    masks = _masks("frames")
    got = _composed(src, vals, W1, b1, extra, masks, G, torch.float32)
    live = torch.from_numpy(NF_ >= 1)
    assert float((got["att"].sum(dim=1)[live] - 1.0).abs().max()) <= 4 * np.finfo(np.float32).eps
    assert not live[0]
    for k in ("att", "pooled", "dextra"):
        assert float(got[k][0].abs().max()) == 0.0, k
    for k in ("dsrc", "dvals"):
        assert float(got[k][:, 0].abs().max()) == 0.0, k
        assert float(got[k][:, 1:].abs().max()) > 0.0, k
    past = torch.from_numpy(np.arange(F_)[None, :] >= NF_[:, None])          # [B,F]
    assert float(got["att"][past].abs().max()) == 0.0 and float(got["dextra"][past].abs().max()) == 0.0
    assert float(got["dsrc"].transpose(0, 1)[past].abs().max()) == 0.0 and float(got["dvals"].transpose(0, 1)[past].abs().max()) == 0.0
    # an empty window (lo > hi) of one head: that head alone is empty
    lo = np.zeros((B_, E_), dtype=np.int32)
    hi = np.full((B_, E_), F_ - 1, dtype=np.int32)
    lo[2, 1], hi[2, 1] = 4, 3
    got = _composed(src, vals, W1, b1, extra, (None, lo, hi), G, torch.float32)
    assert float(got["att"][2, :, 1].abs().max()) == 0.0 and float(got["pooled"][2, 1].abs().max()) == 0.0
    assert float(got["att"][2, :, 0].sum()) > 0.99 and all(np.isfinite(v.numpy()).all() for v in got.values())


@pytest.mark.parametrize("E", [1, 3, 8])
def test_input_extend_windows(E):
    import yt8m_amd.frame_level_models as flm
    F = 24
    nf = torch.tensor([0, 1, E - 1, E, F - 1, F], dtype=torch.int32)
    lo, hi = flm.input_extend_windows(nf, E)
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and tuple(lo.shape) == (6, E)
    for b, n in enumerate(nf.tolist()):
        for i in range(E):
            assert int(lo[b, i]) == (n // E) * i and int(hi[b, i]) == (n // E) * i + 2 * (n // E), (n, i)
    assert int(lo[0].abs().max()) == 0 and int(hi[0].abs().max()) == 0                       # num_frames = 0: the window [0, 0]
    if E > 1:
        assert int(hi[2].max()) == 0 and int(hi[1].max()) == 0                               # num_frames < E: [0, 0] as well
        assert int(hi[5, E - 1]) == (F // E) * (E + 1) and int(hi[5, E - 1]) > F - 1          # the last window runs past num_frames
    wlo, whi = R.windows(nf.numpy(), E)
    assert torch.equal(wlo.to(torch.int32), lo) and torch.equal(whi.to(torch.int32), hi)


@pytest.mark.parametrize("name", PLUGINS)
def test_plugins_on_the_cpu_match_the_restatement(monkeypatch, flags, name):
    """forward and backward on float frames with the composed op: predictions, attention_weight and the gradient of every body variable"""
    import yt8m_amd.frame_level_models as flm
    D, H, E, B, F, V, M, layers = 12, 16, 3, 4, 9, 6, 2, 2
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_extend, flags.moe_num_mixtures = str(H), layers, E, M
    flags.video_level_classifier_model = "MoeExtendModel"
    _stub_native(monkeypatch)
    rs = np.random.RandomState(5)
    nf = torch.tensor([9, 0, 4, 8], dtype=torch.int32)
    x = rs.randn(B, F, D).astype(np.float32)
    x = torch.from_numpy(x * (np.arange(F)[None, :] < nf.numpy()[:, None])[:, :, None].astype(np.float32))
    g = _graph()
    getattr(flm, name)().create_model(x, vocab_size=V, num_frames=nf)
    g.finalize()
    shapes = R.variable_shapes(name, "MoeExtendModel", D, H, layers, E, V, M)
    for k, s in shapes.items():
        g.vars[k].data.copy_(torch.from_numpy((rs.randn(*s) * (0.1 if k.endswith(("biases", "b1", "b2")) else 1.5 / np.sqrt(s[0]))).astype(np.float32)))
    g.begin_step()
    res = getattr(flm, name)().create_model(x, vocab_size=V, num_frames=nf)
    go = torch.from_numpy(rs.randn(B, V).astype(np.float32))
    (res["predictions"] * go).sum().backward()
    P = {k: v.data.double().requires_grad_(True) for k, v in g.vars.items()}
    pooled, aw = R.BODIES[name](x.double(), nf, P, layers, E)
    want = R.moe_extend_model(pooled, P, M, E)
    (want * go.double()).sum().backward()
    assert R.err(res["predictions"], want.detach().numpy()) < 2e-6
    if name == "LstmExtendModel":
        assert R.err(res["attention_weight"], aw.detach().numpy()) < 2e-6
        assert float(res["attention_weight"][1].abs().max()) == 0.0                          # the video without frames
    for k in shapes:
        if not k.startswith(("gates", "experts")):                                           # (the stub head hands no gradient to its own variables)
            assert float(P[k].grad.abs().max()) > 0.0, k
            assert R.err(g.vars[k].grad, P[k].grad.numpy()) < 5e-6, k
