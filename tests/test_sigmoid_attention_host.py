"""CPU checks of the sigmoid-attention LSTM plugins (W/all_frame_models/lstm_attention_model.py, lstm_attention_lstm_model.py,
lstm_multi_attention_model.py) and of their pooling's C ABI (csrc/sigmoid_attention.hip): the lookup by name, the TF-1.0 variable names
and shapes (written from memory, as SURVEY.md Appendix A), the head input widths, --attention_size, the header / signature table /
exports, argument validation without a device, and the composed form of seq_ops.sigmoid_attention against the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sigmoid_attention_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_sigattn_supported", "yt8m_sigattn_workspace_bytes", "yt8m_sigattn_fwd", "yt8m_sigattn_bwd")
PLUGINS = ("LstmAttentionModel", "LstmAttentionLstmModel", "LstmMultiAttentionModel")


def test_find_class_by_name_resolves_the_three_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True
        assert "mask_emb" in cls.__doc__ or "LstmAttentionModel" in cls.__doc__          # the docstrings say that the table is left out


def test_attention_size_flag(flags):
    from yt8m_amd.flags import FLAGS
    assert FLAGS.attention_size == 1
    flags.attention_size = 4
    assert FLAGS.attention_size == 4


def test_library_exports_and_header_declares_the_symbols():
    src, lib = declared_bound_exported(SYMBOLS, r"(int|int64_t)")
    assert "lstm_attention_lstm_model.py:78-92" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits():
    lib = L.lib()
    for B, F, Hs, Hv, A, ok in ((128, 300, 1024, 1024, 1, 1), (128, 300, 1024, 0, 4, 1), (3, 5, 128, 128, 1, 1), (17, 33, 516, 260, 3, 1),
                                (2, 300, 256, 512, 8, 1), (1, 1, 4, 0, 1, 1), (5, 9, 2048, 2048, 8, 1),
                                (128, 300, 1024, 1024, 0, 0), (128, 300, 1024, 1024, 9, 0), (128, 300, 1022, 1024, 1, 0),
                                (128, 300, 1024, 1022, 1, 0), (128, 300, 2052, 0, 1, 0), (128, 300, 1024, 2052, 1, 0), (128, 300, 0, 0, 1, 0),
                                (0, 300, 1024, 0, 1, 0), (128, 0, 1024, 0, 1, 0), (128, 300, 1024, -4, 1, 0), (70000, 300, 1024, 0, 1, 0)):
        assert lib.yt8m_sigattn_supported(B, F, Hs, Hv, A) == ok, (B, F, Hs, Hv, A)
        assert (lib.yt8m_sigattn_workspace_bytes(B, F, Hs, Hv, A) > 0) == bool(ok), (B, F, Hs, Hv, A)
    # the backward partials of the flagship shape: 128 x 10 workgroups x (1024 + 1) floats, their 40 group sums and inner
    assert lib.yt8m_sigattn_workspace_bytes(128, 300, 1024, 1024, 1) == 4 * (128 + 1280 * 1025 + 40 * 1025)


def test_argument_validation_without_device():
    """Every call here fails validation: nothing is launched and no device is needed."""
    lib = L.lib()
    BADARG, SHAPE = -1, -2
    p = [ctypes.c_void_p(256 * k) for k in range(1, 24)]
    B, F, Hs, Hv, A = 3, 5, 128, 64, 2
    need = lib.yt8m_sigattn_workspace_bytes(B, F, Hs, Hv, A)
    f_ptrs = dict(src=p[0], vals=p[1], Wa=p[2], ba=p[3], nf=p[4], att=p[5], den=p[6], pooled=p[7], ws=p[8])

    def fwd(ld_src=Hs, ld_vals=Hv, ws_bytes=need, B=B, F=F, Hs=Hs, Hv=Hv, A=A, **kw):
        a = dict(f_ptrs, **kw)
        return lib.yt8m_sigattn_fwd(a["src"], ld_src, a["vals"], ld_vals, a["Wa"], a["ba"], a["nf"], a["att"], a["den"], a["pooled"], a["ws"],
                                    ws_bytes, B, F, Hs, Hv, A, None)

    b_ptrs = dict(src=p[0], vals=p[1], Wa=p[2], nf=p[4], att=p[5], den=p[6], pooled=p[7], G=p[9], E=p[10], dsrc=p[11], dvals=p[12], dWa=p[13],
                  dba=p[14], ws=p[8])

    def bwd(ld_src=Hs, ld_vals=Hv, ld_dsrc=Hs, ld_dvals=Hv, ws_bytes=need, B=B, F=F, Hs=Hs, Hv=Hv, A=A, **kw):
        a = dict(b_ptrs, **kw)
        return lib.yt8m_sigattn_bwd(a["src"], ld_src, a["vals"], ld_vals, a["Wa"], a["nf"], a["att"], a["den"], a["pooled"], a["G"], a["E"],
                                    a["dsrc"], ld_dsrc, a["dvals"], ld_dvals, a["dWa"], a["dba"], a["ws"], ws_bytes, B, F, Hs, Hv, A, None)

    for call in (fwd, bwd):
        assert call(B=0) == SHAPE and call(F=0) == SHAPE and call(A=0) == SHAPE and call(A=9) == SHAPE
        assert call(Hs=130, ld_src=132) == SHAPE and call(Hv=66, ld_vals=68) == SHAPE and call(Hs=2052, ld_src=2052) == SHAPE
        assert call(ld_src=Hs - 4) == BADARG and call(ld_vals=Hv - 4) == BADARG                  # a leading dimension below its width
        assert call(ws=None) == BADARG and call(ws_bytes=need - 4) == BADARG
        for name in ("src", "Wa", "nf", "att", "den"):
            assert call(**{name: None}) == BADARG, name
    for name in ("ba", "vals", "pooled"):
        assert fwd(**{name: None}) == BADARG, name
    assert fwd(Hv=0) == BADARG                                                                   # vals / pooled given without a width
    assert bwd(dsrc=None) == BADARG and bwd(ld_dsrc=Hs - 4) == BADARG and bwd(ld_dvals=Hv - 4) == BADARG
    assert bwd(vals=None) == BADARG and bwd(pooled=None) == BADARG                               # G needs both
    assert bwd(Hv=0) == BADARG                                                                   # G / dvals without a width
    assert b"sigattn" in lib.yt8m_last_error()


# ---- the plugins' variables on the CPU graph, the native calls stubbed out ----------------------------------------------------------
def _build(name, monkeypatch, flags, D=1152, H=1024, layers=2, A=1, B=2, F=3, V=5):
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.variables import reset_default_graph
    flags.lstm_cells, flags.lstm_layers, flags.attention_size = str(H), layers, A
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    slots = []

    def stack(x, nf, wb, slot=0, **kw):
        slots.append(slot)
        return torch.zeros(F, B, H), [(torch.full((B, H), 1.0 + l), torch.full((B, H), 2.0 + l)) for l in range(len(wb))]

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(seq_ops, "pool_tn", lambda w, x: torch.einsum("bfa,bfd->bad", w, x))
    seen = {}

    class Head(object):
        def create_model(self, model_input, vocab_size, **kw):
            seen["input"], seen["kw"] = model_input, kw
            return {"predictions": torch.arange(model_input.shape[0] * vocab_size, dtype=torch.float32).view(model_input.shape[0], vocab_size)}

    monkeypatch.setattr(flm, "_head", lambda name=None: Head)
    monkeypatch.setattr(flm.ops, "frame_pool", lambda x, kind: x.max(dim=1)[0])
    res = getattr(flm, name)().create_model(torch.zeros(B, F, D), vocab_size=V, num_frames=torch.tensor([3, 1]), l2_penalty=3e-7)
    return g, seen, slots, res


@pytest.mark.parametrize("name", PLUGINS)
@pytest.mark.parametrize("layers", [1, 2])
def test_variable_names_shapes_and_head_input(monkeypatch, flags, name, layers):
    D, H, A, B, V = 1152, 1024, 3, 2, 5
    g, seen, slots, res = _build(name, monkeypatch, flags, D=D, H=H, layers=layers, A=A, V=V)
    want = R.variable_shapes(name, D, H, layers, A, V, 2)
    want = {k: v for k, v in want.items() if not k.startswith(("gates", "experts"))}                 # (the head is stubbed)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(want.items())               # names, shapes, creation order
    fc = "fully_connected" if name == "LstmMultiAttentionModel" else "RNN/fully_connected"
    assert g.vars[fc + "/weights"].l2 == 3e-7 and g.vars[fc + "/biases"].l2 == 0.0                   # the FC weights carry l2_penalty
    assert all(v.l2 == 0.0 for k, v in g.vars.items() if "basic_lstm_cell" in k)
    assert "mask_emb" not in g.vars
    assert seen["kw"]["l2_penalty"] == 3e-7 and tuple(seen["kw"]["original_input"].shape) == (B, 3, D)
    x = seen["input"]
    if name == "LstmAttentionModel":
        assert tuple(x.shape) == (B, D + 2 * layers * H) and slots == [0]
        # [mean_input | c0|h0|c1|h1...]: the stub's c_l = 1 + l, h_l = 2 + l
        assert [float(x[0, D + k * H]) for k in range(2 * layers)] == [v for l in range(layers) for v in (1.0 + l, 2.0 + l)]
    elif name == "LstmAttentionLstmModel":
        assert tuple(x.shape) == (B, H + 2 * layers * H) and slots == [0, 1]                          # slots of their own
        assert [float(x[0, H + k * H]) for k in range(2 * layers)] == [1.0 + l for l in range(layers)] * 2      # ATT c's, then RNN c's
    else:
        assert tuple(x.shape) == (B * A, D) and slots == [0]
        # the maximum over a video's A rows of the stub head's predictions: its last row
        assert tuple(res["predictions"].shape) == (B, V) and float(res["predictions"][1, 0]) == float((B * A - 1) * V)


# ---- the composed form against the restatement -------------------------------------------------------------------------------------
F_, B_, HS_, HV_, A_ = 7, 5, 12, 8, 3
NF_ = np.array([0, 1, 7, 6, 3], dtype=np.int32)


def _operands(scale=1.0):
    rs = np.random.RandomState(7)
    src = rs.randn(F_, B_, HS_).astype(np.float32)
    vals = rs.randn(F_, B_, HV_).astype(np.float32)
    Wa = (scale * rs.randn(HS_, A_) / np.sqrt(HS_)).astype(np.float32)
    ba = (0.1 * rs.randn(A_)).astype(np.float32)
    G, E = rs.randn(B_, A_, HV_).astype(np.float32), rs.randn(B_, F_, A_).astype(np.float32)
    return src, vals, Wa, ba, G, E


def _composed(src, vals, Wa, ba, G, E, dtype):
    import yt8m_amd.seq_ops as seq_ops
    T = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
    ts, tv, tW, tb = T(src), (None if vals is None else T(vals)), T(Wa), T(ba)
    before = dict(seq_ops.SIGMOID_ATTENTION_CALLS)
    att, pooled = seq_ops.sigmoid_attention(ts, tW, tb, torch.from_numpy(NF_), tv)
    assert seq_ops.SIGMOID_ATTENTION_CALLS == dict(before, composed=before["composed"] + 1)          # CPU tensors: the composed form
    loss = (att * torch.from_numpy(E).to(dtype)).sum()
    if pooled is not None:
        loss = loss + (pooled * torch.from_numpy(G).to(dtype)).sum()
    loss.backward()
    got = {"att": att.detach(), "dsrc": ts.grad, "dWa": tW.grad, "dba": tb.grad}
    if vals is not None:
        got.update(pooled=pooled.detach(), dvals=tv.grad)
    return got


@pytest.mark.parametrize("with_values", [True, False])
@pytest.mark.parametrize("scale", [1.0, 20.0])
def test_composed_form_matches_the_restatement(with_values, scale):
    src, vals, Wa, ba, G, E = _operands(scale)
    if not with_values:
        vals = G = None
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 2e-5)):
        ref = R.op_with_grads(src, vals, Wa, ba, NF_, G, E, dtype)
        got = _composed(src, vals, Wa, ba, G, E, dtype)
        assert got["att"].dtype == dtype and tuple(got["att"].shape) == (B_, F_, A_)
        for k, v in got.items():
            assert R.err(v, ref[k]) <= tol, (k, dtype, R.err(v, ref[k]))
    if not with_values:
        assert "pooled" not in got


def test_attention_rows_sum_to_one_and_empty_videos_are_exact_zeros():
    src, vals, Wa, ba, G, E = _operands()
    got = _composed(src, vals, Wa, ba, G, E, torch.float32)
    sums = got["att"].sum(dim=1)                                             # [B,A]
    live = torch.from_numpy(NF_ >= 1)
    assert float((sums[live] - 1.0).abs().max()) <= 4 * np.finfo(np.float32).eps
    assert not live[0]
    for k in ("att", "pooled"):
        assert float(got[k][0].abs().max()) == 0.0, k
    for k in ("dsrc", "dvals"):
        assert float(got[k][:, 0].abs().max()) == 0.0, k
        assert float(got[k][:, 1:].abs().max()) > 0.0, k
    # past a video's num_frames: no weight, no gradient
    past = torch.from_numpy(np.arange(F_)[None, :] >= NF_[:, None])          # [B,F]
    assert float(got["att"][past].abs().max()) == 0.0
    assert float(got["dsrc"].transpose(0, 1)[past].abs().max()) == 0.0 and float(got["dvals"].transpose(0, 1)[past].abs().max()) == 0.0
    # an empty batch reaches neither Wa nor ba
    import yt8m_amd.seq_ops as seq_ops
    tW, tb = torch.from_numpy(Wa).requires_grad_(True), torch.from_numpy(ba).requires_grad_(True)
    att, pooled = seq_ops.sigmoid_attention(torch.from_numpy(src), tW, tb, torch.zeros(B_, dtype=torch.int32), torch.from_numpy(vals))
    ((att * torch.from_numpy(E)).sum() + (pooled * torch.from_numpy(G)).sum()).backward()
    assert float(att.abs().max()) == 0.0 and float(pooled.abs().max()) == 0.0
    assert float(tW.grad.abs().max()) == 0.0 and float(tb.grad.abs().max()) == 0.0
