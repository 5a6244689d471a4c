"""CPU checks of the scalar-gate LSTM plugins (Z/frame_level_models.py:1521-1790) and of their layer's C ABI (csrc/gate_cell.hip): the
lookup by name, the twelve Variables per layer (names, shapes, l2, initial values), the header / signature table / exports, argument
validation without a device, and the composed form of seq_ops.gate_lstm_layer against the fp64 restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gate_lstm_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_gate_lstm_supported", "yt8m_gate_lstm_layer_fwd", "yt8m_gate_lstm_layer_bwd")
PLUGINS = ("LstmGateModel", "LstmGateMultilayerModel")


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True


def test_library_exports_and_header_declares_the_gate_lstm_symbols():
    src, lib = declared_bound_exported(SYMBOLS)
    assert "Z/frame_level_models.py:1583-1640" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits():
    lib = L.lib()
    for B, H, ok in ((128, 1024, 1), (3, 256, 1), (5, 2048, 1), (1, 512, 1), (128, 192, 0), (128, 2304, 0), (128, 0, 0), (0, 1024, 0),
                     (128, 128, 0), (128, 2048 + 256, 0)):
        assert lib.yt8m_gate_lstm_supported(B, H) == ok, (B, H)


def test_argument_validation_without_device():
    """Every call here fails validation or has nothing to do: nothing is launched and no device is needed."""
    lib = L.lib()
    OK, BADARG, SHAPE = 0, -1, -2
    p = [ctypes.c_void_p(256 * k) for k in range(1, 16)]
    H = 256

    def fwd(zv=p[0], zs=p[1], lds=2, Uv=p[2], ldu=2 * H, Us=p[3], hs=p[4], cs=p[5], c_last=p[6], nf=p[7], F=4, B=3, H=H):
        return lib.yt8m_gate_lstm_layer_fwd(zv, zs, lds, Uv, ldu, Us, hs, cs, c_last, nf, F, B, H, None, 0, None)

    def bwd(zv=p[0], zs=p[1], lds=2, Uv=p[2], ldu=2 * H, Us=p[3], hs=p[4], cs=p[5], dout=p[8], dc_last=p[9], dzv=p[10], dzs=p[11],
            work=p[12], nf=p[7], F=4, B=3, H=H):
        return lib.yt8m_gate_lstm_layer_bwd(zv, zs, lds, Uv, ldu, Us, hs, cs, dout, dc_last, dzv, dzs, work, nf, F, B, H, None, 0, None)

    for call in (fwd, bwd):
        assert call(F=-1) == SHAPE and call(B=-1) == SHAPE and call(H=-256) == SHAPE           # negative size
        assert call(ldu=2 * H - 1) == SHAPE                                                     # small ldu
        assert call(lds=1) == SHAPE and call(lds=0) == SHAPE                                    # lds < 2
        assert call(H=192, ldu=384) == SHAPE and call(H=2304, ldu=4608) == SHAPE                # what _supported refuses
        for name in ("zv", "zs", "Uv", "Us", "hs", "cs"):
            assert call(**{name: None}) == BADARG, name                                         # null operand
        assert call(F=0) == OK and call(B=0) == OK and call(H=0) == OK                          # nothing to do
        assert call(F=0, zv=None, zs=None, Uv=None, Us=None, hs=None, cs=None, nf=None) == OK   # ... before anything else
    for name in ("dzv", "dzs", "work"):
        assert bwd(**{name: None}) == BADARG, name
    # num_frames may be null only together with c_last / dc_last
    assert fwd(nf=None) == BADARG and bwd(nf=None) == BADARG
    assert b"gate_lstm" in lib.yt8m_last_error()


# ---- the plugins' Variables on the CPU graph ----------------------------------------------------------------------------------------
def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


def _stub_head(monkeypatch):
    """ops.moe_head has no CPU form: the MoE of the restatement on the Variables' data stands in for it."""
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V_, M_, **k: R.moe(x, Wg.data, We.data, be.data, M_))


def _check_unit(g, scope, D, H):
    for n, shape in R.shapes(D, H).items():
        v = g.vars["%s/%s" % (scope, n)]
        assert tuple(v.data.shape) == shape and v.l2 == 1e-8 and v.trainable, (scope, n)
        if n == "bf":
            assert float(v.data) == 1.0
        elif n[0] == "b":
            assert bool((v.data == np.float32(0.1)).all()), n
        else:
            assert float(v.data.abs().max()) <= 0.2 + 1e-7 and float(v.data.std()) > 0.03, n       # truncated at two stddev of 0.1


def test_lstm_gate_model_variables(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _stub_head(monkeypatch)
    flags.lstm_cells, flags.moe_num_mixtures = "16", 2
    g = _graph()
    B, F, D, V = 3, 5, 8, 10
    res = flm.LstmGateModel().create_model(torch.randn(B, F, D), vocab_size=V, num_frames=torch.tensor([5, 1, 3]))
    assert tuple(res["predictions"].shape) == (B, V)
    names = ["lstm_forward/" + n for n in R.NAMES] + ["gates/weights", "experts/weights", "experts/biases"]
    assert list(g.vars) == names
    _check_unit(g, "lstm_forward", D, 16)
    assert tuple(g.vars["gates/weights"].data.shape) == (16, V * 3)


def test_lstm_gate_multilayer_model_variables(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _stub_head(monkeypatch)
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures = "16", 2, 2
    g = _graph()
    B, F, D, V = 3, 5, 8, 10
    res = flm.LstmGateMultilayerModel().create_model(torch.randn(B, F, D), vocab_size=V, num_frames=torch.tensor([5, 1, 3]))
    assert tuple(res["predictions"].shape) == (B, V)
    names = ["lstm_lsyer%dlstm_forward/%s" % (l, n) for l in range(2) for n in R.NAMES] + ["gates/weights", "experts/weights", "experts/biases"]
    assert list(g.vars) == names                                          # the reference's spelling
    _check_unit(g, "lstm_lsyer0lstm_forward", D, 16)
    _check_unit(g, "lstm_lsyer1lstm_forward", 16, 16)                     # layer 1 reads layer 0's hidden outputs
    assert tuple(g.vars["gates/weights"].data.shape) == (2 * 16, V * 3)   # the layers' memories concatenated


def test_initialisers():
    from yt8m_amd.variables import constant, truncated_normal
    gen = torch.Generator().manual_seed(3)
    t = truncated_normal(0.1)((200, 300), gen, torch.device("cpu"))
    assert t.dtype == torch.float32 and float(t.abs().max()) <= 0.2 + 1e-7
    # a normal truncated at two standard deviations has standard deviation 0.8796 sigma
    assert abs(float(t.std()) - 0.08796) < 2e-3 and abs(float(t.mean())) < 2e-3
    c = constant(0.1)((7,), gen, torch.device("cpu"))
    assert c.dtype == torch.float32 and bool((c == np.float32(0.1)).all())


# ---- the composed form against the restatement ------------------------------------------------------------------------------------
F_, B_, D_, H_ = 6, 3, 8, 16


@pytest.mark.parametrize("nf", [[6, 1, 3], [0, 6, 2]])
def test_composed_form_matches_the_restatement_in_fp64(nf):
    import yt8m_amd.seq_ops as seq_ops
    rs = np.random.RandomState(11)
    P = R.random_unit(rs, D_, H_)
    x = rs.randn(F_, B_, D_).astype(np.float32)
    dout, dc = rs.randn(F_, B_, H_).astype(np.float32), rs.randn(B_, H_).astype(np.float32)
    ref = R.layer_with_grads(x, nf, P, dout, dc, torch.float64)
    Pt = R.to_torch(P, torch.float64, True)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    before = dict(seq_ops.GATE_LSTM_CALLS)
    out, c_last = seq_ops.gate_lstm_layer(xt, *R.operands(Pt), torch.tensor(nf))
    assert seq_ops.GATE_LSTM_CALLS["composed"] == before["composed"] + 1 and seq_ops.GATE_LSTM_CALLS["kernels"] == before["kernels"]
    assert tuple(out.shape) == (F_, B_, H_) and tuple(c_last.shape) == (B_, H_)
    ((out * torch.from_numpy(dout).double()).sum() + (c_last * torch.from_numpy(dc).double()).sum()).backward()   # through both returns
    got = {"out": out, "c_last": c_last, "dx": xt.grad}
    got.update({"d" + n: Pt[n].grad for n in R.NAMES})
    for k in ref:
        assert R.err(got[k], ref[k]) < 1e-12, k
    # the memory after step num_frames - 1, read off the recurrence itself
    for b, n in enumerate(nf):
        if n < 1:
            assert float(c_last[b].detach().abs().max()) == 0.0
    if 0 in nf:
        # the dead row's dc_last reaches no gradient: the same gradients with another dc_last in that row
        b0 = nf.index(0)
        dc2 = dc.copy()
        dc2[b0] += 5.0
        ref2 = R.layer_with_grads(x, nf, P, dout, dc2, torch.float64)
        Pt2 = R.to_torch(P, torch.float64, True)
        x2 = torch.from_numpy(x).double().requires_grad_(True)
        out2, c2 = seq_ops.gate_lstm_layer(x2, *R.operands(Pt2), torch.tensor(nf))
        ((out2 * torch.from_numpy(dout).double()).sum() + (c2 * torch.from_numpy(dc2).double()).sum()).backward()
        assert torch.equal(x2.grad, xt.grad) and all(torch.equal(Pt2[n].grad, Pt[n].grad) for n in R.NAMES)
        assert R.err(x2.grad, ref2["dx"]) < 1e-12


def test_lstm_gate_model_forward_on_cpu_matches_restatement_and_moe_head(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _stub_head(monkeypatch)
    V, M = 10, 2
    flags.lstm_cells, flags.moe_num_mixtures = str(H_), M
    g = _graph()
    rs = np.random.RandomState(12)
    x = torch.from_numpy(rs.randn(B_, F_, D_).astype(np.float32))
    nf = torch.tensor([6, 1, 3])
    p = flm.LstmGateModel().create_model(x, vocab_size=V, num_frames=nf)["predictions"]
    P = {n: g.vars["lstm_forward/" + n].data.double() for n in R.NAMES}
    state, _ = R.rnn_gate(x.double(), nf, P)
    want = R.moe(state, g.vars["gates/weights"].data.double(), g.vars["experts/weights"].data.double(), g.vars["experts/biases"].data.double(), M)
    assert R.err(p, want.numpy()) < 2e-6
    # and the gradient lands in every one of the twelve Variables' slots
    g.finalize()
    g.begin_step()
    p = flm.LstmGateModel().create_model(x, vocab_size=V, num_frames=nf)["predictions"]
    P = {n: g.vars["lstm_forward/" + n].data.double().requires_grad_(True) for n in R.NAMES}
    go = torch.from_numpy(rs.randn(B_, V).astype(np.float32))
    state, _ = R.rnn_gate(x.double(), nf, P)
    (R.moe(state, g.vars["gates/weights"].data.double(), g.vars["experts/weights"].data.double(), g.vars["experts/biases"].data.double(), M)
     * go.double()).sum().backward()
    (p * go).sum().backward()
    for n in R.NAMES:
        assert R.err(g.vars["lstm_forward/" + n].grad, P[n].grad.numpy()) < 5e-6, n
