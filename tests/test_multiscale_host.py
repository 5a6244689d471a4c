"""CPU checks of the multiscale CNN-LSTM plugins (W/all_frame_models/multiscale_cnn_lstm_model.py,
distillchain_multiscale_cnn_lstm_model.py): the lookup by name, the TF-1.0 variable names and shapes (written from memory, as SURVEY.md
Appendix A), the per-scale frame counts handed to the LSTM stacks, and the C-ABI declarations and argument validation of the fused
batch-norm + ReLU + pair-maximum kernels (csrc/multiscale.hip)."""
import ctypes
import os
import re

import pytest
import torch

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

KERNELS = ("yt8m_multiscale_workspace_bytes", "yt8m_colmoments_f32", "yt8m_bn_relu_pool2_tm_fwd", "yt8m_bn_relu_pool2_tm_bwd")


def _build(cls_name, monkeypatch, nf, B=4, F=300, D=1152, H=1024, layers=4, M=4, V=5, **kw):
    """Builds the plugin on the CPU graph with the native calls stubbed out: variable creation, shapes and the frame bookkeeping are
    under test, not arithmetic."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.multiscale_cnn_lstm_layers, FLAGS.moe_num_mixtures = str(H), layers, M
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    stacks = []

    def stack(x_tm, num_frames, wb, **k):
        stacks.append((tuple(x_tm.shape), [int(v) for v in num_frames], k.get("slot")))
        return torch.zeros(x_tm.shape[0], x_tm.shape[1], H), [(torch.zeros(x_tm.shape[1], H), torch.zeros(x_tm.shape[1], H)) for _ in wb]

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: torch.zeros(x.shape[0], W.data.shape[1]))
    monkeypatch.setattr(ops, "batch_norm", lambda x, *a, **k: x)
    monkeypatch.setattr(ops, "activation", lambda x, kind: x)
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: x)
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V_, M_, **k: torch.zeros(x.shape[0], V_))
    try:
        res = getattr(flm, cls_name)().create_model(torch.zeros(B, F, D), vocab_size=V, num_frames=torch.tensor(nf), unknown_kwarg=1, **kw)
    finally:
        FLAGS.reset()
    return {k: tuple(v.data.shape) for k, v in g.vars.items()}, res, stacks


def _want(D=1152, H=1024, layers=4, M=4, V=5, head_extra=0):
    want = {}
    for k in range(1, layers + 1):
        d = D if k == 1 else 1024
        for fs, nfl in ((1, 256), (2, 256), (3, 512)):
            want["cnn%dcnn-filter-len%d" % (k, fs)] = (d * fs, nfl)
        for n in ("gamma", "beta", "moving_mean", "moving_variance"):
            want["cnn%dcluster_bn/%s" % (k, n)] = (1024,)
        want["RNN-rnn%d/basic_lstm_cell/weights" % k] = (1024 + H, 4 * H)
        want["RNN-rnn%d/basic_lstm_cell/biases" % k] = (4 * H,)
        want["gatesmoe%d/weights" % k] = (H + head_extra, V * (M + 1))
        want["expertsmoe%d/weights" % k] = (H + head_extra, V * M)
        want["expertsmoe%d/biases" % k] = (V * M,)
    return want


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in ("MultiscaleCnnLstmModel", "DistillchainMultiscaleCnnLstmModel"):
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name)
        assert cls.accepts_quantized_input is True


def test_flag_defaults_follow_the_reference():
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flags)
    from yt8m_amd.flags import FLAGS
    FLAGS.reset()
    assert FLAGS.multiscale_cnn_lstm_layers == 1 and FLAGS.distillchain_relu_cells == 256


def test_variable_names_shapes_and_frame_chain(monkeypatch):
    nf = [300, 1, 0, 5]
    shapes, res, stacks = _build("MultiscaleCnnLstmModel", monkeypatch, nf)
    assert shapes == _want()
    assert tuple(res["predictions"].shape) == (4, 5)
    assert tuple(res["support_predictions"].shape) == (4, 4 * 5)
    assert [s[0][0] for s in stacks] == [300, 150, 75, 37]
    assert all(s[0][1:] == (4, 1024) for s in stacks)                # time-major [F_k, B, 1024]
    chain = [nf]
    for _ in range(3):
        chain.append([max(n // 2, 1) for n in chain[-1]])
    assert [s[1] for s in stacks] == chain
    assert chain[1] == [150, 1, 1, 2] and chain[3] == [37, 1, 1, 1]
    assert [s[2] for s in stacks] == [0, 1, 2, 3]                    # stacks alive in one step own separate buffers


def test_distillchain_variable_names_and_assertion(monkeypatch):
    with pytest.raises(AssertionError):
        _build("DistillchainMultiscaleCnnLstmModel", monkeypatch, [300, 1, 0, 5])
    shapes, res, _ = _build("DistillchainMultiscaleCnnLstmModel", monkeypatch, [300, 1, 0, 5], layers=2,
                            distillation_predictions=torch.zeros(4, 5))
    want = _want(layers=2, head_extra=256)
    want["distillrelu/weights"] = (5, 256)
    want["distillrelu/biases"] = (256,)
    assert shapes == want
    assert tuple(res["support_predictions"].shape) == (4, 2 * 5)


def test_header_declares_the_multiscale_kernels():
    _, lib = declared_bound_exported(KERNELS, r"(int|int64_t)")
    assert lib.yt8m_abi_version() == 4                           # symbols were added, nothing else moved


def test_multiscale_argument_validation_without_device():
    lib = L.lib()
    one = ctypes.c_void_p(16)                                        # never dereferenced: validation fails first
    n = lib.yt8m_multiscale_workspace_bytes(1024)
    assert n >= 2 * 1024 * 4 and lib.yt8m_multiscale_workspace_bytes(0) == 0
    mom = lambda y, M, C, ld, mm=one, ws=one, wsb=None: lib.yt8m_colmoments_f32(
        y, M, C, ld, mm, one, 1, 1e-3, 0.999, one, one, ws, n if wsb is None else wsb, None)
    assert mom(one, -1, 8, 8) == -2
    assert mom(one, 4, 6, 8) == -2                                   # C % 4
    assert mom(one, 4, 8, 4) == -2                                   # ldy < C
    assert mom(None, 4, 8, 8) == -1
    assert mom(one, 4, 8, 8, mm=None) == -1
    assert mom(one, 4, 8, 8, wsb=16) == -2                           # workspace too small
    assert mom(None, 0, 8, 8, mm=None, ws=None) == 0 and mom(None, 4, 0, 0, mm=None, ws=None) == 0
    fwd = lambda y, F, B, C, ld, a=one, p=one: lib.yt8m_bn_relu_pool2_tm_fwd(y, ld, F, B, C, one, one, one, one, a, C, p, C, None)
    two, three = ctypes.c_void_p(32), ctypes.c_void_p(48)
    assert fwd(one, -1, 2, 8, 8) == -2 and fwd(one, 3, -2, 8, 8) == -2
    assert fwd(one, 3, 2, 6, 8) == -2
    assert fwd(one, 3, 2, 8, 4) == -2
    assert fwd(None, 3, 2, 8, 8, a=two, p=three) == -1
    assert fwd(one, 3, 2, 8, 8, a=None, p=three) == -1
    assert fwd(one, 3, 2, 8, 8, a=one, p=None) == -1                 # in place
    assert fwd(ctypes.c_void_p(20), 3, 2, 8, 8, a=two, p=None) == -1  # not 16-byte aligned
    assert fwd(None, 0, 2, 8, 8, a=None, p=None) == 0 and fwd(None, 3, 0, 8, 8, a=None, p=None) == 0
    bwd = lambda y, F, B, C, ld, da=two, dp=None, dy=three, ws=ctypes.c_void_p(64), wsb=None: lib.yt8m_bn_relu_pool2_tm_bwd(
        y, ld, F, B, C, one, one, one, one, 1, da, C, dp, C, dy, C, None, 0.0, None, 0.0, ws, n if wsb is None else wsb, None)
    assert bwd(one, -1, 2, 8, 8) == -2
    assert bwd(one, 3, 2, 6, 8) == -2
    assert bwd(one, 3, 2, 8, 4) == -2
    assert bwd(None, 3, 2, 8, 8) == -1
    assert bwd(one, 3, 2, 8, 8, da=None, dp=None) == -1              # no gradient at all
    assert bwd(one, 3, 2, 8, 8, ws=None) == -1
    assert bwd(one, 3, 2, 8, 8, dy=one) == -1                        # dy may replace da, never y
    assert bwd(one, 3, 2, 8, 8, wsb=16) == -2
    assert bwd(None, 0, 2, 8, 8, da=None, dy=None, ws=None) == 0
