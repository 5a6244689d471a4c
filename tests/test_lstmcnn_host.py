"""CPU checks of the LSTM + CNN chain plugins (W/all_frame_models/lstm_cnn_deep_combine_chain_model.py,
distillchain_lstm_cnn_deep_combine_chain_model.py): the lookup by name, the variable names and shapes, the stacks' slots, and the C-ABI
declarations and argument validation of the pooled CNN's gather kernels (csrc/cnn_pool_f32.hip)."""
import ctypes
import os
import re

import pytest
import torch

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

KERNELS = ("yt8m_f32_cnn_pool_dw", "yt8m_f32_cnn_pool_dx")
NAMES = ("LstmCnnDeepCombineChainModel", "DistillchainLstmCnnDeepCombineChainModel")


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in NAMES:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name)
        assert cls.accepts_quantized_input is True


def test_library_exports_and_header_declares_the_gather_kernels():
    _, lib = declared_bound_exported(KERNELS)
    assert lib.yt8m_abi_version() == 4                               # symbols were added, nothing else moved


def _build(cls_name, monkeypatch, B=4, F=300, c=128, layers=3, M=4, V=5, **kw):
    """The plugin on the CPU graph with the native calls stubbed out: variable creation, shapes and the stacks' bookkeeping."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.feature_sizes, FLAGS.lstm_layers = "1024,128", "1024,128", 1
    FLAGS.deep_chain_layers, FLAGS.deep_chain_relu_cells, FLAGS.moe_num_mixtures = layers, c, M
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    stacks, pooled_calls, heads = [], [], []

    def stack(x_tm, num_frames, wb, **k):
        H = wb[0][0].data.shape[1] // 4
        stacks.append((tuple(x_tm.shape), H, k.get("slot")))
        return torch.zeros(x_tm.shape[0], x_tm.shape[1], H), [(torch.zeros(x_tm.shape[1], H), torch.zeros(x_tm.shape[1], H)) for _ in wb]

    def pooled(x2d, B_, cnns):
        pooled_calls.append((tuple(x2d.shape), B_, [[tuple(W.data.shape) for W in cnn] for cnn in cnns]))
        return [torch.zeros(B_, sum(W.data.shape[1] for W in cnn)) for cnn in cnns]

    def head(x, Wg, We, be, V_, M_, **k):
        heads.append(x.shape[1])
        return torch.zeros(x.shape[0], V_)

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(seq_ops, "cnn_tm_maxpool", pooled)
    monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: torch.zeros(x.shape[0], W.data.shape[1]))
    monkeypatch.setattr(ops, "activation", lambda x, kind: x)
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: x)
    monkeypatch.setattr(ops, "moe_head", head)
    try:
        res = getattr(flm, cls_name)().create_model(torch.zeros(B, F, 1152), vocab_size=V, num_frames=torch.tensor([300, 1, 7, 5]),
                                                    unknown_kwarg=1, **kw)
    finally:
        FLAGS.reset()
    return {k: tuple(v.data.shape) for k, v in g.vars.items()}, res, stacks, pooled_calls, heads


def _want(c=128, layers=3, M=4, V=5, extra=0, first_stage_reads_relu=False):
    want = {}
    for i, (d, h) in enumerate(((1024, 1024), (128, 128))):
        want["RNN%d/multi_rnn_cell/cell_0/basic_lstm_cell/weights" % i] = (d + h, 4 * h)
        want["RNN%d/multi_rnn_cell/cell_0/basic_lstm_cell/biases" % i] = (4 * h,)
    want["mean-relu/weights"], want["mean-relu/biases"] = (1152, c), (c,)
    for k in range(layers + 1):
        for fs, n in zip((1, 2, 3), (c, 2 * c, c) if k == 0 else (c, c, 2 * c)):
            want["cnn%dcnn-filter-len%d" % (k, fs)] = (1152 * fs, n)
    widths = []
    for l in range(layers + 1):
        scope = "prediction-%d" % l if l < layers else "-main"
        d_in = 4 * c + ((extra + c * (l + 1)) if (l > 0 or first_stage_reads_relu) else 0)
        widths.append(d_in)
        want["gates-%s/weights" % scope] = (d_in, V * (M + 1))
        want["experts-%s/weights" % scope] = (d_in, V * M)
        want["experts-%s/biases" % scope] = (V * M,)
        if l < layers:
            want["relu-%d/weights" % l], want["relu-%d/biases" % l] = (V, c), (c,)
    return want, widths


def test_variable_names_shapes_and_stack_slots(monkeypatch):
    shapes, res, stacks, pooled_calls, heads = _build("LstmCnnDeepCombineChainModel", monkeypatch)
    want, widths = _want()
    assert shapes == want
    assert heads == widths == [512, 768, 896, 1024]                  # stage 0 reads cnn0 alone; no mean_input columns anywhere
    assert tuple(res["predictions"].shape) == (4, 5) and tuple(res["support_predictions"].shape) == (4, 3 * 5)
    assert stacks == [((300, 4, 1024), 1024, 0), ((300, 4, 128), 128, 1)]          # float frames time-major; both alive: own slots
    assert len(pooled_calls) == 1                                    # ONE op for the whole chain, on time-major rows
    assert pooled_calls[0][0] == (300 * 4, 1152) and pooled_calls[0][1] == 4 and len(pooled_calls[0][2]) == 4


def test_distillchain_variable_names_and_assertion(monkeypatch):
    with pytest.raises(AssertionError):
        _build("DistillchainLstmCnnDeepCombineChainModel", monkeypatch)
    shapes, res, _, _, heads = _build("DistillchainLstmCnnDeepCombineChainModel", monkeypatch, layers=2,
                                      distillation_predictions=torch.zeros(4, 5))
    want, widths = _want(layers=2, extra=256, first_stage_reads_relu=True)
    want["distillrelu/weights"], want["distillrelu/biases"] = (5, 256), (256,)
    assert shapes == want
    assert heads == widths == [512 + 256 + 128, 512 + 256 + 256, 512 + 256 + 384]
    assert tuple(res["support_predictions"].shape) == (4, 2 * 5)


def test_parallel_plugin_keeps_its_slots(monkeypatch):
    """LstmParallelFinaloutputModel shares the stacks' loop with the new plugins and still passes no slot of its own."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.feature_sizes, FLAGS.lstm_layers = "64,32", "48,16", 2
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: x)
    reset_default_graph(device=torch.device("cpu"), seed=0)
    seen = []

    def stack(x_tm, num_frames, wb, **k):
        H = wb[0][0].data.shape[1] // 4
        seen.append((tuple(x_tm.shape), k.get("slot", 0)))
        return torch.zeros(x_tm.shape[0], x_tm.shape[1], H), [(torch.zeros(x_tm.shape[1], H), torch.zeros(x_tm.shape[1], H)) for _ in wb]

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    got = {}
    monkeypatch.setattr(flm, "_head", lambda name=None: (lambda: type("Head", (), {
        "create_model": lambda self, model_input, **kw: got.setdefault("state", model_input)})()))
    try:
        flm.LstmParallelFinaloutputModel().create_model(torch.rand(2, 3, 64), vocab_size=5, num_frames=torch.tensor([3, 1]))
    finally:
        FLAGS.reset()
    assert seen == [((3, 2, 48), 0), ((3, 2, 16), 0)]
    assert tuple(got["state"].shape) == (2, 2 * 64 + 2 * 32)


def test_gather_kernels_argument_validation_without_device():
    lib = L.lib()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    dw = lambda x=one, ldx=8, idx=one, g=one, ldg=8, B=2, F=3, D=8, N=8, fs=2, out=two, ldw=8, beta=0.0: lib.yt8m_f32_cnn_pool_dw(
        x, ldx, idx, g, ldg, B, F, D, N, fs, out, ldw, beta, None)
    assert dw(B=-1) == -2 and dw(F=0) == -2 and dw(fs=0) == -2 and dw(fs=17) == -2
    assert dw(D=6) == -2 and dw(D=4100, ldx=4100) == -2              # D % 4, D <= 4096
    assert dw(ldx=4) == -2 and dw(ldx=10) == -2 and dw(ldg=4) == -2 and dw(ldw=4) == -2
    assert dw(beta=0.5) == -1
    assert dw(x=None) == -1 and dw(idx=None) == -1 and dw(g=None) == -1 and dw(out=None) == -1
    assert dw(x=ctypes.c_void_p(20)) == -1                           # not 16-byte aligned
    assert dw(N=0, x=None, idx=None, g=None, out=None) == 0          # an empty problem is a no-op
    fs_ = (ctypes.c_int32 * 2)(1, 3)
    nc_ = (ctypes.c_int32 * 2)(4, 4)
    wt_ = (ctypes.c_void_p * 2)(64, 128)
    dx = lambda idx=one, g=one, ldg=8, B=2, F=3, D=8, n=2, wt=wt_, fs=fs_, nc=nc_, out=two, ldd=8: lib.yt8m_f32_cnn_pool_dx(
        idx, g, ldg, B, F, D, n, wt, fs, nc, out, ldd, None)
    assert dx(B=-1) == -2 and dx(F=0) == -2 and dx(n=0) == -2 and dx(n=33) == -2
    assert dx(fs=(ctypes.c_int32 * 2)(1, 17)) == -2 and dx(nc=(ctypes.c_int32 * 2)(4, 0)) == -2
    assert dx(wt=(ctypes.c_void_p * 2)(64, None)) == -1 and dx(wt=(ctypes.c_void_p * 2)(64, 132)) == -1
    assert dx(D=7) == -2 and dx(D=2050, ldd=2050) == -2 and dx(ldd=6) == -2 and dx(ldd=9) == -2 and dx(ldg=4) == -2
    assert dx(F=20000) == -2                                         # the sort's keys do not fit the LDS
    assert dx(idx=None) == -1 and dx(g=None) == -1 and dx(out=None) == -1 and dx(out=ctypes.c_void_p(36)) == -1
    assert dx(B=0, idx=None, g=None, out=None) == 0
