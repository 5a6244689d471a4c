"""CPU checks of the four Distillchain cascade plugins (W/all_video_models/distillchain_deep_combine_chain_model.py,
W/all_frame_models/distillchain_{lstm_parallel_finaloutput,cnn_deep_combine_chain,lstm_attention_max_pooling}_model.py) and of the
fused link kernel's C ABI (csrc/chain_link.hip): the lookup by name, the header / signature table / exports, argument validation
without a device, and every plugin built on the CPU graph with the native calls stubbed out -- variable names and shapes, the width of
every stage's input, the reference's assertion."""
import ctypes
import os
import re

import pytest
import torch

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

KERNELS = ("yt8m_chain_link_fwd", "yt8m_chain_link_bwd")
FRAME = ("DistillchainLstmParallelFinaloutputModel", "DistillchainCnnDeepCombineChainModel", "DistillchainLstmAttentionMaxPoolingModel")
VIDEO = ("DistillchainDeepCombineChainModel",)


def test_find_class_by_name_resolves_the_four_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in FRAME:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True
    for name in VIDEO:
        assert train.find_class_by_name(name, [flm, vlm]) is getattr(vlm, name) and not hasattr(flm, name)


def test_library_exports_and_header_declares_the_link_kernels():
    _, lib = declared_bound_exported(KERNELS)
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_link_kernels_argument_validation_without_device():
    lib = L.lib()
    a, b, c, d, e = (ctypes.c_void_p(16 * k) for k in range(1, 6))
    fwd = lambda act=1, z=a, y=b, rinv=c, rows=2, cols=8, eps=1e-12, stddev=0.0, seed=1, offset=0: lib.yt8m_chain_link_fwd(
        act, z, y, rinv, rows, cols, eps, stddev, seed, offset, None)
    bwd = lambda act=1, z=a, y=b, rinv=c, dy=d, dz=e, rows=2, cols=8, eps=1e-12: lib.yt8m_chain_link_bwd(
        act, z, y, rinv, dy, dz, rows, cols, eps, None)
    for call in (fwd, bwd):
        for act in (0, 2, 3, 5, -1):                                     # sigmoid, relu6, tanh, unknown: only relu (1) and elu (4)
            assert call(act=act) == -1, act
        assert call(rows=0) == -1 and call(rows=-3) == -1 and call(cols=0) == -1 and call(cols=-1) == -1
        assert call(z=None) == -1 and call(y=None) == -1 and call(rinv=None) == -1
        assert call(eps=0.0) == -1
    assert bwd(dy=None) == -1 and bwd(dz=None) == -1
    assert fwd(stddev=-0.5) == -1 and fwd(stddev=float("nan")) == -1 and fwd(offset=-4) == -1


# ---- the plugins on the CPU graph ---------------------------------------------------------------------------------------------------
class _Stubs(object):
    """The native calls replaced by shape-only stand-ins; records what the plugins asked for."""

    def __init__(self, monkeypatch):
        import yt8m_amd.ops as ops
        import yt8m_amd.seq_ops as seq_ops
        self.stacks, self.heads, self.links = [], [], []

        def stack(x_tm, num_frames, wb, **k):
            H = wb[0][0].data.shape[1] // 4
            self.stacks.append((tuple(x_tm.shape), H, len(wb)))
            return torch.zeros(x_tm.shape[0], x_tm.shape[1], H), [(torch.zeros(x_tm.shape[1], H), torch.zeros(x_tm.shape[1], H)) for _ in wb]

        def head(x, Wg, We, be, V_, M_, **k):
            self.heads.append((x.shape[1], k.get("dx_from", 0)))
            return torch.zeros(x.shape[0], V_)

        def link(z, kind="relu", noise_level=None, seed=None, offset=0, eps=1e-12, graph=None):
            self.links.append((tuple(z.shape), kind, noise_level))
            return z

        def no_composed_form(*a, **k):
            raise AssertionError("a relu -> l2norm of the new plugins left ops.chain_link")

        monkeypatch.setattr(seq_ops, "lstm_stack", stack)
        monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: torch.zeros(x.shape[0], W.data.shape[1]))
        monkeypatch.setattr(ops, "linear_cat", lambda parts, W, b=None, group_parts=(): torch.zeros(parts[0].shape[:-1] + (W.data.shape[1],)))
        monkeypatch.setattr(ops, "moe_head", head)
        monkeypatch.setattr(ops, "chain_link", link)
        monkeypatch.setattr(ops, "activation", no_composed_form)
        monkeypatch.setattr(ops, "add_noise", no_composed_form)
        monkeypatch.setattr(ops, "dropout", lambda x, keep_prob, **k: x)
        monkeypatch.setattr(ops, "frame_pool", lambda x, method: x.amax(1))
        monkeypatch.setattr(seq_ops, "attention_weights", lambda act, nf: act)
        monkeypatch.setattr(seq_ops, "pool_tn", lambda w, out: torch.zeros(w.shape[0], w.shape[2], out.shape[2]))
        self.ops = ops


def _shapes(g):
    return {k: tuple(v.data.shape) for k, v in g.vars.items()}


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


B, F, V, M = 4, 6, 5, 3
NF = torch.tensor([6, 1, 3, 5])


def _moe_vars(want, scope, d_in):
    want["gates-%s/weights" % scope] = (d_in, V * (M + 1))
    want["experts-%s/weights" % scope] = (d_in, V * M)
    want["experts-%s/biases" % scope] = (V * M,)


def test_video_level_plugin_on_the_cpu_graph(monkeypatch, flags):
    import yt8m_amd.video_level_models as vlm
    stubs = _Stubs(monkeypatch)
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.moe_num_mixtures = 2, 12, M
    flags.distillchain_relu_cells, flags.deep_chain_relu_type = 7, "elu"  # distillrelu is deep_chain_relu_cells wide HERE, not 7
    D = 20
    _graph()
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        vlm.DistillchainDeepCombineChainModel().create_model(torch.zeros(B, D), vocab_size=V)
    g = _graph()
    res = vlm.DistillchainDeepCombineChainModel().create_model(torch.zeros(B, D), vocab_size=V, noise_level=0.25, dropout=True, keep_prob=0.5,
                                                               distillation_predictions=torch.zeros(B, V, dtype=torch.float64), unknown=1)
    want = {"distillrelu/weights": (V, 12), "distillrelu/biases": (12,)}
    widths = [D + 12, D + 24, D + 36]                                    # [model_input | distill_norm | relu-0 ...]
    for l, w in enumerate(widths):
        _moe_vars(want, "prediction-%d" % l if l < 2 else "-main", w)
        if l < 2:
            want["relu-%d/weights" % l], want["relu-%d/biases" % l] = (V, 12), (12,)
    assert _shapes(g) == want
    assert stubs.heads == [(w, D) for w in widths]                       # the data input in front is frozen: no dx for its D columns
    assert stubs.links == [((B, 12), "relu", None), ((B, 12), "elu", 0.25), ((B, 12), "elu", 0.25)]
    assert tuple(res["predictions"].shape) == (B, V) and tuple(res["support_predictions"].shape) == (B, 2 * V)
    g = _graph()
    vlm.DistillchainDeepCombineChainModel().create_model(torch.zeros(B, D), vocab_size=V, sub_scope="x-",
                                                         distillation_predictions=torch.zeros(B, V))
    assert "x-distillrelu/weights" in g.vars and "gates-x--main/weights" in g.vars


def test_parallel_finaloutput_plugin_on_the_cpu_graph(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    monkeypatch.setattr(stubs.ops, "l2_normalize", lambda x, eps=1e-12: x)         # the parent's per-slice normalisation of float frames
    flags.lstm_cells, flags.feature_sizes, flags.lstm_layers = "16,8", "12,4", 2
    flags.distillchain_relu_cells, flags.deep_chain_relu_cells, flags.moe_num_mixtures = 10, 99, M
    x = torch.zeros(B, F, 16)
    _graph()
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        flm.DistillchainLstmParallelFinaloutputModel().create_model(x, vocab_size=V, num_frames=NF)
    g = _graph()
    res = flm.DistillchainLstmParallelFinaloutputModel().create_model(x, vocab_size=V, num_frames=NF,
                                                                      distillation_predictions=torch.zeros(B, V), unknown=1)
    want = {"distillrelu/weights": (V, 10), "distillrelu/biases": (10,)}
    for i, (d, h) in enumerate(((12, 16), (4, 8))):
        for l in range(2):
            want["RNN%d/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (i, l)] = ((d if l == 0 else h) + h, 4 * h)
            want["RNN%d/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (i, l)] = (4 * h,)
    width = 2 * 16 + 2 * 8 + 10                                          # final h of every layer of every stack | distill_norm
    want["gates/weights"], want["experts/weights"], want["experts/biases"] = (width, V * (M + 1)), (width, V * M), (V * M,)
    assert _shapes(g) == want
    assert stubs.heads == [(width, 0)] and stubs.links == [((B, 10), "relu", None)]
    assert stubs.stacks == [((F, B, 12), 16, 2), ((F, B, 4), 8, 2)]
    assert tuple(res["predictions"].shape) == (B, V)


def test_cnn_chain_plugin_on_the_cpu_graph(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    monkeypatch.setattr(stubs.ops, "l2_normalize", lambda x, eps=1e-12: x)         # the pooled CNN's normalisation (the parent's op)
    c, D = 8, 9
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.distillchain_relu_cells, flags.moe_num_mixtures = 2, c, 10, M
    x = torch.zeros(B, F, D)
    _graph()
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        flm.DistillchainCnnDeepCombineChainModel().create_model(x, vocab_size=V, num_frames=NF)
    g = _graph()
    res = flm.DistillchainCnnDeepCombineChainModel().create_model(x, vocab_size=V, num_frames=NF,
                                                                  distillation_predictions=torch.zeros(B, V), unknown=1)
    want = {"distillrelu/weights": (V, 10), "distillrelu/biases": (10,), "mean-relu/weights": (D, c), "mean-relu/biases": (c,)}
    for k in range(3):
        for fs, n in zip((1, 2, 3), (c, c, 2 * c)):
            want["cnn%dcnn-filter-len%d" % (k, fs)] = (D * fs, n)
    widths = [4 * c + 10 + c * (l + 1) for l in range(3)]               # [cnn_l | distill_norm | mean_relu_norm | relu-0 ...]: no mean_input
    for l, w in enumerate(widths):
        _moe_vars(want, "prediction-%d" % l if l < 2 else "-main", w)
        if l < 2:
            want["relu-%d/weights" % l], want["relu-%d/biases" % l] = (V, c), (c,)
    assert _shapes(g) == want
    assert stubs.heads == [(w, 0) for w in widths]
    assert stubs.links == [((B, 10), "relu", None)] + [((B, c), "relu", None)] * 3
    assert tuple(res["support_predictions"].shape) == (B, 2 * V)


def test_attention_plugin_on_the_cpu_graph(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    H, A, D = 8, 3, 9
    flags.lstm_cells, flags.lstm_layers, flags.lstm_attentions = str(H), 2, A
    flags.distillchain_relu_cells, flags.deep_chain_relu_cells, flags.moe_num_mixtures = 10, 99, M
    x = torch.zeros(B, F, D)
    _graph()
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        flm.DistillchainLstmAttentionMaxPoolingModel().create_model(x, vocab_size=V, num_frames=NF)
    g = _graph()
    model = flm.DistillchainLstmAttentionMaxPoolingModel()
    res = model.create_model(x, vocab_size=V, num_frames=NF, distillation_predictions=torch.zeros(B, V), unknown=1)
    want = {"distillrelu/weights": (V, 10), "distillrelu/biases": (10,), "attention-/weights": (D + H, A), "attention-/biases": (A,)}
    for l in range(2):
        want["RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % l] = ((D if l == 0 else H) + H, 4 * H)
        want["RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % l] = (4 * H,)
    _moe_vars(want, "sub-moe", H + 10)                                   # [attention output | distill_norm] on each of the A rows of a video
    assert _shapes(g) == want
    assert stubs.heads == [(H + 10, 0)] and stubs.links == [((B, 10), "relu", None)]
    assert tuple(res["predictions"].shape) == (B, V)
    assert model._distill_norm is None                                   # nothing of the step is kept on the model object
    # the tiling itself: row a of video b reads video b's distill_norm behind its attention output
    model._distill_norm = torch.arange(B * 2, dtype=torch.float32).view(B, 2)
    got = model._moe_input(torch.zeros(B, A, H))
    assert tuple(got.shape) == (B, A, H + 2)
    assert torch.equal(got[:, :, H:], model._distill_norm[:, None, :].expand(B, A, 2)) and bool((got[:, :, :H] == 0).all())
    # the parent's path is unchanged by the hook
    g = _graph()
    stubs.heads[:] = []
    flm.LstmAttentionMaxPoolingModel().create_model(x, vocab_size=V, num_frames=NF)
    assert stubs.heads == [(H, 0)] and "distillrelu/weights" not in g.vars
