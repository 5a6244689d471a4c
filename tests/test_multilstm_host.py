"""CPU checks of the multi-LSTM chain plugins (W/all_frame_models/lstm_memory_deep_chain_model.py,
distillchain_lstm_memory_deep_combine_chain_model.py, lstm_parallel_memory_model.py) and of the fused memory-link kernel's C ABI
(csrc/memory_link.hip): the lookup by name, the header / signature table / exports, argument validation without a device, and every
plugin built on the CPU graph with the native calls stubbed out -- variable names and shapes, the number of stacks and their slots, the
stack input prepared once, the width of every stage's input, the reference's assertion."""
import ctypes
import os
import re

import pytest
import torch

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

KERNELS = ("yt8m_memory_link_fwd", "yt8m_memory_link_bwd")
PLUGINS = ("LstmMemoryDeepChainModel", "DistillchainLstmMemoryDeepCombineChainModel", "LstmParallelMemoryModel")


def test_find_class_by_name_resolves_the_three_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True


def test_library_exports_and_header_declares_the_memory_link_kernels():
    _, lib = declared_bound_exported(KERNELS)
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _widths(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def test_memory_link_argument_validation_without_device():
    """Every call here fails validation (or has nothing to do), so nothing is launched and no device is needed."""
    lib = L.lib()
    y, rinv, dy = (ctypes.c_void_p(16 * k) for k in range(1, 4))
    two, w2 = _ptrs(64, 80), _widths(8, 4)
    fwd = lambda nseg=2, src=two, widths=w2, normalize=1, y=y, rinv=rinv, rows=2, eps=1e-12: lib.yt8m_memory_link_fwd(
        nseg, src, widths, normalize, y, rinv, rows, eps, None)
    bwd = lambda nseg=2, widths=w2, normalize=1, y=y, rinv=rinv, dy=dy, dsrc=two, rows=2, eps=1e-12: lib.yt8m_memory_link_bwd(
        nseg, widths, normalize, y, rinv, dy, dsrc, rows, eps, None)
    many, wmany = _ptrs(*[64 + 16 * k for k in range(17)]), _widths(*[4] * 17)
    for call in (fwd, bwd):
        assert call(nseg=0) == -1 and call(nseg=-1) == -1                  # nseg out of range
        for normalize in (0, 1):
            assert call(normalize=normalize, rows=0) == -1 and call(normalize=normalize, rows=-3) == -1
            assert call(normalize=normalize, widths=_widths(8, 0)) == -1 and call(normalize=normalize, widths=_widths(-4, 8)) == -1
            assert call(normalize=normalize, widths=None) == -1
            assert call(normalize=normalize, eps=0.0) == -1 and call(normalize=normalize, eps=-1e-12) == -1
        assert call(rinv=None) == -1                                       # rinv == NULL with normalize
        assert call(y=None) == -1
    assert fwd(nseg=17, src=many, widths=wmany) == -1 and bwd(nseg=17, dsrc=many, widths=wmany) == -1
    assert fwd(src=None) == -1 and fwd(src=_ptrs(64, None)) == -1 and fwd(src=_ptrs(None, 80)) == -1
    assert fwd(normalize=0, y=None) == -1 and fwd(normalize=0, rinv=None, src=_ptrs(64, None)) == -1
    assert bwd(dy=None) == -1 and bwd(dsrc=None) == -1 and bwd(normalize=0, dy=None) == -1
    # no gradient wanted for any segment: valid, nothing to launch
    assert bwd(dsrc=_ptrs(None, None)) == 0 and bwd(normalize=0, y=None, rinv=None, dsrc=_ptrs(None, None)) == 0


def test_op_refuses_more_than_sixteen_tensors_and_has_no_cpu_form(monkeypatch):
    import yt8m_amd.ops as ops
    with pytest.raises(ValueError):
        ops.memory_link([torch.zeros(2, 4)] * 17, normalize=False)
    with pytest.raises(ValueError):
        ops.memory_link([], normalize=True)
    monkeypatch.setattr(ops, "MEMORY_LINK_FUSED", True)
    with pytest.raises(L.Yt8mHipError):                                   # a missing device is an error, not a fall-back to torch.cat
        ops.memory_link([torch.zeros(2, 4), torch.zeros(2, 8)], normalize=False)


# ---- the plugins on the CPU graph ---------------------------------------------------------------------------------------------------
class _Stubs(object):
    """The native calls replaced by shape-only stand-ins; records what the plugins asked for."""

    def __init__(self, monkeypatch):
        import yt8m_amd.frame_level_models as flm
        import yt8m_amd.ops as ops
        import yt8m_amd.seq_ops as seq_ops
        self.stacks, self.heads, self.links, self.memory_links, self.inputs, self.dequants = [], [], [], [], [], []

        def stack(x_tm, num_frames, wb, **k):
            H = wb[0][0].data.shape[1] // 4
            self.stacks.append((tuple(x_tm.shape), H, len(wb), k.get("slot", 0)))
            self.inputs.append(x_tm)
            return torch.zeros(x_tm.shape[0], x_tm.shape[1], H), [(torch.zeros(x_tm.shape[1], H), torch.zeros(x_tm.shape[1], H)) for _ in wb]

        def head(x, Wg, We, be, V_, M_, **k):
            self.heads.append((x.shape[1], k.get("dx_from", 0)))
            return torch.zeros(x.shape[0], V_)

        def link(z, kind="relu", noise_level=None, seed=None, offset=0, eps=1e-12, graph=None):
            self.links.append((tuple(z.shape), kind, noise_level))
            return z

        def memory_link(tensors, normalize, eps=1e-12):
            tensors = list(tensors)
            self.memory_links.append(([t.shape[1] for t in tensors], bool(normalize)))
            return torch.zeros(tensors[0].shape[0], sum(t.shape[1] for t in tensors))

        def dequant(q, num_frames=None):
            self.dequants.append(tuple(q.shape))
            return torch.zeros(q.shape, dtype=torch.float32)

        def no_composed_form(*a, **k):
            raise AssertionError("a relu -> l2norm or a normalised concatenation of the new plugins left ops.chain_link / ops.memory_link")

        self.stack_inputs = []
        stack_input = flm._stack_input

        def counted_stack_input(*a, **k):
            self.stack_inputs.append(a[0].dtype)
            return stack_input(*a, **k)

        monkeypatch.setattr(flm, "_stack_input", counted_stack_input)
        monkeypatch.setattr(seq_ops, "lstm_stack", stack)
        monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: torch.zeros(x.shape[0], W.data.shape[1]))
        monkeypatch.setattr(ops, "moe_head", head)
        monkeypatch.setattr(ops, "chain_link", link)
        monkeypatch.setattr(ops, "memory_link", memory_link)
        monkeypatch.setattr(ops, "dequant_l2norm", dequant)
        monkeypatch.setattr(ops, "activation", no_composed_form)
        monkeypatch.setattr(ops, "l2_normalize", no_composed_form)
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


def _stack_vars(want, scope, D, H, layers):
    for l in range(layers):
        want["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)] = ((D if l == 0 else H) + H, 4 * H)
        want["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)] = (4 * H,)


def _bytes(D):
    return torch.zeros(B, F, D, dtype=torch.uint8)


@pytest.mark.parametrize("u8", [False, True])
def test_memory_deep_chain_plugin_on_the_cpu_graph(monkeypatch, flags, u8):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    H, LL, c, D = 8, 2, 7, 9                                             # D = 9: no byte projection, the float fallback
    flags.lstm_cells, flags.lstm_layers, flags.deep_chain_layers, flags.deep_chain_relu_cells = str(H), LL, 2, c
    flags.moe_num_mixtures, flags.distillchain_relu_cells = M, 99
    assert not flm._lib_u8_ok(D)
    g = _graph()
    res = flm.LstmMemoryDeepChainModel().create_model(_bytes(D) if u8 else torch.zeros(B, F, D), vocab_size=V, num_frames=NF, unknown=1)
    want = {}
    for k in range(3):
        _stack_vars(want, "lstm-%d-RNN" % k, D, H, LL)
    for l, w in enumerate([LL * H, LL * H + c, LL * H + c]):             # stage l + 1 sees only the LATEST relu
        _moe_vars(want, "prediction-%d" % l if l < 2 else "-main", w)
        if l < 2:
            want["relu-%d/weights" % l], want["relu-%d/biases" % l] = (V, c), (c,)
    assert _shapes(g) == want
    assert stubs.heads == [(LL * H, 0), (LL * H + c, 0), (LL * H + c, 0)]
    assert stubs.stacks == [((F, B, D), H, LL, k) for k in range(3)]     # three stacks over the whole input, slots 0, 1, 2
    assert stubs.memory_links == [([H] * LL, False)] * 3 and stubs.links == [((B, c), "relu", None)] * 2
    # the stack input is prepared once: one call, one dequantised tensor, the very same object under every stack
    assert len(stubs.stack_inputs) == 1 and stubs.dequants == ([(B, F, D)] if u8 else [])
    assert all(x is stubs.inputs[0] for x in stubs.inputs)
    assert tuple(res["predictions"].shape) == (B, V) and tuple(res["support_predictions"].shape) == (B, 2 * V)
    g = _graph()
    flm.LstmMemoryDeepChainModel().create_model(torch.zeros(B, F, D), vocab_size=V, num_frames=NF, sub_scope="x-")
    assert "gates-x-prediction-0/weights" in g.vars and "x-relu-1/weights" in g.vars and "lstm-2-RNN/multi_rnn_cell/cell_0/basic_lstm_cell/weights" in g.vars


@pytest.mark.parametrize("u8", [False, True])
def test_distillchain_memory_combine_chain_plugin_on_the_cpu_graph(monkeypatch, flags, u8):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    H, LL, c, dc, D = 8, 2, 7, 10, 9
    flags.lstm_cells, flags.lstm_layers, flags.deep_chain_layers, flags.deep_chain_relu_cells = str(H), LL, 2, c
    flags.moe_num_mixtures, flags.distillchain_relu_cells = M, dc
    x = _bytes(D) if u8 else torch.zeros(B, F, D)
    _graph()
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        flm.DistillchainLstmMemoryDeepCombineChainModel().create_model(x, vocab_size=V, num_frames=NF)
    g = _graph()
    for rec in (stubs.stacks, stubs.heads, stubs.links, stubs.memory_links, stubs.inputs, stubs.dequants, stubs.stack_inputs):
        rec[:] = []
    res = flm.DistillchainLstmMemoryDeepCombineChainModel().create_model(x, vocab_size=V, num_frames=NF,
                                                                         distillation_predictions=torch.zeros(B, V, dtype=torch.float64), unknown=1)
    want = {"distill-relu/weights": (V, dc), "distill-relu/biases": (dc,), "mean-relu/weights": (D, c), "mean-relu/biases": (c,)}
    for k in range(3):
        _stack_vars(want, "lstm-%d-RNN" % k, D, H, LL)
    widths = [LL * H + dc + c * (1 + stage) for stage in range(3)]       # [l2norm(memories) | distill_norm | mean_relu_norm | relu-0 ...]
    for l, w in enumerate(widths):
        _moe_vars(want, "prediction-%d" % l if l < 2 else "-main", w)
        if l < 2:
            want["relu-%d/weights" % l], want["relu-%d/biases" % l] = (V, c), (c,)
    assert _shapes(g) == want and "distillrelu/weights" not in g.vars
    assert stubs.heads == [(w, 0) for w in widths]
    assert stubs.stacks == [((F, B, D), H, LL, k) for k in range(3)]
    assert stubs.memory_links == [([H] * LL, True)] * 3
    assert stubs.links == [((B, dc), "relu", None)] + [((B, c), "relu", None)] * 3
    assert len(stubs.stack_inputs) == 1 and stubs.dequants == ([(B, F, D)] if u8 else [])
    assert all(x_ is stubs.inputs[0] for x_ in stubs.inputs)
    assert tuple(res["predictions"].shape) == (B, V) and tuple(res["support_predictions"].shape) == (B, 2 * V)


def test_parallel_memory_plugin_on_the_cpu_graph(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    monkeypatch.setattr(stubs.ops, "l2_normalize", lambda x, eps=1e-12: x)         # _parallel_stacks' per-slice normalisation of float frames
    flags.lstm_cells, flags.feature_sizes, flags.lstm_layers, flags.moe_num_mixtures = "16,8", "12,4", 2, M
    g = _graph()
    res = flm.LstmParallelMemoryModel().create_model(torch.zeros(B, F, 16), vocab_size=V, num_frames=NF, unknown=1)
    want = {}
    for i, (d, h) in enumerate(((12, 16), (4, 8))):
        _stack_vars(want, "RNN%d" % i, d, h, 2)
    width = 2 * 16 + 2 * 8                                                # final c of every layer of every stack
    want["gates/weights"], want["experts/weights"], want["experts/biases"] = (width, V * (M + 1)), (width, V * M), (V * M,)
    assert _shapes(g) == want
    assert stubs.heads == [(width, 0)] and stubs.links == []
    assert stubs.memory_links == [([16, 16, 8, 8], False)]               # states.extend(c of every layer) per stack: heterogeneous widths
    assert stubs.stacks == [((F, B, 12), 16, 2, 0), ((F, B, 4), 8, 2, 1)]
    assert tuple(res["predictions"].shape) == (B, V)
    with pytest.raises(AssertionError, match="length of lstm_sizes"):
        flags.lstm_cells = "16"
        _graph()
        flm.LstmParallelMemoryModel().create_model(torch.zeros(B, F, 16), vocab_size=V, num_frames=NF)
