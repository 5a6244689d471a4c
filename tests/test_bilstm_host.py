"""CPU checks of the bidirectional LSTM plugins (W/all_frame_models/bilstm_model.py, biunilstm_model.py): the lookup by name, the
TF-1.0 variable names and shapes (written from memory, as SURVEY.md Appendix A), and the C-ABI declarations of the reversal kernels."""
import os
import re

import pytest

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT


def _names_and_shapes(cls_name, monkeypatch, D=1152, H=1024, layers=2):
    """Builds the plugin's variables on the CPU graph with the native calls stubbed out (only the variable creation is under test)."""
    import torch
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers = str(H), layers
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    B, F = 2, 3
    stack = lambda x, nf, wb, **kw: (torch.zeros(F, B, H), [(torch.zeros(B, H), torch.zeros(B, H)) for _ in wb])
    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(seq_ops, "bidirectional_lstm_stacks", lambda xf, xb, nf, wf, wbw, **kw: (stack(xf, nf, wf), stack(xb, nf, wbw)))
    monkeypatch.setattr(seq_ops, "reverse_sequence_tm", lambda x, nf: x)
    monkeypatch.setattr(seq_ops, "bi_concat", lambda a, b, nf: torch.cat([a, b], 2))
    seen = {}
    monkeypatch.setattr(flm, "_head", lambda name=None: (lambda: type("Head", (), {
        "create_model": lambda self, model_input, **kw: seen.setdefault("state", model_input)})()))
    getattr(flm, cls_name)().create_model(torch.zeros(B, F, D), vocab_size=5, num_frames=torch.tensor([3, 1]), unknown_kwarg=1)
    FLAGS.reset()
    return {k: tuple(v.data.shape) for k, v in g.vars.items()}, tuple(seen["state"].shape)


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in ("BiLstmModel", "BiUniLstmModel"):
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name)
        assert cls.accepts_quantized_input is True


def test_bilstm_variable_names_and_shapes(monkeypatch):
    shapes, state = _names_and_shapes("BiLstmModel", monkeypatch)
    want = {}
    for d in ("fw", "bw"):
        for l, din in enumerate((1152, 1024)):
            s = "RNN/bidirectional_rnn/%s/multi_rnn_cell/cell_%d/basic_lstm_cell/" % (d, l)
            want[s + "weights"] = (din + 1024, 4096)
            want[s + "biases"] = (4096,)
    assert shapes == want
    assert state == (2, 8192)                                        # [state_fw || state_bw], 2 L 2H


def test_biunilstm_variable_names_and_shapes(monkeypatch):
    shapes, state = _names_and_shapes("BiUniLstmModel", monkeypatch)
    assert shapes == {
        "RNN/bidirectional_rnn/fw/basic_lstm_cell/weights": (1152 + 1024, 4096),
        "RNN/bidirectional_rnn/fw/basic_lstm_cell/biases": (4096,),
        "RNN/bidirectional_rnn/bw/basic_lstm_cell/weights": (1152 + 1024, 4096),
        "RNN/bidirectional_rnn/bw/basic_lstm_cell/biases": (4096,),
        "RNN/basic_lstm_cell/weights": (2048 + 1024, 4096),         # the third cell reads [out_fw || out_bw]
        "RNN/basic_lstm_cell/biases": (4096,),
    }
    assert state == (2, 6 * 1024)


def test_header_declares_the_reversal_kernels_and_the_stream_sets():
    declared_bound_exported(("yt8m_reverse_sequence_u8", "yt8m_reverse_sequence_f32_tm", "yt8m_lstm_stack_use_streams",
                             "yt8m_lstm_persist_get_cus"))


def test_reversal_and_stream_set_argument_validation_without_device():
    import ctypes
    lib = L.lib()
    one = ctypes.c_void_p(16)                                        # never dereferenced: validation fails first
    assert lib.yt8m_reverse_sequence_u8(one, one, one, -1, 3, 16, None) == -2
    assert lib.yt8m_reverse_sequence_u8(None, None, None, 0, 3, 16, None) == 0      # empty: no-op
    assert lib.yt8m_reverse_sequence_u8(one, None, one, 2, 3, 16, None) == -1       # no num_frames
    assert lib.yt8m_reverse_sequence_u8(one, one, one, 2, 3, 16, None) == -1        # in place
    assert lib.yt8m_reverse_sequence_u8(ctypes.c_void_p(4096), one, ctypes.c_void_p(4096 + 48), 2, 3, 16, None) == -1   # partly overlapping
    assert lib.yt8m_reverse_sequence_f32_tm(one, 4, one, one, 8, 6, 3, 2, 4, None) == -2   # window past ldy
    assert lib.yt8m_reverse_sequence_f32_tm(one, 2, one, one, 8, 0, 3, 2, 4, None) == -2   # ldx < H
    assert lib.yt8m_reverse_sequence_f32_tm(None, 4, None, None, 4, 0, 0, 2, 4, None) == 0
    assert lib.yt8m_lstm_stack_use_streams(2, None) == -1
    f, b = ctypes.c_int(7), ctypes.c_int(7)                          # the CU caps a capping caller restores
    assert lib.yt8m_lstm_persist_get_cus(ctypes.byref(f), ctypes.byref(b)) == 0 and (f.value, b.value) == (-1, -1)
    assert lib.yt8m_lstm_persist_set_cus(96, 64) == 0
    assert lib.yt8m_lstm_persist_get_cus(ctypes.byref(f), ctypes.byref(b)) == 0 and (f.value, b.value) == (96, 64)
    assert lib.yt8m_lstm_persist_set_cus(-1, -1) == 0
    prev = ctypes.c_int(-1)
    assert lib.yt8m_lstm_stack_use_streams(0, ctypes.byref(prev)) == 0 and prev.value == 0
