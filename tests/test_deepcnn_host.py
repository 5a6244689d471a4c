"""CPU checks of DeepCnnDeepCombineChainModel and CnnLstmMemoryModel (W/all_frame_models/deep_cnn_deep_combine_chain_model.py,
cnn_lstm_memory_model.py): the lookup by name, every variable's name, shape and place in the creation order at the training scripts'
settings, the stage widths, the frames each level of the deep CNN sees, the one byte image of the chain, the dropout in front of "-main",
the composed form of seq_ops.max_pool2_tm against fp64, and the C-ABI declarations, argument validation and register allocation of the
one-pass pooling kernels (csrc/deep_cnn.hip)."""
import ctypes
import os
import re

import pytest
import torch

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

KERNELS = ("yt8m_timepool_max_pool2_f32_fwd", "yt8m_timepool_max_pool2_f32_bwd")
NAMES = ("DeepCnnDeepCombineChainModel", "CnnLstmMemoryModel")
D, C, RELU, LAYERS, MIX, V, H = 1152, 128, 256, 2, 4, 5, 1024        # run-chaining-deep-cnn.sh / run-cnn-lstm.sh (V kept small)


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in NAMES:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name)
        assert cls.accepts_quantized_input is True


def test_flag_default_follows_the_reference():
    import yt8m_amd.frame_level_models  # noqa: F401  (defines the flag)
    from yt8m_amd.flags import FLAGS
    FLAGS.reset()
    assert FLAGS.deep_cnn_base_size == 128


def test_library_exports_and_header_declares_the_kernels():
    _, lib = declared_bound_exported(KERNELS)
    assert lib.yt8m_abi_version() == 4                               # symbols were added, nothing else moved


def test_argument_validation_without_device():
    lib = L.lib()
    p = [ctypes.c_void_p(16 * (i + 1)) for i in range(6)]           # never dereferenced: validation fails first
    odd = ctypes.c_void_p(20)                                        # not 16-byte aligned
    err = lambda: lib.yt8m_last_error().decode()

    def fwd(y=p[0], ldy=8, F=3, B=2, C=8, out=p[1], idx=p[2], ldo=8, pooled=p[3], ldp=8):
        return lib.yt8m_timepool_max_pool2_f32_fwd(y, ldy, F, B, C, out, idx, ldo, pooled, ldp, None)

    def bwd(y=p[0], ldy=8, F=3, B=2, C=8, g=p[1], idx=p[2], ldg=8, dp=p[3], lddp=8, dy=p[4], lddy=8):
        return lib.yt8m_timepool_max_pool2_f32_bwd(y, ldy, F, B, C, g, idx, ldg, dp, lddp, dy, lddy, None)

    for call in (fwd, bwd):
        assert call(C=6) == -2 and "multiple of 4" in err()
        assert call(C=0) == -2
        assert call(ldy=10) == -2 and "ldy" in err()
        assert call(ldy=4) == -2
        assert call(F=0) == -2 and call(F=-1) == -2 and call(B=0) == -2
        assert call(F=1 << 16, B=1 << 15) == -2 and "2^31" in err()
        assert call(F=1 << 31, B=1) == -2
        assert call(y=None) == -1 and "null" in err()
        assert call(y=odd) == -1 and "aligned" in err()
        assert call(idx=None) == -1 and call(idx=odd) == -1
    assert fwd(ldo=10) == -2 and fwd(ldo=4) == -2 and fwd(ldp=10) == -2 and fwd(ldp=4) == -2 and "ldo / ldp" in err()
    assert fwd(out=None) == -1 and fwd(out=odd) == -1 and fwd(pooled=odd) == -1
    assert fwd(out=p[0]) == -1 and "alias" in err()
    assert bwd(ldg=10) == -2 and bwd(lddp=10) == -2 and bwd(lddy=10) == -2 and bwd(lddy=4) == -2 and "lddy" in err()
    assert bwd(dy=None) == -1 and "null" in err()
    assert bwd(dy=odd) == -1 and bwd(g=odd) == -1 and bwd(dp=odd) == -1
    assert bwd(dy=p[0]) == -1 and "alias" in err()


def _stubs(monkeypatch, rec):
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops

    def linear(x, W, b=None, bf16=None):
        rec["linear"].append((W.name, x.shape[0]))
        return torch.zeros(x.shape[0], W.data.shape[1])

    def head(x, Wg, We, be, V_, M_, **k):
        rec["heads"].append(x.shape[1])
        return torch.zeros(x.shape[0], V_)

    def dropout(x, keep_prob, **k):
        rec["dropout"].append((x.shape[1], keep_prob))
        return x

    def stack(x_tm, num_frames, wb, **k):
        rec["stacks"].append((tuple(x_tm.shape), [int(v) for v in num_frames], [tuple(W.data.shape) for W, _ in wb]))
        Hs = wb[0][0].data.shape[1] // 4
        return torch.zeros(x_tm.shape[0], x_tm.shape[1], Hs), [(torch.zeros(x_tm.shape[1], Hs), torch.zeros(x_tm.shape[1], Hs)) for _ in wb]

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "activation", lambda x, kind: x)
    monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: x)
    monkeypatch.setattr(ops, "moe_head", head)
    monkeypatch.setattr(ops, "dropout", dropout)


def _build(cls_name, monkeypatch, B=4, F=300, u8=False, **kw):
    """The plugin on the CPU graph with the native calls stubbed out: variable creation, shapes and the frame bookkeeping are under
    test, not arithmetic.  u8: the reader's bytes, with the byte products' gates opened and stand-ins for their kernels, so that the
    device's time-major path runs here."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.deep_chain_layers, FLAGS.deep_chain_relu_cells, FLAGS.deep_cnn_base_size, FLAGS.moe_num_mixtures = LAYERS, RELU, C, MIX
    FLAGS.lstm_cells, FLAGS.lstm_layers = str(H), 2
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    rec = dict(linear=[], heads=[], dropout=[], stacks=[], images=[], cnn=[], pooled=[])
    _stubs(monkeypatch, rec)
    if u8:
        class Images(object):
            def __init__(self, q, num_frames):
                self.B, self.F, self.D = q.shape
                rec["images"].append(tuple(q.shape))

        def cnn(rows, B_, fvars, kind):
            rec["cnn"].append((kind, rows // B_, fvars[0].name))
            return torch.zeros(rows, sum(W.data.shape[1] for W in fvars))

        def pooled(x2d, B_, cnns):
            rec["pooled"].append((x2d.shape[0] // B_, cnns[0][0].name))
            return [torch.zeros(B_, sum(W.data.shape[1] for W in cnn_)) for cnn_ in cnns]

        monkeypatch.setattr(seq_ops, "u8_cnn_supported", lambda q: True)
        monkeypatch.setattr(seq_ops, "u8_attention_supported", lambda q, A: True)
        monkeypatch.setattr(seq_ops, "U8FrameImages", Images)
        monkeypatch.setattr(seq_ops, "u8_frame_scales", lambda q, num_frames, eps=1e-12: None)
        monkeypatch.setattr(seq_ops, "pool_u8_raw", lambda w, q, rs: torch.zeros(q.shape[0], q.shape[2]))
        monkeypatch.setattr(seq_ops, "u8_cnn_tm", lambda frames, fvars: cnn(frames.F * frames.B, frames.B, fvars, "u8"))
        monkeypatch.setattr(seq_ops, "cnn_tm", lambda x2d, B_, fvars: cnn(x2d.shape[0], B_, fvars, "f32"))
        monkeypatch.setattr(seq_ops, "cnn_tm_maxpool", pooled)
    x = torch.zeros(B, F, D, dtype=torch.uint8 if u8 else torch.float32)
    try:
        res = getattr(flm, cls_name)().create_model(x, vocab_size=V, num_frames=torch.tensor([300, 1, 7, 5][:B]), unknown_kwarg=1, **kw)
    finally:
        FLAGS.reset()
    return [(k, tuple(v.data.shape)) for k, v in g.vars.items()], res, rec


def _moe(scope, d_in):
    return [("gates-%s/weights" % scope, (d_in, V * (MIX + 1))), ("experts-%s/weights" % scope, (d_in, V * MIX)),
            ("experts-%s/biases" % scope, (V * MIX,))]


def _deepcnn_vars(k):
    want = []
    for i, (d, sizes, widths) in enumerate(((D, (1, 2, 3), (C, C, 2 * C)), (4 * C, (2, 3), (C, C)), (2 * C, (2, 3), (C, C)))):
        want += [("deepcnn%dcnn%dfilter-len%d" % (k, i, fs), (d * fs, n)) for fs, n in zip(sizes, widths)]
    return want


WIDTHS = [8 * C, D + 8 * C + 2 * RELU, D + 8 * C + 3 * RELU]


def _want_deepcnn():
    want = [("mean-relu/weights", (D, RELU)), ("mean-relu/biases", (RELU,))]
    for l in range(LAYERS):
        want += _deepcnn_vars(l) + _moe("prediction-%d" % l, WIDTHS[l]) + [("relu-%d/weights" % l, (V, RELU)), ("relu-%d/biases" % l, (RELU,))]
    return want + _deepcnn_vars(LAYERS) + _moe("-main", WIDTHS[LAYERS])


def test_deep_cnn_variables_order_widths_and_frame_counts(monkeypatch):
    assert WIDTHS == [1024, 1152 + 1024 + 512, 1152 + 1024 + 768]
    shapes, res, rec = _build("DeepCnnDeepCombineChainModel", monkeypatch)
    assert shapes == _want_deepcnn()                                 # names, shapes and the creation order
    assert rec["heads"] == WIDTHS and rec["dropout"] == []
    assert tuple(res["predictions"].shape) == (4, V) and tuple(res["support_predictions"].shape) == (4, LAYERS * V)
    cnn_rows = [(name, rows // 4) for name, rows in rec["linear"] if "filter-len" in name]
    assert cnn_rows == [(name, F_) for k in range(LAYERS + 1) for (name, _), F_ in zip(_deepcnn_vars(k), (300,) * 3 + (150,) * 2 + (75,) * 2)]


def test_deep_cnn_on_bytes_shares_one_image_and_stays_time_major(monkeypatch):
    shapes, res, rec = _build("DeepCnnDeepCombineChainModel", monkeypatch, u8=True)
    assert shapes == _want_deepcnn() and rec["heads"] == WIDTHS
    assert rec["images"] == [(4, 300, D)]                            # ONE byte image for the three deep CNNs of the chain
    assert rec["cnn"] == [(kind, F_, "deepcnn%dcnn%dfilter-len%d" % (k, i, fs))
                          for k in range(LAYERS + 1) for kind, F_, i, fs in (("u8", 300, 0, 1), ("f32", 150, 1, 2))]
    assert rec["pooled"] == [(75, "deepcnn%dcnn2filter-len2" % k) for k in range(LAYERS + 1)]     # the last level: the gathering op


def test_deep_cnn_dropout_reaches_main_and_short_input_is_refused(monkeypatch):
    _, _, rec = _build("DeepCnnDeepCombineChainModel", monkeypatch, dropout=True, keep_prob=0.9, noise_level=0.2)
    assert rec["dropout"] == [(w, 0.9) for w in WIDTHS]              # every stage, "-main" included
    with pytest.raises(ValueError, match="without frames"):
        _build("DeepCnnDeepCombineChainModel", monkeypatch, F=3)
    _build("DeepCnnDeepCombineChainModel", monkeypatch, F=4)


def test_cnn_lstm_memory_variables_stack_input_and_head_width(monkeypatch):
    want = [("cnn-filter-len%d" % fs, (D * fs, 1024)) for fs in (1, 2, 3)]
    for l, d in enumerate((3072, H)):
        want += [("RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % l, (d + H, 4 * H)),
                 ("RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % l, (4 * H,))]
    want += [("gates/weights", (2 * H, V * (MIX + 1))), ("experts/weights", (2 * H, V * MIX)), ("experts/biases", (V * MIX,))]
    for u8 in (False, True):
        shapes, res, rec = _build("CnnLstmMemoryModel", monkeypatch, u8=u8)
        assert shapes == want
        assert rec["stacks"] == [((300, 4, 3072), [300, 1, 7, 5], [(3072 + H, 4 * H), (2 * H, 4 * H)])]       # time-major float input
        assert rec["heads"] == [2 * H]
        assert tuple(res["predictions"].shape) == (4, V)
        assert rec["images"] == ([(4, 300, D)] if u8 else []) and [c[:2] for c in rec["cnn"]] == ([("u8", 300)] if u8 else [])


def _restate(y):
    """fp64: (max over frames, max over pairs)."""
    F = y.shape[0]
    p = torch.maximum(y[0:2 * (F // 2):2], y[1:2 * (F // 2):2])
    return y.amax(dim=0), p


@pytest.mark.parametrize("F,B,C_", [(1, 3, 4), (2, 1, 4), (7, 5, 6), (12, 2, 9)])
def test_composed_max_pool2_on_cpu_against_fp64(F, B, C_):
    import yt8m_amd.seq_ops as seq_ops
    gen = torch.Generator().manual_seed(F * 100 + B)
    y64 = torch.randn((F, B, C_), generator=gen, dtype=torch.float64)
    y32 = y64.to(torch.float32)
    y64 = y32.to(torch.float64).requires_grad_(True)                 # the same values: maxima are exact
    y = y32.reshape(F * B, C_).clone().requires_grad_(True)
    assert not seq_ops.max_pool2_tm_supported(y, 8)                  # a CPU tensor: the composed form
    m, p = seq_ops.max_pool2_tm(y, F, B)
    m64, p64 = _restate(y64)
    assert tuple(m.shape) == (B, C_) and tuple(p.shape) == (F // 2, B, C_)
    assert torch.equal(m.to(torch.float64), m64) and torch.equal(p.to(torch.float64), p64)
    gm = torch.randn((B, C_), generator=gen, dtype=torch.float64)
    gp = torch.randn((F // 2, B, C_), generator=gen, dtype=torch.float64)
    ((m64 * gm).sum() + (p64 * gp).sum()).backward()
    ((m * gm.to(torch.float32)).sum() + (p * gp.to(torch.float32)).sum()).backward()
    # one fp32 addition per element against the fp64 sum of the same two fp32-representable terms
    want = y64.grad.reshape(F * B, C_)
    assert float((y.grad.to(torch.float64) - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max()) + 1e-30
    m2, none = seq_ops.max_pool2_tm(y.detach(), F, B, want_pool=False)
    assert none is None and torch.equal(m2, m.detach())


def test_deep_cnn_kernels_do_not_spill():
    from test_build_resources import HIPCC, _remarks
    assert os.path.exists(HIPCC), "hipcc is what build() compiles with"
    remarks = _remarks("deep_cnn.hip")
    kernels = {k: v for k, v in remarks.items() if "dc_max_pool2_fwd_kernel" in k or "dc_max_pool2_bwd_kernel" in k}
    assert len(kernels) == 2 == len(remarks), sorted(remarks)
    for k, v in kernels.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (k, v)    # no spills and no stack object
        assert v["VGPRs"] <= 64 and v["Occupancy"] >= 8, (k, v)           # streams: the full eight waves per SIMD
