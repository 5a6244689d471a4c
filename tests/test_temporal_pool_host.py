"""CPU checks of the temporal-pooling LSTM plugins (W/all_frame_models/multires_lstm_memory_deep_combine_chain_model.py,
framehop_lstm_memory_model.py) and of the frame-pyramid kernel's C ABI (csrc/frame_pyramid.hip): the lookup by name, the header /
signature table / exports, argument validation without a device, the pyramid's fp64 restatement against the reference's order of
operations, both plugins built on the CPU graph with the native calls stubbed out, seq_ops.reserve_resident, and the kernel's register
allocation read from hipcc's resource remarks."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT
from test_transform_host import dequantize64_np, l2_normalize_np, resolution_np

CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("yt8m_frame_pyramid_u8", "yt8m_frame_pyramid_supported")
PLUGINS = {"MultiresLstmMemoryDeepCombineChainModel": False, "FramehopLstmMemoryModel": True}
# the kernel tests' shapes (tests/test_gpu_temporal_pool.py)
PYRAMID_WIDTHS = ([1024, 128], [16, 16], [20, 12], [8, 5], [8, 8], [1152])
PYRAMID_B, PYRAMID_F, PYRAMID_LEVELS = 3, 35, 4
PYRAMID_NF = np.array([35, 1, 20], dtype=np.int32)


def pyramid_case(widths, F=PYRAMID_F, B=PYRAMID_B, num_frames=PYRAMID_NF, seed=5):
    """Reader bytes [B,F,sum widths], zero on the padding frames."""
    q = np.random.RandomState(seed + sum(widths)).randint(0, 256, size=(B, F, sum(widths))).astype(np.uint8)
    for b, n in enumerate(num_frames):
        q[b, n:] = 0
    return q


def pyramid_np(x, num_frames, levels, widths, eps=1e-12):
    """The kernel's definition on float64 frames x [B,F,D] (dequantize64_np of the bytes, or floats as they are): per level l the mean over
    every r = 2^(l+1) frames (resolution_np without its normalisation), split by widths, every part l2-normalised, time-major.
    Returns (parts[l][s] [F // r, B, w_s], num_frames_out[l])."""
    parts, frames = [], []
    for l in range(levels):
        raw, n2 = resolution_np(x, num_frames, 2 << l, l2norm=False)
        row, off = [], 0
        for w in widths:
            row.append(l2_normalize_np(raw[:, :, off:off + w], epsilon=eps).transpose(1, 0, 2))
            off += w
        parts.append(row)
        frames.append(n2)
    return parts, frames


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name, quantized in PLUGINS.items():
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is quantized


def test_library_exports_and_header_declares_the_pyramid_kernel():
    _, lib = declared_bound_exported(KERNELS)
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _widths(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def test_frame_pyramid_supported_shapes():
    lib = L.lib()
    sup = lambda D, widths, levels: lib.yt8m_frame_pyramid_supported(D, len(widths), _widths(*widths), levels)
    assert sup(1152, [1024, 128], 4) == 1                                 # the reader's shape at the training script's settings
    for widths in PYRAMID_WIDTHS:
        assert sup(sum(widths), widths, PYRAMID_LEVELS) == 1, widths
    assert sup(32, [16, 16], 2) == 1 and sup(32, [16, 16], 1) == 1 and sup(1152, [1024, 128], 5) == 1
    assert sup(517, [512, 5], 4) == 0                                     # single bytes: 512 columns per row at the most
    assert sup(2052, [2048, 4], 4) == 0 and sup(2048, [2044, 4], 4) == 1  # 4-byte units: 2048
    assert sup(1152, [1024, 128], 6) == 0 and sup(1152, [1024, 128], 0) == 0
    assert sup(1152, [1024, 100], 4) == 0 and sup(16, [16] + [0] * 8, 4) == 0 and sup(16, [16, 0], 4) == 0
    assert lib.yt8m_frame_pyramid_supported(16, 1, None, 4) == 0


def test_frame_pyramid_argument_validation_without_device():
    """Every call here fails validation (or has nothing to do), so nothing is launched and no device is needed."""
    lib = L.lib()
    B, F, D, levels = 2, 35, 32, 2
    q, nf = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 19)
    ys = [(2 << 20) + (1 << 16) * k for k in range(4)]                    # never dereferenced, far apart
    nfo = [(3 << 20) + 256 * k for k in range(2)]

    def call(q=q, nf=nf, B=B, F=F, D=D, levels=levels, widths=(16, 16), nseg=None, y=ys, nf_out=nfo, eps=1e-12):
        return lib.yt8m_frame_pyramid_u8(q, nf, B, F, D, levels, len(widths) if nseg is None else nseg,
                                         None if widths is None else _widths(*widths), None if y is None else _ptrs(*y),
                                         None if nf_out is None else _ptrs(*nf_out), eps, None)

    assert call(levels=0) == -1 and call(levels=-1) == -1
    assert call(levels=6, y=ys * 3, nf_out=nfo * 3) == -1 and b"levels" in lib.yt8m_last_error()      # 2^6 > F = 35
    assert call(F=3) == -1                                                # 2^2 > 3
    assert call(nseg=0) == -1 and call(nseg=-1) == -1 and call(nseg=9, widths=(4,) * 8 + (0,)) == -1
    assert call(widths=(4,) * 9, D=36, y=ys * 5) == -1                    # more segments than the table holds
    assert call(widths=None, nseg=2) == -1
    assert call(widths=(16, 0)) == -1 and call(widths=(-16, 48)) == -1
    assert call(widths=(16, 8)) == -1 and call(D=33) == -1 and b"add up" in lib.yt8m_last_error()
    assert call(q=None) == -1 and call(y=None) == -1 and call(y=ys[:3] + [None]) == -1 and call(y=[None] + ys[1:]) == -1
    assert call(eps=0.0) == -1 and call(eps=-1e-12) == -1
    assert call(B=-1) == -2 and call(D=-32) == -2
    # outputs on top of the input, of num_frames, of each other; a num_frames_out on top of an output
    assert call(y=[q.value] + ys[1:]) == -1 and b"overlap" in lib.yt8m_last_error()
    assert call(y=[q.value + B * F * D - 4] + ys[1:]) == -1 and call(y=ys[:3] + [nf.value]) == -1
    assert call(y=ys[:2] + [ys[0] + 64, ys[3]]) == -1 and call(y=[ys[1]] + ys[1:]) == -1
    assert call(nf_out=[ys[2], nfo[1]]) == -1 and call(nf_out=[nfo[0], nfo[0] + 4]) == -1 and call(nf_out=[q.value + 8, nfo[1]]) == -1
    # a valid call but for its shape: wider than the single-byte form holds
    assert call(D=517, widths=(512, 5), y=[(2 << 20) + (1 << 18) * k for k in range(4)]) == -2
    # an empty batch: a no-op, also without num_frames / num_frames_out
    assert call(B=0) == 0 and call(B=0, nf=None, nf_out=None) == 0


@pytest.mark.parametrize("widths", PYRAMID_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_pyramid_restatement_is_the_reference_and_the_integer_form(widths):
    """The reference normalises the whole row (resolution(), :161), splits it and normalises every part (lstm(), :21); the kernel
    normalises the parts of the mean.  l2norm(part of l2norm(row)) = l2norm(part of row) wherever the sums of squares exceed the epsilon:
    a dequantised byte is never 0, so only an empty group is below it, and that is a zero row either way.  And the mean itself is the
    integer form (512 S - 65025 k) / (32640 r) of csrc/frame_pyramid.hip."""
    q = pyramid_case(widths)
    x = dequantize64_np(q, PYRAMID_NF)
    parts, frames = pyramid_np(x, PYRAMID_NF, PYRAMID_LEVELS, widths)
    D = sum(widths)
    for l in range(PYRAMID_LEVELS):
        r = 2 << l
        F2 = PYRAMID_F // r
        whole, n2 = resolution_np(x, PYRAMID_NF, r, l2norm=True)          # the reference's resolution()
        assert np.array_equal(n2, PYRAMID_NF // r) and np.array_equal(frames[l], n2)
        off = 0
        for s, w in enumerate(widths):
            ref = l2_normalize_np(whole[:, :, off:off + w]).transpose(1, 0, 2)
            assert parts[l][s].shape == (F2, PYRAMID_B, w)
            assert np.abs(parts[l][s] - ref).max() < 1e-15
            off += w
        S = q[:, :F2 * r].reshape(PYRAMID_B, F2, r, D).astype(np.int64).sum(axis=2)
        k = np.clip(PYRAMID_NF[:, None] - np.arange(F2)[None, :] * r, 0, r)
        m = (512 * S - 65025 * k[:, :, None]) / (32640.0 * r)
        raw, _ = resolution_np(x, PYRAMID_NF, r, l2norm=False)
        assert np.abs(m - raw).max() < 1e-14
        empty = k == 0
        assert empty.any() and not np.concatenate(parts[l], axis=2).transpose(1, 0, 2)[empty].any()


# ---- the plugins on the CPU graph ---------------------------------------------------------------------------------------------------
class _Stubs(object):
    """The native calls replaced by shape-only stand-ins; records what the plugins asked for."""

    def __init__(self, monkeypatch):
        import yt8m_amd.ops as ops
        import yt8m_amd.seq_ops as seq_ops
        self.stacks, self.frames, self.heads, self.links, self.memory_links, self.pyramids, self.dropouts = [], [], [], [], [], [], []

        def stack(x_tm, num_frames, wb, **k):
            H = wb[0][0].data.shape[1] // 4
            self.stacks.append((tuple(x_tm.shape), H, len(wb), k.get("slot", 0)))
            self.frames.append(num_frames.tolist())
            B_ = x_tm.shape[0] if x_tm.dtype == torch.uint8 else x_tm.shape[1]
            T_ = x_tm.shape[1] if x_tm.dtype == torch.uint8 else x_tm.shape[0]
            return torch.zeros(T_, B_, H), [(torch.zeros(B_, H), torch.zeros(B_, H)) for _ in wb]

        def head(x, Wg, We, be, V_, M_, **k):
            self.heads.append(x.shape[1])
            return torch.zeros(x.shape[0], V_)

        def link(z, kind="relu", noise_level=None, seed=None, offset=0, eps=1e-12, graph=None):
            self.links.append((tuple(z.shape), kind, noise_level))
            return z

        def memory_link(tensors, normalize, eps=1e-12):
            tensors = list(tensors)
            self.memory_links.append(([t.shape[1] for t in tensors], bool(normalize)))
            return torch.zeros(tensors[0].shape[0], sum(t.shape[1] for t in tensors))

        def pyramid(x, num_frames, levels, widths, eps=1e-12):
            self.pyramids.append((tuple(x.shape), x.dtype, levels, list(widths)))
            B_, F_, _ = x.shape
            return ([[torch.zeros(F_ >> (l + 1), B_, w) for w in widths] for l in range(levels)],
                    [(num_frames // (2 << l)).to(torch.int32) for l in range(levels)])

        def dropout(x, keep_prob, **k):
            self.dropouts.append((x.shape[1], keep_prob))
            return x

        def no_composed_form(*a, **k):
            raise AssertionError("a relu -> l2norm of the new plugins left ops.chain_link")

        monkeypatch.setattr(seq_ops, "lstm_stack", stack)
        monkeypatch.setattr(ops, "linear", lambda x, W, b=None, bf16=None: torch.zeros(x.shape[0], W.data.shape[1]))
        monkeypatch.setattr(ops, "moe_head", head)
        monkeypatch.setattr(ops, "chain_link", link)
        monkeypatch.setattr(ops, "memory_link", memory_link)
        monkeypatch.setattr(ops, "frame_pyramid", pyramid)
        monkeypatch.setattr(ops, "dropout", dropout)
        monkeypatch.setattr(ops, "dequant_l2norm", lambda q, num_frames=None: torch.zeros(q.shape, dtype=torch.float32))
        monkeypatch.setattr(ops, "l2_normalize", lambda x, eps=1e-12: x)  # the per-part normalisation of float frames and of the hop
        monkeypatch.setattr(ops, "activation", no_composed_form)
        monkeypatch.setattr(seq_ops, "_STACK_SCRATCH_MAX", 8)
        monkeypatch.setattr(seq_ops, "_PERSIST_WS_MAX", 16)
        self.seq_ops = seq_ops


def _shapes(g):
    return {k: tuple(v.data.shape) for k, v in g.vars.items()}


def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


B, F, V, M = 4, 13, 5, 3
NF = torch.tensor([13, 1, 12, 5])
FEATS, CELLS, LL, RELU = (8, 8), (8, 4), 2, 7
MEM = LL * sum(CELLS)                                                       # final c of every layer of every stack of a level


def _moe_vars(want, gates, experts, d_in):
    want[gates + "/weights"] = (d_in, V * (M + 1))
    want[experts + "/weights"] = (d_in, V * M)
    want[experts + "/biases"] = (V * M,)


def _stack_vars(want, scope, D, H, layers):
    for l in range(layers):
        want["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)] = ((D if l == 0 else H) + H, 4 * H)
        want["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)] = (4 * H,)


def _set_flags(flags, use_length=False):
    flags.lstm_cells, flags.feature_sizes, flags.lstm_layers = ",".join(map(str, CELLS)), ",".join(map(str, FEATS)), LL
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.moe_num_mixtures = 2, RELU, M
    flags.deep_chain_use_length = use_length


def _level0_shape(u8, w):
    import yt8m_amd.frame_level_models as flm
    return (B, F, w) if u8 and flm._lib_u8_ok(w) else (F, B, w)           # bytes stay batch-major where the byte projection reads them


@pytest.mark.parametrize("use_length", [False, True])
@pytest.mark.parametrize("u8", [False, True])
def test_multires_plugin_on_the_cpu_graph(monkeypatch, flags, u8, use_length):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    _set_flags(flags, use_length)
    x = torch.zeros(B, F, sum(FEATS), dtype=torch.uint8) if u8 else torch.zeros(B, F, sum(FEATS))
    g = _graph()
    res = flm.MultiresLstmMemoryDeepCombineChainModel().create_model(x, vocab_size=V, num_frames=NF, dropout=True, keep_prob=0.9, unknown=1)
    extra = 5 if use_length else 0
    widths = [MEM + extra + RELU * stage for stage in range(3)]          # [memories | length code | relu-0 | relu-1]
    want = {}
    for k in range(3):
        for i, (d, h) in enumerate(zip(FEATS, CELLS)):
            _stack_vars(want, "lstm%dRNN%d" % (k, i), d, h, LL)
        scope = "prediction-%d" % k if k < 2 else "-main"
        _moe_vars(want, "gates-" + scope, "experts-" + scope, widths[k])
        if k < 2:
            want["relu-%d/weights" % k], want["relu-%d/biases" % k] = (V, RELU), (RELU,)
    assert _shapes(g) == want
    assert want["lstm0RNN0/multi_rnn_cell/cell_1/basic_lstm_cell/weights"] == (16, 32) and "gates--main/weights" in want and "relu-0/biases" in want
    assert stubs.pyramids == [((B, F, 16), x.dtype, 2, list(FEATS))]      # ONE call makes every level r >= 2, on the input as it arrived
    # stage 0 reads resolution 4, stage 1 resolution 2, stage 2 the frames; slots 0..5; num_frames // r
    assert stubs.stacks == [((F // r, B, w) if r > 1 else _level0_shape(u8, w), h, LL, 2 * k + i)
                            for k, r in enumerate((4, 2, 1)) for i, (w, h) in enumerate(zip(FEATS, CELLS))]
    assert stubs.frames == [(NF // r).tolist() for r in (4, 2, 1) for _ in FEATS]
    assert len({s[3] for s in stubs.stacks}) == 6
    assert stubs.memory_links == [([8, 8, 4, 4], False)] * 3              # stack-major, then layer
    assert stubs.heads == widths and stubs.links == [((B, RELU), "relu", None)] * 2
    assert stubs.dropouts == [(w, 0.9) for w in widths[:2]]              # the -main call passes no dropout
    assert (stubs.seq_ops._STACK_SCRATCH_MAX, stubs.seq_ops._PERSIST_WS_MAX) == (8, 16)      # 6 stacks of 2 layers fit already
    assert tuple(res["predictions"].shape) == (B, V) and tuple(res["support_predictions"].shape) == (B, 2 * V)


def test_multires_plugin_elu_noise_and_reservation(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    _set_flags(flags)
    flags.deep_chain_layers, flags.deep_chain_relu_type = 4, "elu"
    g = _graph()
    flm.MultiresLstmMemoryDeepCombineChainModel().create_model(torch.zeros(B, 35, 16), vocab_size=V, num_frames=NF, noise_level=0.2,
                                                               sub_scope="x-")
    assert [s[0][0] for s in stubs.stacks] == [2, 2, 4, 4, 8, 8, 17, 17, 35, 35] and [s[3] for s in stubs.stacks] == list(range(10))
    assert stubs.links == [((B, RELU), "elu", 0.2)] * 4 and stubs.dropouts == []
    assert (stubs.seq_ops._STACK_SCRATCH_MAX, stubs.seq_ops._PERSIST_WS_MAX) == (10, 20)     # the script's ten stacks of two layers
    # sub_scope prefixes the chain, not the LSTM scopes (:67, :95)
    assert "gates-x-prediction-3/weights" in g.vars and "x-relu-3/weights" in g.vars and "experts-x--main/biases" in g.vars
    assert "lstm4RNN1/multi_rnn_cell/cell_0/basic_lstm_cell/weights" in g.vars


def test_length_code_buckets():
    import yt8m_amd.frame_level_models as flm
    code = flm._length_code(torch.tensor([60, 61, 120, 121, 240, 241, 0, 180, 181, 300]))
    assert code.dtype == torch.float32 and tuple(code.shape) == (10, 5)
    assert code.argmax(dim=1).tolist() == [0, 1, 1, 2, 3, 4, 0, 2, 3, 4] and code.sum(dim=1).tolist() == [1.0] * 10


@pytest.mark.parametrize("u8", [False, True])
def test_framehop_plugin_on_the_cpu_graph(monkeypatch, flags, u8):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    _set_flags(flags)
    x = torch.zeros(B, F, sum(FEATS), dtype=torch.uint8) if u8 else torch.zeros(B, F, sum(FEATS))
    g = _graph()
    res = flm.FramehopLstmMemoryModel().create_model(x, vocab_size=V, num_frames=NF, unknown=1)
    want = {}
    for k in range(3):
        for i, (d, h) in enumerate(zip(FEATS, CELLS)):
            _stack_vars(want, "lstm%dRNN%d" % (k, i), d if k == 0 else h, h, LL)   # levels >= 1 read the outputs: width H_i
    _moe_vars(want, "gates", "experts", 3 * MEM)
    assert _shapes(g) == want and want["lstm1RNN1/multi_rnn_cell/cell_0/basic_lstm_cell/weights"] == (8, 16)
    assert stubs.stacks == ([(_level0_shape(u8, w), h, LL, i) for i, (w, h) in enumerate(zip(FEATS, CELLS))] +
                            [((T, B, h), h, LL, 2 * k + i) for k, T in ((1, 6), (2, 3)) for i, h in enumerate(CELLS)])
    # every level k >= 1 runs min(num_frames // 2, T_k) steps: the video with 12 frames keeps 6 at level 1 and is cut to 3 at level 2
    assert stubs.frames == [NF.tolist()] * 2 + [[6, 0, 6, 2]] * 2 + [[3, 0, 3, 2]] * 2
    assert len({s[3] for s in stubs.stacks}) == 6 and stubs.pyramids == [] and stubs.memory_links == []
    assert stubs.heads == [3 * MEM]                                       # level-major, then stack, then layer
    assert tuple(res["predictions"].shape) == (B, V)


def test_the_two_refusals(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _Stubs(monkeypatch)
    _set_flags(flags, use_length=True)
    _graph()
    with pytest.raises(ValueError, match="additional_features"):
        flm.FramehopLstmMemoryModel().create_model(torch.zeros(B, F, 16), vocab_size=V, num_frames=NF)
    _set_flags(flags)
    _graph()
    with pytest.raises(ValueError, match="zero frames"):
        flm.MultiresLstmMemoryDeepCombineChainModel().create_model(torch.zeros(B, 3, 16), vocab_size=V, num_frames=NF)


def test_op_refuses_bad_arguments_and_has_no_cpu_form():
    import yt8m_amd.ops as ops
    with pytest.raises(L.Yt8mHipError):                                   # a missing device is an error, not a fall-back to torch
        ops.frame_pyramid(torch.zeros(2, 8, 16, dtype=torch.uint8), torch.tensor([8, 3]), 2, [8, 8])


def test_reserve_resident_raises_and_never_lowers(monkeypatch):
    import yt8m_amd.seq_ops as seq_ops
    monkeypatch.setattr(seq_ops, "_STACK_SCRATCH_MAX", 8)
    monkeypatch.setattr(seq_ops, "_PERSIST_WS_MAX", 16)
    seq_ops.reserve_resident(4, 2)
    assert (seq_ops._STACK_SCRATCH_MAX, seq_ops._PERSIST_WS_MAX) == (8, 16)
    seq_ops.reserve_resident(10, 2)
    assert (seq_ops._STACK_SCRATCH_MAX, seq_ops._PERSIST_WS_MAX) == (10, 20)
    seq_ops.reserve_resident(12, 1)
    assert (seq_ops._STACK_SCRATCH_MAX, seq_ops._PERSIST_WS_MAX) == (12, 20)
    seq_ops.reserve_resident(2, 2)
    assert (seq_ops._STACK_SCRATCH_MAX, seq_ops._PERSIST_WS_MAX) == (12, 20)


def test_reserve_resident_keeps_the_environment_variable():
    """YT8M_STACK_SCRATCH_MAX is read at import: a fresh interpreter is what this test is about."""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; g.load_package(); import yt8m_amd.seq_ops as s; "
            "a = s._STACK_SCRATCH_MAX; s.reserve_resident(10, 2); b = s._STACK_SCRATCH_MAX; s.reserve_resident(40, 2); "
            "print(a, b, s._STACK_SCRATCH_MAX, s._PERSIST_WS_MAX)" % ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, YT8M_STACK_SCRATCH_MAX="12"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == ["12", "12", "40", "80"]


def test_frame_pyramid_kernels_own_no_stack_object_and_do_not_spill():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "--cuda-device-only", "-c", "frame_pyramid.hip",
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", p.stderr)] + [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", p.stderr)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", p.stderr)]
    assert len(names) == 3 and len(scratch) == 3 and len(spills) == 6 and len(vgprs) == 3, p.stderr[-2000:]   # 16-, 4- and 1-byte units
    assert all("frame_pyramid_kernel" in n for n in names)
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
    assert all(v == 0 for v in spills), spills
    assert all(v <= 128 for v in vgprs), vgprs                            # 16 waves of the largest workgroup share a CU's registers
