"""CPU checks of random half-frame inference (Z/frame_level_models.py:4017-4079 LstmRandomModel, :6133-6180 FrameAttentionEvalModel,
:6182-6247 FrameRandomEvalModel) and of its op's C ABI (csrc/frame_subset.hip): the host form of the draw against the restatement, the
shape of every index row, the inclusion frequencies of the draw, the composed gather against the restatement, the lookup by name, the
header / signature table / exports, argument validation without a device, and the three plugins on the CPU graph (the LSTM stack, the
MoE and the frame pooling, which have no CPU form, stubbed by the restatements') against LstmMemoryModel / LstmExtendModel run on the
restated gathers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import frame_subset_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT
from gate_lstm_restatement import moe
from oracle import torch_ref

SYMBOLS = ("yt8m_frame_subset_draw", "yt8m_frame_subset_gather_u8", "yt8m_frame_subset_gather_f32")
PLUGINS = ("LstmRandomModel", "FrameRandomEvalModel", "FrameAttentionEvalModel")
DRAWS = ((1, 4, 2), (3, 5, 2), (16, 300, 150), (2, 1024, 512), (1, 7, 7), (2, 9, 1), (5, 2, 1), (4, 33, 32))      # (E, F, K)


def _index(E, F, K, seed):
    import yt8m_amd.ops as ops
    return ops.frame_subset_index(E, F, K, seed=seed, device="cpu")


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,F,K", DRAWS)
def test_index_rows_are_ascending_distinct_and_in_range(E, F, K):
    for seed in (0, 12345, (1 << 63) + 77):
        index = _index(E, F, K, seed)
        assert index.dtype == torch.int32 and tuple(index.shape) == (E, K) and index.device.type == "cpu"
        a = index.numpy().astype(np.int64)
        assert a.min() >= 0 and a.max() < F
        assert bool((np.diff(a, axis=1) > 0).all())                      # ascending and distinct
        if K == F:
            assert bool((a == np.arange(F)[None, :]).all())              # the identity
        assert np.array_equal(index.numpy(), R.draw(E, F, K, seed))      # the host form is the restatement's draw


def test_inclusion_frequencies_over_seeds_and_over_replicas():
    """F = 8, K = 4: every frame is in the subset with probability 1/2.  Over 2000 draws a frequency's standard deviation is
    sqrt(0.25 / 2000) = 0.0112; the bound 0.06 is a little over five of them (0.056).  The restatement's own largest deviations: 0.007
    over the seeds, 0.024 over the replicas."""
    F, K, N = 8, 4, 2000
    counts = np.zeros(F)
    for seed in range(N):
        counts[_index(1, F, K, seed).numpy()[0]] += 1
    assert float(np.abs(counts / N - 0.5).max()) <= 0.06, counts / N
    index = _index(N, F, K, 12345).numpy()
    freq = np.bincount(index.reshape(-1), minlength=F) / N
    assert float(np.abs(freq - 0.5).max()) <= 0.06, freq
    assert len({tuple(r) for r in index.tolist()}) == 70                 # every one of the C(8, 4) subsets occurs among 2000 replicas


def test_draw_follows_the_graphs_random_op_keys_and_refuses_bad_shapes():
    import yt8m_amd.ops as ops
    from yt8m_amd.variables import random_seed, reset_default_graph
    g = reset_default_graph(device=torch.device("cpu"), seed=3)
    g.begin_step()
    a, b = ops.frame_subset_index(2, 12, 6), ops.frame_subset_index(2, 12, 6)
    assert a.device.type == "cpu" and g._rng_calls == 2
    assert np.array_equal(a.numpy(), R.draw(2, 12, 6, random_seed(3, 0, 0, 0)))
    assert np.array_equal(b.numpy(), R.draw(2, 12, 6, random_seed(3, 0, 0, 1)))
    for E, F, K in ((1, 1, 1), (1, 1025, 2), (1, 8, 0), (1, 8, 9), (-1, 8, 4)):
        with pytest.raises(ValueError):
            ops.frame_subset_index(E, F, K, seed=0, device="cpu")


# ---- the composed form against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("B,F,D,E", [(1, 4, 1, 1), (3, 5, 20, 3), (5, 8, 17, 2)])
def test_composed_form_matches_the_restatement(dtype, B, F, D, E):
    import yt8m_amd.ops as ops
    nf = np.array([0, 1, F, F + 3, -1][:B] if B > 1 else [F - 1], dtype=np.int32)
    x = R.frames(B, F, D, nf, dtype, seed=B + F, padding=255 if dtype == np.uint8 else 0)       # bytes: untrusted padding
    before = dict(ops.FRAME_SUBSET_CALLS)
    y, n, index = ops.frame_subset(torch.from_numpy(x), torch.from_numpy(nf), E, seed=99)
    assert ops.FRAME_SUBSET_CALLS == dict(before, composed=before["composed"] + 1)               # CPU tensors: the composed form
    assert np.array_equal(index.numpy(), R.draw(E, F, F // 2, 99))
    want_y, want_n = R.gather(x, nf, index.numpy())
    assert y.dtype == torch.from_numpy(x).dtype and tuple(y.shape) == (B * E, F // 2, D) and n.dtype == torch.int32
    assert np.array_equal(y.numpy(), want_y) and np.array_equal(n.numpy(), want_n)
    # a hand-made index: -1 and F are padding, left out of the count; K of its own
    hand = torch.tensor([[-1, 0, F - 1, F]] * E, dtype=torch.int32)
    y, n, back = ops.frame_subset(torch.from_numpy(x), torch.from_numpy(nf), E, index=hand)
    want_y, want_n = R.gather(x, nf, hand.numpy())
    assert back is not None and np.array_equal(back.numpy(), hand.numpy())
    assert np.array_equal(y.numpy(), want_y) and np.array_equal(n.numpy(), want_n)
    assert float(np.abs(y.numpy()[:, [0, 3]].astype(np.float64)).max()) == 0.0 and int(n.max()) <= 2
    with pytest.raises(ValueError):
        ops.frame_subset(torch.from_numpy(x), torch.from_numpy(nf), E + 1, index=hand)


# ---- names, header, exports, validation ----------------------------------------------------------------------------------------------
def test_find_class_by_name_resolves_the_plugins(flags):
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True
    assert issubclass(flm.LstmRandomModel, flm.LstmMemoryModel)
    assert not hasattr(flm, "VideoFrameEvalModel")                                    # no script uses it: not built
    assert flags.lstm_random_frames is False
    assert 'FLAGS.train=="train"' in flm.LstmRandomModel.__doc__ and "--lstm_random_frames" in flm.LstmRandomModel.__doc__


def test_library_exports_and_header_declares_the_symbols():
    src, lib = declared_bound_exported(SYMBOLS)
    assert "csrc/frame_subset.hip" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_argument_validation_without_device():
    """Every call here fails validation (or has nothing to do): nothing is launched and no device is needed."""
    lib = L.lib()
    OK, BADARG, SHAPE = 0, -1, -2
    p = [ctypes.c_void_p((k + 1) << 20) for k in range(5)]            # 1 MiB apart: disjoint at the sizes below
    draw = lib.yt8m_frame_subset_draw
    assert draw(p[0], 1, 1, 1, 0, None) == SHAPE and draw(p[0], 1, 1025, 2, 0, None) == SHAPE
    assert draw(p[0], 1, 8, 0, 0, None) == SHAPE and draw(p[0], 1, 8, 9, 0, None) == SHAPE and draw(p[0], -1, 8, 4, 0, None) == SHAPE
    assert draw(None, 1, 8, 4, 0, None) == BADARG and draw(None, 0, 8, 4, 0, None) == OK
    assert b"frame_subset_draw" in lib.yt8m_last_error()
    B, F, D, E, K = 2, 8, 16, 3, 4
    for fn in (lib.yt8m_frame_subset_gather_u8, lib.yt8m_frame_subset_gather_f32):
        call = lambda x=p[0], nf=p[1], idx=p[2], y=p[3], out=p[4], B=B, F=F, D=D, E=E, K=K: fn(x, nf, idx, y, out, B, F, D, E, K, None)
        for dim in ("B", "F", "D", "E", "K"):
            assert call(**{dim: -1}) == SHAPE, dim
        assert call(B=0) == OK and call(E=0) == OK
        for name in ("x", "nf", "idx", "y", "out"):
            assert call(**{name: None}) == BADARG, name
        assert call(y=p[0]) == BADARG and call(out=p[3]) == BADARG and call(out=p[1]) == BADARG and call(idx=p[3]) == BADARG
        assert call(out=p[2]) == BADARG
        assert call(B=1 << 16, E=1 << 8, K=1 << 8, D=1 << 4, F=1 << 9, x=ctypes.c_void_p(1 << 50), y=ctypes.c_void_p(1 << 52)) == SHAPE   # 2^32 items
    assert b"frame_subset_gather" in lib.yt8m_last_error() or b"gather_launch" in lib.yt8m_last_error()


# ---- the plugins on the CPU graph: the stack, the MoE and the frame pooling stubbed by the restatements' ------------------------------
def _stub_native(monkeypatch):
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops

    def stack(x_tm, nf, wb, slot=0, **kw):
        out, c, h = torch_ref.lstm_stack(x_tm.transpose(0, 1), nf, [(ops.as_tensor(W), ops.as_tensor(b)) for W, b in wb])
        return out.transpose(0, 1).contiguous(), list(zip(c, h))

    monkeypatch.setattr(seq_ops, "lstm_stack", stack)
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V_, M_, **k: moe(x, Wg.data, We.data, be.data, M_))
    monkeypatch.setattr(ops, "frame_pool", lambda x, kind: x.max(dim=1)[0] if kind == "max" else x.mean(dim=1))


def _graph(seed=0):
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=seed)


D_, H_, E_, B_, F_, V_, M_, LAYERS_ = 12, 16, 3, 4, 9, 6, 2, 2
NF_ = np.array([9, 0, 1, 6], dtype=np.int32)
SEED_ = 4242


def _setup(flags, head="MoeModel"):
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_extend, flags.moe_num_mixtures = str(H_), LAYERS_, E_, M_
    flags.video_level_classifier_model = head
    x = R.frames(B_, F_, D_, NF_, np.float32, seed=5)
    return torch.from_numpy(x), torch.from_numpy(NF_)


def _randomise(g, rs):
    for k, v in g.vars.items():
        s = tuple(v.data.shape)
        v.data.copy_(torch.from_numpy((rs.randn(*s) * (0.1 if len(s) == 1 else 1.5 / np.sqrt(s[0]))).astype(np.float32)))


def _replica(x, nf, e):
    """(frames, num_frames) of replica e of every video, from the restated draw and gather"""
    y, n = R.gather(x.numpy(), nf.numpy(), R.draw(E_, F_, F_ // 2, SEED_))
    return torch.from_numpy(y[e::E_].copy()), torch.from_numpy(n[e::E_].copy())


def test_frame_random_eval_model_is_the_mean_of_lstm_memory_model_over_the_replicas(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    x, nf = _setup(flags)
    _stub_native(monkeypatch)
    g = _graph()
    flm.LstmMemoryModel().create_model(x, vocab_size=V_, num_frames=nf)
    want_vars = [(k, tuple(v.data.shape)) for k, v in g.vars.items()]
    g = _graph()
    flm.FrameRandomEvalModel().create_model(x, vocab_size=V_, num_frames=nf, frame_subset_seed=SEED_)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == want_vars         # LstmMemoryModel's names, shapes and order
    assert want_vars[0] == ("RNN/multi_rnn_cell/cell_0/basic_lstm_cell/weights", (D_ + H_, 4 * H_))
    assert want_vars[-3][0] == "gates/weights" and want_vars[-3][1] == (LAYERS_ * H_, V_ * (M_ + 1))   # the concatenated memories
    _randomise(g, np.random.RandomState(1))
    got = flm.FrameRandomEvalModel().create_model(x, vocab_size=V_, num_frames=nf, frame_subset_seed=SEED_, is_training=False,
                                                  labels=torch.zeros(B_, V_))["predictions"]
    per = []
    empty = 0
    for e in range(E_):
        xe, ne = _replica(x, nf, e)
        empty += int((ne == 0).sum())
        per.append(flm.LstmMemoryModel().create_model(xe, vocab_size=V_, num_frames=ne, is_training=False)["predictions"])
    assert empty >= E_                                                                # the video without frames, in every replica
    want = torch.stack(per, dim=1).double().mean(dim=1)
    assert tuple(got.shape) == (B_, V_) and float((got.detach().double() - want.detach()).abs().max()) < 2e-6
    # a replica without a frame hands the zero state to the head: video 1's prediction is the head's on a zero row
    zero = flm.LstmMemoryModel().create_model(torch.zeros(1, F_ // 2, D_), vocab_size=V_, num_frames=torch.zeros(1, dtype=torch.int32))
    assert float((got[1] - zero["predictions"][0]).abs().max()) < 2e-6
    # the default key is the graph's next random-op key
    from yt8m_amd.variables import random_seed
    g.begin_step()
    a = flm.FrameRandomEvalModel().create_model(x, vocab_size=V_, num_frames=nf)["predictions"]
    b = flm.FrameRandomEvalModel().create_model(x, vocab_size=V_, num_frames=nf,
                                                frame_subset_seed=random_seed(g.seed, 0, g._rng_step, 0))["predictions"]
    assert torch.equal(a, b)


def test_frame_attention_eval_model_is_the_clipped_mean_of_lstm_extend_model(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    x, nf = _setup(flags, head="MoeExtendModel")
    _stub_native(monkeypatch)
    g = _graph()
    flm.LstmExtendModel().create_model(x, vocab_size=V_, num_frames=nf)
    want_vars = [(k, tuple(v.data.shape)) for k, v in g.vars.items()]
    g = _graph()
    flm.FrameAttentionEvalModel().create_model(x, vocab_size=V_, num_frames=nf, frame_subset_seed=SEED_)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == want_vars
    _randomise(g, np.random.RandomState(2))
    clips = []
    real_clamp = torch.Tensor.clamp
    monkeypatch.setattr(torch.Tensor, "clamp", lambda t, *a, **k: (clips.append((a, k)), real_clamp(t, *a, **k))[1])
    got = flm.FrameAttentionEvalModel().create_model(x, vocab_size=V_, num_frames=nf, frame_subset_seed=SEED_,
                                                     is_training=False)["predictions"]
    monkeypatch.setattr(torch.Tensor, "clamp", real_clamp)
    assert ((0.0, 1.0), {}) in clips                                                  # clip_by_value(predictions, 0, 1) before the mean
    per = []
    for e in range(E_):
        xe, ne = _replica(x, nf, e)
        per.append(flm.LstmExtendModel().create_model(xe, vocab_size=V_, num_frames=ne, is_training=False)["predictions"])
    want = torch.stack(per, dim=1).double().clamp(0.0, 1.0).mean(dim=1)
    assert tuple(got.shape) == (B_, V_) and float((got.detach().double() - want.detach()).abs().max()) < 2e-6


def test_lstm_random_model(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    x, nf = _setup(flags)
    _stub_native(monkeypatch)
    g = _graph()
    flm.LstmMemoryModel().create_model(x, vocab_size=V_, num_frames=nf)
    want_vars = [(k, tuple(v.data.shape)) for k, v in g.vars.items()]
    g = _graph()
    flm.LstmRandomModel().create_model(x, vocab_size=V_, num_frames=nf)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == want_vars
    _randomise(g, np.random.RandomState(3))
    memory = lambda xi, ni, **kw: flm.LstmMemoryModel().create_model(xi, vocab_size=V_, num_frames=ni, **kw)["predictions"]
    rand = lambda **kw: flm.LstmRandomModel().create_model(x, vocab_size=V_, num_frames=nf, **kw)["predictions"]
    # the flag off, the reference as committed: LstmMemoryModel bit for bit, in training and in evaluation, and no random op is drawn
    g.begin_step()
    assert torch.equal(rand(), memory(x, nf)) and torch.equal(rand(is_training=False), memory(x, nf, is_training=False))
    assert torch.equal(rand(frame_subset_seed=SEED_), memory(x, nf)) and g._rng_calls == 0
    # the flag on: training steps run on the restated half with the same seed; evaluation on all frames
    flags.lstm_random_frames = True
    y, n = R.gather(x.numpy(), nf.numpy(), R.draw(1, F_, F_ // 2, SEED_))
    half = memory(torch.from_numpy(y), torch.from_numpy(n))
    assert torch.equal(rand(frame_subset_seed=SEED_), half)
    assert not torch.equal(half, memory(x, nf))
    assert torch.equal(rand(frame_subset_seed=SEED_, is_training=False), memory(x, nf, is_training=False))
    assert g._rng_calls == 0
    rand()                                                                             # the default key: the graph's next random op
    assert g._rng_calls == 1
