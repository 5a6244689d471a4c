"""-m gpu: random half-frame inference on the device (csrc/frame_subset.hip, ops.frame_subset, LstmRandomModel / FrameRandomEvalModel /
FrameAttentionEvalModel): the draw and the gather bit for bit against the numpy restatement at every path of the launcher, the edge values
of num_frames, untrusted padding, out-of-range indices, reruns, and the three plugins on bytes and on floats against their CPU form."""
import ctypes

import numpy as np
import pytest
import torch

import frame_subset_restatement as R
import yt8m_amd._lib as L
from gate_lstm_restatement import moe
from oracle import np_ref, torch_ref

pytestmark = pytest.mark.gpu

SEED = 20240611


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,F,K", [(1, 4, 2), (3, 5, 2), (16, 300, 150), (2, 1024, 512), (1, 7, 7), (2, 9, 1)])
def test_draw_is_the_restatements_bit_for_bit(dev, E, F, K):
    import yt8m_amd.ops as ops
    for seed in (SEED, (1 << 63) + 5):
        index = ops.frame_subset_index(E, F, K, seed=seed, device=dev)
        again = ops.frame_subset_index(E, F, K, seed=seed, device=dev)
        assert index.is_cuda and index.dtype == torch.int32 and tuple(index.shape) == (E, K)
        assert np.array_equal(index.cpu().numpy(), R.draw(E, F, K, seed))
        assert torch.equal(index, again)                                                     # no atomics: a rerun is bit-equal
        assert torch.equal(index.cpu(), ops.frame_subset_index(E, F, K, seed=seed, device="cpu"))    # the host form agrees


def test_draw_refuses_shapes_outside_its_limits(dev):
    index = torch.full((4, 8), -7, dtype=torch.int32, device=dev)
    draw = lambda E, F, K: L.lib().yt8m_frame_subset_draw(ctypes.c_void_p(index.data_ptr()), E, F, K, 1, None)
    assert draw(1, 1, 1) == -2 and draw(1, 1025, 2) == -2 and draw(1, 8, 0) == -2             # YT8M_E_SHAPE
    torch.cuda.synchronize()
    assert int((index != -7).sum()) == 0                                                      # nothing was launched


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
def _run(dev, x, nf, E, fused, **kw):
    import yt8m_amd.ops as ops
    saved = ops.FRAME_SUBSET_FUSED
    ops.FRAME_SUBSET_FUSED = fused
    try:
        before = dict(ops.FRAME_SUBSET_CALLS)
        xd = x if torch.is_tensor(x) else torch.from_numpy(x).to(dev)
        y, n, index = ops.frame_subset(xd, torch.from_numpy(nf), E, **kw)                     # num_frames may be on the host
        key = "kernels" if fused else "composed"
        assert ops.FRAME_SUBSET_CALLS == dict(before, **{key: before[key] + 1})
    finally:
        ops.FRAME_SUBSET_FUSED = saved
    return y, n, index


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("B,F,D,E,offset", [(1, 4, 1, 1, 0), (3, 5, 20, 3, 0), (2, 8, 1152, 2, 0), (2, 8, 1157, 2, 0), (2, 8, 1152, 2, 1)],
                         ids=["one", "scalar-bytes", "vector", "odd-rows", "vector-unaligned"])
def test_gather_is_the_restatements_bit_for_bit(dev, dtype, B, F, D, E, offset):
    """[3,5,20,3]: 20-byte rows take the scalar path for bytes and the vector path for floats; 1157: no dtype's rows are 16-byte multiples;
    offset: the vector-path shape from a pointer one element past a 16-byte boundary."""
    nf = np.array([F - 1, 1, F][:B], dtype=np.int32)
    x = R.frames(B, F, D, nf, dtype, seed=B * F + D)
    xd = torch.from_numpy(x).to(dev)
    if offset:
        base = torch.zeros(x.size + 16, dtype=xd.dtype, device=dev)
        xd = base[offset:offset + x.size].view(B, F, D)
        xd.copy_(torch.from_numpy(x))
        assert xd.is_contiguous() and xd.data_ptr() % 16 != 0
    got = {}
    for fused in (True, False):
        y, n, index = _run(dev, xd, nf, E, fused, seed=SEED)
        assert y.is_cuda and y.dtype == xd.dtype and tuple(y.shape) == (B * E, F // 2, D) and n.dtype == torch.int32
        assert np.array_equal(index.cpu().numpy(), R.draw(E, F, F // 2, SEED))
        want_y, want_n = R.gather(x, nf, index.cpu().numpy())
        assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(n.cpu().numpy(), want_n), fused
        got[fused] = (y, n)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])   # the switch changes no bit
    y2, n2, _ = _run(dev, xd, nf, E, True, seed=SEED)
    assert torch.equal(y2, got[True][0]) and torch.equal(n2, got[True][1])                         # a rerun is bit-equal


def _seed_with_an_empty_replica(E, F):
    """Chosen on the CPU: a key under which some replica leaves frame 0 out (a video of one frame is then empty in it) and some keeps it"""
    for seed in range(SEED, SEED + 64):
        first = R.draw(E, F, F // 2, seed)[:, 0]
        if (first != 0).any() and (first == 0).any():
            return seed
    raise AssertionError("no such key among 64")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_gather_num_frames_edges_untrusted_padding_and_foreign_indices(dev, dtype):
    B, F, D, E = 5, 8, 48, 3
    nf = np.array([0, 1, F, F + 3, -1], dtype=np.int32)                                       # F + 3 and -1 are clamped to F and 0
    seed = _seed_with_an_empty_replica(E, F)
    x = R.frames(B, F, D, nf, dtype, seed=3, padding=255 if dtype == np.uint8 else 7.5)       # padding content must not come through
    y, n, index = _run(dev, x, nf, E, True, seed=seed)
    want_y, want_n = R.gather(x, nf, R.draw(E, F, F // 2, seed))
    assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(n.cpu().numpy(), want_n)
    n = n.cpu().numpy().reshape(B, E)
    assert (n[0] == 0).all() and (n[4] == 0).all() and (n[2] == F // 2).all() and (n[3] == F // 2).all()
    assert (n[1] == 0).any() and (n[1] == 1).any()                                            # the one-frame video: empty in some replica
    yb = y.cpu().numpy().reshape(B, E, F // 2, D)
    for b in range(B):
        for e in range(E):
            assert float(np.abs(yb[b, e, n[b, e]:].astype(np.float64)).max(initial=0.0)) == 0.0     # zeros behind the real frames
    # a hand-made index: -1 and F are padding -- zero rows, left out of the count, x not read there
    hand = torch.tensor([[-1, 0, F - 1, F], [F, 2, -1, 1], [3, 3, F + 100, -(1 << 31)]], dtype=torch.int32)
    y, n, _ = _run(dev, x, nf, E, True, index=hand.to(dev))
    want_y, want_n = R.gather(x, nf, hand.numpy())
    assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(n.cpu().numpy(), want_n)
    assert want_n.reshape(B, E)[2].tolist() == [2, 2, 2]


# ---- the plugins ---------------------------------------------------------------------------------------------------------------------
B_, F_, D_, E_, H_, V_, M_, LAYERS_ = 2, 8, 1152, 3, 8, 17, 2, 2
NF_ = np.array([8, 1], dtype=np.int32)
HEADS = {"LstmRandomModel": "MoeModel", "FrameRandomEvalModel": "MoeModel", "FrameAttentionEvalModel": "MoeExtendModel"}
# H_ = 8 is the cell width of every LstmMemoryModel case of tests/test_gpu_models.py (the smallest at which that file runs the plugin's
# stack on the device), and 1e-4 on the predictions is the bound those cases apply.
TOL = 1e-4


def _cpu_form(monkeypatch, flm, name, x32, seed, values, kw):
    """The plugin on the CPU graph with the composed op and the same key: the stack, the MoE and the frame pooling, which have no CPU
    form, are the restatements'."""
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.variables import reset_default_graph

    def stack(x_tm, nf, wb, slot=0, **k):
        out, c, h = torch_ref.lstm_stack(x_tm.transpose(0, 1), nf, [(ops.as_tensor(W), ops.as_tensor(b)) for W, b in wb])
        return out.transpose(0, 1).contiguous(), list(zip(c, h))

    with monkeypatch.context() as m:
        m.setattr(seq_ops, "lstm_stack", stack)
        m.setattr(ops, "moe_head", lambda x, Wg, We, be, V, M, **k: moe(x, Wg.data, We.data, be.data, M))
        m.setattr(ops, "frame_pool", lambda x, kind: x.max(dim=1)[0] if kind == "max" else x.mean(dim=1))
        g = reset_default_graph(device=torch.device("cpu"), seed=0)
        run = lambda: getattr(flm, name)().create_model(torch.from_numpy(x32), vocab_size=V_, num_frames=torch.from_numpy(NF_),
                                                        frame_subset_seed=seed, **kw)["predictions"]
        with torch.no_grad():
            run()
            if values is None:
                rs = np.random.RandomState(11)
                values = {k: (rs.randn(*v.data.shape) * (0.1 if v.data.dim() == 1 else 1.0 / np.sqrt(v.data.shape[0]))).astype(np.float32)
                          for k, v in g.vars.items()}
            for k, v in values.items():
                g.vars[k].data.copy_(torch.from_numpy(v))
            g.begin_step()
            return run().numpy().astype(np.float64), values


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "floats"])
@pytest.mark.parametrize("name", ["LstmRandomModel", "FrameRandomEvalModel", "FrameAttentionEvalModel"])
def test_plugins_match_their_cpu_form(dev, flags, monkeypatch, name, u8):
    """B = 2, F = 8, D = 1152, E = 3, 8 cells, num_frames (8, 1): the one-frame video is empty in some replica.  Both settings of the
    switch, which give bit-equal gathered tensors, against the CPU composed path under the same key."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    from yt8m_amd.variables import reset_default_graph
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures, flags.moe_num_extend = str(H_), LAYERS_, M_, E_
    flags.video_level_classifier_model = HEADS[name]
    replicas = E_
    kw = dict(is_training=False)
    if name == "LstmRandomModel":
        flags.lstm_random_frames, replicas, kw = True, 1, {}                                  # a training step on one random half
    seed = _seed_with_an_empty_replica(replicas, F_) if replicas > 1 else \
        next(s for s in range(SEED, SEED + 64) if R.draw(1, F_, F_ // 2, s)[0, 0] != 0)
    assert (R.gather(np.zeros((B_, F_, 1), np.uint8), NF_, R.draw(replicas, F_, F_ // 2, seed))[1] == 0).any()
    q = R.frames(B_, F_, D_, NF_, np.uint8, seed=21)
    x32 = np_ref.dequant_l2norm_folded(q, NF_).astype(np.float32)                             # what the transformer hands over: padding rows zero
    want, values = _cpu_form(monkeypatch, flm, name, x32, seed, None, kw)
    xd, nfd = torch.from_numpy(q if u8 else x32).to(dev), torch.from_numpy(NF_).to(dev)
    gathered = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "FRAME_SUBSET_FUSED", fused)
        gathered[fused] = ops.frame_subset(xd, nfd, replicas, seed=seed)[:2]
        g = reset_default_graph(device=dev, seed=0)
        g.begin_step()
        run = lambda: getattr(flm, name)().create_model(xd, vocab_size=V_, num_frames=nfd, frame_subset_seed=seed, **kw)["predictions"]
        with torch.no_grad():
            run()
            assert list(g.vars) == list(values)
            for k, v in values.items():
                g.vars[k].data.copy_(torch.from_numpy(v).to(dev))
            g.begin_step()
            before = dict(ops.FRAME_SUBSET_CALLS)
            got = run()
        torch.cuda.synchronize()
        key = "kernels" if fused else "composed"
        assert ops.FRAME_SUBSET_CALLS == dict(before, **{key: before[key] + 1})
        assert tuple(got.shape) == (B_, V_)
        e = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print("%s %s %s: max |p - cpu form| = %.3g" % (name, "bytes" if u8 else "floats", key, e))
        assert e < TOL, (fused, e)
    assert torch.equal(gathered[True][0], gathered[False][0]) and torch.equal(gathered[True][1], gathered[False][1])
    assert int((gathered[True][1] == 0).sum()) >= 1
