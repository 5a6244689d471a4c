"""Data augmenters on the MI355X (csrc/augment.hip, data_augmentation.py, TrainGraph.step): the kernels against the numpy restatement of
half_augmenter.py / half_video_augmenter.py (test_augment_host.py), the frame-level noise against dequantise + yt8m_add_noise_f32, the
byte path of HalfAugmenter through three plugins at full width against the same plugins fed the reference's float frames, and whole
training steps against steps fed the explicitly augmented batch."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.data_augmentation as da
import yt8m_amd.frame_level_models as flm
import yt8m_amd.ops as ops
import yt8m_amd.train as train
import yt8m_amd.utils as utils
import yt8m_amd.video_level_models as vlm
from yt8m_amd.variables import AUGMENTER_CALL, random_seed, reset_default_graph
from test_augment_host import dequantize_np, half_augment_np, half_video_augment_np

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(rs, B, F, D, nf):
    """Reader-like bytes: random frames, zero bytes on the padding frames."""
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    for b, n in enumerate(nf):
        q[b, n:] = 0
    return q


NF9 = np.array([0, 1, 2, 9, 3, 8, 5], dtype=np.int32)                    # F = 9: n = 0, 1, 2, F, odd, F - 1, ...


@pytest.mark.parametrize("D", [1152, 64, 13])                           # the reader's width, 16-byte rows, the element fall-back
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_half_segments_equal_the_restatement_bit_for_bit(dev, D, dtype):
    rs = np.random.RandomState(D)
    B, F = len(NF9), 9
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)             # padding bytes too: the originals keep them as they are
    x = q if dtype == "u8" else (rs.randn(B, F, D).astype(np.float32))
    y, nf = ops.half_segments(torch.from_numpy(x).to(dev), torch.from_numpy(NF9))
    ref, nf_ref = half_augment_np(x, NF9)
    assert y.dtype == torch.from_numpy(x).dtype and nf.is_cuda
    assert np.array_equal(nf.cpu().numpy(), nf_ref)
    assert np.array_equal(y.cpu().numpy(), ref)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_half_segments_refuse_overlapping_operands(dev, dtype):
    B, F, D = 2, 4, 16
    buf = torch.zeros(4 * B * F * D, dtype=dtype, device=dev)
    nf = torch.tensor([4, 2], dtype=torch.int32, device=dev)
    nfo = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    fn = L.lib().yt8m_half_segments_u8 if dtype == torch.uint8 else L.lib().yt8m_half_segments_f32
    with pytest.raises(ValueError, match="overlap"):
        L.check(fn(_p(buf), _p(nf), _p(buf[B * F * D // 2:]), _p(nfo), B, F, D, _st()))
    with pytest.raises(ValueError, match="overlap"):
        L.check(fn(_p(buf), _p(nf), _p(buf[B * F * D:]), _p(buf[B * F * D:]), B, F, D, _st()))
    L.check(fn(_p(buf), _p(nf), _p(buf[B * F * D:]), _p(nfo), B, F, D, _st()))      # disjoint: fine
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [1152, 13])
def test_half_segment_means_against_fp64_and_the_video_mean_kernel(dev, D):
    rs = np.random.RandomState(7 + D)
    B, F = len(NF9), 9
    q = _frames(rs, B, F, D, NF9)
    qd = torch.from_numpy(q).to(dev)
    m = ops.half_segment_means(qd, torch.from_numpy(NF9)).cpu().numpy().astype(np.float64)
    ref, _ = half_video_augment_np(dequantize_np(q, NF9).astype(np.float64), NF9)
    assert np.isnan(ref[0]).all() and not m[0].any()                      # n = 0: the reference's 0/0, pinned to 0
    live = ~np.isnan(ref).any(axis=1)
    assert np.abs(m[live] - ref[live]).max() <= 1e-6 * np.abs(ref[live]).max()
    assert not m[2 * B + 1].any() and not m[B].any() and not m[2 * B].any()   # n = 1: second half zero; n = 0: both halves zero
    assert np.abs(m[B + 1] - dequantize_np(q, NF9)[1, 0]).max() <= 1e-6 * 2  # n = 1: the first half is frame 0
    mn = ops.half_segment_means(qd, torch.from_numpy(NF9).to(dev), l2norm=True)
    whole = ops.dequant_mean_l2norm(qd, torch.from_numpy(NF9).to(dev))
    assert torch.equal(mn[:B], whole)                                     # bit for bit
    ref_n = np.nan_to_num(ref) / np.maximum(np.sqrt((np.nan_to_num(ref) ** 2).sum(axis=1, keepdims=True)), 1e-6)
    assert np.abs(mn.cpu().numpy() - ref_n).max() < 1e-6


@pytest.mark.parametrize("D", [1152, 13])
def test_dequant_noise_is_dequantise_then_add_noise_bit_for_bit(dev, D):
    rs = np.random.RandomState(3)
    B, F, sigma, seed = 5, 40, 0.2, 0x1234567890ABCDEF
    nf = np.array([40, 0, 1, 17, 39], dtype=np.int32)
    q = torch.from_numpy(_frames(rs, B, F, D, nf)).to(dev)
    nft = torch.from_numpy(nf).to(dev)
    y = ops.dequant_noise(q, nft, sigma, seed)
    live = (torch.arange(F, device=dev).view(1, F) < nft.view(B, 1)).unsqueeze(2)
    x = torch.where(live, utils.Dequantize(q), torch.zeros((), device=dev))
    assert torch.equal(ops.dequantize_frames(q, nft), x)
    assert torch.equal(y, ops.add_noise(x, sigma, seed=seed))
    pad = (y - x)[~live.expand(B, F, D)].double()
    assert pad.numel() == int((F - nf).sum()) * D
    tol = 5 * sigma / np.sqrt(pad.numel())                                # 5 standard errors
    assert abs(pad.mean().item()) < tol and abs(pad.std().item() - sigma) < tol


def _plugin_run(cls, x, y, nf, dev, seen):
    """predictions, loss and every parameter gradient of one forward + backward pass (graph seed 0: the same initial weights)."""
    g = reset_default_graph(device=dev, seed=0)
    model = cls()
    create = model.create_model

    def spy(model_input, **kw):
        seen.append(model_input.dtype)
        return create(model_input, **kw)
    model.create_model = spy
    tg = train.TrainGraph(model, batch_size=x.shape[0] // 3, graph=g)
    tg.forward(x, y, nf)
    g.finalize()
    res = tg.forward(x, y, nf)
    loss = tg.loss(res, y)
    loss.backward()
    grads = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if v.trainable}
    return res["predictions"].detach().cpu().numpy().astype(np.float64), float(loss.detach()), grads


@pytest.mark.parametrize("B,short", [(40, False), (128, False), (40, True)])
@pytest.mark.parametrize("which", ["LstmModel", "CnnDeepCombineChainModel", "LstmPositionalAttentionMaxPoolingModel"])
def test_half_augmenter_byte_path_through_the_plugins_at_full_width(dev, flags, B, which, short):
    """The uint8 batch HalfAugmenter makes (3B videos, still bytes) through the plugin's byte path, against the same plugin fed the
    float frames the reference's augmenter makes (dequantised frames, split, l2-normalised by the transformer).  short: a video of
    one frame sends the whole batch through the float fall-back."""
    rs = np.random.RandomState(B)
    F, D, V = 300, 1152, 4716
    nf = rs.randint(2, F + 1, size=B).astype(np.int32)
    nf[0], nf[1], nf[2] = F, 2, 3
    if short:
        nf[3] = 1
    q = _frames(rs, B, F, D, nf)
    labels = torch.from_numpy(rs.rand(B, V) < 3.4 / V).to(dev)
    x, y3, nf3 = da.HalfAugmenter().augment(torch.from_numpy(q).to(dev), num_frames=torch.from_numpy(nf), labels_batch=labels)
    assert x.shape == (3 * B, F, D) and x.dtype == (torch.float32 if short else torch.uint8) and y3.shape == (3 * B, V)
    cls = getattr(flm, which)
    seen_a, seen_b = [], []
    pa, la, ga = _plugin_run(cls, x, y3, nf3, dev, seen_a)
    xf, nff = half_augment_np(dequantize_np(q, nf), nf)
    assert np.array_equal(nf3.cpu().numpy(), nff)
    xf = torch.from_numpy(xf).to(dev)
    pb, lb, gb = _plugin_run(cls, xf, y3, torch.from_numpy(nff).to(dev), dev, seen_b)
    assert seen_a[-1] == (torch.float32 if short else torch.uint8) and seen_b[-1] == torch.float32
    assert set(ga) == set(gb)
    assert np.abs(pa - pb).max() < 2e-5 and abs(la - lb) < 1e-4 * max(1.0, abs(lb))
    for k in ga:
        assert np.abs(ga[k] - gb[k]).max() <= 2e-4 * max(1.0, np.abs(gb[k]).max()), k


def _params(g):
    return {k: v.data.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items()}


def _close(pa, pb, tol):
    assert set(pa) == set(pb)
    for k in pa:
        assert np.abs(pa[k] - pb[k]).max() <= tol * max(1.0, np.abs(pb[k]).max()), k


def test_half_augmenter_training_step_equals_the_step_on_the_tiled_batch(dev, flags):
    flags.lstm_cells = "256"
    rs = np.random.RandomState(5)
    B, F, D, V = 16, 32, 64, 33
    nf = rs.randint(2, F + 1, size=B).astype(np.int32)
    q = _frames(rs, B, F, D, nf)
    labels = rs.rand(B, V) < 0.1
    kw = dict(batch_size=B, learning_rate_decay_examples=2.5 * B, learning_rate_decay=0.5)

    def run(augmenter, x, y, n):
        g = reset_default_graph(device=dev, seed=0)
        tg = train.TrainGraph(flm.LstmModel(), graph=g, augmenter_class=augmenter, **kw)
        n = torch.from_numpy(n) if augmenter else torch.from_numpy(n).to(dev)         # the augmenter takes the reader's host copy
        outs = [tg.step(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), n) for _ in range(2)]
        return tg, g, outs

    tga, ga, oa = run(da.HalfAugmenter, q, labels, nf)
    qt, nft = half_augment_np(q, nf)
    _, gb, ob = run(None, qt, np.concatenate([labels] * 3), nft)
    assert oa[0]["predictions"].shape[0] == 3 * B
    assert [o["learning_rate"] for o in oa] == [0.01, 0.01]               # batch_size examples per step, not 3B (which would decay)
    assert abs(float(oa[1]["loss"]) - float(ob[1]["loss"])) < 1e-4 * max(1.0, abs(float(ob[1]["loss"])))
    _close(_params(ga), _params(gb), 2e-5)
    res = tga.forward(torch.from_numpy(q).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(nf).to(dev), is_training=False)
    assert res["predictions"].shape[0] == B
    flags.data_augmenter = "HalfAugmenter"
    assert type(train.build_graph(flm.LstmModel(), graph=reset_default_graph(device=dev, seed=0)).augmenter) is da.HalfAugmenter


def test_half_video_augmenter_training_step_with_the_chain_model(dev, flags):
    flags.deep_chain_layers, flags.deep_chain_relu_cells = 2, 32
    rs = np.random.RandomState(9)
    B, F, D, V = 24, 30, 1152, 50
    nf = rs.randint(2, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = 1, 0
    q = _frames(rs, B, F, D, nf)
    labels = rs.rand(B, V) < 0.1

    def run(augmenter, x, y, n):
        g = reset_default_graph(device=dev, seed=0)
        tg = train.TrainGraph(vlm.DeepCombineChainModel(), batch_size=B, graph=g, augmenter_class=augmenter)
        out = tg.step(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(n).to(dev))
        return g, out

    ga, oa = run(da.HalfVideoAugmenter, q, labels, nf)
    m, nfm = half_video_augment_np(dequantize_np(q, nf), nf)
    gb, ob = run(None, np.nan_to_num(m).astype(np.float32), np.concatenate([labels] * 3), nfm)
    assert oa["predictions"].shape[0] == 3 * B
    assert abs(float(oa["loss"]) - float(ob["loss"])) < 1e-4 * max(1.0, abs(float(ob["loss"])))
    _close(_params(ga), _params(gb), 2e-4)


def test_video_level_noise_augmenter_training_step_with_the_chain_model(dev, flags):
    flags.deep_chain_layers, flags.deep_chain_relu_cells = 2, 32
    rs = np.random.RandomState(11)
    B, D, V = 32, 1152, 50
    x = rs.randn(B, D).astype(np.float32)
    labels = rs.rand(B, V) < 0.1

    def run(augmenter, xin):
        g = reset_default_graph(device=dev, seed=0)
        tg = train.TrainGraph(vlm.DeepCombineChainModel(), batch_size=B, graph=g, augmenter_class=augmenter)
        tg.step(xin, torch.from_numpy(labels).to(dev))
        return g

    ga = run(da.NoiseAugmenter, torch.from_numpy(x).to(dev))
    seed = random_seed(0, 0, 0, AUGMENTER_CALL)                           # the first step's augmenter key
    xn = ops.add_noise(torch.from_numpy(x).to(dev), flags.input_noise_level, seed=seed)
    pa, pb = _params(ga), _params(run(None, xn))
    _close(pa, pb, 0.0)
    pc = _params(run(None, torch.from_numpy(x).to(dev)))                  # and the noise did something
    assert any(not np.array_equal(pa[k], pc[k]) for k in pc)
