"""Input transformers on the MI355X (csrc/transform.hip, feature_transform.py, TrainGraph): the resolution kernels against the numpy fp64
restatement of resolution_transformer.py (test_transform_host.py) over every load width and grouping, their argument errors, the
AvgTransformer and EngineerTransformer paths, and whole training steps with ResolutionTransformer on the reader's bytes against the
same steps fed the restatement's floats."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.feature_transform as ft
import yt8m_amd.frame_level_models as flm
import yt8m_amd.ops as ops
import yt8m_amd.train as train
from yt8m_amd.variables import reset_default_graph
from test_transform_host import avg_np, dequantize64_np, engineer_np, resolution_np

pytestmark = pytest.mark.gpu

B10, F19 = 10, 19
NF = np.array([0, 1, 3, 4, 5, 16, 17, 19, 8, 15], dtype=np.int32)
U = 2.0 ** -24                                                           # fp32 unit round-off


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(rs, B, F, D, nf):
    """Reader-like bytes: random frames, zero bytes on the padding frames."""
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    for b, n in enumerate(nf):
        q[b, n:] = 0
    return q


@functools.lru_cache(maxsize=None)
def _case(D):
    """The kernel cases' bytes for one width, and their exact dequantisation (made once, never written to)."""
    q = _frames(np.random.RandomState(100 + D), B10, F19, D, NF)
    x64 = dequantize64_np(q, NF)
    q.setflags(write=False)
    x64.setflags(write=False)
    return q, x64


@functools.lru_cache(maxsize=None)
def _ref(D, r, l2norm):
    y, n_out = resolution_np(_case(D)[1], NF, r, l2norm=bool(l2norm))
    y.setflags(write=False)
    return y, n_out


def _check_against_ref(y, n_out, D, r, l2norm):
    ref, n_ref = _ref(D, r, l2norm)
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
    assert n_out.is_cuda and n_out.dtype == torch.int32 and np.array_equal(n_out.cpu().numpy(), n_ref)
    y = y.cpu().numpy().astype(np.float64)
    err = np.abs(y - ref).max()
    print("D=%d r=%d l2norm=%d: max|y - ref| = %.3g (max|ref| = %.3g)" % (D, r, l2norm, err, np.abs(ref).max()))
    if l2norm:
        assert err < 1e-6
    else:
        assert err <= 1e-6 * np.abs(ref).max()
    empty = (np.arange(F19 // r).reshape(1, -1) * r) >= NF.reshape(-1, 1)         # groups with no real frame
    assert empty.any() and not y[empty].any()
    assert y[~empty].any(axis=-1).all()


# D: 16-byte rows (the reader's width), 16-byte rows again, 4-byte rows only, the element fall-back.
# r: identity grouping, an odd r with F2 = 6, F2 = 4 with a dropped tail, F2 = 2, F2 = 1.
@pytest.mark.parametrize("l2norm", [0, 1])
@pytest.mark.parametrize("r", [1, 3, 4, 8, 19])
@pytest.mark.parametrize("D", [1152, 64, 20, 13])
def test_resolution_mean_u8_against_fp64(dev, D, r, l2norm):
    """l2norm = 0 is where the always-divide-by-r rule of partial groups shows (the normalisation would cancel it)."""
    q = torch.tensor(_case(D)[0]).to(dev)
    y, n_out = ops.resolution_mean(q, torch.from_numpy(NF).to(dev), r, l2norm=bool(l2norm))
    _check_against_ref(y, n_out, D, r, l2norm)
    yh, n_outh = ops.resolution_mean(q, torch.from_numpy(NF), r, l2norm=bool(l2norm))     # num_frames from the host
    assert torch.equal(yh, y) and n_outh.is_cuda and n_outh.dtype == torch.int32 and torch.equal(n_outh, n_out)


# rows wider than a wave keeps in registers (64 lanes x 2 units of 16 bytes, x 8 units of 4 bytes or of 1 byte): the tail of the row
# is scaled in place
@pytest.mark.parametrize("l2norm", [0, 1])
@pytest.mark.parametrize("D", [2064, 2052, 515])
def test_resolution_mean_u8_rows_wider_than_the_registers(dev, D, l2norm):
    q = torch.tensor(_case(D)[0]).to(dev)
    y, n_out = ops.resolution_mean(q, torch.from_numpy(NF).to(dev), 3, l2norm=bool(l2norm))
    _check_against_ref(y, n_out, D, 3, l2norm)


@pytest.mark.parametrize("l2norm", [0, 1])
@pytest.mark.parametrize("r", [1, 3, 4, 8, 19])
@pytest.mark.parametrize("D", [1152, 13, 2052, 515])                     # float4 rows, elements; each also wider than the registers
def test_resolution_mean_f32_on_dequantised_frames_agrees_with_the_byte_kernel(dev, D, r, l2norm):
    q = torch.tensor(_case(D)[0]).to(dev)
    nf = torch.from_numpy(NF).to(dev)
    yq, nq = ops.resolution_mean(q, nf, r, l2norm=bool(l2norm))
    yf, nfo = ops.resolution_mean(ops.dequantize_frames(q, nf), nf, r, l2norm=bool(l2norm))
    assert torch.equal(nq, nfo)
    err = float((yq - yf).abs().max())
    print("D=%d r=%d l2norm=%d: max|f32 - u8| = %.3g" % (D, r, l2norm, err))
    assert err < 1e-6 if l2norm else err <= 1e-6 * float(yq.abs().max())


@pytest.mark.parametrize("r", [1, 3, 4, 8, 19])
@pytest.mark.parametrize("D", [1152, 13])
def test_resolution_mean_f32_is_the_unmasked_mean(dev, D, r):
    """Floats are averaged as they are: the padding rows (non-zero here) count.  Bounds: a sequential fp32 sum of r terms and one
    multiply by 1/r are off by at most (r + 1) u max|x| (u = 2^-24); normalised, the element's and the norm's errors both scale
    with 1 / (the smallest row norm), plus the roundings of the scale and of the product."""
    x = np.random.RandomState(D + r).randn(B10, F19, D).astype(np.float32)
    xd, nf = torch.from_numpy(x).to(dev), torch.from_numpy(NF).to(dev)
    ref, n_ref = resolution_np(x, NF, r, l2norm=False)
    y, n_out = ops.resolution_mean(xd, nf, r, l2norm=False)
    assert np.array_equal(n_out.cpu().numpy(), n_ref)
    tol = (r + 1) * U * np.abs(x).max()
    err = np.abs(y.cpu().numpy() - ref).max()
    print("D=%d r=%d: max|y - ref| = %.3g (bound %.3g)" % (D, r, err, tol))
    assert err <= tol
    refn, _ = resolution_np(x, NF, r)
    yn, _ = ops.resolution_mean(xd, nf, r)
    toln = 2 * tol / np.sqrt((ref ** 2).sum(axis=-1)).min() + 4 * U
    errn = np.abs(yn.cpu().numpy() - refn).max()
    print("D=%d r=%d normalised: max|y - ref| = %.3g (bound %.3g)" % (D, r, errn, toln))
    assert errn <= toln
    # num_frames = NULL (and then no num_frames_out): the same rows
    y0 = torch.full_like(yn, 7.0)
    L.check(L.lib().yt8m_resolution_mean_f32(_p(xd), None, _p(y0), None, B10, F19, D, r, 1, 1e-12, _st()))
    assert torch.equal(y0, yn)


def test_resolution_mean_u8_without_num_frames_takes_every_frame(dev):
    D, r = 64, 4
    q = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(B10, F19, D)).astype(np.uint8)).to(dev)
    full = torch.full((B10,), F19, dtype=torch.int32, device=dev)
    y, n_out = ops.resolution_mean(q, full, r)
    y0, n0 = torch.full_like(y, 7.0), torch.full_like(n_out, -1)
    L.check(L.lib().yt8m_resolution_mean_u8(_p(q), None, _p(y0), _p(n0), B10, F19, D, r, 1, 1e-12, _st()))
    assert torch.equal(y0, y) and n0.tolist() == [F19 // r] * B10
    with pytest.raises(TypeError):
        ops.resolution_mean(q.to(torch.float16), full, r)
    with pytest.raises(ValueError):
        ops.resolution_mean(q[0], full, r)
    for bad in (0, F19 + 1):
        with pytest.raises(ValueError, match="resolution"):
            ops.resolution_mean(q, full, bad)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_resolution_mean_refuses_bad_arguments_and_launches_nothing(dev, dtype):
    B, F, D, r = 2, 8, 16, 2
    n, ny = B * F * D, B * (F // r) * D
    x = torch.ones(n, dtype=dtype, device=dev)
    buf = torch.full((2 * ny + 64,), 7.0, dtype=torch.float32, device=dev)            # y, and room behind it
    nf = torch.tensor([8, 3], dtype=torch.int32, device=dev)
    nfo = torch.full((B,), -1, dtype=torch.int32, device=dev)
    fn = L.lib().yt8m_resolution_mean_u8 if dtype == torch.uint8 else L.lib().yt8m_resolution_mean_f32
    for bad in (0, F + 1):
        with pytest.raises(ValueError, match="resolution"):
            L.check(fn(_p(x), _p(nf), _p(buf), _p(nfo), B, F, D, bad, 1, 1e-12, _st()))
    xin = buf.view(dtype)                                                 # the source inside the destination's buffer
    with pytest.raises(ValueError, match="overlap"):
        L.check(fn(_p(xin), _p(nf), _p(buf[8:]), _p(nfo), B, F, D, r, 1, 1e-12, _st()))
    with pytest.raises(ValueError, match="overlap"):
        L.check(fn(_p(x), _p(nf), _p(buf), _p(buf[ny - 1:].view(torch.int32)), B, F, D, r, 1, 1e-12, _st()))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and nfo.tolist() == [-1, -1]          # nothing ran
    L.check(fn(_p(x), _p(nf), _p(buf), _p(nfo), B, F, D, r, 1, 1e-12, _st()))       # disjoint: fine
    torch.cuda.synchronize()
    assert nfo.tolist() == [4, 1] and bool((buf[ny:] == 7.0).all()) and not bool((buf[:ny] == 7.0).any())


def test_avg_transformer_on_bytes_and_floats(dev):
    D = 64
    q, x64 = _case(D)
    qd, nf = torch.from_numpy(q).to(dev), torch.from_numpy(NF).to(dev)
    a, nfa = ft.AvgTransformer().transform(qd, num_frames=nf)
    assert nfa is nf and torch.equal(a, ops.dequant_mean_l2norm(qd, nf))  # bit for bit
    assert not bool(a[0].any())                                           # n = 0
    x = np.random.RandomState(2).randn(B10, F19, D).astype(np.float32)    # non-zero padding rows: summed like any other
    ref, _ = avg_np(x, NF)
    assert np.isnan(ref[0]).all()
    for nfx in (nf, torch.from_numpy(NF)):                                # num_frames on the device, on the host
        af, nff = ft.AvgTransformer().transform(torch.from_numpy(x).to(dev), num_frames=nfx)
        af = af.cpu().numpy()
        assert nff is nfx and af.shape == (B10, D) and not af[0].any()    # the reference's 0/0, pinned to 0
        assert np.abs(af[1:] - ref[1:]).max() < 1e-6
    ab = a.cpu().numpy()
    assert np.abs(ab[1:] - avg_np(x64, NF)[0][1:]).max() < 1e-6


def _spy_dtype(model, transformer, x, y, nf, dev):
    seen = []
    g = reset_default_graph(device=dev, seed=0)
    create = model.create_model

    def spy(model_input, **kw):
        seen.append((model_input.dtype, tuple(model_input.shape)))
        return create(model_input, **kw)
    model.create_model = spy
    tg = train.TrainGraph(model, batch_size=x.shape[0], graph=g, transformer_class=transformer)
    res = tg.forward(x, y, nf)
    assert bool(torch.isfinite(res["predictions"]).all())
    return seen[-1]


def test_engineer_transformer_keeps_the_byte_path_and_is_the_l2_normalisation(dev, flags):
    flags.lstm_cells = "256"
    rs = np.random.RandomState(4)
    B, F, D, V = 32, 32, 64, 33
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    q = _frames(rs, B, F, D, nf)
    qd, y, nfd = torch.from_numpy(q).to(dev), torch.from_numpy(rs.rand(B, V) < 0.1).to(dev), torch.from_numpy(nf).to(dev)
    assert _spy_dtype(flm.LstmModel(), ft.EngineerTransformer, qd, y, nfd, dev) == (torch.uint8, (B, F, D))
    assert _spy_dtype(flm.LstmModel(), ft.DefaultTransformer, qd, y, nfd, dev) == (torch.uint8, (B, F, D))
    flags.time_resolution = 4
    assert _spy_dtype(flm.LstmModel(), ft.ResolutionTransformer, qd, y, nfd, dev) == (torch.float32, (B, F // 4, D))
    e, nfe = ft.EngineerTransformer().transform(qd, num_frames=nfd)
    assert nfe is nfd and torch.equal(e, ops.dequant_l2norm(qd, nfd))
    x64 = dequantize64_np(q, nf)
    assert np.abs(e.cpu().numpy() - engineer_np(x64)).max() < 1e-6
    ef, _ = ft.EngineerTransformer().transform(torch.from_numpy(x64.astype(np.float32)).to(dev), num_frames=nfd)
    assert np.abs(ef.cpu().numpy() - engineer_np(x64)).max() < 1e-6


def _params(g):
    return {k: v.data.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items()}


@pytest.mark.parametrize("which", ["LstmMemoryModel", "FrameLevelLogisticModel"])
def test_resolution_transformer_training_steps_equal_the_steps_on_the_restatements_floats(dev, flags, which):
    """Run A: two steps on the reader's bytes with ResolutionTransformer.  Run B: the same steps with IdenticalTransformer, fed the
    restatement's floats and n // r.  FrameLevelLogisticModel divides by num_frames: it shows that the transformer's num_frames, not
    the reader's, reaches the model -- and needs n >= r in every video (n // r = 0 is a division by zero in the model, there as
    here), a restriction of that comparison only.

    The byte kernel forms its output in fp64 from exact integer sums and rounds once, so run A's model input equals the restatement's
    floats bit for bit and the runs agree exactly.  (Inputs one ulp apart already move the LstmMemoryModel parameters by 4e-5 in two
    steps: Adam's lr g / (sqrt(v) + 1e-8) amplifies fp32 summation noise in gradient entries near 1e-8.)"""
    flags.lstm_cells = "256"
    flags.time_resolution = r = 4
    rs = np.random.RandomState(6)
    B, F, D, V = 16, 32, 64, 33
    if which == "LstmMemoryModel":
        nf = rs.randint(0, F + 1, size=B).astype(np.int32)
        nf[:4] = [0, 3, 4, 32]
    else:
        nf = rs.randint(r, F + 1, size=B).astype(np.int32)
        nf[:2] = [4, 32]
    q = _frames(rs, B, F, D, nf)
    labels = torch.from_numpy(rs.rand(B, V) < 0.1).to(dev)
    xf, nfr = resolution_np(dequantize64_np(q, nf), nf, r)
    assert np.array_equal(nfr, nf // r)

    def run(transformer, x, n):
        g = reset_default_graph(device=dev, seed=0)
        tg = train.TrainGraph(getattr(flm, which)(), batch_size=B, graph=g, transformer_class=transformer)
        outs = [tg.step(x, labels, n) for _ in range(2)]
        return tg, g, outs

    qd = torch.from_numpy(q).to(dev)
    tga, ga, oa = run(ft.ResolutionTransformer, qd, torch.from_numpy(nf))             # the reader's host copy of num_frames
    _, gb, ob = run(ft.IdenticalTransformer, torch.from_numpy(xf.astype(np.float32)).to(dev), torch.from_numpy(nfr).to(dev))
    la, lb = float(oa[1]["loss"]), float(ob[1]["loss"])
    pa, pb = _params(ga), _params(gb)
    worst = max(np.abs(pa[k] - pb[k]).max() / max(1.0, np.abs(pb[k]).max()) for k in pb)
    print("%s: loss %.7f against %.7f, parameters off by %.3g (relative to max(1, max|p|))" % (which, la, lb, worst))
    assert np.isfinite(lb) and abs(la - lb) < 1e-4 * max(1.0, abs(lb))
    assert set(pa) == set(pb)
    for k in pa:
        assert np.abs(pa[k] - pb[k]).max() <= 2e-5 * max(1.0, np.abs(pb[k]).max()), k
    assert tga.predict(qd, torch.from_numpy(nf), vocab_size=V).shape == (B, V)
    flags.feature_transformer = "ResolutionTransformer"
    assert type(train.build_graph(getattr(flm, which)(), graph=reset_default_graph(device=dev, seed=0)).transformer) \
        is ft.ResolutionTransformer


def test_resolution_transformer_after_the_augmenters(dev, flags):
    """HalfAugmenter's 3B-row byte batch takes the byte kernel, NoiseAugmenter's float batch the float kernel; HalfVideoAugmenter's
    2-D rows are refused."""
    import yt8m_amd.data_augmentation as da
    flags.time_resolution = r = 4
    rs = np.random.RandomState(8)
    B, F, D = 6, 19, 64
    nf = np.array([19, 2, 8, 15, 4, 11], dtype=np.int32)
    q = torch.from_numpy(_frames(rs, B, F, D, nf)).to(dev)
    labels = torch.zeros(B, 5, dtype=torch.bool, device=dev)
    t = ft.ResolutionTransformer()
    xh, _, nfh = da.HalfAugmenter().augment(q, num_frames=torch.from_numpy(nf), labels_batch=labels)
    yh, nh = t.transform(xh, num_frames=nfh)
    assert xh.dtype == torch.uint8 and yh.shape == (3 * B, F // r, D) and yh.dtype == torch.float32
    ref, n_ref = resolution_np(dequantize64_np(xh.cpu().numpy(), nfh.cpu().numpy()), nfh.cpu().numpy(), r)
    assert np.array_equal(nh.cpu().numpy(), n_ref) and np.abs(yh.cpu().numpy() - ref).max() < 1e-6
    xn, _, nfn = da.NoiseAugmenter().augment(q, num_frames=torch.from_numpy(nf), labels_batch=labels, seed=3)
    yn, nn = t.transform(xn, num_frames=nfn)
    refn, nn_ref = resolution_np(xn.cpu().numpy(), nf, r)
    assert xn.dtype == torch.float32 and np.array_equal(nn.cpu().numpy(), nn_ref) and np.abs(yn.cpu().numpy() - refn).max() < 1e-6
    xv, _, nfv = da.HalfVideoAugmenter().augment(q, num_frames=torch.from_numpy(nf), labels_batch=labels)
    with pytest.raises(ValueError, match="--frame_features"):
        t.transform(xv, num_frames=nfv)
