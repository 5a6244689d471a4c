"""The fused link kernel (csrc/chain_link.hip) and the four Distillchain cascade plugins on the MI355X: the kernel through the C ABI
against an fp64 restatement written here, ops.chain_link fused against composed, the plugins through the plugin surface against fp64
restatements assembled from oracle.torch_ref (lstm_stack, moe, cross_entropy), the video-level plugin under elu + noise + dropout, and
whole training steps with their bitwise replay."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.variables import reset_default_graph

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-12))         # what the kernel receives: the float32 nearest 1e-12
ACT = {"relu": 1, "elu": 4}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the link in torch on the CPU, in the dtype of its inputs -------------------------------------------------------------------------
def _link_fwd_ref(z, n, kind):
    """(y, rinv): a = act(z) (+ n), ss = sum a^2, r = rsqrt(max(ss, eps)), y = a r, rinv = r where ss > eps else -r."""
    a = torch.relu(z) if kind == "relu" else torch.where(z > 0, z, torch.exp(z) - 1.0)
    if n is not None:
        a = a + n
    ss = (a * a).sum(1, keepdim=True)
    eps = torch.tensor(EPS, dtype=z.dtype)
    r = 1.0 / torch.sqrt(torch.maximum(ss, eps))
    return a * r, torch.where(ss > eps, r, -r).squeeze(1)


def _link_bwd_ref(z, y, rinv, g, kind):
    """dz from the output: da = R (g - y (y.g)) where rinv > 0 else R g, R = |rinv|; dz = da act'(z), relu' = [z > 0]."""
    R = rinv.abs()[:, None]
    k = (y * g).sum(1, keepdim=True)
    da = torch.where(rinv[:, None] > 0, R * (g - y * k), R * g)
    one = torch.ones_like(z)
    return da * (torch.where(z > 0, one, torch.zeros_like(z)) if kind == "relu" else torch.where(z > 0, one, torch.exp(z)))


def _bound(ref32, ref64):
    """4 x the error of the float32 restatement against the fp64 one, plus one float32 ulp of the largest reference magnitude."""
    big = float(ref64.abs().max()) if ref64.numel() else 0.0
    return 4.0 * float((ref32.double() - ref64).abs().max()) + float(np.spacing(np.float32(big)))


def _case(rows, cols, seed):
    """z with row 0 all <= 0 (two exact zeros among them), row 1 scaled to |z| ~ 1e-8 (ss < eps), a relu tie z == 0 on a later row;
    dy ~ N(0, 1) except on row 1, where it is scaled by 1e-6: the eps branch multiplies it by 1e6, and a per-case bound that adds an
    ulp of the LARGEST magnitude would otherwise stop checking the other rows."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, cols, generator=gen)
    z[0] = -z[0].abs()
    z[0, 0] = 0.0
    z[0, cols - 1] = 0.0
    z[1] *= 1e-8
    if rows > 2:
        z[2, cols // 2] = 0.0
    g = torch.randn(rows, cols, generator=gen)
    g[1] *= 1e-6
    return z, g


SHAPES = [(3, 5),          # partial wave, partial workgroup
          (7, 100),        # cols % 4 == 0 with a tail wave pass
          (5, 257),        # the unaligned single-element path across several passes
          (4, 1024),       # the register-resident limit ...
          (2, 1028),       # ... and the two-read loop above it
          (130, 256)]      # the model's width across many workgroups
OFFSET = {100: 28, 256: 520}           # whole Philox blocks per 16-byte access there; elsewhere rows + 2 (5, 7, 6, 4)


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("kind", ["relu", "elu"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_link_kernels_against_the_fp64_restatement(dev, rows, cols, kind, noise):
    """yt8m_chain_link_fwd / _bwd through ctypes.  Per case and per output the bound is 4 x the largest error of the float32 CPU
    restatement of the same formulas against the fp64 one on the same inputs (never the kernel's output) + one float32 ulp of the largest
    reference magnitude.  rinv is bounded per branch (the rows with ss > eps and the others apart: 1e6 next to ~0.1), its signs and the
    zero patterns are exact.  The noise is what ops.add_noise adds to a zero tensor at the same seed and offset.  The backward kernel
    reads the forward kernel's y and rinv, as the op does.  Guard words behind every output keep their sentinel."""
    lib = L.lib()
    z, g = _case(rows, cols, 100 * rows + cols)
    stddev, seed, offset = (0.3, 0x1234567890ABCDEF + cols, OFFSET.get(cols, rows + 2)) if noise else (0.0, 0, 0)
    n = ops.add_noise(torch.zeros(rows, cols, device=dev), stddev, seed, offset).cpu() if noise else None
    if noise:
        assert 0.1 < float(n.abs().max()) < 6 * stddev                 # noise of the asked size, not zeros
    zd, gd = z.to(dev), g.to(dev)
    yd = torch.full((rows * cols + 8,), -7.0, device=dev)
    dzd = torch.full((rows * cols + 8,), -7.0, device=dev)
    rd = torch.full((rows + 8,), -7.0, device=dev)
    L.check(lib.yt8m_chain_link_fwd(ACT[kind], _p(zd), _p(yd), _p(rd), rows, cols, EPS, stddev, seed, offset, _st()))
    L.check(lib.yt8m_chain_link_bwd(ACT[kind], _p(zd), _p(yd), _p(rd), _p(gd), _p(dzd), rows, cols, EPS, _st()))
    torch.cuda.synchronize()
    assert bool((yd[rows * cols:] == -7.0).all()) and bool((dzd[rows * cols:] == -7.0).all()) and bool((rd[rows:] == -7.0).all())
    y, dz, rinv = yd[:rows * cols].view(rows, cols).cpu(), dzd[:rows * cols].view(rows, cols).cpu(), rd[:rows].cpu()

    y64, r64 = _link_fwd_ref(z.double(), None if n is None else n.double(), kind)
    y32, r32 = _link_fwd_ref(z, n, kind)
    dz64 = _link_bwd_ref(z.double(), y64, r64, g.double(), kind)
    dz32 = _link_bwd_ref(z, y32, r32, g, kind)
    assert torch.equal(rinv > 0, r64 > 0)                                 # the eps branch, exactly
    # all rows, then the rows other than the scaled one: under elu, exp(z) - 1 of |z| ~ 1e-8 is 0 in float32 and -1e-8 in fp64, and the
    # restatement's own error on that row (1e-2 after the 1e6) would otherwise be the bound of every row
    others = torch.arange(rows) != 1
    for sel, tag in ((slice(None), "all rows"), (others, "rows != 1")):
        b_y, b_dz = _bound(y32[sel], y64[sel]), _bound(dz32[sel], dz64[sel])
        e_y, e_dz = float((y[sel].double() - y64[sel]).abs().max()), float((dz[sel].double() - dz64[sel]).abs().max())
        print("(%d,%d) %s noise=%d %s: y err %.3g (bound %.3g)  dz err %.3g (bound %.3g)" % (rows, cols, kind, noise, tag, e_y, b_y, e_dz, b_dz))
        assert e_y <= b_y, tag
        assert e_dz <= b_dz, tag
    for branch in (r64 > 0, r64 <= 0):
        if bool(branch.any()):
            b_r = _bound(r32[branch], r64[branch])
            e_r = float((rinv[branch].double() - r64[branch]).abs().max())
            print("    rinv %s: err %.3g (bound %.3g)" % ("ss > eps" if bool(r64[branch][0] > 0) else "ss <= eps", e_r, b_r))
            assert e_r <= b_r
    zsel = slice(None) if kind == "relu" else others                      # (elu on the scaled row: see above)
    assert torch.equal(y[zsel] == 0, y64[zsel] == 0) and torch.equal(dz[zsel] == 0, dz64[zsel] == 0)      # the zero patterns
    assert bool(rinv[1] < 0) == (not noise)                               # the scaled row takes the eps branch unless noise lifts it
    if kind == "relu" and not noise:
        assert bool((y[0] == 0).all()) and bool((dz[0] == 0).all()) and float(rinv[0]) == -1e6
        assert float(rinv[1]) == -1e6 and float(dz[1].abs().max()) > 0   # the eps branch of the backward pass: 1e6 dy on z > 0
    if rows > 2 and kind == "relu":
        assert float(dz[2, cols // 2]) == 0.0                             # a tie at 0 gets 0


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
def _op_run(z, coef, fused, monkeypatch, **kw):
    monkeypatch.setattr(ops, "CHAIN_LINK_FUSED", fused)
    zd = z.clone().requires_grad_(True)
    y = ops.chain_link(zd, **kw)
    (y * coef).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), zd.grad.cpu()


@pytest.mark.parametrize("rows,cols", [(5, 257), (130, 256)])
@pytest.mark.parametrize("kind,noise_level", [("relu", None), ("elu", 0.3)])
def test_op_fused_against_composed(dev, monkeypatch, rows, cols, kind, noise_level):
    """ops.chain_link with the kernel and with YT8M_CHAIN_LINK_FUSED=0's composed activation -> add_noise -> l2_normalize, values and the
    gradient through torch.autograd, under the kernel test's bound (the float32 restatement against the fp64 one)."""
    z, g = _case(rows, cols, 7 * rows + cols)
    seed, offset = 99, 4
    kw = dict(kind=kind, noise_level=noise_level, seed=seed, offset=offset)
    n = ops.add_noise(torch.zeros(rows, cols, device=dev), noise_level, seed, offset).cpu() if noise_level else None
    yf, dzf = _op_run(z.to(dev), g.to(dev), True, monkeypatch, **kw)
    yc, dzc = _op_run(z.to(dev), g.to(dev), False, monkeypatch, **kw)
    y64, r64 = _link_fwd_ref(z.double(), None if n is None else n.double(), kind)
    y32, r32 = _link_fwd_ref(z, n, kind)
    dz64 = _link_bwd_ref(z.double(), y64, r64, g.double(), kind)
    dz32 = _link_bwd_ref(z, y32, r32, g, kind)
    b_y, b_dz = _bound(y32, y64), _bound(dz32, dz64)
    e_y, e_dz = float((yf - yc).abs().max()), float((dzf - dzc).abs().max())
    print("(%d,%d) %s: fused - composed y %.3g (bound %.3g) dz %.3g (bound %.3g)" % (rows, cols, kind, e_y, b_y, e_dz, b_dz))
    assert e_y <= b_y and e_dz <= b_dz
    assert float((yf.double() - y64).abs().max()) <= b_y and float((dzf.double() - dz64).abs().max()) <= b_dz
    with pytest.raises(ValueError):
        ops.chain_link(z.to(dev), kind="tanh")


@pytest.mark.parametrize("fused", [True, False])
def test_op_takes_a_seed_only_for_noise(dev, monkeypatch, fused):
    """Without noise (None or 0) the graph's random-seed counter stays where it was, in both forms; with noise both take exactly one
    key, the one ops.add_noise would have taken."""
    monkeypatch.setattr(ops, "CHAIN_LINK_FUSED", fused)
    g = reset_default_graph(device=dev, seed=3)
    g.begin_step()
    z = torch.randn(6, 12, device=dev)
    ops.chain_link(z)
    ops.chain_link(z, "elu", noise_level=0.0)
    assert g._rng_calls == 0
    a = ops.chain_link(z, "elu", noise_level=0.2)
    assert g._rng_calls == 1
    g._rng_calls = 0
    b = ops.l2_normalize(ops.add_noise(ops.activation(z, "elu"), 0.2))
    assert g._rng_calls == 1
    # the same draw: the two forms differ in the order of a 12-term sum of squares (<= 12 ulp of ss, half of that in r) on rows of
    # norm 1; another key would move the values by the noise's whole 0.2
    assert float((a - b).abs().max()) <= 16 * float(np.finfo(np.float32).eps)


# ---- the plugins against fp64 ---------------------------------------------------------------------------------------------------------
# Tolerances of tests/test_gpu_lstmcnn.py::test_plugins_match_the_fp64_restatement.
P_TOL, LOSS_TOL, GRAD_TOL = 1e-4, 1e-4, 5e-4
V, LAYERS, CELLS, DCELLS, ATT, MIX, S = 11, 2, 8, 12, 2, 2, 0.5


def _flags(flags):
    import yt8m_amd.frame_level_models, yt8m_amd.losses, yt8m_amd.train  # noqa: F401, E401  (define the flags set below)
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.distillchain_relu_cells, flags.moe_num_mixtures = LAYERS, CELLS, DCELLS, MIX
    flags.lstm_layers, flags.lstm_attentions = 2, ATT
    flags.support_type, flags.support_loss_percent = ",".join(["label"] * LAYERS), S


def _l2n(x):
    from oracle import torch_ref
    return torch_ref.l2_normalize(x, 1)


def _moe(x, P, scope):
    from oracle import torch_ref
    return torch_ref.moe(x, P["gates%s/weights" % scope], P["experts%s/weights" % scope], P["experts%s/biases" % scope], MIX)


def _distill_norm(d, P):
    return _l2n(torch.relu(d @ P["distillrelu/weights"] + P["distillrelu/biases"]))


def _layers(P, scope):
    return [(P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)], P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)])
            for l in range(2)]


def _chain_loss(pred, sup, y):
    from oracle import torch_ref
    return (1.0 - S) * torch_ref.cross_entropy(pred, y) + S * torch_ref.cross_entropy(sup, torch.cat([y] * LAYERS, 1))


def _ref_video(x, nf, d, y, P):
    """W/all_video_models/distillchain_deep_combine_chain_model.py:19-60 (relu, no noise, no dropout)."""
    nxt, sup = torch.cat([x, _distill_norm(d, P)], 1), []
    for l in range(LAYERS):
        sp = _moe(nxt, P, "-prediction-%d" % l)
        sup.append(sp)
        nxt = torch.cat([nxt, _l2n(torch.relu(sp @ P["relu-%d/weights" % l] + P["relu-%d/biases" % l]))], 1)
    pred, sup = _moe(nxt, P, "--main"), torch.cat(sup, 1)
    return pred, sup, _chain_loss(pred, sup, y)


def _ref_parallel(x, nf, d, y, P, feature_sizes):
    """distillchain_lstm_parallel_finaloutput_model.py:34-87."""
    from oracle import torch_ref
    states = torch_ref.lstm_parallel_finaloutput(x, nf, [_layers(P, "RNN%d" % i) for i in range(len(feature_sizes))], feature_sizes)
    pred = _moe(torch.cat([states, _distill_norm(d, P)], 1), P, "")
    return pred, None, torch_ref.cross_entropy(pred, y)


def _ref_cnn(x, nf, d, y, P):
    """distillchain_cnn_deep_combine_chain_model.py:47-103: every stage reads [cnn | distill_norm | mean_relu_norm | relu-0 ..]."""
    B, F, D = x.shape
    mask = (torch.arange(F)[None, :] < nf[:, None]).to(x.dtype)
    mean_input = torch.einsum("ijk,ij->ik", x, mask) / nf.to(x.dtype)[:, None]
    relu_layers = [_distill_norm(d, P), _l2n(torch.relu(mean_input @ P["mean-relu/weights"] + P["mean-relu/biases"]))]

    def cnn(k):
        shifts = [x] + [torch.cat([x.new_zeros(B, i, D), x[:, :F - i]], 1) for i in (1, 2)]
        outs = [torch.cat(shifts[:fs], 2) @ P["cnn%dcnn-filter-len%d" % (k, fs)] for fs in (1, 2, 3)]
        return _l2n(torch.cat(outs, 2).max(1).values)

    nxt, sup = torch.cat([cnn(0)] + relu_layers, 1), []
    for l in range(LAYERS):
        sp = _moe(nxt, P, "-prediction-%d" % l)
        sup.append(sp)
        relu_layers.append(_l2n(torch.relu(sp @ P["relu-%d/weights" % l] + P["relu-%d/biases" % l])))
        nxt = torch.cat([cnn(l + 1)] + relu_layers, 1)
    pred, sup = _moe(nxt, P, "--main"), torch.cat(sup, 1)
    return pred, sup, _chain_loss(pred, sup, y)


def _ref_attention(x, nf, d, y, P):
    """distillchain_lstm_attention_max_pooling_model.py:31-85: distill_norm tiled over the A rows of a video, behind the attention output."""
    from oracle import torch_ref
    outputs, _, _ = torch_ref.lstm_stack(x, nf, _layers(P, "RNN"))
    pooled = torch_ref.attention_pool(x, outputs, nf, P["attention-/weights"], P["attention-/biases"])     # [B,A,H]
    B, A, H = pooled.shape
    dn = _distill_norm(d, P)
    inp = torch.cat([pooled, dn[:, None, :].expand(B, A, dn.shape[1])], 2)
    pred = _moe(inp.reshape(B * A, -1), P, "-sub-moe").view(B, A, -1).max(1).values
    return pred, None, torch_ref.cross_entropy(pred, y)


def _plugin(name):
    """(class, chain?, restatement, flag settings, input width, byte-path batch, the parent's byte-path predicate)"""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.video_level_models as vlm
    if name == "video":
        return vlm.DistillchainDeepCombineChainModel, True, _ref_video, {}, 16, None, None
    if name == "parallel":
        return (flm.DistillchainLstmParallelFinaloutputModel, False, lambda *a: _ref_parallel(*a, feature_sizes=[8, 8]),
                dict(lstm_cells="8,4", feature_sizes="8,8"), 16, 3, lambda q: all(flm._lib_u8_ok(fs) for fs in (8, 8)))
    if name == "cnn":
        return (flm.DistillchainCnnDeepCombineChainModel, True, _ref_cnn, {}, 16, 16,
                lambda q: seq_ops.u8_cnn_supported(q) and seq_ops.u8_attention_supported(q, 1))
    return (flm.DistillchainLstmAttentionMaxPoolingModel, False, _ref_attention, dict(lstm_cells="8"), 8, 3,
            lambda q: flm._lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, ATT))


def _data(name, path, dev, seed):
    """(model input as the trainer hands it over, fp64 frames of the restatement, num_frames, labels, distillation predictions, rs)"""
    from oracle import np_ref
    _, _, _, _, D, Bu8, supported = _plugin(name)
    rs = np.random.RandomState(seed)
    B = Bu8 if path == "bytes" else 3
    y = rs.rand(B, V) < 0.2
    d = rs.rand(B, V).astype(np.float32)
    if name == "video":
        x = rs.randn(B, D).astype(np.float32)
        return x, torch.from_numpy(x.astype(np.float64)), None, y, d, rs
    F = 12 if path == "bytes" else 7
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1                                                  # ragged, including 1 and F
    x64 = np_ref.dequant_l2norm_folded(q, nf)
    if path == "bytes":
        assert supported(torch.from_numpy(q).to(dev)), "the shape of this case must take the parent's byte path"
        return q, torch.from_numpy(x64), nf, y, d, rs
    return x64.astype(np.float32), torch.from_numpy(x64), nf, y, d, rs


def _graph(name, x, y, nf, d, dev, seed=0):
    """The plugin's TrainGraph after one forward pass (variables created, arenas frozen).  Float frames arrive transformed already."""
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    cls, chain = _plugin(name)[:2]
    g = reset_default_graph(device=dev, seed=seed)
    tg = train.TrainGraph(cls(), label_loss_fn=losses.MultiTaskCrossEntropyLoss() if chain else None, multitask=chain,
                          batch_size=x.shape[0], graph=g,
                          transformer_class=None if x.dtype == np.uint8 else ft.IdenticalTransformer)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), None if nf is None else torch.from_numpy(nf).to(dev))
    kw = {} if d is None else {"distillation_predictions": torch.from_numpy(d).to(dev)}
    tg.forward(*args, **kw)
    g.finalize()
    return g, tg, args, kw


def _draw(g, rs):
    """A contractive recurrence (0.06), filters at the initialiser's 0.1, heads and FCs 0.2 (as tests/test_gpu_lstmcnn.py)."""
    scale = lambda k: 0.06 if "basic_lstm_cell" in k else (0.1 if "cnn-filter" in k else 0.2)
    return {k: (rs.randn(*v.data.shape) * scale(k)).astype(np.float32) for k, v in g.vars.items()}


def _inject(g, P, dev):
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))


CASES = [("video", "floats"), ("parallel", "floats"), ("parallel", "bytes"), ("cnn", "floats"), ("cnn", "bytes"),
         ("attention", "floats"), ("attention", "bytes")]


@pytest.mark.parametrize("name,path", CASES)
def test_plugins_match_the_fp64_restatement(dev, flags, name, path):
    """Each plugin through TrainGraph.forward / loss / backward at B = 3 (16 where the CNN's byte path wants whole K blocks), F = 7
    (floats) or 12 (bytes) with ragged num_frames including 1 and F, V = 11, 2 chain layers, 8 relu cells, 12 distillrelu cells, 2
    attentions, two-layer stacks of 8 (and 4) cells, at the smallest width the parent's byte-path predicate accepts: predictions,
    support predictions where there are any, the loss and the gradient of EVERY variable against the fp64 restatement.  The restatement
    takes plain fp64 maxima: a seed on which fp32 and fp64 disagree about an argmax is to be changed, the bounds stay."""
    _flags(flags)
    cls, chain, ref, fl, _, _, _ = _plugin(name)
    for k, v in fl.items():
        setattr(flags, k, v)
    x, x64, nf, y, d, rs = _data(name, path, dev, 11 + len(name))
    with pytest.raises(AssertionError, match="distillation feature must be used"):
        _graph(name, x, y, nf, None, dev)
    g, tg, args, kw = _graph(name, x, y, nf, d, dev)
    assert {"distillrelu/weights", "distillrelu/biases"} <= set(g.vars)
    assert tuple(g.vars["distillrelu/weights"].data.shape) == (V, CELLS if name == "video" else DCELLS)
    P = _draw(g, rs)
    _inject(g, P, dev)
    res = tg.forward(*args, **kw)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    tp = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in P.items()}
    pr, spr, lr = ref(x64, None if nf is None else torch.from_numpy(nf), torch.from_numpy(d.astype(np.float64)),
                      torch.from_numpy(y).double(), tp)
    lr.backward()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    ep = np.abs(f64(res["predictions"]) - pr.detach().numpy()).max()
    el = abs(float(loss.detach()) - float(lr.detach())) / max(1.0, abs(float(lr.detach())))
    grads = {k: f64(v.grad) for k, v in g.vars.items() if v.trainable}
    assert set(grads) == set(tp)
    unit = lambda k: np.abs(grads[k] - tp[k].grad.numpy()).max() / max(1.0, float(tp[k].grad.abs().max()))
    worst = max(tp, key=unit)
    print("%s %s: predictions %.3g loss %.3g worst gradient %s %.3g" % (name, path, ep, el, worst, unit(worst)))
    assert ep < P_TOL and el < LOSS_TOL
    if chain:
        assert tuple(res["support_predictions"].shape) == (x.shape[0], LAYERS * V)
        assert np.abs(f64(res["support_predictions"]) - spr.detach().numpy()).max() < P_TOL
    else:
        assert "support_predictions" not in res
    assert float(tp["distillrelu/weights"].grad.abs().max()) > 0 and np.abs(grads["distillrelu/weights"]).max() > 0
    for k in tp:
        assert unit(k) <= GRAD_TOL, k


def test_video_plugin_with_elu_noise_and_dropout(dev, flags, monkeypatch):
    """--deep_chain_relu_type=elu, a noise level and dropout: a step from the same seeds is bit-identical, another graph seed moves it,
    and the fused links draw what the composed ones draw (forward passes of the two forms from the same seeds agree to P_TOL; a key
    taken in another order would shift the noise by its whole 0.1)."""
    _flags(flags)
    flags.deep_chain_relu_type, flags.noise_level, flags.dropout, flags.keep_prob = "elu", 0.1, True, 0.75
    flags.distillation_features = flags.distillation_as_input = True     # the step hands the reader's distillation predictions on
    x, _, _, y, d, rs = _data("video", "floats", dev, 23)
    P = None
    params, preds = {}, {}
    for tag, seed, fused in (("a", 5, True), ("b", 5, True), ("other seed", 6, True), ("composed", 5, False)):
        monkeypatch.setattr(ops, "CHAIN_LINK_FUSED", fused)
        g, tg, args, kw = _graph("video", x, y, None, d, dev, seed=seed)
        P = P or _draw(g, rs)
        _inject(g, P, dev)
        g._rng_step = 0                                                  # the step below is forward pass 1 of every graph
        preds[tag] = tg.forward(*args, **kw)["predictions"].detach().cpu()
        g._rng_step = 0
        out = tg.step(*args[:2], distill_labels_batch=kw["distillation_predictions"])
        torch.cuda.synchronize()
        assert np.isfinite(float(out["loss"]))
        params[tag] = g.params.detach().cpu().clone()
    assert torch.equal(params["a"], params["b"]) and torch.equal(preds["a"], preds["b"])
    assert not torch.equal(preds["a"], preds["other seed"])
    e = float((preds["a"] - preds["composed"]).abs().max())
    print("fused - composed predictions under elu + noise + dropout: %.3g" % e)
    assert e < P_TOL


@pytest.mark.parametrize("name", ["video", "parallel", "cnn", "attention"])
def test_whole_training_step_and_its_bitwise_replay(dev, flags, name):
    """One TrainGraph.step per plugin under --distillation_features --distillation_as_input --multitask
    --label_loss=MultiTaskCrossEntropyLoss (the two plugins without a chain take the plain loss), on the byte path where there is one:
    a finite loss, every parameter moved; then a second step taken twice from the same state: bit-identical parameters."""
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    _flags(flags)
    cls, chain, _, fl, _, _, _ = _plugin(name)
    for k, v in fl.items():
        setattr(flags, k, v)
    flags.distillation_features = flags.distillation_as_input = True
    flags.multitask, flags.label_loss = chain, "MultiTaskCrossEntropyLoss" if chain else "CrossEntropyLoss"
    x, _, nf, y, d, rs = _data(name, "floats" if name == "video" else "bytes", dev, 31)
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(cls(), label_loss_fn=train.find_class_by_name(flags.label_loss, [losses])(), batch_size=x.shape[0], graph=g)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)) + (() if nf is None else (torch.from_numpy(nf).to(dev),))
    kw = dict(distill_labels_batch=torch.from_numpy(d).to(dev))
    out = tg.step(*args, **kw)
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    assert np.isfinite(float(out["loss"]))
    assert "distillrelu/weights" in g.vars
    before = g.params.detach().clone()
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step = tg.global_step
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step = step
        out = tg.step(*args, **kw)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        assert np.isfinite(float(out["loss"]))
        after.append(g.params.detach().clone())
    assert torch.equal(after[0], after[1])
    assert not torch.equal(after[0], before)
