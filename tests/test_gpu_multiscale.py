"""MultiscaleCnnLstmModel / DistillchainMultiscaleCnnLstmModel (W/all_frame_models/multiscale_cnn_lstm_model.py,
distillchain_multiscale_cnn_lstm_model.py) on the MI355X: the batch-norm + ReLU + pair-maximum kernels (csrc/multiscale.hip) through
the C ABI against torch in float64, both plugins through the plugin surface against an fp64 restatement built here
(oracle.torch_ref.batch_norm_train / lstm_stack / moe / cross_entropy around explicit shifted concatenations), the fused time-major
path against the generic composition at the model's own shape, and one whole training step of each."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.variables import reset_default_graph

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
BN_EPS, BN_DECAY = 1e-3, 0.999


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(dev, C):
    n = L.lib().yt8m_multiscale_workspace_bytes(C)
    return torch.empty(n // 4, dtype=torch.float32, device=dev), n


def _maxerr(a, ref64):
    return float((a.double() - ref64).abs().max())


# ---- kernels ----------------------------------------------------------------------------------------------------------------------
def _affine32(y, mean, rstd, gamma, beta):
    return (y - mean) * rstd * gamma + beta                       # bn_apply_kernel's expression, in torch fp32


def _close_to_fp32_affine(got, want32):
    """|got - want| <= 4 eps max(1, |want|): both sides evaluate the same fp32 operations on the same statistics, the kernel with the last
    multiply-add contracted (one rounding fewer) -- at most one ulp of the product plus one of the sum."""
    return bool(((got - want32).abs() <= 4 * EPS32 * want32.abs().clamp(min=1.0)).all())


def _kernel_inputs(dev, F, B, C, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    M = F * B
    colscale = 0.5 + torch.rand(C, generator=g) * 2.0
    colshift = torch.randn(C, generator=g)
    y = (torch.randn(M, C, generator=g) * colscale + colshift).to(dev)
    gamma = (0.5 + torch.rand(C, generator=g)).to(dev)
    beta = (torch.rand(C, generator=g) - 0.5).to(dev)
    return y, gamma, beta


@pytest.mark.parametrize("F,B,C", [(7, 3, 8), (66, 32, 1024), (300, 128, 1024)])   # odd F and B, both stack regimes' rows, the model's shape
def test_colmoments_and_forward_kernel_against_float64(dev, F, B, C):
    lib = L.lib()
    M = F * B
    y, gamma, beta = _kernel_inputs(dev, F, B, C, 11 + F)
    ws, nws = _ws(dev, C)
    mm0 = torch.randn(C, device=dev)
    mv0 = torch.rand(C, device=dev) + 0.5
    mm, mv = mm0.clone(), mv0.clone()
    mean = torch.empty(C, device=dev)
    rstd = torch.empty(C, device=dev)
    L.check(lib.yt8m_colmoments_f32(_p(y), M, C, C, _p(mm), _p(mv), 1, BN_EPS, BN_DECAY, _p(mean), _p(rstd), _p(ws), nws, _st()))
    y64 = y.double()
    mean64 = y64.mean(0)
    var64 = ((y64 - mean64) ** 2).mean(0)
    # column statistics are sums over up to 38 400 terms: bounded by FOUR times the error of torch's own fp32 reduction of the same
    # columns against fp64 (the largest over the columns), measured here on the same data -- the reference for the bound is torch
    # fp32 vs fp64, not the kernel
    t_mean = y.sum(0) / M
    t_var = ((y - t_mean) ** 2).sum(0) / M
    b_mean = 4 * _maxerr(t_mean, mean64)
    b_var = 4 * _maxerr(t_var, var64)
    e_mean, e_var = _maxerr(mean, mean64), None
    var_k = 1.0 / rstd.double() ** 2 - BN_EPS                   # the variance the kernel's rstd stands for
    # (rstd itself is one sqrt and one division away from var: 2 ulp of rstd = 4 ulp of var + eps, relative)
    e_var = float(((var_k - var64).abs() - 4 * EPS32 * (var64 + BN_EPS)).clamp(min=0).max())
    print("colmoments (%d,%d,%d): mean err %.3g (bound %.3g), var err beyond rstd rounding %.3g (bound %.3g)" % (F, B, C, e_mean, b_mean, e_var, b_var))
    assert e_mean <= b_mean
    assert e_var <= b_var
    # moving averages: yt8m_batchnorm_fwd's expression on the kernel's own mean / variance
    dec, om = float(np.float32(BN_DECAY)), float(np.float32(1.0) - np.float32(BN_DECAY))       # the kernel's fp32 constants
    assert _close_to_fp32_affine(mm, dec * mm0 + om * mean)
    want_mv = BN_DECAY * mv0.double() + (1.0 - BN_DECAY) * var64
    assert float((mv.double() - want_mv).abs().max()) <= 4 * EPS32 * float(want_mv.abs().max()) + (1.0 - BN_DECAY) * b_var

    # forward: a, p against the fp32 torch expression on the kernel's statistics; margins of ldy / lda / ldp = C + 8 keep their sentinel
    a = torch.empty(F, B, C, device=dev)
    p = torch.empty(F // 2, B, C, device=dev)
    L.check(lib.yt8m_bn_relu_pool2_tm_fwd(_p(y), C, F, B, C, _p(gamma), _p(beta), _p(mean), _p(rstd), _p(a), C, _p(p), C, _st()))
    a32 = torch.relu(_affine32(y, mean, rstd, gamma, beta)).view(F, B, C)
    assert _close_to_fp32_affine(a, a32)
    assert torch.equal(p, torch.maximum(a[0:F // 2 * 2:2], a[1:F // 2 * 2:2]))            # the pooling itself is exact
    assert float((a > 0).float().mean()) > 0.2                       # a fair share of both ReLU branches
    yw = torch.full((M, C + 8), -7.0, device=dev)
    yw[:, :C] = y
    aw = torch.full((F, B, C + 8), -7.0, device=dev)
    pw = torch.full((F // 2, B, C + 8), -7.0, device=dev)
    L.check(lib.yt8m_bn_relu_pool2_tm_fwd(_p(yw), C + 8, F, B, C, _p(gamma), _p(beta), _p(mean), _p(rstd), _p(aw), C + 8, _p(pw), C + 8, _st()))
    assert torch.equal(aw[:, :, :C], a) and torch.equal(pw[:, :, :C], p)
    assert bool((aw[:, :, C:] == -7.0).all()) and bool((pw[:, :, C:] == -7.0).all()) and bool((yw[:, C:] == -7.0).all())
    mean_w = torch.empty(C, device=dev)
    rstd_w = torch.empty(C, device=dev)
    L.check(lib.yt8m_colmoments_f32(_p(yw), M, C, C + 8, _p(mm.clone()), _p(mv.clone()), 1, BN_EPS, BN_DECAY, _p(mean_w), _p(rstd_w), _p(ws), nws, _st()))
    assert torch.equal(mean_w, mean) and torch.equal(rstd_w, rstd)   # fixed-order reduction: the leading dimension changes nothing
    # pooled = NULL (the last scale): a unchanged
    a2 = torch.empty_like(a)
    L.check(lib.yt8m_bn_relu_pool2_tm_fwd(_p(y), C, F, B, C, _p(gamma), _p(beta), _p(mean), _p(rstd), _p(a2), C, None, C, _st()))
    assert torch.equal(a2, a)
    # inference mode: the moving statistics, which stay as they are
    mm1, mv1 = mm.clone(), mv.clone()
    L.check(lib.yt8m_colmoments_f32(None, M, C, C, _p(mm1), _p(mv1), 0, BN_EPS, BN_DECAY, _p(mean_w), _p(rstd_w), None, 0, _st()))
    assert torch.equal(mm1, mm) and torch.equal(mv1, mv) and torch.equal(mean_w, mm)
    assert _close_to_fp32_affine(rstd_w, 1.0 / torch.sqrt(mv + BN_EPS))
    L.check(lib.yt8m_bn_relu_pool2_tm_fwd(_p(y), C, F, B, C, _p(gamma), _p(beta), _p(mean_w), _p(rstd_w), _p(a2), C, _p(p), C, _st()))
    assert _close_to_fp32_affine(a2, torch.relu(_affine32(y, mean_w, rstd_w, gamma, beta)).view(F, B, C))
    assert torch.equal(p, torch.maximum(a2[0:F // 2 * 2:2], a2[1:F // 2 * 2:2]))


def _bwd_reference(y, mean, rstd, gamma, beta, da, dp, F, B, C, dtype):
    """g (gradient at the batch norm's output), xhat, column sums and dy in `dtype` from the SAME fp32 inputs.  The pooled gradient goes
    through torch's amax (which splits between equal maxima): the restatement of the tie rule the kernel's comment argues for."""
    c = lambda t: None if t is None else t.to(dtype)
    y_, mean_, rstd_, gamma_, beta_ = c(y), c(mean), c(rstd), c(gamma), c(beta)
    xhat = (y_ - mean_) * rstd_
    v = (xhat * gamma_ + beta_).view(F, B, C).detach().requires_grad_(True)
    a = torch.relu(v)
    out = (a * c(da)).sum() if da is not None else a.sum() * 0
    if dp is not None:
        F2 = F // 2
        out = out + (a[:F2 * 2].view(F2, 2, B, C).amax(1) * c(dp)).sum()
    out.backward()
    g = v.grad.view(F * B, C)
    return g, xhat


@pytest.mark.parametrize("F,B,C,mode", [(F_, B_, C_, m_) for F_, B_, C_ in [(7, 3, 8), (66, 32, 1024)] for m_ in ("train", "last-scale", "inference")] +
                         [(300, 128, 1024, "train")])               # dp = NULL and inference at the two smaller shapes, the model's shape once
def test_backward_kernel_against_float64(dev, F, B, C, mode):
    """dgamma / dbeta / dy for given statistics.  The ReLU mask and the pair argmax are discontinuous in y, so a float64 reference that
    evaluates the affine in another precision would disagree on the few elements within rounding of a switch (tens of millions of
    elements are drawn): the inputs are nudged so that no batch-norm output lies within 1e-3 of zero and no pair of positive outputs
    within 1e-3 of each other -- the statistics are INPUTS of the backward entry point, so they stay those of the un-nudged draw."""
    lib = L.lib()
    M = F * B
    training = mode != "inference"
    y, gamma, beta = _kernel_inputs(dev, F, B, C, 23 + F)
    mean = y.double().mean(0).float()
    rstd = (1.0 / torch.sqrt(((y.double() - mean.double()) ** 2).mean(0) + BN_EPS)).float()
    unit = 1.0 / (rstd * gamma)                                      # a step of y that moves the output by 1
    v = _affine32(y, mean, rstd, gamma, beta)
    y = torch.where(v.abs() < 1e-3, y + 4e-3 * unit * torch.where(v >= 0, 1.0, -1.0), y)
    v = _affine32(y, mean, rstd, gamma, beta).view(F, B, C)
    F2 = F // 2
    close = ((v[0:F2 * 2:2] - v[1:F2 * 2:2]).abs() < 1e-3) & (v[0:F2 * 2:2] > 0) & (v[1:F2 * 2:2] > 0)
    y3 = y.view(F, B, C)
    y3[0:F2 * 2:2] += torch.where(close, 4e-3 * unit, torch.zeros_like(unit))
    g_ = torch.Generator(device="cpu").manual_seed(5)
    da = torch.randn(F, B, C, generator=g_).to(dev)
    dp = torch.randn(F2, B, C, generator=g_).to(dev) if mode != "last-scale" else None
    ws, nws = _ws(dev, C)
    dy = torch.full((M, C + 8), -7.0, device=dev)
    dgamma = torch.full((C,), 3.0, device=dev)                      # dgamma accumulates (beta 1), dbeta overwrites (beta 0)
    dbeta = torch.full((C,), 3.0, device=dev)
    L.check(lib.yt8m_bn_relu_pool2_tm_bwd(_p(y), C, F, B, C, _p(gamma), _p(beta), _p(mean), _p(rstd), int(training), _p(da), C, _p(dp), C,
                                          _p(dy), C + 8, _p(dgamma), 1.0, _p(dbeta), 0.0, _p(ws), nws, _st()))
    assert bool((dy[:, C:] == -7.0).all())
    g64, x64 = _bwd_reference(y, mean, rstd, gamma, beta, da, dp, F, B, C, torch.float64)
    g32, x32 = _bwd_reference(y, mean, rstd, gamma, beta, da, dp, F, B, C, torch.float32)
    assert torch.equal(g64 != 0, g32 != 0)                           # the nudge worked: both precisions take the same switches
    s1, s2 = g64.sum(0), (g64 * x64).sum(0)
    # bound: four times the error of torch's own fp32 evaluation of the same column sums against fp64 (largest over the columns)
    b1 = 4 * _maxerr(g32.sum(0), s1)
    b2 = 4 * _maxerr((g32 * x32).sum(0), s2)
    e1, e2 = _maxerr(dbeta, s1), _maxerr(dgamma - 3.0, s2)
    print("bwd %s (%d,%d,%d): dbeta err %.3g (bound %.3g), dgamma err %.3g (bound %.3g)" % (mode, F, B, C, e1, b1, e2, b2))
    assert e1 <= b1
    assert e2 <= b2 + EPS32 * float((s2.abs() + 3.0).max())           # (+ the rounding of adding onto the 3.0 already there)
    k = (gamma * rstd).double()
    if training:
        dy64 = k * (g64 - s1 / M - x64 * (s2 / M))
        mag = k * (g64.abs() + (s1 / M).abs() + (x64 * (s2 / M)).abs())
        tol = 8 * EPS32 * mag.clamp(min=1.0) + k * (b1 + x64.abs() * b2) / M     # a few roundings of the largest term + the sums' error
    else:
        dy64 = k * g64
        tol = 4 * EPS32 * dy64.abs().clamp(min=1.0)
    assert bool(((dy[:, :C].double() - dy64).abs() <= tol).all())
    # in place of da, parameter gradients not wanted: the same dy
    da2 = da.clone()
    L.check(lib.yt8m_bn_relu_pool2_tm_bwd(_p(y), C, F, B, C, _p(gamma), _p(beta), _p(mean), _p(rstd), int(training), _p(da2), C, _p(dp), C,
                                          _p(da2), C, None, 0.0, None, 0.0, _p(ws), nws, _st()))
    assert torch.equal(da2.view(M, C), dy[:, :C])


# ---- the plugins ------------------------------------------------------------------------------------------------------------------
def _restate(x, nf, labels, P, L_, M_, s, training=True, distill=None):
    """The model in the dtype and on the device of x [B,F,D] (batch-major, as the reference): returns predictions, support predictions,
    the multitask loss (1 - s) CE(p, y) + s CE(support, [y] * L) and the batch moments of every scale."""
    from oracle import torch_ref
    B = x.shape[0]
    inp, n, subs, moments = x, nf, [], []
    dn = None
    if distill is not None:
        dn = torch_ref.l2_normalize(torch.relu(distill @ P["distillrelu/weights"] + P["distillrelu/biases"]))
    for k in range(1, L_ + 1):
        Fk, Dk = inp.shape[1], inp.shape[2]
        outs = []
        for fs in (1, 2, 3):
            shifted = [inp] + [torch.cat([inp.new_zeros(B, i, Dk), inp[:, :Fk - i]], 1) for i in range(1, fs)]
            outs.append(torch.cat(shifted, 2) @ P["cnn%dcnn-filter-len%d" % (k, fs)])
        yk = torch.cat(outs, 2).reshape(B * Fk, -1)
        bn = "cnn%dcluster_bn/" % k
        if training:
            z, mu, var = torch_ref.batch_norm_train(yk, P[bn + "gamma"], P[bn + "beta"], eps=BN_EPS)
            assert float(var.detach().min()) > 1e-3, "a column's batch variance is tiny: the comparison would measure conditioning"
            moments.append((mu.detach(), var.detach()))
        else:
            z = P[bn + "gamma"] * (yk - P[bn + "moving_mean"]) * torch.rsqrt(P[bn + "moving_variance"] + BN_EPS) + P[bn + "beta"]
        a = torch.relu(z).view(B, Fk, -1)
        _, c, _ = torch_ref.lstm_stack(a, n, [(P["RNN-rnn%d/basic_lstm_cell/weights" % k], P["RNN-rnn%d/basic_lstm_cell/biases" % k])])
        head = c[0] if dn is None else torch.cat([c[0], dn], 1)
        subs.append(torch_ref.moe(head, P["gatesmoe%d/weights" % k], P["expertsmoe%d/weights" % k], P["expertsmoe%d/biases" % k], M_))
        inp = a[:, :Fk // 2 * 2].reshape(B, Fk // 2, 2, -1).amax(2)
        n = torch.clamp(n // 2, min=1)
    pred = sum(subs) / float(L_)
    support = torch.cat(subs, 1)
    yl = labels.to(x.dtype)
    loss = (1.0 - s) * torch_ref.cross_entropy(pred, yl) + s * torch_ref.cross_entropy(support, torch.cat([yl] * L_, 1))
    return pred, support, loss, moments


def _draw(shapes, rs, scale=0.06, filter_scale=0.1):
    """Weights for the small-shape comparisons: a contractive recurrence (scale ~ 0.06, as the bidirectional tests), filters at the
    initialiser's 0.1, gamma near 1, beta around 0.2 so that a fair share of the ReLU inputs is positive, fresh moving averages."""
    P = {}
    for k, shp in shapes.items():
        if k.endswith("/gamma"):
            P[k] = 1.0 + 0.1 * rs.randn(*shp)
        elif k.endswith("/beta"):
            P[k] = 0.2 + 0.2 * rs.randn(*shp)
        elif k.endswith("/moving_mean"):
            P[k] = np.zeros(shp)
        elif k.endswith("/moving_variance"):
            P[k] = np.ones(shp)
        elif "cnn-filter" in k:
            P[k] = rs.randn(*shp) * filter_scale
        else:
            P[k] = rs.randn(*shp) * scale
    return {k: v.astype(np.float32) for k, v in P.items()}


def _make_graph(model, x, y, nf, dev, distill=None):
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(model, label_loss_fn=losses.MultiTaskCrossEntropyLoss(), multitask=True, batch_size=x.shape[0], graph=g)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    kw = {} if distill is None else {"distillation_predictions": torch.from_numpy(distill).to(dev)}
    tg.forward(*args, **kw)
    g.finalize()
    return g, tg, args, kw


def _run_plugin(model, x, y, nf, dev, P=None, draw=None, distill=None):
    g, tg, args, kw = _make_graph(model, x, y, nf, dev, distill)
    if P is None:
        P = draw({k: tuple(v.data.shape) for k, v in g.vars.items()}) if draw else \
            {k: v.data.detach().cpu().numpy().copy() for k, v in g.vars.items()}
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    calls = dict(seq_ops.NATIVE_CALLS)
    res = tg.forward(*args, **kw)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    native = (seq_ops.NATIVE_CALLS["fwd"] - calls["fwd"], seq_ops.NATIVE_CALLS["bwd"] - calls["bwd"])
    grads = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if v.trainable}
    moving = {k: v.data.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if not v.trainable}
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    return dict(p=f64(res["predictions"]), sp=f64(res["support_predictions"]), loss=float(loss.detach()), grads=grads, moving=moving,
                P=P, native=native)


def _oracle(x64, nf, y, P, L_, M_, s, device="cpu", dtype=torch.float64, distill=None):
    tp = {k: torch.from_numpy(v.astype(np.float64)).to(device=device, dtype=dtype).requires_grad_(not k.split("/")[-1].startswith("moving_"))
          for k, v in P.items()}
    d = None if distill is None else torch.from_numpy(distill).to(device=device, dtype=dtype)
    pred, support, loss, moments = _restate(x64.to(device=device, dtype=dtype), torch.from_numpy(nf).to(device), torch.from_numpy(y).to(device),
                                            tp, L_, M_, s, distill=d)
    loss.backward()
    return pred.detach().cpu().numpy(), support.detach().cpu().numpy(), float(loss.detach()), tp, moments


# Tolerances of tests/test_gpu_bilstm.py::_check.  They are valid only where fp32 itself stays well inside them: the restatement run on
# the CPU in float32 against float64 at the small shape below with _draw's scales differs by (measured, u8 / float input)
#   predictions 2.7e-7 / 4.7e-7, support predictions 6.8e-7 / 7.2e-7, relative loss 2.5e-8 / 4.6e-8, gradients at most 4.6e-7 / 4.5e-7
#   of max(1, max|ref|) (expertsmoe3/weights); smallest batch variance of a column 3.2e-3 / 2.7e-3 at scale 1, above 3 at scales 2, 3
# -- two decades below a quarter of the tolerance everywhere (2.5e-5, 2.5e-5, 1.25e-4).
P_TOL, LOSS_TOL, GRAD_TOL = 1e-4, 1e-4, 5e-4


def _check(run, pr, spr, lr, tp, moments, L_, p_tol=P_TOL, loss_tol=LOSS_TOL, grad_tol=GRAD_TOL):
    ep, es = np.abs(run["p"] - pr).max(), np.abs(run["sp"] - spr).max()
    el = abs(run["loss"] - lr) / max(1.0, abs(lr))
    print("predictions %.3g support %.3g loss %.3g" % (ep, es, el))
    worst = ("", 0.0)
    for k, t in tp.items():
        if t.grad is not None:
            r = t.grad.cpu().numpy().astype(np.float64)
            e = np.abs(run["grads"][k] - r).max() / max(1.0, np.abs(r).max())
            worst = max(worst, (k, e), key=lambda kv: kv[1])
    print("worst gradient %s %.3g" % worst)
    assert ep < p_tol and es < p_tol
    assert el < loss_tol
    for k in range(1, L_ + 1):                                       # every scale's variables are there with a non-zero gradient
        names = ["cnn%dcnn-filter-len%d" % (k, fs) for fs in (1, 2, 3)] + ["cnn%dcluster_bn/gamma" % k, "cnn%dcluster_bn/beta" % k] + \
                ["RNN-rnn%d/basic_lstm_cell/weights" % k, "RNN-rnn%d/basic_lstm_cell/biases" % k] + \
                ["gatesmoe%d/weights" % k, "expertsmoe%d/weights" % k, "expertsmoe%d/biases" % k]
        for n in names:
            assert n in run["grads"] and np.abs(run["grads"][n]).max() > 0, n
    for k, t in tp.items():
        if t.grad is not None:
            r = t.grad.cpu().numpy().astype(np.float64)
            assert np.abs(run["grads"][k] - r).max() <= grad_tol * max(1.0, np.abs(r).max()), k
    for k, (mu, var) in enumerate(moments, 1):                       # one update of the moving averages the run started from
        mu, var = mu.cpu().numpy().astype(np.float64), var.cpu().numpy().astype(np.float64)
        mm, mv = run["moving"]["cnn%dcluster_bn/moving_mean" % k], run["moving"]["cnn%dcluster_bn/moving_variance" % k]
        mm0 = run["P"]["cnn%dcluster_bn/moving_mean" % k].astype(np.float64)
        mv0 = run["P"]["cnn%dcluster_bn/moving_variance" % k].astype(np.float64)
        want_mm, want_mv = BN_DECAY * mm0 + (1 - BN_DECAY) * mu, BN_DECAY * mv0 + (1 - BN_DECAY) * var
        # (fp32 rounding of the stored value + the statistics' own tolerance scaled by 1 - decay)
        assert np.abs(mm - want_mm).max() <= 4 * EPS32 * max(1.0, np.abs(want_mm).max()) + (1 - BN_DECAY) * p_tol * max(1.0, np.abs(mu).max()), k
        assert np.abs(mv - want_mv).max() <= 4 * EPS32 * max(1.0, want_mv.max()) + (1 - BN_DECAY) * p_tol * max(1.0, var.max()), k


def _small_case(u8, seed=5):
    from oracle import np_ref
    rs = np.random.RandomState(seed + u8)
    B, F, D, V = 32, 66, 64, 13
    nf = rs.randint(0, F + 1, size=B).astype(np.int32)
    nf[0], nf[1], nf[2], nf[3], nf[4] = F, 1, 0, 37, 48               # all frames, one, none, an odd and an even count
    y = rs.rand(B, V) < 0.2
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf))
    x = q if u8 else x64.numpy().astype(np.float32)
    if not u8:
        x64 = torch.from_numpy(x.astype(np.float64))
    return rs, x, x64, y, nf, V


def _small_flags(flags, L_=3):
    import yt8m_amd.frame_level_models, yt8m_amd.losses  # noqa: F401, E401  (define the flags set below)
    flags.lstm_cells, flags.multiscale_cnn_lstm_layers, flags.moe_num_mixtures = "256", L_, 2
    flags.is_training = True
    flags.support_type, flags.support_loss_percent = ",".join(["label"] * L_), 1.0


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_multiscale_plugin_matches_the_fp64_restatement(dev, flags, monkeypatch, u8, fused):
    """B = 32, F = 66, D = 64, H = 256, L = 3, V = 13, M = 2.  The frame chain is 66, 33, 16: scale 2 drops an odd frame, scale 3 (512
    rows) is below the native stack's smallest problem, so both forms of the stack are crossed."""
    import yt8m_amd.frame_level_models as flm
    monkeypatch.setattr(seq_ops, "MULTISCALE_FUSED", fused)
    _small_flags(flags)
    rs, x, x64, y, nf, V = _small_case(u8)
    run = _run_plugin(flm.MultiscaleCnnLstmModel(), x, y, nf, dev, draw=lambda shapes: _draw(shapes, rs))
    assert run["native"] == (2, 2), run["native"]
    pr, spr, lr, tp, moments = _oracle(x64, nf, y, run["P"], 3, 2, 1.0)
    assert run["sp"].shape == (32, 3 * V)
    _check(run, pr, spr, lr, tp, moments, 3)


def test_distillchain_plugin_matches_the_fp64_restatement(dev, flags):
    import yt8m_amd.frame_level_models as flm
    _small_flags(flags)
    rs, x, x64, y, nf, V = _small_case(True, seed=9)
    distill = rs.rand(32, V).astype(np.float32)
    run = _run_plugin(flm.DistillchainMultiscaleCnnLstmModel(), x, y, nf, dev, draw=lambda shapes: _draw(shapes, rs), distill=distill)
    assert "distillrelu/weights" in run["grads"] and np.abs(run["grads"]["distillrelu/weights"]).max() > 0
    pr, spr, lr, tp, moments = _oracle(x64, nf, y, run["P"], 3, 2, 1.0, distill=distill.astype(np.float64))
    _check(run, pr, spr, lr, tp, moments, 3)


def _model_case(seed):
    rs = np.random.RandomState(seed)
    B, F, D, V = 128, 300, 1152, 4716
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1], nf[2] = F, 1, 0
    y = rs.rand(B, V) < 3.4 / V
    y[:, 0] = True                                                     # every video has a label
    return rs, q, nf, y


def _model_flags(flags):
    import yt8m_amd.frame_level_models, yt8m_amd.losses  # noqa: F401, E401  (define the flags set below)
    flags.lstm_cells, flags.multiscale_cnn_lstm_layers, flags.moe_num_mixtures = "1024", 4, 4
    flags.is_training = True
    flags.support_type, flags.support_loss_percent = "label,label,label,label", 0.5


def _init_with_bn(g, rs, dev):
    """The variables' own initial values (filters 0.1, xavier elsewhere), gamma / beta moved off 1 / 0 so that their gradients differ."""
    P = {k: v.data.detach().cpu().numpy().copy() for k, v in g.vars.items()}
    for k in P:
        if k.endswith("/gamma"):
            P[k] = (1.0 + 0.1 * rs.randn(*P[k].shape)).astype(np.float32)
        elif k.endswith("/beta"):
            P[k] = (0.2 * rs.randn(*P[k].shape)).astype(np.float32)
    return P


def _run_model_shape(q, y, nf, dev, P, rs):
    import yt8m_amd.frame_level_models as flm
    if P is None:
        g, _, _, _ = _make_graph(flm.MultiscaleCnnLstmModel(), q, y, nf, dev)
        P = _init_with_bn(g, rs, dev)
    return _run_plugin(flm.MultiscaleCnnLstmModel(), q, y, nf, dev, P=P)


# Gradients of the fused path against the generic one.  The starting point, 1e-4 of max(1, max|g|), is the bound of two schedules of the
# SAME kernels (test_overlapped_directions_equal_the_sequential_form_at_the_bench_shape).  Here the two paths are different fp32-grade
# evaluations: the CNN's products are cut differently (one K = fs D product on a concatenated input against fs products on row windows,
# each on the three-f16-product forms with 2^-21 per term under its own operand scales), and the batch norm's column sums over 38 400 /
# 19 200 rows are added in different orders (the generic kernel: 9 600 terms one after the other per lane) before they are subtracted
# from every row's gradient.  Measured on the MI355X: predictions 8.3e-7, loss 1.6e-7, worst gradient 7.3e-4 (cnn2cnn-filter-len1; the
# batch-norm gammas 1.5e-4, every LSTM / MoE variable below 3e-5); the fused path alone is 7.8e-5 from the float64 restatement at this
# shape.  Widened to 1e-3: ten times the starting constant, 1.4 times the measured value.
FUSED_VS_GENERIC_GRAD_TOL = 1e-3


def test_fused_equals_generic_at_the_model_shape(dev, flags, monkeypatch):
    """B = 128, F = 300, D = 1152 uint8, H = 1024, L = 4, V = 4716, M = 4: predictions, loss and every gradient of the fused time-major
    path against the generic composition (1e-5 on predictions and loss, FUSED_VS_GENERIC_GRAD_TOL on gradients).  All
    four stacks run natively (37 * 128 rows at scale 4)."""
    _model_flags(flags)
    rs, q, nf, y = _model_case(1)
    monkeypatch.setattr(seq_ops, "MULTISCALE_FUSED", True)
    a = _run_model_shape(q, y, nf, dev, None, rs)
    monkeypatch.setattr(seq_ops, "MULTISCALE_FUSED", False)
    b = _run_model_shape(q, y, nf, dev, a["P"], rs)
    assert a["native"] == b["native"] == (4, 4)
    ep, el = np.abs(a["p"] - b["p"]).max(), abs(a["loss"] - b["loss"]) / max(1.0, abs(a["loss"]))
    worst = max(((k, np.abs(a["grads"][k] - b["grads"][k]).max() / max(1.0, np.abs(a["grads"][k]).max())) for k in a["grads"]),
                key=lambda kv: kv[1])
    print("fused vs generic: predictions %.3g loss %.3g worst gradient %s %.3g" % ((ep, el) + worst))
    assert ep < 1e-5 and np.abs(a["sp"] - b["sp"]).max() < 1e-5 and el < 1e-5
    for k in a["grads"]:
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= FUSED_VS_GENERIC_GRAD_TOL * max(1.0, np.abs(a["grads"][k]).max()), k
    for k in a["moving"]:
        # each path's batch statistic is within P_TOL * max(1, max|statistic|) of float64 (what _check asks of either); it enters the
        # moving average times 1 - decay, and the stored fp32 value rounds once more.  (Measured: 2.0e-6 on a moving variance of 1.13,
        # i.e. 2e-3 on a batch variance of ~125: the generic kernel adds 4 800 squares one after the other per lane.)
        stat = (a["moving"][k] - BN_DECAY * a["P"][k].astype(np.float64)) / (1 - BN_DECAY)
        bound = 4 * EPS32 * max(1.0, np.abs(a["moving"][k]).max()) + 2 * (1 - BN_DECAY) * P_TOL * max(1.0, np.abs(stat).max())
        assert np.abs(a["moving"][k] - b["moving"][k]).max() <= bound, k


def test_multiscale_plugin_matches_the_fp64_restatement_at_the_model_shape(dev, flags):
    """The same shape against the fp64 restatement run on the device in float64, weights at the initialisers' scale."""
    from oracle import np_ref
    _model_flags(flags)
    rs, q, nf, y = _model_case(7)
    run = _run_model_shape(q, y, nf, dev, None, rs)
    assert run["native"] == (4, 4), run["native"]
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf))
    pr, spr, lr, tp, moments = _oracle(x64, nf, y, run["P"], 4, 4, 0.5, device=dev)
    _check(run, pr, spr, lr, tp, moments, 4)


def test_training_step_fused_like_generic_and_inference_uses_the_moving_averages(dev, flags, monkeypatch):
    """One whole TrainGraph.step (forward, backward, clip + Adam, the stacks' early optimiser pass included) at the model's shape, fused
    and generic from the same parameters: the parameters after the step agree (as
    test_overlapped_training_step_updates_the_parameters_like_the_sequential_one compares them).  Then forward(is_training=False) on the
    fused graph equals the restatement's inference form on the moving averages the step left behind."""
    import yt8m_amd.frame_level_models as flm
    from oracle import np_ref
    _model_flags(flags)
    rs, q, nf, y = _model_case(9)
    after, grads, P, keep = {}, {}, None, None
    for fused in (False, True):
        monkeypatch.setattr(seq_ops, "MULTISCALE_FUSED", fused)
        g, tg, args, _ = _make_graph(flm.MultiscaleCnnLstmModel(), q, y, nf, dev)
        if P is None:
            P = {k: torch.from_numpy(v).to(dev) for k, v in _init_with_bn(g, rs, dev).items()}
        for k, v in g.vars.items():
            v.data.copy_(P[k])
        torch.cuda.synchronize()
        tg.step(*args)                                                 # no synchronisation until the parameters are read
        after[fused] = {k: v.data.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items()}
        grads[fused] = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if v.trainable}
        seq_ops.check_persist_errors()
        keep = (g, tg, args)
    for k in grads[False]:
        gs, go = grads[False][k], grads[True][k]
        tol = FUSED_VS_GENERIC_GRAD_TOL * max(1.0, np.abs(gs).max())
        assert np.abs(gs - go).max() <= tol, k
        dp = np.abs(after[False][k] - after[True][k])
        p0 = P[k].detach().cpu().numpy().astype(np.float64)
        step = np.abs(after[False][k] - p0)
        # Adam's first step is ~lr_t * sign(g) where the (clipped) gradient is far above its epsilon.  The two paths are different
        # fp32-grade evaluations whose gradients agree to `tol` (asserted above; measured at most 4.1e-4), so only elements above four
        # times that bound are certain to have one sign in both -- there the two updates must agree to rounding; a pass that read a
        # stale or half-written gradient buffer would move these elements differently.  (The bidirectional test's rule, 1e-3 of the
        # largest gradient, assumes identical arithmetic: here it sits below the agreement of the two paths for the CNN filters.)
        firm = np.abs(gs) > 4 * tol
        assert firm.any(), k
        assert dp[firm].max() <= 1e-6 + 1e-3 * step[firm].max(), (k, dp[firm].max())
    g, tg, args = keep
    moved = after[True]["cnn1cluster_bn/moving_mean"]
    assert np.abs(moved - P["cnn1cluster_bn/moving_mean"].cpu().numpy()).max() > 0      # the step updated the moving averages
    with torch.no_grad():
        res = tg.forward(*args, is_training=False)
    now = {k: v.data.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items()}
    assert all(np.array_equal(now[k], after[True][k]) for k in now if "moving_" in k)  # ... and inference leaves them alone
    tp = {k: torch.from_numpy(v).to(dev) for k, v in now.items()}
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf)).to(dev)
    with torch.no_grad():
        pr, spr, _, _ = _restate(x64, args[2], args[1], tp, 4, 4, 0.5, training=False)
    ep = float((res["predictions"].double() - pr).abs().max())
    es = float((res["support_predictions"].double() - spr).abs().max())
    print("inference: predictions %.3g support %.3g" % (ep, es))
    assert ep < P_TOL and es < P_TOL
