"""LstmCnnDeepCombineChainModel / DistillchainLstmCnnDeepCombineChainModel (W/all_frame_models/lstm_cnn_deep_combine_chain_model.py,
distillchain_lstm_cnn_deep_combine_chain_model.py) on the MI355X: the pooled CNN's gather kernels (csrc/cnn_pool_f32.hip) through the C ABI
against float64 index_add, seq_ops.cnn_tm_maxpool against float64 and against the composed form (seq_ops.cnn_tm + a max over the frames),
both plugins through the plugin surface against an fp64 restatement built here (oracle.torch_ref.lstm_stack / moe / cross_entropy around
explicit shifted concatenations), pooled against composed at the training script's shape, and whole training steps."""
import ctypes
import time

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.variables import reset_default_graph, zeros

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SCRIPT_CHAIN = [[(1, 128), (2, 256), (3, 128)]] + [[(1, 128), (2, 128), (3, 256)]] * 3      # run-chaining-lstm-cnn.sh: c = 128, 3 layers


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _maxerr(a, ref64):
    return float((a.double() - ref64).abs().max())


# ---- the kernels with idx given ---------------------------------------------------------------------------------------------------
def _dx_ref(idx, g, Ws, shapes, F, B, D, dtype):
    """dx [F B, D] by index_add on the CPU in `dtype`: one source row g[b, n] W_k[i D : (i + 1) D, n] per (video, column, shift)."""
    dx = torch.zeros(F * B, D, dtype=dtype)
    bb = torch.arange(B)[:, None]
    c0 = 0
    for (fs, N), W in zip(shapes, Ws):
        W = W.to(dtype)
        for i in range(fs):
            t = idx[:, c0:c0 + N].long() - i
            ok = t >= 0
            src = g[:, c0:c0 + N, None].to(dtype) * W[i * D:(i + 1) * D].t()[None]                 # [B, N, D]
            dx.index_add_(0, (t * B + bb)[ok], src[ok])
        c0 += N
    return dx


def _dw_ref(x, idx, g, c0, fs, N, F, B, D, dtype, old=None):
    """dW [fs D, N] of one filter by index_add on the CPU in `dtype` (the terms of a column in ascending b), on top of `old`."""
    bb = torch.arange(B)[:, None]
    nn = torch.arange(N)[None, :].expand(B, N)
    out = []
    for i in range(fs):
        t = idx[:, c0:c0 + N].long() - i
        ok = t >= 0
        acc = torch.zeros(N, D, dtype=dtype)
        acc.index_add_(0, nn[ok], g[:, c0:c0 + N].to(dtype)[ok][:, None] * x.to(dtype)[(t * B + bb)[ok]])
        out.append(acc.t())
    dW = torch.cat(out, 0)
    return dW if old is None else old.to(dtype) + dW


@pytest.mark.parametrize("F,B,D,chain", [(7, 3, 12, [[(1, 5), (2, 3), (3, 6)], [(1, 1), (3, 7)]]),      # odd everything, D in one partial slice
                                         (33, 5, 132, [[(1, 8), (2, 12), (4, 4)]] * 2),              # a 4-float tail slice, a filter of length 4
                                         (300, 128, 1152, SCRIPT_CHAIN)])                            # the model's shape, the script's filters
def test_gather_kernels_against_float64_index_add(dev, F, B, D, chain):
    """yt8m_f32_cnn_pool_dw / _dx with idx GIVEN: the result does not depend on which frame won a maximum.  idx holds 0, 1 and F - 1 (so
    idx - i < 0 and the last row both occur) and video 0 points every column at ONE frame.  Leading dimensions wider than the rows; the
    margins keep their sentinel.  Bound: FOUR times the error of torch's own fp32 evaluation of the same sums (index_add on the CPU,
    fp32) against fp64, largest over the tensor, measured here on the same data -- the reference for the bound is torch fp32 vs fp64,
    never the kernel (the rule of test_colmoments_and_forward_kernel_against_float64)."""
    lib = L.lib()
    gen = torch.Generator(device="cpu").manual_seed(3 + F)
    shapes = [s for cnn in chain for s in cnn]
    Ntot = sum(n for _, n in shapes)
    ldx, ldg = D + 4, Ntot + 5
    x = torch.randn(F * B, D, generator=gen)
    g = torch.randn(B, Ntot, generator=gen)
    idx = torch.randint(0, F, (B, Ntot), generator=gen, dtype=torch.int32)
    idx[:, 0], idx[:, 1 % Ntot], idx[:, 2 % Ntot] = 0, 1, F - 1
    idx[B - 1, :] = torch.tensor([0, 1, F - 1], dtype=torch.int32).repeat(Ntot)[:Ntot]
    idx[0, :] = 1                                                      # one frame takes every column of video 0
    Ws = [torch.randn(fs * D, n, generator=gen) * 0.1 for fs, n in shapes]
    xw = torch.full((F * B, ldx), -7.0)
    xw[:, :D] = x
    gw = torch.full((B, ldg), -7.0)
    gw[:, :Ntot] = g
    iw = torch.full((B, ldg), -1, dtype=torch.int32)
    iw[:, :Ntot] = idx
    xd, gd, idd = xw.to(dev), gw.to(dev), iw.to(dev)

    # dx: every CNN of the chain in one call
    n = len(shapes)
    wts = [W.t().contiguous().to(dev) for W in Ws]
    wt = (ctypes.c_void_p * n)(*[t.data_ptr() for t in wts])
    fsa = (ctypes.c_int32 * n)(*[fs for fs, _ in shapes])
    nca = (ctypes.c_int32 * n)(*[nc for _, nc in shapes])
    lddx = D + 2
    runs = []
    for _ in range(2):
        dxd = torch.full((F * B, lddx), float("nan"), device=dev)
        dxd[:, D:] = -7.0
        L.check(lib.yt8m_f32_cnn_pool_dx(_p(idd), _p(gd), ldg, B, F, D, n, wt, fsa, nca, _p(dxd), lddx, _st()))
        torch.cuda.synchronize()
        runs.append(dxd.cpu())
    assert torch.equal(runs[0][:, :D], runs[1][:, :D])                # bit for bit: no float atomics, an order fixed by the inputs
    assert bool((runs[0][:, D:] == -7.0).all())
    dx64 = _dx_ref(idx, g, Ws, shapes, F, B, D, torch.float64)
    b_dx = 4 * _maxerr(_dx_ref(idx, g, Ws, shapes, F, B, D, torch.float32), dx64)
    e_dx = _maxerr(runs[0][:, :D], dx64)
    print("dx (%d,%d,%d): err %.3g (bound %.3g), largest |dx| %.3g" % (F, B, D, e_dx, b_dx, float(dx64.abs().max())))
    assert e_dx <= b_dx
    assert float(dx64[1 * B + 0].abs().max()) > 0 and bool((dx64.abs().sum(1) == 0).any())      # a crowded row and untouched rows exist

    # dw: one call per filter, beta 0 and 1
    c0 = 0
    for k, ((fs, N), W) in enumerate(zip(shapes, Ws)):
        lddw = N + 3
        for beta in ((0.0, 1.0) if F * B * D < 1 << 20 else (float(k % 2),)):      # (the model's shape: beta alternates over its 12 filters)
            old = torch.randn(fs * D, N, generator=gen)
            dwd = torch.full((fs * D, lddw), -7.0, device=dev)
            dwd[:, :N] = old.to(dev)
            L.check(lib.yt8m_f32_cnn_pool_dw(_p(xd), ldx, _p(idd, c0), _p(gd, c0), ldg, B, F, D, N, fs, _p(dwd), lddw, beta, _st()))
            got = dwd.cpu()
            assert bool((got[:, N:] == -7.0).all())
            o = old if beta else None
            dw64 = _dw_ref(x, idx, g, c0, fs, N, F, B, D, torch.float64, o)
            b_dw = 4 * _maxerr(_dw_ref(x, idx, g, c0, fs, N, F, B, D, torch.float32, o), dw64)
            e_dw = _maxerr(got[:, :N], dw64)
            if k < 3 or e_dw > b_dw:
                print("dw filter %d beta %g: err %.3g (bound %.3g)" % (k, beta, e_dw, b_dw))
            assert e_dw <= b_dw, (k, beta)
        c0 += N
    assert bool((xd[:, D:] == -7.0).all()) and bool((gd[:, Ntot:] == -7.0).all())


# ---- cnn_tm_maxpool ---------------------------------------------------------------------------------------------------------------
def _shifted_cnn(x, Ws, D):
    """cnn_output [B,F,sum N] in the dtype of x [B,F,D]: per filter the input concatenated with its 1 .. fs - 1 frame shifts (zero padding
    in front) times W [fs D, N]."""
    B, F, _ = x.shape
    outs = []
    for W in Ws:
        fs = W.shape[0] // D
        sh = [x] + [torch.cat([x.new_zeros(B, min(i, F), D), x[:, :max(F - i, 0)]], 1) for i in range(1, fs)]
        outs.append(torch.cat(sh, 2) @ W)
    return torch.cat(outs, 2)


def _ragged_rows(rs, F, B, D):
    nf = rs.randint(1, F + 1, size=B)
    nf[0], nf[1], nf[2] = F, 1, 0                                      # video 2 is all zeros
    x = rs.randn(B, F, D).astype(np.float32)
    x[np.arange(F)[None, :] >= nf[:, None]] = 0.0
    return x, nf


def _run_maxpool(dev, x_bfd, chain_w, coef, composed):
    """The op (or the composed form) on x [B,F,D] handed over time-major: pooled [B, Ntot], idx, dx [B,F,D], [dW]."""
    B, F, D = x_bfd.shape
    g = reset_default_graph(device=dev, seed=0)
    cnns = [[g.get_variable("c%df%d" % (c, k), W.shape, zeros) for k, W in enumerate(cnn)] for c, cnn in enumerate(chain_w)]
    g.finalize()
    for cv, cw in zip(cnns, chain_w):
        for v, W in zip(cv, cw):
            v.data.copy_(torch.from_numpy(W).to(dev))
    g.begin_step()
    x = torch.from_numpy(x_bfd).to(dev).transpose(0, 1).reshape(F * B, D).contiguous().requires_grad_(True)
    idx = None
    if composed:
        pooled = [seq_ops.cnn_tm(x, B, cnn).view(F, B, -1).amax(0) for cnn in cnns]
    else:
        pooled, idx = seq_ops.cnn_tm_maxpool(x, B, cnns, want_idx=True)
    p = torch.cat(pooled, 1)
    (p * torch.from_numpy(coef).to(dev)).sum().backward()
    torch.cuda.synchronize()
    dx = x.grad.view(F, B, D).transpose(0, 1).cpu()
    return p.detach().cpu(), (None if idx is None else idx.cpu().long()), dx, [v.grad.detach().cpu().clone() for cv in cnns for v in cv]


def _grads_at_idx(x_bfd, flat_w, D, idx, coef, dtype):
    """The gradients of sum coef[b, n] cnn_output[b, idx[b, n], n] on the CPU in `dtype`: what the pooled op's backward must give for
    the frames it chose."""
    x = torch.from_numpy(x_bfd).to(dtype).requires_grad_(True)
    tw = [torch.from_numpy(W).to(dtype).requires_grad_(True) for W in flat_w]
    y = _shifted_cnn(x, tw, D)
    (y.gather(1, idx[:, None, :]).squeeze(1) * torch.from_numpy(coef).to(dtype)).sum().backward()
    return y.detach(), x.grad, [t.grad for t in tw]


@pytest.mark.parametrize("F,chain", [(9, [[(1, 8), (2, 8), (3, 12)], [(1, 4), (2, 16), (3, 4)]]), (2, [[(1, 32), (2, 32), (4, 64)]]),
                                     (1, [[(1, 8), (3, 8)], [(2, 4)]])])                    # F below the filter lengths too
@pytest.mark.parametrize("whole_chain", [False, True])                 # one set of products per CNN (the default) / for the chain
def test_cnn_tm_maxpool_against_float64_and_the_composed_form(dev, monkeypatch, F, chain, whole_chain):
    """seq_ops.cnn_tm_maxpool on x that requires grad, ragged zero rows at the end of the videos, one video all zeros (B = 32, D = 48: the
    shape of test_pooled_u8_cnn_equals_the_pooled_output_of_the_unpooled_op and its bound on the pooled values, 2e-6 max(1, max|p|)).
    Argmax: for EVERY (b, n) the fp64 output at the op's idx is within that bound of the fp64 maximum.  Gradients: against the fp64
    gradient evaluated AT THE OP'S OWN idx -- a near-tie that fp32 resolves differently is a valid answer, no (b, n) is left out -- within
    four times the error of torch's fp32 evaluation of the same expression against fp64 (the kernels' rule above).  Then against the
    composed form: its amax splits the gradient of a tied maximum evenly, the op routes it to the first frame; maxima tie only at 0 (a
    whole window of zero rows), whose terms land on padding rows of dx and on nothing in dW -- so dx is compared on the live rows, within
    the 2e-4 max(1, max|g|) that test_cnn_chain_plugin_takes_the_raw_uint8_frames allows two forms of one fp32 CNN."""
    monkeypatch.setattr(seq_ops, "CNN_POOL_WHOLE_CHAIN", whole_chain)
    rs = np.random.RandomState(41 + F)
    B, D = 32, 48
    x, nf = _ragged_rows(rs, F, B, D)
    chain_w = [[(rs.randn(fs * D, n) * 0.1).astype(np.float32) for fs, n in cnn] for cnn in chain]
    flat_w = [W for cnn in chain_w for W in cnn]
    Ntot = sum(W.shape[1] for W in flat_w)
    coef = rs.randn(B, Ntot).astype(np.float32)
    p, idx, dx, dws = _run_maxpool(dev, x, chain_w, coef, composed=False)
    assert int(idx.min()) >= 0 and int(idx.max()) < F
    y64, dx64, dw64 = _grads_at_idx(x, flat_w, D, idx, coef, torch.float64)
    _, dx32, dw32 = _grads_at_idx(x, flat_w, D, idx, coef, torch.float32)
    p64 = y64.max(1).values
    tol = 2e-6 * max(1.0, float(p64.abs().max()))
    at_idx = y64.gather(1, idx[:, None, :]).squeeze(1)
    print("F=%d pooled err %.3g argmax gap %.3g (bound %.3g)" % (F, _maxerr(p, p64), float((p64 - at_idx).max()), tol))
    assert _maxerr(p, p64) < tol
    assert float((p64 - at_idx).max()) <= tol                        # every (b, n): the chosen frame attains the maximum
    assert bool((p[2] == 0).all()) and bool((idx[2] == 0).all())      # the all-zero video: 0 at the first frame
    b_dx = 4 * _maxerr(dx32, dx64)
    print("dx err %.3g (bound %.3g)" % (_maxerr(dx, dx64), b_dx))
    assert _maxerr(dx, dx64) <= b_dx
    for k, (a, r32, r64) in enumerate(zip(dws, dw32, dw64)):
        assert _maxerr(a, r64) <= 4 * _maxerr(r32, r64), k
    pc, _, dxc, dwc = _run_maxpool(dev, x, chain_w, coef, composed=True)
    assert _maxerr(pc, p.double()) < tol
    live = torch.from_numpy(np.arange(F)[None, :] < nf[:, None])
    assert float((dx - dxc)[live].abs().max() if live.any() else 0.0) <= 2e-4 * max(1.0, float(dx.abs().max()))
    for k, (a, b_) in enumerate(zip(dws, dwc)):
        assert float((a - b_).abs().max()) <= 2e-4 * max(1.0, float(b_.abs().max())), k


# ---- the plugins ------------------------------------------------------------------------------------------------------------------
def _restate(x, nf, labels, P, L_, M_, s, feature_sizes, lstm_layers, distill=None):
    """Both models in the dtype and on the device of x [B,F,D] (batch-major, as the reference): predictions, support predictions and the
    multitask loss (1 - s) CE(p, y) + s CE(support, [y] * L)."""
    from oracle import torch_ref
    B, F, D = x.shape
    relu_layers = []
    if distill is not None:
        relu_layers.append(torch_ref.l2_normalize(torch.relu(distill @ P["distillrelu/weights"] + P["distillrelu/biases"])))
    mask = (torch.arange(F, device=x.device)[None, :] < nf[:, None]).to(x.dtype)
    mean_input = torch.einsum("ijk,ij->ik", x, mask) / nf.to(x.dtype)[:, None]
    outs, off = [], 0
    for i, fs in enumerate(feature_sizes):
        sub = torch_ref.l2_normalize(x[:, :, off:off + fs], 2)
        off += fs
        layers = [(P["RNN%d/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (i, l)], P["RNN%d/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (i, l)])
                  for l in range(lstm_layers)]
        outs.append(torch_ref.lstm_stack(sub, nf, layers)[0])          # [B,F,H_i], zeros at frames >= num_frames
    lstm_output = torch.cat(outs, 2)
    Dc = lstm_output.shape[2]
    relu_layers.append(torch_ref.l2_normalize(torch.relu(mean_input @ P["mean-relu/weights"] + P["mean-relu/biases"])))

    def cnn(k):
        y = _shifted_cnn(lstm_output, [P["cnn%dcnn-filter-len%d" % (k, fs)] for fs in (1, 2, 3)], Dc)
        return torch_ref.l2_normalize(y.max(1).values)                 # over ALL max_frames rows, padding included

    nxt = cnn(0) if distill is None else torch.cat([cnn(0)] + relu_layers, 1)
    sup = []
    for l in range(L_):
        sc = "prediction-%d" % l
        sp = torch_ref.moe(nxt, P["gates-%s/weights" % sc], P["experts-%s/weights" % sc], P["experts-%s/biases" % sc], M_)
        sup.append(sp)
        relu_layers.append(torch_ref.l2_normalize(torch.relu(sp @ P["relu-%d/weights" % l] + P["relu-%d/biases" % l])))
        nxt = torch.cat([cnn(l + 1)] + relu_layers, 1)
    pred = torch_ref.moe(nxt, P["gates--main/weights"], P["experts--main/weights"], P["experts--main/biases"], M_)
    support = torch.cat(sup, 1)
    yl = labels.to(x.dtype)
    loss = (1.0 - s) * torch_ref.cross_entropy(pred, yl) + s * torch_ref.cross_entropy(support, torch.cat([yl] * L_, 1))
    return pred, support, loss


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
    res = tg.forward(*args, **kw)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    grads = {k: f64(v.grad) for k, v in g.vars.items() if v.trainable}
    return dict(p=f64(res["predictions"]), sp=f64(res["support_predictions"]), loss=float(loss.detach()), grads=grads, P=P)


def _oracle(x64, nf, y, P, L_, M_, s, feature_sizes, lstm_layers, distill=None, device="cpu"):
    tp = {k: torch.from_numpy(v.astype(np.float64)).to(device).requires_grad_(True) for k, v in P.items()}
    d = None if distill is None else torch.from_numpy(distill.astype(np.float64)).to(device)
    pred, support, loss = _restate(x64.to(device), torch.from_numpy(nf).to(device), torch.from_numpy(y).to(device), tp, L_, M_, s,
                                   feature_sizes, lstm_layers, distill=d)
    loss.backward()
    return pred.detach().cpu().numpy(), support.detach().cpu().numpy(), float(loss.detach()), tp


def _draw(shapes, rs):
    """A contractive recurrence (0.06, as the bidirectional and multiscale tests), filters at the initialiser's 0.1, heads and FCs 0.2."""
    scale = lambda k: 0.06 if "basic_lstm_cell" in k else (0.1 if "cnn-filter" in k else 0.2)
    return {k: (rs.randn(*shp) * scale(k)).astype(np.float32) for k, shp in shapes.items()}


# Tolerances of test_cnn_chain_plugin_takes_the_raw_uint8_frames (the sibling plugin at its small shape) against the fp64 restatement.
P_TOL, LOSS_TOL, GRAD_TOL = 1e-4, 1e-4, 5e-4
SMALL = dict(B=16, F=9, V=13, L_=2, M_=2, cells=8, feature_sizes=[64, 32], lstm_sizes=[128, 64], lstm_layers=2, s=0.5)


def _small_flags(flags, c=SMALL):
    import yt8m_amd.frame_level_models, yt8m_amd.losses  # noqa: F401, E401  (define the flags set below)
    flags.feature_sizes, flags.lstm_cells = ",".join(map(str, c["feature_sizes"])), ",".join(map(str, c["lstm_sizes"]))
    flags.lstm_layers, flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.moe_num_mixtures = c["lstm_layers"], c["L_"], c["cells"], c["M_"]
    flags.support_type, flags.support_loss_percent = ",".join(["label"] * c["L_"]), c["s"]


def _small_case(seed, dev, c=SMALL, short=False):
    import yt8m_amd.frame_level_models as flm
    from oracle import np_ref
    rs = np.random.RandomState(seed)
    B, F, D = c["B"], c["F"], sum(c["feature_sizes"])
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, (4 if short else F) + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1                                                # ragged num_frames >= 1, including 1 and F
    y = rs.rand(B, c["V"]) < 0.2
    qt = torch.from_numpy(q).to(dev)
    assert seq_ops.u8_attention_supported(qt, 1) and all(flm._lib_u8_ok(fs) for fs in c["feature_sizes"]), \
        "the shape of this test must take the uint8 path"
    return rs, q, torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf)), y, nf


def _want_names(L_, lstm_layers, distill):
    names = {"mean-relu/weights", "mean-relu/biases"}
    for i in range(2):
        for l in range(lstm_layers):
            names |= {"RNN%d/multi_rnn_cell/cell_%d/basic_lstm_cell/%s" % (i, l, w) for w in ("weights", "biases")}
    for k in range(L_ + 1):
        names |= {"cnn%dcnn-filter-len%d" % (k, fs) for fs in (1, 2, 3)}
    for sc in ["prediction-%d" % l for l in range(L_)] + ["-main"]:
        names |= {"gates-%s/weights" % sc, "experts-%s/weights" % sc, "experts-%s/biases" % sc}
    for l in range(L_):
        names |= {"relu-%d/weights" % l, "relu-%d/biases" % l}
    if distill:
        names |= {"distillrelu/weights", "distillrelu/biases"}
    return names


def _check(run, pr, spr, lr, tp):
    ep, es = np.abs(run["p"] - pr).max(), np.abs(run["sp"] - spr).max()
    el = abs(run["loss"] - lr) / max(1.0, abs(lr))
    worst = max(((k, np.abs(run["grads"][k] - t.grad.cpu().numpy()).max() / max(1.0, float(t.grad.abs().max()))) for k, t in tp.items()),
                key=lambda kv: kv[1])
    print("predictions %.3g support %.3g loss %.3g worst gradient %s %.3g" % ((ep, es, el) + worst))
    assert ep < P_TOL and es < P_TOL
    assert el < LOSS_TOL
    for k, t in tp.items():
        r = t.grad.cpu().numpy()
        assert np.abs(run["grads"][k]).max() > 0, k
        assert np.abs(run["grads"][k] - r).max() <= GRAD_TOL * max(1.0, np.abs(r).max()), k


@pytest.mark.parametrize("distill", [False, True])
def test_plugins_match_the_fp64_restatement(dev, flags, distill):
    """B = 16, F = 9, uint8 [B,9,96] split 64 | 32, two-layer stacks of 128 and 64 cells, c = 8, L = 2, V = 13, M = 2, multitask loss.
    The restatement takes plain fp64 maxima: a seed on which fp32 and fp64 disagree about an argmax (a near-tie) is to be CHANGED, the
    bounds stay (none of the seeds below needed that)."""
    import yt8m_amd.frame_level_models as flm
    _small_flags(flags)
    c = SMALL
    rs, q, x64, y, nf = _small_case(5 + distill, dev)
    d = rs.rand(c["B"], c["V"]).astype(np.float32) if distill else None
    cls = flm.DistillchainLstmCnnDeepCombineChainModel if distill else flm.LstmCnnDeepCombineChainModel
    if distill:
        with pytest.raises(AssertionError):
            _make_graph(cls(), q, y, nf, dev)
    run = _run_plugin(cls(), q, y, nf, dev, draw=lambda shapes: _draw(shapes, rs), distill=d)
    assert set(run["P"]) == set(run["grads"]) == _want_names(c["L_"], c["lstm_layers"], distill)
    assert run["sp"].shape == (c["B"], c["L_"] * c["V"])
    pr, spr, lr, tp = _oracle(x64, nf, y, run["P"], c["L_"], c["M_"], c["s"], c["feature_sizes"], c["lstm_layers"], distill=d)
    _check(run, pr, spr, lr, tp)


def test_maxima_on_padding_rows_do_not_reach_the_lstm_parameters(dev, flags, monkeypatch):
    """The pooled maximum may sit at a frame >= num_frames: with the candidate gate's bias at +2 every LSTM output is positive, with
    negative filters every CNN output of a live window is negative, and the 0 of the first all-padding window wins on a short video.  The
    dx rows there are padding rows of the stacks' outputs -- constants of dynamic_rnn: they must not reach the LSTM parameters."""
    import yt8m_amd.frame_level_models as flm
    _small_flags(flags)
    c = SMALL
    rs, q, x64, y, nf = _small_case(17, dev, short=True)
    seen = []
    monkeypatch.setattr(flm, "_pooled_cnn_chain", lambda out_tm, cnns: seen.append(
        seq_ops.cnn_tm_maxpool(out_tm.reshape(-1, out_tm.shape[2]), out_tm.shape[1], cnns, want_idx=True)) or seen[-1][0])

    def draw(shapes):
        P = _draw(shapes, rs)
        for k in P:
            if "cnn-filter" in k:
                P[k] = -np.abs(P[k])
            elif k.endswith("basic_lstm_cell/biases"):
                H = P[k].shape[0] // 4
                P[k][H:2 * H] = 2.0                                    # gate order i, j, f, o: a positive candidate, so c > 0 and h > 0
        return P

    run = _run_plugin(flm.LstmCnnDeepCombineChainModel(), q, y, nf, dev, draw=draw)
    idx = seen[-1][1].cpu().numpy()
    beyond = idx >= nf[:, None]
    print("maxima at padding frames: %d of %d" % (beyond.sum(), beyond.size))
    assert beyond[2:].mean() > 0.9 and not beyond[0].any()             # the short videos' maxima; the full-length video has no padding
    pr, spr, lr, tp = _oracle(x64, nf, y, run["P"], c["L_"], c["M_"], c["s"], c["feature_sizes"], c["lstm_layers"])
    _check(run, pr, spr, lr, tp)


# ---- the script's shape -----------------------------------------------------------------------------------------------------------
def _script_flags(flags):
    import yt8m_amd.frame_level_models, yt8m_amd.losses  # noqa: F401, E401
    flags.feature_sizes, flags.lstm_cells, flags.lstm_layers = "1024,128", "1024,128", 1
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.moe_num_mixtures = 3, 128, 4
    flags.support_type, flags.support_loss_percent = "label,label,label", 0.05


def _script_case(seed, B):
    rs = np.random.RandomState(seed)
    F, D, V = 300, 1152, 4716
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1
    y = rs.rand(B, V) < 3.4 / V
    y[:, 0] = True
    return q, nf, y


def _composed_chain(out_tm, cnns):
    F, B, D = out_tm.shape
    x = out_tm.reshape(F * B, D)
    return [seq_ops.cnn_tm(x, B, cnn).view(F, B, -1).amax(0) for cnn in cnns]


def test_pooled_equals_composed_at_the_scripts_shape(dev, flags, monkeypatch):
    """B = 128, F = 300, uint8 [B,300,1152], cells 1024 | 128, one layer, c = 128, L = 3, M = 4, V = 4716: one forward + backward of the
    pooled form and of the composed form (seq_ops.cnn_tm + amax, put into frame_level_models._pooled_cnn_chain) from the same weights.
    Predictions within 2e-5 (the sibling's byte-against-float comparison).  Gradients: both are fp32-grade evaluations with differently
    cut sums; the bound is FOUR times the composed form's own worst gradient error (in units of max(1, max|g|) per variable) against the
    fp64 restatement, measured here at B = 8 -- the largest batch whose fp64 restatement on the host stays under a minute.
    Measured on the MI355X: see DESIGN_LOG.md 17."""
    import yt8m_amd.frame_level_models as flm
    from oracle import np_ref
    _script_flags(flags)
    pooled_fn = flm._pooled_cnn_chain
    # the composed form against fp64 at B = 8
    q8, nf8, y8 = _script_case(3, 8)
    monkeypatch.setattr(flm, "_pooled_cnn_chain", _composed_chain)
    small = _run_plugin(flm.LstmCnnDeepCombineChainModel(), q8, y8, nf8, dev)
    t0 = time.time()
    _, _, _, tp = _oracle(torch.from_numpy(np_ref.dequant_l2norm_folded(q8, nf8)), nf8, y8, small["P"], 3, 4, 0.05, [1024, 128], 1)
    host_s = time.time() - t0
    unit = lambda a, b: np.abs(a - b).max() / max(1.0, np.abs(b).max())
    e_c = max(unit(small["grads"][k], t.grad.numpy()) for k, t in tp.items())
    # pooled against composed at B = 128
    q, nf, y = _script_case(1, 128)
    b = _run_plugin(flm.LstmCnnDeepCombineChainModel(), q, y, nf, dev)
    monkeypatch.setattr(flm, "_pooled_cnn_chain", pooled_fn)
    a = _run_plugin(flm.LstmCnnDeepCombineChainModel(), q, y, nf, dev, P=b["P"])
    ep, es = np.abs(a["p"] - b["p"]).max(), np.abs(a["sp"] - b["sp"]).max()
    worst = max(((k, unit(a["grads"][k], b["grads"][k])) for k in a["grads"]), key=lambda kv: kv[1])
    print("composed vs fp64 at B = 8: worst gradient %.3g (host %.0f s); pooled vs composed at B = 128: predictions %.3g support %.3g "
          "worst gradient %s %.3g (bound %.3g)" % ((e_c, host_s, ep, es) + worst + (4 * e_c,)))
    assert ep < 2e-5 and es < 2e-5
    for k in a["grads"]:
        assert unit(a["grads"][k], b["grads"][k]) <= 4 * e_c, k


@pytest.mark.parametrize("distill", [False, True])
def test_whole_training_step_and_its_bitwise_replay(dev, flags, distill):
    """One TrainGraph.step (forward, backward, clip + Adam) of each plugin at B = 32 of the script's shape: finite loss, every parameter
    moved.  Then a second step, taken twice from the same state (parameters and Adam moments restored): bit-identical parameters --
    nothing in the step, the gathered dx included, depends on the order in which the device happened to run it."""
    import yt8m_amd.frame_level_models as flm
    _script_flags(flags)
    q, nf, y = _script_case(11, 32)
    d = np.random.RandomState(2).rand(32, 4716).astype(np.float32) if distill else None
    cls = flm.DistillchainLstmCnnDeepCombineChainModel if distill else flm.LstmCnnDeepCombineChainModel
    import yt8m_amd.train  # noqa: F401  (defines the distillation flags)
    flags.distillation_features = flags.distillation_as_input = distill     # the step hands the reader's distillation predictions on
    g, tg, args, _ = _make_graph(cls(), q, y, nf, dev, d)
    kw = dict(distill_labels_batch=torch.from_numpy(d).to(dev)) if distill else {}
    before = {k: v.data.detach().clone() for k, v in g.vars.items()}
    out = tg.step(*args, **kw)
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    assert np.isfinite(float(out["loss"]))
    for k, v in g.vars.items():
        assert bool(torch.isfinite(v.data).all()) and not torch.equal(v.data, before[k]), k
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step = tg.global_step
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step = step
        tg.step(*args, **kw)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        after.append(g.params.detach().clone())
    assert torch.equal(after[0], after[1])
