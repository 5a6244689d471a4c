"""The frame-pyramid kernel (csrc/frame_pyramid.hip) and the two temporal-pooling LSTM plugins on the MI355X: the kernel through the C ABI
against the fp64 restatement of tests/test_temporal_pool_host.py and against the existing resolution kernel, ops.frame_pyramid fused
against composed, the plugins through the plugin surface against fp64 restatements assembled from oracle.torch_ref (lstm_stack, moe,
cross_entropy, l2_normalize), and whole training steps with their bitwise replay."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
from test_temporal_pool_host import PYRAMID_B, PYRAMID_F, PYRAMID_LEVELS, PYRAMID_NF, PYRAMID_WIDTHS, pyramid_case, pyramid_np
from test_transform_host import dequantize64_np, resolution_np
from yt8m_amd.variables import reset_default_graph

pytestmark = pytest.mark.gpu

EPS = 1e-12
GUARD = -7.0
NGUARD = 8                               # guard words behind every output
U = 2.0 ** -24


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _outputs(B, F, levels, widths, dev):
    """Guard-filled flat buffers: y[l][s] of (F >> (l + 1)) * B * w floats + NGUARD guard words, num_frames_out[l] of B + NGUARD."""
    ys = [[torch.full(((F >> (l + 1)) * B * w + NGUARD,), GUARD, device=dev) for w in widths] for l in range(levels)]
    ns = [torch.full((B + NGUARD,), -7, dtype=torch.int32, device=dev) for _ in range(levels)]
    return ys, ns


def _call(q, nf, B, F, levels, widths, ys, ns):
    n = len(widths)
    return L.lib().yt8m_frame_pyramid_u8(_p(q), _p(nf), B, F, sum(widths), levels, n, (ctypes.c_int64 * n)(*widths),
                                         (ctypes.c_void_p * (levels * n))(*[t.data_ptr() for row in ys for t in row]),
                                         None if ns is None else (ctypes.c_void_p * levels)(*[t.data_ptr() for t in ns]), EPS, _st())


def _check(q, nf, B, F, levels, widths, ys, ns, tag):
    """Outputs against the fp64 restatement: max |y - ref| < 1e-6 (the bound of tests/test_gpu_transform.py::_check_against_ref for the
    same arithmetic on rows of norm 1), empty groups exactly zero, num_frames_out exact, every guard word intact."""
    frames = np.full(B, F, dtype=np.int32) if nf is None else nf
    ref, nref = pyramid_np(dequantize64_np(q, frames), frames, levels, widths)
    worst = 0.0
    for l in range(levels):
        r = 2 << l
        F2 = F // r
        empty = (np.arange(F2).reshape(-1, 1) * r) >= frames.reshape(1, -1)                # [F2, B]: groups with no real frame
        for s, w in enumerate(widths):
            flat = ys[l][s].cpu().numpy()
            assert (flat[F2 * B * w:] == GUARD).all(), (tag, l, s)
            y = flat[:F2 * B * w].reshape(F2, B, w).astype(np.float64)
            worst = max(worst, float(np.abs(y - ref[l][s]).max()))
            assert not y[empty].any(), (tag, l, s)
            assert y[~empty].any(axis=-1).all(), (tag, l, s)
        if ns is not None:
            n_out = ns[l].cpu().numpy()
            assert np.array_equal(n_out[:B], nref[l]) and (n_out[B:] == -7).all(), (tag, l)
    print("%s: max|y - ref| = %.3g" % (tag, worst))
    assert worst < 1e-6
    return ref


@pytest.mark.parametrize("widths", PYRAMID_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_frame_pyramid_kernel_against_the_fp64_restatement(dev, widths):
    """B = 3, F = 35, 4 levels of 17, 8, 4 and 2 rows: frames 32..34 reach level 0 only (the partial tail block); num_frames = 35, 1, 20:
    a video whose coarse levels are empty but for a one-frame group, ragged groups elsewhere; the bytes of the padding frames are zero.
    Widths: 16-byte units, 4-byte units with a segment boundary off a 16-byte line, single bytes, one segment."""
    B, F, levels = PYRAMID_B, PYRAMID_F, PYRAMID_LEVELS
    q = pyramid_case(widths)
    qd, nfd = torch.from_numpy(q).to(dev), torch.from_numpy(PYRAMID_NF).to(dev)
    ys, ns = _outputs(B, F, levels, widths, dev)
    L.check(_call(qd, nfd, B, F, levels, widths, ys, ns))
    _check(q, PYRAMID_NF, B, F, levels, widths, ys, ns, "widths %s" % widths)
    if widths == [1152]:
        # against the existing kernel: both are single fp32 roundings of fp64 values that differ only in summation order, the outputs
        # are at most 1 in magnitude -- within one ulp of 1
        differ = 0
        for l in range(levels):
            old, n_old = ops.resolution_mean(qd, nfd, 2 << l, l2norm=True)
            new = ys[l][0][:(F >> (l + 1)) * B * 1152].view(F >> (l + 1), B, 1152)
            assert torch.equal(n_old, ns[l][:B])
            d = (new - old.transpose(0, 1)).abs()
            differ += int((d > 0).sum())
            assert float(d.max()) <= 2.0 ** -23
        print("against yt8m_resolution_mean_u8: %d elements differ" % differ)


def test_frame_pyramid_kernel_without_a_tail_and_without_num_frames(dev):
    B, levels, widths = PYRAMID_B, PYRAMID_LEVELS, [16, 16]
    # F = 32: every level ends on the block's edge
    nf = np.array([32, 1, 20], dtype=np.int32)
    q = pyramid_case(widths, F=32, num_frames=nf)
    ys, ns = _outputs(B, 32, levels, widths, dev)
    L.check(_call(torch.from_numpy(q).to(dev), torch.from_numpy(nf).to(dev), B, 32, levels, widths, ys, ns))
    _check(q, nf, B, 32, levels, widths, ys, ns, "F = 32")
    # num_frames = NULL: every frame is real (and no num_frames_out either)
    q = np.random.RandomState(3).randint(0, 256, size=(B, PYRAMID_F, 32)).astype(np.uint8)
    ys, _ = _outputs(B, PYRAMID_F, levels, widths, dev)
    L.check(_call(torch.from_numpy(q).to(dev), None, B, PYRAMID_F, levels, widths, ys, None))
    full = np.full(B, PYRAMID_F, dtype=np.int32)
    ref, _ = pyramid_np(dequantize64_np(q, full), full, levels, widths)
    for l in range(levels):
        for s in range(2):
            flat = ys[l][s].cpu().numpy()
            n = (PYRAMID_F >> (l + 1)) * B * 16
            assert (flat[n:] == GUARD).all() and np.abs(flat[:n].reshape(-1, B, 16) - ref[l][s]).max() < 1e-6


def test_frame_pyramid_kernel_many_workgroups(dev):
    B, F, levels, widths = 130, 35, 2, [16, 16]
    nf = np.random.RandomState(7).randint(0, F + 1, size=B).astype(np.int32)
    nf[:3] = (F, 1, 0)
    q = pyramid_case(widths, F=F, B=B, num_frames=nf)
    ys, ns = _outputs(B, F, levels, widths, dev)
    L.check(_call(torch.from_numpy(q).to(dev), torch.from_numpy(nf).to(dev), B, F, levels, widths, ys, ns))
    _check(q, nf, B, F, levels, widths, ys, ns, "B = 130")


def test_frame_pyramid_kernel_refuses_an_unsupported_shape(dev):
    """517 columns in single bytes are more than a lane's registers hold: the error, and nothing written."""
    B, F, levels, widths = 2, 8, 2, [512, 5]
    assert not ops.frame_pyramid_supported(517, widths, levels)
    q = torch.zeros(B, F, 517, dtype=torch.uint8, device=dev)
    ys, ns = _outputs(B, F, levels, widths, dev)
    assert _call(q, None, B, F, levels, widths, ys, ns) == -2 and b"unsupported" in L.lib().yt8m_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for row in ys for t in row) and all(bool((t == -7).all()) for t in ns)


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [[8, 8], [1024, 128]], ids=lambda w: "x".join(map(str, w)))
def test_op_fused_and_composed_against_the_restatement(dev, monkeypatch, widths):
    q = pyramid_case(widths)
    ref, nref = pyramid_np(dequantize64_np(q, PYRAMID_NF), PYRAMID_NF, PYRAMID_LEVELS, widths)
    calls = []
    mean = ops.resolution_mean
    monkeypatch.setattr(ops, "resolution_mean", lambda *a, **k: calls.append(1) or mean(*a, **k))
    for fused in (True, False):
        monkeypatch.setattr(ops, "FRAME_PYRAMID_FUSED", fused)
        del calls[:]
        parts, frames = ops.frame_pyramid(torch.from_numpy(q).to(dev), torch.from_numpy(PYRAMID_NF), PYRAMID_LEVELS, widths)
        assert len(calls) == (0 if fused else PYRAMID_LEVELS)             # the kernel ran / every level was composed
        for l in range(PYRAMID_LEVELS):
            assert frames[l].is_cuda and frames[l].dtype == torch.int32 and np.array_equal(frames[l].cpu().numpy(), nref[l])
            for s, w in enumerate(widths):
                y = parts[l][s]
                assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (PYRAMID_F >> (l + 1), PYRAMID_B, w)
                assert not y.requires_grad
                err = np.abs(y.cpu().numpy() - ref[l][s]).max()
                assert err < 1e-6, (fused, l, s, err)
    with pytest.raises(ValueError):
        ops.frame_pyramid(torch.from_numpy(q).to(dev), torch.from_numpy(PYRAMID_NF), 6, widths)          # 2^6 > F
    with pytest.raises(ValueError):
        ops.frame_pyramid(torch.from_numpy(q).to(dev), torch.from_numpy(PYRAMID_NF), 2, widths[:1])      # widths do not add up


def test_op_on_floats_takes_the_composed_form(dev, monkeypatch):
    """Floats are averaged as they are (the padding rows, non-zero here, count).  Bounds of
    tests/test_gpu_transform.py::test_resolution_mean_f32_is_the_unmasked_mean, per part: a sequential fp32 sum of r terms and one
    multiply by 1/r are off by at most (r + 1) u max|x|; normalised, the element's and the norm's errors both scale with 1 / (the
    smallest part norm), plus the roundings of the scale and of the product."""
    widths, levels = [8, 8], 3
    x = np.random.RandomState(2).randn(PYRAMID_B, PYRAMID_F, 16).astype(np.float32)
    monkeypatch.setattr(ops, "FRAME_PYRAMID_FUSED", True)
    parts, frames = ops.frame_pyramid(torch.from_numpy(x).to(dev), torch.from_numpy(PYRAMID_NF).to(dev), levels, widths)
    ref, nref = pyramid_np(x.astype(np.float64), PYRAMID_NF, levels, widths)
    for l in range(levels):
        r = 2 << l
        raw, _ = resolution_np(x, PYRAMID_NF, r, l2norm=False)
        tol = (r + 1) * U * np.abs(x).max()
        assert np.array_equal(frames[l].cpu().numpy(), nref[l])
        for s in range(2):
            toln = 2 * tol / np.sqrt((raw[:, :, 8 * s:8 * s + 8] ** 2).sum(axis=-1)).min() + 4 * U
            err = np.abs(parts[l][s].cpu().numpy() - ref[l][s]).max()
            print("floats r=%d part %d: max|y - ref| = %.3g (bound %.3g)" % (r, s, err, toln))
            assert err <= toln


# ---- the plugins against fp64 ---------------------------------------------------------------------------------------------------------
# Tolerances of tests/test_gpu_multilstm.py::test_plugins_match_the_fp64_restatement.
P_TOL, LOSS_TOL, GRAD_TOL = 1e-4, 1e-4, 5e-4
B, V, LAYERS, RELU, MIX, S = 3, 11, 2, 8, 2, 0.5
FEATURES, CELLS = [8, 8], [8, 4]


def _flags(flags):
    import yt8m_amd.frame_level_models, yt8m_amd.losses, yt8m_amd.train  # noqa: F401, E401  (define the flags set below)
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.moe_num_mixtures = LAYERS, RELU, MIX
    flags.lstm_layers, flags.lstm_cells, flags.feature_sizes = 2, ",".join(map(str, CELLS)), ",".join(map(str, FEATURES))
    flags.support_type, flags.support_loss_percent = ",".join(["label"] * LAYERS), S


def _l2n(x, dim):
    from oracle import torch_ref
    return torch_ref.l2_normalize(x, dim)


def _moe(x, P, scope):
    from oracle import torch_ref
    return torch_ref.moe(x, P["gates%s/weights" % scope], P["experts%s/weights" % scope], P["experts%s/biases" % scope], MIX)


def _layers(P, scope):
    return [(P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)], P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)])
            for l in range(2)]


def _tower_level(row, nf, P, level, sizes):
    """lstm() of both reference files on an l2-normalised row [B,T,sum sizes]: split, every part normalised again, one stack per part
    under lstm<level>RNN<i>.  Returns (final c of every layer, stack-major, side by side; the top outputs side by side)."""
    from oracle import torch_ref
    states, outs, off = [], [], 0
    for i, fs in enumerate(sizes):
        out, c, _ = torch_ref.lstm_stack(_l2n(row[:, :, off:off + fs], 2), nf, _layers(P, "lstm%dRNN%d" % (level, i)))
        states.extend(c)
        outs.append(out)
        off += fs
    return torch.cat(states, 1), torch.cat(outs, 2)


def _ref_multires(x, nf, y, P):
    """multires_lstm_memory_deep_combine_chain_model.py:48-100, 149-165 on the frames as the model receives them."""
    from oracle import torch_ref

    def memories(stage):
        r = 2 ** (LAYERS - stage)
        xm, n = x, nf
        if r > 1:
            T = x.shape[1] // r
            xm = x[:, :T * r].reshape(x.shape[0], T, r, x.shape[2]).mean(2)
            n = torch.div(nf, r, rounding_mode="floor")
        return _tower_level(_l2n(xm, 2), n, P, stage, FEATURES)[0]

    extra, sup = [], []
    nxt = memories(0)
    for l in range(LAYERS):
        sp = _moe(nxt, P, "-prediction-%d" % l)
        sup.append(sp)
        extra.append(_l2n(torch.relu(sp @ P["relu-%d/weights" % l] + P["relu-%d/biases" % l]), 1))
        nxt = torch.cat([memories(l + 1)] + extra, 1)
    pred, sup = _moe(nxt, P, "--main"), torch.cat(sup, 1)
    loss = (1.0 - S) * torch_ref.cross_entropy(pred, y) + S * torch_ref.cross_entropy(sup, torch.cat([y] * LAYERS, 1))
    return pred, sup, loss


def _ref_framehop(x, nf, y, P):
    """framehop_lstm_memory_model.py:59-126: every level k >= 1 is given the ORIGINAL num_frames // 2 and runs no further than its T_k
    rows; the outputs past a video's length are zero rows, selected as they are."""
    from oracle import torch_ref
    state, out = _tower_level(_l2n(x, 2), nf, P, 0, FEATURES)
    states = [state]
    for k in range(1, LAYERS + 1):
        T = out.shape[1] // 2
        hop = out[:, :2 * T].reshape(out.shape[0], T, 2, out.shape[2])[:, :, 1]              # SELECT: rows 1, 3, 5, ..
        steps = torch.minimum(torch.div(nf, 2, rounding_mode="floor"), torch.tensor(T))
        if k == 2:
            assert int((torch.div(nf, 2, rounding_mode="floor") > T).sum()) >= 1             # a video with n // 2 > T_2 is in the case
        state, out = _tower_level(_l2n(hop, 2), steps, P, k, CELLS)
        assert not out[torch.arange(T)[None, :] >= steps[:, None]].any()                     # the zero rows past the sequence length
        states.append(state)
    pred = _moe(torch.cat(states, 1), P, "")
    return pred, None, torch_ref.cross_entropy(pred, y)


def _plugin(name):
    import yt8m_amd.frame_level_models as flm
    if name == "multires":
        return flm.MultiresLstmMemoryDeepCombineChainModel, True, _ref_multires
    return flm.FramehopLstmMemoryModel, False, _ref_framehop


def _data(name, path, seed):
    """(model input as the trainer hands it over, fp64 frames of the restatement, num_frames, labels, rs)."""
    from oracle import np_ref
    rs = np.random.RandomState(seed)
    y = rs.rand(B, V) < 0.2
    if path == "bytes":
        F = 13
        nf = np.array([13, 1, 6] if name == "multires" else [13, 1, 12], dtype=np.int32)
        q = rs.randint(0, 256, size=(B, F, 16)).astype(np.uint8)
        for b, n in enumerate(nf):
            q[b, n:] = 0
        # multires reads the reader's frames as they are (IdenticalTransformer); framehop normalises them first either way
        return q, torch.from_numpy(dequantize64_np(q, nf)), nf, y, rs
    F = 9 if name == "multires" else 13
    nf = np.array([F, 1, F - 1], dtype=np.int32)
    q = rs.randint(0, 256, size=(B, F, 16)).astype(np.uint8)
    x = np_ref.dequant_l2norm_folded(q, nf).astype(np.float32)           # what the DefaultTransformer hands over
    return x, torch.from_numpy(x.astype(np.float64)), nf, y, rs


def _graph(name, x, y, nf, dev, seed=0):
    """The plugin's TrainGraph after one forward pass (variables created, arenas frozen).  multires: IdenticalTransformer, the training
    script's; framehop: the default transformer, folded into the model on bytes (float frames arrive transformed already)."""
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    cls, chain, _ = _plugin(name)
    g = reset_default_graph(device=dev, seed=seed)
    identical = name == "multires" or x.dtype != np.uint8
    tg = train.TrainGraph(cls(), label_loss_fn=losses.MultiTaskCrossEntropyLoss() if chain else None, multitask=chain,
                          batch_size=x.shape[0], graph=g, transformer_class=ft.IdenticalTransformer if identical else None)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    tg.forward(*args)
    g.finalize()
    return g, tg, args


def _stack_index(k):
    """Which stack of the tower a variable belongs to (lstm<level>RNN<i> -> 2 level + i), 0 for everything else."""
    if k.startswith("lstm") and "RNN" in k.split("/")[0]:
        level, i = k.split("/")[0][4:].split("RNN")
        return 2 * int(level) + int(i)
    return 0


def _draw(g, rs):
    """The draws of tests/test_gpu_multilstm.py::_draw -- a contractive recurrence (0.06), heads and FCs 0.2 -- with stack k's weights at
    1 / (k + 1) of that scale: a scratch slot that two stacks shared by mistake shows as one stack wrong."""
    scale = lambda k: 0.06 / (1 + _stack_index(k)) if "basic_lstm_cell" in k else 0.2
    return {k: (rs.randn(*v.data.shape) * scale(k)).astype(np.float32) for k, v in g.vars.items()}


CASES = [("multires", "bytes", True), ("multires", "bytes", False), ("multires", "floats", True), ("framehop", "bytes", True),
         ("framehop", "floats", True)]


@pytest.mark.parametrize("name,path,fused", CASES, ids=lambda v: {True: "kernel", False: "composed"}.get(v, v))
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, path, fused):
    """Each plugin through TrainGraph.forward / loss / backward at B = 3, V = 11, features 8,8, cells 8,4, two LSTM layers,
    deep_chain_layers = 2, 2 mixtures, 8 relu cells: predictions, support predictions, the loss and the gradient of EVERY variable against
    the fp64 restatement.  multires on bytes under IdenticalTransformer (F = 13, num_frames 13, 1, 6) with the pyramid kernel and
    composed, and on pre-normalised floats (F = 9); framehop on bytes (F = 13, num_frames 13, 1, 12: 12 // 2 = 6 > T_2 = 3) and floats.
    The video with one frame has zero-length coarse levels: its memories there are zero in both."""
    monkeypatch.setattr(ops, "FRAME_PYRAMID_FUSED", fused)
    _flags(flags)
    cls, chain, ref = _plugin(name)
    x, x64, nf, y, rs = _data(name, path, 17 + len(name))
    calls = []
    pyramid = ops.frame_pyramid
    monkeypatch.setattr(ops, "frame_pyramid", lambda *a, **k: calls.append(a[0].dtype) or pyramid(*a, **k))
    g, tg, args = _graph(name, x, y, nf, dev)
    assert calls == ([args[0].dtype] if name == "multires" else [])       # once per forward pass, on the input as it arrived
    stacks = sorted({k.split("/")[0] for k in g.vars if "basic_lstm_cell" in k})
    assert stacks == ["lstm%dRNN%d" % (k, i) for k in range(LAYERS + 1) for i in range(2)]
    P = _draw(g, rs)
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    tp = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in P.items()}
    pr, spr, lr = ref(x64, torch.from_numpy(nf), torch.from_numpy(y).double(), tp)
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
        assert tuple(res["support_predictions"].shape) == (B, LAYERS * V)
        assert np.abs(f64(res["support_predictions"]) - spr.detach().numpy()).max() < P_TOL
    else:
        assert "support_predictions" not in res
    for k in tp:
        if "basic_lstm_cell" in k:                                       # every stack takes part: a gradient that is not just zeros
            assert float(tp[k].grad.abs().max()) > 0 and np.abs(grads[k]).max() > 0, k
        assert unit(k) <= GRAD_TOL, k


@pytest.mark.parametrize("name", ["multires", "framehop"])
def test_whole_training_step_and_its_bitwise_replay(dev, flags, monkeypatch, name):
    """One TrainGraph.step per plugin on bytes -- multires under --multitask --label_loss=MultiTaskCrossEntropyLoss --dropout
    --keep_prob=0.9 --feature_transformer=IdenticalTransformer with the pyramid kernel, framehop under the plain loss: a finite loss,
    every parameter moved, no persistent-recurrence error, no eviction from the resident tables; then a second step taken twice from the
    same state: bit-identical parameters."""
    monkeypatch.setattr(ops, "FRAME_PYRAMID_FUSED", True)
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    _flags(flags)
    cls, chain, _ = _plugin(name)
    flags.multitask, flags.label_loss = chain, "MultiTaskCrossEntropyLoss" if chain else "CrossEntropyLoss"
    if chain:
        flags.dropout, flags.keep_prob, flags.feature_transformer = True, 0.9, "IdenticalTransformer"
    x, _, nf, y, rs = _data(name, "bytes", 31)
    g = reset_default_graph(device=dev, seed=0)
    tg = train.build_graph(cls(), batch_size=x.shape[0], graph=g)          # loss and transformer from the flags, as the trainer does
    assert type(tg.label_loss_fn) is getattr(losses, flags.label_loss)
    assert type(tg.transformer) is (ft.IdenticalTransformer if chain else ft.DefaultTransformer)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    tg.forward(*args)
    g.finalize()
    initial = {k: v.data.detach().clone() for k, v in g.vars.items() if v.trainable}
    out = tg.step(*args)
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    assert np.isfinite(float(out["loss"]))
    for k, v in g.vars.items():                                          # every parameter moved
        if v.trainable:
            assert not torch.equal(v.data, initial[k]), k
    before = g.params.detach().clone()
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step, rng_step = tg.global_step, g._rng_step                       # (the dropout masks are keyed by the forward pass's number)
    evictions = seq_ops._STACK_SCRATCH.evictions, seq_ops._PERSIST_WS.evictions
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step, g._rng_step = step, rng_step
        out = tg.step(*args)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        assert np.isfinite(float(out["loss"]))
        after.append(g.params.detach().clone())
    assert torch.equal(after[0], after[1])
    assert not torch.equal(after[0], before)
    assert (seq_ops._STACK_SCRATCH.evictions, seq_ops._PERSIST_WS.evictions) == evictions     # six stacks of a step stay resident
