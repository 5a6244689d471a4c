"""Bidirectional LSTM plugins (W/all_frame_models/bilstm_model.py, biunilstm_model.py) on the MI355X: the reverse_sequence kernels
(csrc/sequence.hip) bit for bit against a torch gather, both plugins through the plugin surface against an fp64 restatement built here
(oracle.torch_ref.lstm_stack on frames reversed by an explicit per-video loop, the MoE head, the cross entropy), and the overlapped
schedule of the two directions against the sequential one."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.variables import reset_default_graph

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rev_index(F, nf):
    """[B, F] source frame of every output frame: n - 1 - t below n, t from n on."""
    idx = np.tile(np.arange(F), (len(nf), 1))
    for b, n in enumerate(nf):
        n = min(max(int(n), 0), F)
        idx[b, :n] = np.arange(n)[::-1]
    return torch.from_numpy(idx)


def _reverse_loop(x, nf):
    """reverse_sequence on [B, F, ...] (batch-major) by a per-video Python loop."""
    y = x.clone()
    for b, n in enumerate(nf):
        n = int(n)
        if n > 0:
            y[b, :n] = x[b, :n].flip(0)
    return y


@pytest.mark.parametrize("D", [64, 1152, 13])                       # 16-byte rows, the reader's width, byte fall-back
def test_reverse_sequence_u8_is_a_gather_and_its_own_inverse(dev, D):
    rs = np.random.RandomState(D)
    B, F = 7, 9
    q = torch.from_numpy(rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)).to(dev)
    nf = np.array([0, 1, F, 4, F - 1, 2, 7], dtype=np.int32)
    nft = torch.from_numpy(nf).to(dev)
    y = seq_ops.reverse_sequence_u8(q, nft)
    idx = _rev_index(F, nf).to(dev)
    ref = torch.gather(q, 1, idx.view(B, F, 1).expand(B, F, D))
    assert torch.equal(y, ref)
    assert torch.equal(seq_ops.reverse_sequence_u8(y, nft), q)
    assert torch.equal(y.cpu(), _reverse_loop(q.cpu(), nf))


def test_reverse_sequence_u8_refuses_in_place(dev):
    q = torch.zeros((2, 3, 16), dtype=torch.uint8, device=dev)
    nf = torch.tensor([3, 1], dtype=torch.int32, device=dev)
    lib = L.lib()
    assert lib.yt8m_reverse_sequence_u8(_p(q), _p(nf), _p(q), 2, 3, 16, _st()) == -1


@pytest.mark.parametrize("H", [128, 6])                             # float4 rows, scalar fall-back
def test_reverse_sequence_f32_tm_writes_only_its_column_window(dev, H):
    rs = np.random.RandomState(H)
    F, B = 11, 6
    x = torch.from_numpy(rs.randn(F, B, H).astype(np.float32)).to(dev)
    nf = np.array([0, 1, F, 5, 10, 3], dtype=np.int32)
    nft = torch.from_numpy(nf).to(dev)
    ref = _reverse_loop(x.transpose(0, 1).cpu(), nf).transpose(0, 1)
    y = seq_ops.reverse_sequence_tm(x, nft)
    assert torch.equal(y.cpu(), ref)
    assert torch.equal(seq_ops.reverse_sequence_tm(y, nft), x)
    # leading dimension 3H, column offset H: columns [H, 2H) hold the reversal, the rest keeps its sentinel
    out = torch.full((F, B, 3 * H), -7.0, dtype=torch.float32, device=dev)
    lib = L.lib()
    L.check(lib.yt8m_reverse_sequence_f32_tm(_p(x), H, _p(nft), _p(out), 3 * H, H, F, B, H, _st()))
    o = out.cpu()
    assert torch.equal(o[:, :, H:2 * H], ref)
    assert bool((o[:, :, :H] == -7.0).all()) and bool((o[:, :, 2 * H:] == -7.0).all())
    # strided source (the right half of a [F,B,2H] gradient) back into a contiguous block: the inverse
    back = torch.empty((F, B, H), dtype=torch.float32, device=dev)
    L.check(lib.yt8m_reverse_sequence_f32_tm(_p(out[:, :, H:]), 3 * H, _p(nft), _p(back), H, 0, F, B, H, _st()))
    assert torch.equal(back, x)


def test_bi_concat_forward_and_gradient(dev):
    rs = np.random.RandomState(3)
    F, B, H = 8, 5, 32
    nf = np.array([0, 1, 8, 3, 6], dtype=np.int32)
    nft = torch.from_numpy(nf).to(dev)
    a = torch.from_numpy(rs.randn(F, B, H).astype(np.float32)).to(dev).requires_grad_(True)
    b = torch.from_numpy(rs.randn(F, B, H).astype(np.float32)).to(dev).requires_grad_(True)
    g = torch.from_numpy(rs.randn(F, B, 2 * H).astype(np.float32)).to(dev)
    l1 = seq_ops.bi_concat(a, b, nft)
    rb = _reverse_loop(b.detach().transpose(0, 1).cpu(), nf).transpose(0, 1)
    assert torch.equal(l1.detach().cpu(), torch.cat([a.detach().cpu(), rb], 2))
    l1.backward(g)
    assert torch.equal(a.grad.cpu(), g[:, :, :H].cpu())
    assert torch.equal(b.grad.cpu(), _reverse_loop(g[:, :, H:].transpose(0, 1).cpu(), nf).transpose(0, 1))


# ---- the plugins ------------------------------------------------------------------------------------------------------------------
def _run_plugin(model, x, y, nf, dev, P=None, rs=None, scale=0.06):
    import yt8m_amd.train as train
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(model, batch_size=x.shape[0], graph=g)
    xd, yd, nfd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev)
    tg.forward(xd, yd, nfd)
    g.finalize()
    if P is None:
        # (a contractive recurrence, as in the uni-directional native-stack test of tests/test_gpu_round3.py: with large weights 32 steps
        # amplify fp32 rounding chaotically on any implementation)
        # The bw direction's weights at a third of the fw scale: the stack's scratch carries max |W| scale words from its forward call to
        # its backward call, so with equal scales a scratch the two directions shared by mistake would go unnoticed.
        P = {k: (rs.randn(*v.shape) * (scale / 3 if "/bw/" in k else scale)).astype(np.float32) for k, v in g.vars.items()}
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    calls = dict(seq_ops.NATIVE_CALLS)
    res = tg.forward(xd, yd, nfd)
    loss = tg.loss(res, yd)
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    native = (seq_ops.NATIVE_CALLS["fwd"] - calls["fwd"], seq_ops.NATIVE_CALLS["bwd"] - calls["bwd"])
    grads = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if v.trainable}
    return res["predictions"].detach().cpu().numpy().astype(np.float64), float(loss.detach()), grads, P, native


def _oracle(which, x64, nf, y, P, L_, device="cpu"):
    """fp64 restatement (on `device`: the bench shape's 300 steps run it on the GPU, still in float64)."""
    from oracle import torch_ref
    tp = {k: torch.from_numpy(v.astype(np.float64)).to(device).requires_grad_(True) for k, v in P.items()}
    x64 = x64.to(device)
    nft = torch.from_numpy(nf).to(device)
    xr = _reverse_loop(x64, nf)
    if which == "bi":
        lay = lambda d: [(tp["RNN/bidirectional_rnn/%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (d, l)],
                          tp["RNN/bidirectional_rnn/%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (d, l)]) for l in range(L_)]
        _, cf, hf = torch_ref.lstm_stack(x64, nft, lay("fw"))
        _, cb, hb = torch_ref.lstm_stack(xr, nft, lay("bw"))
        state = torch.cat([t for l in range(L_) for t in (cf[l], hf[l])] + [t for l in range(L_) for t in (cb[l], hb[l])], 1)
    else:
        cell = lambda s: [(tp[s + "basic_lstm_cell/weights"], tp[s + "basic_lstm_cell/biases"])]
        of, cf, hf = torch_ref.lstm_stack(x64, nft, cell("RNN/bidirectional_rnn/fw/"))
        ob, cb, hb = torch_ref.lstm_stack(xr, nft, cell("RNN/bidirectional_rnn/bw/"))
        l1 = torch.cat([of, _reverse_loop(ob, nf)], 2)
        _, c2, h2 = torch_ref.lstm_stack(l1, nft, cell("RNN/"))
        state = torch.cat([cf[0], hf[0], cb[0], hb[0], c2[0], h2[0]], 1)
    pr = torch_ref.moe(state, tp["gates/weights"], tp["experts/weights"], tp["experts/biases"], 2)
    lr = torch_ref.cross_entropy(pr, torch.from_numpy(y.astype(np.float64)).to(device))
    lr.backward()
    return pr.detach().cpu().numpy(), float(lr.detach()), tp


def _check(pa, la, ga, pr, lr, tp, which):
    assert np.abs(pa - pr).max() < 1e-4
    assert abs(la - lr) < 1e-4 * max(1.0, abs(lr))
    dirs = ["RNN/bidirectional_rnn/fw/", "RNN/bidirectional_rnn/bw/"] + (["RNN/basic_lstm_cell/"] if which == "biuni" else [])
    for d in dirs:                                                   # every direction's weights have a gradient, and it matches
        assert any(k.startswith(d) for k in ga), d
    for k, t in tp.items():
        if t.grad is not None:
            r = t.grad.cpu().numpy()
            assert np.abs(ga[k] - r).max() <= 5e-4 * max(1.0, np.abs(r).max()), k


@pytest.mark.parametrize("which,u8", [("bi", True), ("bi", False), ("biuni", True), ("biuni", False)])
@pytest.mark.parametrize("overlap", [False, True])
def test_bidirectional_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, which, u8, overlap):
    from oracle import np_ref
    import yt8m_amd.frame_level_models as flm
    monkeypatch.setattr(seq_ops, "BI_OVERLAP", overlap)
    rs = np.random.RandomState(5 + u8)
    B, F, D, H, V = 32, 32, 64, 256, 13                               # F B = 1024 rows: the native stack's smallest
    flags.lstm_cells, flags.lstm_layers = str(H), 2
    nf = rs.randint(0, F + 1, size=B).astype(np.int32)
    nf[0], nf[1], nf[2] = F, 1, 0
    y = rs.rand(B, V) < 0.2
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf))
    x = q if u8 else x64.numpy().astype(np.float32)
    if not u8:
        x64 = torch.from_numpy(x.astype(np.float64))
    model = flm.BiLstmModel() if which == "bi" else flm.BiUniLstmModel()
    runs = seq_ops.BI_OVERLAP_RUNS[0]
    pa, la, ga, P, native = _run_plugin(model, x, y, nf, dev, rs=rs)
    n_stacks = 2 if which == "bi" else 3
    assert native == (n_stacks, n_stacks), native                   # both directions (and BiUni's layer 2) on the native stack
    assert (seq_ops.BI_OVERLAP_RUNS[0] > runs) == overlap
    pr, lr, tp = _oracle(which, x64, nf, y, P, 2 if which == "bi" else 1)
    _check(pa, la, ga, pr, lr, tp, which)


def test_overlapped_directions_equal_the_sequential_form_at_the_bench_shape(dev, flags, monkeypatch):
    """B = 128, F = 300, D = 1152 uint8, H = 1024, L = 2: predictions, loss and every gradient of the overlapped schedule against the
    sequential one (same kernels, same arithmetic per direction), the persistent time-out words clear after each."""
    import yt8m_amd.frame_level_models as flm
    rs = np.random.RandomState(1)
    B, F, D, V = 128, 300, 1152, 4716
    flags.lstm_cells, flags.lstm_layers = "1024", 2
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1
    y = rs.rand(B, V) < 3.4 / V
    monkeypatch.setattr(seq_ops, "BI_OVERLAP", False)
    pa, la, ga, P, na = _run_plugin(flm.BiLstmModel(), q, y, nf, dev, rs=np.random.RandomState(2))
    monkeypatch.setattr(seq_ops, "BI_OVERLAP", True)
    pb, lb, gb, _, nb = _run_plugin(flm.BiLstmModel(), q, y, nf, dev, P=P)
    assert na == nb == (2, 2)
    assert np.abs(pa - pb).max() < 1e-5 and abs(la - lb) < 1e-5 * max(1.0, abs(la))
    for k in ga:
        assert np.abs(ga[k] - gb[k]).max() <= 1e-4 * max(1.0, np.abs(ga[k]).max()), k


@pytest.mark.parametrize("which", ["bi", "biuni"])
def test_bidirectional_plugins_match_the_fp64_restatement_at_the_bench_shape(dev, flags, which):
    """B = 128, F = 300, D = 1152 uint8 frames, H = 1024 (L = 2 for BiLstm), V = 4716: predictions, loss and every gradient through the
    plugin surface against the fp64 restatement (run on the device in float64: 300 steps of a 1024-cell stack).  Weights at the scale
    of the variables' own initialiser (xavier: ~0.02), the bw direction's at a third of it."""
    from oracle import np_ref
    import yt8m_amd.frame_level_models as flm
    rs = np.random.RandomState(7)
    B, F, D, V = 128, 300, 1152, 4716
    flags.lstm_cells, flags.lstm_layers = "1024", 2
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1], nf[2] = F, 1, 0
    y = rs.rand(B, V) < 3.4 / V
    y[:, 0] = True                                                     # every video has a label
    model = flm.BiLstmModel() if which == "bi" else flm.BiUniLstmModel()
    pa, la, ga, P, native = _run_plugin(model, q, y, nf, dev, rs=rs, scale=0.02)
    n_stacks = 2 if which == "bi" else 3
    assert native == (n_stacks, n_stacks), native
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf))
    pr, lr, tp = _oracle(which, x64, nf, y, P, 2 if which == "bi" else 1, device=dev)
    _check(pa, la, ga, pr, lr, tp, which)


def test_overlapped_training_step_updates_the_parameters_like_the_sequential_one(dev, flags, monkeypatch):
    """One whole TrainGraph.step (forward, backward, clip + Adam -- the early pass inside a stack's backward included) of BiLstmModel at
    the bench shape, with no device synchronisation inside it, in the overlapped and in the sequential form from the same parameters:
    the optimiser pass on the caller's stream must see the bw direction's gradients that the overlapped form computes on a side
    stream, so the parameters after the step agree."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    rs = np.random.RandomState(9)
    B, F, D, V = 128, 300, 1152, 4716
    flags.lstm_cells, flags.lstm_layers = "1024", 2
    q = torch.from_numpy(rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)).to(dev)
    nf = torch.from_numpy(rs.randint(1, F + 1, size=B).astype(np.int32)).to(dev)
    y = torch.from_numpy(rs.rand(B, V) < 3.4 / V).to(dev)
    after, grads, P = {}, {}, None
    for overlap in (False, True):
        monkeypatch.setattr(seq_ops, "BI_OVERLAP", overlap)
        g = reset_default_graph(device=dev, seed=0)
        tg = train.TrainGraph(flm.BiLstmModel(), batch_size=B, graph=g)
        tg.forward(q, y, nf)
        g.finalize()
        if P is None:
            P = {k: v.data.detach().clone() for k, v in g.vars.items()}
        for k, v in g.vars.items():
            v.data.copy_(P[k])
        torch.cuda.synchronize()
        runs = seq_ops.BI_OVERLAP_RUNS[0]
        tg.step(q, y, nf)                                              # no synchronisation until the parameters are read
        assert (seq_ops.BI_OVERLAP_RUNS[0] > runs) == overlap
        after[overlap] = {k: v.data.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if v.trainable}
        grads[overlap] = {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in g.vars.items() if v.trainable}
        seq_ops.check_persist_errors()
    assert any("/bw/" in k for k in after[True])
    for k in after[False]:
        gs, go = grads[False][k], grads[True][k]
        assert np.abs(gs - go).max() <= 1e-4 * max(1.0, np.abs(gs).max()), k
        dp = np.abs(after[False][k] - after[True][k])
        p0 = P[k].detach().cpu().numpy().astype(np.float64)
        step = np.abs(after[False][k] - p0)
        # where the gradient is clearly non-zero Adam's first step is ~lr_t * sign(g): the two forms must agree there to rounding; a
        # pass that read a stale or half-written gradient buffer would move these elements differently
        firm = np.abs(gs) > 1e-3 * max(np.abs(gs).max(), 1e-30)
        assert firm.any(), k
        assert dp[firm].max() <= 1e-6 + 1e-3 * step[firm].max(), (k, dp[firm].max())
