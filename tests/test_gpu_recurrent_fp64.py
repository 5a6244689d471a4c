"""-m gpu: the GRU and LayerNorm-LSTM layers at H = 1024 (the plugins' default width) element by element against the fp64 restatement
(oracle/torch_ref.gru_stack / lnlstm_stack): outputs, final states, dx and every parameter gradient.  At this width the GRU forward
runs on the persistent kernel (csrc/gru_persist.inl) by default and the hoisted input projections and their dx take the three-f16-
product (h2) forms from 512 frame rows on; the tests at H <= 512 (tests/test_gpu_kernels.py) reach neither.  A checksum over a whole
model (tests/test_gpu_fullsize_recurrent_golden.py) can average a subtly wrong element away; these bounds do not."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import torch_ref
import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
B, HH = 128, 1024


def _vars(dev, arrays):
    from yt8m_amd.variables import reset_default_graph, zeros
    g = reset_default_graph(device=dev)
    g.begin_step()
    vs = [g.get_variable("v%d" % i, a.shape, zeros) for i, a in enumerate(arrays)]
    g.finalize()
    for v, a in zip(vs, arrays):
        v.data.copy_(torch.from_numpy(a).to(dev))
    return vs


def _frames(rs, F, Din):
    """l2-normalised frames (what layer 0 reads) time-major [F,B,Din] as float32"""
    x = rs.randn(F, B, Din)
    return (x / np.linalg.norm(x, axis=2, keepdims=True)).astype(np.float32)


def _num_frames(rs, F, boundary):
    nf = rs.randint(0, F + 1, size=B).astype(np.int32)
    nf[:8] = [0, 1, F, F - 1, boundary - 1, boundary, boundary + 1, 2]
    return nf


def _xavier(rs, shape):
    return ((rs.random_sample(shape) * 2 - 1) * np.sqrt(6.0 / (shape[0] + shape[1]))).astype(np.float32)


def _err(got, ref):
    """max |got - ref| relative to max(1, max |ref|)"""
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else got
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def _launches():
    n = ctypes.c_int64(0)
    L.check(L.lib().yt8m_lstm_persist_placement_stats(ctypes.byref(n), None, None, 1))
    return n.value


@pytest.mark.parametrize("Din,F", [(64, 40), (1152, 24)])
@pytest.mark.parametrize("persist", [True, False])
def test_gru_layer_at_h1024_matches_fp64(dev, monkeypatch, persist, Din, F):
    """seq_ops.gru_layer at B = 128, H = 1024 with the persistent forward on (the default) and off, against torch_ref.gru_stack in
    fp64: ragged num_frames with 0, 1, F and lengths around a mid-sequence boundary, a gradient on every output AND on the final state
    (GruWithPoolingModel feeds one).  Din = 1152: the hoisted products and dx on the h2 forms; Din = 64: the fp32 products."""
    rs = np.random.RandomState(71 + Din)
    x = _frames(rs, F, Din)
    nf = _num_frames(rs, F, F // 2)
    arrs = [_xavier(rs, (Din + HH, 2 * HH)), (1 + 0.05 * rs.randn(2 * HH)).astype(np.float32),
            _xavier(rs, (Din + HH, HH)), (0.05 * rs.randn(HH)).astype(np.float32)]
    go, gh = rs.randn(F, B, HH).astype(np.float32), rs.randn(B, HH).astype(np.float32)
    monkeypatch.setattr(seq_ops, "GRU_PERSIST_FWD", persist)
    assert L.lib().yt8m_gru_persist_supported(B, HH), "the persistent GRU forward is the default at B = 128, H = 1024"
    Wg, bg, Wc, bc = _vars(dev, arrs)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    _launches()
    out, h = seq_ops.gru_layer(xt, Wg, bg, Wc, bc, torch.from_numpy(nf).to(dev))
    torch.cuda.synchronize()
    assert _launches() == (1 if persist else 0)
    ((out * torch.from_numpy(go).to(dev)).sum() + (h * torch.from_numpy(gh).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    tx = torch.from_numpy(x.astype(np.float64)).transpose(0, 1).requires_grad_(True)
    tp = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in arrs]
    to, th = torch_ref.gru_stack(tx, torch.from_numpy(nf.astype(np.int64)), [tuple(tp)])
    ((to * torch.from_numpy(go.astype(np.float64)).transpose(0, 1)).sum() + (th[0] * torch.from_numpy(gh.astype(np.float64))).sum()).backward()
    e = {"out": _err(out.transpose(0, 1), to.detach().numpy()), "h": _err(h, th[0].detach().numpy()),
         "dx": _err(xt.grad.transpose(0, 1), tx.grad.numpy())}
    e.update({n: _err(v.grad, t.grad.numpy()) for n, v, t in zip(("dWg", "dbg", "dWc", "dbc"), (Wg, bg, Wc, bc), tp)})
    print("GRU H=1024 Din=%d F=%d persist=%s:" % (Din, F, persist), " ".join("%s %.2g" % kv for kv in e.items()))
    # measured on an MI355X: outputs / final state <= 1.2e-7, gradients <= 6.1e-7 (persistent forward on or off)
    assert e["out"] < 2e-6 and e["h"] < 2e-6, e
    assert max(e["dx"], e["dWg"], e["dbg"], e["dWc"], e["dbc"]) < 5e-6, e
    # dead rows: the state is carried through unchanged, the outputs are zero
    assert float(out[:, 0].abs().max()) == 0.0 and float(h[0].abs().max()) == 0.0


def test_chained_persistent_gru_forward_parts_match_fp64(dev):
    """Two chained yt8m_gru_persist_fwd launches (steps [0, k) then [k, F), the second starting from hs[k] that the first wrote) against
    an fp64 GRU recurrence on the same hoisted inputs: videos that end exactly on the boundary (num_frames = k), one step before and after
    it, and 0, 1, F; outputs, every state hs[t], r * h and the final state.  The single launch over [0, F) gives the same values."""
    lib = L.lib()
    F, k = 36, 17
    assert lib.yt8m_gru_persist_supported(B, HH)
    g = torch.Generator(device=dev).manual_seed(73)
    zg0 = torch.randn((F, B, 2 * HH), device=dev, generator=g) * 0.5 + torch.cat([torch.ones(HH, device=dev), torch.zeros(HH, device=dev)])
    zc0 = torch.randn((F, B, HH), device=dev, generator=g) * 0.5
    Wg = (torch.rand((HH, 2 * HH), device=dev, generator=g) - 0.5) * 0.1
    Wc = (torch.rand((HH, HH), device=dev, generator=g) - 0.5) * 0.1
    nf = torch.from_numpy(_num_frames(np.random.RandomState(74), F, k)).to(dev)
    # fp64 recurrence
    h = torch.zeros((B, HH), dtype=torch.float64, device=dev)
    Wgd, Wcd = Wg.double(), Wc.double()
    hs_ref, rh_ref, out_ref = [h], [], []
    for t in range(F):
        r, u = torch.sigmoid(zg0[t].double() + h @ Wgd).chunk(2, 1)
        c = torch.tanh(zc0[t].double() + (r * h) @ Wcd)
        hn = u * h + (1 - u) * c
        live = (t < nf).unsqueeze(1)
        rh_ref.append(r * h)
        h = torch.where(live, hn, h)
        hs_ref.append(h)
        out_ref.append(torch.where(live, hn, torch.zeros_like(hn)))
    hs_ref, rh_ref, out_ref = torch.stack(hs_ref), torch.stack(rh_ref), torch.stack(out_ref)
    nbytes = lib.yt8m_gru_persist_workspace_bytes(B, HH, F)
    res = {}
    for parts in ([(0, F)], [(0, k), (k, F - k)]):
        zg, zc = zg0.clone(), zc0.clone()
        hs = torch.zeros((F + 1, B, HH), device=dev)
        rh = torch.zeros((F, B, HH), device=dev)
        out = torch.full((F, B, HH), float("nan"), device=dev)
        pws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        for t0, T in parts:
            L.check(lib.yt8m_gru_persist_fwd(_p(zg), _p(zc), _p(Wg), 2 * HH, _p(Wc), HH, _p(hs), _p(rh), _p(out), _p(nf), t0, T, B, HH,
                                             _p(pws), nbytes, _stream()))
        torch.cuda.synchronize()
        e = {"out": float((out.double() - out_ref).abs().max()), "hs": float((hs.double() - hs_ref).abs().max()),
             "rh": float((rh.double() - rh_ref).abs().max())}
        print("persistent GRU forward, parts %s:" % (parts,), e)
        assert max(e.values()) < 2e-6, (parts, e)                  # measured 2.5e-7
        res[len(parts)] = (out, hs)
    assert float((res[1][0] - res[2][0]).abs().max()) < 1e-6 and float((res[1][1] - res[2][1]).abs().max()) < 1e-6


@pytest.mark.parametrize("keep", [1.0, 0.7])
def test_lnlstm_layer_at_h1024_matches_fp64(dev, keep):
    """seq_ops.lnlstm_layer at B = 128, H = 1024, D = 1152 (hoisted product and dx on the h2 forms) with and without recurrent dropout,
    against torch_ref.lnlstm_stack in fp64: outputs, final (c, h), dx, the weights' and all ten gamma / beta gradients."""
    F, Din = 24, 1152
    rs = np.random.RandomState(75)
    x = _frames(rs, F, Din)
    nf = _num_frames(rs, F, F // 2)
    arrs = [_xavier(rs, (Din + HH, 4 * HH))]
    arrs += [(rs.rand(HH) + 0.5).astype(np.float32) for _ in range(5)] + [(rs.randn(HH) * 0.2).astype(np.float32) for _ in range(5)]
    go, gc, gh = rs.randn(F, B, HH).astype(np.float32), rs.randn(B, HH).astype(np.float32), rs.randn(B, HH).astype(np.float32)
    vs = _vars(dev, arrs)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    seed = 0x5EED0017
    out, c, h = seq_ops.lnlstm_layer(xt, vs[0], vs[1:6], vs[6:11], torch.from_numpy(nf).to(dev), forget_bias=1.0, keep_prob=keep, seed=seed)
    ((out * torch.from_numpy(go).to(dev)).sum() + (c * torch.from_numpy(gc).to(dev)).sum()
     + (h * torch.from_numpy(gh).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    tx = torch.from_numpy(x.astype(np.float64)).transpose(0, 1).requires_grad_(True)
    tp = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in arrs]
    to, tc, th = torch_ref.lnlstm_stack(tx, torch.from_numpy(nf.astype(np.int64)), [(tp[0], tp[1:6], tp[6:11])],
                                        dropout_spec=None if keep >= 1 else (keep, [seed]))
    ((to * torch.from_numpy(go.astype(np.float64)).transpose(0, 1)).sum() + (tc[0] * torch.from_numpy(gc.astype(np.float64))).sum()
     + (th[0] * torch.from_numpy(gh.astype(np.float64))).sum()).backward()
    e = {"out": _err(out.transpose(0, 1), to.detach().numpy()), "c": _err(c, tc[0].detach().numpy()), "h": _err(h, th[0].detach().numpy()),
         "dx": _err(xt.grad.transpose(0, 1), tx.grad.numpy())}
    e.update({"d%d" % i: _err(v.grad, t.grad.numpy()) for i, (v, t) in enumerate(zip(vs, tp))})
    print("LN-LSTM H=1024 keep=%g:" % keep, " ".join("%s %.2g" % kv for kv in e.items()))
    # measured on an MI355X: outputs / final states <= 6.7e-6, gradients <= 5.6e-6 (with or without dropout)
    assert e["out"] < 2e-5 and e["c"] < 2e-5 and e["h"] < 2e-5, e
    assert max(v for n, v in e.items() if n not in ("out", "c", "h")) < 2e-5, e
