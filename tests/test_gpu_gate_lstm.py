"""-m gpu: the scalar-gate LSTM layer (csrc/gate_cell.hip, seq_ops.gate_lstm_layer) and LstmGateMultilayerModel against the fp64
restatement (tests/gate_lstm_restatement.py).

Bounds.  The measure is the fp64 tests' max |got - ref| / max(1, max |ref|).  Per quantity the bound is EIGHT times the error of the
float32 restatement (plain torch on the CPU, same inputs) against the float64 one, never below what tests/test_gpu_recurrent_fp64.py holds
the GRU layer to at this width: 2e-6 for outputs and states, 5e-6 for gradients.  The margin covers what the float32 restatement does not
have: the K-split summation order of the products, the 2^-21 per-term error of the three-f16-product hoisted forms and the ~1.5e-7 per
value of the v_exp / v_rcp gate functions compounding over F steps.  Every test prints the measured errors and the float32 restatement's.

Measured on an MI355X (largest error per group, the float32 restatement's error of the same quantity in brackets):
  C ABI, (3, 256, 5) / (5, 2048, 4) / (128, 1024, 6), either backward product form: outputs and states 2.5e-7 / 2.5e-7 / 3.9e-7
    [2.6e-7 / 9.0e-7 / 4.0e-7], dzv and dzs 2.1e-7 / 2.4e-7 / 2.6e-7 [1.9e-7 / 2.8e-7 / 1.8e-7]
  gate_lstm_layer at H = 1024, kernels: floats out 3.3e-7 c_last 3.6e-7 [1.9e-7, 2.6e-7], gradients 5.3e-7 (dWs) [3.2e-7];
    bytes out 1.6e-7 c_last 2.0e-7 [8.8e-8, 1.4e-7], gradients 7.7e-7 (dUs) [2.8e-7]
  the composed form on the device: floats out 6.3e-7, gradients 1.0e-6 (dWv); bytes c_last 3.6e-7, gradients 1.0e-6 (dWv)
  H = 192 composed: out 8.5e-8 [1.1e-7], gradients 8.5e-7 (dbi) [1.8e-7]
  LstmGateMultilayerModel: predictions 2.3e-7 [1.5e-7], loss 1.3e-8 [1.3e-8], gradients 2.8e-7 [2.1e-7]
The floors (2e-6 / 5e-6) are the binding bound for nearly every quantity, and nothing comes nearer to its bound than a fifth of it (composed
dWv, 1.0e-6 of 5e-6).  Two bias gradients sit above 8 x their own float32 figure while far below the floor: dbs on bytes, 4.6e-7 [5.3e-8],
and dbf at H = 192, 1.2e-7 [2.3e-9] -- sums over F B rows of the two scalar gates' gradients, which torch on the CPU adds pairwise.
"""
import numpy as np
import pytest
import torch

import gate_lstm_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6


def _floor(name):
    return GRAD_FLOOR if name.startswith("d") else OUT_FLOOR


def _report(tag, got, ref64, ref32):
    """prints measured / float32-restatement errors per quantity, then asserts got within the bound"""
    bound = R.bounds(ref64, ref32, _floor)
    e = {k: R.err(got[k], ref64[k]) for k in ref64}
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % (k, e[k], R.err(ref32[k], ref64[k]), bound[k]) for k in ref64))
    for k in ref64:
        assert e[k] <= bound[k], (tag, k, e[k], bound[k])


def _lengths(B, F, shift):
    """num_frames holding 0, 1, F, F - 1 and a mid value (rotated by `shift`, so that short batches differ)"""
    pat = [0, 1, F, F - 1, F // 2]
    return np.array([pat[(b + shift) % 5] for b in range(B)], dtype=np.int32)


# ---- through the C ABI on given hoisted inputs: the two step kernels apart from the hoisted GEMMs ------------------------------------
ABI_CASES = [(3, 256, 5, 2, 0, 0), (5, 2048, 4, 16, 0, 0), (128, 1024, 6, 2, 64, 2), (4, 512, 3, 2, 0, 1)]
PAD = 7.25          # what the caller leaves in the padding columns of zs / dzs


@pytest.mark.parametrize("B,H,F,lds,ldu_extra,shift", ABI_CASES)
def test_step_kernels_match_fp64_through_the_c_abi(dev, monkeypatch, B, H, F, lds, ldu_extra, shift):
    """yt8m_gate_lstm_layer_fwd / _bwd at (B, H, F) = (3, 256, 5): one unit per thread, odd B; (5, 2048, 4): the widest supported, lds = 16;
    (128, 1024, 6): the plugins' shape, ldu = 2H + 64; (4, 512, 3): two units per thread.  o, g, i, f, every hs[t] and cs[t], c_last,
    dzv and dzs against fp64; with dout null, dzv and dzs are exactly zero at and past each row's num_frames; the padding columns of
    zs and dzs keep the caller's bits.
    Measured on an MI355X: see DESIGN_LOG.md "Scalar-gate LSTM"."""
    lib = L.lib()
    assert lib.yt8m_gate_lstm_supported(B, H)
    rs = np.random.RandomState(100 + H)
    nf = _lengths(B, F, shift)
    zv = (0.8 * rs.randn(F, B, 2 * H)).astype(np.float32)
    zs = (0.8 * rs.randn(F, B, 2) + [0.1, 1.0]).astype(np.float32)
    lim = np.sqrt(6.0 / (2 * H))
    Uv = ((rs.random_sample((H, 2 * H)) * 2 - 1) * lim).astype(np.float32)
    Us = ((rs.random_sample((2, H)) * 2 - 1) * lim).astype(np.float32)
    dout, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
    ref = {dt: R.recurrence_with_grads(zv, zs, Uv, Us, nf, dout, dc, dt) for dt in (torch.float64, torch.float32)}
    ldu = 2 * H + ldu_extra
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zv_d = d(zv)
    zs_d = torch.full((F, B, lds), PAD, device=dev)
    zs_d[:, :, :2] = d(zs)
    Uv_d = torch.full((H, ldu), 1.0e3, device=dev)                      # (a read of the padding columns would wreck every value)
    Uv_d[:, :2 * H] = d(Uv)
    Us_d, nf_d = d(Us), d(nf)
    hs = torch.full((F + 1, B, H), float("nan"), device=dev)
    cs = torch.full((F + 1, B, H), float("nan"), device=dev)
    hs[0].zero_()
    cs[0].zero_()
    c_last = torch.full((B, H), float("nan"), device=dev)
    ws = torch.empty(lib.yt8m_gemm_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    L.check(lib.yt8m_gate_lstm_layer_fwd(_p(zv_d), _p(zs_d), lds, _p(Uv_d), ldu, _p(Us_d), _p(hs), _p(cs), _p(c_last), _p(nf_d), F, B, H,
                                         _p(ws), ws.numel() * 4, _stream()))
    torch.cuda.synchronize()

    def backward(dout_d, dc_d, packed):
        monkeypatch.setenv("YT8M_GATE_LSTM_PACKED_BWD", packed)          # read by the library at every call
        dzv = torch.full((F, B, 2 * H), float("nan"), device=dev)
        dzs = torch.full((F, B, lds), PAD, device=dev)
        work = torch.full((4, B, H), float("nan"), device=dev)
        L.check(lib.yt8m_gate_lstm_layer_bwd(_p(zv_d), _p(zs_d), lds, _p(Uv_d), ldu, _p(Us_d), _p(hs), _p(cs), _p(dout_d), _p(dc_d), _p(dzv),
                                             _p(dzs), _p(work), _p(nf_d), F, B, H, _p(ws), ws.numel() * 4, _stream()))
        torch.cuda.synchronize()
        return dzv, dzs

    assert float(c_last[torch.from_numpy(nf < 1).to(dev)].abs().sum()) == 0.0             # rows with no frame: zeros
    ref0 = R.recurrence_with_grads(zv, zs, Uv, Us, nf, None, dc, torch.float64)
    past = torch.from_numpy(np.arange(F)[:, None] >= nf[None, :]).to(dev)                # [F, B]
    assert past.any()
    for packed in ("1", "0"):                    # dzv . [Uog|Uc]^T on the packed step launcher (the default) and as the grouped GEMM
        dzv, dzs = backward(d(dout), d(dc), packed)
        got = {"o": zv_d[:, :, :H], "g": zv_d[:, :, H:], "i": zs_d[:, :, 0], "f": zs_d[:, :, 1], "hs": hs, "cs": cs, "c_last": c_last,
               "dzv": dzv, "dzs": dzs[:, :, :2]}
        _report("gate LSTM C ABI B=%d H=%d F=%d lds=%d ldu=%d packed_bwd=%s:" % (B, H, F, lds, ldu, packed), got, ref[torch.float64],
                ref[torch.float32])
        if lds > 2:
            pad = torch.full((F, B, lds - 2), PAD, device=dev)
            assert torch.equal(zs_d[:, :, 2:].view(torch.int32), pad.view(torch.int32))
            assert torch.equal(dzs[:, :, 2:].view(torch.int32), pad.view(torch.int32))
        # only c_last carries a gradient: every step at or past a row's num_frames gets exactly zero, by the arithmetic alone
        dzv0, dzs0 = backward(None, d(dc), packed)
        assert float(dzv0[past].abs().sum()) == 0.0 and float(dzs0[:, :, :2][past].abs().sum()) == 0.0
        assert R.err(dzv0, ref0["dzv"]) <= GRAD_FLOOR and R.err(dzs0[:, :, :2], ref0["dzs"]) <= GRAD_FLOOR
        assert float(dzv0[~past].abs().max()) > 0.0


# ---- seq_ops.gate_lstm_layer at the plugins' width -----------------------------------------------------------------------------------
B_, H_ = 128, 1024
_REF = {}


def _layer_case(Din, F, u8):
    """inputs and both restatements of one op case, computed once and shared by the kernel and the composed run"""
    key = (Din, F, u8)
    if key not in _REF:
        from oracle import np_ref
        rs = np.random.RandomState(200 + Din)
        nf = rs.randint(0, F + 1, size=B_).astype(np.int32)
        nf[:5] = [0, 1, F, F - 1, F // 2]
        if u8:
            q = rs.randint(0, 256, size=(B_, F, Din)).astype(np.uint8)
            x = np.ascontiguousarray(np_ref.dequant_l2norm_folded(q, nf).transpose(1, 0, 2))       # [F,B,D] fp64, padding rows zero
        else:
            q = None
            x = rs.randn(F, B_, Din)
            x = x / np.linalg.norm(x, axis=2, keepdims=True)
            x = x * (np.arange(F)[:, None] < nf[None, :])[:, :, None]                             # padding frames are zero rows
        P = R.random_unit(rs, Din, H_)
        dout, dc = rs.randn(F, B_, H_).astype(np.float32), rs.randn(B_, H_).astype(np.float32)
        x32 = x.astype(np.float32)
        # the fp64 reference reads the float32 frames the float path is given; on bytes it reads the exact dequantised frames
        ref = {dt: R.layer_with_grads(x32 if not u8 else x, nf, P, dout, dc, dt) for dt in (torch.float64, torch.float32)}
        _REF[key] = (q, x32, nf, P, dout, dc, ref)
    return _REF[key]


@pytest.mark.parametrize("fused", [True, False], ids=["kernels", "composed"])
@pytest.mark.parametrize("Din,F,u8", [(64, 12, False), (1152, 8, True)], ids=["floats", "bytes"])
def test_gate_lstm_layer_at_h1024_matches_fp64(dev, monkeypatch, Din, F, u8, fused):
    """seq_ops.gate_lstm_layer at B = 128, H = 1024 on float frames (Din = 64, F = 12) and on the reader's bytes (Din = 1152, F = 8) with a
    gradient on out_tm AND on c_last: out_tm, c_last, dx (floats) and the gradient of every operand against fp64; on the step kernels
    (the shape is supported and the kernel path is taken) and with YT8M_GATE_LSTM_FUSED=0's composed form."""
    q, x32, nf, P, dout, dc, ref = _layer_case(Din, F, u8)
    assert L.lib().yt8m_gate_lstm_supported(B_, H_)
    monkeypatch.setattr(seq_ops, "GATE_LSTM_FUSED", fused)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nf_d = d(nf)
    if u8:
        qd = d(q)
        assert seq_ops.u8_hoisted_supported(qd), "the shape of this case must take the byte path"
        x_in = seq_ops.U8FrameImages(qd, nf_d)
    else:
        x_in = d(x32).requires_grad_(True)
    ops_ = [t.to(dev).contiguous().requires_grad_(True) for t in R.operands(R.to_torch(P, torch.float32))]
    before = dict(seq_ops.GATE_LSTM_CALLS)
    out, c_last = seq_ops.gate_lstm_layer(x_in, *ops_, nf_d)
    took = "kernels" if fused else "composed"
    assert seq_ops.GATE_LSTM_CALLS[took] == before[took] + 1 and sum(seq_ops.GATE_LSTM_CALLS.values()) == sum(before.values()) + 1
    ((out * d(dout)).sum() + (c_last * d(dc)).sum()).backward()
    torch.cuda.synchronize()
    names = ("dWv", "dbv", "dWs", "dbs", "dUv", "dUs")
    pack = lambda r: dict(zip(names, R.operands({n: r["d" + n] for n in R.NAMES})))
    r64, r32 = ({"out": r["out"], "c_last": r["c_last"], **({} if u8 else {"dx": r["dx"]}), **pack(r)} for r in (ref[torch.float64], ref[torch.float32]))
    got = {"out": out, "c_last": c_last, **({} if u8 else {"dx": x_in.grad}), **{n: t.grad for n, t in zip(names, ops_)}}
    _report("gate_lstm_layer H=1024 Din=%d F=%d %s %s:" % (Din, F, "bytes" if u8 else "floats", took), got, r64, r32)
    assert float(c_last[0].detach().abs().max()) == 0.0                  # num_frames = 0: zeros


def test_refused_shape_takes_the_composed_form(dev):
    """H = 192 is no multiple of 256: yt8m_gate_lstm_supported refuses it and the op computes the same function composed."""
    B, H, F, Din = 16, 192, 5, 64
    assert not L.lib().yt8m_gate_lstm_supported(B, H)
    rs = np.random.RandomState(31)
    nf = _lengths(B, F, 0)
    x = rs.randn(F, B, Din)
    x = (x / np.linalg.norm(x, axis=2, keepdims=True) * (np.arange(F)[:, None] < nf[None, :])[:, :, None]).astype(np.float32)
    P = R.random_unit(rs, Din, H)
    dout, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
    ref = {dt: R.layer_with_grads(x, nf, P, dout, dc, dt) for dt in (torch.float64, torch.float32)}
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = d(x).requires_grad_(True)
    Pt = {n: t.to(dev).requires_grad_(True) for n, t in R.to_torch(P, torch.float32).items()}
    before = dict(seq_ops.GATE_LSTM_CALLS)
    out, c_last = seq_ops.gate_lstm_layer(xt, *R.operands(Pt), d(nf))
    assert seq_ops.GATE_LSTM_CALLS["composed"] == before["composed"] + 1 and seq_ops.GATE_LSTM_CALLS["kernels"] == before["kernels"]
    ((out * d(dout)).sum() + (c_last * d(dc)).sum()).backward()
    got = {"out": out, "c_last": c_last, "dx": xt.grad, **{"d" + n: Pt[n].grad for n in R.NAMES}}
    _report("gate_lstm_layer H=192 composed:", got, ref[torch.float64], ref[torch.float32])


# ---- LstmGateMultilayerModel through TrainGraph ---------------------------------------------------------------------------------------
def test_multilayer_model_loss_and_every_gradient_match_fp64(dev, flags):
    """LstmGateMultilayerModel, 2 layers of 256 cells, B = 16, F = 6, D = 1152 on the reader's bytes, V = 32, 2 mixtures, through
    TrainGraph.forward / loss / backward: the loss and the gradient of every variable against the restatement followed by the MoE head and
    CrossEntropyLoss in fp64 (bound: eight times the same pipeline in float32, floors as above)."""
    from oracle import np_ref
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    B, F, D, H, V, M = 16, 6, 1152, 256, 32, 2
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures = str(H), 2, M
    rs = np.random.RandomState(41)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = _lengths(B, F, 1)
    y = rs.rand(B, V) < 0.2
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(flm.LstmGateMultilayerModel(), batch_size=B, graph=g)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    assert seq_ops.u8_hoisted_supported(args[0]) and L.lib().yt8m_gate_lstm_supported(B, H)
    tg.forward(*args)
    g.finalize()
    scopes = ["lstm_lsyer%dlstm_forward" % l for l in range(2)]
    assert [k for k in g.vars if k.startswith("lstm_")] == ["%s/%s" % (s, n) for s in scopes for n in R.NAMES]
    # a trained unit's scale instead of the initial values: the gates leave their linear range, the head sees both layers
    Pl = [R.random_unit(rs, D if l == 0 else H, H) for l in range(2)]
    head = {"gates/weights": 0.2 * rs.randn(2 * H, V * (M + 1)), "experts/weights": 0.2 * rs.randn(2 * H, V * M), "experts/biases": 0.2 * rs.randn(V * M)}
    vals = {"%s/%s" % (s, n): Pl[l][n] for l, s in enumerate(scopes) for n in R.NAMES}
    vals.update({k: v.astype(np.float32) for k, v in head.items()})
    assert set(vals) == set(g.vars)
    for k, v in vals.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    before = dict(seq_ops.GATE_LSTM_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    assert seq_ops.GATE_LSTM_CALLS["kernels"] == before["kernels"] + 2 and seq_ops.GATE_LSTM_CALLS["composed"] == before["composed"]
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf))

    def pipeline(dtype):
        tp = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in vals.items()}
        layers = [{n: tp["%s/%s" % (s, n)] for n in R.NAMES} for s in scopes]
        state = R.multilayer(x64.to(dtype), torch.from_numpy(nf), layers)
        p = R.moe(state, tp["gates/weights"], tp["experts/weights"], tp["experts/biases"], M)
        lr = R.cross_entropy(p, torch.from_numpy(y))
        lr.backward()
        out = {"predictions": p.detach().numpy(), "loss": np.array([float(lr.detach())])}
        out.update({"d:" + k: t.grad.numpy() for k, t in tp.items()})
        return out

    r64, r32 = pipeline(torch.float64), pipeline(torch.float32)
    got = {"predictions": res["predictions"], "loss": loss.detach().view(1)}
    got.update({"d:" + k: v.grad for k, v in g.vars.items()})
    _report("LstmGateMultilayerModel 2 x 256, bytes:", got, r64, r32)
    for k in vals:
        assert float(np.abs(r64["d:" + k]).max()) > 0.0, k                # every variable takes part
