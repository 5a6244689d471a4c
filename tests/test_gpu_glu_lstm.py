"""-m gpu: the input-memory LSTM layer (csrc/glu_lstm.hip, seq_ops.glu_lstm_layer) and LstmGlu2MultilayerModel against the fp64
restatement (tests/glu_lstm_restatement.py), which is in the reference's form: it multiplies l2_normalize(x_prev) by V* at every step,
where the kernels carry x_prev.V* as a state.

Bounds.  The measure is tests/test_gpu_gate_lstm.py's: max |got - ref| / max(1, max |ref|) against fp64.  Per quantity the bound is EIGHT
times the error of the float32 restatement (plain torch on the CPU, same inputs, the reference's form) against the float64 one, never
below that file's floors: 2e-6 for outputs and states, 5e-6 for gradients.  The margin covers a different but correct summation order
(the carried projections against a product per step, the K-split of the products, the 2^-21 per-term error of the three-f16-product
hoisted forms, ~1.5e-7 per value of the v_exp / v_rcp gate functions); on the CPU the carried form needs at most 4 x.
Quantities with a batch axis are held to the bound TWICE: over the whole tensor (the measure above) and row by row, each row against
eight times the float32 restatement's error in that row.  The second is the sharper one: behind a video's end the input memory decays,
r = rsqrt(max(sum x_prev^2, 1e-12)) grows to 1e6, and the gradients with respect to x.V* of those frames -- 1e6 times the others' --
would otherwise set the scale every other row is measured on.
Every test prints the measured errors and the float32 restatement's.  Measured values: DESIGN_LOG.md section 32.
"""
import numpy as np
import pytest
import torch

import glu_lstm_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
BATCH_AXIS = {"c_last": 0, "out": 1, "dx": 1, "o": 1, "g": 1, "s": 1, "hs": 1, "cs": 1, "xm": 1, "n2": 1, "qv": 1, "qs": 1, "dzv": 1,
              "dpv": 1, "dzs": 1, "dps": 1, "dx_direct": 1}


def _floor(name):
    return GRAD_FLOOR if name.startswith("d") else OUT_FLOOR


def _np(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


def _row_errs(got, ref, axis):
    """the measure row by row: [B] errors of `got` against `ref` along the batch axis"""
    g, r = (np.moveaxis(_np(a), axis, 0) for a in (got, ref))
    g, r = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
    return np.abs(g - r).max(1) / np.maximum(1.0, np.abs(r).max(1))


def _report(tag, got, ref64, ref32):
    """prints measured / float32-restatement errors per quantity, then asserts got within the bound: over the whole tensor and, where
    the quantity has a batch axis, row by row"""
    bound = R.bounds(ref64, ref32, _floor)
    e = {k: R.err(got[k], ref64[k]) for k in ref64}
    rows = {}
    for k in ref64:
        if k in BATCH_AXIS:
            eb, fb = _row_errs(got[k], ref64[k], BATCH_AXIS[k]), _row_errs(ref32[k], ref64[k], BATCH_AXIS[k])
            rows[k] = (eb, np.maximum(8.0 * fb, _floor(k)))
    worst = {k: float((eb / bb).max()) for k, (eb, bb) in rows.items()}
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g%s)" % (k, e[k], R.err(ref32[k], ref64[k]), bound[k],
                                                                ", worst row at %.2g of its bound" % worst[k] if k in worst else "")
                        for k in ref64))
    for k in ref64:
        assert np.isfinite(_np(got[k])).all(), (tag, k)
        assert e[k] <= bound[k], (tag, k, e[k], bound[k])
        if k in rows:
            eb, bb = rows[k]
            assert (eb <= bb).all(), (tag, k, "row", int(np.argmax(eb / bb)), float((eb / bb).max()))


def _lengths(B, F, shift):
    """num_frames holding 0, 1, F, F - 1 and a mid value (rotated by `shift`, so that short batches differ)"""
    pat = [0, 1, F, F - 1, F // 2]
    return np.array([pat[(b + shift) % 5] for b in range(B)], dtype=np.int32)


def _float_frames(rs, F, B, D, nf):
    """l2-normalised frames [F,B,D] as float32-valued fp64, zero rows behind each video's end"""
    x = rs.randn(F, B, D)
    x = x / np.linalg.norm(x, axis=2, keepdims=True) * (np.arange(F)[:, None] < nf[None, :])[:, :, None]
    return x.astype(np.float32).astype(np.float64)


# ---- through the C ABI: the two step kernels apart from the hoisted GEMMs -----------------------------------------------------------
PAD = 7.25          # what the caller leaves in the padding columns of zs / dzs


def _run_abi_case(dev, monkeypatch, B, H, F, D, lds, ldu_extra, shift, u8, windows, nf=None):
    """One case of yt8m_glu_lstm_layer_fwd / _bwd against the restatement.  The hoisted products are made here in fp64 and rounded to
    float32.  windows: zv | pv and dzv | dpv are column windows of one [F,B,4H] tensor (ldv = lddv = 4H), else matrices of their own."""
    from oracle import np_ref
    lib = L.lib()
    assert lib.yt8m_glu_lstm_supported(B, H, D)
    rs = np.random.RandomState(100 + H + F)
    nf = _lengths(B, F, shift) if nf is None else np.asarray(nf, dtype=np.int32)
    d = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)
    if u8:
        q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
        x = np.ascontiguousarray(np_ref.dequant_l2norm_folded(q, nf).transpose(1, 0, 2))            # [F,B,D] fp64, padding rows zero
        q_d = d(q, np.uint8)
        xr_d = seq_ops.u8_frame_scales(q_d, d(nf, np.int32)).t().contiguous()                      # [F,B]
        x_d = None
    else:
        x = _float_frames(rs, F, B, D, nf)
        q_d = xr_d = None
        x_d = d(x)
    P = R.random_unit(rs, D, H)
    Wv, bv, Ws, bs, Vv, Vs, Uv, Us = R.operands({n: a.astype(np.float64) for n, a in P.items()})
    dout, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
    ref = {dt: R.recurrence_with_grads(x, P, nf, dout, dc, dt) for dt in (torch.float64, torch.float32)}
    ref0 = R.recurrence_with_grads(x, P, nf, None, dc, torch.float64)
    past = np.arange(F)[:, None] >= nf[None, :]                                                    # [F,B]
    assert past.any() and (~past).any()
    if u8:                                          # the byte path's contract: dpv / dps of a padding frame are written as zeros
        for r in (ref[torch.float64], ref[torch.float32], ref0):
            r["dpv"], r["dps"] = r["dpv"] * ~past[:, :, None], r["dps"] * ~past[:, :, None]
            del r["dx_direct"]                                                                    # the frames are data
    ldv = 4 * H if windows else 2 * H
    ldu = 2 * H + ldu_extra
    zvp = torch.full((F, B, 4 * H), float("nan"), device=dev)
    if windows:
        zv_d, pv_d = zvp[:, :, :2 * H], zvp[:, :, 2 * H:]
    else:
        zv_d, pv_d = torch.empty((F, B, 2 * H), device=dev), torch.empty((F, B, 2 * H), device=dev)
    zv_d.copy_(d(x @ Wv + bv))
    pv_d.copy_(d(x @ Vv))
    zs_d = torch.full((F, B, lds), PAD, device=dev)
    zs_d[:, :, :8] = d(np.concatenate([x @ Ws + bs, x @ Vs], axis=2))
    ps_in = zs_d[:, :, 4:8].clone()
    pv_in = pv_d.clone()
    Uv_d = torch.full((H, ldu), 1.0e3, device=dev)                      # (a read of the padding columns would wreck every value)
    Uv_d[:, :2 * H] = d(Uv)
    Us_d, nf_d = d(Us), d(nf, np.int32)
    tape = lambda *shape: torch.full((F + 1,) + shape, float("nan"), device=dev)
    hs, cs, qv, qs, xm, n2 = tape(B, H), tape(B, H), tape(B, 2 * H), tape(B, 4), tape(B, D), tape(B)
    for t_ in (hs, cs, qv, qs, xm, n2):
        t_[0].zero_()
    c_last = torch.full((B, H), float("nan"), device=dev)
    ws = torch.empty(lib.yt8m_gemm_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    L.check(lib.yt8m_glu_lstm_layer_fwd(_p(zv_d), _p(pv_d), ldv, _p(zs_d), lds, _p(Uv_d), ldu, _p(Us_d), _p(x_d), _p(q_d), _p(xr_d), _p(hs),
                                        _p(cs), _p(qv), _p(qs), _p(xm), _p(n2), _p(c_last), _p(nf_d), F, B, H, D, _p(ws), ws.numel() * 4,
                                        _stream()))
    torch.cuda.synchronize()
    assert float(c_last[torch.from_numpy(nf < 1).to(dev)].abs().sum()) == 0.0             # rows with no frame: zeros
    assert torch.equal(pv_d, pv_in) and torch.equal(zs_d[:, :, 4:8], ps_in)               # x.V* is read only
    fwd = {"o": zv_d[:, :, :H], "g": zv_d[:, :, H:], "s": zs_d[:, :, :4], "hs": hs, "cs": cs, "xm": xm, "n2": n2, "qv": qv, "qs": qs,
           "c_last": c_last}

    def backward(dout_d, dc_d, packed):
        monkeypatch.setenv("YT8M_GLU_LSTM_PACKED_BWD", packed)           # read by the library at every call
        dv4 = torch.full((F, B, 4 * H), float("nan"), device=dev)
        if windows:
            dzv, dpv = dv4[:, :, :2 * H], dv4[:, :, 2 * H:]
        else:
            dzv, dpv = torch.full((F, B, 2 * H), float("nan"), device=dev), torch.full((F, B, 2 * H), float("nan"), device=dev)
        dzs = torch.full((F, B, lds), PAD, device=dev)
        dxd = None if u8 else torch.full((F, B, D), float("nan"), device=dev)
        work = torch.full((B * (8 * H + D + 8),), float("nan"), device=dev)
        L.check(lib.yt8m_glu_lstm_layer_bwd(_p(zv_d), _p(pv_d), ldv, _p(zs_d), lds, _p(Uv_d), ldu, _p(Us_d), _p(x_d), _p(q_d), _p(xr_d),
                                            _p(hs), _p(cs), _p(qv), _p(qs), _p(xm), _p(n2), _p(dout_d), _p(dc_d), _p(dzv), _p(dpv), ldv,
                                            _p(dzs), _p(dxd), _p(work), _p(nf_d), F, B, H, D, _p(ws), ws.numel() * 4, _stream()))
        torch.cuda.synchronize()
        out = {"dzv": dzv, "dpv": dpv, "dzs": dzs[:, :, :4], "dps": dzs[:, :, 4:8]}
        if not u8:
            out["dx_direct"] = dxd
        return out, dzs

    past_d = torch.from_numpy(past).to(dev)
    for packed in ("1", "0"):                    # dzv . [Uog|Uc]^T on the packed step launcher (the default) and as the grouped GEMM
        grads, dzs = backward(d(dout), d(dc), packed)
        _report("glu LSTM C ABI B=%d H=%d F=%d D=%d lds=%d ldv=%d ldu=%d %s packed_bwd=%s:" % (B, H, F, D, lds, ldv, ldu,
                                                                                                 "bytes" if u8 else "floats", packed),
                {**fwd, **grads}, ref[torch.float64], ref[torch.float32])
        if lds > 8:
            pad = torch.full((F, B, lds - 8), PAD, device=dev)
            assert torch.equal(zs_d[:, :, 8:].view(torch.int32), pad.view(torch.int32))
            assert torch.equal(dzs[:, :, 8:].view(torch.int32), pad.view(torch.int32))
        # only c_last carries a gradient: every step at or past a row's num_frames gets exactly zero, by the arithmetic alone
        g0, _ = backward(None, d(dc), packed)
        for k, v in g0.items():
            assert float(v[past_d].abs().sum()) == 0.0, k
            assert (_row_errs(v, ref0[k], 1) <= GRAD_FLOOR).all(), k
        assert float(g0["dzv"][~past_d].abs().max()) > 0.0 and float(g0["dpv"][~past_d].abs().max()) > 0.0
    return nf, fwd, grads, ref[torch.float64]


ABI_CASES = [(3, 256, 5, 64, 8, 0, 0, False, False), (5, 2048, 4, 1152, 16, 0, 0, True, True), (128, 1024, 6, 1024, 8, 64, 2, False, True),
             (4, 512, 3, 64, 8, 0, 1, False, False)]


@pytest.mark.parametrize("B,H,F,D,lds,ldu_extra,shift,u8,windows", ABI_CASES)
def test_step_kernels_match_fp64_through_the_c_abi(dev, monkeypatch, B, H, F, D, lds, ldu_extra, shift, u8, windows):
    """yt8m_glu_lstm_layer_fwd / _bwd at (B, H, F, D, lds) = (3, 256, 5, 64, 8): one unit per thread, odd B, float frames, zv and pv
    matrices of their own; (5, 2048, 4, 1152, 16): the widest supported, the reader's bytes, two passes of the loop over D, padding
    columns in zs / dzs, windows of one 4H-wide tensor; (128, 1024, 6, 1024, 8): the plugins' shape, ldu = 2H + 64;
    (4, 512, 3, 64, 8): two units per thread.  Lengths mix F,
    F - 1, F / 2, 1 and 0.  Every tape (o, g, the four scalar gates, hs, cs, xm, n2, qv, qs), c_last and every emitted gradient block
    (dzv, dpv, dzs, dps, dx_direct on float frames) against fp64; with dout null, every emitted gradient is exactly zero at and past
    each row's num_frames; the padding columns keep the caller's bits; x.V* is read only."""
    _run_abi_case(dev, monkeypatch, B, H, F, D, lds, ldu_extra, shift, u8, windows)


def test_three_hundred_steps_keep_the_carried_projections(dev, monkeypatch):
    """(B, H, F, D) = (4, 256, 300, 64), lengths 300, 299, 1, 0: qv, qs and n2 accumulated over the workload's step count against
    x_prev.V* and sum x_prev^2 taken afresh at every step in fp64.  The row of length 1 runs 299 steps on zero frames: its input memory
    decays below the l2-normalisation's epsilon (the 1e-12 branch with x_prev != 0: r stays 1e6 and dn2 is zero from there on)."""
    nf, fwd, grads, ref = _run_abi_case(dev, monkeypatch, 4, 256, 300, 64, 8, 0, 0, False, True, nf=[300, 299, 1, 0])
    n2 = ref["n2"][:, 2]
    assert (n2[1:] > 0).all() and n2[1] > 1e-3 and n2[-1] < 1e-12                        # ... and that row does cross the epsilon
    assert float(np.abs(ref["dpv"][:, 2]).max()) > 1e3                                    # where the gradients w.r.t. x.V* grow like r


def test_row_without_frames_takes_the_epsilon_branch(dev, monkeypatch):
    """A row with num_frames = 0 has all-zero frames: n2 = 0 at every step, r = 1e6 (the 1e-12 branch), x_prev.V* = 0.  Its values are
    finite and match (the test above holds them to the bound row by row; here: the row alone), its input memory, carried projections
    and dx_direct are exactly zero -- dn2 is zero in that branch, and nothing else reaches dxm --, and dpv is of the order of r."""
    B, H, F, D = 3, 256, 5, 64
    nf, fwd, grads, ref = _run_abi_case(dev, monkeypatch, B, H, F, D, 8, 0, 0, False, True, nf=[0, F, 0])
    for b in (0, 2):
        for k in ("xm", "n2", "qv", "qs"):
            assert float(fwd[k][:, b].abs().max()) == 0.0, k
        assert float(fwd["c_last"][b].abs().max()) == 0.0
        assert float(grads["dx_direct"][:, b].abs().max()) == 0.0
        for k, v in {**fwd, **grads}.items():
            row = v[b] if k == "c_last" else v[:, b]
            assert bool(torch.isfinite(row).all()), k
        assert float(grads["dpv"][:, b].abs().max()) > 1e3
        assert float(fwd["hs"][1:, b].abs().max()) > 0.0                 # the row still runs: biases and recurrent weights


# ---- seq_ops.glu_lstm_layer at the plugins' width -----------------------------------------------------------------------------------
B_, H_ = 128, 1024
_REF = {}
OP_NAMES = ("dWv", "dbv", "dWs", "dbs", "dVv", "dVs", "dUv", "dUs")


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
            x = _float_frames(rs, F, B_, Din, nf)
        P = R.random_unit(rs, Din, H_)
        dout, dc = rs.randn(F, B_, H_).astype(np.float32), rs.randn(B_, H_).astype(np.float32)
        pack = lambda r: dict(zip(OP_NAMES, R.operands({n: r["d" + n] for n in R.NAMES})))
        ref = {}
        for dt in (torch.float64, torch.float32):
            r = R.layer_with_grads(x, nf, P, dout, dc, dt)
            ref[dt] = {"out": r["out"], "c_last": r["c_last"], **({} if u8 else {"dx": r["dx"]}), **pack(r)}
        _REF[key] = (q, x.astype(np.float32), nf, P, dout, dc, ref)
    return _REF[key]


@pytest.mark.parametrize("fused", [True, False], ids=["kernels", "composed"])
@pytest.mark.parametrize("Din,F,u8", [(64, 12, False), (1152, 8, True)], ids=["floats", "bytes"])
def test_glu_lstm_layer_at_h1024_matches_fp64(dev, monkeypatch, Din, F, u8, fused):
    """seq_ops.glu_lstm_layer at B = 128, H = 1024 on float frames (Din = 64, F = 12) and on the reader's bytes (Din = 1152, F = 8) with a
    gradient on out_tm AND on c_last: out_tm, c_last, dx (floats) and the gradient of every operand against fp64; on the step kernels
    (the shape is supported and the kernel path is taken) and with YT8M_GLU_LSTM_FUSED=0's composed form."""
    q, x32, nf, P, dout, dc, ref = _layer_case(Din, F, u8)
    assert L.lib().yt8m_glu_lstm_supported(B_, H_, Din)
    monkeypatch.setattr(seq_ops, "GLU_LSTM_FUSED", fused)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nf_d = d(nf)
    if u8:
        qd = d(q)
        assert seq_ops.u8_hoisted_supported(qd), "the shape of this case must take the byte path"
        x_in = seq_ops.U8FrameImages(qd, nf_d)
    else:
        x_in = d(x32).requires_grad_(True)
    ops_ = [t.to(dev).contiguous().requires_grad_(True) for t in R.operands(R.to_torch(P, torch.float32))]
    before = dict(seq_ops.GLU_LSTM_CALLS)
    out, c_last = seq_ops.glu_lstm_layer(x_in, *ops_, nf_d)
    took = "kernels" if fused else "composed"
    assert seq_ops.GLU_LSTM_CALLS[took] == before[took] + 1 and sum(seq_ops.GLU_LSTM_CALLS.values()) == sum(before.values()) + 1
    ((out * d(dout)).sum() + (c_last * d(dc)).sum()).backward()
    torch.cuda.synchronize()
    names = ("dWv", "dbv", "dWs", "dbs", "dVv", "dVs", "dUv", "dUs")
    got = {"out": out, "c_last": c_last, **({} if u8 else {"dx": x_in.grad}), **{n: t.grad for n, t in zip(names, ops_)}}
    _report("glu_lstm_layer H=1024 Din=%d F=%d %s %s:" % (Din, F, "bytes" if u8 else "floats", took), got, ref[torch.float64], ref[torch.float32])
    assert float(c_last[0].detach().abs().max()) == 0.0                  # num_frames = 0: zeros


def test_refused_shape_takes_the_composed_form(dev):
    """H = 192 is no multiple of 256: yt8m_glu_lstm_supported refuses it and the op computes the same function composed."""
    B, H, F, Din = 16, 192, 5, 64
    assert not L.lib().yt8m_glu_lstm_supported(B, H, Din)
    rs = np.random.RandomState(31)
    nf = _lengths(B, F, 0)
    x = _float_frames(rs, F, B, Din, nf)
    P = R.random_unit(rs, Din, H)
    dout, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
    ref = {dt: R.layer_with_grads(x, nf, P, dout, dc, dt) for dt in (torch.float64, torch.float32)}
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = d(x.astype(np.float32)).requires_grad_(True)
    Pt = {n: t.to(dev).requires_grad_(True) for n, t in R.to_torch(P, torch.float32).items()}
    before = dict(seq_ops.GLU_LSTM_CALLS)
    out, c_last = seq_ops.glu_lstm_layer(xt, *R.operands(Pt), d(nf))
    assert seq_ops.GLU_LSTM_CALLS["composed"] == before["composed"] + 1 and seq_ops.GLU_LSTM_CALLS["kernels"] == before["kernels"]
    ((out * d(dout)).sum() + (c_last * d(dc)).sum()).backward()
    got = {"out": out, "c_last": c_last, "dx": xt.grad, **{"d" + n: Pt[n].grad for n in R.NAMES}}
    _report("glu_lstm_layer H=192 composed:", got, ref[torch.float64], ref[torch.float32])


# ---- LstmGlu2MultilayerModel through TrainGraph ---------------------------------------------------------------------------------------
def test_multilayer_model_loss_and_every_gradient_match_fp64(dev, flags):
    """LstmGlu2MultilayerModel, 2 layers of 256 cells, B = 16, F = 6, D = 1152 on the reader's bytes, V = 32, 2 mixtures, through
    TrainGraph.forward / loss / backward: the loss and the gradient of all 51 variables against the restatement followed by the MoE head
    and CrossEntropyLoss in fp64 (bound: eight times the same pipeline in float32, floors as above)."""
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
    tg = train.TrainGraph(flm.LstmGlu2MultilayerModel(), batch_size=B, graph=g)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    assert seq_ops.u8_hoisted_supported(args[0]) and L.lib().yt8m_glu_lstm_supported(B, H, D) and L.lib().yt8m_glu_lstm_supported(B, H, H)
    tg.forward(*args)
    g.finalize()
    scopes = ["lstm_lsyer%dlstm_forward" % l for l in range(2)]
    assert [k for k in g.vars if k.startswith("lstm_")] == ["%s/%s" % (s, n) for s in scopes for n in R.NAMES]
    assert len(g.vars) == 51
    # a trained unit's scale instead of the initial values: the gates leave their linear range, the head sees both layers
    Pl = [R.random_unit(rs, D if l == 0 else H, H) for l in range(2)]
    head = {"gates/weights": 0.2 * rs.randn(2 * H, V * (M + 1)), "experts/weights": 0.2 * rs.randn(2 * H, V * M), "experts/biases": 0.2 * rs.randn(V * M)}
    vals = {"%s/%s" % (s, n): Pl[l][n] for l, s in enumerate(scopes) for n in R.NAMES}
    vals.update({k: v.astype(np.float32) for k, v in head.items()})
    assert set(vals) == set(g.vars)
    for k, v in vals.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    monkey_before = dict(seq_ops.GLU_LSTM_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    took = "kernels" if seq_ops.GLU_LSTM_FUSED else "composed"           # the default form, whichever the measurements made it
    assert seq_ops.GLU_LSTM_CALLS[took] == monkey_before[took] + 2 and sum(seq_ops.GLU_LSTM_CALLS.values()) == sum(monkey_before.values()) + 2
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
    _report("LstmGlu2MultilayerModel 2 x 256, bytes (%s):" % took, got, r64, r32)
    for k in vals:
        assert float(np.abs(r64["d:" + k]).max()) > 0.0, k                # every variable takes part
