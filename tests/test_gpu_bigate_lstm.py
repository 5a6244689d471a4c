"""-m gpu: the frame-order scalar-gate recurrence (csrc/gate_cell.hip), seq_ops.bigate_lstm_layer in its three forms and
LstmBigluModel against the fp64 restatement (tests/bigate_lstm_restatement.py), which makes the reference's reverse_sequence copies.

Bounds.  As tests/test_gpu_gate_lstm.py: the measure is max |got - ref| / max(1, max |ref|); per quantity the bound is EIGHT times the
error of the float32 restatement (plain torch on the CPU, same inputs) against the float64 one, never below what
tests/test_gpu_recurrent_fp64.py holds a layer to at this width: 2e-6 for outputs and states, 5e-6 for gradients.  Every test prints the
measured errors and the float32 restatement's.

Measured on an MI355X (largest error per group, the float32 restatement's error of the same quantity in brackets):
  C ABI, identity row map / r(i, b), the three window layouts and either backward product form alike to the digit shown:
    (3, 256, 5): outputs and states 2.5e-7 / 2.8e-7 (g) [3.6e-7 / 3.2e-7], dzv and dzs 2.2e-7 / 2.5e-7 [1.7e-7 / 1.4e-7]
    (4, 512, 3): 2.7e-7 / 2.7e-7 [1.5e-7 / 3.2e-7], gradients 1.7e-7 / 2.0e-7 [1.2e-7 / 1.3e-7]
    (128, 1024, 6): 3.5e-7 / 3.2e-7 [3.1e-7 / 3.2e-7], gradients 2.3e-7 / 2.1e-7 [1.4e-7 / 1.5e-7]
    (5, 2048, 4): 2.7e-7 / 2.6e-7 [9.8e-7 / 9.9e-7], gradients 2.6e-7 / 2.7e-7 [1.8e-7 / 1.4e-7]
    (3, 256, 5) with num_frames -1, F + 2, 2: 2.4e-7 (g) [3.4e-7], gradients 5.9e-7 (dzs) [3.1e-7]; equal to the bit to the step-order run over
      copies made by yt8m_reverse_sequence_f32_tm
  bigate_lstm_layer at H = 1024, floats: frame order and reversed copies c1_last 2.3e-7 [1.5e-7], gradients 1.2e-6 (dUs2) [1.2e-6];
    composed c1_last 3.5e-7, dUs2 1.4e-6
  bytes: frame order c2_last 1.9e-7 [1.0e-7], gradients 1.9e-6 (dUs1) [1.5e-6, bound 1.2e-5]; reversed copies c2_last 1.9e-7, dUs1 3.5e-6;
    composed c2_last 2.6e-7, dUs1 1.5e-6
  frame order against reversed copies: floats y, out2, c1_last, c2_last and the pass-2 gradients equal to the bit, pass-1 gradients
    2.1e-7 - 3.2e-7; bytes outputs 1.4e-7 - 2.1e-7, gradients up to 2.6e-6 (dUs1, bound 1.2e-5), the next 9.8e-7 (dUs2)
  H = 192 composed: c2_last 6.1e-8 [7.2e-8], gradients 8.1e-7 (dfw/bi) [8.0e-7]
  LstmBigluModel: predictions 1.1e-7 [1.3e-7], loss 5.5e-8 [4.6e-8], gradients 1.9e-7 (lstm_forward/bc) [1.4e-7]
The floors (2e-6 / 5e-6) are the binding bound for nearly every quantity; nothing comes nearer to its bound than 0.3 of it (dUs1 on bytes
over reversed copies, 3.5e-6 of 1.2e-5: a sum over F B rows of a two-column gradient against h, its float32 figure already 1.5e-6).
"""
import numpy as np
import pytest
import torch

import bigate_lstm_restatement as R
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


# ---- through the C ABI on given hoisted inputs, in frame order ------------------------------------------------------------------------
ABI_SHAPES = [(3, 256, 5, 0), (4, 512, 3, 0), (128, 1024, 6, 64), (5, 2048, 4, 0)]            # B, H, F, ldu - 2H
LAYOUTS = {"ldz2H": (2, 0), "ldz4H_left": (4, 0), "ldz4H_right": (4, 1)}                       # ldz / H, which half of the joint buffer
LDS = 4
PAD = 7.25           # what the caller leaves in the columns outside the pass's window
_ABI_REF = {}


def _abi_case(B, H, F, reverse, shift):
    """inputs and both restatements of one (shape, reverse): computed once, shared by the three layouts"""
    key = (B, H, F, reverse)
    if key not in _ABI_REF:
        rs = np.random.RandomState(100 + H + reverse)
        nf = _lengths(B, F, shift)
        zv = (0.8 * rs.randn(F, B, 2 * H)).astype(np.float32)
        zs = (0.8 * rs.randn(F, B, 2) + 0.1).astype(np.float32)
        lim = np.sqrt(6.0 / (2 * H))
        Uv = ((rs.random_sample((H, 2 * H)) * 2 - 1) * lim).astype(np.float32)
        Us = ((rs.random_sample((2, H)) * 2 - 1) * lim).astype(np.float32)
        dy, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
        ref = {dt: R.recurrence_with_grads(zv, zs, Uv, Us, nf, reverse, dy, dc, dt) for dt in (torch.float64, torch.float32)}
        ref0 = R.recurrence_with_grads(zv, zs, Uv, Us, nf, reverse, None, dc, torch.float64)
        _ABI_REF[key] = (nf, zv, zs, Uv, Us, dy, dc, ref, ref0)
    return _ABI_REF[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("B,H,F,ldu_extra", ABI_SHAPES)
def test_frame_order_kernels_match_fp64_through_the_c_abi(dev, monkeypatch, B, H, F, ldu_extra, reverse, layout):
    """yt8m_gate_lstm_frames_fwd / _bwd at (B, H, F) = (3, 256, 5): one unit per thread, odd B; (4, 512, 3): two; (128, 1024, 6): four,
    the plugin's width, ldu = 2H + 64; (5, 2048, 4): eight.  Each with the identity row map and with r(i, b), on a buffer of its own
    (ldz = 2H) and on either half of a joint [F, B, 4H] buffer with the matching column pair of a four-column zs.  In frame order against
    fp64: o, g, i, f in place, y, hprev, c_last, dzv, dzs; cs in step order.  y, hprev and the window of dzv / dzs start as NaN and end
    finite: every row is written.  The columns outside the window keep the caller's bits.  With dy null, dzv and dzs are exactly zero
    at every frame at or past a row's num_frames and non-zero before it.  Both forms of the backward product; a second call from the
    same inputs gives the same bits."""
    lib = L.lib()
    assert lib.yt8m_gate_lstm_frames_supported(B, H)
    shift = ABI_SHAPES.index((B, H, F, ldu_extra)) + reverse
    nf, zv, zs, Uv, Us, dy, dc, ref, ref0 = _abi_case(B, H, F, reverse, shift)
    wide, half = LAYOUTS[layout]
    ldz, c0, s0 = wide * H, half * 2 * H, half * 2
    ldu = 2 * H + ldu_extra
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Uv_d = torch.full((H, ldu), 1.0e3, device=dev)                      # (a read of the padding columns would wreck every value)
    Uv_d[:, :2 * H] = d(Uv)
    Us_d, nf_d = d(Us), d(nf)
    ws = torch.empty(lib.yt8m_gemm_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    nan = float("nan")

    def window(buf, col, width):
        return buf[:, :, col:col + width]

    def forward():
        zv_d, zs_d = torch.full((F, B, ldz), PAD, device=dev), torch.full((F, B, LDS), PAD, device=dev)
        window(zv_d, c0, 2 * H).copy_(d(zv))
        window(zs_d, s0, 2).copy_(d(zs))
        y, hprev = torch.full((F, B, H), nan, device=dev), torch.full((F, B, H), nan, device=dev)
        cs = torch.full((F + 1, B, H), nan, device=dev)
        cs[0].zero_()
        c_last, work = torch.full((B, H), nan, device=dev), torch.full((4, B, H), nan, device=dev)
        L.check(lib.yt8m_gate_lstm_frames_fwd(_p(window(zv_d, c0, 2 * H)), ldz, _p(window(zs_d, s0, 2)), LDS, _p(Uv_d), ldu, _p(Us_d), _p(y),
                                              _p(hprev), _p(cs), _p(c_last), _p(work), _p(nf_d), reverse, F, B, H, _p(ws), ws.numel() * 4,
                                              _stream()))
        torch.cuda.synchronize()
        return zv_d, zs_d, y, hprev, cs, c_last

    def backward(fw, dy_d, dc_d, packed):
        monkeypatch.setenv("YT8M_GATE_LSTM_PACKED_BWD", packed)          # read by the library at every call
        zv_d, zs_d, _, _, cs, _ = fw
        dzv, dzs = torch.full((F, B, ldz), PAD, device=dev), torch.full((F, B, LDS), PAD, device=dev)
        window(dzv, c0, 2 * H).fill_(nan)
        window(dzs, s0, 2).fill_(nan)
        work = torch.full((6, B, H), nan, device=dev)
        L.check(lib.yt8m_gate_lstm_frames_bwd(_p(window(zv_d, c0, 2 * H)), ldz, _p(window(zs_d, s0, 2)), LDS, _p(Uv_d), ldu, _p(Us_d), _p(cs),
                                              _p(dy_d), _p(dc_d), _p(window(dzv, c0, 2 * H)), ldz, _p(window(dzs, s0, 2)), LDS, _p(work),
                                              _p(nf_d), reverse, F, B, H, _p(ws), ws.numel() * 4, _stream()))
        torch.cuda.synchronize()
        return dzv, dzs

    def outside_keeps_pad(buf, col, width):
        mask = torch.ones(buf.shape[2], dtype=torch.bool, device=dev)
        mask[col:col + width] = False
        rest = buf[:, :, mask]
        return torch.equal(rest.contiguous().view(torch.int32), torch.full_like(rest, PAD).view(torch.int32))

    bits = lambda ts: [t.contiguous().view(torch.int32) for t in ts]
    fw = forward()
    zv_d, zs_d, y, hprev, cs, c_last = fw
    assert all(torch.equal(a, b) for a, b in zip(bits(fw), bits(forward())))                         # a rerun: the same bits
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(hprev).all()) and bool(torch.isfinite(cs).all())
    assert outside_keeps_pad(zv_d, c0, 2 * H) and outside_keeps_pad(zs_d, s0, 2)
    assert float(c_last[torch.from_numpy(nf < 1).to(dev)].abs().sum()) == 0.0                        # rows with no frame: zeros
    past = torch.from_numpy(np.arange(F)[:, None] >= nf[None, :]).to(dev)                           # [F, B], by FRAME
    assert past.any() and (~past).any()
    zvw, zsw = window(zv_d, c0, 2 * H), window(zs_d, s0, 2)
    for packed in ("1", "0"):                    # dzc . [Uog|Uc]^T on the packed step launcher (the default) and as the grouped GEMM
        dzv, dzs = backward(fw, d(dy), d(dc), packed)
        assert all(torch.equal(a, b) for a, b in zip(bits((dzv, dzs)), bits(backward(fw, d(dy), d(dc), packed))))
        assert outside_keeps_pad(dzv, c0, 2 * H) and outside_keeps_pad(dzs, s0, 2)
        dzvw, dzsw = window(dzv, c0, 2 * H), window(dzs, s0, 2)
        assert bool(torch.isfinite(dzvw).all()) and bool(torch.isfinite(dzsw).all())
        got = {"o": zvw[:, :, :H], "g": zvw[:, :, H:], "i": zsw[:, :, 0], "f": zsw[:, :, 1], "y": y, "hprev": hprev, "cs": cs, "c_last": c_last,
               "dzv": dzvw, "dzs": dzsw}
        _report("gate LSTM frames C ABI B=%d H=%d F=%d reverse=%d %s ldu=%d packed_bwd=%s:" % (B, H, F, reverse, layout, ldu, packed), got,
                ref[torch.float64], ref[torch.float32])
        # only c_last carries a gradient: every frame at or past a row's num_frames gets exactly zero, by the arithmetic alone
        dzv0, dzs0 = backward(fw, None, d(dc), packed)
        dzv0, dzs0 = window(dzv0, c0, 2 * H), window(dzs0, s0, 2)
        assert float(dzv0[past].abs().sum()) == 0.0 and float(dzs0[past].abs().sum()) == 0.0
        assert R.err(dzv0, ref0["dzv"]) <= GRAD_FLOOR and R.err(dzs0, ref0["dzs"]) <= GRAD_FLOOR
        assert bool((dzv0[~past].abs().sum(dim=1) > 0.0).all()) and bool((dzs0[~past].abs().sum(dim=1) > 0.0).all())


def test_out_of_range_num_frames_is_clamped_as_the_copy_kernels_clamp_it(dev):
    """reverse = 1 with num_frames = -1 (the identity), F + 2 (all F frames reversed) and 2, at (B, H, F) = (3, 256, 5): against the fp64
    restatement, whose flips clamp alike, and bit for bit against the same kernels with reverse = 0 over copies made by
    yt8m_reverse_sequence_f32_tm -- the rule the header promises to match.  c_last is zeros for the two rows out of range."""
    lib = L.lib()
    B, H, F = 3, 256, 5
    nf = np.array([-1, F + 2, 2], dtype=np.int32)
    rs = np.random.RandomState(77)
    zv, zs = (0.8 * rs.randn(F, B, 2 * H)).astype(np.float32), (0.8 * rs.randn(F, B, 2) + 0.1).astype(np.float32)
    lim = np.sqrt(6.0 / (2 * H))
    Uv, Us = (((rs.random_sample(s) * 2 - 1) * lim).astype(np.float32) for s in ((H, 2 * H), (2, H)))
    dy, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
    ref = {dt: R.recurrence_with_grads(zv, zs, Uv, Us, nf, 1, dy, dc, dt) for dt in (torch.float64, torch.float32)}
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Uv_d, Us_d, nf_d, dc_d = d(Uv), d(Us), d(nf), d(dc)
    ws = torch.empty(lib.yt8m_gemm_workspace_bytes() // 4, dtype=torch.float32, device=dev)
    new = lambda *s: torch.full(s, float("nan"), device=dev)

    def run(zv_d, zs_d, dy_d, reverse):
        y, hprev, cs, c_last, dzv, dzs = new(F, B, H), new(F, B, H), new(F + 1, B, H), new(B, H), new(F, B, 2 * H), new(F, B, 2)
        cs[0].zero_()
        work = new(6, B, H)                      # (every operand is held until the synchronise: a freed block may be handed out again)
        tail = (_p(work), _p(nf_d), reverse, F, B, H, _p(ws), ws.numel() * 4, _stream())
        L.check(lib.yt8m_gate_lstm_frames_fwd(_p(zv_d), 2 * H, _p(zs_d), 2, _p(Uv_d), 2 * H, _p(Us_d), _p(y), _p(hprev), _p(cs), _p(c_last), *tail))
        L.check(lib.yt8m_gate_lstm_frames_bwd(_p(zv_d), 2 * H, _p(zs_d), 2, _p(Uv_d), 2 * H, _p(Us_d), _p(cs), _p(dy_d), _p(dc_d), _p(dzv), 2 * H,
                                              _p(dzs), 2, *tail))
        torch.cuda.synchronize()
        return {"o": zv_d[:, :, :H], "g": zv_d[:, :, H:], "i": zs_d[:, :, 0], "f": zs_d[:, :, 1], "y": y, "hprev": hprev, "cs": cs, "c_last": c_last,
                "dzv": dzv, "dzs": dzs}

    got = run(d(zv), d(zs), d(dy), 1)
    _report("gate LSTM frames C ABI num_frames -1, F + 2, 2:", got, ref[torch.float64], ref[torch.float32])
    assert float(got["c_last"][:2].abs().sum()) == 0.0 and float(got["c_last"][2].abs().max()) > 0.0
    rev = lambda t: seq_ops._reverse_tm_into(t.contiguous(), nf_d, torch.empty_like(t.contiguous()), 0)
    step = run(rev(d(zv)), rev(d(zs)), rev(d(dy)), 0)                                       # step order over reversed copies
    for k in ("y", "hprev", "dzv", "dzs"):
        assert torch.equal(rev(step[k]).view(torch.int32), got[k].view(torch.int32)), k
    assert torch.equal(step["cs"].view(torch.int32), got["cs"].view(torch.int32)) and torch.equal(step["c_last"], got["c_last"])


# ---- seq_ops.bigate_lstm_layer at the plugin's width ---------------------------------------------------------------------------------
B_, H_ = 128, 1024
GRADS = ("dWv", "dbv", "dWs", "dbs", "dUv1", "dUs1", "dVv", "dVs", "dUv2", "dUs2")
OP_CASES = {"floats": (64, 12, False), "bytes": (1152, 8, True)}
_REF, _GOT = {}, {}


def _layer_case(name):
    """inputs and both restatements of one op case, computed once and shared by the three forms"""
    if name not in _REF:
        from oracle import np_ref
        Din, F, u8 = OP_CASES[name]
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
        Pf, Pb = R.random_unit(rs, R.NAMES_FW, Din, H_), R.random_unit(rs, R.NAMES_BW, Din, H_)
        grads = [rs.randn(F, B_, H_).astype(np.float32), rs.randn(F, B_, H_).astype(np.float32), rs.randn(B_, H_).astype(np.float32),
                 rs.randn(B_, H_).astype(np.float32)]
        x32 = x.astype(np.float32)
        # the fp64 reference reads the float32 frames the float path is given; on bytes it reads the exact dequantised frames
        ref = {dt: R.by_operand(R.layer_with_grads(x32 if not u8 else x, nf, Pf, Pb, *grads, dt), with_dx=not u8)
               for dt in (torch.float64, torch.float32)}
        _REF[name] = (q, x32, nf, Pf, Pb, grads, ref)
    return _REF[name]


FORMS = {"frame_order": (True, False), "reversed_copies": (True, True), "composed": (False, False)}        # FUSED, REVERSED


def _run_form(dev, monkeypatch, name, form):
    """one forward + backward of the op in `form`, through all four returns (memoised: the agreement test reads both kernel forms)"""
    if (name, form) in _GOT:
        return _GOT[(name, form)]
    q, x32, nf, Pf, Pb, grads, _ = _layer_case(name)
    u8 = OP_CASES[name][2]
    fused, rev = FORMS[form]
    monkeypatch.setattr(seq_ops, "BIGATE_LSTM_FUSED", fused)
    monkeypatch.setattr(seq_ops, "BIGATE_LSTM_REVERSED", rev)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nf_d = d(nf)
    if u8:
        qd = d(q)
        assert seq_ops.u8_hoisted_supported(qd), "the shape of this case must take the byte path"
        x_in = seq_ops.U8FrameImages(qd, nf_d)
    else:
        x_in = d(x32).requires_grad_(True)
    ops_ = [t.to(dev).contiguous().requires_grad_(True) for t in R.operands(R.to_torch(Pf, torch.float32), R.to_torch(Pb, torch.float32))]
    before = dict(seq_ops.BIGATE_LSTM_CALLS)
    outs = seq_ops.bigate_lstm_layer(x_in, *ops_, nf_d)
    assert seq_ops.BIGATE_LSTM_CALLS[form] == before[form] + 1 and sum(seq_ops.BIGATE_LSTM_CALLS.values()) == sum(before.values()) + 1
    sum((o * d(g)).sum() for o, g in zip(outs, grads)).backward()
    torch.cuda.synchronize()
    got = dict(zip(("y", "out2", "c1_last", "c2_last"), (o.detach() for o in outs)))
    if not u8:
        got["dx"] = x_in.grad
    got.update({n: t.grad for n, t in zip(GRADS, ops_)})
    _GOT[(name, form)] = got
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_bigate_lstm_layer_at_h1024_matches_fp64(dev, monkeypatch, name, form):
    """seq_ops.bigate_lstm_layer at B = 128, H = 1024 on float frames (Din = 64, F = 12) and on the reader's bytes (Din = 1152, F = 8) with
    a gradient on all four returns: y, out2, c1_last, c2_last, dx (floats) and the gradient of every operand against fp64; on the
    frame-order kernels, on the same kernels over reversed copies (YT8M_BIGATE_LSTM_REVERSED=1) and with YT8M_BIGATE_LSTM_FUSED=0's
    composed form on the device.  BIGATE_LSTM_CALLS says which form ran."""
    assert L.lib().yt8m_gate_lstm_frames_supported(B_, H_)
    ref = _layer_case(name)[6]
    got = _run_form(dev, monkeypatch, name, form)
    assert set(got) == set(ref[torch.float64])
    _report("bigate_lstm_layer H=1024 %s %s:" % (name, form), got, ref[torch.float64], ref[torch.float32])
    assert float(got["c1_last"][0].abs().max()) == 0.0 and float(got["c2_last"][0].abs().max()) == 0.0   # num_frames = 0: zeros


@pytest.mark.parametrize("name", list(OP_CASES))
def test_frame_order_and_reversed_copies_agree(dev, monkeypatch, name):
    """The two kernel forms of one case against each other, within the bounds either is held to against fp64."""
    ref = _layer_case(name)[6]
    a, b = _run_form(dev, monkeypatch, name, "frame_order"), _run_form(dev, monkeypatch, name, "reversed_copies")
    bound = R.bounds(ref[torch.float64], ref[torch.float32], _floor)
    e = {k: R.err(a[k], b[k].detach().cpu().double().numpy()) for k in bound}
    print("bigate_lstm_layer %s frame order against reversed copies:" % name, " ".join("%s %.2g" % kv for kv in e.items()))
    for k in bound:
        assert e[k] <= bound[k], (k, e[k], bound[k])


def test_refused_shape_takes_the_composed_form(dev):
    """H = 192 is no multiple of 256: yt8m_gate_lstm_frames_supported refuses it and the op computes the same function composed."""
    B, H, F, Din = 16, 192, 5, 64
    assert not L.lib().yt8m_gate_lstm_frames_supported(B, H)
    rs = np.random.RandomState(31)
    nf = _lengths(B, F, 0)
    x = rs.randn(F, B, Din)
    x = (x / np.linalg.norm(x, axis=2, keepdims=True) * (np.arange(F)[:, None] < nf[None, :])[:, :, None]).astype(np.float32)
    Pf, Pb = R.random_unit(rs, R.NAMES_FW, Din, H), R.random_unit(rs, R.NAMES_BW, Din, H)
    grads = [rs.randn(F, B, H).astype(np.float32), rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32),
             rs.randn(B, H).astype(np.float32)]
    ref = {dt: R.layer_with_grads(x, nf, Pf, Pb, *grads, dt) for dt in (torch.float64, torch.float32)}
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = d(x).requires_grad_(True)
    Pft = {n: t.to(dev).requires_grad_(True) for n, t in R.to_torch(Pf, torch.float32).items()}
    Pbt = {n: t.to(dev).requires_grad_(True) for n, t in R.to_torch(Pb, torch.float32).items()}
    before = dict(seq_ops.BIGATE_LSTM_CALLS)
    outs = seq_ops.bigate_lstm_layer(xt, *R.operands(Pft, Pbt), d(nf))
    assert seq_ops.BIGATE_LSTM_CALLS["composed"] == before["composed"] + 1 and sum(seq_ops.BIGATE_LSTM_CALLS.values()) == sum(before.values()) + 1
    sum((o * d(g)).sum() for o, g in zip(outs, grads)).backward()
    got = dict(zip(("y", "out2", "c1_last", "c2_last"), outs), dx=xt.grad)
    got.update({"dfw/" + n: Pft[n].grad for n in R.NAMES_FW})
    got.update({"dbw/" + n: Pbt[n].grad for n in R.NAMES_BW})
    _report("bigate_lstm_layer H=192 composed:", got, ref[torch.float64], ref[torch.float32])


# ---- LstmBigluModel through TrainGraph ---------------------------------------------------------------------------------------------
def test_lstm_biglu_model_loss_and_every_gradient_match_fp64(dev, flags):
    """LstmBigluModel, 256 cells, 2 mixtures, on the reader's bytes [4, 8, 1152] with lengths 0, 1, 8 and 4, V = 32, through
    TrainGraph.forward / loss / backward: the loss and the gradient of every one of the 31 Variables against the restatement followed by
    the MoE head and CrossEntropyLoss in fp64 (bound: eight times the same pipeline in float32, floors as above).  The frame-order
    kernels are engaged."""
    from oracle import np_ref
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    B, F, D, H, V, M = 4, 8, 1152, 256, 32, 2
    flags.lstm_cells, flags.moe_num_mixtures = str(H), M
    rs = np.random.RandomState(41)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = np.array([0, 1, 8, 4], dtype=np.int32)
    y = rs.rand(B, V) < 0.2
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(flm.LstmBigluModel(), batch_size=B, graph=g)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    assert seq_ops.u8_hoisted_supported(args[0]) and L.lib().yt8m_gate_lstm_frames_supported(B, H)
    tg.forward(*args)
    g.finalize()
    head = ["gatesbackward/weights", "expertsbackward/weights", "expertsbackward/biases"]
    assert list(g.vars) == ["lstm_forward/" + n for n in R.NAMES_FW] + ["lstm_backward/" + n for n in R.NAMES_BW] + head
    # a trained unit's scale instead of the initial values: the gates leave their linear range, the head sees both memories
    Pf, Pb = R.random_unit(rs, R.NAMES_FW, D, H), R.random_unit(rs, R.NAMES_BW, D, H)
    vals = {"lstm_forward/" + n: Pf[n] for n in R.NAMES_FW}
    vals.update({"lstm_backward/" + n: Pb[n] for n in R.NAMES_BW})
    vals.update({"gatesbackward/weights": (0.2 * rs.randn(2 * H, V * (M + 1))).astype(np.float32),
                 "expertsbackward/weights": (0.2 * rs.randn(2 * H, V * M)).astype(np.float32),
                 "expertsbackward/biases": (0.2 * rs.randn(V * M)).astype(np.float32)})
    assert set(vals) == set(g.vars) and len(vals) == 31
    for k, v in vals.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    before = dict(seq_ops.BIGATE_LSTM_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    took = "reversed_copies" if seq_ops.BIGATE_LSTM_REVERSED else "frame_order"
    assert seq_ops.BIGATE_LSTM_CALLS[took] == before[took] + 1 and seq_ops.BIGATE_LSTM_CALLS["composed"] == before["composed"]
    x64 = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf))

    def pipeline(dtype):
        tp = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in vals.items()}
        p = R.model_forward(x64.to(dtype), torch.from_numpy(nf), {n: tp["lstm_forward/" + n] for n in R.NAMES_FW},
                            {n: tp["lstm_backward/" + n] for n in R.NAMES_BW}, *(tp[k] for k in head), M)
        lr = R.cross_entropy(p, torch.from_numpy(y))
        lr.backward()
        out = {"predictions": p.detach().numpy(), "loss": np.array([float(lr.detach())])}
        out.update({"d:" + k: t.grad.numpy() for k, t in tp.items()})
        return out

    r64, r32 = pipeline(torch.float64), pipeline(torch.float32)
    got = {"predictions": res["predictions"], "loss": loss.detach().view(1)}
    got.update({"d:" + k: v.grad for k, v in g.vars.items()})
    _report("LstmBigluModel 256 cells, bytes:", got, r64, r32)
    for k in vals:
        assert float(np.abs(r64["d:" + k]).max()) > 0.0, k                # every variable takes part
    assert float(res["predictions"][0].detach().abs().max()) > 0.0         # (the row without frames still gets the head's biases)
