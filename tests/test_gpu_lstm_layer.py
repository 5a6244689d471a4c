"""-m gpu: the wide LSTM step (csrc/lstm_wide.hip), seq_ops.lstm_clip_layer and LstmLayerModel against the fp64 restatement
(tests/lstm_layer_restatement.py).

Bounds.  The measure is the fp64 tests' max |got - ref| / max(1, max |ref|).  Per quantity the bound is EIGHT times the error of the
float32 restatement (plain torch on the CPU, same inputs) against the float64 one, never below 2e-6 for outputs and states or 5e-6 for
gradients (the project's rule, tests/test_gpu_gate_lstm.py).  The margin covers what the float32 restatement does not have: the summation
order of the MFMA products and the 2^-21 per-term error of the three-f16-product forms.  Every test prints the measured errors and the
float32 restatement's.

Measured on an MI355X (largest error per quantity, the float32 restatement's error of the same quantity in brackets):
  C ABI, gates / cs / hs at (B, H, T) = (1, 256, 2): 1.8e-7 / 1.2e-7 / 6.8e-8 [3.5e-7 / 2.8e-7 / 9.0e-8]; (128, 256, 1): 9.1e-8 / 9.8e-8 /
    1.2e-7 [9.3e-8 / 9.8e-8 / 8.5e-8]; (130, 512, 3): 6.3e-7 / 2.3e-7 / 2.8e-7 [5.2e-7 / 2.3e-7 / 2.6e-7]; (321, 1024, 4): 1.3e-6 / 4.4e-7 /
    6.4e-7 [5.7e-7 / 2.3e-7 / 3.2e-7] -- the gates at K = 1024 are the largest figure, 1.3e-6 of a bound of 4.6e-6
  lstm_clip_layer, wide / packed step route, at [4, 30, 128, 256, 5]: bytes out 9.7e-8 / 7.0e-8 [1.0e-7], dW 2.0e-7 / 1.9e-7 [1.6e-7], db
    1.3e-7 / 2.0e-7 [1.8e-7]; floats out 8.8e-8 / 7.3e-8 [1.1e-7], dW 1.5e-7 / 2.0e-7 [1.4e-7], db 1.1e-7 / 1.2e-7 [1.1e-7]
    at [3, 32, 128, 256, 10]: bytes out 1.4e-7 / 1.2e-7 [1.8e-7], dW 2.1e-7 / 1.7e-7 [1.5e-7], db 1.3e-7 / 9.7e-8 [1.4e-7]; floats out
    1.7e-7 / 1.2e-7 [1.7e-7], dW 2.0e-7 / 2.2e-7 [2.1e-7], db 1.8e-7 / 1.8e-7 [1.8e-7]
  LstmLayerModel, wide / packed: predictions 1.2e-7 / 1.2e-7 [1.3e-7], loss 3.0e-8 [4.4e-8], gradients at most 4.0e-7 / 4.1e-7 (the RNN-1
    biases) [4.4e-7]
The floors (2e-6 / 5e-6) are the binding bound everywhere but the gates and hs of the two widest C ABI cases.
"""
import math

import numpy as np
import pytest
import torch

import lstm_layer_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
ROWS = 128                  # the kernel's row tile (asserted against yt8m_lstm_wide_row_tile below)
CELL = "%s/multi_rnn_cell/cell_0/basic_lstm_cell/%s"


def _floor(name):
    return GRAD_FLOOR if name.startswith("d") else OUT_FLOOR


def _report(tag, got, ref64, ref32):
    """prints measured / float32-restatement errors per quantity, then asserts got within the bound"""
    bound = R.bounds(ref64, ref32, _floor)
    e = {k: R.err(got[k], ref64[k]) for k in ref64}
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % (k, e[k], R.err(ref32[k], ref64[k]), bound[k]) for k in ref64))
    for k in ref64:
        assert e[k] <= bound[k], (tag, k, e[k], bound[k])


def _weights(rs, d_in, H, gain=2.0):
    """A cell's weights at a trained cell's scale (a multiple of the Glorot limit, so that the gates leave their linear range)."""
    lim = gain * math.sqrt(6.0 / (d_in + H + 4 * H))
    return ((rs.random_sample((d_in + H, 4 * H)) * 2 - 1) * lim).astype(np.float32), (0.1 * rs.randn(4 * H)).astype(np.float32)


# ---- the step kernel through the C ABI on given hoisted inputs ------------------------------------------------------------------------
ABI_CASES = [(1, 256, 2), (ROWS, 256, 1), (ROWS + 2, 512, 3), (2 * ROWS + ROWS // 2 + 1, 1024, 4)]


@pytest.mark.parametrize("B,H,T", ABI_CASES)
def test_wide_steps_match_fp64_through_the_c_abi(dev, B, H, T):
    """yt8m_lstm_wide_prepare / _steps_fwd at (B, H, T) = (1, 256, 2): a single row; (R, 256, 1): one exact row tile; (R + 2, 512, 3): a
    partial tile, both h images reused; (2R + R/2 + 1, 1024, 4): the model's width.  The activated gates, every cs[t] and hs[t] against
    fp64; W_h has leading dimension 4H + 64 with 1e3 in the padding columns; the tape slots past T keep the caller's NaN fill; a second
    run on the same inputs gives the same bits."""
    lib = L.lib()
    assert lib.yt8m_lstm_wide_row_tile() == ROWS and lib.yt8m_lstm_wide_supported(B, H)
    rs = np.random.RandomState(300 + H + B)
    z = (0.8 * rs.randn(T, B, 4 * H)).astype(np.float32)
    Wh = _weights(rs, 0, H, gain=3.0)[0]
    ref = {dt: R.steps(z, Wh, 1.0, dt) for dt in (torch.float64, torch.float32)}
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ldw = 4 * H + 64
    Wh_d = torch.full((H, ldw), 1.0e3, device=dev)                      # (a read of the padding columns would wreck every value)
    Wh_d[:, :4 * H] = d(Wh)
    need = lib.yt8m_lstm_wide_workspace_bytes(B, H)

    def run():
        z_d = torch.full((T + 1, B, 4 * H), float("nan"), device=dev)
        z_d[:T] = d(z)
        cs = torch.full((T + 2, B, H), float("nan"), device=dev)
        hs = torch.full((T + 2, B, H), float("nan"), device=dev)
        cs[0].zero_()
        hs[0].zero_()
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        L.check(lib.yt8m_lstm_wide_prepare(_p(Wh_d), ldw, B, H, _p(ws), need, _stream()))
        L.check(lib.yt8m_lstm_wide_steps_fwd(_p(z_d), _p(ws), need, _p(cs), _p(hs), None, 0, T, B, H, 1.0, _stream()))
        torch.cuda.synchronize()
        return z_d, cs, hs

    z_d, cs, hs = run()
    got = {"gates": z_d[:T], "cs": cs[:T + 1], "hs": hs[:T + 1]}
    _report("wide step C ABI B=%d H=%d T=%d:" % (B, H, T), got, ref[torch.float64], ref[torch.float32])
    for t in (z_d[T], cs[T + 1], hs[T + 1]):
        assert bool(torch.isnan(t).all())                               # nothing past T was written
    z2, cs2, hs2 = run()
    for a, b in ((z_d, z2), (cs, cs2), (hs, hs2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_wide_steps_continue_from_a_given_state(dev):
    """t0 > 0: the first h image is built from hs[t0], so two calls of two steps give the bits of one call of four."""
    lib = L.lib()
    B, H, T = ROWS + 2, 256, 4
    rs = np.random.RandomState(7)
    z = torch.from_numpy((0.8 * rs.randn(T, B, 4 * H)).astype(np.float32)).to(dev)
    Wh = torch.from_numpy(_weights(rs, 0, H, gain=3.0)[0]).to(dev)
    need = lib.yt8m_lstm_wide_workspace_bytes(B, H)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(lib.yt8m_lstm_wide_prepare(_p(Wh), 4 * H, B, H, _p(ws), need, _stream()))
    res = []
    for parts in (((0, 4),), ((0, 2), (2, 2))):
        zc = z.clone()
        cs, hs = torch.zeros((T + 1, B, H), device=dev), torch.zeros((T + 1, B, H), device=dev)
        for t0, n in parts:
            L.check(lib.yt8m_lstm_wide_steps_fwd(_p(zc), _p(ws), need, _p(cs), _p(hs), None, t0, n, B, H, 1.0, _stream()))
        torch.cuda.synchronize()
        res.append((zc, cs, hs))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][2][T].abs().max()) > 0.0


def _graph_fallbacks():
    """how many step chains the library could not capture as a hipGraph and launched plainly instead (csrc/runtime.hip)"""
    import ctypes
    f = ctypes.c_int64(0)
    L.check(L.lib().yt8m_graph_cache_stats(None, None, ctypes.byref(f), None))
    return f.value


# ---- seq_ops.lstm_clip_layer on the device ---------------------------------------------------------------------------------------------
CLIP_SHAPES = {"even": (4, 30, 128, 256, 5, [0, 3, 17, 30]), "truncated": (3, 32, 128, 256, 10, [7, 25, 32])}
_REF = {}


def _clip_case(shape, u8):
    """inputs and both restatements of one op case, computed once and shared by the runs with and without the wide kernel.  The lengths
    cover 0, less than U1, a non-multiple of U1 and F; dout is zero on the clips at or past num_frames // U1, as RNN-2 leaves it."""
    key = (shape, u8)
    if key not in _REF:
        B, F, D, H, U1, nf = CLIP_SHAPES[shape]
        U2 = F // U1
        rs = np.random.RandomState(400 + F + int(u8))
        nf = np.array(nf, dtype=np.int32)
        W, b = _weights(rs, D, H)
        dead = np.arange(U2)[:, None] >= (nf // U1)[None, :]                            # [U2, B]
        dout = (rs.randn(U2, B, H) * ~dead[:, :, None]).astype(np.float32)
        if u8:
            raw = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
            other = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
            x = R.frames_from_bytes(raw, nf, torch.float64)
        else:
            raw = rs.randn(B, F, D)
            raw = (raw / np.linalg.norm(raw, axis=2, keepdims=True)).astype(np.float32)  # padding frames hold data: the op masks them
            other = (2.0 * rs.randn(B, F, D)).astype(np.float32)
            x = torch.from_numpy(raw)
        frame_dead = np.arange(F)[None, :] >= ((nf // U1) * U1)[:, None]                 # frames of the dead clips, and the dropped ones
        raw2 = np.where(frame_dead[:, :, None], other, raw)
        ref = {dt: R.clip_with_grads(x, nf, U1, W, b, dout, dt) for dt in (torch.float64, torch.float32)}
        _REF[key] = (raw, raw2, nf, W, b, dout, dead, ref)
    return _REF[key]


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "kernel-off"])
@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "floats"])
@pytest.mark.parametrize("shape", list(CLIP_SHAPES))
def test_clip_layer_matches_fp64(dev, monkeypatch, shape, u8, wide):
    """seq_ops.lstm_clip_layer at [B, F, D, H, U1] = [4, 30, 128, 256, 5] and [3, 32, 128, 256, 10] (two frames dropped) on the reader's
    bytes and on float frames, with WIDE_MIN_ROWS = 1 (the wide step kernel) and with the kernel off (an existing step route): the
    memories [U2, B, H], dW and db against fp64; and the clips at or past num_frames // U1, whose memories RNN-2 never reads, contribute
    exactly nothing to dW and db -- the same bits from a run whose dead clips hold other frames."""
    B, F, D, H, U1, _ = CLIP_SHAPES[shape]
    raw, raw2, nf, W, b, dout, dead, ref = _clip_case(shape, u8)
    monkeypatch.setattr(seq_ops, "WIDE", wide)
    monkeypatch.setattr(seq_ops, "WIDE_MIN_ROWS", 1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    took = "wide" if wide else seq_ops.CLIP_FWD_EXISTING

    def run(frames):
        Wt, bt = d(W).requires_grad_(True), d(b).requires_grad_(True)
        before = dict(seq_ops.LSTM_CLIP_CALLS)
        out = seq_ops.lstm_clip_layer(d(frames), d(nf), U1, Wt, bt)
        assert seq_ops.LSTM_CLIP_CALLS[took] == before[took] + 1 and sum(seq_ops.LSTM_CLIP_CALLS.values()) == sum(before.values()) + 1
        (out * d(dout)).sum().backward()
        torch.cuda.synchronize()
        return {"out": out.detach(), "dW": Wt.grad, "db": bt.grad}

    fallbacks = _graph_fallbacks()
    got = run(raw)
    assert _graph_fallbacks() == fallbacks                              # the existing step routes ran where their chains can be captured
    assert tuple(got["out"].shape) == (F // U1, B, H)
    _report("lstm_clip_layer %s %s %s:" % (CLIP_SHAPES[shape][:5], "bytes" if u8 else "floats", took), got, ref[torch.float64],
            ref[torch.float32])
    assert dead.any() and not dead.all()
    got2 = run(raw2)
    live = torch.from_numpy(~dead).to(dev)
    assert torch.equal(got2["out"][live], got["out"][live])
    assert not torch.equal(got2["out"], got["out"])                      # the other frames did reach the dead clips' memories
    assert torch.equal(got2["dW"], got["dW"]) and torch.equal(got2["db"], got["db"])


# ---- LstmLayerModel through TrainGraph -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "kernel-off"])
def test_model_predictions_loss_and_every_gradient_match_fp64(dev, flags, monkeypatch, wide):
    """LstmLayerModel, 256 cells, B = 4, F = 30, D = 128 on the reader's bytes, --lstm_length 5, MoeModel with V = 20 and 2 mixtures,
    through TrainGraph.forward / loss / backward: predictions, loss and the gradient of every Variable against the restatement in fp64
    (bound: eight times the same pipeline in float32, floors as above).  Videos 0 and 1 (num_frames 0 and 3 < U1) hand zeros to the head."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    B, F, D, H, U1, nf = CLIP_SHAPES["even"]
    V, M = 20, 2
    monkeypatch.setattr(seq_ops, "WIDE", wide)
    monkeypatch.setattr(seq_ops, "WIDE_MIN_ROWS", 1)
    flags.lstm_cells, flags.lstm_length, flags.moe_num_mixtures = str(H), U1, M
    rs = np.random.RandomState(51)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = np.array(nf, dtype=np.int32)
    y = rs.rand(B, V) < 0.2
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(flm.LstmLayerModel(), batch_size=B, graph=g)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    tg.forward(*args)
    g.finalize()
    names = [CELL % (s, n) for s in ("RNN-1", "RNN-2") for n in ("weights", "biases")] + ["gates/weights", "experts/weights", "experts/biases"]
    assert list(g.vars) == names
    vals = {}
    vals[names[0]], vals[names[1]] = _weights(rs, D, H)
    vals[names[2]], vals[names[3]] = _weights(rs, H, H)
    vals.update({"gates/weights": (0.2 * rs.randn(H, V * (M + 1))).astype(np.float32),
                 "experts/weights": (0.2 * rs.randn(H, V * M)).astype(np.float32), "experts/biases": (0.2 * rs.randn(V * M)).astype(np.float32)})
    for k, v in vals.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    took = "wide" if wide else seq_ops.CLIP_FWD_EXISTING
    before = dict(seq_ops.LSTM_CLIP_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    assert seq_ops.LSTM_CLIP_CALLS[took] == before[took] + 1 and sum(seq_ops.LSTM_CLIP_CALLS.values()) == sum(before.values()) + 1
    x64 = R.frames_from_bytes(q, nf, torch.float64)
    r64, r32 = (R.model_with_grads(x64, nf, U1, vals, y, M, dt) for dt in (torch.float64, torch.float32))
    got = {"predictions": res["predictions"], "loss": loss.detach().view(())}
    got.update({"d:" + k: v.grad for k, v in g.vars.items()})
    _report("LstmLayerModel 256 cells, bytes, %s:" % took, got, r64, r32)
    for k in vals:
        assert float(np.abs(r64["d:" + k]).max()) > 0.0, k                # every variable takes part
    # rows 0 and 1 reached the head as zeros: their predictions are the head's response to a zero row, the same for both
    assert torch.equal(res["predictions"][0], res["predictions"][1])
