"""-m gpu: the sigmoid attention pooling (csrc/sigmoid_attention.hip, seq_ops.sigmoid_attention) and the three plugins on it against the
fp64 restatement (tests/sigmoid_attention_restatement.py).

Bounds.  The measure is the gate tests' max |got - ref| / max(1, max |ref|) against the fp64 restatement on the same float32 inputs.  Per
quantity the bound is ensemble_restatement.bound in that measure: FOUR times the error of the float32 restatement (plain torch on the CPU)
against the float64 one plus one float32 ulp of the largest reference magnitude.  It is never derived from the kernels' output.  Every
test prints the measured errors and the float32 restatement's.  WIDER names the quantities that get the gate tests' factor 8 and floors
(2e-6 outputs, 5e-6 gradients) instead, with the reason.

Measured on an MI355X (largest error per quantity over the twenty C ABI cases, the float32 restatement's error of the same case in brackets;
first the cases with logits of order 1, then the two with Wa x 20):
  att 5.5e-8 [5.5e-8] / 4.1e-7 [4.3e-7], den 1.9e-7 [5.8e-8] / 1.1e-7 [7.6e-8], pooled 9.4e-8 [6.4e-8] / 4.6e-7 [3.9e-7],
  dvals 6.2e-8 [6.2e-8] / 2.3e-7 [2.8e-7] on the 4 x bound, the nearest approach den at 0.56 of it ((33, 17, 516, 260, 3), every pointer 4 bytes off);
  dsrc 6.2e-7 [2.0e-7] / 3.3e-6 [7.7e-6], dWa 7.5e-7 [5.3e-7] / 3.2e-6 [6.4e-6], dba 2.8e-6 [1.4e-6] / 4.2e-6 [7.4e-6] on the wider one; on
  the 4 x bound dsrc missed once, 3.3e-7 against 3.27e-7 [7.8e-8] at (33, 17, 516, 260, 3) with both gradients, and dba twice at
  (5, 3, 128, 128, 1), 4.0e-7 against 2.2e-7 [5.0e-8] and 4.3e-8 against 4.2e-8 [8.7e-9].  At full F, (300, 2, 256, 512, 8) with 300 and 299
  frames, every quantity is nearer to fp64 than the float32 restatement (dWa 2.6e-7 [9.1e-7], dsrc 6.8e-9 [1.1e-8]).
  the op: kernels dba 2.8e-6 [1.4e-6], dsrc 3.3e-7 [7.8e-8]; composed dba 1.5e-6 [1.4e-6], dsrc 1.4e-7 [7.8e-8]
  the twelve plugin cases: predictions 2.8e-7 [2.1e-7], loss 9.2e-8 [9.2e-8], gradients 5.2e-7 [3.2e-7] (LstmAttentionLstmModel, 2 layers,
  bytes, RNN/.../cell_1/.../biases) against floors of 2e-6 / 5e-6
"""
import numpy as np
import pytest
import torch

import sigmoid_attention_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
# quantity -> reason
WIDER = {"dsrc": "dz = (dt - inner) att (1 - sig) subtracts two float32 numbers of the size of vals . G, up to 4 sqrt(Hv) = 64 at Hv = 260: an "
                 "ulp of that, 4e-6 to 8e-6, times att (1 - sig) <= 1/4 stays in dz in ANY summation order, and for a video of ONE frame, "
                 "whose exact dz is 0, it is all of dz; the float32 restatement's own draw of that noise is no measure of it",
         "dWa": "dz's noise as in dsrc, and a sum over up to F B = 600 rows: 32 rows per thread, then the workgroups' partials 32 at a time, where torch adds pairwise",
         "dba": "as dWa; with A = 1 it is one number, whose float32 error is a matter of luck (3.3e-7 on one host, 5.0e-8 on another)"}
GUARD = 16            # floats around every output
SENTINEL = -1234.5


def _bound(name, r32, r64):
    ref64 = torch.from_numpy(np.asarray(r64, dtype=np.float64))
    ref32 = torch.from_numpy(np.asarray(r32, dtype=np.float64))
    big = max(1.0, float(ref64.abs().max()) if ref64.numel() else 0.0)
    if name in WIDER:
        floor = GRAD_FLOOR if name.startswith("d") else OUT_FLOOR
        return max(8.0 * R.err(r32, r64), floor)
    return R.bound(ref32, ref64) / big


def _report(tag, got, ref64, ref32):
    """prints measured / float32-restatement errors and bounds per quantity, then asserts every one of them"""
    rows = [(k, R.err(got[k], ref64[k]), R.err(ref32[k], ref64[k]), _bound(k, ref32[k], ref64[k])) for k in got]
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % r for r in rows))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, (tag, bad)


def _lengths(B, F, shift):
    """num_frames holding 0, 1, F, F - 1 and a mid value (rotated by `shift`): the _lengths of tests/test_gpu_gate_lstm.py"""
    pat = [0, 1, F, F - 1, F // 2]
    return np.array([pat[(b + shift) % 5] for b in range(B)], dtype=np.int32)


class _Guarded(object):
    """A device buffer of `rows` rows of `ld` floats (the first `width` of each are the operand) between GUARD sentinel floats, `off`
    floats past a 16-byte boundary; everything that is not operand is sentinel and must stay so."""

    def __init__(self, dev, rows, width, ld=None, off=0, data=None):
        ld = width if ld is None else ld
        self.rows, self.width, self.ld = rows, width, ld
        self.buf = torch.full((GUARD + off + rows * ld + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.flat = self.buf[GUARD + off:GUARD + off + rows * ld]
        assert self.flat.data_ptr() % 16 == 4 * off
        self.view = self.flat.view(rows, ld)[:, :width]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).view(rows, width))
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[GUARD + off:GUARD + off + rows * ld].view(rows, ld)[:, :width] = False

    def intact(self):
        return bool((self.buf[self.mask] == SENTINEL).all())

    def get(self, shape):
        return self.view.contiguous().view(shape)


# (F, B, Hs, Hv, A): odd B | widths multiples of 4 and of nothing larger, odd A, partial-wave tails | the plugins' width | full F: the
# time split and its fixed-order finish, largest A, Hs != Hv
SHAPES = [(5, 3, 128, 128, 1), (33, 17, 516, 260, 3), (9, 5, 1024, 1024, 1), (300, 2, 256, 512, 8)]
# G and E | E absent | G absent | weights only (Hv = 0)
VARIANTS = ["GE", "G", "E", "weights"]
EXTRA = [((33, 17, 516, 260, 3), "misaligned"), ((9, 5, 1024, 1024, 1), "dirty"), ((300, 2, 256, 512, 8), "saturated"),
         ((33, 17, 516, 260, 3), "saturated")]
_ABI_REF = {}


def _abi_case(shape, variant):
    """inputs and both restatements of one case, computed once"""
    key = (shape, variant)
    if key not in _ABI_REF:
        F, B, Hs, Hv, A = shape
        rs = np.random.RandomState(F * 1000 + Hs + len(variant))
        nf = _lengths(B, F, 2 if B == 2 else 0)               # B = 2: F and F - 1, so that every time chunk is in play
        live = (np.arange(F)[:, None] < nf[None, :])[:, :, None]
        src = rs.randn(F, B, Hs).astype(np.float32)
        if variant != "dirty":
            src = src * live                                  # a stack leaves zero rows past num_frames
        vals = rs.randn(F, B, Hv).astype(np.float32) * (live if variant != "dirty" else 1.0)
        scale = 20.0 if variant == "saturated" else 1.0       # logits of order 1; x 20: the sigmoids saturate
        Wa = (scale * rs.randn(Hs, A) / np.sqrt(Hs)).astype(np.float32)
        ba = (0.1 * rs.randn(A)).astype(np.float32)
        G = None if variant in ("E", "weights") else rs.randn(B, A, Hv).astype(np.float32)
        E = None if variant == "G" else rs.randn(B, F, A).astype(np.float32)
        if variant == "weights":
            vals = None
        ref = {dt: R.op_with_grads(src, vals, Wa, ba, nf, G, E, dt) for dt in (torch.float64, torch.float32)}
        assert all(np.isfinite(v).all() for v in ref[torch.float32].values())
        _ABI_REF[key] = (nf, src, vals.astype(np.float32) if vals is not None else None, Wa, ba, G, E, ref)
    return _ABI_REF[key]


@pytest.mark.parametrize("shape,variant", [(s, v) for s in SHAPES for v in VARIANTS] + EXTRA,
                         ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else p)
def test_kernels_match_fp64_through_the_c_abi(dev, shape, variant):
    """yt8m_sigattn_fwd / _bwd against the fp64 restatement on the same float32 inputs: att, den, pooled, dsrc, dvals, dWa, dba under the
    bound; guard words around every output, in the padding columns of the strided ones and behind the workspace keep their sentinel;
    dsrc and dvals are exactly zero at and past each row's num_frames; a second run, with the optional outputs not asked for, is bit-equal
    and leaves them untouched.  Variants: both gradients, each one absent, weights only; every pointer 4 bytes off a 16-byte boundary;
    non-zero src / vals rows past num_frames (the mask, not the data, does the work); Wa x 20."""
    F, B, Hs, Hv, A = shape
    if variant == "weights":
        Hv = 0
    lib = L.lib()
    assert lib.yt8m_sigattn_supported(B, F, Hs, Hv, A)
    nf, src, vals, Wa, ba, G, E, ref = _abi_case(shape, variant)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    off = 1 if variant == "misaligned" else 0
    pad = 8 if Hs == 1024 else 0                                                 # row strides larger than the widths
    mk = lambda rows, width, ld=None, data=None: _Guarded(dev, rows, width, ld, off, data)
    nf_d = torch.from_numpy(nf).to(dev)
    src_d = mk(F * B, Hs, Hs + pad, src)
    vals_d = mk(F * B, Hv, Hv + pad, vals) if Hv else None
    Wa_d, ba_d = mk(Hs, A, data=Wa), mk(1, A, data=ba)
    G_d = mk(B * A, Hv, data=G) if G is not None else None
    E_d = mk(B * F, A, data=E) if E is not None else None
    need = int(lib.yt8m_sigattn_workspace_bytes(B, F, Hs, Hv, A))
    assert need > 0 and need % 16 == 0
    ws = mk(1, need // 4)
    P = lambda g: None if g is None else _p(g.flat)
    LD = lambda g: 0 if g is None else g.ld

    def forward():
        att, den, pooled = mk(B * F, A), mk(B, A), (mk(B * A, Hv) if Hv else None)
        L.check(lib.yt8m_sigattn_fwd(P(src_d), LD(src_d), P(vals_d), LD(vals_d), P(Wa_d), P(ba_d), _p(nf_d), P(att), P(den), P(pooled),
                                     P(ws), need, B, F, Hs, Hv, A, _stream()))
        torch.cuda.synchronize()
        return att, den, pooled

    def backward(att, den, pooled, optional):
        dsrc = mk(F * B, Hs, Hs + pad)
        dvals = mk(F * B, Hv, Hv + pad) if (Hv and optional) else None
        dWa, dba = (mk(Hs, A), mk(1, A)) if optional else (None, None)
        L.check(lib.yt8m_sigattn_bwd(P(src_d), LD(src_d), P(vals_d), LD(vals_d), P(Wa_d), _p(nf_d), P(att), P(den), P(pooled), P(G_d), P(E_d),
                                     P(dsrc), LD(dsrc), P(dvals), LD(dvals), P(dWa), P(dba), P(ws), need, B, F, Hs, Hv, A, _stream()))
        torch.cuda.synchronize()
        return dsrc, dvals, dWa, dba

    att, den, pooled = forward()
    dsrc, dvals, dWa, dba = backward(att, den, pooled, True)
    got = {"att": att.get((B, F, A)), "den": den.get((B, A)), "dsrc": dsrc.get((F, B, Hs)), "dWa": dWa.get((Hs, A)), "dba": dba.get((A,))}
    if Hv:
        got.update(pooled=pooled.get((B, A, Hv)), dvals=dvals.get((F, B, Hv)))
    for name, g in (("src", src_d), ("vals", vals_d), ("Wa", Wa_d), ("ba", ba_d), ("G", G_d), ("E", E_d), ("att", att), ("den", den),
                    ("pooled", pooled), ("dsrc", dsrc), ("dvals", dvals), ("dWa", dWa), ("dba", dba), ("workspace", ws)):
        assert g is None or g.intact(), "guard words of %s" % name
    _report("sigattn C ABI %s %s:" % (shape, variant), got, {k: r64[k] for k in got}, r32)
    # rows of a video without frames, and every row at or past num_frames: exact zeros
    past = torch.from_numpy(np.arange(F)[:, None] >= nf[None, :]).to(dev)        # [F,B]
    assert past.any() and ((nf == 0).any() or B == 2)
    assert float(got["dsrc"][past].abs().sum()) == 0.0 and float(got["att"].transpose(0, 1)[past].abs().sum()) == 0.0
    empty = torch.from_numpy(nf == 0).to(dev)
    assert bool((got["den"][empty] == np.float32(1e-8)).all())
    if Hv:
        assert float(got["dvals"][past].abs().sum()) == 0.0 and float(got["pooled"][empty].abs().sum()) == 0.0
        if G is None:
            assert float(got["dvals"].abs().sum()) == 0.0
    # a second run is bit-equal; without the optional outputs dsrc keeps its bits
    att2, den2, pooled2 = forward()
    dsrc2, _, _, _ = backward(att2, den2, pooled2, False)
    dsrc3, dvals3, dWa3, dba3 = backward(att2, den2, pooled2, True)
    same = lambda a, b: torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))
    assert same(att, att2) and same(den, den2) and (not Hv or same(pooled, pooled2))
    assert same(dsrc, dsrc2) and same(dsrc, dsrc3) and same(dWa, dWa3) and same(dba, dba3) and (not Hv or same(dvals, dvals3))
    assert ws.intact()


def test_refused_shapes_launch_nothing(dev):
    """A shape yt8m_sigattn_supported refuses: YT8M_E_SHAPE and the outputs keep their sentinel."""
    lib = L.lib()
    F, B, Hs, A = 4, 3, 130, 1
    assert not lib.yt8m_sigattn_supported(B, F, Hs, 0, A)
    src, Wa, ba = _Guarded(dev, F * B, Hs), _Guarded(dev, Hs, A), _Guarded(dev, 1, A)
    att, den, ws = _Guarded(dev, B * F, A), _Guarded(dev, B, A), _Guarded(dev, 1, 1 << 16)
    nf = torch.full((B,), F, dtype=torch.int32, device=dev)
    rc = lib.yt8m_sigattn_fwd(_p(src.flat), Hs, None, 0, _p(Wa.flat), _p(ba.flat), _p(nf), _p(att.flat), _p(den.flat), None, _p(ws.flat),
                              4 << 16, B, F, Hs, 0, A, _stream())
    torch.cuda.synchronize()
    assert rc == -2
    assert bool((att.buf == SENTINEL).all()) and bool((den.buf == SENTINEL).all()) and bool((ws.buf == SENTINEL).all())


# ---- seq_ops.sigmoid_attention on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["kernels", "composed"])
@pytest.mark.parametrize("with_values", [True, False], ids=["pooled", "weights"])
def test_op_fused_against_composed(dev, monkeypatch, fused, with_values):
    """seq_ops.sigmoid_attention at (F, B, Hs, Hv, A) = (33, 17, 516, 260, 3) with a gradient on att AND on pooled, on the kernels
    (SIGMOID_ATTENTION_CALLS shows that they ran) and with YT8M_SIGMOID_ATTENTION_FUSED=0's composed form: both against fp64."""
    shape = (33, 17, 516, 260, 3)
    F, B, Hs, Hv, A = shape
    nf, src, vals, Wa, ba, G, E, ref = _abi_case(shape, "GE" if with_values else "weights")
    monkeypatch.setattr(seq_ops, "SIGMOID_ATTENTION_FUSED", fused)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ts, tW, tb = (d(a).requires_grad_(True) for a in (src, Wa, ba))
    tv = d(vals).requires_grad_(True) if with_values else None
    before = dict(seq_ops.SIGMOID_ATTENTION_CALLS)
    att, pooled = seq_ops.sigmoid_attention(ts, tW, tb, d(nf), tv)
    took = "kernels" if fused else "composed"
    assert seq_ops.SIGMOID_ATTENTION_CALLS == dict(before, **{took: before[took] + 1})
    loss = (att * d(E)).sum()
    if with_values:
        loss = loss + (pooled * d(G)).sum()
    else:
        assert pooled is None
    loss.backward()
    torch.cuda.synchronize()
    got = {"att": att, "dsrc": ts.grad, "dWa": tW.grad, "dba": tb.grad}
    if with_values:
        got.update(pooled=pooled, dvals=tv.grad)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    if fused:
        _report("sigmoid_attention %s kernels:" % (shape,), got, {k: r64[k] for k in got}, r32)
    else:                                   # the composed form runs through the library's GEMMs and pooling kernels: the gate tests' bound
        for k in got:
            e = R.err(got[k], r64[k])
            print("sigmoid_attention composed %s %.2g (fp32 %.2g)" % (k, e, R.err(r32[k], r64[k])))
            assert e <= max(8.0 * R.err(r32[k], r64[k]), GRAD_FLOOR if k.startswith("d") else OUT_FLOOR), k


# ---- the plugins through create_model -------------------------------------------------------------------------------------------------
PLUGINS = ("LstmAttentionModel", "LstmAttentionLstmModel", "LstmMultiAttentionModel")
B_, F_, H_, V_, M_, A_ = 5, 9, 256, 32, 2, 3
# The plugins' bound is the gate tests' from the start (gate_lstm_restatement.bounds: 8 x the float32 pipeline's error, floors 2e-6 /
# 5e-6): the stacks' hoisted products and the head run as three-f16-product GEMMs with a 2^-21 per-term error and a K-split summation
# order, and the recurrences use v_exp / v_rcp gate functions compounding over F steps -- none of which the float32 restatement has.


def _plugin_inputs(u8, seed):
    from oracle import np_ref
    rs = np.random.RandomState(seed)
    D = 1152 if u8 else 64
    nf = _lengths(B_, F_, 1)
    if u8:
        q = rs.randint(0, 256, size=(B_, F_, D)).astype(np.uint8)
        x64 = np_ref.dequant_l2norm_folded(q, nf)                                    # [B,F,D] fp64, padding rows zero
        x_in = q
    else:
        x = rs.randn(B_, F_, D)
        x = x / np.linalg.norm(x, axis=2, keepdims=True) * (np.arange(F_)[None, :] < nf[:, None])[:, :, None]
        x_in = x.astype(np.float32)
        x64 = x_in.astype(np.float64)
    y = rs.rand(B_, V_) < 0.2
    return rs, D, nf, x_in, x64, y


def _trained_values(rs, shapes):
    """a trained model's scale instead of the initial values: the gates leave their linear range, the attention is not flat"""
    vals = {}
    for k, s in shapes.items():
        if k.endswith("biases"):
            vals[k] = (0.1 * rs.randn(*s)).astype(np.float32)
        elif "fully_connected" in k:
            vals[k] = (4.0 * rs.randn(*s) / np.sqrt(s[0])).astype(np.float32)
        else:
            vals[k] = (rs.randn(*s) * (0.2 if k.startswith(("gates", "experts")) else 1.0 / np.sqrt(s[0]))).astype(np.float32)
    return vals


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "floats"])
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("name", PLUGINS)
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, layers, u8):
    """Each plugin through TrainGraph.forward / loss / backward at B = 5, F = 9, 256 cells, 1 and 2 layers, V = 32, 2 mixtures, on the
    reader's bytes (D = 1152) and on float frames (D = 64), with the kernels engaged: predictions, loss and the gradient of EVERY variable
    against the restatement followed by the MoE head and CrossEntropyLoss in fp64."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    monkeypatch.setattr(seq_ops, "SIGMOID_ATTENTION_FUSED", True)
    A = A_ if name == "LstmMultiAttentionModel" else 1
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures, flags.attention_size = str(H_), layers, M_, A
    rs, D, nf, x_in, x64, y = _plugin_inputs(u8, 50 + layers)
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(getattr(flm, name)(), batch_size=B_, graph=g)
    args = (torch.from_numpy(x_in).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    if u8:
        assert flm._lib_u8_ok(D) and seq_ops.u8_attention_supported(args[0], A), "the shape of this case must take the byte path"
    tg.forward(*args)
    g.finalize()
    shapes = R.variable_shapes(name, D, H_, layers, A, V_, M_)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(shapes.items())
    vals = _trained_values(rs, shapes)
    for k, v in vals.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev))
    before = dict(seq_ops.SIGMOID_ATTENTION_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    assert seq_ops.SIGMOID_ATTENTION_CALLS == dict(before, kernels=before["kernels"] + 1)

    def pipeline(dtype):
        tp = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in vals.items()}
        p = R.predictions(name, torch.from_numpy(x64).to(dtype), torch.from_numpy(nf), tp, layers, M_)
        lr = R.cross_entropy(p, torch.from_numpy(y))
        lr.backward()
        out = {"predictions": p.detach().numpy(), "loss": np.array([float(lr.detach())])}
        out.update({"d:" + k: t.grad.numpy() for k, t in tp.items()})
        return out

    r64, r32 = pipeline(torch.float64), pipeline(torch.float32)
    got = {"predictions": res["predictions"], "loss": loss.detach().view(1)}
    got.update({"d:" + k: v.grad for k, v in g.vars.items()})
    bound = R.bounds(r64, r32, lambda k: GRAD_FLOOR if k.startswith("d") else OUT_FLOOR)
    e = {k: R.err(got[k], r64[k]) for k in r64}
    print("%s layers=%d %s:" % (name, layers, "bytes" if u8 else "floats"),
          " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % (k, e[k], R.err(r32[k], r64[k]), bound[k]) for k in r64))
    bad = [(k, e[k], bound[k]) for k in r64 if not e[k] <= bound[k]]
    assert not bad, bad
    for k in vals:
        assert float(np.abs(r64["d:" + k]).max()) > 0.0, k                         # every variable takes part


@pytest.mark.parametrize("name", PLUGINS)
def test_a_training_step_and_its_bitwise_replay(dev, flags, monkeypatch, name):
    """Two TrainGraph.step calls (cross entropy, clip, Adam) of each plugin on the reader's bytes with the kernels: finite losses, every
    variable moved; the same two steps taken twice from the same state leave bit-identical parameters and Adam moments."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    monkeypatch.setattr(seq_ops, "SIGMOID_ATTENTION_FUSED", True)
    A = A_ if name == "LstmMultiAttentionModel" else 1
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures, flags.attention_size = str(H_), 2, M_, A
    _, D, nf, x_in, _, y = _plugin_inputs(True, 77)
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(getattr(flm, name)(), batch_size=B_, graph=g)
    args = (torch.from_numpy(x_in).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    before = dict(seq_ops.SIGMOID_ATTENTION_CALLS)
    out = tg.step(*args)
    assert np.isfinite(float(out["loss"])) and tuple(out["predictions"].shape) == (B_, V_)
    assert seq_ops.SIGMOID_ATTENTION_CALLS["kernels"] > before["kernels"] and seq_ops.SIGMOID_ATTENTION_CALLS["composed"] == before["composed"]
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step = tg.global_step
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step = step
        for _ in range(2):
            out = tg.step(*args)
            assert np.isfinite(float(out["loss"]))
        torch.cuda.synchronize()
        after.append([t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)])
    assert all(torch.equal(a, b) for a, b in zip(*after))
    for v in g.trainable_variables():
        assert not torch.equal(after[0][0][v.offset:v.offset + v.numel()], state[0][v.offset:v.offset + v.numel()]), v.name
