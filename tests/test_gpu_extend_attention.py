"""-m gpu: the windowed softmax attention pooling (csrc/softmax_attention.hip, seq_ops.softmax_attention_tm), the two Extend plugins and
their two heads against the fp64 restatement (tests/extend_attention_restatement.py).

Bounds.  The measure is max |got - ref| / max(1, max |ref|) against the fp64 restatement on the same float32 inputs.  Per quantity the
bound is ensemble_restatement.bound in that measure: FOUR times the error of the float32 restatement (plain torch on the CPU, in the
reference's form: softmax over all frames, times the mask, renormalised) against the float64 one plus one float32 ulp of the largest
reference magnitude.  It is never derived from the kernels' output.  Every test prints the measured errors and the float32
restatement's.  WIDER names the quantities that get the gate tests' factor 8 and floors (2e-6 outputs, 5e-6 gradients) instead, with the
reason.  Every case asserts that the float32 restatement is finite and that the sum it divides by is positive on every non-empty (b, e).

Measured on an MI355X (largest error per quantity over the thirty-two C ABI cases, the float32 restatement's error of the same case in
brackets; first the cases with logits of order 1, then the three with W1 and extra x 6):
  att 1.2e-7 [2.2e-7] / 6.4e-7 [1.9e-6], pooled 2.7e-7 [6.1e-7] / 7.0e-7 [2.2e-6], dvals 1.9e-7 [5.3e-7] / 3.2e-7 [9.8e-7] on the 4 x bound,
  the nearest approach dvals at 0.28 of it ((5, 3, 128, 128, 1), both masks);
  dsrc 1.9e-7 [4.1e-7] / 1.5e-6 [3.4e-6], dW1 3.2e-7 [1.1e-6] / 1.0e-6 [1.2e-6], dextra 2.6e-7 [6.8e-7] / 1.4e-6 [3.0e-6] on the wider one, the
  nearest approach dW1 at 0.11 of it (shared (300, 2, 256, 256, 8), windows, x 6); db1 is exact zeros (below) [3.8e-6 / 4.5e-7].
  An earlier form of the backward took dt - inner from two dot products, inner = pooled . G from a pre-pass, and added dz up for db1: every
  other quantity held its bound, db1 did not (1.7e-5 against 1.1e-5 [1.4e-6] at (9, 5, 1024, 1024, 4) with both masks; 7.8e-6 against 5e-6
  [4.8e-7] at (33, 17, 516, 260, 3) x 6).  The rounding of the stored float32 pooled, times sqrt(Hv) |G|, is an error of ONE sign in every dz
  of a (video, head), which a sum over the frames keeps.  The kernels now take (vals - pooled) . G per element, add pooled up with
  compensated sums, and write db1, whose exact value is 0 for every operand, as zeros.
  the op: kernels dsrc 6.2e-8 [1.8e-7], dW1 1.4e-7 [4.2e-7]; composed dsrc 8.2e-7 [8.2e-7], db1 3.6e-6 [3.8e-6] (rounding noise: the exact value is 0)
  the eight plugin cases: predictions 2.2e-7 [1.8e-7], loss 8.9e-8 [1.9e-8], attention_weight 9.8e-8 [5.2e-8] against floors of 2e-6 / 5e-6
"""
import numpy as np
import pytest
import torch

import extend_attention_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
# quantity -> reason
_DZ = ("dz = att (dt - inner) subtracts two float32 numbers of the size of vals . G, up to 4 sqrt(Hv): an ulp of that times att stays in dz in "
       "ANY summation order, and for a window of ONE frame, whose exact dz is 0, it is all of dz; the float32 restatement's own draw of that "
       "noise is no measure of it")
WIDER = {"dsrc": _DZ,
         "dextra": "dextra IS dz: " + _DZ,
         "dW1": "dz's noise as in dsrc, and a sum over up to F B = 600 rows: 64 rows per thread, then the workgroups' partials 32 at a time, where torch adds pairwise",
         "db1": "its exact value is 0 (a softmax does not see a shift of all its logits): the float32 restatement's and the composed form's are rounding "
                "noise of sum dz; the kernels write exact zeros"}
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
    """num_frames holding 0, 1, F, F - 1 and a mid value (rotated by `shift`): the _lengths of tests/test_gpu_sigmoid_attention.py"""
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


def _offset(dev, a, off):
    """an integer operand `off` elements of 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pad = 4 * off // t.element_size()
    buf = torch.zeros((t.numel() + pad,), dtype=t.dtype, device=dev)
    buf[pad:].copy_(t.view(-1))
    return buf[pad:]


# (F, B, Hs, Hv, E), Hv None: the shared mode.  odd B | widths multiples of 4 and of nothing larger, odd E, partial-wave tails, a
# partial chunk | the plugins' width | full F: five chunks and their fixed-order finish, largest E, Hs != Hv
SHAPES = [(5, 3, 128, 128, 1), (33, 17, 516, 260, 3), (9, 5, 1024, 1024, 4), (300, 2, 256, 512, 8), (33, 17, 516, None, 3), (300, 2, 256, None, 8)]
MASKS = ["frames", "window", "both"]
# windows that start and end on frames 31, 32, 33 and on the chunk edge 63, 64, 65; windows of one frame; an empty one; the last frame
EDGES = np.array([[[31, 31], [32, 32], [33, 33], [31, 33], [63, 63], [64, 64], [63, 65], [65, 65]],
                  [[0, 0], [299, 299], [31, 32], [32, 33], [63, 64], [64, 65], [298, 305], [5, 4]]], dtype=np.int32)
EXTRA = [((33, 17, 516, 260, 3), "frames", "noextra"), ((300, 2, 256, None, 8), "window", "noextra"),
         ((33, 17, 516, 260, 3), "both", "misaligned"), ((33, 17, 516, None, 3), "both", "misaligned"),
         ((9, 5, 1024, 1024, 4), "both", "dirty"), ((33, 17, 516, None, 3), "frames", "dirty"), ((300, 2, 256, 512, 8), "edges", "dirty"),
         ((300, 2, 256, 512, 8), "both", "saturated"), ((33, 17, 516, 260, 3), "frames", "saturated"), ((300, 2, 256, None, 8), "window", "saturated"),
         ((300, 2, 256, 512, 8), "edges", "plain"), ((300, 2, 256, None, 8), "edges", "plain"),
         ((33, 17, 516, 260, 3), "oneframe", "plain"), ((33, 17, 516, None, 3), "oneframe", "plain")]
_ABI_REF = {}


def _abi_case(shape, mask, variant):
    """inputs and both restatements of one case, computed once"""
    key = (shape, mask, variant)
    if key not in _ABI_REF:
        F, B, Hs, Hv, E = shape
        shared = Hv is None
        rs = np.random.RandomState(F * 1000 + Hs + 7 * len(mask) + len(variant))
        nf = _lengths(B, F, 2 if B == 2 else 0)               # B = 2: F and F - 1, so that every time chunk is in play
        live = (np.arange(F)[:, None] < nf[None, :])[:, :, None]
        src = (rs.randn(F, B, Hs) * live).astype(np.float32)  # a stack leaves zero rows past num_frames
        vals = None if shared else (rs.randn(F, B, Hv) * live).astype(np.float32)
        scale = 6.0 if variant == "saturated" else 1.0        # logits of order 1; x 6: a few frames take all the weight
        W1 = (scale * rs.randn(Hs, E) / np.sqrt(Hs)).astype(np.float32)
        b1 = (0.1 * rs.randn(E)).astype(np.float32)
        extra = None if variant == "noextra" else (scale * 0.5 * rs.randn(B, F, E)).astype(np.float32)
        G = rs.randn(B, E, Hs if shared else Hv).astype(np.float32)
        valid = np.ascontiguousarray(live[:, :, 0].T).astype(np.uint8) if mask in ("frames", "both") else None
        lo = hi = None
        if mask in ("window", "both"):                        # InputExtendModel's windows: they reach into the padding rows
            lo, hi = (t.numpy().astype(np.int32) for t in R.windows(nf, E))
        elif mask == "edges":
            lo, hi = np.ascontiguousarray(EDGES[:, :, 0]), np.ascontiguousarray(EDGES[:, :, 1])
        elif mask == "oneframe":
            lo = np.array([[(7 * b + 11 * e) % F for e in range(E)] for b in range(B)], dtype=np.int32)
            hi = lo.copy()
        m = R.mask(F, B, E, valid, lo, hi)
        ref = {dt: R.op_with_grads(src, vals, W1, b1, extra, valid, lo, hi, G, dt) for dt in (torch.float64, torch.float32)}
        r32 = ref[torch.float32]
        nonempty = m.any(dim=1).numpy()
        assert all(np.isfinite(v).all() for v in r32.values())
        assert (r32["den"][nonempty] > 0).all(), "the reference's float32 form underflows on a non-empty (b, e)"
        for r in ref.values():
            del r["den"]
        _ABI_REF[key] = (nf, src, vals, W1, b1, extra, valid, lo, hi, G, m.numpy(), ref)
    return _ABI_REF[key]


def _ids(p):
    if isinstance(p, tuple):
        return "x".join("shared" if v is None else str(v) for v in p)
    return p


@pytest.mark.parametrize("shape,mask,variant", [(s, m, "plain") for s in SHAPES for m in MASKS] + EXTRA, ids=_ids)
def test_kernels_match_fp64_through_the_c_abi(dev, shape, mask, variant):
    """yt8m_smattn_fwd / _bwd against the fp64 restatement on the same float32 inputs: att, pooled, dsrc, dvals, dW1, db1, dextra under the
    bound; guard words around every output, in the padding columns of the strided ones and behind the workspace keep their sentinel;
    att, dsrc, dvals and dextra are exactly zero where the mask is; a second run is bit-equal, and so is every run with ONE optional
    output left NULL.  Masks: the frames of each video, InputExtendModel's windows (which reach into the padding rows), both, windows on
    the chunk edges, windows of one frame.  Variants: no extra; every pointer 4 bytes off a 16-byte boundary and odd leading dimensions;
    NaN in every row of src and vals that no head unmasks; W1 and extra x 6."""
    F, B, Hs, Hv, E = shape
    shared = Hv is None
    Hv = Hs if shared else Hv
    lib = L.lib()
    assert lib.yt8m_smattn_supported(B, F, Hs, Hv, E)
    nf, src, vals, W1, b1, extra, valid, lo, hi, G, m, ref = _abi_case(shape, mask, variant)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    mis = variant == "misaligned"
    off = 1 if mis else 0
    pad = 5 if mis else (8 if Hs == 1024 else 0)                                 # row strides larger than the widths; odd when misaligned
    mk = lambda rows, width, ld=None, data=None: _Guarded(dev, rows, width, ld, off, data)
    row_live = m.any(axis=2).T                                                   # [F,B]: some head unmasks the row
    if variant == "dirty":                                                       # the mask, not the data, does the work
        src = np.where(row_live[:, :, None], src, np.float32(np.nan))
        vals = None if shared else np.where(row_live[:, :, None], vals, np.float32(np.nan))
        assert np.isnan(src).any()
    src_d = mk(F * B, Hs, Hs + pad, src)
    vals_d = src_d if shared else mk(F * B, Hv, Hv + pad, vals)
    W1_d, b1_d = mk(Hs, E, data=W1), mk(1, E, data=b1)
    extra_d = None if extra is None else mk(B * F, E, data=extra)
    G_d = mk(B * E, Hv, data=G)
    I = lambda a: None if a is None else _offset(dev, a, off)
    valid_d, lo_d, hi_d = I(valid), I(lo), I(hi)
    need = int(lib.yt8m_smattn_workspace_bytes(B, F, Hs, Hv, E))
    assert need > 0 and need % 16 == 0
    ws = mk(1, need // 4)
    P = lambda g: None if g is None else _p(g.flat)
    LD = lambda g: 0 if g is None else g.ld

    def forward():
        att, pooled = mk(B * F, E), mk(B * E, Hv)
        L.check(lib.yt8m_smattn_fwd(P(src_d), LD(src_d), P(vals_d), LD(vals_d), P(W1_d), P(b1_d), P(extra_d), _p(valid_d), _p(lo_d), _p(hi_d),
                                    P(att), P(pooled), P(ws), need, B, F, Hs, Hv, E, _stream()))
        torch.cuda.synchronize()
        return att, pooled

    def backward(att, pooled, drop=None):
        dsrc = mk(F * B, Hs, Hs + pad)
        o = {"dvals": None if (shared or drop == "dvals") else mk(F * B, Hv, Hv + pad),
             "dW1": None if drop == "dW1" else mk(Hs, E), "db1": None if drop == "db1" else mk(1, E),
             "dextra": None if drop == "dextra" else mk(B * F, E)}
        L.check(lib.yt8m_smattn_bwd(P(src_d), LD(src_d), P(vals_d), LD(vals_d), P(W1_d), _p(valid_d), _p(lo_d), _p(hi_d), P(att), P(pooled),
                                    P(G_d), P(dsrc), LD(dsrc), P(o["dvals"]), LD(o["dvals"]), P(o["dW1"]), P(o["db1"]), P(o["dextra"]), P(ws),
                                    need, B, F, Hs, Hv, E, _stream()))
        torch.cuda.synchronize()
        return dict(o, dsrc=dsrc)

    att, pooled = forward()
    out = backward(att, pooled)
    got = {"att": att.get((B, F, E)), "pooled": pooled.get((B, E, Hv)), "dsrc": out["dsrc"].get((F, B, Hs)), "dW1": out["dW1"].get((Hs, E)),
           "db1": out["db1"].get((E,)), "dextra": out["dextra"].get((B, F, E))}
    if not shared:
        got["dvals"] = out["dvals"].get((F, B, Hv))
    for name, g in [("src", src_d), ("vals", vals_d), ("W1", W1_d), ("b1", b1_d), ("extra", extra_d), ("G", G_d), ("att", att),
                    ("pooled", pooled), ("workspace", ws)] + list(out.items()):
        assert g is None or g.intact(), "guard words of %s" % name
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    if extra is None:                                                            # dextra = dz is written with or without an extra
        r64, r32 = dict(r64), dict(r32)
        for r, dt in ((r64, torch.float64), (r32, torch.float32)):
            zero = R.op_with_grads(np.where(np.isnan(src), 0, src), None if shared else np.where(np.isnan(vals), 0, vals), W1, b1,
                                   np.zeros((B, F, E), np.float32), valid, lo, hi, G, dt)
            r["dextra"] = zero["dextra"]
    _report("smattn C ABI %s %s %s:" % (_ids(shape), mask, variant), got, {k: r64[k] for k in got}, r32)
    # exact zeros: att and dextra where the mask is, the rows of dsrc and dvals that no head unmasks, all of an empty (b, e)
    masked = torch.from_numpy(~m).to(dev)                                        # [B,F,E]
    dead = torch.from_numpy(~row_live).to(dev)                                   # [F,B]
    empty = torch.from_numpy(~m.any(axis=1)).to(dev)                             # [B,E]
    assert masked.any() and (dead.any() or (B == 2 and mask == "window"))      # (two full videos' windows cover every frame)
    assert float(got["att"][masked].abs().sum()) == 0.0 and float(got["dextra"][masked].abs().sum()) == 0.0
    assert float(got["dsrc"][dead].abs().sum()) == 0.0 and float(got["pooled"][empty].abs().sum()) == 0.0
    assert float(got["db1"].abs().sum()) == 0.0          # b1 shifts all logits of a head alike: the kernels write its exact derivative, 0
    if not shared:
        assert float(got["dvals"][dead].abs().sum()) == 0.0
    if mask == "edges" or (mask in ("frames", "both") and (nf == 0).any()):
        assert empty.any()
    sums = got["att"].sum(dim=1)
    assert float((sums[~empty] - 1.0).abs().max()) <= 1e-5
    # a second run is bit-equal; so is every run with one optional output left NULL
    same = lambda a, b: torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))
    att2, pooled2 = forward()
    assert same(att, att2) and same(pooled, pooled2)
    for drop in (None, "dvals", "dW1", "db1", "dextra"):
        if drop == "dvals" and shared:
            continue
        out2 = backward(att2, pooled2, drop)
        for k, g in out2.items():
            assert (g is None) == (k == drop or (k == "dvals" and shared)), (drop, k)
            assert g is None or same(g, out[k]), (drop, k)
    assert ws.intact()


def test_refused_shapes_launch_nothing(dev):
    """A shape yt8m_smattn_supported refuses: YT8M_E_SHAPE and the outputs keep their sentinel."""
    lib = L.lib()
    F, B, Hs, E = 4, 3, 130, 1
    assert not lib.yt8m_smattn_supported(B, F, Hs, Hs, E)
    src, W1, b1 = _Guarded(dev, F * B, Hs), _Guarded(dev, Hs, E), _Guarded(dev, 1, E)
    att, pooled, ws = _Guarded(dev, B * F, E), _Guarded(dev, B * E, Hs), _Guarded(dev, 1, 1 << 16)
    rc = lib.yt8m_smattn_fwd(_p(src.flat), Hs, _p(src.flat), Hs, _p(W1.flat), _p(b1.flat), None, None, None, None, _p(att.flat), _p(pooled.flat),
                             _p(ws.flat), 4 << 16, B, F, Hs, Hs, E, _stream())
    torch.cuda.synchronize()
    assert rc == -2
    assert bool((att.buf == SENTINEL).all()) and bool((pooled.buf == SENTINEL).all()) and bool((ws.buf == SENTINEL).all())


# ---- seq_ops.softmax_attention_tm on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["kernels", "composed"])
@pytest.mark.parametrize("shape", [(33, 17, 516, 260, 3), (33, 17, 516, None, 3)], ids=_ids)
def test_op_fused_against_composed(dev, monkeypatch, fused, shape):
    """seq_ops.softmax_attention_tm with both masks and an extra through autograd, on the kernels (SOFTMAX_ATTENTION_CALLS shows that they
    ran) and with YT8M_SOFTMAX_ATTENTION_FUSED=0's composed form, two value tensors and the shared mode (one gradient): both against fp64."""
    F, B, Hs, Hv, E = shape
    shared = Hv is None
    nf, src, vals, W1, b1, extra, valid, lo, hi, G, m, ref = _abi_case(shape, "both", "plain")
    monkeypatch.setattr(seq_ops, "SOFTMAX_ATTENTION_FUSED", fused)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ts, tW, tb, tx = (d(a).requires_grad_(True) for a in (src, W1, b1, extra))
    tv = ts if shared else d(vals).requires_grad_(True)
    before = dict(seq_ops.SOFTMAX_ATTENTION_CALLS)
    att, pooled = seq_ops.softmax_attention_tm(ts, tW, tb, tv, extra=tx, valid=d(valid), lo=d(lo), hi=d(hi))
    took = "kernels" if fused else "composed"
    assert seq_ops.SOFTMAX_ATTENTION_CALLS == dict(before, **{took: before[took] + 1})
    assert not att.requires_grad
    (pooled * d(G)).sum().backward()
    torch.cuda.synchronize()
    got = {"att": att, "pooled": pooled, "dsrc": ts.grad, "dW1": tW.grad, "db1": tb.grad, "dextra": tx.grad}
    if not shared:
        got["dvals"] = tv.grad
    r64, r32 = ref[torch.float64], ref[torch.float32]
    if fused:
        _report("softmax_attention_tm %s kernels:" % _ids(shape), got, {k: r64[k] for k in got}, r32)
    else:                                   # the composed form runs through the library's GEMMs and pooling kernels: the gate tests' bound
        for k in got:
            e = R.err(got[k], r64[k])
            print("softmax_attention_tm composed %s %.2g (fp32 %.2g)" % (k, e, R.err(r32[k], r64[k])))
            assert e <= max(8.0 * R.err(r32[k], r64[k]), GRAD_FLOOR if k.startswith("d") else OUT_FLOOR), k


# ---- the plugins through create_model -------------------------------------------------------------------------------------------------
B_, F_, H_, V_, M_, E_ = 5, 9, 256, 32, 2, 3
CASES = [("LstmExtendModel", "MoeExtendModel", 1), ("LstmExtendModel", "MoeExtendModel", 2), ("InputExtendModel", "MoeExtendModel", 2),
         ("LstmExtendModel", "MoeExtendDistillChainModel", 2)]
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
        if k.endswith("biases") or k in ("b1", "b2"):
            vals[k] = (0.1 * rs.randn(*s)).astype(np.float32)
        elif k in ("W1", "W2"):
            vals[k] = (4.0 * rs.randn(*s) / np.sqrt(s[0])).astype(np.float32)
        else:
            vals[k] = (rs.randn(*s) * (0.2 if k.startswith(("gates", "experts")) else 1.0 / np.sqrt(s[0]))).astype(np.float32)
    return vals


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "floats"])
@pytest.mark.parametrize("name,head,layers", CASES)
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, head, layers, u8):
    """Each plugin with its head through TrainGraph.forward / loss / backward at B = 5, F = 9, 256 cells, E = 3, V = 32, 2 mixtures, on the
    reader's bytes (D = 1152) and on float frames (D = 64), with the kernels engaged: predictions, loss and the gradient of EVERY variable
    (and LstmExtendModel's attention_weight) against the restatement followed by CrossEntropyLoss in fp64."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    monkeypatch.setattr(seq_ops, "SOFTMAX_ATTENTION_FUSED", True)
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures, flags.moe_num_extend = str(H_), layers, M_, E_
    flags.video_level_classifier_model = head
    distill = head == "MoeExtendDistillChainModel"
    rs, D, nf, x_in, x64, y = _plugin_inputs(u8, 60 + layers)
    dp = rs.rand(B_, V_).astype(np.float32) if distill else None
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(getattr(flm, name)(), batch_size=B_, graph=g)
    args = (torch.from_numpy(x_in).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    kw = dict(distillation_predictions=torch.from_numpy(dp).to(dev)) if distill else {}
    if u8:
        assert flm._lib_u8_ok(D) and seq_ops.u8_attention_supported(args[0], E_), "the shape of this case must take the byte path"
    tg.forward(*args, **kw)
    g.finalize()
    shapes = R.variable_shapes(name, head, D, H_, layers, E_, V_, M_, distill=distill)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(shapes.items())
    vals = _trained_values(rs, shapes)
    for k, v in vals.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev))
    before = dict(seq_ops.SOFTMAX_ATTENTION_CALLS)
    res = tg.forward(*args, **kw)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    assert seq_ops.SOFTMAX_ATTENTION_CALLS == dict(before, kernels=before["kernels"] + 1)

    def pipeline(dtype):
        tp = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in vals.items()}
        x = torch.from_numpy(x64).to(dtype)
        pooled, aw = R.BODIES[name](x, torch.from_numpy(nf), tp, layers, E_)
        dl = None if dp is None else torch.from_numpy(dp).to(dtype)
        p = R.moe_extend_distill_chain_model(pooled, tp, M_, E_, dl) if distill else R.moe_extend_model(pooled, tp, M_, E_)
        lr = R.cross_entropy(p, torch.from_numpy(y))
        lr.backward()
        out = {"predictions": p.detach().numpy(), "loss": np.array([float(lr.detach())]), "attention_weight": aw.detach().numpy()}
        out.update({"d:" + k: t.grad.numpy() for k, t in tp.items()})
        return out

    r64, r32 = pipeline(torch.float64), pipeline(torch.float32)
    got = {"predictions": res["predictions"], "loss": loss.detach().view(1)}
    if name == "LstmExtendModel":
        got["attention_weight"] = res["attention_weight"]
        assert tuple(got["attention_weight"].shape) == (B_, E_ * F_)
    else:
        del r64["attention_weight"], r32["attention_weight"]
    got.update({"d:" + k: v.grad for k, v in g.vars.items()})
    bound = R.bounds(r64, r32, lambda k: GRAD_FLOOR if k.startswith("d") else OUT_FLOOR)
    e = {k: R.err(got[k], r64[k]) for k in r64}
    print("%s + %s layers=%d %s:" % (name, head, layers, "bytes" if u8 else "floats"),
          " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % (k, e[k], R.err(r32[k], r64[k]), bound[k]) for k in r64))
    bad = [(k, e[k], bound[k]) for k in r64 if not e[k] <= bound[k]]
    assert not bad, bad
    for k in vals:
        assert float(np.abs(r64["d:" + k]).max()) > 0.0, k                         # every variable takes part
