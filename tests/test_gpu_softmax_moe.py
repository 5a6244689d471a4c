"""-m gpu: the label-softmax mixture kernels and the split softmax loss kernel (csrc/softmax_moe.hip; ops.softmax_moe,
ops.split_softmax_loss), Z's MoeSoftmaxModel and losses.SplitSoftmaxLoss against the fp64 restatement (tests/softmax_moe_restatement.py).

Bounds.  The measure is max |got - ref| / max(1, max |ref|) against the fp64 restatement on the same float32 inputs, as
tests/test_gpu_mix_chain.py.  For the ops' own quantities (out, stats, dZg, dZe, the loss and dp through the C ABI; the same and dhead
through autograd, in both forms) the bound is ensemble_restatement.bound in that measure: FOUR times the error of the float32
restatement (plain torch on the CPU, in the reference's form) against the float64 one plus one float32 ulp of the largest reference
magnitude.  It is never derived from the kernels' output.  Every case prints the measured errors with the float32 restatement's beside
them and asserts that the float32 restatement is finite.  WIDER names the quantities that get the gate tests' factor 8 and floors
(2e-6 outputs, 5e-6 gradients) instead, with the reason: the plugin's quantities, which sit behind the MoE products.

The loss cases keep the appended probability 1 - sum >= 0.05, where the reference's formula (which the restatement is, without the
product's clamp) is finite in float32; the clamp itself is pinned on the CPU (tests/test_softmax_moe_host.py) and, for the kernel, by
test_the_kernel_clamps_the_appended_probability against the restatement's clamp=True form.

q sums to 1 in the extreme kind (the dropped label holds no mass) within 2e-6: T is a float32 sum of S terms in a tree of depth
8 + S / 256 (at most 15 roundings of 2^-24 at S = 1793) and each q is rounded once more.

Measured on an MI355X (largest error per quantity, the float32 restatement's error of the same case in brackets):
  softmax_moe through the C ABI, the 33 cases: out 7.4e-8 [4.5e-8], stats 9.1e-8 [5.2e-8], dZg 5.9e-8 [8.9e-8], dZe 7.6e-8 [1.6e-8] (0.81 of
    its bound at (1, 2, 1, 0) misaligned, the nearest approach; the head's columns and the column maxima are bit-exact)
  through autograd, kernels: out 3.0e-8, dZg 2.5e-8 [1.8e-8], dZe 3.5e-8 [5.4e-8], dhead is dout's columns bit for bit; composed: out
    4.7e-8 [7.7e-8]
  split_softmax_loss through the C ABI, the 10 cases: loss 8.6e-8 [2.3e-8] (0.43 of its bound), dp 2.5e-7 [2.5e-7]; through autograd on a
    window: loss 1.1e-7 [9.2e-8], dp 7.7e-8 [2.5e-8]; the clamped row: loss 5.5e-8 [1.4e-8], dp 8.7e-8 [8.7e-8]
  the 8 model cases, on the wider rule: predictions 9.0e-8 [8.7e-8], predictions_class 1.0e-7 [9.5e-8], loss 6.5e-8 [1.1e-9] (kernels,
    SplitSoftmaxLoss, workload: 0.03 of the floor), gradients 2.7e-6 [8.5e-6] (class_experts biases under SplitSoftmaxLoss, whose
    reference gradient is large: 0.04 of 8 x the float32 restatement's error)
"""
import functools

import numpy as np
import pytest
import torch

import softmax_moe_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.train  # noqa: F401
import yt8m_amd.video_level_models  # noqa: F401  (defines the flags the model reads)
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
_PRODUCTS = ("a plugin quantity: behind the MoE heads' and the class blocks' products, which the device runs K-split and, where they are "
             "large, as three f16 products with 2^-21 per term under per-operand scales -- none of which the float32 restatement on the "
             "CPU draws (the reason of tests/test_gpu_mix_chain.py and tests/test_gpu_distill_head.py)")
WIDER = {"predictions": _PRODUCTS, "predictions_class": _PRODUCTS, "model loss": _PRODUCTS, "gradient": _PRODUCTS}
GUARD = 16            # floats around every buffer
SENTINEL = -1234.5


def _bound(name, r32, r64):
    ref64 = torch.as_tensor(np.asarray(r64, dtype=np.float64))
    ref32 = torch.as_tensor(np.asarray(r32, dtype=np.float64))
    assert bool(torch.isfinite(ref32).all()), name
    big = max(1.0, float(ref64.abs().max()) if ref64.numel() else 0.0)
    if name in WIDER:
        return max(8.0 * R.err(r32, r64), GRAD_FLOOR if name == "gradient" else OUT_FLOOR)
    return R.bound(ref32, ref64) / big


def _report(tag, got, ref64, ref32, kind=None):
    """prints measured / float32-restatement errors and bounds per quantity, then asserts every one of them"""
    rows = [(k, R.err(got[k], ref64[k]), R.err(ref32[k], ref64[k]), _bound(kind or k, ref32[k], ref64[k])) for k in got]
    print(tag, " ".join("%s %.2g (fp32 %.2g, bound %.2g)" % r for r in rows))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, (tag, bad)


def _np(d):
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


class _Guarded(object):
    """A device buffer of n floats between GUARD sentinel floats, `off` floats past a 16-byte boundary; everything is sentinel until
    written, and what is not operand must stay so."""

    def __init__(self, dev, n, off=0, data=None):
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD + off:GUARD + off + n]
        assert self.view.data_ptr() % 16 == 4 * off
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).view(-1))
        self.n, self.off = n, off

    def intact(self):
        lo = GUARD + self.off
        return bool((self.buf[:lo] == SENTINEL).all()) and bool((self.buf[lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def written(self):
        return bool((self.view != SENTINEL).all())


# ---- the head kernels through the C ABI ---------------------------------------------------------------------------------------------------
# (rows, S, M, V1): one row, the smallest S and M, no head; fewer labels than lanes; a partial last wave; exactly one wave; one label more
# than a wave, M = 8; more than one pass per thread; the workload row; the two sizes either side of the register-resident threshold
# S <= 256 * (36 / (M + 1)) at M = 4 (1792 | 1793) and at M = 8 (1024 | 1025): above it every pass reads the logits again
MOE_SHAPES = [(1, 2, 1, 0), (3, 7, 2, 1), (5, 63, 3, 10), (2, 64, 4, 0), (2, 65, 8, 3), (3, 257, 3, 37), (2, 1717, 4, 3000), (2, 1792, 4, 5),
              (2, 1793, 4, 5), (1, 1024, 8, 0), (1, 1025, 8, 2)]
MOE_KINDS = ["plain", "misaligned", "extreme"]


def _moe_case(rows, S, M, V1, kind):
    rs = np.random.RandomState(1000 * rows + S + 10 * M + V1 + len(kind))
    Zg = (2 * rs.randn(rows, S, M + 1)).astype(np.float32)
    Ze = (2 * rs.randn(rows, S, M)).astype(np.float32)
    if kind == "extreme":
        Ze[:, :, M - 1] = 0.5                                              # one mixture with all-equal logits
        Ze[:, 0, 0] = 80.0                                                 # one expert logit at +80
        Ze[:, S - 1, :] = -1e4                                             # the dropped label holds zero mass: q sums to 1
    head = rs.rand(rows, V1).astype(np.float32) if V1 else None
    dout = rs.randn(rows, V1 + S - 1).astype(np.float32)
    return Zg.reshape(rows, -1), Ze.reshape(rows, -1), head, dout


@functools.lru_cache(maxsize=None)
def _moe_refs(rows, S, M, V1, kind):
    case = _moe_case(rows, S, M, V1, kind)
    Zg, Ze, head, dout = case
    return case, _np(R.kernel_with_grads(Zg, Ze, head, S, M, dout, torch.float64)), _np(R.kernel_with_grads(Zg, Ze, head, S, M, dout, torch.float32))


@pytest.mark.parametrize("kind", MOE_KINDS)
@pytest.mark.parametrize("rows,S,M,V1", MOE_SHAPES)
def test_softmax_moe_through_the_c_abi(dev, rows, S, M, V1, kind):
    lib = L.lib()
    assert lib.yt8m_softmax_moe_supported(S, M) == 1
    assert lib.yt8m_softmax_moe_resident(S, M) == int(S <= 256 * (36 // (M + 1)))
    (Zg, Ze, head, dout), r64, r32 = _moe_refs(rows, S, M, V1, kind)
    W = V1 + S - 1
    offs = {"Zg": 1, "Ze": 2, "head": 3, "dout": 1, "out": 3, "stats": 2, "dZg": 1, "dZe": 3} if kind == "misaligned" else {}
    new = lambda name, n, data=None: _Guarded(dev, n, offs.get(name, 0), data)
    hb = new("head", rows * V1, head) if V1 else None
    gb = new("dout", rows * W, dout)

    def run(inplace=False, pitch=0):
        zb, eb = new("Zg", Zg.size, Zg), new("Ze", Ze.size, Ze)
        out, stats = new("out", rows * W), new("stats", rows * (2 * M + 1))
        dzg, dze = (zb, eb) if inplace else (new("dZg", Zg.size), new("dZe", Ze.size))
        g = gb
        if pitch:                                                          # dout inside wider rows
            wide = np.full((rows, W + pitch), 7.5, dtype=np.float32)
            wide[:, 2:2 + W] = dout
            g = new("dout", wide.size, wide)
        L.check(lib.yt8m_softmax_moe_fwd(_p(zb.view), _p(eb.view), _p(hb.view) if V1 else None, _p(out.view), _p(stats.view), rows, S, M, V1,
                                         _stream()))
        L.check(lib.yt8m_softmax_moe_bwd(_p(zb.view), _p(eb.view), _p(stats.view), _p(g.view), W + pitch, V1 + (2 if pitch else 0),
                                         _p(dzg.view), _p(dze.view), rows, S, M, _stream()))
        torch.cuda.synchronize()
        for b in (zb, eb, out, stats, dzg, dze, g):
            assert b.intact()
        if not inplace:                                                    # the operands are only read
            assert torch.equal(zb.view.cpu(), torch.from_numpy(Zg).view(-1)) and torch.equal(eb.view.cpu(), torch.from_numpy(Ze).view(-1))
        return out, stats, dzg, dze

    outs = run()
    out, stats, dzg, dze = outs
    for b in outs:
        assert b.written()                                                 # every element of every output was overwritten
    assert (hb is None or hb.intact()) and gb.intact() and torch.equal(gb.view.cpu(), torch.from_numpy(dout).view(-1))
    got = {"out": out.view.cpu().view(rows, W), "stats": stats.view.cpu().view(rows, 2 * M + 1), "dZg": dzg.view.cpu().view(rows, -1),
           "dZe": dze.view.cpu().view(rows, -1)}
    _report("softmax_moe c abi (%d,%d,%d,%d) %s:" % (rows, S, M, V1, kind), got, r64, r32)
    if V1:
        assert torch.equal(got["out"][:, :V1], torch.from_numpy(head))     # the head is copied bit for bit
    assert torch.equal(got["stats"][:, :M].double(), torch.from_numpy(r64["stats"][:, :M]))         # the column maxima are exact
    q = got["out"][:, V1:].double()
    assert bool((q >= 0).all()) and bool((q.sum(1) <= 1 + 2e-6).all())
    if kind == "extreme":
        assert float((q.sum(1) - 1).abs().max()) <= 2e-6
        assert bool(torch.isfinite(got["dZg"]).all()) and bool(torch.isfinite(got["dZe"]).all())
    # a second run gives the same bits; so do gradients written over the logits, and a dout read inside wider rows
    for other in (run(), run(inplace=True), run(pitch=5)):
        assert all(torch.equal(a.view, b.view) for a, b in zip(other, outs))


def test_refused_softmax_moe_arguments_launch_nothing(dev):
    lib = L.lib()
    b = [_Guarded(dev, 4096, 0, np.zeros(4096)) for _ in range(4)]
    outs = [_Guarded(dev, 4096) for _ in range(4)]
    fwd = lambda rows=2, S=8, M=3, V1=4, head=b[2]: lib.yt8m_softmax_moe_fwd(_p(b[0].view), _p(b[1].view), None if head is None else _p(head.view),
                                                                               _p(outs[0].view), _p(outs[1].view), rows, S, M, V1, _stream())
    assert fwd(rows=0) == -2 and fwd(S=1) == -2 and fwd(S=65537) == -2 and fwd(M=0) == -2 and fwd(M=9) == -2 and fwd(V1=-1) == -2
    assert fwd(head=None) == -1 and fwd(V1=0) == -1
    bwd = lambda S=8, M=3, ldd=11, c0=4: lib.yt8m_softmax_moe_bwd(_p(b[0].view), _p(b[1].view), _p(b[2].view), _p(b[3].view), ldd, c0,
                                                                  _p(outs[2].view), _p(outs[3].view), 2, S, M, _stream())
    assert bwd(S=1) == -2 and bwd(M=9) == -2 and bwd(ldd=10) == -1 and bwd(c0=-1) == -1
    loss = lambda B=2, V=8, bound=3, ldp=8, dt=1: lib.yt8m_split_softmax_loss_fwd_bwd(_p(b[0].view), ldp, 0, _p(b[1].view), dt, _p(outs[0].view),
                                                                                     _p(outs[1].view), B, V, bound, 1e-5, 1e-7, 1.0,
                                                                                     _p(outs[2].view), _stream())
    assert loss(B=0) == -2 and loss(bound=0) == -2 and loss(bound=8) == -2 and loss(ldp=7) == -1 and loss(dt=2) == -1
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---- the loss kernel through the C ABI ----------------------------------------------------------------------------------------------------
# (rows, V, bound): the smallest; the host shape; one infrequent label behind a wide sigmoid part; the workload; a wide softmax part
LOSS_SHAPES = [(1, 3, 1), (5, 37, 10), (3, 300, 299), (2, 4716, 3000), (2, 4716, 1000)]


def _loss_case(rows, V, bound, seed=0):
    rs = np.random.RandomState(rows + V + bound + seed)
    p = rs.rand(rows, V).astype(np.float64)
    p[:, bound:] *= (0.5 + 0.45 * rs.rand(rows, 1)) / p[:, bound:].sum(1, keepdims=True)      # the appended probability >= 0.05
    p = p.astype(np.float32)
    assert float((1 - p[:, bound:].astype(np.float64).sum(1)).min()) >= 0.05 - 1e-6
    y = rs.rand(rows, V) < (0.3 if V < 100 else 6.0 / V)
    y[0, bound:] = False                                                   # a row without infrequent labels
    if rows > 1:
        y[1] = False                                                       # a row with no labels at all
    if rows > 2:
        y[2, bound:] = True                                                # and one with every infrequent label
    return p, y


@functools.lru_cache(maxsize=None)
def _loss_refs(rows, V, bound, dtype):
    p, y = _loss_case(rows, V, bound)
    y = y.astype(dtype)
    if dtype == np.float32:
        y = (y * np.random.RandomState(V).rand(rows, V)).astype(np.float32)            # soft labels, as the distillation blends hand over
    return (p, y), _np(R.loss_with_grads(p, y, bound, torch.float64)), _np(R.loss_with_grads(p, y, bound, torch.float32))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
@pytest.mark.parametrize("rows,V,bound", LOSS_SHAPES)
def test_split_softmax_loss_through_the_c_abi(dev, rows, V, bound, dtype):
    lib = L.lib()
    (p, y), r64, r32 = _loss_refs(rows, V, bound, dtype)
    assert np.isfinite(float(r32["loss"]))
    ldp, c0 = V + 3, 2                                                     # p inside wider rows: a nonzero pitch and column start
    wide = np.full((rows, ldp), 0.25, dtype=np.float32)
    wide[:, c0:c0 + V] = p
    pb = _Guarded(dev, wide.size, 1, wide)
    yt = torch.from_numpy(y).to(dev)
    ldt = 0 if dtype == np.uint8 else 1
    ws = _Guarded(dev, lib.yt8m_split_softmax_loss_workspace_bytes(rows) // 4)
    up = torch.full((1,), 0.5, dtype=torch.float32, device=dev)

    def run():
        loss, dp, dp2 = _Guarded(dev, 1), _Guarded(dev, rows * V, 3), _Guarded(dev, rows * V, 1)
        L.check(lib.yt8m_split_softmax_loss_fwd_bwd(_p(pb.view), ldp, c0, _p(yt), ldt, _p(loss.view), _p(dp.view), rows, V, bound, 10e-6, 10e-8,
                                                    1.0, _p(ws.view), _stream()))
        L.check(lib.yt8m_split_softmax_loss_bwd(_p(pb.view), ldp, c0, _p(yt), ldt, _p(up), _p(dp2.view), rows, V, bound, 10e-6, 10e-8, 2.0,
                                                _stream()))
        torch.cuda.synchronize()
        for b in (loss, dp, dp2, ws, pb):
            assert b.intact()
        return loss, dp, dp2

    loss, dp, dp2 = run()
    assert dp.written() and dp2.written() and torch.equal(pb.view.cpu(), torch.from_numpy(wide).view(-1))
    got = {"loss": loss.view.cpu()[0], "dp": dp.view.cpu().view(rows, V)}
    _report("split_softmax_loss c abi (%d,%d,%d) %s:" % (rows, V, bound, np.dtype(dtype).name), got, r64, r32)
    assert torch.equal(dp2.view, dp.view)                                  # 2.0 * 0.5 upstream, read on the device: the same bits
    assert all(torch.equal(a.view, b.view) for a, b in zip(run(), (loss, dp, dp2)))       # a second run gives the same bits
    # the value alone (dp NULL) is the same value
    loss2 = _Guarded(dev, 1)
    L.check(lib.yt8m_split_softmax_loss_fwd_bwd(_p(pb.view), ldp, c0, _p(yt), ldt, _p(loss2.view), None, rows, V, bound, 10e-6, 10e-8, 1.0,
                                                _p(ws.view), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(loss2.view, loss.view)


def test_the_kernel_clamps_the_appended_probability(dev):
    """The host test's row (float32 sum 1 + 2^-23 over the softmax part): finite, and the restatement's clamp=True form."""
    p = np.zeros((2, 8), dtype=np.float32)
    p[:, :3] = 0.3
    p[0, 3:5] = np.float32(0.5), np.float32(0.5) + np.float32(2.0 ** -23)
    p[1, 3:] = 0.1
    y = np.zeros((2, 8), dtype=bool)
    y[0, 4] = y[1, 5] = True
    pt = torch.from_numpy(p).to(dev).requires_grad_(True)
    before = dict(ops.SPLIT_SOFTMAX_LOSS_CALLS)
    saved, ops.SPLIT_SOFTMAX_LOSS_FUSED = ops.SPLIT_SOFTMAX_LOSS_FUSED, True
    try:
        loss = ops.split_softmax_loss(pt, torch.from_numpy(y).to(dev), 3)
    finally:
        ops.SPLIT_SOFTMAX_LOSS_FUSED = saved
    assert ops.SPLIT_SOFTMAX_LOSS_CALLS == dict(before, kernels=before["kernels"] + 1)
    loss.backward()
    r64, r32 = (R.loss_with_grads(p, y, 3, dt, clamp=True) for dt in (torch.float64, torch.float32))
    assert not np.isfinite(float(R.loss_with_grads(p, y, 3, torch.float32)["loss"]))    # the reference's formula
    _report("clamped row:", {"loss": loss.detach().cpu(), "dp": pt.grad.cpu()}, _np(r64), _np(r32))


# ---- both ops through autograd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,S,M,V1", [(5, 28, 3, 10), (3, 1717, 4, 3000), (2, 1793, 4, 0)])
def test_softmax_moe_autograd_fused_and_composed_against_the_restatement(dev, monkeypatch, rows, S, M, V1):
    (Zg, Ze, head, dout), r64, r32 = _moe_refs(rows, S, M, V1, "plain")
    d = lambda a: torch.from_numpy(a).to(dev)
    runs = {}
    for fused, overwrite in ((True, False), (True, True), (False, False)):
        monkeypatch.setattr(ops, "SOFTMAX_MOE_FUSED", fused)
        key = "kernels" if fused else "composed"
        for rep in range(2):
            zg, ze = d(Zg).requires_grad_(True), d(Ze).requires_grad_(True)
            h = d(head).requires_grad_(True) if V1 else None
            before = dict(ops.SOFTMAX_MOE_CALLS)
            out = ops.softmax_moe(zg * 1.0, ze * 1.0, S, M, head=h, overwrite_logits=overwrite)       # (the op's own logits: not the leaves)
            assert ops.SOFTMAX_MOE_CALLS == dict(before, **{key: before[key] + 1})
            out.backward(d(dout))
            torch.cuda.synchronize()
            got = {"out": out.detach().cpu(), "dZg": zg.grad.cpu(), "dZe": ze.grad.cpu()}
            if V1:
                got["dhead"] = h.grad.cpu()
            if rep:
                assert all(torch.equal(got[k], runs[(fused, overwrite)][k]) for k in got)       # two runs: the same bits
            runs[(fused, overwrite)] = got
        _report("softmax_moe autograd (%d,%d,%d,%d) %s%s:" % (rows, S, M, V1, key, " overwrite" if overwrite else ""), got,
                {k: r64[k] for k in got}, r32)
    assert all(torch.equal(runs[(True, True)][k], v) for k, v in runs[(True, False)].items())


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.float32], ids=["bool", "uint8", "float32"])
@pytest.mark.parametrize("rows,V,bound", [(5, 37, 10), (2, 4716, 3000)])
def test_split_softmax_loss_autograd_fused_and_composed_on_a_window(dev, monkeypatch, rows, V, bound, dtype):
    """p is a column window of a wider tensor, as a piece of predictions_class is; scale = 0.1 as calculate_loss_mix passes it."""
    p, y = _loss_case(rows, V, bound, seed=3)
    labels = torch.from_numpy(y).to(dev).to(dtype)
    r64, r32 = (_np(R.loss_with_grads(p, y, bound, dt, scale=0.1)) for dt in (torch.float64, torch.float32))
    wide = np.full((rows, 2 * V + 1), 0.5, dtype=np.float32)
    wide[:, V:2 * V] = p
    for fused in (True, False):
        monkeypatch.setattr(ops, "SPLIT_SOFTMAX_LOSS_FUSED", fused)
        key = "kernels" if fused else "composed"
        runs = []
        for rep in range(2):
            wt = torch.from_numpy(wide).to(dev).requires_grad_(True)
            before = dict(ops.SPLIT_SOFTMAX_LOSS_CALLS)
            loss = ops.split_softmax_loss(wt[:, V:2 * V], labels, bound, scale=0.1)
            assert ops.SPLIT_SOFTMAX_LOSS_CALLS == dict(before, **{key: before[key] + 1})
            loss.backward()
            torch.cuda.synchronize()
            g = wt.grad.cpu()
            assert float(g[:, :V].abs().max()) == 0.0 and float(g[:, 2 * V:].abs().max()) == 0.0
            runs.append({"loss": loss.detach().cpu(), "dp": g[:, V:2 * V]})
        assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
        _report("split_softmax_loss autograd (%d,%d,%d) %s:" % (rows, V, bound, key), runs[0], r64, r32)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
MODEL_SHAPES = {"host": (5, 36, 37, 10, 3, 7, 3), "workload": (16, 1152, 4716, 3000, 4, 100, 2)}       # B, D, V, bound, M, C, layers


@functools.lru_cache(maxsize=None)
def _model_case(shape):
    B, D, V, V1, M, C, layers = MODEL_SHAPES[shape]
    rs = np.random.RandomState(60 + B)
    x = rs.randn(B, D).astype(np.float32)
    if D > 100:
        x /= np.linalg.norm(x, axis=1, keepdims=True)                     # video-level features are l2-normalised
    y = rs.rand(B, V) < (0.2 if V < 100 else 3.4 / V)
    if V > 100:
        y[0, V1 + 5] = True                                                # at least one infrequent label in the batch
    return x, y, R.draw(R.variable_shapes(D, V, V1, M, C, layers), rs)


@functools.lru_cache(maxsize=None)
def _model_refs(shape, loss_name):
    B, D, V, V1, M, C, layers = MODEL_SHAPES[shape]
    x, y, P = _model_case(shape)
    return tuple(R.reference(x, y, P, M, C, layers, V1, dt, loss_name) for dt in (torch.float64, torch.float32))


def _train_graph(dev, B, loss_name):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=dev, seed=0)
    return g, train.TrainGraph(vlm.MoeSoftmaxModel(), label_loss_fn=getattr(losses, loss_name)(), batch_size=B, graph=g,
                               transformer_class=ft.IdenticalTransformer)


def _load(g, P, dev):
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    torch.cuda.synchronize()


def _grads(g):
    return {k: (v.grad if v.grad_written else torch.zeros_like(v.grad)).detach().cpu() for k, v in g.vars.items() if v.trainable}


def _set(flags, shape):
    B, D, V, V1, M, C, layers = MODEL_SHAPES[shape]
    flags.moe_num_mixtures, flags.class_size, flags.moe_layers, flags.softmax_bound = M, C, layers, V1


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("loss_name", ["CrossEntropyLoss", "SplitSoftmaxLoss"])
@pytest.mark.parametrize("shape", ["host", "workload"])
def test_model_matches_the_fp64_restatement_on_the_device(dev, flags, monkeypatch, shape, loss_name, fused):
    """--model=MoeSoftmaxModel through TrainGraph.forward / loss / backward under either --label_loss: predictions, predictions_class,
    the training loss and every Variable's gradient; the features are data, as in video-level use."""
    monkeypatch.setattr(ops, "SOFTMAX_MOE_FUSED", fused)
    monkeypatch.setattr(ops, "SPLIT_SOFTMAX_LOSS_FUSED", fused)
    B, D, V, V1, M, C, layers = MODEL_SHAPES[shape]
    _set(flags, shape)
    x, y, P = _model_case(shape)
    r64, r32 = _model_refs(shape, loss_name)
    g, tg = _train_graph(dev, B, loss_name)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    tg.forward(*args)
    assert list(g.vars) == list(P)
    _load(g, P, dev)
    before = dict(ops.SOFTMAX_MOE_CALLS), dict(ops.SPLIT_SOFTMAX_LOSS_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    form = "kernels" if fused else "composed"
    assert ops.SOFTMAX_MOE_CALLS == dict(before[0], **{form: before[0][form] + layers + 1})
    n_loss = layers + 1 if loss_name == "SplitSoftmaxLoss" else 0
    assert ops.SPLIT_SOFTMAX_LOSS_CALLS == dict(before[1], **{form: before[1][form] + n_loss})
    tag = "MoeSoftmaxModel %s %s %s:" % (shape, loss_name, form)
    got = {"predictions": res["predictions"].detach().cpu(), "predictions_class": res["predictions_class"].detach().cpu()}
    assert tuple(got["predictions_class"].shape) == (B, layers * V)
    _report(tag, got, {k: r64[k].numpy() for k in got}, {k: r32[k].numpy() for k in got})
    _report(tag, {"loss": loss.detach().cpu()}, {"loss": r64["loss"].numpy()}, {"loss": r32["loss"].numpy()}, kind="model loss")
    grads = _grads(g)
    assert set(grads) == set(r64["grads"])
    _report(tag + " gradients", grads, _np(r64["grads"]), _np(r32["grads"]), kind="gradient")
    for k in grads:
        assert float(grads[k].abs().max()) > 0, k


def test_one_training_step_of_moe_softmax_model_under_split_softmax_loss(dev, flags):
    """TrainGraph.step on the device's own clip + Adam pass reports the loss of forward / loss bit for bit and moves every Variable."""
    B = MODEL_SHAPES["host"][0]
    _set(flags, "host")
    x, y, P = _model_case("host")
    g, tg = _train_graph(dev, B, "SplitSoftmaxLoss")
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    tg.forward(*args)
    _load(g, P, dev)
    loss = tg.loss(tg.forward(*args), args[1]).detach()
    start = {k: v.data.clone() for k, v in g.vars.items()}
    out = tg.step(*args)
    torch.cuda.synchronize()
    assert float(out["loss"]) == float(loss)
    out2 = tg.step(*args)
    torch.cuda.synchronize()
    for k, v in g.vars.items():
        assert bool(torch.isfinite(v.data).all()) and not torch.equal(v.data, start[k]), k
    assert np.isfinite(float(out["loss"])) and float(out2["loss"]) < float(out["loss"])
