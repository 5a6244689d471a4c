"""The label losses of csrc/losses.hip on the MI355X against the fp64 restatement of tests/test_losses_host.py: the two batch-agreement
losses at the smallest shapes that reach each code path and on constructed batches (ties at the extrema, a tied 20th value, rows
without a positive inside the top 20, a separated batch), whole training steps under them, and the three pointwise losses.

Tolerance.  The composition of each loss from float32 torch ops (the same restatement, run in float32 on the CPU) is off from
the float64 one, over test_losses_host.SHAPES and both weight settings below, by at most

                      loss, relative      dL/dp, relative to max |dL/dp|
    BatchAgreement       1.15e-7                 2.27e-7
    TopKBatchAgreement   9.56e-8                 8.20e-8
    pointwise            1.14e-7                 1.03e-7

The kernels get 4 x those figures (they add in another order and take logf / expf from another library).  What decides a branch
is a comparison of float32 values of p with each other, which float64 repeats exactly: the extrema, the thresholds, the counts
and the numbers of tied elements the kernels leave in their statistics block must equal the restatement's, with no tolerance."""
import faulthandler
import functools

import numpy as np
import pytest
import torch

import yt8m_amd.feature_transform as ft
import yt8m_amd.losses as losses
import yt8m_amd.ops as ops
import yt8m_amd.train as train
import yt8m_amd.video_level_models as vlm
from yt8m_amd.variables import reset_default_graph
from test_losses_host import (SHAPES, batch_agreement_parts, batch_agreement_ref, case, hinge_ref, loss_and_grad,
                              mse_ref, smoothing_ref, topk_batch_agreement_parts, topk_batch_agreement_ref, weighted_xent_ref)

pytestmark = pytest.mark.gpu

FACTOR = 4.0
TOL = {"ba": (FACTOR * 1.15e-7, FACTOR * 2.27e-7), "tk": (FACTOR * 9.56e-8, FACTOR * 8.20e-8), "pw": (FACTOR * 1.14e-7, FACTOR * 1.03e-7)}
U = 2.0 ** -24
# (a, N): the flags' defaults, and weights of the order of the cross entropy itself (N = the number of rows)
SETTINGS = {"default": lambda B: (0.1, 1024.0), "heavy": lambda B: (0.5, float(B))}


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this module ends within a minute or takes the process down (a watchdog thread: it also ends a call that hangs
    inside the runtime, which a Python-level alarm cannot)."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _labels(y, lt, dev):
    return (y.to(torch.uint8) if lt == "u8" else y.to(torch.float32)).to(dev)


def _check(tag, kind, loss, dp, loss64, dp64):
    tol_l, tol_d = TOL[kind]
    el = abs(float(loss) - loss64) / abs(loss64)
    ed = float(np.abs(dp.detach().cpu().numpy().astype(np.float64) - dp64).max() / np.abs(dp64).max())
    print("%s: loss %.8g (fp64 %.8g) off by %.3g of it (bound %.3g); dL/dp off by %.3g of max |dL/dp| = %.3g (bound %.3g)"
          % (tag, float(loss), loss64, el, tol_l, ed, np.abs(dp64).max(), tol_d))
    assert el <= tol_l and ed <= tol_d


def _ba_stats_equal(stats, parts, y64, p64):
    """The statistics that decide the masks, bit for bit."""
    st = stats.cpu()
    S = ops.BA_STATS
    assert float(st[S["min_pp"]]) == float(parts["min_pp"]) and float(st[S["max_np"]]) == float(parts["max_np"])
    assert float(st[S["n_fn"]]) == float(parts["n_fn"]) and float(st[S["n_fp"]]) == float(parts["n_fp"])
    assert float(st[S["ties_max_np"]]) == float(((p64 * (1 - y64)) == parts["max_np"]).sum())
    assert float(st[S["ties_min_pp"]]) == float(((p64 * y64 + (1 - y64)) == parts["min_pp"]).sum())


@functools.lru_cache(maxsize=None)
def _ba_ref(B, V, setting):
    p, y = case(B, V)
    a, N = SETTINGS[setting](B)
    loss64, dp64 = loss_and_grad(batch_agreement_ref, p, y.double(), a, N)
    parts = {k: v.detach() for k, v in batch_agreement_parts(p.double(), y.double(), a, N).items()}
    dp64.setflags(write=False)
    return loss64, dp64, parts


@functools.lru_cache(maxsize=None)
def _tk_ref(B, V, setting):
    p, y = case(B, V)
    a, _ = SETTINGS[setting](B)
    loss64, dp64 = loss_and_grad(topk_batch_agreement_ref, p, y.double(), a)
    parts = {k: v.detach() for k, v in topk_batch_agreement_parts(p.double(), y.double(), a).items()}
    dp64.setflags(write=False)
    return loss64, dp64, parts


@pytest.mark.parametrize("setting", ["default", "heavy"])
@pytest.mark.parametrize("lt", ["u8", "f32"])
@pytest.mark.parametrize("B,V", SHAPES)
def test_batch_agreement_against_fp64(dev, B, V, lt, setting):
    p, y = case(B, V)
    a, N = SETTINGS[setting](B)
    loss64, dp64, parts = _ba_ref(B, V, setting)
    pd, yd = p.to(dev), _labels(y, lt, dev)
    loss, stats = ops.batch_agreement_fwd(pd, yd, a, N)
    dp = ops.batch_agreement_bwd(pd, yd, stats, torch.ones(1, device=dev))
    _ba_stats_equal(stats, parts, y.double(), p.double())
    _check("BatchAgreement [%d,%d] %s %s" % (B, V, lt, setting), "ba", loss, dp, loss64, dp64)


@pytest.mark.parametrize("setting", ["default", "heavy"])
@pytest.mark.parametrize("lt", ["u8", "f32"])
@pytest.mark.parametrize("B,V", SHAPES)
def test_topk_batch_agreement_against_fp64(dev, B, V, lt, setting):
    p, y = case(B, V)
    a, _ = SETTINGS[setting](B)
    loss64, dp64, parts = _tk_ref(B, V, setting)
    pd, yd = p.to(dev), _labels(y, lt, dev)
    loss, stats = ops.topk_batch_agreement_fwd(pd, yd, a)
    dp = ops.topk_batch_agreement_bwd(pd, yd, stats, torch.ones(1, device=dev), a)
    st = stats.cpu().double()
    assert float(st[0]) == float(parts["min_pp"]) and torch.equal(st[1:], parts["tau"])       # the thresholds themselves: exact
    _check("TopKBatchAgreement [%d,%d] %s %s" % (B, V, lt, setting), "tk", loss, dp, loss64, dp64)


def _autograd(fn, pd, *args, upstream=1.0):
    q = pd.clone().requires_grad_(True)
    loss = fn(q, *args)
    (loss * upstream).backward()
    return loss.detach(), q.grad


def test_ties_at_both_extrema_share_the_gradient(dev):
    """Two negatives at max_np = 0.75, two positives at min_pp = 0.25 (test_losses_host pins that the restatement gives each of a
    pair one half of dL/dr).  Untied, the same batch sends all of it to one element: the halves are visible at 1e-3 of max |dL/dp|."""
    p = torch.tensor([[0.75, 0.25, 0.5, 0.125], [0.25, 0.75, 0.375, 0.625]])
    y = torch.tensor([[0, 1, 1, 0], [1, 0, 0, 1]], dtype=torch.bool)
    a, N = 0.5, 2.0
    loss64, dp64 = loss_and_grad(batch_agreement_ref, p, y.double(), a, N)
    parts = batch_agreement_parts(p.double(), y.double(), a, N)
    for lt in ("u8", "f32"):
        pd, yd = p.to(dev), _labels(y, lt, dev)
        loss, stats = ops.batch_agreement_fwd(pd, yd, a, N)
        dp = ops.batch_agreement_bwd(pd, yd, stats, torch.ones(1, device=dev))
        _ba_stats_equal(stats, parts, y.double(), p.double())
        assert float(stats[ops.BA_STATS["ties_max_np"]]) == 2 and float(stats[ops.BA_STATS["ties_min_pp"]]) == 2
        _check("ties " + lt, "ba", loss, dp, loss64, dp64)
    q = p.clone()
    q[1, 1] = 0.75 - 2.0 ** -10                                            # untie max_np
    _, dq64 = loss_and_grad(batch_agreement_ref, q, y.double(), a, N)
    assert abs(dq64[0, 0] - dp64[0, 0]) > 1e-3 * np.abs(dp64).max()       # the whole of dL/dr instead of half of it
    _, stats = ops.batch_agreement_fwd(q.to(dev), y.to(dev), a, N)
    dq = ops.batch_agreement_bwd(q.to(dev), y.to(dev), stats, torch.ones(1, device=dev))
    assert float(stats[ops.BA_STATS["ties_max_np"]]) == 1
    assert float(np.abs(dq.cpu().numpy() - dq64).max()) <= TOL["ba"][1] * np.abs(dq64).max()


def _topk_rows_batch():
    """[4, 24], every value a multiple of 1/64.  Row 0: the 20th and 21st largest values are equal (21 classes pass p >= tau), one of
    the two is a positive.  Row 1: every positive outside the top 20.  Row 2: no positive.  Row 3: positives inside and outside."""
    rs = np.random.RandomState(7)
    p = np.zeros((4, 24), dtype=np.float32)
    y = np.zeros((4, 24), dtype=bool)
    vals = np.arange(60, 36, -1) / 64.0                                   # 24 distinct values, descending
    tied = vals.copy()
    tied[20] = tied[19]                                                   # ranks 20 and 21 tie
    perm = rs.permutation(24)
    p[0, perm] = tied
    y[0, perm[19]] = y[0, perm[3]] = True
    y[0, perm[23]] = True
    perm = rs.permutation(24)
    p[1, perm] = vals
    y[1, perm[20:]] = True
    p[2, rs.permutation(24)] = vals - 0.25
    perm = rs.permutation(24)
    p[3, perm] = vals
    y[3, perm[[2, 10, 22]]] = True
    return torch.from_numpy(p), torch.from_numpy(y)


def test_topk_rows_with_a_tied_threshold_and_without_positives_in_the_top_20(dev):
    p, y = _topk_rows_batch()
    a = 0.5
    parts = topk_batch_agreement_parts(p.double(), y.double(), a)
    assert int((p[0] >= parts["tau"][0]).sum()) == 21                     # the tie widens the mask
    assert float(parts["fn"][1].sum()) == 4 and float(parts["fn"][2].sum()) == 0 and float(parts["min_pp"]) == 41 / 64.0
    loss64, dp64 = loss_and_grad(topk_batch_agreement_ref, p, y.double(), a)
    for lt in ("u8", "f32"):
        pd, yd = p.to(dev), _labels(y, lt, dev)
        loss, stats = ops.topk_batch_agreement_fwd(pd, yd, a)
        dp = ops.topk_batch_agreement_bwd(pd, yd, stats, torch.ones(1, device=dev), a)
        st = stats.cpu().double()
        assert float(st[0]) == float(parts["min_pp"]) and torch.equal(st[1:], parts["tau"])
        _check("top-k rows " + lt, "tk", loss, dp, loss64, dp64)
        # w is 1 or 1 + a exactly: the weight of every element, read off the gradient, is the restatement's
        plain = ops.xent_bwd(pd, yd, None, torch.ones(1, device=dev))
        w = (dp / plain).cpu().double()
        assert float((w - parts["w"]).abs().max()) < 8 * U
    # the selection itself on values of either sign, many of them equal: the 20th largest as torch.topk counts it
    rs = np.random.RandomState(5)
    x = torch.from_numpy((rs.randint(-40, 41, size=(6, 300)) / 8.0).astype(np.float32))
    x[0, :25] = 5.0                                                       # more than 20 copies of the maximum
    x[1] = -x[1].abs() - 1.0                                              # a row of negative values only
    _, sx = ops.topk_batch_agreement_fwd(x.to(dev), torch.zeros(6, 300, dtype=torch.bool, device=dev), a)
    assert torch.equal(sx[1:].cpu(), torch.topk(x, 20, dim=1).values[:, 19])
    # only rows 1 and 2: no positive inside any top 20, min_pp = 1 and no false positive anywhere
    loss2, stats2 = ops.topk_batch_agreement_fwd(p[1:3].to(dev), y[1:3].to(dev), a)
    assert float(stats2[0]) == 1.0
    want = float(topk_batch_agreement_ref(p[1:3].double(), y[1:3].double(), a))
    assert abs(float(loss2) - want) <= TOL["tk"][0] * want


def test_a_perfectly_separated_batch(dev):
    """No false negative, no false positive: 0 / 0 in both centres, NaN from BatchAgreement as from the reference; the top-k loss has
    every weight 1 and is the plain cross entropy."""
    rs = np.random.RandomState(11)
    B, V = 3, 40
    y = rs.rand(B, V) < 0.1
    y[:, 0] = True
    p = np.where(y, 0.6 + 0.38 * rs.rand(B, V), 0.02 + 0.38 * rs.rand(B, V)).astype(np.float32)
    pd, yd = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    assert np.isnan(float(batch_agreement_ref(torch.from_numpy(p).double(), torch.from_numpy(y).double(), 0.1, 1024.0)))
    loss, stats = ops.batch_agreement_fwd(pd, yd, 0.1, 1024.0)
    assert np.isnan(float(loss))
    assert float(stats[ops.BA_STATS["n_fn"]]) == 0 and float(stats[ops.BA_STATS["n_fp"]]) == 0
    dp = ops.batch_agreement_bwd(pd, yd, stats, torch.ones(1, device=dev))
    assert bool(torch.isnan(dp).all())                                    # w itself is NaN: so is every element's gradient
    tk, dtk = _autograd(ops.topk_batch_agreement_cross_entropy, pd, yd, 0.5)
    ce, dce = _autograd(ops.cross_entropy, pd, yd)
    print("separated batch: top-k loss %.8g, cross entropy %.8g" % (float(tk), float(ce)))
    assert np.isfinite(float(tk)) and abs(float(tk) - float(ce)) <= TOL["tk"][0] * float(ce)
    assert float((dtk - dce).abs().max()) <= TOL["tk"][1] * float(dce.abs().max())


@pytest.mark.parametrize("B,V", [(3, 37), (5, 1030)])
def test_zero_agreement_is_the_plain_cross_entropy(dev, B, V):
    p, y = case(B, V)
    pd, yd = p.to(dev), y.to(dev)
    ce, dce = _autograd(ops.cross_entropy, pd, yd)
    for kind, fn, args in (("ba", ops.batch_agreement_cross_entropy, (yd, 0.0, 1024.0)), ("tk", ops.topk_batch_agreement_cross_entropy, (yd, 0.0))):
        loss, dp = _autograd(fn, pd, *args)
        el, ed = abs(float(loss) - float(ce)) / float(ce), float((dp - dce).abs().max() / dce.abs().max())
        print("a = 0, %s [%d,%d]: loss off by %.3g, dL/dp by %.3g" % (kind, B, V, el, ed))
        assert el <= TOL[kind][0] and ed <= TOL[kind][1]


def test_upstream_scalars_and_bitwise_replay(dev):
    """dL/dp carries the device scalar and the host scalar; the autograd path is the fwd / bwd pair; a second call gives the same bits
    (per-workgroup partial sums, added in a fixed order)."""
    B, V = 64, 4716
    p, y = case(B, V)
    pd, yd = p.to(dev), y.to(dev)
    up = torch.tensor([0.37], device=dev)
    for kind, ref, fwd, bwd, auto, args in (
            ("ba", _ba_ref, ops.batch_agreement_fwd, ops.batch_agreement_bwd, ops.batch_agreement_cross_entropy, (0.1, 1024.0)),
            ("tk", _tk_ref, ops.topk_batch_agreement_fwd, ops.topk_batch_agreement_bwd, ops.topk_batch_agreement_cross_entropy, (0.1,))):
        loss64, dp64, _ = ref(B, V, "default")
        bargs = args[:1] if kind == "tk" else ()
        loss, stats = fwd(pd, yd, *args)
        dp = bwd(pd, yd, stats, up, *bargs, upstream=2.0)
        _check(kind + " upstream 0.37 * 2", kind, loss, dp, loss64, dp64 * (0.37 * 2.0))
        loss_b, stats_b = fwd(pd, yd, *args)
        dp_b = bwd(pd, yd, stats_b, up, *bargs, upstream=2.0)
        assert torch.equal(loss, loss_b) and torch.equal(stats, stats_b) and torch.equal(dp, dp_b)
        la, da = _autograd(auto, pd, yd, *args, upstream=0.37)
        assert torch.equal(la, loss)
        _check(kind + " autograd, upstream 0.37", kind, la, da, loss64, dp64 * 0.37)
        la2, da2 = _autograd(auto, pd, yd, *args, upstream=0.37)
        assert torch.equal(la, la2) and torch.equal(da, da2)


def _params(g):
    return {k: v.data.detach().clone() for k, v in g.vars.items()}


@pytest.mark.parametrize("name", ["BatchAgreementCrossEntropyLoss", "TopKBatchAgreementCrossEntropyLoss"])
def test_a_training_step_of_the_logistic_model(dev, flags, name):
    """One TrainGraph.step with --label_loss=<name> (B = 8 rows, --batch_size = 16: N is the flag): the gradients the optimiser is
    given against autograd through the fp64 restatement of sigmoid(x W + b) and the loss.  Their bound: the loss kernels' own, plus
    the rounding of the two float32 products (D + B terms).  Two steps, run twice, replay bit for bit."""
    B, D, V = 8, 16, 37
    flags.label_loss, flags.batch_agreement, flags.batch_size = name, 0.5, 16
    rs = np.random.RandomState(21)
    x = torch.from_numpy(rs.randn(B, D).astype(np.float32))
    y = torch.from_numpy(rs.rand(B, V) < 0.1)

    def run(lr, steps):
        g = reset_default_graph(device=dev, seed=0)
        tg = train.build_graph(vlm.LogisticModel(), batch_size=B, graph=g, transformer_class=ft.IdenticalTransformer, base_learning_rate=lr)
        assert type(tg.label_loss_fn) is getattr(losses, name)
        outs = [tg.step(x.to(dev), y.to(dev)) for _ in range(steps)]
        return g, outs

    g, outs = run(0.0, 1)                                                 # lr = 0: the parameters stay what the gradients were taken at
    W = g.vars["fully_connected/weights"].data.detach().cpu().double().requires_grad_(True)
    b = g.vars["fully_connected/biases"].data.detach().cpu().double().requires_grad_(True)
    p64 = torch.sigmoid(x.double() @ W + b)
    if name.startswith("TopK"):
        loss64 = topk_batch_agreement_ref(p64, y.double(), 0.5)
    else:
        loss64 = batch_agreement_ref(p64, y.double(), 0.5, 16.0)
    loss64.backward()
    tol = TOL["ba" if not name.startswith("TopK") else "tk"]
    loss64 = loss64.detach()
    el = abs(float(outs[0]["loss"]) - float(loss64)) / float(loss64)
    print("%s step: loss %.8g (fp64 %.8g), off by %.3g" % (name, float(outs[0]["loss"]), float(loss64), el))
    assert el <= tol[0] + 2 * D * U
    for v, ref in ((g.vars["fully_connected/weights"], W.grad), (g.vars["fully_connected/biases"], b.grad)):
        err = float((v.grad.detach().cpu().double() - ref).abs().max() / ref.abs().max())
        print("%s step: d%s off by %.3g of its max %.3g" % (name, v.name, err, float(ref.abs().max())))
        assert err <= tol[1] + 2 * (D + B) * U
    ga, oa = run(0.01, 2)
    gb, ob = run(0.01, 2)
    assert torch.equal(oa[1]["loss"], ob[1]["loss"]) and torch.equal(ga.params, gb.params) and torch.equal(ga.grads, gb.grads)
    assert not torch.equal(ga.params, g.params)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("B,V", [(3, 37), (5, 1030)])
def test_pointwise_losses_against_fp64(dev, flags, B, V, smooth):
    """Through the loss classes, as --label_loss selects them.  --label_smoothing reaches WeightedCrossEntropyLoss and
    MeanSquareErrorLoss, not HingeLoss (W/losses.py:132-148).  b = 0.5 puts positives above 0.5 on the flat side of the hinge and the
    one at exactly 0.5 on the kink (value 0, gradient 0)."""
    flags.label_smoothing = smooth
    flags.false_negative_punishment, flags.false_positive_punishment = 2.0, 0.5
    p, y = case(B, V)
    p = p.clone()
    i = int(torch.nonzero(y[0])[0])
    p[0, i] = 0.5
    y64 = smoothing_ref(y.double()) if smooth else y.double()
    pd = p.to(dev)
    for lt in ("u8", "f32"):
        yd = _labels(y, lt, dev)
        for tag, cls, kw, ref, args in (("weighted", losses.WeightedCrossEntropyLoss, {}, weighted_xent_ref, (y64, 2.0, 0.5)),
                                        ("mse", losses.MeanSquareErrorLoss, {}, mse_ref, (y64,)),
                                        ("hinge", losses.HingeLoss, {"b": 0.5}, hinge_ref, (y.double(), 0.5))):
            loss64, dp64 = loss_and_grad(ref, p, *args, upstream=0.7)
            loss, dp = _autograd(lambda q: cls().calculate_loss(q, yd, weights=None, **kw), pd, upstream=0.7)
            _check("%s [%d,%d] %s smoothing=%s" % (tag, B, V, lt, smooth), "pw", loss, dp, loss64, dp64)
            if tag == "hinge":
                assert float(dp[0, i]) == 0.0 and float(dp64[0, i]) == 0.0
    # value and gradient from one pass are the two passes' (the forward of the autograd path asks for no gradient)
    for kind, c0, c1 in (("weighted_xent", 2.0, 0.5), ("mse", 1.0, 1.0), ("hinge", 0.5, 1.0)):
        l1, d1 = ops.pointwise_loss_fwd(pd, yd, kind, c0, c1, want_dp=True, upstream=0.7)
        l2, _ = ops.pointwise_loss_fwd(pd, yd, kind, c0, c1)
        d2 = ops.pointwise_loss_bwd(pd, yd, kind, torch.tensor([0.7], device=dev), c0, c1)
        assert torch.equal(l1, l2) and float((d1 - d2).abs().max()) <= 4 * U * float(d1.abs().max())


def test_the_losses_refuse_what_the_kernels_cannot_take(dev):
    p = torch.full((2, 24), 0.5, device=dev)
    with pytest.raises(TypeError):
        ops.batch_agreement_fwd(p, torch.zeros(2, 24, dtype=torch.int64, device=dev), 0.1, 2.0)
    with pytest.raises(ValueError):
        ops.topk_batch_agreement_fwd(p[:, :19], torch.zeros(2, 19, dtype=torch.bool, device=dev), 0.1)
    with pytest.raises(ValueError):
        ops.batch_agreement_fwd(p[:0], torch.zeros(0, 24, dtype=torch.bool, device=dev), 0.1, 2.0)
    with pytest.raises(KeyError):
        ops.pointwise_loss_fwd(p, p, "softmax")
