"""-m gpu: the stage-step kernels (csrc/mix_link.hip, ops.mix_link), Z's combine chain heads (MoeMix4Model, MoeKnowledgeModel),
LstmExtendCombineModel and the mix loss rule against the fp64 restatement (tests/mix_chain_restatement.py).

Bounds.  The measure is max |got - ref| / max(1, max |ref|) against the fp64 restatement on the same float32 inputs.  For the op's own
quantities (out, dprev, dz through the C ABI; out and every gradient through autograd, in both forms -- the complement form u2 - z2 is
held to the same bound against the reference's form with its materialised 1 - p) the bound is ensemble_restatement.bound in that
measure: FOUR times the error of the float32 restatement (plain torch on the CPU, in the reference's form) against the float64 one plus
one float32 ulp of the largest reference magnitude.  It is never derived from the kernels' output.  Every case prints the measured
errors with the float32 restatement's beside them and asserts that the float32 restatement is finite.  WIDER names the quantities that
get the gate tests' factor 8 and floors (2e-6 outputs, 5e-6 gradients) instead, with the reason: the plugins' quantities, which sit
behind the MoE products.

The clamped kind gives one row pre-activations of 1e-8 size, all positive: below zero tf.nn.elu is exp(x) - 1, which at -1e-8 is 0 or
-6e-8 depending on how the last bit of exp falls -- times the 1e6 of the clamped row that is no property of the step under test.

Measured on an MI355X (largest error per quantity, the float32 restatement's error of the same case in brackets):
  mix_link through the C ABI, the 48 cases: out 3.3e-8 [3.3e-8], dz 6.3e-8 [6.1e-8] (0.21 of its bound, (5, 37, 37, 37) plain, clamped);
    dprev is dy's columns bit for bit
  through autograd, kernels: out 6.1e-8 [9.2e-7], dp 3.3e-7 [3.2e-7] (0.24 of its bound, the nearest approach), dq 6.3e-8 [6.8e-8],
    dW1 1.4e-7 [3.0e-7], dW2 1.4e-7 [4.2e-7], db1 9.4e-8 [1.6e-7], db2 8.1e-8 [4.0e-7]; composed: out 1.9e-7, dp 3.6e-7, dW1 1.4e-7,
    dW2 1.9e-7, db1 8.5e-8, db2 1.2e-7 -- the complement form with its float64 column sum is no further from fp64 than the reference's
  the 8 head cases, on the wider rule: predictions 1.3e-7 [9.1e-8], predictions_class 1.5e-7 [1.5e-7], loss 7.4e-8 [5.8e-8], gradients
    2.6e-7 [5.0e-7] (MoeKnowledgeModel, workload shape): at most 0.07 of the floors
  LstmExtendCombineModel on bytes: predictions 5.8e-8 [8.1e-8], predictions_class 5.6e-8 [6.2e-8], loss 5.3e-8 [5.3e-8], gradients 4.7e-8 [5.3e-8]
  the rule through TrainGraph: loss 7.4e-8 [5.8e-8], gradients 1.4e-7 [1.2e-7]; TrainGraph.step reports the same loss bit for bit
"""
import functools

import numpy as np
import pytest
import torch

import extend_attention_restatement as XR
import mix_chain_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
import yt8m_amd.train  # noqa: F401  (defines --frame_features)
from yt8m_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
_PRODUCTS = ("a plugin quantity: behind the MoE heads' products and (in frame-level use) the recurrence, which the device runs K-split "
             "and, where they are large, as three f16 products with 2^-21 per term under per-operand scales, with v_exp / v_rcp gate "
             "functions -- none of which the float32 restatement on the CPU draws (the reason of tests/test_gpu_gate_lstm.py and "
             "tests/test_gpu_distill_head.py)")
WIDER = {"predictions": _PRODUCTS, "predictions_class": _PRODUCTS, "loss": _PRODUCTS, "gradient": _PRODUCTS}
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


# ---- mix_link through the C ABI -----------------------------------------------------------------------------------------------------------
# (rows, Wprev, C, dx_from, normalised): one row; rows that do not fill the last workgroup and widths with no factor 4; C with a factor 4
# under a Wprev with one; the scripts' first stage; a stage with earlier links in front; none mode, the frame-level form; the widest
# segment the kernel takes (C = 1024: a full register file of passes) -- C = 1025 is on the other side of that threshold and is refused
# (test_refused_mix_link_arguments_launch_nothing); dx_from with no factor 4 under widths that have one (the single-element path by dx_from alone)
LINK_SHAPES = [(1, 4, 1, 0, True), (5, 37, 37, 37, True), (3, 36, 100, 0, True), (6, 1152, 100, 1152, True), (2, 1752, 256, 1152, True),
               (5, 1024, 200, 0, False), (2, 8, 1024, 0, True), (3, 36, 100, 5, True)]
LINK_KINDS = ["plain", "misaligned", "clamped"]


def _link_case(rows, Wprev, C, kind, plain, seed):
    rs = np.random.RandomState(seed)
    prev = rs.randn(rows, Wprev).astype(np.float32)
    z = rs.randn(rows, 2 * C).astype(np.float32)
    u = (0.5 * rs.randn(2 * C)).astype(np.float32)
    dy = rs.randn(rows, Wprev + 2 * C).astype(np.float32)
    if kind == "clamped":                                                  # row 1 % rows: both sums of squares below eps = 1e-12
        u = (np.float32(1e-8) * (1 + rs.rand(2 * C))).astype(np.float32)
        r = 1 % rows
        z[r] = (np.float32(1e-8) * (1 + rs.rand(2 * C))).astype(np.float32)
        if not plain:
            z[r, C:] = -z[r, C:]                                          # u2 - z2 > 0
    return prev, z, u, dy


@functools.lru_cache(maxsize=None)
def _link_refs(rows, Wprev, C, norm, kind, plain):
    prev, z, u, dy = _link_case(rows, Wprev, C, kind, plain, 100 * rows + Wprev + C + len(kind) + int(plain))
    scale = R.link_scale(C, 1152) if norm else None
    r64 = R.kernel_with_grads(prev, z, u, plain, scale, dy, torch.float64)
    r32 = R.kernel_with_grads(prev, z, u, plain, scale, dy, torch.float32)
    return (prev, z, u, dy), _np(r64), _np(r32)


@pytest.mark.parametrize("kind", LINK_KINDS)
@pytest.mark.parametrize("plain", [False, True], ids=["complement", "plain"])
@pytest.mark.parametrize("rows,Wprev,C,dx_from,norm", LINK_SHAPES)
def test_mix_link_through_the_c_abi(dev, rows, Wprev, C, dx_from, norm, plain, kind):
    lib = L.lib()
    assert lib.yt8m_mix_link_supported(Wprev, C) == 1
    (prev, z, u, dy), r64, r32 = _link_refs(rows, Wprev, C, norm, kind, plain)
    bits = (ops.MIX_LINK_PLAIN if plain else 0) | (0 if norm else ops.MIX_LINK_NONE)
    scale = float(R.link_scale(C, 1152))
    W = Wprev + 2 * C
    off = 1 if kind == "misaligned" else 0                    # every pointer 4 bytes past a 16-byte boundary
    new = lambda n, data=None: _Guarded(dev, n, off, data)
    pb, zb, ub, gb = new(rows * Wprev, prev), new(rows * 2 * C, z), new(2 * C, u), new(rows * W, dy)

    def run(want_dprev=True):
        out, stats = new(rows * W), new(2 * rows)
        dprev, dz = (new(rows * Wprev) if want_dprev else None), new(rows * 2 * C)
        L.check(lib.yt8m_mix_link_fwd(bits, _p(pb.view), _p(zb.view), _p(ub.view), _p(out.view), _p(stats.view), rows, Wprev, C, scale, 1e-12,
                                      _stream()))
        L.check(lib.yt8m_mix_link_bwd(bits, _p(zb.view), _p(ub.view), _p(stats.view), _p(gb.view), _p(dprev.view) if want_dprev else None,
                                      _p(dz.view), rows, Wprev, C, dx_from, scale, _stream()))
        torch.cuda.synchronize()
        return out, stats, dprev, dz

    outs = run()
    out, stats, dprev, dz = outs
    for b in [pb, zb, ub, gb] + list(outs):
        assert b.intact()
    for b in (out, stats, dz):
        assert b.written()                                    # every element of every output was overwritten
    for b, src in ((pb, prev), (zb, z), (ub, u), (gb, dy)):
        assert torch.equal(b.view.cpu(), torch.from_numpy(src).view(-1))          # the operands are only read
    dp = dprev.view.cpu().view(rows, Wprev)
    assert bool((dp[:, :dx_from] == SENTINEL).all())          # the data columns in front are neither computed nor written
    got = {"out": out.view.cpu().view(rows, W), "dprev": dp[:, dx_from:], "dz": dz.view.cpu().view(rows, 2 * C)}
    ref64 = dict(r64, dprev=r64["dprev"][:, dx_from:])
    ref32 = dict(r32, dprev=r32["dprev"][:, dx_from:])
    if dx_from == Wprev:                                      # nothing of dprev is asked for
        del got["dprev"]
    _report("mix_link c abi (%d,%d,%d,%d) %s %s %s:" % (rows, Wprev, C, dx_from, "plain" if plain else "complement",
                                                        "norm" if norm else "none", kind), got, ref64, ref32)
    assert torch.equal(got["out"][:, :Wprev], torch.from_numpy(prev)) and torch.equal(dp[:, dx_from:], torch.from_numpy(dy[:, dx_from:Wprev]))
    sc = stats.view.cpu().view(2, rows)
    if not norm:
        assert bool((sc == 1).all())
    elif kind == "clamped":
        r = 1 % rows
        assert float(sc[0, r]) == -1e6 and float(sc[1, r]) == -1e6 and (rows < 2 or bool((sc[:, 0] > 0).all()))
    else:
        assert bool((sc > 0).all())
    # a second run gives the same bits
    outs2 = run()
    assert all(torch.equal(a.buf, b.buf) for a, b in zip(outs2, outs))
    # an unrequested dprev is untouched, dz unchanged
    spare = new(rows * Wprev)
    outs3 = run(want_dprev=False)
    assert spare.untouched() and outs3[2] is None and torch.equal(outs3[3].buf, dz.buf) and torch.equal(outs3[0].buf, out.buf)


def test_refused_mix_link_arguments_launch_nothing(dev):
    lib = L.lib()
    b = [_Guarded(dev, 4096, 0, np.zeros(4096)) for _ in range(3)]
    out, s = _Guarded(dev, 8192), _Guarded(dev, 8)
    assert lib.yt8m_mix_link_supported(8, 1025) == 0          # the other side of the widest segment
    call = lambda mode=0, rows=2, Wprev=8, C=8: lib.yt8m_mix_link_fwd(mode, _p(b[0].view), _p(b[1].view), _p(b[2].view), _p(out.view),
                                                                      _p(s.view), rows, Wprev, C, 0.5, 1e-12, _stream())
    assert call(mode=4) == -1 and call(rows=0) == -2 and call(Wprev=0) == -2 and call(C=1025) == -2
    back = lambda dx_from=0, C=8: lib.yt8m_mix_link_bwd(0, _p(b[0].view), _p(b[1].view), _p(b[2].view), _p(b[0].view), _p(out.view),
                                                        _p(out.view), 2, 8, C, dx_from, 0.5, _stream())
    assert back(dx_from=9) == -1 and back(C=1025) == -2
    torch.cuda.synchronize()
    assert out.untouched() and s.untouched()


# ---- ops.mix_link through autograd --------------------------------------------------------------------------------------------------------
# (rows, Wprev, V, C, dx_from, K: the columns of q, 0 = the complement mode, normalised)
OP_SHAPES = [(5, 37, 37, 37, 37, 0, True), (6, 1152, 4716, 100, 1152, 0, True), (6, 1352, 4716, 100, 1152, 25, True),
             (5, 1024, 4716, 200, 0, 0, False), (3, 36, 37, 1025, 0, 0, True)]


@functools.lru_cache(maxsize=None)
def _op_refs(rows, Wprev, V, C, K, norm):
    rs = np.random.RandomState(rows + Wprev + V + C + K)
    prev = rs.randn(rows, Wprev).astype(np.float32)
    p = rs.rand(rows, V).astype(np.float32)
    if V > 100:
        p = (p ** 8).astype(np.float32)                                   # most labels near 0, a few near 1
    q = rs.rand(rows, K).astype(np.float32) if K else None
    P = R.draw({"W1": (V, C), "b1": (C,), "W2": (K or V, C), "b2": (C,)}, rs)
    dy = rs.randn(rows, Wprev + 2 * C).astype(np.float32)
    scale = R.link_scale(C, 1152) if norm else None
    a = (prev, p, q, P["W1"], P["b1"], P["W2"], P["b2"], scale, dy)
    return (prev, p, q, P, dy), _np(R.link_with_grads(*a, torch.float64)), _np(R.link_with_grads(*a, torch.float32))


@pytest.mark.parametrize("rows,Wprev,V,C,dx_from,K,norm", OP_SHAPES)
def test_mix_link_autograd_fused_and_composed_against_the_restatement(dev, flags, monkeypatch, rows, Wprev, V, C, dx_from, K, norm):
    from yt8m_amd.variables import reset_default_graph, zeros
    (prev, p, q, P, dy), r64, r32 = _op_refs(rows, Wprev, V, C, K, norm)
    d = lambda a: torch.from_numpy(a).to(dev)
    scale = float(R.link_scale(C, 1152))
    takes_kernels = C <= 1024                                              # wider segments are refused: the composed form either way
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "MIX_LINK_FUSED", fused)
        monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", fused)
        key = "kernels" if (fused and takes_kernels) else "composed"
        for rep in range(2):
            g = reset_default_graph(device=dev, seed=0)
            vs = {k: g.get_variable(k, v.shape, zeros) for k, v in P.items()}
            g.finalize()
            for k, v in P.items():
                vs[k].data.copy_(d(v))
            g.begin_step()
            pt, xt = d(prev).requires_grad_(True), d(p).requires_grad_(True)
            qt = d(q).requires_grad_(True) if K else None
            before = dict(ops.MIX_LINK_CALLS)
            out = ops.mix_link(pt, xt, vs["W1"], vs["b1"], vs["W2"], vs["b2"], q=qt, norm=norm, scale=scale, dx_from=dx_from)
            assert ops.MIX_LINK_CALLS[key] == before[key] + 1 and sum(ops.MIX_LINK_CALLS.values()) == sum(before.values()) + 1
            out.backward(d(dy))
            torch.cuda.synchronize()
            got = {"out": out.detach().cpu(), "dp": xt.grad.cpu()}
            got.update({"d" + k: v.grad.detach().cpu().clone() for k, v in vs.items()})
            if K:
                got["dq"] = qt.grad.cpu()
            dprev = pt.grad.cpu()
            if fused and takes_kernels:
                assert float(dprev[:, :dx_from].abs().max() if dx_from else 0.0) == 0.0       # data columns: zeros, not computed
            if dx_from < Wprev:
                got["dprev"] = dprev[:, dx_from:]
            if rep:
                assert all(torch.equal(got[k], runs[fused][k]) for k in got)                 # two runs: the same bits
            runs[fused] = got
        ref64 = dict(r64, dprev=r64["dprev"][:, dx_from:])
        ref32 = dict(r32, dprev=r32["dprev"][:, dx_from:])
        _report("mix_link autograd (%d,%d,%d,%d,%d,%d) %s %s:" % (rows, Wprev, V, C, dx_from, K, "norm" if norm else "none", key),
                runs[fused], {k: ref64[k] for k in got}, ref32)
    # prev as data (the first stage in video-level use): no dprev is asked for, the rest is the same
    monkeypatch.setattr(ops, "MIX_LINK_FUSED", True)
    monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", True)
    xt = d(p).requires_grad_(True)
    g.begin_step()
    for v in vs.values():
        v.grad_written = False
    ops.mix_link(d(prev), xt, vs["W1"], vs["b1"], vs["W2"], vs["b2"], q=d(q) if K else None, norm=norm, scale=scale,
                 dx_from=Wprev).backward(d(dy))
    assert torch.equal(xt.grad.cpu(), runs[True]["dp"]) and torch.equal(vs["W2"].grad.cpu(), runs[True]["dW2"])


def test_cpu_and_float64_tensors_take_the_composed_form_when_the_kernels_are_asked_for(dev, monkeypatch):
    from yt8m_amd.variables import reset_default_graph, zeros
    monkeypatch.setattr(ops, "MIX_LINK_FUSED", True)
    monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", True)
    g = reset_default_graph(device=dev, seed=0)
    vs = [g.get_variable(k, s, zeros) for k, s in (("W1", (8, 4)), ("b1", (4,)), ("W2", (8, 4)), ("b2", (4,)))]
    before = dict(ops.MIX_LINK_CALLS)
    # the composed form is made of ops.linear and ops.activation, which are device float32 code: a CPU or float64 tensor reaches them,
    # not the fused kernels, and is refused there as by every other op
    with pytest.raises((L.Yt8mHipError, TypeError)):
        ops.mix_link(torch.rand(3, 5), torch.rand(3, 8), *vs)
    with pytest.raises((L.Yt8mHipError, TypeError)):
        ops.mix_link(torch.rand(3, 5, device=dev).double(), torch.rand(3, 8, device=dev).double(), *vs)
    assert ops.MIX_LINK_CALLS == dict(before, composed=before["composed"] + 2)


# ---- the heads as plugins -----------------------------------------------------------------------------------------------------------------
def _train_graph(model, dev, B, identical=True):
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=dev, seed=0)
    kw = {"transformer_class": ft.IdenticalTransformer} if identical else {}
    return g, train.TrainGraph(model, label_loss_fn=losses.CrossEntropyLoss(), batch_size=B, graph=g, **kw)


def _load(g, P, dev):
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    torch.cuda.synchronize()


def _grads(g):
    return {k: (v.grad if v.grad_written else torch.zeros_like(v.grad)).detach().cpu() for k, v in g.vars.items() if v.trainable}


HEAD_SHAPES = {"host": (5, 36, 37, 3, 7, 3, 6), "workload": (8, 1152, 4716, 2, 100, 3, 25)}       # B, D, V, M, C, layers, K


def _seq(shape):
    B, D, V, M, C, layers, K = HEAD_SHAPES[shape]
    rs = np.random.RandomState(V + K)
    return ((rs.rand(V, K) < 0.3) + 0.1 * rs.rand(V, K)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _head_refs(name, shape):
    B, D, V, M, C, layers, K = HEAD_SHAPES[shape]
    rs = np.random.RandomState(50 + R.HEADS.index(name) + B)
    x = rs.randn(B, D).astype(np.float32)
    if D > 100:
        x /= np.linalg.norm(x, axis=1, keepdims=True)                     # video-level features are l2-normalised
    y = rs.rand(B, V) < (0.2 if V < 100 else 3.4 / V)
    P = R.draw(R.variable_shapes(name, D, V, M, C, layers, K), rs)
    seq = _seq(shape).astype(np.float32) if name == "MoeKnowledgeModel" else None
    r64 = R.reference(name, x, y, P, M, C, layers, torch.float64, seq=seq)
    r32 = R.reference(name, x, y, P, M, C, layers, torch.float32, seq=seq)
    return (x, y, P), r64, r32


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("shape", ["host", "workload"])
@pytest.mark.parametrize("name", R.HEADS)
def test_head_matches_the_fp64_restatement_on_the_device(dev, flags, monkeypatch, tmp_path, name, shape, fused):
    """--model=<head> through TrainGraph.forward / loss / backward: predictions, predictions_class, the mix loss under CrossEntropyLoss
    and every Variable's gradient; the features are data, as in video-level use (no head gradient is computed for them)."""
    import yt8m_amd.video_level_models as vlm
    monkeypatch.setattr(ops, "MIX_LINK_FUSED", fused)
    monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", fused)
    B, D, V, M, C, layers, K = HEAD_SHAPES[shape]
    flags.moe_num_mixtures, flags.class_size, flags.moe_layers = M, C, layers
    flags.class_file = str(tmp_path / "labels_knowledge.out")
    np.savetxt(flags.class_file, _seq(shape))
    (x, y, P), r64, r32 = _head_refs(name, shape)
    g, tg = _train_graph(getattr(vlm, name)(), dev, B)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    tg.forward(*args)
    assert list(g.vars) == list(P)
    _load(g, P, dev)
    before = dict(ops.MIX_LINK_CALLS)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    form = "kernels" if fused else "composed"
    assert ops.MIX_LINK_CALLS == dict(before, **{form: before[form] + layers})
    tag = "%s %s %s:" % (name, shape, form)
    got = {"predictions": res["predictions"].detach().cpu(), "predictions_class": res["predictions_class"].detach().cpu(),
           "loss": loss.detach().cpu()}
    assert tuple(got["predictions_class"].shape) == (B, layers * V)
    _report(tag, got, {k: r64[k].numpy() for k in got}, {k: r32[k].numpy() for k in got})
    grads = _grads(g)
    assert set(grads) == set(r64["grads"])
    _report(tag + " gradients", grads, _np(r64["grads"]), _np(r32["grads"]), kind="gradient")
    for k in grads:
        assert float(grads[k].abs().max()) > 0, k


EXT = dict(B=4, F=12, D=1152, H=256, E=2, V=32, M=2, C=16, layers=2)


@functools.lru_cache(maxsize=None)
def _extend_refs():
    from oracle import np_ref
    c = EXT
    rs = np.random.RandomState(77)
    q = rs.randint(0, 256, size=(c["B"], c["F"], c["D"])).astype(np.uint8)
    nf = np.array([c["F"], 1, c["F"] - 1, c["F"] // 2], dtype=np.int32)
    y = rs.rand(c["B"], c["V"]) < 0.2
    shapes = XR.variable_shapes("LstmExtendModel", None, c["D"], c["H"], 1, c["E"], c["V"], c["M"])
    shapes.update(R.variable_shapes("MoeMix4Model", c["H"], c["V"], c["M"], c["C"], c["layers"]))
    P = {}
    for k, s in shapes.items():                                            # a trained model's scale (tests/test_gpu_extend_attention.py)
        if k.endswith("biases") or k in ("b1", "b2"):
            P[k] = (0.1 * rs.randn(*s)).astype(np.float32)
        elif k in ("W1", "W2"):
            P[k] = (4.0 * rs.randn(*s) / np.sqrt(s[0])).astype(np.float32)
        else:
            P[k] = (rs.randn(*s) / np.sqrt(s[0])).astype(np.float32)
    x64 = np_ref.dequant_l2norm_folded(q, nf)

    def pipeline(dtype):
        tp = R.to_torch(P, dtype)
        pooled, _ = XR.lstm_extend_model(torch.from_numpy(x64).to(dtype), torch.from_numpy(nf), tp, 1, c["E"])
        p, pc = R.extend_combine_tail(pooled, tp, c["M"], c["C"], c["layers"], c["E"])
        loss = R.mix_loss(p, pc, torch.from_numpy(y), c["layers"])
        loss.backward()
        return {"predictions": p.detach(), "predictions_class": pc.detach(), "loss": loss.detach(),
                "grads": {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in tp.items()}}

    return (q, nf, y, P), pipeline(torch.float64), pipeline(torch.float32)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_lstm_extend_combine_model_matches_fp64_on_bytes(dev, flags, monkeypatch, fused):
    """--model=LstmExtendCombineModel --frame_features, 256 cells, B = 4, F = 12, D = 1152 on the reader's bytes, E = 2, V = 32, 2
    mixtures, --class_size=16, --moe_layers=2: the head's input is the attention-pooled rows and hands its gradient to the pooling and
    the recurrence (dprev of the stage-step kernel); both results are the maximum over a video's E rows."""
    import yt8m_amd.frame_level_models as flm
    monkeypatch.setattr(ops, "MIX_LINK_FUSED", fused)
    monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", fused)
    c = EXT
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures, flags.moe_num_extend = str(c["H"]), 1, c["M"], c["E"]
    flags.class_size, flags.moe_layers, flags.frame_features = c["C"], c["layers"], True
    (q, nf, y, P), r64, r32 = _extend_refs()
    g, tg = _train_graph(flm.LstmExtendCombineModel(), dev, c["B"], identical=False)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    tg.forward(*args)
    assert list(g.vars) == list(P)
    _load(g, P, dev)
    before = dict(ops.MIX_LINK_CALLS)
    res = tg.forward(*args)
    assert "attention_weight" not in res
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    form = "kernels" if fused else "composed"
    assert ops.MIX_LINK_CALLS == dict(before, **{form: before[form] + c["layers"]})
    tag = "LstmExtendCombineModel %s:" % form
    got = {"predictions": res["predictions"].detach().cpu(), "predictions_class": res["predictions_class"].detach().cpu(),
           "loss": loss.detach().cpu()}
    assert tuple(got["predictions"].shape) == (c["B"], c["V"]) and tuple(got["predictions_class"].shape) == (c["B"], c["layers"] * c["V"])
    _report(tag, got, {k: r64[k].numpy() for k in got}, {k: r32[k].numpy() for k in got})
    grads = {k: v.view(r64["grads"][k].shape) for k, v in _grads(g).items()}
    assert set(grads) == set(r64["grads"])
    _report(tag + " gradients", grads, _np(r64["grads"]), _np(r32["grads"]), kind="gradient")
    assert float(grads["RNN/multi_rnn_cell/cell_0/basic_lstm_cell/weights"].abs().max()) > 0


def test_one_training_step_of_moe_mix4_under_the_rule(dev, flags, monkeypatch):
    """The rule through TrainGraph: forward / loss / backward gives the float64 restatement's mix loss and every gradient; TrainGraph.step
    on the device's own clip + Adam pass then reports the same loss and moves every Variable."""
    import yt8m_amd.video_level_models as vlm
    monkeypatch.setattr(ops, "MIX_LINK_FUSED", True)
    monkeypatch.setattr(ops, "MIX_LINK_FUSED_Q", True)
    B, D, V, M, C, layers, K = HEAD_SHAPES["host"]
    flags.moe_num_mixtures, flags.class_size, flags.moe_layers = M, C, layers
    (x, y, P), r64, r32 = _head_refs("MoeMix4Model", "host")
    g, tg = _train_graph(vlm.MoeMix4Model(), dev, B)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    tg.forward(*args)
    _load(g, P, dev)
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    plain = tg.label_loss_fn.calculate_loss(res["predictions"].detach(), args[1])
    assert float(loss.detach()) > float(plain)                                     # the class term is in it
    loss.backward()
    torch.cuda.synchronize()
    _report("MoeMix4Model rule:", {"loss": loss.detach().cpu()}, {"loss": r64["loss"].numpy()}, {"loss": r32["loss"].numpy()})
    _report("MoeMix4Model rule gradients", _grads(g), _np(r64["grads"]), _np(r32["grads"]), kind="gradient")
    start = {k: v.data.clone() for k, v in g.vars.items()}
    out = tg.step(*args)
    torch.cuda.synchronize()
    assert float(out["loss"]) == float(loss)                              # the step trains on the rule's loss, bit for bit
    out2 = tg.step(*args)
    torch.cuda.synchronize()
    for k, v in g.vars.items():
        assert bool(torch.isfinite(v.data).all()) and not torch.equal(v.data, start[k]), k
    assert np.isfinite(float(out["loss"])) and float(out2["loss"]) < float(out["loss"])
