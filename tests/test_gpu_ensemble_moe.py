"""The ensemble stage's MoE plugins on the MI355X: the kernels of csrc/ensemble_tensor.hip through the C ABI against the fp64 restatement
of tests/ensemble_moe_restatement.py on the same float32 inputs, ops.ens_tensor_moe / ens_mix fused against composed, the three plugins
through create_model against their fp64 restatement in both forms of the ops, and a training step per plugin through EnsembleTrainGraph
with its bitwise replay.  The harness is tests/test_gpu_ensemble.py's: guard words around every output and the workspace, a pointer 4 bytes
off a 16-byte boundary, a bit-equal second run.

Bound per output (R.bound): 4 x the error of the float32 CPU restatement against the fp64 one, plus one float32 ulp of the largest
reference magnitude; never derived from the kernel's output."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ensemble_moe_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.ensemble_level_models  # noqa: F401  (defines the flags set below)
import yt8m_amd.ops as ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 8
TOP = None                               # M = yt8m_ens_tensor_max_methods()

# (B, V, M)
SHAPES = [(3, 5, 1),                     # M = 1: out bit-equal to x, dW and db exactly 0; a partial wave
          (5, 67, 2),                    # V % 4 != 0 across two waves
          (17, 130, 9),                  # row tails: 16 + 1 rows of the forward's workgroup, an odd row count in the backward; 8 + 1 methods
          (33, 256, 74),                 # the models' M: 4 x 8 + 1 forward rows, 9 x 8 + 2 methods (k groups and the backward's l groups)
          (2, 4716, 74),                 # the models' V
          (2, 64, 80),                   # the top of the supported range
          (2, 64, TOP),                  # ... as the library reports it
          (16, 70, 8),                   # exactly one k group / l group, exactly the rows of one forward workgroup
          (13, 70, 16), (12, 70, 17),    # either side of the 16-method kernels; 17: 12 rows = one workgroup of the 48-method forward
          (13, 70, 48), (9, 70, 49)]     # either side of the 48-method kernels; 49: 8 + 1 rows of the 80-method forward
VARIANTS = ["plain", "exact-large-logits", "offset4"]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _place(t, dev, shift):
    """t on the device, `shift` floats into a buffer of its own (shift 1: a pointer 4 bytes off a 16-byte boundary)."""
    buf = torch.empty(t.numel() + shift, dtype=torch.float32, device=dev)
    view = buf[shift:].view(t.shape)
    view.copy_(t)
    return view


def _guarded(n, dev, shift):
    """n output floats behind `shift` and in front of GUARD sentinel words."""
    buf = torch.full((shift + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[shift:shift + n]


def _intact(buf, n, shift):
    return bool((buf[:shift] == SENTINEL).all()) and bool((buf[shift + n:] == SENTINEL).all())


def _methods(M):
    return L.lib().yt8m_ens_tensor_max_methods() if M is TOP else M


@functools.lru_cache(maxsize=None)
def _case(Bn, V, M, exact):
    """plain: x uniform in [0, 1] with an exact 0 and an exact 1, W uniform in [-1, 1], b ~ N(0, 1).
    exact large logits: x in {0, 1/4, ..., 1}, W multiples of 1/2 in [-8, 8], b integers in [-80, 80] with +80 and -80 in one row: every
    logit is a multiple of 1/8 below 2^10, exact in float32 in any summation order, and exp of it overflows without the maximum
    subtracted.  a: a softmax row per video; dout ~ N(0, 1).  With the references (fp64, float32) of both ops, computed once."""
    gen = torch.Generator().manual_seed(1000 * Bn + V + M + (7 if exact else 0))
    if exact:
        x = torch.randint(0, 5, (Bn, V, M), generator=gen).float() / 4.0
        W = torch.randint(-16, 17, (V, M, M), generator=gen).float() / 2.0
        b = torch.randint(-80, 81, (V, M), generator=gen).float()
        b[0, 0] = 80.0
        b[0, M - 1] = -80.0 if M > 1 else 80.0
        W[0, :, 0] = 8.0
        x[Bn - 1, 0, :] = 1.0                                            # logit (Bn - 1, 0, 0) = 80 + 8 M
    else:
        x = torch.rand(Bn, V, M, generator=gen)
        W = torch.rand(V, M, M, generator=gen) * 2.0 - 1.0
        b = torch.randn(V, M, generator=gen)
    x[0, 0, 0] = 0.0
    x[Bn - 1, V - 1, M - 1] = 1.0
    if M > 1:
        x[0, V // 2, 1] = 1.0
        x[Bn - 1, 1, 0] = 0.0
    a = torch.softmax(torch.randn(Bn, M, generator=gen), dim=-1)
    dout = torch.randn(Bn, V, generator=gen)
    refs = {"tensor64": R.tensor_moe_with_grads(x, W, b, dout, torch.float64), "tensor32": R.tensor_moe_with_grads(x, W, b, dout, torch.float32),
            "mix64": R.mix_with_grads(x, a, dout, torch.float64), "mix32": R.mix_with_grads(x, a, dout, torch.float32)}
    return x, W, b, a, dout, refs


def _run_tensor(lib, dev, x, W, b, dout, shift):
    Bn, V, M = x.shape
    xm = _place(x.permute(2, 0, 1).contiguous(), dev, shift)             # method-major [M, B, V]
    Wt = _place(W.permute(1, 2, 0).contiguous(), dev, shift)             # [k, l, V]
    bt = _place(b.t().contiguous(), dev, shift)                          # [l, V]
    dd = _place(dout, dev, shift)
    sizes = (("out", Bn * V), ("stat", 2 * Bn * V), ("dWt", M * M * V), ("dbt", M * V))
    bufs = {k: _guarded(n, dev, shift) for k, n in sizes}
    out, stat, dWt, dbt = (bufs[k][1] for k, _ in sizes)
    nbytes = lib.yt8m_ens_tensor_bwd_workspace_bytes(Bn, V, M)
    assert nbytes >= 0
    wbuf, ws = _guarded(nbytes // 4, dev, 0)
    L.check(lib.yt8m_ens_tensor_fwd(_p(xm), _p(Wt), _p(bt), _p(out), _p(stat), Bn, V, M, _st()))
    L.check(lib.yt8m_ens_tensor_bwd(_p(xm), _p(Wt), _p(bt), _p(out), _p(stat), _p(dd), _p(dWt), _p(dbt), _p(wbuf), nbytes, Bn, V, M, _st()))
    # prediction only: no stat
    ob2, out2 = _guarded(Bn * V, dev, shift)
    L.check(lib.yt8m_ens_tensor_fwd(_p(xm), _p(Wt), _p(bt), _p(out2), None, Bn, V, M, _st()))
    torch.cuda.synchronize()
    for k, n in sizes:
        assert _intact(bufs[k][0], n, shift), "guard words around %s" % k
    assert _intact(wbuf, nbytes // 4, 0), "guard words behind the workspace"
    assert _intact(ob2, Bn * V, shift) and torch.equal(out2, out)
    mx, inv = stat.view(2, Bn, V).cpu().double()                         # lse = max + log sum, formed in fp64 from the two planes
    return (out.view(Bn, V).cpu(), mx - torch.log(inv), dWt.view(M, M, V).permute(2, 0, 1).contiguous().cpu(),
            dbt.view(M, V).t().contiguous().cpu())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("Bn,V,M", SHAPES)
def test_tensor_kernels_against_the_fp64_restatement(dev, Bn, V, M, variant):
    """yt8m_ens_tensor_fwd / _bwd through ctypes: out, lse, dW and db under R.bound; guard words keep their sentinel; a second run is
    bit-equal; with M = 1 out is x to the bit and both gradients are exactly 0."""
    lib = L.lib()
    M = _methods(M)
    shift = 1 if variant == "offset4" else 0
    x, W, b, _, dout, refs = _case(Bn, V, M, variant == "exact-large-logits")
    got = _run_tensor(lib, dev, x, W, b, dout, shift)
    again = _run_tensor(lib, dev, x, W, b, dout, shift)
    for g1, g2 in zip(got, again):
        assert torch.equal(g1, g2)                                       # no atomics: the same bits
    assert all(bool(torch.isfinite(t).all()) for t in refs["tensor32"])
    if variant == "exact-large-logits" and M > 1:
        assert float(refs["tensor64"][1].max()) >= 80 + 8 * M > 88.8     # exp of the largest logit overflows float32
    for tag, g, r32, r64 in zip(("out", "lse", "dW", "db"), got, refs["tensor32"], refs["tensor64"]):
        assert bool(torch.isfinite(g).all()), tag
        err, bnd = float((g.double() - r64).abs().max()), R.bound(r32, r64)
        print("(%d,%d,%d) %s %s: err %.3g (bound %.3g)" % (Bn, V, M, variant, tag, err, bnd))
        assert err <= bnd, tag
    if M == 1:
        assert torch.equal(got[0], x[:, :, 0])
        assert bool((got[2] == 0).all()) and bool((got[3] == 0).all())


def _run_mix(lib, dev, x, a, dout, shift):
    Bn, V, M = x.shape
    xm = _place(x.permute(2, 0, 1).contiguous(), dev, shift)
    ad, dd = _place(a, dev, shift), _place(dout, dev, shift)
    ob, out = _guarded(Bn * V, dev, shift)
    ab, da = _guarded(Bn * M, dev, shift)
    L.check(lib.yt8m_ens_mix_fwd(_p(xm), _p(ad), _p(out), Bn, V, M, _st()))
    L.check(lib.yt8m_ens_mix_bwd(_p(xm), _p(dd), _p(da), Bn, V, M, _st()))
    torch.cuda.synchronize()
    assert _intact(ob, Bn * V, shift) and _intact(ab, Bn * M, shift)
    return out.view(Bn, V).cpu(), da.view(Bn, M).cpu()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("Bn,V,M", SHAPES)
def test_mix_kernels_against_the_fp64_restatement(dev, Bn, V, M, shift):
    """yt8m_ens_mix_fwd / _bwd at the shapes of the tensor kernels, aligned and 4 bytes off."""
    lib = L.lib()
    M = _methods(M)
    x, _, _, a, dout, refs = _case(Bn, V, M, False)
    got = _run_mix(lib, dev, x, a, dout, shift)
    again = _run_mix(lib, dev, x, a, dout, shift)
    for tag, g, g2, r32, r64 in zip(("out", "da"), got, again, refs["mix32"], refs["mix64"]):
        assert torch.equal(g, g2), tag
        err, bnd = float((g.double() - r64).abs().max()), R.bound(r32, r64)
        print("(%d,%d,%d) shift %d mix %s: err %.3g (bound %.3g)" % (Bn, V, M, shift, tag, err, bnd))
        assert err <= bnd, tag


def test_refusals_leave_the_outputs_untouched(dev):
    lib = L.lib()
    x, W, b, a, dout, _ = _case(4, 8, 3, False)
    xm, Wt, bt = x.permute(2, 0, 1).contiguous().to(dev), W.permute(1, 2, 0).contiguous().to(dev), b.t().contiguous().to(dev)
    ad, dd = a.to(dev), dout.to(dev)
    ob, out = _guarded(32, dev, 0)
    sb, stat = _guarded(72, dev, 0)
    top = lib.yt8m_ens_tensor_max_methods()
    calls = [lambda: lib.yt8m_ens_tensor_fwd(None, _p(Wt), _p(bt), _p(out), _p(stat), 4, 8, 3, _st()),
             lambda: lib.yt8m_ens_tensor_fwd(_p(xm), _p(Wt), _p(bt), _p(out), _p(stat), 0, 8, 3, _st()),
             lambda: lib.yt8m_ens_tensor_fwd(_p(xm), _p(Wt), _p(bt), _p(out), _p(stat), 4, 8, top + 1, _st()),
             lambda: lib.yt8m_ens_tensor_bwd(_p(xm), _p(Wt), _p(bt), _p(out), _p(stat), _p(dd), _p(stat), _p(out), _p(stat), -1, 4, 8, 3, _st()),
             lambda: lib.yt8m_ens_tensor_bwd(_p(xm), _p(Wt), _p(bt), _p(out), _p(stat), None, _p(stat), _p(out), None, 0, 4, 8, 3, _st()),
             lambda: lib.yt8m_ens_mix_fwd(_p(xm), None, _p(out), 4, 8, 3, _st()),
             lambda: lib.yt8m_ens_mix_bwd(_p(xm), _p(dd), _p(out), 4, 0, 3, _st())]
    for i, call in enumerate(calls):
        assert call() == -1, i
    torch.cuda.synchronize()
    assert bool((ob == SENTINEL).all()) and bool((sb == SENTINEL).all())
    del ad


# ---- the ops --------------------------------------------------------------------------------------------------------------------------
def _op_run(fused, monkeypatch, x, W, b, a, dout, dev):
    import yt8m_amd.ensemble as ensemble
    monkeypatch.setattr(ops, "ENS_TENSOR_FUSED", fused)
    monkeypatch.setattr(ops, "ENS_MIX_FUSED", fused)
    xd = ensemble.stack_methods(x.permute(2, 0, 1).contiguous().to(dev))
    assert ops.ens_method_major(xd) and ops._ens_tensor_fused(xd) == fused and ops._ens_mix_fused(xd) == fused
    Wd, bd, ad = (t.to(dev).requires_grad_(True) for t in (W, b, a))
    out = ops.ens_tensor_moe(xd, Wd, bd)
    assert (type(out.grad_fn).__name__ == "_EnsTensorMoeBackward") == fused
    out.backward(dout.to(dev))
    mo = ops.ens_mix(xd, ad)
    assert (type(mo.grad_fn).__name__ == "_EnsMixBackward") == fused
    mo.backward(dout.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), Wd.grad.cpu(), bd.grad.cpu(), mo.detach().cpu(), ad.grad.cpu()


def test_ops_fused_against_composed(dev, monkeypatch):
    """ops.ens_tensor_moe and ops.ens_mix with the kernels and in their composed torch forms at (33, 256, 74): values and the gradients
    that autograd hands to W [V, M, M], b [V, M] and a [B, M], the fused form against fp64 under R.bound and against the composed form
    under twice that (each within the bound of fp64)."""
    x, W, b, a, dout, refs = _case(33, 256, 74, False)
    f = _op_run(True, monkeypatch, x, W, b, a, dout, dev)
    c = _op_run(False, monkeypatch, x, W, b, a, dout, dev)
    pairs = [("out", 0, "tensor", 0), ("dW", 1, "tensor", 2), ("db", 2, "tensor", 3), ("mix", 3, "mix", 0), ("da", 4, "mix", 1)]
    for tag, i, op, j in pairs:
        r64, r32 = refs[op + "64"][j], refs[op + "32"][j]
        bnd = R.bound(r32, r64)
        ef, ec, efc = (float((f[i].double() - r64).abs().max()), float((c[i].double() - r64).abs().max()), float((f[i] - c[i]).abs().max()))
        print("%s: fused %.3g composed %.3g fused - composed %.3g (bound %.3g)" % (tag, ef, ec, efc, bnd))
        assert ef <= bnd and efc <= 2 * bnd, tag


def test_inputs_outside_the_kernels_take_the_composed_forms(dev, monkeypatch):
    """More methods than the kernels take, a contiguous [B, V, M] input and an x that requires a gradient: the composed forms, counted."""
    monkeypatch.setattr(ops, "ENS_TENSOR_FUSED", True)
    monkeypatch.setattr(ops, "ENS_MIX_FUSED", True)
    top = L.lib().yt8m_ens_tensor_max_methods()
    gen = torch.Generator().manual_seed(4)

    def count(x, M, tensor_kernels, mix_kernels):
        W, b = torch.randn(6, M, M, generator=gen).to(dev), torch.randn(6, M, generator=gen).to(dev)
        a = torch.softmax(torch.randn(3, M, generator=gen), dim=-1).to(dev)
        before = dict(ops.ENS_TENSOR_CALLS), dict(ops.ENS_MIX_CALLS)
        out, mo = ops.ens_tensor_moe(x, W, b), ops.ens_mix(x, a)
        ref, mref = R.tensor_moe(x.detach().cpu().double(), W.cpu().double(), b.cpu().double())[0], R.mix(x.detach().cpu().double(), a.cpu().double())
        assert float((out.detach().cpu().double() - ref).abs().max()) < 1e-5 and float((mo.detach().cpu().double() - mref).abs().max()) < 1e-5
        dt = {k: ops.ENS_TENSOR_CALLS[k] - before[0][k] for k in before[0]}
        dm = {k: ops.ENS_MIX_CALLS[k] - before[1][k] for k in before[1]}
        assert dt == {"kernels": int(tensor_kernels), "composed": int(not tensor_kernels)}, dt
        assert dm == {"kernels": int(mix_kernels), "composed": int(not mix_kernels)}, dm

    mm = lambda M: torch.rand(M, 3, 6, generator=gen).to(dev).permute(1, 2, 0)
    count(mm(5), 5, True, True)
    count(mm(top), top, True, True)
    count(mm(top + 1), top + 1, False, True)                             # the per-video mix has no cap on M
    count(mm(5).contiguous(), 5, False, False)
    count(mm(5).requires_grad_(True), 5, False, False)


# ---- the plugins ------------------------------------------------------------------------------------------------------------------------
# tolerances of tests/test_gpu_ensemble.py::test_plugins_match_the_fp64_restatement: the fully-connected layers run through the library's
# GEMMs
P_TOL, GRAD_TOL = 1e-4, 5e-4
PLUGIN_SHAPES = [(5, 67, 3, 20, 8), (17, 130, 9, 40, 16)]


@functools.lru_cache(maxsize=None)
def _plugin_case(name, shape):
    B, V, M, D, cells = shape
    x, orig, P, coef = R.plugin_case(name, B, V, M, D, cells, seed=len(name) + B)
    return x, orig, P, coef, R.plugin_reference(name, x, orig, P, coef)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("shape", PLUGIN_SHAPES)
@pytest.mark.parametrize("name", sorted(R.PLUGINS))
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, shape, fused):
    """Each plugin through create_model: predictions and the gradient of EVERY variable, with the kernels and with the composed forms."""
    monkeypatch.setattr(ops, "ENS_TENSOR_FUSED", fused)
    monkeypatch.setattr(ops, "ENS_MIX_FUSED", fused)
    flags.attention_relu_cells = shape[4]
    x, orig, P, coef, (p64, g64) = _plugin_case(name, shape)
    before = ops.ENS_TENSOR_CALLS["kernels"] + ops.ENS_MIX_CALLS["kernels"]
    pred, grads, g = R.run_plugin(name, x, orig, P, coef, dev, shape[4])
    torch.cuda.synchronize()
    assert (ops.ENS_TENSOR_CALLS["kernels"] + ops.ENS_MIX_CALLS["kernels"] - before == 2) == fused      # create_model ran twice
    ep = float((pred.double() - p64).abs().max())
    unit = lambda k: float((grads[k].double() - g64[k]).abs().max()) / max(1.0, float(g64[k].abs().max()))
    print("%s %s fused=%d: predictions %.3g worst gradient %.3g" % (name, shape, fused, ep, max(unit(k) for k in g64)))
    assert ep < P_TOL
    assert set(grads) == set(g64)
    for k in g64:
        assert unit(k) <= GRAD_TOL, k
        assert float(grads[k].abs().max()) > 0, k


@pytest.mark.parametrize("name", sorted(R.PLUGINS))
def test_a_training_step_and_its_bitwise_replay(dev, flags, monkeypatch, name):
    """EnsembleTrainGraph.step (cross entropy, clip, Adam) with the kernels on the path: finite losses, every variable moved; the same
    two steps taken twice from the same state leave bit-identical parameters and Adam moments."""
    import yt8m_amd.ensemble as ensemble
    import yt8m_amd.ensemble_level_models as elm
    import yt8m_amd.train as train
    from yt8m_amd.variables import reset_default_graph
    monkeypatch.setattr(ops, "ENS_TENSOR_FUSED", True)
    monkeypatch.setattr(ops, "ENS_MIX_FUSED", True)
    flags.attention_relu_cells = 7
    rs = np.random.RandomState(41)
    Bt, Vt, Mt, Dt = 6, 37, 3, 6
    x = torch.from_numpy(rs.rand(Mt, Bt, Vt).astype(np.float32)).to(dev).permute(1, 2, 0)
    y = torch.from_numpy(rs.rand(Bt, Vt) < 0.2).to(dev)
    orig = torch.from_numpy(rs.randn(Bt, Dt).astype(np.float32)).to(dev)
    g = reset_default_graph(device=dev, seed=0)
    tg = ensemble.EnsembleTrainGraph(train.find_class_by_name(name, [elm])(), batch_size=Bt, graph=g)
    before = ops.ENS_TENSOR_CALLS["kernels"] + ops.ENS_MIX_CALLS["kernels"]
    out = tg.step(x, y, original_input=orig)
    assert ops.ENS_TENSOR_CALLS["kernels"] + ops.ENS_MIX_CALLS["kernels"] > before
    assert np.isfinite(float(out["loss"])) and tuple(out["predictions"].shape) == tuple(y.shape)
    if name == "MoeModel":                                               # tensor_bias starts at zero and has moved
        assert float(g.vars["tensor_bias"].data.abs().max()) > 0
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step = tg.global_step
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step = step
        for _ in range(2):
            out = tg.step(x, y, original_input=orig)
            assert np.isfinite(float(out["loss"]))
        torch.cuda.synchronize()
        after.append([t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)])
    assert all(torch.equal(p, q) for p, q in zip(*after))
    for v in g.trainable_variables():
        assert not torch.equal(after[0][0][v.offset:v.offset + v.numel()], state[0][v.offset:v.offset + v.numel()]), v.name
