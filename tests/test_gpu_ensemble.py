"""The ensemble stage on the MI355X: the kernels of csrc/ensemble.hip through the C ABI against the fp64 restatement of
tests/ensemble_restatement.py on the same float32 inputs, ops.ens_combine fused against composed, every plugin of ensemble_level_models.py
through create_model against its fp64 restatement in both forms of the op, training steps through EnsembleTrainGraph with their bitwise
replay, and a two-level run over prediction dumps.

Bound per output (R.bound, the _bound of tests/test_gpu_distillchain.py): 4 x the error of the float32 CPU restatement against the fp64
one, plus one float32 ulp of the largest reference magnitude; never derived from the kernel's output."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_restatement as R
import yt8m_amd._lib as L
import yt8m_amd.ensemble_level_models  # noqa: F401  (defines the flags set below)
import yt8m_amd.ops as ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 8

# (B, V, M, J; gate given?)
SHAPES = [(3, 5, 1, 1, True),          # M = 1: out bit-equal to x, every gradient exactly 0; a partial wave on the single-element path
          (5, 67, 2, 3, True),         # V % 4 != 0 across two waves
          (17, 130, 9, 4, True),       # the forward's 4-row groups end in a tail of 1; two backward chunks (9 + 8 rows); V % 4 != 0
          (33, 256, 74, 4, True),      # the 16-byte path at the models' M; three backward chunks of 11; a method-range tail (74 = 18 x 4 + 2)
          (3, 4716, 74, 4, True),      # the models' V
          (2, 64, 130, 1, False)]      # gate None, M above the models'
VARIANTS = ["plain", "logit", "scaled80", "offset4"]


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


def _case(Bn, V, M, J, gated, variant, seed):
    """x [B, V, M] in [0, 1] with an exact 0 and an exact 1, tables ~ N(0, 1) (scaled80: uniform in [-80, 80], so that a sum of
    exponentials without the maximum subtracted overflows float32 at exp(80) x M > 3.4e38 ... exp(88.7)), gate = a softmax row (J > 1)
    or one positive number per row, dout ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(Bn, V, M, generator=gen)
    x[0, 0, 0] = 0.0
    x[Bn - 1, V - 1, M - 1] = 1.0
    if M > 1:
        x[0, V // 2, 1] = 1.0
        x[Bn - 1, 1, 0] = 0.0
    W = torch.randn(J, V, M, generator=gen)
    if variant == "scaled80":
        W = (torch.rand(J, V, M, generator=gen) * 2.0 - 1.0) * 80.0
        W[0, 0, 0] = 80.0
        W[0, 0, M - 1] = -80.0 if M > 1 else 80.0
    gate = None
    if gated:
        gate = torch.softmax(torch.randn(Bn, J, generator=gen), dim=-1) if J > 1 else torch.rand(Bn, 1, generator=gen) + 0.5
        if variant == "scaled80" and J > 1:
            gate[0] = 0.0
            gate[0, 0] = 1.0                                             # row 0's logits are table 0's: +-80 is reached
    return x, W, gate, torch.randn(Bn, V, generator=gen)


def _run_kernels(lib, dev, x, W, gate, kind, dout, shift):
    Bn, V, M = x.shape
    J = W.shape[0]
    xm = _place(x.permute(2, 0, 1).contiguous(), dev, shift)             # method-major [M, B, V]
    Wt = _place(W.permute(0, 2, 1).contiguous(), dev, shift)             # [J, M, V]
    gd = None if gate is None else gate.to(dev)
    dd = _place(dout, dev, shift)
    sizes = (("out", Bn * V), ("stat", 2 * Bn * V), ("dWt", J * M * V), ("dgate", Bn * J))
    bufs = {k: _guarded(n, dev, shift) for k, n in sizes}
    out, stat, dWt, dgate = (bufs[k][1] for k, _ in sizes)
    nbytes = lib.yt8m_ens_combine_bwd_workspace_bytes(Bn, V, M, J)
    assert nbytes > 0
    wbuf, ws = _guarded(nbytes // 4, dev, 0)
    xf = 0 if kind is None else 1
    L.check(lib.yt8m_ens_combine_fwd(_p(xm), _p(Wt), None if gd is None else _p(gd), xf, _p(out), _p(stat), Bn, V, M, J, _st()))
    L.check(lib.yt8m_ens_combine_bwd(_p(xm), _p(Wt), None if gd is None else _p(gd), xf, _p(out), _p(stat), _p(dd), _p(dWt),
                                     None if gd is None else _p(dgate), _p(ws), nbytes, Bn, V, M, J, _st()))
    torch.cuda.synchronize()
    for k, n in sizes:
        assert _intact(bufs[k][0], n, shift), "guard words around %s" % k
    assert _intact(wbuf, nbytes // 4, 0), "guard words behind the workspace"
    if gd is None:
        assert bool((dgate == SENTINEL).all())                           # not asked for: untouched
    mx, inv = stat.view(2, Bn, V).cpu().double()                         # lse = max + log sum, formed in fp64 from the two planes
    return (out.view(Bn, V).cpu(), mx - torch.log(inv), dWt.view(J, M, V).permute(0, 2, 1).contiguous().cpu(),
            None if gd is None else dgate.view(Bn, J).cpu())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("Bn,V,M,J,gated", SHAPES)
def test_combine_kernels_against_the_fp64_restatement(dev, Bn, V, M, J, gated, variant):
    """yt8m_ens_combine_fwd / _bwd through ctypes: out, lse, dW and dgate under R.bound; guard words keep their sentinel; a second run is
    bit-equal; with M = 1 out is x to the bit and every gradient is exactly 0."""
    lib = L.lib()
    kind = "logit" if variant == "logit" else None
    shift = 1 if variant == "offset4" else 0
    x, W, gate, dout = _case(Bn, V, M, J, gated, variant, seed=1000 * Bn + V + M)
    got = _run_kernels(lib, dev, x, W, gate, kind, dout, shift)
    again = _run_kernels(lib, dev, x, W, gate, kind, dout, shift)
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b)           # no atomics: the same bits
    ref64 = R.combine_with_grads(x, W, gate, kind, dout, torch.float64)
    ref32 = R.combine_with_grads(x, W, gate, kind, dout, torch.float32)
    assert all(bool(torch.isfinite(t).all()) for t in ref32 if t is not None)
    for tag, g, r32, r64 in zip(("out", "lse", "dW", "dgate"), got, ref32, ref64):
        if g is None:
            assert r64 is None
            continue
        assert bool(torch.isfinite(g).all()), tag
        err, bnd = float((g.double() - r64).abs().max()), R.bound(r32, r64)
        print("(%d,%d,%d,%d) %s %s: err %.3g (bound %.3g)" % (Bn, V, M, J, variant, tag, err, bnd))
        assert err <= bnd, tag
    if M == 1:
        if kind is None:
            assert torch.equal(got[0], x[:, :, 0])
        assert bool((got[2] == 0).all()) and bool((got[3] == 0).all())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("Bn,V,M,J,gated", SHAPES)
def test_moments_kernel_against_the_fp64_restatement(dev, Bn, V, M, J, gated, shift):
    """yt8m_ens_moments at the shapes of the combine, aligned and 4 bytes off: the mean alone and the mean with the unbiased variance."""
    lib = L.lib()
    x = _case(Bn, V, M, J, gated, "plain", seed=7 * Bn + V + M)[0]
    xm = _place(x.permute(2, 0, 1).contiguous(), dev, shift)
    m64, v64 = R.moments(x.double())
    m32, v32 = R.moments(x)
    for want_var in (False, True):
        mb, mean = _guarded(Bn * V, dev, shift)
        vb, var = _guarded(Bn * V, dev, shift)
        status = lib.yt8m_ens_moments(_p(xm), _p(mean), _p(var) if want_var else None, Bn, V, M, _st())
        torch.cuda.synchronize()
        if want_var and M < 2:
            assert status == -1 and bool((mb == SENTINEL).all()) and bool((vb == SENTINEL).all())       # refused, nothing written
            continue
        L.check(status)
        assert _intact(mb, Bn * V, shift) and _intact(vb, Bn * V, shift)
        e = float((mean.view(Bn, V).cpu().double() - m64).abs().max())
        assert e <= R.bound(m32, m64), ("mean", e)
        if M == 1:
            assert torch.equal(mean.view(Bn, V).cpu(), x[:, :, 0])
        if want_var:
            e = float((var.view(Bn, V).cpu().double() - v64).abs().max())
            assert e <= R.bound(v32, v64), ("var", e)
        else:
            assert bool((var == SENTINEL).all())


def test_refusals_leave_the_outputs_untouched(dev):
    lib = L.lib()
    x, W, gate, dout = _case(4, 8, 3, 2, True, "plain", seed=5)
    xm, Wt, gd, dd = x.permute(2, 0, 1).contiguous().to(dev), W.permute(0, 2, 1).contiguous().to(dev), gate.to(dev), dout.to(dev)
    ob, out = _guarded(32, dev, 0)
    lb, lse = _guarded(64, dev, 0)
    calls = [lambda: lib.yt8m_ens_combine_fwd(None, _p(Wt), _p(gd), 0, _p(out), _p(lse), 4, 8, 3, 2, _st()),
             lambda: lib.yt8m_ens_combine_fwd(_p(xm), _p(Wt), _p(gd), 0, _p(out), _p(lse), 0, 8, 3, 2, _st()),
             lambda: lib.yt8m_ens_combine_fwd(_p(xm), _p(Wt), _p(gd), 0, _p(out), _p(lse), 4, 8, 3, 5, _st()),
             lambda: lib.yt8m_ens_combine_fwd(_p(xm), _p(Wt), _p(gd), 2, _p(out), _p(lse), 4, 8, 3, 2, _st()),
             lambda: lib.yt8m_ens_combine_fwd(_p(xm), _p(Wt), None, 0, _p(out), _p(lse), 4, 8, 3, 2, _st()),
             lambda: lib.yt8m_ens_combine_bwd(_p(xm), _p(Wt), _p(gd), 0, _p(out), _p(lse), _p(dd), _p(out), None, _p(lse), 1 << 20, 4, 8, 3, 2,
                                              _st())]
    for i, call in enumerate(calls):
        assert call() == -1, i
    torch.cuda.synchronize()
    assert bool((ob == SENTINEL).all()) and bool((lb == SENTINEL).all())


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
def _op_run(fused, monkeypatch, x, W, gate, kind, dout, dev):
    import yt8m_amd.ensemble as ensemble
    monkeypatch.setattr(ops, "ENSEMBLE_FUSED", fused)
    xd = ensemble.stack_methods(x.permute(2, 0, 1).contiguous().to(dev))
    assert ops.ens_method_major(xd) and ops._ens_fused(xd, W.shape[0]) == fused
    Wd = W.to(dev).requires_grad_(True)
    gd = None if gate is None else gate.to(dev).requires_grad_(True)
    out = ops.ens_combine(xd, Wd, gd, xform=kind)
    assert (type(out.grad_fn).__name__ == "_EnsCombineBackward") == fused
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), Wd.grad.cpu(), None if gd is None else gd.grad.cpu()


@pytest.mark.parametrize("gated,kind", [(True, None), (False, "logit")])
def test_op_fused_against_composed(dev, monkeypatch, gated, kind):
    """ops.ens_combine with the kernels and in its composed torch form at (33, 256, 74, 4) (one table without a gate): values and the
    gradients that autograd hands to W [J, V, M] and gate, each against fp64 and against the other under R.bound.  Contiguous [B, V, M]
    inputs and inputs that require a gradient take the composed form."""
    Bn, V, M = 33, 256, 74
    J = 4 if gated else 1
    x, W, gate, dout = _case(Bn, V, M, J, gated, "plain", seed=77)
    f = _op_run(True, monkeypatch, x, W, gate, kind, dout, dev)
    c = _op_run(False, monkeypatch, x, W, gate, kind, dout, dev)
    r64 = R.combine_with_grads(x, W, gate, kind, dout, torch.float64)
    r32 = R.combine_with_grads(x, W, gate, kind, dout, torch.float32)
    for tag, a, b, i in (("out", f[0], c[0], 0), ("dW", f[1], c[1], 2), ("dgate", f[2], c[2], 3)):
        if a is None:
            continue
        bnd = R.bound(r32[i], r64[i])
        ef, ec, efc = (float((a.double() - r64[i]).abs().max()), float((b.double() - r64[i]).abs().max()), float((a - b).abs().max()))
        print("%s: fused %.3g composed %.3g fused - composed %.3g (bound %.3g)" % (tag, ef, ec, efc, bnd))
        assert ef <= bnd and efc <= 2 * bnd, tag                          # each within the bound of fp64: within twice of each other
    monkeypatch.setattr(ops, "ENSEMBLE_FUSED", True)
    xd = x.to(dev)
    assert not ops._ens_fused(xd, J)                                      # contiguous [B, V, M]
    assert not ops._ens_fused(xd.permute(2, 0, 1).contiguous().permute(1, 2, 0).requires_grad_(True), J)
    assert not ops._ens_fused(xd.permute(2, 0, 1).contiguous().permute(1, 2, 0), 5)             # more tables than the kernels take
    m, v = ops.ens_moments(xd.permute(2, 0, 1).contiguous().permute(1, 2, 0), variance=True)
    mc, vc = ops.ens_moments(xd, variance=True)
    m64, v64 = R.moments(x.double())
    assert float((m.cpu().double() - m64).abs().max()) <= R.bound(R.moments(x)[0], m64)
    assert float((v.cpu().double() - v64).abs().max()) <= R.bound(R.moments(x)[1], v64)
    assert float((mc.cpu().double() - m64).abs().max()) < 1e-6 and float((vc.cpu().double() - v64).abs().max()) < 1e-6


# ---- the plugins ------------------------------------------------------------------------------------------------------------------------
B, V, M, D, J, RANK, CELLS = 5, 37, 3, 6, 4, 2, 7
# tolerances of tests/test_gpu_lstmcnn.py::test_plugins_match_the_fp64_restatement: the gates' fully-connected layers run through the
# library's GEMMs
P_TOL, GRAD_TOL = 1e-4, 5e-4


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", sorted(R.PLUGINS))
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, fused):
    """Every plugin through create_model at B = 5, V = 37, M = 3 (J = 4 tables of rank 2, 7 relu cells, 6 input features): predictions
    and the gradient of EVERY variable, with the kernels and with the composed form of the op."""
    monkeypatch.setattr(ops, "ENSEMBLE_FUSED", fused)
    flags.moe_num_mixtures, flags.attention_matrix_rank, flags.attention_relu_cells = J, RANK, CELLS
    x, orig, P, coef = R.plugin_case(name, B, V, M, D, J, RANK, CELLS, seed=len(name))
    pred, grads, g = R.run_plugin(name, x, orig, P, coef, dev, J, RANK, CELLS)
    torch.cuda.synchronize()
    p64, g64 = R.plugin_reference(name, x, orig, P, coef)
    ep = float((pred.double() - p64).abs().max())
    unit = lambda k: float((grads[k].double() - g64[k]).abs().max()) / max(1.0, float(g64[k].abs().max()))
    print("%s fused=%d: predictions %.3g worst gradient %.3g" % (name, fused, ep, max([unit(k) for k in g64] + [0.0])))
    assert ep < P_TOL
    assert set(grads) == set(g64)
    for k in g64:
        assert unit(k) <= GRAD_TOL, k
        if k != "ensemble_bias":
            assert float(grads[k].abs().max()) > 0, k
    if name == "AttentionLinmatrixModel":
        assert bool((grads["ensemble_bias"] == 0).all())


def _train_case(name, dev, seed):
    rs = np.random.RandomState(seed)
    Bt, Vt, Mt = 6, 37, 3
    x = torch.from_numpy(rs.rand(Mt, Bt, Vt).astype(np.float32)).to(dev).permute(1, 2, 0)
    y = torch.from_numpy(rs.rand(Bt, Vt) < 0.2).to(dev)
    orig = torch.from_numpy(rs.randn(Bt, D).astype(np.float32)).to(dev)
    return x, y, orig


@pytest.mark.parametrize("name", ["MatrixRegressionModel", "AttentionMatrixModel", "AttentionMoeMatrixModel"])
def test_two_training_steps_and_their_bitwise_replay(dev, flags, monkeypatch, name):
    """Two EnsembleTrainGraph.step calls (cross entropy, clip, Adam) with the kernels: finite losses, every variable moved; the same two
    steps taken twice from the same state leave bit-identical parameters and Adam moments."""
    import yt8m_amd.ensemble as ensemble
    import yt8m_amd.ensemble_level_models as elm
    from yt8m_amd.variables import reset_default_graph
    monkeypatch.setattr(ops, "ENSEMBLE_FUSED", True)
    flags.moe_num_mixtures, flags.attention_matrix_rank, flags.attention_relu_cells = J, RANK, CELLS
    x, y, orig = _train_case(name, dev, 41)
    g = reset_default_graph(device=dev, seed=0)
    tg = ensemble.EnsembleTrainGraph(getattr(elm, name)(), batch_size=x.shape[0], graph=g)
    out = tg.step(x, y, original_input=orig)
    assert np.isfinite(float(out["loss"])) and tuple(out["predictions"].shape) == tuple(y.shape)
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
    assert all(torch.equal(a, b) for a, b in zip(*after))
    for v in g.trainable_variables():
        moved = not torch.equal(after[0][0][v.offset:v.offset + v.numel()], state[0][v.offset:v.offset + v.numel()])
        assert moved == (v.name != "ensemble_bias"), v.name


def test_two_level_run_over_prediction_dumps(dev, flags, monkeypatch, tmp_path):
    """Three dumps -> EnsembleInput -> MatrixRegressionModel trained for a few steps -> its predictions dumped -> that dump read as a
    method of a second EnsembleInput, bit for bit."""
    import yt8m_amd.ensemble as ensemble
    import yt8m_amd.ensemble_level_models as elm
    from yt8m_amd import inference
    from yt8m_amd.variables import reset_default_graph
    monkeypatch.setattr(ops, "ENSEMBLE_FUSED", True)
    Vd, n = 12, 10
    rs = np.random.RandomState(9)
    ids = [("vid%02d" % i).encode() for i in range(n)]
    labels = rs.rand(n, Vd) < 0.3
    files = []
    for k in range(3):
        # noisy views of the labels: something to learn
        p = np.clip(labels * 0.6 + rs.rand(n, Vd) * 0.4 * (k + 1) / 3.0, 0.0, 1.0).astype(np.float32)
        path = str(tmp_path / ("method%d.tfrecord" % k))
        inference.write_to_record(path, ids, labels, p)
        files.append([path])
    inp = ensemble.EnsembleInput(files, num_classes=Vd)
    g = reset_default_graph(device=dev, seed=0)
    tg = ensemble.EnsembleTrainGraph(elm.MatrixRegressionModel(), batch_size=n, graph=g, base_learning_rate=0.05)
    losses = []
    for _ in range(4):
        for vids, x, lab, original in inp.batches(batch_size=n, device=dev):
            assert x.is_cuda and x.stride() == (Vd, 1, n * Vd) and vids == ids
            losses.append(float(tg.step(x, lab)["loss"]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    vids, x, lab, _ = next(inp.batches(batch_size=n, device=dev))
    pred = tg.predict(x)
    second = str(tmp_path / "level2.tfrecord")
    inference.write_to_record(second, vids, lab, pred)
    got = list(ensemble.EnsembleInput([files[0], [second]], num_classes=Vd).batches(batch_size=n, device=dev))
    assert len(got) == 1
    _, x2, lab2, _ = got[0]
    assert tuple(x2.shape) == (n, Vd, 2) and torch.equal(x2[:, :, 1], pred) and torch.equal(x2[:, :, 0], x[:, :, 0])
    assert torch.equal(lab2, lab)
    mean = elm.MeanModel().create_model(x2)["predictions"]
    assert float((mean - (x2[:, :, 0] + x2[:, :, 1]) / 2).abs().max()) <= float(np.spacing(np.float32(1.0)))
