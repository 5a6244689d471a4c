"""CPU checks of the ensemble stage (youtube-8m_amd/ensemble.py, ensemble_level_models.py, ops.ens_combine / ens_moments, csrc/ensemble.hip's
C ABI): flags and the lookup by name, header / signature table / exports, every refusal without a device, each plugin on CPU tensors (the
composed form of the op) against the fp64 restatement of the reference's formulas in tests/ensemble_restatement.py, and EnsembleInput over
prediction dumps written by inference.write_to_record."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import ensemble_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_ens_max_gates", "yt8m_ens_combine_fwd", "yt8m_ens_combine_bwd_workspace_bytes", "yt8m_ens_combine_bwd", "yt8m_ens_moments")
B, V, M, D, J, RANK, CELLS = 5, 37, 3, 6, 4, 2, 7


def test_flags_and_classes_resolve(flags):
    import yt8m_amd.ensemble_level_models as elm
    import yt8m_amd.train as train
    assert flags.attention_matrix_rank == 3 and flags.attention_relu_cells == 128 and flags.moe_num_mixtures == 2
    for name in R.PLUGINS:
        assert train.find_class_by_name(name, [elm]) is getattr(elm, name)
    assert not hasattr(elm, "AttentionRectifiedLinearModel")            # undefined name at line 44 of the reference: cannot run there
    with pytest.raises(StopIteration):
        train.find_class_by_name("AttentionRectifiedLinearModel", [elm])
    assert "AttentionRectifiedLinearModel" in elm.__doc__ and "InputMoeModel" in elm.__doc__ and "EnsembleFrameReader" in elm.__doc__


def test_library_exports_and_header_declares_the_kernels():
    _, lib = declared_bound_exported(SYMBOLS, r"(int|int64_t)")
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved
    assert lib.yt8m_ens_max_gates() == 4


def test_every_refusal_is_badarg_and_launches_nothing():
    """Fake non-null pointers: a call that got past its checks would fault, so -1 also shows that nothing was launched."""
    lib = L.lib()
    p = [ctypes.c_void_p(64 * k) for k in range(1, 11)]
    fwd = lambda x=p[0], Wt=p[1], gate=p[2], xform=0, out=p[3], stat=p[4], B=2, V=8, M=3, J=2: lib.yt8m_ens_combine_fwd(
        x, Wt, gate, xform, out, stat, B, V, M, J, None)
    bwd = lambda x=p[0], Wt=p[1], gate=p[2], xform=0, out=p[3], stat=p[4], dout=p[5], dWt=p[6], dgate=p[7], ws=p[8], nbytes=1 << 30, B=2, V=8, \
        M=3, J=2: lib.yt8m_ens_combine_bwd(x, Wt, gate, xform, out, stat, dout, dWt, dgate, ws, nbytes, B, V, M, J, None)
    mom = lambda x=p[0], mean=p[1], var=p[2], B=2, V=8, M=3: lib.yt8m_ens_moments(x, mean, var, B, V, M, None)
    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(Wt=None) == -1 and call(out=None) == -1
        for dim in ("B", "V", "M"):
            assert call(**{dim: 0}) == -1 and call(**{dim: -2}) == -1
        assert call(J=0) == -1 and call(J=5) == -1 and call(J=-1) == -1  # the cap: yt8m_ens_max_gates() = 4
        assert call(xform=2) == -1 and call(xform=-1) == -1
        assert call(gate=None, J=2) == -1 if call is fwd else call(gate=None, dgate=None, J=2) == -1
    assert bwd(stat=None) == -1 and bwd(dout=None) == -1 and bwd(dWt=None) == -1
    assert bwd(dgate=None) == -1 and bwd(gate=None, J=1) == -1           # dgate goes with gate
    assert bwd(ws=None) == -1 and bwd(nbytes=12) == -1             # 16 bytes are needed here
    assert mom(x=None) == -1 and mom(mean=None) == -1 and mom(B=0) == -1 and mom(V=-1) == -1 and mom(M=0) == -1
    assert mom(M=1) == -1                                                # the unbiased variance of one method
    assert lib.yt8m_ens_combine_bwd_workspace_bytes(0, 8, 3, 2) == -1 and lib.yt8m_ens_combine_bwd_workspace_bytes(2, 8, 3, 5) == -1
    # one chunk: only the dgate partials of the single-element path (ceil(8 / 64) tiles x ceil(3 / 8) ranges) x B x J floats
    assert lib.yt8m_ens_combine_bwd_workspace_bytes(2, 8, 3, 2) == 1 * 2 * 2 * 4
    # 17 rows: two chunks of partial tables in front of them
    assert lib.yt8m_ens_combine_bwd_workspace_bytes(17, 8, 3, 2) == (2 * 2 * 3 * 8 + 1 * 17 * 2) * 4


def test_glorot_uniform_follows_the_fan_rule_of_tf_1_0():
    from yt8m_amd.variables import glorot_uniform
    gen = torch.Generator().manual_seed(0)
    for shape, fans in (((50,), 100), ((30, 70), 100), ((4, 30, 70), 400), ((4, 1, 1), 8)):
        t = glorot_uniform(shape, gen, torch.device("cpu"))
        lim = math.sqrt(6.0 / fans)
        assert tuple(t.shape) == shape and float(t.abs().max()) <= lim
        if t.numel() >= 50:
            assert float(t.abs().max()) > 0.8 * lim


# ---- the op on the CPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated,kind", [(True, None), (False, None), (True, "logit"), (False, "logit")])
def test_op_on_cpu_tensors_is_the_composed_form(monkeypatch, gated, kind):
    """CPU tensors take the torch form whatever the switch says; values and both gradients against the fp64 restatement under its own
    bound (4 x the float32 restatement's error + one ulp)."""
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "ENSEMBLE_FUSED", True)
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(B, V, M, generator=gen)
    x[0, 0, 0], x[1, 2, 1] = 0.0, 1.0
    W = torch.randn(J if gated else 1, V, M, generator=gen).requires_grad_(True)
    gate = torch.softmax(torch.randn(B, J, generator=gen), -1).requires_grad_(True) if gated else None
    dout = torch.randn(B, V, generator=gen)
    out = ops.ens_combine(x, W, gate, xform=kind)
    out.backward(dout)
    o64, _, dW64, dg64 = R.combine_with_grads(x, W.detach(), None if gate is None else gate.detach(), kind, dout, torch.float64)
    o32, _, dW32, dg32 = R.combine_with_grads(x, W.detach(), None if gate is None else gate.detach(), kind, dout, torch.float32)
    assert float((out.detach().double() - o64).abs().max()) <= R.bound(o32, o64)
    assert float((W.grad.double() - dW64).abs().max()) <= R.bound(dW32, dW64)
    if gated:
        assert float((gate.grad.double() - dg64).abs().max()) <= R.bound(dg32, dg64)
    mean, var = ops.ens_moments(x, variance=True)
    m64, v64 = R.moments(x.double())
    m32, v32 = R.moments(x)
    assert float((mean.double() - m64).abs().max()) <= R.bound(m32, m64) and float((var.double() - v64).abs().max()) <= R.bound(v32, v64)
    with pytest.raises(ValueError):
        ops.ens_combine(x, W, gate, xform="probit")
    with pytest.raises(ValueError):
        ops.ens_combine(x, torch.zeros(2, V, M), None)
    with pytest.raises(ValueError):
        ops.ens_moments(x[:, :, :1], variance=True)


# ---- the plugins on the CPU graph -----------------------------------------------------------------------------------------------------
def _cpu_native(monkeypatch):
    """The three native calls of the gate's fully-connected layers as torch ops on the CPU; the variables still enter through
    ops.as_tensor, so their gradients land in the arena as on the device."""
    import yt8m_amd.ops as ops

    def linear(x, W, b=None, bf16=None):
        y = x @ ops.as_tensor(W)
        return y if b is None else y + ops.as_tensor(b)

    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "l2norm_fwd", lambda x, eps=1e-12: x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=eps)))
    monkeypatch.setattr(ops, "activation", lambda x, kind: {"relu": torch.relu}[kind](x))
    return ops


def _plugin_flags(flags):
    flags.moe_num_mixtures, flags.attention_matrix_rank, flags.attention_relu_cells = J, RANK, CELLS


# float32 arithmetic against fp64 on sums of at most D + V = 43 terms of magnitude <= a few: 1e-5 on predictions in [0, 1]; gradients
# relative to the largest entry of the variable's fp64 gradient (or 1), 1e-4
P_TOL, GRAD_TOL = 1e-5, 1e-4


@pytest.mark.parametrize("name", sorted(R.PLUGINS))
def test_plugin_on_cpu_tensors_against_the_fp64_restatement(monkeypatch, flags, name):
    _plugin_flags(flags)
    _cpu_native(monkeypatch)
    x, orig, P, coef = R.plugin_case(name, B, V, M, D, J, RANK, CELLS, seed=len(name))
    pred, grads, g = R.run_plugin(name, x, orig, P, coef, torch.device("cpu"), J, RANK, CELLS)
    p64, g64 = R.plugin_reference(name, x, orig, P, coef)
    assert tuple(pred.shape) == (B, V)
    assert float((pred.double() - p64).abs().max()) < P_TOL
    assert set(grads) == set(g64)
    for k in g64:
        err = float((grads[k].double() - g64[k]).abs().max()) / max(1.0, float(g64[k].abs().max()))
        assert err < GRAD_TOL, (k, err)
        if k != "ensemble_bias" and name != "MeanModel":
            assert float(g64[k].abs().max()) > 0 and float(grads[k].abs().max()) > 0, k
    l2 = {v.name: v.l2 for v in g.vars.values()}
    if name == "MatrixRegressionModel":
        assert l2 == {"ensemble_weight1d": 1e-8, "ensemble_weight2d": 1e-7}                       # 10 x the penalty on the matrix
    if name == "AttentionLinmatrixModel":
        assert l2["ensemble_bias"] == 0.0 and l2["ensemble_weight"] == 1e-8
        assert bool((grads["ensemble_bias"] == 0).all())                                         # exactly zero, not merely small
        assert float(g64["ensemble_bias"].abs().max()) < 1e-12                                   # and zero in the reference's formula too


def test_attention_plugins_need_original_input(monkeypatch, flags):
    import yt8m_amd.ensemble_level_models as elm
    from yt8m_amd.variables import reset_default_graph
    _plugin_flags(flags)
    _cpu_native(monkeypatch)
    for name in ("AttentionLinearModel", "AttentionMatrixModel", "AttentionLinmatrixModel", "AttentionMoeMatrixModel"):
        reset_default_graph(device=torch.device("cpu"), seed=0).begin_step()
        with pytest.raises(ValueError, match="original_input"):
            getattr(elm, name)().create_model(torch.rand(B, V, M), vocab_size=V)


def test_ensemble_train_graph_fixes_the_identical_transformer():
    import yt8m_amd.ensemble as ensemble
    import yt8m_amd.ensemble_level_models as elm
    import yt8m_amd.feature_transform as ft
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    tg = ensemble.EnsembleTrainGraph(elm.MeanModel(), batch_size=4, graph=g)
    assert type(tg.transformer) is ft.IdenticalTransformer
    x = torch.rand(4, 6, 3)
    assert torch.equal(tg.predict(x), x.mean(2))                         # no l2-normalisation of the predictions
    with pytest.raises(ValueError):
        ensemble.EnsembleTrainGraph(elm.MeanModel(), graph=g, transformer_class=ft.DefaultTransformer)


# ---- EnsembleInput ----------------------------------------------------------------------------------------------------------------------
def _write_dumps(tmp_path, n_methods, ids, labels, seed, feature_name="predictions"):
    from yt8m_amd import inference
    rs = np.random.RandomState(seed)
    preds, files = [], []
    for k in range(n_methods):
        p = rs.rand(len(ids), labels.shape[1]).astype(np.float32)
        d = tmp_path / ("method%d" % k)
        d.mkdir()
        # two shards per method, 4 + 3 videos
        inference.write_to_record(str(d / "predictions-0000.tfrecord"), ids[:4], labels[:4], p[:4], feature_name)
        inference.write_to_record(str(d / "predictions-0001.tfrecord"), ids[4:], labels[4:], p[4:], feature_name)
        preds.append(p)
        files.append(sorted(str(f) for f in d.iterdir()))
    return preds, files


def test_ensemble_input_yields_the_method_major_view_and_raises_on_an_id_mismatch(tmp_path):
    import yt8m_amd.ensemble as ensemble
    Vd, n = 12, 7
    ids = [("vid%02d" % i).encode() for i in range(n)]
    rs = np.random.RandomState(1)
    labels = rs.rand(n, Vd) < 0.3
    preds, files = _write_dumps(tmp_path, 3, ids, labels, seed=2)
    inp = ensemble.EnsembleInput(files, num_classes=Vd)
    got = list(inp.batches(batch_size=3))
    assert [len(b[0]) for b in got] == [3, 1, 3]                         # batches never span shards
    row = 0
    for vids, x, lab, original in got:
        k = len(vids)
        assert vids == ids[row:row + k] and original is None
        assert tuple(x.shape) == (k, Vd, 3) and x.stride() == (Vd, 1, k * Vd)
        assert x.permute(2, 0, 1).is_contiguous()
        for m in range(3):
            assert np.array_equal(x[:, :, m].numpy(), preds[m][row:row + k])                      # bit-exact planes
        assert np.array_equal(lab.numpy(), labels[row:row + k])                                   # labels of the first method
        row += k
    assert row == n
    # a method whose second shard holds other videos
    from yt8m_amd import inference
    other = list(ids)
    other[5] = b"vidXX"
    inference.write_to_record(files[1][1], other[4:], labels[4:], preds[1][4:])
    it = ensemble.EnsembleInput(files, num_classes=Vd).batches(batch_size=4)
    next(it)
    with pytest.raises(ValueError, match="video ids of method 1 differ"):
        next(it)
    # a method with fewer videos
    inference.write_to_record(files[1][1], ids[4:6], labels[4:6], preds[1][4:6])
    it = ensemble.EnsembleInput(files, num_classes=Vd).batches(batch_size=4)
    next(it)
    with pytest.raises(ValueError):
        next(it)
    with pytest.raises(ValueError):
        ensemble.EnsembleInput([])


def test_ensemble_input_reads_and_checks_the_original_input(tmp_path):
    import yt8m_amd.ensemble as ensemble
    from yt8m_amd import inference
    Vd, n = 12, 7
    ids = [("vid%02d" % i).encode() for i in range(n)]
    labels = np.random.RandomState(4).rand(n, Vd) < 0.3
    preds, files = _write_dumps(tmp_path, 2, ids, labels, seed=5)
    # the input features travel in the same container: a float feature "mean_rgb" of width Vd per video
    feats = np.random.RandomState(6).randn(n, Vd).astype(np.float32)
    d = tmp_path / "model_input"
    d.mkdir()
    inference.write_to_record(str(d / "a-0000.tfrecord"), ids[:4], labels[:4], feats[:4], "mean_rgb")
    inference.write_to_record(str(d / "a-0001.tfrecord"), ids[4:], labels[4:], feats[4:], "mean_rgb")
    kw = dict(num_classes=Vd, input_data_pattern=str(d / "*.tfrecord"), input_feature_names=["mean_rgb"], input_feature_sizes=[Vd])
    got = list(ensemble.EnsembleInput(files, **kw).batches(batch_size=4))
    assert np.array_equal(torch.cat([b[3] for b in got]).numpy(), feats)
    inference.write_to_record(str(d / "a-0001.tfrecord"), [b"zz"] + ids[5:], labels[4:], feats[4:], "mean_rgb")
    it = ensemble.EnsembleInput(files, **kw).batches(batch_size=4)
    next(it)
    with pytest.raises(ValueError, match="input features"):
        next(it)
