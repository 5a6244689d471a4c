"""CPU checks of the ensemble stage's MoE plugins (ensemble_level_models.MoeModel / InputMoeModel / AttentionMoeModel, ops.ens_tensor_moe /
ens_mix, csrc/ensemble_tensor.hip's C ABI): the lookup by name, header / signature table / exports, every refusal without a device, the
composed ops and each plugin on CPU tensors against the fp64 restatement of tests/ensemble_moe_restatement.py, and the backward formulas
that the kernels implement against autograd in fp64."""
import ctypes
import os
import re

import pytest
import torch

import ensemble_moe_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_ens_tensor_max_methods", "yt8m_ens_tensor_fwd", "yt8m_ens_tensor_bwd_workspace_bytes", "yt8m_ens_tensor_bwd",
           "yt8m_ens_mix_fwd", "yt8m_ens_mix_bwd")
B, V, M, D, CELLS = 5, 37, 3, 6, 7


def test_classes_resolve_and_the_left_out_names_do_not(flags):
    import yt8m_amd.ensemble_level_models as elm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    assert flags.attention_relu_cells == 128
    for name in R.PLUGINS:
        assert train.find_class_by_name(name, [elm]) is getattr(elm, name)
    assert elm.MoeModel is not vlm.MoeModel and elm.MoeModel.__module__.endswith("ensemble_level_models")
    for name in ("DeepCombineChainModel", "LogisticModel"):
        assert not hasattr(elm, name)
        with pytest.raises(StopIteration):
            train.find_class_by_name(name, [elm])
        assert name in elm.__doc__


def test_switches_are_read_at_import():
    import yt8m_amd.ops as ops
    src = open(os.path.join(ROOT, "youtube-8m_amd", "ops.py")).read()
    for env, attr in (("YT8M_ENS_TENSOR_FUSED", "ENS_TENSOR_FUSED"), ("YT8M_ENS_MIX_FUSED", "ENS_MIX_FUSED")):
        default = re.search(r'^%s = os\.environ\.get\("%s", "([01])"\) != "0"$' % (attr, env), src, re.M)
        assert default, env
        if env not in os.environ:
            assert getattr(ops, attr) == (default.group(1) == "1")


def test_library_exports_and_header_declares_the_kernels():
    _, lib = declared_bound_exported(SYMBOLS, r"(int|int64_t)")
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved
    assert lib.yt8m_ens_tensor_max_methods() >= 80


def test_every_refusal_is_badarg_and_launches_nothing():
    """Fake non-null pointers: a call that got past its checks would fault, so -1 also shows that nothing was launched."""
    lib = L.lib()
    top = lib.yt8m_ens_tensor_max_methods()
    p = [ctypes.c_void_p(64 * k) for k in range(1, 11)]
    fwd = lambda x=p[0], Wt=p[1], bt=p[2], out=p[3], stat=p[4], B=2, V=8, M=3: lib.yt8m_ens_tensor_fwd(x, Wt, bt, out, stat, B, V, M, None)
    bwd = lambda x=p[0], Wt=p[1], bt=p[2], out=p[3], stat=p[4], dout=p[5], dWt=p[6], dbt=p[7], ws=p[8], nbytes=1 << 30, B=2, V=8, M=3: \
        lib.yt8m_ens_tensor_bwd(x, Wt, bt, out, stat, dout, dWt, dbt, ws, nbytes, B, V, M, None)
    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(Wt=None) == -1 and call(bt=None) == -1 and call(out=None) == -1
        for dim in ("B", "V", "M"):
            assert call(**{dim: 0}) == -1 and call(**{dim: -2}) == -1
        assert call(M=top + 1) == -1
    assert bwd(stat=None) == -1 and bwd(dout=None) == -1 and bwd(dWt=None) == -1 and bwd(dbt=None) == -1
    need = lib.yt8m_ens_tensor_bwd_workspace_bytes(2, 8, 3)
    assert need >= 0 and bwd(nbytes=need - 1) == -1                      # a workspace smaller than asked for
    if need > 0:
        assert bwd(ws=None, nbytes=need) == -1
    for bad in ((0, 8, 3), (2, -1, 3), (2, 8, 0), (2, 8, top + 1)):
        assert lib.yt8m_ens_tensor_bwd_workspace_bytes(*bad) == -1
    mf = lambda x=p[0], a=p[1], out=p[2], B=2, V=8, M=3: lib.yt8m_ens_mix_fwd(x, a, out, B, V, M, None)
    mb = lambda x=p[0], dout=p[1], da=p[2], B=2, V=8, M=3: lib.yt8m_ens_mix_bwd(x, dout, da, B, V, M, None)
    assert mf(x=None) == -1 and mf(a=None) == -1 and mf(out=None) == -1
    assert mb(x=None) == -1 and mb(dout=None) == -1 and mb(da=None) == -1
    for call in (mf, mb):
        for dim in ("B", "V", "M"):
            assert call(**{dim: 0}) == -1 and call(**{dim: -2}) == -1


def test_every_instantiation_compiles_without_scratch():
    """hipcc's own resource remarks for csrc/ensemble_tensor.hip (cross-compiles without a GPU): no kernel owns a stack object or
    spills a VGPR -- a thread's rows (forward) or weight and gradient columns (backward) stay in registers."""
    import subprocess
    csrc = os.path.join(ROOT, "youtube-8m_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "--cuda-device-only", "-c",
           "ensemble_tensor.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(n) for n in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    spills = [int(n) for n in re.findall(r"VGPRs Spill: (\d+)", p.stderr)]
    assert len(names) == 9 and len(scratch) == 9 and len(spills) == 9   # 3 + 3 matrix kernels, 2 + 1 mix kernels
    assert sum("ens_tensor_fwd_kernel" in n for n in names) == 3 and sum("ens_tensor_bwd_kernel" in n for n in names) == 3
    assert scratch == [0] * 9 and spills == [0] * 9, dict(zip(names, zip(scratch, spills)))


# ---- the ops on the CPU -----------------------------------------------------------------------------------------------------------------
def _case(seed, Bn=B, Vn=V, Mn=M):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(Bn, Vn, Mn, generator=gen)
    x[0, 0, 0], x[1, 2, Mn - 1] = 0.0, 1.0
    W = torch.rand(Vn, Mn, Mn, generator=gen) * 2.0 - 1.0
    b = torch.randn(Vn, Mn, generator=gen)
    a = torch.softmax(torch.randn(Bn, Mn, generator=gen), dim=-1)
    return x, W, b, a, torch.randn(Bn, Vn, generator=gen)


def test_ops_on_cpu_tensors_are_the_composed_forms(monkeypatch):
    """CPU tensors take the torch forms whatever the switches say (counted as such); values and gradients against the fp64 restatement
    under its own bound (4 x the float32 restatement's error + one ulp)."""
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "ENS_TENSOR_FUSED", True)
    monkeypatch.setattr(ops, "ENS_MIX_FUSED", True)
    x, W, b, a, dout = _case(3)
    before = dict(ops.ENS_TENSOR_CALLS), dict(ops.ENS_MIX_CALLS)
    Wl, bl, al = W.clone().requires_grad_(True), b.clone().requires_grad_(True), a.clone().requires_grad_(True)
    out = ops.ens_tensor_moe(x, Wl, bl)
    out.backward(dout)
    r64, r32 = R.tensor_moe_with_grads(x, W, b, dout, torch.float64), R.tensor_moe_with_grads(x, W, b, dout, torch.float32)
    for got, i in ((out.detach(), 0), (Wl.grad, 2), (bl.grad, 3)):
        assert float((got.double() - r64[i]).abs().max()) <= R.bound(r32[i], r64[i]), i
    mo = ops.ens_mix(x, al)
    mo.backward(dout)
    m64, m32 = R.mix_with_grads(x, a, dout, torch.float64), R.mix_with_grads(x, a, dout, torch.float32)
    assert float((mo.detach().double() - m64[0]).abs().max()) <= R.bound(m32[0], m64[0])
    assert float((al.grad.double() - m64[1]).abs().max()) <= R.bound(m32[1], m64[1])
    assert ops.ENS_TENSOR_CALLS == {"kernels": before[0]["kernels"], "composed": before[0]["composed"] + 1}
    assert ops.ENS_MIX_CALLS == {"kernels": before[1]["kernels"], "composed": before[1]["composed"] + 1}
    with pytest.raises(ValueError):
        ops.ens_tensor_moe(x, W[:, :, :2], b)
    with pytest.raises(ValueError):
        ops.ens_tensor_moe(x, W, b[:, :2])
    with pytest.raises(ValueError):
        ops.ens_mix(x, a[:, :2])


@pytest.mark.parametrize("Mn", [1, 3, 9])
def test_the_backward_formulas_of_the_kernels_are_autograds_in_fp64(Mn):
    """dg = dout p (x - out), dW[v,k,l] = sum_b x[b,v,k] dg[b,v,l], db = sum_b dg; da[b,k] = sum_v dout[b,v] x[b,v,k]: against autograd
    in fp64, to rounding.  With one method out is x and both gradients are exactly zero."""
    x, W, b, a, dout = (t.double() for t in _case(11 + Mn, Mn=Mn))
    out, dW, db = R.tensor_moe_formulas(x, W, b, dout)
    o64, _, dW64, db64 = R.tensor_moe_with_grads(x, W, b, dout, torch.float64)
    assert float((out - o64).abs().max()) < 1e-14 and float((dW - dW64).abs().max()) < 1e-13 and float((db - db64).abs().max()) < 1e-13
    if Mn == 1:
        assert torch.equal(out, x[:, :, 0]) and bool((dW == 0).all()) and bool((db == 0).all())
    mo, da = R.mix_formulas(x, a, dout)
    m64, da64 = R.mix_with_grads(x, a, dout, torch.float64)
    assert float((mo - m64).abs().max()) < 1e-14 and float((da - da64).abs().max()) < 1e-13


# ---- the plugins on the CPU graph -----------------------------------------------------------------------------------------------------
def _cpu_native(monkeypatch):
    """The native calls of the fully-connected layers as torch ops on the CPU (tests/test_ensemble_host.py's); the variables still enter
    through ops.as_tensor, so their gradients land in the arena as on the device."""
    import yt8m_amd.ops as ops

    def linear(x, W, b=None, bf16=None):
        y = x @ ops.as_tensor(W)
        return y if b is None else y + ops.as_tensor(b)

    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "l2norm_fwd", lambda x, eps=1e-12: x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=eps)))
    monkeypatch.setattr(ops, "activation", lambda x, kind: {"relu": torch.relu}[kind](x))
    return ops


# float32 arithmetic against fp64 on sums of at most V = 37 terms of magnitude <= a few (tests/test_ensemble_host.py's tolerances)
P_TOL, GRAD_TOL = 1e-5, 1e-4


@pytest.mark.parametrize("name", sorted(R.PLUGINS))
def test_plugin_on_cpu_tensors_against_the_fp64_restatement(monkeypatch, flags, name):
    flags.attention_relu_cells = CELLS
    _cpu_native(monkeypatch)
    x, orig, P, coef = R.plugin_case(name, B, V, M, D, CELLS, seed=len(name))
    pred, grads, g = R.run_plugin(name, x, orig, P, coef, torch.device("cpu"), CELLS)
    p64, g64 = R.plugin_reference(name, x, orig, P, coef)
    assert tuple(pred.shape) == (B, V)
    assert float((pred.double() - p64).abs().max()) < P_TOL
    assert set(grads) == set(g64)
    for k in g64:
        err = float((grads[k].double() - g64[k]).abs().max()) / max(1.0, float(g64[k].abs().max()))
        assert err < GRAD_TOL, (k, err)
        assert float(g64[k].abs().max()) > 0 and float(grads[k].abs().max()) > 0, k
    l2 = {v.name: v.l2 for v in g.vars.values()}
    if name == "MoeModel":
        assert l2 == {"tensor_weight": 1e-8, "tensor_bias": 1e-8}
    if name == "AttentionMoeModel":
        assert l2["gate/weights"] == 1e-8 and l2["relu-sub0/weights"] == 1e-8 and "gate/biases" not in l2


def test_moe_model_initialisers(flags):
    """tensor_weight: glorot_uniform with the N-D fans of variables.py (limit sqrt(6 / (2 M V))); tensor_bias: zeros."""
    import math

    import yt8m_amd.ensemble_level_models as elm
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=torch.device("cpu"), seed=0)
    g.begin_step()
    elm.MoeModel().create_model(torch.rand(2, 40, 5), vocab_size=40)
    W, b = g.vars["tensor_weight"].data, g.vars["tensor_bias"].data
    lim = math.sqrt(6.0 / (2 * 5 * 40))
    assert tuple(W.shape) == (40, 5, 5) and 0.8 * lim < float(W.abs().max()) <= lim
    assert tuple(b.shape) == (40, 5) and bool((b == 0).all())


def test_input_and_attention_moe_need_original_input(monkeypatch, flags):
    import yt8m_amd.ensemble_level_models as elm
    from yt8m_amd.variables import reset_default_graph
    flags.attention_relu_cells = CELLS
    _cpu_native(monkeypatch)
    for name in ("InputMoeModel", "AttentionMoeModel"):
        reset_default_graph(device=torch.device("cpu"), seed=0).begin_step()
        with pytest.raises(ValueError, match="original_input"):
            getattr(elm, name)().create_model(torch.rand(B, V, M), vocab_size=V)
