"""CPU checks of the input-memory LSTM plugins (Z/frame_level_models.py:631-885) and of their layer's C ABI (csrc/glu_lstm.hip): the
lookup by name, the 24 Variables per layer (names, shapes, l2, initial values), the header / signature table / exports, argument
validation without a device, and the composed form of seq_ops.glu_lstm_layer against the fp64 restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import glu_lstm_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_glu_lstm_supported", "yt8m_glu_lstm_layer_fwd", "yt8m_glu_lstm_layer_bwd")
PLUGINS = ("LstmGlu2Model", "LstmGlu2MultilayerModel")


def test_find_class_by_name_resolves_both_models():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    for name in PLUGINS:
        cls = train.find_class_by_name(name, [flm, vlm])
        assert cls is getattr(flm, name) and not hasattr(vlm, name)
        assert cls.accepts_quantized_input is True


def test_library_exports_and_header_declares_the_glu_lstm_symbols():
    src, lib = declared_bound_exported(SYMBOLS)
    assert "Z/frame_level_models.py:695-792" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits():
    lib = L.lib()
    for B, H, D, ok in ((128, 1024, 1152, 1), (3, 256, 64, 1), (5, 2048, 2048, 1), (1, 512, 4, 1), (128, 1024, 1024, 1),
                        (128, 192, 1152, 0), (128, 2304, 1152, 0), (128, 0, 1152, 0), (0, 1024, 1152, 0), (128, 128, 1152, 0),
                        (128, 1024, 1150, 0), (128, 1024, 2052, 0), (128, 1024, 0, 0), (128, 1024, 2, 0)):
        assert lib.yt8m_glu_lstm_supported(B, H, D) == ok, (B, H, D)


def test_argument_validation_without_device():
    """Every call here fails validation or has nothing to do: nothing is launched and no device is needed."""
    lib = L.lib()
    OK, BADARG, SHAPE = 0, -1, -2
    p = [ctypes.c_void_p(256 * k) for k in range(1, 32)]
    H, D = 256, 64
    fwd_ptrs = dict(zv=p[0], pv=p[1], zs=p[2], Uv=p[3], Us=p[4], x=p[5], xq=None, xr=None, hs=p[6], cs=p[7], qv=p[8], qs=p[9], xm=p[10],
                    n2=p[11], c_last=p[12], nf=p[13])

    def fwd(ldv=2 * H, lds=8, ldu=2 * H, F=4, B=3, H=H, D=D, **kw):
        a = dict(fwd_ptrs, **kw)
        return lib.yt8m_glu_lstm_layer_fwd(a["zv"], a["pv"], ldv, a["zs"], lds, a["Uv"], ldu, a["Us"], a["x"], a["xq"], a["xr"], a["hs"],
                                           a["cs"], a["qv"], a["qs"], a["xm"], a["n2"], a["c_last"], a["nf"], F, B, H, D, None, 0, None)

    bwd_ptrs = dict(fwd_ptrs, dout=p[14], dc_last=p[15], dzv=p[16], dpv=p[17], dzs=p[18], dx_direct=p[19], work=p[20])
    del bwd_ptrs["c_last"]

    def bwd(ldv=2 * H, lds=8, ldu=2 * H, lddv=2 * H, F=4, B=3, H=H, D=D, **kw):
        a = dict(bwd_ptrs, **kw)
        return lib.yt8m_glu_lstm_layer_bwd(a["zv"], a["pv"], ldv, a["zs"], lds, a["Uv"], ldu, a["Us"], a["x"], a["xq"], a["xr"], a["hs"],
                                           a["cs"], a["qv"], a["qs"], a["xm"], a["n2"], a["dout"], a["dc_last"], a["dzv"], a["dpv"], lddv,
                                           a["dzs"], a["dx_direct"], a["work"], a["nf"], F, B, H, D, None, 0, None)

    for call in (fwd, bwd):
        assert call(F=-1) == SHAPE and call(B=-1) == SHAPE and call(H=-256) == SHAPE and call(D=-4) == SHAPE     # negative size
        assert call(ldu=2 * H - 1) == SHAPE and call(ldv=2 * H - 1) == SHAPE                                    # small ldu / ldv
        assert call(lds=7) == SHAPE and call(lds=4) == SHAPE                                                    # lds < 8
        assert call(H=192, ldu=384, ldv=384) == SHAPE and call(H=2304, ldu=4608, ldv=4608) == SHAPE             # what _supported refuses
        assert call(D=66) == SHAPE and call(D=2052) == SHAPE and call(D=0) == SHAPE
        for name in ("zv", "pv", "zs", "Uv", "Us", "hs", "cs", "qv", "qs", "xm", "n2"):
            assert call(**{name: None}) == BADARG, name                                                         # null operand
        assert call(x=None) == BADARG and call(xq=p[21]) == BADARG                  # neither kind of frames; both
        assert call(x=None, xq=p[21]) == BADARG                                     # bytes without their row scales
        assert call(x=ctypes.c_void_p(260)) == BADARG and call(xm=ctypes.c_void_p(264)) == BADARG               # misaligned float4 rows
        assert call(x=None, xq=ctypes.c_void_p(258), xr=p[22]) == BADARG
        assert call(F=0) == OK and call(B=0) == OK and call(H=0) == OK                                          # nothing to do
        assert call(F=0, **{k: None for k in fwd_ptrs if k != "c_last"}) == OK                                  # ... before anything else
    assert bwd(lddv=2 * H - 1) == SHAPE
    for name in ("dzv", "dpv", "dzs", "work"):
        assert bwd(**{name: None}) == BADARG, name
    assert bwd(dx_direct=ctypes.c_void_p(260)) == BADARG
    # num_frames may be null only together with c_last / dc_last
    assert fwd(nf=None) == BADARG and bwd(nf=None) == BADARG
    assert b"glu_lstm" in lib.yt8m_last_error()


# ---- the plugins' Variables on the CPU graph ----------------------------------------------------------------------------------------
def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


def _stub_head(monkeypatch):
    """ops.moe_head has no CPU form: the MoE of the restatement on the Variables' data stands in for it."""
    import yt8m_amd.ops as ops
    monkeypatch.setattr(ops, "moe_head", lambda x, Wg, We, be, V_, M_, **k: R.moe(x, Wg.data, We.data, be.data, M_))


def _check_unit(g, scope, D, H):
    assert len(R.NAMES) == 24 and len(set(R.NAMES)) == 24
    for n, shape in R.shapes(D, H).items():
        v = g.vars["%s/%s" % (scope, n)]
        assert tuple(v.data.shape) == shape and v.l2 == 1e-8 and v.trainable, (scope, n)
        if n in ("bf", "bfx"):
            assert float(v.data) == 1.0, n
        elif n[0] == "b":
            assert bool((v.data == np.float32(0.1)).all()), n
        elif v.data.numel() >= 64:
            assert float(v.data.abs().max()) <= 0.2 + 1e-7 and float(v.data.std()) > 0.03, n       # truncated at two stddev of 0.1
        else:
            assert float(v.data.abs().max()) <= 0.2 + 1e-7 and float(v.data.abs().max()) > 0.0, n


def test_shapes_follow_the_reference():
    s = R.shapes(8, 16)
    assert s["Wi"] == (8, 1) and s["Ui"] == (16, 1) and s["Vi"] == (8, 1) and s["bi"] == (1,) and s["Vfx"] == (8, 1) and s["Ufx"] == (16, 1)
    assert s["Wog"] == (8, 16) and s["Vog"] == (8, 16) and s["Uog"] == (16, 16) and s["bog"] == (16,)
    assert s["Wc"] == (8, 16) and s["Vc"] == (8, 16) and s["Uc"] == (16, 16) and s["bc"] == (16,) and s["bfx"] == (1,)


def test_lstm_glu2_model_variables(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _stub_head(monkeypatch)
    flags.lstm_cells, flags.moe_num_mixtures = "16", 2
    g = _graph()
    B, F, D, V = 3, 5, 8, 10
    res = flm.LstmGlu2Model().create_model(torch.randn(B, F, D), vocab_size=V, num_frames=torch.tensor([5, 1, 3]))
    assert tuple(res["predictions"].shape) == (B, V)
    names = ["lstm_forward/" + n for n in R.NAMES] + ["gates/weights", "experts/weights", "experts/biases"]
    assert list(g.vars) == names                                          # create_recurrent_unit's order
    _check_unit(g, "lstm_forward", D, 16)
    assert tuple(g.vars["gates/weights"].data.shape) == (16, V * 3)


def test_lstm_glu2_multilayer_model_variables(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _stub_head(monkeypatch)
    flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures = "16", 2, 2
    g = _graph()
    B, F, D, V = 3, 5, 8, 10
    res = flm.LstmGlu2MultilayerModel().create_model(torch.randn(B, F, D), vocab_size=V, num_frames=torch.tensor([5, 1, 3]))
    assert tuple(res["predictions"].shape) == (B, V)
    names = ["lstm_lsyer%dlstm_forward/%s" % (l, n) for l in range(2) for n in R.NAMES] + ["gates/weights", "experts/weights", "experts/biases"]
    assert list(g.vars) == names                                          # the reference's spelling
    _check_unit(g, "lstm_lsyer0lstm_forward", D, 16)
    _check_unit(g, "lstm_lsyer1lstm_forward", 16, 16)                     # layer 1 reads layer 0's hidden outputs
    assert tuple(g.vars["gates/weights"].data.shape) == (2 * 16, V * 3)   # the layers' memories concatenated


# ---- the composed form against the restatement ------------------------------------------------------------------------------------
F_, B_, D_, H_ = 6, 3, 8, 16


@pytest.mark.parametrize("nf", [[6, 1, 3], [0, 6, 2]])
def test_composed_form_matches_the_restatement_in_fp64(nf):
    import yt8m_amd.seq_ops as seq_ops
    rs = np.random.RandomState(11)
    P = R.random_unit(rs, D_, H_)
    x = rs.randn(F_, B_, D_).astype(np.float32)
    dout, dc = rs.randn(F_, B_, H_).astype(np.float32), rs.randn(B_, H_).astype(np.float32)
    ref = R.layer_with_grads(x, nf, P, dout, dc, torch.float64)
    Pt = R.to_torch(P, torch.float64, True)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    before = dict(seq_ops.GLU_LSTM_CALLS)
    out, c_last = seq_ops.glu_lstm_layer(xt, *R.operands(Pt), torch.tensor(nf))
    assert seq_ops.GLU_LSTM_CALLS["composed"] == before["composed"] + 1 and seq_ops.GLU_LSTM_CALLS["kernels"] == before["kernels"]
    assert tuple(out.shape) == (F_, B_, H_) and tuple(c_last.shape) == (B_, H_)
    ((out * torch.from_numpy(dout).double()).sum() + (c_last * torch.from_numpy(dc).double()).sum()).backward()   # through both returns
    got = {"out": out, "c_last": c_last, "dx": xt.grad}
    got.update({"d" + n: Pt[n].grad for n in R.NAMES})
    for k in ref:
        assert float(np.abs(ref[k]).max()) > 0.0, k                      # every one of the 24 Variables takes part
        assert R.err(got[k], ref[k]) < 1e-12, k
    for b, n in enumerate(nf):
        if n < 1:
            assert float(c_last[b].detach().abs().max()) == 0.0
    if 0 in nf:
        # the dead row's dc_last reaches no gradient: the same gradients with another dc_last in that row
        b0 = nf.index(0)
        dc2 = dc.copy()
        dc2[b0] += 5.0
        ref2 = R.layer_with_grads(x, nf, P, dout, dc2, torch.float64)
        Pt2 = R.to_torch(P, torch.float64, True)
        x2 = torch.from_numpy(x).double().requires_grad_(True)
        out2, c2 = seq_ops.glu_lstm_layer(x2, *R.operands(Pt2), torch.tensor(nf))
        ((out2 * torch.from_numpy(dout).double()).sum() + (c2 * torch.from_numpy(dc2).double()).sum()).backward()
        assert torch.equal(x2.grad, xt.grad) and all(torch.equal(Pt2[n].grad, Pt[n].grad) for n in R.NAMES)
        assert R.err(x2.grad, ref2["dx"]) < 1e-12


def test_restated_c_abi_quantities_are_consistent_with_the_layer():
    """recurrence_with_grads (what the GPU tests hold the C ABI to) against layer_with_grads in fp64: the tapes are the layer's, and the
    gradients with respect to the hoisted products give back the layer's weight gradients and dx as the hoisted products over them."""
    rs = np.random.RandomState(5)
    F, B, D, H = 7, 4, 12, 16
    P = R.random_unit(rs, D, H)
    nf = np.array([7, 0, 3, 1], dtype=np.int32)
    x = rs.randn(F, B, D)
    x = (x / np.linalg.norm(x, axis=2, keepdims=True) * (np.arange(F)[:, None] < nf[None, :])[:, :, None]).astype(np.float32)
    dout, dc = rs.randn(F, B, H).astype(np.float32), rs.randn(B, H).astype(np.float32)
    lay = R.layer_with_grads(x, nf, P, dout, dc, torch.float64)
    rec = R.recurrence_with_grads(x, P, nf, dout, dc, torch.float64)
    assert R.err(rec["hs"][1:], lay["out"]) < 1e-13 and R.err(rec["c_last"], lay["c_last"]) < 1e-13
    Wv, bv, Ws, bs, Vv, Vs, Uv, Us = R.operands({n: np.asarray(a, dtype=np.float64) for n, a in P.items()})
    x2 = x.reshape(F * B, D).astype(np.float64)
    flat = lambda a: a.reshape(F * B, -1)
    dW = dict(zip(("dWv", "dbv", "dWs", "dbs", "dVv", "dVs", "dUv", "dUs"), R.operands({n: lay["d" + n] for n in R.NAMES})))
    h2 = flat(rec["hs"][:F])
    assert R.err(x2.T @ flat(rec["dzv"]), dW["dWv"]) < 1e-12 and R.err(x2.T @ flat(rec["dpv"]), dW["dVv"]) < 1e-12
    assert R.err(x2.T @ flat(rec["dzs"]), dW["dWs"]) < 1e-12 and R.err(x2.T @ flat(rec["dps"]), dW["dVs"]) < 1e-12
    assert R.err(flat(rec["dzv"]).sum(0), dW["dbv"]) < 1e-12 and R.err(flat(rec["dzs"]).sum(0), dW["dbs"]) < 1e-12
    assert R.err(h2.T @ flat(rec["dzv"]), dW["dUv"]) < 1e-12 and R.err(flat(rec["dzs"]).T @ h2, dW["dUs"]) < 1e-12
    dx = flat(rec["dzv"]) @ Wv.T + flat(rec["dpv"]) @ Vv.T + flat(rec["dzs"]) @ Ws.T + flat(rec["dps"]) @ Vs.T + flat(rec["dx_direct"])
    assert R.err(dx.reshape(F, B, D), lay["dx"]) < 1e-12
    assert R.err(rec["qv"], rec["xm"] @ Vv) < 1e-13 and R.err(rec["n2"], (rec["xm"] ** 2).sum(2)) < 1e-13


def test_lstm_glu2_model_forward_on_cpu_matches_restatement_and_moe_head(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    _stub_head(monkeypatch)
    V, M = 10, 2
    flags.lstm_cells, flags.moe_num_mixtures = str(H_), M
    g = _graph()
    rs = np.random.RandomState(12)
    x = torch.from_numpy(rs.randn(B_, F_, D_).astype(np.float32))
    nf = torch.tensor([6, 1, 3])
    p = flm.LstmGlu2Model().create_model(x, vocab_size=V, num_frames=nf)["predictions"]
    P = {n: g.vars["lstm_forward/" + n].data.double() for n in R.NAMES}
    state, _ = R.rnn_gate(x.double(), nf, P)
    want = R.moe(state, g.vars["gates/weights"].data.double(), g.vars["experts/weights"].data.double(), g.vars["experts/biases"].data.double(), M)
    assert R.err(p, want.numpy()) < 2e-6
    # and the gradient lands in every one of the 24 Variables' slots
    g.finalize()
    g.begin_step()
    p = flm.LstmGlu2Model().create_model(x, vocab_size=V, num_frames=nf)["predictions"]
    P = {n: g.vars["lstm_forward/" + n].data.double().requires_grad_(True) for n in R.NAMES}
    go = torch.from_numpy(rs.randn(B_, V).astype(np.float32))
    state, _ = R.rnn_gate(x.double(), nf, P)
    (R.moe(state, g.vars["gates/weights"].data.double(), g.vars["experts/weights"].data.double(), g.vars["experts/biases"].data.double(), M)
     * go.double()).sum().backward()
    (p * go).sum().backward()
    for n in R.NAMES:
        assert float(P[n].grad.abs().max()) > 0.0, n
        assert R.err(g.vars["lstm_forward/" + n].grad, P[n].grad.numpy()) < 5e-6, n


def test_step_kernels_use_no_scratch_and_spill_no_vgpr(tmp_path):
    """Cross-compiles csrc/glu_lstm.hip for gfx950 with the resource remarks: every glu_lstm_* kernel runs without scratch memory and
    without VGPR spills (the figures are in DESIGN_LOG.md section 32)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "youtube-8m_amd", "csrc", "glu_lstm.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "glu_lstm.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    mine = {k: v for k, v in kernels.items() if "glu_lstm_" in k}
    assert len(mine) == 8, sorted(kernels)                                 # fwd and bwd at 1, 2, 4, 8 units per thread
    for k, v in mine.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and 0 < v["VGPRs"] <= 256, (k, v)
