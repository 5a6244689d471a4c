"""-m gpu: a full-size optimiser TRAJECTORY of the headline configuration (BASELINE configs[3]: LstmModel 2 x 1024 over ragged uint8
[128, 300, 1152] frames + MoE head) against the fp64 restatement's committed fixture (tests/golden/trajectory_kat.json, written by
tests/golden/make_trajectory_golden.py): per step the label loss, every tensor's gradient norm as the per-tensor clip sees it
(W/utils.py:164-174), the learning rate of the staircase (W/train.py:301-311), and after the last step the checksums of every
parameter tensor (W/train.py:435-466: + l2 w, clip, TF-Adam).  VERDICT r5 #6 / #8: the single-pass fixtures pin one forward +
backward; clip + Adam + the LR schedule were pinned at tiny sizes only, and the f16 ("h2") recurrences / products had never been
inside a multi-step training comparison.  Here they are engaged (asserted), and the sticky clamp counter of the h2 split passes must
stay zero over the whole run (yt8m_h2_degraded)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fullsize_cases as fc  # noqa: E402

import yt8m_amd._lib as L  # noqa: E402
import yt8m_amd.frame_level_models as flm  # noqa: E402
import yt8m_amd.seq_ops as seq_ops  # noqa: E402
import yt8m_amd.train as train  # noqa: E402
from yt8m_amd.variables import reset_default_graph  # noqa: E402

pytestmark = pytest.mark.gpu
PATH = os.path.join(HERE, "golden", "trajectory_kat.json")
# h2 split elements flushed to zero over the whole replay, as this test prints it ("h2 split passes: 0 clamped, N flushed elements"),
# measured on an MI355X with the library's default partition and knobs: 6.0 % of the 3.1e9 elements the run splits
FLUSHED_MEASURED = 184520422


def _degraded(reset=False):
    c = (ctypes.c_uint64 * 2)()
    L.check(L.lib().yt8m_h2_degraded(c, int(reset), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return int(c[0]), int(c[1])


def test_full_size_training_trajectory_matches_the_fp64_restatement(dev, flags):
    if not os.path.exists(PATH):
        pytest.skip("no fixture (python tests/golden/make_trajectory_golden.py)")
    ref = json.load(open(PATH))
    cfg = ref["config"]
    assert cfg == "c3_lstm"
    lib = L.lib()
    B = fc.BATCH[cfg]
    if not lib.yt8m_lstm_persist_bwd_supported(B, fc.H):
        pytest.skip("persistent recurrence not available on this device")
    assert lib.yt8m_lstm_persist_bwd_on_f16_pipe(B, fc.H) == 1, "the replay must run the f16 recurrences (H = 1024)"
    hy = ref["hyper"]
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(flm.LstmModel(), batch_size=hy["batch_size"], base_learning_rate=hy["base_lr"], clip_gradient_norm=hy["clip"],
                          learning_rate_decay_examples=hy["decay_examples"], learning_rate_decay=hy["decay"], graph=g)
    assert len({st["learning_rate"] for st in ref["steps"]}) >= 2, "the fixture must cross a step of the LR staircase"
    I = fc.make_inputs(cfg, 0)
    x, y, nf = torch.from_numpy(I["x"]).to(dev), torch.from_numpy(I["y"]).to(dev), torch.from_numpy(I["nf"]).to(dev)
    tg.forward(x, y, nf)                                          # creates the variables
    tg.ensure_finalized()
    P = fc.make_params(cfg)
    assert {k: tuple(v.data.shape) for k, v in g.vars.items()} == {k: tuple(v.shape) for k, v in P.items()}
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev))
    del P
    names = [v.name for v in g.trainable_variables()]
    _degraded(reset=True)
    n0 = dict(seq_ops.NATIVE_CALLS)
    worst = {"loss": 0.0, "norm": 0.0}
    for s, st in enumerate(ref["steps"]):
        I = fc.make_inputs(cfg, s)
        x, y, nf = torch.from_numpy(I["x"]).to(dev), torch.from_numpy(I["y"]).to(dev), torch.from_numpy(I["nf"]).to(dev)
        out = tg.step(x, y, nf)
        loss = float(out["loss"])
        # the first step sees the injected weights exactly: fp32 rounding only.  Later steps inherit the parameters of an Adam
        # trajectory whose per-element update m / (sqrt(v) + eps) is a steep function of small gradients: 2e-4
        tol = 2e-5 if s == 0 else 2e-4
        worst["loss"] = max(worst["loss"], abs(loss - st["loss"]) / abs(st["loss"]))
        assert abs(loss - st["loss"]) <= tol * abs(st["loss"]), (s, loss, st["loss"])
        assert out["learning_rate"] == pytest.approx(st["learning_rate"], rel=1e-12)
        norms = torch.sqrt(g.norms.double()).cpu().numpy()
        for i, k in enumerate(names):
            want = st["grad_norms"][k]
            rel = abs(norms[i] - want) / max(want, 1e-30)
            worst["norm"] = max(worst["norm"], rel)
            assert rel <= (1e-4 if s == 0 else 1e-3), (s, k, norms[i], want)
    assert seq_ops.NATIVE_CALLS["bwd"] == n0["bwd"] + len(ref["steps"]), "the native recurrent stack did not run every step"
    torch.cuda.synchronize()
    for k, ck in ref["params"].items():
        w = g.vars[k].data.double().flatten()
        scale = ck["abs_sum"]
        assert abs(float(w.sum()) - ck["sum"]) <= 1e-3 * scale, (k, "sum", float(w.sum()), ck["sum"], scale)
        assert abs(float(w.abs().sum()) - ck["abs_sum"]) <= 1e-3 * scale, (k, "abs_sum", float(w.abs().sum()), ck["abs_sum"])
        idx = torch.tensor(ck["top_idx"], device=w.device)
        top = np.asarray(ck["top_val"])
        assert np.abs(w[idx].cpu().numpy() - top).max() <= 2e-3 * np.abs(top).max(), (k, "top-20 values")
    clamped, flushed = _degraded()
    total = sum(v.data.numel() for v in g.vars.values())
    print("trajectory replay: worst loss rel %.3g, worst grad-norm rel %.3g; h2 split passes: %d clamped, %d flushed elements"
          % (worst["loss"], worst["norm"], clamped, flushed))
    assert clamped == 0, "an h2 operand outgrew its scale during the run (%d clamped elements)" % clamped
    # flushed elements (more than 2^-38 below their operand's maximum: early time steps of a part whose gradients have decayed, under the
    # part's one scale word) contribute below 2^-14 ulp of the products' leading terms.  Reported; bounded by twice what this replay
    # flushes on an MI355X (FLUSHED_MEASURED) -- a run that flushes far more has lost the scale of its dz operands -- and, as before, as a
    # share of what the run split (per step and layer: dz once per orientation for dx and dW, F B 4H elements each)
    split = 2 * 2 * fc.F * B * 4 * fc.H * len(ref["steps"])
    assert flushed <= 0.2 * split, (flushed, split)
    assert flushed <= 2 * FLUSHED_MEASURED + 1000, (flushed, FLUSHED_MEASURED)


def test_h2_split_counts_what_it_clamps_and_flushes(dev):
    """The sticky counters themselves: a static scale that the operand outgrows clamps (counted), elements far below a device-measured
    maximum flush (counted), a well-scaled operand counts nothing; reset zeroes them."""
    import yt8m_amd.ops as ops
    _degraded(reset=True)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn((200, 130), device=dev, generator=g)
    ops.h2_split(x, scale=1024.0)
    assert _degraded() == (0, 0)
    xb = x.clone()
    xb[3, 7], xb[199, 129] = 1.0e3, -1.0e3                          # 1e3 * 1024 > 65504: two clamped elements
    ops.h2_split(xb, scale=1024.0)
    assert _degraded() == (2, 0)
    xs = x.clone()
    xs[0, 0] = 1.0e-30                                             # under the measured maximum (~4): 2^-100 below -> flushed
    xs[5, 5] = 0.0                                                 # an exact zero is not a flush
    ops.h2_split(xs, dynamic=True)
    assert _degraded() == (2, 1)
    assert _degraded(reset=True) == (2, 1) and _degraded() == (0, 0)
