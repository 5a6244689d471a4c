"""-m gpu: the recurrent plugins outside BASELINE.json -- GruPoolingModel, GruWithPoolingModel, LayerNormLstmMemoryModel -- at their
default sizes (B = 128, F = 300, D = 1152, H = 1024, 2 layers, MoE head over V = 4716, raw uint8 frames with ragged num_frames)
through the HIP path, forward AND backward, against the checksums of the fp64 restatement (tests/golden/fullsize_recurrent_kat.json,
written by tests/golden/make_fullsize_golden.py).  This runs the persistent GRU forward, the per-step GRU backward, the LN-LSTM cells,
the byte-path layer 0 and the large-row h2 forms of the hoisted products at the shapes that are trained.

The fixture also records, per tensor, how far an fp32 CPU run of the same restatement lands from fp64 (`fp32_cpu_rel`, in _check's
units): a bound is only meaningful if it leaves that difference 3x headroom, which is asserted before the device is compared."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import fullsize_cases as fc  # noqa: E402
from test_gpu_fullsize_golden import _check  # noqa: E402

import yt8m_amd.frame_level_models as flm  # noqa: E402
import yt8m_amd.train as train  # noqa: E402
from yt8m_amd.variables import reset_default_graph  # noqa: E402

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(HERE, "golden", "fullsize_recurrent_kat.json")))
MODELS = {"r0_gru_pooling": flm.GruPoolingModel, "r1_gru_with_pooling": flm.GruWithPoolingModel,
          "r2_lnlstm_memory": flm.LayerNormLstmMemoryModel}
# the fp32 bounds of tests/test_gpu_fullsize_golden.py: loss, predictions, every gradient (relative to the tensor's mean magnitude)
REL = {"loss": 1e-5, "predictions": 1e-4, "grads": 5e-4}
HEADROOM = 3.0


def _rel(got, ref):
    """The smallest `rel` under which _check accepts `got` (the device's difference, in the units of the fixture's fp32_cpu_rel)."""
    g = got.detach().double().flatten()
    scale = ref["abs_sum"] + 1e-6 * ref["n"]
    r = max(abs(float(g.sum()) - ref["sum"]), abs(float(g.abs().sum()) - ref["abs_sum"])) / scale
    if ref["abs_sum"] >= 1e-9 * ref["n"]:
        top = torch.tensor(ref["top_val"], dtype=torch.float64)
        r = max(r, float((g[torch.tensor(ref["top_idx"], device=g.device)].cpu() - top).abs().max()) / (10 * float(top.abs().max())))
    return r


def test_every_recurrent_case_has_a_fixture():
    assert sorted(KAT) == sorted(fc.RECURRENT_CASES)


@pytest.mark.parametrize("cfg", fc.RECURRENT_CASES)
def test_recurrent_plugin_at_full_size_matches_the_fp64_checksums(dev, flags, cfg):
    ref = KAT[cfg]
    cond = ref["fp32_cpu_rel"]
    # the case is well-conditioned: fp32 rounding alone stays 3x inside every bound used below
    assert HEADROOM * cond["loss"] <= REL["loss"], cond["loss"]
    assert HEADROOM * cond["predictions"] <= REL["predictions"], cond["predictions"]
    for k, r in cond["grads"].items():
        assert HEADROOM * r <= REL["grads"], (k, r)
    I = fc.make_inputs(cfg)
    B = fc.BATCH[cfg]
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(MODELS[cfg](), batch_size=B, graph=g)
    x, y = torch.from_numpy(I["x"]).to(dev), torch.from_numpy(I["y"]).to(dev)
    nf = torch.from_numpy(I["nf"]).to(dev)
    tg.forward(x, y, nf)
    g.finalize()
    P = fc.make_params(cfg)
    assert {k: tuple(v.data.shape) for k, v in g.vars.items()} == {k: tuple(v.shape) for k, v in P.items()}
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev))
    del P
    res = tg.forward(x, y, nf)
    loss = tg.loss(res, y)
    loss.backward()
    torch.cuda.synchronize()
    got = {"loss": abs(float(loss) - ref["loss"]) / abs(ref["loss"])}
    print("%s: loss rel %.3g (fp32 CPU %.3g)" % (cfg, got["loss"], cond["loss"]))
    assert got["loss"] <= REL["loss"], (float(loss), ref["loss"])
    rp = _rel(res["predictions"], ref["predictions"])
    rg = max((_rel(g.vars[k].grad, c), k) for k, c in ref["grads"].items())
    print("%s: predictions rel %.3g (fp32 CPU %.3g), worst gradient rel %.3g (%s; fp32 CPU %.3g)"
          % (cfg, rp, cond["predictions"], rg[0], rg[1], cond["grads"][rg[1]]))
    _check("predictions", res["predictions"], ref["predictions"], REL["predictions"])
    for k, c in ref["grads"].items():
        _check("grad " + k, g.vars[k].grad, c, REL["grads"])
