"""Writes tests/golden/fullsize_kat.json: checksums of predictions, loss and EVERY gradient tensor of the five BASELINE.json
configurations at their full sizes (tests/golden/fullsize_cases.py), computed by the fp64 torch restatement (oracle/torch_ref.py
autograd; SURVEY.md 8c last row).  The reference itself cannot produce them (Python 2 / TensorFlow 1.0): like models_kat.json this
pins the RESTATEMENT and gives the HIP path one whole-configuration comparison, backward pass included, at the real shapes.
Takes a few minutes and ~25 GB of host memory:   python tests/golden/make_fullsize_golden.py [config ...]

The recurrent cases (fullsize_cases.RECURRENT_CASES) go to fullsize_recurrent_kat.json instead.  A 300-step recurrence can amplify
rounding until no tolerance means anything, so for them the same restatement also runs in fp32 and the fixture records, per tensor,
the smallest `rel` of tests/test_gpu_fullsize_golden.py::_check under which that fp32 run would pass against the fp64 checksums.  A
case whose fp32 run does not pass the GPU test's own bounds with 3x headroom is ill-conditioned and is not written."""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import torch_ref  # noqa: E402
import fullsize_cases as fc  # noqa: E402

torch.set_num_threads(os.cpu_count() or 1)
DST = {"base": os.path.join(HERE, "fullsize_kat.json"), "recurrent": os.path.join(HERE, "fullsize_recurrent_kat.json")}
OUT = {k: json.load(open(v)) if os.path.exists(v) else {} for k, v in DST.items()}
# tests/test_gpu_fullsize_golden.py's fp32 bounds: loss, predictions, gradients
BOUND = {"loss": 1e-5, "predictions": 1e-4, "grads": 5e-4}
HEADROOM = 3.0


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype)


def frames(q, nf, dtype=torch.float64):
    x = torch_ref.l2_normalize(torch_ref.dequantize(torch.from_numpy(q), dtype), 2)
    mask = torch.arange(q.shape[1])[None, :] < torch.from_numpy(nf.astype(np.int64))[:, None]
    return x * mask[:, :, None].to(x.dtype)                       # zero padding AFTER dequantise (W/readers.py:178-187)


def recurrent_state(cfg, P, x, nf):
    """The head input of the recurrent plugins (W/all_frame_models/gru_pooling_model.py, gru_with_pooling_model.py,
    layernorm_lstm_memory_model.py): mean of the top layer's outputs over the live frames, [mean || h_0 || h_1], [c_0 || c_1]."""
    if cfg == "r2_lnlstm_memory":
        s = "RNN/multi_rnn_cell/cell_%d/layer_norm_basic_lstm_cell/"
        layers = [(P[s % l + "weights"], [P[s % l + n + "/gamma"] for n in fc.LN_GATES], [P[s % l + n + "/beta"] for n in fc.LN_GATES])
                  for l in range(2)]
        _, c, _ = torch_ref.lnlstm_stack(x, nf, layers)
        return torch.cat(c, 1)
    s = "RNN/multi_rnn_cell/cell_%d/gru_cell/"
    layers = [tuple(P[s % l + k] for k in ("gates/weights", "gates/biases", "candidate/weights", "candidate/biases")) for l in range(2)]
    out, h = torch_ref.gru_stack(x, nf, layers)
    mean = out.sum(1) / nf.clamp(min=1).to(out.dtype)[:, None]
    return mean if cfg == "r0_gru_pooling" else torch.cat([mean] + h, 1)


def fp32_rel(v32, ref):
    """The smallest `rel` under which _check (tests/test_gpu_fullsize_golden.py) accepts v32 against the fp64 checksum, and how many
    of v32's 20 largest-magnitude positions are the fixture's."""
    a = np.asarray(v32, dtype=np.float64).ravel()
    scale = ref["abs_sum"] + 1e-6 * ref["n"]
    r = max(abs(a.sum() - ref["sum"]), abs(np.abs(a).sum() - ref["abs_sum"])) / scale
    if ref["abs_sum"] >= 1e-9 * ref["n"]:
        top = np.asarray(ref["top_val"])
        r = max(r, np.abs(a[ref["top_idx"]] - top).max() / (10 * np.abs(top).max() + 1e-300))
    overlap = len(set(np.argsort(-np.abs(a), kind="stable")[:20].tolist()) & set(ref["top_idx"]))
    return float(r), overlap


def restate(cfg, dtype):
    P = {k: T(v, dtype).requires_grad_(True) for k, v in fc.make_params(cfg).items()}
    I = fc.make_inputs(cfg)
    y = T(I["y"], dtype)
    nf = None if I["nf"] is None else torch.from_numpy(I["nf"].astype(np.int64))
    st = recurrent_state(cfg, P, frames(I["x"], I["nf"], dtype), nf)
    p = torch_ref.moe(st, P["gates/weights"], P["experts/weights"], P["experts/biases"], fc.M)
    loss = torch_ref.cross_entropy(p, y)
    loss.backward()
    return P, p.detach(), loss.detach()


for cfg in (sys.argv[1:] or fc.CONFIGS):
    t0 = time.time()
    if cfg in fc.RECURRENT_CASES:
        P, p, loss = restate(cfg, torch.float64)
        rec = {"batch": fc.BATCH[cfg], "loss": float(loss), "predictions": fc.checksum(p.numpy()),
               "grads": {k: fc.checksum(v.grad.numpy()) for k, v in P.items()}}
        del P, p, loss
        P, p, loss = restate(cfg, torch.float32)
        cond = {"loss": abs(float(loss) - rec["loss"]) / abs(rec["loss"]), "grads": {}}
        cond["predictions"], worst_overlap = fp32_rel(p.numpy(), rec["predictions"])
        for k, v in P.items():
            cond["grads"][k], ov = fp32_rel(v.grad.numpy(), rec["grads"][k])
            worst_overlap = min(worst_overlap, ov)
        cond["min_top20_overlap"] = worst_overlap
        del P, p, loss
        rec["fp32_cpu_rel"] = cond
        rec["seconds"] = round(time.time() - t0, 1)
        worst_g = max(cond["grads"].items(), key=lambda kv: kv[1])
        print(cfg, "loss %.6f" % rec["loss"], "fp32 CPU rel: loss %.2g predictions %.2g worst grad %.2g (%s), top-20 overlap >= %d"
              % (cond["loss"], cond["predictions"], worst_g[1], worst_g[0], worst_overlap), "%.0f s" % rec["seconds"], flush=True)
        ok = (HEADROOM * cond["loss"] <= BOUND["loss"] and HEADROOM * cond["predictions"] <= BOUND["predictions"]
              and HEADROOM * worst_g[1] <= BOUND["grads"] and worst_overlap >= 16)
        if not ok:
            sys.exit("%s is ill-conditioned: its fp32 run misses the GPU test's bounds %s with %gx headroom -- not written"
                     % (cfg, BOUND, HEADROOM))
        OUT["recurrent"][cfg] = rec
        json.dump(OUT["recurrent"], open(DST["recurrent"], "w"), indent=0, sort_keys=True)
        continue
    P = {k: T(v).requires_grad_(True) for k, v in fc.make_params(cfg).items()}
    I = fc.make_inputs(cfg)
    y = T(I["y"])
    nf = None if I["nf"] is None else torch.from_numpy(I["nf"].astype(np.int64))
    sup = None
    if cfg == "c0_logistic":
        p = torch_ref.logistic(torch_ref.l2_normalize(T(I["x"]), 1), P["fully_connected/weights"], P["fully_connected/biases"])
    elif cfg == "c1_moe":
        p = torch_ref.moe(torch_ref.l2_normalize(T(I["x"]), 1), P["gates/weights"], P["experts/weights"], P["experts/biases"], fc.M)
    elif cfg == "c2_netvlad":
        h = torch_ref.netvlad_hidden(frames(I["x"], I["nf"]), nf, P["netvlad/cluster_weights"], P["netvlad/cluster_biases"],
                                     P["netvlad/centres"], P["netvlad/hidden/weights"], P["netvlad/hidden/biases"])
        p = torch_ref.moe(h, P["gates/weights"], P["experts/weights"], P["experts/biases"], fc.M)
    elif cfg == "c3_lstm":
        layers = [(P["RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % l], P["RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % l])
                  for l in range(2)]
        st = torch_ref.lstm_model_state(frames(I["x"], I["nf"]), nf, layers)
        p = torch_ref.moe(st, P["gates/weights"], P["experts/weights"], P["experts/biases"], fc.M)
    else:
        p, sup = torch_ref.gated_netvlad_attention_chain(frames(I["x"], I["nf"]), nf, P, fc.CH_L, fc.M, fc.A, bf16_heads=True)
    if sup is None:
        loss = torch_ref.cross_entropy(p, y)
    else:                                                         # MultiTaskCrossEntropyLoss, support_type "label" x L, 10 % (W/losses.py:271-279)
        loss = 0.9 * torch_ref.cross_entropy(p, y) + 0.1 * torch_ref.cross_entropy(sup, y.repeat(1, fc.CH_L))
    loss.backward()
    rec = {"batch": fc.BATCH[cfg], "loss": float(loss), "predictions": fc.checksum(p.detach().numpy()), "grads": {}}
    if sup is not None:
        rec["support_predictions"] = fc.checksum(sup.detach().numpy())
    for k, v in P.items():
        rec["grads"][k] = fc.checksum(v.grad.numpy())
    rec["seconds"] = round(time.time() - t0, 1)
    OUT["base"][cfg] = rec
    print(cfg, "loss %.6f" % rec["loss"], "%.0f s" % rec["seconds"], flush=True)
    del P, p, loss
    json.dump(OUT["base"], open(DST["base"], "w"), indent=0, sort_keys=True)
print("done")
