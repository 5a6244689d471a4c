"""The fused chain link (ops.chain_link, csrc/chain_link.hip) and the four Distillchain cascade plugins at their training scripts' shapes.
`kernels`: forward + backward of ops.chain_link through autograd, the fused kernel against the composed activation -> add_noise ->
l2_normalize (the YT8M_CHAIN_LINK_FUSED=0 form), for relu without noise and elu with noise, at [128, 128], [128, 256], [1024, 256] and
[8192, 256] (the attention plugin's B * A): hip events around back-to-back calls, the two forms alternating inside every repeat, the
spread over the repeats recorded, values and gradients compared.
Step legs (one per plugin): whole training steps (fp32, clip + Adam, learning rate 0) of the plugin with the switch on, with it off, and
of its non-distill parent, in ONE process and in turn inside every repeat, at the flags of the reference's cascade scripts
(run-cascade-76-chaining-video / -parallel-lstm / -chaining-cnn / -multiple-attention-pooling.sh) on raw uint8 frames.  The summary row
of a leg states on - off against the spread the leg saw between its own repeats.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/distillchain_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `kernels`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 4716
# leg: (module, plugin, parent, batch, frame level?, flags of the script)
LEGS = {
    "video": ("video_level_models", "DistillchainDeepCombineChainModel", "DeepCombineChainModel", 512, False,
              dict(moe_num_mixtures=4, deep_chain_layers=4, deep_chain_relu_cells=256, multitask=True, label_loss="MultiTaskCrossEntropyLoss",
                   support_type="label,label,label,label", support_loss_percent=0.05)),
    "parallel": ("frame_level_models", "DistillchainLstmParallelFinaloutputModel", "LstmParallelFinaloutputModel", 128, True,
                 dict(feature_sizes="1024,128", lstm_cells="1024,128", moe_num_mixtures=4)),
    "cnn": ("frame_level_models", "DistillchainCnnDeepCombineChainModel", "CnnDeepCombineChainModel", 128, True,
            dict(deep_chain_layers=3, deep_chain_relu_cells=256, moe_num_mixtures=4, multitask=True, label_loss="MultiTaskCrossEntropyLoss",
                 support_type="label,label,label", support_loss_percent=0.05)),
    "attention": ("frame_level_models", "DistillchainLstmAttentionMaxPoolingModel", "LstmAttentionMaxPoolingModel", 128, True,
                  dict(lstm_cells="1024", lstm_attentions=8, moe_num_mixtures=8)),
}
KERNEL_SHAPES = ((128, 128), (128, 256), (1024, 256), (8192, 256))
KERNEL_KINDS = (("relu", None), ("elu", 0.1))


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.load_package()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _events_us(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _median(v):
    return sorted(v)[len(v) // 2]


def kernels(iters, repeats):
    import torch
    dev = _setup()
    import yt8m_amd.ops as ops
    for rows, cols in KERNEL_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(rows + cols)
        z = torch.randn((rows, cols), device=dev, generator=gen)
        coef = torch.randn((rows, cols), device=dev, generator=gen)
        for kind, noise in KERNEL_KINDS:
            def run(fused):
                ops.CHAIN_LINK_FUSED = fused
                q = z.detach().requires_grad_(True)
                y = ops.chain_link(q, kind, noise, seed=7)
                y.backward(coef)
                return y.detach(), q.grad

            forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
            us = {k: [] for k in forms}
            for f in forms.values():                                         # warm-up: every form for as long as it is timed
                _events_us(f, iters)
            for _ in range(repeats):                                         # alternating: both forms see the same machine
                for k, f in forms.items():
                    us[k].append(_events_us(f, iters))
            (yf, df), (yc, dc) = forms["fused"](), forms["composed"]()
            ops.CHAIN_LINK_FUSED = True
            f_, c_ = us["fused"], us["composed"]
            print(json.dumps(dict(
                leg="kernel", rows=rows, cols=cols, kind=kind, noise_level=noise, what="forward + backward through autograd",
                launches_fused=2, launches_composed=(3 if noise else 2) + 2,
                fused_us=round(_median(f_), 2), fused_us_min=round(min(f_), 2), fused_us_max=round(max(f_), 2),
                composed_us=round(_median(c_), 2), composed_us_min=round(min(c_), 2), composed_us_max=round(max(c_), 2),
                composed_over_fused=round(_median(c_) / _median(f_), 2), fused_not_slower=bool(_median(f_) <= _median(c_)),
                y_diff_fused_composed=float((yf - yc).abs().max()), grad_diff_fused_composed_rel_to_max=float((df - dc).abs().max() / dc.abs().max()),
                repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                        % iters)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = _setup()
    import importlib
    import yt8m_amd.ops as ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    module, plugin, parent, B, frames, fl = LEGS[leg]
    mod = importlib.import_module("yt8m_amd." + module)
    FLAGS.reset()
    FLAGS.batch_size = B
    FLAGS.distillation_features = FLAGS.distillation_as_input = True
    for k, v in fl.items():
        setattr(FLAGS, k, v)
    gen = torch.Generator(device=dev).manual_seed(1)
    if frames:
        F, D = 300, 1152
        x = torch.randint(0, 256, (B, F, D), device=dev, generator=gen, dtype=torch.uint8)
        nf = torch.randint(1, F + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
        nf[0], nf[1] = F, 1
    else:
        x = torch.randn((B, 1152), device=dev, generator=gen)
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    y[:, 0] = True
    batch = (x, y, nf) if frames else (x, y)
    distill = torch.rand((B, V), device=dev, generator=gen) * 0.05
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    graphs = {}
    for name, cls in (("plugin", plugin), ("parent", parent)):
        g = reset_default_graph(device=dev, seed=0)
        graphs[name] = train.build_graph(getattr(mod, cls)(), batch_size=B, graph=g, base_learning_rate=0.0)
    forms = {"fused": ("plugin", True, dict(distill_labels_batch=distill)), "composed": ("plugin", False, dict(distill_labels_batch=distill)),
             "parent": ("parent", True, {})}

    def run(form, n):
        which, fused, kw = forms[form]
        ops.CHAIN_LINK_FUSED = fused
        for _ in range(n):
            out = graphs[which].step(*batch, **kw)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses = {k: run(k, warmup) for k in forms}
    ms = {k: [] for k in forms}
    for _ in range(repeats):                                             # in turn: every form sees the same machine
        for k in forms:
            t0 = time.perf_counter()
            run(k, steps)
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    ops.CHAIN_LINK_FUSED = True
    finite = all(np.isfinite(v) for v in losses.values())
    row = dict(leg=leg, plugin=plugin, parent=parent, B=B, V=V, input="uint8 [B,300,1152]" if frames else "float32 [B,1152]",
               flags=fl, steps=steps, warmup=warmup, repeats=repeats, losses_after_warmup=losses,
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row["%s_ms_per_step" % k] = round(_median(v), 3)
        row["%s_ms_min" % k], row["%s_ms_max" % k] = round(min(v), 3), round(max(v), 3)
    spread = max(max(ms["fused"]) - min(ms["fused"]), max(ms["composed"]) - min(ms["composed"]))
    row["fused_minus_composed_ms"] = round(_median(ms["fused"]) - _median(ms["composed"]), 3)
    row["spread_between_repeats_ms"] = round(spread, 3)
    row["fused_within_spread_of_composed"] = bool(_median(ms["fused"]) - _median(ms["composed"]) <= spread)
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--kernel_iters", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    rows = []
    for leg in a.legs or ["kernels"] + list(LEGS):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--kernel_iters", str(a.kernel_iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print("leg %s failed with exit status %d: stopping" % (leg, r.returncode), flush=True)
            return r.returncode or 1
        for ln in lines:
            rows.append(json.loads(ln))
            print(ln, flush=True)
        if a.out:                                                        # after every leg: a later leg's failure keeps the earlier rows
            with open(a.out, "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
