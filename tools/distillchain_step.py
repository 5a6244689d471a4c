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
import json
import sys

import steplib

V = steplib.V
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


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
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
            us = steplib.alternate(forms, iters, repeats)
            (yf, df), (yc, dc) = forms["fused"](), forms["composed"]()
            ops.CHAIN_LINK_FUSED = True
            f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
            print(json.dumps(dict(
                leg="kernel", rows=rows, cols=cols, kind=kind, noise_level=noise, what="forward + backward through autograd",
                launches_fused=2, launches_composed=(3 if noise else 2) + 2,
                **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
                composed_over_fused=round(c_ / f_, 2), fused_not_slower=bool(f_ <= c_),
                y_diff_fused_composed=float((yf - yc).abs().max()), grad_diff_fused_composed_rel_to_max=float((df - dc).abs().max() / dc.abs().max()),
                repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                        % iters)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
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
    x, y, nf, gen = steplib.random_batch(dev, B, 300 if frames else None, "ends", first_label=True)
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
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    ops.CHAIN_LINK_FUSED = True
    finite = all(np.isfinite(v) for v in losses.values())
    row = dict(leg=leg, plugin=plugin, parent=parent, B=B, V=V, input="uint8 [B,300,1152]" if frames else "float32 [B,1152]",
               flags=fl, steps=steps, warmup=warmup, repeats=repeats, losses_after_warmup=losses,
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row.update(steplib.fused_against_composed(ms))
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def parser():
    ap = steplib.arg_parser(steps=20, warmup=3, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--kernel_iters", type=int, default=200)
    return ap


def main():
    a = steplib.parse_args(parser(), ["kernels"] + list(LEGS))
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    return steplib.drive(__file__, a.legs or ["kernels"] + list(LEGS), steplib.child_args(a, "repeats", "kernel_iters"), a.timeout, a.out)


if __name__ == "__main__":
    sys.exit(main())
