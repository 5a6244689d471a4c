"""The fused memory link (ops.memory_link, csrc/memory_link.hip) and the three multi-LSTM plugins at their training scripts' shapes.
`link` (timed first, and run twice by the driver: two repeats of the leg): forward + backward of ops.memory_link through autograd, the
fused kernel against the composed torch.cat -> l2_normalize (the YT8M_MEMORY_LINK_FUSED=0 form), with and without normalize, at
[128; 1024], [128; 1024, 1024] and [384; 1024, 1024]: hip events around back-to-back calls, the two forms alternating inside every
repeat, the spread over the repeats recorded, values and gradients compared.  The driver adds a `link_summary` row: whether the fused
median was below the composed one at every shape in both repeats of the leg -- what decides the default of the switch.
Step legs (one per plugin): whole training steps (fp32, clip + Adam, learning rate 0) of the plugin with the switch on, with it off, and
of the single-stack model it is measured against, in ONE process and in turn inside every repeat, on raw uint8 frames [128, 300, 1152].
The row states the plugin's step over N x the baseline's (N = the number of stacks of the plugin per stack of the baseline).
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/multilstm_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `link`"""
import json
import sys

import steplib

V, B, F = steplib.V, 128, 300
CHAIN = dict(multitask=True, label_loss="MultiTaskCrossEntropyLoss", support_loss_percent=0.05)
# leg: (plugin, baseline, stacks of the plugin per stack of the baseline, distillation input?, flags)
LEGS = {
    "chain": ("LstmMemoryDeepChainModel", "LstmMemoryModel", 2, False,
              dict(lstm_cells="1024", lstm_layers=2, deep_chain_layers=1, deep_chain_relu_cells=200, moe_num_mixtures=4, support_type="label",
                   **CHAIN)),
    "distill": ("DistillchainLstmMemoryDeepCombineChainModel", "LstmMemoryModel", 3, True,
                dict(lstm_cells="1024", lstm_layers=1, deep_chain_layers=2, deep_chain_relu_cells=256, distillchain_relu_cells=256,
                     moe_num_mixtures=4, support_type="label,label", **CHAIN)),
    "parallel": ("LstmParallelMemoryModel", "LstmParallelFinaloutputModel", 1, False,
                 dict(lstm_cells="1024,128", feature_sizes="1024,128", lstm_layers=2, moe_num_mixtures=4)),
}
LINK_SHAPES = ((128, (1024,)), (128, (1024, 1024)), (384, (1024, 1024)))


def link(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    for rows, widths in LINK_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(rows + sum(widths))
        parts = [torch.randn((rows, w), device=dev, generator=gen) for w in widths]
        coef = torch.randn((rows, sum(widths)), device=dev, generator=gen)
        for normalize in (True, False):
            def run(fused):
                ops.MEMORY_LINK_FUSED = fused
                leaves = [t.detach().requires_grad_(True) for t in parts]
                y = ops.memory_link(leaves, normalize)
                y.backward(coef)
                return y.detach(), torch.cat([t.grad for t in leaves], 1)

            forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
            us = steplib.alternate(forms, iters, repeats)
            (yf, df), (yc, dc) = forms["fused"](), forms["composed"]()
            ops.MEMORY_LINK_FUSED = True
            f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
            n = len(widths)
            print(json.dumps(dict(
                leg="link", rows=rows, widths=list(widths), normalize=normalize, what="forward + backward through autograd",
                launches_fused=2, launches_composed=(1 if n > 1 else 0) + n + (2 if normalize else 0),
                **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
                composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
                y_diff_fused_composed=float((yf - yc).abs().max()), grad_diff_fused_composed_rel_to_max=float((df - dc).abs().max() / dc.abs().max()),
                repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                        % iters)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    import yt8m_amd.ops as ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    plugin, baseline, n_stacks, distill_in, fl = LEGS[leg]
    FLAGS.reset()
    FLAGS.batch_size = B
    if distill_in:
        FLAGS.distillation_features = FLAGS.distillation_as_input = True
    for k, v in fl.items():
        setattr(FLAGS, k, v)
    x, y, nf, gen = steplib.random_batch(dev, B, F, "ends", first_label=True)
    batch = (x, y, nf)
    distill = torch.rand((B, V), device=dev, generator=gen) * 0.05
    # learning rate 0 (the step does the same work): the steps repeat one random batch.  The baseline has no support predictions: it
    # takes the plain loss, whatever the leg's flags say
    graphs = {"plugin": train.build_graph(getattr(flm, plugin)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                          base_learning_rate=0.0),
              "baseline": train.build_graph(getattr(flm, baseline)(), label_loss_fn=losses.CrossEntropyLoss(), multitask=False, batch_size=B,
                                            graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)}
    kw = dict(distill_labels_batch=distill) if distill_in else {}
    forms = {"fused": ("plugin", True, kw), "composed": ("plugin", False, kw), "baseline": ("baseline", True, {})}

    def run(form, n):
        which, fused, kw_ = forms[form]
        ops.MEMORY_LINK_FUSED = fused
        for _ in range(n):
            out = graphs[which].step(*batch, **kw_)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    ops.MEMORY_LINK_FUSED = True
    finite = all(np.isfinite(v) for v in losses_.values())
    row = dict(leg=leg, plugin=plugin, baseline=baseline, B=B, V=V, input="uint8 [B,300,1152]", flags=fl, steps=steps, warmup=warmup,
               repeats=repeats, losses_after_warmup=losses_, stacks_per_baseline_stack=n_stacks,
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row.update(steplib.fused_against_composed(ms))
    row["plugin_over_n_baselines"] = round(steplib.median(ms["fused"]) / (n_stacks * steplib.median(ms["baseline"])), 3)
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def summarise(rows):
    return steplib.verdict_after(rows, "link", "leg_repeat", "fused is the default only if this holds over two repeats of the leg")


def parser():
    ap = steplib.arg_parser(steps=10, warmup=3, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--link_iters", type=int, default=200)
    return ap


def main():
    a = steplib.parse_args(parser(), ["link"] + list(LEGS))
    if a.child == "link":
        return link(a.link_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["link", "link"] + list(LEGS)                       # the link leg twice: its verdict wants two repeats of the leg
    return steplib.drive(__file__, steplib.numbered(legs, "link", "leg_repeat"), steplib.child_args(a, "repeats", "link_iters"),
                         a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
