"""Z's --loss_function kinds (csrc/xent_variants.hip) at the video-level shapes: [1024, 4716], [128, 4716] and [1024, 3 * 4716], the
predictions_class of the final submission's entry 1 (float labels tiled along the columns, as TrainGraph._mix_loss tiles them).
`kernels`: forward + backward of each of the seven kinds through ops.xent_variant against the same function composed from torch
device ops -- the float32 restatement of tests/loss_function_restatement.py moved to the device -- and, for scale, ops.cross_entropy:
hip events around every single call, the forms in turn, 20 calls each, their median and [min, max] recorded, losses and gradients
compared; a call timed on its own includes the host's share of it (allocations, autograd, the launches), which the device cannot
hide behind earlier work, so every form is also timed over windows of 100 back-to-back calls, five windows with the forms in turn
(`*_us_queued`, with their min and max).  Two kinds of predictions: `uniform` in (0.02, 0.98), where loss_relabel takes the relabelled
branch, and `trained`, where it keeps the labels.  The leg runs twice (`run`).
Step legs: a MoeMix4Model training step (fp32, clip + Adam, learning rate 0) at entry 1's script shape -- B = 1024, 1152 inputs, 4
mixtures, --moe_layers=3, --class_size=100 -- under loss_relabel, under loss_weight and with the flag unset.  Every leg runs in a child
process of its own under its own time limit, the step legs `--repeats` times in turn; the driver stops at the first leg that fails.
usage: python tools/loss_function_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `kernels`"""
import json
import os
import sys

import steplib

LEGS = ("mix4_loss_relabel", "mix4_loss_weight", "mix4_flag_unset")
FLAG_OF_LEG = {"mix4_loss_relabel": "loss_relabel", "mix4_loss_weight": "loss_weight", "mix4_flag_unset": None}
D, V = 1152, steplib.V
SHAPES = ((1024, V, 1), (128, V, 1), (1024, V, 3))              # (rows, labels, pieces along the columns)
CALLS = 20
QUEUED = 100
WINDOWS = 5


def _inputs(kind, B, L, dev):
    import torch
    gen = torch.Generator(device=dev).manual_seed(B + L)
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    u = torch.rand((B, L * V), device=dev, generator=gen)
    labels = y if L == 1 else y.to(torch.float32).repeat(1, L)
    if kind == "uniform":
        p = 0.02 + 0.96 * u
    else:                      # positives mostly high, negatives mostly near 0, one in a thousand of either on the wrong side
        wrong = torch.rand((B, L * V), device=dev, generator=gen) < 1e-3
        high = (labels > 0) ^ wrong
        p = torch.where(high, 0.5 + 0.48 * u, 0.001 + 0.05 * u)
    return p.contiguous(), labels.contiguous()


def _queued_fields(prefix, windows):
    return {prefix + "_us_queued": round(steplib.median(windows), 2), prefix + "_us_queued_min": round(min(windows), 2),
            prefix + "_us_queued_max": round(max(windows), 2)}


def kernels(calls):
    import torch
    dev = steplib.setup()
    sys.path.insert(0, os.path.join(steplib.ROOT, "tests"))
    import yt8m_amd.ops as ops
    import loss_function_restatement as R
    for B, _, L in SHAPES:
        for kind in ("uniform", "trained"):
            p, y = _inputs(kind, B, L, dev)
            yf = y.to(torch.float32)

            def fwd_bwd(fn, *args):
                q = p.detach().requires_grad_(True)
                loss = fn(q, *args)
                loss.backward()
                return loss.detach(), q.grad

            forms = {("cross_entropy", "fused"): lambda: fwd_bwd(ops.cross_entropy, y)}
            for name in R.NAMES:
                forms[(name, "fused")] = lambda name=name: fwd_bwd(ops.xent_variant, y, name)
                forms[(name, "composed")] = lambda name=name: fwd_bwd(lambda q: R.restatement(name, q, yf))
            for fn in forms.values():                                      # allocator, autograd and code objects warm
                for _ in range(10):
                    fn()
            us = steplib.alternate(forms, 1, calls)
            queued = steplib.alternate(forms, QUEUED, WINDOWS)
            for name in ("cross_entropy",) + R.NAMES:
                lf, df = forms[(name, "fused")]()
                row = dict(leg="kernel", loss_function=name, predictions=kind, B=B, V=L * V, labels=str(y.dtype).replace("torch.", ""),
                           what="forward + backward through autograd", **steplib.spread_fields("fused", us[(name, "fused")], "us"),
                           calls=calls, **_queued_fields("fused", queued[(name, "fused")]), queued_calls=QUEUED, queued_windows=WINDOWS,
                           loss_value=float(lf),
                           timing="hip events around every single call (torch allocations and autograd included), the forms in turn; "
                                  "median, min and max of the calls.  *_us_queued: hip events around %d back-to-back calls, the forms in turn, median, "
                                  "min and max of %d such windows" % (QUEUED, WINDOWS))
                if (name, "composed") in forms:
                    lc, dc = forms[(name, "composed")]()
                    c = us[(name, "composed")]
                    row.update(**steplib.spread_fields("composed", c, "us"), **_queued_fields("composed", queued[(name, "composed")]),
                               composed_over_fused=round(steplib.median(c) / steplib.median(us[(name, "fused")]), 2),
                               fused_below_composed=bool(steplib.median(us[(name, "fused")]) < steplib.median(c)),
                               loss_rel_diff_fused_composed=abs(float(lf) - float(lc)) / abs(float(lc)),
                               grad_diff_fused_composed_rel_to_max=float((df - dc).abs().max() / dc.abs().max()))
                print(json.dumps(row), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup):
    import numpy as np
    dev = steplib.setup()
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    B = 1024
    FLAGS.reset()
    FLAGS.batch_size, FLAGS.moe_num_mixtures, FLAGS.moe_layers, FLAGS.class_size = B, 4, 3, 100
    FLAGS.loss_function = FLAG_OF_LEG[leg]
    g = reset_default_graph(device=dev, seed=0)
    # learning rate 0 (the step does the same work): the steps repeat one random batch, and the branch of loss_relabel stays the first step's
    tg = train.build_graph(vlm.MoeMix4Model(), batch_size=B, graph=g, base_learning_rate=0.0)
    assert type(tg.label_loss_fn) is losses.CrossEntropyLoss
    x, y, _, _ = steplib.random_batch(dev, B, D=D)
    loss_first = steplib.warm_up(lambda: tg.step(x, y), warmup)
    out, elapsed, _ = steplib.timed_steps(lambda: tg.step(x, y), steps)
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model="MoeMix4Model", loss_function=FLAG_OF_LEG[leg], B=B, D=D, V=V, moe_num_mixtures=4, moe_layers=3,
                          class_size=100, ms_per_step=round(elapsed / steps * 1e3, 3), steps=steps, warmup=warmup, loss_first=loss_first,
                          loss=float(out["loss"]), params_finite=finite,
                          timing="host clock around the steps, ending in a device synchronise")), flush=True)
    return 0 if finite and np.isfinite(loss_first) else 1


def parser():
    ap = steplib.arg_parser(steps=50, warmup=5, timeout=300)
    ap.add_argument("--repeats", type=int, default=2, help="times every leg runs (the step legs in turn)")
    ap.add_argument("--calls", type=int, default=CALLS, help="timed calls of every form of the kernel leg")
    return ap


def main():
    a = steplib.parse_args(parser(), ("kernels",) + LEGS)
    if a.child == "kernels":
        return kernels(a.calls)
    if a.child:
        return child(a.child, a.steps, a.warmup)
    legs = a.legs or ["kernels"] + list(LEGS)
    plan = [("kernels", {"run": run}) for run in range(a.repeats) if "kernels" in legs]
    plan += [(leg, {"rep": rep}) for rep in range(a.repeats) for leg in legs if leg != "kernels"]
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "calls"), a.timeout, a.out, summarise=steplib.per_leg_medians)


if __name__ == "__main__":
    sys.exit(main())
