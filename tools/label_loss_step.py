"""The batch-agreement label losses at the bench's video-level shapes (B = 1024 and B = 128 rows of V = 4716 classes).
`kernels`: forward + backward of BatchAgreementCrossEntropyLoss and TopKBatchAgreementCrossEntropyLoss through their autograd
functions (csrc/losses.hip) against the same functions composed from torch device ops -- the float32 restatement of
tests/test_losses_host.py moved to the device -- and, for scale, ops.cross_entropy: hip events around back-to-back calls, the forms
alternating inside every repeat, the spread over the repeats recorded, losses and gradients compared.  Then the fused forward and
backward calls on their own, with the bandwidth they reach on the bytes their passes imply (a pass reads p and the uint8 labels; the
backward pass also writes dL/dp).  Two kinds of predictions: `uniform` in (0.02, 0.98), where almost every element is a false
negative or a false positive and takes the whole weight formula, and `trained`, where few are.  The shader clock is read before and
after the timed section (read only; null where the tool is missing).
Step legs: a MoeModel training step (fp32, clip + Adam, learning rate 0) at B = 1024 under either loss and under CrossEntropyLoss
with the fused head + loss off (--nofused_head_loss: the step the two losses add their cost to).  Every leg runs in a child process
of its own under its own time limit, the step legs `--repeats` times in turn; the driver stops at the first leg that fails.
usage: python tools/label_loss_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `kernels`"""
import json
import os
import subprocess
import sys

import steplib

LEGS = ("moe_batch_agreement", "moe_topk_batch_agreement", "moe_cross_entropy_unfused")
LOSS_OF_LEG = {"moe_batch_agreement": "BatchAgreementCrossEntropyLoss", "moe_topk_batch_agreement": "TopKBatchAgreementCrossEntropyLoss",
               "moe_cross_entropy_unfused": "CrossEntropyLoss"}
D, V = 1152, steplib.V
AGREEMENT = 0.1


def _shader_clock():
    """What rocm-smi shows for the shader clock right now (a read); None without the tool."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        card = next(iter(json.loads(r.stdout).values()))
        return next((v for k, v in card.items() if "sclk" in k.lower()), None)
    except Exception:
        return None


def _inputs(kind, B, dev):
    import torch
    gen = torch.Generator(device=dev).manual_seed(B)
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    u = torch.rand((B, V), device=dev, generator=gen)
    if kind == "uniform":
        p = 0.02 + 0.96 * u
    else:                      # positives mostly high, negatives mostly near 0, one in a thousand of either on the wrong side
        wrong = torch.rand((B, V), device=dev, generator=gen) < 1e-3
        high = y ^ wrong
        p = torch.where(high, 0.5 + 0.48 * u, 0.001 + 0.05 * u)
    return p.contiguous(), y


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    sys.path.insert(0, os.path.join(steplib.ROOT, "tests"))
    import yt8m_amd.ops as ops
    import test_losses_host as H
    clock_before = _shader_clock()
    for B in (1024, 128):
        for kind in ("uniform", "trained"):
            p, y = _inputs(kind, B, dev)
            yf = y.to(torch.float32)
            N = float(B)

            def fwd_bwd(fn, *args):
                q = p.detach().requires_grad_(True)
                loss = fn(q, *args)
                loss.backward()
                return loss.detach(), q.grad

            forms = {
                ("batch_agreement", "fused"): lambda: fwd_bwd(ops.batch_agreement_cross_entropy, y, AGREEMENT, N),
                ("batch_agreement", "composed"): lambda: fwd_bwd(H.batch_agreement_ref, yf, AGREEMENT, N),
                ("topk_batch_agreement", "fused"): lambda: fwd_bwd(ops.topk_batch_agreement_cross_entropy, y, AGREEMENT),
                ("topk_batch_agreement", "composed"): lambda: fwd_bwd(H.topk_batch_agreement_ref, yf, AGREEMENT),
                ("cross_entropy", "fused"): lambda: fwd_bwd(ops.cross_entropy, y),
            }
            us = steplib.alternate(forms, iters, repeats)
            for loss_name in ("batch_agreement", "topk_batch_agreement", "cross_entropy"):
                lf, df = forms[(loss_name, "fused")]()
                row = dict(leg="kernel", loss=loss_name, predictions=kind, B=B, V=V, what="forward + backward through autograd",
                           **steplib.spread_fields("fused", us[(loss_name, "fused")], "us"), repeats=repeats, loss_value=float(lf),
                           timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                  % iters)
                if (loss_name, "composed") in forms:
                    lc, dc = forms[(loss_name, "composed")]()
                    c = us[(loss_name, "composed")]
                    row.update(**steplib.spread_fields("composed", c, "us"),
                               composed_over_fused=round(steplib.median(c) / steplib.median(us[(loss_name, "fused")]), 2),
                               loss_rel_diff_fused_composed=abs(float(lf) - float(lc)) / abs(float(lc)),
                               grad_diff_fused_composed_rel_to_max=float((df - dc).abs().max() / dc.abs().max()))
                print(json.dumps(row), flush=True)
            # the fused calls on their own, against the bytes of their passes
            up = torch.ones(1, device=dev)
            _, st_ba = ops.batch_agreement_fwd(p, y, AGREEMENT, N)
            _, st_tk = ops.topk_batch_agreement_fwd(p, y, AGREEMENT)
            read = 5 * B * V                                                 # float32 p + uint8 labels
            calls = {
                "batch_agreement_fwd": (lambda: ops.batch_agreement_fwd(p, y, AGREEMENT, N), 3 * read, "extrema, moments, loss: 3 reads of (p, y)"),
                "batch_agreement_bwd": (lambda: ops.batch_agreement_bwd(p, y, st_ba, up), read + 4 * B * V, "1 read of (p, y), 1 write of dL/dp"),
                "topk_batch_agreement_fwd": (lambda: ops.topk_batch_agreement_fwd(p, y, AGREEMENT), 2 * read + 4 * B * V,
                                             "threshold selection (1 read of p), min_pp, loss: 2 reads of (p, y)"),
                "topk_batch_agreement_bwd": (lambda: ops.topk_batch_agreement_bwd(p, y, st_tk, up, AGREEMENT), read + 4 * B * V,
                                             "1 read of (p, y), 1 write of dL/dp"),
                "topk_rows_k20": (lambda: ops.topk_rows(p, 20), 4 * B * V, "for comparison, the eval path's top-k (values and indices): 1 read of p"),
                "xent_bwd": (lambda: ops.xent_bwd(p, y, None, up), read + 4 * B * V, "1 read of (p, y), 1 write of dL/dp"),
            }
            cus = steplib.alternate({k: c[0] for k, c in calls.items()}, iters, repeats)
            for k, (_, nbytes, what) in calls.items():
                med = steplib.median(cus[k])
                print(json.dumps(dict(leg="call", call=k, predictions=kind, B=B, V=V, us_per_call=round(med, 2), us_min=round(min(cus[k]), 2),
                                      us_max=round(max(cus[k]), 2), algorithmic_bytes=nbytes, passes=what,
                                      tb_per_s_on_algorithmic_bytes=round(nbytes / (med * 1e-6) / 1e12, 3))), flush=True)
    print(json.dumps(dict(leg="clock", shader_clock_before=clock_before, shader_clock_after=_shader_clock(),
                          device=torch.cuda.get_device_name(0))), flush=True)
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
    FLAGS.label_loss, FLAGS.batch_size, FLAGS.batch_agreement = LOSS_OF_LEG[leg], B, AGREEMENT
    if leg == "moe_cross_entropy_unfused":
        FLAGS.fused_head_loss = False
    g = reset_default_graph(device=dev, seed=0)
    # learning rate 0 (the step does the same work): the steps repeat one random batch, which the model would otherwise learn by
    # heart within some tens of steps -- a perfectly separated batch, where BatchAgreementCrossEntropyLoss is NaN by definition
    tg = train.build_graph(vlm.MoeModel(), batch_size=B, graph=g, base_learning_rate=0.0)
    assert type(tg.label_loss_fn) is getattr(losses, LOSS_OF_LEG[leg])
    x, y, _, _ = steplib.random_batch(dev, B, D=D)
    loss_first = steplib.warm_up(lambda: tg.step(x, y), warmup)
    out, elapsed, _ = steplib.timed_steps(lambda: tg.step(x, y), steps)
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model="MoeModel", label_loss=LOSS_OF_LEG[leg], fused_head_loss=bool(FLAGS.fused_head_loss), B=B, D=D,
                          V=V, ms_per_step=round(elapsed / steps * 1e3, 3), steps=steps, warmup=warmup, loss_first=loss_first,
                          loss=float(out["loss"]), params_finite=finite,
                          timing="host clock around the steps, ending in a device synchronise")), flush=True)
    return 0 if finite and np.isfinite(loss_first) else 1


def parser():
    ap = steplib.arg_parser(steps=50, warmup=5, timeout=300)
    ap.add_argument("--repeats", type=int, default=5, help="times every step leg runs (in turn), and timing repeats of the kernel leg")
    ap.add_argument("--kernel_iters", type=int, default=100)
    return ap


def main():
    a = steplib.parse_args(parser(), ("kernels",) + LEGS)
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup)
    return steplib.drive(__file__, steplib.repeated_plan(a.legs or ["kernels"] + list(LEGS), "kernels", a.repeats),
                         steplib.child_args(a, "repeats", "kernel_iters"), a.timeout, a.out, summarise=steplib.per_leg_medians)


if __name__ == "__main__":
    sys.exit(main())
