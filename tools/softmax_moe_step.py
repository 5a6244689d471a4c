"""The label-softmax mixture block and the split softmax loss (ops.softmax_moe, ops.split_softmax_loss, csrc/softmax_moe.hip) and
MoeSoftmaxModel on them at its training script's shape (--moe_num_mixtures=4 --moe_layers=3 --class_size=100 --softmax_bound=3000).
`kernels`: forward + backward through autograd, the kernels (YT8M_SOFTMAX_MOE_FUSED=1 / YT8M_SPLIT_SOFTMAX_LOSS_FUSED=1) against the
composed torch form, alternating inside every repeat: the block from its two logit matrices to the whole prediction row at
[B; S; M] = [128; 1717; 4], [1024; 1717; 4], [1024; 3717; 4] and [128; 1717; 8] with a 3000-wide sigmoid part in front, and the loss at
[128, 4716] and [1024, 4716], bound 3000.  Hip events around back-to-back calls, values and gradients compared.  The driver adds one
`kernels_summary` row per switch: whether the kernels' median was below the composed form's at every shape in every run of the leg --
what decides each default on its own.
`launches`: the entry points alone through the C ABI at the same shapes, with the bytes each has to move and the rate in TB/s.
`steps`: whole training steps of MoeSoftmaxModel at B = 1024 on float features (fp32, clip + Adam, learning rate 0) under
--label_loss=CrossEntropyLoss (the mix rule) and SplitSoftmaxLoss, each with both switches on and off, and of MoeMix4Model under the
script's flags as the same-run yardstick, in ONE process and in turn inside every repeat.
Every leg runs in a child process of its own under its own time limit, and every leg runs twice (rows numbered by `run`); the driver
stops at the first leg that fails.
usage: python tools/softmax_moe_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: kernels launches steps"""
import ctypes
import json
import sys

import steplib

V = steplib.V
BOUND = 3000
# (rows, S, M): the workload's S = 4716 - 3000 + 1 at both batch sizes, a softmax part of 3716 labels (bound 1000: not register-resident),
# and 8 mixtures
CASES = [(128, 1717, 4), (1024, 1717, 4), (1024, 3717, 4), (128, 1717, 8)]
LOSS_CASES = [(128, V, BOUND), (1024, V, BOUND)]
SCRIPT = dict(moe_num_mixtures=4, moe_layers=3, class_size=100, softmax_bound=BOUND)
SWITCHES = {"softmax_moe": "YT8M_SOFTMAX_MOE_FUSED", "split_softmax_loss": "YT8M_SPLIT_SOFTMAX_LOSS_FUSED"}


def _operands(dev, rows, S, M, V1):
    import torch
    gen = torch.Generator(device=dev).manual_seed(rows + S + M)
    Zg = torch.randn((rows, S * (M + 1)), device=dev, generator=gen)
    Ze = torch.randn((rows, S * M), device=dev, generator=gen)
    head = torch.rand((rows, V1), device=dev, generator=gen)
    dout = torch.randn((rows, V1 + S - 1), device=dev, generator=gen)
    return Zg, Ze, head, dout


def _loss_operands(dev, rows, Vv, bound):
    import torch
    gen = torch.Generator(device=dev).manual_seed(rows)
    p = torch.rand((rows, Vv), device=dev, generator=gen)
    p[:, bound:] *= 0.9 / p[:, bound:].sum(dim=1, keepdim=True)
    y = torch.rand((rows, Vv), device=dev, generator=gen) < 3.4 / Vv
    return p, y


def _row(op, us, rf, rc, repeats, timing, **fields):
    f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
    return dict(leg="kernels", op=op, switch=SWITCHES[op], **fields, **steplib.spread_fields("fused", us["fused"], "us"),
                **steplib.spread_fields("composed", us["composed"], "us"), composed_over_fused=round(c_ / f_, 2),
                fused_below_composed=bool(f_ < c_),
                max_rel_diff_fused_composed=max(float((a - b).abs().max() / b.abs().max().clamp(min=1.0)) for a, b in zip(rf, rc)),
                repeats=repeats, timing=timing)


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    timing = "hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats" % iters
    for rows, S, M in CASES:
        Zg, Ze, head, dout = _operands(dev, rows, S, M, BOUND)

        def run(fused):
            ops.SOFTMAX_MOE_FUSED = fused
            zg, ze, h = Zg.detach().requires_grad_(True), Ze.detach().requires_grad_(True), head.detach().requires_grad_(True)
            out = ops.softmax_moe(zg, ze, S, M, head=h)
            out.backward(dout)
            return [out.detach(), zg.grad, ze.grad, h.grad]

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        print(json.dumps(_row("softmax_moe", us, rf, rc, repeats, timing, rows=rows, S=S, M=M, V1=BOUND,
                              what="forward + backward through autograd from the two logit matrices and the sigmoid part to the whole "
                                   "prediction row",
                              launches_fused="1 kernel forward, 1 kernel backward (fresh gradient tensors)")), flush=True)
    for rows, Vv, bound in LOSS_CASES:
        p, y = _loss_operands(dev, rows, Vv, bound)

        def run_loss(fused):
            ops.SPLIT_SOFTMAX_LOSS_FUSED = fused
            pt = p.detach().requires_grad_(True)
            loss = ops.split_softmax_loss(pt, y, bound)
            loss.backward()
            return [loss.detach().reshape(1), pt.grad]

        forms = {"fused": lambda: run_loss(True), "composed": lambda: run_loss(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        print(json.dumps(_row("split_softmax_loss", us, rf, rc, repeats, timing, rows=rows, V=Vv, bound=bound,
                              what="the loss and its gradient through autograd on bool labels",
                              launches_fused="2 kernels forward (rows, then the fp64 finish), 1 kernel backward")), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def launches(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    lib = L.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    timing = "hip events over %d back-to-back calls through the C ABI" % iters

    def rows_of(kernel, us, nbytes, **fields):
        med = steplib.median(us)
        print(json.dumps(dict(leg="launches", kernel=kernel, **fields, bytes=nbytes, **steplib.spread_fields("call", us, "us"),
                              TB_per_s=round(nbytes / med / 1e6, 3), streaming_read_TB_per_s="6.0-6.3", timing=timing)), flush=True)

    for rows, S, M in CASES:
        Zg, Ze, head, dout = _operands(dev, rows, S, M, BOUND)
        W = BOUND + S - 1
        out, stats = torch.empty((rows, W), device=dev), torch.empty((rows, 2 * M + 1), device=dev)
        dZg, dZe = torch.empty_like(Zg), torch.empty_like(Ze)
        fwd = lambda: L.check(lib.yt8m_softmax_moe_fwd(p(Zg), p(Ze), p(head), p(out), p(stats), rows, S, M, BOUND, st()))
        bwd = lambda: L.check(lib.yt8m_softmax_moe_bwd(p(Zg), p(Ze), p(stats), p(dout), W, BOUND, p(dZg), p(dZe), rows, S, M, st()))
        fwd()
        logits = rows * S * (2 * M + 1)
        nbytes_of = {"fwd": 4 * (logits + rows * (BOUND + W + 2 * M + 1)),                  # logits, head; out, stats
                     "bwd": 4 * (2 * logits + rows * (S - 1 + 2 * M + 1))}                  # logits, dq, stats; the two gradients
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, val in us.items():
            rows_of("softmax_moe_" + k, val, nbytes_of[k], rows=rows, S=S, M=M, V1=BOUND,
                    register_resident=bool(lib.yt8m_softmax_moe_resident(S, M)))
    for rows, Vv, bound in LOSS_CASES:
        pr, y = _loss_operands(dev, rows, Vv, bound)
        yb = y.view(torch.uint8)
        loss, dp = torch.empty((1,), device=dev), torch.empty_like(pr)
        ws = torch.empty((rows,), device=dev)
        up = torch.ones((1,), device=dev)
        value = lambda: L.check(lib.yt8m_split_softmax_loss_fwd_bwd(p(pr), Vv, 0, p(yb), 0, p(loss), None, rows, Vv, bound, 10e-6, 10e-8, 1.0,
                                                                    p(ws), st()))
        grad = lambda: L.check(lib.yt8m_split_softmax_loss_bwd(p(pr), Vv, 0, p(yb), 0, p(up), p(dp), rows, Vv, bound, 10e-6, 10e-8, 1.0, st()))
        us = steplib.alternate({"value": value, "gradient": grad}, iters, repeats)
        rows_of("split_softmax_loss value (2 launches)", us["value"], rows * Vv * 5 + 8 * rows, rows=rows, V=Vv, bound=bound)
        rows_of("split_softmax_loss gradient", us["gradient"], rows * Vv * 9, rows=rows, V=Vv, bound=bound)
    return 0


def steps_leg(steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.losses as losses
    import yt8m_amd.ops as ops
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    B = 1024

    def set_flags():
        """A graph keeps none of the flags it was built under: they are set again before every run of a form."""
        FLAGS.reset()
        FLAGS.batch_size = B
        for k, v in SCRIPT.items():
            setattr(FLAGS, k, v)

    x, y, _, _ = steplib.random_batch(dev, B, None, first_label=True)
    y[:, BOUND + 7] = True                                                # every row has an infrequent label too
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    set_flags()
    graphs = {}
    for which, model, loss in (("ce", vlm.MoeSoftmaxModel, losses.CrossEntropyLoss), ("split", vlm.MoeSoftmaxModel, losses.SplitSoftmaxLoss),
                               ("yardstick", vlm.MoeMix4Model, losses.CrossEntropyLoss)):
        graphs[which] = train.build_graph(model(), label_loss_fn=loss(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                          base_learning_rate=0.0)
    forms = {"ce_fused": ("ce", True), "ce_composed": ("ce", False), "split_fused": ("split", True), "split_composed": ("split", False),
             "yardstick": ("yardstick", True)}
    saved = ops.SOFTMAX_MOE_FUSED, ops.SPLIT_SOFTMAX_LOSS_FUSED

    def run(form, n):
        which, fused = forms[form]
        set_flags()
        ops.SOFTMAX_MOE_FUSED = ops.SPLIT_SOFTMAX_LOSS_FUSED = fused
        for _ in range(n):
            out = graphs[which].step(x, y)
        torch.cuda.synchronize()
        return float(out["loss"])

    first = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    ops.SOFTMAX_MOE_FUSED, ops.SPLIT_SOFTMAX_LOSS_FUSED = saved
    FLAGS.reset()
    row = dict(leg="steps", model="MoeSoftmaxModel", yardstick="MoeMix4Model", B=B, V=V, input="float32 [B,1152]", flags=SCRIPT, steps=steps,
               warmup=warmup, repeats=repeats, losses_after_warmup=first, calls=dict(softmax_moe=dict(ops.SOFTMAX_MOE_CALLS),
                                                                                     split_softmax_loss=dict(ops.SPLIT_SOFTMAX_LOSS_CALLS)),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    for loss in ("ce", "split"):
        pair = {"fused": ms[loss + "_fused"], "composed": ms[loss + "_composed"]}
        row.update({loss + "_" + k: v for k, v in steplib.fused_against_composed(pair).items()})
    print(json.dumps(row), flush=True)
    return 0 if all(np.isfinite(v) for v in first.values()) else 1


def summarise(rows):
    """The rows, then one `kernels_summary` row per switch over every run of the `kernels` leg so far."""
    out = list(rows)
    for op, switch in SWITCHES.items():
        timed = [r for r in rows if r.get("leg") == "kernels" and r.get("op") == op]
        if timed:
            out.append(dict(leg="kernels_summary", op=op, switch=switch, runs=len({r["run"] for r in timed}), rows=len(timed),
                            fused_below_composed_everywhere=bool(all(r["fused_below_composed"] for r in timed)),
                            rule="the kernel is the default only if this holds over two runs of the leg"))
    return out


LEGS = ["kernels", "launches", "steps"]


def parser():
    ap = steplib.arg_parser(steps=10, warmup=3, timeout=300)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--kernel_iters", type=int, default=50)
    return ap


def main():
    a = steplib.parse_args(parser(), LEGS)
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child == "launches":
        return launches(a.kernel_iters, a.repeats)
    if a.child:
        return steps_leg(a.steps, a.warmup, a.repeats)
    plan = [(leg, {"run": run}) for run in range(2) for leg in (a.legs or LEGS)]      # every leg twice
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "kernel_iters"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
