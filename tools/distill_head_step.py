"""The head-input and blend ops of Z's cascade heads (ops.distill_input, ops.distill_blend, csrc/distill_head.hip) and the heads on them at
their training scripts' shapes (Z/train_scripts/run-cascade-chaining-video-normalize.sh, run-cascade-lstm-s.sh, run-cascade-lstm-s-split.sh).
`kernels`: forward + backward through autograd, the kernels against the composed forms (the YT8M_DISTILL_INPUT_FUSED=0 /
YT8M_DISTILL_BLEND_FUSED=0 forms), alternating inside every repeat: distill_input in the Chain and Norm2 modes at [B; D + 256; V] =
[128; 1024; 4716], [128; 2048; 4716] and [1024; 1152; 4716] and in the Split mode (v0 = 1000) at the first; distill_blend at [128, 4716]
and [1024, 4716] with (V1, w) = (4716, 0.2) and (1000, 1.0).  x takes a gradient at the first two shapes (an LSTM memory) and is data at
[1024; 1152; 4716] (the video-level step).  Hip events around back-to-back calls, values and gradients compared.  The driver adds a
`kernels_summary` row per op: whether the kernels' median was below the composed form's at every shape in every run of the leg -- what
decides the defaults.
`launches`: the four entry points alone through the C ABI at the same shapes, with the bytes each has to move and the rate in TB/s.
Step legs: whole training steps (fp32, clip + Adam, learning rate 0) at the scripts' flags -- 8 mixtures -- with both switches on, both
off, and of the parent, in ONE process and in turn inside every repeat: `norm2_b128` and `norm2_b1024`, MoeDistillChainNorm2Model on
float features against MoeModel; `gate_chain` and `gate_split`, LstmGateModel + MoeDistillChainModel / MoeDistillSplitModel at B = 128,
F = 300 on the reader's bytes against LstmGateModel + MoeModel.
Every leg runs in a child process of its own under its own time limit, and every leg runs twice (rows numbered by `run`); the driver
stops at the first leg that fails.
usage: python tools/distill_head_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: kernels launches and LEGS"""
import ctypes
import json
import sys

import steplib

V = steplib.V
C = 256
# (mode, B, D, v0, x takes a gradient)
INPUT_CASES = [(mode, B, D, 0, grad) for B, D, grad in ((128, 1024 - C, True), (128, 2048 - C, True), (1024, 1152, False))
               for mode in ("chain", "norm2")] + [("split", 128, 1024 - C, 1000, True)]
BLEND_CASES = [(B, V1, w) for B in (128, 1024) for V1, w in ((V, 0.2), (1000, 1.0))]
# leg: (model, head, parent head, batch, frame level?, flags of the script)
LEGS = {
    "norm2_b128": ("MoeDistillChainNorm2Model", None, "MoeModel", 128, False, dict(moe_num_mixtures=8)),
    "norm2_b1024": ("MoeDistillChainNorm2Model", None, "MoeModel", 1024, False, dict(moe_num_mixtures=8)),
    "gate_chain": ("LstmGateModel", "MoeDistillChainModel", "MoeModel", 128, True, dict(moe_num_mixtures=8, lstm_cells="1024")),
    "gate_split": ("LstmGateModel", "MoeDistillSplitModel", "MoeModel", 128, True, dict(moe_num_mixtures=8, lstm_cells="1024", softmax_bound=1000)),
}


def _input_operands(dev, B, D, seed):
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((B, D), device=dev, generator=gen)
    z = torch.randn((B, C), device=dev, generator=gen)
    t = torch.rand((B, V), device=dev, generator=gen)
    dy = torch.randn((B, D + C), device=dev, generator=gen)
    return x, z, t, dy


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    timing = "hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats" % iters
    for mode, B, D, v0, grad in INPUT_CASES:
        x, z, t, dy = _input_operands(dev, B, D, B + D)

        def run(fused):
            ops.DISTILL_INPUT_FUSED = fused
            xq, zq = x.detach().requires_grad_(grad), z.detach().requires_grad_(True)
            y = ops.distill_input(xq, zq, t, mode, v0)
            y.backward(dy)
            return [y.detach(), zq.grad] + ([xq.grad] if grad else [])

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        ops.DISTILL_INPUT_FUSED = False
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        norm_x, relu, div, norm_c = ops.DISTILL_MODES[mode]
        composed_fwd = int(relu) + 2 * int(div) + int(norm_c) + int(norm_x) + 1          # act, sum + divide (+ mask), l2norms, cat
        print(json.dumps(dict(
            leg="kernels", op="distill_input", mode=mode, B=B, D=D, C=C, V=V, v0=v0, x_takes_gradient=grad,
            what="forward + backward through autograd", launches_fused=2, ops_composed_forward=composed_fwd,
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            max_rel_diff_fused_composed=max(float((a - b).abs().max() / b.abs().max().clamp(min=1.0)) for a, b in zip(rf, rc)),
            repeats=repeats, timing=timing)), flush=True)
    for B, V1, w in BLEND_CASES:
        gen = torch.Generator(device=dev).manual_seed(B + V1)
        p1, t, dout = torch.rand((B, V1), device=dev, generator=gen), torch.rand((B, V), device=dev, generator=gen), torch.randn((B, V), device=dev, generator=gen)

        def run(fused):
            ops.DISTILL_BLEND_FUSED = fused
            pq = p1.detach().requires_grad_(True)
            out = ops.distill_blend(pq, t, w, V1)
            out.backward(dout)
            return [out.detach(), pq.grad]

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        ops.DISTILL_BLEND_FUSED = False
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        print(json.dumps(dict(
            leg="kernels", op="distill_blend", B=B, V=V, V1=V1, w=w, what="forward + backward through autograd", launches_fused=2,
            ops_composed_forward=3 + int(V1 < V),
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            max_abs_diff_fused_composed=max(float((a - b).abs().max()) for a, b in zip(rf, rc)), repeats=repeats, timing=timing)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def launches(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    import yt8m_amd.ops as ops
    lib = L.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    timing = "hip events over %d back-to-back calls through the C ABI" % iters
    for mode, B, D, v0, grad in INPUT_CASES:
        x, z, t, dy = _input_operands(dev, B, D, B + D)
        bits = ops._distill_mode_bits(mode)
        div = ops.DISTILL_MODES[mode][2]
        y, dx, dz = torch.empty((B, D + C), device=dev), (torch.empty((B, D), device=dev) if grad else None), torch.empty((B, C), device=dev)
        s = torch.empty((3, B), device=dev)
        fwd = lambda: L.check(lib.yt8m_distill_input_fwd(bits, p(x), p(z), p(t), V, v0, V, p(y), p(s[0]), p(s[1]), p(s[2]), B, D, C, 1e-12, st()))
        bwd = lambda: L.check(lib.yt8m_distill_input_bwd(bits, p(z), p(y), p(s[0]), p(s[1]), p(s[2]), p(dy), p(dx), p(dz), B, D, C, st()))
        fwd()
        nbytes_of = {"fwd": 4 * B * (D + C + (V - v0 if div else 0) + D + C + 3),
                     "bwd": 4 * B * (C + 2 * C + C + 3 + (3 * D if grad else 0))}      # z, y and dy of the class part, dz; y, dy, dx of the x part
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, val in us.items():
            med = steplib.median(val)
            print(json.dumps(dict(leg="launches", kernel="distill_input_" + k, mode=mode, B=B, D=D, C=C, V=V, v0=v0, dx=grad, bytes=nbytes_of[k],
                                  **steplib.spread_fields("call", val, "us"), TB_per_s=round(nbytes_of[k] / med / 1e6, 3), timing=timing)), flush=True)
    for B, V1, w in BLEND_CASES:
        gen = torch.Generator(device=dev).manual_seed(B + V1)
        p1, t, dout = torch.rand((B, V1), device=dev, generator=gen), torch.rand((B, V), device=dev, generator=gen), torch.randn((B, V), device=dev, generator=gen)
        out, dp1 = torch.empty((B, V), device=dev), torch.empty((B, V1), device=dev)
        fwd = lambda: L.check(lib.yt8m_distill_blend_fwd(p(p1), p(t), V, p(out), B, V, V1, w, st()))
        bwd = lambda: L.check(lib.yt8m_distill_blend_bwd(p(dout), p(dp1), B, V, V1, w, st()))
        nbytes_of = {"fwd": 4 * B * (V1 + V + V), "bwd": 4 * B * 2 * V1}
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, val in us.items():
            med = steplib.median(val)
            print(json.dumps(dict(leg="launches", kernel="distill_blend_" + k, B=B, V=V, V1=V1, w=w, bytes=nbytes_of[k],
                                  **steplib.spread_fields("call", val, "us"), TB_per_s=round(nbytes_of[k] / med / 1e6, 3), timing=timing)), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    model, head, parent_head, B, frames, fl = LEGS[leg]

    def set_flags(which):
        """A graph keeps none of the flags it was built under: they are set again before every run of a form."""
        FLAGS.reset()
        FLAGS.batch_size = B
        for k, v in fl.items():
            setattr(FLAGS, k, v)
        if which == "plugin":
            FLAGS.distillation_features = FLAGS.distillation_as_input = True
            if head:
                FLAGS.video_level_classifier_model = head
        elif frames:
            FLAGS.video_level_classifier_model = parent_head

    x, y, nf, gen = steplib.random_batch(dev, B, 300 if frames else None, "ends", first_label=True)
    batch = (x, y, nf) if frames else (x, y)
    distill = torch.rand((B, V), device=dev, generator=gen) * 0.05
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    graphs = {}
    for which in ("plugin", "parent"):
        set_flags(which)
        cls = getattr(flm, model) if frames else getattr(vlm, model if which == "plugin" else parent_head)
        graphs[which] = train.build_graph(cls(), batch_size=B, graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)
    forms = {"fused": ("plugin", True), "composed": ("plugin", False), "parent": ("parent", False)}

    def run(form, n):
        which, fused = forms[form]
        set_flags(which)
        ops.DISTILL_INPUT_FUSED = ops.DISTILL_BLEND_FUSED = fused
        kw = dict(distill_labels_batch=distill) if which == "plugin" else {}
        for _ in range(n):
            out = graphs[which].step(*batch, **kw)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        return float(out["loss"])

    losses = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    ops.DISTILL_INPUT_FUSED = ops.DISTILL_BLEND_FUSED = False
    FLAGS.reset()
    finite = all(np.isfinite(v) for v in losses.values())
    row = dict(leg=leg, model=model, head=head or model, parent=(model + " + " if frames else "") + parent_head, B=B, V=V,
               input="uint8 [B,300,1152]" if frames else "float32 [B,1152]", flags=fl, ensemble_w=1.0, steps=steps, warmup=warmup,
               repeats=repeats, losses_after_warmup=losses, calls=dict(ops.DISTILL_CALLS),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row.update(steplib.fused_against_composed(ms))
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def summarise(rows):
    """The rows, then one `kernels_summary` row per op over every run of the `kernels` leg so far."""
    out = list(rows)
    for op in ("distill_input", "distill_blend"):
        timed = [r for r in rows if r.get("leg") == "kernels" and r.get("op") == op]
        if timed:
            out.append(dict(leg="kernels_summary", op=op, runs=len({r["run"] for r in timed}), rows=len(timed),
                            fused_below_composed_everywhere=bool(all(r["fused_below_composed"] for r in timed)),
                            rule="the kernel is the default only if this holds over two runs of the leg"))
    return out


def parser():
    ap = steplib.arg_parser(steps=20, warmup=3, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--kernel_iters", type=int, default=200)
    return ap


def main():
    a = steplib.parse_args(parser(), ["kernels", "launches"] + list(LEGS))
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child == "launches":
        return launches(a.kernel_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["kernels", "launches"] + list(LEGS)
    plan = [(leg, {"run": run}) for run in range(2) for leg in legs]      # every leg twice
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "kernel_iters"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
