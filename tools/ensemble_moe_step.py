"""The ensemble stage's per-class matrix mix and per-video mix (ops.ens_tensor_moe, ops.ens_mix, csrc/ensemble_tensor.hip) and their three
plugins at the training scripts' shapes.
`tensor_op`, `mix_op` (each run twice by the driver: two repeats of the leg): forward + backward of the op through autograd, the fused
kernels against the composed torch form (the YT8M_ENS_TENSOR_FUSED=0 / YT8M_ENS_MIX_FUSED=0 form), on method-major predictions
[1024, 4716, 74], [128, 4716, 74], [1024, 4716, 30] and [1024, 4716, 9]: hip events around back-to-back calls, the two forms alternating
inside every repeat, the spread over the repeats recorded, values and gradients compared.  The fused form's time includes the re-layout
of the weights (103 MB at M = 74) and of their gradient.  The driver adds a `<leg>_summary` row: whether the fused median was below the
composed one at every shape in both repeats of the leg -- what decides the default of the op's switch.
`kernels`: the four kernels alone through the C ABI at [1024, 4716, 74], with the bytes each has to move and its FLOPs computed from the
shapes, the rates in TB/s and TFLOP/s (to be read against 6 TB/s and 157 TFLOP/s of fp32).
Step legs: whole training steps (cross entropy, clip, Adam; learning rate 0) of MoeModel, InputMoeModel and AttentionMoeModel
(--attention_relu_cells=128) at B = 1024, M = 74 with the switches on and off, and of MatrixRegressionModel as the yardstick, in ONE
process per leg and in turn inside every repeat.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/ensemble_moe_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]
legs: tensor_op mix_op kernels moe input attention matrix"""
import ctypes
import json
import sys

import steplib

V = steplib.V
OP_SHAPES = ((1024, V, 74), (128, V, 74), (1024, V, 30), (1024, V, 9))
LEGS = {
    "moe": ("MoeModel", dict()),
    "input": ("InputMoeModel", dict()),
    "attention": ("AttentionMoeModel", dict(attention_relu_cells=128)),
    "matrix": ("MatrixRegressionModel", dict()),
}
D_INPUT = 1152
HBM_TB_S, FP32_TFLOPS = 6.0, 157.0


def _inputs(dev, B, M, seed):
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((M, B, V), device=dev, generator=gen).permute(1, 2, 0)            # method-major, as EnsembleInput delivers it
    W = torch.rand((V, M, M), device=dev, generator=gen) * 2.0 - 1.0
    b = torch.randn((V, M), device=dev, generator=gen)
    a = torch.softmax(torch.randn((B, M), device=dev, generator=gen), dim=-1)
    coef = torch.randn((B, V), device=dev, generator=gen)
    return x, W, b, a, coef


def op(which, iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
    for B, _, M in OP_SHAPES:
        x, W, b, a, coef = _inputs(dev, B, M, B + M)

        def run(fused):
            if which == "tensor_op":
                ops.ENS_TENSOR_FUSED = fused
                Wl, bl = W.detach().requires_grad_(True), b.detach().requires_grad_(True)
                y = ops.ens_tensor_moe(x, Wl, bl)
                y.backward(coef)
                return y.detach(), Wl.grad, bl.grad
            ops.ENS_MIX_FUSED = fused
            al = a.detach().requires_grad_(True)
            y = ops.ens_mix(x, al)
            y.backward(coef)
            return y.detach(), al.grad

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        f, c = forms["fused"](), forms["composed"]()
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        print(json.dumps(dict(
            leg=which, B=B, V=V, M=M, what="forward + backward through autograd", x_bytes=4 * B * V * M,
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            y_diff_fused_composed=float((f[0] - c[0]).abs().max()),
            grad_diff_fused_composed_rel_to_max=[rel(p, q) for p, q in zip(f[1:], c[1:])],
            repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations, autograd and the re-layout of the weights "
                                    "included), median of the repeats" % iters)), flush=True)
        del x, W, b, a, coef, f, c
        torch.cuda.empty_cache()
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    lib = L.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, M = 1024, 74
    x, W, b, a, dout = _inputs(dev, B, M, 5)
    Wt, bt = W.permute(1, 2, 0).contiguous(), b.t().contiguous()
    out, stat = torch.empty((B, V), device=dev), torch.empty((2, B, V), device=dev)
    dWt, dbt, da = torch.empty_like(Wt), torch.empty_like(bt), torch.empty_like(a)
    nbytes = lib.yt8m_ens_tensor_bwd_workspace_bytes(B, V, M)
    ws = torch.empty(max(nbytes, 16) // 4, device=dev)
    forms = {
        "tensor_fwd": lambda: L.check(lib.yt8m_ens_tensor_fwd(p(x), p(Wt), p(bt), p(out), p(stat), B, V, M, st())),
        "tensor_bwd": lambda: L.check(lib.yt8m_ens_tensor_bwd(p(x), p(Wt), p(bt), p(out), p(stat), p(dout), p(dWt), p(dbt), p(ws), nbytes,
                                                               B, V, M, st())),
        "mix_fwd": lambda: L.check(lib.yt8m_ens_mix_fwd(p(x), p(a), p(out), B, V, M, st())),
        "mix_bwd": lambda: L.check(lib.yt8m_ens_mix_bwd(p(x), p(dout), p(da), B, V, M, st())),
        "relayout_W": lambda: W.permute(1, 2, 0).contiguous(),
    }
    xb, wb, bv = 4 * B * V * M, 4 * V * M * (M + 1), 4 * B * V
    # what each call has to move once: x; the weights; the out / stat / dout planes; backward: the weight gradients written
    nbytes_of = {"tensor_fwd": xb + wb + 3 * bv, "tensor_bwd": xb + 2 * wb + 4 * bv, "mix_fwd": xb + bv + 4 * B * M,
                 "mix_bwd": xb + bv + 4 * B * M, "relayout_W": 8 * V * M * M}
    flops_of = {"tensor_fwd": 2.0 * B * V * M * M, "tensor_bwd": 4.0 * B * V * M * M, "mix_fwd": 2.0 * B * V * M, "mix_bwd": 2.0 * B * V * M,
                "relayout_W": 0.0}
    us = steplib.alternate(forms, iters, repeats)
    for k, v in us.items():
        med = steplib.median(v)
        print(json.dumps(dict(leg="kernels", kernel=k, B=B, V=V, M=M, bytes=nbytes_of[k], flops=flops_of[k],
                              **steplib.spread_fields("call", v, "us"), TB_per_s=round(nbytes_of[k] / med / 1e6, 3),
                              TFLOP_per_s=round(flops_of[k] / med / 1e6, 2), against_TB_per_s=HBM_TB_S, against_fp32_TFLOP_per_s=FP32_TFLOPS,
                              timing="hip events over %d back-to-back calls through the C ABI" % iters)), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.ensemble as ensemble
    import yt8m_amd.ensemble_level_models as elm
    import yt8m_amd.ops as ops
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    plugin, fl = LEGS[leg]
    B, M = 1024, 74
    FLAGS.reset()
    FLAGS.batch_size = B
    for k, v in fl.items():
        setattr(FLAGS, k, v)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((M, B, V), device=dev, generator=gen).permute(1, 2, 0)
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    orig = torch.randn((B, D_INPUT), device=dev, generator=gen)
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    tg = ensemble.EnsembleTrainGraph(getattr(elm, plugin)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                     base_learning_rate=0.0)
    forms = {"fused": True, "composed": False}

    def run(form, n):
        # the yardstick leg has neither op on its path: its two forms are the same step, and their difference is the noise of the run
        ops.ENS_TENSOR_FUSED = ops.ENS_MIX_FUSED = forms[form]
        for _ in range(n):
            out = tg.step(x, y, original_input=orig)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    finite = all(np.isfinite(v) for v in losses_.values())
    row = dict(leg=leg, plugin=plugin, B=B, V=V, M=M, input="method-major float32 [B, V, M] + original_input [B, %d]" % D_INPUT, flags=fl,
               steps=steps, warmup=warmup, repeats=repeats, losses_after_warmup=losses_,
               loss_diff_fused_composed=abs(losses_["fused"] - losses_["composed"]),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row.update(steplib.fused_against_composed(ms))
    row["composed_over_fused"] = round(steplib.median(ms["composed"]) / steplib.median(ms["fused"]), 2)
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


RULE = "fused is the default only if this holds over two repeats of the leg"


def summarise(rows):
    return steplib.verdict_after(steplib.verdict_after(rows, "tensor_op", "tensor_repeat", RULE), "mix_op", "mix_repeat", RULE)


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=5)
    return ap


def main():
    a = steplib.parse_args(parser(), ["tensor_op", "mix_op", "kernels"] + list(LEGS))
    if a.child in ("tensor_op", "mix_op"):
        return op(a.child, a.op_iters, a.repeats)
    if a.child == "kernels":
        return kernels(a.op_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["tensor_op", "mix_op", "kernels"] * 2 + list(LEGS) * 2                  # every leg twice
    plan = steplib.numbered(steplib.numbered(legs, "tensor_op", "tensor_repeat"), "mix_op", "mix_repeat")
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "op_iters"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
