"""The ensemble stage's combine (ops.ens_combine, csrc/ensemble.hip) and two of its plugins at the training scripts' shapes.
`op` (timed first, and run twice by the driver: two repeats of the leg): forward + backward of ops.ens_combine through autograd, the fused
kernels against the composed torch form (the YT8M_ENSEMBLE_FUSED=0 form), on method-major predictions [1024, 4716, 74], [1024, 4716, 9]
and [128, 4716, 74] with J = 4 gated tables and with J = 1 table and no gate: hip events around back-to-back calls, the two forms
alternating inside every repeat, the spread over the repeats recorded, values and gradients compared.  The driver adds an `op_summary`
row: whether the fused median was below the composed one at every shape in both repeats of the leg -- what decides the default of the
switch.
`kernels`: yt8m_ens_combine_fwd, yt8m_ens_combine_bwd and yt8m_ens_moments alone through the C ABI at [1024, 4716, 74], with the bytes
each has to move computed from the shapes and the rate in TB/s (to be read against the 6.0-6.3 TB/s a streaming read reaches on this chip).
Step legs: whole training steps (cross entropy, clip, Adam; learning rate 0) of MatrixRegressionModel and of AttentionMatrixModel (J = 4,
R = 8, as E/ensemble_scripts/train-attention_matrix_model.sh) at B = 1024, M = 74 with the switch on and off, in ONE process and in turn
inside every repeat.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/ensemble_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op kernels matrix attention"""
import ctypes
import json
import sys

import steplib

V = steplib.V
OP_SHAPES = ((1024, V, 74), (1024, V, 9), (128, V, 74))
LEGS = {
    "matrix": ("MatrixRegressionModel", dict()),
    "attention": ("AttentionMatrixModel", dict(moe_num_mixtures=4, attention_matrix_rank=8)),
}
D_INPUT = 1152


def _inputs(dev, B, M, J, seed):
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((M, B, V), device=dev, generator=gen).permute(1, 2, 0)            # method-major, as EnsembleInput delivers it
    W = torch.randn((J, V, M), device=dev, generator=gen)
    gate = torch.softmax(torch.randn((B, J), device=dev, generator=gen), dim=-1) if J > 1 else None
    coef = torch.randn((B, V), device=dev, generator=gen)
    return x, W, gate, coef


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    for B, _, M in OP_SHAPES:
        for J in (4, 1):
            x, W, gate, coef = _inputs(dev, B, M, J, B + M + J)

            def run(fused):
                ops.ENSEMBLE_FUSED = fused
                Wl = W.detach().requires_grad_(True)
                gl = None if gate is None else gate.detach().requires_grad_(True)
                y = ops.ens_combine(x, Wl, gl)
                y.backward(coef)
                return y.detach(), Wl.grad, None if gl is None else gl.grad

            forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
            us = steplib.alternate(forms, iters, repeats)
            (yf, wf, gf), (yc, wc, gc) = forms["fused"](), forms["composed"]()
            f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
            print(json.dumps(dict(
                leg="op", B=B, V=V, M=M, J=J, gate=gate is not None, what="forward + backward through autograd", x_bytes=4 * B * V * M,
                **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
                composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
                y_diff_fused_composed=float((yf - yc).abs().max()),
                dW_diff_fused_composed_rel_to_max=float((wf - wc).abs().max() / wc.abs().max()),
                dgate_diff_fused_composed_rel_to_max=None if gf is None else float((gf - gc).abs().max() / gc.abs().max()),
                repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                        % iters)), flush=True)
            del x, W, gate, coef
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
    for J in (4, 1):
        x, W, gate, dout = _inputs(dev, B, M, J, 5 + J)
        Wt = W.permute(0, 2, 1).contiguous()
        out, mean, var = (torch.empty((B, V), device=dev) for _ in range(3))
        stat = torch.empty((2, B, V), device=dev)
        dWt, dgate = torch.empty_like(Wt), None if gate is None else torch.empty_like(gate)
        nbytes = lib.yt8m_ens_combine_bwd_workspace_bytes(B, V, M, J)
        ws = torch.empty(nbytes // 4, device=dev)
        fwd = lambda: L.check(lib.yt8m_ens_combine_fwd(p(x), p(Wt), p(gate), 0, p(out), p(stat), B, V, M, J, st()))
        bwd = lambda: L.check(lib.yt8m_ens_combine_bwd(p(x), p(Wt), p(gate), 0, p(out), p(stat), p(dout), p(dWt), p(dgate), p(ws), nbytes,
                                                       B, V, M, J, st()))
        mom = lambda: L.check(lib.yt8m_ens_moments(p(x), p(mean), p(var), B, V, M, st()))
        xb, tb, bv = 4 * B * V * M, 4 * J * V * M, 4 * B * V
        chunks = min(8, (B + 15) // 16)
        dgate_parts = 0 if gate is None else 4 * B * J * ((V + 255) // 256) * ((M + 3) // 4)
        # what each call has to move: x once; the tables; out / stat / dout planes; backward: the per-chunk partial tables written and
        # read once more, the dgate partials likewise
        nbytes_of = {"fwd": xb + tb + 3 * bv, "bwd": xb + tb + 4 * bv + (2 * chunks + 1) * tb + 2 * dgate_parts, "moments": xb + 2 * bv}
        forms = {"fwd": fwd, "bwd": bwd}
        if J == 4:
            forms["moments"] = mom
        us = steplib.alternate(forms, iters, repeats)
        for k, v in us.items():
            med = steplib.median(v)
            print(json.dumps(dict(leg="kernels", kernel=k, B=B, V=V, M=M, J=J if k != "moments" else None, bytes=nbytes_of[k],
                                  **steplib.spread_fields("call", v, "us"), TB_per_s=round(nbytes_of[k] / med / 1e6, 3),
                                  x_only_TB_per_s=round(xb / med / 1e6, 3), measured_streaming_read_TB_per_s="6.0-6.3",
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
        ops.ENSEMBLE_FUSED = forms[form]
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


def summarise(rows):
    return steplib.verdict_after(rows, "op", "leg_repeat", "fused is the default only if this holds over two repeats of the leg")


def parser():
    ap = steplib.arg_parser(steps=10, warmup=3, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=10)
    return ap


def main():
    a = steplib.parse_args(parser(), ["op", "kernels"] + list(LEGS))
    if a.child == "op":
        return op(a.op_iters, a.repeats)
    if a.child == "kernels":
        return kernels(a.op_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["op", "op", "kernels"] + list(LEGS)                # the op leg twice: its verdict wants two repeats of the leg
    return steplib.drive(__file__, steplib.numbered(legs, "op", "leg_repeat"), steplib.child_args(a, "repeats", "op_iters"),
                         a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
