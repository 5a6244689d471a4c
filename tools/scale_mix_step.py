"""The per-label mix of the scales (ops.scale_mix, csrc/scale_mix.hip) and the three LstmMultiscale plugins on it at the training shape.
`op` (timed first, and run twice by the driver): forward + backward of ops.scale_mix through autograd, the kernels against the composed
form (the YT8M_SCALE_MIX_FUSED=0 form: torch.stack, softmax(dim=0), multiply, sum), at [L, B, V] = [4,128,4716] (the scripts' four
scales), [8,128,4716], [2,128,4716] (the cascade model's two scales) and [4,1024,4716]: hip events around back-to-back calls, the two
forms alternating inside every repeat, values and gradients compared.  Every plane takes a gradient, as outside a training step.  The
driver adds an `op_summary` row: whether the kernels' median was below the composed one at every shape in both runs -- what decides the
default.
`kernels`: yt8m_scale_mix_fwd and yt8m_scale_mix_bwd alone through the C ABI at the same shapes, with the bytes each has to move (fwd:
2 L planes read, one written; bwd: 2 L + 2 read, 2 L written) and the rate in TB/s.
`step`: whole training steps (the Z rule's cross entropy on prediction_frames, clip, Adam; learning rate 0) of the three plugins under
the scripts' flags -- 4 scales, 1024 cells, 4 mixtures; the cascade model also with 2 scales and 8 mixtures -- at B = 128, F = 300 on the
reader's bytes with the switch on and off, MultiscaleCnnLstmModel (4 scales) and LstmGateModel in the same run for the scale.  In a
training step predictions are built without a graph: the switch moves the forward launch only.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/scale_mix_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op kernels step"""
import ctypes
import json
import sys

import steplib

V = steplib.V
SHAPES = ((4, 128, V), (8, 128, V), (2, 128, V), (4, 1024, V))           # (L, B, V)
B, F = 128, 300
# (plugin, --moe_num_extend, --moe_num_mixtures, cascade input): Z/train_scripts' lstm_multiscale4_moe4, lstm_gate_multiscale4_moe4,
# distillchain_lstm_multiscale_layer4_moe8's family at 4 mixtures and at layer2_moe8
PLUGINS = (("LstmMultiscaleModel", 4, 4, False), ("LstmMultiscale2Model", 4, 4, False), ("LstmMultiscaleDitillChainModel", 4, 4, True),
           ("LstmMultiscaleDitillChainModel", 2, 8, True))
SCALE = ("MultiscaleCnnLstmModel", "LstmGateModel")


def _inputs(dev, shape, seed):
    import torch
    L_, B_, V_ = shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.rand((B_, V_), device=dev, generator=gen) for _ in range(L_)]
    zs = [2.0 * torch.randn((B_, V_), device=dev, generator=gen) for _ in range(L_)]
    g = torch.randn((B_, V_), device=dev, generator=gen)
    return ps, zs, g


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    for shape in SHAPES:
        L_, B_, V_ = shape
        ps, zs, g = _inputs(dev, shape, sum(shape))

        def run(fused):
            ops.SCALE_MIX_FUSED = fused
            pt = [p.detach().requires_grad_(True) for p in ps]
            zt = [z.detach().requires_grad_(True) for z in zs]
            out = ops.scale_mix(pt, zt)
            out.backward(g)
            return [out.detach()] + [t.grad for t in pt] + [t.grad for t in zt]

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        ops.SCALE_MIX_FUSED = False
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        diff = max(float((a - b).abs().max()) for a, b in zip(rf, rc))
        print(json.dumps(dict(
            leg="op", L=L_, B=B_, V=V_, what="forward + backward through autograd", plane_bytes=4 * B_ * V_,
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_), max_abs_diff_fused_composed=diff,
            calls=dict(ops.SCALE_MIX_CALLS), repeats=repeats,
            timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats" % iters)),
            flush=True)
        del ps, zs, g
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
    table = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    for shape in SHAPES:
        L_, B_, V_ = shape
        ps, zs, g = _inputs(dev, shape, sum(shape))
        out = torch.empty((B_, V_), device=dev)
        dp, dz = [torch.empty_like(out) for _ in range(L_)], [torch.empty_like(out) for _ in range(L_)]
        tp, tz, tdp, tdz = table(ps), table(zs), table(dp), table(dz)
        fwd = lambda: L.check(lib.yt8m_scale_mix_fwd(L_, tp, tz, p(out), B_, V_, st()))
        bwd = lambda: L.check(lib.yt8m_scale_mix_bwd(L_, tp, tz, p(out), p(g), tdp, tdz, B_, V_, st()))
        fwd()
        plane = 4 * B_ * V_
        nbytes_of = {"fwd": (2 * L_ + 1) * plane, "bwd": (4 * L_ + 2) * plane}
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, val in us.items():
            med = steplib.median(val)
            print(json.dumps(dict(leg="kernels", kernel=k, L=L_, B=B_, V=V_, bytes=nbytes_of[k], **steplib.spread_fields("call", val, "us"),
                                  TB_per_s=round(nbytes_of[k] / med / 1e6, 3), measured_streaming_read_TB_per_s="6.0-6.3",
                                  timing="hip events over %d back-to-back calls through the C ABI" % iters)), flush=True)
        del ps, zs, g, out, dp, dz
        torch.cuda.empty_cache()
    return 0


def step(steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    x, y, nf, gen = steplib.random_batch(dev, B, F, "ends", first_label=True)
    distill = torch.rand((B, V), device=dev, generator=gen) * 0.05
    rc = 0

    def flags_for(name, num_extend, mixtures, cascade):
        FLAGS.reset()
        FLAGS.batch_size = B
        fl = dict(lstm_cells="1024", moe_num_mixtures=mixtures, is_training=True)
        if name in SCALE:
            fl.update(multiscale_cnn_lstm_layers=4)
        else:
            fl.update(moe_num_extend=num_extend)
        if cascade:
            fl.update(distillation_features=True, distillation_as_input=True)
        for k, v in fl.items():
            setattr(FLAGS, k, v)
        return fl

    for plugin, num_extend, mixtures, cascade in PLUGINS:
        # learning rate 0 (the step does the same work): the steps repeat one random batch.  A graph keeps the flags it was built under.
        graphs, flags_of = {}, {}
        for name in (plugin,) + SCALE:
            flags_of[name] = flags_for(name, num_extend, mixtures, cascade and name == plugin)
            graphs[name] = train.build_graph(getattr(flm, name)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                             base_learning_rate=0.0)
        forms = {"fused": (plugin, True), "composed": (plugin, False), "multiscale_cnn_lstm": (SCALE[0], False), "lstm_gate": (SCALE[1], False)}

        def run(form, n):
            which, fused = forms[form]
            flags_for(which, num_extend, mixtures, cascade and which == plugin)
            ops.SCALE_MIX_FUSED = fused
            kw = {"distill_labels_batch": distill} if (cascade and which == plugin) else {}
            for _ in range(n):
                out = graphs[which].step(x, y, nf, **kw)
            torch.cuda.synchronize()
            seq_ops.check_persist_errors()
            return float(out["loss"])

        losses_ = {k: run(k, warmup) for k in forms}
        ms = steplib.steps_in_turn(run, forms, steps, repeats)
        ops.SCALE_MIX_FUSED = False
        row = dict(leg="step", plugin=plugin, scale=list(SCALE), B=B, V=V, input="uint8 [B,300,1152]", flags=flags_of[plugin], steps=steps,
                   warmup=warmup, repeats=repeats, losses_after_warmup=losses_, calls=dict(ops.SCALE_MIX_CALLS),
                   timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
        for k, v in ms.items():
            row.update(steplib.spread_fields(k, v, "ms"))
        row.update(steplib.fused_against_composed(ms))
        row["fused_below_composed"] = bool(steplib.median(ms["fused"]) < steplib.median(ms["composed"]))
        print(json.dumps(row), flush=True)
        rc = rc or (0 if all(np.isfinite(v) for v in losses_.values()) else 1)
        del graphs
        torch.cuda.empty_cache()
    FLAGS.reset()
    return rc


def summarise(rows):
    return steplib.verdict_after(rows, "op", "leg_repeat", "the kernels are the default only if this holds over two runs of the leg")


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=20)
    return ap


def main():
    a = steplib.parse_args(parser(), ["op", "kernels", "step"])
    if a.child == "op":
        return op(a.op_iters, a.repeats)
    if a.child == "kernels":
        return kernels(a.op_iters, a.repeats)
    if a.child == "step":
        return step(a.steps, a.warmup, a.repeats)
    legs = a.legs or ["op", "op", "kernels", "step"]                     # the op leg twice: its verdict wants two runs of the leg
    return steplib.drive(__file__, steplib.numbered(legs, "op", "leg_repeat"), steplib.child_args(a, "repeats", "op_iters"), a.timeout, a.out,
                         summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
