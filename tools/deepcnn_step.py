"""seq_ops.max_pool2_tm (csrc/deep_cnn.hip) and the two plugins on the byte CNN at their training scripts' shapes.
`op` (timed first, and run twice by the driver: two runs of the leg): seq_ops.max_pool2_tm forward plus backward through autograd, the
one-pass kernels against the composed form (YT8M_DEEP_CNN_FUSED=0: yt8m_timepool_max_f32, a pair maximum from torch ops, and in backward
a zero-fill, a scatter, the pair maximum's backward and an add), at the shapes of OP_SHAPES: hip events around back-to-back calls, the two
forms alternating inside every repeat, the spread over the repeats recorded, the values compared; then the two launches alone through the
C ABI on buffers made once, with the bytes their shapes imply.  The driver adds an `op_summary` row:
whether the kernels' median was below the composed one at every shape in both runs of the leg -- what decides the default of the switch
(DESIGN_LOG.md section 23's rule).
Step legs: whole training steps (fp32, clip + Adam, learning rate 0) on raw uint8 frames [128, 300, 1152], V = 4716 --
`deepcnn`: DeepCnnDeepCombineChainModel at run-chaining-deep-cnn.sh's flags with the switch on and off, and CnnDeepCombineChainModel at
the same chain flags as the yardstick, the three in turn inside every repeat; `cnnlstm`: CnnLstmMemoryModel at run-cnn-lstm.sh's flags
and LstmMemoryModel with the same cells in turn, with the (F, D, H) of every native stack call of a step.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/deepcnn_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op deepcnn cnnlstm"""
import ctypes
import json
import os
import sys

import steplib

V, B, F = steplib.V, 128, 300
CHAIN = dict(deep_chain_layers=2, deep_chain_relu_cells=256, moe_num_mixtures=4, multitask=True, label_loss="MultiTaskCrossEntropyLoss",
             support_type="label,label", dropout=True, keep_prob=1.0)
# leg: [(form, plugin, flags, YT8M_DEEP_CNN_FUSED or None)] -- training_scripts/run-chaining-deep-cnn.sh, run-cnn-lstm.sh
LEGS = {
    "deepcnn": [("fused", "DeepCnnDeepCombineChainModel", dict(CHAIN, deep_cnn_base_size=128), "1"),
                ("composed", "DeepCnnDeepCombineChainModel", dict(CHAIN, deep_cnn_base_size=128), "0"),
                ("yardstick", "CnnDeepCombineChainModel", dict(CHAIN), None)],
    "cnnlstm": [("cnnlstm", "CnnLstmMemoryModel", dict(lstm_cells="1024", lstm_layers=2, moe_num_mixtures=8), None),
                ("yardstick", "LstmMemoryModel", dict(lstm_cells="1024", lstm_layers=2, moe_num_mixtures=8), None)],
}
OP_SHAPES = ((300, 128, 512), (150, 128, 256), (300, 32, 512))          # level 0 and level 1 of the script's deep CNN, a quarter batch


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as _lib
    import yt8m_amd.seq_ops as seq_ops
    lib = _lib.lib()
    for f, b, c in OP_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(f + b + c)
        y = torch.randn((f * b, c), device=dev, generator=gen).requires_grad_(True)
        gm = torch.randn((b, c), device=dev, generator=gen)
        gp = torch.randn((f // 2, b, c), device=dev, generator=gen)

        def run(fused):
            os.environ["YT8M_DEEP_CNN_FUSED"] = "1" if fused else "0"
            y.grad = None
            m, p = seq_ops.max_pool2_tm(y, f, b)
            torch.autograd.backward([m, p], [gm, gp])
            return m.detach(), p.detach(), y.grad

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        same = all(bool(torch.equal(a, c_)) for a, c_ in zip(forms["fused"](), forms["composed"]()))
        full, half, small = 4 * f * b * c, 4 * (f // 2) * b * c, 4 * b * c
        moved = (full + half + 2 * small) + (full + half + 2 * small + full)     # forward: y -> p, m, idx; backward: y, dp, g, idx -> dy
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        # the two launches alone, through the C ABI on buffers made once: no autograd, no allocation
        yd, dy = y.detach(), torch.empty((f * b, c), device=dev)
        m, idx = torch.empty((b, c), device=dev), torch.empty((b, c), device=dev, dtype=torch.int32)
        pooled = torch.empty((f // 2, b, c), device=dev)
        st, P = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), lambda t: ctypes.c_void_p(t.data_ptr())
        kernels = {
            "fwd_kernel": lambda: _lib.check(lib.yt8m_timepool_max_pool2_f32_fwd(P(yd), c, f, b, c, P(m), P(idx), c, P(pooled), c, st)),
            "bwd_kernel": lambda: _lib.check(lib.yt8m_timepool_max_pool2_f32_bwd(P(yd), c, f, b, c, P(gm), P(idx), c, P(gp), c, P(dy), c, st))}
        ku = steplib.alternate(kernels, iters, repeats)
        kbytes = {"fwd_kernel": full + half + 2 * small, "bwd_kernel": 2 * full + half + 2 * small}
        krow = {}
        for k, v in ku.items():
            krow.update(steplib.spread_fields(k, v, "us"))
            krow[k + "_bytes"] = kbytes[k]
            krow[k + "_tb_per_s"] = round(kbytes[k] / steplib.median(v) * 1e-6, 3)
        print(json.dumps(dict(
            leg="op", F=f, B=b, C=c, launches_fused=2, bytes_moved_fused=moved,
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            fused_tb_per_s=round(moved / f_ * 1e-6, 3), composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            outputs_and_dy_bitwise_equal=same, repeats=repeats, **krow,
            timing="hip events over %d back-to-back forward + backward calls (torch allocations included), median of the repeats" % iters)),
            flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    batch = steplib.random_batch(dev, B, F, "ends", first_label=True)[:3]
    stacks = []                                                           # (F, D, H) per native stack call
    native_forward = seq_ops._LstmStack._native_forward

    def recording_forward(ctx, *a, **k):
        stacks.append((a[1].F, a[1].D, a[1].H))
        return native_forward(ctx, *a, **k)

    seq_ops._LstmStack._native_forward = staticmethod(recording_forward)
    graphs, flags_of = {}, {}

    def enter(form):
        """The flags and the switch of a form: a step reads both."""
        _, _, fl, switch = next(e for e in LEGS[leg] if e[0] == form)
        FLAGS.reset()
        FLAGS.batch_size = B
        for k, v in fl.items():
            setattr(FLAGS, k, v)
        if switch is not None:
            os.environ["YT8M_DEEP_CNN_FUSED"] = switch

    for form, plugin, fl, _ in LEGS[leg]:
        enter(form)
        # learning rate 0 (the step does the same work): the steps repeat one random batch
        graphs[form] = train.build_graph(getattr(flm, plugin)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                         base_learning_rate=0.0)
        flags_of[form] = fl

    def run(form, n):
        enter(form)
        for _ in range(n):
            out = graphs[form].step(*batch)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_, stacks_of = {}, {}
    for form in graphs:
        losses_[form] = run(form, warmup)
        del stacks[:]
        run(form, 1)
        stacks_of[form] = [list(s) for s in stacks]
    ms = steplib.steps_in_turn(run, graphs, steps, repeats)
    seq_ops.check_persist_errors()
    finite = all(np.isfinite(v) for v in losses_.values())
    row = dict(leg=leg, B=B, V=V, input="uint8 [B,300,1152]", plugins={e[0]: e[1] for e in LEGS[leg]}, flags=flags_of, steps=steps,
               warmup=warmup, repeats=repeats, losses_after_warmup=losses_, native_stacks_F_D_H=stacks_of,
               max_memory_allocated_bytes=int(torch.cuda.max_memory_allocated()),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    if "composed" in ms:                                                 # this row states no verdict: the op leg's summary decides the default
        against = steplib.fused_against_composed(ms)
        row.update((k, against[k]) for k in ("fused_minus_composed_ms", "spread_between_repeats_ms"))
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def summarise(rows):
    return steplib.verdict_after(rows, "op", "leg_run", "the kernels are the default only if this holds over two runs of the leg")


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=20)
    return ap


def main():
    a = steplib.parse_args(parser(), ["op"] + list(LEGS))
    if a.child == "op":
        return op(a.op_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["op", "op"] + list(LEGS)                           # the op leg twice: its verdict wants two runs of the leg
    return steplib.drive(__file__, steplib.numbered(legs, "op", "leg_run"), steplib.child_args(a, "repeats", "op_iters"),
                         a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
