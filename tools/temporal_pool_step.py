"""The frame pyramid (ops.frame_pyramid, csrc/frame_pyramid.hip) and the two temporal-pooling LSTM plugins at their training scripts' shapes.
`pyramid` (timed first, and run twice by the driver: two runs of the leg): ops.frame_pyramid on reader bytes, the one-pass kernel against
the composed form (YT8M_FRAME_PYRAMID_FUSED=0: per level resolution_mean -> slices -> l2_normalize -> transpose copy), at the shapes of
PYRAMID_SHAPES: hip events around back-to-back calls, the two forms alternating inside every repeat, the spread over the repeats recorded,
the values compared.  The driver adds a `pyramid_summary` row: whether the kernel's median was below the composed one at every shape in both
runs of the leg -- what decides the default of the switch (DESIGN_LOG.md section 23's rule).
Step legs (one per plugin): whole training steps (fp32, clip + Adam, learning rate 0) of the plugin at its training script's flags on raw
uint8 frames [128, 300, 1152] under IdenticalTransformer -- the multi-resolution one with the switch on and off, in turn inside every
repeat -- with the bytes the ten stacks keep resident (native scratch, persistent workspaces) and on their tapes, and the evictions of the
resident tables during the timed steps.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/temporal_pool_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `pyramid`"""
import json
import sys

import steplib

V, B, F = steplib.V, 128, 300
TOWER = dict(feature_sizes="1024,128", lstm_cells="512,64", lstm_layers=2, deep_chain_layers=4, deep_chain_relu_cells=256, moe_num_mixtures=4,
             feature_transformer="IdenticalTransformer")
# leg: (plugin, flags) -- training_scripts/run-chaining-multi-resolution-lstm.sh, run-temporal-pooling-lstm.sh
LEGS = {
    "multires": ("MultiresLstmMemoryDeepCombineChainModel",
                 dict(multitask=True, label_loss="MultiTaskCrossEntropyLoss", support_type="label,label,label,label", support_loss_percent=0.05,
                      dropout=True, keep_prob=0.9, **TOWER)),
    "framehop": ("FramehopLstmMemoryModel", dict(TOWER)),
}
# (B, F, widths, levels): the reader's shape at the script's settings, a quarter of the batch, two levels only
PYRAMID_SHAPES = ((128, 300, (1024, 128), 4), (32, 300, (1024, 128), 4), (128, 300, (1024, 128), 2))


def pyramid(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    for b, f, widths, levels in PYRAMID_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(b + levels)
        q = torch.randint(0, 256, (b, f, sum(widths)), device=dev, generator=gen, dtype=torch.uint8)
        nf = torch.randint(1, f + 1, (b,), device=dev, generator=gen, dtype=torch.int32)
        nf[0], nf[1] = f, 1

        def run(fused):
            ops.FRAME_PYRAMID_FUSED = fused
            return ops.frame_pyramid(q, nf, levels, widths)

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        (pf, nf_f), (pc, nf_c) = forms["fused"](), forms["composed"]()
        ops.FRAME_PYRAMID_FUSED = True
        diff = max(float((a - c).abs().max()) for ra, rc in zip(pf, pc) for a, c in zip(ra, rc))
        same_frames = all(bool(torch.equal(a, c)) for a, c in zip(nf_f, nf_c))
        out_bytes = sum(4 * (f >> (l + 1)) * b * sum(widths) for l in range(levels))
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        n = len(widths)
        print(json.dumps(dict(
            leg="pyramid", B=b, F=f, widths=list(widths), levels=levels, launches_fused=1, launches_composed=levels * (1 + 3 * n),
            bytes_read_once=b * f * sum(widths), bytes_written=out_bytes,
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            fused_tb_per_s=round((b * f * sum(widths) + out_bytes) / f_ * 1e-6, 3),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            y_diff_fused_composed=diff, num_frames_equal=same_frames, repeats=repeats,
            timing="hip events over %d back-to-back calls (torch allocations included), median of the repeats" % iters)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    plugin, fl = LEGS[leg]
    FLAGS.reset()
    FLAGS.batch_size = B
    for k, v in fl.items():
        setattr(FLAGS, k, v)
    batch = steplib.random_batch(dev, B, F, "ends", first_label=True)[:3]
    tapes = []                                                            # (tape bytes, scratch bytes, (F, D, H)) per native stack call
    native_forward = seq_ops._LstmStack._native_forward

    def recording_forward(ctx, *a, **k):
        res = native_forward(ctx, *a, **k)
        tapes.append((ctx.native[1].numel(), ctx.native[2].numel(), (a[1].F, a[1].D, a[1].H)))
        return res

    seq_ops._LstmStack._native_forward = staticmethod(recording_forward)
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    tg = train.build_graph(getattr(flm, plugin)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)
    forms = {"fused": True, "composed": False} if leg == "multires" else {"fused": True}

    def run(form, n):
        ops.FRAME_PYRAMID_FUSED = forms[form]
        for _ in range(n):
            out = tg.step(*batch)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    del tapes[:]
    run("fused", 1)
    step_tapes = list(tapes)
    evictions = seq_ops._STACK_SCRATCH.evictions, seq_ops._PERSIST_WS.evictions
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    ops.FRAME_PYRAMID_FUSED = True
    seq_ops.check_persist_errors()
    finite = all(np.isfinite(v) for v in losses_.values())
    resident = lambda table: sum(int(ent[0].numel()) for ent in table.values())
    row = dict(leg=leg, plugin=plugin, B=B, V=V, input="uint8 [B,300,1152]", flags=fl, steps=steps, warmup=warmup, repeats=repeats,
               losses_after_warmup=losses_, native_stack_calls_per_step=len(step_tapes),
               native_stacks_F_D_H=[list(d) for _, _, d in step_tapes],
               tape_bytes_per_step=sum(t for t, _, _ in step_tapes), stack_scratch_bytes_of_a_step=sum(s for _, s, _ in step_tapes),
               tape_bytes_per_native_stack=[t for t, _, _ in step_tapes], scratch_bytes_per_native_stack=[s for _, s, _ in step_tapes],
               resident_stack_scratch_buffers=len(seq_ops._STACK_SCRATCH), resident_stack_scratch_bytes=resident(seq_ops._STACK_SCRATCH),
               resident_persist_workspaces=len(seq_ops._PERSIST_WS), resident_persist_workspace_bytes=resident(seq_ops._PERSIST_WS),
               stack_scratch_max=seq_ops._STACK_SCRATCH_MAX, persist_ws_max=seq_ops._PERSIST_WS_MAX,
               evictions_during_the_timed_steps=[seq_ops._STACK_SCRATCH.evictions - evictions[0], seq_ops._PERSIST_WS.evictions - evictions[1]],
               max_memory_allocated_bytes=int(torch.cuda.max_memory_allocated()),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    if "composed" in ms:                                                 # this row states no verdict: the pyramid leg's summary decides the default
        against = steplib.fused_against_composed(ms)
        row.update((k, against[k]) for k in ("fused_minus_composed_ms", "spread_between_repeats_ms"))
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def summarise(rows):
    return steplib.verdict_after(rows, "pyramid", "leg_run", "the kernel is the default only if this holds over two runs of the leg")


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--pyramid_iters", type=int, default=50)
    return ap


def main():
    a = steplib.parse_args(parser(), ["pyramid"] + list(LEGS))
    if a.child == "pyramid":
        return pyramid(a.pyramid_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["pyramid", "pyramid"] + list(LEGS)                 # the pyramid leg twice: its verdict wants two runs of the leg
    return steplib.drive(__file__, steplib.numbered(legs, "pyramid", "leg_run"), steplib.child_args(a, "repeats", "pyramid_iters"),
                         a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
