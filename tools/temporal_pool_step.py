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
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, F, D = 4716, 128, 300, 1152
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


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.load_package()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _events_us(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _median(v):
    return sorted(v)[len(v) // 2]


def pyramid(iters, repeats):
    import torch
    dev = _setup()
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
        us = {k: [] for k in forms}
        for fn in forms.values():                                            # warm-up: every form for as long as it is timed
            _events_us(fn, iters)
        for _ in range(repeats):                                             # alternating: both forms see the same machine
            for k, fn in forms.items():
                us[k].append(_events_us(fn, iters))
        (pf, nf_f), (pc, nf_c) = forms["fused"](), forms["composed"]()
        ops.FRAME_PYRAMID_FUSED = True
        diff = max(float((a - c).abs().max()) for ra, rc in zip(pf, pc) for a, c in zip(ra, rc))
        same_frames = all(bool(torch.equal(a, c)) for a, c in zip(nf_f, nf_c))
        out_bytes = sum(4 * (f >> (l + 1)) * b * sum(widths) for l in range(levels))
        f_, c_ = us["fused"], us["composed"]
        n = len(widths)
        print(json.dumps(dict(
            leg="pyramid", B=b, F=f, widths=list(widths), levels=levels, launches_fused=1, launches_composed=levels * (1 + 3 * n),
            bytes_read_once=b * f * sum(widths), bytes_written=out_bytes,
            fused_us=round(_median(f_), 2), fused_us_min=round(min(f_), 2), fused_us_max=round(max(f_), 2),
            composed_us=round(_median(c_), 2), composed_us_min=round(min(c_), 2), composed_us_max=round(max(c_), 2),
            fused_tb_per_s=round((b * f * sum(widths) + out_bytes) / _median(f_) * 1e-6, 3),
            composed_over_fused=round(_median(c_) / _median(f_), 2), fused_below_composed=bool(_median(f_) < _median(c_)),
            y_diff_fused_composed=diff, num_frames_equal=same_frames, repeats=repeats,
            timing="hip events over %d back-to-back calls (torch allocations included), median of the repeats" % iters)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = _setup()
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
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randint(0, 256, (B, F, D), device=dev, generator=gen, dtype=torch.uint8)
    nf = torch.randint(1, F + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
    nf[0], nf[1] = F, 1
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    y[:, 0] = True
    batch = (x, y, nf)
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
    ms = {k: [] for k in forms}
    for _ in range(repeats):                                             # in turn: every form sees the same machine
        for k in forms:
            t0 = time.perf_counter()
            run(k, steps)
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
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
        row["%s_ms_per_step" % k] = round(_median(v), 3)
        row["%s_ms_min" % k], row["%s_ms_max" % k] = round(min(v), 3), round(max(v), 3)
    if "composed" in ms:
        spread = max(max(ms["fused"]) - min(ms["fused"]), max(ms["composed"]) - min(ms["composed"]))
        row["fused_minus_composed_ms"] = round(_median(ms["fused"]) - _median(ms["composed"]), 3)
        row["spread_between_repeats_ms"] = round(spread, 3)
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--pyramid_iters", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    if a.child == "pyramid":
        return pyramid(a.pyramid_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    rows = []
    pyramid_runs = 0
    for leg in a.legs or ["pyramid", "pyramid"] + list(LEGS):            # the pyramid leg twice: its verdict wants two runs of the leg
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--pyramid_iters", str(a.pyramid_iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print("leg %s failed with exit status %d: stopping" % (leg, r.returncode), flush=True)
            return r.returncode or 1
        for ln in lines:
            row = json.loads(ln)
            if leg == "pyramid":
                row["leg_run"] = pyramid_runs
            rows.append(row)
            print(json.dumps(row), flush=True)
        if leg == "pyramid":
            pyramid_runs += 1
            timed = [r_ for r_ in rows if r_.get("leg") == "pyramid"]
            summary = dict(leg="pyramid_summary", leg_runs=pyramid_runs, rows=len(timed),
                           fused_below_composed_everywhere=bool(all(r_["fused_below_composed"] for r_ in timed)),
                           rule="the kernel is the default only if this holds over two runs of the leg")
            rows = [r_ for r_ in rows if r_.get("leg") != "pyramid_summary"] + [summary]
            print(json.dumps(summary), flush=True)
        if a.out:                                                        # after every leg: a later leg's failure keeps the earlier rows
            with open(a.out, "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
