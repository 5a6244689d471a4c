"""The fused memory link (ops.memory_link, csrc/memory_link.hip) and the three multi-LSTM plugins at their training scripts' shapes.
`link` (timed first, and run twice by the driver: two repeats of the leg): forward + backward of ops.memory_link through autograd, the
fused kernel against the composed torch.cat -> l2_normalize (the YT8M_MEMORY_LINK_FUSED=0 form), with and without normalize, at
[128; 1024], [128; 1024, 1024] and [384; 1024, 1024]: hip events around back-to-back calls, the two forms alternating inside every
repeat, the spread over the repeats recorded, values and gradients compared.  The driver adds a `link_summary` row: whether the fused
median was below the composed one at every shape in both repeats of the leg -- what decides the default of the switch.
Step legs (one per plugin): whole training steps (fp32, clip + Adam, learning rate 0) of the plugin with the switch on, with it off, and
of the single-stack model it is measured against, in ONE process and in turn inside every repeat, on raw uint8 frames [128, 300, 1152].
The row states the plugin's step over N x the baseline's (N = the number of stacks of the plugin per stack of the baseline).
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/multilstm_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `link`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, F, D = 4716, 128, 300, 1152
CHAIN = dict(multitask=True, label_loss="MultiTaskCrossEntropyLoss", support_loss_percent=0.05)
# leg: (plugin, baseline, stacks of the plugin per stack of the baseline, distillation input?, flags)
LEGS = {
    "chain": ("LstmMemoryDeepChainModel", "LstmMemoryModel", 2, False,
              dict(lstm_cells="1024", lstm_layers=2, deep_chain_layers=1, deep_chain_relu_cells=200, moe_num_mixtures=4, support_type="label",
                   **CHAIN)),
    "distill": ("DistillchainLstmMemoryDeepCombineChainModel", "LstmMemoryModel", 3, True,
                dict(lstm_cells="1024", lstm_layers=1, deep_chain_layers=2, deep_chain_relu_cells=256, distillchain_relu_cells=256,
                     moe_num_mixtures=4, support_type="label,label", **CHAIN)),
    "parallel": ("LstmParallelMemoryModel", "LstmParallelFinaloutputModel", 1, False,
                 dict(lstm_cells="1024,128", feature_sizes="1024,128", lstm_layers=2, moe_num_mixtures=4)),
}
LINK_SHAPES = ((128, (1024,)), (128, (1024, 1024)), (384, (1024, 1024)))


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


def link(iters, repeats):
    import torch
    dev = _setup()
    import yt8m_amd.ops as ops
    for rows, widths in LINK_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(rows + sum(widths))
        parts = [torch.randn((rows, w), device=dev, generator=gen) for w in widths]
        coef = torch.randn((rows, sum(widths)), device=dev, generator=gen)
        for normalize in (True, False):
            def run(fused):
                ops.MEMORY_LINK_FUSED = fused
                leaves = [t.detach().requires_grad_(True) for t in parts]
                y = ops.memory_link(leaves, normalize)
                y.backward(coef)
                return y.detach(), torch.cat([t.grad for t in leaves], 1)

            forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
            us = {k: [] for k in forms}
            for f in forms.values():                                         # warm-up: every form for as long as it is timed
                _events_us(f, iters)
            for _ in range(repeats):                                         # alternating: both forms see the same machine
                for k, f in forms.items():
                    us[k].append(_events_us(f, iters))
            (yf, df), (yc, dc) = forms["fused"](), forms["composed"]()
            ops.MEMORY_LINK_FUSED = True
            f_, c_ = us["fused"], us["composed"]
            n = len(widths)
            print(json.dumps(dict(
                leg="link", rows=rows, widths=list(widths), normalize=normalize, what="forward + backward through autograd",
                launches_fused=2, launches_composed=(1 if n > 1 else 0) + n + (2 if normalize else 0),
                fused_us=round(_median(f_), 2), fused_us_min=round(min(f_), 2), fused_us_max=round(max(f_), 2),
                composed_us=round(_median(c_), 2), composed_us_min=round(min(c_), 2), composed_us_max=round(max(c_), 2),
                composed_over_fused=round(_median(c_) / _median(f_), 2), fused_below_composed=bool(_median(f_) < _median(c_)),
                y_diff_fused_composed=float((yf - yc).abs().max()), grad_diff_fused_composed_rel_to_max=float((df - dc).abs().max() / dc.abs().max()),
                repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                        % iters)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = _setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    import yt8m_amd.ops as ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    plugin, baseline, n_stacks, distill_in, fl = LEGS[leg]
    FLAGS.reset()
    FLAGS.batch_size = B
    if distill_in:
        FLAGS.distillation_features = FLAGS.distillation_as_input = True
    for k, v in fl.items():
        setattr(FLAGS, k, v)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randint(0, 256, (B, F, D), device=dev, generator=gen, dtype=torch.uint8)
    nf = torch.randint(1, F + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
    nf[0], nf[1] = F, 1
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    y[:, 0] = True
    batch = (x, y, nf)
    distill = torch.rand((B, V), device=dev, generator=gen) * 0.05
    # learning rate 0 (the step does the same work): the steps repeat one random batch.  The baseline has no support predictions: it
    # takes the plain loss, whatever the leg's flags say
    graphs = {"plugin": train.build_graph(getattr(flm, plugin)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                          base_learning_rate=0.0),
              "baseline": train.build_graph(getattr(flm, baseline)(), label_loss_fn=losses.CrossEntropyLoss(), multitask=False, batch_size=B,
                                            graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)}
    kw = dict(distill_labels_batch=distill) if distill_in else {}
    forms = {"fused": ("plugin", True, kw), "composed": ("plugin", False, kw), "baseline": ("baseline", True, {})}

    def run(form, n):
        which, fused, kw_ = forms[form]
        ops.MEMORY_LINK_FUSED = fused
        for _ in range(n):
            out = graphs[which].step(*batch, **kw_)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    ms = {k: [] for k in forms}
    for _ in range(repeats):                                             # in turn: every form sees the same machine
        for k in forms:
            t0 = time.perf_counter()
            run(k, steps)
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    ops.MEMORY_LINK_FUSED = True
    finite = all(np.isfinite(v) for v in losses_.values())
    row = dict(leg=leg, plugin=plugin, baseline=baseline, B=B, V=V, input="uint8 [B,300,1152]", flags=fl, steps=steps, warmup=warmup,
               repeats=repeats, losses_after_warmup=losses_, stacks_per_baseline_stack=n_stacks,
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row["%s_ms_per_step" % k] = round(_median(v), 3)
        row["%s_ms_min" % k], row["%s_ms_max" % k] = round(min(v), 3), round(max(v), 3)
    spread = max(max(ms["fused"]) - min(ms["fused"]), max(ms["composed"]) - min(ms["composed"]))
    row["fused_minus_composed_ms"] = round(_median(ms["fused"]) - _median(ms["composed"]), 3)
    row["spread_between_repeats_ms"] = round(spread, 3)
    row["fused_within_spread_of_composed"] = bool(_median(ms["fused"]) - _median(ms["composed"]) <= spread)
    row["plugin_over_n_baselines"] = round(_median(ms["fused"]) / (n_stacks * _median(ms["baseline"])), 3)
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--link_iters", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    if a.child == "link":
        return link(a.link_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    rows = []
    link_runs = 0
    for leg in a.legs or ["link", "link"] + list(LEGS):                  # the link leg twice: its verdict wants two repeats of the leg
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--link_iters", str(a.link_iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print("leg %s failed with exit status %d: stopping" % (leg, r.returncode), flush=True)
            return r.returncode or 1
        for ln in lines:
            row = json.loads(ln)
            if leg == "link":
                row["leg_repeat"] = link_runs
            rows.append(row)
            print(json.dumps(row), flush=True)
        if leg == "link":
            link_runs += 1
            timed = [r_ for r_ in rows if r_.get("leg") == "link"]
            summary = dict(leg="link_summary", leg_repeats=link_runs, rows=len(timed),
                           fused_below_composed_everywhere=bool(all(r_["fused_below_composed"] for r_ in timed)),
                           rule="fused is the default only if this holds over two repeats of the leg")
            rows = [r_ for r_ in rows if r_.get("leg") != "link_summary"] + [summary]
            print(json.dumps(summary), flush=True)
        if a.out:                                                        # after every leg: a later leg's failure keeps the earlier rows
            with open(a.out, "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
