"""LstmLayerModel's clip pass (seq_ops.lstm_clip_layer, csrc/lstm_wide.hip) at the training scripts' shapes.
`kernel`: the recurrence alone on given hoisted inputs, STEPS = 10 steps per call, at B' in {960, 3840} x H in {512, 1024}: forward on the
wide step kernel (yt8m_lstm_wide_steps_fwd; the first h image is part of the call, as in the op) / the packed step launcher
(yt8m_lstm_steps_fwd with Wp) / the grouped GEMM + gate kernel (Wp = NULL), backward on yt8m_lstm_steps_bwd with Wq / with Wq = NULL; us
per step, and for the wide kernel its f16 FLOP/s (three products) against 2.5 PF and its bytes per second (z in, gates out, c in and out, h
out, the h image out and in: 52 B' H bytes) against the 6.0-6.3 TB/s streaming rate.
`op`: forward + backward of lstm_clip_layer through autograd at [B, F, D, H, U1] = [128, 300, 1152, 1024, 10] and [32, 300, 1152, 1024, 10]
on bytes, [128, 300, 1024, 1024, 10] on floats and [128, 300, 1152, 1024, 30] on bytes, on every forward x backward route, the forms
alternating inside every repeat.  `step`: whole training steps (fp32, clip + Adam, learning rate 0) of LstmLayerModel (--moe_num_mixtures=8)
with the wide kernel on and off and of LstmMemoryModel with two layers of 1024 cells, in ONE process and in turn inside every repeat.
The driver runs every leg twice and adds summary rows: whether the wide forward's median was below BOTH existing forward routes at every
op shape in both runs (what decides the default of YT8M_LSTM_WIDE), the backward route with the lower median everywhere, and the smallest
B' of the kernel leg at which the wide kernel wins (WIDE_MIN_ROWS).  The opponent is always an existing route.
usage: python tools/lstm_layer_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: kernel op step"""
import json
import sys

import steplib

V, B, F = steplib.V, 128, 300
STEPS = 10
KERNEL_SHAPES = ((960, 512), (960, 1024), (3840, 512), (3840, 1024))                       # B', H
OP_SHAPES = ((128, 300, 1152, 1024, 10, True), (32, 300, 1152, 1024, 10, True), (128, 300, 1024, 1024, 10, False),
             (128, 300, 1152, 1024, 30, True))                                              # B, F, D, H, U1, bytes?
FWD_ROUTES, BWD_ROUTES = ("wide", "packed", "gemm"), ("packed", "gemm")
STEP_FLAGS = dict(lstm_cells="1024", lstm_layers=2, moe_num_mixtures=8)


def kernel(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    import yt8m_amd.ops as ops
    from yt8m_amd.ops import _p, _stream
    lib = L.lib()
    torch.cuda.set_stream(torch.cuda.Stream(dev))                      # not the legacy default stream: the packed chains replay as hipGraphs
    for Bp, H in KERNEL_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(Bp + H)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
        z0 = rnd(STEPS, Bp, 4 * H) * 0.5
        Wh = (torch.rand((H, 4 * H), device=dev, generator=gen) * 2 - 1) * (6.0 / (5 * H)) ** 0.5
        z = z0.clone()
        cs, hs = torch.zeros((STEPS + 1, Bp, H), device=dev), torch.zeros((STEPS + 1, Bp, H), device=dev)
        dz, work, dc = torch.empty_like(z), torch.empty((4, Bp, H), device=dev), rnd(Bp, H)
        npk = lib.yt8m_lstm_packed_floats(Bp, H)
        Wp, Wq = torch.empty(npk, device=dev), torch.empty(npk, device=dev)
        L.check(lib.yt8m_lstm_pack(_p(Wh), 4 * H, H, _p(Wp), _p(Wq), _stream()))
        need = lib.yt8m_lstm_wide_workspace_bytes(Bp, H)
        wws = torch.empty(need, dtype=torch.uint8, device=dev)
        L.check(lib.yt8m_lstm_wide_prepare(_p(Wh), 4 * H, Bp, H, _p(wws), need, _stream()))
        ws = ops._workspace(dev)

        def fwd(route):
            z.copy_(z0)
            if route == "wide":
                L.check(lib.yt8m_lstm_wide_steps_fwd(_p(z), _p(wws), need, _p(cs), _p(hs), None, 0, STEPS, Bp, H, 1.0, _stream()))
            else:
                L.check(lib.yt8m_lstm_steps_fwd(_p(z), _p(Wh), 4 * H, _p(Wp) if route == "packed" else None, _p(cs), _p(hs), None, None, 0,
                                                STEPS, Bp, H, 1.0, _p(ws), ws.numel() * 4, _stream()))

        def bwd(route):
            work.zero_()
            work[1].copy_(dc)
            L.check(lib.yt8m_lstm_steps_bwd(_p(z), _p(Wh), 4 * H, _p(Wq) if route == "packed" else None, _p(cs), None, _p(dz), _p(work), 0, None,
                                            0, STEPS, Bp, H, _p(ws), ws.numel() * 4, _stream()))

        forms = {"fwd_" + r: (lambda r=r: fwd(r)) for r in FWD_ROUTES}
        forms["copy"] = lambda: z.copy_(z0)
        us = steplib.alternate(forms, iters, repeats)
        ref = {}
        for r in FWD_ROUTES:                                           # the routes agree (and leave the tape of the last one for bwd)
            fwd(r)
            ref[r] = (z.clone(), cs.clone())
        diff = max(float((ref[r][k] - ref["gemm"][k]).abs().max()) for r in ("wide", "packed") for k in (0, 1))
        usb = steplib.alternate({"bwd_" + r: (lambda r=r: bwd(r)) for r in BWD_ROUTES}, iters, repeats)
        m = {k: steplib.median(v) for k, v in {**us, **usb}.items()}
        per = {k: round((m[k] - (m["copy"] if k.startswith("fwd") else 0.0)) / STEPS, 2) for k in m if k != "copy"}
        wide_s = per["fwd_wide"] * 1e-6
        flops, nbytes = 3 * 2.0 * Bp * H * 4 * H, 52.0 * Bp * H
        print(json.dumps(dict(
            leg="kernel", rows=Bp, H=H, steps_per_call=STEPS, us_per_step=per, wide_below_both=bool(per["fwd_wide"] < min(per["fwd_packed"], per["fwd_gemm"])),
            wide_f16_tflops=round(flops / wide_s / 1e12, 1), wide_share_of_2p5_pf=round(flops / wide_s / 2.5e15, 3),
            wide_tb_per_s=round(nbytes / wide_s / 1e12, 2), wide_share_of_6_tb_per_s=round(nbytes / wide_s / 6.0e12, 3),
            max_abs_diff_to_gemm_route=diff, repeats=repeats,
            timing="hip events over %d back-to-back calls of %d steps, median of the repeats, the z refill subtracted" % (iters, STEPS))), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def _route(seq_ops, fwd, bwd):
    seq_ops.WIDE, seq_ops.WIDE_MIN_ROWS = fwd == "wide", 1
    seq_ops.CLIP_FWD_EXISTING = fwd if fwd != "wide" else "packed"
    seq_ops.CLIP_BWD = bwd


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.seq_ops as seq_ops
    saved = seq_ops.WIDE, seq_ops.WIDE_MIN_ROWS, seq_ops.CLIP_FWD_EXISTING, seq_ops.CLIP_BWD
    for B_, F_, D, H, U1, u8 in OP_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(B_ + D + U1)
        nf = torch.randint(1, F_ + 1, (B_,), device=dev, generator=gen, dtype=torch.int32)
        nf[0], nf[1] = F_, 1
        if u8:
            x = torch.randint(0, 256, (B_, F_, D), device=dev, generator=gen, dtype=torch.uint8)
        else:
            x = torch.nn.functional.normalize(torch.randn((B_, F_, D), device=dev, generator=gen), dim=2)
        W = (torch.rand((D + H, 4 * H), device=dev, generator=gen) * 2 - 1) * (6.0 / (D + 5 * H)) ** 0.5
        b = torch.randn((4 * H,), device=dev, generator=gen) * 0.1
        go = torch.randn((F_ // U1, B_, H), device=dev, generator=gen)

        def run(fwd, bwd):
            _route(seq_ops, fwd, bwd)
            Wt, bt = W.detach().requires_grad_(True), b.detach().requires_grad_(True)
            out = seq_ops.lstm_clip_layer(x, nf, U1, Wt, bt)
            (out * go).sum().backward()
            return out.detach(), Wt.grad, bt.grad

        forms = {"%s+%s" % (f, g): (lambda f=f, g=g: run(f, g)) for f in FWD_ROUTES for g in BWD_ROUTES}
        us = steplib.alternate(forms, iters, repeats)
        m = {k: round(steplib.median(v), 1) for k, v in us.items()}
        base = forms["gemm+gemm"]()
        rel = lambda a, c: float((a - c).abs().max() / c.abs().max().clamp(min=1e-30))
        diffs = {k: max(rel(a, c) for a, c in zip(fn(), base)) for k, fn in forms.items() if k != "gemm+gemm"}
        wide_ok = all(m["wide+" + g] < min(m["packed+" + g], m["gemm+" + g]) for g in BWD_ROUTES)
        print(json.dumps(dict(
            leg="op", B=B_, F=F_, D=D, H=H, U1=U1, rows=B_ * (F_ // U1), input="uint8 frames" if u8 else "float frames",
            what="forward + backward of lstm_clip_layer through autograd, forward route + backward route", median_us=m,
            min_us={k: round(min(v), 1) for k, v in us.items()}, max_us={k: round(max(v), 1) for k, v in us.items()},
            wide_below_both_existing=bool(wide_ok), bwd_packed_below_gemm=bool(all(m[f + "+packed"] < m[f + "+gemm"] for f in FWD_ROUTES)),
            bwd_gemm_below_packed=bool(all(m[f + "+gemm"] < m[f + "+packed"] for f in FWD_ROUTES)),
            best_existing_fwd="packed" if sum(m["packed+" + g] for g in BWD_ROUTES) < sum(m["gemm+" + g] for g in BWD_ROUTES) else "gemm",
            max_rel_diff_to_gemm_routes=diffs, repeats=repeats,
            timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats" % iters)), flush=True)
    seq_ops.WIDE, seq_ops.WIDE_MIN_ROWS, seq_ops.CLIP_FWD_EXISTING, seq_ops.CLIP_BWD = saved
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def step(steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.batch_size = B
    for k, v in STEP_FLAGS.items():
        setattr(FLAGS, k, v)
    batch = steplib.random_batch(dev, B, F, "ends", first_label=True)[:3]
    graphs = {name: train.build_graph(getattr(flm, name)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)
              for name in ("LstmLayerModel", "LstmMemoryModel")}
    forms = {"wide": ("LstmLayerModel", True), "kernel_off": ("LstmLayerModel", False), "baseline": ("LstmMemoryModel", True)}
    default = seq_ops.WIDE

    def run(form, n):
        which, seq_ops.WIDE = forms[form]
        for _ in range(n):
            out = graphs[which].step(*batch)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    seq_ops.WIDE = default
    row = dict(leg="step", plugin="LstmLayerModel", baseline="LstmMemoryModel", B=B, V=V, input="uint8 [B,300,1152]", flags=STEP_FLAGS,
               lstm_length=FLAGS.lstm_length, steps=steps, warmup=warmup, repeats=repeats, losses_after_warmup=losses_,
               calls=dict(seq_ops.LSTM_CLIP_CALLS), wide_min_rows=seq_ops.WIDE_MIN_ROWS, existing_fwd=seq_ops.CLIP_FWD_EXISTING, bwd=seq_ops.CLIP_BWD,
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row["wide_below_kernel_off"] = bool(steplib.median(ms["wide"]) < steplib.median(ms["kernel_off"]))
    row["plugin_over_baseline"] = round(steplib.median(ms["wide"]) / steplib.median(ms["baseline"]), 3)
    print(json.dumps(row), flush=True)
    return 0 if all(np.isfinite(v) for v in losses_.values()) else 1


def summarise(rows):
    """The rows, then the verdicts over every run so far of the op and kernel legs."""
    ops_, kern = [r for r in rows if r.get("leg") == "op"], [r for r in rows if r.get("leg") == "kernel"]
    out = list(rows)
    if ops_:
        out.append(dict(leg="op_summary", rows=len(ops_), runs=1 + max(r.get("leg_repeat", 0) for r in ops_),
                        wide_below_both_existing_everywhere=bool(all(r["wide_below_both_existing"] for r in ops_)),
                        bwd_packed_below_gemm_everywhere=bool(all(r["bwd_packed_below_gemm"] for r in ops_)),
                        bwd_gemm_below_packed_everywhere=bool(all(r["bwd_gemm_below_packed"] for r in ops_)),
                        best_existing_fwd=sorted({r["best_existing_fwd"] for r in ops_}),
                        rule="the wide forward is the default only if its median is the lower one at every shape in both runs of the leg; "
                             "the backward route is the one with the lower median at every shape in both runs"))
    if kern:
        won = sorted({r["rows"] for r in kern if r["wide_below_both"]} - {r["rows"] for r in kern if not r["wide_below_both"]})
        out.append(dict(leg="kernel_summary", rows=len(kern), smallest_rows_where_wide_wins_at_every_H_in_every_run=won[0] if won else None))
    return out


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=3, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=2)
    return ap


def main():
    a = steplib.parse_args(parser(), ["kernel", "op", "step"])
    if a.child == "kernel":
        return kernel(a.op_iters, a.repeats)
    if a.child == "op":
        return op(a.op_iters, a.repeats)
    if a.child == "step":
        return step(a.steps, a.warmup, a.repeats)
    legs = a.legs or ["kernel", "op", "step", "kernel", "op", "step"]                     # every leg twice
    plan = [(leg, {"leg_repeat": legs[:i].count(leg)}) for i, leg in enumerate(legs)]
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "op_iters"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
