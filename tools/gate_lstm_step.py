"""The scalar-gate LSTM layer (seq_ops.gate_lstm_layer, csrc/gate_cell.hip) and LstmGateModel at the training scripts' shapes.
`op` (timed first, and run twice by the driver: two runs of the leg): forward + backward of ONE layer through autograd, the step kernels
against the composed torch form (the YT8M_GATE_LSTM_FUSED=0 form), at [F, B, D, H] = [300, 128, 1152, 1024] and [300, 32, 1152, 1024] on
the reader's bytes and [300, 128, 1024, 1024] on floats (a second layer): hip events around back-to-back calls, the two forms alternating
inside every repeat, the spread over the repeats recorded, values and gradients compared.  Each row also times the two entry points alone
(yt8m_gate_lstm_layer_fwd / _bwd on given hoisted inputs: recurrent product + step kernel, per step) and the recurrent product alone
(the same grouped GEMM issued F times), so the step kernels' own share is their difference.  The driver adds an `op_summary` row: whether
the kernels' median was below the composed one at every shape in both runs of the leg -- what decides the default of the switch.
`step`: whole training steps (fp32, clip + Adam, learning rate 0) of LstmGateModel (--moe_num_mixtures=8) with the switch on and off and
of LstmMemoryModel with one layer of 1024 cells, in ONE process and in turn inside every repeat, on raw uint8 frames [128, 300, 1152].
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/gate_lstm_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op step"""
import json
import os
import sys

import steplib

V, B, F = steplib.V, 128, 300
OP_SHAPES = ((300, 128, 1152, 1024, True), (300, 32, 1152, 1024, True), (300, 128, 1024, 1024, False))     # F, B, D, H, bytes?
STEP_FLAGS = dict(lstm_cells="1024", lstm_layers=1, moe_num_mixtures=8)


def op(iters, repeats):
    import ctypes
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.ops import _p, _stream
    lib = L.lib()
    switch = os.environ.get("YT8M_GATE_LSTM_PACKED_BWD")                 # what the autograd rows run under
    for F_, B_, D, H, u8 in OP_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(F_ + B_ + D)
        nf = torch.randint(1, F_ + 1, (B_,), device=dev, generator=gen, dtype=torch.int32)
        nf[0], nf[1] = F_, 1
        if u8:
            q = torch.randint(0, 256, (B_, F_, D), device=dev, generator=gen, dtype=torch.uint8)
            assert seq_ops.u8_hoisted_supported(q)
        else:
            x = torch.tanh(torch.randn((F_, B_, D), device=dev, generator=gen))              # a lower layer's hidden outputs, |h| < 1
        draw = lambda *s: torch.randn(s, device=dev, generator=gen) * 0.03
        params = [draw(D, 2 * H), draw(2 * H) + 0.1, draw(D, 2), draw(2) + 0.5, draw(H, 2 * H), draw(2, H)]
        go, gc = torch.randn((F_, B_, H), device=dev, generator=gen), torch.randn((B_, H), device=dev, generator=gen)

        def run(fused):
            seq_ops.GATE_LSTM_FUSED = fused
            leaves = [t.detach().requires_grad_(True) for t in params]
            frames = seq_ops.U8FrameImages(q, nf) if u8 else x                               # (made per call, as a training step does)
            out, c_last = seq_ops.gate_lstm_layer(frames, *leaves, nf)
            ((out * go).sum() + (c_last * gc).sum()).backward()
            return out.detach(), c_last.detach(), [t.grad for t in leaves]

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        assert lib.yt8m_gate_lstm_supported(B_, H)
        us = steplib.alternate(forms, iters, repeats)
        (of, cf, gf), (oc, cc, gcmp) = forms["fused"](), forms["composed"]()
        seq_ops.GATE_LSTM_FUSED = True
        # the entry points alone on given hoisted inputs, and the recurrent product alone
        zv0, zs0 = torch.randn((F_, B_, 2 * H), device=dev, generator=gen) * 0.5, torch.randn((F_, B_, 2), device=dev, generator=gen) * 0.5
        zv, zs = zv0.clone(), zs0.clone()
        hs, cs = torch.zeros((F_ + 1, B_, H), device=dev), torch.zeros((F_ + 1, B_, H), device=dev)
        c_last, dzv, dzs = torch.empty((B_, H), device=dev), torch.empty((F_, B_, 2 * H), device=dev), torch.empty((F_, B_, 2), device=dev)
        work = torch.empty((4, B_, H), device=dev)
        ws = ops._workspace(dev)
        Uv, Us = params[4], params[5]

        def fwd():
            zv.copy_(zv0)
            zs.copy_(zs0)
            L.check(lib.yt8m_gate_lstm_layer_fwd(_p(zv), _p(zs), 2, _p(Uv), 2 * H, _p(Us), _p(hs), _p(cs), _p(c_last), _p(nf), F_, B_, H,
                                                 _p(ws), ws.numel() * 4, _stream()))

        def bwd(packed):
            os.environ["YT8M_GATE_LSTM_PACKED_BWD"] = packed             # the library reads it at every call
            L.check(lib.yt8m_gate_lstm_layer_bwd(_p(zv), _p(zs), 2, _p(Uv), 2 * H, _p(Us), _p(hs), _p(cs), _p(go), _p(gc), _p(dzv), _p(dzs),
                                                 _p(work), _p(nf), F_, B_, H, _p(ws), ws.numel() * 4, _stream()))

        def copies():
            zv.copy_(zv0)
            zs.copy_(zs0)

        pf = L.GemmProblem(B_, 2 * H, H, hs.data_ptr(), H, Uv.data_ptr(), 2 * H, dzv.data_ptr(), 2 * H, None, 1.0)
        pb = L.GemmProblem(B_, H, 2 * H, dzv.data_ptr(), 2 * H, Uv.data_ptr(), 2 * H, work.data_ptr(), H, None, 1.0)

        def products(transB, pr):
            arr = (L.GemmProblem * 1)(pr)
            for _ in range(F_):
                L.check(lib.yt8m_gemm_f32_grouped(0, transB, 1, arr, _p(ws), ws.numel() * 4, _stream()))

        alone = steplib.alternate({"fwd": fwd, "copies": copies, "bwd": lambda: bwd("0"), "bwd_packed": lambda: bwd("1"),
                                   "fwd_product": lambda: products(0, pf), "bwd_product": lambda: products(1, pb)}, iters, repeats)
        if switch is None:
            del os.environ["YT8M_GATE_LSTM_PACKED_BWD"]
        else:
            os.environ["YT8M_GATE_LSTM_PACKED_BWD"] = switch
        m = {k: steplib.median(v) for k, v in alone.items()}
        fwd_step, bwd_step = (m["fwd"] - m["copies"]) / F_, m["bwd"] / F_
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        print(json.dumps(dict(
            leg="op", F=F_, B=B_, D=D, H=H, input="uint8 frames" if u8 else "float frames", what="forward + backward of one layer through autograd",
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            fwd_us_per_step=round(fwd_step, 2), fwd_product_us_per_step=round(m["fwd_product"] / F_, 2),
            fwd_kernel_us_per_step_by_difference=round(fwd_step - m["fwd_product"] / F_, 2),
            bwd_us_per_step=round(bwd_step, 2), bwd_product_us_per_step=round(m["bwd_product"] / F_, 2),
            bwd_kernel_us_per_step_by_difference=round(bwd_step - m["bwd_product"] / F_, 2),
            bwd_packed_us_per_step=round(m["bwd_packed"] / F_, 2), packed_bwd_below_gemm_bwd=bool(m["bwd_packed"] < m["bwd"]),
            packed_bwd_switch=switch or "unset (the library's default)",
            out_diff_fused_composed=float((of - oc).abs().max()), c_last_diff_fused_composed=float((cf - cc).abs().max()),
            grad_diff_fused_composed_rel_to_max=max(rel(a, b) for a, b in zip(gf, gcmp)),
            repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                    % iters)), flush=True)
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
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    graphs = {name: train.build_graph(getattr(flm, name)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)
              for name in ("LstmGateModel", "LstmMemoryModel")}
    forms = {"fused": ("LstmGateModel", True), "composed": ("LstmGateModel", False), "baseline": ("LstmMemoryModel", True)}

    def run(form, n):
        which, fused = forms[form]
        seq_ops.GATE_LSTM_FUSED = fused
        for _ in range(n):
            out = graphs[which].step(*batch)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    seq_ops.GATE_LSTM_FUSED = True
    row = dict(leg="step", plugin="LstmGateModel", baseline="LstmMemoryModel", B=B, V=V, input="uint8 [B,300,1152]", flags=STEP_FLAGS, steps=steps,
               warmup=warmup, repeats=repeats, losses_after_warmup=losses_, calls=dict(seq_ops.GATE_LSTM_CALLS),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row.update(steplib.fused_against_composed(ms))
    row["fused_below_composed"] = bool(steplib.median(ms["fused"]) < steplib.median(ms["composed"]))
    row["plugin_over_baseline"] = round(steplib.median(ms["fused"]) / steplib.median(ms["baseline"]), 3)
    print(json.dumps(row), flush=True)
    return 0 if all(np.isfinite(v) for v in losses_.values()) else 1


def summarise(rows):
    return steplib.verdict_after(rows, "op", "leg_repeat", "the kernels are the default only if this holds over two runs of the leg")


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=3, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=3)
    return ap


def main():
    a = steplib.parse_args(parser(), ["op", "step"])
    if a.child == "op":
        return op(a.op_iters, a.repeats)
    if a.child == "step":
        return step(a.steps, a.warmup, a.repeats)
    legs = a.legs or ["op", "op", "step"]                                # the op leg twice: its verdict wants two runs of the leg
    return steplib.drive(__file__, steplib.numbered(legs, "op", "leg_repeat"), steplib.child_args(a, "repeats", "op_iters"), a.timeout, a.out,
                         summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
