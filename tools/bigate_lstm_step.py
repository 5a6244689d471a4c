"""The scalar-gate pair of LstmBigluModel (seq_ops.bigate_lstm_layer, the frame-order form of csrc/gate_cell.hip) and the model at the training scripts' shapes.
`op` (timed first, and run twice by the driver: two runs of the leg): forward + backward of the op through autograd in its three forms
-- the frame-order kernels, the same kernels over reversed copies (YT8M_BIGATE_LSTM_REVERSED=1) and the composed torch loops (a few
iterations only) -- at [F, B, D, H] = [300, 128, 1152, 1024] and [300, 32, 1152, 1024] on the reader's bytes and [300, 128, 1024, 1024] on
floats: hip events around back-to-back calls, the two kernel forms alternating inside every repeat, the spread over the repeats
recorded, values and gradients compared.  Each row also times ONE pass alone on given hoisted inputs, per step: the frame-order entry
points with either row map beside the step-order ones of the same file (yt8m_gate_lstm_layer_fwd / _bwd).  The driver adds an `op_summary` row: whether the frame-order median was below the
reversed-copies one at every shape in both runs of the leg -- what decides the default of the switch.
`step`: whole training steps (fp32, clip + Adam, learning rate 0) of LstmBigluModel (--moe_num_mixtures=8) in both kernel forms and of
LstmGateModel and LstmGlu2Model, in ONE process and in turn inside every repeat, on raw uint8 frames [128, 300, 1152].
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/bigate_lstm_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op step"""
import json
import sys

import steplib

V, B, F = steplib.V, 128, 300
OP_SHAPES = ((300, 128, 1152, 1024, True), (300, 32, 1152, 1024, True), (300, 128, 1024, 1024, False))     # F, B, D, H, bytes?
STEP_FLAGS = dict(lstm_cells="1024", lstm_layers=1, moe_num_mixtures=8)
RULE = "the frame-order form is the default only if this holds over two runs of the leg"


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.ops import _p, _stream
    lib = L.lib()
    default = seq_ops.BIGATE_LSTM_REVERSED                                                   # the package's default form, put back per shape
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
        # Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2
        params = [draw(D, 4 * H), draw(4 * H) + 0.1, draw(D, 4), draw(4) + 0.1, draw(H, 2 * H), draw(2, H), draw(H, 2 * H), draw(H, 2),
                  draw(H, 2 * H), draw(2, H)]
        gos = [torch.randn((F_, B_, H), device=dev, generator=gen), torch.randn((F_, B_, H), device=dev, generator=gen),
               torch.randn((B_, H), device=dev, generator=gen), torch.randn((B_, H), device=dev, generator=gen)]

        def run(fused, rev):
            seq_ops.BIGATE_LSTM_FUSED, seq_ops.BIGATE_LSTM_REVERSED = fused, rev
            leaves = [t.detach().requires_grad_(True) for t in params]
            frames = seq_ops.U8FrameImages(q, nf) if u8 else x                               # (made per call, as a training step does)
            outs = seq_ops.bigate_lstm_layer(frames, *leaves, nf)
            sum((o * g).sum() for o, g in zip(outs, gos)).backward()
            return [o.detach() for o in outs], [t.grad for t in leaves]

        forms = {"frame_order": lambda: run(True, False), "reversed_copies": lambda: run(True, True)}
        assert lib.yt8m_gate_lstm_frames_supported(B_, H)
        before = dict(seq_ops.BIGATE_LSTM_CALLS)
        us = steplib.alternate(forms, iters, repeats)
        us.update(steplib.alternate({"composed": lambda: run(False, False)}, 1, 1))           # the torch loops: one warm-up, one timed call
        assert all(seq_ops.BIGATE_LSTM_CALLS[k] > before[k] for k in before), "every form must have run"
        (of, gf), (orv, grv), (oc, gc) = run(True, False), run(True, True), run(False, False)
        seq_ops.BIGATE_LSTM_FUSED, seq_ops.BIGATE_LSTM_REVERSED = True, default
        # one pass alone on given hoisted inputs: the frame-order entry points with either row map beside the step-order ones of
        # csrc/gate_cell.hip (the same cell; their product accumulates in place, theirs needs no scratch row and no hprev)
        new = lambda *s: torch.empty(s, device=dev)
        zv0, zs0 = torch.randn((F_, B_, 2 * H), device=dev, generator=gen) * 0.5, torch.randn((F_, B_, 2), device=dev, generator=gen) * 0.5
        zv, zs, yb, hp, c_last, dzv, dzs = zv0.clone(), zs0.clone(), new(F_, B_, H), new(F_, B_, H), new(B_, H), new(F_, B_, 2 * H), new(F_, B_, 2)
        hs, cs = torch.zeros((F_ + 1, B_, H), device=dev), torch.zeros((F_ + 1, B_, H), device=dev)
        work, ws = new(6, B_, H), ops._workspace(dev)
        Uv, Us, tail = params[4], params[5], (F_, B_, H, _p(ws), ws.numel() * 4, _stream())

        def copies():
            zv.copy_(zv0)
            zs.copy_(zs0)

        def frames_fwd(rev):
            copies()
            L.check(lib.yt8m_gate_lstm_frames_fwd(_p(zv), 2 * H, _p(zs), 2, _p(Uv), 2 * H, _p(Us), _p(yb), _p(hp), _p(cs), _p(c_last), _p(work),
                                                  _p(nf), rev, *tail))

        def frames_bwd(rev):
            L.check(lib.yt8m_gate_lstm_frames_bwd(_p(zv), 2 * H, _p(zs), 2, _p(Uv), 2 * H, _p(Us), _p(cs), _p(gos[0]), _p(gos[2]), _p(dzv), 2 * H,
                                                  _p(dzs), 2, _p(work), _p(nf), rev, *tail))

        def layer_fwd():
            copies()
            L.check(lib.yt8m_gate_lstm_layer_fwd(_p(zv), _p(zs), 2, _p(Uv), 2 * H, _p(Us), _p(hs), _p(cs), _p(c_last), _p(nf), *tail))

        def layer_bwd():
            L.check(lib.yt8m_gate_lstm_layer_bwd(_p(zv), _p(zs), 2, _p(Uv), 2 * H, _p(Us), _p(hs), _p(cs), _p(gos[0]), _p(gos[2]), _p(dzv), _p(dzs),
                                                 _p(work), _p(nf), *tail))

        alone = steplib.alternate({"copies": copies, "frames_fwd_identity": lambda: frames_fwd(0), "frames_fwd_reverse": lambda: frames_fwd(1),
                                   "layer_fwd": layer_fwd, "frames_bwd_identity": lambda: frames_bwd(0), "frames_bwd_reverse": lambda: frames_bwd(1),
                                   "layer_bwd": layer_bwd}, iters, repeats)
        m = {k: steplib.median(v) for k, v in alone.items()}
        per_step = {k + "_us_per_step": round((m[k] - (m["copies"] if "fwd" in k else 0.0)) / F_, 2) for k in m if k != "copies"}
        f_, r_ =steplib.median(us["frame_order"]), steplib.median(us["reversed_copies"])
        spread = max(max(us[k]) - min(us[k]) for k in ("frame_order", "reversed_copies"))
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        print(json.dumps(dict(
            leg="op", F=F_, B=B_, D=D, H=H, input="uint8 frames" if u8 else "float frames",
            what="forward + backward of both passes through autograd, a gradient on all four returns",
            **steplib.spread_fields("frame_order", us["frame_order"], "us"), **steplib.spread_fields("reversed_copies", us["reversed_copies"], "us"),
            composed_us=round(us["composed"][0], 2), composed_over_frame_order=round(us["composed"][0] / f_, 2),
            frame_order_minus_reversed_copies_us=round(f_ - r_, 2), spread_between_repeats_us=round(spread, 2),
            difference_within_spread=bool(abs(f_ - r_) <= spread), frame_order_below_reversed_copies=bool(f_ < r_), **per_step,
            out_diff_frame_order_reversed_copies=max(float((a - b).abs().max()) for a, b in zip(of, orv)),
            grad_diff_frame_order_reversed_copies_rel_to_max=max(rel(a, b) for a, b in zip(gf, grv)),
            out_diff_frame_order_composed=max(float((a - b).abs().max()) for a, b in zip(of, oc)),
            grad_diff_frame_order_composed_rel_to_max=max(rel(a, b) for a, b in zip(gf, gc)),
            repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats; "
                                    "composed: one call" % iters)), flush=True)
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
              for name in ("LstmBigluModel", "LstmGateModel", "LstmGlu2Model")}
    forms = {"frame_order": ("LstmBigluModel", False), "reversed_copies": ("LstmBigluModel", True), "gate": ("LstmGateModel", False),
             "glu2": ("LstmGlu2Model", False)}
    default = seq_ops.BIGATE_LSTM_REVERSED

    def run(form, n):
        which, seq_ops.BIGATE_LSTM_REVERSED = forms[form]
        for _ in range(n):
            out = graphs[which].step(*batch)
        torch.cuda.synchronize()
        return float(out["loss"])

    losses_ = {k: run(k, warmup) for k in forms}
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    seq_ops.BIGATE_LSTM_REVERSED = default
    row = dict(leg="step", plugin="LstmBigluModel", beside=["LstmGateModel", "LstmGlu2Model"], B=B, V=V, input="uint8 [B,300,1152]", flags=STEP_FLAGS,
               steps=steps, warmup=warmup, repeats=repeats, losses_after_warmup=losses_, calls=dict(seq_ops.BIGATE_LSTM_CALLS),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    med = {k: steplib.median(v) for k, v in ms.items()}
    spread = max(max(ms[k]) - min(ms[k]) for k in ("frame_order", "reversed_copies"))
    row.update(frame_order_minus_reversed_copies_ms=round(med["frame_order"] - med["reversed_copies"], 3), spread_between_repeats_ms=round(spread, 3),
               difference_within_spread=bool(abs(med["frame_order"] - med["reversed_copies"]) <= spread),
               frame_order_below_reversed_copies=bool(med["frame_order"] < med["reversed_copies"]),
               biglu_over_gate=round(med["frame_order"] / med["gate"], 3), biglu_over_glu2=round(med["frame_order"] / med["glu2"], 3))
    print(json.dumps(row), flush=True)
    return 0 if all(np.isfinite(v) for v in losses_.values()) else 1


def summarise(rows):
    """The rows with an `op_summary` row after the last run of the op leg: whether the frame-order median was below the
    reversed-copies one in every timed row of every run so far."""
    last = max((i for i, r in enumerate(rows) if "leg_repeat" in r), default=None)
    if last is None:
        return rows
    timed = [r for r in rows if r.get("leg") == "op"]
    summary = {"leg": "op_summary", "leg_repeats": rows[last]["leg_repeat"] + 1, "rows": len(timed),
               "frame_order_below_reversed_copies_everywhere": bool(all(r["frame_order_below_reversed_copies"] for r in timed)), "rule": RULE}
    return rows[:last + 1] + [summary] + rows[last + 1:]


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
