"""The sigmoid attention pooling (seq_ops.sigmoid_attention, csrc/sigmoid_attention.hip) and the three plugins on it at the training shape.
`op` (timed first, and run twice by the driver): forward + backward of seq_ops.sigmoid_attention through autograd, the kernels against the
composed form (the YT8M_SIGMOID_ATTENTION_FUSED=0 form: ops.linear on the [F B, Hs] view, torch sigmoid / mask / sum / divide, pool_tn on
a batch-major copy), at [F, B, Hs, Hv, A] = [300,128,1024,1024,1] (LstmAttentionLstmModel), [300,128,1024,0,1] (LstmAttentionModel),
[300,32,1024,1024,1] and [300,128,1024,0,4] (LstmMultiAttentionModel): hip events around back-to-back calls, the two forms alternating
inside every repeat, values and gradients compared.  Wa and ba are Variables of a graph, as in the plugins.  The driver adds an
`op_summary` row: whether the kernels' median was below the composed one at every shape in both runs -- what decides the default.
`kernels`: yt8m_sigattn_fwd and yt8m_sigattn_bwd alone through the C ABI at the same shapes, with the bytes each has to move computed from
the shapes (forward reads src and vals once; backward reads them once and writes as much) and the rate in TB/s.
`step`: whole training steps (cross entropy, clip, Adam; learning rate 0) of the three plugins at B = 128, F = 300 on the reader's bytes
with the switch on and off, LstmModel and LstmMemoryModel with the same cells in the same run for the scale.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/sigmoid_attention_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op kernels step"""
import ctypes
import json
import sys

import steplib

V = steplib.V
SHAPES = ((300, 128, 1024, 1024, 1), (300, 128, 1024, 0, 1), (300, 32, 1024, 1024, 1), (300, 128, 1024, 0, 4))
B, F = 128, 300
STEP_FLAGS = dict(lstm_cells="1024", lstm_layers=1, moe_num_mixtures=8, attention_size=4)      # W/eval_scripts/eval-att-lstm.sh's cells
PLUGINS = ("LstmAttentionLstmModel", "LstmAttentionModel", "LstmMultiAttentionModel")
SCALE = ("LstmModel", "LstmMemoryModel")


def _inputs(dev, shape, seed):
    import torch
    F_, B_, Hs, Hv, A = shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    nf = torch.randint(F_ // 2, F_ + 1, (B_,), device=dev, generator=gen, dtype=torch.int32)
    live = (torch.arange(F_, device=dev)[:, None] < nf[None, :]).to(torch.float32)[:, :, None]
    src = torch.tanh(torch.randn((F_, B_, Hs), device=dev, generator=gen)) * live                  # what a stack leaves: zero past num_frames
    vals = torch.tanh(torch.randn((F_, B_, Hv), device=dev, generator=gen)) * live if Hv else None
    G = torch.randn((B_, A, Hv), device=dev, generator=gen) if Hv else None
    E = torch.randn((B_, F_, A), device=dev, generator=gen)
    return nf, src, vals, G, E


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.variables import reset_default_graph, xavier_uniform, zeros
    for shape in SHAPES:
        F_, B_, Hs, Hv, A = shape
        nf, src, vals, G, E = _inputs(dev, shape, sum(shape))
        g = reset_default_graph(device=dev, seed=0)
        Wa = g.get_variable("fully_connected/weights", (Hs, A), xavier_uniform)
        ba = g.get_variable("fully_connected/biases", (A,), zeros)
        g.finalize()

        def run(fused):
            seq_ops.SIGMOID_ATTENTION_FUSED = fused
            g.begin_step()
            s = src.detach().requires_grad_(True)
            v = None if vals is None else vals.detach().requires_grad_(True)
            att, pooled = seq_ops.sigmoid_attention(s, Wa, ba, nf, v)
            if Hv:                              # the gradient the plugin hands back: LstmAttentionLstmModel's reaches pooled alone
                pooled.backward(G)
            else:
                att.backward(E)
            return att.detach(), (None if pooled is None else pooled.detach()), s.grad, (None if v is None else v.grad), Wa.grad.clone(), ba.grad.clone()

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        seq_ops.SIGMOID_ATTENTION_FUSED = True
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        rel = lambda a, b: None if a is None else float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        names = ("att", "pooled", "dsrc", "dvals", "dWa", "dba")
        print(json.dumps(dict(
            leg="op", F=F_, B=B_, Hs=Hs, Hv=Hv, A=A, what="forward + backward through autograd", src_vals_bytes=4 * F_ * B_ * (Hs + Hv),
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            diff_fused_composed_rel_to_max={n: rel(a, b) for n, a, b in zip(names, rf, rc)}, calls=dict(seq_ops.SIGMOID_ATTENTION_CALLS),
            repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                    % iters)), flush=True)
        del nf, src, vals, G, E
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
    for shape in SHAPES:
        F_, B_, Hs, Hv, A = shape
        nf, src, vals, G, E = _inputs(dev, shape, sum(shape))
        Wa = torch.randn((Hs, A), device=dev) / Hs ** 0.5
        ba = torch.zeros((A,), device=dev)
        att, den = torch.empty((B_, F_, A), device=dev), torch.empty((B_, A), device=dev)
        pooled = torch.empty((B_, A, Hv), device=dev) if Hv else None
        dsrc, dvals = torch.empty_like(src), (torch.empty_like(vals) if Hv else None)
        dWa, dba = torch.empty_like(Wa), torch.empty_like(ba)
        nbytes = lib.yt8m_sigattn_workspace_bytes(B_, F_, Hs, Hv, A)
        ws = torch.empty(nbytes // 4, device=dev)
        fwd = lambda: L.check(lib.yt8m_sigattn_fwd(p(src), Hs, p(vals), Hv, p(Wa), p(ba), p(nf), p(att), p(den), p(pooled), p(ws), nbytes,
                                                   B_, F_, Hs, Hv, A, st()))
        bwd = lambda: L.check(lib.yt8m_sigattn_bwd(p(src), Hs, p(vals), Hv, p(Wa), p(nf), p(att), p(den), p(pooled), p(G), p(None if Hv else E),
                                                   p(dsrc), Hs, p(dvals), Hv, p(dWa), p(dba), p(ws), nbytes, B_, F_, Hs, Hv, A, st()))
        fwd()
        live = float(nf.sum()) / (F_ * B_)                   # rows past num_frames are not read; the backward still writes them
        full = 4 * F_ * B_ * (Hs + Hv)
        chunks = (F_ + 31) // 32
        small = 4 * (3 * B_ * F_ * A + 2 * chunks * B_ * A * Hv)
        parts = 4 * 2 * B_ * chunks * (Hs * A + A)
        nbytes_of = {"fwd": int(full * live) + small, "bwd": int(full * live) + full + parts + small}
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, v in us.items():
            med = steplib.median(v)
            print(json.dumps(dict(leg="kernels", kernel=k, F=F_, B=B_, Hs=Hs, Hv=Hv, A=A, bytes=nbytes_of[k], live_rows=round(live, 3),
                                  **steplib.spread_fields("call", v, "us"), TB_per_s=round(nbytes_of[k] / med / 1e6, 3),
                                  measured_streaming_read_TB_per_s="6.0-6.3",
                                  timing="hip events over %d back-to-back calls through the C ABI" % iters)), flush=True)
        del src, vals, dsrc, dvals, ws
        torch.cuda.empty_cache()
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
    rc = 0
    for plugin in PLUGINS:
        # learning rate 0 (the step does the same work): the steps repeat one random batch
        graphs = {name: train.build_graph(getattr(flm, name)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)
                  for name in (plugin,) + SCALE}
        forms = {"fused": (plugin, True), "composed": (plugin, False), "lstm": ("LstmModel", True), "lstm_memory": ("LstmMemoryModel", True)}

        def run(form, n):
            which, fused = forms[form]
            seq_ops.SIGMOID_ATTENTION_FUSED = fused
            for _ in range(n):
                out = graphs[which].step(*batch)
            torch.cuda.synchronize()
            return float(out["loss"])

        losses_ = {k: run(k, warmup) for k in forms}
        ms = steplib.steps_in_turn(run, forms, steps, repeats)
        seq_ops.SIGMOID_ATTENTION_FUSED = True
        row = dict(leg="step", plugin=plugin, scale=list(SCALE), B=B, V=V, input="uint8 [B,300,1152]", flags=STEP_FLAGS, steps=steps,
                   warmup=warmup, repeats=repeats, losses_after_warmup=losses_, calls=dict(seq_ops.SIGMOID_ATTENTION_CALLS),
                   timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
        for k, v in ms.items():
            row.update(steplib.spread_fields(k, v, "ms"))
        row.update(steplib.fused_against_composed(ms))
        row["fused_below_composed"] = bool(steplib.median(ms["fused"]) < steplib.median(ms["composed"]))
        print(json.dumps(row), flush=True)
        rc = rc or (0 if all(np.isfinite(v) for v in losses_.values()) else 1)
        del graphs
        torch.cuda.empty_cache()
    return rc


def summarise(rows):
    return steplib.verdict_after(rows, "op", "leg_repeat", "the kernels are the default only if this holds over two runs of the leg")


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=10)
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
