"""The windowed softmax attention pooling (seq_ops.softmax_attention_tm, csrc/softmax_attention.hip) and the two Extend plugins on it at the
training shape.
`op` (timed first, and run twice by the driver): forward + backward of seq_ops.softmax_attention_tm through autograd, the kernels against
the composed form (the YT8M_SOFTMAX_ATTENTION_FUSED=0 form: ops.linear on the [F B, Hs] view, a masked softmax in torch, pool_tn on a
batch-major copy), at [F, B, Hs, Hv, E] = [300,128,1024,shared,8] (LstmExtendModel), [300,128,1024,1024,4] windowed (InputExtendModel),
[300,32,1024,shared,8] and [300,128,1024,shared,1]: hip events around back-to-back calls, the two forms alternating inside every repeat,
values and gradients compared.  W1 and b1 are Variables of a graph, as in the plugins; extra takes a gradient, as the plugins' does.  The
driver adds an `op_summary` row: whether the kernels' median was below the composed one at every shape in both runs -- what decides the
default.
`kernels`: yt8m_smattn_fwd and yt8m_smattn_bwd alone through the C ABI at the same shapes, with the bytes each has to move computed from
the shapes (the rows of src and vals that some head unmasks once each way, every row of the gradients written, the partials written and
read back) and the rate in TB/s.
`step`: whole training steps (cross entropy, clip, Adam; learning rate 0) of the two plugins under the scripts' flags at B = 128, F = 300
on the reader's bytes with the switch on and off, LstmAttentionMaxPoolingModel, LstmModel and LstmMemoryModel with the same cells in the
same run for the scale.
Every leg runs in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/extend_attention_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op kernels step"""
import ctypes
import json
import sys

import steplib

V = steplib.V
# (F, B, Hs, Hv or None = the shared mode, E, windowed)
SHAPES = ((300, 128, 1024, None, 8, False), (300, 128, 1024, 1024, 4, True), (300, 32, 1024, None, 8, False), (300, 128, 1024, None, 1, False))
B, F = 128, 300
# Z/train_scripts/run-attention-pooling.sh and run-attention-pooling-lstm2lstm.sh: the flags' default cells and layers, 8 mixtures
STEP_FLAGS = dict(lstm_cells="1024", lstm_layers=2, moe_num_mixtures=8, video_level_classifier_model="MoeExtendModel")
PLUGINS = (("LstmExtendModel", 8), ("InputExtendModel", 4))
SCALE = ("LstmAttentionMaxPoolingModel", "LstmModel", "LstmMemoryModel")


def _inputs(dev, shape, seed):
    import torch
    F_, B_, Hs, Hv, E, windowed = shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    nf = torch.randint(F_ // 2, F_ + 1, (B_,), device=dev, generator=gen, dtype=torch.int32)
    live = (torch.arange(F_, device=dev)[:, None] < nf[None, :]).to(torch.float32)[:, :, None]
    src = torch.tanh(torch.randn((F_, B_, Hs), device=dev, generator=gen)) * live                  # what a stack leaves: zero past num_frames
    vals = None if Hv is None else torch.tanh(torch.randn((F_, B_, Hv), device=dev, generator=gen)) * live
    extra = 0.5 * torch.randn((B_, F_, E), device=dev, generator=gen)
    G = torch.randn((B_, E, Hs if Hv is None else Hv), device=dev, generator=gen)
    if windowed:                                                                                    # InputExtendModel's windows
        step = (nf // E).view(-1, 1)
        lo = (step * torch.arange(E, device=dev, dtype=torch.int32).view(1, -1)).contiguous()
        hi = (lo + 2 * step).contiguous()
    else:                                                                                           # LstmExtendModel on bytes
        lo, hi = None, (nf - 1).view(-1, 1).expand(B_, E).contiguous()
    return nf, src, vals, extra, G, lo, hi


def _unmasked_rows(nf, lo, hi, F_):
    """the share of the F B rows that some head unmasks"""
    import torch
    t = torch.arange(F_, device=nf.device).view(1, F_, 1)
    m = t <= hi.view(hi.shape[0], 1, -1)
    if lo is not None:
        m = m & (t >= lo.view(lo.shape[0], 1, -1))
    return float(m.any(dim=2).float().mean())


def _tag(shape):
    F_, B_, Hs, Hv, E, windowed = shape
    return dict(F=F_, B=B_, Hs=Hs, Hv="shared" if Hv is None else Hv, E=E, mask="windows" if windowed else "frames")


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.seq_ops as seq_ops
    from yt8m_amd.variables import constant, reset_default_graph, truncated_normal
    for shape in SHAPES:
        F_, B_, Hs, Hv, E, windowed = shape
        nf, src, vals, extra, G, lo, hi = _inputs(dev, shape, sum(v or 0 for v in shape))
        g = reset_default_graph(device=dev, seed=0)
        W1 = g.get_variable("W1", (Hs, E), truncated_normal(0.1))
        b1 = g.get_variable("b1", (E,), constant(0.1))
        g.finalize()

        def run(fused):
            seq_ops.SOFTMAX_ATTENTION_FUSED = fused
            g.begin_step()
            s = src.detach().requires_grad_(True)
            v = s if vals is None else vals.detach().requires_grad_(True)
            x = extra.detach().requires_grad_(True)
            att, pooled = seq_ops.softmax_attention_tm(s, W1, b1, v, extra=x, lo=lo, hi=hi)
            pooled.backward(G)
            return att.detach(), pooled.detach(), s.grad, (None if vals is None else v.grad), W1.grad.clone(), b1.grad.clone(), x.grad

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        seq_ops.SOFTMAX_ATTENTION_FUSED = True
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        # db1's exact value is 0: the difference is given in absolute terms there
        rel = lambda a, b: None if a is None else float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        names = ("att", "pooled", "dsrc", "dvals", "dW1", "db1", "dextra")
        diff = {n: (float((a - b).abs().max()) if n == "db1" else rel(a, b)) for n, a, b in zip(names, rf, rc)}
        rows_bytes = 4 * F_ * B_ * (Hs + (0 if Hv is None else Hv))
        print(json.dumps(dict(
            leg="op", **_tag(shape), what="forward + backward through autograd", src_vals_bytes=rows_bytes,
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            diff_fused_composed_rel_to_max_db1_absolute=diff, calls=dict(seq_ops.SOFTMAX_ATTENTION_CALLS),
            repeats=repeats, timing="hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats"
                                    % iters)), flush=True)
        del nf, src, vals, extra, G
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
        F_, B_, Hs, Hv, E, windowed = shape
        nf, src, vals, extra, G, lo, hi = _inputs(dev, shape, sum(v or 0 for v in shape))
        shared = Hv is None
        hv = Hs if shared else Hv
        v = src if shared else vals
        W1 = torch.randn((Hs, E), device=dev) / Hs ** 0.5
        b1 = torch.zeros((E,), device=dev)
        att, pooled = torch.empty((B_, F_, E), device=dev), torch.empty((B_, E, hv), device=dev)
        dsrc, dvals = torch.empty_like(src), (None if shared else torch.empty_like(vals))
        dW1, db1, dextra = torch.empty_like(W1), torch.empty_like(b1), torch.empty_like(extra)
        nbytes = lib.yt8m_smattn_workspace_bytes(B_, F_, Hs, hv, E)
        ws = torch.empty(nbytes // 4, device=dev)
        fwd = lambda: L.check(lib.yt8m_smattn_fwd(p(src), Hs, p(v), hv, p(W1), p(b1), p(extra), None, p(lo), p(hi), p(att), p(pooled), p(ws),
                                                  nbytes, B_, F_, Hs, hv, E, st()))
        bwd = lambda: L.check(lib.yt8m_smattn_bwd(p(src), Hs, p(v), hv, p(W1), None, p(lo), p(hi), p(att), p(pooled), p(G), p(dsrc), Hs, p(dvals),
                                                  hv, p(dW1), p(db1), p(dextra), p(ws), nbytes, B_, F_, Hs, hv, E, st()))
        fwd()
        live = _unmasked_rows(nf, lo, hi, F_)                # rows no head unmasks are not read; the backward still writes them
        read = 4 * F_ * B_ * (Hs + (0 if shared else hv))    # (the shared mode walks ONE tensor; its second read is the caches')
        chunks = (F_ + 63) // 64
        small = 4 * 4 * B_ * F_ * E
        pool_parts = 4 * 2 * chunks * B_ * E * hv            # written by the chunks, read by the finish
        dw_parts = 4 * 2 * B_ * chunks * Hs * E
        nbytes_of = {"fwd": int(read * live) + pool_parts + small, "bwd": int(read * live) + read + dw_parts + small}
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, val in us.items():
            med = steplib.median(val)
            print(json.dumps(dict(leg="kernels", kernel=k, **_tag(shape), bytes=nbytes_of[k], unmasked_rows=round(live, 3),
                                  partials_bytes=pool_parts if k == "fwd" else dw_parts,
                                  **steplib.spread_fields("call", val, "us"), TB_per_s=round(nbytes_of[k] / med / 1e6, 3),
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
    batch = steplib.random_batch(dev, B, F, "ends", first_label=True)[:3]
    rc = 0
    for plugin, num_extend in PLUGINS:
        FLAGS.reset()
        FLAGS.batch_size = B
        flags_ = dict(STEP_FLAGS, moe_num_extend=num_extend, lstm_attentions=num_extend)
        for k, v in flags_.items():
            setattr(FLAGS, k, v)
        # learning rate 0 (the step does the same work): the steps repeat one random batch
        graphs = {}
        for name in (plugin,) + SCALE:
            FLAGS.video_level_classifier_model = "MoeExtendModel" if name == plugin else "MoeModel"
            graphs[name] = train.build_graph(getattr(flm, name)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0),
                                             base_learning_rate=0.0)
        forms = {"fused": (plugin, True), "composed": (plugin, False), "lstm_attention_max_pooling": (SCALE[0], True),
                 "lstm": ("LstmModel", True), "lstm_memory": ("LstmMemoryModel", True)}

        def run(form, n):
            which, fused = forms[form]
            seq_ops.SOFTMAX_ATTENTION_FUSED = fused
            FLAGS.video_level_classifier_model = "MoeExtendModel" if which == plugin else "MoeModel"
            for _ in range(n):
                out = graphs[which].step(*batch)
            torch.cuda.synchronize()
            return float(out["loss"])

        losses_ = {k: run(k, warmup) for k in forms}
        ms = steplib.steps_in_turn(run, forms, steps, repeats)
        seq_ops.SOFTMAX_ATTENTION_FUSED = True
        row = dict(leg="step", plugin=plugin, scale=list(SCALE), B=B, V=V, input="uint8 [B,300,1152]", flags=flags_, steps=steps,
                   warmup=warmup, repeats=repeats, losses_after_warmup=losses_, calls=dict(seq_ops.SOFTMAX_ATTENTION_CALLS),
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
