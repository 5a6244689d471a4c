"""The stage step of Z's combine chain heads (ops.mix_link, csrc/mix_link.hip) and the heads on it at their training scripts' shapes
(--moe_num_mixtures=4 --moe_layers=3 --class_size=100; LstmExtendCombineModel with --frame_features and 8 heads).
`kernels`: forward + backward of one stage step through autograd -- from the previous stage's input and prediction to the next stage's
input, the class_inputs products included -- the kernels (YT8M_MIX_LINK_FUSED=1: one product, the complement as u2 - z2) against the
composed form (two products, a materialised 1 - p), alternating inside every repeat, at [rows; Wprev; C] = [1024; 1152; 100],
[1024; 1552; 100], [128; 1152; 100] and, in none mode, [1024; 1024; 200], V = 4716, and the MoeKnowledge form (the second segment from a
given q [rows, 25], switch YT8M_MIX_LINK_FUSED_Q) at the first.  prev takes a gradient from column 1152 on, as in a later stage of the video-level heads; in none mode all of it does (an LSTM's pooled rows).  Hip events around back-to-back calls,
values and gradients compared.  The driver adds a `kernels_summary` row: whether the kernels' median was below the composed form's at
every shape in every run of the leg -- what decides the default.
`launches`: the two entry points alone through the C ABI at the same shapes, with the bytes each has to move and the rate in TB/s.
Step legs: whole training steps (fp32, cross entropy under the mix loss rule, clip + Adam, learning rate 0) with the switch on, off,
and of a same-run yardstick, in ONE process and in turn inside every repeat: `mix4` and `knowledge`, MoeMix4Model / MoeKnowledgeModel at
B = 1024 on float features against DeepCombineChainModel; `extend_combine`, LstmExtendCombineModel at B = 128, F = 300 on the reader's
bytes against LstmExtendModel + MoeExtendModel.
Every leg runs in a child process of its own under its own time limit, and every leg runs twice (rows numbered by `run`); the driver
stops at the first leg that fails.
usage: python tools/mix_chain_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: kernels launches and LEGS"""
import ctypes
import json
import os
import sys
import tempfile

import steplib

V = steplib.V
D = 1152
K = 25                     # the columns of the knowledge leg's class matrix (the reference's own file is not in its repository)
# (rows, Wprev, C, normalised, dx_from, columns of q: 0 = the complement mode)
CASES = [(1024, 1152, 100, True, 1152, 0), (1024, 1552, 100, True, 1152, 0), (128, 1152, 100, True, 1152, 0), (1024, 1024, 200, False, 0, 0),
         (1024, 1152, 100, True, 1152, K)]
SCRIPT = dict(moe_num_mixtures=4, moe_layers=3, class_size=100)
# leg: (model, yardstick, batch, frame level?, flags of the script, flags of the yardstick)
LEGS = {
    "mix4": ("MoeMix4Model", "DeepCombineChainModel", 1024, False, SCRIPT, dict(moe_num_mixtures=4)),
    "knowledge": ("MoeKnowledgeModel", "DeepCombineChainModel", 1024, False, SCRIPT, dict(moe_num_mixtures=4)),
    "extend_combine": ("LstmExtendCombineModel", "LstmExtendModel", 128, True,
                       dict(SCRIPT, frame_features=True, moe_num_extend=8, lstm_cells="1024"),
                       dict(moe_num_mixtures=4, moe_num_extend=8, lstm_cells="1024", video_level_classifier_model="MoeExtendModel")),
}


def _operands(dev, rows, Wprev, C, seed):
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    prev = torch.randn((rows, Wprev), device=dev, generator=gen)
    p = torch.rand((rows, V), device=dev, generator=gen) ** 8           # most labels near 0, a few near 1
    dy = torch.randn((rows, Wprev + 2 * C), device=dev, generator=gen)
    return prev, p, dy


def _scale(C):
    import torch
    return float(torch.sqrt(torch.tensor(float(C)) / D))


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    from yt8m_amd.variables import reset_default_graph, xavier_uniform, zeros
    timing = "hip events over %d back-to-back calls (torch allocations and autograd included), median of the repeats" % iters
    for rows, Wprev, C, norm, dx_from, Kq in CASES:
        prev, p, dy = _operands(dev, rows, Wprev, C, rows + Wprev + C)
        q = torch.rand((rows, Kq), device=dev) if Kq else None
        g = reset_default_graph(device=dev, seed=0)
        W1, b1 = g.get_variable("class_inputs1-0/weights", (V, C), xavier_uniform), g.get_variable("class_inputs1-0/biases", (C,), zeros)
        W2, b2 = g.get_variable("class_inputs2-0/weights", (Kq or V, C), xavier_uniform), g.get_variable("class_inputs2-0/biases", (C,), zeros)
        g.finalize()
        scale = _scale(C)

        def run(fused):
            ops.MIX_LINK_FUSED = ops.MIX_LINK_FUSED_Q = fused
            for v in (W1, b1, W2, b2):
                v.grad_written = False
            pq, xq = prev.detach().requires_grad_(True), p.detach().requires_grad_(True)
            y = ops.mix_link(pq, xq, W1, b1, W2, b2, q=q, norm=norm, scale=scale, dx_from=dx_from)
            y.backward(dy)
            return [y.detach(), xq.grad, pq.grad[:, dx_from:], W1.grad.clone(), W2.grad.clone(), b1.grad.clone(), b2.grad.clone()]

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        ops.MIX_LINK_FUSED = ops.MIX_LINK_FUSED_Q = False
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        print(json.dumps(dict(
            leg="kernels", op="mix_link", rows=rows, Wprev=Wprev, C=C, V=V, mode="norm" if norm else "none", dx_from=dx_from,
            second="q [rows, %d] (the MoeKnowledge form)" % Kq if Kq else "complement",
            what="forward + backward of one stage step through autograd, the class_inputs products included",
            launches_fused="1 product + 1 kernel forward; 1 kernel + 1 column sum + 1 product for dp + 1 grouped product for dW backward",
            ops_composed_forward=2 + 1 + 2 + (4 if norm else 0) + 1,          # products, 1 - p, elu, l2norm and scale, cat
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            max_rel_diff_fused_composed=max(float((a - b).abs().max() / b.abs().max().clamp(min=1.0)) for a, b in zip(rf, rc) if a.numel()),
            repeats=repeats, timing=timing)), flush=True)
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def launches(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    lib = L.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    timing = "hip events over %d back-to-back calls through the C ABI" % iters
    for rows, Wprev, C, norm, dx_from, Kq in CASES[:4]:
        prev, _, dy = _operands(dev, rows, Wprev, C, rows + Wprev + C)
        gen = torch.Generator(device=dev).manual_seed(C)
        z, u = torch.randn((rows, 2 * C), device=dev, generator=gen), torch.randn((2 * C,), device=dev, generator=gen)
        out, stats = torch.empty((rows, Wprev + 2 * C), device=dev), torch.empty((2, rows), device=dev)
        dprev, dz = torch.zeros((rows, Wprev), device=dev), torch.empty((rows, 2 * C), device=dev)
        bits, scale = (0 if norm else 2), _scale(C)
        fwd = lambda: L.check(lib.yt8m_mix_link_fwd(bits, p(prev), p(z), p(u), p(out), p(stats), rows, Wprev, C, scale, 1e-12, st()))
        bwd = lambda: L.check(lib.yt8m_mix_link_bwd(bits, p(z), p(u), p(stats), p(dy), p(dprev), p(dz), rows, Wprev, C, dx_from, scale, st()))
        fwd()
        nbytes_of = {"fwd": 4 * (rows * (Wprev + 2 * C + Wprev + 2 * C + 2) + 2 * C),          # prev, z, out, stats; u
                     "bwd": 4 * (rows * (2 * C + 2 * C + 2 * C + 2 + 2 * (Wprev - dx_from)) + 2 * C)}      # z, dy's segments, dz, stats, the copied columns
        us = steplib.alternate({"fwd": fwd, "bwd": bwd}, iters, repeats)
        for k, val in us.items():
            med = steplib.median(val)
            print(json.dumps(dict(leg="launches", kernel="mix_link_" + k, rows=rows, Wprev=Wprev, C=C, mode="norm" if norm else "none",
                                  dx_from=dx_from, bytes=nbytes_of[k], **steplib.spread_fields("call", val, "us"),
                                  TB_per_s=round(nbytes_of[k] / med / 1e6, 3), timing=timing)), flush=True)
    return 0


def child(leg, steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    model, yardstick, B, frames, fl, yfl = LEGS[leg]
    class_file = None
    if model == "MoeKnowledgeModel":
        rs = np.random.RandomState(0)
        fd, class_file = tempfile.mkstemp(suffix=".out")
        os.close(fd)
        np.savetxt(class_file, (rs.rand(V, K) < 0.1).astype(np.float64))

    def set_flags(which):
        """A graph keeps none of the flags it was built under: they are set again before every run of a form."""
        FLAGS.reset()
        FLAGS.batch_size = B
        for k, v in (fl if which == "plugin" else yfl).items():
            setattr(FLAGS, k, v)
        if class_file:
            FLAGS.class_file = class_file

    x, y, nf, _ = steplib.random_batch(dev, B, 300 if frames else None, "ends", first_label=True)
    batch = (x, y, nf) if frames else (x, y)
    # learning rate 0 (the step does the same work): the steps repeat one random batch
    graphs = {}
    for which, name in (("plugin", model), ("yardstick", yardstick)):
        set_flags(which)
        cls = getattr(flm, name) if frames else getattr(vlm, name)
        graphs[which] = train.build_graph(cls(), batch_size=B, graph=reset_default_graph(device=dev, seed=0), base_learning_rate=0.0)
    forms = {"fused": ("plugin", True), "composed": ("plugin", False), "yardstick": ("yardstick", False)}

    def run(form, n):
        which, fused = forms[form]
        set_flags(which)
        ops.MIX_LINK_FUSED = ops.MIX_LINK_FUSED_Q = fused
        for _ in range(n):
            out = graphs[which].step(*batch)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        return float(out["loss"])

    try:
        losses = {k: run(k, warmup) for k in forms}
        ms = steplib.steps_in_turn(run, forms, steps, repeats)
    finally:
        if class_file:
            os.unlink(class_file)
    ops.MIX_LINK_FUSED = ops.MIX_LINK_FUSED_Q = False
    FLAGS.reset()
    finite = all(np.isfinite(v) for v in losses.values())
    row = dict(leg=leg, model=model, yardstick=yardstick + (" + MoeExtendModel" if frames else ""), B=B, V=V,
               input="uint8 [B,300,1152]" if frames else "float32 [B,1152]", flags=fl, yardstick_flags=yfl, steps=steps, warmup=warmup,
               repeats=repeats, losses_after_warmup=losses, calls=dict(ops.MIX_LINK_CALLS),
               timing="host clock around the steps of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    row.update(steplib.fused_against_composed(ms))
    print(json.dumps(row), flush=True)
    return 0 if finite else 1


def summarise(rows):
    """The rows, then one `kernels_summary` row per switch over every run of the `kernels` leg so far."""
    out = list(rows)
    for second in ("complement", "q"):
        timed = [r for r in rows if r.get("leg") == "kernels" and r.get("op") == "mix_link" and r["second"].startswith(second)]
        if timed:
            out.append(dict(leg="kernels_summary", op="mix_link", second=second, switch="YT8M_MIX_LINK_FUSED" + ("_Q" if second == "q" else ""), runs=len({r["run"] for r in timed}), rows=len(timed),
                            fused_below_composed_everywhere=bool(all(r["fused_below_composed"] for r in timed)),
                            rule="the kernel is the default only if this holds over two runs of the leg"))
    return out


def parser():
    ap = steplib.arg_parser(steps=10, warmup=3, timeout=300)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--kernel_iters", type=int, default=100)
    return ap


def main():
    a = steplib.parse_args(parser(), ["kernels", "launches"] + list(LEGS))
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child == "launches":
        return launches(a.kernel_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup, a.repeats)
    legs = a.legs or ["kernels", "launches"] + list(LEGS)
    plan = [(leg, {"run": run}) for run in range(2) for leg in legs]      # every leg twice
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "kernel_iters"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
