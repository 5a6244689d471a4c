"""ResolutionTransformer at the bench's frame-level shape (B = 128 videos of F = 300 uint8 frames, D = 1152).
`kernels`: yt8m_resolution_mean_u8 (one pass over the bytes) against the same function composed from the ops the project had before it,
ops.dequantize_frames -> view(B, F2, r, D).mean(2) -> ops.l2norm_fwd, for r = 2, 8 and 30: hip events around back-to-back calls, the two
forms alternating inside every repeat, the spread over the repeats recorded, the outputs compared, and the achieved bandwidth on the
bytes the shapes imply (fused: the real frames once + the fp32 output; the same bytes are charged to the composition, which moves more).
Step legs: LstmMemoryModel ms / step (fp32 step with clip + Adam) with --feature_transformer=ResolutionTransformer --time_resolution=8,
fused and composed, and under DefaultTransformer (all 300 frames) for scale.  Every leg runs in a child process of its own under its own
time limit, the step legs `--repeats` times in turn; the driver stops at the first leg that fails.
usage: python tools/resolution_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: see LEGS, and `kernels`"""
import json
import sys

import steplib

LEGS = ("lstmmem_resolution_fused", "lstmmem_resolution_composed", "lstmmem_default")
B, F, D = 128, 300, 1152
RESOLUTION = 8


def composed_resolution_mean(q, num_frames, r):
    """The ResolutionTransformer from the ops that were there before the fused kernel: three passes, a fp32 [B,F,D] copy in between."""
    import torch
    import yt8m_amd.ops as ops
    Bq, Fq, Dq = q.shape
    F2 = Fq // r
    nf = num_frames.to(q.device)
    x = ops.dequantize_frames(q, nf)
    m = x[:, :F2 * r].view(Bq, F2, r, Dq).mean(2)
    return ops.l2norm_fwd(m), torch.div(nf, r, rounding_mode="floor").to(torch.int32)


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    q, _, nf, _ = steplib.random_batch(dev, B, F)
    live = torch.arange(F, device=dev).view(1, F) < nf.view(B, 1)
    q = q * live.unsqueeze(2).to(torch.uint8)                                # the reader's zero padding
    for r in (2, 8, 30):
        F2 = F // r
        fused = lambda: ops.resolution_mean(q, nf, r)
        composed = lambda: composed_resolution_mean(q, nf, r)
        (yf, nff), (yc, nfc) = fused(), composed()
        assert torch.equal(nff, nfc)
        diff = float((yf - yc).abs().max())
        for _ in range(3):
            fused()
            composed()
        us = {"fused": [], "composed": []}
        for _ in range(repeats):                                             # alternating: both forms see the same machine
            us["fused"].append(steplib.events_us(fused, iters))
            us["composed"].append(steplib.events_us(composed, iters))
        nbytes = int(torch.minimum(nf, torch.tensor(F2 * r, device=dev)).sum()) * D + 4 * B * F2 * D
        for form in ("fused", "composed"):
            med = steplib.median(us[form])
            print(json.dumps(dict(leg="kernel", form=form, resolution=r, B=B, F=F, D=D, us_per_call=round(med, 2),
                                  us_min=round(min(us[form]), 2), us_max=round(max(us[form]), 2), repeats=repeats, algorithmic_bytes=nbytes,
                                  tb_per_s_on_algorithmic_bytes=round(nbytes / (med * 1e-6) / 1e12, 3), max_abs_diff_fused_composed=diff,
                                  timing="hip events over %d back-to-back calls (torch allocations included), median of the repeats"
                                         % iters)), flush=True)
        print(json.dumps(dict(leg="kernel_ratio", resolution=r,
                              composed_over_fused=round(steplib.median(us["composed"]) / steplib.median(us["fused"]), 2),
                              slowest_fused_us=round(max(us["fused"]), 2), fastest_composed_us=round(min(us["composed"]), 2))), flush=True)
    return 0


def child(leg, steps, warmup):
    import numpy as np
    dev = steplib.setup()
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph

    class ComposedResolutionTransformer(object):
        def transform(self, model_input_raw, num_frames, **unused_params):
            return composed_resolution_mean(model_input_raw, num_frames, FLAGS.time_resolution)

    transformer = {"lstmmem_resolution_fused": ft.ResolutionTransformer, "lstmmem_resolution_composed": ComposedResolutionTransformer,
                   "lstmmem_default": ft.DefaultTransformer}[leg]
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers, FLAGS.time_resolution = "1024", 2, RESOLUTION
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(flm.LstmMemoryModel(), batch_size=B, graph=g, transformer_class=transformer)
    x, y, nf, _ = steplib.random_batch(dev, B, F)
    loss_first = steplib.warm_up(lambda: tg.step(x, y, nf), warmup, seq_ops.check_persist_errors)
    out, elapsed, _ = steplib.timed_steps(lambda: tg.step(x, y, nf), steps)
    seq_ops.check_persist_errors()
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model="LstmMemoryModel", transformer=transformer.__name__, videos=B, frames=F,
                          time_resolution=RESOLUTION if "resolution" in leg else None, ms_per_step=round(elapsed / steps * 1e3, 3), steps=steps,
                          warmup=warmup, loss_first=loss_first, loss=float(out["loss"]), params_finite=finite,
                          timing="host clock around the steps, ending in a device synchronise")), flush=True)
    return 0 if finite and np.isfinite(loss_first) else 1


def parser():
    ap = steplib.arg_parser(steps=20, warmup=3, timeout=300)
    ap.add_argument("--repeats", type=int, default=3, help="times every step leg runs (in turn), and timing repeats of the kernel leg")
    ap.add_argument("--kernel_iters", type=int, default=50)
    return ap


def main():
    a = steplib.parse_args(parser(), ("kernels",) + LEGS)
    if a.child == "kernels":
        return kernels(a.kernel_iters, a.repeats)
    if a.child:
        return child(a.child, a.steps, a.warmup)
    return steplib.drive(__file__, steplib.repeated_plan(a.legs or ["kernels"] + list(LEGS), "kernels", a.repeats),
                         steplib.child_args(a, "repeats", "kernel_iters"), a.timeout, a.out, summarise=steplib.per_leg_medians)


if __name__ == "__main__":
    sys.exit(main())
