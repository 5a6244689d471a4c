"""ms / step of the data augmenters at the bench's frame-level shape (F = 300, D = 1152 uint8 frames, fp32 step with clip + Adam): each
plugin with HalfAugmenter on B = 128 videos against the same plugin with DefaultAugmenter fed the pre-tiled 384-row byte batch (the
difference is what the augmentation itself costs), and DeepCombineChainModel with HalfVideoAugmenter at B = 200 against the pre-averaged
600-row float batch.  `--kernels` times the augment kernels alone with hip events (run it under `rocprofv3 --kernel-trace --stats` for the
profiler's view) and reports the achieved bandwidth on the bytes the shapes imply.  Every leg runs in a child process of its own under
its own time limit; the driver stops at the first leg that fails.
usage: python tools/augment_step.py [--steps K] [--warmup W] [--out FILE] [leg ...]      legs: see LEGS, and `kernels`"""
import json
import sys

import steplib

LEGS = {                                     # leg -> (model, augmenter, videos per step)
    "lstm_half": ("LstmModel", "HalfAugmenter", 128),
    "lstm_tiled": ("LstmModel", "DefaultAugmenter", 128),
    "cnn_half": ("CnnDeepCombineChainModel", "HalfAugmenter", 128),
    "cnn_tiled": ("CnnDeepCombineChainModel", "DefaultAugmenter", 128),
    "attn_half": ("LstmPositionalAttentionMaxPoolingModel", "HalfAugmenter", 128),
    "attn_tiled": ("LstmPositionalAttentionMaxPoolingModel", "DefaultAugmenter", 128),
    "chain_halfvideo": ("DeepCombineChainModel", "HalfVideoAugmenter", 200),
    "chain_tiled": ("DeepCombineChainModel", "DefaultAugmenter", 200),
}
F, D = 300, 1152


def kernels(iters):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    gen = torch.Generator(device=dev).manual_seed(1)
    for name, B in (("half_segments_u8", 128), ("half_segment_means_u8", 200), ("dequant_noise_u8", 128)):
        q = torch.randint(0, 256, (B, F, D), device=dev, generator=gen, dtype=torch.uint8)
        nf = torch.randint(F // 2, F + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
        if name == "half_segments_u8":
            fn, nbytes = (lambda: ops.half_segments(q, nf)), B * F * D + 3 * B * F * D          # read the bytes once, write 3 copies
        elif name == "half_segment_means_u8":
            fn, nbytes = (lambda: ops.half_segment_means(q, nf, l2norm=True)), B * F * D + 12 * B * D
        else:
            fn, nbytes = (lambda: ops.dequant_noise(q, nf, 0.2, 7)), 5 * B * F * D                 # 1 byte in, 4 bytes out
        for _ in range(3):
            fn()
        us = steplib.events_us(fn, iters)
        row = dict(leg="kernel", kernel=name, B=B, F=F, D=D, us_per_call=round(us, 2), bytes=nbytes,
                   tb_per_s=round(nbytes / (us * 1e-6) / 1e12, 3), timing="hip events over %d back-to-back calls (torch allocations included)" % iters)
        print(json.dumps(row), flush=True)
    return 0


def child(leg, steps, warmup):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.data_augmentation as da
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    model_name, aug, B = LEGS[leg]
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers = "1024", 2
    g = reset_default_graph(device=dev, seed=0)
    model = getattr(flm, model_name, None) or getattr(vlm, model_name)
    tg = train.TrainGraph(model(), batch_size=B, graph=g, augmenter_class=getattr(da, aug))
    x, y, nf, _ = steplib.random_batch(dev, B, F)
    nf_host = nf.cpu()                                                     # the reader's host copy: the augmenter's no-sync path
    if aug == "DefaultAugmenter":                                          # the batch the augmenter would make, made up front
        if model_name == "DeepCombineChainModel":
            x, nf_host = ops.half_segment_means(x, nf), torch.cat([nf.cpu(), (nf.cpu() // 2).clamp(min=1), (nf.cpu() // 2).clamp(min=1)])
        else:
            x, nf = ops.half_segments(x, nf)
            nf_host = nf
        y = torch.cat([y, y, y])
    loss_first = steplib.warm_up(lambda: tg.step(x, y, nf_host), warmup, seq_ops.check_persist_errors)
    out, elapsed, _ = steplib.timed_steps(lambda: tg.step(x, y, nf_host), steps)
    seq_ops.check_persist_errors()
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model=model_name, augmenter=aug, videos=B, rows=int(out["predictions"].shape[0]),
                          input=str(x.dtype).replace("torch.", ""), ms_per_step=round(elapsed / steps * 1e3, 3), steps=steps, warmup=warmup,
                          loss_first=loss_first, loss=float(out["loss"]), params_finite=finite)), flush=True)
    return 0 if finite and np.isfinite(loss_first) else 1


def summarise(rows):
    by = {r["leg"]: r["ms_per_step"] for r in rows if "ms_per_step" in r}
    costs = []
    for base in ("lstm", "cnn", "attn", "chain"):
        aug = base + ("_halfvideo" if base == "chain" else "_half")
        if aug in by and base + "_tiled" in by:
            costs.append(dict(leg=base + "_augment_cost", ms_per_step=round(by[aug] - by[base + "_tiled"], 3)))
    return rows + costs


def parser():
    return steplib.arg_parser(steps=20, warmup=3, timeout=300)


def main():
    a = steplib.parse_args(parser(), list(LEGS) + ["kernels"])
    if a.child == "kernels":
        return kernels(a.steps)
    if a.child:
        return child(a.child, a.steps, a.warmup)
    return steplib.drive(__file__, a.legs or list(LEGS) + ["kernels"], steplib.child_args(a), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
