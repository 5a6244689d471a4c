"""ms / step of MultiscaleCnnLstmModel at its own shape (B = 128, F = 300, D = 1152 uint8 frames, H = 1024, 4 scales, 4 mixtures,
multitask loss, fp32 step with clip + Adam; W/training_scripts/run-multiscale-cnn-lstm-model.sh): the fused time-major path, the
generic composition (YT8M_MULTISCALE_FUSED=0: the price of this function when built from the other plugins' ops), LstmModel for context,
and the new kernels alone (device-event times, the bytes their shapes imply, the resulting TB/s).  Every leg runs in a child process of
its own under its own time limit; the driver stops at the first leg that fails; without a GPU a leg fails, nothing falls back.  The
default order alternates fused and generic twice: the difference between the two runs of one leg is the repeat-to-repeat spread the
comparison has to be read against.  The timed window of a leg is device-synchronised at both ends and at least --min_seconds long.
usage: python tools/multiscale_step.py [--steps K] [--warmup W] [--out FILE] [leg ...]    legs: fused generic lstm kernels"""
import json
import sys

import steplib

LEGS = {
    "fused": ("MultiscaleCnnLstmModel", "1"),
    "generic": ("MultiscaleCnnLstmModel", "0"),
    "lstm": ("LstmModel", "1"),
    "kernels": (None, "1"),
}
DEFAULT_ORDER = ["fused", "generic", "fused", "generic", "lstm", "kernels"]
HBM_PEAK_TBS, HBM_MEASURED_TBS, INFINITY_CACHE_MIB = 8.0, 6.3, 256     # MI355X: spec, float4 copy, last-level cache


def child_step(leg, steps, warmup, min_seconds):
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    B, F = 128, 300
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers = "1024", 2
    FLAGS.multiscale_cnn_lstm_layers, FLAGS.moe_num_mixtures, FLAGS.is_training = 4, 4, True
    FLAGS.support_type, FLAGS.support_loss_percent = "label,label,label,label", 0.1
    multiscale = LEGS[leg][0] == "MultiscaleCnnLstmModel"
    g = reset_default_graph(device=dev, seed=0)
    kw = dict(label_loss_fn=losses.MultiTaskCrossEntropyLoss(), multitask=True) if multiscale else {}
    tg = train.TrainGraph(getattr(flm, LEGS[leg][0])(), batch_size=B, graph=g, **kw)
    x, y, nf, _ = steplib.random_batch(dev, B, F)
    calls = dict(seq_ops.NATIVE_CALLS)
    loss_first = steplib.warm_up(lambda: tg.step(x, y, nf), warmup, seq_ops.check_persist_errors)
    native = seq_ops.NATIVE_CALLS["fwd"] - calls["fwd"]
    out, elapsed, done = steplib.timed_steps(lambda: tg.step(x, y, nf), steps, min_seconds)
    seq_ops.check_persist_errors()
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model=LEGS[leg][0], fused=bool(seq_ops.MULTISCALE_FUSED) if multiscale else None,
                          ms_per_step=round(elapsed / done * 1e3, 3), steps=done, warmup=warmup, window_s=round(elapsed, 3),
                          loss_first=loss_first, loss=float(out["loss"]), params_finite=finite,
                          native_stacks_per_step=native / max(warmup, 1))), flush=True)
    return 0 if finite else 1


def child_kernels(reps):
    """The new kernels alone at (F, B, C) = (300, 128, 1024), fp32.  Bytes = what the shapes imply (4 M C per full tensor, half of it per
    pooled one): moments read y twice; forward reads y, writes a and p; backward pass 1 reads y, da, dp, pass 2 reads them again and
    writes dy.  The 157 MB tensors partly fit the 256 MiB Infinity Cache (a kernel's second read of y, or the reads of a tensor the
    previous kernel just wrote, may come from it): figures up to the measured HBM rate (6.3 TB/s; 8 TB/s spec) can be read against HBM,
    anything above only against the cache."""
    import torch
    dev = steplib.setup()
    import ctypes
    import yt8m_amd._lib as L
    lib = L.lib()
    F, B, C = 300, 128, 1024
    M = F * B
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = torch.randn(M, C, device=dev)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
    mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    a, pooled = torch.empty(F, B, C, device=dev), torch.empty(F // 2, B, C, device=dev)
    da, dp, dy = torch.randn(F, B, C, device=dev), torch.randn(F // 2, B, C, device=dev), torch.empty(M, C, device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    nws = lib.yt8m_multiscale_workspace_bytes(C)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
    full = 4.0 * M * C
    half = 4.0 * (F // 2) * B * C
    cases = {
        "colmoments": (2 * full, lambda: lib.yt8m_colmoments_f32(p(y), M, C, C, p(mm), p(mv), 1, 1e-3, 0.999, p(mean), p(rstd), p(ws), nws, st())),
        "bn_relu_pool2_fwd": (2 * full + half, lambda: lib.yt8m_bn_relu_pool2_tm_fwd(p(y), C, F, B, C, p(gamma), p(beta), p(mean), p(rstd), p(a), C,
                                                                                     p(pooled), C, st())),
        "bn_relu_pool2_bwd": (2 * (2 * full + half) + full, lambda: lib.yt8m_bn_relu_pool2_tm_bwd(
            p(y), C, F, B, C, p(gamma), p(beta), p(mean), p(rstd), 1, p(da), C, p(dp), C, p(dy), C, p(dg), 0.0, p(db), 0.0, p(ws), nws, st())),
    }
    rows = []
    for name, (nbytes, fn) in cases.items():
        for _ in range(3):
            L.check(fn())
        us = steplib.events_us(lambda: L.check(fn()), reps)
        rows.append(dict(kernel=name, us=round(us, 1), mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / us / 1e6, 2)))
    print(json.dumps(dict(leg="kernels", shape=[F, B, C], reps=reps, hbm_peak_tb_per_s=HBM_PEAK_TBS, hbm_measured_tb_per_s=HBM_MEASURED_TBS,
                          infinity_cache_mib=INFINITY_CACHE_MIB, tensor_mbytes=round(full / 1e6, 1), kernels=rows)), flush=True)
    return 0


def summarise(rows):
    by = steplib.ms_by_leg(rows)
    if not ("fused" in by and "generic" in by):
        return rows
    spread = lambda v: round(max(v) - min(v), 3) if len(v) > 1 else None
    fused, generic = min(by["fused"]), min(by["generic"])
    return rows + [dict(fused_ms=by["fused"], generic_ms=by["generic"], fused_spread_ms=spread(by["fused"]),
                        generic_spread_ms=spread(by["generic"]), fused_over_generic=round(fused / generic, 3),
                        lstm_ms=by.get("lstm"), fused_default=max(by["fused"]) <= max(by["generic"]))]


def parser():
    ap = steplib.arg_parser(steps=10, warmup=3, timeout=300)
    ap.add_argument("--min_seconds", type=float, default=1.0, help="shortest timed window of a leg")
    return ap


def main():
    a = steplib.parse_args(parser(), list(LEGS))
    if a.child:
        return child_kernels(50) if a.child == "kernels" else child_step(a.child, a.steps, a.warmup, a.min_seconds)
    return steplib.drive(__file__, a.legs or DEFAULT_ORDER, steplib.child_args(a, "min_seconds"), a.timeout, a.out,
                         env_of=lambda leg: {"YT8M_MULTISCALE_FUSED": LEGS[leg][1]}, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
