"""ms / step of MultiscaleCnnLstmModel at its own shape (B = 128, F = 300, D = 1152 uint8 frames, H = 1024, 4 scales, 4 mixtures,
multitask loss, fp32 step with clip + Adam; W/training_scripts/run-multiscale-cnn-lstm-model.sh): the fused time-major path, the
generic composition (YT8M_MULTISCALE_FUSED=0: the price of this function when built from the other plugins' ops), LstmModel for context,
and the new kernels alone (device-event times, the bytes their shapes imply, the resulting TB/s).  Every leg runs in a child process of
its own under its own time limit; the driver stops at the first leg that fails; without a GPU a leg fails, nothing falls back.  The
default order alternates fused and generic twice: the difference between the two runs of one leg is the repeat-to-repeat spread the
comparison has to be read against.  The timed window of a leg is device-synchronised at both ends and at least --min_seconds long.
usage: python tools/multiscale_step.py [--steps K] [--warmup W] [--out FILE] [leg ...]    legs: fused generic lstm kernels"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {
    "fused": ("MultiscaleCnnLstmModel", "1"),
    "generic": ("MultiscaleCnnLstmModel", "0"),
    "lstm": ("LstmModel", "1"),
    "kernels": (None, "1"),
}
DEFAULT_ORDER = ["fused", "generic", "fused", "generic", "lstm", "kernels"]
HBM_PEAK_TBS, HBM_MEASURED_TBS, INFINITY_CACHE_MIB = 8.0, 6.3, 256     # MI355X: spec, float4 copy, last-level cache


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.load_package()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return torch, dev


def child_step(leg, steps, warmup, min_seconds):
    torch, dev = _setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    B, F, D, V = 128, 300, 1152, 4716
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers = "1024", 2
    FLAGS.multiscale_cnn_lstm_layers, FLAGS.moe_num_mixtures, FLAGS.is_training = 4, 4, True
    FLAGS.support_type, FLAGS.support_loss_percent = "label,label,label,label", 0.1
    multiscale = LEGS[leg][0] == "MultiscaleCnnLstmModel"
    g = reset_default_graph(device=dev, seed=0)
    kw = dict(label_loss_fn=losses.MultiTaskCrossEntropyLoss(), multitask=True) if multiscale else {}
    tg = train.TrainGraph(getattr(flm, LEGS[leg][0])(), batch_size=B, graph=g, **kw)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randint(0, 256, (B, F, D), device=dev, generator=gen, dtype=torch.uint8)
    nf = torch.randint(F // 2, F + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    calls = dict(seq_ops.NATIVE_CALLS)
    loss_first = None
    for _ in range(warmup):
        o = tg.step(x, y, nf)
        seq_ops.check_persist_errors()
        if loss_first is None:
            loss_first = float(o["loss"])
    native = seq_ops.NATIVE_CALLS["fwd"] - calls["fwd"]
    done, elapsed = 0, 0.0
    while elapsed < min_seconds:                                       # whole windows of `steps` steps until the window is long enough
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = tg.step(x, y, nf)
        torch.cuda.synchronize()
        elapsed += time.perf_counter() - t0
        done += steps
    seq_ops.check_persist_errors()
    finite = all(bool(torch.isfinite(v.data).all()) for v in g.trainable_variables())
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
    torch, dev = _setup()
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
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            L.check(fn())
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        rows.append(dict(kernel=name, us=round(us, 1), mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / us / 1e6, 2)))
    print(json.dumps(dict(leg="kernels", shape=[F, B, C], reps=reps, hbm_peak_tb_per_s=HBM_PEAK_TBS, hbm_measured_tb_per_s=HBM_MEASURED_TBS,
                          infinity_cache_mib=INFINITY_CACHE_MIB, tensor_mbytes=round(full / 1e6, 1), kernels=rows)), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min_seconds", type=float, default=1.0, help="shortest timed window of a leg")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child_kernels(50) if a.child == "kernels" else child_step(a.child, a.steps, a.warmup, a.min_seconds)
    rows = []
    for leg in a.legs or DEFAULT_ORDER:
        env = dict(os.environ, YT8M_MULTISCALE_FUSED=LEGS[leg][1])
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--min_seconds", str(a.min_seconds)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print("leg %s failed with exit status %d: stopping" % (leg, r.returncode), flush=True)
            return r.returncode or 1
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    by = {}
    for r in rows:
        if "ms_per_step" in r:
            by.setdefault(r["leg"], []).append(r["ms_per_step"])
    if "fused" in by and "generic" in by:
        spread = lambda v: round(max(v) - min(v), 3) if len(v) > 1 else None
        fused, generic = min(by["fused"]), min(by["generic"])
        summary = dict(fused_ms=by["fused"], generic_ms=by["generic"], fused_spread_ms=spread(by["fused"]),
                       generic_spread_ms=spread(by["generic"]), fused_over_generic=round(fused / generic, 3),
                       lstm_ms=by.get("lstm"), fused_default=max(by["fused"]) <= max(by["generic"]))
        print(json.dumps(summary), flush=True)
        rows.append(summary)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
