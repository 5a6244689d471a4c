"""ms / step of LstmCnnDeepCombineChainModel at its training script's shape (W/training_scripts/run-chaining-lstm-cnn.sh: B = 128, F = 300,
D = 1152 uint8 frames, all 300 frames, cells 1024 | 128, one layer, 3 chain layers of 128 relu cells, 4 mixtures, multitask loss with
label supports; fp32 step with clip + Adam).  Legs: pooled (the package's form: one op for the chain whose backward gathers,
seq_ops.cnn_tm_maxpool), pooled_chain (the same with ONE set of products for the whole chain instead of one per CNN), composed
(frame_level_models._pooled_cnn_chain replaced by seq_ops.cnn_tm + a max over the frames: the price of this function when built from the
other plugins' ops), parallel (LstmParallelFinaloutputModel with the same cells, for context), kernels (the two gather kernels alone:
device-event times, the bytes their shapes imply, the resulting TB/s).  Every leg runs in a child process of its own under its own time
limit; the driver stops at the first leg that fails; without a GPU a leg fails, nothing falls back.  The default order alternates pooled
and composed twice: the difference between the two runs of one leg is the repeat-to-repeat spread the comparison has to be read against.
The timed window of a leg is device-synchronised at both ends and at least --min_seconds long.
usage: python tools/lstmcnn_step.py [--steps K] [--warmup W] [--out FILE] [leg ...]    legs: pooled pooled_chain composed parallel kernels"""
import json
import sys

import steplib

LEGS = {
    "pooled": "LstmCnnDeepCombineChainModel",
    "pooled_chain": "LstmCnnDeepCombineChainModel",
    "composed": "LstmCnnDeepCombineChainModel",
    "parallel": "LstmParallelFinaloutputModel",
    "kernels": None,
}
DEFAULT_ORDER = ["pooled", "composed", "pooled", "composed", "pooled_chain", "parallel", "kernels"]
B, F, D = 128, 300, 1152
CHAIN = [[(1, 128), (2, 256), (3, 128)]] + [[(1, 128), (2, 128), (3, 256)]] * 3          # (filter length, columns) per CNN, c = 128


def gather_bytes(B_, F_, D_, chain):
    """Bytes from shapes.  Both kernels gather one D-float row per (video, column, shift): rows of x for dw (one call per filter), rows
    of the transposed filters for dx; dw also writes the filters' gradients, dx its [F B, D] output; g and idx are read once each."""
    terms = sum(fs * n for cnn in chain for fs, n in cnn)
    cols = sum(n for cnn in chain for _, n in cnn)
    rows = 4.0 * B_ * terms * D_
    return dict(dw=rows + 4.0 * terms * D_ + 8.0 * B_ * terms, dx=rows + 4.0 * F_ * B_ * D_ + 8.0 * B_ * cols)


def child_step(leg, steps, warmup, min_seconds):
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses as losses
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    FLAGS.reset()
    FLAGS.feature_sizes, FLAGS.lstm_cells, FLAGS.lstm_layers = "1024,128", "1024,128", 1
    FLAGS.deep_chain_layers, FLAGS.deep_chain_relu_cells, FLAGS.moe_num_mixtures = 3, 128, 4
    FLAGS.support_type, FLAGS.support_loss_percent = "label,label,label", 0.05
    if leg == "composed":
        def composed(out_tm, cnns):
            F_, B_, D_ = out_tm.shape
            x = out_tm.reshape(F_ * B_, D_)
            return [seq_ops.cnn_tm(x, B_, cnn).view(F_, B_, -1).amax(0) for cnn in cnns]
        flm._pooled_cnn_chain = composed
    seq_ops.CNN_POOL_WHOLE_CHAIN = leg == "pooled_chain"
    chain = LEGS[leg] == "LstmCnnDeepCombineChainModel"
    g = reset_default_graph(device=dev, seed=0)
    kw = dict(label_loss_fn=losses.MultiTaskCrossEntropyLoss(), multitask=True) if chain else {}
    tg = train.TrainGraph(getattr(flm, LEGS[leg])(), batch_size=B, graph=g, **kw)
    x, y, nf, _ = steplib.random_batch(dev, B, F, "all")                  # all 300 frames
    calls = dict(seq_ops.NATIVE_CALLS)
    loss_first = steplib.warm_up(lambda: tg.step(x, y, nf), warmup, seq_ops.check_persist_errors)
    native = seq_ops.NATIVE_CALLS["fwd"] - calls["fwd"]
    out, elapsed, done = steplib.timed_steps(lambda: tg.step(x, y, nf), steps, min_seconds)
    seq_ops.check_persist_errors()
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model=LEGS[leg], ms_per_step=round(elapsed / done * 1e3, 3), steps=done, warmup=warmup,
                          window_s=round(elapsed, 3), loss_first=loss_first, loss=float(out["loss"]), params_finite=finite,
                          native_stacks_per_step=native / max(warmup, 1))), flush=True)
    return 0 if finite else 1


def child_kernels(reps):
    """yt8m_f32_cnn_pool_dw (the 12 calls of one backward pass, timed together) and yt8m_f32_cnn_pool_dx (one call) at the script's
    shape on random argmax frames.  Both are gathers from L2 / Infinity Cache, not streams: the [F B, 1152] fp32 operand of dw is 177 MB
    (it does not fit the cache whole), the transposed filters of dx 21 MB (they do)."""
    import torch
    dev = steplib.setup()
    import ctypes
    import yt8m_amd._lib as L
    lib = L.lib()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = [s for cnn in CHAIN for s in cnn]
    Ntot = sum(n for _, n in shapes)
    x = torch.randn(F * B, D, device=dev)
    g = torch.randn(B, Ntot, device=dev)
    idx = torch.randint(0, F, (B, Ntot), device=dev, dtype=torch.int32)
    Ws = [torch.randn(fs * D, n, device=dev) * 0.1 for fs, n in shapes]
    dWs = [torch.empty_like(W) for W in Ws]
    wts = [W.t().contiguous() for W in Ws]
    n = len(shapes)
    wt = (ctypes.c_void_p * n)(*[t.data_ptr() for t in wts])
    fsa = (ctypes.c_int32 * n)(*[fs for fs, _ in shapes])
    nca = (ctypes.c_int32 * n)(*[nc for _, nc in shapes])
    dx = torch.empty(F * B, D, device=dev)

    def dw_all():
        c0, rc = 0, 0
        for (fs, N), dW in zip(shapes, dWs):
            rc |= lib.yt8m_f32_cnn_pool_dw(p(x), D, p(idx, c0), p(g, c0), Ntot, B, F, D, N, fs, p(dW), N, 0.0, st())
            c0 += N
        return rc

    nbytes = gather_bytes(B, F, D, CHAIN)
    cases = {"f32_cnn_pool_dw x12": (nbytes["dw"], dw_all),
             "f32_cnn_pool_dx": (nbytes["dx"], lambda: lib.yt8m_f32_cnn_pool_dx(p(idx), p(g), Ntot, B, F, D, n, wt, fsa, nca, p(dx), D, st()))}
    rows = []
    for name, (nb, fn) in cases.items():
        for _ in range(3):
            L.check(fn())
        us = steplib.events_us(lambda: L.check(fn()), reps)
        rows.append(dict(kernel=name, us=round(us, 1), mbytes=round(nb / 1e6, 1), tb_per_s=round(nb / us / 1e6, 2)))
    print(json.dumps(dict(leg="kernels", shape=[F, B, D], columns=Ntot, reps=reps, kernels=rows)), flush=True)
    return 0


def summarise(rows):
    by = steplib.ms_by_leg(rows)
    if not ("pooled" in by and "composed" in by):
        return rows
    spread = lambda v: round(max(v) - min(v), 3) if len(v) > 1 else None
    sp, sc = spread(by["pooled"]), spread(by["composed"])
    gain = min(by["composed"]) - max(by["pooled"])                     # the smallest difference any pairing of the runs shows
    return rows + [dict(pooled_ms=by["pooled"], composed_ms=by["composed"], pooled_spread_ms=sp, composed_spread_ms=sc,
                        pooled_over_composed=round(min(by["pooled"]) / min(by["composed"]), 3), pooled_chain_ms=by.get("pooled_chain"),
                        parallel_ms=by.get("parallel"), pooled_faster_beyond_spread=bool(gain > max(sp or 0.0, sc or 0.0)))]


def parser():
    ap = steplib.arg_parser(steps=10, warmup=3, timeout=300)
    ap.add_argument("--min_seconds", type=float, default=1.0, help="shortest timed window of a leg")
    return ap


def main():
    a = steplib.parse_args(parser(), list(LEGS))
    if a.child:
        return child_kernels(20) if a.child == "kernels" else child_step(a.child, a.steps, a.warmup, a.min_seconds)
    return steplib.drive(__file__, a.legs or DEFAULT_ORDER, steplib.child_args(a, "min_seconds"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
