"""ms / step of the bidirectional LSTM plugins at the bench's frame-level shape (B = 128, F = 300, D = 1152 uint8 frames, H = 1024, L = 2,
MoE head, fp32 step with clip + Adam): LstmModel, BiLstmModel with the two directions one after the other and overlapped
(YT8M_BI_OVERLAP), BiUniLstmModel.  Every leg runs in a child process of its own under its own time limit; the driver stops at the
first leg that fails.  The persistent recurrences' sticky time-out words (seq_ops.check_persist_errors) are read after every warm-up
step and once after the timed steps (the words are sticky: a time-out in any of them is still reported; a read per timed step would
put a synchronisation into the timing); after the last step every parameter must be finite.  `loss_first` is the loss of the first
step; `loss` the last one's -- on these uniform-noise frames with fixed labels the MoE head saturates within the warm-up, and the last
loss comes out the same for every model (the positives' -log(eps) average), so it is no evidence about the model.
usage: python tools/bilstm_step.py [--steps K] [--warmup W] [--out FILE] [leg ...]    legs: lstm bilstm_seq bilstm_overlap biuni"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {
    "lstm": ("LstmModel", "0"),
    "bilstm_seq": ("BiLstmModel", "0"),
    "bilstm_overlap": ("BiLstmModel", "1"),
    "biuni": ("BiUniLstmModel", "0"),
}


def child(leg, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.load_package()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, F, D, V = 128, 300, 1152, 4716
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers = "1024", 2
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(getattr(flm, LEGS[leg][0])(), batch_size=B, graph=g)
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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tg.step(x, y, nf)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    seq_ops.check_persist_errors()
    finite = all(bool(torch.isfinite(v.data).all()) for v in g.trainable_variables())
    print(json.dumps(dict(leg=leg, model=LEGS[leg][0], overlap=LEGS[leg][1] == "1", ms_per_step=round(ms, 3), steps=steps, warmup=warmup,
                          loss_first=loss_first, loss=float(out["loss"]), params_finite=finite, native_stacks_per_step=native / max(warmup, 1),
                          overlap_runs=seq_ops.BI_OVERLAP_RUNS[0])), flush=True)
    return 0 if finite else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    rows = []
    for leg in a.legs or list(LEGS):
        env = dict(os.environ, YT8M_BI_OVERLAP=LEGS[leg][1])
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print("leg %s failed with exit status %d: stopping" % (leg, r.returncode), flush=True)
            return r.returncode or 1
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    by = {r["leg"]: r["ms_per_step"] for r in rows}
    if "lstm" in by and "bilstm_seq" in by and "bilstm_overlap" in by:
        summary = dict(bilstm_seq_over_lstm=round(by["bilstm_seq"] / by["lstm"], 3),
                       bilstm_overlap_over_lstm=round(by["bilstm_overlap"] / by["lstm"], 3),
                       overlap_default=by["bilstm_overlap"] < by["bilstm_seq"])
        print(json.dumps(summary), flush=True)
        rows.append(summary)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
