"""ms / step of the bidirectional LSTM plugins at the bench's frame-level shape (B = 128, F = 300, D = 1152 uint8 frames, H = 1024, L = 2,
MoE head, fp32 step with clip + Adam): LstmModel, BiLstmModel with the two directions one after the other and overlapped
(YT8M_BI_OVERLAP), BiUniLstmModel.  Every leg runs in a child process of its own under its own time limit; the driver stops at the
first leg that fails.  The persistent recurrences' sticky time-out words (seq_ops.check_persist_errors) are read after every warm-up
step and once after the timed steps (the words are sticky: a time-out in any of them is still reported; a read per timed step would
put a synchronisation into the timing); after the last step every parameter must be finite.  `loss_first` is the loss of the first
step; `loss` the last one's -- on these uniform-noise frames with fixed labels the MoE head saturates within the warm-up, and the last
loss comes out the same for every model (the positives' -log(eps) average), so it is no evidence about the model.
usage: python tools/bilstm_step.py [--steps K] [--warmup W] [--out FILE] [leg ...]    legs: lstm bilstm_seq bilstm_overlap biuni"""
import json
import sys

import steplib

LEGS = {
    "lstm": ("LstmModel", "0"),
    "bilstm_seq": ("BiLstmModel", "0"),
    "bilstm_overlap": ("BiLstmModel", "1"),
    "biuni": ("BiUniLstmModel", "0"),
}


def child(leg, steps, warmup):
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    B, F = 128, 300
    FLAGS.reset()
    FLAGS.lstm_cells, FLAGS.lstm_layers = "1024", 2
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(getattr(flm, LEGS[leg][0])(), batch_size=B, graph=g)
    x, y, nf, _ = steplib.random_batch(dev, B, F)
    calls = dict(seq_ops.NATIVE_CALLS)
    loss_first = steplib.warm_up(lambda: tg.step(x, y, nf), warmup, seq_ops.check_persist_errors)
    native = seq_ops.NATIVE_CALLS["fwd"] - calls["fwd"]
    out, elapsed, _ = steplib.timed_steps(lambda: tg.step(x, y, nf), steps)
    seq_ops.check_persist_errors()
    finite = steplib.params_finite(g)
    print(json.dumps(dict(leg=leg, model=LEGS[leg][0], overlap=LEGS[leg][1] == "1", ms_per_step=round(elapsed / steps * 1e3, 3), steps=steps,
                          warmup=warmup, loss_first=loss_first, loss=float(out["loss"]), params_finite=finite,
                          native_stacks_per_step=native / max(warmup, 1), overlap_runs=seq_ops.BI_OVERLAP_RUNS[0])), flush=True)
    return 0 if finite else 1


def summarise(rows):
    by = {r["leg"]: r["ms_per_step"] for r in rows}
    if not ("lstm" in by and "bilstm_seq" in by and "bilstm_overlap" in by):
        return rows
    return rows + [dict(bilstm_seq_over_lstm=round(by["bilstm_seq"] / by["lstm"], 3),
                        bilstm_overlap_over_lstm=round(by["bilstm_overlap"] / by["lstm"], 3),
                        overlap_default=by["bilstm_overlap"] < by["bilstm_seq"])]


def parser():
    return steplib.arg_parser(steps=20, warmup=3, timeout=300)


def main():
    a = steplib.parse_args(parser(), list(LEGS))
    if a.child:
        return child(a.child, a.steps, a.warmup)
    return steplib.drive(__file__, a.legs or list(LEGS), steplib.child_args(a), a.timeout, a.out,
                         env_of=lambda leg: {"YT8M_BI_OVERLAP": LEGS[leg][1]}, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
