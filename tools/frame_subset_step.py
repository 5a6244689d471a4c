"""Random half-frame inference (ops.frame_subset, csrc/frame_subset.hip) and the two inference plugins on it at the scripts' shapes.
`op`: the draw and the gather of ops.frame_subset, the gather kernel against the composed form (the YT8M_FRAME_SUBSET_FUSED=0 form:
index_select, a comparison and a sum, a multiply; the draw is the same launch in both), at [B, F, D, E] = [32,300,1152,16] on bytes
(Z/infer_scripts/infer-lstm_random_mean_moe8.sh), [32,300,1152,8] on bytes (infer-lstm_attention_max_mean.sh), [128,300,1152,1] on bytes
(a training step of LstmRandomModel under --lstm_random_frames) and [32,300,1152,16] on floats: hip events around back-to-back calls,
the two forms alternating inside every repeat, the results compared bit for bit.  The driver adds an `op_summary` row: whether the
kernels' median was below the composed one at every shape in every run of the leg -- what decides the default.
`kernels`: yt8m_frame_subset_draw and yt8m_frame_subset_gather_* alone through the C ABI at the same shapes, with the bytes each has to
move (draw: the index written; gather: the chosen real frames read, every output row written, the index and num_frames read, the counts
written) and the rate in TB/s -- also with every source frame counted once, however many replicas chose it: the re-reads are cache hits.
`predict`: whole TrainGraph.predict calls at B = 32, F = 300 on the reader's bytes under the scripts' flags (1024 cells, 2 layers, 8
mixtures): FrameRandomEvalModel with E = 16 and FrameAttentionEvalModel (MoeExtendModel head) with E = 8, each with the switch on and
off, and LstmMemoryModel.predict on a pre-gathered [512,150,1152] batch in the same run as the yardstick: FrameRandomEvalModel minus
the yardstick is what the selection (and the mean) costs.
Every leg runs twice, each run in a child process of its own under its own time limit; the driver stops at the first leg that fails.
usage: python tools/frame_subset_step.py [--steps K] [--warmup W] [--repeats N] [--out FILE] [leg ...]      legs: op kernels predict"""
import ctypes
import json
import sys

import steplib

SHAPES = ((32, 300, 1152, 16, "uint8"), (32, 300, 1152, 8, "uint8"), (128, 300, 1152, 1, "uint8"), (32, 300, 1152, 16, "float32"))
B, F, D = 32, 300, 1152
SEED = 7


def _inputs(dev, shape):
    """Frames as the reader pads them (zeros past num_frames) and num_frames in F // 2 .. F"""
    import torch
    B_, F_, D_, E_, dtype = shape
    q, _, nf, gen = steplib.random_batch(dev, B_, F_, "half", D=D_)
    live = (torch.arange(F_, device=dev)[None, :] < nf[:, None])[:, :, None]
    if dtype == "uint8":
        return q * live.to(torch.uint8), nf
    return torch.randn((B_, F_, D_), device=dev, generator=gen) * live.to(torch.float32), nf


def op(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd.ops as ops
    for shape in SHAPES:
        B_, F_, D_, E_, dtype = shape
        x, nf = _inputs(dev, shape)

        def run(fused):
            ops.FRAME_SUBSET_FUSED = fused
            return ops.frame_subset(x, nf, E_, seed=SEED)

        forms = {"fused": lambda: run(True), "composed": lambda: run(False)}
        us = steplib.alternate(forms, iters, repeats)
        rf, rc = forms["fused"](), forms["composed"]()
        ops.FRAME_SUBSET_FUSED = False
        f_, c_ = steplib.median(us["fused"]), steplib.median(us["composed"])
        print(json.dumps(dict(
            leg="op", B=B_, F=F_, D=D_, E=E_, K=F_ // 2, dtype=dtype, what="draw + gather (ops.frame_subset)",
            output_bytes=rf[0].numel() * rf[0].element_size(),
            **steplib.spread_fields("fused", us["fused"], "us"), **steplib.spread_fields("composed", us["composed"], "us"),
            composed_over_fused=round(c_ / f_, 2), fused_below_composed=bool(f_ < c_),
            bit_equal_fused_composed=bool(all(torch.equal(a, b) for a, b in zip(rf, rc))), empty_replicas=int((rf[1] == 0).sum()),
            calls=dict(ops.FRAME_SUBSET_CALLS), repeats=repeats,
            timing="hip events over %d back-to-back calls (torch allocations included), median of the repeats" % iters)), flush=True)
        del x, nf, rf, rc
        torch.cuda.empty_cache()
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    return 0


def kernels(iters, repeats):
    import torch
    dev = steplib.setup()
    import yt8m_amd._lib as L
    lib = L.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shape in SHAPES:
        B_, F_, D_, E_, dtype = shape
        K_ = F_ // 2
        x, nf = _inputs(dev, shape)
        index = torch.empty((E_, K_), dtype=torch.int32, device=dev)
        y = torch.empty((B_ * E_, K_, D_), dtype=x.dtype, device=dev)
        nf_out = torch.empty((B_ * E_,), dtype=torch.int32, device=dev)
        fn = lib.yt8m_frame_subset_gather_u8 if dtype == "uint8" else lib.yt8m_frame_subset_gather_f32
        draw = lambda: L.check(lib.yt8m_frame_subset_draw(p(index), E_, F_, K_, SEED, st()))
        gather = lambda: L.check(fn(p(x), p(nf), p(index), p(y), p(nf_out), B_, F_, D_, E_, K_, st()))
        draw()
        gather()
        torch.cuda.synchronize()
        row_bytes = D_ * x.element_size()
        small = 4 * (E_ * K_ + B_ + B_ * E_)
        nbytes_of = {"draw": 4 * E_ * K_, "gather": (int(nf_out.sum()) + B_ * E_ * K_) * row_bytes + small}
        # a real frame that several replicas chose is fetched from memory once and served from cache afterwards
        live = (index.view(E_, 1, K_) < nf.view(1, B_, 1))
        seen = torch.zeros((B_, F_), dtype=torch.bool, device=dev)
        seen[torch.arange(B_, device=dev).view(1, B_, 1).expand(E_, B_, K_)[live], index.view(E_, 1, K_).expand(E_, B_, K_)[live].long()] = True
        unique_of = {"draw": 4 * E_ * K_, "gather": (int(seen.sum()) + B_ * E_ * K_) * row_bytes + small}
        us = steplib.alternate({"draw": draw, "gather": gather}, iters, repeats)
        for k, val in us.items():
            med = steplib.median(val)
            print(json.dumps(dict(leg="kernels", kernel=k, B=B_, F=F_, D=D_, E=E_, K=K_, dtype=dtype, bytes=nbytes_of[k],
                                  bytes_each_source_frame_once=unique_of[k], **steplib.spread_fields("call", val, "us"),
                                  TB_per_s=round(nbytes_of[k] / med / 1e6, 4), TB_per_s_each_source_frame_once=round(unique_of[k] / med / 1e6, 4),
                                  measured_streaming_read_TB_per_s="6.0-6.3",
                                  timing="hip events over %d back-to-back calls through the C ABI" % iters)), flush=True)
        del x, nf, index, y, nf_out
        torch.cuda.empty_cache()
    return 0


def predict(steps, warmup, repeats):
    import numpy as np
    import torch
    dev = steplib.setup()
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops
    import yt8m_amd.train as train
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    x, nf = _inputs(dev, (B, F, D, 1, "uint8"))
    E_RANDOM, E_ATTENTION = 16, 8
    ops.FRAME_SUBSET_FUSED = True
    xg, nfg, _ = ops.frame_subset(x, nf, E_RANDOM, seed=SEED)              # the yardstick's batch: [512,150,1152] bytes, gathered once
    ops.FRAME_SUBSET_FUSED = False
    plugins = {"FrameRandomEvalModel": dict(moe_num_extend=E_RANDOM, video_level_classifier_model="MoeModel"),
               "FrameAttentionEvalModel": dict(moe_num_extend=E_ATTENTION, video_level_classifier_model="MoeExtendModel"),
               "LstmMemoryModel": dict(video_level_classifier_model="MoeModel")}

    def flags_for(name):
        FLAGS.reset()
        FLAGS.batch_size = B
        fl = dict(lstm_cells="1024", lstm_layers=2, moe_num_mixtures=8, **plugins[name])
        for k, v in fl.items():
            setattr(FLAGS, k, v)
        return fl

    graphs, flags_of = {}, {}
    for name in plugins:
        flags_of[name] = flags_for(name)
        graphs[name] = train.build_graph(getattr(flm, name)(), batch_size=B, graph=reset_default_graph(device=dev, seed=0))
    forms = {"random_fused": ("FrameRandomEvalModel", True, (x, nf)), "random_composed": ("FrameRandomEvalModel", False, (x, nf)),
             "attention_fused": ("FrameAttentionEvalModel", True, (x, nf)), "attention_composed": ("FrameAttentionEvalModel", False, (x, nf)),
             "lstm_memory_pregathered": ("LstmMemoryModel", False, (xg, nfg))}
    last = {}

    def run(form, n):
        which, fused, batch = forms[form]
        flags_for(which)
        ops.FRAME_SUBSET_FUSED = fused
        for _ in range(n):
            last[form] = graphs[which].predict(*batch)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()

    for k in forms:
        run(k, warmup)
    ms = steplib.steps_in_turn(run, forms, steps, repeats)
    ops.FRAME_SUBSET_FUSED = False
    FLAGS.reset()
    finite = {k: bool(torch.isfinite(v).all()) and tuple(v.shape)[0] == (512 if k == "lstm_memory_pregathered" else B) for k, v in last.items()}
    row = dict(leg="predict", B=B, F=F, input="uint8 [32,300,1152]", yardstick_input="uint8 [512,150,1152]", flags=flags_of, steps=steps,
               warmup=warmup, repeats=repeats, finite_and_shaped=finite, calls=dict(ops.FRAME_SUBSET_CALLS),
               timing="host clock around the predict calls of one form, ending in a device synchronise; forms in turn inside every repeat")
    for k, v in ms.items():
        row.update(steplib.spread_fields(k, v, "ms"))
    med = {k: steplib.median(v) for k, v in ms.items()}
    row["random_fused_minus_yardstick_ms"] = round(med["random_fused"] - med["lstm_memory_pregathered"], 3)
    row["random_composed_minus_yardstick_ms"] = round(med["random_composed"] - med["lstm_memory_pregathered"], 3)
    print(json.dumps(row), flush=True)
    return 0 if all(finite.values()) and np.isfinite(list(med.values())).all() else 1


def summarise(rows):
    return steplib.verdict_after(rows, "op", "leg_repeat", "the kernels are the default only if this holds over two runs of the leg")


def parser():
    ap = steplib.arg_parser(steps=5, warmup=2, timeout=420)
    ap.add_argument("--repeats", type=int, default=5, help="timing repeats inside every leg")
    ap.add_argument("--op_iters", type=int, default=20)
    return ap


def main():
    a = steplib.parse_args(parser(), ["op", "kernels", "predict"])
    if a.child == "op":
        return op(a.op_iters, a.repeats)
    if a.child == "kernels":
        return kernels(a.op_iters, a.repeats)
    if a.child == "predict":
        return predict(a.steps, a.warmup, a.repeats)
    legs = a.legs or ["op", "op", "kernels", "kernels", "predict", "predict"]           # every leg twice; the op leg's verdict wants both runs
    plan = steplib.numbered(steplib.numbered(legs, "op", "leg_repeat"), "kernels", "run")
    plan = steplib.numbered(plan, "predict", "run")
    return steplib.drive(__file__, plan, steplib.child_args(a, "repeats", "op_iters"), a.timeout, a.out, summarise=summarise)


if __name__ == "__main__":
    sys.exit(main())
