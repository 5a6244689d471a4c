"""CPU pin of the chain contract of the nine chain plugins (DESIGN_LOG.md section 25): the ORDER in which a plugin creates its variables
(Graph.get_variable draws every initial value from one generator and appends to one arena, so the order decides the weights and the
optimiser layout) and the ORDER of its native calls -- the random ones (ops.dropout, ops.add_noise, a noisy ops.chain_link) take the
graph's Philox keys in that order.  Every plugin is built once per case on a CPU graph with the native calls replaced by shape-only
stand-ins that append to ONE event list; the ordered variables, the events and the result's keys are compared with
tests/chain_order_expected.json, recorded before the nine loops became one driver (`python tests/test_chain_order_host.py --record`
rewrites that file: only for a change that means to move the contract).  Uses public class names and ops / seq_ops attributes only."""
import json
import os
import sys

import pytest
import torch

from conftest import ROOT

EXPECTED = os.path.join(ROOT, "tests", "chain_order_expected.json")
B, F, V, M, D = 4, 13, 5, 3, 16
RELU, DISTILL = 7, 6                                                      # --deep_chain_relu_cells, --distillchain_relu_cells
NF = [13, 1, 12, 5]
SPLIT = dict(feature_sizes="8,8", lstm_cells="8,4")                       # the plugins that split their input by feature
WHOLE = dict(lstm_cells="8")
NOISY = dict(dropout=True, keep_prob=0.9, noise_level=0.2)

# row of the design log's table -> (module, class, flags, needs distillation_predictions, frame-level)
PLUGINS = {
    1: ("video_level_models", "DeepCombineChainModel", {}, False, False),
    2: ("video_level_models", "DistillchainDeepCombineChainModel", {}, True, False),
    3: ("frame_level_models", "CnnDeepCombineChainModel", {}, False, True),
    4: ("frame_level_models", "DistillchainCnnDeepCombineChainModel", {}, True, True),
    5: ("frame_level_models", "LstmCnnDeepCombineChainModel", SPLIT, False, True),
    6: ("frame_level_models", "DistillchainLstmCnnDeepCombineChainModel", SPLIT, True, True),
    7: ("frame_level_models", "LstmMemoryDeepChainModel", WHOLE, False, True),
    8: ("frame_level_models", "DistillchainLstmMemoryDeepCombineChainModel", WHOLE, True, True),
    9: ("frame_level_models", "MultiresLstmMemoryDeepCombineChainModel", SPLIT, False, True),
}


def _cases():
    """id -> (row, uint8 input, extra flags, extra create_model arguments)."""
    import yt8m_amd.frame_level_models as flm
    cases = {}
    for row, (module, name, _, _, frames) in PLUGINS.items():
        cases["%d-float" % row] = (row, False, {}, {})
        cases["%d-scoped" % row] = (row, False, {}, dict(sub_scope="x-"))
        if frames and getattr(getattr(flm, name), "accepts_quantized_input", False):
            cases["%d-uint8" % row] = (row, True, {}, {})
    for row in (1, 2, 9):
        cases["%d-noisy" % row] = (row, False, {}, NOISY)
    for row in (1, 2):
        cases["%d-noise0" % row] = (row, False, {}, dict(NOISY, noise_level=0.0))
    cases["1-elu-pooled-grad"] = (1, False, dict(deep_chain_relu_type="elu"), dict(support_pool="halves", input_grad=True))
    cases["9-no-layers"] = (9, False, dict(deep_chain_layers=0), NOISY)
    cases["9-length-elu"] = (9, False, dict(deep_chain_use_length=True, deep_chain_relu_type="elu"), {})
    return cases


def _shape(t):
    return list(t.shape)


def _install(mp, events):
    """The native calls as shape-only stand-ins that append to `events`."""
    import yt8m_amd.ops as ops
    import yt8m_amd.seq_ops as seq_ops

    def stack(x_tm, num_frames, wb, **k):
        H = wb[0][0].data.shape[1] // 4
        events.append(["lstm_stack", wb[0][0].name.split("/multi_rnn_cell")[0], _shape(x_tm), k.get("slot", 0)])
        bytes_ = x_tm.dtype == torch.uint8                                # bytes arrive batch-major
        B_, T_ = (x_tm.shape[0], x_tm.shape[1]) if bytes_ else (x_tm.shape[1], x_tm.shape[0])
        return torch.zeros(T_, B_, H), [(torch.zeros(B_, H), torch.zeros(B_, H)) for _ in wb]

    def head(x, Wg, We, be, V_, M_, **k):
        events.append(["moe_head", x.shape[1], k.get("dx_from", 0)])
        return torch.zeros(x.shape[0], V_)

    def chain_link(z, kind="relu", noise_level=None, **k):
        events.append(["chain_link", _shape(z), kind, noise_level])
        return z

    def activation(x, kind):
        events.append(["activation", _shape(x), kind])
        return x

    def add_noise(x, stddev, **k):
        events.append(["add_noise", _shape(x), stddev])
        return x

    def dropout(x, keep_prob, **k):
        events.append(["dropout", _shape(x), keep_prob])
        return x

    def l2_normalize(x, eps=1e-12):
        events.append(["l2_normalize", _shape(x)])
        return x

    def memory_link(tensors, normalize, eps=1e-12):
        tensors = list(tensors)
        events.append(["memory_link", [t.shape[1] for t in tensors], bool(normalize)])
        return torch.zeros(tensors[0].shape[0], sum(t.shape[1] for t in tensors))

    def pyramid(x, num_frames, levels, widths, eps=1e-12):
        B_, F_, _ = x.shape
        return ([[torch.zeros(F_ >> (l + 1), B_, w) for w in widths] for l in range(levels)],
                [(num_frames // (2 << l)).to(torch.int32) for l in range(levels)])

    mp.setattr(seq_ops, "lstm_stack", stack)
    mp.setattr(seq_ops, "cnn_tm_maxpool", lambda x2d, B_, cnns: [torch.zeros(B_, sum(W.data.shape[1] for W in cnn)) for cnn in cnns])
    mp.setattr(ops, "moe_head", head)
    mp.setattr(ops, "chain_link", chain_link)
    mp.setattr(ops, "activation", activation)
    mp.setattr(ops, "add_noise", add_noise)
    mp.setattr(ops, "dropout", dropout)
    mp.setattr(ops, "l2_normalize", l2_normalize)
    mp.setattr(ops, "memory_link", memory_link)
    mp.setattr(ops, "frame_pyramid", pyramid)
    mp.setattr(ops, "linear", lambda x, W, b=None, bf16=None: torch.zeros(x.shape[:-1] + (W.data.shape[1],)))
    mp.setattr(ops, "frame_pool", lambda x, method: x.amax(1))
    mp.setattr(ops, "dequant_l2norm", lambda q, num_frames=None, eps=1e-12: torch.zeros(q.shape, dtype=torch.float32))


def _record(mp, case):
    """{"vars": [[name, shape]] in creation order, "events": the stand-ins' calls in order, "result": {key: shape}} of one case."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.video_level_models as vlm
    from yt8m_amd.flags import FLAGS
    from yt8m_amd.variables import reset_default_graph
    row, u8, extra_flags, kwargs = _cases()[case]
    module, name, plugin_flags, distill, frames = PLUGINS[row]
    kwargs = dict(kwargs)
    FLAGS.reset()
    try:
        FLAGS.deep_chain_layers, FLAGS.lstm_layers, FLAGS.moe_num_mixtures = 2, 1, M
        FLAGS.deep_chain_relu_cells, FLAGS.distillchain_relu_cells = RELU, DISTILL
        for k, v in dict(plugin_flags, **extra_flags).items():
            setattr(FLAGS, k, v)
        events = []
        _install(mp, events)
        shape = (B, F, D) if frames else (B, D)
        x = torch.zeros(shape, dtype=torch.uint8 if u8 else torch.float32, requires_grad=bool(kwargs.pop("input_grad", False)))
        if kwargs.get("support_pool") == "halves":                        # [B, V] -> [B / 2, V], as a caller that reduces rows would
            kwargs["support_pool"] = lambda p: p.view(B // 2, 2, V).amax(1)
        if frames:
            kwargs["num_frames"] = torch.tensor(NF)
        if distill:
            kwargs["distillation_predictions"] = torch.zeros(B, V)
        g = reset_default_graph(device=torch.device("cpu"), seed=0)
        res = getattr({"video_level_models": vlm, "frame_level_models": flm}[module], name)().create_model(
            x, vocab_size=V, unknown=1, **kwargs)
    finally:
        FLAGS.reset()
    return {"vars": [[k, list(v.data.shape)] for k, v in g.vars.items()], "events": events,
            "result": {k: _shape(v) for k, v in res.items()}}


def _expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones():
    cases = _cases()
    assert sorted(cases) == sorted(_expected())
    assert {c[0] for c in cases.values()} == set(range(1, 10))           # all nine rows
    assert {"%d-uint8" % r for r in range(3, 9)} <= set(cases) and "9-uint8" not in cases


@pytest.mark.parametrize("case", sorted(_cases()))
def test_creation_order_native_call_order_and_result_keys(monkeypatch, case):
    want = _expected()[case]
    got = json.loads(json.dumps(_record(monkeypatch, case)))              # tuples and floats as the file holds them
    assert got["vars"] == want["vars"]
    assert got["events"] == want["events"]
    assert list(got["result"].items()) == list(want["result"].items())


def _dump(obj):
    """One variable / event per line."""
    out = ["{"]
    for i, (case, rec) in enumerate(sorted(obj.items())):
        out.append(' %s: {' % json.dumps(case))
        for key in ("vars", "events"):
            out.append('  "%s": [' % key)
            out.extend("   %s%s" % (json.dumps(item), "," if j + 1 < len(rec[key]) else "") for j, item in enumerate(rec[key]))
            out.append("  ],")
        out.append('  "result": %s' % json.dumps(rec["result"]))
        out.append(" }" + ("," if i + 1 < len(obj) else ""))
    out.append("}")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_chain_order_host.py --record"
    recorded = {}
    for case_id in _cases():
        with pytest.MonkeyPatch.context() as mp_:
            recorded[case_id] = _record(mp_, case_id)
    with open(EXPECTED, "w") as f:
        f.write(_dump(recorded))
    print("recorded %d cases" % len(recorded))
