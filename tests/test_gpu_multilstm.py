"""The fused memory-link kernel (csrc/memory_link.hip) and the three multi-LSTM plugins on the MI355X: the kernels through the C ABI
against an fp64 restatement written here, ops.memory_link fused against composed, the plugins through the plugin surface against fp64
restatements assembled from oracle.torch_ref (lstm_stack, moe, cross_entropy), and whole training steps with their bitwise replay."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.variables import reset_default_graph

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-12))         # what the kernel receives: the float32 nearest 1e-12
GUARD = -7.0


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the link in torch on the CPU, in the dtype of its inputs -------------------------------------------------------------------------
def _link_fwd_ref(x):
    """(y, rinv) of the concatenated rows x: ss = sum x^2, r = rsqrt(max(ss, eps)), y = x r, rinv = r where ss > eps else -r."""
    ss = (x * x).sum(1, keepdim=True)
    eps = torch.tensor(EPS, dtype=x.dtype)
    r = 1.0 / torch.sqrt(torch.maximum(ss, eps))
    return x * r, torch.where(ss > eps, r, -r).squeeze(1)


def _link_bwd_ref(y, rinv, g):
    """d from the output: R (g - y (y.g)) where rinv > 0 else R g, R = |rinv|."""
    R = rinv.abs()[:, None]
    k = (y * g).sum(1, keepdim=True)
    return torch.where(rinv[:, None] > 0, R * (g - y * k), R * g)


def _bound(ref32, ref64):
    """4 x the error of the float32 restatement against the fp64 one, plus one float32 ulp of the largest reference magnitude."""
    big = float(ref64.abs().max()) if ref64.numel() else 0.0
    return 4.0 * float((ref32.double() - ref64).abs().max()) + float(np.spacing(np.float32(big)))


def _case(rows, widths, seed):
    """The concatenated rows x [rows, sum widths] with row 0 all zero (ss = 0: the eps branch) and row 1 scaled to |x| ~ 1e-8 (0 < ss <
    eps); dy ~ N(0, 1) except on these two rows, where it is scaled by 1e-6: the eps branch multiplies it by 1e6, and a per-case bound
    that adds an ulp of the LARGEST magnitude (and 4 x the restatement's error there) would otherwise stop checking the other rows."""
    gen = torch.Generator().manual_seed(seed)
    C = sum(widths)
    x = torch.randn(rows, C, generator=gen)
    x[0] = 0.0
    x[1] *= 1e-8
    g = torch.randn(rows, C, generator=gen)
    g[:2] *= 1e-6
    return x, g


def _refs(x, g):
    """{name: (float32 restatement, fp64 restatement)} for y, d, rinv."""
    y64, r64 = _link_fwd_ref(x.double())
    y32, r32 = _link_fwd_ref(x)
    return {"y": (y32, y64), "d": (_link_bwd_ref(y32, r32, g), _link_bwd_ref(y64, r64, g.double())), "rinv": (r32, r64)}


CASES = [(3, [5]),                       # partial wave, scalar path
         (5, [7, 6]),                    # scalar path, segment boundary off a 16-byte line
         (7, [100]),                     # aligned path with a tail pass
         (4, [512, 512]),                # the register-resident limit (1024 columns) ...
         (2, [1024, 4]),                 # ... and the two-read loop one 16-byte step above it
         (3, [1024, 4]),                 # (the same with a row that is divided by its own norm: the loop's sum is checked numerically)
         (3, [1022, 3]),                 # the scalar two-read loop, one column above the limit
         (130, [8, 8]),                  # many workgroups
         (3, [1024, 128, 1024, 128]),    # the parallel model's layout
         (3, [4] * 16)]                  # the nseg limit


def _buffers(rows, widths, dev):
    return [torch.full((rows * w + 8,), GUARD, device=dev) for w in widths]


def _run_bwd(lib, widths, normalize, yd, rd, gd, bufs, rows, skip=()):
    n = len(widths)
    dsrc = (ctypes.c_void_p * n)(*[None if s in skip else bufs[s].data_ptr() for s in range(n)])
    L.check(lib.yt8m_memory_link_bwd(n, (ctypes.c_int64 * n)(*widths), normalize, _p(yd), _p(rd), _p(gd), dsrc, rows, EPS, _st()))


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("rows,widths", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) and len(v) < 5 else None)
def test_memory_link_kernels_against_the_fp64_restatement(dev, rows, widths, normalize):
    """yt8m_memory_link_fwd / _bwd through ctypes.  normalize = 1: per case and per output the bound is 4 x the largest error of the float32
    CPU restatement of the same formulas against the fp64 one on the same inputs (never the kernel's output) + one float32 ulp of the
    largest reference magnitude; rinv is bounded per branch (1e6 next to ~0.1) and its signs are exact; the backward kernel reads the
    forward kernel's y and rinv, as the op does.  normalize = 0: exact copies both ways.  Guard words behind every output keep their
    sentinel; a NULL dsrc entry leaves that segment's buffer untouched and the others bit-identical."""
    lib = L.lib()
    n, C = len(widths), sum(widths)
    x, g = _case(rows, widths, 100 * rows + C)
    offs = np.concatenate([[0], np.cumsum(widths)])
    srcs = [x[:, offs[s]:offs[s + 1]].contiguous().to(dev) for s in range(n)]
    gd = g.to(dev)
    yd = torch.full((rows * C + 8,), GUARD, device=dev)
    rd = torch.full((rows + 8,), GUARD, device=dev)
    L.check(lib.yt8m_memory_link_fwd(n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs]), (ctypes.c_int64 * n)(*widths), normalize,
                                     _p(yd), _p(rd), rows, EPS, _st()))
    bufs = _buffers(rows, widths, dev)
    _run_bwd(lib, widths, normalize, yd, rd, gd, bufs, rows)
    skipped = _buffers(rows, widths, dev)
    _run_bwd(lib, widths, normalize, yd, rd, gd, skipped, rows, skip=(0,))
    torch.cuda.synchronize()
    assert bool((yd[rows * C:] == GUARD).all()) and bool((rd[rows if normalize else 0:] == GUARD).all())
    for s, w in enumerate(widths):
        assert bool((bufs[s][rows * w:] == GUARD).all()) and bool((skipped[s][rows * w:] == GUARD).all())
        assert torch.equal(skipped[s], bufs[s]) if s else bool((skipped[s] == GUARD).all())      # NULL: nothing written
    y = yd[:rows * C].view(rows, C).cpu()
    d = torch.cat([bufs[s][:rows * w].view(rows, w).cpu() for s, w in enumerate(widths)], 1)
    if not normalize:
        assert torch.equal(y, x) and torch.equal(d, g)
        return
    rinv = rd[:rows].cpu()
    refs = _refs(x, g)
    r64 = refs["rinv"][1]
    assert torch.equal(rinv > 0, r64 > 0)                                 # the eps branch, exactly
    for r32, ref in refs.values():                                        # no bound collapses to its ulp term (checked on the CPU when the
        assert float((r32.double() - ref).abs().max()) > 0                # cases were fixed): the restatements differ on every output
    # all rows, then the rows that are divided by their own norm by themselves: the two eps rows carry O(1) values in d (1e6 x 1e-6 dy)
    # next to the others' ~0.1 / sqrt(C), and their rounding would otherwise be most of the bound of every row
    for sel, tag in ((slice(None), "all rows"), (slice(2, None), "rows >= 2")):
        for name, got in (("y", y), ("d", d)):
            r32, ref = refs[name]
            if ref[sel].numel() == 0:
                continue
            b, e = _bound(r32[sel], ref[sel]), float((got[sel].double() - ref[sel]).abs().max())
            print("(%d; %s) %s %s err %.3g (bound %.3g)" % (rows, widths, tag, name, e, b))
            assert e <= b, (name, tag)
    for branch in (r64 > 0, r64 <= 0):
        if bool(branch.any()):
            b_r = _bound(refs["rinv"][0][branch], r64[branch])
            e_r = float((rinv[branch].double() - r64[branch]).abs().max())
            print("    rinv %s: err %.3g (bound %.3g)" % ("ss > eps" if bool(r64[branch][0] > 0) else "ss <= eps", e_r, b_r))
            assert e_r <= b_r
    assert bool((y[0] == 0).all()) and float(rinv[0]) == -1e6 and float(rinv[1]) == -1e6
    assert torch.equal(d[0], g[0] * 1e6) and float(d[1].abs().max()) > 0  # the eps branch of the backward pass: 1e6 dy


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
def _op_run(parts, coef, normalize, fused, monkeypatch):
    monkeypatch.setattr(ops, "MEMORY_LINK_FUSED", fused)
    leaves = [t.clone().requires_grad_(True) for t in parts]
    y = ops.memory_link(leaves, normalize)
    (y * coef).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), [t.grad for t in leaves]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("rows,widths", [(5, [7, 6]), (130, [8, 8])])
def test_op_fused_against_composed(dev, monkeypatch, rows, widths, normalize):
    """ops.memory_link with the kernel and with YT8M_MEMORY_LINK_FUSED=0's torch.cat -> l2_normalize, values and the gradients through
    torch.autograd, under the kernel test's bound (the float32 restatement against the fp64 one); exact without normalize.  The fused
    form hands back one contiguous gradient per input."""
    x, g = _case(rows, widths, 7 * rows + sum(widths))
    offs = np.concatenate([[0], np.cumsum(widths)])
    parts = [x[:, offs[s]:offs[s + 1]].contiguous().to(dev) for s in range(len(widths))]
    yf, gf = _op_run(parts, g.to(dev), normalize, True, monkeypatch)
    yc, gc = _op_run(parts, g.to(dev), normalize, False, monkeypatch)
    assert all(t.is_contiguous() and tuple(t.shape) == (rows, w) for t, w in zip(gf, widths))
    df, dc = torch.cat([t.cpu() for t in gf], 1), torch.cat([t.cpu() for t in gc], 1)
    if not normalize:
        assert torch.equal(yf, x) and torch.equal(yc, x) and torch.equal(df, g) and torch.equal(dc, g)
        return
    refs = _refs(x, g)
    b_y, b_d = _bound(*refs["y"]), _bound(*refs["d"])
    e_y, e_d = float((yf - yc).abs().max()), float((df - dc).abs().max())
    print("(%d; %s): fused - composed y %.3g (bound %.3g) d %.3g (bound %.3g)" % (rows, widths, e_y, b_y, e_d, b_d))
    assert e_y <= b_y and e_d <= b_d
    assert float((yf.double() - refs["y"][1]).abs().max()) <= b_y and float((df.double() - refs["d"][1]).abs().max()) <= b_d
    # an input that wants no gradient gets none, the others are unchanged
    monkeypatch.setattr(ops, "MEMORY_LINK_FUSED", True)
    leaves = [parts[0].clone(), parts[1].clone().requires_grad_(True)]
    (ops.memory_link(leaves, True) * g.to(dev)).sum().backward()
    assert leaves[0].grad is None and torch.equal(leaves[1].grad, gf[1])


# ---- the plugins against fp64 ---------------------------------------------------------------------------------------------------------
# Tolerances of tests/test_gpu_distillchain.py::test_plugins_match_the_fp64_restatement.
P_TOL, LOSS_TOL, GRAD_TOL = 1e-4, 1e-4, 5e-4
V, LAYERS, CELLS, DCELLS, MIX, S, H = 11, 2, 8, 12, 2, 0.5, 8


def _flags(flags):
    import yt8m_amd.frame_level_models, yt8m_amd.losses, yt8m_amd.train  # noqa: F401, E401  (define the flags set below)
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.distillchain_relu_cells, flags.moe_num_mixtures = LAYERS, CELLS, DCELLS, MIX
    flags.lstm_layers, flags.lstm_cells = 2, str(H)
    flags.support_type, flags.support_loss_percent = ",".join(["label"] * LAYERS), S


def _l2n(x):
    from oracle import torch_ref
    return torch_ref.l2_normalize(x, 1)


def _moe(x, P, scope):
    from oracle import torch_ref
    return torch_ref.moe(x, P["gates%s/weights" % scope], P["experts%s/weights" % scope], P["experts%s/biases" % scope], MIX)


def _relu_norm(x, P, scope):
    return _l2n(torch.relu(x @ P[scope + "/weights"] + P[scope + "/biases"]))


def _layers(P, scope):
    return [(P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)], P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)])
            for l in range(2)]


def _memories(x, nf, P, scope):
    """concat of the final c of every layer of the stack under `scope` (state_is_tuple=True -> x.c)."""
    from oracle import torch_ref
    return torch.cat(torch_ref.lstm_stack(x, nf, _layers(P, scope))[1], 1)


def _chain_loss(pred, sup, y):
    from oracle import torch_ref
    return (1.0 - S) * torch_ref.cross_entropy(pred, y) + S * torch_ref.cross_entropy(sup, torch.cat([y] * LAYERS, 1))


def _ref_chain(x, nf, d, y, P):
    """lstm_memory_deep_chain_model.py:38-55: stage 0 reads stack 0's memories, stage l + 1 [stack l + 1's memories | relu_norm_l]."""
    nxt, sup = _memories(x, nf, P, "lstm-0-RNN"), []
    for l in range(LAYERS):
        sp = _moe(nxt, P, "-prediction-%d" % l)
        sup.append(sp)
        nxt = torch.cat([_memories(x, nf, P, "lstm-%d-RNN" % (l + 1)), _relu_norm(sp, P, "relu-%d" % l)], 1)
    pred, sup = _moe(nxt, P, "--main"), torch.cat(sup, 1)
    return pred, sup, _chain_loss(pred, sup, y)


def _ref_distill(x, nf, d, y, P):
    """distillchain_lstm_memory_deep_combine_chain_model.py:33-80: every stage reads [l2norm(memories) | distill | mean-relu | relu-0 ..]."""
    F = x.shape[1]
    mask = (torch.arange(F)[None, :] < nf[:, None]).to(x.dtype)
    mean_input = torch.einsum("ijk,ij->ik", x, mask) / nf.to(x.dtype)[:, None]
    relu_layers = [_relu_norm(d, P, "distill-relu"), _relu_norm(mean_input, P, "mean-relu")]
    nxt, sup = torch.cat([_l2n(_memories(x, nf, P, "lstm-0-RNN"))] + relu_layers, 1), []
    for l in range(LAYERS):
        sp = _moe(nxt, P, "-prediction-%d" % l)
        sup.append(sp)
        relu_layers.append(_relu_norm(sp, P, "relu-%d" % l))
        nxt = torch.cat([_l2n(_memories(x, nf, P, "lstm-%d-RNN" % (l + 1)))] + relu_layers, 1)
    pred, sup = _moe(nxt, P, "--main"), torch.cat(sup, 1)
    return pred, sup, _chain_loss(pred, sup, y)


FEATURES = [8, 8]


def _ref_parallel(x, nf, d, y, P):
    """lstm_parallel_memory_model.py:30-73: per feature an l2-normalised slice and a stack, head input = every layer's final c."""
    from oracle import torch_ref
    states, off = [], 0
    for i, fs in enumerate(FEATURES):
        states.append(_memories(torch_ref.l2_normalize(x[:, :, off:off + fs], 2), nf, P, "RNN%d" % i))
        off += fs
    pred = _moe(torch.cat(states, 1), P, "")
    return pred, None, torch_ref.cross_entropy(pred, y)


def _plugin(name):
    """(class, chain?, distillation?, restatement, flag settings, input width, the byte path's predicate)"""
    import yt8m_amd.frame_level_models as flm
    if name == "chain":
        return flm.LstmMemoryDeepChainModel, True, False, _ref_chain, {}, 8, lambda q: flm._lib_u8_ok(q.shape[2])
    if name == "distill":
        return (flm.DistillchainLstmMemoryDeepCombineChainModel, True, True, _ref_distill, {}, 8,
                lambda q: flm._lib_u8_ok(q.shape[2]) and seq_ops.u8_attention_supported(q, 1))
    return (flm.LstmParallelMemoryModel, False, False, _ref_parallel, dict(lstm_cells="8,4", feature_sizes="8,8"), 16,
            lambda q: all(flm._lib_u8_ok(fs) for fs in FEATURES))


def _data(name, path, dev, seed):
    """(model input as the trainer hands it over, fp64 frames of the restatement, num_frames, labels, distillation predictions, rs).
    B = 3; F = 7 for floats, 12 on bytes; D = 8 (16 for the two 8-wide features): the smallest the stack's byte predicate accepts."""
    from oracle import np_ref
    _, _, _, _, _, D, supported = _plugin(name)
    rs = np.random.RandomState(seed)
    B = 3
    y = rs.rand(B, V) < 0.2
    d = rs.rand(B, V).astype(np.float32)
    F = 12 if path == "bytes" else 7
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1                                                  # ragged, including 1 and F
    x64 = np_ref.dequant_l2norm_folded(q, nf)
    if path == "bytes":
        assert supported(torch.from_numpy(q).to(dev)), "the shape of this case must take the byte path"
        return q, torch.from_numpy(x64), nf, y, d, rs
    return x64.astype(np.float32), torch.from_numpy(x64), nf, y, d, rs


def _graph(name, x, y, nf, d, dev, seed=0):
    """The plugin's TrainGraph after one forward pass (variables created, arenas frozen).  Float frames arrive transformed already."""
    import yt8m_amd.feature_transform as ft
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    cls, chain = _plugin(name)[:2]
    g = reset_default_graph(device=dev, seed=seed)
    tg = train.TrainGraph(cls(), label_loss_fn=losses.MultiTaskCrossEntropyLoss() if chain else None, multitask=chain,
                          batch_size=x.shape[0], graph=g,
                          transformer_class=None if x.dtype == np.uint8 else ft.IdenticalTransformer)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    kw = {} if d is None else {"distillation_predictions": torch.from_numpy(d).to(dev)}
    tg.forward(*args, **kw)
    g.finalize()
    return g, tg, args, kw


def _stack_index(k):
    """Which stack a variable belongs to (lstm-<k>-RNN or RNN<k>), 0 for everything else."""
    for i in (1, 2):
        if k.startswith("lstm-%d-RNN/" % i) or k.startswith("RNN%d/" % i):
            return i
    return 0


def _draw(g, rs):
    """The draws of tests/test_gpu_distillchain.py::_draw -- a contractive recurrence (0.06), heads and FCs 0.2 -- with stack k's weights
    at 1 / (k + 1) of that scale: the stack's scratch carries max |W| scale words from its forward call to its backward call, so with
    equal scales a scratch slot that two stacks shared by mistake would go unnoticed; like this it shows as one stack wrong."""
    scale = lambda k: 0.06 / (1 + _stack_index(k)) if "basic_lstm_cell" in k else 0.2
    return {k: (rs.randn(*v.data.shape) * scale(k)).astype(np.float32) for k, v in g.vars.items()}


def _inject(g, P, dev):
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))


PLUGIN_CASES = [(n, p) for n in ("chain", "distill", "parallel") for p in ("floats", "bytes")]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name,path", PLUGIN_CASES)
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, path, fused):
    """Each plugin through TrainGraph.forward / loss / backward at B = 3, F = 7 (floats) or 12 (bytes) with ragged num_frames including 1
    and F, V = 11, 2 chain layers, 8 relu cells, 12 distill cells, two-layer stacks of 8 cells ((8, 4) for the parallel one): predictions,
    support predictions where there are any, the loss and the gradient of EVERY variable against the fp64 restatement, with the memory
    link as the fused kernel and composed."""
    monkeypatch.setattr(ops, "MEMORY_LINK_FUSED", fused)
    _flags(flags)
    cls, chain, distill, ref, fl, _, _ = _plugin(name)
    for k, v in fl.items():
        setattr(flags, k, v)
    x, x64, nf, y, d, rs = _data(name, path, dev, 11 + len(name))
    if distill:
        with pytest.raises(AssertionError, match="distillation feature must be used"):
            _graph(name, x, y, nf, None, dev)
    g, tg, args, kw = _graph(name, x, y, nf, d if distill else None, dev)
    stacks = sorted({k.split("/")[0] for k in g.vars if "basic_lstm_cell" in k})
    assert stacks == (["RNN0", "RNN1"] if name == "parallel" else ["lstm-%d-RNN" % k for k in range(LAYERS + 1)])
    assert ("distill-relu/weights" in g.vars) == distill and "distillrelu/weights" not in g.vars
    P = _draw(g, rs)
    _inject(g, P, dev)
    res = tg.forward(*args, **kw)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    tp = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in P.items()}
    pr, spr, lr = ref(x64, torch.from_numpy(nf), torch.from_numpy(d.astype(np.float64)), torch.from_numpy(y).double(), tp)
    lr.backward()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    ep = np.abs(f64(res["predictions"]) - pr.detach().numpy()).max()
    el = abs(float(loss.detach()) - float(lr.detach())) / max(1.0, abs(float(lr.detach())))
    grads = {k: f64(v.grad) for k, v in g.vars.items() if v.trainable}
    assert set(grads) == set(tp)
    unit = lambda k: np.abs(grads[k] - tp[k].grad.numpy()).max() / max(1.0, float(tp[k].grad.abs().max()))
    worst = max(tp, key=unit)
    print("%s %s: predictions %.3g loss %.3g worst gradient %s %.3g" % (name, path, ep, el, worst, unit(worst)))
    assert ep < P_TOL and el < LOSS_TOL
    if chain:
        assert tuple(res["support_predictions"].shape) == (x.shape[0], LAYERS * V)
        assert np.abs(f64(res["support_predictions"]) - spr.detach().numpy()).max() < P_TOL
    else:
        assert "support_predictions" not in res
    for k in tp:
        if "basic_lstm_cell" in k:                                       # every stack takes part: a gradient that is not just zeros
            assert float(tp[k].grad.abs().max()) > 0 and np.abs(grads[k]).max() > 0, k
        assert unit(k) <= GRAD_TOL, k


@pytest.mark.parametrize("name", ["chain", "distill", "parallel"])
def test_whole_training_step_and_its_bitwise_replay(dev, flags, monkeypatch, name):
    """One TrainGraph.step per plugin under --multitask --label_loss=MultiTaskCrossEntropyLoss (LstmParallelMemoryModel takes the plain
    loss) on the byte path: a finite loss, every parameter moved, no persistent-recurrence error; then a second step taken twice from
    the same state: bit-identical parameters.  With the fused memory link (the composed form is torch's own ops)."""
    monkeypatch.setattr(ops, "MEMORY_LINK_FUSED", True)
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    _flags(flags)
    cls, chain, distill, _, fl, _, _ = _plugin(name)
    for k, v in fl.items():
        setattr(flags, k, v)
    if distill:
        flags.distillation_features = flags.distillation_as_input = True
    flags.multitask, flags.label_loss = chain, "MultiTaskCrossEntropyLoss" if chain else "CrossEntropyLoss"
    x, _, nf, y, d, rs = _data(name, "bytes", dev, 31)
    g = reset_default_graph(device=dev, seed=0)
    tg = train.TrainGraph(cls(), label_loss_fn=train.find_class_by_name(flags.label_loss, [losses])(), batch_size=x.shape[0], graph=g)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    kw = dict(distill_labels_batch=torch.from_numpy(d).to(dev)) if distill else {}
    tg.forward(*args, **({"distillation_predictions": kw["distill_labels_batch"]} if distill else {}))
    g.finalize()
    initial = {k: v.data.detach().clone() for k, v in g.vars.items() if v.trainable}
    out = tg.step(*args, **kw)
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    assert np.isfinite(float(out["loss"]))
    for k, v in g.vars.items():                                          # every parameter moved
        if v.trainable:
            assert not torch.equal(v.data, initial[k]), k
    before = g.params.detach().clone()
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step = tg.global_step
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step = step
        out = tg.step(*args, **kw)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        assert np.isfinite(float(out["loss"]))
        after.append(g.params.detach().clone())
    assert torch.equal(after[0], after[1])
    assert not torch.equal(after[0], before)
