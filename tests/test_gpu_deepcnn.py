"""DeepCnnDeepCombineChainModel / CnnLstmMemoryModel (W/all_frame_models/deep_cnn_deep_combine_chain_model.py, cnn_lstm_memory_model.py) on
the MI355X: the one-pass pooling kernels (csrc/deep_cnn.hip) through the C ABI, bitwise against a float32 numpy restatement with guard
words around every output; seq_ops.max_pool2_tm's kernel form bitwise against its composed form; both plugins through the plugin surface,
on the reader's bytes and on float frames, against fp64 restatements built here (oracle.torch_ref.lstm_stack / moe / cross_entropy around
explicit shifted concatenations and plain fp64 maxima); a one-frame video whose maxima sit on the padding's zeros; whole training steps."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.variables import reset_default_graph

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
GUARD = 64                                                             # floats in front of and behind every buffer


# ---- the kernels through the C ABI ------------------------------------------------------------------------------------------------
def _planted(F, B, C, seed):
    """Seeded normal values [F,B,C] with exact ties where the tie rules decide: column 0 repeats frame 0's value on every third frame,
    column 1 holds equal values inside every pair, column 2 is all-equal, and the trailing third of the frames of every odd video is exact
    zeros (the padding: a CNN output row whose window lies in it)."""
    rs = np.random.RandomState(seed)
    y = rs.randn(F, B, C).astype(np.float32)
    y[::3, :, 0] = y[0, :, 0]
    h = F // 2
    y[1:2 * h:2, :, 1] = y[0:2 * h:2, :, 1]
    y[:, :, 2] = np.float32(0.5)
    y[F - F // 3:, 1::2, :] = 0.0
    return y, rs


def _restate_fwd(y):
    h = y.shape[0] // 2
    return y.max(0), y.argmax(0).astype(np.int32), np.maximum(y[0:2 * h:2], y[1:2 * h:2])


def _restate_bwd(y, idx, g, dp):
    """scatter(g) + route(dp) in float32: at most one addition per element."""
    F, B, C = y.shape
    h = F // 2
    scat = np.zeros((F, B, C), np.float32)
    if g is not None:
        np.put_along_axis(scat, idx[None].astype(np.int64), g[None], 0)
    route = np.zeros((F, B, C), np.float32)
    if dp is not None and h:
        first = y[0:2 * h:2] >= y[1:2 * h:2]
        route[0:2 * h:2] = np.where(first, dp, np.float32(0))
        route[1:2 * h:2] = np.where(first, np.float32(0), dp)
    return scat + route


class _Win(object):
    """rows x C window (row stride ld, first column col0) of a device buffer with GUARD words either side, everything outside the window's
    values a sentinel; `want()` = the whole buffer as it must look after a kernel wrote `values` into the window."""

    def __init__(self, dev, rows, C, ld, col0=0, values=None, dtype=np.float32):
        self.rows, self.C, self.ld, self.col0 = rows, C, ld, col0
        self.host = np.full(2 * GUARD + rows * ld, SENTINEL, np.float32).view(dtype).copy()
        self.dtype = dtype
        if values is not None:
            self._window(self.host)[...] = values.reshape(rows, C)
        self.t = torch.from_numpy(self.host.view(np.int32)).to(dev)
        self.p = ctypes.c_void_p(self.t.data_ptr() + 4 * (GUARD + col0))

    def _window(self, flat):
        return flat[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)[:, self.col0:self.col0 + self.C]

    def want(self, values):
        w = self.host.copy()
        self._window(w)[...] = values.reshape(self.rows, self.C)
        return w.view(np.int32)

    def got(self):
        return self.t.cpu().numpy()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _kernel_case(dev, F, B, C, extra):
    """Forward with and without `pooled`, backward with every operand and with g / dp NULL: all outputs bitwise, guards untouched."""
    lib = L.lib()
    ld, col0 = C + extra, (4 if extra else 0)
    y, rs = _planted(F, B, C, seed=F * 1000 + B * 10 + C)
    out_r, idx_r, p_r = _restate_fwd(y)
    h = F // 2
    gy = _Win(dev, F * B, C, ld, col0, y)
    for with_pool in (True, False):
        out, idx, pooled = _Win(dev, B, C, ld, col0), _Win(dev, B, C, ld, col0, dtype=np.int32), _Win(dev, max(h * B, 1), C, ld, col0)
        L.check(lib.yt8m_timepool_max_pool2_f32_fwd(gy.p, ld, F, B, C, out.p, idx.p, ld, pooled.p if with_pool else None, ld, _st()))
        torch.cuda.synchronize()
        assert np.array_equal(out.got(), out.want(out_r))
        assert np.array_equal(idx.got(), idx.want(idx_r))
        if with_pool and h:
            assert np.array_equal(pooled.got(), pooled.want(p_r))
        else:
            assert np.array_equal(pooled.got(), pooled.host.view(np.int32))   # no pooled rows / NULL: nothing written
        assert np.array_equal(gy.got(), gy.host.view(np.int32))
    g = rs.randn(B, C).astype(np.float32)
    dp = rs.randn(h, B, C).astype(np.float32)
    gg, gidx, gdp = _Win(dev, B, C, ld, col0, g), _Win(dev, B, C, ld, col0, idx_r, dtype=np.int32), _Win(dev, max(h * B, 1), C, ld, col0,
                                                                                                      dp if h else None)
    for use_g, use_dp in ((True, True), (False, True), (True, False)):
        dy = _Win(dev, F * B, C, ld, col0)
        L.check(lib.yt8m_timepool_max_pool2_f32_bwd(gy.p, ld, F, B, C, gg.p if use_g else None, gidx.p, ld, gdp.p if use_dp else None, ld,
                                                    dy.p, ld, _st()))
        torch.cuda.synchronize()
        want = _restate_bwd(y, idx_r, g if use_g else None, dp if use_dp else None)
        assert np.array_equal(dy.got(), dy.want(want)), (use_g, use_dp)
    ties = int((y == out_r[None]).sum(0).max())
    assert ties > 1 or F == 1                                            # the data does exercise the first-frame rule


@pytest.mark.parametrize("F,B,C", [(1, 3, 4), (2, 1, 4), (3, 5, 8), (9, 16, 36), (35, 3, 260), (4, 130, 8), (300, 2, 512)])
def test_kernels_bitwise_against_numpy(dev, F, B, C):
    """(1,3,4) no pooled rows; (3,5,8) an unpaired last frame; (9,16,36) a partial column tile; (35,3,260) several tiles and a partial
    one, three pair rounds of the 16 classes; (4,130,8) more videos than a backward row block; (300,2,512) the script's F and C."""
    _kernel_case(dev, F, B, C, extra=0)


def test_kernels_on_a_column_window(dev):
    """ldy, ldo, ldp, lddy larger than C: a window of a wider matrix, its neighbours untouched."""
    _kernel_case(dev, 9, 16, 36, extra=8)


def test_a_refused_shape_leaves_its_buffers_untouched(dev):
    lib = L.lib()
    F, B, C = 4, 3, 8
    y, _ = _planted(F, B, C, seed=1)
    gy = _Win(dev, F * B, C, C, 0, y)
    out, idx, pooled, dy = _Win(dev, B, C, C), _Win(dev, B, C, C, dtype=np.int32), _Win(dev, 2 * B, C, C), _Win(dev, F * B, C, C)
    assert lib.yt8m_timepool_max_pool2_f32_fwd(gy.p, C, F, B, 6, out.p, idx.p, C, pooled.p, C, _st()) == -2
    assert lib.yt8m_timepool_max_pool2_f32_fwd(gy.p, C + 2, F, B, C, out.p, idx.p, C, pooled.p, C, _st()) == -2
    assert lib.yt8m_timepool_max_pool2_f32_fwd(ctypes.c_void_p(gy.p.value + 4), C, F, B, C, out.p, idx.p, C, pooled.p, C, _st()) == -1
    assert lib.yt8m_timepool_max_pool2_f32_bwd(gy.p, C, F, B, 6, out.p, idx.p, C, pooled.p, C, dy.p, C, _st()) == -2
    assert lib.yt8m_timepool_max_pool2_f32_bwd(gy.p, C, 0, B, C, out.p, idx.p, C, pooled.p, C, dy.p, C, _st()) == -2
    assert lib.yt8m_timepool_max_pool2_f32_bwd(gy.p, C, F, B, C, out.p, None, C, pooled.p, C, dy.p, C, _st()) == -1
    torch.cuda.synchronize()
    for w in (out, idx, pooled, dy, gy):
        assert np.array_equal(w.got(), w.host.view(np.int32))


# ---- the op: the kernels against the composed form ----------------------------------------------------------------------------------
def _count_calls(monkeypatch, names):
    lib, calls = L.lib(), {n: 0 for n in names}

    def wrap(name):
        fn = getattr(lib, name)

        def counted(*a):
            calls[name] += 1
            return fn(*a)
        monkeypatch.setattr(lib, name, counted)

    for n in names:
        wrap(n)
    return calls


@pytest.mark.parametrize("F,B,C", [(9, 16, 36), (300, 2, 512)])
def test_op_fused_equals_composed_bitwise(dev, monkeypatch, F, B, C):
    y_np, rs = _planted(F, B, C, seed=7 + F)
    gm = torch.from_numpy(rs.randn(B, C).astype(np.float32)).to(dev)
    gp = torch.from_numpy(rs.randn(F // 2, B, C).astype(np.float32)).to(dev)
    calls = _count_calls(monkeypatch, ["yt8m_timepool_max_pool2_f32_fwd", "yt8m_timepool_max_pool2_f32_bwd", "yt8m_timepool_max_f32"])
    got = {}
    for form, env in (("fused", "1"), ("composed", "0")):
        monkeypatch.setenv("YT8M_DEEP_CNN_FUSED", env)                   # read at call time
        y = torch.from_numpy(y_np).to(dev).view(F * B, C).requires_grad_(True)
        before = dict(calls)
        m, p = seq_ops.max_pool2_tm(y, F, B)
        ((m * gm).sum() + (p * gp).sum()).backward()
        m_only, none = seq_ops.max_pool2_tm(y.detach(), F, B, want_pool=False)
        torch.cuda.synchronize()
        assert none is None and torch.equal(m_only, m)
        got[form] = (m.detach(), p.detach(), y.grad)
        used = {k: calls[k] - before[k] for k in calls}
        assert used == (dict(yt8m_timepool_max_pool2_f32_fwd=2, yt8m_timepool_max_pool2_f32_bwd=1, yt8m_timepool_max_f32=0) if form == "fused"
                        else dict(yt8m_timepool_max_pool2_f32_fwd=0, yt8m_timepool_max_pool2_f32_bwd=0, yt8m_timepool_max_f32=2)), (form, used)
    for a, b in zip(got["fused"], got["composed"]):
        assert a.shape == b.shape and torch.equal(a, b)
    out_r, _, p_r = _restate_fwd(y_np)
    assert np.array_equal(got["fused"][0].cpu().numpy(), out_r) and np.array_equal(got["fused"][1].cpu().numpy(), p_r)


# ---- the plugins --------------------------------------------------------------------------------------------------------------------
# Bounds of the sibling plugins (tests/test_gpu_lstmcnn.py): predictions and loss 1e-4, gradients 5e-4 max(1, max|g|) per variable.
P_TOL, LOSS_TOL, GRAD_TOL = 1e-4, 1e-4, 5e-4
SMALL = dict(B=16, F=9, D=96, V=13, L_=2, M_=2, c=8, cells=8, s=0.5, H=128, lstm_layers=2)
DEEP_SIZES = ((1, 2, 3), (2, 3), (2, 3))


def _shifted_cnn(x, Ws, D):
    """cnn_output [B,F,sum N] in the dtype of x [B,F,D]: per filter the input concatenated with its 1 .. fs - 1 frame shifts (zero padding
    in front) times W [fs D, N]."""
    B, F, _ = x.shape
    outs = []
    for W in Ws:
        fs = W.shape[0] // D
        sh = [x] + [torch.cat([x.new_zeros(B, min(i, F), D), x[:, :max(F - i, 0)]], 1) for i in range(1, fs)]
        outs.append(torch.cat(sh, 2) @ W)
    return torch.cat(outs, 2)


def _deep_maxima(x, P, k):
    """[max over the frames of level i's output] of deepcnn<k>, plain maxima in the dtype of x; a level reads the pair maxima of the
    level before (an odd last frame dropped)."""
    maxima, inp = [], x
    for i, sizes in enumerate(DEEP_SIZES):
        y = _shifted_cnn(inp, [P["deepcnn%dcnn%dfilter-len%d" % (k, i, fs)] for fs in sizes], inp.shape[2])
        maxima.append(y.max(1).values)
        h = y.shape[1] // 2
        inp = torch.maximum(y[:, 0:2 * h:2], y[:, 1:2 * h:2])
    return maxima


def _mean_input(x, nf):
    mask = (torch.arange(x.shape[1], device=x.device)[None, :] < nf[:, None]).to(x.dtype)
    return torch.einsum("ijk,ij->ik", x, mask) / nf.to(x.dtype)[:, None]


def _restate_deep(x, nf, labels, P, c=SMALL):
    """DeepCnnDeepCombineChainModel in the dtype of x [B,F,D] (batch-major, as the reference): predictions, support predictions and the
    multitask loss (1 - s) CE(p, y) + s CE(support, [y] * L)."""
    from oracle import torch_ref
    L_, M_, s = c["L_"], c["M_"], c["s"]
    mean_input = _mean_input(x, nf)
    relu_layers = [torch_ref.l2_normalize(torch.relu(mean_input @ P["mean-relu/weights"] + P["mean-relu/biases"]))]
    deep = lambda k: torch_ref.l2_normalize(torch.cat(_deep_maxima(x, P, k), 1))
    nxt, sup = deep(0), []
    for l in range(L_):
        sc = "prediction-%d" % l
        sp = torch_ref.moe(nxt, P["gates-%s/weights" % sc], P["experts-%s/weights" % sc], P["experts-%s/biases" % sc], M_)
        sup.append(sp)
        relu_layers.append(torch_ref.l2_normalize(torch.relu(sp @ P["relu-%d/weights" % l] + P["relu-%d/biases" % l])))
        nxt = torch.cat([mean_input, deep(l + 1)] + relu_layers, 1)
    pred = torch_ref.moe(nxt, P["gates--main/weights"], P["experts--main/weights"], P["experts--main/biases"], M_)
    support = torch.cat(sup, 1)
    yl = labels.to(x.dtype)
    loss = (1.0 - s) * torch_ref.cross_entropy(pred, yl) + s * torch_ref.cross_entropy(support, torch.cat([yl] * L_, 1))
    return pred, support, loss


def _restate_cnnlstm(x, nf, labels, P, c=SMALL):
    """CnnLstmMemoryModel in the dtype of x: predictions, None, CE(p, y)."""
    from oracle import torch_ref
    y = _shifted_cnn(x, [P["cnn-filter-len%d" % fs] for fs in (1, 2, 3)], x.shape[2])
    layers = [(P["RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % l], P["RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % l])
              for l in range(c["lstm_layers"])]
    _, cs, _ = torch_ref.lstm_stack(torch_ref.l2_normalize(y, 2), nf, layers)
    pred = torch_ref.moe(torch.cat(cs, 1), P["gates/weights"], P["experts/weights"], P["experts/biases"], c["M_"])
    return pred, None, torch_ref.cross_entropy(pred, labels.to(x.dtype))


RESTATE = {"DeepCnnDeepCombineChainModel": _restate_deep, "CnnLstmMemoryModel": _restate_cnnlstm}


def _small_flags(flags, c=SMALL):
    import yt8m_amd.frame_level_models, yt8m_amd.losses, yt8m_amd.train  # noqa: F401, E401  (define the flags set below)
    flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.deep_cnn_base_size, flags.moe_num_mixtures = c["L_"], c["cells"], c["c"], c["M_"]
    flags.support_type, flags.support_loss_percent = ",".join(["label"] * c["L_"]), c["s"]
    flags.lstm_cells, flags.lstm_layers = str(c["H"]), c["lstm_layers"]


def _draw(shapes, rs, negative_filters=False):
    """As tests/test_gpu_lstmcnn.py::_draw: a contractive recurrence (0.06), filters at the initialiser's 0.1, heads and FCs 0.2."""
    scale = lambda k: 0.06 if "basic_lstm_cell" in k else (0.1 if "filter-len" in k else 0.2)
    P = {k: (rs.randn(*shp) * scale(k)).astype(np.float32) for k, shp in shapes.items()}
    if negative_filters:
        P = {k: (-np.abs(v) if "filter-len" in k else v) for k, v in P.items()}
    return P


def _small_case(seed, c=SMALL, F=None, one_frame=False):
    """(rs, q uint8 [B,F,D], x64 = the frames as the transformer hands them over, labels, num_frames ragged, including 1 and F)."""
    from oracle import np_ref
    rs = np.random.RandomState(seed)
    B, F, D = c["B"], F or c["F"], c["D"]
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1
    if one_frame:
        nf[:] = 1
    y = rs.rand(B, c["V"]) < 0.2
    return rs, q, torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf)), y, nf


def _make_graph(model, q, y, nf, dev, multitask):
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    g = reset_default_graph(device=dev, seed=0)
    loss_fn = losses.MultiTaskCrossEntropyLoss() if multitask else losses.CrossEntropyLoss()
    tg = train.TrainGraph(model, label_loss_fn=loss_fn, multitask=multitask, batch_size=q.shape[0], graph=g)
    args = (torch.from_numpy(q).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(nf).to(dev))
    tg.forward(*args)
    g.finalize()
    return g, tg, args


def _run_plugin(name, q, y, nf, dev, draw):
    import yt8m_amd.frame_level_models as flm
    g, tg, args = _make_graph(getattr(flm, name)(), q, y, nf, dev, multitask=name.startswith("DeepCnn"))
    P = draw({k: tuple(v.data.shape) for k, v in g.vars.items()})
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(dev).view(g.vars[k].data.shape))
    res = tg.forward(*args)
    loss = tg.loss(res, args[1])
    loss.backward()
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    assert all(v.trainable for v in g.vars.values())
    grads = {k: f64(v.grad) for k, v in g.vars.items()}
    return dict(p=f64(res["predictions"]), sp=f64(res["support_predictions"]) if "support_predictions" in res else None,
                loss=float(loss.detach()), grads=grads, P=P)


def _oracle(name, x, nf, y, P, dtype=torch.float64, c=SMALL):
    tp = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in P.items()}
    pred, support, loss = RESTATE[name](x.to(dtype), torch.from_numpy(nf), torch.from_numpy(y), tp, c)
    loss.backward()
    f64 = lambda t: None if t is None else t.detach().numpy().astype(np.float64)
    return dict(p=f64(pred), sp=f64(support), loss=float(loss.detach()), grads={k: f64(t.grad) for k, t in tp.items()})


def _check(run, ref):
    """Every trainable variable against the restatement, every gradient non-zero; each figure printed before it is asserted."""
    ep = np.abs(run["p"] - ref["p"]).max()
    es = 0.0 if ref["sp"] is None else np.abs(run["sp"] - ref["sp"]).max()
    el = abs(run["loss"] - ref["loss"]) / max(1.0, abs(ref["loss"]))
    unit = lambda k: np.abs(run["grads"][k] - ref["grads"][k]).max() / max(1.0, np.abs(ref["grads"][k]).max())
    worst = max(((k, unit(k)) for k in ref["grads"]), key=lambda kv: kv[1])
    print("predictions %.3g support %.3g loss %.3g worst gradient %s %.3g" % ((ep, es, el) + worst))
    assert set(run["grads"]) == set(ref["grads"])
    assert ep < P_TOL and es < P_TOL
    assert el < LOSS_TOL
    for k in ref["grads"]:
        assert np.abs(run["grads"][k]).max() > 0, k
        assert unit(k) <= GRAD_TOL, k


_ORACLES = {}
SEEDS = {"DeepCnnDeepCombineChainModel": 5, "CnnLstmMemoryModel": 6}


def _case_with_oracle(name):
    """The small case of a plugin, its drawn variables and its fp64 restatement: made once, shared by the tests that compare against it."""
    if name not in _ORACLES:
        rs, q, x64, y, nf = _small_case(SEEDS[name])
        case = _ORACLES[name] = dict(q=q, x64=x64, y=y, nf=nf, P=None, ref=None)

        def draw(shapes):                                               # the graph names the variables; they are drawn once
            if case["P"] is None:
                case["P"] = _draw(shapes, rs)
            return case["P"]

        case["draw"] = draw
    return _ORACLES[name]


def _want_names(name, c=SMALL):
    if name == "CnnLstmMemoryModel":
        return {"cnn-filter-len%d" % fs for fs in (1, 2, 3)} | {"gates/weights", "experts/weights", "experts/biases"} | \
            {"RNN/multi_rnn_cell/cell_%d/basic_lstm_cell/%s" % (l, w) for l in range(c["lstm_layers"]) for w in ("weights", "biases")}
    names = {"mean-relu/weights", "mean-relu/biases"}
    for k in range(c["L_"] + 1):
        names |= {"deepcnn%dcnn%dfilter-len%d" % (k, i, fs) for i, sizes in enumerate(DEEP_SIZES) for fs in sizes}
    for sc in ["prediction-%d" % l for l in range(c["L_"])] + ["-main"]:
        names |= {"gates-%s/weights" % sc, "experts-%s/weights" % sc, "experts-%s/biases" % sc}
    for l in range(c["L_"]):
        names |= {"relu-%d/weights" % l, "relu-%d/biases" % l}
    return names


@pytest.mark.parametrize("frames", ["bytes", "floats"])
@pytest.mark.parametrize("name,form", [("DeepCnnDeepCombineChainModel", "fused"), ("DeepCnnDeepCombineChainModel", "composed"),
                                       ("CnnLstmMemoryModel", None)])
def test_plugins_match_the_fp64_restatement(dev, flags, monkeypatch, name, form, frames):
    """B = 16, F = 9 (levels of 9, 4 and 2 frames), uint8 [B,9,96], V = 13; the deep CNN with c = 8, 2 chain layers, 2 mixtures and the
    multitask loss at s = 0.5, in both forms of seq_ops.max_pool2_tm; the CNN-LSTM with two layers of 128 cells.  bytes: the plugin reads
    the reader's bytes; floats: the transformer dequantises first (--fold_dequant=False).  The restatement takes plain fp64 maxima: a
    seed on which fp32 and fp64 disagree about an argmax (a near-tie) is to be CHANGED, the bounds stay (the seeds here were checked on
    the CPU, the restatement in fp32 against itself in fp64: inside the bounds)."""
    _small_flags(flags)
    flags.fold_dequant = frames == "bytes"
    case = _case_with_oracle(name)
    if frames == "bytes":
        qt = torch.from_numpy(case["q"]).to(dev)
        assert seq_ops.u8_cnn_supported(qt) and seq_ops.u8_attention_supported(qt, 1), "the shape of this test must take the uint8 path"
    if form is not None:
        monkeypatch.setenv("YT8M_DEEP_CNN_FUSED", "1" if form == "fused" else "0")
    calls = _count_calls(monkeypatch, ["yt8m_timepool_max_pool2_f32_fwd", "yt8m_timepool_max_pool2_f32_bwd"])
    run = _run_plugin(name, case["q"], case["y"], case["nf"], dev, case["draw"])
    assert set(run["P"]) == _want_names(name)
    # two levels per deep CNN go through the op (the last one through the gathering op), three deep CNNs, forward twice (graph + run)
    assert calls == ({"yt8m_timepool_max_pool2_f32_fwd": 12, "yt8m_timepool_max_pool2_f32_bwd": 6} if form == "fused" else
                     {"yt8m_timepool_max_pool2_f32_fwd": 0, "yt8m_timepool_max_pool2_f32_bwd": 0})
    if case["ref"] is None:
        case["ref"] = _oracle(name, case["x64"], case["nf"], case["y"], run["P"])
    _check(run, case["ref"])


def test_one_frame_videos_whose_maxima_sit_on_the_padding(dev, flags):
    """num_frames = 1 of F = 12 for every video and filters drawn negative: most rows of every level are exactly 0 (windows wholly in
    the padding), the pairs among them tie at 0 and the padding's zero wins columns of the global maximum, on several rows at once.  The
    first-frame rule and the fp64 restatement's (torch's) rule hand those gradients to different rows -- all of them rows whose inputs
    are zero: the variables' gradients still match."""
    _small_flags(flags)
    name = "DeepCnnDeepCombineChainModel"
    rs, q, x64, y, nf = _small_case(23, F=12, one_frame=True)
    run = _run_plugin(name, q, y, nf, dev, lambda shapes: _draw(shapes, rs, negative_filters=True))
    with torch.no_grad():
        P64 = {k: torch.from_numpy(v).double() for k, v in run["P"].items()}
        maxima = torch.cat([m for k in range(SMALL["L_"] + 1) for m in _deep_maxima(x64, P64, k)], 1)
    zeros = int((maxima == 0).sum())
    print("pooled columns with a maximum of exactly 0: %d of %d" % (zeros, maxima.numel()))
    assert zeros > maxima.numel() // 10
    _check(run, _oracle(name, x64, nf, y, run["P"]))


# ---- whole steps ----------------------------------------------------------------------------------------------------------------------
def _script_case(seed, B):
    rs = np.random.RandomState(seed)
    F, D, V = 300, 1152, 4716
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1] = F, 1
    y = rs.rand(B, V) < 3.4 / V
    y[:, 0] = True
    return q, nf, y


@pytest.mark.parametrize("name", ["DeepCnnDeepCombineChainModel", "CnnLstmMemoryModel"])
def test_whole_training_step_and_its_bitwise_replay(dev, flags, name):
    """One TrainGraph.step (forward, backward, clip + Adam) of each plugin at B = 32 of its training script's shape and flags: finite
    loss, every parameter moved.  Then a second step, taken twice from the same state (parameters and Adam moments restored):
    bit-identical parameters -- nothing in the step depends on the order in which the device happened to run it."""
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.losses, yt8m_amd.train  # noqa: F401, E401  (define the flags set below)
    if name == "DeepCnnDeepCombineChainModel":                          # run-chaining-deep-cnn.sh
        flags.deep_chain_layers, flags.deep_chain_relu_cells, flags.deep_cnn_base_size, flags.moe_num_mixtures = 2, 256, 128, 4
        flags.support_type, flags.dropout, flags.keep_prob = "label,label", True, 1.0
    else:                                                               # run-cnn-lstm.sh
        flags.lstm_cells, flags.lstm_layers, flags.moe_num_mixtures = "1024", 2, 8
    q, nf, y = _script_case(11, 32)
    g, tg, args = _make_graph(getattr(flm, name)(), q, y, nf, dev, multitask=name.startswith("DeepCnn"))
    before = {k: v.data.detach().clone() for k, v in g.vars.items()}
    out = tg.step(*args)
    torch.cuda.synchronize()
    seq_ops.check_persist_errors()
    assert np.isfinite(float(out["loss"]))
    for k, v in g.vars.items():
        assert bool(torch.isfinite(v.data).all()) and not torch.equal(v.data, before[k]), k
    state = [t.detach().clone() for t in (g.params, g.adam_m, g.adam_v)]
    step = tg.global_step
    after = []
    for _ in range(2):
        for t, s in zip((g.params, g.adam_m, g.adam_v), state):
            t.copy_(s)
        tg.global_step = step
        tg.step(*args)
        torch.cuda.synchronize()
        seq_ops.check_persist_errors()
        after.append(g.params.detach().clone())
    assert torch.equal(after[0], after[1])
