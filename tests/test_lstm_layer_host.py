"""CPU checks of LstmLayerModel (Z/frame_level_models.py:3629-3683) and of the wide LSTM step's C ABI (csrc/lstm_wide.hip): the lookup
by name, --lstm_length, the four cell Variables (names, shapes, initial values), what reaches the second LSTM and the head, the dropped
frames, the header / signature table / exports, yt8m_lstm_wide_supported's limits, argument validation without a device, the composed
form of seq_ops.lstm_clip_layer against the fp64 restatement, and the register allocation of the wide step kernel read from hipcc's
resource remarks."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lstm_layer_restatement as R
import yt8m_amd._lib as L
from cabi_helpers import declared_bound_exported
from conftest import ROOT

SYMBOLS = ("yt8m_lstm_wide_supported", "yt8m_lstm_wide_row_tile", "yt8m_lstm_wide_workspace_bytes", "yt8m_lstm_wide_prepare",
           "yt8m_lstm_wide_steps_fwd")
CELL = "%s/multi_rnn_cell/cell_0/basic_lstm_cell/%s"


def test_find_class_by_name_resolves_the_model_in_frame_level_models_only():
    import yt8m_amd.frame_level_models as flm
    import yt8m_amd.train as train
    import yt8m_amd.video_level_models as vlm
    cls = train.find_class_by_name("LstmLayerModel", [flm, vlm])
    assert cls is flm.LstmLayerModel and not hasattr(vlm, "LstmLayerModel")
    assert cls.accepts_quantized_input is True


def test_lstm_length_flag(flags):
    import yt8m_amd.frame_level_models  # noqa: F401
    assert flags.lstm_length == 10 and isinstance(flags.lstm_length, int)


def test_library_exports_and_header_declares_the_wide_symbols():
    src, lib = declared_bound_exported(SYMBOLS, r"int(?:64_t)?")
    assert "Z/frame_level_models.py:3653-3668" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved


def test_supported_states_the_kernels_limits():
    lib = L.lib()
    for B, H, ok in ((3840, 1024, 1), (960, 512, 1), (1, 256, 1), (129, 32, 1), (1 << 20, 4096, 1), (3840, 1000, 0), (3840, 16, 0),
                     (3840, 0, 0), (0, 1024, 0), (-1, 1024, 0), (3840, 4096 + 32, 0), ((1 << 20) + 1, 1024, 0)):
        assert lib.yt8m_lstm_wide_supported(B, H) == ok, (B, H)
        assert (lib.yt8m_lstm_wide_workspace_bytes(B, H) > 0) == bool(ok), (B, H)
    R_ = lib.yt8m_lstm_wide_row_tile()
    assert R_ == 128
    # the scale word, the image of W_h^T (4H rows) and two images of h over whole row tiles: 2 KiB per 32 rows x 16 k
    img = lambda rows, K: (rows // 32) * (K // 16) * 2048
    assert lib.yt8m_lstm_wide_workspace_bytes(R_ + 2, 512) == 256 + img(2048, 512) + 2 * img(2 * R_, 512)


def test_argument_validation_without_device():
    """Every call here fails validation or has nothing to do: nothing is launched and no device is needed."""
    lib = L.lib()
    OK, BADARG, SHAPE = 0, -1, -2
    p = [ctypes.c_void_p(256 * k) for k in range(1, 8)]
    H, B = 256, 5
    need = lib.yt8m_lstm_wide_workspace_bytes(B, H)

    def prepare(Wh=p[0], ldw=4 * H, B=B, H=H, ws=p[1], nbytes=need):
        return lib.yt8m_lstm_wide_prepare(Wh, ldw, B, H, ws, nbytes, None)

    def fwd(z=p[0], ws=p[1], nbytes=need, cs=p[2], hs=p[3], nf=None, t0=0, T=2, B=B, H=H):
        return lib.yt8m_lstm_wide_steps_fwd(z, ws, nbytes, cs, hs, nf, t0, T, B, H, 1.0, None)

    assert prepare(B=-1) == SHAPE and prepare(H=-256) == SHAPE and fwd(B=-1) == SHAPE and fwd(H=-256) == SHAPE    # negative size
    assert fwd(T=-1) == SHAPE and fwd(t0=-1) == SHAPE
    assert prepare(ldw=4 * H - 1) == SHAPE                                                       # small ldw
    assert prepare(H=200, ldw=800) == SHAPE and fwd(H=200) == SHAPE                              # what _supported refuses
    assert prepare(Wh=None) == BADARG and prepare(ws=None) == BADARG                             # null operand
    for name in ("z", "ws", "cs", "hs"):
        assert fwd(**{name: None}) == BADARG, name
    assert prepare(nbytes=need - 1) == BADARG and fwd(nbytes=need - 1) == BADARG                 # small workspace
    assert prepare(ws=ctypes.c_void_p(264)) == BADARG and fwd(ws=ctypes.c_void_p(264)) == BADARG  # misaligned workspace
    assert fwd(nf=p[4]) == BADARG                                                                # the wide step takes no lengths
    assert b"num_frames must be NULL" in lib.yt8m_last_error()
    assert prepare(B=0) == OK and prepare(H=0) == OK and fwd(T=0) == OK and fwd(B=0) == OK and fwd(H=0) == OK    # nothing to do
    assert prepare(B=0, Wh=None, ws=None) == OK and fwd(T=0, z=None, ws=None, cs=None, hs=None) == OK            # ... before anything else


# ---- the plugin on the CPU graph ----------------------------------------------------------------------------------------------------
def _graph():
    from yt8m_amd.variables import reset_default_graph
    return reset_default_graph(device=torch.device("cpu"), seed=0)


class _Stubs(object):
    """The second LSTM and the head replaced by shape-only stand-ins that record what the plugin handed them."""

    def __init__(self, monkeypatch):
        import yt8m_amd.ops as ops
        import yt8m_amd.seq_ops as seq_ops
        self.stacks, self.heads = [], []

        def stack(x_tm, num_frames, wb, **k):
            H = wb[0][0].data.shape[1] // 4
            self.stacks.append((x_tm, num_frames.clone(), [(W.name, b.name) for W, b in wb], k.get("slot", 0)))
            return torch.zeros(x_tm.shape[0], x_tm.shape[1], H), [(torch.ones(x_tm.shape[1], H), torch.zeros(x_tm.shape[1], H)) for _ in wb]

        def head(x, Wg, We, be, V_, M_, **k):
            self.heads.append(x)
            return torch.zeros(x.shape[0], V_)

        monkeypatch.setattr(seq_ops, "lstm_stack", stack)
        monkeypatch.setattr(ops, "moe_head", head)


def test_variables_and_what_the_second_lstm_and_the_head_receive(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    B, F, D, H, V = 3, 32, 8, 16, 10
    flags.lstm_cells, flags.moe_num_mixtures, flags.lstm_layers = str(H), 2, 5       # --lstm_layers is read and not used
    g = _graph()
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.randn(B, F, D).astype(np.float32))
    nf = torch.tensor([32, 9, 25])
    res = flm.LstmLayerModel().create_model(x, vocab_size=V, num_frames=nf)
    assert tuple(res["predictions"].shape) == (B, V)
    names = [CELL % (s, n) for s in ("RNN-1", "RNN-2") for n in ("weights", "biases")] + ["gates/weights", "experts/weights", "experts/biases"]
    assert list(g.vars) == names
    for scope, d_in in (("RNN-1", D), ("RNN-2", H)):
        W, b = g.vars[CELL % (scope, "weights")], g.vars[CELL % (scope, "biases")]
        assert tuple(W.data.shape) == (d_in + H, 4 * H) and tuple(b.data.shape) == (4 * H,) and W.trainable and b.trainable
        lim = math.sqrt(6.0 / (d_in + H + 4 * H))                      # _lstm_cells' initialisers: xavier_uniform and zeros
        assert float(W.data.abs().max()) <= lim and float(W.data.abs().max()) > 0.9 * lim and abs(float(W.data.mean())) < 0.1 * lim
        assert float(b.data.abs().max()) == 0.0
    # F = 32, U1 = 10: three clips, two frames dropped; RNN-2 reads [U2, B, H] with num_frames // U1 in a slot of its own
    (x_tm, lengths, wb, slot), = stubs.stacks
    assert tuple(x_tm.shape) == (3, B, H) and lengths.tolist() == [3, 0, 2] and slot == 1
    assert wb == [(CELL % ("RNN-2", "weights"), CELL % ("RNN-2", "biases"))]
    W1, b1 = g.vars[CELL % ("RNN-1", "weights")].data.double(), g.vars[CELL % ("RNN-1", "biases")].data.double()
    want = R.clip_recurrence(x.double(), nf, 10, W1, b1)
    assert R.err(x_tm, want.numpy()) < 2e-6
    x2 = x.clone()
    x2[:, 30:] += 7.0                                                     # the dropped frames reach nothing
    _graph()                                                              # (the same seed: the same initial values)
    stubs2 = _Stubs(monkeypatch)
    flm.LstmLayerModel().create_model(x2, vocab_size=V, num_frames=nf)
    assert torch.equal(stubs2.stacks[0][0], x_tm)
    # the head receives the final MEMORY of RNN-2, [B, H] (the stub's c is ones, its h zeros)
    (head_in,) = stubs.heads
    assert tuple(head_in.shape) == (B, H) and bool((head_in == 1).all())


def test_lstm_length_changes_the_clips(monkeypatch, flags):
    import yt8m_amd.frame_level_models as flm
    stubs = _Stubs(monkeypatch)
    flags.lstm_cells, flags.moe_num_mixtures, flags.lstm_length = "8", 2, 4
    _graph()
    flm.LstmLayerModel().create_model(torch.zeros(2, 13, 8), vocab_size=5, num_frames=torch.tensor([13, 7]))
    (x_tm, lengths, _, _), = stubs.stacks
    assert tuple(x_tm.shape) == (3, 2, 8) and lengths.tolist() == [3, 1]


# ---- the composed form against the restatement --------------------------------------------------------------------------------------
B_, F_, U1_, D_, H_ = 3, 12, 4, 16, 8
NF_ = [0, 3, 12]


def test_composed_clip_layer_matches_the_restatement_in_fp64():
    import yt8m_amd.seq_ops as seq_ops
    rs = np.random.RandomState(21)
    lim = math.sqrt(6.0 / (D_ + H_ + 4 * H_))
    W = ((rs.random_sample((D_ + H_, 4 * H_)) * 2 - 1) * 3 * lim).astype(np.float32)
    b = (0.1 * rs.randn(4 * H_)).astype(np.float32)
    x = rs.randn(B_, F_, D_).astype(np.float32)                                # padding frames hold data: the op must mask them
    dout = rs.randn(F_ // U1_, B_, H_).astype(np.float32)
    ref = R.clip_with_grads(x, NF_, U1_, W, b, dout, torch.float64)
    Wt = torch.from_numpy(W).double().requires_grad_(True)
    bt = torch.from_numpy(b).double().requires_grad_(True)
    before = dict(seq_ops.LSTM_CLIP_CALLS)
    out = seq_ops.lstm_clip_layer(torch.from_numpy(x).double(), torch.tensor(NF_), U1_, Wt, bt)
    assert seq_ops.LSTM_CLIP_CALLS["composed"] == before["composed"] + 1
    assert all(seq_ops.LSTM_CLIP_CALLS[k] == before[k] for k in ("wide", "packed", "gemm"))
    assert tuple(out.shape) == (F_ // U1_, B_, H_)
    (out * torch.from_numpy(dout).double()).sum().backward()
    for k, got in (("out", out), ("dW", Wt.grad), ("db", bt.grad)):
        assert R.err(got, ref[k]) < 1e-12, k
    # the dead clips -- every clip of video 0, clips 1 and 2 of video 1 -- saw zero vectors only: their memories are the cell's
    # response to U1 zero frames, whatever the padding frames held, and equal each other
    zero = R.clip_recurrence(torch.zeros(1, U1_, D_, dtype=torch.float64), [U1_], U1_, Wt.detach(), bt.detach())[0, 0]
    for j, bb in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1)):
        assert R.err(out[j, bb], zero.numpy()) < 1e-12, (j, bb)
    assert float((out[0, 1].detach() - zero).abs().max()) > 1e-3               # the clip with three real frames differs
    x2 = x.copy()
    x2[0] += 3.0
    x2[1, 3:] -= 2.0
    out2 = seq_ops.lstm_clip_layer(torch.from_numpy(x2).double(), torch.tensor(NF_), U1_, Wt, bt)
    assert torch.equal(out2, out)


def test_clip_lengths():
    import yt8m_amd.seq_ops as seq_ops
    got = seq_ops.clip_lengths(torch.tensor([0, 3, 12, 25, 40]), 10, 3)
    assert got.dtype == torch.int32 and got.view(5, 3).tolist() == [[0, 0, 0], [3, 0, 0], [10, 2, 0], [10, 10, 5], [10, 10, 10]]


# ---- the wide step kernel's registers, from hipcc's own resource remarks (cross-compiles without a GPU) -------------------------------
def test_wide_step_kernel_does_not_spill_and_keeps_two_waves_per_simd():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "--cuda-device-only", "-c", "lstm_wide.hip",
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, cwd=os.path.join(ROOT, "youtube-8m_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert len(out) == 2, sorted(out)
    for k, v in out.items():
        assert v.get("VGPRs Spill", 0) == 0 and v.get("ScratchSize", 0) == 0, (k, v)
    (step,) = [v for k, v in out.items() if "lstm_wide_step_kernel" in k]
    # the head comment's claim: two workgroups of four waves per CU = two waves per SIMD, at most 256 VGPRs, 32 KiB of LDS each
    assert step["Occupancy"] == 2 and step["VGPRs"] <= 256 and step["AGPRs"] == 0 and step["LDS Size"] == 32768, step
