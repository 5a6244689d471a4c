"""-m gpu: every dispatch branch of the one-launch-per-step recurrences (the LSTM half of csrc/sequence.hip, csrc/lstm_fused.hip,
csrc/lstm_bf16.hip, csrc/cells.hip and the host pieces of csrc/step_kernels.h) through the C ABI with raw pointers, against the fp64
restatement of tests/step_restatement.py (tied to the oracle by tests/test_step_restatement_host.py), on both sides of every threshold,
with sentinel margins around every output, the tape slots outside the time range compared bit for bit, and the refusals of each entry
point.  Every call is issued on a side stream: the packed time-range forms are captured into hipGraphs, and the default stream cannot be
captured.

BRANCH_TABLE below is the reading of the dispatchers this module was written from: (entry point, condition as written in the .hip file,
kernel instantiation launched as the profiler prints it, the case of this module that takes it).  Refusals are rows with kernel
"(none)"; an arm no case takes says "left out:" and why.  tests/test_step_branch_table.py checks the table against the sources and the
list recorded from a profiled run of this module (tests/golden/step_kernels_seen.txt, profiles/step_branches_kernel_stats.csv).

Bounds.  None is taken from anything the code under test produced.
  Measure: max |got - ref| / max(1, max |ref|) per quantity.  Bound: EIGHT times the error of the float32 restatement (plain torch on
    the CPU, the same inputs) against the float64 one, never below 2e-6 for results and states or 5e-6 for gradients (the rule of
    tests/test_gpu_gate_lstm.py and tests/test_gpu_lstm_layer.py).  Weights have a trained cell's scale (gain 3 over the Glorot limit).
  Single-step cases (T = 1 of the time-range forms from a state the host wrote, F = 1 of the whole-layer forms from a given state):
    nothing compounds, every output of the step is compared element by element under that rule.
  Bare products: LN-LSTM's z after step 0 (EP_ADD, A = the host's h0) and the dh half of `work` after a T = 1 / F = 1 backward (BEP 0,
    A = the dz the same call wrote, itself held to fp64) element by element to (K + S + 2) u (|A| |B|)_ij + u |result|, S = 4 wave
    parts, u = 2^-24 (the derived bound of tests/test_gpu_gemm_branches.py).
  bf16 forms: the reference is the restatement with bf16-rounded product operands.  Single forward steps start from an h that is exact
    in bf16 and take the float32 rule; multi-step forward tapes and every backward keep 2e-3 (of max |dz| for gradients) against the
    emulation, the bound of tests/test_gpu_round4.py::test_bf16_*_recurrence_against_a_rounding_emulation, whose docstring says what
    is left (values within 1e-7 of a bf16 rounding boundary).  The T = 1 backward product is also held to the bare-product bound with
    the rounded operands (K = 4H, u = 2^-24: the products of bf16 values are exact in fp32).
Rows with t >= num_frames[b] are compared bit for bit: state copied through, out = 0, dz = 0, (dh, dc) carried.
Each case prints its errors next to its bounds.

Measured on an MI355X, in the profiled run the two records are from (largest error per quantity over all cases of a family, the
float32 restatement's error of the same case in brackets; the module prints this list at its end):
  gate kernels alone: gates / c / h / out 8.3e-8 / 8.3e-8 / 8.6e-8 / 8.2e-8 [8.3e-8 / 8.3e-8 / 8.6e-8 / 8.7e-8]; dz / dc_prev 8.6e-8 /
    6.0e-8 [1.0e-7 / 7.8e-8]; dh_prev of live rows exactly 0
  whole-layer LSTM (packed and generic): gates 1.3e-6 [1.1e-6] (generic, H = 192, F = 1), cs 3.5e-7 [3.1e-7], hs = out 5.6e-7 [5.4e-7];
    dz 3.4e-7 [3.1e-7], dh 8.0e-7 [3.6e-7], dc 5.7e-7 [2.4e-7] (generic, H = 128 without a workspace)
  time-range LSTM: gates 7.9e-7 [8.8e-7], cs 3.3e-7 [3.0e-7], hs = out 3.8e-7 [3.5e-7]; dz 2.5e-7 [1.6e-7], dh 4.9e-7 [5.3e-7], dc
    3.7e-7 [2.2e-7]; captured and replayed chains: gates 4.1e-7 [1.2e-6], hs 2.4e-7 [2.5e-7], dz 1.3e-7 [2.5e-7], dh 1.9e-7 [3.5e-7]
  bare products, largest |got - ref| as a fraction of the element's bound: LSTM T = 1 / F = 1 backward 0.0027, LN-LSTM z of step 0
    0.0050, LN-LSTM F = 1 backward 0.0017, bf16 T = 1 backward 0.00043
  bf16: single forward step out 1.8e-7 [7.0e-7]; T = 3 tape gates 1.4e-4, cs 5.1e-5, hs 6.3e-5 (the float32 restatement of the
    emulation differs from the float64 one by the same: an h on a bf16 rounding boundary) of 2e-3; T = 1 dz 9.8e-8 [1.1e-7]; multi-step
    dz / dh / dc 1.5e-5 / 1.3e-4 / 1.8e-5 absolute, of 2e-3 max |dz| (3.4e-3 to 8.5e-3 in these cases)
  GRU packed: zg / zc / rh 3.6e-7 / 1.0e-6 / 6.5e-7 [4.9e-7 / 1.2e-6 / 6.4e-7], hs 9.0e-7 [8.9e-7]; dzg / dzc / dh 2.2e-7 / 2.3e-7 / 2.5e-7
    [2.5e-7 / 2.7e-7 / 4.3e-7].  GRU generic: zc 1.3e-6 [1.1e-6], hs 1.0e-6 [9.8e-7]; dzg / dzc / dh 2.7e-7 / 3.4e-7 / 3.6e-7 [2.5e-7 /
    2.2e-7 / 2.6e-7]
  LN-LSTM: z 9.8e-7 [1.0e-6], stats 1.2e-7 [6.8e-8], cs 6.7e-7 [5.7e-7], hs = out 2.9e-6 [2.4e-6] (H = 1025, PT = 8, keep_prob 0.75);
    dz 5.0e-7 [4.8e-7], dyb 5.8e-7 [2.9e-7], dyg 5.6e-7 [1.4e-7], dh 2.3e-6 [9.8e-7], dc 5.2e-7 [4.1e-7]
The floors are the binding bound nearly everywhere; no case needed more than 0.38 of its bound (dh of the LN-LSTM at H = 1025, F = 1: 2.1e-6 of 5.5e-6), and no kernel bug was found.  Everything
bitwise held bit for bit.  The children (modes 0000 / 1111 / 2222 / 3333, no packed cells, no graph) stayed within the same bounds.
"""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "yt8m_amd" not in sys.modules:              # the children run this file as a script, without the suite's conftest
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import __graft_entry__
    __graft_entry__.load_package()

import step_restatement as R  # noqa: E402
import yt8m_amd._lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

_F = "lstm_step_fwd_kernel<%d, %d, %d>"
_B = "lstm_step_bwd_kernel<%d, %d>"
_MODES_CHILD = "child: test_step_mode_and_switch_children"
BRANCH_TABLE = [
    # ---- sequence.hip: the pointwise gate block ------------------------------------------------------------------------------------
    ("yt8m_lstm_gates_fwd", "B >= 0 && H >= 0 / B * H == 0 / null, else YT8M_E_*", "(none)", "test_refusals[gates_fwd]; test_zero_size_calls"),
    ("yt8m_lstm_gates_fwd", "(single kernel) live = nf ? t < nf[b] : true; out may be NULL", "lstm_gates_fwd_kernel",
     "test_lstm_gates_kernels[5-12], [33-192] (nf ragged / NULL, out given / NULL); every generic LSTM case"),
    ("yt8m_lstm_gates_bwd", "B >= 0 && H >= 0 / B * H == 0 / null, else YT8M_E_*", "(none)", "test_refusals[gates_bwd]; test_zero_size_calls"),
    ("yt8m_lstm_gates_bwd", "(single kernel) dout may be NULL", "lstm_gates_bwd_kernel",
     "test_lstm_gates_kernels (dout given / NULL); the first launch of every packed backward range"),
    # ---- sequence.hip: whole-layer drivers -----------------------------------------------------------------------------------------
    ("yt8m_lstm_layer_fwd", "negative / zero size / null / ldw < 4 * H, else YT8M_E_*", "(none)", "test_refusals[layer_fwd]; test_zero_size_calls"),
    ("yt8m_lstm_layer_fwd", "gemm_workspace && lstm_fused_supported(B, H, gemm_workspace_bytes): cell_pack + lstm_step_fwd per step",
     "lstm_pack_kernel " + _F % (4, 0, 2), "test_lstm_layer_packed[B-H-F]: H = 128, 256, 384, B = 1, 16, 17, 32, 33, F = 1, 5; ldw = 4H + 64"),
    ("yt8m_lstm_layer_fwd", "else: grouped GEMM + lstm_gates_fwd per step", "lstm_gates_fwd_kernel",
     "test_lstm_layer_generic: H = 12, 192, H = 128 with the workspace 4 bytes short, H = 128 with a NULL workspace (the GEMM takes S = 1)"),
    ("yt8m_lstm_layer_bwd", "negative / zero size / null / ldw < 4 * H, else YT8M_E_*", "(none)", "test_refusals[layer_bwd]; test_zero_size_calls"),
    ("yt8m_lstm_layer_bwd", "seed_state: dh_final / dc_final given (copy) or NULL (memset)", "(none)", "test_lstm_layer_packed / _generic: finals given and NULL"),
    ("yt8m_lstm_layer_bwd", "gemm_workspace && lstm_fused_supported: cell_pack (Wq) + lstm_bwd_range_packed",
     "lstm_pack_kernel lstm_gates_bwd_kernel " + _B % (2, 2) + " " + _B % (0, 2),
     "test_lstm_layer_packed: F = 1 (gate kernel + plain product only), F = 5 (four fused launches); dout given / NULL"),
    ("yt8m_lstm_layer_bwd", "else: lstm_gates_bwd + grouped GEMM per step", "lstm_gates_bwd_kernel", "test_lstm_layer_generic"),
    # ---- sequence.hip: time-range forms --------------------------------------------------------------------------------------------
    ("yt8m_lstm_packed_floats", "lstm_fused_supported(B, H, 4 * H * 4H) ? H * 4 * H : 0", "(none)", "test_support_queries: H = 128, 384 / 12, 192, 64; B = 0"),
    ("yt8m_lstm_pack", "Wh && H > 0 && ldw >= 4 * H && (Wp || Wq) / H % 128, else YT8M_E_*", "(none)", "test_refusals[pack]: H = 192, both destinations NULL, ldw < 4H"),
    ("yt8m_lstm_pack", "(single kernel) Wp and / or Wq", "lstm_pack_kernel", "every packed time-range case packs Wp alone and Wq alone; ldw = 4H + 64"),
    ("yt8m_lstm_steps_fwd", "negative / zero size / null / ldw < 4 * H, else YT8M_E_*", "(none)", "test_refusals[steps_fwd]; test_zero_size_calls"),
    ("yt8m_lstm_steps_fwd", "!Wp: direct issue (grouped GEMM + gate kernel), no capture", "lstm_gates_fwd_kernel",
     "test_lstm_time_ranges[generic-*]: (5, 12), (33, 192), and (33, 128) with Wp NULL; graph statistics unchanged"),
    ("yt8m_lstm_steps_fwd", "Wp && !lstm_fused_supported(B, H, .): YT8M_E_SHAPE", "(none)", "test_refusals[steps_fwd]: Wp given at H = 192"),
    ("yt8m_lstm_steps_fwd", "Wp: run_chain(graph_key(1, ...)) over lstm_step_fwd", _F % (4, 0, 2),
     "test_lstm_time_ranges[packed-*]: T = 1 at t0 = 0 and t0 = 3, ranges (0, 2) + (2, 3); test_graph_capture_and_replay"),
    ("yt8m_lstm_steps_bwd", "negative / phase not 0 or 1 / zero size / null / ldw < 4 * H, else YT8M_E_*", "(none)", "test_refusals[steps_bwd]: phase = 2; test_zero_size_calls"),
    ("yt8m_lstm_steps_bwd", "Wq && !lstm_fused_supported: YT8M_E_SHAPE", "(none)", "test_refusals[steps_bwd]: Wq given at H = 192"),
    ("yt8m_lstm_steps_bwd", "!Wq: direct issue, lstm_bwd_range generic arm", "lstm_gates_bwd_kernel", "test_lstm_time_ranges[generic-*]; phase 0 and 1"),
    ("yt8m_lstm_steps_bwd", "Wq: run_chain(graph_key(2, ...)); T = 1: gate kernel + add_dzWt (BEP 0)", "lstm_gates_bwd_kernel " + _B % (0, 2),
     "test_lstm_time_ranges[packed-*]: T = 1 at t0 = 0 and 3, phase 0 and 1; the bare product"),
    ("yt8m_lstm_steps_bwd", "Wq, t > t_lo: lstm_step_bwd_fused (BEP 2)", _B % (2, 2),
     "test_lstm_time_ranges[packed-*]: T = 2 (one fused launch), ranges (2, 3) + (0, 2); test_graph_capture_and_replay"),
    # ---- lstm_fused.hip ------------------------------------------------------------------------------------------------------------
    ("yt8m_lstm_steps_fwd", "lstm_step_fwd: step_mode(0) = 2 (default \"2122\"); in kernel: row >= B clamped, nf NULL, out NULL, !live copy-through",
     _F % (4, 0, 2), "B = 1, 17, 33 (partial 32-row tiles), 16, 32; H = 128 (one 32-k block per wave), 256, 384 (48 groups)"),
    ("yt8m_lstm_steps_fwd", "step_mode(0) = 0 / 1 / 3", " ".join(_F % (4, 0, m) for m in (0, 1, 3)), _MODES_CHILD),
    ("yt8m_lstm_steps_bwd", "step_mode(2) = 0 / 1 / 3", " ".join(_B % (b, m) for b in (0, 2) for m in (0, 1, 3)), _MODES_CHILD),
    ("yt8m_lnlstm_layer_fwd", "cell_step_add4: step_mode(0) = 0 / 1 / 3", " ".join(_F % (4, 1, m) for m in (0, 1, 3)), _MODES_CHILD),
    ("yt8m_gru_layer_fwd", "gru_step_gates / gru_step_cand: step_mode(1) = 0 / 2 / 3",
     " ".join(_F % (g, e, m) for g, e in ((2, 2), (1, 3)) for m in (0, 2, 3)), _MODES_CHILD),
    ("yt8m_gru_layer_bwd", "gru_step_bwd_cand / cell_step_bwd(G = 2): step_mode(3) = 0 / 1 / 3", " ".join(_B % (1, m) for m in (0, 1, 3)), _MODES_CHILD),
    # ---- lstm_bf16.hip -------------------------------------------------------------------------------------------------------------
    ("yt8m_lstm_packed16_elems", "B >= 1 && H >= 256 && H % 256 == 0 ? H * 4 * H : 0", "(none)", "test_support_queries: H = 256, 512 / 128, 384"),
    ("yt8m_lstm_pack_bf16", "bad operand / H % 256, else YT8M_E_*", "(none)", "test_refusals[pack_bf16]: H = 128, both NULL, ldw < 4H"),
    ("yt8m_lstm_pack_bf16", "(single kernel)", "lstm_pack16_kernel", "test_lstm_bf16[*]: Wp16 and Wq16 in one call; ldw = 4H + 64"),
    ("yt8m_lstm_steps_fwd_bf16", "negative / zero size / null / H % 256, else YT8M_E_*", "(none)", "test_refusals[steps_fwd_bf16]: H = 128; test_zero_size_calls"),
    ("yt8m_lstm_steps_fwd_bf16", "run_chain(graph_key(3, ...))", "lstm_step_fwd16_kernel", "test_lstm_bf16[B-H]: H = 256, 512, B = 1, 17, 33; T = 1 at t0 = 1, T = 3"),
    ("yt8m_lstm_steps_bwd_bf16", "negative / phase / zero size / null / H % 256, else YT8M_E_*", "(none)", "test_refusals[steps_bwd_bf16]: H = 128, phase = 2"),
    ("yt8m_lstm_steps_bwd_bf16", "run_chain(graph_key(4, ...)): gate kernel + cast, t == t0: plain product", "lstm_gates_bwd_kernel cast_rows16_kernel lstm_step_bwd16_kernel<false>",
     "test_lstm_bf16: T = 1 reaches <false> only"),
    ("yt8m_lstm_steps_bwd_bf16", "t > t0: fused", "lstm_step_bwd16_kernel<true>", "test_lstm_bf16: T = 3, phase 1 on entry"),
    # ---- cells.hip: GRU ------------------------------------------------------------------------------------------------------------
    ("yt8m_gru_layer_fwd", "negative / zero size / null / ldg < 2 * H || ldc < H, else YT8M_E_*", "(none)", "test_refusals[gru_fwd]; test_zero_size_calls"),
    ("yt8m_gru_layer_fwd", "packed_ok(B, H, 3, ws, bytes): H % 256 == 0 && bytes >= 4 * 3 * H * H", "lstm_pack_kernel " + _F % (2, 2, 1) + " " + _F % (1, 3, 1),
     "test_gru_layer[packed-*]: H = 256, B = 1, 17, 33, F = 1, 5; ldg = 2H + 32, ldc = H + 32"),
    ("yt8m_gru_layer_fwd", "else: grouped GEMM + gru_gates_kernel + grouped GEMM + gru_out_kernel", "gru_gates_kernel gru_out_kernel",
     "test_gru_layer[generic-*]: H = 128 (the LSTM packs at this H, the cells do not), H = 12, H = 256 with the workspace one float short"),
    ("yt8m_gru_layer_fwd", "YT8M_NO_PACKED_CELLS set: generic at a packed shape", "gru_gates_kernel gru_out_kernel", _MODES_CHILD),
    ("yt8m_gru_layer_bwd", "negative / zero size / null / leading dimensions, else YT8M_E_*", "(none)", "test_refusals[gru_bwd]; test_zero_size_calls"),
    ("yt8m_gru_layer_bwd", "packed: gru_bwd1 + gru_step_bwd_cand (BEP 1) + add_dzWt(G = 2, BEP 0 at K < 4H)",
     "lstm_pack_kernel gru_bwd1_kernel " + _B % (1, 2) + " " + _B % (0, 2), "test_gru_layer[packed-*]; dout / dh_final given and NULL"),
    ("yt8m_gru_layer_bwd", "!packed: gru_bwd1 + GEMM + gru_bwd2 + GEMM", "gru_bwd1_kernel gru_bwd2_kernel", "test_gru_layer[generic-*]"),
    # ---- cells.hip: LayerNorm-LSTM -------------------------------------------------------------------------------------------------
    ("yt8m_lnlstm_layer_fwd", "negative / H > 256 * ROW_PT / keep_prob not in (0, 1] / zero size / null / ldw, else YT8M_E_*", "(none)",
     "test_refusals[lnlstm_fwd]: H = 2049, keep_prob 0 and 1.5; test_zero_size_calls"),
    ("yt8m_lnlstm_layer_fwd", "packed_ok(B, H, 4, ...): cell_step_add4 (EP_ADD)", "lstm_pack_kernel " + _F % (4, 1, 2),
     "test_lnlstm_layer[512], [768], [1024], [1280], [2048]; the bare product of step 0"),
    ("yt8m_lnlstm_layer_fwd", "YT8M_ROW_KERNEL: H <= 512", "lnlstm_fwd_kernel<2>", "test_lnlstm_layer[12], [300] (generic product, ragged tail), [512] (packed)"),
    ("yt8m_lnlstm_layer_fwd", "YT8M_ROW_KERNEL: H <= 1024", "lnlstm_fwd_kernel<4>", "test_lnlstm_layer[513] (ragged tail of one unit), [768], [1024]"),
    ("yt8m_lnlstm_layer_fwd", "YT8M_ROW_KERNEL: else (ROW_PT)", "lnlstm_fwd_kernel<8>", "test_lnlstm_layer[1025] (ragged), [1280], [2048]"),
    ("yt8m_lnlstm_layer_bwd", "negative / H > 2048 / keep_prob / zero size / null / ldw, else YT8M_E_*", "(none)", "test_refusals[lnlstm_bwd]; test_zero_size_calls"),
    ("yt8m_lnlstm_layer_bwd", "packed: add_dzWt (BEP 0, K = 4H)", "lstm_pack_kernel " + _B % (0, 2), "test_lnlstm_layer: the packed H; F = 1: the bare product"),
    ("yt8m_lnlstm_layer_bwd", "YT8M_ROW_KERNEL: H <= 512 / <= 1024 / else", "lnlstm_bwd_kernel<2> lnlstm_bwd_kernel<4> lnlstm_bwd_kernel<8>", "test_lnlstm_layer (the H of the forward rows)"),
    ("yt8m_lnlstm_layer_fwd", "YT8M_NO_PACKED_CELLS set: generic at a packed shape", "lnlstm_fwd_kernel<2>", _MODES_CHILD),
    # ---- step_kernels.h / runtime.hip: capture and replay ---------------------------------------------------------------------------
    ("yt8m_lstm_steps_fwd", "run_chain: key not cached (capture) / cached (replay) / another forget_bias (a second capture)", _F % (4, 0, 2),
     "test_graph_capture_and_replay: the replay is held to the fp64 of the NEW data"),
    ("yt8m_lstm_steps_fwd", "run_chain: YT8M_NO_GRAPH set: direct issue", _F % (4, 0, 2), _MODES_CHILD + " (bits equal to the parent's captured run)"),
    ("yt8m_lstm_steps_fwd", "run_chain: capture refused by the runtime (fallbacks)", "(none)", "left out: needs a stream that cannot be captured; every case asserts fallbacks == 0"),
]

OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-6
U = 2.0 ** -24
PAD = 256
SENT = -7.0
F64, F32 = torch.float64, torch.float32
OK, E_BADARG, E_SHAPE = 0, -1, -2
WORST = {}                       # quantity -> (err, fp32 restatement's err, case)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


class G:
    """An operand of a given shape inside a larger buffer whose margins hold `fill` (the sentinel for outputs, NaN for operands that are
    only read).  seal() records every bit after the host wrote its inputs; only(...) then asserts that nothing but the named part of
    the operand changed -- margins, the rows of other steps, read operands."""

    def __init__(self, dev, shape, dtype=F32, fill=SENT, src=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape)) if len(shape) else 1
        self.buf = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.t = self.buf[PAD:PAD + self.n].view(self.shape)
        if src is not None:
            self.t.copy_(src)
        self.snap = None

    def seal(self):
        self.snap = _bits(self.buf).clone()
        return self

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def changed(self):
        ch = _bits(self.buf) != self.snap
        assert not bool(ch[:PAD].any()) and not bool(ch[PAD + self.n:].any()), "a margin was written"
        return ch[PAD:PAD + self.n].view(self.shape)

    def only(self, *index):
        ch = self.changed().clone()
        if index:
            ch[index if len(index) > 1 else index[0]] = False
        return not bool(ch.any())


def _ro(dev, src):
    """a read-only operand: NaN margins, sealed"""
    return G(dev, src.shape, src.dtype, float("nan") if src.dtype.is_floating_point else -1, src).seal()


def _P(x):
    return None if x is None else (x.p if isinstance(x, G) else ctypes.c_void_p(x.data_ptr()))


def _padded(dev, W, ld):
    """W [rows, cols] with leading dimension ld: 1e3 in the padding columns (a read of them would wreck every value), NaN around"""
    g = G(dev, (W.shape[0], ld), F32, float("nan"))
    g.t.fill_(1.0e3)
    g.t[:, :W.shape[1]] = W
    return g.seal()


class Check:
    """collects the figures of one case, prints each next to its bound, fails at the end with every miss"""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def _note(self, name, e, f, b):
        print("%s %s: err %.3g (fp32 %.3g, bound %.3g)" % (self.tag, name, e, f, b))
        key = "%s: %s" % (" ".join(self.tag.split()[:2]), re.sub(r"\[.*?\]", "", name))
        if not (e <= WORST.get(key, (-1.0,))[0]):
            WORST[key] = (e, f, self.tag)
        if not e <= b:
            self.bad.append("%s: err %.6g > bound %.6g" % (name, e, b))

    def hold(self, name, got, r64, r32, grad=False, tol=None):
        if r64.numel() == 0:
            return
        f = R.err(r32, r64)
        self._note(name, R.err(got, r64), f, tol if tol is not None else R.bound(r64, r32, GRAD_FLOOR if grad else OUT_FLOOR))

    def absolute(self, name, got, r64, bound):
        self._note(name, float((got.double().cpu() - r64).abs().max()), float("nan"), bound)

    def product(self, name, got, ref64, absprod64, K):
        """element by element: |got - ref| <= (K + 4 + 2) u (|A| |B|)_ij + u |ref|; prints the largest ratio to the bound (bound 1)"""
        b = (K + 6) * U * absprod64 + U * ref64.abs() + 1e-30
        self._note(name + " / elementwise bound", float(((got.double().cpu() - ref64).abs() / b).max()), float("nan"), 1.0)

    def true(self, name, cond):
        if not cond:
            self.bad.append(name)

    def done(self):
        assert not self.bad, "%s: %s" % (self.tag, "; ".join(self.bad))


def _graph_stats():
    v = [ctypes.c_int64(0) for _ in range(4)]
    L.check(L.lib().yt8m_graph_cache_stats(*[ctypes.byref(x) for x in v]))
    return dict(zip(("hits", "captures", "fallbacks", "entries"), (x.value for x in v)))


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _ragged(rs, B, F):
    """ragged lengths that always hold F, 0 and 1 (as far as B rows allow)"""
    nf = rs.randint(0, F + 1, size=B).astype(np.int32)
    for k, v in enumerate((F, 0, 1)):
        if k < B:
            nf[k] = v
    return nf


def _wh(rs, H, G_, gain=3.0):
    """recurrent weights [H, G H] at a trained cell's scale: `gain` times the Glorot limit, so that the gates leave their linear range"""
    lim = gain * np.sqrt(6.0 / (H + G_ * H))
    return torch.from_numpy(((rs.random_sample((H, G_ * H)) * 2 - 1) * lim).astype(np.float32))


def _randn(rs, *shape, scale=1.0):
    return torch.from_numpy((scale * rs.randn(*shape)).astype(np.float32))


def _live(nf, t0, T, B):
    return torch.stack([R.live_rows(nf, t, B) for t in range(t0, t0 + T)])


@pytest.fixture(scope="module")
def stream(dev):
    return torch.cuda.Stream(dev)


@pytest.fixture(autouse=True)
def side_stream(stream):
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def worst_errors():
    yield
    print("\nLARGEST ERRORS PER QUANTITY")
    for k in sorted(WORST):
        print("  %s: %.2g [%.2g] (%s)" % ((k,) + WORST[k]))


# =================================================================================================================================
# BasicLSTM
class LstmCase:
    """Inputs of one (B, H) layer over S tape steps, and the tape an fp64 forward leaves (rounded to float32): the host writes the state
    of any step from it, and the backward cases read its gates and cell states.  Nothing here comes from the device."""

    def __init__(self, B, H, S, seed, fb=1.0, bf16=False, nf=True):
        rs = np.random.RandomState(seed)
        self.B, self.H, self.S, self.fb, self.bf16 = B, H, S, fb, bf16
        self.z = _randn(rs, S, B, 4 * H, scale=0.8)
        self.Wh = _wh(rs, H, 4)
        self.nf = _ragged(rs, B, S) if nf else None
        c0 = _randn(rs, B, H, scale=0.5)
        h0 = torch.from_numpy(rs.uniform(-0.9, 0.9, size=(B, H)).astype(np.float32))
        self.dout = _randn(rs, S, B, H)
        self.dh0, self.dc0 = _randn(rs, B, H), _randn(rs, B, H)
        cs = torch.zeros((S + 1, B, H), dtype=F64)
        hs = torch.zeros((S + 1, B, H), dtype=F64)
        cs[0], hs[0] = c0.double(), (R.bf16r(h0) if bf16 else h0).double()
        f = R.lstm_range_fwd(self.z.double(), self.Wh.double(), cs, hs, self.nf, 0, S, fb, bf16)
        lv = _live(self.nf, 0, S, B)[:, :, None]
        self.gates = torch.where(lv, f["gates"], f["pre"]).float()
        self.cs = f["cs"].float()
        self.hs = R.bf16r(f["hs"].float()) if bf16 else f["hs"].float()         # bf16 forms: every host-written h is exact in bf16


def _pack16(dev, c, Whd, ldw):
    wp, wq = (G(dev, (c.H * 4 * c.H,), torch.bfloat16) for _ in range(2))
    L.check(L.lib().yt8m_lstm_pack_bf16(Whd.p, ldw, c.H, wp.p, wq.p, _st()))
    torch.cuda.synchronize()
    return wp.seal(), wq.seal()


class LstmFwd:
    """One forward call: route "packed" (Wp given / the whole-layer form with a workspace that fits), "generic" (no Wp / a workspace
    that does not fit) or "bf16"; entry "steps" or "layer" (t0 = 0)."""

    def __init__(self, dev, c, route, t0, T, entry="steps", ldw_pad=0, out=True, ws_bytes=None, ws_null=False):
        B, H, S = c.B, c.H, c.S
        self.dev, self.c, self.route, self.t0, self.T, self.entry = dev, c, route, t0, T, entry
        self.ldw = 4 * H + ldw_pad
        self.z, self.cs, self.hs = G(dev, (S, B, 4 * H)), G(dev, (S + 1, B, H)), G(dev, (S + 1, B, H))
        self.out = G(dev, (S, B, H)) if out else None
        self.hs16 = G(dev, (S + 1, B, H), torch.bfloat16) if route == "bf16" else None
        self.nf = None if c.nf is None else torch.from_numpy(c.nf).to(dev)
        if ws_bytes is None:
            ws_bytes = 4 * H * 4 * H if route == "packed" else (1 << 20)
        self.ws = None if ws_null else G(dev, (ws_bytes,), torch.uint8, 0xA5).seal()
        self.ws_bytes = 0 if ws_null else ws_bytes
        self.Wp = None
        self.load(c)

    def load(self, c):
        """the inputs of case c into the same buffers (the replay of a captured chain reads them there)"""
        self.c, t0, T = c, self.t0, self.T
        for g in (self.z, self.cs, self.hs, self.out, self.hs16):
            if g is not None:
                g.buf.fill_(SENT)
        if self.nf is not None:
            self.nf.copy_(torch.from_numpy(c.nf))                  # the pointer is part of a captured chain's key, the contents are read at replay
        self.z.t[t0:t0 + T] = c.z[t0:t0 + T]
        self.cs.t[t0], self.hs.t[t0] = c.cs[t0], c.hs[t0]
        if self.hs16 is not None:
            self.hs16.t[t0] = c.hs[t0].to(torch.bfloat16)
        self.Wh = _padded(self.dev, c.Wh, self.ldw)
        if self.entry == "steps" and self.route == "packed":
            if self.Wp is None:
                self.Wp = G(self.dev, (c.H * 4 * c.H,))
            L.check(L.lib().yt8m_lstm_pack(self.Wh.p, self.ldw, c.H, self.Wp.p, None, _st()))
            torch.cuda.synchronize()
            self.Wp.seal()
        if self.route == "bf16":
            self.Wp, _ = _pack16(self.dev, c, self.Wh, self.ldw)
        for g in (self.z, self.cs, self.hs, self.out, self.hs16):
            if g is not None:
                g.seal()

    def call(self, fb=None):
        c, lib = self.c, L.lib()
        fb = c.fb if fb is None else fb
        self.fb = fb
        if self.route == "bf16":
            rc = lib.yt8m_lstm_steps_fwd_bf16(self.z.p, self.Wp.p, self.cs.p, self.hs.p, self.hs16.p, _P(self.out), _P(self.nf), self.t0, self.T,
                                              c.B, c.H, fb, _st())
        elif self.entry == "layer":
            assert self.t0 == 0
            rc = lib.yt8m_lstm_layer_fwd(self.z.p, self.Wh.p, self.ldw, self.cs.p, self.hs.p, _P(self.out), _P(self.nf), self.T, c.B, c.H, fb,
                                         _P(self.ws), self.ws_bytes, _st())
        else:
            rc = lib.yt8m_lstm_steps_fwd(self.z.p, self.Wh.p, self.ldw, _P(self.Wp), self.cs.p, self.hs.p, _P(self.out), _P(self.nf), self.t0,
                                         self.T, c.B, c.H, fb, _P(self.ws), self.ws_bytes, _st())
        L.check(rc)
        torch.cuda.synchronize()

    def check(self, tag):
        c, t0, T, B = self.c, self.t0, self.T, self.c.B
        bf16, k = self.route == "bf16", Check(tag)
        rng, nxt = slice(t0, t0 + T), slice(t0 + 1, t0 + T + 1)
        ref = {dt: R.lstm_range_fwd(c.z.to(dt), c.Wh.to(dt), c.cs.to(dt), c.hs.to(dt), c.nf, t0, T, self.fb, bf16) for dt in (F64, F32)}
        r64, r32 = ref[F64], ref[F32]
        tol = 2e-3 if bf16 and T > 1 else None
        lv = _live(c.nf, t0, T, B)
        zg, csg, hsg = self.z.t[rng].cpu(), self.cs.t[t0:t0 + T + 1].cpu(), self.hs.t[t0:t0 + T + 1].cpu()
        k.hold("gates", zg[lv], r64["gates"][lv], r32["gates"][lv], tol=tol)
        if self.route == "generic":             # the GEMM adds h . Wh to every row; the gate kernel leaves the rows without a frame as they are
            k.hold("z of rows past num_frames", zg[~lv], r64["pre"][~lv], r32["pre"][~lv])
        else:
            k.true("z of rows past num_frames changed", _same_bits(zg[~lv], c.z[rng][~lv]))
        k.hold("cs", csg[1:], r64["cs"][1:], r32["cs"][1:], tol=tol)
        k.hold("hs", hsg[1:], r64["hs"][1:], r32["hs"][1:], tol=tol)
        k.true("state of rows past num_frames not copied bit for bit",
               _same_bits(csg[1:][~lv], csg[:-1][~lv]) and _same_bits(hsg[1:][~lv], hsg[:-1][~lv]))
        k.true("z: a step outside the range or a margin was written", self.z.only(rng))
        k.true("cs / hs: a slot outside the range was written", self.cs.only(nxt) and self.hs.only(nxt))
        if self.out is not None:
            og = self.out.t[rng].cpu()
            k.hold("out", og, r64["out"], r32["out"], tol=tol)
            k.true("out of rows past num_frames is not +0", bool((_bits(og[~lv]) == 0).all()))
            k.true("out: a step outside the range was written", self.out.only(rng))
        if bf16:
            k.true("hs16 is not the bf16 rounding of hs", _same_bits(self.hs16.t[nxt].cpu(), hsg[1:].to(torch.bfloat16)))
            k.true("hs16: a slot outside the range was written", self.hs16.only(nxt))
        k.true("W_h or packed weights changed", self.Wh.only() and (self.Wp is None or self.Wp.only()))
        k.true("workspace margin", self.ws is None or self.ws.changed() is not None)
        k.done()
        return self


class LstmBwd:
    """One backward call over steps [t0, t0 + T) on the tape of the case (gates, cs written by the host)."""

    def __init__(self, dev, c, route, t0, T, entry="steps", phase=0, ldw_pad=0, dout=True, finals=True, ws_bytes=None, ws_null=False):
        B, H, S = c.B, c.H, c.S
        self.dev, self.route, self.t0, self.T, self.entry, self.phase, self.finals = dev, route, t0, T, entry, phase, finals
        self.ldw, self.with_dout = 4 * H + ldw_pad, dout
        self.dz, self.work = G(dev, (S, B, 4 * H)), G(dev, (4, B, H))
        self.dz16 = G(dev, (S, B, 4 * H), torch.bfloat16) if route == "bf16" else None
        nan = float("nan")
        self.gates, self.cs = G(dev, (S, B, 4 * H), fill=nan), G(dev, (S + 1, B, H), fill=nan)
        self.dout = G(dev, (S, B, H), fill=nan) if dout else None
        self.nf = None if c.nf is None else torch.from_numpy(c.nf).to(dev)
        if ws_bytes is None:
            ws_bytes = 4 * H * 4 * H if route == "packed" else (1 << 20)
        self.ws = None if ws_null else G(dev, (ws_bytes,), torch.uint8, 0xA5).seal()
        self.ws_bytes = 0 if ws_null else ws_bytes
        self.Wq = None
        self.load(c)

    def load(self, c):
        self.c, dev = c, self.dev
        for g in (self.dz, self.work, self.dz16):
            if g is not None:
                g.buf.fill_(SENT)
        for g, src in ((self.gates, c.gates), (self.cs, c.cs), (self.dout, c.dout)):   # the same buffers: a captured chain reads them at replay
            if g is not None:
                g.t.copy_(src)
                g.seal()
        if self.nf is not None:
            self.nf.copy_(torch.from_numpy(c.nf))
        zero = torch.zeros_like(c.dh0)
        self.seed = (c.dh0, c.dc0) if self.finals else (zero, zero)
        hc, cc = R.halves(self.phase)[:2]
        if self.entry == "steps":               # the caller seeds the running gradients; the whole-layer form seeds them itself
            self.work.t[hc], self.work.t[cc] = self.seed
        else:
            self.dhf, self.dcf = (_ro(dev, c.dh0), _ro(dev, c.dc0)) if self.finals else (None, None)
        self.Wh = _padded(dev, c.Wh, self.ldw)
        if self.entry == "steps" and self.route == "packed":
            if self.Wq is None:
                self.Wq = G(dev, (c.H * 4 * c.H,))
            L.check(L.lib().yt8m_lstm_pack(self.Wh.p, self.ldw, c.H, None, self.Wq.p, _st()))
            torch.cuda.synchronize()
            self.Wq.seal()
        if self.route == "bf16":
            _, self.Wq = _pack16(dev, c, self.Wh, self.ldw)
        for g in (self.dz, self.work, self.dz16):
            if g is not None:
                g.seal()

    def call(self):
        c, lib = self.c, L.lib()
        if self.route == "bf16":
            rc = lib.yt8m_lstm_steps_bwd_bf16(self.gates.p, self.Wq.p, self.cs.p, _P(self.dout), self.dz.p, self.dz16.p, self.work.p, self.phase,
                                              _P(self.nf), self.t0, self.T, c.B, c.H, _st())
        elif self.entry == "layer":
            assert self.t0 == 0 and self.phase == 0
            rc = lib.yt8m_lstm_layer_bwd(self.gates.p, self.Wh.p, self.ldw, self.cs.p, _P(self.dout), _P(self.dcf), _P(self.dhf), self.dz.p,
                                         self.work.p, _P(self.nf), self.T, c.B, c.H, _P(self.ws), self.ws_bytes, _st())
        else:
            rc = lib.yt8m_lstm_steps_bwd(self.gates.p, self.Wh.p, self.ldw, _P(self.Wq), self.cs.p, _P(self.dout), self.dz.p, self.work.p,
                                         self.phase, _P(self.nf), self.t0, self.T, c.B, c.H, _P(self.ws), self.ws_bytes, _st())
        L.check(rc)
        torch.cuda.synchronize()

    def check(self, tag):
        c, t0, T, B, H = self.c, self.t0, self.T, self.c.B, self.c.H
        bf16, k = self.route == "bf16", Check(tag)
        rng = slice(t0, t0 + T)
        hc, cc, hp, cp = R.halves(self.phase)
        ref = {}
        for dt in (F64, F32):
            w0 = torch.zeros((4, B, H), dtype=dt)
            w0[hc], w0[cc] = self.seed[0].to(dt), self.seed[1].to(dt)
            ref[dt] = R.lstm_range_bwd(c.gates.to(dt), c.cs.to(dt), c.Wh.to(dt), c.dout.to(dt) if self.with_dout else None, w0, self.phase,
                                       c.nf, t0, T, bf16)
        (dz64, w64, ph), (dz32, w32, _) = ref[F64], ref[F32]
        fh, fc = R.halves(ph)[:2]
        lv = _live(c.nf, t0, T, B)
        dzg, wg = self.dz.t[rng].cpu(), self.work.t.cpu()
        if bf16:
            scale = 2e-3 * float(dz64.abs().max())
            if T == 1:
                k.hold("dz[T=1]", dzg, dz64, dz32, grad=True)       # the pointwise kernel alone: no product upstream
            else:
                k.absolute("dz, bf16", dzg, dz64, scale)
            k.absolute("dh, bf16", wg[fh], w64[fh], scale)
            k.absolute("dc, bf16", wg[fc], w64[fc], scale)
            k.true("dz16 is not the bf16 rounding of dz", _same_bits(self.dz16.t[rng].cpu(), dzg.to(torch.bfloat16)))
            k.true("dz16: a step outside the range was written", self.dz16.only(rng))
        else:
            k.hold("dz", dzg, dz64, dz32, grad=True)
            k.hold("dh", wg[fh], w64[fh], w32[fh], grad=True)
            k.hold("dc", wg[fc], w64[fc], w32[fc], grad=True)
        k.true("dz of rows past num_frames is not +0", bool((_bits(dzg[~lv]) == 0).all()))
        k.true("dz: a step outside the range or a margin was written", self.dz.only(rng))
        if c.nf is not None:
            dead = torch.from_numpy(c.nf <= t0)                    # no frame in the whole range: (dh, dc) carried unchanged
            k.true("(dh, dc) of rows without frames not carried bit for bit",
                   _same_bits(wg[fh][dead], self.seed[0][dead]) and _same_bits(wg[fc][dead], self.seed[1][dead]))
        if T == 1:
            if self.entry == "steps":
                k.true("T = 1: the half of work the step reads was written", self.work.only(slice(2 * (1 - self.phase), 2 * (1 - self.phase) + 2)))
            if self.route != "generic":          # BEP 0 / <false>: dh = carried part + dz . Wh^T, A = the dz this call wrote
                A = (R.bf16r(dzg[0]) if bf16 else dzg[0]).double()
                Bm = (R.bf16r(c.Wh) if bf16 else c.Wh).double()
                carried = torch.where(lv[0][:, None], torch.zeros((B, H), dtype=F64), self.seed[0].double())
                k.product("dh = dz . Wh^T", wg[fh], carried + A @ Bm.t(), A.abs() @ Bm.abs().t(), 4 * H)
        k.true("a read operand changed", self.gates.only() and self.cs.only() and self.Wh.only() and (self.dout is None or self.dout.only())
               and (self.Wq is None or self.Wq.only()))
        k.true("workspace margin", self.ws is None or self.ws.changed() is not None)
        k.done()
        return self


def _no_graph_traffic(before):
    d = _delta(before, _graph_stats())
    return d["captures"] == 0 and d["hits"] == 0 and d["fallbacks"] == 0


def test_support_queries():
    lib = L.lib()
    for H in (128, 256, 384, 1024):
        assert lib.yt8m_lstm_packed_floats(1, H) == H * 4 * H and lib.yt8m_lstm_packed_floats(33, H) == H * 4 * H
    for B, H in ((1, 12), (1, 192), (1, 64), (0, 128), (1, 0)):
        assert lib.yt8m_lstm_packed_floats(B, H) == 0
    for H in (256, 512):
        assert lib.yt8m_lstm_packed16_elems(1, H) == H * 4 * H
    for B, H in ((1, 128), (1, 384), (0, 256), (33, 12)):
        assert lib.yt8m_lstm_packed16_elems(B, H) == 0


@pytest.mark.parametrize("B,H", [(5, 12), (33, 192)])
def test_lstm_gates_kernels(dev, B, H):
    """yt8m_lstm_gates_fwd / _bwd alone: one step from a host-written state, ragged num_frames and NULL, out / dout given and NULL."""
    lib = L.lib()
    for variant, (nf_on, out_on) in enumerate(((True, True), (False, False))):
        c = LstmCase(B, H, 3, 10 * B + H + variant, fb=1.0 if variant == 0 else 0.0, nf=nf_on)
        t = 1
        k = Check("gates kernels B=%d H=%d %s:" % (B, H, "ragged, out" if nf_on else "nf NULL, out NULL"))
        lv = R.live_rows(c.nf, t, B)
        # forward: z holds the finished pre-activation (the product is the caller's)
        pre = (c.z[t].double() + c.hs[t].double() @ c.Wh.double()).float()
        z, cp, hp = G(dev, (B, 4 * H), src=pre).seal(), _ro(dev, c.cs[t]), _ro(dev, c.hs[t])
        cn, hn, out = G(dev, (B, H)).seal(), G(dev, (B, H)).seal(), G(dev, (B, H)).seal() if out_on else None
        nf = None if c.nf is None else torch.from_numpy(c.nf).to(dev)
        L.check(lib.yt8m_lstm_gates_fwd(z.p, cp.p, hp.p, cn.p, hn.p, _P(out), _P(nf), t, B, H, c.fb, _st()))
        torch.cuda.synchronize()
        zeroW = torch.zeros((H, 4 * H))
        r = {dt: R.lstm_step_fwd(pre.to(dt), zeroW.to(dt), c.cs[t].to(dt), c.hs[t].to(dt), lv, c.fb) for dt in (F64, F32)}
        zg = z.t.cpu()
        k.hold("gates", zg[lv], r[F64][1][lv], r[F32][1][lv])
        k.true("z of rows past num_frames changed", _same_bits(zg[~lv], pre[~lv]))
        k.hold("c", cn.t, r[F64][2], r[F32][2])
        k.hold("h", hn.t, r[F64][3], r[F32][3])
        k.true("state not copied bit for bit", _same_bits(cn.t.cpu()[~lv], c.cs[t][~lv]) and _same_bits(hn.t.cpu()[~lv], c.hs[t][~lv]))
        if out is not None:
            k.hold("out", out.t, r[F64][4], r[F32][4])
            k.true("out of rows past num_frames is not +0", bool((_bits(out.t.cpu()[~lv]) == 0).all()))
        k.true("margins / read operands", all(g.changed() is not None for g in (z, cn, hn)) and cp.only() and hp.only())
        # backward
        gates, cprev, cnew, dh, dc = _ro(dev, c.gates[t]), _ro(dev, c.cs[t]), _ro(dev, c.cs[t + 1]), _ro(dev, c.dh0), _ro(dev, c.dc0)
        dout = _ro(dev, c.dout[t]) if out_on else None
        dz, dcp, dhp = G(dev, (B, 4 * H)).seal(), G(dev, (B, H)).seal(), G(dev, (B, H)).seal()
        L.check(lib.yt8m_lstm_gates_bwd(gates.p, cprev.p, cnew.p, dh.p, dc.p, _P(dout), dz.p, dcp.p, dhp.p, _P(nf), t, B, H, _st()))
        torch.cuda.synchronize()
        r = {dt: R.lstm_gates_bwd(c.gates[t].to(dt), c.cs[t].to(dt), c.cs[t + 1].to(dt), c.dh0.to(dt), c.dc0.to(dt),
                                  c.dout[t].to(dt) if out_on else None, lv) for dt in (F64, F32)}
        for name, g, i in (("dz", dz, 0), ("dc_prev", dcp, 1), ("dh_prev", dhp, 2)):
            k.hold(name, g.t, r[F64][i], r[F32][i], grad=True)
        k.true("dz of rows past num_frames is not +0", bool((_bits(dz.t.cpu()[~lv]) == 0).all()))
        k.true("(dh, dc) not carried bit for bit", _same_bits(dhp.t.cpu()[~lv], c.dh0[~lv]) and _same_bits(dcp.t.cpu()[~lv], c.dc0[~lv]))
        k.true("dh_prev of live rows is not +0", bool((_bits(dhp.t.cpu()[lv]) == 0).all()))
        k.true("margins / read operands", all(g.changed() is not None for g in (dz, dcp, dhp)) and all(g.only() for g in (gates, cprev, cnew, dh, dc)))
        k.done()


PACKED_LAYER = [(B, 128, F) for B in (1, 16, 17, 32, 33) for F in (1, 5)] + [(33, 256, 1), (17, 256, 5), (33, 384, 1), (17, 384, 5)]


@pytest.mark.parametrize("B,H,F", PACKED_LAYER)
def test_lstm_layer_packed(dev, B, H, F):
    """yt8m_lstm_layer_fwd / _bwd on the packed route (workspace exactly 4 * H * 4H bytes) from a host-written state: F = 1 is the
    single step (gate kernel + plain product backward), F = 5 the chain.  ldw = 4H + 64 with 1e3 in the padding columns; the first
    variant has num_frames, out, dout and the final-state gradients, the second has them NULL and forget_bias 0."""
    for variant in (0, 1):
        full = variant == 0
        c = LstmCase(B, H, F, 7 * B + H + F + variant, fb=1.0 if full else 0.0, nf=full)
        tag = "lstm layer packed B=%d H=%d F=%d %s" % (B, H, F, "full" if full else "NULLs fb=0")
        before = _graph_stats()
        f = LstmFwd(dev, c, "packed", 0, F, entry="layer", ldw_pad=64, out=full)
        f.call()
        f.check(tag + " fwd:")
        assert not f.ws.only()                                     # the packed weights went into the workspace
        b = LstmBwd(dev, c, "packed", 0, F, entry="layer", ldw_pad=64, dout=full, finals=full)
        b.call()
        b.check(tag + " bwd:")
        assert not b.ws.only() and _no_graph_traffic(before)       # the whole-layer forms issue directly


GENERIC_LAYER = {"H12": (5, 12, {}), "H192": (33, 192, {}), "H128-workspace-4-bytes-short": (33, 128, dict(ws_bytes=4 * 128 * 512 - 4)),
                 "H128-null-workspace": (17, 128, dict(ws_null=True))}


@pytest.mark.parametrize("name", sorted(GENERIC_LAYER))
@pytest.mark.parametrize("F", [1, 5])
def test_lstm_layer_generic(dev, name, F):
    """The grouped-GEMM route of the whole-layer forms: H = 12, H = 192 (above 128, no multiple), H = 128 with a workspace 4 bytes too
    small for the packed weights, H = 128 without a workspace (the GEMM then takes no K split)."""
    B, H, kw = GENERIC_LAYER[name]
    c = LstmCase(B, H, F, 3 * B + H + F)
    tag = "lstm layer generic %s F=%d" % (name, F)
    LstmFwd(dev, c, "generic", 0, F, entry="layer", **kw).call_and_check(tag + " fwd:")
    LstmBwd(dev, c, "generic", 0, F, entry="layer", **kw).call_and_check(tag + " bwd:")


def _cc(self, tag):
    self.call()
    return self.check(tag)


LstmFwd.call_and_check = _cc
LstmBwd.call_and_check = _cc

RANGE_CASES = {"packed-33-128": ("packed", 33, 128), "packed-17-256": ("packed", 17, 256), "packed-1-384": ("packed", 1, 384),
               "generic-5-12": ("generic", 5, 12), "generic-33-192": ("generic", 33, 192), "generic-33-128-no-Wp": ("generic", 33, 128)}


@pytest.mark.parametrize("name", sorted(RANGE_CASES))
def test_lstm_time_ranges(dev, name):
    """yt8m_lstm_steps_fwd / _bwd over a tape of 5 steps, every range against fp64 from the state the host wrote: T = 1 at t0 = 0 and
    t0 = 3 (the sharp single steps; backward entered with phase 0 and 1), T = 2 (one fused backward launch), the ranges (0, 2) + (2, 3)
    forward and (2, 3) + (0, 2) backward with the carried phase.  Tape slots and dz steps outside [t0, t0 + T) keep their sentinel."""
    route, B, H = RANGE_CASES[name]
    c = LstmCase(B, H, 5, 11 * B + H)
    L.check(L.lib().yt8m_graph_cache_clear())
    before = _graph_stats()
    calls = 0
    for t0, T in ((0, 1), (3, 1), (0, 2), (2, 3)):
        LstmFwd(dev, c, route, t0, T, ldw_pad=64 if t0 == 3 else 0, out=t0 != 3).call_and_check("lstm steps %s fwd t0=%d T=%d:" % (name, t0, T))
        calls += 1
    for t0, T, phase in ((0, 1, 0), (3, 1, 1), (1, 2, 1), (2, 3, 0), (0, 2, 1)):
        LstmBwd(dev, c, route, t0, T, phase=phase, ldw_pad=64 if t0 == 3 else 0, dout=t0 != 3).call_and_check(
            "lstm steps %s bwd t0=%d T=%d phase=%d:" % (name, t0, T, phase))
        calls += 1
    c0 = LstmCase(B, H, 5, 11 * B + H + 1, nf=False)                # num_frames NULL: every row runs every step
    LstmFwd(dev, c0, route, 1, 2).call_and_check("lstm steps %s fwd t0=1 T=2 nf NULL:" % name)
    LstmBwd(dev, c0, route, 1, 2).call_and_check("lstm steps %s bwd t0=1 T=2 nf NULL:" % name)
    calls += 2
    d = _delta(before, _graph_stats())
    # every packed call has its own buffers: one capture each; the generic form issues directly
    assert d == (dict(hits=0, captures=calls, fallbacks=0, entries=calls) if route == "packed" else dict(hits=0, captures=0, fallbacks=0, entries=0)), d


def test_lstm_two_ranges_carry_the_phase(dev):
    """(2, 3) then (0, 2) backward in ONE work buffer with phase' = (phase + T) % 2 carried, and (0, 2) then (2, 3) forward in one tape,
    packed at (33, 128): the whole tape against fp64."""
    c = LstmCase(33, 128, 5, 99)
    f = LstmFwd(dev, c, "packed", 0, 5)
    f.t0, f.T = 0, 2
    f.call()
    f.t0, f.T = 2, 3
    f.call()
    f.t0, f.T = 0, 5
    f.check("lstm steps packed fwd ranges (0,2)+(2,3):")
    b = LstmBwd(dev, c, "packed", 0, 5, phase=1)
    b.t0, b.T = 2, 3
    b.call()
    b.t0, b.T, b.phase = 0, 2, (1 + 3) % 2
    b.call()
    b.t0, b.T, b.phase = 0, 5, 1
    b.check("lstm steps packed bwd ranges (2,3)+(0,2) from phase 1:")


def test_graph_capture_and_replay(dev):
    """run_chain after yt8m_graph_cache_clear: a call captures; the same call over NEW data in the same buffers replays and is held to
    the fp64 of the new data; the same pointers with another forget_bias capture a second graph."""
    lib = L.lib()
    B, H, T = 33, 128, 3
    c1, c2 = LstmCase(B, H, T, 1), LstmCase(B, H, T, 2)
    L.check(lib.yt8m_graph_cache_clear())
    s0 = _graph_stats()
    f = LstmFwd(dev, c1, "packed", 0, T)
    f.call()
    f.check("graph fwd, captured:")
    assert _delta(s0, _graph_stats()) == dict(hits=0, captures=1, fallbacks=0, entries=1)
    f.load(c2)
    f.call()
    f.check("graph fwd, replayed over new data:")
    assert _delta(s0, _graph_stats()) == dict(hits=1, captures=1, fallbacks=0, entries=1)
    f.load(c2)
    f.call(fb=0.0)
    f.check("graph fwd, another forget_bias:")
    assert _delta(s0, _graph_stats()) == dict(hits=1, captures=2, fallbacks=0, entries=2)
    b = LstmBwd(dev, c1, "packed", 0, T)
    b.call()
    b.check("graph bwd, captured:")
    assert _delta(s0, _graph_stats()) == dict(hits=1, captures=3, fallbacks=0, entries=3)
    b.load(c2)
    b.call()
    b.check("graph bwd, replayed over new data:")
    assert _delta(s0, _graph_stats()) == dict(hits=2, captures=3, fallbacks=0, entries=3)


@pytest.mark.parametrize("B,H", [(1, 256), (17, 256), (33, 256), (17, 512)])
def test_lstm_bf16(dev, B, H):
    """The bf16-operand forms: T = 1 from an h that is exact in bf16 (forward under the float32 rule; backward reaches
    lstm_step_bwd16_kernel<false> only), T = 3 (the fused <true> launches, phase 1 on entry)."""
    c = LstmCase(B, H, 4, 5 * B + H, bf16=True)
    tag = "lstm bf16 B=%d H=%d" % (B, H)
    LstmFwd(dev, c, "bf16", 1, 1, ldw_pad=64).call_and_check(tag + " fwd t0=1 T=1:")
    LstmFwd(dev, c, "bf16", 0, 3, out=False).call_and_check(tag + " fwd t0=0 T=3:")
    LstmBwd(dev, c, "bf16", 2, 1, ldw_pad=64).call_and_check(tag + " bwd t0=2 T=1:")
    LstmBwd(dev, c, "bf16", 1, 3, phase=1, dout=False).call_and_check(tag + " bwd t0=1 T=3 phase=1:")
    c0 = LstmCase(B, H, 2, 5 * B + H + 1, bf16=True, nf=False)
    LstmFwd(dev, c0, "bf16", 0, 2).call_and_check(tag + " fwd t0=0 T=2 nf NULL:")
    LstmBwd(dev, c0, "bf16", 0, 2).call_and_check(tag + " bwd t0=0 T=2 nf NULL:")


# =================================================================================================================================
# GRU
def _gru_run(dev, tag, B, H, F, seed, full=True, ldg_pad=0, ldc_pad=0, ws_bytes=None, expect_packed=None):
    lib = L.lib()
    rs = np.random.RandomState(seed)
    zg, zc = _randn(rs, F, B, 2 * H, scale=0.8), _randn(rs, F, B, H, scale=0.8)
    Wg, Wc = _wh(rs, H, 2), _wh(rs, H, 1)
    nf = _ragged(rs, B, F) if full else None
    h0 = torch.from_numpy(rs.uniform(-0.9, 0.9, size=(B, H)).astype(np.float32))
    dout, dhf = (_randn(rs, F, B, H), _randn(rs, B, H))
    dout, dhf = (dout, dhf) if full else (None, None)
    ldg, ldc = 2 * H + ldg_pad, H + ldc_pad
    ws_bytes = 4 * 3 * H * H if ws_bytes is None else ws_bytes
    k = Check(tag)
    ref = {dt: R.gru_layer(zg.to(dt), zc.to(dt), Wg.to(dt), Wc.to(dt), nf, None if dout is None else dout.to(dt),
                           None if dhf is None else dhf.to(dt), h0=h0.to(dt)) for dt in (F64, F32)}
    r64, r32 = ref[F64], ref[F32]
    lv = _live(nf, 0, F, B)
    nfd = None if nf is None else torch.from_numpy(nf).to(dev)
    Wgd, Wcd = _padded(dev, Wg, ldg), _padded(dev, Wc, ldc)
    # forward
    zgd, zcd = G(dev, (F, B, 2 * H), src=zg).seal(), G(dev, (F, B, H), src=zc).seal()
    hs = G(dev, (F + 1, B, H))
    hs.t[0] = h0
    hs.seal()
    rh, out = G(dev, (F, B, H)).seal(), G(dev, (F, B, H)).seal() if full else None
    ws = G(dev, (ws_bytes,), torch.uint8, 0xA5).seal()
    L.check(lib.yt8m_gru_layer_fwd(zgd.p, zcd.p, Wgd.p, ldg, Wcd.p, ldc, hs.p, rh.p, _P(out), _P(nfd), F, B, H, ws.p, ws_bytes, _st()))
    torch.cuda.synchronize()
    if expect_packed:
        k.true("packed route not taken (the workspace holds no packed weights)", not ws.only())
    for name, g in (("zg", zgd), ("zc", zcd), ("rh", rh)):
        k.hold(name, g.t, r64[name], r32[name])
        k.true(name + " margin", g.changed() is not None)
    hg = hs.t.cpu()
    k.hold("hs", hg[1:], r64["hs"][1:], r32["hs"][1:])
    k.true("h of rows past num_frames not copied bit for bit", _same_bits(hg[1:][~lv], hg[:-1][~lv]))
    k.true("hs[0] or a margin was written", hs.only(slice(1, F + 1)))
    if out is not None:
        k.hold("out", out.t, r64["out"], r32["out"])
        k.true("out of rows past num_frames is not +0", bool((_bits(out.t.cpu()[~lv]) == 0).all()) and out.changed() is not None)
    k.true("weights changed", Wgd.only() and Wcd.only())
    # backward on the tape the host wrote
    zga, zca, hsa = _ro(dev, r64["zg"].float()), _ro(dev, r64["zc"].float()), _ro(dev, r64["hs"].float())
    b = {}
    for dt in (F64, F32):                     # the same float32 tape in both precisions
        ru, cc, hh = r64["zg"].float().to(dt), r64["zc"].float().to(dt), r64["hs"].float().to(dt)
        dh = torch.zeros((B, H), dtype=dt) if dhf is None else dhf.to(dt)
        dzg, dzc = [], []
        for t in range(F - 1, -1, -1):
            a, bb, dh = R.gru_step_bwd(ru[t], cc[t], hh[t], dh, None if dout is None else dout[t].to(dt), Wg.to(dt), Wc.to(dt), R.live_rows(nf, t, B))
            dzg.insert(0, a), dzc.insert(0, bb)
        b[dt] = (torch.stack(dzg), torch.stack(dzc), dh)
    doutd, dhfd = (None if dout is None else _ro(dev, dout)), (None if dhf is None else _ro(dev, dhf))
    dzgd, dzcd, work = G(dev, (F, B, 2 * H)).seal(), G(dev, (F, B, H)).seal(), G(dev, (3, B, H)).seal()
    ws2 = G(dev, (ws_bytes,), torch.uint8, 0xA5).seal()
    L.check(lib.yt8m_gru_layer_bwd(zga.p, zca.p, Wgd.p, ldg, Wcd.p, ldc, hsa.p, _P(doutd), _P(dhfd), dzgd.p, dzcd.p, work.p, _P(nfd), F, B, H,
                                   ws2.p, ws_bytes, _st()))
    torch.cuda.synchronize()
    k.hold("dzg", dzgd.t, b[F64][0], b[F32][0], grad=True)
    k.hold("dzc", dzcd.t, b[F64][1], b[F32][1], grad=True)
    wg = work.t.cpu()
    k.hold("dh", wg[F % 2], b[F64][2], b[F32][2], grad=True)
    k.true("dzg / dzc of rows past num_frames are not +0", bool((_bits(dzgd.t.cpu()[~lv]) == 0).all()) and bool((_bits(dzcd.t.cpu()[~lv]) == 0).all()))
    if nf is not None and dhf is not None:
        dead = torch.from_numpy(nf == 0)
        k.true("dh of rows without frames not carried bit for bit", _same_bits(wg[F % 2][dead], dhf[dead]))
    k.true("margins / read operands", all(g.changed() is not None for g in (dzgd, dzcd, work, ws2)) and
           all(g.only() for g in (zga, zca, hsa, Wgd, Wcd)) and (doutd is None or doutd.only()))
    if expect_packed:
        k.true("packed backward wrote the GEMM's drh scratch", work.only(slice(0, 2)))
        k.true("packed route not taken (backward)", not ws2.only())
    k.done()


GRU_CASES = [("packed", B, 256, F, {}) for B in (1, 17, 33) for F in (1, 5)] + [
    ("generic", 17, 128, 1, {}), ("generic", 17, 128, 5, {}), ("generic", 5, 12, 1, {}), ("generic", 5, 12, 5, {}),
    ("generic", 17, 256, 1, dict(ws_bytes=4 * 3 * 256 * 256 - 4)), ("generic", 33, 256, 5, dict(ws_bytes=4 * 3 * 256 * 256 - 4))]


@pytest.mark.parametrize("route,B,H,F,kw", GRU_CASES, ids=["%s-%d-%d-%d%s" % (r, b, h, f, "-short" if kw else "") for r, b, h, f, kw in GRU_CASES])
def test_gru_layer(dev, route, B, H, F, kw):
    """yt8m_gru_layer_fwd / _bwd from a host-written h0: F = 1 is the single step, F = 5 the chain; first with num_frames, out, dout and
    dh_final and ldg = 2H + 32, ldc = H + 32, then with all of them NULL and dense weights."""
    for full in (True, False):
        _gru_run(dev, "gru %s B=%d H=%d F=%d %s:" % (route, B, H, F, "full" if full else "NULLs"), B, H, F, 13 * B + H + F + int(full), full=full,
                 ldg_pad=32 if full else 0, ldc_pad=32 if full else 0, expect_packed=route == "packed", **kw)


# =================================================================================================================================
# LayerNorm-LSTM
LN_SEED = 0x1234567


def _ln_run(dev, tag, B, H, F, keep, seed, full=True):
    lib = L.lib()
    rs = np.random.RandomState(seed)
    fb = 1.0 if full else 0.0
    z = _randn(rs, F, B, 4 * H, scale=0.8)
    Wh = _wh(rs, H, 4)
    gamma = torch.from_numpy((1.0 + 0.3 * rs.randn(5, H)).astype(np.float32))
    beta = torch.from_numpy((0.3 * rs.randn(5, H)).astype(np.float32))
    nf = _ragged(rs, B, F) if full else None
    c0 = _randn(rs, B, H, scale=0.5)
    h0 = torch.from_numpy(rs.uniform(-0.9, 0.9, size=(B, H)).astype(np.float32))
    dout, dcf, dhf = (_randn(rs, F, B, H), _randn(rs, B, H), _randn(rs, B, H)) if full else (None, None, None)
    ldw = 4 * H + (64 if full else 0)
    packed = H % 256 == 0 and os.environ.get("YT8M_NO_PACKED_CELLS") is None
    ws_bytes = 4 * H * 4 * H if H % 256 == 0 else (1 << 20)
    k = Check(tag)
    ref = {dt: R.lnlstm_layer(z.to(dt), Wh.to(dt), gamma.to(dt), beta.to(dt), nf, fb, keep, LN_SEED, backward=False, c0=c0.to(dt), h0=h0.to(dt))
           for dt in (F64, F32)}
    r64, r32 = ref[F64], ref[F32]
    lv = _live(nf, 0, F, B)
    nfd = None if nf is None else torch.from_numpy(nf).to(dev)
    Whd, gd, bd = _padded(dev, Wh, ldw), _ro(dev, gamma), _ro(dev, beta)
    zd = G(dev, (F, B, 4 * H), src=z).seal()
    stats, out = G(dev, (F, B, 10)).seal(), G(dev, (F, B, H)).seal() if full else None
    cs, hs = G(dev, (F + 1, B, H)), G(dev, (F + 1, B, H))
    cs.t[0], hs.t[0] = c0, h0
    cs.seal(), hs.seal()
    ws = G(dev, (ws_bytes,), torch.uint8, 0xA5).seal()
    L.check(lib.yt8m_lnlstm_layer_fwd(zd.p, Whd.p, ldw, gd.p, bd.p, stats.p, cs.p, hs.p, _P(out), _P(nfd), F, B, H, fb, keep, LN_SEED, ws.p,
                                      ws_bytes, _st()))
    torch.cuda.synchronize()
    zg, sg, cg, hg = zd.t.cpu(), stats.t.cpu(), cs.t.cpu(), hs.t.cpu()
    if packed:
        k.true("packed route not taken (the workspace holds no packed weights)", not ws.only())
    k.hold("z (raw)", zg, r64["z"], r32["z"])
    if packed:                                   # EP_ADD exposes the bare product: step 0, A = the host's h0
        A, Bm = h0.double(), Wh.double()
        k.product("z[0] = z + h0 . Wh", zg[0], z[0].double() + A @ Bm, A.abs() @ Bm.abs(), H)
    k.hold("stats", sg[lv], r64["stats"][lv], r32["stats"][lv])
    k.true("stats of rows past num_frames were written", bool((_bits(sg[~lv]) == _bits(torch.tensor(SENT))).all()))
    k.hold("cs", cg[1:], r64["cs"][1:], r32["cs"][1:])
    k.hold("hs", hg[1:], r64["hs"][1:], r32["hs"][1:])
    k.true("state of rows past num_frames not copied bit for bit", _same_bits(cg[1:][~lv], cg[:-1][~lv]) and _same_bits(hg[1:][~lv], hg[:-1][~lv]))
    k.true("cs[0] / hs[0] or a margin was written", cs.only(slice(1, F + 1)) and hs.only(slice(1, F + 1)))
    if out is not None:
        k.hold("out", out.t, r64["out"], r32["out"])
        k.true("out of rows past num_frames is not +0", bool((_bits(out.t.cpu()[~lv]) == 0).all()) and out.changed() is not None)
    k.true("margins / read operands", zd.changed() is not None and stats.changed() is not None and ws.changed() is not None and
           Whd.only() and gd.only() and bd.only())
    # backward on the tape the host wrote (raw z, stats, cs of the fp64 forward, rounded to float32)
    zt, ct = r64["z"].float(), r64["cs"].float()
    st = torch.where(lv[:, :, None], r64["stats"].float(), torch.full((), SENT))
    b = {}
    for dt in (F64, F32):
        dh = torch.zeros((B, H), dtype=dt) if dhf is None else dhf.to(dt)
        dc = torch.zeros((B, H), dtype=dt) if dcf is None else dcf.to(dt)
        Wd, gmd, btd = Wh.to(dt), gamma.to(dt), beta.to(dt)
        dz, dyb, dyg = [], [], []
        for t in range(F - 1, -1, -1):
            a, bb, g2, dc, dh = R.lnlstm_step_bwd(zt[t].to(dt), Wd, gmd, btd, ct[t].to(dt), ct[t + 1].to(dt), dh, dc,
                                                  None if dout is None else dout[t].to(dt), R.live_rows(nf, t, B), fb,
                                                  R.keep_scale(t, B, H, keep, LN_SEED, dt))
            dz.insert(0, a), dyb.insert(0, bb), dyg.insert(0, g2)
        b[dt] = dict(dz=torch.stack(dz), dyb=torch.stack(dyb), dyg=torch.stack(dyg), dh=dh, dc=dc)
    ztd, std, ctd = _ro(dev, zt), _ro(dev, st), _ro(dev, ct)
    doutd, dcfd, dhfd = (None if a is None else _ro(dev, a) for a in (dout, dcf, dhf))
    dzd, dybd, dygd, work = G(dev, (F, B, 4 * H)).seal(), G(dev, (F, B, 5 * H)).seal(), G(dev, (F, B, 5 * H)).seal(), G(dev, (4, B, H)).seal()
    ws2 = G(dev, (ws_bytes,), torch.uint8, 0xA5).seal()
    L.check(lib.yt8m_lnlstm_layer_bwd(ztd.p, Whd.p, ldw, gd.p, bd.p, std.p, ctd.p, _P(doutd), _P(dcfd), _P(dhfd), dzd.p, dybd.p, dygd.p, work.p,
                                      _P(nfd), F, B, H, fb, keep, LN_SEED, ws2.p, ws_bytes, _st()))
    torch.cuda.synchronize()
    fh, fc = R.halves(F % 2)[:2]
    wg, dzg = work.t.cpu(), dzd.t.cpu()
    for name, g in (("dz", dzd), ("dyb", dybd), ("dyg", dygd)):
        k.hold(name, g.t, b[F64][name], b[F32][name], grad=True)
        k.true(name + " of rows past num_frames is not +0", bool((_bits(g.t.cpu()[~lv]) == 0).all()) and g.changed() is not None)
    k.hold("dh", wg[fh], b[F64]["dh"], b[F32]["dh"], grad=True)
    k.hold("dc", wg[fc], b[F64]["dc"], b[F32]["dc"], grad=True)
    if nf is not None:
        dead = torch.from_numpy(nf == 0)
        k.true("(dh, dc) of rows without frames not carried bit for bit", _same_bits(wg[fh][dead], dhf[dead]) and _same_bits(wg[fc][dead], dcf[dead]))
    if packed and F == 1:                        # BEP 0 exposes the bare product, A = the dz this call wrote
        A, Bm = dzg[0].double(), Wh.double()
        carried = torch.where(lv[0][:, None], torch.zeros((B, H), dtype=F64), (torch.zeros((B, H)) if dhf is None else dhf).double())
        k.product("dh = dz . Wh^T", wg[fh], carried + A @ Bm.t(), A.abs() @ Bm.abs().t(), 4 * H)
    k.true("margins / read operands", work.changed() is not None and ws2.changed() is not None and
           all(g.only() for g in (ztd, std, ctd, Whd, gd, bd)) and (doutd is None or doutd.only()))
    k.done()


@pytest.mark.parametrize("H", [12, 300, 512, 513, 768, 1024, 1025, 1280, 2048])
def test_lnlstm_layer(dev, H):
    """yt8m_lnlstm_layer_fwd / _bwd at B = 3 from a host-written state: F = 1 (the single step; keep_prob 0.75) and F = 2 with keep_prob
    1.0 (everything given, ldw = 4H + 64) and 0.75 (num_frames, out, dout and the final-state gradients NULL, forget_bias 0)."""
    _ln_run(dev, "lnlstm layer H=%d B=3 F=1 keep=0.75 full:" % H, 3, H, 1, 0.75, 31 + H)
    _ln_run(dev, "lnlstm layer H=%d B=3 F=2 keep=1 full:" % H, 3, H, 2, 1.0, 32 + H)
    _ln_run(dev, "lnlstm layer H=%d B=3 F=2 keep=0.75 NULLs:" % H, 3, H, 2, 0.75, 33 + H, full=False)


def test_lnlstm_layer_two_row_tiles(dev):
    """B = 33: two 32-row tiles forward and three 16-row tiles backward in the packed products, H = 256 (PT = 2)."""
    _ln_run(dev, "lnlstm layer H=256 B=33 F=2 keep=0.75 full:", 33, 256, 2, 0.75, 77)
    _ln_run(dev, "lnlstm layer H=256 B=33 F=1 keep=1 full:", 33, 256, 1, 1.0, 78)


# =================================================================================================================================
# refusals and zero-size calls
def _entry(dev, name, B=3, H=12, F=2, **over):
    """(function, argument list, outputs) of a well-formed call of an entry point on sentinel-filled buffers; `over` replaces arguments by
    name.  Nothing here is meant to run a kernel: the buffers are sized for the shape, so that a refusal that fails to refuse is a wrong
    return code, not a fault."""
    lib = L.lib()
    Bq, Hq, Fq = max(B, 1), max(H, 1), max(F, 1)
    g = lambda *shape, **kw: G(dev, shape, **kw).seal()
    z, dz, gates = g(Fq, Bq, 4 * Hq), g(Fq, Bq, 4 * Hq), g(Fq, Bq, 4 * Hq)
    cs, hs, out, dout = g(Fq + 1, Bq, Hq), g(Fq + 1, Bq, Hq), g(Fq, Bq, Hq), g(Fq, Bq, Hq)
    Wh, Wx = g(Hq, 4 * Hq), g(Hq * 4 * Hq)
    work, fin = g(4, Bq, Hq), g(Bq, Hq)
    nf = G(dev, (Bq,), torch.int32, 1).seal()
    ws = G(dev, (1 << 16,), torch.uint8, 0xA5).seal()
    st = _st()
    A = {
        "gates_fwd": (lib.yt8m_lstm_gates_fwd, [("z", z), ("c_prev", cs), ("h_prev", hs), ("c_new", out), ("h_new", dout), ("out", work), ("nf", nf),
                                                ("t", 0), ("B", B), ("H", H), ("fb", 1.0)], [z, out, dout, work]),
        "gates_bwd": (lib.yt8m_lstm_gates_bwd, [("gates", gates), ("c_prev", cs), ("c_new", hs), ("dh", fin), ("dc", out), ("dout", dout), ("dz", dz),
                                                ("dc_prev", work), ("dh_prev", z), ("nf", nf), ("t", 0), ("B", B), ("H", H)], [dz, work, z]),
        "layer_fwd": (lib.yt8m_lstm_layer_fwd, [("z", z), ("Wh", Wh), ("ldw", 4 * H), ("cs", cs), ("hs", hs), ("out", out), ("nf", nf), ("F", F),
                                                ("B", B), ("H", H), ("fb", 1.0), ("ws", ws), ("ws_bytes", ws.n)], [z, cs, hs, out, ws]),
        "layer_bwd": (lib.yt8m_lstm_layer_bwd, [("gates", gates), ("Wh", Wh), ("ldw", 4 * H), ("cs", cs), ("dout", dout), ("dcf", fin), ("dhf", fin),
                                                ("dz", dz), ("work", work), ("nf", nf), ("F", F), ("B", B), ("H", H), ("ws", ws), ("ws_bytes", ws.n)],
                      [dz, work, ws]),
        "pack": (lib.yt8m_lstm_pack, [("Wh", Wh), ("ldw", 4 * H), ("H", H), ("Wp", Wx), ("Wq", z)], [Wx, z]),
        "steps_fwd": (lib.yt8m_lstm_steps_fwd, [("z", z), ("Wh", Wh), ("ldw", 4 * H), ("Wp", None), ("cs", cs), ("hs", hs), ("out", out), ("nf", nf),
                                                ("t0", 0), ("T", F), ("B", B), ("H", H), ("fb", 1.0), ("ws", ws), ("ws_bytes", ws.n)],
                      [z, cs, hs, out, ws]),
        "steps_bwd": (lib.yt8m_lstm_steps_bwd, [("gates", gates), ("Wh", Wh), ("ldw", 4 * H), ("Wq", None), ("cs", cs), ("dout", dout), ("dz", dz),
                                                ("work", work), ("phase", 0), ("nf", nf), ("t0", 0), ("T", F), ("B", B), ("H", H), ("ws", ws),
                                                ("ws_bytes", ws.n)], [dz, work, ws]),
        "pack_bf16": (lib.yt8m_lstm_pack_bf16, [("Wh", Wh), ("ldw", 4 * H), ("H", H), ("Wp", Wx), ("Wq", z)], [Wx, z]),
        "steps_fwd_bf16": (lib.yt8m_lstm_steps_fwd_bf16, [("z", z), ("Wp", Wx), ("cs", cs), ("hs", hs), ("hs16", dout), ("out", out), ("nf", nf),
                                                          ("t0", 0), ("T", F), ("B", B), ("H", H), ("fb", 1.0)], [z, cs, hs, dout, out]),
        "steps_bwd_bf16": (lib.yt8m_lstm_steps_bwd_bf16, [("gates", gates), ("Wq", Wx), ("cs", cs), ("dout", dout), ("dz", dz), ("dz16", z),
                                                          ("work", work), ("phase", 0), ("nf", nf), ("t0", 0), ("T", F), ("B", B), ("H", H)],
                           [dz, z, work]),
        "gru_fwd": (lib.yt8m_gru_layer_fwd, [("zg", z), ("zc", out), ("Wg", Wh), ("ldg", 2 * H), ("Wc", Wx), ("ldc", H), ("hs", hs), ("rh", dout),
                                             ("out", work), ("nf", nf), ("F", F), ("B", B), ("H", H), ("ws", ws), ("ws_bytes", ws.n)],
                    [z, out, hs, dout, work, ws]),
        "gru_bwd": (lib.yt8m_gru_layer_bwd, [("zg", gates), ("zc", out), ("Wg", Wh), ("ldg", 2 * H), ("Wc", Wx), ("ldc", H), ("hs", hs), ("dout", dout),
                                             ("dhf", fin), ("dzg", dz), ("dzc", z), ("work", work), ("nf", nf), ("F", F), ("B", B), ("H", H), ("ws", ws),
                                             ("ws_bytes", ws.n)], [dz, z, work, ws]),
        "lnlstm_fwd": (lib.yt8m_lnlstm_layer_fwd, [("z", z), ("Wh", Wh), ("ldw", 4 * H), ("gamma", gates), ("beta", dz), ("stats", work), ("cs", cs),
                                                   ("hs", hs), ("out", out), ("nf", nf), ("F", F), ("B", B), ("H", H), ("fb", 1.0), ("keep", 1.0),
                                                   ("seed", 5), ("ws", ws), ("ws_bytes", ws.n)], [z, work, cs, hs, out, ws]),
        "lnlstm_bwd": (lib.yt8m_lnlstm_layer_bwd, [("z", gates), ("Wh", Wh), ("ldw", 4 * H), ("gamma", cs), ("beta", hs), ("stats", out), ("cs", dout),
                                                   ("dout", fin), ("dcf", None), ("dhf", None), ("dz", dz), ("dyb", z), ("dyg", Wx), ("work", work),
                                                   ("nf", nf), ("F", F), ("B", B), ("H", H), ("fb", 1.0), ("keep", 1.0), ("seed", 5), ("ws", ws),
                                                   ("ws_bytes", ws.n)], [dz, z, Wx, work, ws]),
    }
    fn, args, outs = A[name]
    assert not set(over) - {a for a, _ in args}, (name, over)
    vals = [over.get(a, v) for a, v in args]
    vals = [dict(args)[v] if isinstance(v, str) else v for v in vals]       # a string names another argument's buffer
    return fn, [_P(v) if isinstance(v, G) or v is None else v for v in vals] + [st], outs


# entry point -> [(what, expected code, overrides of the well-formed call at (B, H, F) = (3, 12, 2))]
_NEG = [("B < 0", E_SHAPE, dict(B=-1)), ("H < 0", E_SHAPE, dict(H=-1))]
_NEGF = _NEG + [("F < 0", E_SHAPE, dict(F=-1))]
_NEGT = _NEG + [("T < 0", E_SHAPE, dict(T=-1)), ("t0 < 0", E_SHAPE, dict(t0=-1))]
REFUSALS = {
    "gates_fwd": _NEG + [("%s NULL" % a, E_BADARG, {a: None}) for a in ("z", "c_prev", "h_prev", "c_new", "h_new")],
    "gates_bwd": _NEG + [("%s NULL" % a, E_BADARG, {a: None}) for a in ("gates", "c_prev", "c_new", "dh", "dc", "dz", "dc_prev", "dh_prev")],
    "layer_fwd": _NEGF + [("ldw < 4H", E_SHAPE, dict(ldw=47))] + [("%s NULL" % a, E_BADARG, {a: None}) for a in ("z", "Wh", "cs", "hs")],
    "layer_bwd": _NEGF + [("ldw < 4H", E_SHAPE, dict(ldw=47))] + [("%s NULL" % a, E_BADARG, {a: None}) for a in ("gates", "Wh", "cs", "dz", "work")],
    "pack": [("H = 192", E_SHAPE, dict(H=192, ldw=768)), ("H = 12", E_SHAPE, {}), ("both destinations NULL", E_BADARG, dict(H=128, ldw=512, Wp=None, Wq=None)),
             ("ldw < 4H", E_BADARG, dict(H=128, ldw=511)), ("Wh NULL", E_BADARG, dict(H=128, ldw=512, Wh=None)), ("H = 0", E_BADARG, dict(H=0))],
    "steps_fwd": _NEGT + [("ldw < 4H", E_SHAPE, dict(ldw=47)), ("Wp given at H = 192", E_SHAPE, dict(H=192, ldw=768, Wp="z")),
                          ("Wp given at H = 12", E_SHAPE, dict(Wp="z"))] + [("%s NULL" % a, E_BADARG, {a: None}) for a in ("z", "Wh", "cs", "hs")],
    "steps_bwd": _NEGT + [("phase = 2", E_BADARG, dict(phase=2)), ("phase = -1", E_BADARG, dict(phase=-1)), ("ldw < 4H", E_SHAPE, dict(ldw=47)),
                          ("Wq given at H = 192", E_SHAPE, dict(H=192, ldw=768, Wq="dz")), ("Wq given at H = 12", E_SHAPE, dict(Wq="dz"))] +
                 [("%s NULL" % a, E_BADARG, {a: None}) for a in ("gates", "Wh", "cs", "dz", "work")],
    "pack_bf16": [("H = 128", E_SHAPE, dict(H=128, ldw=512)), ("both NULL", E_BADARG, dict(H=256, ldw=1024, Wp=None, Wq=None)),
                  ("ldw < 4H", E_BADARG, dict(H=256, ldw=1023)), ("Wh NULL", E_BADARG, dict(H=256, ldw=1024, Wh=None))],
    "steps_fwd_bf16": _NEGT + [("H = 128", E_SHAPE, dict(H=128)), ("H = 12", E_SHAPE, {})] +
                      [("%s NULL" % a, E_BADARG, {a: None}) for a in ("z", "Wp", "cs", "hs", "hs16")],
    "steps_bwd_bf16": _NEGT + [("H = 128", E_SHAPE, dict(H=128)), ("H = 12", E_SHAPE, {}), ("phase = 2", E_BADARG, dict(phase=2))] +
                      [("%s NULL" % a, E_BADARG, {a: None}) for a in ("gates", "Wq", "cs", "dz", "dz16", "work")],
    "gru_fwd": _NEGF + [("ldg < 2H", E_SHAPE, dict(ldg=23)), ("ldc < H", E_SHAPE, dict(ldc=11))] +
               [("%s NULL" % a, E_BADARG, {a: None}) for a in ("zg", "zc", "Wg", "Wc", "hs", "rh")],
    "gru_bwd": _NEGF + [("ldg < 2H", E_SHAPE, dict(ldg=23)), ("ldc < H", E_SHAPE, dict(ldc=11))] +
               [("%s NULL" % a, E_BADARG, {a: None}) for a in ("zg", "zc", "Wg", "Wc", "hs", "dzg", "dzc", "work")],
    "lnlstm_fwd": _NEGF + [("H = 2049", E_SHAPE, dict(H=2049, ldw=8196)), ("keep_prob 0", E_BADARG, dict(keep=0.0)), ("keep_prob 1.5", E_BADARG, dict(keep=1.5)),
                           ("ldw < 4H", E_SHAPE, dict(ldw=47))] + [("%s NULL" % a, E_BADARG, {a: None}) for a in ("z", "Wh", "gamma", "beta", "stats", "cs", "hs")],
    "lnlstm_bwd": _NEGF + [("H = 2049", E_SHAPE, dict(H=2049, ldw=8196)), ("keep_prob 0", E_BADARG, dict(keep=0.0)), ("keep_prob 1.5", E_BADARG, dict(keep=1.5)),
                           ("ldw < 4H", E_SHAPE, dict(ldw=47))] +
                  [("%s NULL" % a, E_BADARG, {a: None}) for a in ("z", "Wh", "gamma", "beta", "stats", "cs", "dz", "dyb", "dyg", "work")],
}
# the refusals whose well-formed call has no (B, F) of its own or another base shape
_BASE = {"pack": dict(B=1, H=12, F=1), "pack_bf16": dict(B=1, H=12, F=1)}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(dev, name):
    """Every refusal of an entry point: the return code, and no byte of any output or of the workspace changed.  An override given as a
    string names the buffer of the well-formed call that stands in for a packed-weight pointer (the call must refuse before reading it)."""
    for what, code, over in REFUSALS[name]:
        kw = dict(_BASE.get(name, {}))
        kw.update(over)
        fn, args, outs = _entry(dev, name, **kw)
        rc = fn(*args)
        torch.cuda.synchronize()
        print("refusal %s: %s -> %d (%s)" % (name, what, rc, L.lib().yt8m_last_error().decode("utf-8", "replace")))
        assert rc == code, (name, what, rc, code)
        assert all(g.only() for g in outs), (name, what, "an output changed")


ZERO = {"gates_fwd": ("B", "H"), "gates_bwd": ("B", "H"), "layer_fwd": ("F", "B", "H"), "layer_bwd": ("F", "B", "H"), "steps_fwd": ("T", "B", "H"),
        "steps_bwd": ("T", "B", "H"), "steps_fwd_bf16": ("T", "B", "H"), "steps_bwd_bf16": ("T", "B", "H"), "gru_fwd": ("F", "B", "H"),
        "gru_bwd": ("F", "B", "H"), "lnlstm_fwd": ("F", "B", "H"), "lnlstm_bwd": ("F", "B", "H")}


def test_zero_size_calls(dev):
    """A call with a zero dimension returns YT8M_OK and writes nothing -- with every pointer NULL as well."""
    L.check(L.lib().yt8m_graph_cache_clear())
    before = _graph_stats()
    for name, dims in sorted(ZERO.items()):
        for d in dims:
            fn, args, outs = _entry(dev, name, **{d: 0})
            assert fn(*args) == OK, (name, d)
            nulls = [None if isinstance(a, ctypes.c_void_p) else a for a in args[:-1]] + [args[-1]]
            assert fn(*nulls) == OK, (name, d, "NULL pointers")
            torch.cuda.synchronize()
            assert all(g.only() for g in outs), (name, d, "an output changed")
    assert _no_graph_traffic(before)


# =================================================================================================================================
# the process-wide switches: one fresh child process per setting
CHILD_SETTINGS = [("YT8M_STEP_MODE", "0000"), ("YT8M_STEP_MODE", "1111"), ("YT8M_STEP_MODE", "2222"), ("YT8M_STEP_MODE", "3333"),
                  ("YT8M_NO_PACKED_CELLS", "1"), ("YT8M_NO_GRAPH", "1")]


def _digest_case(dev):
    """the bits of one packed time-range forward and backward at (33, 128), T = 3: the same in a process that captures and in one that
    issues directly"""
    c = LstmCase(33, 128, 3, 4242)
    f = LstmFwd(dev, c, "packed", 0, 3).call_and_check("digest lstm steps fwd (33, 128):")
    b = LstmBwd(dev, c, "packed", 0, 3).call_and_check("digest lstm steps bwd (33, 128):")
    h = hashlib.sha1()
    for g in (f.z, f.cs, f.hs, f.out, b.dz, b.work):
        h.update(g.buf.cpu().numpy().tobytes())
    return h.hexdigest()


def _child_cases(dev):
    """one small packed case per kernel class against the same fp64 bounds"""
    c = LstmCase(33, 128, 5, 4243)
    LstmFwd(dev, c, "packed", 3, 1).call_and_check("child lstm steps fwd (33, 128) T=1:")
    LstmFwd(dev, c, "packed", 0, 5).call_and_check("child lstm steps fwd (33, 128) T=5:")
    LstmBwd(dev, c, "packed", 3, 1, phase=1).call_and_check("child lstm steps bwd (33, 128) T=1:")
    LstmBwd(dev, c, "packed", 0, 5).call_and_check("child lstm steps bwd (33, 128) T=5:")
    nopack = os.environ.get("YT8M_NO_PACKED_CELLS") is not None
    for F in (1, 5):
        _gru_run(dev, "child gru (17, 256) F=%d:" % F, 17, 256, F, 500 + F, ldg_pad=32, ldc_pad=32, expect_packed=not nopack)
    for F in (1, 2):
        _ln_run(dev, "child lnlstm (3, 256) F=%d:" % F, 3, 256, F, 0.75, 600 + F)


def _child():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        before = _graph_stats()
        _child_cases(dev)
        d = _delta(before, _graph_stats())
        assert d["fallbacks"] == 0, d
        if os.environ.get("YT8M_NO_GRAPH") is not None:
            assert d["captures"] == 0 and d["hits"] == 0, d
            print("DIGEST %s" % _digest_case(dev))
        else:
            assert d["captures"] == 4, d
    torch.cuda.synchronize()
    print("STEP-CHILD-OK")


def test_step_mode_and_switch_children(dev):
    """YT8M_STEP_MODE (read once per process), YT8M_NO_PACKED_CELLS and YT8M_NO_GRAPH (static reads): a fresh process per setting, one
    after the other, each runs one small packed case per kernel class -- LSTM forward and backward at (33, 128), GRU at (17, 256),
    LN-LSTM at (3, 256) -- against the same fp64 bounds and prints its errors.  The exit status of a child is asserted before the
    next one starts.  The NO_GRAPH child's bits equal this process's captured run of the same case."""
    L.check(L.lib().yt8m_graph_cache_clear())
    mine = _digest_case(dev)
    base = {k: v for k, v in os.environ.items() if k not in {s for s, _ in CHILD_SETTINGS}}
    for var, val in CHILD_SETTINGS:
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child"]
        res = subprocess.run(cmd, env=dict(base, **{var: val}), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True, timeout=240)
        print("---- child %s=%s" % (var, val))
        print(res.stdout)
        assert res.returncode == 0, "the child with %s=%s ended with status %d" % (var, val, res.returncode)
        assert "STEP-CHILD-OK" in res.stdout
        lines = re.findall(r"^(child .*?): err (\S+) \(fp32 \S+, bound (\S+)\)$", res.stdout, re.M)
        assert len(lines) >= 40, len(lines)
        for what, e, b in lines:
            assert float(e) <= float(b), (var, val, what)
        if var == "YT8M_NO_GRAPH":
            assert re.search(r"^DIGEST (\w+)$", res.stdout, re.M).group(1) == mine


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        _child()
    else:
        sys.exit("run this module with pytest -m gpu")
