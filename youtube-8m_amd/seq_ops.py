"""Frame-axis autograd ops over the C ABI: BasicLSTM layer (whole recurrence in one call), attention weights,
NetVLAD assignment / aggregation, batched pooling GEMMs.  See include/yt8m_hip.h for the kernel contracts."""
import ctypes
import os
import warnings
import weakref

import torch

from . import _lib, ops
from .ops import _p, _stream, _dev, _f32c, _token

# ---- switches (environment defaults), each read at call time as an attribute of this module: tests assign to them ----
PERSIST = os.environ.get("YT8M_LSTM_PERSIST", "1") != "0"        # persistent recurrence kernels (csrc/lstm_persist.hip)
PERSIST_BWD = os.environ.get("YT8M_LSTM_PERSIST_BWD", "1") != "0"
# Partition of the time axis when the recurrence runs on the persistent kernels (0: the caller's `chunks`).  A whole-chip forward
# launch leaves no CU for the other layer's projection, so cutting the forward pass only adds launches: ONE chunk.  The backward
# launches take half the chip and run beside the weight-gradient GEMMs: three parts (shorter lone first / last phases and a
# shorter GEMM tail than two; BASELINE configs[3], B = 128: 24.3 ms/step against 24.8 with 2 + 2, 24.4 with 1 + 4).
PERSIST_FWD_CHUNKS = int(os.environ.get("YT8M_LSTM_PERSIST_FWD_CHUNKS", "1"))
PERSIST_BWD_CHUNKS = int(os.environ.get("YT8M_LSTM_PERSIST_BWD_CHUNKS", "3"))
REC_STREAM_PRIORITY = int(os.environ.get("YT8M_REC_STREAM_PRIORITY", "-1"))
PERSIST_STEP_IMAGES = os.environ.get("YT8M_PERSIST_STEP_IMAGES", "1") != "0"
PERSIST_STEP_IMAGES_MAX_BYTES = 8 << 30                 # per layer; larger launches keep the two-image exchange
PERSIST_CHECK = os.environ.get("YT8M_PERSIST_CHECK", "0") == "1"  # debug: synchronise + check the timeout word after each launch
# GRUCell forward on the persistent protocol (csrc/gru_persist.inl); the library switch YT8M_GRU_PERSIST=0 turns it off too.
# Measured at B = 128, H = 1024, F = 300 (profiles/r6_gru_persist.txt): 13.9 us/step in one launch against 17.6 in 600.  A persistent
# backward ran at 29.0 us/step against 20.3 for the per-step launches (two exchange rounds per step on a K = 3H reduction: every
# item's fragment fetch is exposed with four tiles per workgroup) and was removed.
GRU_PERSIST_FWD = os.environ.get("YT8M_GRU_PERSIST_FWD", "1") != "0"
X3 = os.environ.get("YT8M_GEMM_X3", "1") != "0"      # hoisted fp32 products on the bf16 pipe (three-plane split, csrc/gemm_x3.hip)
X3_MIN_ROWS = 1024                                      # F * B below which the fp32-MFMA kernel's smaller tiles win
REC_BF16 = os.environ.get("YT8M_REC_BF16", "1") != "0"       # compute_dtype=bfloat16: bf16 operands for the recurrent product too (csrc/lstm_bf16.hip); False = hoisted
                      # products only
NATIVE_STACK = os.environ.get("YT8M_LSTM_STACK_NATIVE", "1") != "0"   # whole stack behind yt8m_lstm_stack_fwd / _bwd (csrc/lstm_stack.hip)
NATIVE_DROPOUT = os.environ.get("YT8M_NATIVE_DROPOUT", "1") != "0"   # DropoutWrapper inside yt8m_lstm_stack_fwd / _bwd (round 6)
# --compute_dtype=bfloat16 on the native stack (round 4): hoisted products on one-plane bf16 operand images (b1 kernel), the
# recurrence itself on the fp32-grade persistent kernels -- i.e. "bf16 operands" applies to the input projections, dx and the
# weight gradients only (torch_ref.lstm_stack(bf16_operands="input") is its value emulation).  YT8M_LSTM_STACK_BF16=0 keeps the
# Python orchestration with the per-step bf16 recurrence kernels (csrc/lstm_bf16.hip).
NATIVE_BF16 = os.environ.get("YT8M_LSTM_STACK_BF16", "1") != "0"
# Per-layer reports of the native stack's gradients under a reducer (each layer's collective starts when THAT layer's last
# weight-gradient product is done: yt8m_lstm_stack_layer_done_wait).  Opt-in: on one GPU with a 1-rank RCCL group the extra stream
# costs 1.5-1.7 ms of the 23.6 ms step (profiles/r3_force_reducer.md; more hardware queues -- GPU_MAX_HW_QUEUES=8 -- do not help),
# more than the ~0.3 ms of layer-1 all-reduce it can hide on eight.
DP_LAYER_BUCKETS = os.environ.get("YT8M_DP_LAYER_BUCKETS", "0") != "0"
# Clip + Adam of the already-final gradients inside the recurrent stack's backward pass:
# train.TrainGraph.step (single device) leaves its optimiser arguments in graph.early_optimizer before backward(); when the native
# stack's backward pass starts, every trainable variable that has reported its gradient final (Variable.grad_done: for LstmModel the
# MoE head, 97 of 114 M parameters) gets its per-tensor clip + Adam update on the library's weight-gradient stream, behind the
# operand-image preparation and while the top layer's first recurrence runs alone on half the chip
# (yt8m_lstm_stack_set_early_optimizer: the library enqueues it).  The same kernels on the same numbers as the end-of-step pass -- which then only covers what
# is left (graph.early_done).  A side stream that started at once took CUs from that recurrence (25.2 -> 26.7 ms/step in round 2);
# here the recurrence is enqueued first.  YT8M_EARLY_ADAM=0 turns it off.
EARLY_ADAM = os.environ.get("YT8M_EARLY_ADAM", "1") != "0"
# Overlapped directions (opt-in; measured in DESIGN_LOG.md "BiLstmModel"): the bw stack is issued from a side stream on the library's
# second stream set, both directions' forward recurrences capped at half the chip.  The library's residency gate (csrc/lstm_persist.hip,
# PersistGate) admits a persistent launch beside the running ones only while all of them fit the chip together, so two capped
# recurrences run side by side and nothing whole-chip ever overlaps another persistent launch.
BI_OVERLAP = os.environ.get("YT8M_BI_OVERLAP", "0") != "0"
MULTISCALE_FUSED = os.environ.get("YT8M_MULTISCALE_FUSED", "1") != "0"   # 0: the plugin composes the scale from ops.linear / ops.batch_norm / torch
_STACK_SCRATCH_MAX = int(os.environ.get("YT8M_STACK_SCRATCH_MAX", "8"))   # resident scratch buffers of the native stack (a few GB each)

_PERSIST_WS_MAX = 16                                    # resident workspaces of the persistent recurrence launches
U8_BETA = 128.0 * 4.0 / 255.0 + (4.0 / 512.0 - 2.0)     # dequantise(q) = (4/255) (q - 128) + U8_BETA


def _nf(num_frames):
    return None if num_frames is None else num_frames.to(torch.int32).contiguous()


class _LstmLayer(torch.autograd.Function):
    """One BasicLSTMCell layer under tf.nn.dynamic_rnn, time-major.

    x_tm [F,B,in]; W "weights" [in+H, 4H] (rows 0..in-1 act on x_t, the rest on h); b "biases" [4H].
    Returns (out_tm [F,B,H], c_final [B,H], h_final [B,H]).  Forward = one hoisted input GEMM over all steps +
    yt8m_lstm_layer_fwd; backward = yt8m_lstm_layer_bwd + four hoisted GEMMs / column sums."""

    @staticmethod
    def forward(ctx, x_tm, token, W, b, num_frames, forget_bias):
        x_tm = _f32c(x_tm)
        _dev(x_tm)
        F, B, Din = x_tm.shape
        H = W.data.shape[1] // 4
        assert W.data.shape[0] == Din + H, "cell weights must be [in + H, 4H]"
        z = torch.empty((F, B, 4 * H), dtype=torch.float32, device=x_tm.device)
        ops.gemm(x_tm.view(F * B, Din), W.data[:Din], out=z.view(F * B, 4 * H), bias=b.data)
        cs = torch.empty((F + 1, B, H), dtype=torch.float32, device=x_tm.device)
        hs = torch.empty((F + 1, B, H), dtype=torch.float32, device=x_tm.device)
        cs[0].zero_()
        hs[0].zero_()
        out = torch.empty((F, B, H), dtype=torch.float32, device=x_tm.device)
        nf = _nf(num_frames)
        Wh = W.data[Din:]
        ws = ops._workspace(x_tm.device)
        _lib.check(_lib.lib().yt8m_lstm_layer_fwd(_p(z), _p(Wh), 4 * H, _p(cs), _p(hs), _p(out), _p(nf), F, B, H,
                                                  float(forget_bias), _p(ws), ws.numel() * 4, _stream()))
        ctx.save_for_backward(x_tm)
        ctx.state = (z, cs, hs, nf, W, b)
        ctx.set_materialize_grads(False)
        return out, cs[F], hs[F]

    @staticmethod
    def backward(ctx, dout, dc_final, dh_final):
        (x_tm,) = ctx.saved_tensors
        gates, cs, hs, nf, W, b = ctx.state
        ctx.state = None
        F, B, Din = x_tm.shape
        H = W.data.shape[1] // 4
        dev = x_tm.device
        dz = torch.empty((F, B, 4 * H), dtype=torch.float32, device=dev)
        work = torch.empty((4, B, H), dtype=torch.float32, device=dev)
        dout = None if dout is None else _f32c(dout)
        dc_final = None if dc_final is None else _f32c(dc_final)
        dh_final = None if dh_final is None else _f32c(dh_final)
        Wh = W.data[Din:]
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_lstm_layer_bwd(_p(gates), _p(Wh), 4 * H, _p(cs), _p(dout), _p(dc_final), _p(dh_final),
                                                  _p(dz), _p(work), _p(nf), F, B, H, _p(ws), ws.numel() * 4, _stream()))
        dz2 = dz.view(F * B, 4 * H)
        if W.grad is not None:
            beta = W.grad_beta()
            ops.gemm(x_tm.view(F * B, Din), dz2, out=W.grad[:Din], transA=True, beta=beta, role="dw")
            ops.gemm(hs[:F].view(F * B, H), dz2, out=W.grad[Din:], transA=True, beta=beta, role="dw")
            W.grad_done()
        if b.grad is not None:
            ops.colsum(dz2, b.grad.view(-1), beta=b.grad_beta())
            b.grad_done()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dz2, W.data[:Din], transB=True).view(F, B, Din)
        return dx, None, None, None, None, None


def lstm_layer(x_tm, W, b, num_frames, forget_bias=1.0):
    return _LstmLayer.apply(x_tm, _token(W._graph), W, b, num_frames, forget_bias)


class _FloatFrames(object):
    """Float frames x_tm [F,B,D] as a recurrent layer's hoisted input, behind the surface U8FrameImages offers for the reader's bytes:
    F, B, D, device, `saved` (the tensor the layer saves for backward), project / weight_grad / dx."""

    def __init__(self, x_tm, bf16):
        x_tm = _f32c(x_tm)
        _dev(x_tm)
        self.F, self.B, self.D = x_tm.shape
        self.device, self.saved, self.bf16 = x_tm.device, x_tm, bf16
        self.x2 = x_tm.view(self.F * self.B, self.D)

    def project(self, Wrows, bias, out2d):
        ops.hoisted_fwd(self.x2, Wrows, out=out2d, bias=bias, bf16=self.bf16)

    def weight_grad(self, dy2d, gWrows, beta):
        ops.hoisted_dw(self.x2, dy2d, gWrows, beta=beta, bf16=self.bf16)

    def dx(self, dy2d, Wrows, into=None):
        """dx [F,B,D] = dy2d . Wrows^T, added to `into` (an earlier dx of the same frames) where given."""
        out = None if into is None else into.view(self.F * self.B, self.D)
        return ops.hoisted_dx(dy2d, Wrows, out=out, beta=0.0 if into is None else 1.0, bf16=self.bf16).view(self.F, self.B, self.D)


def _hoisted_input(x_tm, bf16):
    """The layer-0 input of a GRU / LayerNorm-LSTM layer: the reader's bytes (U8FrameImages) as they are, float frames wrapped."""
    return x_tm if isinstance(x_tm, U8FrameImages) else _FloatFrames(x_tm, bf16)


class _Hoisted(object):
    """One hoisted input block of a cell layer and its share of backward: z [F B, N] = frames . W + b over all steps at once.  W [D,n]
    and b [n] are detached to contiguous fp32; with pad_to > n both are zero-padded to N = pad_to columns in scratch (the byte
    products' scaled epilogue stores float4: N % 4 == 0) -- the step kernels touch the first n columns of such rows, the gradients
    come back with the padding sliced off."""

    def __init__(self, frames, W, b, pad_to=0):
        self.frames, self.n = frames, W.shape[1]
        W, b = W.detach().float().contiguous(), b.detach().float().reshape(-1)
        if pad_to > self.n:
            Wp, bp = self._new(W.shape[0], pad_to, zero=True), self._new(pad_to, zero=True)
            Wp[:, :self.n].copy_(W)
            bp[:self.n].copy_(b)
            W, b = Wp, bp
        self.W = W
        self.z = self._new(frames.F * frames.B, W.shape[1])
        frames.project(W, b, self.z)

    def _new(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=self.frames.device)

    def dz_buffer(self):
        """dz [F B, N] for the kernels to fill."""
        # the padding columns are zeroed once: the kernel writes the block's own columns only, the hoisted products read every column
        return self._new(*self.z.shape, zero=self.z.shape[1] > self.n)

    def grads(self, dz, need_W, need_b):
        """(gW [D,n], gb [n]) from dz [F B, N]; None for what is not needed."""
        gW = gb = None
        if need_W:
            gW = self._new(*self.W.shape)
            self.frames.weight_grad(dz, gW, 0.0)
            gW = gW[:, :self.n]
        if need_b:
            gb = ops.colsum(dz, self._new(dz.shape[1]))[:self.n]
        return gW, gb

    def dx(self, dz, into=None):
        """dx [F,B,D] = dz . W^T, added to `into` where given (None on byte frames: they are data)."""
        return self.frames.dx(dz, self.W, into=into)


class _GruLayer(torch.autograd.Function):
    """One tf.contrib.rnn.GRUCell layer under tf.nn.dynamic_rnn (W/all_frame_models/gru_pooling_model.py:34-47), time-major.
    x_tm [F,B,in]; Wg "gates/weights" [in+H, 2H] (r | u), bg "gates/biases" [2H]; Wc "candidate/weights" [in+H, H],
    bc "candidate/biases" [H].  Returns (out_tm [F,B,H], h_final [B,H]).  The input halves of both projections are hoisted
    GEMMs over all steps; yt8m_gru_layer_fwd / _bwd hold the time loop."""

    @staticmethod
    def forward(ctx, x_tm, token, Wg, bg, Wc, bc, num_frames):
        bf = ops.FLAGS.compute_dtype == "bfloat16"
        frames = _hoisted_input(x_tm, bf)
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = Wc.data.shape[1]
        assert Wg.data.shape == (Din + H, 2 * H) and Wc.data.shape[0] == Din + H, "GRU weights must be [in + H, 2H] / [in + H, H]"
        zg = torch.empty((F, B, 2 * H), dtype=torch.float32, device=dev)
        zc = torch.empty((F, B, H), dtype=torch.float32, device=dev)
        frames.project(Wg.data[:Din], bg.data, zg.view(F * B, 2 * H))
        frames.project(Wc.data[:Din], bc.data, zc.view(F * B, H))
        hs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        hs[0].zero_()
        rh = torch.empty((F, B, H), dtype=torch.float32, device=dev)
        out = torch.empty((F, B, H), dtype=torch.float32, device=dev)
        nf = _nf(num_frames)
        L = _lib.lib()
        # one persistent forward launch (csrc/gru_persist.inl) where the shape allows it, else the per-step kernels (2 launches per
        # time step); YT8M_GRU_PERSIST=0 forces the latter
        if F > 0 and L.yt8m_gru_persist_supported(B, H) and GRU_PERSIST_FWD:
            pws = _persist_ws(dev, torch.cuda.current_stream(dev), "gru", L.yt8m_gru_persist_workspace_bytes(B, H, F))
            _lib.check(L.yt8m_gru_persist_fwd(_p(zg), _p(zc), _p(Wg.data[Din:]), 2 * H, _p(Wc.data[Din:]), H, _p(hs), _p(rh), _p(out),
                                              _p(nf), 0, F, B, H, _p(pws), pws.numel(), _stream()))
        else:
            ws = ops._workspace(dev)
            _lib.check(L.yt8m_gru_layer_fwd(_p(zg), _p(zc), _p(Wg.data[Din:]), 2 * H, _p(Wc.data[Din:]), H, _p(hs), _p(rh),
                                            _p(out), _p(nf), F, B, H, _p(ws), ws.numel() * 4, _stream()))
        ctx.save_for_backward(frames.saved)
        ctx.frames = frames
        ctx.state = (zg, zc, hs, rh, nf, Wg, bg, Wc, bc)
        ctx.bf16 = bf
        ctx.set_materialize_grads(False)
        return out, hs[F]

    @staticmethod
    def backward(ctx, dout, dh_final):
        ctx.saved_tensors                                            # (the frames' tensor: checked against in-place changes)
        frames = ctx.frames
        zg, zc, hs, rh, nf, Wg, bg, Wc, bc = ctx.state
        ctx.state = ctx.frames = None
        F, B, Din = frames.F, frames.B, frames.D
        H = Wc.data.shape[1]
        dev = frames.device
        dzg = torch.empty((F, B, 2 * H), dtype=torch.float32, device=dev)
        dzc = torch.empty((F, B, H), dtype=torch.float32, device=dev)
        work = torch.empty((3, B, H), dtype=torch.float32, device=dev)
        dout = None if dout is None else _f32c(dout)
        dh_final = None if dh_final is None else _f32c(dh_final)
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_gru_layer_bwd(_p(zg), _p(zc), _p(Wg.data[Din:]), 2 * H, _p(Wc.data[Din:]), H, _p(hs), _p(dout),
                                                 _p(dh_final), _p(dzg), _p(dzc), _p(work), _p(nf), F, B, H, _p(ws),
                                                 ws.numel() * 4, _stream()))
        g2, c2 = dzg.view(F * B, 2 * H), dzc.view(F * B, H)
        bf = ctx.bf16
        if Wg.grad is not None:
            beta = Wg.grad_beta()
            frames.weight_grad(g2, Wg.grad[:Din], beta)
            ops.gemm_any(hs[:F].view(F * B, H), g2, out=Wg.grad[Din:], transA=True, beta=beta, role="dw", bf16=bf)
            Wg.grad_done()
        if Wc.grad is not None:
            beta = Wc.grad_beta()
            frames.weight_grad(c2, Wc.grad[:Din], beta)
            ops.gemm_any(rh.view(F * B, H), c2, out=Wc.grad[Din:], transA=True, beta=beta, role="dw", bf16=bf)
            Wc.grad_done()
        if bg.grad is not None:
            ops.colsum(g2, bg.grad.view(-1), beta=bg.grad_beta())
            bg.grad_done()
        if bc.grad is not None:
            ops.colsum(c2, bc.grad.view(-1), beta=bc.grad_beta())
            bc.grad_done()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = frames.dx(c2, Wc.data[:Din], into=frames.dx(g2, Wg.data[:Din]))
        return dx, None, None, None, None, None, None


def gru_layer(x_tm, Wg, bg, Wc, bc, num_frames):
    return _GruLayer.apply(x_tm, _token(Wg._graph), Wg, bg, Wc, bc, num_frames)


class _LnLstmLayer(torch.autograd.Function):
    """One tf.contrib.rnn.LayerNormBasicLSTMCell layer under tf.nn.dynamic_rnn
    (W/all_frame_models/layernorm_lstm_memory_model.py:37-58), time-major.  W "weights" [in+H, 4H] (no bias); gammas / betas:
    five Variables each, in the order input, transform, forget, output, state.  keep_prob < 1 = the cell's dropout_keep_prob
    (tf.nn.dropout on the candidate g; mask = Philox stream of `seed`, replayed in backward).
    Returns (out_tm, c_final, h_final) -- c is the layer-normalised cell state, as in the TF cell."""

    @staticmethod
    def forward(ctx, x_tm, token, W, gammas, betas, num_frames, forget_bias, keep_prob, seed):
        bf = ops.FLAGS.compute_dtype == "bfloat16"
        frames = _hoisted_input(x_tm, bf)
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = W.data.shape[1] // 4
        assert W.data.shape[0] == Din + H, "cell weights must be [in + H, 4H]"
        z = torch.empty((F, B, 4 * H), dtype=torch.float32, device=dev)
        frames.project(W.data[:Din], None, z.view(F * B, 4 * H))
        gamma = torch.stack([v.data for v in gammas]).contiguous()
        beta = torch.stack([v.data for v in betas]).contiguous()
        stats = torch.zeros((F, B, 10), dtype=torch.float32, device=dev)
        cs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        hs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        cs[0].zero_()
        hs[0].zero_()
        out = torch.empty((F, B, H), dtype=torch.float32, device=dev)
        nf = _nf(num_frames)
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_lnlstm_layer_fwd(_p(z), _p(W.data[Din:]), 4 * H, _p(gamma), _p(beta), _p(stats), _p(cs), _p(hs),
                                                    _p(out), _p(nf), F, B, H, float(forget_bias), float(keep_prob), int(seed),
                                                    _p(ws), ws.numel() * 4, _stream()))
        ctx.save_for_backward(frames.saved)
        ctx.frames = frames
        ctx.state = (z, gamma, beta, stats, cs, hs, nf, W, gammas, betas, float(forget_bias), float(keep_prob), int(seed))
        ctx.bf16 = bf
        ctx.set_materialize_grads(False)
        return out, cs[F], hs[F]

    @staticmethod
    def backward(ctx, dout, dc_final, dh_final):
        ctx.saved_tensors                                            # (the frames' tensor: checked against in-place changes)
        frames = ctx.frames
        z, gamma, beta, stats, cs, hs, nf, W, gammas, betas, fb, keep, seed = ctx.state
        ctx.state = ctx.frames = None
        F, B, Din = frames.F, frames.B, frames.D
        H = W.data.shape[1] // 4
        dev = frames.device
        dz = torch.empty((F, B, 4 * H), dtype=torch.float32, device=dev)
        dyb = torch.empty((F, B, 5 * H), dtype=torch.float32, device=dev)
        dyg = torch.empty((F, B, 5 * H), dtype=torch.float32, device=dev)
        work = torch.empty((4, B, H), dtype=torch.float32, device=dev)
        dout = None if dout is None else _f32c(dout)
        dc_final = None if dc_final is None else _f32c(dc_final)
        dh_final = None if dh_final is None else _f32c(dh_final)
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_lnlstm_layer_bwd(_p(z), _p(W.data[Din:]), 4 * H, _p(gamma), _p(beta), _p(stats), _p(cs), _p(dout),
                                                    _p(dc_final), _p(dh_final), _p(dz), _p(dyb), _p(dyg), _p(work), _p(nf), F, B, H,
                                                    fb, keep, seed, _p(ws), ws.numel() * 4, _stream()))
        dz2 = dz.view(F * B, 4 * H)
        if W.grad is not None:
            b = W.grad_beta()
            frames.weight_grad(dz2, W.grad[:Din], b)
            ops.gemm_any(hs[:F].view(F * B, H), dz2, out=W.grad[Din:], transA=True, beta=b, role="dw", bf16=ctx.bf16)
            W.grad_done()
        yb, yg = dyb.view(F * B, 5 * H), dyg.view(F * B, 5 * H)
        for k in range(5):
            for v, src in ((gammas[k], yg), (betas[k], yb)):
                if v.grad is not None:
                    ops.colsum(src[:, k * H:(k + 1) * H], v.grad.view(-1), beta=v.grad_beta())
                    v.grad_done()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = frames.dx(dz2, W.data[:Din])
        return dx, None, None, None, None, None, None, None, None


def lnlstm_layer(x_tm, W, gammas, betas, num_frames, forget_bias=1.0, keep_prob=1.0, seed=None):
    if seed is None:
        seed = W._graph.next_random_seed() if float(keep_prob) < 1.0 else 0
    return _LnLstmLayer.apply(x_tm, _token(W._graph), W, tuple(gammas), tuple(betas), num_frames, forget_bias, keep_prob, seed)


# ---- scalar-gate LSTM layer (Z/frame_level_models.py:1521-1790; csrc/gate_cell.hip, step order) ----------------------
GATE_LSTM_FUSED = os.environ.get("YT8M_GATE_LSTM_FUSED", "1") != "0"   # 0: the composed torch form everywhere (A/B runs, tests)
GATE_LSTM_CALLS = {"kernels": 0, "composed": 0}     # which form ran (tests assert that the kernels engaged)
_GATE_U8_LDS = 4                                    # the byte products' scaled epilogue stores float4: N % 4 == 0


def _gate_last_memory(cs, num_frames):
    """cs [F,B,H] (the memory after every step) -> cs[num_frames[b] - 1][b]; zeros for rows whose num_frames is not in 1..F."""
    F, B = cs.shape[0], cs.shape[1]
    nf = num_frames.to(torch.int64)
    valid = ((nf >= 1) & (nf <= F)).to(cs.dtype).unsqueeze(1)
    return cs[(nf - 1).clamp(0, F - 1), torch.arange(B, device=cs.device)] * valid


def _composed_cell_input(x_tm, Wv, bv, Ws, bs):
    """The prologue of the composed cells: x_tm as float frames [F,B,D] (U8FrameImages in the bytes' meaning: dequantised, padding
    zeroed, l2-normalised) and its hoisted projections zv [F,B,2H], zs [F,B,number of scalar gates]."""
    if isinstance(x_tm, U8FrameImages):
        x_tm = ops.dequant_l2norm(x_tm.q, x_tm.nf).transpose(0, 1)
    F, B, D = x_tm.shape
    x2 = x_tm.reshape(F * B, D)
    return x_tm, (x2 @ Wv + bv).view(F, B, Wv.shape[1]), (x2 @ Ws + bs).view(F, B, Ws.shape[1])


def _cell_frames_shape(x_tm):
    """(B, D) of frames the cells' step kernels read -- U8FrameImages, or float32 device frames [F,B,D] -- else None."""
    if isinstance(x_tm, U8FrameImages):
        return x_tm.B, x_tm.D
    if x_tm.is_cuda and x_tm.dtype == torch.float32:
        return x_tm.shape[1], x_tm.shape[2]
    return None


def gate_lstm_layer_composed(x_tm, Wv, bv, Ws, bs, Uv, Us, num_frames):
    """gate_lstm_layer in plain torch under autograd: a Python time loop over all F steps, in the dtype of its operands."""
    GATE_LSTM_CALLS["composed"] += 1
    x_tm, zv, zs = _composed_cell_input(x_tm, Wv, bv, Ws, bs)
    (F, B), H = x_tm.shape[:2], Uv.shape[0]
    h = c = torch.zeros((B, H), dtype=zv.dtype, device=zv.device)
    hs, cs = [], []
    for t in range(F):
        s = torch.sigmoid(zs[t] + h @ Us.t())
        v = zv[t] + h @ Uv
        i, f = s[:, 0:1], s[:, 1:2]
        o, g = torch.sigmoid(v[:, :H]), torch.tanh(v[:, H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), _gate_last_memory(torch.stack(cs), num_frames)


class _GateLstmLayer(torch.autograd.Function):
    """One layer of the scalar-gate cell on the step kernels (yt8m_gate_lstm_layer_fwd / _bwd hold the time loop); the parameters are
    tensors under autograd.  The four input projections are two hoisted products over all steps: the vector block [Wog|Wc] and the
    scalar block [Wi|Wf], the latter zero-padded to _GATE_U8_LDS columns in scratch on the byte path."""

    @staticmethod
    def forward(ctx, x_tm, Wv, bv, Ws, bs, Uv, Us, num_frames):
        bf = ops.FLAGS.compute_dtype == "bfloat16"
        frames = _hoisted_input(x_tm, bf)
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = Uv.shape[0]
        assert tuple(Wv.shape) == (Din, 2 * H) and tuple(Ws.shape) == (Din, 2) and tuple(Uv.shape) == (H, 2 * H) \
            and tuple(Us.shape) == (2, H) and bv.numel() == 2 * H and bs.numel() == 2, "gate LSTM operands: Wv [in,2H], Ws [in,2], Uv [H,2H], Us [2,H]"
        lds = _GATE_U8_LDS if isinstance(frames, U8FrameImages) else 2
        Uv, Us = _f32c(Uv.detach()), _f32c(Us.detach())
        v, sc = _Hoisted(frames, Wv, bv), _Hoisted(frames, Ws, bs, pad_to=lds)
        hs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        cs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        hs[0].zero_()
        cs[0].zero_()
        c_last = torch.empty((B, H), dtype=torch.float32, device=dev)
        nf = _nf(num_frames)
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_gate_lstm_layer_fwd(_p(v.z), _p(sc.z), lds, _p(Uv), 2 * H, _p(Us), _p(hs), _p(cs), _p(c_last), _p(nf),
                                                       F, B, H, _p(ws), ws.numel() * 4, _stream()))
        GATE_LSTM_CALLS["kernels"] += 1
        ctx.save_for_backward(frames.saved)
        ctx.frames = frames
        ctx.state = (v, sc, hs, cs, nf, Uv, Us, lds)
        ctx.bf16 = bf
        ctx.set_materialize_grads(False)
        return hs[1:], c_last

    @staticmethod
    def backward(ctx, dout, dc_last):
        ctx.saved_tensors                                            # (the frames' tensor: checked against in-place changes)
        frames = ctx.frames
        v, sc, hs, cs, nf, Uv, Us, lds = ctx.state
        ctx.state = ctx.frames = None
        F, B, dev = frames.F, frames.B, frames.device
        H = Uv.shape[0]
        v2, dzs = v.dz_buffer(), sc.dz_buffer()
        work = torch.empty((4, B, H), dtype=torch.float32, device=dev)
        dout = None if dout is None else _f32c(dout)
        dc_last = None if dc_last is None else _f32c(dc_last)
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_gate_lstm_layer_bwd(_p(v.z), _p(sc.z), lds, _p(Uv), 2 * H, _p(Us), _p(hs), _p(cs), _p(dout), _p(dc_last),
                                                       _p(v2), _p(dzs), _p(work), _p(nf), F, B, H, _p(ws), ws.numel() * 4, _stream()))
        h2 = hs[:F].view(F * B, H)
        need = ctx.needs_input_grad
        gUv = gUs = dx = None
        gWv, gbv = v.grads(v2, need[1], need[2])
        gWs, gbs = sc.grads(dzs, need[3], need[4])
        if need[5]:
            gUv = ops.gemm_any(h2, v2, transA=True, role="dw", bf16=ctx.bf16)
        if need[6]:
            gUs = ops.gemm_any(dzs, h2, transA=True, role="dw", bf16=ctx.bf16)[:2]
        if need[0]:
            dx = sc.dx(dzs, into=v.dx(v2))
        return dx, gWv, gbv, gWs, gbs, gUv, gUs, None


def gate_lstm_supported(x_tm, H):
    """Whether gate_lstm_layer runs x_tm (U8FrameImages, or float frames [F,B,in]) at H cells on the step kernels."""
    shape = _cell_frames_shape(x_tm) if GATE_LSTM_FUSED else None
    return shape is not None and bool(_lib.lib().yt8m_gate_lstm_supported(int(shape[0]), int(H)))


def gate_lstm_layer(x_tm, Wv, bv, Ws, bs, Uv, Us, num_frames):
    """One layer of the scalar-gate LSTM cell of Z/frame_level_models.py:1583-1640 (LstmGateModel.create_recurrent_unit; :1733-1790 in
    LstmGateMultilayerModel) under its tf.while_loop (:1554-1565 / :1708-1720), time-major:
        i = sigmoid(x.Wi + h.Ui + bi) [B,1]     f = sigmoid(x.Wf + h.Uf + bf) [B,1]
        o = sigmoid(x.Wog + h.Uog + bog) [B,H]  g = tanh(x.Wc + h.Uc + bc) [B,H]       c' = f c + i g,  h' = o tanh(c'),  h_0 = c_0 = 0.
    x_tm: float frames [F,B,in] or U8FrameImages; Wv = [Wog|Wc] [in,2H], bv = [bog|bc] [2H], Ws = [Wi|Wf] [in,2], bs = [bi|bf] [2],
    Uv = [Uog|Uc] [H,2H], Us = [Ui^T; Uf^T] [2,H]: tensors under autograd.  Every row runs all F steps (no copy-through, no masking; the
    padding frames are zero rows of x).  Returns (out_tm [F,B,H] = every step's h, c_last [B,H] = the memory after step
    num_frames - 1, the reference's gather at :1570-1574 / :1728-1729).  Rows with num_frames < 1: the reference's flat gather index is then
    the previous video's last frame (out of range for the first video); here such a row's c_last is zeros and it receives no gradient.
    Device tensors at shapes yt8m_gate_lstm_supported takes run on the step kernels (csrc/gate_cell.hip); CPU tensors, other shapes and
    YT8M_GATE_LSTM_FUSED=0 take gate_lstm_layer_composed, which computes the same function."""
    if gate_lstm_supported(x_tm, Uv.shape[0]):
        return _GateLstmLayer.apply(x_tm, Wv, bv, Ws, bs, Uv, Us, num_frames)
    return gate_lstm_layer_composed(x_tm, Wv, bv, Ws, bs, Uv, Us, num_frames)


# ---- the scalar-gate pair of LstmBigluModel (Z/frame_level_models.py:887-1158; csrc/gate_cell.hip, frame order) ------------------
BIGATE_LSTM_FUSED = os.environ.get("YT8M_BIGATE_LSTM_FUSED", "1") != "0"   # 0: the composed torch form everywhere (A/B runs, tests)
# The form the kernels run in.  0: frame order -- the first pass walks every video's frames backwards inside the kernels, ONE byte
# image, ONE [D,4H] and ONE [D,4] hoisted product for both passes, nothing reversed anywhere.  1: reversed copies -- the first pass
# runs in step order over a reversed copy of the frames with an operand image and hoisted products of its own, and y and its gradient
# are reversed by the copy kernel.  The default follows the project's rule (tools/bigate_lstm_step.py, DESIGN_LOG.md 37).
BIGATE_LSTM_REVERSED = os.environ.get("YT8M_BIGATE_LSTM_REVERSED", "0") != "0"
BIGATE_LSTM_CALLS = {"frame_order": 0, "reversed_copies": 0, "composed": 0}     # which form ran (tests assert it)


def _reverse_sequence_tm_torch(x, num_frames):
    """tf.reverse_sequence on time-major x [F,B,...] in plain torch (any device and dtype, under autograd); num_frames clamped to 0..F
    as the copy kernels clamp it."""
    F, B = x.shape[:2]
    t = torch.arange(F, device=x.device).unsqueeze(1)
    n = num_frames.to(device=x.device, dtype=torch.int64).clamp(0, F).unsqueeze(0)
    return x[torch.where(t < n, n - 1 - t, t), torch.arange(B, device=x.device).unsqueeze(0)]


def _bigate_pass_composed(x, y, W, b, Wsc, bsc, V, Vsc, Uv, Us):
    """One while_loop of LstmBigluModel over x [F,B,D] (and y [F,B,H] through V* where given), in the reference's order of operations
    x.W + y.V + h.U + b: every step's h and c, [F,B,H] each."""
    (F, B), H = x.shape[:2], Uv.shape[0]
    h = c = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    hs, cs = [], []
    for t in range(F):
        s, v = x[t] @ Wsc, x[t] @ W
        if y is not None:
            s, v = s + y[t] @ Vsc, v + y[t] @ V
        s = torch.sigmoid(s + h @ Us.t() + bsc)
        v = v + h @ Uv + b
        o, g = torch.sigmoid(v[:, :H]), torch.tanh(v[:, H:])
        c = s[:, 1:2] * c + s[:, 0:1] * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), torch.stack(cs)


def bigate_lstm_layer_composed(x_tm, Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2, num_frames):
    """bigate_lstm_layer in plain torch under autograd, in the reference's form: two Python time loops over all F steps WITH the two
    reverse_sequence copies (of the frames and of the first pass' hidden outputs); in the dtype of its operands."""
    BIGATE_LSTM_CALLS["composed"] += 1
    if isinstance(x_tm, U8FrameImages):
        x_tm = ops.dequant_l2norm(x_tm.q, x_tm.nf).transpose(0, 1)
    H = Uv1.shape[0]
    bv, bs = bv.reshape(-1), bs.reshape(-1)
    h1, cs1 = _bigate_pass_composed(_reverse_sequence_tm_torch(x_tm, num_frames), None, Wv[:, :2 * H], bv[:2 * H], Ws[:, :2], bs[:2],
                                    None, None, Uv1, Us1)
    y = _reverse_sequence_tm_torch(h1, num_frames)
    out2, cs2 = _bigate_pass_composed(x_tm, y, Wv[:, 2 * H:], bv[2 * H:], Ws[:, 2:], bs[2:], Vv, Vs, Uv2, Us2)
    return y, out2, _gate_last_memory(cs1, num_frames), _gate_last_memory(cs2, num_frames)


class _BigateLstmLayer(torch.autograd.Function):
    """Both passes of LstmBigluModel on the frame-order step kernels (yt8m_gate_lstm_frames_fwd / _bwd hold the time loops); the
    parameters are tensors under autograd.  A pass owns a column window (zv [F B, 2H], zs [F B, 2]) of the hoisted pre-activations; the
    kernels take windows of wider buffers.
    Frame order (reversed_copies False): the windows are the halves of ONE zv [F B, 4H] and ONE zs [F B, 4], filled by one product
    each; pass 1 runs with reverse = 1 and writes y in frame order; y.[Vog|Vc] and y.[Vi|Vf] are added to pass 2's windows as hoisted
    products over all steps; backward mirrors it and ends in one weight-gradient product per block over the joint dzv / dzs.
    Reversed copies: the way reverse_sequence_u8 / _reverse_tm_into and gate_lstm_layer's own products would have done it -- pass 1 with
    reverse = 0 over a reversed copy of the frames with its own image, buffers and products (the scalar blocks zero-padded to four
    columns), y and dy reversed by the copy kernel.  Same kernels, same arithmetic per step: what the frame-order form is measured
    against."""

    @staticmethod
    def forward(ctx, x_tm, Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2, num_frames, reversed_copies):
        bf = ops.FLAGS.compute_dtype == "bfloat16"
        frames = _hoisted_input(x_tm, bf)
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = Uv1.shape[0]
        assert tuple(Wv.shape) == (Din, 4 * H) and tuple(Ws.shape) == (Din, 4) and bv.numel() == 4 * H and bs.numel() == 4 \
            and tuple(Uv1.shape) == (H, 2 * H) and tuple(Uv2.shape) == (H, 2 * H) and tuple(Us1.shape) == (2, H) \
            and tuple(Us2.shape) == (2, H) and tuple(Vv.shape) == (H, 2 * H) and tuple(Vs.shape) == (H, 2), \
            "bigate LSTM operands: Wv [in,4H], Ws [in,4], Uv1, Uv2, Vv [H,2H], Us1, Us2 [2,H], Vs [H,2]"
        Uv1, Us1, Vv, Vs, Uv2, Us2 = (_f32c(t.detach()) for t in (Uv1, Us1, Vv, Vs, Uv2, Us2))
        bv, bs = bv.reshape(-1), bs.reshape(-1)
        nf = _nf(num_frames)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        # blocks: the (vector, scalar) hoisted blocks -- one pair for both passes, or one pair per pass; win1, win2: each pass' windows
        if not reversed_copies:
            blocks = [(_Hoisted(frames, Wv, bv), _Hoisted(frames, Ws, bs))]
            zv, zs = blocks[0][0].z, blocks[0][1].z
            win1, win2 = (zv[:, :2 * H], zs[:, :2]), (zv[:, 2 * H:], zs[:, 2:])
        else:
            if isinstance(frames, U8FrameImages):
                frames1 = U8FrameImages(reverse_sequence_u8(frames.q, nf), nf)
            else:
                frames1 = _FloatFrames(_reverse_tm_into(frames.saved, nf, torch.empty_like(frames.saved), 0), bf)
            blocks = [(_Hoisted(fr, Wv[:, k * 2 * H:(k + 1) * 2 * H], bv[k * 2 * H:(k + 1) * 2 * H]),
                       _Hoisted(fr, Ws[:, 2 * k:2 * k + 2], bs[2 * k:2 * k + 2], pad_to=_GATE_U8_LDS)) for k, fr in enumerate((frames1, frames))]
            win1, win2 = ((v.z, sc.z[:, :2]) for v, sc in blocks)
        ws = ops._workspace(dev)
        lib = _lib.lib()

        def run(win, Uv, Us, reverse):
            out, hprev, cs, c_last = new(F, B, H), new(F, B, H), new(F + 1, B, H), new(B, H)
            cs[0].zero_()
            work = new(4, B, H)
            _lib.check(lib.yt8m_gate_lstm_frames_fwd(_p(win[0]), win[0].stride(0), _p(win[1]), win[1].stride(0), _p(Uv), 2 * H, _p(Us),
                                                     _p(out), _p(hprev), _p(cs), _p(c_last), _p(work), _p(nf), reverse, F, B, H, _p(ws),
                                                     ws.numel() * 4, _stream()))
            return out, hprev, cs, c_last

        if not reversed_copies:
            y, hp1, cs1, c1_last = run(win1, Uv1, Us1, 1)
        else:
            h1, hp1, cs1, c1_last = run(win1, Uv1, Us1, 0)                                   # step order
            y = _reverse_tm_into(h1, nf, new(F, B, H), 0)
        y2 = y.view(F * B, H)
        ops.hoisted_fwd(y2, Vv, out=win2[0], beta=1.0, bf16=bf)
        ops.gemm_any(y2, Vs, out=win2[1], beta=1.0, bf16=bf)
        out2, hp2, cs2, c2_last = run(win2, Uv2, Us2, 0)
        BIGATE_LSTM_CALLS["reversed_copies" if reversed_copies else "frame_order"] += 1
        ctx.save_for_backward(frames.saved, y)                       # (y is an output: saved through autograd, not on ctx)
        ctx.frames = frames
        ctx.state = (bool(reversed_copies), blocks, win1, win2, hp1, hp2, cs1, cs2, nf, Uv1, Us1, Vv, Vs, Uv2, Us2)
        ctx.bf16 = bf
        ctx.set_materialize_grads(False)
        return y, out2, c1_last, c2_last

    @staticmethod
    def backward(ctx, dy_in, dout2, dc1_last, dc2_last):
        _, y = ctx.saved_tensors                                     # (the frames' tensor: checked against in-place changes)
        frames = ctx.frames
        reversed_copies, blocks, win1, win2, hp1, hp2, cs1, cs2, nf, Uv1, Us1, Vv, Vs, Uv2, Us2 = ctx.state
        ctx.state = ctx.frames = None
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = Uv1.shape[0]
        bf = ctx.bf16
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        dzb = [(v.dz_buffer(), sc.dz_buffer()) for v, sc in blocks]                            # as `blocks`
        if not reversed_copies:
            dzv, dzsc = dzb[0]                                                                 # every column is written by a pass
            dw1, dw2 = (dzv[:, :2 * H], dzsc[:, :2]), (dzv[:, 2 * H:], dzsc[:, 2:])
        else:
            dw1, dw2 = ((dzv, dzsc[:, :2]) for dzv, dzsc in dzb)
        ws = ops._workspace(dev)
        lib = _lib.lib()
        opt = lambda t: None if t is None else _f32c(t)

        def run(win, Uv, Us, cs, dy, dc_last, dw, reverse):
            work = new(6, B, H)
            _lib.check(lib.yt8m_gate_lstm_frames_bwd(_p(win[0]), win[0].stride(0), _p(win[1]), win[1].stride(0), _p(Uv), 2 * H, _p(Us),
                                                     _p(cs), _p(dy), _p(dc_last), _p(dw[0]), dw[0].stride(0), _p(dw[1]), dw[1].stride(0),
                                                     _p(work), _p(nf), reverse, F, B, H, _p(ws), ws.numel() * 4, _stream()))

        run(win2, Uv2, Us2, cs2, opt(dout2), opt(dc2_last), dw2, 0)
        # dy = dzv2 . [Vog|Vc]^T + dzs2 . [Vi|Vf]^T (+ the caller's gradient of y)
        dy = None if dy_in is None else _f32c(dy_in).clone().view(F * B, H)
        dy = ops.gemm_any(dw2[0], Vv, out=dy, transB=True, beta=0.0 if dy is None else 1.0, bf16=bf)
        ops.gemm_any(dw2[1], Vs, out=dy, transB=True, beta=1.0, bf16=bf)
        dy = dy.view(F, B, H)
        if not reversed_copies:
            run(win1, Uv1, Us1, cs1, dy, opt(dc1_last), dw1, 1)
        else:
            run(win1, Uv1, Us1, cs1, _reverse_tm_into(dy, nf, new(F, B, H), 0), opt(dc1_last), dw1, 0)
        need = ctx.needs_input_grad
        gUv1 = gUs1 = gVv = gVs = gUv2 = gUs2 = dx = None
        # per block pair: (gWv, gbv), (gWs, gbs) and dx; pass 1's pair on reversed copies saw the reversed frames
        gv = [v.grads(dzv, need[1], need[2]) for (v, _), (dzv, _) in zip(blocks, dzb)]
        gs = [sc.grads(dzsc, need[3], need[4]) for (_, sc), (_, dzsc) in zip(blocks, dzb)]
        dxs = [sc.dx(dzsc, into=v.dx(dzv)) if need[0] else None for (v, sc), (dzv, dzsc) in zip(blocks, dzb)]
        if not reversed_copies:
            (gWv, gbv), (gWs, gbs), dx = gv[0], gs[0], dxs[0]
        else:
            cat = lambda parts, dim: None if parts[0] is None else torch.cat(parts, dim=dim)     # (layout glue)
            gWv, gbv = cat([g[0] for g in gv], 1), cat([g[1] for g in gv], 0)
            gWs, gbs = cat([g[0] for g in gs], 1), cat([g[1] for g in gs], 0)
            if dxs[1] is not None:
                dx = dxs[1].add_(_reverse_tm_into(dxs[0], nf, new(F, B, Din), 0))
        # the recurrent and the y weights: products of tensors in one order (frame order; step order for pass 1 on reversed copies)
        dw = lambda A, Bm: ops.gemm_any(A, Bm, transA=True, role="dw", bf16=bf)
        h1, h2, y2 = hp1.view(F * B, H), hp2.view(F * B, H), y.view(F * B, H)
        if need[5]:
            gUv1 = dw(h1, dw1[0])
        if need[6]:
            gUs1 = dw(dw1[1], h1)
        if need[7]:
            gVv = dw(y2, dw2[0])
        if need[8]:
            gVs = dw(y2, dw2[1])
        if need[9]:
            gUv2 = dw(h2, dw2[0])
        if need[10]:
            gUs2 = dw(dw2[1], h2)
        return dx, gWv, gbv, gWs, gbs, gUv1, gUs1, gVv, gVs, gUv2, gUs2, None, None


def bigate_lstm_supported(x_tm, H):
    """Whether bigate_lstm_layer runs x_tm (U8FrameImages, or float frames [F,B,in]) at H cells on the frame-order step kernels."""
    shape = _cell_frames_shape(x_tm) if BIGATE_LSTM_FUSED else None
    return shape is not None and bool(_lib.lib().yt8m_gate_lstm_frames_supported(int(shape[0]), int(H)))


def bigate_lstm_layer(x_tm, Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2, num_frames):
    """The two scalar-gate recurrences of LstmBigluModel (Z/frame_level_models.py:887-1101), time-major.  With n_b = num_frames[b] and
    rev = tf.reverse_sequence(., num_frames) (frames 0 .. n_b - 1 of every video reversed, the padding frames left where they are):
      pass 1 (create_forward_recurrent_unit, :975-1032), over rev(x) from h = c = 0, all F steps:
        i = sigmoid(x.Wi1 + h.Ui1 + bi1) [B,1]     f = sigmoid(x.Wf1 + h.Uf1 + bf1) [B,1]
        o = sigmoid(x.Wog1 + h.Uog1 + bog1) [B,H]  g = tanh(x.Wc1 + h.Uc1 + bc1) [B,H]     c' = f c + i g,  h' = o tanh(c');
      y = rev(its hidden outputs) (:941);
      pass 2 (create_backward_recurrent_unit, :1034-1101), over x in frame order: the same cell where every gate also gets y_t . V*.
    x_tm: float frames [F,B,in] or U8FrameImages; Wv = [Wog1|Wc1|Wog2|Wc2] [in,4H], bv [4H] alike, Ws = [Wi1|Wf1|Wi2|Wf2] [in,4], bs [4]
    alike, Uv1, Uv2 = [Uog|Uc] [H,2H], Us1, Us2 = [Ui^T; Uf^T] [2,H], Vv = [Vog|Vc] [H,2H], Vs = [Vi|Vf] [H,2]: tensors under autograd.
    Returns (y_tm [F,B,H], out2_tm [F,B,H] = pass 2's hidden outputs, c1_last [B,H] = pass 1's memory after STEP num_frames - 1 (:943),
    c2_last [B,H] = pass 2's (:967)), all four differentiable.  Rows with num_frames < 1: c1_last and c2_last are zeros and the row
    receives no gradient through them (as gate_lstm_layer).
    Device tensors at shapes yt8m_gate_lstm_frames_supported takes run on the frame-order step kernels of csrc/gate_cell.hip -- in frame order, or
    with YT8M_BIGATE_LSTM_REVERSED=1 over reversed copies; CPU tensors, other dtypes and shapes and YT8M_BIGATE_LSTM_FUSED=0 take
    bigate_lstm_layer_composed, which computes the same function in the reference's form."""
    if bigate_lstm_supported(x_tm, Uv1.shape[0]):
        return _BigateLstmLayer.apply(x_tm, Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2, num_frames, BIGATE_LSTM_REVERSED)
    return bigate_lstm_layer_composed(x_tm, Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2, num_frames)


# ---- input-memory LSTM layer (Z/frame_level_models.py:631-885; csrc/glu_lstm.hip) -------------------------------------------
# The default form follows the project's rule: the kernels only if their median is the lower one at every shape of tools/glu_lstm_step.py
# in both runs (DESIGN_LOG.md 32).  1: the step kernels where the shape is supported; 0: the composed torch form everywhere.
GLU_LSTM_FUSED = os.environ.get("YT8M_GLU_LSTM_FUSED", "1") != "0"
GLU_LSTM_CALLS = {"kernels": 0, "composed": 0}      # which form ran (tests assert that the kernels engaged)
_GLU_LDS = 8                                        # zs | ps: the eight scalar projections of a frame, one row


def glu_lstm_layer_composed(x_tm, Wv, bv, Ws, bs, Vv, Vs, Uv, Us, num_frames):
    """glu_lstm_layer in plain torch under autograd, in the reference's form: a Python time loop over all F steps that carries xm and
    multiplies hx = l2_normalize(xm) by [Vog|Vc] and Vs at every step; in the dtype of its operands."""
    GLU_LSTM_CALLS["composed"] += 1
    x_tm, zv, zs = _composed_cell_input(x_tm, Wv, bv, Ws, bs)
    (F, B, D), H = x_tm.shape, Uv.shape[0]
    h = c = torch.zeros((B, H), dtype=zv.dtype, device=zv.device)
    xm = torch.zeros((B, D), dtype=zv.dtype, device=zv.device)
    hs, cs = [], []
    for t in range(F):
        hx = xm * torch.rsqrt((xm * xm).sum(1, keepdim=True).clamp(min=1e-12))
        s = torch.sigmoid(zs[t] + hx @ Vs + h @ Us.t())
        v = zv[t] + hx @ Vv + h @ Uv
        i, f, ix, fx = s[:, 0:1], s[:, 1:2], s[:, 2:3], s[:, 3:4]
        o, g = torch.sigmoid(v[:, :H]), torch.tanh(v[:, H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        xm = fx * xm + ix * x_tm[t]
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), _gate_last_memory(torch.stack(cs), num_frames)


class _GluLstmLayer(torch.autograd.Function):
    """One layer of the input-memory cell on the step kernels (yt8m_glu_lstm_layer_fwd / _bwd hold the time loop); the parameters are
    tensors under autograd.  The twelve input projections are two hoisted products over all steps: x.[Wog|Wc|Vog|Vc] -> zv | pv and
    x.[Wi|Wf|Wix|Wfx|Vi|Vf|Vix|Vfx] -> zs | ps; the kernels carry xm's projections as states and read the frames themselves (floats,
    or U8FrameImages.q / .r: no fp32 copy of the bytes is made)."""

    @staticmethod
    def forward(ctx, x_tm, Wv, bv, Ws, bs, Vv, Vs, Uv, Us, num_frames):
        bf = ops.FLAGS.compute_dtype == "bfloat16"
        frames = _hoisted_input(x_tm, bf)
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = Uv.shape[0]
        assert tuple(Wv.shape) == (Din, 2 * H) and tuple(Vv.shape) == (Din, 2 * H) and tuple(Ws.shape) == (Din, 4) \
            and tuple(Vs.shape) == (Din, 4) and tuple(Uv.shape) == (H, 2 * H) and tuple(Us.shape) == (4, H) and bv.numel() == 2 * H \
            and bs.numel() == 4, "glu LSTM operands: Wv, Vv [in,2H], Ws, Vs [in,4], Uv [H,2H], Us [4,H]"
        u8 = isinstance(frames, U8FrameImages)
        lds = _GLU_LDS
        Uv, Us = _f32c(Uv.detach()), _f32c(Us.detach())
        pad = torch.nn.functional.pad                                # the V halves (pv, ps) carry no bias
        v = _Hoisted(frames, torch.cat([Wv.detach(), Vv.detach()], dim=1), pad(bv.detach().reshape(-1), (0, 2 * H)))
        sc = _Hoisted(frames, torch.cat([Ws.detach(), Vs.detach()], dim=1), pad(bs.detach().reshape(-1), (0, 4)))
        zvp, zs = v.z, sc.z
        tape = lambda *shape: torch.empty((F + 1,) + shape, dtype=torch.float32, device=dev)
        hs, cs, qv, qs, xm, n2 = tape(B, H), tape(B, H), tape(B, 2 * H), tape(B, 4), tape(B, Din), tape(B)
        for s in (hs, cs, qv, qs, xm, n2):
            s[0].zero_()
        c_last = torch.empty((B, H), dtype=torch.float32, device=dev)
        nf = _nf(num_frames)
        ws = ops._workspace(dev)
        xin = (None, frames.q, frames.r) if u8 else (frames.x2, None, None)
        _lib.check(_lib.lib().yt8m_glu_lstm_layer_fwd(_p(zvp), _p(zvp[:, 2 * H:]), 4 * H, _p(zs), lds, _p(Uv), 2 * H, _p(Us), _p(xin[0]),
                                                      _p(xin[1]), _p(xin[2]), _p(hs), _p(cs), _p(qv), _p(qs), _p(xm), _p(n2), _p(c_last),
                                                      _p(nf), F, B, H, Din, _p(ws), ws.numel() * 4, _stream()))
        GLU_LSTM_CALLS["kernels"] += 1
        ctx.save_for_backward(frames.saved)
        ctx.frames = frames
        ctx.state = (v, sc, hs, cs, qv, qs, xm, n2, nf, Uv, Us, xin)
        ctx.bf16 = bf
        ctx.set_materialize_grads(False)
        return hs[1:], c_last

    @staticmethod
    def backward(ctx, dout, dc_last):
        ctx.saved_tensors                                            # (the frames' tensor: checked against in-place changes)
        frames = ctx.frames
        v, sc, hs, cs, qv, qs, xm, n2, nf, Uv, Us, xin = ctx.state
        zvp, zs = v.z, sc.z
        ctx.state = ctx.frames = None
        F, B, Din, dev = frames.F, frames.B, frames.D, frames.device
        H = Uv.shape[0]
        lds = _GLU_LDS
        need = ctx.needs_input_grad
        dv4 = v.dz_buffer()                                                         # dzv | dpv
        ds8 = sc.dz_buffer()                                                        # dzs | dps: the kernel writes all eight columns
        dxd = torch.empty((F, B, Din), dtype=torch.float32, device=dev) if (need[0] and xin[0] is not None) else None
        work = torch.empty((B * (8 * H + Din + 8),), dtype=torch.float32, device=dev)
        dout = None if dout is None else _f32c(dout)
        dc_last = None if dc_last is None else _f32c(dc_last)
        ws = ops._workspace(dev)
        _lib.check(_lib.lib().yt8m_glu_lstm_layer_bwd(_p(zvp), _p(zvp[:, 2 * H:]), 4 * H, _p(zs), lds, _p(Uv), 2 * H, _p(Us), _p(xin[0]),
                                                      _p(xin[1]), _p(xin[2]), _p(hs), _p(cs), _p(qv), _p(qs), _p(xm), _p(n2), _p(dout),
                                                      _p(dc_last), _p(dv4), _p(dv4[:, 2 * H:]), 4 * H, _p(ds8), _p(dxd), _p(work), _p(nf),
                                                      F, B, H, Din, _p(ws), ws.numel() * 4, _stream()))
        h2 = hs[:F].view(F * B, H)
        gWv = gbv = gWs = gbs = gVv = gVs = gUv = gUs = dx = None
        # dpv_t and dps_t grow like r = 1 / ||xm||: up to 1e6 on the frames behind a video's end, where xm decays below the normalisation's
        # epsilon and x_t = 0.  On bytes the kernel writes those rows as zeros; on float frames they are kept (dx reads them), so the
        # products over dpv / dps keep the fp32-grade form instead of the weight-gradient role's one scale per matrix.
        u8 = xin[0] is None
        if u8:
            gW4, gW8 = v.grads(dv4, need[1] or need[5], False)[0], sc.grads(ds8, need[3] or need[6], False)[0]
        else:
            gW4 = gW8 = None
            if need[1] or need[5]:
                gW4 = torch.empty((Din, 4 * H), dtype=torch.float32, device=dev)
                frames.weight_grad(dv4[:, :2 * H], gW4[:, :2 * H], 0.0)
                ops.gemm_any(frames.x2, dv4[:, 2 * H:], out=gW4[:, 2 * H:], transA=True, bf16=ctx.bf16)
            if need[3] or need[6]:
                gW8 = ops.gemm_any(frames.x2, ds8, out=torch.empty((Din, lds), dtype=torch.float32, device=dev), transA=True, bf16=ctx.bf16)
        if gW4 is not None:
            gWv, gVv = gW4[:, :2 * H], gW4[:, 2 * H:]
        if gW8 is not None:
            gWs, gVs = gW8[:, :4], gW8[:, 4:8]
        if need[2]:
            gbv = ops.colsum(dv4[:, :2 * H], torch.empty((2 * H,), dtype=torch.float32, device=dev))
        if need[4]:
            gbs = sc.grads(ds8, False, True)[1][:4]
        if need[7]:
            gUv = ops.gemm_any(h2, dv4[:, :2 * H], transA=True, role="dw", bf16=ctx.bf16)
        if need[8]:
            gUs = ops.gemm_any(ds8[:, :4], h2, transA=True, role="dw", bf16=ctx.bf16)
        if need[0]:
            dx = sc.dx(ds8, into=v.dx(dv4))
            if dx is not None:
                dx.add_(dxd)
        return dx, gWv, gbv, gWs, gbs, gVv, gVs, gUv, gUs, None


def glu_lstm_supported(x_tm, H):
    """Whether glu_lstm_layer runs x_tm (U8FrameImages, or float frames [F,B,in]) at H cells on the step kernels."""
    shape = _cell_frames_shape(x_tm) if GLU_LSTM_FUSED else None
    return shape is not None and bool(_lib.lib().yt8m_glu_lstm_supported(int(shape[0]), int(H), int(shape[1])))


def glu_lstm_layer(x_tm, Wv, bv, Ws, bs, Vv, Vs, Uv, Us, num_frames):
    """One layer of the input-memory LSTM cell of Z/frame_level_models.py:695-792 (LstmGlu2Model.create_recurrent_unit; :848 in
    LstmGlu2MultilayerModel) under its tf.while_loop (:666-677 / :862-873), time-major.  With xm the memory of the input (x_prev in the
    reference) and hx = xm * rsqrt(max(sum xm^2, 1e-12)) (tf.nn.l2_normalize), all states starting at 0:
        s = sigmoid(x.Ws + hx.Vs + h.Us + bs) [B,4] = i | f | ix | fx
        o = sigmoid(x.Wog + hx.Vog + h.Uog + bog) [B,H]     g = tanh(x.Wc + hx.Vc + h.Uc + bc) [B,H]
        c' = f c + i g,  h' = o tanh(c'),  xm' = fx xm + ix x.
    x_tm: float frames [F,B,in] or U8FrameImages; Wv = [Wog|Wc], Vv = [Vog|Vc] [in,2H], bv = [bog|bc] [2H]; Ws = [Wi|Wf|Wix|Wfx],
    Vs = [Vi|Vf|Vix|Vfx] [in,4], bs = [bi|bf|bix|bfx] [4]; Uv = [Uog|Uc] [H,2H], Us = [Ui|Uf|Uix|Ufx]^T [4,H]: tensors under autograd.
    Every row runs all F steps (no copy-through, no masking; the padding frames are zero rows of x).  Returns (out_tm [F,B,H] = every
    step's h, c_last [B,H] = the memory after step num_frames - 1, the reference's gather at :682-686 / :882-883).  Rows with
    num_frames < 1: c_last is zeros and the row receives no gradient through it (as gate_lstm_layer).
    Device tensors at shapes yt8m_glu_lstm_supported takes run on the step kernels (csrc/glu_lstm.hip), which carry xm.V as a state instead
    of multiplying at every step; CPU tensors, other shapes and YT8M_GLU_LSTM_FUSED=0 take glu_lstm_layer_composed, which computes the
    same function in the reference's form."""
    if glu_lstm_supported(x_tm, Uv.shape[0]):
        return _GluLstmLayer.apply(x_tm, Wv, bv, Ws, bs, Vv, Vs, Uv, Us, num_frames)
    return glu_lstm_layer_composed(x_tm, Wv, bv, Ws, bs, Vv, Vs, Uv, Us, num_frames)


# ---- MultiRNNCell stack, pipelined over time chunks: streams, resident buffers, native descriptor ----------
_SIDE = {}            # (device, persistent) -> the stack's layer / weight-gradient streams; (device, name) -> a one-off side stream


def _side_streams(device, L, persistent=False):
    """Per device: one stream per layer (its projection / dx GEMMs and its recurrence run in order on it) and one for the
    weight-gradient GEMMs.  Measured on the 2-layer BASELINE configs[3] stack (B = 128): a separate GEMM stream per layer is
    no better (51.7 vs 49.0 ms/step).  The layer streams are HIGH priority when the recurrence is the persistent kernel: it needs
    every workgroup resident, and behind a high-priority queue it takes freed CUs before the remaining workgroups of a running
    weight-gradient GEMM do (a partially resident recurrence spins on its CUs while the GEMM crawls on the rest: 28.6 vs 46.6
    ms/step run to run without it).  With the per-step kernels (600 launches) priority queues are far worse (96 ms), so those
    keep normal streams."""
    pool = _SIDE.setdefault((device, bool(persistent)), dict(r=[], w=None))
    if persistent and len(pool["r"]) < L:
        # the library's own streams (csrc/lstm_stack.hip): every stream of a process is multiplexed onto a few hardware queues, and a
        # second set of layer streams next to the native stack's put both layers of this orchestration on ONE queue (bf16 variant of
        # the bench: 19.9 -> 46 ms/step)
        with torch.cuda.device(device):
            arr, w = (ctypes.c_void_p * L)(), ctypes.c_void_p()
            _lib.check(_lib.lib().yt8m_lstm_stack_streams(L, arr, ctypes.byref(w)))
        pool["r"] = [torch.cuda.ExternalStream(int(arr[l]), device=device) for l in range(L)]
        pool["w"] = torch.cuda.ExternalStream(int(w.value), device=device)
    while len(pool["r"]) < L:
        pool["r"].append(torch.cuda.Stream(device=device, priority=REC_STREAM_PRIORITY if persistent else 0))
    if pool["w"] is None:
        pool["w"] = torch.cuda.Stream(device=device)
    return pool["r"][:L], pool["r"][:L], pool["w"]


def _side_stream(dev, name, priority=0):                           # the one side stream `name` of a device, made on first use
    if (dev, name) not in _SIDE:
        _SIDE[(dev, name)] = torch.cuda.Stream(device=dev, priority=priority)
    return _SIDE[(dev, name)]


def _chunks(F, n):
    n = max(1, min(int(n), F))
    step = (F + n - 1) // n
    return [(t0, min(step, F - t0)) for t0 in range(0, F, step)]


def _bwd_parts(F, fwd_parts, persistent=False):
    if persistent and PERSIST_BWD_CHUNKS > 0:
        return _chunks(F, PERSIST_BWD_CHUNKS)
    return fwd_parts


# Evicted buffers that something may still launch on (an autograd ctx between its forward and its backward keeps the tensor
# alive): weak references, checked -- and dropped -- by the next check_persist_errors(), so a time-out in such a backward pass is
# still reported.  A tensor nobody holds any more cannot be launched on and needs no check beyond the one at eviction.
_RETIRED = []


def _retire(ent, checker):
    checker(*ent)                                                    # what ran so far (synchronises that stream)
    _RETIRED.append((weakref.ref(ent[0]), ent[1:], checker))


class _ResidentBuffers(dict):
    """key -> (buffer, calling stream, ...): zero-initialised resident device buffers, least recently USED first (dicts keep insertion
    order).  A buffer's first line is the sticky error word of include/yt8m_hip.h: zeroed once, here; an entry is only dropped after
    `checker(*entry)` has read its status (a time-out is never lost with the eviction)."""

    def __init__(self, checker, warning=None):
        self.checker, self.warning, self.evictions = checker, warning, 0

    def buffer(self, key, nbytes, dev, rest, capacity):
        ent = self.pop(key, None)
        if ent is None:
            if len(self) >= capacity:                                # other shapes: drop the least recently used entry
                _retire(self.pop(next(iter(self))), self.checker)
                self.evictions += 1
                if self.warning and self.evictions in (64, 1024):    # a model cycling through more shapes re-zeroes a buffer per miss
                    warnings.warn(self.warning % self.evictions)
            ent = (torch.zeros(int(nbytes), dtype=torch.uint8, device=dev),) + rest
        self[key] = ent                                              # (back) at the recently-used end
        return ent[0]


def _check_ws(ws, stream):
    """Reads (and clears) the sticky error word of one workspace on ITS device and the stream its launches are ordered through."""
    with torch.cuda.device(ws.device):
        _lib.check(_lib.lib().yt8m_lstm_persist_status(_p(ws), ctypes.c_void_p(stream.cuda_stream)))


def _check_stack(scratch, stream, desc):
    with torch.cuda.device(scratch.device):
        _lib.check(_lib.lib().yt8m_lstm_stack_status(ctypes.byref(desc), _p(scratch), ctypes.c_void_p(stream.cuda_stream)))


# (device, caller's stream, layer, bytes) -> scratch workspace of that layer's persistent launches (~0.6 GB each)
_PERSIST_WS = _ResidentBuffers(_check_ws, "yt8m_amd: %d persistent-recurrence workspaces evicted; raise seq_ops._PERSIST_WS_MAX")
# (device, calling stream, description) -> zero-initialised scratch of the native stack (a few GB each: keep the table small)
_STACK_SCRATCH = _ResidentBuffers(_check_stack)


def _persist_ws(dev, main, l, nbytes):
    """Scratch of the persistent recurrence launches of layer `l` (control words + exchange images; nothing in it outlives a
    launch): ONE resident buffer per (device, calling stream, layer, size), reused by every step.  Every launch that touches it is
    ordered through the calling stream -- a stack's forward and backward both start from an event of that stream and join it
    before they return -- so two users of one key never overlap on the GPU.  Allocating it per step pinned ~0.6 GB per layer and
    step (32 steps' worth before the old table was cleared) and put two hipMalloc calls into every backward pass; on some boxes
    each of those waits ~17 ms on a DMA fence inside the driver, which made the step host-bound (25 -> 38-42 ms)."""
    return _PERSIST_WS.buffer((dev.index, main.cuda_stream, l, int(nbytes)), nbytes, dev, (main,), _PERSIST_WS_MAX)


def _stack_scratch(dev, main, desc, slot=0):
    # (the size is part of the key: the library's layout depends on its knobs too -- a test that flips YT8M_STACK_H2 in-process must
    # not be handed the other layout's buffer.)  `slot`: stacks that are alive in one step together -- the two directions of a
    # bidirectional RNN -- own separate buffers even when their shapes agree: the scratch carries the forward's scale words into the
    # backward call, so a shared one would hand the second stack's weight maxima to the first one's backward pass
    need = _lib.lib().yt8m_lstm_stack_scratch_bytes(ctypes.byref(desc))
    key = (dev.index, main.cuda_stream, need) + tuple(getattr(desc, f) for f, _ in desc._fields_
                                                      if f not in ("forget_bias", "input_keep_prob", "reserved0", "dropout_seed"))
    if slot:
        key += (("slot", int(slot)),)
    return _STACK_SCRATCH.buffer(key, need, dev, (main, desc), _STACK_SCRATCH_MAX)


def reserve_resident(stacks, layers):
    """Room in the two resident tables for a plugin that keeps `stacks` LSTM stacks of `layers` layers alive between its forward and its
    backward pass, each under a key of its own (slot, shape): _STACK_SCRATCH_MAX becomes at least `stacks` and _PERSIST_WS_MAX at least
    stacks * layers.  Never lowers either (YT8M_STACK_SCRATCH_MAX and an earlier, larger reservation stay).  With smaller tables every
    step of such a plugin would evict -- synchronise on, free and re-zero -- buffers that the very next step needs again."""
    global _STACK_SCRATCH_MAX, _PERSIST_WS_MAX
    _STACK_SCRATCH_MAX = max(_STACK_SCRATCH_MAX, int(stacks))
    _PERSIST_WS_MAX = max(_PERSIST_WS_MAX, int(stacks) * int(layers))


def check_persist_errors():
    """Synchronises and raises if ANY persistent-recurrence launch since the previous check gave up waiting for a tile (bounded
    spins set a sticky error word instead of hanging the GPU; no later launch clears it).  The training loop calls this at its
    checkpoints; tests run with PERSIST_CHECK per launch."""
    errs = []

    def check(checker, *ent):
        try:
            checker(*ent)
        except _lib.Yt8mHipError as e:                               # read (= clear) every word before raising
            errs.append(e)
    for cache in (_PERSIST_WS, _STACK_SCRATCH):
        for ent in list(cache.values()):
            check(cache.checker, *ent)
    retired, _RETIRED[:] = list(_RETIRED), []
    for ref, rest, checker in retired:
        ws = ref()
        if ws is not None:
            check(checker, ws, *rest)
            _RETIRED.append((ref, rest, checker))                    # still alive: stays on the list
    if errs:
        raise errs[-1]


def _tape_view(lib, desc, tape, layer, which, shape):
    ptr = ctypes.c_void_p()
    _lib.check(lib.yt8m_lstm_stack_view(ctypes.byref(desc), _p(tape), layer, which, ctypes.byref(ptr)))
    off = ptr.value - tape.data_ptr()
    n = 4
    for d in shape:
        n *= d
    return tape[off:off + n].view(torch.float32).view(*shape)


NATIVE_CALLS = {"fwd": 0, "bwd": 0}     # how often the native path ran (tests assert that it engaged)
DP_LAYER_BUCKETS_USED = [0]
EARLY_ADAM_RUNS = [0]      # how often the early pass ran (tests assert that it engaged)


def _stack_desc(B, F, D, H, L, u8, forget_bias, need_dx, bf16=False, keep_prob=None, seeds=None):
    # 0 = the library's own partition (csrc/lstm_stack.hip: one forward launch per layer, three unequal backward parts) unless the
    # environment / a test names a number of parts
    fwd = PERSIST_FWD_CHUNKS if (PERSIST_FWD_CHUNKS != 1 or "YT8M_LSTM_PERSIST_FWD_CHUNKS" in os.environ) else 0
    bwd = PERSIST_BWD_CHUNKS if (PERSIST_BWD_CHUNKS != 3 or "YT8M_LSTM_PERSIST_BWD_CHUNKS" in os.environ) else 0
    d = _lib.LstmStackDesc(int(B), int(F), int(D), int(H), int(L), int(bool(u8)) | (2 if bf16 else 0), float(forget_bias), int(fwd),
                           int(bwd), int(bool(need_dx)))                       # input_u8: bit 0 uint8 frames, bit 1 bf16 operand images
    if keep_prob is not None and float(keep_prob) < 1.0:                       # DropoutWrapper(input_keep_prob) inside the stack (ABI 4)
        d.input_keep_prob = float(keep_prob)
        for l, sd in enumerate(list(seeds)[:8]):
            d.dropout_seed[l] = int(sd) & 0xFFFFFFFFFFFFFFFF
    return d


# ---- clip + Adam of the already-final gradients inside the recurrent stack's backward pass (see EARLY_ADAM) ------------------------------
class _EarlyOpt(object):
    """The early pass as a descriptor the library consumes (yt8m_lstm_stack_set_early_optimizer, round 5): yt8m_lstm_stack_bwd
    enqueues sqnorm / Adam (/ the image tile pass) of `ranges` itself -- no Python runs inside the native call any more (the ctypes
    callback of rounds 3-4 swallowed exceptions and had no equivalent for a non-Python host)."""

    def __init__(self, graph, ranges):
        self.graph, self.ranges = graph, ranges
        a = graph.early_optimizer
        o = _lib.OptRanges()
        o.w, o.m, o.v, o.g = graph.params.data_ptr(), graph.adam_m.data_ptr(), graph.adam_v.data_ptr(), graph.grads.data_ptr()
        o.chunks, o.tensor_chunk_start = graph.chunks.data_ptr(), graph.chunk_start_dev.data_ptr()
        self._tcs = (ctypes.c_int32 * len(graph.chunk_start))(*graph.chunk_start)
        o.tensor_chunk_start_host = ctypes.cast(self._tcs, ctypes.c_void_p)
        o.l2, o.partial, o.norms = graph.l2.data_ptr(), graph.partial.data_ptr(), graph.norms.data_ptr()
        wi = getattr(graph, "wimg", None)
        if wi is not None and wi.active:                             # image-owning matrices: the tile pass rewrites their images
            self._jt = (ctypes.c_int32 * len(wi.job_tensor))(*wi.job_tensor)
            self._tb = (ctypes.c_int64 * len(wi.tile_base))(*wi.tile_base)
            o.skip_tensor, o.jobs = wi.skip_dev.data_ptr(), wi.jobs_dev.data_ptr()
            o.job_tensor_host, o.job_tile_base_host = ctypes.cast(self._jt, ctypes.c_void_p), ctypes.cast(self._tb, ctypes.c_void_p)
            o.njobs = len(wi.job_tensor)
        o.nranges = len(ranges)
        for i, (lo, hi) in enumerate(ranges):
            o.range_lo[i], o.range_hi[i] = lo, hi
        o.gscale, o.clip, o.lr_t, o.beta1, o.beta2, o.eps = 1.0, a["clip"], a["lr_t"], a["beta1"], a["beta2"], a["eps"]
        side = getattr(graph, "side_pending", None)
        if side:                                                     # the head's weight gradients may still be on their side stream
            o.after_stream = side[-1].cuda_stream
        self.desc = o

    def finish(self, lib, ok):
        _lib.check(lib.yt8m_lstm_stack_set_early_optimizer(None))    # (a call that failed before the window keeps it armed)
        self.graph.early_active = None
        if ok:                                                       # the native call enqueued the pass: the end-of-step pass
            self.graph.early_done = list(self.ranges)                # covers the rest (train.TrainGraph.step)
            EARLY_ADAM_RUNS[0] += 1


def _ready_ranges(ready):
    """Maximal runs [lo, hi) of True in `ready` (trainable-variable indices whose gradients are final)."""
    ranges, i, n = [], 0, len(ready)
    while i < n:
        if ready[i]:
            j = i
            while j + 1 < n and ready[j + 1]:
                j += 1
            ranges.append((i, j + 1))
            i = j + 1
        else:
            i += 1
    return ranges


def _early_optimizer_hook(graph, lib):
    if not EARLY_ADAM or graph is None or getattr(graph, "early_optimizer", None) is None or graph.grad_ready_hook is not None:
        return None
    if getattr(graph, "early_done", None):
        return None                                                  # one recurrent stack per step takes the head
    tv = graph.trainable_variables()
    ranges = _ready_ranges([bool(getattr(v, "_done_reported", False)) and v.grad_written for v in tv])
    # worth a launch pair only for a substantial share of the parameters
    if not ranges or sum(tv[k].numel() for lo, hi in ranges for k in range(lo, hi)) < (1 << 22):
        return None
    if len(ranges) > 8:                                              # the descriptor carries eight; the rest waits for the end of the step
        ranges = sorted(sorted(ranges, key=lambda r: -sum(tv[k].numel() for k in range(*r)))[:8])
    e = _EarlyOpt(graph, ranges)
    _lib.check(lib.yt8m_lstm_stack_set_early_optimizer(ctypes.byref(e.desc)))
    graph.early_active = list(ranges)                                # Variable.grad_beta refuses later contributions to these
    return e


class _StreamSet(object):
    """Selects the library's stream set for the native stack calls inside the block (yt8m_lstm_stack_use_streams; 0 = the default)."""

    def __init__(self, lib, stream_set):
        self.lib, self.set, self.prev = lib, int(stream_set), None

    def __enter__(self):
        if self.set:
            prev = ctypes.c_int()
            _lib.check(self.lib.yt8m_lstm_stack_use_streams(self.set, ctypes.byref(prev)))
            self.prev = prev.value
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            _lib.check(self.lib.yt8m_lstm_stack_use_streams(self.prev, None))
        return False


class _ByteFrames(object):
    """The reader's bytes [B,F,D] under the orchestrated stack's layer-0 projection (csrc/u8proj.hip): one pass writes (q - 128) as bf16 in
    time-major order, the row norms `rrow`, and the fp32 frames `x_tm` that only the weight-gradient product still reads.  `image`: one-plane
    operand image for the x3 kernel when every time chunk starts on a 32-row group of it; else `copies`: three bf16 copies side by side."""

    def __init__(self, lib, q, nf, parts):
        _dev(q)
        q = q.contiguous()
        B, F, D = q.shape
        self.rrow = torch.empty((F * B,), dtype=torch.float32, device=q.device)
        self.x_tm = torch.empty((F, B, D), dtype=torch.float32, device=q.device)
        self.image = self.copies = None
        if X3 and D % 16 == 0 and all((t0 * B) % 32 == 0 for t0, _ in parts):
            self.image = torch.empty(((F * B + 31) // 32) * (D // 16) * 1024, dtype=torch.uint8, device=q.device)
            _lib.check(lib.yt8m_u8_frames_image(_p(q), _p(nf), B, F, D, 1e-12, _p(self.image), _p(self.x_tm), _p(self.rrow), _stream()))
        else:
            self.copies = ops._bf16_empty(F * B, 3 * D, q.device)
            _lib.check(lib.yt8m_u8_frames_to_bf16_tm(_p(q), _p(nf), B, F, D, 1e-12, 3, _p(self.copies), self.copies.stride(0), _p(self.x_tm), _p(self.rrow), _stream()))


class _StackLayer(object):
    """One layer of the orchestrated stack: its buffers and its two forms, each chosen once; every method enqueues on the current stream.
    `hoisted` (dx, weight gradients): "bf16" copies of both operands on the bf16 MFMA kernel | "x3" three-plane split of both on the bf16
    pipe (csrc/gemm_x3.hip) | "fp32" MFMA kernel; `proj` (input projection): the same, or "u8image" / "u8copies" of layer 0's _ByteFrames.
    `rec_fwd`, `rec_bwd`: "bf16" per-step kernels on bf16 operands (csrc/lstm_bf16.hip) | "persist" one launch per chunk, W_h resident in
    registers (csrc/lstm_persist.hip) | "steps" per-step fp32 kernels."""
    FWD_ONLY = ("WxT", "WxT3", "W3T", "Wcs", "Wp16", "hs16")        # operand images the backward pass drops when it starts
    WxT = WxT3 = W3T = Wcs = Wp16 = hs16 = Wxb = Wx3 = None

    def __init__(self, lib, x, W, b, nf, forget_bias, bf16, drop, pws, undropped=None, bytes_=None):
        # drop: (keep_prob, seed) | None.  Layer 0 only: undropped = the frames under dropout (x: the buffer of their dropped copy), bytes_
        self.lib, self.x, self.W, self.b, self.nf, self.forget_bias = lib, x, W, b, nf, float(forget_bias)
        self.undropped, self.bytes, self.drop = undropped, bytes_, drop
        F, B, Din = x.shape
        H = W.data.shape[1] // 4
        assert W.data.shape[0] == Din + H, "cell weights must be [in + H, 4H]"
        self.F, self.B, self.Din, self.H, dev = F, B, Din, H, x.device
        self.z = torch.empty((F, B, 4 * H), dtype=torch.float32, device=dev)
        self.cs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        self.hs = torch.empty((F + 1, B, H), dtype=torch.float32, device=dev)
        self.out = torch.empty((F, B, H), dtype=torch.float32, device=dev)
        npk = lib.yt8m_lstm_packed_floats(B, H)
        self.Wp = torch.empty(npk, dtype=torch.float32, device=dev) if npk else None
        # decided on the whole sequence, not the chunk: every partition of the time axis runs the same arithmetic
        self.hoisted = "bf16" if bf16 and Din % 2 == 0 else "x3" if X3 and F * B >= X3_MIN_ROWS and H >= 128 else "fp32"
        self.proj = self.hoisted
        if bytes_ is not None and drop is None and self.hoisted != "bf16":
            self.proj = "u8image" if bytes_.image is not None else "u8copies"
        self.rec16 = self.hoisted == "bf16" and REC_BF16 and lib.yt8m_lstm_packed16_elems(B, H) > 0
        self.pws = None if self.rec16 else pws
        self.rec_fwd = self._recurrence(False)

    def _recurrence(self, backward):
        if self.rec16:
            return "bf16"
        if self.pws is not None and (not backward or (PERSIST_BWD and self.lib.yt8m_lstm_persist_bwd_supported(self.B, self.H))):
            return "persist"
        return "steps"

    def _rows(self, buf, t0, T):
        return buf[t0:t0 + T].view(T * self.B, buf.shape[2])

    def prepare_fwd(self):
        lib, Din, H, W, dev = self.lib, self.Din, self.H, self.W.data, self.x.device
        self.cs[0].zero_()
        self.hs[0].zero_()
        if self.Wp is not None:
            _lib.check(lib.yt8m_lstm_pack(_p(W[Din:]), 4 * H, H, _p(self.Wp), None, _stream()))
        if self.proj in ("u8image", "u8copies"):
            # 3-way bf16 split of (4/255) W_x, transposed ([4H, 3 D], K-contiguous) + the column sums of W_x
            if self.proj == "u8image":
                self.W3T = ops.x3_split(W[:Din], plain=False, trans=True, scale=4.0 / 255.0)[1]
            else:
                self.W3T = ops._bf16_empty(4 * H, 3 * Din, dev)
                _lib.check(lib.yt8m_split3_bf16_t(_p(W[:Din]), 4 * H, Din, 4 * H, 4.0 / 255.0, _p(self.W3T), self.W3T.stride(0), _stream()))
            self.Wcs = torch.empty((4 * H,), dtype=torch.float32, device=dev)
            ops.colsum(W[:Din], self.Wcs)
        elif self.proj == "x3":                                     # W_x^T as the K-contiguous operand of the projection
            self.WxT3 = ops.x3_split(W[:Din], plain=False, trans=True)[1]
        elif self.proj == "bf16":                                   # W_x^T once per step, K-contiguous for the NT product
            self.WxT = ops.cast_bf16(W[:Din], transpose=True)
        if self.rec16:                                              # bf16 operands for the recurrent product too
            self.hs16 = torch.empty((self.F + 1, self.B, H), dtype=torch.bfloat16, device=dev)
            self.hs16[0].zero_()
            self.Wp16 = torch.empty(H * 4 * H, dtype=torch.bfloat16, device=dev)
            _lib.check(lib.yt8m_lstm_pack_bf16(_p(W[Din:]), 4 * H, H, _p(self.Wp16), None, _stream()))

    def project(self, t0, T):
        """z[t0:t0+T] = dropout(x[t0:t0+T]) . W_x + b"""
        lib, B, Din, H, bias = self.lib, self.B, self.Din, self.H, self.b.data
        xc, zc = self._rows(self.x, t0, T), self._rows(self.z, t0, T)
        if self.drop is not None:
            src = xc if self.undropped is None else self._rows(self.undropped, t0, T)
            _lib.check(lib.yt8m_dropout_f32(_p(src), _p(xc), xc.numel(), self.drop[0], self.drop[1], t0 * B * Din, _stream()))
        if self.proj == "u8image":
            q, ws = self.bytes, ops._workspace(self.x.device)
            _lib.check(lib.yt8m_gemm_x1x3_nt(T * B, 4 * H, Din, _p(q.image[(t0 * B // 32) * (Din // 16) * 1024:]), _p(self.W3T.buf),
                                             _p(zc), 4 * H, _p(bias), _p(q.rrow[t0 * B:]), _p(self.Wcs), U8_BETA, _p(ws), ws.numel() * 4, _stream()))
        elif self.proj == "u8copies":
            q = self.bytes
            ops.gemm_bf16_nt_grouped([dict(A=q.copies[t0 * B:(t0 + T) * B], B=self.W3T, out=zc)])
            _lib.check(lib.yt8m_rowscale_bias_f32(_p(zc), T * B, 4 * H, 4 * H, _p(q.rrow[t0 * B:]), _p(self.Wcs), U8_BETA, _p(bias), _stream()))
        elif self.proj == "bf16":
            ops.gemm_bf16_nt_grouped([dict(A=ops.cast_bf16(xc), B=self.WxT, out=zc, bias=bias)])
        elif self.proj == "x3":
            ops.gemm_x3_grouped([dict(A=ops.x3_split(xc)[0], B=self.WxT3, out=zc, bias=bias)])
        else:
            ops.gemm(xc, self.W.data[:Din], out=zc, bias=bias)

    def recur_fwd(self, t0, T):
        lib, B, Din, H, fb = self.lib, self.B, self.Din, self.H, self.forget_bias
        z, cs, hs, out, nf, Wh = _p(self.z), _p(self.cs), _p(self.hs), _p(self.out), _p(self.nf), self.W.data[Din:]
        ws = ops._workspace(self.x.device)
        if self.rec_fwd == "bf16":
            _lib.check(lib.yt8m_lstm_steps_fwd_bf16(z, _p(self.Wp16), cs, hs, _p(self.hs16), out, nf, t0, T, B, H, fb, _stream()))
        elif self.rec_fwd == "persist":
            _lib.check(lib.yt8m_lstm_persist_fwd(z, _p(Wh), 4 * H, cs, hs, out, nf, t0, T, B, H, fb, _p(self.pws), self.pws.numel(), _stream()))
            if PERSIST_CHECK:
                _lib.check(lib.yt8m_lstm_persist_status(_p(self.pws), _stream()))
        else:
            _lib.check(lib.yt8m_lstm_steps_fwd(z, _p(Wh), 4 * H, _p(self.Wp), cs, hs, out, nf, t0, T, B, H, fb, _p(ws), ws.numel() * 4, _stream()))

    def release(self, names):
        for name in names:
            setattr(self, name, None)

    def alloc_bwd(self, dout_top, top, wants_dx):                   # (dout: the caller's on top, else written from above)
        F, B, H, dev, self.wants_dx = self.F, self.B, self.H, self.x.device, wants_dx
        self.dz = torch.empty((F, B, 4 * H), dtype=torch.float32, device=dev)
        self.work = torch.empty((4, B, H), dtype=torch.float32, device=dev)
        self.dout = (None if dout_top is None else _f32c(dout_top)) if top else torch.empty((F, B, H), dtype=torch.float32, device=dev)
        npk = self.lib.yt8m_lstm_packed_floats(B, H)
        self.Wq = torch.empty(npk, dtype=torch.float32, device=dev) if npk else None

    def prepare_bwd(self, dh, dc):
        lib, Din, H, W = self.lib, self.Din, self.H, self.W.data
        for row, d in ((self.work[0], dh), (self.work[1], dc)):
            if d is None:
                row.zero_()
            else:
                row.copy_(d)
        self.phase = 0
        self.rec_bwd = self._recurrence(True)
        if self.rec16:
            self.dz16 = torch.empty((self.F, self.B, 4 * H), dtype=torch.bfloat16, device=self.x.device)
            self.Wq16 = torch.empty(H * 4 * H, dtype=torch.bfloat16, device=self.x.device)
            _lib.check(lib.yt8m_lstm_pack_bf16(_p(W[Din:]), 4 * H, H, None, _p(self.Wq16), _stream()))
        elif self.Wq is not None:
            _lib.check(lib.yt8m_lstm_pack(_p(W[Din:]), 4 * H, H, None, _p(self.Wq), _stream()))

    def recur_bwd(self, t0, T):
        lib, B, Din, H = self.lib, self.B, self.Din, self.H
        z, cs, dout, dz, work, nf, Wh = _p(self.z), _p(self.cs), _p(self.dout), _p(self.dz), _p(self.work), _p(self.nf), self.W.data[Din:]
        ws = ops._workspace(self.x.device)
        if self.rec_bwd == "bf16":
            _lib.check(lib.yt8m_lstm_steps_bwd_bf16(z, _p(self.Wq16), cs, dout, dz, _p(self.dz16), work, self.phase, nf, t0, T, B, H, _stream()))
        elif self.rec_bwd == "persist":
            # (no dbias_rows: the bias gradient as per-row sums in the epilogue measured SLOWER, 37.1 -> 40.3 ms/step --
            # four more scattered read-modify-writes per lane and item in front of the exchange loads)
            _lib.check(lib.yt8m_lstm_persist_bwd(z, _p(Wh), 4 * H, cs, dout, dz, work, self.phase, None, nf, t0, T, B, H, _p(self.pws), self.pws.numel(), _stream()))
            if PERSIST_CHECK:
                _lib.check(lib.yt8m_lstm_persist_status(_p(self.pws), _stream()))
        else:
            _lib.check(lib.yt8m_lstm_steps_bwd(z, _p(Wh), 4 * H, _p(self.Wq), cs, dout, dz, work, self.phase, nf, t0, T, B, H, _p(ws), ws.numel() * 4, _stream()))
        self.phase = (self.phase + T) % 2

    def dx_operands(self, t0, T):
        """(dz as the dx product reads it, bf16: its transposed copy for the dW products, the event that says so); first chunk: W_x too."""
        dzc, Wx = self._rows(self.dz, t0, T), self.W.data[:self.Din]
        if self.hoisted == "bf16":                                  # dz feeds dx (plain) and both dW products (transposed)
            if self.rec16:                                          # the step kernels already wrote the plain bf16 copy
                dzb, dzT = self._rows(self.dz16, t0, T), ops.cast_bf16(dzc, transpose=True)
            else:
                dzb, dzT = ops.cast_bf16_both(dzc)
            if self.Wxb is None:
                self.Wxb = ops.cast_bf16(Wx)
            return dzb, dzT, torch.cuda.current_stream(dzc.device).record_event()
        if self.hoisted == "x3" and self.wants_dx:                  # dz as stored feeds dx: on the layer stream (critical path);
            dz3 = ops.x3_split(dzc)[0]                              # its transposed image (both dW products) is made by weight_grad
            if self.Wx3 is None:
                self.Wx3 = ops.x3_split(Wx)[0]
            return dz3, None, None
        return None, None, None

    def dx(self, t0, T, dst, dz):
        """dst[t0:t0+T] = dz . W_x^T, through the dropout mask the forward pass applied to this layer's input."""
        out = self._rows(dst, t0, T)
        if self.hoisted == "x3":
            ops.gemm_x3_grouped([dict(A=dz[0], B=self.Wx3, out=out)])
        elif self.hoisted == "bf16":
            ops.gemm_bf16_nt_grouped([dict(A=dz[0], B=self.Wxb, out=out)])
        else:
            ops.gemm(self._rows(self.dz, t0, T), self.W.data[:self.Din], out=out, transB=True)
        if self.drop is not None:
            ops.dropout_(dst[t0:t0 + T], self.drop[0], self.drop[1], t0 * self.B * self.Din)

    def weight_grad(self, t0, T, beta, dz):
        """W.grad = beta W.grad + [x ; h]^T dz over the chunk."""
        Din, gW = self.Din, self.W.grad
        xc, hc, dzc = self._rows(self.x, t0, T), self._rows(self.hs, t0, T), self._rows(self.dz, t0, T)
        if self.hoisted == "bf16":
            ops.gemm_bf16_nt_grouped([dict(A=ops.cast_bf16(xc, transpose=True), B=dz[1], out=gW[:Din], beta=beta),
                                      dict(A=ops.cast_bf16(hc, transpose=True), B=dz[1], out=gW[Din:], beta=beta)])
        elif self.hoisted == "x3":
            dzT3 = ops.x3_split(dzc, plain=False, trans=True)[1]
            xT3 = ops.x3_split(xc, plain=False, trans=True)[1]
            hT3 = ops.x3_split(hc, plain=False, trans=True)[1]
            ops.gemm_x3_grouped([dict(A=xT3, B=dzT3, out=gW[:Din], beta=beta), dict(A=hT3, B=dzT3, out=gW[Din:], beta=beta)])
        else:
            ops.gemm(xc, dzc, out=gW[:Din], transA=True, beta=beta, role="dw")
            ops.gemm(hc, dzc, out=gW[Din:], transA=True, beta=beta, role="dw")

    def bias_grad(self, t0, T, beta):
        ops.colsum(self._rows(self.dz, t0, T), self.b.grad.view(-1), beta=beta)


def _stack_dispatch(lib, x_tm, wb, forget_bias, input_keep_prob, seeds, bf16, need_dx):
    """Native stack or orchestration, decided once: (desc, u8, drop, pers, own, B, F), desc = the native call's descriptor or None.
    u8: raw reader bytes [B,F,D] (batch-major); drop: DropoutWrapper is active; pers: the persistent recurrence covers every layer;
    own: the fp32 stack on it cuts time its own way (PERSIST_FWD_CHUNKS) -- `chunks` is the caller's hint for the per-step pipeline."""
    L = len(wb) // 2
    Hs = [w.data.shape[1] // 4 for w in wb[0::2]]
    u8 = x_tm.dtype == torch.uint8
    B, F = (x_tm.shape[0], x_tm.shape[1]) if u8 else (x_tm.shape[1], x_tm.shape[0])
    drop = input_keep_prob is not None and float(input_keep_prob) < 1.0
    pers = PERSIST and all(lib.yt8m_lstm_persist_supported(B, h) for h in Hs)
    free = pers and os.environ.get("YT8M_PERSIST_CUS") is None                  # no caller-supplied CU budget
    own = free and not bf16
    # The product's own configuration runs entirely inside the library (csrc/lstm_stack.hip: partition, streams, operand images,
    # product forms -- the path bench.py measures); everything else (caller's chunks, dropout, bf16 operands, per-step kernels,
    # tuning knobs) keeps the orchestration, built from the same per-call entry points.
    # (round 6: DropoutWrapper(input_keep_prob) stays on the native stack -- the mask is applied where the operand images are built,
    # csrc/lstm_stack.hip -- for a float input on the f16 product forms; yt8m_lstm_stack_supported refuses the rest and the
    # orchestration takes over.  YT8M_NATIVE_DROPOUT=0 keeps dropout on the orchestration.)
    drop_native = drop and NATIVE_DROPOUT and not u8 and not bf16 and L <= 8
    desc = None
    if (NATIVE_STACK and free and (not bf16 or NATIVE_BF16) and X3 and PERSIST_BWD and PERSIST_STEP_IMAGES and
            (not drop or drop_native) and PERSIST_FWD_CHUNKS > 0 and PERSIST_BWD_CHUNKS > 0 and len(set(Hs)) == 1):
        D0 = x_tm.shape[2]
        desc = _stack_desc(B, F, D0, Hs[0], L, u8, forget_bias, (not u8) and bool(need_dx), bf16=bool(bf16),
                           keep_prob=input_keep_prob if drop else None, seeds=seeds if drop else None)
        if not ((u8 or x_tm.dtype == torch.float32) and wb[0].data.shape[0] == D0 + Hs[0] and lib.yt8m_lstm_stack_supported(ctypes.byref(desc))):
            desc = None
    return desc, u8, drop, pers, own, B, F


def _stack_grads(dx, L):                                            # nothing for apply()'s nine other arguments and 2 L Variables
    return (dx,) + (None,) * (9 + 2 * L)


class _LstmStack(torch.autograd.Function):
    """MultiRNNCell([BasicLSTMCell] * L) under tf.nn.dynamic_rnn (W/all_frame_models/lstm_model.py:34-47), time-major, as ONE
    op so that the layers can be pipelined: the sequence is cut into time chunks; layer l's hoisted input projection of
    chunk c (a GEMM stream) starts as soon as layer l-1 has finished the recurrence of chunk c, and its own recurrence of
    chunk c (a high-priority stream per layer) follows -- while layer l-1 is already in chunk c+1.  The MFMA-bound GEMMs then
    overlap the latency-bound recurrence steps.  Backward runs the same wavefront in reverse time order (top layer first;
    the dx GEMM of a chunk releases the layer below) and every weight-gradient GEMM goes to a further stream, accumulating
    chunk by chunk.  Same kernels and the same per-step arithmetic as the unpipelined op; chunks = 1 is the sequential form.
    forward() / backward() are that wavefront over _StackLayer's operations; the product's own configuration runs in the library instead.

    input_keep_prob < 1 is tf.contrib.rnn.DropoutWrapper(cell, input_keep_prob) around every layer
    (W/all_frame_models/lstm_memory_model.py:36-45): the INPUT of each layer (frames for layer 0, the outputs of the layer
    below otherwise -- never the recurrent state) goes through tf.nn.dropout with a fresh mask per time step.  Here: one
    Philox key per layer (seeds), element index = position in the [F,B,in] tensor, applied chunk by chunk on the layer's
    stream right before the projection GEMM (in place on the lower layer's output buffer, which nothing else reads) and
    replayed on the dx chunk in backward.

    bf16 (compute_dtype=bfloat16): the hoisted products (input projection, its weight gradients and dx) take bf16 copies of
    their operands on the bf16 MFMA path (fp32 accumulate, fp32 master weights and gradients); the recurrence -- state, gates,
    recurrent product -- stays fp32.

    apply(x_tm [F,B,D], token, num_frames, forget_bias, chunks, input_keep_prob, seeds, bf16, W_0, b_0, ..., W_{L-1}, b_{L-1})
      -> (out_top [F,B,H], c_0, h_0, ..., c_{L-1}, h_{L-1})"""

    @staticmethod
    def forward(ctx, x_tm, token, num_frames, forget_bias, chunks, input_keep_prob, seeds, bf16, slot, stream_set, *wb):
        lib = _lib.lib()
        nf = _nf(num_frames)
        L = len(wb) // 2
        desc, u8, drop, pers, own, B, F = _stack_dispatch(lib, x_tm, wb, forget_bias, input_keep_prob, seeds, bf16, ctx.needs_input_grad[0])
        if desc is not None:
            return _LstmStack._native_forward(ctx, lib, desc, x_tm, nf, wb, slot, stream_set)
        parts = _chunks(F, PERSIST_FWD_CHUNKS if own and PERSIST_FWD_CHUNKS > 0 else chunks)
        # the backward pass may cut time differently (all buffers are whole-layer): its first recurrence chunk runs with nothing
        # beside it, so shorter chunks shorten that pipeline fill; the forward recurrence owns the chip and wants few launches
        bwd_parts = _bwd_parts(F, _chunks(F, chunks), own)
        q = _ByteFrames(lib, x_tm, nf, parts) if u8 else None
        x_tm = _f32c(q.x_tm if u8 else x_tm)
        _dev(x_tm)
        assert (F, B) == tuple(x_tm.shape[:2])
        dev = x_tm.device
        main = torch.cuda.current_stream(dev)
        rs, gs, _ = _side_streams(dev, L, pers)
        bf16 = bool(bf16) and B % 2 == 0 and min(T for _, T in parts) * B >= ops.BF16_MIN_ROWS
        layers, inp = [], x_tm
        for l in range(L):                                          # every buffer comes from the main stream's pool
            if drop and l == 0:
                inp = torch.empty_like(x_tm)                        # dropped copy of the frames (the input itself is data)
            H = wb[2 * l].data.shape[1] // 4
            pws = lib.yt8m_lstm_persist_workspace_bytes(B, H) if PERSIST else 0
            # one exchange image per step of the longest launch (forward or backward partition): XCD-L2-shared state fetch
            big = lib.yt8m_lstm_persist_workspace_bytes_steps(B, H, max(T for _, T in parts + bwd_parts)) if pws and PERSIST_STEP_IMAGES else 0
            if 0 < big <= PERSIST_STEP_IMAGES_MAX_BYTES:
                pws = big
            layers.append(_StackLayer(lib, inp, wb[2 * l], wb[2 * l + 1], nf, forget_bias, bf16, (float(input_keep_prob), int(seeds[l])) if drop else None,
                                      _persist_ws(dev, main, (slot, l) if slot else l, pws) if pws else None,
                                      x_tm if drop and l == 0 else None, q if l == 0 else None))
            inp = layers[-1].out
        start = main.record_event()
        for l, st in enumerate(layers):
            gs[l].wait_event(start)
            with torch.cuda.stream(rs[l]):
                rs[l].wait_event(start)
                st.prepare_fwd()
        r_done = [[torch.cuda.Event() for _ in parts] for _ in range(L)]
        for c, (t0, T) in enumerate(parts):
            for l, st in enumerate(layers):
                with torch.cuda.stream(gs[l]):                      # hoisted input projection of the chunk
                    if l > 0:
                        gs[l].wait_event(r_done[l - 1][c])
                    st.project(t0, T)
                    g_ev = gs[l].record_event()
                with torch.cuda.stream(rs[l]):                      # recurrence steps of the chunk
                    rs[l].wait_event(g_ev)
                    st.recur_fwd(t0, T)
                    r_done[l][c].record(rs[l])
        for l, st in enumerate(layers):
            main.wait_event(r_done[l][-1])
            st.release(("undropped", "bytes"))                      # what only forward() needed
        ctx.layers, ctx.parts, ctx.pers = layers, bwd_parts, pers
        ctx.set_materialize_grads(False)
        return (layers[-1].out,) + tuple(t for st in layers for t in (st.cs[F], st.hs[F]))

    @staticmethod
    def _native_forward(ctx, lib, desc, x, nf, wb, slot=0, stream_set=0):
        x = x.contiguous()
        _dev(x)
        dev = x.device
        main = torch.cuda.current_stream(dev)
        L, B, F, H = desc.L, desc.B, desc.F, desc.H
        Ws, bs = wb[0::2], wb[1::2]
        for l, w in enumerate(Ws):
            assert w.data.is_contiguous() and tuple(w.data.shape) == ((desc.D if l == 0 else H) + H, 4 * H), "cell weights must be [in + H, 4H]"
        tape = torch.empty(lib.yt8m_lstm_stack_tape_bytes(ctypes.byref(desc)), dtype=torch.uint8, device=dev)
        scratch = _stack_scratch(dev, main, desc, slot)
        Wp = (ctypes.c_void_p * L)(*[w.data.data_ptr() for w in Ws])
        bp = (ctypes.c_void_p * L)(*[b.data.data_ptr() for b in bs])
        with _StreamSet(lib, stream_set):
            _lib.check(lib.yt8m_lstm_stack_fwd(ctypes.byref(desc), _p(x), _p(nf), Wp, bp, _p(tape), tape.numel(), _p(scratch), scratch.numel(),
                                               _stream()))
        NATIVE_CALLS["fwd"] += 1
        if PERSIST_CHECK:
            _check_stack(scratch, main, desc)
        ctx.native = (desc, tape, scratch, x, nf, Ws, bs)
        ctx.stream_set = stream_set
        g_ = Ws[0]._graph
        if g_ is not None and torch.is_grad_enabled():
            # the stack's backward pass will follow whatever consumes these outputs: ops that run before it in the backward pass (the
            # classifier head) may leave their weight gradients to a side stream instead of the chain the first recurrence waits on
            g_.defer_head_dw = True
        ctx.layers = None
        ctx.set_materialize_grads(False)
        outs = [_tape_view(lib, desc, tape, L - 1, 0, (F, B, H))]
        for l in range(L):
            outs += [_tape_view(lib, desc, tape, l, 1, (B, H)), _tape_view(lib, desc, tape, l, 2, (B, H))]
        return tuple(outs)

    @staticmethod
    def _native_backward(ctx, dout_top, dfinal):
        desc, tape, scratch, x, nf, Ws, bs = ctx.native
        ctx.native = None
        lib = _lib.lib()
        L = desc.L
        dev = x.device
        keep = []

        def c32(t):
            if t is None:
                return None
            t = _f32c(t)
            keep.append(t)
            return t

        dout_top = c32(dout_top)
        dcs = [c32(dfinal[2 * l]) for l in range(L)]
        dhs = [c32(dfinal[2 * l + 1]) for l in range(L)]
        arr = lambda ts: (ctypes.c_void_p * L)(*[None if t is None else t.data_ptr() for t in ts])
        dW = [w.grad if w.grad is not None else None for w in Ws]
        db = [b.grad if b.grad is not None else None for b in bs]
        for g in dW + db:
            assert g is None or g.is_contiguous()
        bW = (ctypes.c_float * L)(*[float(w.grad_beta()) if w.grad is not None else 0.0 for w in Ws])
        bb = (ctypes.c_float * L)(*[float(b.grad_beta()) if b.grad is not None else 0.0 for b in bs])
        dx = torch.empty((desc.F, desc.B, desc.D), dtype=torch.float32, device=dev) if desc.need_dx else None
        Wp = (ctypes.c_void_p * L)(*[w.data.data_ptr() for w in Ws])
        early = _early_optimizer_hook(Ws[0]._graph, lib)
        ok = False
        try:
            with _StreamSet(lib, getattr(ctx, "stream_set", 0)):
                _lib.check(lib.yt8m_lstm_stack_bwd(ctypes.byref(desc), _p(x), _p(nf), Wp, _p(tape), tape.numel(), _p(scratch), scratch.numel(),
                                                   _p(dout_top), arr(dcs), arr(dhs), arr(dW), arr(db), bW, bb, _p(dx), _stream()))
            ok = True
        finally:
            if early is not None:
                early.finish(lib, ok)
        NATIVE_CALLS["bwd"] += 1
        ops.join_side_work(Ws[0]._graph)                             # gradients an earlier op left on a side stream: visible from here on
        g_ = Ws[0]._graph
        if getattr(ctx, "stream_set", 0) and g_ is not None:
            # the overlapped bw direction (bidirectional_lstm_stacks): autograd runs this backward on the side stream its forward ran on,
            # and nothing else orders the caller's stream after it -- no leaf gradient comes out of it.  Its weight / bias gradients (and
            # the early clip + Adam it may have enqueued) are joined like any other side work: by the next stack backward or by
            # TrainGraph.step before the optimiser pass (ops.join_side_work)
            if getattr(g_, "side_pending", None) is None:
                g_.side_pending = []
            g_.side_pending.append(torch.cuda.current_stream(dev))
        if PERSIST_CHECK:
            _check_stack(scratch, torch.cuda.current_stream(dev), desc)
        g = Ws[0]._graph
        if g is not None and g.grad_ready_hook is not None and DP_LAYER_BUCKETS:
            # data parallel: report each layer's gradients from a side stream that waits for THAT layer only (the library records
            # the point on its weight-gradient stream: layer L-1's gradients are final a whole last part before layer 0's), so
            # the reducer's collective for layer L-1 is on the wire while layer 0's last weight-gradient products still run
            side = _side_stream(dev, "dp")
            for l in reversed(range(L)):
                _lib.check(lib.yt8m_lstm_stack_layer_done_wait(l, ctypes.c_void_p(side.cuda_stream)))
                with torch.cuda.stream(side):
                    for v in (Ws[l], bs[l]):
                        if v.grad is not None:
                            v.grad_done()
            DP_LAYER_BUCKETS_USED[0] += 1
        else:
            for v in list(Ws) + list(bs):
                if v.grad is not None:
                    v.grad_done()
        return _stack_grads(dx, L)

    @staticmethod
    def backward(ctx, dout_top, *dfinal):
        if getattr(ctx, "native", None) is not None:
            return _LstmStack._native_backward(ctx, dout_top, dfinal)
        layers, parts = ctx.layers, ctx.parts
        ctx.layers = None
        L = len(layers)
        dev = layers[0].x.device
        main = torch.cuda.current_stream(dev)
        rs, gs, sw = _side_streams(dev, L, ctx.pers)
        need_dx = ctx.needs_input_grad[0]
        dx = torch.empty_like(layers[0].x) if need_dx else None
        for st in layers:                                           # forward-only images go before anything is allocated
            st.release(st.FWD_ONLY)
        for l, st in enumerate(layers):                            # buffers come from the main stream's pool
            st.alloc_bwd(dout_top, l == L - 1, l > 0 or need_dx)
        start = main.record_event()
        sw.wait_event(start)
        for l, st in enumerate(layers):
            gs[l].wait_event(start)
            with torch.cuda.stream(rs[l]):
                rs[l].wait_event(start)
                st.prepare_bwd(dfinal[2 * l + 1], dfinal[2 * l])
        seen = set()

        def beta(v):                                                # a Variable's first chunk: grad_beta(), later ones add
            first = id(v) not in seen
            seen.add(id(v))
            return v.grad_beta() if first else 1.0

        last = []
        for c in range(len(parts) - 1, -1, -1):
            t0, T = parts[c]
            dx_ev = None                                            # dx GEMM of the layer above for this chunk
            for l in range(L - 1, -1, -1):
                st = layers[l]
                with torch.cuda.stream(rs[l]):
                    if dx_ev is not None:
                        rs[l].wait_event(dx_ev)
                    st.recur_bwd(t0, T)
                    rb = rs[l].record_event()
                dx_ev = None
                with torch.cuda.stream(gs[l]):
                    gs[l].wait_event(rb)
                    dz = st.dx_operands(t0, T)
                    if st.wants_dx:
                        st.dx(t0, T, layers[l - 1].dout if l > 0 else dx, dz)
                        dx_ev = gs[l].record_event()
                        if c == 0:
                            last.append(dx_ev)
                with torch.cuda.stream(sw):
                    sw.wait_event(rb)
                    if st.W.grad is not None:
                        if dz[2] is not None:                       # bf16: dz^T made on the dx stream
                            sw.wait_event(dz[2])
                            dz[1].record_stream(sw)
                        st.weight_grad(t0, T, beta(st.W), dz)
                    if st.b.grad is not None:
                        st.bias_grad(t0, T, beta(st.b))
        main.wait_event(sw.record_event())                          # sw waited for every recurrence chunk
        for e in last:
            main.wait_event(e)
        for st in layers:
            for v in (st.W, st.b):
                if v.grad is not None:
                    v.grad_done()
        return _stack_grads(dx, L)


def lstm_stack(x_tm, num_frames, weights_biases, forget_bias=1.0, chunks=4, input_keep_prob=None, seeds=None, bf16=False, slot=0,
               stream_set=0):
    """weights_biases: [(W_0, b_0), ...] Variables.  Returns (out_top, [(c_l, h_l), ...]).
    input_keep_prob < 1: DropoutWrapper(input_keep_prob) on every layer; seeds = one Philox key per layer (default: the
    graph's random stream).  slot: which of the stack's cached buffers (native scratch, persistent workspaces) this stack owns --
    stacks alive in one step together take different slots.  stream_set: the library's stream set of the native calls (0 or 1,
    see bidirectional_lstm_stacks)."""
    flat = [v for wb in weights_biases for v in wb]
    if input_keep_prob is not None and float(input_keep_prob) < 1.0 and seeds is None:
        seeds = [flat[0]._graph.next_random_seed() for _ in weights_biases]
    res = _LstmStack.apply(x_tm, _token(flat[0]._graph), num_frames, forget_bias, int(chunks), input_keep_prob,
                           tuple(seeds) if seeds is not None else None, bool(bf16), int(slot), int(stream_set), *flat)
    return res[0], [(res[1 + 2 * l], res[2 + 2 * l]) for l in range(len(weights_biases))]


# ---- LstmLayerModel's clip pass (Z/frame_level_models.py:3653-3668): one BasicLSTMCell over every clip of every video as ONE batch ---------
# YT8M_LSTM_WIDE: 1 = the wide step kernel (csrc/lstm_wide.hip) runs the forward recurrence of lstm_clip_layer at B' >= WIDE_MIN_ROWS rows
# where yt8m_lstm_wide_supported takes the shape; 0 = an existing per-step route always.  The default and WIDE_MIN_ROWS come from
# tools/lstm_layer_step.py (profiles/lstm_layer_step.jsonl, DESIGN_LOG.md 38); nothing but lstm_clip_layer reaches the kernel.
WIDE = os.environ.get("YT8M_LSTM_WIDE", "1") != "0"      # on: its median was below both existing routes at every op-leg shape in both runs
# the smallest B' of the kernel leg (960 and 3840 rows x H = 512 and 1024): the wide step was below both existing routes at all four
# shapes in both runs, 26 us against 34 (packed) at 960 x 512 and 126 against 376 at 3840 x 1024; nothing below 960 rows was measured
WIDE_MIN_ROWS = 960
# the forward route without the wide kernel -- "packed" (yt8m_lstm_steps_fwd with Wp) | "gemm" (Wp = NULL): packed was the faster existing
# route at every op-leg shape in both runs
CLIP_FWD_EXISTING = "packed"
# the backward route -- "packed" (yt8m_lstm_steps_bwd with Wq) | "gemm" (Wq = NULL).  Neither was lower at EVERY op-leg shape in both runs
# (gemm by 1-7 % at 1280 and 3840 rows, the two within 1 % of each other and in either order at 960 rows), so the rule picks neither and
# the route every other caller of the step kernels takes stays
CLIP_BWD = "packed"
LSTM_CLIP_CALLS = {"wide": 0, "packed": 0, "gemm": 0, "composed": 0}     # which forward form ran (tests assert it)


def clip_lengths(num_frames, clip, clips):
    """The valid frames of every clip, [B * clips] int32 by row b * clips + j: min(max(n_b - clip j, 0), clip)."""
    j = torch.arange(clips, device=num_frames.device, dtype=torch.int64)
    return (num_frames.to(torch.int64)[:, None] - clip * j[None, :]).clamp(0, clip).reshape(-1).to(torch.int32)


def lstm_clip_layer_composed(x, num_frames, clip, W, b, forget_bias=1.0):
    """lstm_clip_layer in plain torch under autograd: a Python time loop over the `clip` steps, in the dtype of its operands."""
    LSTM_CLIP_CALLS["composed"] += 1
    if x.dtype == torch.uint8:
        x = ops.dequant_l2norm(x, num_frames)
    B, F, D = x.shape
    U2, H = F // clip, W.shape[1] // 4
    live = (torch.arange(F, device=x.device)[None, :] < num_frames.to(x.device)[:, None]).to(x.dtype)
    xc = (x * live[:, :, None])[:, :clip * U2].reshape(B * U2, clip, D).to(W.dtype)
    h = c = torch.zeros((B * U2, H), dtype=W.dtype, device=x.device)
    for t in range(clip):
        i, j, f, o = (torch.cat([xc[:, t], h], dim=1) @ W + b).split(H, dim=1)
        c = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(c) * torch.sigmoid(o)
    return c.view(B, U2, H).transpose(0, 1)


def _on_rec_stream(dev, fn):
    """fn's launches on a recurrence side stream, between two joins with the current stream: the packed step chains are captured and
    replayed as hipGraphs (csrc/runtime.hip), which a capture on the legacy default stream cannot do."""
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev, "clip", REC_STREAM_PRIORITY)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        fn()
    main.wait_stream(side)


class _ClipParam(object):
    """What _StackLayer reads of a Variable, for a parameter that reaches the op as a tensor under autograd."""

    def __init__(self, data):
        self.data, self.grad = data, None


class _LstmClipLayer(torch.autograd.Function):
    """lstm_clip_layer on the device: _StackLayer's hoisted products and buffers (the byte and float product forms of the orchestrated
    stack) around U1 recurrence steps over B' = B U2 rows -- the wide step kernel, or yt8m_lstm_steps_fwd -- and yt8m_lstm_steps_bwd
    seeded with the final memories' gradient alone.  The wide steps and every product run on the current stream, the existing step
    routes on a side stream joined at both ends (_on_rec_stream); the frames are data (no dx)."""

    @staticmethod
    def forward(ctx, frames, W, b, nf_clip, B, forget_bias, route, bwd_route):
        lib = _lib.lib()
        u8 = frames.dtype == torch.uint8
        U1 = frames.shape[1] if u8 else frames.shape[0]
        q = _ByteFrames(lib, frames, nf_clip, [(0, U1)]) if u8 else None
        x_tm = q.x_tm if u8 else _f32c(frames)
        _dev(x_tm)
        st = _StackLayer(lib, x_tm, _ClipParam(_f32c(W.detach())), _ClipParam(_f32c(b.detach())), None, forget_bias, False, None, None,
                         None, q)
        st.out = None                                               # only the final memories leave the op
        if route != "packed":
            st.Wp = None
        Bp, H, dev = st.B, st.H, x_tm.device
        st.prepare_fwd()
        st.project(0, U1)
        if route == "wide":
            need = lib.yt8m_lstm_wide_workspace_bytes(Bp, H)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _lib.check(lib.yt8m_lstm_wide_prepare(_p(st.W.data[st.Din:]), 4 * H, Bp, H, _p(ws), need, _stream()))
            _lib.check(lib.yt8m_lstm_wide_steps_fwd(_p(st.z), _p(ws), need, _p(st.cs), _p(st.hs), None, 0, U1, Bp, H, st.forget_bias,
                                                    _stream()))
        else:
            _on_rec_stream(dev, lambda: st.recur_fwd(0, U1))
        LSTM_CLIP_CALLS[route] += 1
        st.release(("undropped", "bytes"))
        ctx.st, ctx.B, ctx.bwd_route = st, B, bwd_route
        return st.cs[U1].view(B, Bp // B, H).transpose(0, 1).contiguous()          # row b U2 + j -> (j, b)

    @staticmethod
    def backward(ctx, dout):
        st, B = ctx.st, ctx.B
        ctx.st = None
        if dout is None:
            return (None,) * 8
        U1, Bp, H = st.F, st.B, st.H
        dc = _f32c(dout).transpose(0, 1).contiguous().view(Bp, H)   # (j, b) -> row b U2 + j
        st.release(st.FWD_ONLY)
        st.alloc_bwd(None, True, False)
        if ctx.bwd_route != "packed":
            st.Wq = None
        st.prepare_bwd(None, dc)
        _on_rec_stream(dc.device, lambda: st.recur_bwd(0, U1))
        dz = st.dx_operands(0, U1)
        gW = gb = None
        if ctx.needs_input_grad[1]:
            gW = st.W.grad = torch.empty_like(st.W.data)
            st.weight_grad(0, U1, 0.0, dz)
        if ctx.needs_input_grad[2]:
            gb = st.b.grad = torch.empty_like(st.b.data)
            st.bias_grad(0, U1, 0.0)
        return None, gW, gb, None, None, None, None, None


def lstm_clip_route(rows, H):
    """The forward route lstm_clip_layer takes at `rows` clip rows of H cells: "wide" | CLIP_FWD_EXISTING."""
    if WIDE and rows >= WIDE_MIN_ROWS and _lib.lib().yt8m_lstm_wide_supported(int(rows), int(H)):
        return "wide"
    return CLIP_FWD_EXISTING


def lstm_clip_layer(x, num_frames, clip, W, b, forget_bias=1.0):
    """RNN-1 of Z/frame_level_models.py:3629-3683 (LstmLayerModel) as one op: every video of x [B,F,D] -- the reader's bytes or float
    frames -- is cut into U2 = F // clip clips of `clip` frames (the frames past clip U2 are dropped), one BasicLSTMCell(forget_bias) runs
    over all B U2 clips as one batch for `clip` steps from zero state with no lengths (dynamic_rnn, sequence_length=None), and the final
    MEMORIES come back time-major for the second LSTM: [U2, B, H], row (j, b) = clip j of video b.  Frames at or past num_frames are zero
    vectors, as the reader pads them: on the bytes the image builders mask them by the clip's valid count clip_lengths(), on floats by a
    multiply.  W [D + H, 4H], b [4H]: tensors under autograd (ops.as_tensor of the cell's Variables); the frames are data, no dx.
    Device: the hoisted projection and the weight gradients are the orchestrated stack's products (_StackLayer); the recurrence runs on
    the wide step kernel (lstm_clip_route) or an existing per-step route, the backward on yt8m_lstm_steps_bwd; --compute_dtype=bfloat16 does not reach this op (its
    products keep the fp32-grade forms).  CPU tensors take lstm_clip_layer_composed, which computes the same function."""
    clip = int(clip)
    B, F, D = x.shape
    U2, H = F // clip, W.shape[1] // 4
    assert clip >= 1 and U2 >= 1, "lstm_clip_layer needs at least one whole clip"
    if not x.is_cuda:
        return lstm_clip_layer_composed(x, num_frames, clip, W, b, forget_bias)
    if F != clip * U2:
        x = x[:, :clip * U2].contiguous()
    nf = num_frames.to(x.device)
    if x.dtype == torch.uint8:
        frames, nf_clip = x.contiguous().view(B * U2, clip, D), clip_lengths(nf, clip, U2)
    else:                                                           # (layout glue on data: the mask and the time-major copy in one pass)
        live = (torch.arange(clip * U2, device=x.device)[None, :] < nf[:, None]).to(x.dtype)
        frames, nf_clip = (x * live[:, :, None]).view(B * U2, clip, D).transpose(0, 1).contiguous(), None
    return _LstmClipLayer.apply(frames, W, b, nf_clip, B, float(forget_bias), lstm_clip_route(B * U2, H), CLIP_BWD)


# ---- tf.nn.bidirectional_dynamic_rnn: time reversal per video + the two directions' stacks -----------------------------------------
def reverse_sequence_u8(q, num_frames):
    """tf.reverse_sequence(q, num_frames, seq_axis=1) on the reader's bytes [B,F,D] (csrc/sequence.hip): frames 0 .. n_b - 1 of
    every video reversed, the padding frames left where they are.  The bytes are data: no gradient."""
    _dev(q)
    q = q.contiguous()
    B, F, D = q.shape
    out = torch.empty_like(q)
    nf = _nf(num_frames.to(q.device))
    _lib.check(_lib.lib().yt8m_reverse_sequence_u8(_p(q), _p(nf), _p(out), B, F, D, _stream()))
    return out


def _reverse_tm_into(x, nf, out, col0):
    """x [F,B,H] fp32 (rows contiguous, any row stride) reversed per video into columns [col0, col0 + H) of out [F,B,ldy]."""
    F, B, H = x.shape
    assert x.stride(2) == 1 and x.stride(0) == B * x.stride(1) and out.stride(2) == 1 and out.stride(0) == B * out.stride(1)
    _lib.check(_lib.lib().yt8m_reverse_sequence_f32_tm(_p(x), x.stride(1), _p(nf), _p(out), out.stride(1), int(col0), F, B, H, _stream()))
    return out


class _ReverseTM(torch.autograd.Function):
    """tf.reverse_sequence on time-major fp32 [F,B,H]; its own gradient (the reversal is an involution)."""

    @staticmethod
    def forward(ctx, x, num_frames):
        _dev(x)
        x = _f32c(x)
        ctx.nf = _nf(num_frames.to(x.device))
        return _reverse_tm_into(x, ctx.nf, torch.empty_like(x), 0)

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g)
        return _reverse_tm_into(g, ctx.nf, torch.empty_like(g), 0), None


def reverse_sequence_tm(x, num_frames):
    return _ReverseTM.apply(x, num_frames)


class _BiConcat(torch.autograd.Function):
    """concat([out_fw, reverse_sequence(out_bw)], axis=2) time-major -> [F,B,2H]: the bw half is written reversed straight into its
    column window by the reversal kernel (no cat / flip); backward: the left half of the gradient as is, the right half reversed back
    into a contiguous [F,B,H] by the same kernel."""

    @staticmethod
    def forward(ctx, out_fw, out_bw, num_frames):
        _dev(out_fw, out_bw)
        F, B, H = out_fw.shape
        ctx.nf, ctx.H = _nf(num_frames.to(out_fw.device)), H
        l1 = torch.empty((F, B, 2 * H), dtype=torch.float32, device=out_fw.device)
        l1[:, :, :H].copy_(out_fw)                                  # (layout glue)
        _reverse_tm_into(_f32c(out_bw), ctx.nf, l1, H)
        return l1

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g)
        F, B, _ = g.shape
        H = ctx.H
        d_fw = g[:, :, :H].contiguous()
        d_bw = _reverse_tm_into(g[:, :, H:], ctx.nf, torch.empty((F, B, H), dtype=torch.float32, device=g.device), 0)
        return d_fw, d_bw, None


def bi_concat(out_fw, out_bw, num_frames):
    return _BiConcat.apply(out_fw, out_bw, num_frames)


BI_OVERLAP_RUNS = [0]          # how often the overlapped form ran (tests assert that it engaged)


def bidirectional_lstm_stacks(x_fw, x_bw, num_frames, wb_fw, wb_bw, forget_bias=1.0, chunks=4, bf16=False, overlap=None):
    """The two directions of tf.nn.bidirectional_dynamic_rnn over already reversed bw input (reverse_sequence_u8 / _tm): two independent
    stacks that own separate scratch (slot 0 / 1).  overlap (default YT8M_BI_OVERLAP): bw on a side stream and the library's second
    stream set, forward recurrences of both capped at half the chip; False: one after the other on the caller's stream (the reference
    form).  Returns ((out_fw, finals_fw), (out_bw_reversed_time, finals_bw))."""
    if overlap is None:
        overlap = BI_OVERLAP
    kw = dict(forget_bias=forget_bias, chunks=chunks, bf16=bf16)
    if not overlap:
        return lstm_stack(x_fw, num_frames, wb_fw, slot=0, **kw), lstm_stack(x_bw, num_frames, wb_bw, slot=1, **kw)
    lib = _lib.lib()
    dev = x_fw.device
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev, "bi", REC_STREAM_PRIORITY)
    side.wait_stream(main)
    half = torch.cuda.get_device_properties(dev).multi_processor_count // 2
    prev_f, prev_b = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(lib.yt8m_lstm_persist_get_cus(ctypes.byref(prev_f), ctypes.byref(prev_b)))
    # (a tighter cap the caller set stays; the backward launches keep theirs -- half the chip by default)
    _lib.check(lib.yt8m_lstm_persist_set_cus(min(prev_f.value, half) if prev_f.value > 0 else half, prev_b.value))
    try:
        fw = lstm_stack(x_fw, num_frames, wb_fw, slot=0, stream_set=0, **kw)
        with torch.cuda.stream(side):
            bw = lstm_stack(x_bw, num_frames, wb_bw, slot=1, stream_set=1, **kw)
    finally:
        _lib.check(lib.yt8m_lstm_persist_set_cus(prev_f.value, prev_b.value))   # process-wide: the caller's values, whatever happens
    main.wait_stream(side)
    for t in [bw[0]] + [v for pair in bw[1] for v in pair]:
        t.record_stream(main)                                        # made on the side stream, read on the caller's
    x_bw.record_stream(side)
    BI_OVERLAP_RUNS[0] += 1
    return fw, bw


class _AttnSoftmax(torch.autograd.Function):
    """mask * softmax over frames, renormalised (lstm_attention_max_pooling_model.py:59-60).  act, w: [B,F,A]."""

    @staticmethod
    def forward(ctx, act, num_frames):
        act = _f32c(act)
        _dev(act)
        B, F, A = act.shape
        w = torch.empty_like(act)
        nf = _nf(num_frames)
        _lib.check(_lib.lib().yt8m_attn_softmax_fwd(_p(act), _p(nf), _p(w), B, F, A, _stream()))
        ctx.save_for_backward(w)
        ctx.nf = nf
        return w

    @staticmethod
    def backward(ctx, dw):
        (w,) = ctx.saved_tensors
        dw = _f32c(dw)
        B, F, A = w.shape
        dact = torch.empty_like(w)
        _lib.check(_lib.lib().yt8m_attn_softmax_bwd(_p(w), _p(dw), _p(ctx.nf), _p(dact), B, F, A, _stream()))
        return dact, None


def attention_weights(act, num_frames):
    return _AttnSoftmax.apply(act, num_frames)


class _SoftmaxRows(torch.autograd.Function):
    """a = softmax over the last axis, zeroed on padding frames (NetVLAD assignment)."""

    @staticmethod
    def forward(ctx, s, num_frames):
        s = _f32c(s)
        _dev(s)
        B, F, K = s.shape
        a = torch.empty_like(s)
        nf = _nf(num_frames)
        _lib.check(_lib.lib().yt8m_softmax_rows_fwd(_p(s), _p(nf), _p(a), B, F, K, _stream()))
        ctx.save_for_backward(a)
        ctx.nf = nf
        return a

    @staticmethod
    def backward(ctx, da):
        (a,) = ctx.saved_tensors
        da = _f32c(da)
        B, F, K = a.shape
        ds = torch.empty_like(a)
        _lib.check(_lib.lib().yt8m_softmax_rows_bwd(_p(a), _p(da), _p(ctx.nf), _p(ds), B, F, K, _stream()))
        return ds, None


def masked_softmax_rows(s, num_frames):
    return _SoftmaxRows.apply(s, num_frames)


POOL_STREAM_MIN = 1 << 22      # elements of x from which the streaming pooling kernels replace the padded batched GEMM


def _pool_stream_ok(w, x):
    B, F, A = w.shape
    H = x.shape[2]
    return (A <= 16 and x.numel() >= POOL_STREAM_MIN and x.data_ptr() % 16 == 0
            and _lib.lib().yt8m_attn_pool_supported(B, F, A, H) == 1)


class _PoolTN(torch.autograd.Function):
    """C[b] = w[b]^T . x[b]   (w [B,F,A], x [B,F,H] -> [B,A,H]): attention pooling
    (lstm_attention_max_pooling_model.py:63) and NetVLAD aggregation (Appendix B).  A handful of attentions over a large
    frame block takes the streaming kernels (yt8m_attn_pool_*: x crosses HBM once per pass); otherwise one batched GEMM."""

    @staticmethod
    def forward(ctx, w, x):
        w, x = _f32c(w), _f32c(x)
        ctx.save_for_backward(w, x)
        if _pool_stream_ok(w, x):
            B, F, A = w.shape
            H = x.shape[2]
            C = torch.empty((B, A, H), dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().yt8m_attn_pool_fwd(_p(w), _p(x), _p(C), B, F, A, H, _stream()))
            return C
        return ops.gemm_batched(w, x, transA=True)

    @staticmethod
    def backward(ctx, dC):
        w, x = ctx.saved_tensors
        dC = _f32c(dC)
        if _pool_stream_ok(w, x):
            B, F, A = w.shape
            H = x.shape[2]
            dw = torch.empty_like(w) if ctx.needs_input_grad[0] else None
            dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
            if dw is not None or dx is not None:
                _lib.check(_lib.lib().yt8m_attn_pool_bwd(_p(w), _p(x), _p(dC), _p(dw), _p(dx), B, F, A, H, _stream()))
            return dw, dx
        dw = ops.gemm_batched(x, dC, transB=True) if ctx.needs_input_grad[0] else None   # [F,H].[H,A]
        dx = ops.gemm_batched(w, dC) if ctx.needs_input_grad[1] else None                # [F,A].[A,H]
        return dw, dx


def pool_tn(w, x):
    return _PoolTN.apply(w, x)


# ---- attention branch straight from the reader's uint8 frames (csrc/gemm_skinny.hip, uint8 rows) -----------------------------
# x = diag(rs) (a0 q + c0): Dequantize (W/utils.py:23-38), mask and l2-normalise (W/all_feature_transform/default_transformer.py:4-8)
# of the frames W/readers.py:178-187 hands over as uint8, folded into the logit FC, the pooling and their gradients.

def u8_attention_supported(q, A):
    if q.dtype != torch.uint8 or q.dim() != 3 or not q.is_cuda:
        return False
    B, F, D = q.shape
    L = _lib.lib()
    return bool(D % 4 == 0 and D <= 2048 and L.yt8m_attn_pool_supported(B, F, A, D) == 1 and L.yt8m_skinny_supported(B * F, D, A) == 1)


def u8_frame_scales(q, num_frames, eps=1e-12):
    """rs [B,F] = 1 / ||a0 q + c0|| per frame, 0 for the padding frames."""
    q = q.contiguous()
    _dev(q)
    B, F, D = q.shape
    rs = torch.empty((B, F), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().yt8m_u8_frame_scales(_p(q), _p(_nf(num_frames)), B, F, D, float(eps), _p(rs), _stream()))
    return rs


def pool_u8_raw(w, q, rs):
    """C [B,A,D] = (w (.) rs)^T (a0 q + c0) without autograd (w [B,F,A])."""
    B, F, A = w.shape
    D = q.shape[2]
    C = torch.empty((B, A, D), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().yt8m_attn_pool_fwd_u8(_p(w), _p(q), _p(rs), _p(C), B, F, A, D, _stream()))
    return C


class _PoolU8(torch.autograd.Function):
    """att[b] = w[b]^T x[b] of W/all_frame_models/lstm_attention_max_pooling_model.py:63 with x from the raw frames; the
    gradient goes to the weights only (the frames are the input)."""

    @staticmethod
    def forward(ctx, w, q, rs):
        w = _f32c(w)
        _dev(w, q, rs)
        ctx.save_for_backward(q, rs)
        ctx.shape = tuple(w.shape)
        return pool_u8_raw(w, q, rs)

    @staticmethod
    def backward(ctx, dC):
        q, rs = ctx.saved_tensors
        dC = _f32c(dC)
        B, F, A = ctx.shape
        D = q.shape[2]
        dCsum = dC.sum(dim=2)                                         # [B,A]: the rank-1 remainder of the dequantise affine
        dw = torch.empty((B, F, A), dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().yt8m_attn_pool_dw_u8(_p(q), _p(rs), _p(dC), _p(dCsum), _p(dw), B, F, A, D, _stream()))
        return dw, None, None


def pool_tn_u8(w, q, rs):
    return _PoolU8.apply(w, q, rs)


class _AttnLogitsU8(torch.autograd.Function):
    """act [B,F,A] = slim.fully_connected(concat(x, parts...)) of lstm_attention_max_pooling_model.py:51-56 /
    lstm_positional_attention_max_pooling_model.py:77-84 with x from the raw frames: W rows [0, D) meet the frames, the following rows
    the other parts in concatenation order -- kinds[i] = 0: a per-frame float tensor [B,F,K_i] (the LSTM outputs, a positional embedding),
    kinds[i] = 1: a per-video vector [B,K_i] that the reference tiles over the frames (the mean frame)."""

    @staticmethod
    def forward(ctx, token, W, b, q, rs, kinds, *parts):
        _dev(q, rs)
        B, F, D = q.shape
        N = W.data.shape[1]
        parts = [_f32c(p).reshape(B * F, p.shape[-1]) if k == 0 else _f32c(p) for k, p in zip(kinds, parts)]
        assert W.data.shape[0] == D + sum(p.shape[1] for p in parts), "parts do not add up to the weight's input width"
        Wx = W.data[:D]
        cs = Wx.sum(dim=0)
        y = torch.empty((B * F, N), dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().yt8m_skinny_fwd_u8(_p(q), D, _p(Wx), Wx.stride(0), _p(b.data if b is not None else None), _p(rs), _p(cs),
                                                 _p(y), N, B * F, D, N, 0.0, _stream()))
        ops._cat_parts_fwd(y, W, D, parts, kinds, F)                  # the byte part has written y: every other part accumulates
        ctx.save_for_backward(q, rs, *parts)
        ctx.W, ctx.b, ctx.kinds = W, b, tuple(kinds)
        return y.view(B, F, N)

    @staticmethod
    def backward(ctx, dy):
        q, rs = ctx.saved_tensors[:2]
        parts = ctx.saved_tensors[2:]
        W, b, kinds = ctx.W, ctx.b, ctx.kinds
        B, F, D = q.shape
        dy = _f32c(dy).view(B * F, -1)
        N = dy.shape[1]
        wbeta = W.grad_beta() if (W.trainable and W.grad is not None) else None
        if wbeta is not None:
            gx = W.grad[:D]
            ws = ops._workspace(q.device)
            _lib.check(_lib.lib().yt8m_skinny_dw_u8(_p(q), D, _p(dy), N, _p(rs), _p(gx), gx.stride(0), B * F, D, N, float(wbeta),
                                                    _p(ws), ws.numel() * 4, _stream()))
        dparts = ops._cat_parts_bwd(dy, W, b, wbeta, D, parts, kinds, F, ctx.needs_input_grad[6:])
        dparts = [d if (d is None or kind == 1) else d.view(B, F, -1) for kind, d in zip(kinds, dparts)]
        return (None, None, None, None, None, None) + tuple(dparts)


def attention_logits_u8(q, rs, mean_x, W, b, parts=None):
    """Default form (parts None): concat(x, tile(mean_x)).  parts: the tensors that follow the frames in the concatenation, in order --
    [B,F,K] per-frame float tensors and / or [B,K] per-video vectors (tiled over the frames)."""
    if parts is None:
        parts = [mean_x]
    kinds = tuple(1 if p.dim() == 2 else 0 for p in parts)
    return _AttnLogitsU8.apply(_token(W._graph), W, b, q, rs, kinds, *parts)


U8_ALPHA = 4.0 / 255.0


def _u8_frames_supported(q):
    """What every product on U8FrameImages needs: the reader's bytes [B,F,D] on the device, D in whole K blocks of 16 that the byte
    projection covers."""
    if q.dtype != torch.uint8 or q.dim() != 3 or not q.is_cuda:
        return False
    B, F, D = q.shape
    return bool(D % 16 == 0 and 16 <= D <= 2048 and F >= 1 and _lib.lib().yt8m_u8_proj_supported(D))


def u8_cnn_supported(q):
    """The einsum CNN of W/all_frame_models/cnn_deep_combine_chain_model.py:60-82 straight from the reader's bytes (u8_cnn): the shifted
    weight-gradient products want whole K blocks per shift (B % 16 == 0)."""
    return _u8_frames_supported(q) and q.shape[0] % 16 == 0


def u8_hoisted_supported(q):
    """A recurrent layer's hoisted input projection straight from the reader's bytes (GRU and LayerNorm-LSTM layers outside the native
    stack): whole K blocks of frame rows for the weight gradient (F B % 16 == 0)."""
    return _u8_frames_supported(q) and (q.shape[1] * q.shape[0]) % 16 == 0


def _colsum_row(x):
    return ops.colsum(x, torch.empty((x.shape[1],), dtype=torch.float32, device=x.device))


def _colsum_row_torch(x):
    return x.sum(0).contiguous()


class U8FrameImages(object):
    """Operand images of one batch of raw frames q [B,F,D] uint8, made ONCE per step and shared by every product that reads the frames:
    `img` = (q - 128) as a one-plane half image in TIME-major row order t B + b (exact; yt8m_u8_frames_image_f16), `r` [F B] = 1 / ||a0 q + c0||
    per frame (0 on the padding frames), `trans()` = the transposed image (K = frame rows) for weight gradients, made on first use.
    project / weight_grad are the two products on them, x = the dequantised, l2-normalised, padding-masked frames (W/utils.py:23-38,
    readers.py:178-187, default_transformer.py:4-8); a recurrent layer takes them as its hoisted input (as _FloatFrames for floats), the
    einsum CNN once per shift: in time-major row order a shift by i frames is a row offset of i B."""

    def __init__(self, q, num_frames, eps=1e-12):
        q = q.contiguous()
        _dev(q)
        self.q, self.nf = q, _nf(num_frames)
        self.B, self.F, self.D = q.shape
        self.device = q.device
        M = self.F * self.B
        self.img = torch.empty(((M + 31) // 32) * (self.D // 16) * 1024, dtype=torch.uint8, device=q.device)
        self.r = torch.empty((M,), dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().yt8m_u8_frames_image_f16(_p(q), _p(self.nf), self.B, self.F, self.D, float(eps), _p(self.img), None, _p(self.r),
                                                       _stream()))
        self.saved = self.r                                           # what a layer saves for backward
        self._t = None

    def trans(self):
        if self._t is None:
            M = self.F * self.B
            self._t = torch.empty(((self.D + 31) // 32) * ((M + 15) // 16) * 1024, dtype=torch.uint8, device=self.q.device)
            _lib.check(_lib.lib().yt8m_u8_frames_image_t_f16(_p(self.q), _p(self.nf), self.B, self.F, self.D, _p(self._t), _stream()))
        return self._t

    def project(self, Wrows, bias, out2d, *, row_shift=0, image=None, beta=0.0):
        """out2d[row_shift B ..] = x[.. M - row_shift B] . Wrows (+ bias) (+ itself if beta == 1), out2d [F B rows (t B + b), N] (a column
        window of a wider matrix will do): two f16 products of the frames' half image against (alpha Wrows)^T under a device-measured
        scale, the affine remainder in the epilogue (yt8m_gemm_h1x2_nt_ex) -- the form the native LSTM stack's layer 0 takes.
        image = (H2Image of a taller W^T, first of Wrows' rows in it): Wrows is that K window of an operand image made by the caller."""
        out = out2d[row_shift * self.B:]
        rows, D = out.shape[0], self.D
        if rows <= 0:
            return
        w2, k0 = image or (ops.h2_split(Wrows, plain=False, trans=True, scale=U8_ALPHA, dynamic=True)[1], 0)
        bptr = ctypes.c_void_p(w2.buf.data_ptr() + k0 // 16 * 2048)     # K blocks of 16: two 1 KiB half planes each
        N = Wrows.shape[1]
        cs = _colsum_row(Wrows)
        ws = ops._workspace(self.device)
        _lib.check(_lib.lib().yt8m_gemm_h1x2_nt_ex(rows, N, D, _p(self.img), 0, bptr, w2.K // 16 if w2.K > D else 0, _p(out), out.stride(0),
                                                   _p(bias), 1.0, _p(w2.dinv), _p(self.r), _p(cs), U8_BETA, float(beta), _p(ws),
                                                   ws.numel() * 4, _stream()))

    def weight_grad(self, dy2d, gWrows, beta, *, row_shift=0, colsum=_colsum_row):
        """gWrows [D, N] (beta = 0 / 1: overwrite / accumulate) (+)= x[.. M - row_shift B]^T . dy2d[row_shift B ..]: the transposed byte
        image at K offset 0 against (r (.) dy)^T written by one pass over dy (yt8m_h2_split_ex), the affine remainder as a rank-1 term of
        the epilogue.  colsum: how that pass' per-tile partial sums are reduced (the CNN keeps torch's sum, see DESIGN_LOG.md 16).  The
        frames are data: no dx."""
        M, D = self.F * self.B, self.D
        part = dy2d[row_shift * self.B:].contiguous()                 # dy of the frames that saw this shift
        rows, N = part.shape
        if rows <= 0:
            if beta == 0.0:
                gWrows.zero_()
            return
        dev = part.device
        lib = _lib.lib()
        word = ops.h2_absmax(part)
        dzT = ops.image_buffer(N, rows, 2, dev)
        dzTs = ops.image_buffer(N, rows, 2, dev)
        ntile = (rows + 63) // 64
        cp = torch.empty((ntile, N), dtype=torch.float32, device=dev)
        cps = torch.empty((ntile, N), dtype=torch.float32, device=dev)
        _lib.check(lib.yt8m_h2_split_ex(_p(part), rows, N, N, 1.0, _p(word), _p(self.r), None, _p(dzT), _p(dzTs), _p(cp), _p(cps), _stream()))
        csr = colsum(cps)
        ws = ops._workspace(dev)
        _lib.check(lib.yt8m_gemm_h1x2_nt_ex(D, N, rows, _p(self.trans()), (M + 15) // 16, _p(dzTs), 0, _p(gWrows), N, None, U8_ALPHA, _p(word),
                                            None, _p(csr), U8_BETA / U8_ALPHA, float(beta), _p(ws), ws.numel() * 4, _stream()))

    def dx(self, dy2d, Wrows, into=None):
        return None                                                   # the frames are data


def _u8_cnn_dense(frames, filters):
    """y [F B rows (t B + b), sum N_k]: for every filter k and shift i < fs_k
        y_k[rows i B ..] += x[rows .. M - i B] . W_k[i D : (i + 1) D]
    as ONE frames.project launch against the K range [i D, (i + 1) D) of the filter's half-plane image (alpha W_k)^T -- one image and
    one device-measured scale per filter --, accumulated in place."""
    D = frames.D
    Ntot = sum(W.data.shape[1] for W in filters)
    y = torch.empty((frames.F * frames.B, Ntot), dtype=torch.float32, device=frames.device)
    c0 = 0
    for W in filters:
        assert W.data.shape[0] % D == 0 and W.data.is_contiguous(), "cnn filter must be [fs * D, N]"
        fs, N = W.data.shape[0] // D, W.data.shape[1]
        _, w2 = ops.h2_split(W.data, plain=False, trans=True, scale=U8_ALPHA, dynamic=True)     # [N rows, K = fs D]
        for i in range(fs):
            frames.project(W.data[i * D:(i + 1) * D], None, y[:, c0:c0 + N], row_shift=i, image=(w2, i * D), beta=1.0 if i else 0.0)
        c0 += N
    return y


def _u8_cnn_dw(frames, filters, dyt):
    """Weight gradients of _u8_cnn_dense from dyt [F B rows (t B + b), sum N_k]: per filter slice x[.. M - i B]^T . dy_k[i B ..]
    (frames.weight_grad)."""
    D = frames.D
    c0 = 0
    for W in filters:
        fs, N = W.data.shape[0] // D, W.data.shape[1]
        if W.trainable and W.grad is not None:
            wbeta = float(W.grad_beta())
            for i in range(fs):
                frames.weight_grad(dyt[:, c0:c0 + N], W.grad[i * D:(i + 1) * D], wbeta, row_shift=i, colsum=_colsum_row_torch)
            W.grad_done()
        c0 += N


class _CnnU8(torch.autograd.Function):
    """cnn_output [B,F,sum N_k] of cnn_deep_combine_chain_model.py:60-82 -- for every filter k of length fs_k, einsum("ijk,kl->ijl") of
    concat(x, x shifted by 1 frame, ..., by fs_k - 1 frames) with W_k [fs_k D, N_k] -- without the concatenations and without a float
    copy of the frames (_u8_cnn_dense).  Backward: the slice's weight gradient x[.. M - i B]^T . dy_k[i B ..] from the transposed byte
    image at K offset 0 (the recurrent stack's layer-0 form).  The frames are data: no dx.  (The model pools this output over the frames:
    _PooledCnnU8 is the form it uses; this one is the plain `cnn` of the reference class.)"""

    @staticmethod
    def forward(ctx, token, frames, *filters):
        y = _u8_cnn_dense(frames, filters)
        ctx.frames, ctx.filters = frames, filters
        return y.view(frames.F, frames.B, y.shape[1]).transpose(0, 1).contiguous()          # [B,F,N] (layout glue)

    @staticmethod
    def backward(ctx, dy):
        frames, filters = ctx.frames, ctx.filters
        M = frames.F * frames.B
        dyt = _f32c(dy).transpose(0, 1).contiguous().view(M, dy.shape[2])      # time-major rows, as the images
        _u8_cnn_dw(frames, filters, dyt)
        return (None, None) + (None,) * len(filters)


def _u8_cnn_partials(frames, filters):
    """z [F B rows (t B + b), sum_k fs_k N_k] with z[., zbase_k + i N_k + n] = x . W_k[i D : (i + 1) D][:, n]: ONE product for the whole CNN
    (every filter's shift slices side by side as the rows of one half-plane image under one device-measured scale; N = 1152 instead of
    six launches of N = 128 / 256 on 256-wide tiles), the shifts are summed by the pooling pass (yt8m_timepool_shiftmax_f32).  Needs
    N_k % 32 == 0 (a slice then is a whole number of the image's 32-row groups)."""
    B, F, D = frames.B, frames.F, frames.D
    M = F * B
    dev = frames.q.device
    lib = _lib.lib()
    Ntz = sum(W.data.shape[0] // D * W.data.shape[1] for W in filters)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    for W in filters:                                                                            # max |W| over all filters (atomicMax)
        _lib.check(lib.yt8m_h2_absmax(_p(W.data), W.data.shape[0], W.data.shape[1], W.data.shape[1], _p(word), _stream()))
    nbytes = lambda rows, K: ops.image_bytes(rows, K, 2)
    img = torch.empty(sum(W.data.shape[0] // D * nbytes(W.data.shape[1], D) for W in filters), dtype=torch.uint8, device=dev)
    cs = torch.empty((Ntz,), dtype=torch.float32, device=dev)
    off, c = 0, 0
    for W in filters:
        fs, N = W.data.shape[0] // D, W.data.shape[1]
        for i in range(fs):
            Wi = W.data[i * D:(i + 1) * D]
            _lib.check(lib.yt8m_h2_split(_p(Wi), D, N, N, U8_ALPHA, _p(word), None, ctypes.c_void_p(img.data_ptr() + off), None, _stream()))
            ops.colsum(Wi, cs[c:c + N])
            off += nbytes(N, D)
            c += N
    z = torch.empty((M, Ntz), dtype=torch.float32, device=dev)
    ws = ops._workspace(dev)
    _lib.check(lib.yt8m_gemm_h1x2_nt_ex(M, Ntz, D, _p(frames.img), 0, _p(img), 0, _p(z), Ntz, None, 1.0, _p(word), _p(frames.r), _p(cs), U8_BETA,
                                        0.0, _p(ws), ws.numel() * 4, _stream()))
    return z


class _PooledCnnU8(torch.autograd.Function):
    """tf.reduce_max(cnn_output, axis=1) of cnn_deep_combine_chain_model.py:100-106 on the raw frames: the dense products of
    _u8_cnn_dense, the pooling in time-major order with the argmax kept (yt8m_timepool_max_f32), and a backward that uses what the
    pooling did to the gradient -- it is non-zero at ONE frame per (video, column), so each filter slice's gradient is B gathered frame
    rows per column (yt8m_u8_cnn_pool_dw) instead of a [D, F B] x [F B, N] product."""

    @staticmethod
    def forward(ctx, token, frames, *filters):
        B, F, D = frames.B, frames.F, frames.D
        dev = frames.q.device
        Ntot = sum(W.data.shape[1] for W in filters)
        out = torch.empty((B, Ntot), dtype=torch.float32, device=dev)
        idx = torch.empty((B, Ntot), dtype=torch.int32, device=dev)
        if all(W.data.shape[1] % 32 == 0 for W in filters) and len(filters) <= 8:
            z = _u8_cnn_partials(frames, filters)                     # one product; the pooling pass sums the shifts
            fs = (ctypes.c_int32 * len(filters))(*[W.data.shape[0] // D for W in filters])
            nc = (ctypes.c_int32 * len(filters))(*[W.data.shape[1] for W in filters])
            _lib.check(_lib.lib().yt8m_timepool_shiftmax_f32(_p(z), F, B, z.shape[1], len(filters), fs, nc, _p(out), _p(idx), Ntot, _stream()))
        else:
            y = _u8_cnn_dense(frames, filters)                        # one product per (filter, shift), accumulated in place
            _lib.check(_lib.lib().yt8m_timepool_max_f32(_p(y), F, B, Ntot, Ntot, _p(out), _p(idx), Ntot, _stream()))
        ctx.frames, ctx.filters, ctx.idx = frames, filters, idx
        return out

    @staticmethod
    def backward(ctx, g):
        frames, filters, idx = ctx.frames, ctx.filters, ctx.idx
        ctx.idx = None
        B, F, D = frames.B, frames.F, frames.D
        g = _f32c(g)
        Ntot = g.shape[1]
        lib = _lib.lib()
        c0 = 0
        for W in filters:
            fs, N = W.data.shape[0] // D, W.data.shape[1]
            if W.trainable and W.grad is not None:
                wbeta = float(W.grad_beta())
                _lib.check(lib.yt8m_u8_cnn_pool_dw(_p(frames.q), _p(frames.r), ctypes.c_void_p(idx.data_ptr() + c0 * 4),
                                                   ctypes.c_void_p(g.data_ptr() + c0 * 4), Ntot, B, F, D, N, fs, _p(W.grad), wbeta,
                                                   _stream()))
                W.grad_done()
            c0 += N
        return (None, None) + (None,) * len(filters)


def u8_cnn(frames, filters):
    """frames: U8FrameImages; filters: the cnn-filter Variables [fs_k D, N_k] in output-column order -> cnn_output [B,F,sum N_k]."""
    return _CnnU8.apply(_token(filters[0]._graph), frames, *filters)


def u8_cnn_maxpool(frames, filters):
    """... -> reduce_max over the frames of that output, [B, sum N_k] (needs sum N_k % 4 == 0: else pool u8_cnn's output)."""
    return _PooledCnnU8.apply(_token(filters[0]._graph), frames, *filters)


def vlad_q_supported(D):
    """The intra-normalisation can hand out q = ||vlad[b,k,:]||^2 (csrc/netvlad.hip, register-resident kernels)."""
    return bool(_lib.lib().yt8m_vlad_finish_q_supported(int(D)))


def _finish_fwd(agg, a, n, centres, eps, want_q):
    B, K, D = agg.shape
    vlad = torch.empty_like(agg)
    q = torch.empty((B, K), dtype=torch.float32, device=agg.device) if want_q else None
    F = a.shape[1] if a is not None else 0
    if want_q:
        _lib.check(_lib.lib().yt8m_vlad_finish_q_fwd(_p(agg), _p(a), _p(centres.data), _p(vlad), _p(n), _p(q), B, F, K, D, eps, _stream()))
    else:
        _lib.check(_lib.lib().yt8m_vlad_finish_fwd(_p(agg), _p(a), _p(centres.data), _p(vlad), _p(n), B, F, K, D, eps, _stream()))
    return vlad, q


def _finish_bwd(agg, n, c, dvlad, dq, eps):
    B, K, D = agg.shape
    dagg = torch.empty_like(agg)
    dn = torch.empty((B, K), dtype=torch.float32, device=agg.device)
    dc = c.grad if c.grad is not None else None
    beta = c.grad_beta() if dc is not None else 0.0
    if dq is not None:
        _lib.check(_lib.lib().yt8m_vlad_finish_q_bwd(_p(agg), _p(n), _p(c.data), _p(dvlad), _p(dq), _p(dagg), _p(dn), _p(dc), beta, B, K,
                                                     D, eps, _stream()))
    else:
        _lib.check(_lib.lib().yt8m_vlad_finish_bwd(_p(agg), _p(n), _p(c.data), _p(dvlad), _p(dagg), _p(dn), _p(dc), beta, B, K, D, eps,
                                                   _stream()))
    if dc is not None:
        c.grad_done()
    return dagg, dn


class _VladFinish(torch.autograd.Function):
    """vlad[b,k,:] = l2norm_D(agg[b,k,:] - (sum_f a[b,f,k]) * c[k,:])   (residual aggregation +
    intra-normalisation in one pass, yt8m_vlad_finish_fwd/bwd); c is a Variable.  want_q: also q [B,K] = ||vlad[b,k,:]||^2
    (differentiable: its gradient reaches the clamped rows only), for the caller's descriptor-wide l2-normalisation."""

    @staticmethod
    def forward(ctx, agg, a, token, centres, eps, want_q):
        agg, a = _f32c(agg), _f32c(a)
        _dev(agg, a)
        B, K, D = agg.shape
        n = torch.empty((B, K), dtype=torch.float32, device=agg.device)
        vlad, q = _finish_fwd(agg, a, n, centres, eps, want_q)
        ctx.save_for_backward(agg, n)
        ctx.centres, ctx.F, ctx.eps, ctx.want_q = centres, a.shape[1], eps, want_q
        return (vlad, q) if want_q else vlad

    @staticmethod
    def backward(ctx, dvlad, dq=None):
        agg, n = ctx.saved_tensors
        if dvlad is None:
            dvlad = torch.zeros_like(agg)
        dagg, dn = _finish_bwd(agg, n, ctx.centres, _f32c(dvlad), None if dq is None else _f32c(dq), ctx.eps)
        da = dn.unsqueeze(1).expand(-1, ctx.F, -1) if ctx.needs_input_grad[1] else None   # broadcast view, no copy
        return dagg, da, None, None, None, None


def vlad_finish(agg, a, centres, eps=1e-12, want_q=False):
    return _VladFinish.apply(agg, a, _token(centres._graph), centres, eps, bool(want_q))


# ---- fused NetVLAD pooling on raw uint8 frames (csrc/netvlad_fused.hip) ---------------------------------------------
_NV_WS = {}


def _netvlad_workspace(B, F, D, K, device):
    need = _lib.lib().yt8m_netvlad_workspace_bytes(B, F, D, K)
    ws = _NV_WS.get(device)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _NV_WS[device] = ws
    return ws


def netvlad_fused_supported(q, K):
    return (q.dtype == torch.uint8 and q.dim() == 3 and q.is_cuda
            and bool(_lib.lib().yt8m_netvlad_supported(q.shape[0], q.shape[1], q.shape[2], K)))


def netvlad_fwd_u8(q, num_frames, Wc, bc, nsplit=2, eps=1e-12):
    """(cT [B,K,Fp], n [B,K], agg [B,K,D]) from raw uint8 frames (yt8m_netvlad_fwd_u8).  cT[b,k,f] = a[b,f,k] / ||deq(q[b,f])||
    with the frames contiguous and zero padded to Fp = 32*ceil(F/32): what the aggregation and the backward consume."""
    _dev(q, Wc, bc)
    q = q.contiguous()
    B, F, D = q.shape
    K = Wc.shape[1]
    nf = _nf(num_frames)
    Fp = (F + 31) // 32 * 32
    cT = torch.empty((B, K, Fp), dtype=torch.float32, device=q.device)
    n = torch.empty((B, K), dtype=torch.float32, device=q.device)
    agg = torch.empty((B, K, D), dtype=torch.float32, device=q.device)
    ws = _netvlad_workspace(B, F, D, K, q.device)
    _lib.check(_lib.lib().yt8m_netvlad_fwd_u8(_p(q), _p(nf), _p(_f32c(Wc)), _p(_f32c(bc)), B, F, D, K, int(nsplit), eps, _p(cT),
                                              _p(n), _p(agg), _p(ws), ws.numel(), _stream()))
    return cT, n, agg


def netvlad_bwd_u8(q, num_frames, cT, dagg, dn, dWc, dWc_beta, dbc, dbc_beta, nsplit=2, eps=1e-12):
    _dev(q, cT, dagg, dn, dWc, dbc)
    B, F, D = q.shape
    K = cT.shape[1]
    nf = _nf(num_frames)
    ws = _netvlad_workspace(B, F, D, K, q.device)
    _lib.check(_lib.lib().yt8m_netvlad_bwd_u8(_p(q), _p(nf), _p(cT), _p(_f32c(dagg)), _p(_f32c(dn)), B, F, D, K, int(nsplit), eps,
                                              _p(dWc), float(dWc_beta), _p(dbc), float(dbc_beta), _p(ws), ws.numel(), _stream()))


class _NetVladPoolU8(torch.autograd.Function):
    """uint8 frames -> intra-normalised VLAD descriptor [B,K,D], the dequantise + l2-normalise of
    the input pipeline folded into the two GEMMs; backward writes dW_c, db_c, dcentres into the gradient arena.  want_q: as
    _VladFinish."""

    @staticmethod
    def forward(ctx, q, num_frames, token, Wc, bc, centres, nsplit, eps, want_q):
        q = q.contiguous()
        cT, n, agg = netvlad_fwd_u8(q, num_frames, Wc.data, bc.data, nsplit)
        vlad, qn = _finish_fwd(agg, None, n, centres, eps, want_q)
        ctx.saved = (q, num_frames, cT, agg, n)
        ctx.vars = (Wc, bc, centres)
        ctx.cfg = (nsplit, eps)
        return (vlad, qn) if want_q else vlad

    @staticmethod
    def backward(ctx, dvlad, dq=None):
        q, num_frames, cT, agg, n = ctx.saved
        Wc, bc, c = ctx.vars
        nsplit, eps = ctx.cfg
        ctx.saved = None
        if dvlad is None:
            dvlad = torch.zeros_like(agg)
        dagg, dn = _finish_bwd(agg, n, c, _f32c(dvlad), None if dq is None else _f32c(dq), eps)
        if Wc.grad is not None and bc.grad is not None:
            netvlad_bwd_u8(q, num_frames, cT, dagg, dn, Wc.grad, Wc.grad_beta(), bc.grad.view(-1), bc.grad_beta(), nsplit)
            Wc.grad_done()
            bc.grad_done()
        return (None,) * 9


def netvlad_pool_u8(q, num_frames, Wc, bc, centres, nsplit=2, eps=1e-12, want_q=False):
    return _NetVladPoolU8.apply(q, num_frames, _token(Wc._graph), Wc, bc, centres, int(nsplit), eps, bool(want_q))


# ---- MultiscaleCnnLstmModel: CNN -> batch norm -> ReLU -> (LSTM input, pair-max for the next scale), everything time-major ------------
def bn_relu_pool2_supported(x, C):
    """The fused scale (csrc/multiscale.hip): a device tensor and C % 4 == 0 (16-byte column accesses)."""
    return bool(x.is_cuda and C % 4 == 0 and C >= 4)


class _CnnU8TM(torch.autograd.Function):
    """_CnnU8 without the layout glue: the einsum CNN on the reader's bytes with its output LEFT time-major [F B rows (t B + b), sum N_k]
    (what _u8_cnn_dense writes), the gradient taken time-major too."""

    @staticmethod
    def forward(ctx, token, frames, *filters):
        ctx.frames, ctx.filters = frames, filters
        return _u8_cnn_dense(frames, filters)

    @staticmethod
    def backward(ctx, dy):
        _u8_cnn_dw(ctx.frames, ctx.filters, _f32c(dy))
        return (None, None) + (None,) * len(ctx.filters)


def u8_cnn_tm(frames, filters):
    """frames: U8FrameImages; filters: cnn-filter Variables [fs_k D, N_k] in output-column order -> cnn_output [F B, sum N_k] time-major."""
    return _CnnU8TM.apply(_token(filters[0]._graph), frames, *filters)


def _cnn_tm_dense(x, B, filters):
    """y [M rows (t B + b), sum N_k] of _CnnTM from x [M, D] fp32: one grouped launch per shift (the products of one shift write disjoint
    column windows), accumulated in place."""
    M, D = x.shape
    Ntot = sum(W.data.shape[1] for W in filters)
    y = torch.empty((M, Ntot), dtype=torch.float32, device=x.device)
    fsmax = max(W.data.shape[0] // D for W in filters)
    for i in range(fsmax):                                         # products of one shift write disjoint column windows: one group
        rows = M - i * B
        items, role, c0 = [], "h2", 0
        for W in filters:
            fs, N = W.data.shape[0] // D, W.data.shape[1]
            assert W.data.shape[0] == fs * D, "cnn filter must be [fs * D, N]"
            if i < fs:
                if rows > 0:
                    items.append(dict(A=x[:rows], B=W.data[i * D:(i + 1) * D], out=y[i * B:, c0:c0 + N], beta=1.0 if i else 0.0))
                    # a fully-connected layer's forward form, whatever the compute dtype: the group takes the role when every product does
                    role = role if ops._dense_plan(rows, N, D, False, need_dx=False).fwd == "h2" else None
                elif i == 0:
                    y[:, c0:c0 + N].zero_()
            c0 += N
        if items:
            ops.gemm_grouped(items, role=role)
    return y


class _CnnTM(torch.autograd.Function):
    """The einsum CNN of W/all_frame_models/multiscale_cnn_lstm_model.py:12-38 on float frames in time-major order, x [F B rows (t B + b), D]:
    a shift by i frames is a row offset of i B, so filter k's output is
        y[i B :, cols_k] += x[: M - i B] . W_k[i D : (i + 1) D]          for i < fs_k   (the first i B rows get no term: zero padding)
    -- one product per (filter, shift) on row windows, no concatenated [., 2 D] / [., 3 D] inputs.  Backward: the slice's weight gradient
    x[: M - i B]^T . dy[i B :, cols_k] and dx[: M - i B] += dy[i B :, cols_k] . W_k[i D : (i + 1) D]^T."""

    @staticmethod
    def forward(ctx, x, token, B, *filters):
        x = _f32c(x)
        _dev(x)
        y = _cnn_tm_dense(x, B, filters)
        ctx.save_for_backward(x)
        ctx.filters, ctx.B = filters, B
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        filters, B = ctx.filters, ctx.B
        dy = _f32c(dy)
        M, D = x.shape
        dw, c0 = [], 0
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        first = True
        for W in filters:
            fs, N = W.data.shape[0] // D, W.data.shape[1]
            train = W.trainable and W.grad is not None
            wbeta = float(W.grad_beta()) if train else 0.0
            for i in range(fs):
                rows = M - i * B
                if rows <= 0:
                    if train and wbeta == 0.0:
                        W.grad[i * D:(i + 1) * D].zero_()
                    continue
                if train:
                    dw.append(dict(A=x[:rows], B=dy[i * B:, c0:c0 + N], out=W.grad[i * D:(i + 1) * D], beta=wbeta))
                if dx is not None:
                    if first and rows < M:
                        dx.zero_()
                    ops.gemm(dy[i * B:, c0:c0 + N], W.data[i * D:(i + 1) * D], out=dx[:rows], transB=True, beta=0.0 if first else 1.0)
                    first = False
            c0 += N
        if dw:
            ops.gemm_grouped(dw, transA=True, role="dw")               # disjoint gradient slices: one group
        for W in filters:
            if W.trainable and W.grad is not None:
                W.grad_done()
        if dx is not None and first:
            dx.zero_()
        return (dx, None, None) + (None,) * len(filters)


def cnn_tm(x_tm2d, B, filters):
    """x_tm2d [F B, D] float time-major (B videos per frame); filters as u8_cnn_tm -> cnn_output [F B, sum N_k] time-major."""
    return _CnnTM.apply(x_tm2d, _token(filters[0]._graph), int(B), *filters)


def cnn_tm_maxpool_supported(D, cnns):
    """The pooled chain (csrc/cnn_pool.hip, cnn_pool_f32.hip): 16-byte column windows per filter and per CNN, rows of D floats the
    gather kernels cover, at most 32 filters in all."""
    filters = [W for cnn in cnns for W in cnn]
    return bool(D % 4 == 0 and 4 <= D <= 2048 and len(filters) <= 32 and all(W.data.shape[1] % 4 == 0 and W.data.shape[1] >= 4 and
                                                                              W.data.shape[0] // D <= 16 for W in filters))


# The CNNs of a chain read the same x.  False: one set of products and one pooling pass per CNN (y [F B, sum N_k of the CNN], 79 MB at
# the script's shape, is pooled while the last-level cache still holds it); True: one set for the whole chain (y 314 MB).  Measured by
# tools/lstmcnn_step.py, see DESIGN_LOG.md 17.
CNN_POOL_WHOLE_CHAIN = False


class _PooledCnnChainTM(torch.autograd.Function):
    """tf.reduce_max(cnn(x), axis=1) of W/all_frame_models/lstm_cnn_deep_combine_chain_model.py:13-41,66-68,86-88 for EVERY CNN of the chain
    at once, x [F B rows (t B + b), D] fp32 time-major with a gradient (the LSTM outputs): the products of _CnnTM, the pooling over all F
    rows in time-major order with the argmax kept (yt8m_timepool_max_f32), and a backward that uses what the pooling did to the gradient
    -- non-zero at ONE frame per (video, column): B gathered rows of x per (column, shift) for a filter (yt8m_f32_cnn_pool_dw) and, for x,
    one gathered sum per row over the whole chain (yt8m_f32_cnn_pool_dx), instead of the dense [D, F B] x [F B, N] and
    [F B, N] x [N, D] products of a gradient that is all zeros but B sum N entries."""

    @staticmethod
    def forward(ctx, x, token, B, sizes, *filters):
        x = _f32c(x)
        _dev(x)
        M, D = x.shape
        F = M // B
        assert F * B == M and F >= 1
        lib = _lib.lib()
        Ntot = sum(W.data.shape[1] for W in filters)
        out = torch.empty((B, Ntot), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, Ntot), dtype=torch.int32, device=x.device)
        k0 = c0 = 0
        for n in ([len(filters)] if CNN_POOL_WHOLE_CHAIN else sizes):
            y = _cnn_tm_dense(x, B, filters[k0:k0 + n])
            N = y.shape[1]
            _lib.check(lib.yt8m_timepool_max_f32(_p(y), F, B, N, N, ctypes.c_void_p(out.data_ptr() + c0 * 4),
                                                 ctypes.c_void_p(idx.data_ptr() + c0 * 4), Ntot, _stream()))
            k0 += n
            c0 += N
        ctx.save_for_backward(x, idx)
        ctx.filters, ctx.B = filters, B
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, g, _):
        x, idx = ctx.saved_tensors
        filters, B = ctx.filters, ctx.B
        M, D = x.shape
        F = M // B
        g = _f32c(g)
        Ntot = g.shape[1]
        lib = _lib.lib()
        c0 = 0
        for W in filters:
            fs, N = W.data.shape[0] // D, W.data.shape[1]
            if W.trainable and W.grad is not None:
                wbeta = float(W.grad_beta())
                _lib.check(lib.yt8m_f32_cnn_pool_dw(_p(x), D, ctypes.c_void_p(idx.data_ptr() + c0 * 4), ctypes.c_void_p(g.data_ptr() + c0 * 4),
                                                    Ntot, B, F, D, N, fs, _p(W.grad), N, wbeta, _stream()))
            c0 += N
        dx = None
        if ctx.needs_input_grad[0]:
            n = len(filters)
            wts = [W.data.t().contiguous() for W in filters]          # [N_k, fs_k D]: a term's walk over d is contiguous (layout glue)
            wt = (ctypes.c_void_p * n)(*[t.data_ptr() for t in wts])
            fs = (ctypes.c_int32 * n)(*[W.data.shape[0] // D for W in filters])
            nc = (ctypes.c_int32 * n)(*[W.data.shape[1] for W in filters])
            dx = torch.empty_like(x)
            _lib.check(lib.yt8m_f32_cnn_pool_dx(_p(idx), _p(g), Ntot, B, F, D, n, wt, fs, nc, _p(dx), D, _stream()))
        for W in filters:                                              # (after dx has read the filters: a finished gradient may be consumed)
            if W.trainable and W.grad is not None:
                W.grad_done()
        return (dx, None, None, None) + (None,) * len(filters)


def cnn_tm_maxpool(x_tm2d, B, cnns, want_idx=False):
    """x_tm2d [F B, D] float time-major (B videos per frame, padding rows zeros: no num_frames here); cnns: one list of cnn-filter
    Variables [fs_k D, N_k] per CNN of a chain, all reading x -> [reduce_max over the F frames of that CNN's output [B, sum N_k]] per CNN
    (and, want_idx, the frames [B, sum over the chain] int32 the maxima were taken from)."""
    filters = [W for cnn in cnns for W in cnn]
    assert cnn_tm_maxpool_supported(x_tm2d.shape[1], cnns), "cnn_tm_maxpool: filter columns in multiples of 4, D % 4 == 0, D <= 2048"
    out, idx = _PooledCnnChainTM.apply(x_tm2d, _token(filters[0]._graph), int(B), tuple(len(c) for c in cnns), *filters)
    pooled = list(torch.split(out, [sum(W.data.shape[1] for W in cnn) for cnn in cnns], dim=1))
    return (pooled, idx) if want_idx else pooled


_MS_WS = {}


def _multiscale_ws(dev, C):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, int(C))
    ws = _MS_WS.get(key)
    if ws is None:
        ws = torch.empty(_lib.lib().yt8m_multiscale_workspace_bytes(int(C)) // 4, dtype=torch.float32, device=dev)
        _MS_WS[key] = ws
    return ws


class _BnReluPool2TM(torch.autograd.Function):
    """slim.batch_norm(center, scale) over all F B rows, ReLU, and the max over frame pairs (2j, 2j + 1) of
    W/all_frame_models/multiscale_cnn_lstm_model.py:39-45,116,123-127 in ONE pass over the CNN output y [F B, C] (time-major):
    a [F,B,C] is the LSTM's input as it stands, p [F // 2, B, C] the next scale's (csrc/multiscale.hip).  Backward recomputes a and xhat
    from y: nothing but y, the column statistics and the two outputs is kept."""

    @staticmethod
    def forward(ctx, y, token, gamma, beta, mm, mv, is_training, eps, decay, F, B, want_pool):
        y = _f32c(y)
        _dev(y)
        M, C = y.shape
        assert M == F * B
        dev = y.device
        lib = _lib.lib()
        ws = _multiscale_ws(dev, C)
        mean = torch.empty((C,), dtype=torch.float32, device=dev)
        rstd = torch.empty((C,), dtype=torch.float32, device=dev)
        _lib.check(lib.yt8m_colmoments_f32(_p(y), M, C, C, _p(mm.data), _p(mv.data), int(bool(is_training)), float(eps), float(decay),
                                           _p(mean), _p(rstd), _p(ws), ws.numel() * 4, _stream()))
        a = torch.empty((F, B, C), dtype=torch.float32, device=dev)
        p = torch.empty((F // 2, B, C), dtype=torch.float32, device=dev) if want_pool else None
        _lib.check(lib.yt8m_bn_relu_pool2_tm_fwd(_p(y), C, F, B, C, _p(gamma.data), _p(beta.data), _p(mean), _p(rstd), _p(a), C,
                                                 _p(p) if (p is not None and p.numel()) else None, C, _stream()))
        ctx.save_for_backward(y, mean, rstd)
        ctx.vars = (gamma, beta, bool(is_training), F, B)
        if p is None:
            p = a.new_empty((0,))
            ctx.mark_non_differentiable(p)
        return a, p

    @staticmethod
    def backward(ctx, da, dp):
        y, mean, rstd = ctx.saved_tensors
        gamma, beta, is_training, F, B = ctx.vars
        M, C = y.shape
        lib = _lib.lib()
        da = _f32c(da) if da is not None else None
        dp = _f32c(dp) if (dp is not None and dp.numel()) else None
        gg, gb = gamma.grad, beta.grad
        if da is None and dp is None:
            da = torch.zeros((F, B, C), dtype=torch.float32, device=y.device)
        ws = _multiscale_ws(y.device, C)
        dy = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        bg = gamma.grad_beta() if gg is not None else 0.0
        bb = beta.grad_beta() if gb is not None else 0.0
        _lib.check(lib.yt8m_bn_relu_pool2_tm_bwd(_p(y), C, F, B, C, _p(gamma.data), _p(beta.data), _p(mean), _p(rstd), int(is_training),
                                                 _p(da), C, _p(dp), C, _p(dy), C, _p(gg), float(bg), _p(gb), float(bb), _p(ws),
                                                 ws.numel() * 4, _stream()))
        if gg is not None:
            gamma.grad_done()
        if gb is not None:
            beta.grad_done()
        return (dy,) + (None,) * 11


def bn_relu_pool2_tm(y, gamma, beta, moving_mean, moving_variance, is_training, F, B, want_pool=True, eps=1e-3, decay=0.999):
    """y [F B, C] time-major -> (a [F,B,C], p [F // 2, B, C] or None)."""
    a, p = _BnReluPool2TM.apply(y, _token(gamma._graph), gamma, beta, moving_mean, moving_variance, bool(is_training), float(eps),
                                float(decay), int(F), int(B), bool(want_pool))
    return a, (p if want_pool else None)


# ---- DeepCnnDeepCombineChainModel: max over all frames (classifier) + max over frame pairs (next level) of a CNN level's output --------
# Which form max_pool2_tm takes on the device, read at call time: the one-pass kernels of csrc/deep_cnn.hip, or the composed form
# (yt8m_timepool_max_f32 + a pair maximum from torch ops).  The default follows DESIGN_LOG.md section 23's rule on tools/deepcnn_step.py's
# op leg (section 28 has the rows).
DEEP_CNN_FUSED_DEFAULT = "1"


def deep_cnn_fused():
    return os.environ.get("YT8M_DEEP_CNN_FUSED", DEEP_CNN_FUSED_DEFAULT) != "0"


def max_pool2_tm_supported(y, C):
    """The one-pass kernels (csrc/deep_cnn.hip): a device tensor and C % 4 == 0 (16-byte column accesses)."""
    return bool(y.is_cuda and C % 4 == 0 and C >= 4)


def _max_pool2_kernel_ok(y, F, B, C):
    return max_pool2_tm_supported(y, C) and y.dtype == torch.float32 and 1 <= B < 65536 and F >= 1 and F * B < (1 << 31) - 64


class _MaxPool2TM(torch.autograd.Function):
    """tf.reduce_max over all frames and tf.nn.pool(MAX, window 2, stride 2, VALID) of
    W/all_frame_models/deep_cnn_deep_combine_chain_model.py:59-61,93 in ONE pass over a CNN level's output y [F B, C] (time-major), and
    ONE backward pass that writes dy (csrc/deep_cnn.hip).  Keeps y (the CNN's output, alive anyway) and the frames of the maxima."""

    @staticmethod
    def forward(ctx, y, F, B, want_pool):
        y = _f32c(y)
        _dev(y)
        M, C = y.shape
        assert M == F * B
        dev = y.device
        m = torch.empty((B, C), dtype=torch.float32, device=dev)
        idx = torch.empty((B, C), dtype=torch.int32, device=dev)
        p = torch.empty((F // 2, B, C), dtype=torch.float32, device=dev) if want_pool else None
        _lib.check(_lib.lib().yt8m_timepool_max_pool2_f32_fwd(_p(y), C, F, B, C, _p(m), _p(idx), C,
                                                              _p(p) if (p is not None and p.numel()) else None, C, _stream()))
        ctx.save_for_backward(y, idx)
        ctx.dims = (F, B)
        if p is None:
            p = y.new_empty((0,))
            ctx.mark_non_differentiable(p)
        ctx.mark_non_differentiable(idx)
        return m, p, idx

    @staticmethod
    def backward(ctx, g, dp, _):
        y, idx = ctx.saved_tensors
        F, B = ctx.dims
        C = y.shape[1]
        g = _f32c(g) if g is not None else None
        dp = _f32c(dp) if (dp is not None and dp.numel()) else None
        dy = torch.empty_like(y)
        _lib.check(_lib.lib().yt8m_timepool_max_pool2_f32_bwd(_p(y), C, F, B, C, _p(g), _p(idx), C, _p(dp), C, _p(dy), C, _stream()))
        return dy, None, None, None


class _TimepoolMaxTM(torch.autograd.Function):
    """The composed form's maximum over all frames on the device: yt8m_timepool_max_f32 with the frames kept; backward a zero-fill and a
    scatter of g to them."""

    @staticmethod
    def forward(ctx, y, F, B):
        y = _f32c(y)
        _dev(y)
        C = y.shape[1]
        m = torch.empty((B, C), dtype=torch.float32, device=y.device)
        idx = torch.empty((B, C), dtype=torch.int32, device=y.device)
        _lib.check(_lib.lib().yt8m_timepool_max_f32(_p(y), F, B, C, C, _p(m), _p(idx), C, _stream()))
        ctx.save_for_backward(idx)
        ctx.dims = (F, B, C)
        ctx.mark_non_differentiable(idx)
        return m, idx

    @staticmethod
    def backward(ctx, g, _):
        (idx,) = ctx.saved_tensors
        F, B, C = ctx.dims
        dy = torch.zeros((F, B, C), dtype=torch.float32, device=g.device)
        dy.scatter_(0, idx.to(torch.int64)[None], _f32c(g)[None])
        return dy.view(F * B, C), None, None


def _pair_max(y3):
    """max(y[2j], y[2j + 1]) [F // 2, B, C] from torch ops, the first frame taking a tie in the gradient (the kernel's rule; amax would
    split it)."""
    F = y3.shape[0]
    pairs = y3[:2 * (F // 2)].reshape(F // 2, 2, y3.shape[1], y3.shape[2])
    y0, y1 = pairs[:, 0], pairs[:, 1]
    return torch.where(y0 >= y1, y0, y1)


def max_pool2_tm(y, F, B, want_pool=True):
    """y [F B, C] time-major (row t B + b) -> (m [B, C] = max over the F frames, p [F // 2, B, C] = max over the frame pairs (2j, 2j + 1),
    an odd last frame dropped; None unless want_pool).  On the device the one-pass kernels of csrc/deep_cnn.hip unless
    YT8M_DEEP_CNN_FUSED=0 or they refuse the shape; then, and for every CPU tensor, the composed form: yt8m_timepool_max_f32 (amax off the
    device) plus a pair maximum from torch ops."""
    M, C = y.shape
    assert M == F * B and F >= 1, "max_pool2_tm: y must be [F B, C]"
    if deep_cnn_fused() and _max_pool2_kernel_ok(y, F, B, C):
        m, p, _ = _MaxPool2TM.apply(y, int(F), int(B), bool(want_pool))
        return m, (p if want_pool else None)
    if max_pool2_tm_supported(y, C) and y.dtype == torch.float32:       # (yt8m_timepool_max_f32 wants C % 4 == 0 too)
        m, _ = _TimepoolMaxTM.apply(y, int(F), int(B))
    else:
        m = y.view(F, B, C).amax(dim=0)
    return m, (_pair_max(y.view(F, B, C)) if want_pool else None)


# ---- sigmoid attention pooling over time-major rows (W/all_frame_models/lstm_attention_model.py:61-73; csrc/sigmoid_attention.hip) ---
# The default form follows the project's rule: the kernels only if their median is the lower one at every shape of
# tools/sigmoid_attention_step.py in both runs (DESIGN_LOG.md 33).  1: the kernels where the shape is supported; 0: the composed form.
SIGMOID_ATTENTION_FUSED = os.environ.get("YT8M_SIGMOID_ATTENTION_FUSED", "1") != "0"
SIGMOID_ATTENTION_CALLS = {"kernels": 0, "composed": 0}      # which form ran (tests assert that the kernels engaged)
_SIGATTN_EPS = 1e-8


def _is_variable(v):
    return hasattr(v, "_graph") and not torch.is_tensor(v)


def _attention_fc(src_tm, W, b):
    """The composed attention forms' FC on the [F B, Hs] view of src_tm: ops.linear on the device when W, b are Variables, else a plain
    product with their tensors.  Returns [F B, heads]."""
    F, B, Hs = src_tm.shape
    if _is_variable(W) and src_tm.is_cuda:
        return ops.linear(src_tm.reshape(F * B, Hs), W, b)
    Wt, bt = (ops.as_tensor(v) if _is_variable(v) else v for v in (W, b))
    return src_tm.reshape(F * B, Hs) @ Wt + bt


def _attention_ws(nbytes, dev):
    """The workspace of an attention kernel call: nbytes as float32 elements, never empty."""
    return torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=dev)


def sigmoid_attention_composed(src_tm, Wa, ba, num_frames, values_tm=None):
    """sigmoid_attention from existing ops, as the reference writes it, in the dtype of its operands: the FC on the [F B, Hs] view
    (ops.linear on the device when Wa, ba are Variables, else a plain product), torch sigmoid / mask / sum / divide, and pool_tn on a
    batch-major copy of the values (an einsum off the device)."""
    SIGMOID_ATTENTION_CALLS["composed"] += 1
    F, B = src_tm.shape[:2]
    z = _attention_fc(src_tm, Wa, ba)
    A = z.shape[1]
    n = num_frames.to(src_tm.device).to(torch.int64).clamp(0, F)
    mask = (torch.arange(F, device=src_tm.device)[:, None] < n[None, :]).to(z.dtype)              # [F,B]
    s = torch.sigmoid(z).view(F, B, A) * mask[:, :, None]
    att = (s / (s.sum(dim=0, keepdim=True) + _SIGATTN_EPS)).permute(1, 0, 2).contiguous()         # [B,F,A]
    if values_tm is None:
        return att, None
    if values_tm.is_cuda and values_tm.dtype == torch.float32:
        return att, pool_tn(att, values_tm.transpose(0, 1).contiguous())
    return att, torch.einsum("bfa,fbh->bah", att, values_tm)


def _rows_tm(t):
    """A [F,B,H] float32 tensor as the kernels read it: (tensor, row stride in floats); rows (t, b) at (t B + b) ld."""
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    B = t.shape[1]
    if t.shape[2] > 0 and not (t.stride(2) == 1 and t.stride(0) == B * t.stride(1) and t.stride(1) >= t.shape[2]):
        t = t.contiguous()
    return t, t.stride(1)


class _SigmoidAttention(torch.autograd.Function):
    """yt8m_sigattn_fwd / _bwd under autograd: gradients to src_tm, Wa, ba and values_tm, from the gradient of att and / or of pooled."""

    @staticmethod
    def forward(ctx, src_tm, Wa, ba, num_frames, values_tm):
        src, ld_src = _rows_tm(src_tm)
        _dev(src, Wa, ba, values_tm)
        F, B, Hs = src.shape
        A = Wa.shape[1]
        assert tuple(Wa.shape) == (Hs, A) and ba.numel() == A, "sigmoid attention operands: Wa [Hs,A], ba [A]"
        Wa, ba = _f32c(Wa.detach()), _f32c(ba.detach().view(-1))
        vals, ld_vals, Hv = None, 0, 0
        if values_tm is not None:
            assert tuple(values_tm.shape[:2]) == (F, B), "values_tm must be [F,B,Hv] like src_tm"
            vals, ld_vals = _rows_tm(values_tm)
            Hv = vals.shape[2]
        dev = src.device
        lib = _lib.lib()
        nf = _nf(num_frames)
        att = torch.empty((B, F, A), dtype=torch.float32, device=dev)
        den = torch.empty((B, A), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, A, Hv), dtype=torch.float32, device=dev) if Hv else None
        nbytes = int(lib.yt8m_sigattn_workspace_bytes(B, F, Hs, Hv, A))
        ws = _attention_ws(nbytes, dev)
        _lib.check(lib.yt8m_sigattn_fwd(_p(src), ld_src, _p(vals), ld_vals, _p(Wa), _p(ba), _p(nf), _p(att), _p(den), _p(pooled), _p(ws),
                                        nbytes, B, F, Hs, Hv, A, _stream()))
        SIGMOID_ATTENTION_CALLS["kernels"] += 1
        ctx.save_for_backward(src, vals, Wa, att, den, pooled)
        ctx.nf, ctx.nbytes = nf, nbytes
        ctx.set_materialize_grads(False)
        return att, pooled

    @staticmethod
    def backward(ctx, datt, dpooled):
        src, vals, Wa, att, den, pooled = ctx.saved_tensors
        if datt is None and dpooled is None:
            return None, None, None, None, None
        F, B, Hs = src.shape
        A = Wa.shape[1]
        Hv = vals.shape[2] if vals is not None else 0
        dev = src.device
        E = None if datt is None else _f32c(datt)
        G = None if dpooled is None else _f32c(dpooled)
        need = ctx.needs_input_grad
        dsrc = torch.empty((F, B, Hs), dtype=torch.float32, device=dev)
        dvals = torch.empty((F, B, Hv), dtype=torch.float32, device=dev) if (vals is not None and need[4]) else None
        dWa = torch.empty((Hs, A), dtype=torch.float32, device=dev) if need[1] else None
        dba = torch.empty((A,), dtype=torch.float32, device=dev) if need[2] else None
        ld_src, ld_vals = src.stride(1), (vals.stride(1) if vals is not None else 0)
        ws = _attention_ws(ctx.nbytes, dev)
        _lib.check(_lib.lib().yt8m_sigattn_bwd(_p(src), ld_src, _p(vals), ld_vals, _p(Wa), _p(ctx.nf), _p(att), _p(den), _p(pooled), _p(G),
                                               _p(E), _p(dsrc), Hs, _p(dvals), Hv, _p(dWa), _p(dba), _p(ws), ctx.nbytes, B, F, Hs, Hv, A,
                                               _stream()))
        return (dsrc if need[0] else None), dWa, dba, None, dvals


def sigmoid_attention_supported(src_tm, A, values_tm=None):
    """Whether sigmoid_attention runs these operands on the kernels of csrc/sigmoid_attention.hip."""
    if not SIGMOID_ATTENTION_FUSED or not (torch.is_tensor(src_tm) and src_tm.is_cuda and src_tm.dtype == torch.float32 and src_tm.dim() == 3):
        return False
    Hv = 0
    if values_tm is not None:
        if not (values_tm.is_cuda and values_tm.dtype == torch.float32 and tuple(values_tm.shape[:2]) == tuple(src_tm.shape[:2])):
            return False
        Hv = values_tm.shape[2]
        if Hv == 0:
            return False
    F, B, Hs = src_tm.shape
    return bool(_lib.lib().yt8m_sigattn_supported(int(B), int(F), int(Hs), int(Hv), int(A)))


def sigmoid_attention(src_tm, Wa, ba, num_frames, values_tm=None):
    """The sigmoid attention pooling of W/all_frame_models/lstm_attention_model.py:61-73, lstm_attention_lstm_model.py:78-92 and
    lstm_multi_attention_model.py:63-78 on TIME-major operands, m[t,b] = 1 for t < clamp(num_frames[b], 0, F):
        s = sigmoid(src_tm . Wa + ba) m;   att[b,t,a] = s[t,b,a] / (sum_t s + 1e-8);   pooled[b,a,:] = sum_t att[b,t,a] values_tm[t,b,:]
    src_tm [F,B,Hs] (an LSTM stack's outputs), Wa [Hs,A] and ba [A] (Variables, or tensors under autograd), values_tm [F,B,Hv] or None.
    Returns (att [B,F,A] -- the layout pool_tn / pool_tn_u8 read -- and pooled [B,A,Hv], None without values).  A video with
    num_frames = 0 gets att = 0 and pooled = 0 and receives no gradient.  The reference's mask_emb lookup table is this mask.
    Device tensors at shapes yt8m_sigattn_supported takes run on the kernels (one pass over src_tm and values_tm each way, no batch-major
    copy); CPU tensors, other shapes and YT8M_SIGMOID_ATTENTION_FUSED=0 take sigmoid_attention_composed, which computes the same
    function."""
    A = (Wa.data if _is_variable(Wa) else Wa).shape[1]
    if sigmoid_attention_supported(src_tm, A, values_tm):
        Wt, bt = (ops.as_tensor(v) if _is_variable(v) else v for v in (Wa, ba))
        return _SigmoidAttention.apply(src_tm, Wt, bt, num_frames, values_tm)
    return sigmoid_attention_composed(src_tm, Wa, ba, num_frames, values_tm)


# ---- windowed softmax attention pooling over time-major rows (Z/frame_level_models.py:5218-5223, :6059-6064; csrc/softmax_attention.hip)
# The default form follows the project's rule: the kernels only if their median is the lower one at every shape of
# tools/extend_attention_step.py in both runs (DESIGN_LOG.md 34).  1: the kernels where the shape is supported; 0: the composed form.
SOFTMAX_ATTENTION_FUSED = os.environ.get("YT8M_SOFTMAX_ATTENTION_FUSED", "1") != "0"
SOFTMAX_ATTENTION_CALLS = {"kernels": 0, "composed": 0}      # which form ran (tests assert that the kernels engaged)


def softmax_attention_mask(F, B, E, valid=None, lo=None, hi=None, device=None):
    """m [B,F,E] bool: valid[b,t] != 0 and lo[b,e] <= t <= hi[b,e] (inclusive; an absent operand does not restrict)."""
    m = torch.ones((B, F, E), dtype=torch.bool, device=device)
    t = torch.arange(F, device=device).view(1, F, 1)
    if lo is not None:
        m = m & (t >= lo.to(device).to(torch.int64).view(B, 1, E))
    if hi is not None:
        m = m & (t <= hi.to(device).to(torch.int64).view(B, 1, E))
    if valid is not None:
        m = m & (valid.to(device).view(B, F, 1) != 0)
    return m


def softmax_attention_tm_composed(src_tm, W1, b1, values_tm, extra=None, valid=None, lo=None, hi=None):
    """softmax_attention_tm from existing ops, in the dtype of its operands: the FC on the [F B, Hs] view (ops.linear on the device when
    W1, b1 are Variables, else a plain product), a masked softmax over the frames in torch (max over the unmasked frames, so finite
    where the reference's softmax-times-mask underflows), and pool_tn on a batch-major copy of the values (an einsum off the device).
    A (b, e) without an unmasked frame gets att = 0 and pooled = 0 and neither receives nor sends a gradient; att is detached."""
    SOFTMAX_ATTENTION_CALLS["composed"] += 1
    F, B = src_tm.shape[:2]
    z = _attention_fc(src_tm, W1, b1)
    E = z.shape[1]
    z = z.view(F, B, E).permute(1, 0, 2)                                                          # [B,F,E]
    if extra is not None:
        z = z + extra
    m = softmax_attention_mask(F, B, E, valid, lo, hi, src_tm.device)
    zm = z.masked_fill(~m, float("-inf"))
    M = zm.detach().amax(dim=1, keepdim=True)
    p = torch.exp(zm - torch.where(torch.isfinite(M), M, torch.zeros_like(M)))                    # 0 on the masked frames
    L = p.sum(dim=1, keepdim=True)
    att = (p / torch.where(L > 0, L, torch.ones_like(L))).contiguous()                            # [B,F,E]
    if values_tm.is_cuda and values_tm.dtype == torch.float32:
        pooled = pool_tn(att, values_tm.transpose(0, 1).contiguous())
    else:
        pooled = torch.einsum("bfe,fbh->beh", att, values_tm)
    return att.detach(), pooled


class _SoftmaxAttentionTM(torch.autograd.Function):
    """yt8m_smattn_fwd / _bwd under autograd: gradients to src_tm, W1, b1, values_tm and extra from the gradient of pooled; att is not
    differentiable.  values_tm None is the shared mode (the values ARE src_tm): src_tm then receives the one sum of both gradients."""

    @staticmethod
    def forward(ctx, src_tm, W1, b1, values_tm, extra, valid, lo, hi):
        src, ld_src = _rows_tm(src_tm)
        _dev(src, W1, b1, values_tm, extra)
        F, B, Hs = src.shape
        E = W1.shape[1]
        assert tuple(W1.shape) == (Hs, E) and b1.numel() == E, "softmax attention operands: W1 [Hs,E], b1 [E]"
        W1, b1 = _f32c(W1.detach()), _f32c(b1.detach().view(-1))
        shared = values_tm is None
        if shared:
            vals, ld_vals = src, ld_src
        else:
            assert tuple(values_tm.shape[:2]) == (F, B), "values_tm must be [F,B,Hv] like src_tm"
            vals, ld_vals = _rows_tm(values_tm)
        Hv = vals.shape[2]
        dev = src.device
        if extra is not None:
            assert tuple(extra.shape) == (B, F, E), "extra must be [B,F,E]"
            extra = _f32c(extra.detach())
        valid = None if valid is None else valid.to(device=dev, dtype=torch.uint8).contiguous().view(B, F)
        lo, hi = (None if w is None else w.to(device=dev, dtype=torch.int32).contiguous().view(B, E) for w in (lo, hi))
        lib = _lib.lib()
        att = torch.empty((B, F, E), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, E, Hv), dtype=torch.float32, device=dev)
        nbytes = int(lib.yt8m_smattn_workspace_bytes(B, F, Hs, Hv, E))
        ws = _attention_ws(nbytes, dev)
        _lib.check(lib.yt8m_smattn_fwd(_p(src), ld_src, _p(vals), ld_vals, _p(W1), _p(b1), _p(extra), _p(valid), _p(lo), _p(hi), _p(att),
                                       _p(pooled), _p(ws), nbytes, B, F, Hs, Hv, E, _stream()))
        SOFTMAX_ATTENTION_CALLS["kernels"] += 1
        ctx.save_for_backward(src, None if shared else vals, W1, att, pooled)
        ctx.masks, ctx.nbytes, ctx.has_extra = (valid, lo, hi), nbytes, extra is not None
        ctx.mark_non_differentiable(att)
        ctx.set_materialize_grads(False)
        return att, pooled

    @staticmethod
    def backward(ctx, _datt, dpooled):
        src, vals, W1, att, pooled = ctx.saved_tensors
        if dpooled is None:
            return (None,) * 8
        shared = vals is None
        F, B, Hs = src.shape
        E = W1.shape[1]
        Hv = Hs if shared else vals.shape[2]
        dev = src.device
        G = _f32c(dpooled)
        need = ctx.needs_input_grad
        valid, lo, hi = ctx.masks
        dsrc = torch.empty((F, B, Hs), dtype=torch.float32, device=dev)
        dvals = torch.empty((F, B, Hv), dtype=torch.float32, device=dev) if (not shared and need[3]) else None
        dW1 = torch.empty((Hs, E), dtype=torch.float32, device=dev) if need[1] else None
        db1 = torch.empty((E,), dtype=torch.float32, device=dev) if need[2] else None
        dextra = torch.empty((B, F, E), dtype=torch.float32, device=dev) if (ctx.has_extra and need[4]) else None
        ld_src = src.stride(1)
        v, ld_vals = (src, ld_src) if shared else (vals, vals.stride(1))
        ws = _attention_ws(ctx.nbytes, dev)
        _lib.check(_lib.lib().yt8m_smattn_bwd(_p(src), ld_src, _p(v), ld_vals, _p(W1), _p(valid), _p(lo), _p(hi), _p(att), _p(pooled), _p(G),
                                              _p(dsrc), Hs, _p(dvals), Hv, _p(dW1), _p(db1), _p(dextra), _p(ws), ctx.nbytes, B, F, Hs, Hv, E,
                                              _stream()))
        return (dsrc if need[0] else None), dW1, db1, dvals, dextra, None, None, None


def softmax_attention_tm_supported(src_tm, E, values_tm, extra=None):
    """Whether softmax_attention_tm runs these operands on the kernels of csrc/softmax_attention.hip."""
    ok = lambda t: torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
    if not SOFTMAX_ATTENTION_FUSED or not (ok(src_tm) and src_tm.dim() == 3 and ok(values_tm) and values_tm.dim() == 3):
        return False
    if tuple(values_tm.shape[:2]) != tuple(src_tm.shape[:2]):
        return False
    F, B, Hs = src_tm.shape
    if extra is not None and not (ok(extra) and tuple(extra.shape) == (B, F, E)):
        return False
    return bool(_lib.lib().yt8m_smattn_supported(int(B), int(F), int(Hs), int(values_tm.shape[2]), int(E)))


def softmax_attention_tm(src_tm, W1, b1, values_tm, extra=None, valid=None, lo=None, hi=None):
    """The windowed softmax attention pooling of Z/frame_level_models.py:5218-5223 (LstmExtendModel) and :6059-6064 (InputExtendModel)
    on TIME-major operands, per head e of E:
        z[t,b,e] = src_tm[t,b,:] . W1[:,e] + b1[e] + extra[b,t,e];   m[t,b,e] = valid[b,t] (lo[b,e] <= t <= hi[b,e])
        att[b,t,e] = m exp(z - M) / sum_t' m exp(z[t'] - M),  M[b,e] = max of z over the frames with m = 1
        pooled[b,e,:] = sum_t att[b,t,e] values_tm[t,b,:]
    src_tm [F,B,Hs] and values_tm [F,B,Hv] (LSTM stacks' outputs), W1 [Hs,E] and b1 [E] (Variables, or tensors under autograd), extra
    [B,F,E] (batch-major, what attention_logits_u8 writes) or None, valid [B,F] (any non-zero is 1) or None = all ones, lo / hi [B,E]
    integers, inclusive, or None = 0 / F - 1.  Returns (att [B,F,E], detached: it is for "attention_weight" and carries no gradient, and
    pooled [B,E,Hv]).  The reference writes softmax over all F frames, times the mask, divided by its sum: the same function.  A (b, e)
    without an unmasked frame is NaN there; here it gets att = 0 and pooled = 0 and neither receives nor sends a gradient (the
    convention of sigmoid_attention).
    values_tm IS src_tm (the same tensor object) is the shared mode: the rows are read once for the logits and the pooling, and src_tm
    receives ONE gradient tensor holding the sum of both.  Device tensors at shapes yt8m_smattn_supported takes run on the kernels (no
    batch-major copy); CPU tensors, other shapes and YT8M_SOFTMAX_ATTENTION_FUSED=0 take softmax_attention_tm_composed, which computes
    the same function."""
    E = (W1.data if _is_variable(W1) else W1).shape[1]
    if softmax_attention_tm_supported(src_tm, E, values_tm, extra):
        Wt, bt = (ops.as_tensor(v) if _is_variable(v) else v for v in (W1, b1))
        return _SoftmaxAttentionTM.apply(src_tm, Wt, bt, None if values_tm is src_tm else values_tm, extra, valid, lo, hi)
    return softmax_attention_tm_composed(src_tm, W1, b1, values_tm, extra, valid, lo, hi)
