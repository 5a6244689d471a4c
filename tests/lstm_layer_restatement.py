"""Restatement of LstmLayerModel (Z/frame_level_models.py:3629-3683, Z = youtube-8m-zhangteng of the reference) in plain torch, in a given
dtype (float64 for the reference values, float32 for the error bound):
    clips    x [B,F,D] -> [B U2, U1, D], U2 = F // U1, frames at or past U1 U2 dropped, frames at or past num_frames zero vectors
    RNN-1    BasicLSTMCell(H, forget_bias=1.0) over all B U2 clips for U1 steps from zero state, no lengths:
             i|j|f|o = [x_t, h] . W + b,  c = c sigmoid(f + 1) + sigmoid(i) tanh(j),  h = tanh(c) sigmoid(o)
    RNN-2    the same cell with its own Variables over the clip memories [B, U2, H] with sequence_length = num_frames // U1
             (dynamic_rnn's copy-through: a row past its length keeps its state)
    head     MoeModel on the final memory of RNN-2 [B, H].
Shared by tests/test_lstm_layer_host.py and tests/test_gpu_lstm_layer.py; not a test module."""
import numpy as np
import torch

from gate_lstm_restatement import bounds, cross_entropy, err, moe  # noqa: F401  (the fp64 tests' measure and the head, shared)

U8_A0, U8_C0 = 4.0 / 255.0, 4.0 / 512.0 - 2.0          # utils.Dequantize of the reader's bytes


def frames_from_bytes(q, num_frames, dtype):
    """The reader's bytes [B,F,D] -> dequantised, l2-normalised frames with the padding frames zero, in `dtype`."""
    x = torch.from_numpy(np.asarray(q)).to(dtype) * U8_A0 + U8_C0
    x = x / torch.sqrt(torch.clamp((x * x).sum(dim=2, keepdim=True), min=1e-12))
    return mask_frames(x, num_frames)


def mask_frames(x, num_frames):
    nf = torch.as_tensor(np.asarray(num_frames))
    live = (torch.arange(x.shape[1])[None, :] < nf[:, None]).to(x.dtype)
    return x * live[:, :, None]


def cell(x, h, c, W, b, forget_bias=1.0):
    H = W.shape[1] // 4
    i, j, f, o = (torch.cat([x, h], dim=1) @ W + b).split(H, dim=1)
    c = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
    return torch.tanh(c) * torch.sigmoid(o), c


def clip_recurrence(x, num_frames, clip, W, b):
    """x [B,F,D] float frames (masked here) -> the clips' final memories, time-major [U2, B, H]."""
    B, F, D = x.shape
    U2, H = F // clip, W.shape[1] // 4
    xc = mask_frames(x, num_frames)[:, :clip * U2].reshape(B * U2, clip, D)
    h = c = torch.zeros((B * U2, H), dtype=x.dtype)
    for t in range(clip):
        h, c = cell(xc[:, t], h, c, W, b)
    return c.view(B, U2, H).transpose(0, 1)


def clip_with_grads(x, num_frames, clip, W, b, dout, dtype):
    """The clip recurrence in `dtype` on numpy operands: out [U2,B,H] and dW, db for the loss sum(out * dout)."""
    Wt = torch.from_numpy(np.asarray(W)).to(dtype).clone().requires_grad_(True)
    bt = torch.from_numpy(np.asarray(b)).to(dtype).clone().requires_grad_(True)
    xt = x.to(dtype) if torch.is_tensor(x) else torch.from_numpy(np.asarray(x)).to(dtype)
    out = clip_recurrence(xt, num_frames, clip, Wt, bt)
    (out * torch.from_numpy(np.asarray(dout)).to(dtype)).sum().backward()
    return {"out": out.detach().numpy(), "dW": Wt.grad.numpy(), "db": bt.grad.numpy()}


def steps(z, Wh, forget_bias, dtype):
    """The recurrence on GIVEN hoisted inputs (what the C ABI takes): z [T,B,4H] = x_t . W_x + b, Wh [H,4H] -> the activated gates
    [T,B,4H] and cs, hs [T + 1, B, H] from zero state, as numpy in `dtype`."""
    z = torch.from_numpy(np.asarray(z)).to(dtype)
    Wh = torch.from_numpy(np.asarray(Wh)).to(dtype)
    T, B, H4 = z.shape
    H = H4 // 4
    h = c = torch.zeros((B, H), dtype=dtype)
    gates, cs, hs = [], [c], [h]
    for t in range(T):
        i, j, f, o = (z[t] + h @ Wh).split(H, dim=1)
        i, j, f, o = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + forget_bias), torch.sigmoid(o)
        c = c * f + i * j
        h = torch.tanh(c) * o
        gates.append(torch.cat([i, j, f, o], dim=1))
        cs.append(c)
        hs.append(h)
    return {"gates": torch.stack(gates).numpy(), "cs": torch.stack(cs).numpy(), "hs": torch.stack(hs).numpy()}


def second_lstm(state_c_tm, lengths, W, b):
    """dynamic_rnn of the cell over state_c_tm [U2,B,H] with sequence_length = lengths -> the final memory [B,H]."""
    U2, B, H = state_c_tm.shape
    n = torch.as_tensor(np.asarray(lengths))
    h = c = torch.zeros((B, H), dtype=state_c_tm.dtype)
    for t in range(U2):
        h2, c2 = cell(state_c_tm[t], h, c, W, b)
        live = (t < n).to(state_c_tm.dtype)[:, None]
        h, c = live * h2 + (1 - live) * h, live * c2 + (1 - live) * c
    return c


def model(x, num_frames, clip, P, M):
    """The whole model on float frames x [B,F,D]; P: the seven Variables by name (torch, one dtype) -> (predictions, state_out)."""
    cellname = "%s/multi_rnn_cell/cell_0/basic_lstm_cell/%s"
    state_c = clip_recurrence(x, num_frames, clip, P[cellname % ("RNN-1", "weights")], P[cellname % ("RNN-1", "biases")])
    lengths = torch.as_tensor(np.asarray(num_frames)) // clip
    state_out = second_lstm(state_c, lengths, P[cellname % ("RNN-2", "weights")], P[cellname % ("RNN-2", "biases")])
    return moe(state_out, P["gates/weights"], P["experts/weights"], P["experts/biases"], M), state_out


def model_with_grads(x, num_frames, clip, P, labels, M, dtype):
    """predictions, loss (cross entropy) and every Variable's gradient of the loss, as numpy, computed in `dtype`."""
    Pt = {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    p, _ = model(x.to(dtype), num_frames, clip, Pt, M)
    loss = cross_entropy(p, torch.from_numpy(np.asarray(labels)))
    loss.backward()
    res = {"predictions": p.detach().numpy(), "loss": np.asarray(float(loss.detach()))}
    res.update({"d:" + k: v.grad.numpy() for k, v in Pt.items()})
    return res
