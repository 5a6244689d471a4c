"""Restatement of the Extend attention models, their heads and their pooling in plain torch, in the dtype of its inputs (float64 for the
reference values, float32 for the error bound), in the form of Z/frame_level_models.py:5218-5223 and :6059-6064 (Z = youtube-8m-zhangteng
of the reference):
    rnn_attention = softmax(outputs . W1 + b1 + input . W2 + b2, over ALL frames) * mask
    rnn_attention = rnn_attention / reduce_sum(rnn_attention, axis=1)
    rnn_out       = einsum("aij,ajk->aik", transpose(rnn_attention), values)
A (video, head) without an unmasked frame is 0 / 0 there; the project's convention puts zeros (no weight, no gradient).  The LSTM stacks
are oracle/torch_ref.lstm_stack; moe, cross_entropy, err and bounds come from gate_lstm_restatement, bound from ensemble_restatement.
Shared by tests/test_extend_attention_host.py and tests/test_gpu_extend_attention.py; not a test module."""
import numpy as np
import torch

from ensemble_restatement import bound  # noqa: F401
from gate_lstm_restatement import bounds, cross_entropy, err, moe  # noqa: F401
from oracle import torch_ref

CLASS_SIZE = 256


def mask(F, B, E, valid=None, lo=None, hi=None):
    """[B,F,E] bool: valid[b,t] != 0 and lo[b,e] <= t <= hi[b,e]; an absent operand does not restrict"""
    t = torch.arange(F).view(1, F, 1)
    m = torch.ones((B, F, E), dtype=torch.bool)
    if lo is not None:
        m = m & (t >= torch.as_tensor(np.asarray(lo)).to(torch.int64).view(B, 1, E))
    if hi is not None:
        m = m & (t <= torch.as_tensor(np.asarray(hi)).to(torch.int64).view(B, 1, E))
    if valid is not None:
        m = m & (torch.as_tensor(np.asarray(valid)).view(B, F, 1) != 0)
    return m


def windows(num_frames, E):
    """InputExtendModel's windows (Z/frame_level_models.py:6022-6030): lo = (num_frames // E) i, hi = lo + 2 (num_frames // E), int64 [B,E]"""
    step = torch.as_tensor(np.asarray(num_frames)).to(torch.int64).view(-1, 1) // E
    lo = step * torch.arange(E).view(1, E)
    return lo, lo + 2 * step


def attention(logits, m):
    """logits [B,F,E], m [B,F,E] bool -> (rnn_attention [B,F,E], the sum it was divided by [B,E]): softmax over all F frames, times the
    mask, divided by its sum; zeros where the mask of a (b, e) is empty."""
    rnn_attention = torch.softmax(logits, dim=1) * m.to(logits.dtype)
    s = rnn_attention.sum(dim=1, keepdim=True)
    return rnn_attention / torch.where(m.any(dim=1, keepdim=True), s, torch.ones_like(s)), s[:, 0, :]


def pool(att, values):
    """att [B,F,E], values [B,F,H] -> [B,E,H]: einsum('aij,ajk->aik', transpose(att, [0,2,1]), values)"""
    return torch.einsum("aij,ajk->aik", att.transpose(1, 2), values)


def op_with_grads(src_tm, vals_tm, W1, b1, extra, valid, lo, hi, G, dtype):
    """The op on time-major numpy float32 operands in `dtype`: src_tm [F,B,Hs], vals_tm [F,B,Hv] or None (the shared mode: the values are
    src_tm), extra [B,F,E] or None, G [B,E,Hv] (gradient at pooled).  Returns numpy att [B,F,E], den [B,E] (the sum the reference's form
    divides by), pooled [B,E,Hv], dsrc (in the shared mode the sum of both gradients), dvals (not in the shared mode), dW1, db1, dextra
    (with extra) for the loss sum(pooled G)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    src = T(src_tm).requires_grad_(True)
    vals = src if vals_tm is None else T(vals_tm).requires_grad_(True)
    W, b = T(W1).requires_grad_(True), T(b1).requires_grad_(True)
    x = None if extra is None else T(extra).requires_grad_(True)
    F, B, _ = src.shape
    logits = src.transpose(0, 1) @ W + b
    if x is not None:
        logits = logits + x
    att, den = attention(logits, mask(F, B, W.shape[1], valid, lo, hi))
    pooled = pool(att, vals.transpose(0, 1))
    (pooled * T(G)).sum().backward()
    grad = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    out = {"att": att.detach().numpy(), "den": den.detach().numpy(), "pooled": pooled.detach().numpy(), "dsrc": grad(src), "dW1": grad(W),
           "db1": grad(b)}
    if vals_tm is not None:
        out["dvals"] = grad(vals)
    if x is not None:
        out["dextra"] = grad(x)
    return out


def _layers(P, scope, L):
    return [(P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)], P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)])
            for l in range(L)]


def _logits(outputs, model_input, P):
    return outputs @ P["W1"] + P["b1"] + model_input @ P["W2"] + P["b2"]


def lstm_extend_model(model_input, num_frames, P, L, E):
    """-> (pooled [B E, H], attention_weight [B, E F]): frames_bool = (sum |x| > 0) per frame"""
    B, F, _ = model_input.shape
    outputs, _, _ = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "RNN", L))
    frames_bool = (model_input.abs().sum(dim=2) > 0).view(B, F, 1).expand(B, F, E)
    att, _ = attention(_logits(outputs, model_input, P), frames_bool)
    return pool(att, outputs).reshape(B * E, -1), att.transpose(1, 2).reshape(B, E * F)


def input_extend_model(model_input, num_frames, P, L, E):
    """-> (pooled [B E, H], attention_weight [B, E F]): the windows alone are the mask (frames_bool_all is computed and not used)"""
    B, F, _ = model_input.shape
    outputs, _, _ = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "RNN_Attention", L))
    outputs_features, _, _ = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "RNN", L))
    lo, hi = windows(num_frames, E)
    att, _ = attention(_logits(outputs, model_input, P), mask(F, B, E, None, lo, hi))
    return pool(att, outputs_features).reshape(B * E, -1), att.transpose(1, 2).reshape(B, E * F)


BODIES = {"LstmExtendModel": lstm_extend_model, "InputExtendModel": input_extend_model}


def moe_extend_model(model_input, P, M, E):
    """Z/video_level_models.py:2272-2330: rows [B E, width] -> predictions [B, V], the maximum over a video's E rows"""
    p = moe(model_input, P["gates/weights"], P["experts/weights"], P["experts/biases"], M)
    return p.view(model_input.shape[0] // E, E, -1).max(dim=1)[0]


def moe_extend_distill_chain_model(model_input, P, M, E, distill_labels=None):
    """Z/video_level_models.py:2332-2400: class_input = relu(FC(distill_labels)) (256 wide, not normalised) tiled over a video's E rows
    and concatenated behind the input"""
    if distill_labels is not None:
        class_input = torch.relu(distill_labels @ P["class_inputs/weights"] + P["class_inputs/biases"])
        class_input = class_input.view(-1, 1, CLASS_SIZE).repeat(1, E, 1).reshape(-1, CLASS_SIZE)
        model_input = torch.cat((model_input, class_input), dim=1)
    return moe_extend_model(model_input, P, M, E)


def predictions(name, head, model_input, num_frames, P, L, M, E, distill_labels=None):
    """The whole plugin with its head: predictions [B,V]"""
    pooled, _ = BODIES[name](model_input, num_frames, P, L, E)
    if head == "MoeExtendDistillChainModel":
        return moe_extend_distill_chain_model(pooled, P, M, E, distill_labels)
    return moe_extend_model(pooled, P, M, E)


def variable_shapes(name, head, D, H, L, E, V, M, distill=False):
    """The variables in creation order: {name: shape}"""
    s = {}
    for scope in (("RNN_Attention", "RNN") if name == "InputExtendModel" else ("RNN",)):
        for l in range(L):
            s["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)] = ((D if l == 0 else H) + H, 4 * H)
            s["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)] = (4 * H,)
    s.update({"W1": (H, E), "b1": (E,), "W2": (D, E), "b2": (E,)})
    width = H
    if head == "MoeExtendDistillChainModel" and distill:
        s["class_inputs/weights"] = (V, CLASS_SIZE)
        s["class_inputs/biases"] = (CLASS_SIZE,)
        width += CLASS_SIZE
    if head is not None:
        s["gates/weights"] = (width, V * (M + 1))
        s["experts/weights"] = (width, V * M)
        s["experts/biases"] = (V * M,)
    return s
