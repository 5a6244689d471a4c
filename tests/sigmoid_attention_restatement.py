"""Restatement of the sigmoid-attention LSTM models and of their pooling in plain torch, in the dtype of its inputs (float64 for the
reference values, float32 for the error bound), following W/all_frame_models/lstm_attention_model.py:56-74,
lstm_attention_lstm_model.py:64-93 and lstm_multi_attention_model.py:57-90 (W = youtube-8m-wangheda of the reference):
    attention_fc = sigmoid(outputs . weights + biases)            [B,F,A]
    attention    = attention_fc * mask;  attention = attention / (reduce_sum(attention, axis=1) + 1e-8)
    pooled       = reduce_sum(attention * values, axis=1)         (einsum "ijk,ijl->ikl" for A > 1)
mask_emb's lookup is the comparison t < num_frames.  The LSTM stacks are oracle/torch_ref.lstm_stack (BasicLSTMCell under dynamic_rnn);
heads, err and bounds come from gate_lstm_restatement, bound from ensemble_restatement.  Shared by tests/test_sigmoid_attention_host.py
and tests/test_gpu_sigmoid_attention.py; not a test module."""
import numpy as np
import torch

from ensemble_restatement import bound  # noqa: F401
from gate_lstm_restatement import bounds, cross_entropy, err, moe  # noqa: F401
from oracle import torch_ref


def frame_mask(num_frames, F, dtype):
    """[B,F]: 1 for t < clamp(num_frames, 0, F)"""
    n = torch.as_tensor(np.asarray(num_frames)).to(torch.int64).clamp(0, F)
    return (torch.arange(F)[None, :] < n[:, None]).to(dtype)


def attention(outputs, weights, biases, num_frames):
    """outputs [B,F,H] (batch-major, as the reference holds them) -> (attention [B,F,A], attention_sum [B,A])."""
    attention_fc = torch.sigmoid(outputs @ weights + biases)
    att = attention_fc * frame_mask(num_frames, outputs.shape[1], outputs.dtype)[:, :, None]
    attention_sum = att.sum(dim=1, keepdim=True) + 1e-8
    return att / attention_sum, attention_sum[:, 0, :]


def pool(att, values):
    """att [B,F,A], values [B,F,D] -> [B,A,D]"""
    return torch.einsum("ijk,ijl->ikl", att, values)


def op_with_grads(src_tm, vals_tm, Wa, ba, num_frames, G, E, dtype):
    """The op on time-major numpy float32 operands in `dtype`: src_tm [F,B,Hs], vals_tm [F,B,Hv] or None, G [B,A,Hv] or None (gradient
    at pooled), E [B,F,A] or None (gradient at att).  Returns numpy att [B,F,A], den [B,A], pooled [B,A,Hv], dsrc [F,B,Hs], dvals
    [F,B,Hv], dWa, dba for the loss sum(pooled G) + sum(att E) (zeros where nothing reaches a quantity)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    src = T(src_tm).requires_grad_(True)
    vals = None if vals_tm is None else T(vals_tm).requires_grad_(True)
    W, b = T(Wa).requires_grad_(True), T(ba).requires_grad_(True)
    att, den = attention(src.transpose(0, 1), W, b, num_frames)
    res = {"att": att, "den": den}
    loss = 0.0
    if vals is not None:
        res["pooled"] = pool(att, vals.transpose(0, 1))
        if G is not None:
            loss = loss + (res["pooled"] * T(G)).sum()
    if E is not None:
        loss = loss + (att * T(E)).sum()
    if torch.is_tensor(loss):
        loss.backward()
    grad = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    out = {k: v.detach().numpy() for k, v in res.items()}
    out.update({"dsrc": grad(src), "dWa": grad(W), "dba": grad(b)})
    if vals is not None:
        out["dvals"] = grad(vals)
    return out


def _layers(P, scope, L):
    return [(P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)], P["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)])
            for l in range(L)]


def lstm_attention_model(model_input, num_frames, P, L):
    """-> final_state [B, D + 2 L H] = [mean_input | c0|h0|c1|h1...] (state_is_tuple=False)."""
    outputs, c, h = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "RNN", L))
    att, _ = attention(outputs, P["RNN/fully_connected/weights"], P["RNN/fully_connected/biases"], num_frames)
    mean_input = (att * model_input).sum(dim=1)
    return torch.cat([mean_input] + [t for pair in zip(c, h) for t in pair], dim=1)


def lstm_attention_lstm_model(model_input, num_frames, P, L):
    """-> final_state [B, H + 2 L H] = [attended_output | ATT memories c | RNN memories c]."""
    att_outputs, att_c, _ = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "ATT", L))
    outputs, c, _ = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "RNN", L))
    att, _ = attention(att_outputs, P["RNN/fully_connected/weights"], P["RNN/fully_connected/biases"], num_frames)
    attended_output = (att * outputs).sum(dim=1)
    return torch.cat([attended_output] + att_c + c, dim=1)


def lstm_multi_attention_model(model_input, num_frames, P, L):
    """-> attention_input [B, A, D]; the head runs on its B A rows and the prediction is the maximum over a video's A rows."""
    outputs, _, _ = torch_ref.lstm_stack(model_input, num_frames, _layers(P, "RNN", L))
    att, _ = attention(outputs, P["fully_connected/weights"], P["fully_connected/biases"], num_frames)
    return pool(att, model_input)


BODIES = {"LstmAttentionModel": lstm_attention_model, "LstmAttentionLstmModel": lstm_attention_lstm_model,
          "LstmMultiAttentionModel": lstm_multi_attention_model}


def predictions(name, model_input, num_frames, P, L, M):
    """The whole plugin with the MoE head (W/all_video_models/moe_model.py): predictions [B,V]."""
    head_input = BODIES[name](model_input, num_frames, P, L)
    if name != "LstmMultiAttentionModel":
        return moe(head_input, P["gates/weights"], P["experts/weights"], P["experts/biases"], M)
    B, A, D = head_input.shape
    p = moe(head_input.reshape(B * A, D), P["gates/weights"], P["experts/weights"], P["experts/biases"], M)
    return p.view(B, A, -1).max(dim=1)[0]


def variable_shapes(name, D, H, L, A, V, M):
    """The plugins' variables in creation order: {name: shape}."""
    s = {}
    for scope in (("ATT", "RNN") if name == "LstmAttentionLstmModel" else ("RNN",)):
        for l in range(L):
            s["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/weights" % (scope, l)] = ((D if l == 0 else H) + H, 4 * H)
            s["%s/multi_rnn_cell/cell_%d/basic_lstm_cell/biases" % (scope, l)] = (4 * H,)
    fc = "fully_connected" if name == "LstmMultiAttentionModel" else "RNN/fully_connected"
    s[fc + "/weights"] = (H, A if name == "LstmMultiAttentionModel" else 1)
    s[fc + "/biases"] = (s[fc + "/weights"][1],)
    width = {"LstmAttentionModel": D + 2 * L * H, "LstmAttentionLstmModel": H + 2 * L * H, "LstmMultiAttentionModel": D}[name]
    s["gates/weights"] = (width, V * (M + 1))
    s["experts/weights"] = (width, V * M)
    s["experts/biases"] = (V * M,)
    return s
