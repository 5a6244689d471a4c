"""Restatement of the scalar-gate LSTM models in plain torch, in the dtype of its inputs (float64 for the reference values, float32 for
the error bound), with the variable names of Z/frame_level_models.py:1521-1790 (Z = youtube-8m-zhangteng of the reference):
    i = sigmoid(x.Wi + h.Ui + bi) [B,1]     f = sigmoid(x.Wf + h.Uf + bf) [B,1]
    o = sigmoid(x.Wog + h.Uog + bog) [B,H]  c_ = tanh(x.Wc + h.Uc + bc) [B,H]       c = f * c_prev + i * c_,  h = o * tanh(c)
run over all max_frames steps from h = c = 0, the memory gathered at frame num_frames - 1 (zeros for num_frames < 1: the project's
convention).  Shared by tests/test_gate_lstm_host.py and tests/test_gpu_gate_lstm.py; not a test module."""
import numpy as np
import torch

NAMES = ("Wi", "Ui", "bi", "Wf", "Uf", "bf", "Wog", "Uog", "bog", "Wc", "Uc", "bc")


def shapes(emb_dim, hidden_dim):
    return {"Wi": (emb_dim, 1), "Ui": (hidden_dim, 1), "bi": (1,), "Wf": (emb_dim, 1), "Uf": (hidden_dim, 1), "bf": (1,),
            "Wog": (emb_dim, hidden_dim), "Uog": (hidden_dim, hidden_dim), "bog": (hidden_dim,),
            "Wc": (emb_dim, hidden_dim), "Uc": (hidden_dim, hidden_dim), "bc": (hidden_dim,)}


def random_unit(rs, emb_dim, hidden_dim, scale=None):
    """The twelve arrays (float32) in create_recurrent_unit's order: weights uniform with the spread of a Glorot draw (a trained unit's
    scale, so that the gates leave their linear range), biases around the reference's constants."""
    P = {}
    for n, s in shapes(emb_dim, hidden_dim).items():
        if n[0] == "b":
            P[n] = ((1.0 if n == "bf" else 0.1) + 0.05 * rs.randn(*s)).astype(np.float32)
        else:
            lim = scale if scale is not None else np.sqrt(6.0 / (s[0] + hidden_dim))
            P[n] = ((rs.random_sample(s) * 2 - 1) * lim).astype(np.float32)
    return P


def operands(P):
    """The twelve Variables -> the operands of seq_ops.gate_lstm_layer: Wv, bv, Ws, bs, Uv, Us."""
    cat = torch.cat if torch.is_tensor(P["Wi"]) else (lambda ts, dim=0: np.concatenate(ts, axis=dim))
    Us = cat([P["Ui"], P["Uf"]], 1)
    return (cat([P["Wog"], P["Wc"]], 1), cat([P["bog"], P["bc"]], 0), cat([P["Wi"], P["Wf"]], 1), cat([P["bi"], P["bf"]], 0),
            cat([P["Uog"], P["Uc"]], 1), Us.t() if torch.is_tensor(Us) else Us.T)


def unit(x, previous_hidden_state, c_prev, P):
    """create_recurrent_unit's unit(x, hidden_memory_tm1) -> (i, f, o, c_, c, current_hidden_state)."""
    i = torch.sigmoid(x @ P["Wi"] + previous_hidden_state @ P["Ui"] + P["bi"])
    f = torch.sigmoid(x @ P["Wf"] + previous_hidden_state @ P["Uf"] + P["bf"])
    o = torch.sigmoid(x @ P["Wog"] + previous_hidden_state @ P["Uog"] + P["bog"])
    c_ = torch.tanh(x @ P["Wc"] + previous_hidden_state @ P["Uc"] + P["bc"])
    c = f * c_prev + i * c_
    return i, f, o, c_, c, o * torch.tanh(c)


def gather_last(state_outputs, num_frames):
    """state_outputs [B,F,H] -> row num_frames - 1 of every video; zeros where num_frames is not in 1..F."""
    B, F = state_outputs.shape[:2]
    nf = num_frames.to(torch.int64)
    valid = ((nf >= 1) & (nf <= F)).to(state_outputs.dtype).unsqueeze(1)
    return state_outputs[torch.arange(B), (nf - 1).clamp(0, F - 1)] * valid


def rnn_gate(model_input, num_frames, P):
    """model_input [B,F,D] -> (state_outputs [B,H] gathered at num_frames - 1, hidden_outputs [B,F,H])."""
    B, max_frames = model_input.shape[:2]
    hidden_dim = P["Uog"].shape[0]
    h = c = torch.zeros((B, hidden_dim), dtype=model_input.dtype)
    hidden, state = [], []
    for t in range(max_frames):
        _, _, _, _, c, h = unit(model_input[:, t, :], h, c, P)
        hidden.append(h)
        state.append(c)
    return gather_last(torch.stack(state, dim=1), num_frames), torch.stack(hidden, dim=1)


def multilayer(model_input, num_frames, layers):
    """LstmGateMultilayerModel's body: layers = [P_0, P_1, ...] -> the layers' gathered memories concatenated [B, L H]."""
    hidden_outputs, state_outputs = model_input, []
    for P in layers:
        state_output, hidden_outputs = rnn_gate(hidden_outputs, num_frames, P)
        state_outputs.append(state_output)
    return torch.cat(state_outputs, dim=1)


def moe(x, Wg, We, be, M):
    """W/all_video_models/moe_model.py:40-64 (the head both plugins end in by default)."""
    B = x.shape[0]
    V = We.shape[1] // M
    g = torch.softmax((x @ Wg).view(B, V, M + 1), dim=2)
    e = torch.sigmoid((x @ We + be).view(B, V, M))
    return (g[:, :, :M] * e).sum(2)


def cross_entropy(p, labels, eps=10e-6):
    """W/losses.py:114-130."""
    y = labels.to(p.dtype)
    return -(y * torch.log(p + eps) + (1 - y) * torch.log(1 - p + eps)).sum(1).mean()


def to_torch(P, dtype, requires_grad=False):
    return {n: torch.from_numpy(np.asarray(a)).to(dtype).clone().requires_grad_(requires_grad) for n, a in P.items()}


def layer_with_grads(x_tm, num_frames, P, dout, dc_last, dtype):
    """One layer on time-major frames x_tm [F,B,D] (numpy float32) in `dtype`: out_tm [F,B,H], c_last [B,H], dx [F,B,D] and the twelve
    parameter gradients for the loss sum(out_tm * dout) + sum(c_last * dc_last)."""
    x = torch.from_numpy(x_tm).to(dtype).transpose(0, 1).clone().requires_grad_(True)
    Pt = to_torch(P, dtype, True)
    state, hidden = rnn_gate(x, torch.from_numpy(np.asarray(num_frames)), Pt)
    loss = (hidden.transpose(0, 1) * torch.from_numpy(dout).to(dtype)).sum() + (state * torch.from_numpy(dc_last).to(dtype)).sum()
    loss.backward()
    res = {"out": hidden.detach().transpose(0, 1).numpy(), "c_last": state.detach().numpy(), "dx": x.grad.transpose(0, 1).numpy()}
    res.update({"d" + n: Pt[n].grad.numpy() for n in NAMES})
    return res


def recurrence_with_grads(zv, zs, Uv, Us, num_frames, dout, dc_last, dtype):
    """The recurrence on GIVEN hoisted inputs (what the C ABI takes): zv [F,B,2H] = x.[Wog|Wc] + [bog|bc], zs [F,B,2] = x.[Wi|Wf] +
    [bi|bf], Uv [H,2H], Us [2,H]; dout [F,B,H] or None, dc_last [B,H] or None.  Returns o, g [F,B,H], i, f [F,B], hs, cs [F+1,B,H],
    c_last [B,H] and dzv [F,B,2H], dzs [F,B,2] (zeros when neither gradient is given), all in `dtype` as numpy."""
    zv_t = torch.from_numpy(zv).to(dtype).clone().requires_grad_(True)
    zs_t = torch.from_numpy(zs).to(dtype).clone().requires_grad_(True)
    Uv_t, Us_t = torch.from_numpy(Uv).to(dtype), torch.from_numpy(Us).to(dtype)
    F, B, H2 = zv.shape
    H = H2 // 2
    h = c = torch.zeros((B, H), dtype=dtype)
    hs, cs, og, sg = [h], [c], [], []
    for t in range(F):
        s = torch.sigmoid(zs_t[t] + h @ Us_t.t())
        v = zv_t[t] + h @ Uv_t
        o, g = torch.sigmoid(v[:, :H]), torch.tanh(v[:, H:])
        c = s[:, 1:2] * c + s[:, 0:1] * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        og.append(torch.cat([o, g], dim=1))
        sg.append(s)
    hs, cs, og, sg = torch.stack(hs), torch.stack(cs), torch.stack(og), torch.stack(sg)
    c_last = gather_last(cs[1:].transpose(0, 1), torch.from_numpy(np.asarray(num_frames)))
    loss = 0.0
    if dout is not None:
        loss = loss + (hs[1:] * torch.from_numpy(dout).to(dtype)).sum()
    if dc_last is not None:
        loss = loss + (c_last * torch.from_numpy(dc_last).to(dtype)).sum()
    if torch.is_tensor(loss):
        loss.backward()
    n = lambda t: t.detach().numpy()
    return {"o": n(og[:, :, :H]), "g": n(og[:, :, H:]), "i": n(sg[:, :, 0]), "f": n(sg[:, :, 1]), "hs": n(hs), "cs": n(cs), "c_last": n(c_last),
            "dzv": n(zv_t.grad) if zv_t.grad is not None else np.zeros(zv.shape), "dzs": n(zs_t.grad) if zs_t.grad is not None else np.zeros(zs.shape)}


def err(got, ref):
    """max |got - ref| relative to max(1, max |ref|): the fp64 tests' measure"""
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def bounds(ref64, ref32, floor):
    """Per quantity: eight times the float32 restatement's error against the float64 one, never below `floor(name)`."""
    return {k: max(8.0 * err(ref32[k], ref64[k]), floor(k)) for k in ref64}
