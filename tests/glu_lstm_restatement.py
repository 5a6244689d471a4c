"""Restatement of the input-memory LSTM models in plain torch, in the dtype of its inputs (float64 for the reference values, float32 for
the error bound), with the variable names of Z/frame_level_models.py:631-885 (Z = youtube-8m-zhangteng of the reference).  Per step, with
previous_hidden_x = l2_normalize(x_prev) carried beside x_prev:
    i, f, ix, fx = sigmoid(x.W* + previous_hidden_x.V* + previous_hidden_state.U* + b*)   [B,1] each
    o = sigmoid(x.Wog + previous_hidden_x.Vog + previous_hidden_state.Uog + bog)          [B,H]
    c_ = tanh(x.Wc + previous_hidden_x.Vc + previous_hidden_state.Uc + bc)                [B,H]
    c = f * c_prev + i * c_,   current_x = fx * x_prev + ix * x,   current_hidden_x = l2_normalize(current_x),   h = o * tanh(c)
run over all max_frames steps from zeros, the memory c gathered at frame num_frames - 1 (zeros for num_frames < 1: the project's
convention).  This is the reference's form: the product with V* is made at every step.  Shared by tests/test_glu_lstm_host.py and
tests/test_gpu_glu_lstm.py; not a test module."""
import numpy as np
import torch

from gate_lstm_restatement import bounds, cross_entropy, err, gather_last, moe, to_torch  # noqa: F401  (shared measure and head)

NAMES = ("Wi", "Ui", "Vi", "bi", "Wf", "Vf", "Uf", "bf", "Wog", "Vog", "Uog", "bog", "Wc", "Vc", "Uc", "bc",
         "Wix", "Vix", "Uix", "bix", "Wfx", "Vfx", "Ufx", "bfx")
SCALARS = ("i", "f", "ix", "fx")


def shapes(emb_dim, hidden_dim):
    out = {}
    for n in NAMES:
        wide = n[1:] in ("og", "c")
        if n[0] == "b":
            out[n] = (hidden_dim,) if wide else (1,)
        else:
            out[n] = (hidden_dim if n[0] == "U" else emb_dim, hidden_dim if wide else 1)
    return out


def random_unit(rs, emb_dim, hidden_dim, scale=None):
    """The 24 arrays (float32) in create_recurrent_unit's order: weights uniform with the spread of a Glorot draw (a trained unit's
    scale, so that the gates leave their linear range; stddev = 0.1 makes the recurrence chaotic), biases around the reference's
    constants."""
    P = {}
    for n, s in shapes(emb_dim, hidden_dim).items():
        if n[0] == "b":
            P[n] = ((1.0 if n in ("bf", "bfx") else 0.1) + 0.05 * rs.randn(*s)).astype(np.float32)
        else:
            lim = scale if scale is not None else np.sqrt(6.0 / (s[0] + hidden_dim))
            P[n] = ((rs.random_sample(s) * 2 - 1) * lim).astype(np.float32)
    return P


def operands(P):
    """The 24 Variables -> the operands of seq_ops.glu_lstm_layer: Wv, bv, Ws, bs, Vv, Vs, Uv, Us."""
    cat = torch.cat if torch.is_tensor(P["Wi"]) else (lambda ts, dim=0: np.concatenate(ts, axis=dim))
    Us = cat([P["U" + n] for n in SCALARS], 1)
    return (cat([P["Wog"], P["Wc"]], 1), cat([P["bog"], P["bc"]], 0), cat([P["W" + n] for n in SCALARS], 1),
            cat([P["b" + n] for n in SCALARS], 0), cat([P["Vog"], P["Vc"]], 1), cat([P["V" + n] for n in SCALARS], 1),
            cat([P["Uog"], P["Uc"]], 1), Us.t() if torch.is_tensor(Us) else Us.T)


def l2_normalize(x, epsilon=1e-12):
    """tf.nn.l2_normalize(x, dim=1): x * rsqrt(max(sum(x^2), epsilon))"""
    return x * torch.rsqrt((x * x).sum(1, keepdim=True).clamp(min=epsilon))


def unit(x, previous_hidden_x, x_prev, previous_hidden_state, c_prev, P):
    """create_recurrent_unit's unit(x, hidden_memory_tm0, hidden_memory_tm1) -> (gates dict, current_hidden_x, current_x,
    current_hidden_state, c)."""
    pre = lambda n: x @ P["W" + n] + previous_hidden_x @ P["V" + n] + previous_hidden_state @ P["U" + n] + P["b" + n]
    i, f, ix, fx = (torch.sigmoid(pre(n)) for n in SCALARS)
    o = torch.sigmoid(pre("og"))
    c_ = torch.tanh(pre("c"))
    c = f * c_prev + i * c_
    current_x = fx * x_prev + ix * x
    current_hidden_x = l2_normalize(current_x)
    current_hidden_state = o * torch.tanh(c)
    return {"i": i, "f": f, "ix": ix, "fx": fx, "o": o, "g": c_}, current_hidden_x, current_x, current_hidden_state, c


def rnn_gate(model_input, num_frames, P, tape=None):
    """model_input [B,F,D] -> (state_outputs [B,H] gathered at num_frames - 1, hidden_outputs [B,F,H]).  tape (a dict) receives
    every step's gates and states."""
    B, max_frames, emb_dim = model_input.shape
    hidden_dim = P["Uog"].shape[0]
    h = c = torch.zeros((B, hidden_dim), dtype=model_input.dtype)
    hx = xp = torch.zeros((B, emb_dim), dtype=model_input.dtype)
    hidden, state = [], []
    for t in range(max_frames):
        gates, hx, xp, h, c = unit(model_input[:, t, :], hx, xp, h, c, P)
        hidden.append(h)
        state.append(c)
        if tape is not None:
            for k, v in gates.items():
                tape.setdefault(k, []).append(v)
            tape.setdefault("xm", []).append(xp)
    return gather_last(torch.stack(state, dim=1), num_frames), torch.stack(hidden, dim=1)


def multilayer(model_input, num_frames, layers):
    """LstmGlu2MultilayerModel's body: layers = [P_0, P_1, ...] -> the layers' gathered memories concatenated [B, L H]."""
    hidden_outputs, state_outputs = model_input, []
    for P in layers:
        state_output, hidden_outputs = rnn_gate(hidden_outputs, num_frames, P)
        state_outputs.append(state_output)
    return torch.cat(state_outputs, dim=1)


def layer_with_grads(x_tm, num_frames, P, dout, dc_last, dtype):
    """One layer on time-major frames x_tm [F,B,D] (numpy) in `dtype`: out_tm [F,B,H], c_last [B,H], dx [F,B,D] and the 24 parameter
    gradients for the loss sum(out_tm * dout) + sum(c_last * dc_last) (either may be None)."""
    x = torch.from_numpy(np.asarray(x_tm)).to(dtype).transpose(0, 1).clone().requires_grad_(True)
    Pt = to_torch(P, dtype, True)
    state, hidden = rnn_gate(x, torch.from_numpy(np.asarray(num_frames)), Pt)
    loss = 0.0
    if dout is not None:
        loss = loss + (hidden.transpose(0, 1) * torch.from_numpy(dout).to(dtype)).sum()
    if dc_last is not None:
        loss = loss + (state * torch.from_numpy(dc_last).to(dtype)).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = {"out": hidden.detach().transpose(0, 1).numpy(), "c_last": state.detach().numpy(), "dx": zero(x).transpose(0, 1).numpy()}
    res.update({"d" + n: zero(Pt[n]).numpy() for n in NAMES})
    return res


def recurrence_with_grads(x_tm, P, num_frames, dout, dc_last, dtype):
    """What the C ABI computes, restated in the REFERENCE's form (the product with V* at every step) on frames x_tm [F,B,D] (numpy) and
    the unit P, in `dtype`: the tapes o, g [F,B,H], s [F,B,4] = i | f | ix | fx, hs, cs [F+1,B,H], xm [F+1,B,D], n2 [F+1,B],
    qv [F+1,B,2H] = xm.[Vog|Vc], qs [F+1,B,4] = xm.Vs, c_last, and -- for the loss sum(hs[1:] * dout) + sum(c_last * dc_last), either may
    be None -- the gradients with respect to the hoisted products a caller of the C ABI hands over: dzv [F,B,2H] (x.[Wog|Wc] + b),
    dzs [F,B,4], dpv [F,B,2H] (x.[Vog|Vc]), dps [F,B,4] (x.Vs) and dx_direct [F,B,D], the part of dx that reaches x through
    current_x = fx * x_prev + ix * x without passing through a product.
    The reference has no node for x_t.V* and does not tell the two ways current_x is read apart, so these gradients are taken through
    zero-valued leaves and a second copy of the state: epv_t, eps_t enter running sums E' = fx E + ix e_t that are identically zero and
    are added as r * E beside previous_hidden_x.V*; dz* are leaves added to the pre-activations; x_prev is carried twice with the same
    values, xn for the norm (r = rsqrt(max(sum xn^2, 1e-12))) and xm for the product (previous_hidden_x = xm * r), and ex_t is added to
    x_t in xn alone.  Adding 0.0 is exact and both copies hold the same bits, so every value of the forward pass is the reference
    form's, bit for bit in either dtype."""
    Pt = to_torch(P, dtype)
    Wv, bv, Ws, bs, Vv, Vs, Uv, Us = operands(Pt)
    x = torch.from_numpy(np.asarray(x_tm)).to(dtype)
    F, B, D = x.shape
    H = Uv.shape[0]
    leaf = lambda *shape: torch.zeros(shape, dtype=dtype, requires_grad=True)
    ezv, epv, ezs, eps_, ex = leaf(F, B, 2 * H), leaf(F, B, 2 * H), leaf(F, B, 4), leaf(F, B, 4), leaf(F, B, D)
    h = c = torch.zeros((B, H), dtype=dtype)
    xm, Ev, Es = torch.zeros((B, D), dtype=dtype), torch.zeros((B, 2 * H), dtype=dtype), torch.zeros((B, 4), dtype=dtype)
    xn = xm
    T = {k: [] for k in ("o", "g", "s")}
    T.update({"hs": [h], "cs": [c], "xm": [xm], "qv": [xm @ Vv], "qs": [xm @ Vs], "n2": [(xm * xm).sum(1)]})
    for t in range(F):
        r = torch.rsqrt((xn * xn).sum(1, keepdim=True).clamp(min=1e-12))
        hx = xm * r
        s = torch.sigmoid(x[t] @ Ws + hx @ Vs + h @ Us.t() + bs + r * Es + ezs[t])
        v = x[t] @ Wv + hx @ Vv + h @ Uv + bv + r * Ev + ezv[t]
        o, g = torch.sigmoid(v[:, :H]), torch.tanh(v[:, H:])
        c = s[:, 1:2] * c + s[:, 0:1] * g
        h = o * torch.tanh(c)
        ix, fx = s[:, 2:3], s[:, 3:4]
        xm, xn, Ev, Es = fx * xm + ix * x[t], fx * xn + ix * (x[t] + ex[t]), fx * Ev + ix * epv[t], fx * Es + ix * eps_[t]
        for k, val in (("o", o), ("g", g), ("s", s), ("hs", h), ("cs", c), ("xm", xm), ("qv", xm @ Vv), ("qs", xm @ Vs),
                       ("n2", (xm * xm).sum(1))):
            T[k].append(val)
    T = {k: torch.stack(v) for k, v in T.items()}
    c_last = gather_last(T["cs"][1:].transpose(0, 1), torch.from_numpy(np.asarray(num_frames)))
    loss = 0.0
    if dout is not None:
        loss = loss + (T["hs"][1:] * torch.from_numpy(dout).to(dtype)).sum()
    if dc_last is not None:
        loss = loss + (c_last * torch.from_numpy(dc_last).to(dtype)).sum()
    if torch.is_tensor(loss):
        loss.backward()
    grad = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = {k: v.detach().numpy() for k, v in T.items()}
    dpv, dps = grad(epv), grad(eps_)
    res.update({"c_last": c_last.detach().numpy(), "dzv": grad(ezv).numpy(), "dpv": dpv.numpy(), "dzs": grad(ezs).numpy(), "dps": dps.numpy(),
                "dx_direct": grad(ex).numpy()})
    return res
