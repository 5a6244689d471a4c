"""Restatement of LstmBigluModel (Z/frame_level_models.py:887-1158, Z = youtube-8m-zhangteng of the reference) in plain torch, in the
dtype of its inputs (float64 for the reference values, float32 for the error bound), with the reference's variable names and WITH its
two tf.reverse_sequence copies, made row by row with flip -- it shares no indexing with the frame-order kernels it checks:
    pass 1 over reverse_sequence(model_input, num_frames), from h = c = 0, all max_frames steps (create_forward_recurrent_unit):
        i = sigmoid(x.Wi + h.Ui + bi) [B,1]     f = sigmoid(x.Wf + h.Uf + bf) [B,1]
        o = sigmoid(x.Wog + h.Uog + bog) [B,H]  c_ = tanh(x.Wc + h.Uc + bc) [B,H]       c = f * c_prev + i * c_,  h = o * tanh(c)
    y = reverse_sequence(pass 1's hidden states, num_frames)
    pass 2 over model_input in order (create_backward_recurrent_unit): the same cell, every gate with + y_t.V* (Vi, Vf [H,1]; Vog, Vc [H,H])
    head: MoE on [c1 | c2], both memories gathered at step num_frames - 1 (zeros for num_frames < 1: the project's convention).
Shared by tests/test_bigate_lstm_host.py and tests/test_gpu_bigate_lstm.py; not a test module."""
import numpy as np
import torch

from gate_lstm_restatement import bounds, cross_entropy, err, gather_last, moe, to_torch  # noqa: F401  (re-exported)

NAMES_FW = ("Wi", "Ui", "bi", "Wf", "Uf", "bf", "Wog", "Uog", "bog", "Wc", "Uc", "bc")
NAMES_BW = ("Wi", "Ui", "Vi", "bi", "Wf", "Vf", "Uf", "bf", "Wog", "Vog", "Uog", "bog", "Wc", "Vc", "Uc", "bc")


def shapes(names, emb_dim, hidden_dim):
    """name -> shape, in the order of `names`: W* are emb_dim tall, U* and V* hidden_dim tall; og and c are hidden_dim wide, i and f 1."""
    out = {}
    for n in names:
        width = hidden_dim if n[1:] in ("og", "c") else 1
        out[n] = (width,) if n[0] == "b" else (emb_dim if n[0] == "W" else hidden_dim, width)
    return out


def random_unit(rs, names, emb_dim, hidden_dim, scale=None):
    """The unit's arrays (float32) in the reference's order: weights uniform with the spread of a Glorot draw (a trained unit's scale,
    so that the gates leave their linear range), every bias -- bf too -- around the reference's 0.1."""
    P = {}
    for n, s in shapes(names, emb_dim, hidden_dim).items():
        if n[0] == "b":
            P[n] = (0.1 + 0.05 * rs.randn(*s)).astype(np.float32)
        else:
            lim = scale if scale is not None else np.sqrt(6.0 / (s[0] + hidden_dim))
            P[n] = ((rs.random_sample(s) * 2 - 1) * lim).astype(np.float32)
    return P


def operands(Pf, Pb):
    """The 12 + 16 Variables -> the operands of seq_ops.bigate_lstm_layer: Wv, bv, Ws, bs, Uv1, Us1, Vv, Vs, Uv2, Us2."""
    tt = torch.is_tensor(Pf["Wi"])
    cat = torch.cat if tt else (lambda ts, dim=0: np.concatenate(ts, axis=dim))
    tr = (lambda a: a.t()) if tt else (lambda a: a.T)
    return (cat([Pf["Wog"], Pf["Wc"], Pb["Wog"], Pb["Wc"]], 1), cat([Pf["bog"], Pf["bc"], Pb["bog"], Pb["bc"]], 0),
            cat([Pf["Wi"], Pf["Wf"], Pb["Wi"], Pb["Wf"]], 1), cat([Pf["bi"], Pf["bf"], Pb["bi"], Pb["bf"]], 0),
            cat([Pf["Uog"], Pf["Uc"]], 1), tr(cat([Pf["Ui"], Pf["Uf"]], 1)),
            cat([Pb["Vog"], Pb["Vc"]], 1), cat([Pb["Vi"], Pb["Vf"]], 1),
            cat([Pb["Uog"], Pb["Uc"]], 1), tr(cat([Pb["Ui"], Pb["Uf"]], 1)))


def operand_grads(gf, gb):
    """The same packing for gradients: gf / gb map a Variable's name to its gradient; returns dWv .. dUs2 by operand name."""
    names = ("dWv", "dbv", "dWs", "dbs", "dUv1", "dUs1", "dVv", "dVs", "dUv2", "dUs2")
    return dict(zip(names, operands(gf, gb)))


def reverse_sequence(x, num_frames):
    """tf.reverse_sequence(x, num_frames, seq_axis=1) on batch-major x [B,F,...]: frames 0 .. n_b - 1 of every video flipped, the
    rest left where they are (n_b clamped to 0..F), one video at a time."""
    F = x.shape[1]
    rows = []
    for b in range(x.shape[0]):
        n = min(max(int(num_frames[b]), 0), F)
        rows.append(torch.cat([x[b, :n].flip(0), x[b, n:]], dim=0))
    return torch.stack(rows)


def forward_unit(x, previous_hidden_state, c_prev, P):
    """create_forward_recurrent_unit's unit(x, hidden_memory_tm1) -> (i, f, o, c_, c, current_hidden_state)."""
    i = torch.sigmoid(x @ P["Wi"] + previous_hidden_state @ P["Ui"] + P["bi"])
    f = torch.sigmoid(x @ P["Wf"] + previous_hidden_state @ P["Uf"] + P["bf"])
    o = torch.sigmoid(x @ P["Wog"] + previous_hidden_state @ P["Uog"] + P["bog"])
    c_ = torch.tanh(x @ P["Wc"] + previous_hidden_state @ P["Uc"] + P["bc"])
    c = f * c_prev + i * c_
    return i, f, o, c_, c, o * torch.tanh(c)


def backward_unit(x, y, previous_hidden_state, c_prev, P):
    """create_backward_recurrent_unit's unit(x, y, hidden_memory_tm1) -> (i, f, o, c_, c, current_hidden_state)."""
    i = torch.sigmoid(x @ P["Wi"] + y @ P["Vi"] + previous_hidden_state @ P["Ui"] + P["bi"])
    f = torch.sigmoid(x @ P["Wf"] + y @ P["Vf"] + previous_hidden_state @ P["Uf"] + P["bf"])
    o = torch.sigmoid(x @ P["Wog"] + y @ P["Vog"] + previous_hidden_state @ P["Uog"] + P["bog"])
    c_ = torch.tanh(x @ P["Wc"] + y @ P["Vc"] + previous_hidden_state @ P["Uc"] + P["bc"])
    c = f * c_prev + i * c_
    return i, f, o, c_, c, o * torch.tanh(c)


def model_states(model_input, num_frames, Pf, Pb):
    """model_input [B,F,D] -> (c1 [B,H], c2 [B,H] gathered at step num_frames - 1, y [B,F,H], pass 2's hidden states [B,F,H])."""
    B, max_frames = model_input.shape[:2]
    hidden_dim = Pf["Uog"].shape[0]
    model_input_reverse = reverse_sequence(model_input, num_frames)
    h = c = torch.zeros((B, hidden_dim), dtype=model_input.dtype)
    hidden, state = [], []
    for t in range(max_frames):
        _, _, _, _, c, h = forward_unit(model_input_reverse[:, t, :], h, c, Pf)
        hidden.append(h)
        state.append(c)
    forward_state_outputs = gather_last(torch.stack(state, dim=1), num_frames)
    x_outputs_reverse = reverse_sequence(torch.stack(hidden, dim=1), num_frames)
    h = c = torch.zeros((B, hidden_dim), dtype=model_input.dtype)
    hidden, state = [], []
    for t in range(max_frames):
        _, _, _, _, c, h = backward_unit(model_input[:, t, :], x_outputs_reverse[:, t, :], h, c, Pb)
        hidden.append(h)
        state.append(c)
    backward_state_outputs = gather_last(torch.stack(state, dim=1), num_frames)
    return forward_state_outputs, backward_state_outputs, x_outputs_reverse, torch.stack(hidden, dim=1)


def model_forward(model_input, num_frames, Pf, Pb, Wg, We, be, M):
    """LstmBigluModel's predictions: sub_moe on concat(c1, c2)."""
    c1, c2, _, _ = model_states(model_input, num_frames, Pf, Pb)
    return moe(torch.cat([c1, c2], dim=1), Wg, We, be, M)


def layer_with_grads(x_tm, num_frames, Pf, Pb, dy, dout2, dc1, dc2, dtype):
    """Both passes on time-major frames x_tm [F,B,D] (numpy) in `dtype`: y, out2 [F,B,H], c1_last, c2_last [B,H], dx [F,B,D] and the
    28 parameter gradients ("dfw/<name>", "dbw/<name>") for the loss sum(y dy) + sum(out2 dout2) + sum(c1_last dc1) + sum(c2_last dc2)."""
    x = torch.from_numpy(np.asarray(x_tm)).to(dtype).transpose(0, 1).clone().requires_grad_(True)
    Pft, Pbt = to_torch(Pf, dtype, True), to_torch(Pb, dtype, True)
    c1, c2, y, out2 = model_states(x, torch.from_numpy(np.asarray(num_frames)), Pft, Pbt)
    t = lambda a: torch.from_numpy(a).to(dtype)
    loss = (y.transpose(0, 1) * t(dy)).sum() + (out2.transpose(0, 1) * t(dout2)).sum() + (c1 * t(dc1)).sum() + (c2 * t(dc2)).sum()
    loss.backward()
    res = {"y": y.detach().transpose(0, 1).numpy(), "out2": out2.detach().transpose(0, 1).numpy(), "c1_last": c1.detach().numpy(),
           "c2_last": c2.detach().numpy(), "dx": x.grad.transpose(0, 1).numpy()}
    res.update({"dfw/" + n: Pft[n].grad.numpy() for n in NAMES_FW})
    res.update({"dbw/" + n: Pbt[n].grad.numpy() for n in NAMES_BW})
    return res


def by_operand(res, with_dx=True):
    """layer_with_grads' result keyed as the op's returns and operands: y, out2, c1_last, c2_last, [dx,] dWv .. dUs2."""
    out = {k: res[k] for k in ("y", "out2", "c1_last", "c2_last") + (("dx",) if with_dx else ())}
    out.update(operand_grads({n: res["dfw/" + n] for n in NAMES_FW}, {n: res["dbw/" + n] for n in NAMES_BW}))
    return out


def _reverse_tm(x, num_frames):
    return reverse_sequence(x.transpose(0, 1), num_frames).transpose(0, 1)


def recurrence_with_grads(zv, zs, Uv, Us, num_frames, reverse, dy, dc_last, dtype):
    """One pass on GIVEN hoisted inputs in FRAME order (what the C ABI takes): zv [F,B,2H], zs [F,B,2], Uv [H,2H], Us [2,H]; dy [F,B,H]
    (w.r.t. y, frame order) or None, dc_last [B,H] or None.  With `reverse` the pass runs over reverse_sequence copies of zv and zs and
    everything time-indexed but cs is reversed back.  Returns, in frame order, o, g [F,B,H], i, f [F,B], y (the step's new h), hprev
    (the h it came from) [F,B,H]; cs [F+1,B,H] in STEP order; c_last [B,H]; dzv [F,B,2H], dzs [F,B,2] (zeros when neither gradient is
    given), all in `dtype` as numpy."""
    nf = np.asarray(num_frames)
    zv_t = torch.from_numpy(zv).to(dtype).clone().requires_grad_(True)
    zs_t = torch.from_numpy(zs).to(dtype).clone().requires_grad_(True)
    Uv_t, Us_t = torch.from_numpy(Uv).to(dtype), torch.from_numpy(Us).to(dtype)
    F, B, H2 = zv.shape
    H = H2 // 2
    zv_s, zs_s = (_reverse_tm(zv_t, nf), _reverse_tm(zs_t, nf)) if reverse else (zv_t, zs_t)
    h = c = torch.zeros((B, H), dtype=dtype)
    hs, cs, og, sg = [h], [c], [], []
    for t in range(F):
        s = torch.sigmoid(zs_s[t] + h @ Us_t.t())
        v = zv_s[t] + h @ Uv_t
        o, g = torch.sigmoid(v[:, :H]), torch.tanh(v[:, H:])
        c = s[:, 1:2] * c + s[:, 0:1] * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        og.append(torch.cat([o, g], dim=1))
        sg.append(s)
    hs, cs, og, sg = torch.stack(hs), torch.stack(cs), torch.stack(og), torch.stack(sg)
    back = (lambda a: _reverse_tm(a, nf)) if reverse else (lambda a: a)
    y, hprev, og, sg = back(hs[1:]), back(hs[:-1]), back(og), back(sg)
    c_last = gather_last(cs[1:].transpose(0, 1), torch.from_numpy(nf))
    loss = 0.0
    if dy is not None:
        loss = loss + (y * torch.from_numpy(dy).to(dtype)).sum()
    if dc_last is not None:
        loss = loss + (c_last * torch.from_numpy(dc_last).to(dtype)).sum()
    if torch.is_tensor(loss):
        loss.backward()
    n = lambda a: a.detach().numpy()
    return {"o": n(og[:, :, :H]), "g": n(og[:, :, H:]), "i": n(sg[:, :, 0]), "f": n(sg[:, :, 1]), "y": n(y), "hprev": n(hprev), "cs": n(cs),
            "c_last": n(c_last), "dzv": n(zv_t.grad) if zv_t.grad is not None else np.zeros(zv.shape),
            "dzs": n(zs_t.grad) if zs_t.grad is not None else np.zeros(zs.shape)}
