"""One step of each recurrent cell of the per-step kernels (csrc/sequence.hip, lstm_fused.hip, lstm_bf16.hip, cells.hip), forward and
backward, written out in plain torch for a given dtype, with the quantities the C ABI stores: the activated gates over z, rh and the
dzg / dzc split of the GRU, stats / dyb / dyg of the LayerNorm-LSTM with the philox dropout mask of oracle/philox.py.  The loops over
steps apply the num_frames copy-through (state carried, out = 0, dz = 0, (dh, dc) carried) and the (dh, dc) phase convention of
`work` [4, B, H]: the running gradients sit in work[0], work[1] when phase is 0 and in work[2], work[3] when it is 1; every step flips it.

tests/test_step_restatement_host.py ties F steps of each cell in fp64 to oracle/torch_ref.py (values and autograd gradients) and to
oracle/np_ref.py; tests/test_gpu_step_branches.py holds the kernels to these functions in fp64 and takes its bounds from the same
functions in float32."""
import numpy as np
import torch

from oracle import philox

LN_EPS = 1e-12


def T(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dt)


def bf16r(t):
    """round to nearest even to bf16 and back, in t's dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def live_rows(nf, t, B):
    return torch.ones(B, dtype=torch.bool) if nf is None else torch.as_tensor(np.asarray(nf) > t)


def err(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def bound(ref64, ref32, floor):
    """EIGHT times the float32 restatement's error against the float64 one, never below the floor"""
    return max(floor, 8.0 * err(ref32, ref64))


# ---- BasicLSTM -------------------------------------------------------------------------------------------------------------------------
def lstm_step_fwd(z, Wh, c, h, live, fb, bf16=False):
    """-> pre (z + h . Wh), gates (activated i|j|f|o), c_new, h_new, out; the last three with the copy-through applied"""
    pre = z + (bf16r(h) @ bf16r(Wh) if bf16 else h @ Wh)
    i, j, f, o = pre.chunk(4, 1)
    gi, gj, gf, go = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + fb), torch.sigmoid(o)
    cn = c * gf + gi * gj
    hn = torch.tanh(cn) * go
    m = live[:, None]
    return pre, torch.cat([gi, gj, gf, go], 1), torch.where(m, cn, c), torch.where(m, hn, h), torch.where(m, hn, torch.zeros_like(hn))


def lstm_gates_bwd(gates, c_prev, c_new, dh, dc, dout, live):
    """the pointwise half of a backward step -> dz, dc_prev, the part of dh_prev that is not the product (0, or dh carried)"""
    i, j, f, o = gates.chunk(4, 1)
    tc = torch.tanh(c_new)
    dht = dh if dout is None else dh + dout
    dct = dc + dht * o * (1 - tc * tc)
    dz = torch.cat([dct * j * i * (1 - i), dct * i * (1 - j * j), dct * c_prev * f * (1 - f), dht * tc * o * (1 - o)], 1)
    m = live[:, None]
    zero = torch.zeros_like(dh)
    return torch.where(m, dz, torch.zeros_like(dz)), torch.where(m, dct * f, dc), torch.where(m, zero, dh)


def lstm_step_bwd(gates, c_prev, c_new, dh, dc, dout, Wh, live, bf16=False):
    """-> dz, dc_prev, dh_prev = carried part + dz . Wh^T"""
    dz, dcp, dhp = lstm_gates_bwd(gates, c_prev, c_new, dh, dc, dout, live)
    return dz, dcp, dhp + (bf16r(dz) @ bf16r(Wh).t() if bf16 else dz @ Wh.t())


def lstm_range_fwd(z, Wh, cs, hs, nf, t0, n, fb, bf16=False):
    """steps [t0, t0 + n) from (cs[t0], hs[t0]); z [F, B, 4H] holds the hoisted input part.  -> dict of pre, gates, out over the range
    and the tapes cs, hs [n + 1] (slot 0 = the given state)"""
    B = z.shape[1]
    cs, hs, pre, gates, out = [cs[t0]], [hs[t0]], [], [], []
    for t in range(t0, t0 + n):
        p, g, c, h, o = lstm_step_fwd(z[t], Wh, cs[-1], hs[-1], live_rows(nf, t, B), fb, bf16)
        pre.append(p), gates.append(g), cs.append(c), hs.append(h), out.append(o)
    return {"pre": torch.stack(pre), "gates": torch.stack(gates), "out": torch.stack(out), "cs": torch.stack(cs), "hs": torch.stack(hs)}


def halves(phase):
    """(dh_cur, dc_cur, dh_prev, dc_prev) as indices into work [4, B, H]"""
    return (2, 3, 0, 1) if phase else (0, 1, 2, 3)


def lstm_range_bwd(gates, cs, Wh, dout, work, phase, nf, t0, n, bf16=False):
    """steps t0 + n - 1 down to t0 on a copy of `work` -> dz over the range [n, B, 4H], work, phase' = (phase + n) % 2"""
    B = gates.shape[1]
    work, dz = work.clone(), []
    for t in range(t0 + n - 1, t0 - 1, -1):
        hc, cc, hp, cp = halves(phase)
        d, work[cp], work[hp] = lstm_step_bwd(gates[t], cs[t], cs[t + 1], work[hc], work[cc], None if dout is None else dout[t], Wh,
                                              live_rows(nf, t, B), bf16)
        dz.insert(0, d)
        phase ^= 1
    return torch.stack(dz), work, phase


# ---- GRU -------------------------------------------------------------------------------------------------------------------------------
def gru_step_fwd(zg, zc, Wg, Wc, h, live):
    """-> ru (sigmoid, stored over zg), c (tanh, stored over zc), rh, h_new, out"""
    ru = torch.sigmoid(zg + h @ Wg)
    r, u = ru.chunk(2, 1)
    rh = r * h
    c = torch.tanh(zc + rh @ Wc)
    m = live[:, None]
    hn = torch.where(m, u * h + (1 - u) * c, h)
    return ru, c, rh, hn, torch.where(m, hn, torch.zeros_like(hn))


def gru_step_bwd(ru, c, h, dh_cur, dout, Wg, Wc, live):
    """-> dzg [B, 2H] (r | u), dzc [B, H], dh_prev"""
    r, u = ru.chunk(2, 1)
    m = live[:, None]
    zero = torch.zeros_like(h)
    dh = dh_cur if dout is None else dh_cur + dout
    dzu = torch.where(m, dh * (h - c) * u * (1 - u), zero)
    dzc = torch.where(m, dh * (1 - u) * (1 - c * c), zero)
    dhp = torch.where(m, dh * u, dh_cur)
    drh = dzc @ Wc.t()
    dzr = torch.where(m, drh * h * r * (1 - r), zero)
    dhp = dhp + torch.where(m, drh * r, zero)
    dzg = torch.cat([dzr, dzu], 1)
    return dzg, dzc, dhp + dzg @ Wg.t()


def gru_layer(zg, zc, Wg, Wc, nf, dout=None, dh_final=None, backward=True, h0=None):
    """F steps from h0 (zeros if not given) -> dict: zg, zc (activated), rh, hs [F + 1], out, and dzg, dzc, dh (the gradient that
    reaches h_0)"""
    F, B, H = zc.shape
    hs, ru, c, rh, out = [torch.zeros((B, H), dtype=zc.dtype) if h0 is None else h0], [], [], [], []
    for t in range(F):
        a, b, d, h, o = gru_step_fwd(zg[t], zc[t], Wg, Wc, hs[-1], live_rows(nf, t, B))
        ru.append(a), c.append(b), rh.append(d), hs.append(h), out.append(o)
    res = {"zg": torch.stack(ru), "zc": torch.stack(c), "rh": torch.stack(rh), "hs": torch.stack(hs), "out": torch.stack(out)}
    if backward:
        dh = torch.zeros((B, H), dtype=zc.dtype) if dh_final is None else dh_final
        dzg, dzc = [], []
        for t in range(F - 1, -1, -1):
            a, b, dh = gru_step_bwd(ru[t], c[t], hs[t], dh, None if dout is None else dout[t], Wg, Wc, live_rows(nf, t, B))
            dzg.insert(0, a), dzc.insert(0, b)
        res.update({"dzg": torch.stack(dzg), "dzc": torch.stack(dzc), "dh": dh})
    return res


# ---- LayerNormBasicLSTMCell ------------------------------------------------------------------------------------------------------------
def keep_scale(t, B, H, keep, seed, dt):
    """1 / keep where the philox mask of step t keeps the candidate, else 0 (ones at keep_prob 1): element (t B + b) H + h"""
    if keep >= 1.0:
        return torch.ones((B, H), dtype=dt)
    m = torch.from_numpy(philox.dropout_mask(B * H, keep, seed, offset=t * B * H)).view(B, H)
    return torch.where(m, torch.ones((), dtype=dt) / torch.tensor(keep, dtype=dt), torch.zeros((), dtype=dt))


def _ln(x, g, b):
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    n = (x - mean) * rstd
    return n * g + b, mean, rstd, n


def lnlstm_step_fwd(z, Wh, gamma, beta, c, h, live, fb, ks):
    """gamma, beta [5, H] (input, transform, forget, output, state).  -> zr (raw z + h . Wh, what the tape keeps), stats [B, 10]
    (mean, rstd of the four gates and of the state; defined on live rows only), c_new, h_new, out"""
    zr = z + h @ Wh
    y, st = [], []
    for k, v in enumerate(zr.chunk(4, 1)):
        yk, mean, rstd, _ = _ln(v, gamma[k], beta[k])
        y.append(yk), st.extend([mean, rstd])
    i, g, f, o = torch.sigmoid(y[0]), torch.tanh(y[1]) * ks, torch.sigmoid(y[2] + fb), torch.sigmoid(y[3])
    cn, mean, rstd, _ = _ln(c * f + i * g, gamma[4], beta[4])
    st.extend([mean, rstd])
    hn = torch.tanh(cn) * o
    m = live[:, None]
    return zr, torch.cat(st, 1), torch.where(m, cn, c), torch.where(m, hn, h), torch.where(m, hn, torch.zeros_like(hn))


def lnlstm_step_bwd(zr, Wh, gamma, beta, c_prev, c_new, dh_cur, dc_cur, dout, live, fb, ks):
    """-> dz [B, 4H] (w.r.t. the raw pre-activations), dyb, dyg [B, 5H], dc_prev, dh_prev"""
    n, y, rs = [], [], []
    for k, v in enumerate(zr.chunk(4, 1)):
        yk, _, rstd, nk = _ln(v, gamma[k], beta[k])
        y.append(yk), n.append(nk), rs.append(rstd)
    i, tj, f, o = torch.sigmoid(y[0]), torch.tanh(y[1]), torch.sigmoid(y[2] + fb), torch.sigmoid(y[3])
    g = tj * ks
    _, _, rstd_s, ns = _ln(c_prev * f + i * g, gamma[4], beta[4])
    tc = torch.tanh(c_new)
    dh = dh_cur if dout is None else dh_cur + dout
    dcn = dc_cur + dh * o * (1 - tc * tc)
    dns = dcn * gamma[4]
    dcp = rstd_s * (dns - dns.mean(1, keepdim=True) - ns * (dns * ns).mean(1, keepdim=True))
    dy = [dcp * g * i * (1 - i), dcp * i * ks * (1 - tj * tj), dcp * c_prev * f * (1 - f), dh * tc * o * (1 - o)]
    dz = []
    for k in range(4):
        dn = dy[k] * gamma[k]
        dz.append(rs[k] * (dn - dn.mean(1, keepdim=True) - n[k] * (dn * n[k]).mean(1, keepdim=True)))
    m = live[:, None]
    dz = torch.where(m, torch.cat(dz, 1), torch.zeros_like(zr))
    dyb = torch.cat(dy + [dcn], 1)
    dyg = torch.cat([dy[k] * n[k] for k in range(4)] + [dcn * ns], 1)
    dyb, dyg = torch.where(m, dyb, torch.zeros_like(dyb)), torch.where(m, dyg, torch.zeros_like(dyg))
    return dz, dyb, dyg, torch.where(m, dcp * f, dc_cur), torch.where(m, torch.zeros_like(dh), dh_cur) + dz @ Wh.t()


def lnlstm_layer(z, Wh, gamma, beta, nf, fb, keep, seed, dout=None, dc_final=None, dh_final=None, backward=True, c0=None, h0=None):
    """F steps from (c0, h0) (zeros if not given) -> dict: z (raw), stats, cs, hs [F + 1], out and dz, dyb, dyg, dh, dc"""
    F, B, H4 = z.shape
    H, dt = H4 // 4, z.dtype
    zero = torch.zeros((B, H), dtype=dt)
    cs, hs, zr, stats, out = [zero if c0 is None else c0], [zero if h0 is None else h0], [], [], []
    ks = [keep_scale(t, B, H, keep, seed, dt) for t in range(F)]
    for t in range(F):
        a, s, c, h, o = lnlstm_step_fwd(z[t], Wh, gamma, beta, cs[-1], hs[-1], live_rows(nf, t, B), fb, ks[t])
        zr.append(a), stats.append(s), cs.append(c), hs.append(h), out.append(o)
    res = {"z": torch.stack(zr), "stats": torch.stack(stats), "cs": torch.stack(cs), "hs": torch.stack(hs), "out": torch.stack(out)}
    if backward:
        dh = torch.zeros((B, H), dtype=dt) if dh_final is None else dh_final
        dc = torch.zeros((B, H), dtype=dt) if dc_final is None else dc_final
        dz, dyb, dyg = [], [], []
        for t in range(F - 1, -1, -1):
            a, b, g, dc, dh = lnlstm_step_bwd(zr[t], Wh, gamma, beta, cs[t], cs[t + 1], dh, dc, None if dout is None else dout[t],
                                              live_rows(nf, t, B), fb, ks[t])
            dz.insert(0, a), dyb.insert(0, b), dyg.insert(0, g)
        res.update({"dz": torch.stack(dz), "dyb": torch.stack(dyb), "dyg": torch.stack(dyg), "dh": dh, "dc": dc})
    return res
