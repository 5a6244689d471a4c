"""Not -m gpu: ties tests/step_restatement.py, the reference of tests/test_gpu_step_branches.py, to the project's oracle before anything
runs on a GPU.  F steps of each restatement in fp64 reproduce oracle/torch_ref.lstm_stack, gru_stack and lnlstm_stack -- values and
autograd gradients -- and oracle/np_ref.dynamic_rnn_lstm to 1e-12, on ragged lengths holding 0, 1 and F.

The oracle takes frames x and weights [x | h] -> gates; the restatement takes the hoisted input part z.  With the input rows of the
weight matrix set to the identity, x[:, t] IS z[t] and the autograd gradient of x IS dz; the gradient of the recurrent rows is
sum_t h_{t-1}^T dz_t, and those of gamma / beta are the column sums of dyg / dyb."""
import numpy as np
import torch

import step_restatement as R
from oracle import np_ref, torch_ref

F, B, H = 5, 6, 7
NF = np.array([F, 0, 1, 3, 2, F], dtype=np.int32)
TOL = 1e-12
DT = torch.float64


def _close(name, a, b):
    e = float((torch.as_tensor(a) - torch.as_tensor(b)).abs().max())
    assert e <= TOL, (name, e)


def _rand(rs, *shape):
    return torch.from_numpy(rs.randn(*shape))


def test_lstm_steps_reproduce_the_oracle_and_its_gradients():
    rs = np.random.RandomState(1)
    Wh = _rand(rs, H, 4 * H) * 0.6
    x = _rand(rs, B, F, 4 * H).requires_grad_(True)
    W = torch.cat([torch.eye(4 * H, dtype=DT), Wh], 0).requires_grad_(True)
    dout, dcf, dhf = _rand(rs, F, B, H), _rand(rs, B, H), _rand(rs, B, H)
    nf = torch.from_numpy(NF)
    for fb in (1.0, 0.0):
        x.grad = W.grad = None
        outs, c, h = torch_ref.lstm_stack(x, nf, [(W, torch.zeros(4 * H, dtype=DT))], forget_bias=fb)
        ((outs.transpose(0, 1) * dout).sum() + (c[0] * dcf).sum() + (h[0] * dhf).sum()).backward()
        z = x.detach().transpose(0, 1).contiguous()
        zero = torch.zeros((F + 1, B, H), dtype=DT)
        f = R.lstm_range_fwd(z, Wh, zero, zero, NF, 0, F, fb)
        _close("out", f["out"], outs.detach().transpose(0, 1))
        _close("c", f["cs"][F], c[0].detach())
        _close("h", f["hs"][F], h[0].detach())
        work = torch.zeros((4, B, H), dtype=DT)
        work[0], work[1] = dhf, dcf
        dz, work2, phase = R.lstm_range_bwd(f["gates"], f["cs"], Wh, dout, work, 0, NF, 0, F)
        assert phase == F % 2
        _close("dz", dz, x.grad.transpose(0, 1))
        _close("dWh", sum(f["hs"][t].t() @ dz[t] for t in range(F)), W.grad[4 * H:])
        # two ranges with the carried phase give the same as one; a row without frames carries (dh, dc) through unchanged
        dz_b, work_b, pb = R.lstm_range_bwd(f["gates"], f["cs"], Wh, dout, work, 0, NF, 3, 2)
        dz_a, work_a, pa = R.lstm_range_bwd(f["gates"], f["cs"], Wh, dout, work_b, pb, NF, 0, 3)
        _close("dz, two ranges", torch.cat([dz_a, dz_b]), dz)
        hc, cc = R.halves(pa)[:2]
        _close("dh", work_a[hc], work2[R.halves(phase)[0]])
        assert torch.equal(work_a[hc][1], dhf[1]) and torch.equal(work_a[cc][1], dcf[1])
        # entered with phase 1: the same values from the other half
        w1 = torch.zeros((4, B, H), dtype=DT)
        w1[2], w1[3] = dhf, dcf
        dz1, w1b, p1 = R.lstm_range_bwd(f["gates"], f["cs"], Wh, dout, w1, 1, NF, 0, F)
        assert p1 == (1 + F) % 2 and torch.equal(dz1, dz) and torch.equal(w1b[R.halves(p1)[0]], work2[R.halves(phase)[0]])
        # the numpy oracle
        o_np, st = np_ref.dynamic_rnn_lstm(x.detach().numpy(), NF, [(W.detach().numpy(), np.zeros(4 * H))], forget_bias=fb)
        _close("np out", f["out"], torch.from_numpy(o_np).transpose(0, 1))
        _close("np c", f["cs"][F], torch.from_numpy(st[0][0]))
        _close("np h", f["hs"][F], torch.from_numpy(st[0][1]))


def test_bf16_lstm_steps_reproduce_the_oracles_operand_rounding():
    rs = np.random.RandomState(2)
    Wh = _rand(rs, H, 4 * H) * 0.6
    # x and the identity are exact in bf16, so rounding [x | h] and W rounds h and W_h only
    x = R.bf16r(_rand(rs, B, F, 4 * H))
    W = torch.cat([torch.eye(4 * H, dtype=DT), Wh], 0)
    outs, c, h = torch_ref.lstm_stack(x, torch.from_numpy(NF), [(W, torch.zeros(4 * H, dtype=DT))], bf16_operands=True)
    zero = torch.zeros((F + 1, B, H), dtype=DT)
    f = R.lstm_range_fwd(x.transpose(0, 1).contiguous(), Wh, zero, zero, NF, 0, F, 1.0, bf16=True)
    _close("out", f["out"], outs.transpose(0, 1))
    _close("c", f["cs"][F], c[0])
    plain = R.lstm_range_fwd(x.transpose(0, 1).contiguous(), Wh, zero, zero, NF, 0, F, 1.0)
    assert float((plain["out"] - f["out"]).abs().max()) > 1e-5           # the rounding is not a no-op


def test_gru_steps_reproduce_the_oracle_and_its_gradients():
    rs = np.random.RandomState(3)
    Wg_h, Wc_h = _rand(rs, H, 2 * H) * 0.6, _rand(rs, H, H) * 0.6
    x = _rand(rs, B, F, 3 * H).requires_grad_(True)
    eye = torch.eye(3 * H, dtype=DT)
    Wg = torch.cat([eye[:, :2 * H], Wg_h], 0).requires_grad_(True)
    Wc = torch.cat([eye[:, 2 * H:], Wc_h], 0).requires_grad_(True)
    dout, dhf = _rand(rs, F, B, H), _rand(rs, B, H)
    outs, h = torch_ref.gru_stack(x, torch.from_numpy(NF), [(Wg, torch.zeros(2 * H, dtype=DT), Wc, torch.zeros(H, dtype=DT))])
    ((outs.transpose(0, 1) * dout).sum() + (h[0] * dhf).sum()).backward()
    z = x.detach().transpose(0, 1)
    r = R.gru_layer(z[:, :, :2 * H].contiguous(), z[:, :, 2 * H:].contiguous(), Wg_h, Wc_h, NF, dout, dhf)
    _close("out", r["out"], outs.detach().transpose(0, 1))
    _close("h", r["hs"][F], h[0].detach())
    _close("dzg", r["dzg"], x.grad.transpose(0, 1)[:, :, :2 * H])
    _close("dzc", r["dzc"], x.grad.transpose(0, 1)[:, :, 2 * H:])
    _close("dWg_h", sum(r["hs"][t].t() @ r["dzg"][t] for t in range(F)), Wg.grad[3 * H:])
    _close("dWc_h", sum(r["rh"][t].t() @ r["dzc"][t] for t in range(F)), Wc.grad[3 * H:])
    assert torch.equal(r["dh"][1], dhf[1])                               # no frames: the final-state gradient is carried through


def test_lnlstm_steps_reproduce_the_oracle_and_its_gradients():
    rs = np.random.RandomState(4)
    Wh = _rand(rs, H, 4 * H) * 0.6
    W = torch.cat([torch.eye(4 * H, dtype=DT), Wh], 0).requires_grad_(True)
    dout, dcf, dhf = _rand(rs, F, B, H), _rand(rs, B, H), _rand(rs, B, H)
    for keep, fb in ((1.0, 1.0), (0.75, 0.0)):
        x = _rand(rs, B, F, 4 * H).requires_grad_(True)
        W.grad = None
        ga = [(1.0 + 0.3 * _rand(rs, H)).requires_grad_(True) for _ in range(5)]
        be = [(0.3 * _rand(rs, H)).requires_grad_(True) for _ in range(5)]
        outs, c, h = torch_ref.lnlstm_stack(x, torch.from_numpy(NF), [(W, ga, be)], forget_bias=fb,
                                            dropout_spec=None if keep >= 1.0 else (keep, [77]))
        ((outs.transpose(0, 1) * dout).sum() + (c[0] * dcf).sum() + (h[0] * dhf).sum()).backward()
        gamma, beta = torch.stack([g.detach() for g in ga]), torch.stack([b.detach() for b in be])
        r = R.lnlstm_layer(x.detach().transpose(0, 1).contiguous(), Wh, gamma, beta, NF, fb, keep, 77, dout, dcf, dhf)
        _close("out", r["out"], outs.detach().transpose(0, 1))
        _close("c", r["cs"][F], c[0].detach())
        _close("h", r["hs"][F], h[0].detach())
        _close("dz", r["dz"], x.grad.transpose(0, 1))
        _close("dWh", sum(r["hs"][t].t() @ r["dz"][t] for t in range(F)), W.grad[4 * H:])
        for k in range(5):
            _close("dgamma %d" % k, r["dyg"][:, :, k * H:(k + 1) * H].sum((0, 1)), ga[k].grad)
            _close("dbeta %d" % k, r["dyb"][:, :, k * H:(k + 1) * H].sum((0, 1)), be[k].grad)
        assert torch.equal(r["dh"][1], dhf[1]) and torch.equal(r["dc"][1], dcf[1])
        if keep < 1.0:                                                    # the mask dropped some candidates and kept others
            ks = torch.stack([R.keep_scale(t, B, H, keep, 77, DT) for t in range(F)])
            assert 0 < int((ks == 0).sum()) < ks.numel()
