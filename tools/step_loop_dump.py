"""sha256 of every output of the per-step recurrence entry points (csrc/sequence.hip, cells.hip, lstm_bf16.hip) from fixed seeds, at
the shapes of tests/test_gpu_step_loops.py: for comparing two builds of the library byte for byte (YT8M_LIB=<other build>).
usage: python tools/step_loop_dump.py > A.txt ; YT8M_LIB=... python tools/step_loop_dump.py > B.txt ; diff A.txt B.txt"""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
import yt8m_amd._lib as L  # noqa: E402
from yt8m_amd import ops  # noqa: E402

F = 5
dev = torch.device("cuda:0")
lib = L.lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def show(case, **arrays):
    torch.cuda.synchronize()
    for name, t in arrays.items():
        print("%-28s %-8s %s" % (case, name, hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()))


def inputs(B, H, G):
    """z [F,B,G*H], Wh [H,G*H], ragged num_frames holding 0, 1 and F, gradients of the outputs and of the final state."""
    g = torch.Generator(device=dev).manual_seed(1000 * B + H + G)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)  # noqa: E731
    nf = torch.randint(0, F + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    nf[0], nf[1], nf[2] = F, 0, 1
    Wh = (torch.rand((H, G * H), device=dev, generator=g) - 0.5) * (2.0 / H ** 0.5)
    return rnd(F, B, G * H) * 0.8, Wh, nf, rnd(F, B, H), rnd(B, H), rnd(B, H)


def zeros(*shape, **kw):
    return torch.zeros(shape, device=dev, **kw)


def lstm(B, H):
    case = "lstm B=%d H=%d" % (B, H)
    z0, Wh, nf, dout, dcf, dhf = inputs(B, H, 4)
    ws = ops._workspace(dev)
    wsb = ws.numel() * 4
    z, cs, hs, out = z0.clone(), zeros(F + 1, B, H), zeros(F + 1, B, H), zeros(F, B, H)
    L.check(lib.yt8m_lstm_layer_fwd(_p(z), _p(Wh), 4 * H, _p(cs), _p(hs), _p(out), _p(nf), F, B, H, 1.0, _p(ws), wsb, _st()))
    show(case + " layer_fwd", z=z, cs=cs, hs=hs, out=out)
    dz, work = zeros(F, B, 4 * H), zeros(4, B, H)
    L.check(lib.yt8m_lstm_layer_bwd(_p(z), _p(Wh), 4 * H, _p(cs), _p(dout), _p(dcf), _p(dhf), _p(dz), _p(work), _p(nf), F, B, H, _p(ws), wsb, _st()))
    show(case + " layer_bwd", dz=dz, work=work)
    Wp = Wq = None
    if lib.yt8m_lstm_packed_floats(B, H):
        Wp, Wq = zeros(H * 4 * H), zeros(H * 4 * H)
        L.check(lib.yt8m_lstm_pack(_p(Wh), 4 * H, H, _p(Wp), _p(Wq), _st()))
    z2, cs2, hs2, out2 = z0.clone(), zeros(F + 1, B, H), zeros(F + 1, B, H), zeros(F, B, H)
    for t0, T in ((0, 2), (2, 3)):
        L.check(lib.yt8m_lstm_steps_fwd(_p(z2), _p(Wh), 4 * H, _p(Wp), _p(cs2), _p(hs2), _p(out2), _p(nf), t0, T, B, H, 1.0, _p(ws), wsb, _st()))
    show(case + " steps_fwd", z=z2, cs=cs2, hs=hs2, out=out2)
    dz2, work2, phase = zeros(F, B, 4 * H), zeros(4, B, H), 0
    work2[0], work2[1] = dhf, dcf
    for t0, T in ((3, 2), (0, 3)):
        L.check(lib.yt8m_lstm_steps_bwd(_p(z2), _p(Wh), 4 * H, _p(Wq), _p(cs2), _p(dout), _p(dz2), _p(work2), phase, _p(nf), t0, T, B, H,
                                        _p(ws), wsb, _st()))
        phase = (phase + T) % 2
    show(case + " steps_bwd", dz=dz2, work=work2)


def lstm_bf16(B, H):
    case = "lstm_bf16 B=%d H=%d" % (B, H)
    z0, Wh, nf, dout, dcf, dhf = inputs(B, H, 4)
    Wp16, Wq16 = zeros(H * 4 * H, dtype=torch.bfloat16), zeros(H * 4 * H, dtype=torch.bfloat16)
    L.check(lib.yt8m_lstm_pack_bf16(_p(Wh), 4 * H, H, _p(Wp16), _p(Wq16), _st()))
    z, cs, hs, out, hs16 = z0.clone(), zeros(F + 1, B, H), zeros(F + 1, B, H), zeros(F, B, H), zeros(F + 1, B, H, dtype=torch.bfloat16)
    for t0, T in ((0, 2), (2, 3)):
        L.check(lib.yt8m_lstm_steps_fwd_bf16(_p(z), _p(Wp16), _p(cs), _p(hs), _p(hs16), _p(out), _p(nf), t0, T, B, H, 1.0, _st()))
    show(case + " steps_fwd_bf16", z=z, cs=cs, hs=hs, hs16=hs16, out=out)
    dz, dz16, work, phase = zeros(F, B, 4 * H), zeros(F, B, 4 * H, dtype=torch.bfloat16), zeros(4, B, H), 0
    work[0], work[1] = dhf, dcf
    for t0, T in ((3, 2), (0, 3)):
        L.check(lib.yt8m_lstm_steps_bwd_bf16(_p(z), _p(Wq16), _p(cs), _p(dout), _p(dz), _p(dz16), _p(work), phase, _p(nf), t0, T, B, H, _st()))
        phase = (phase + T) % 2
    show(case + " steps_bwd_bf16", dz=dz, dz16=dz16, work=work)


def gru(B, H):
    case = "gru B=%d H=%d" % (B, H)
    zg, Wg, nf, dout, _, dhf = inputs(B, H, 2)
    zc, Wc = inputs(B, H, 1)[:2]
    ws = ops._workspace(dev)
    wsb = ws.numel() * 4
    hs, rh, out = zeros(F + 1, B, H), zeros(F, B, H), zeros(F, B, H)
    L.check(lib.yt8m_gru_layer_fwd(_p(zg), _p(zc), _p(Wg), 2 * H, _p(Wc), H, _p(hs), _p(rh), _p(out), _p(nf), F, B, H, _p(ws), wsb, _st()))
    show(case + " layer_fwd", zg=zg, zc=zc, hs=hs, rh=rh, out=out)
    dzg, dzc, work = zeros(F, B, 2 * H), zeros(F, B, H), zeros(3, B, H)
    L.check(lib.yt8m_gru_layer_bwd(_p(zg), _p(zc), _p(Wg), 2 * H, _p(Wc), H, _p(hs), _p(dout), _p(dhf), _p(dzg), _p(dzc), _p(work), _p(nf),
                                   F, B, H, _p(ws), wsb, _st()))
    show(case + " layer_bwd", dzg=dzg, dzc=dzc, work=work)


def lnlstm(B, H):
    case = "lnlstm B=%d H=%d" % (B, H)
    z0, Wh, nf, dout, dcf, dhf = inputs(B, H, 4)
    g = torch.Generator(device=dev).manual_seed(7)
    gamma = 1.0 + 0.1 * torch.randn((5, H), device=dev, generator=g)
    beta = 0.1 * torch.randn((5, H), device=dev, generator=g)
    ws = ops._workspace(dev)
    wsb = ws.numel() * 4
    z, stats, cs, hs, out = z0.clone(), zeros(F, B, 10), zeros(F + 1, B, H), zeros(F + 1, B, H), zeros(F, B, H)
    L.check(lib.yt8m_lnlstm_layer_fwd(_p(z), _p(Wh), 4 * H, _p(gamma), _p(beta), _p(stats), _p(cs), _p(hs), _p(out), _p(nf), F, B, H,
                                      1.0, 0.8, 12345, _p(ws), wsb, _st()))
    show(case + " layer_fwd", z=z, stats=stats, cs=cs, hs=hs, out=out)
    dz, dyb, dyg, work = zeros(F, B, 4 * H), zeros(F, B, 5 * H), zeros(F, B, 5 * H), zeros(4, B, H)
    L.check(lib.yt8m_lnlstm_layer_bwd(_p(z), _p(Wh), 4 * H, _p(gamma), _p(beta), _p(stats), _p(cs), _p(dout), _p(dcf), _p(dhf), _p(dz),
                                      _p(dyb), _p(dyg), _p(work), _p(nf), F, B, H, 1.0, 0.8, 12345, _p(ws), wsb, _st()))
    show(case + " layer_bwd", dz=dz, dyb=dyb, dyg=dyg, work=work)


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream(dev)):     # (the legacy default stream cannot be captured: the time-range forms would issue directly)
        lstm(33, 128)          # packed
        lstm(5, 12)            # generic
        lstm_bf16(33, 256)
        for cell in (gru, lnlstm):
            cell(33, 256)      # packed
            cell(5, 12)        # generic
