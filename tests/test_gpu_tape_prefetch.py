"""-m gpu: the tape prefetch of the f16-form backward recurrence (csrc/lstm_persist.hip lstm_persist_bwd_kernel<.., H2, TPF>: throw-away
scalar loads that warm the saved-activation lines of the next step in L2) touches no value on the data path, so a launch with it
(yt8m_lstm_persist_set_tape_prefetch(1)) and without it (2) must agree BITWISE: dz and the final dh / dc of the direct entry point, and
through the LSTM stack the outputs, final states, dx and every weight and bias gradient.  The switch is per LAUNCHING thread, so the stack's
backward runs with autograd's worker threads off, and every comparison first proves from the library's launch counters that the two runs took
different kernels.  Shapes: pad rows in the last 16-row tile (B = 40: three tiles, B = 50: four), the headline's geometry (B = 128, H = 1024), launches of 1, 2, 3 steps and longer ones, a part
with t0 > 0 beside a neighbouring part's tape, a null and a non-null dout."""
import ctypes

import pytest
import torch

import yt8m_amd._lib as _lib
import yt8m_amd.seq_ops as seq_ops
from yt8m_amd.ops import _p, _stream
from yt8m_amd.variables import reset_default_graph, xavier_uniform, zeros

pytestmark = pytest.mark.gpu


class _Arm:
    """The calling thread's launches with the prefetch on (1) or off (2); the default again afterwards."""

    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        _lib.check(self.lib.yt8m_lstm_persist_set_tape_prefetch(self.mode))

    def __exit__(self, *exc):
        _lib.check(self.lib.yt8m_lstm_persist_set_tape_prefetch(0))


class _BwdCus:
    """CU budget of the following backward launches (32 CUs: one row group at H = 512, so that B = 50 -- four tiles per workgroup --
    takes the rotated epilogue and with it the f16 form and the prefetch)."""

    def __init__(self, lib, cus):
        self.lib, self.cus = lib, cus

    def __enter__(self):
        self.f, self.b = ctypes.c_int(-1), ctypes.c_int(-1)
        _lib.check(self.lib.yt8m_lstm_persist_get_cus(ctypes.byref(self.f), ctypes.byref(self.b)))
        if self.cus is not None:
            _lib.check(self.lib.yt8m_lstm_persist_set_cus(self.f.value, self.cus))

    def __exit__(self, *exc):
        _lib.check(self.lib.yt8m_lstm_persist_set_cus(self.f.value, self.b.value))


def _launches(lib):
    """(f16-form backward launches with the prefetch, without it) of the process so far."""
    w, wo = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.yt8m_lstm_persist_tape_prefetch_launches(ctypes.byref(w), ctypes.byref(wo)))
    return w.value, wo.value


def _counted(lib, mode, f16, fn):
    """fn() under arm `mode`; asserts that its f16-form backward launches, if the shape has any, all ran that arm's kernel."""
    w0, wo0 = _launches(lib)
    with _Arm(lib, mode):
        res = fn()
    w1, wo1 = _launches(lib)
    took, other = (w1 - w0, wo1 - wo0) if mode == 1 else (wo1 - wo0, w1 - w0)
    assert other == 0
    assert (took > 0) == bool(f16)
    return res


def _tape(dev, B, F, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    gates = torch.rand((F, B, 4 * H), device=dev, generator=g)
    gates[:, :, H:2 * H] = gates[:, :, H:2 * H] * 2 - 1                     # the tanh gate
    Wh = (torch.rand((H, 4 * H), device=dev, generator=g) - 0.5) * 0.08
    cs = torch.randn((F + 1, B, H), device=dev, generator=g) * 0.7
    dout = torch.randn((F, B, H), device=dev, generator=g) * 0.01
    nf = torch.randint(1, F + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    nf[0], nf[1] = F, 1
    word = torch.zeros(64, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().yt8m_h2_absmax(_p(Wh), H, 4 * H, 4 * H, _p(word), _stream()))
    return gates, Wh, cs, dout, nf, word


def _bwd(lib, tape, with_dout, t0, T):
    gates, Wh, cs, dout, nf, word = tape
    F, B, H4 = gates.shape
    H = H4 // 4
    dev = gates.device
    dz = torch.zeros((F, B, 4 * H), device=dev)
    work = torch.zeros((4, B, H), device=dev)
    g = torch.Generator(device=dev).manual_seed(99)
    work[0] = torch.randn((B, H), device=dev, generator=g) * 0.02          # running (dh, dc) handed in by the caller
    work[1] = torch.randn((B, H), device=dev, generator=g) * 0.02
    pws = torch.zeros(lib.yt8m_lstm_persist_workspace_bytes_steps(B, H, T), dtype=torch.uint8, device=dev)
    _lib.check(lib.yt8m_lstm_persist_bwd_h2(_p(gates), _p(Wh), 4 * H, _p(cs), _p(dout) if with_dout else None, _p(dz), _p(work), 0, None,
                                            _p(nf), t0, T, B, H, _p(word), _p(pws), pws.numel(), _stream()))
    torch.cuda.synchronize()
    _lib.check(lib.yt8m_lstm_persist_status(_p(pws), _stream()))
    return dz, work


_TAPES = {}


def _shared_tape(dev, B, F, H):
    key = (B, F, H)
    if key not in _TAPES:
        _TAPES[key] = _tape(dev, B, F, H, seed=11 + B)
    return _TAPES[key]


# (B, H, F, backward CU budget or None, takes the f16 form)
_SHAPES = [(40, 512, 9, None, False), (50, 512, 12, None, False), (50, 512, 12, 32, True), (128, 1024, 16, None, True)]
# (t0, T): one, two, three steps, the whole tape (longer than PF_DIST + 2), a middle part with a neighbour's tape on either side
_PARTS = [(0, 1), (0, 2), (3, 3), (0, None), (2, 6)]


@pytest.mark.parametrize("with_dout", [True, False], ids=["dout", "no-dout"])
@pytest.mark.parametrize("t0,T", _PARTS)
@pytest.mark.parametrize("B,H,F,cus,f16", _SHAPES)
def test_backward_launch_is_bitwise_the_same_with_and_without_the_prefetch(dev, B, H, F, cus, f16, t0, T, with_dout):
    lib = _lib.lib()
    T = F - t0 if T is None else T
    tape = _shared_tape(dev, B, F, H)
    with _BwdCus(lib, cus):
        assert lib.yt8m_lstm_persist_bwd_on_f16_pipe(B, H) == (1 if f16 else 0)   # the shapes that reach the kernel with the prefetch
        dz0, w0 = _counted(lib, 2, f16, lambda: _bwd(lib, tape, with_dout, t0, T))
        dz1, w1 = _counted(lib, 1, f16, lambda: _bwd(lib, tape, with_dout, t0, T))
    assert float(dz0[t0:t0 + T].abs().max()) > 0
    assert torch.equal(dz0, dz1)                                           # (steps outside the part stay zero in both)
    assert torch.equal(w0, w1)                                             # final dh / dc


def test_the_setter_refuses_other_modes():
    lib = _lib.lib()
    assert lib.yt8m_lstm_persist_set_tape_prefetch(3) != 0
    assert lib.yt8m_lstm_persist_set_tape_prefetch(-1) != 0
    _lib.check(lib.yt8m_lstm_persist_set_tape_prefetch(0))


def _stack(dev, B, F, D, H, L, nf):
    g = reset_default_graph(device=dev, seed=0)
    g.begin_step()
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand((F, B, D), device=dev, generator=gen) - 0.5
    wb, d_in = [], D
    for l in range(L):
        wb.append((g.get_variable("l%d/w" % l, (d_in + H, 4 * H), xavier_uniform), g.get_variable("l%d/b" % l, (4 * H,), zeros)))
        d_in = H
    g.finalize()
    x.requires_grad_(True)
    out, finals = seq_ops.lstm_stack(x, nf, wb, chunks=1)
    res = [out] + [t for p in finals for t in p]
    gen2 = torch.Generator(device=dev).manual_seed(7)
    sum((r * torch.rand(r.shape, device=dev, generator=gen2)).sum() for r in res).backward()   # a non-null dout and final-state gradients
    torch.cuda.synchronize()
    return [r.detach().clone() for r in res] + [x.grad.clone(), g.grads.clone()]      # g.grads: every weight and bias gradient


@pytest.mark.parametrize("B,F,D,H,L,cus,f16", [(40, 12, 96, 512, 2, None, False), (50, 24, 96, 512, 2, 32, True), (128, 16, 128, 1024, 2, None, True)])
def test_lstm_stack_gradients_are_bitwise_the_same_with_and_without_the_prefetch(dev, B, F, D, H, L, cus, f16):
    """The product's own partition: one forward launch per layer, three backward parts (two of them with t0 > 0); ragged num_frames.
    autograd would run the stack's backward -- the launches under test -- on its device worker thread, which the per-thread switch set
    here does not reach: with multithreading off it runs them on this thread.  B = 50 takes the f16 form (pad rows in its last tile) on a
    32-CU backward budget -- with F = 24, because only the native stack asks for the f16 form and it wants every backward part to be a
    multiple of 16 frame rows (three parts of 8 steps x 50 rows); B = 40 (three tiles) never takes it and compares the fp32-pipe form with
    itself."""
    lib = _lib.lib()
    nf = torch.randint(0, F + 1, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(3), dtype=torch.int32)
    nf[0], nf[1] = F, 0
    with _BwdCus(lib, cus), torch.autograd.set_multithreading_enabled(False):
        assert lib.yt8m_lstm_persist_bwd_on_f16_pipe(B, H) == (1 if f16 else 0)
        off = _counted(lib, 2, f16, lambda: _stack(dev, B, F, D, H, L, nf))
        on = _counted(lib, 1, f16, lambda: _stack(dev, B, F, D, H, L, nf))
    assert float(off[-1].abs().max()) > 0
    for a, b in zip(off, on):
        assert torch.equal(a, b)
