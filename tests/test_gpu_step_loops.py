"""The per-step BasicLSTM time loops of csrc/sequence.hip and csrc/lstm_bf16.hip: the whole-layer entry points and the time-range
ones run the same loop, so whole layer = time ranges, bit for bit where the same kernels run.  Called through _lib directly (the
persistent kernels cannot take over), F = 5, ragged num_frames holding 0, 1 and F, at the smallest shapes that reach both paths:
packed (B, H) = (33, 128) -- B no multiple of the 32- / 16-row tiles, Wp / Wq from yt8m_lstm_pack -- and generic (5, 12)."""
import ctypes

import pytest
import torch

import yt8m_amd._lib as L
from yt8m_amd import ops

pytestmark = pytest.mark.gpu

F = 5
PATHS = {"packed": (33, 128), "generic": (5, 12)}
SEAM_RTOL = 1e-6       # max|d dz| <= 1e-6 max|dz| where a plain product + a stand-alone gate kernel replace one fused launch
                       # (the bound of test_gpu_models.py::test_lstm_stack_pipelined_equals_sequential for the same situation)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _graph_stats(lib):
    v = [ctypes.c_int64(0) for _ in range(4)]
    lib.yt8m_graph_cache_stats(*[ctypes.byref(x) for x in v])
    return dict(zip(("hits", "captures", "fallbacks", "entries"), (x.value for x in v)))


class _Layer(object):
    """Fixed inputs of one (B, H) layer and, for the backward tests, the state a forward left (computed once, only read afterwards)."""

    def __init__(self, dev, B, H, forward):
        g = torch.Generator(device=dev).manual_seed(1000 * B + H)
        self.dev, self.B, self.H, self.lib = dev, B, H, L.lib()
        self.z0 = torch.randn((F, B, 4 * H), device=dev, generator=g) * 0.8
        self.Wh = (torch.rand((H, 4 * H), device=dev, generator=g) - 0.5) * (2.0 / H ** 0.5)
        self.nf = torch.randint(0, F + 1, (B,), device=dev, generator=g, dtype=torch.int32)
        self.nf[0], self.nf[1], self.nf[2] = F, 0, 1
        self.dout = torch.randn((F, B, H), device=dev, generator=g)
        self.dcf = torch.randn((B, H), device=dev, generator=g)
        self.dhf = torch.randn((B, H), device=dev, generator=g)
        self.packed = self.lib.yt8m_lstm_packed_floats(B, H) > 0
        self.Wp, self.Wq = self.pack(True), self.pack(False)
        self.gates, self.cs = forward(self)[:2] if forward else (None, None)
        torch.cuda.synchronize()

    @property
    def ws(self):
        return ops._workspace(self.dev)                 # per stream

    def pack(self, fwd):
        if not self.packed:
            return None
        w = torch.empty(self.H * 4 * self.H, device=self.dev)
        L.check(self.lib.yt8m_lstm_pack(_p(self.Wh), 4 * self.H, self.H, _p(w) if fwd else None, None if fwd else _p(w), _st()))
        return w

    def fwd_buffers(self):
        B, H = self.B, self.H
        return (torch.empty((F, B, 4 * H), device=self.dev), torch.empty((F + 1, B, H), device=self.dev),
                torch.empty((F + 1, B, H), device=self.dev), torch.empty((F, B, H), device=self.dev))

    def reset(self, bufs):
        z, cs, hs, out = bufs
        z.copy_(self.z0)
        for t in (cs, hs, out):
            t.zero_()

    def seeded_work(self):
        work = torch.zeros((4, self.B, self.H), device=self.dev)
        work[0], work[1] = self.dhf, self.dcf
        return work


def _layer_fwd(s):
    bufs = s.fwd_buffers()
    s.reset(bufs)
    z, cs, hs, out = bufs
    L.check(s.lib.yt8m_lstm_layer_fwd(_p(z), _p(s.Wh), 4 * s.H, _p(cs), _p(hs), _p(out), _p(s.nf), F, s.B, s.H, 1.0, _p(s.ws),
                                      s.ws.numel() * 4, _st()))
    torch.cuda.synchronize()
    return bufs


def _steps_bwd(s, ranges):
    """yt8m_lstm_steps_bwd over `ranges` (latest first) from hand-seeded work; returns dz, work, the carried phase."""
    dz, work, phase = torch.zeros((F, s.B, 4 * s.H), device=s.dev), s.seeded_work(), 0
    for t0, T in ranges:
        L.check(s.lib.yt8m_lstm_steps_bwd(_p(s.gates), _p(s.Wh), 4 * s.H, _p(s.Wq), _p(s.cs), _p(s.dout), _p(dz), _p(work), phase,
                                          _p(s.nf), t0, T, s.B, s.H, _p(s.ws), s.ws.numel() * 4, _st()))
        phase = (phase + T) % 2
    torch.cuda.synchronize()
    return dz, work, phase


@pytest.fixture(scope="module", params=sorted(PATHS))
def layer(request, dev):
    return _Layer(dev, *PATHS[request.param], forward=_layer_fwd)


@pytest.fixture(scope="module")
def stream(dev):
    return torch.cuda.Stream(dev)


@pytest.fixture(autouse=True)
def side_stream(stream):
    """Every call of a test is issued on a stream other than the legacy default one, as the layer pipeline of seq_ops does: the
    packed time-range forms are captured into hipGraphs, and the default stream cannot be captured."""
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        yield
    torch.cuda.synchronize()


def _close(a, b, ref):
    """max|a - b| <= SEAM_RTOL max|ref|, the figure printed first."""
    err, scale = float((a - b).abs().max()), float(ref.abs().max())
    print("max|delta| %.3e  max|ref| %.3e  ratio %.3e" % (err, scale, err / scale))
    return scale > 0 and err <= SEAM_RTOL * scale


def test_forward_whole_layer_equals_time_ranges(layer):
    s, lib = layer, layer.lib
    whole = _layer_fwd(s)
    assert bool(torch.isfinite(whole[3]).all()) and float(whole[3].abs().max()) > 0
    L.check(lib.yt8m_graph_cache_clear())
    before = _graph_stats(lib)
    bufs = s.fwd_buffers()
    z, cs, hs, out = bufs
    for _ in range(2):                                  # same buffers twice: on the packed path the second pass replays two hipGraphs
        s.reset(bufs)
        for t0, T in ((0, 2), (2, 3)):
            L.check(lib.yt8m_lstm_steps_fwd(_p(z), _p(s.Wh), 4 * s.H, _p(s.Wp), _p(cs), _p(hs), _p(out), _p(s.nf), t0, T, s.B, s.H, 1.0,
                                            _p(s.ws), s.ws.numel() * 4, _st()))
        torch.cuda.synchronize()
        for name, a, b in zip(("z", "cs", "hs", "out"), whole, bufs):
            assert torch.equal(a, b), name
    after = _graph_stats(lib)
    delta = {k: after[k] - before[k] for k in after}
    # only the packed time-range form is captured; the generic one takes host-side split-K decisions and issues directly
    assert delta == (dict(hits=2, captures=2, fallbacks=0, entries=2) if s.packed else dict(hits=0, captures=0, fallbacks=0, entries=0))


def test_backward_whole_layer_equals_one_time_range(layer):
    s = layer
    dz_a, work_a = torch.zeros((F, s.B, 4 * s.H), device=s.dev), torch.zeros((4, s.B, s.H), device=s.dev)
    L.check(s.lib.yt8m_lstm_layer_bwd(_p(s.gates), _p(s.Wh), 4 * s.H, _p(s.cs), _p(s.dout), _p(s.dcf), _p(s.dhf), _p(dz_a), _p(work_a),
                                      _p(s.nf), F, s.B, s.H, _p(s.ws), s.ws.numel() * 4, _st()))
    dz_b, work_b, phase = _steps_bwd(s, [(0, F)])
    assert bool(torch.isfinite(dz_a).all()) and float(dz_a.abs().max()) > 0
    assert torch.equal(dz_a, dz_b)                      # the same launches in the same order
    # the last (dh, dc) sit in the half of work that phase' = (0 + F) % 2 names; the other half holds the step before
    assert phase == F % 2
    last = slice(2 * phase, 2 * phase + 2)
    assert torch.equal(work_a[last], work_b[last])
    assert not torch.equal(work_a[last], work_a[2 - 2 * phase:4 - 2 * phase])
    dead = s.nf == 0                                    # a video without frames carries the final-state gradients through unchanged
    assert torch.equal(work_a[last][0][dead], s.dhf[dead]) and torch.equal(work_a[last][1][dead], s.dcf[dead])


def test_backward_two_time_ranges_equal_one(layer):
    s = layer
    dz_1, work_1, p1 = _steps_bwd(s, [(0, F)])
    dz_2, work_2, p2 = _steps_bwd(s, [(3, 2), (0, 3)])
    assert p1 == p2 == F % 2
    last = slice(2 * p1, 2 * p1 + 2)
    if s.packed:                                        # at the seam a plain product + the stand-alone gate kernel replace one fused launch
        assert _close(dz_2, dz_1, dz_1)
        assert _close(work_2[last], work_1[last], work_1[last])
    else:                                               # the same two kernels per step either way
        assert torch.equal(dz_1, dz_2) and torch.equal(work_1[last], work_2[last])


def test_bf16_backward_two_time_ranges_equal_one(dev):
    """yt8m_lstm_steps_bwd_bf16 at (B, H) = (33, 256), the smallest H the form accepts, on the state yt8m_lstm_steps_fwd_bf16 left."""
    B, H = 33, 256
    s = _Layer(dev, B, H, forward=None)
    lib = s.lib
    assert lib.yt8m_lstm_packed16_elems(B, H) == H * 4 * H
    Wp16, Wq16 = (torch.empty(H * 4 * H, dtype=torch.bfloat16, device=dev) for _ in range(2))
    L.check(lib.yt8m_lstm_pack_bf16(_p(s.Wh), 4 * H, H, _p(Wp16), _p(Wq16), _st()))
    gates, cs, hs, out = s.fwd_buffers()
    s.reset((gates, cs, hs, out))
    hs16 = torch.zeros((F + 1, B, H), dtype=torch.bfloat16, device=dev)
    L.check(lib.yt8m_lstm_steps_fwd_bf16(_p(gates), _p(Wp16), _p(cs), _p(hs), _p(hs16), _p(out), _p(s.nf), 0, F, B, H, 1.0, _st()))

    def bwd(ranges):
        dz, dz16 = torch.zeros((F, B, 4 * H), device=dev), torch.zeros((F, B, 4 * H), dtype=torch.bfloat16, device=dev)
        work, phase = s.seeded_work(), 0
        for t0, T in ranges:
            L.check(lib.yt8m_lstm_steps_bwd_bf16(_p(gates), _p(Wq16), _p(cs), _p(s.dout), _p(dz), _p(dz16), _p(work), phase, _p(s.nf),
                                                 t0, T, B, H, _st()))
            phase = (phase + T) % 2
        torch.cuda.synchronize()
        return dz, work, phase

    dz_1, work_1, p1 = bwd([(0, F)])
    dz_2, work_2, p2 = bwd([(3, 2), (0, 3)])
    assert bool(torch.isfinite(dz_1).all()) and p1 == p2 == F % 2
    assert _close(dz_2, dz_1, dz_1)
