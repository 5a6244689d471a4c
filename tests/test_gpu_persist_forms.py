"""-m gpu: the launches of the persistent recurrences agree with the plan table of tests/test_persist_plan_host.py.

One row of GPU_TABLE is one direct C-ABI launch of T = 4 steps (two where a bf16 / h2 request is compared with the plain entry), keyed
by the device's CU count: on another device the rows are looked up under its count and skip where the table has no such row.  Per row:
the status is clean, yt8m_lstm_persist_placement_stats reports exactly one launch of the plan's grid, the tape-prefetch counters move
by what the plan's TPF says, a request the plan answers with the fp32 form gives the plain entry's bytes (the kernels are bitwise
reproducible: fixed summation order, csrc/lstm_persist.hip), a request the plan grants gives different bytes and its query says 1, and
the refusals return YT8M_E_SHAPE with no launch counted.  No numerical limit is set here: the forms' accuracy is pinned by
test_gpu_round3 / 4, test_gpu_h2_recur, test_gpu_x3, test_gpu_tape_prefetch, test_gpu_recurrent_fp64 and test_gpu_trajectory."""
import ctypes

import pytest
import torch

import yt8m_amd._lib as L
from yt8m_amd.ops import _p, _stream
from test_persist_plan_host import GPU_TABLE, TABLE, fields

pytestmark = pytest.mark.gpu

E_SHAPE = -2
PLANS = dict(TABLE + GPU_TABLE)
_skipped = []
_inputs = {}
_plain = {}


def _i64():
    return ctypes.c_int64(0)


def _stats(lib, reset):
    a, b, c = _i64(), _i64(), _i64()
    L.check(lib.yt8m_lstm_persist_placement_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), reset))
    return a.value, b.value


def _tpf(lib):
    a, b = _i64(), _i64()
    L.check(lib.yt8m_lstm_persist_tape_prefetch_launches(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def _data(dev, B, H, T):
    if (B, H) not in _inputs:
        g = torch.Generator(device=dev).manual_seed(B * 7 + H)
        r = lambda *s: torch.randn(s, device=dev, generator=g)
        gates = torch.rand((T, B, 4 * H), device=dev, generator=g)
        gates[:, :, H:2 * H] = gates[:, :, H:2 * H] * 2 - 1
        nf = torch.randint(1, T + 1, (B,), device=dev, generator=g, dtype=torch.int32)
        nf[0] = T
        word = torch.zeros(64, dtype=torch.int32, device=dev)
        Wh = (torch.rand((H, 4 * H), device=dev, generator=g) - 0.5) * 0.08
        L.check(L.lib().yt8m_h2_absmax(_p(Wh), H, 4 * H, 4 * H, _p(word), _stream()))
        _inputs[(B, H)] = dict(z=r(T, B, 4 * H) * 0.5, Wh=Wh, cs=r(T + 1, B, H) * 0.5, hs=r(T + 1, B, H) * 0.3, gates=gates, dout=r(T, B, H) * 0.01,
                               work=r(4, B, H) * 0.02, nf=nf, word=word, zg=r(T, B, 2 * H) * 0.5, zc=r(T, B, H) * 0.5,
                               Wg=(torch.rand((H, 2 * H), device=dev, generator=g) - 0.5) * 0.08,
                               Wc=(torch.rand((H, H), device=dev, generator=g) - 0.5) * 0.08)
    return _inputs[(B, H)]


def _launch(lib, dev, d, B, H, T, ws, product, images, gru):
    """-> (return code, output tensors, workspace)"""
    x = _data(dev, B, H, T)
    pws = torch.zeros(ws, dtype=torch.uint8, device=dev)
    if gru:
        zg, zc, hs = x["zg"].clone(), x["zc"].clone(), x["hs"].clone()
        rh, out = torch.zeros((T, B, H), device=dev), torch.zeros((T, B, H), device=dev)
        rc = lib.yt8m_gru_persist_fwd(_p(zg), _p(zc), _p(x["Wg"]), 2 * H, _p(x["Wc"]), H, _p(hs), _p(rh), _p(out), _p(x["nf"]), 0, T, B, H,
                                      _p(pws), ws, _stream())
        return rc, (zg, zc, hs, rh, out), pws
    if d == "fwd":
        z, cs, hs, out = x["z"].clone(), x["cs"].clone(), x["hs"].clone(), torch.zeros((T, B, H), device=dev)
        head = [_p(z), _p(x["Wh"]), 4 * H, _p(cs), _p(hs), _p(out), _p(x["nf"]), 0, T, B, H, 1.0]
        tail = [_p(pws), ws, _stream()]
        rc = (lib.yt8m_lstm_persist_fwd(*head, *tail) if product == 0 else lib.yt8m_lstm_persist_fwd_bf16(*head, *tail) if product == 1
              else lib.yt8m_lstm_persist_fwd_h2(*head, _p(x["word"]), *tail))
        return rc, (z, cs, hs, out), pws
    dz, work = torch.zeros((T, B, 4 * H), device=dev), x["work"].clone()
    head = [_p(x["gates"]), _p(x["Wh"]), 4 * H, _p(x["cs"]), _p(x["dout"]), _p(dz), _p(work), 0]
    tail = [_p(pws), ws, _stream()]
    if images:
        plain = torch.zeros(lib.yt8m_x3_image_bytes(T * B, 4 * H), dtype=torch.uint8, device=dev)
        im = L.PersistBwdImages(plain.data_ptr(), None, None, None, None, None)
        rc = lib.yt8m_lstm_persist_bwd_images(*head, _p(x["nf"]), 0, T, B, H, _p(pws), ws, ctypes.byref(im), _stream())
        return rc, (dz, plain), pws
    mid = [None, _p(x["nf"]), 0, T, B, H]
    rc = (lib.yt8m_lstm_persist_bwd(*head, *mid, *tail) if product == 0 else lib.yt8m_lstm_persist_bwd_bf16(*head, *mid, *tail) if product == 1
          else lib.yt8m_lstm_persist_bwd_h2(*head, *mid, _p(x["word"]), *tail))
    return rc, (dz, work), pws


@pytest.mark.parametrize("row", range(len(GPU_TABLE)), ids=[c.replace(" ", "_") for c, _ in GPU_TABLE])
def test_launch_agrees_with_the_plan(dev, row):
    lib = L.lib()
    t = GPU_TABLE[row][0].split()
    t[1] = str(torch.cuda.get_device_properties(dev).multi_processor_count)
    case = " ".join(t)
    if case not in PLANS:
        _skipped.append(case)
        pytest.skip("the plan table has no row for this device's CU count")
    d, mode, B, H, T, ws, product, images, gru = t[0], int(t[4]), int(t[5]), int(t[6]), int(t[7]), int(t[8]), int(t[9]), int(t[10]), int(t[12])
    f = fields(PLANS[case])
    # the workspace sizes the table states are the library's
    sizes = (lib.yt8m_gru_persist_workspace_bytes(B, H, T),) if gru else (lib.yt8m_lstm_persist_workspace_bytes(B, H),
                                                                         lib.yt8m_lstm_persist_workspace_bytes_steps(B, H, T))
    assert ws in sizes
    L.check(lib.yt8m_lstm_persist_set_tape_prefetch(mode))
    try:
        _stats(lib, 1)
        tpf0 = _tpf(lib)
        rc, outs, pws = _launch(lib, dev, d, B, H, T, ws, product, images, gru)
        torch.cuda.synchronize()
        tpf1 = _tpf(lib)
    finally:
        L.check(lib.yt8m_lstm_persist_set_tape_prefetch(0))
    if f["code"] != "0":
        assert rc == E_SHAPE and int(f["code"]) == E_SHAPE
        assert _stats(lib, 1) == (0, 0) and tpf1 == tpf0
        return
    L.check(rc)
    L.check(lib.yt8m_lstm_persist_status(_p(pws), _stream()))
    assert _stats(lib, 1) == (1, int(f["grid"]))
    h2_form = d == "bwd" and f["form"] == "h2"
    assert (tpf1[0] - tpf0[0], tpf1[1] - tpf0[1]) == ((1, 0) if f.get("TPF") == "1" else (0, 1) if h2_form else (0, 0))
    assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
    if gru or images:
        return
    if product == 0:
        _plain[(d, B, H, ws)] = outs
        return
    if (d, B, H, ws) not in _plain:                      # (the plain entry's row comes first in the table: only when rows are deselected)
        _plain[(d, B, H, ws)] = _launch(lib, dev, d, B, H, T, ws, 0, 0, 0)[1]
    ref = _plain[(d, B, H, ws)]
    same = all(torch.equal(a, b) for a, b in zip(outs, ref))
    if f["form"] == "fp32":
        assert same, "the plan says this request falls back to the fp32 form"
    else:
        assert not same, "the plan says this request is granted"
        assert (lib.yt8m_lstm_persist_fwd_on_bf16_pipe(B, H) if d == "fwd" else lib.yt8m_lstm_persist_bwd_on_f16_pipe(B, H)) == 1


def test_no_row_was_skipped_on_a_256_cu_device(dev):
    if torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        assert _skipped == []
