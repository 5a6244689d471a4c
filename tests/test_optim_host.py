"""Not -m gpu: what tests/test_gpu_optim_branches.py relies on, checked without a device.

* the float64 reference of tests/optim_restatement.py agrees with oracle/np_ref.py (clip_by_norm, adam_step), the definition of the
  algorithm, when both get the same widened float32 constants;
* on the data of every GPU case a correct float32 implementation (restatement_f32) stays within HALF of each derived bound, and every
  wrong variant falls outside a bound on at least one case -- so the GPU test admits a right kernel and refuses a subtly wrong one;
* the chunk table Graph.finalize builds for the GPU module's tensor sizes has the properties csrc/optim.hip relies on;
* the optimiser entry points refuse bad arguments and treat empty problems as no-ops before touching a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import np_ref  # noqa: E402
import optim_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return R.host_cases()


def test_reference_agrees_with_the_oracle_on_widened_constants():
    case = R.make_case([(1027,), (300,)], 5)
    h = R.hyper()
    ref = R.reference(case, h)
    f = lambda x: np.float64(np.float32(x))
    b1, b2, t = f(h["b1"]), f(h["b2"]), 7
    lr = f(h["lr_t"]) * (1 - b1 ** t) / np.sqrt(1 - b2 ** t)                # adam_step turns it back into lr_t
    for i, n in enumerate(case["sizes"]):
        o = case["offsets"][i]
        w, m, v, g = (case[k][o:o + n].astype(np.float64) for k in "wmvg")
        ge = g * f(h["gscale"]) + np.float64(case["l2"][i]) * w
        assert abs(np.sum(ge * ge) - ref["n2"][i]) <= 1e-13 * ref["n2"][i]
        w1, m1, v1 = np_ref.adam_step(w, m, v, np_ref.clip_by_norm(ge, f(h["clip"])), lr, t, beta1=b1, beta2=b2, eps=f(h["eps"]))
        for got, want in ((ref["w"][o:o + n], w1), (ref["m"][o:o + n], m1), (ref["v"][o:o + n], v1)):
            assert float(np.abs(got - want).max()) <= 1e-13 * float(np.abs(want).max())
    g = R.clip_case(257, True)
    assert float(np.abs(R.clip_reference(g, 1.0) - np_ref.clip_by_norm(g.astype(np.float64), 1.0)).max()) <= 1e-15


def test_case_data_has_the_edges_the_issue_asks_for(cases):
    c = R.chunk_case()
    assert c["sizes"][:16] == [1, 3, 4, 5, 63, 64, 65, 1021, 1024, 1027, 4095, 4096, 4097, 8192, 12289, 257 * 4096 + 5]
    assert c["chunk_start"][16] - c["chunk_start"][15] > 256                 # the i += 256 loop of sqnorm_final_kernel
    assert {int(c["chunks"][c["chunk_start"][t + 1] - 1][1]) % 4 for t in range(len(c["sizes"]))} == {0, 1, 2, 3}
    ref = R.reference(c, R.hyper())
    norms = np.sqrt(ref["n2"])
    assert (norms < 0.5).sum() >= 4 and (norms > 2.0).sum() >= 4             # below and above clip = 1
    multi = np.diff(c["chunk_start"]) > 1
    assert (norms[multi] > 2.0).any() and (norms[multi] < 0.5).any()
    # cold elements: sqrt(v') of the size of eps in the tensors without l2
    cold = c["cold"][c["l2"][R.element_maps(c)[0][c["cold"]]] == 0]
    assert len(cold) >= 8 and (np.sqrt(ref["v"][cold]) < 1e-7).all() and (np.abs(c["g"][cold]) >= 1e-9).all() \
        and (np.abs(c["g"][cold]) <= 1e-6).all()
    assert len(c["zero"]) >= 14 and (ref["w"][c["zero"]] == c["w"][c["zero"]]).all()
    for name, case, h, tensors, skip in cases:                                # the assumption behind K_N (see the derivation)
        ref = R.reference(case, h)
        live = ref["n2"] > 0
        assert (R.n2_abs(case, h)[live] <= 1.21 * ref["n2"][live]).all(), name
        assert R.padding_intact(case, case["w"]) and R.padding_intact(case, case["g"])
    # the h2 steps: max |w| crosses a power of two in the second one and only there
    mx = [np.abs(case["w"][:case["sizes"][0]]).max() for name, case, h, t, s in cases if name.startswith("h2-")]
    _, w3, _, _ = R.restatement_f32(*[(case, h) for name, case, h, t, s in cases if name == "h2-step3"][0])
    mx.append(np.abs(w3[:10010]).max())
    e = [int(np.frexp(x)[1]) for x in mx]
    assert e[0] == e[1] and e[2] == e[1] + 1 and e[3] == e[2], (mx, e)


def test_a_correct_fp32_implementation_stays_within_half_of_every_bound(cases):
    for name, case, h, tensors, skip in cases:
        if name.startswith("h2-"):                                            # (held to its headers and image bytes, not to these bounds)
            continue
        ref = R.reference(case, h, tensors=tensors, skip=skip)
        n2, w, m, v = R.restatement_f32(case, h, tensors=tensors, skip=skip)
        r = R.ratios(ref, n2 if h["clip"] > 0 else None, w, m, v, tensors=tensors)
        print("%s: float32 restatement error / bound %s" % (name, " ".join("%s %.3f" % kv for kv in sorted(r.items()))))
        assert max(r.values()) <= 0.5, (name, r)
        keep = np.setdiff1d(np.arange(case["total"]), ref["updated"])
        for a, k in ((w, "w"), (m, "m"), (v, "v")):
            assert (a.view(np.uint32)[keep] == case[k].view(np.uint32)[keep]).all(), (name, k)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_is_outside_a_bound_on_some_case(cases, variant):
    caught = []
    for name, case, h, tensors, skip in cases:
        if (h["clip"] <= 0 and variant.startswith("norm")) or name.startswith("h2-"):
            continue
        ref = R.reference(case, h, tensors=tensors, skip=skip)
        bad = R.reference(case, h, tensors=tensors, skip=skip, variant=variant)
        r = R.ratios(ref, bad["n2"] if h["clip"] > 0 else None, bad["w"], bad["m"], bad["v"], tensors=tensors)
        if max(r.values()) > 1.0:
            caught.append((name, max(r, key=r.get), max(r.values())))
    print(variant, caught)
    assert any(name.startswith("chunk") for name, _, _ in caught), (variant, caught)
    if variant == "eps_in_root":                                             # ... and it is the cold elements that show it
        c, h = R.chunk_case(), R.hyper()
        ref, bad = R.reference(c, h), R.reference(c, h, variant=variant)
        b = R.bounds(ref)["w"]
        cold = c["cold"]
        assert (np.abs(bad["w"][cold] - ref["w"][cold]) > b[cold]).sum() >= 8


def test_chunk_table_of_graph_finalize():
    from yt8m_amd.variables import ALIGN, CHUNK, Graph, zeros
    for shapes in (R.chunk_case()["shapes"], R.tile_case()["shapes"], R.h2_case()["shapes"]):
        g = Graph(device="cpu", seed=0)
        for i, s in enumerate(shapes):
            g.get_variable("t%d" % i, s, zeros)
        g.finalize()
        want = R.layout([int(np.prod(s)) for s in shapes])
        ch = g.chunks.numpy()
        assert (ch == want["chunks"]).all() and g.chunk_start == want["chunk_start"].tolist() and g.total == want["total"]
        assert g.params.numel() == g.total and g.chunk_start_dev.tolist() == g.chunk_start
        tv = g.trainable_variables()
        seen = np.zeros(g.total, dtype=np.int32)
        for c, (x, y, z, _) in enumerate(ch):
            v = tv[z]
            assert 1 <= y <= CHUNK and x % 4 == 0 and v.offset <= x and x + y <= v.offset + v.numel(), (c, x, y, z)
            seen[x:x + y] += 1
        owned = np.zeros(g.total, dtype=bool)
        for v in tv:
            assert v.offset % ALIGN == 0
            owned[v.offset:v.offset + v.numel()] = True
        assert (seen[owned] == 1).all() and (seen[~owned] == 0).all()
        assert g.chunk_start == [int((ch[:, 2] < t).sum()) for t in range(len(tv) + 1)]        # the prefix count


def _job(R_=130, C=77, offset=0, tensor=0, specs=()):
    j = L.WimgJob()
    j.offset, j.R, j.C, j.tensor, j.nspec = offset, R_, C, tensor, len(specs)
    for i, (plain, trans, row0, rows, scale, planes) in enumerate(specs[:4]):
        s = j.spec[i]
        s.plain, s.trans, s.row0, s.rows, s.scale, s.planes = plain, trans, row0, rows, scale, planes
    return j


def test_wimg_jobs_layout_refusals_and_tile_bases():
    lib = L.lib()
    img = 4096

    def layout(*jobs, n=None):
        arr = (L.WimgJob * max(len(jobs), 1))(*jobs)
        return lib.yt8m_wimg_jobs_layout(arr, len(jobs) if n is None else n), arr

    ok = (img, None, 0, 130, 1.0, 3)
    assert layout(_job(specs=[ok]))[0] == 3 * 2
    assert layout(_job(specs=[(img, None, 32, 98, 1.0, 3)]))[0] == -2        # row0 % 64 != 0
    assert b"row window" in lib.yt8m_last_error()
    assert layout(_job(specs=[(img, None, 0, 100, 1.0, 3)]))[0] == -2        # ends neither on a tile nor with the matrix
    assert layout(_job(specs=[(img, None, 64, 67, 1.0, 3)]))[0] == -2        # ends beyond the matrix
    assert layout(_job(specs=[(img, None, 64, 66, 1.0, 3)]))[0] == 6         # ends with the matrix
    assert layout(_job(specs=[(img, None, 64, 64, 1.0, 3)]))[0] == 6         # ends on a tile
    assert layout(_job(specs=[(img, None, 0, 130, 1.0, 4)]))[0] == -1        # planes = 4
    assert layout(_job(specs=[(img, None, 0, 130, 1.0, 0)]))[0] == -1
    assert layout(_job(specs=[(img, img, 0, 130, 1.0, 2)]))[0] == 6          # planes = 2 is the h2 form
    assert layout(_job(specs=[(None, None, 0, 130, 1.0, 3)]))[0] == -1       # no image
    assert b"needs an image" in lib.yt8m_last_error()
    assert layout(_job(specs=[(img + 8, None, 0, 130, 1.0, 3)]))[0] == -1    # misaligned image
    assert layout(_job(specs=[(img, img + 4, 0, 130, 1.0, 3)]))[0] == -1
    five = _job(specs=[ok])
    five.nspec = 5
    assert layout(five)[0] == -1
    assert layout(_job(offset=6, specs=[ok]))[0] == -2                        # offset % 4 != 0
    assert layout(_job(R_=0, specs=[]))[0] == -2
    assert layout(_job(specs=[ok]), n=0)[0] == -1                             # njobs = 0
    assert lib.yt8m_wimg_jobs_layout(None, 1) == -1
    many = (L.WimgJob * 4097)(*[_job(specs=[]) for _ in range(4097)])
    assert lib.yt8m_wimg_jobs_layout(many, 4097) == -1 and lib.yt8m_wimg_jobs_layout(many, 4096) == 4096 * 6
    assert layout(_job(R_=(1 << 31) - 1, C=(1 << 31) - 1, specs=[]))[0] == -2 and b"too many tiles" in lib.yt8m_last_error()
    total, arr = layout(_job(64, 64, 0, 0, [(img, None, 0, 64, 1.0, 1)]), _job(130, 77, 4096, 2, []),
                        _job(33, 200, 16384, 5, [(None, img, 0, 33, 0.5, 3)]))
    assert total == 1 + 6 + 4 and [arr[i].tile_base for i in range(3)] == [0, 1, 7]


def test_optimizer_entry_points_refuse_and_skip_without_device():
    lib = L.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)                      # never dereferenced: validation fails first
    sq = lib.yt8m_sqnorm_multi
    assert sq(one, one, one, -1, one, 1.0, one, one, 0, 1, None, 0, None) == -2
    assert sq(one, one, one, 1, one, 1.0, one, one, -1, 1, None, 0, None) == -2
    assert sq(one, one, one, 1 << 31, one, 1.0, one, one, 0, 1, None, 0, None) == -2
    assert sq(None, None, None, 5, None, 1.0, None, None, 0, 0, None, 0, None) == 0              # no tensors: a no-op
    for k in (0, 1, 2, 4, 6, 7):                                             # w, g, chunks, l2, partial, norms
        a = [one, one, one, 1, one, 1.0, one, one, 0, 1, None, 0, None]
        a[k] = None
        assert sq(*a) == -1, k
    assert sq(odd, one, one, 1, one, 1.0, one, one, 0, 1, None, 0, None) == -1 and b"aligned" in lib.yt8m_last_error()
    assert sq(one, odd, one, 1, one, 1.0, one, one, 0, 1, None, 0, None) == -1
    ad = lib.yt8m_adam_multi_ex
    hp = (1.0, 0.01, 0.9, 0.999, 1e-8)
    assert ad(one, one, one, one, one, -1, one, 1.0, one, *hp, None, None) == -2
    assert ad(one, one, one, one, one, 1 << 31, one, 1.0, one, *hp, None, None) == -2
    assert ad(None, None, None, None, None, 0, None, 1.0, None, *hp, None, None) == 0            # no chunks: a no-op
    for k in (0, 1, 2, 3, 4, 6):
        a = [one, one, one, one, one, 1, one, 1.0, one, *hp, None, None]
        a[k] = None
        assert ad(*a) == -1, k
    assert ad(one, one, one, one, one, 1, one, 1.0, None, *hp, None, None) == -1 and b"norms" in lib.yt8m_last_error()
    assert lib.yt8m_adam_multi(one, one, one, one, one, 1, one, 1.0, None, *hp, None) == -1
    assert lib.yt8m_adam_multi(None, None, None, None, None, 0, None, 1.0, None, *hp, None) == 0
    ti = lib.yt8m_adam_tiles
    assert ti(one, one, one, one, one, -1, 0, 1, one, 1.0, one, *hp, 1, None) == -2
    assert ti(one, one, one, one, one, 1, -1, 1, one, 1.0, one, *hp, 1, None) == -2
    assert ti(one, one, one, one, one, 1, 0, 1 << 31, one, 1.0, one, *hp, 1, None) == -2
    assert ti(None, None, None, None, None, 0, 0, 5, None, 1.0, None, *hp, 1, None) == 0         # no jobs / no tiles: no-ops
    assert ti(None, None, None, None, None, 3, 0, 0, None, 1.0, None, *hp, 1, None) == 0
    assert ti(None, one, one, one, one, 1, 0, 1, one, 1.0, one, *hp, 1, None) == -1
    assert ti(one, one, one, one, None, 1, 0, 1, one, 1.0, one, *hp, 1, None) == -1
    for k in (1, 2, 3, 8):                                                   # m, v, g, l2 are needed with do_adam only
        a = [one, one, one, one, one, 1, 0, 1, one, 1.0, one, *hp, 1, None]
        a[k] = None
        assert ti(*a) == -1, k
    assert ti(one, one, one, one, one, 1, 0, 1, one, 1.0, None, *hp, 1, None) == -1              # clip > 0 needs norms
    assert ti(odd, None, None, None, one, 1, 0, 1, None, 1.0, None, *hp, 0, None) == -1 and b"aligned" in lib.yt8m_last_error()
    rg = lib.yt8m_optimizer_ranges
    assert rg(None, None) == -1

    def desc(**kw):
        o = L.OptRanges()
        for k in ("w", "m", "v", "g", "chunks", "tensor_chunk_start", "tensor_chunk_start_host", "l2", "partial", "norms"):
            setattr(o, k, 16)
        o.nranges, o.clip = 1, 1.0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    assert rg(ctypes.byref(desc(nranges=0)), None) == -1 and rg(ctypes.byref(desc(nranges=9)), None) == -1
    for k in ("w", "m", "v", "g", "chunks", "tensor_chunk_start", "tensor_chunk_start_host", "l2", "partial", "norms"):
        assert rg(ctypes.byref(desc(**{k: None})), None) == -1, k
    assert rg(ctypes.byref(desc(njobs=-1)), None) == -1
    assert rg(ctypes.byref(desc(njobs=1)), None) == -1 and b"image jobs" in lib.yt8m_last_error()
    bad = desc()
    bad.range_lo[0], bad.range_hi[0] = 3, 2
    assert rg(ctypes.byref(bad), None) == -1 and b"range" in lib.yt8m_last_error()
    bad.range_lo[0], bad.range_hi[0] = -1, 2
    assert rg(ctypes.byref(bad), None) == -1
    empty = desc(nranges=3)                                                  # three empty ranges: nothing is read, nothing is launched
    for i in range(3):
        empty.range_lo[i] = empty.range_hi[i] = 4 * i
    assert rg(ctypes.byref(empty), None) == 0
    cl = lib.yt8m_clip_by_norm_f32
    assert cl(one, one, -1, 1.0, one, None) == -1 and cl(one, one, 4, 0.0, one, None) == -1 and cl(one, one, 4, -1.0, one, None) == -1
    assert cl(None, None, 0, 1.0, None, None) == 0                                               # n = 0: a no-op
    assert cl(None, one, 4, 1.0, one, None) == -1 and cl(one, None, 4, 1.0, one, None) == -1 and cl(one, one, 4, 1.0, None, None) == -1
    assert torch.zeros(1).device.type == "cpu"
