"""-m gpu: every branch of the flat-arena optimiser pass (csrc/optim.hip: per-tensor gradient norm, tf.clip_by_norm, TF-1 Adam, the
64 x 64 tile pass that rewrites the resident operand images) against the float64 reference of tests/optim_restatement.py, at every
chunk, tile and range edge, through ops.sqnorm_and_adam and through the raw C ABI.

BRANCH_TABLE below is the reading of the seven extern "C" entry points this module was written from: one row per `if` / `else` arm and per
in-kernel path choice, as (entry point, condition as written in optim.hip, kernel launched, case of this module that takes it).
tests/test_optim_branch_table.py checks every kernel named here against the source and every __global__ of the source against the kernel
list recorded from a profiled run of this module (tests/golden/optim_kernels_seen.txt, profiles/optim_branches_kernel_stats.csv).

Bounds.  Weights, Adam slots and norms are held to the bounds derived in tests/optim_restatement.py from the count of float32 roundings
on each path (K_N = 32, K_M = 24, K_V = 45, K_W = 51; tests/test_optim_host.py shows that a correct float32 implementation stays within
half of them on this module's data and that five subtly wrong ones do not stay within them).  Everything a call must not write --
tensors outside a range, skipped tensors, the gradient arena, norms of other tensors, the 64-float padding between tensors, which holds a
NaN sentinel in all four arenas -- is compared bit for bit, and so are the operand images, against oracle/x3_ref.py applied to the
float32 weights the device holds.  Every case prints its error / bound ratios."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L
import yt8m_amd.ops as ops
from conftest import ROOT
from yt8m_amd.variables import Graph, zeros

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import optim_restatement as R  # noqa: E402
import x3_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu

HOST = "tests/test_optim_host.py::test_optimizer_entry_points_refuse_and_skip_without_device"
HOST_JOBS = "tests/test_optim_host.py::test_wimg_jobs_layout_refusals_and_tile_bases"

BRANCH_TABLE = [
    # ---- yt8m_sqnorm_multi ----------------------------------------------------------------------------------------------------------
    ("yt8m_sqnorm_multi", "nchunks >= 0 && ntensors >= 0 && tensor_base >= 0 && nchunks < 2^31 else YT8M_E_SHAPE; null operand, "
     "arena not 16-byte aligned: YT8M_E_BADARG", "(none)", HOST),
    ("yt8m_sqnorm_multi", "ntensors == 0: no-op", "(none)", HOST),
    ("yt8m_sqnorm_multi", "nchunks > 0", "sqnorm_chunk_kernel", "test_chunk_pass[*-clip1]: 281 chunks"),
    ("yt8m_sqnorm_multi", "in kernel: i + 3 < ch.y (float4), k = 0 .. 3", "sqnorm_chunk_kernel",
     "test_chunk_pass[*-clip1]: tensors of 4, 64, 1024 (k = 0 only), 4096 (all four), 4097, 8192, 12289, 257 * 4096 + 5"),
    ("yt8m_sqnorm_multi", "in kernel: else (scalar tail, j < ch.y && j < i + 4)", "sqnorm_chunk_kernel",
     "test_chunk_pass[*-clip1]: last chunks of 1, 3, 5, 6 (residue 2), 63, 65, 1021, 1027, 4095 floats, the 1-float chunk of 4097"),
    ("yt8m_sqnorm_multi", "(always)", "sqnorm_final_kernel", "test_chunk_pass[*-clip1]"),
    ("yt8m_sqnorm_multi", "in kernel: tcs (tensor_chunk_start given); i += 256 over a tensor of 258 chunks", "sqnorm_final_kernel",
     "test_chunk_pass[ops-clip1]; chunk_base > 0: test_chunk_sub_range, test_optimizer_ranges_two_disjoint_ranges"),
    ("yt8m_sqnorm_multi", "in kernel: else (tensor_chunk_start == NULL: the chunks[i].z == t scan)", "sqnorm_final_kernel",
     "test_chunk_pass[raw-clip1]"),
    # ---- yt8m_adam_multi / yt8m_adam_multi_ex ---------------------------------------------------------------------------------------
    ("yt8m_adam_multi", "(forwards to yt8m_adam_multi_ex with skip_tensor = NULL)", "adam_chunk_kernel",
     "test_chunk_pass[raw-clip1], [raw-clip0] (norms = NULL)"),
    ("yt8m_adam_multi_ex", "nchunks >= 0 && nchunks < 2^31 else YT8M_E_SHAPE; null operand; clip <= 0 || norms else YT8M_E_BADARG", "(none)", HOST),
    ("yt8m_adam_multi_ex", "nchunks == 0: no-op", "(none)", HOST),
    ("yt8m_adam_multi_ex", "(always)", "adam_chunk_kernel", "test_chunk_pass[ops-*]"),
    ("yt8m_adam_multi_ex", "in kernel: skip && skip[ch.z]: return", "adam_chunk_kernel",
     "test_chunk_skip_mask (tensors 3, 8, 15 flagged); test_tile_pass (every image-owning matrix)"),
    ("yt8m_adam_multi_ex", "in kernel: h.clip > 0 (cs from norms) / else cs = 1", "adam_chunk_kernel", "test_chunk_pass[*-clip1] / [*-clip0]"),
    ("yt8m_adam_multi_ex", "in kernel: i + 3 < ch.y (float4) / else scalar tail", "adam_chunk_kernel", "test_chunk_pass: the sizes above"),
    # ---- yt8m_wimg_jobs_layout (host only) ------------------------------------------------------------------------------------------
    ("yt8m_wimg_jobs_layout", "jobs && 1 <= njobs <= 4096; R, C, offset; 0 <= nspec <= 4; planes 1 / 2 / 3; an image; 16-byte aligned "
     "images; the row window; tiles < 2^31; else YT8M_E_BADARG / YT8M_E_SHAPE", "(none)", HOST_JOBS),
    ("yt8m_wimg_jobs_layout", "tile_base = cumulative tile count, returns the total", "(none)", HOST_JOBS + "; test_tile_pass (through wimg.py)"),
    # ---- yt8m_adam_tiles ------------------------------------------------------------------------------------------------------------
    ("yt8m_adam_tiles", "njobs >= 0 && ntiles >= 0 && ntiles < 2^31 && tile0 >= 0 else YT8M_E_SHAPE; null operands (m, v, g, l2 with "
     "do_adam only); clip > 0 needs norms; arena alignment", "(none)", HOST),
    ("yt8m_adam_tiles", "njobs == 0 || ntiles == 0: no-op", "(none)", HOST),
    ("yt8m_adam_tiles", "(always) in kernel: si >= nspec, planes != 2, no image: return; else roll the header", "wimg_roll_kernel",
     "test_tile_pass (planes 1 and 3, 2 .. 4 specs: all three returns); test_h2_images (the roll)"),
    ("yt8m_adam_tiles", "do_adam", "adam_tile_kernel<true>", "test_tile_pass, test_h2_images"),
    ("yt8m_adam_tiles", "else (images only)", "adam_tile_kernel<false>", "test_tile_pass (first build), test_h2_images (first build)"),
    ("yt8m_adam_tiles", "in kernel: while (j + 1 < njobs && tile >= jobs[j + 1].tile_base): several jobs; tile0 > 0", "adam_tile_kernel<true>",
     "test_tile_pass: six jobs from tile 0, then jobs 2 .. 4 of the array (tile0 = 3)"),
    ("yt8m_adam_tiles", "in kernel: r0 + r < R (rows beyond the matrix are zeros)", "adam_tile_kernel<true> adam_tile_kernel<false>",
     "test_tile_pass: R = 65, 130, 33, 200"),
    ("yt8m_adam_tiles", "in kernel: vec && c0 + c4 + 3 < C (float4 row)", "adam_tile_kernel<true> adam_tile_kernel<false>",
     "test_tile_pass: C = 64, 16, 136 and 200 (the last tile holds 8 columns)"),
    ("yt8m_adam_tiles", "in kernel: else (scalar tile row; c0 + c4 + k < C)", "adam_tile_kernel<true> adam_tile_kernel<false>",
     "test_tile_pass: C = 63, 77 ((C & 3) != 0); C = 16, 136, 200 beyond the last column"),
    ("yt8m_adam_tiles", "in kernel: ADAM: h.clip > 0", "adam_tile_kernel<true>", "test_tile_pass (norms below and above clip)"),
    ("yt8m_adam_tiles", "in kernel: r0 < w0 || r0 >= w0 + wr: tile outside the window", "adam_tile_kernel<true> adam_tile_kernel<false>",
     "test_tile_pass: windows (0, 128) of 130 and 200 rows, (128, 72), (128, 2), (64, 64) and (128, 64) of 192, (64, 1) of 65"),
    ("yt8m_adam_tiles", "in kernel: S.plain / S.trans; planes == 3 / else 1; scale", "adam_tile_kernel<true> adam_tile_kernel<false>",
     "test_tile_pass: both orientations with 3 planes and with 1, scale 4 / 255 and 2"),
    ("yt8m_adam_tiles", "in kernel: h2 (planes == 2): scale from header word 0, tile maximum into word 1 of plain and trans",
     "adam_tile_kernel<true> adam_tile_kernel<false>", "test_h2_images: (130, 77), (200, 136) plain and transposed; the all-zero matrix (scale 1)"),
    ("yt8m_adam_tiles", "in kernel: row < round32(rows) && kb < KB", "adam_tile_kernel<true> adam_tile_kernel<false>",
     "test_tile_pass: image rows 1, 2, 33, 63, 65, 72, 77, 130, 200; K = 16, 63, 72, 77, 130"),
    # ---- yt8m_optimizer_ranges ------------------------------------------------------------------------------------------------------
    ("yt8m_optimizer_ranges", "o && 1 <= nranges <= 8; null operand; njobs needs its tables; lo >= 0 && hi >= lo; else YT8M_E_BADARG", "(none)", HOST),
    ("yt8m_optimizer_ranges", "after_stream && after_stream != stream: wait for it", "adam_chunk_kernel",
     "test_optimizer_ranges_one_range[side] (a side stream wrote the gradients)"),
    ("yt8m_optimizer_ranges", "else (no after_stream, or the same stream)", "adam_chunk_kernel", "test_optimizer_ranges_one_range[plain], [clip0]"),
    ("yt8m_optimizer_ranges", "hi == lo: continue", "(none)", "test_optimizer_ranges_two_disjoint_ranges: (7, 7) between (0, 5) and (9, 18); " + HOST),
    ("yt8m_optimizer_ranges", "o->clip > 0", "sqnorm_chunk_kernel sqnorm_final_kernel", "test_optimizer_ranges_one_range[plain], [side]; else: [clip0]"),
    ("yt8m_optimizer_ranges", "o->njobs ? o->skip_tensor : nullptr; jobs of [lo, hi): j1 > j0", "adam_tile_kernel<true>",
     "test_optimizer_ranges_with_image_jobs: ranges (0, 2) and (4, 6) of seven tensors, jobs inside and outside; (2, 3) holds no job"),
    # ---- yt8m_clip_by_norm_f32 ------------------------------------------------------------------------------------------------------
    ("yt8m_clip_by_norm_f32", "n >= 0 && max_norm > 0; null operand; else YT8M_E_BADARG", "(none)", HOST),
    ("yt8m_clip_by_norm_f32", "n == 0: no-op", "(none)", HOST + "; test_clip_by_norm_empty"),
    ("yt8m_clip_by_norm_f32", "(always) 256 workgroups, stride 65536", "clip_sqnorm_kernel",
     "test_clip_by_norm: n = 1, 255, 256, 257 (one element per lane), 65539, 4096 * 256 + 7 (17 per lane)"),
    ("yt8m_clip_by_norm_f32", "blocks = min((n + 255) / 256, 4096): below the cap one element per lane, past it the stride loop", "clip_scale_kernel",
     "test_clip_by_norm: n = 65539 (257 workgroups), 4096 * 256 + 7 (capped); out of place and in place; norm below and above max_norm"),
]

NORM_SENT = -7.0
WORST = {"norms": 0.0, "m": 0.0, "v": 0.0, "w": 0.0}
ALPHA = float(np.float32(4.0 / 255.0))


def _st(stream=None):
    return ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None


def _hp(h):
    return dict(gscale=float(h["gscale"]), clip=float(h["clip"]), beta1=float(h["b1"]), beta2=float(h["b2"]), eps=float(h["eps"]))


def _load(g, case, only_grads=False):
    pairs = ((g.grads, "g"),) if only_grads else ((g.params, "w"), (g.adam_m, "m"), (g.adam_v, "v"), (g.grads, "g"))
    for t, k in pairs:
        t.copy_(torch.from_numpy(case[k]))                                   # (a byte copy: the NaN sentinel keeps its payload)
    g.norms.fill_(NORM_SENT)


def _graph(dev, case):
    g = Graph(device=dev, seed=0)
    g.begin_step()
    for i, s in enumerate(case["shapes"]):
        g.get_variable("t%d" % i, s, zeros, l2=float(case["l2"][i]))
    g.finalize()
    assert g.total == case["total"] and (g.chunks.cpu().numpy() == case["chunks"]).all() and g.chunk_start == case["chunk_start"].tolist()
    assert (g.l2.cpu().numpy() == case["l2"]).all()
    _load(g, case)
    return g


def _state(g):
    torch.cuda.synchronize()
    return dict(w=g.params.cpu().numpy(), m=g.adam_m.cpu().numpy(), v=g.adam_v.cpu().numpy(), g=g.grads.cpu().numpy(),
                norms=g.norms.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(name, case, h, got, tensors=None, skip=None, norms_before=None):
    """got (the device's state after the call on `case`) against the float64 reference: the updated elements and norms within the
    derived bounds; everything else, the padding's sentinel included, bit for bit what it was."""
    ref = R.reference(case, h, tensors=tensors, skip=skip)
    clip = float(h["clip"]) > 0
    r = R.ratios(ref, got["norms"] if clip else None, got["w"], got["m"], got["v"], tensors=tensors)
    for k in r:
        WORST[k] = max(WORST[k], r[k])
    print("%s: error / bound norms %.3f m %.3f v %.3f w %.3f (bounds: K_N %g K_M %g K_V %g K_W %g times 2^-24; worst so far %s)"
          % (name, r["norms"], r["m"], r["v"], r["w"], R.K_N, R.K_M, R.K_V, R.K_W, " ".join("%s %.3f" % kv for kv in sorted(WORST.items()))))
    assert max(r.values()) <= 1.0, (name, r)
    keep = np.setdiff1d(np.arange(case["total"]), ref["updated"])
    for k in "wmv":
        assert R.padding_intact(case, got[k]), (name, k, "padding written")
        assert (_bits(got[k])[keep] == _bits(case[k])[keep]).all(), (name, k, "written outside the update")
    assert (_bits(got["g"]) == _bits(case["g"])).all(), (name, "gradients written")
    zero = np.intersect1d(case["zero"], ref["updated"])
    assert (_bits(got["w"])[zero] == _bits(case["w"])[zero]).all() and (_bits(got["m"])[zero] == 0).all() and (_bits(got["v"])[zero] == 0).all()
    before = np.full(len(case["sizes"]), NORM_SENT, dtype=np.float32) if norms_before is None else norms_before
    on = R._active(case, tensors, None) if clip else np.zeros(len(case["sizes"]), dtype=bool)
    assert (_bits(got["norms"])[~on] == _bits(before)[~on]).all(), (name, "norms of other tensors written")
    return ref


# ---- chunk pass -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_case():
    return R.chunk_case()


def _raw_pass(g, h, skip=None, tcs=False):
    lib = L.lib()
    nT = len(g.trainable_variables())
    if float(h["clip"]) > 0:
        L.check(lib.yt8m_sqnorm_multi(_p(g.params), _p(g.grads), _p(g.chunks), g.nchunks, _p(g.l2), float(h["gscale"]), _p(g.partial),
                                      _p(g.norms), 0, nT, _p(g.chunk_start_dev) if tcs else None, 0, _st()))
    args = (_p(g.params), _p(g.adam_m), _p(g.adam_v), _p(g.grads), _p(g.chunks), g.nchunks, _p(g.l2), float(h["gscale"]),
            _p(g.norms) if float(h["clip"]) > 0 else None, float(h["clip"]), float(h["lr_t"]), float(h["b1"]), float(h["b2"]), float(h["eps"]))
    if skip is None:
        L.check(lib.yt8m_adam_multi(*args, _st()))
    else:
        L.check(lib.yt8m_adam_multi_ex(*args, _p(skip), _st()))


@pytest.mark.parametrize("clip", [1.0, 0.0], ids=["clip1", "clip0"])
@pytest.mark.parametrize("path", ["ops", "raw"])
def test_chunk_pass(dev, chunk_case, path, clip):
    """Tensors of 1 .. 257 * 4096 + 5 floats in one arena: every residue of the last chunk, one to four unrolled iterations, a tensor of
    258 chunks.  ops: ops.sqnorm_and_adam (tensor_chunk_start given); raw: the C ABI with tensor_chunk_start = NULL and yt8m_adam_multi
    (norms = NULL at clip = 0)."""
    h = R.hyper(clip=clip)
    g = _graph(dev, chunk_case)
    assert g.nchunks == 281 and g.chunk_start[16] - g.chunk_start[15] == 258
    if path == "ops":
        ops.sqnorm_and_adam(g, float(h["lr_t"]), **_hp(h))
    else:
        _raw_pass(g, h)
    _check("chunk pass %s clip %g" % (path, clip), chunk_case, h, _state(g))


def test_chunk_sub_range(dev, chunk_case):
    h = R.hyper()
    g = _graph(dev, chunk_case)
    ops.sqnorm_and_adam(g, float(h["lr_t"]), tensors=R.SUB_RANGE, **_hp(h))
    _check("chunk pass tensors %s" % (R.SUB_RANGE,), chunk_case, h, _state(g), tensors=[R.SUB_RANGE])


def test_chunk_skip_mask(dev, chunk_case):
    """yt8m_adam_multi_ex with flags on a small, a middle and the 258-chunk tensor: their norms are computed, nothing else of them moves."""
    h = R.hyper()
    g = _graph(dev, chunk_case)
    skip = R.skip_mask(len(chunk_case["sizes"]))
    _raw_pass(g, h, skip=torch.from_numpy(skip).to(dev), tcs=True)
    ref = _check("chunk pass with skip_tensor", chunk_case, h, _state(g), skip=skip)
    assert len(np.intersect1d(ref["updated"], np.arange(chunk_case["offsets"][15], chunk_case["offsets"][15] + 100))) == 0


def test_chunk_second_step(dev, chunk_case):
    """A second step from the state the first one left on the device (no longer cold: m, v of every element are in use)."""
    h1, h2 = R.hyper(), R.hyper(lr_t=0.02)
    g = _graph(dev, chunk_case)
    ops.sqnorm_and_adam(g, float(h1["lr_t"]), **_hp(h1))
    s1 = _state(g)
    _check("chunk pass step 1", chunk_case, h1, s1)
    case2 = R.next_step_case(chunk_case, s1["w"], s1["m"], s1["v"], 21)
    _load(g, case2, only_grads=True)
    ops.sqnorm_and_adam(g, float(h2["lr_t"]), **_hp(h2))
    _check("chunk pass step 2", case2, h2, _state(g))


# ---- yt8m_optimizer_ranges ----------------------------------------------------------------------------------------------------------------
class _Ranges(object):
    """yt8m_opt_ranges over a graph (what seq_ops._EarlyOpt builds for the recurrent stack's early pass)."""

    def __init__(self, g, ranges, h, after=None):
        o = L.OptRanges()
        o.w, o.m, o.v, o.g = g.params.data_ptr(), g.adam_m.data_ptr(), g.adam_v.data_ptr(), g.grads.data_ptr()
        o.chunks, o.tensor_chunk_start = g.chunks.data_ptr(), g.chunk_start_dev.data_ptr()
        self.tcs = (ctypes.c_int32 * len(g.chunk_start))(*g.chunk_start)
        o.tensor_chunk_start_host = ctypes.cast(self.tcs, ctypes.c_void_p)
        o.l2, o.partial, o.norms = g.l2.data_ptr(), g.partial.data_ptr(), g.norms.data_ptr()
        wi = g.wimg
        if wi is not None and wi.active:
            self.jt = (ctypes.c_int32 * len(wi.job_tensor))(*wi.job_tensor)
            self.tb = (ctypes.c_int64 * len(wi.tile_base))(*wi.tile_base)
            o.skip_tensor, o.jobs = wi.skip_dev.data_ptr(), wi.jobs_dev.data_ptr()
            o.job_tensor_host, o.job_tile_base_host = ctypes.cast(self.jt, ctypes.c_void_p), ctypes.cast(self.tb, ctypes.c_void_p)
            o.njobs = len(wi.job_tensor)
        o.nranges = len(ranges)
        for i, (lo, hi) in enumerate(ranges):
            o.range_lo[i], o.range_hi[i] = lo, hi
        o.gscale, o.clip, o.lr_t, o.beta1, o.beta2, o.eps = (float(h[k]) for k in ("gscale", "clip", "lr_t", "b1", "b2", "eps"))
        if after is not None:
            o.after_stream = after.cuda_stream
        self.desc = o

    def run(self):
        L.check(L.lib().yt8m_optimizer_ranges(ctypes.byref(self.desc), _st()))


def _same_bits(a, b, what):
    for k in ("w", "m", "v", "g", "norms"):
        assert (_bits(a[k]) == _bits(b[k])).all(), (what, k)


@pytest.mark.parametrize("mode", ["plain", "side", "clip0"])
def test_optimizer_ranges_one_range(dev, chunk_case, mode):
    """The whole arena as one range: bitwise what ops.sqnorm_and_adam leaves, and within the float64 bounds.  side: the gradients are
    written by a side stream that is still busy when the call is made, and after_stream names it; clip0: no norm pass, after_stream is
    the calling stream itself (nothing to wait for)."""
    h = R.hyper(clip=0.0 if mode == "clip0" else 1.0)
    nT = len(chunk_case["sizes"])
    twin = _graph(dev, chunk_case)
    ops.sqnorm_and_adam(twin, float(h["lr_t"]), **_hp(h))
    want = _state(twin)
    g = _graph(dev, chunk_case)
    after = None
    if mode == "side":
        g.grads.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        src = torch.from_numpy(chunk_case["g"]).to(dev)
        busy = torch.ones((2048, 2048), device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(8):
                busy = (busy @ busy) * (1.0 / 2048.0)
            g.grads.copy_(src)
        after = side
    elif mode == "clip0":
        after = torch.cuda.current_stream()
    r = _Ranges(g, [(0, nT)], h, after=after)
    r.run()
    got = _state(g)
    _same_bits(got, want, "ranges %s" % mode)
    _check("optimizer_ranges one range (%s)" % mode, chunk_case, h, got)


def test_optimizer_ranges_two_disjoint_ranges(dev, chunk_case):
    h = R.hyper()
    twin = _graph(dev, chunk_case)
    for lo, hi in R.TWO_RANGES:
        ops.sqnorm_and_adam(twin, float(h["lr_t"]), tensors=(lo, hi), **_hp(h))
    g = _graph(dev, chunk_case)
    _Ranges(g, R.TWO_RANGES, h).run()
    got = _state(g)
    _same_bits(got, _state(twin), "two ranges")
    ref = _check("optimizer_ranges %s" % (R.TWO_RANGES,), chunk_case, h, got, tensors=R.TWO_RANGES)
    lo, hi = chunk_case["offsets"][5], chunk_case["offsets"][9]
    assert not ((ref["updated"] >= lo) & (ref["updated"] < hi)).any()         # tensors 5 .. 8 lie between the ranges


# ---- tile pass ----------------------------------------------------------------------------------------------------------------------------
TILE_KEYS = [(0, 0, 64, 0, 3, 1.0), (0, 0, 64, 1, 3, 1.0),
             (1, 0, 65, 0, 1, 1.0), (1, 0, 65, 1, 3, 1.0), (1, 64, 1, 0, 3, 1.0),                       # a one-row window that ends with the matrix
             (3, 0, 130, 0, 3, 1.0), (3, 0, 130, 1, 1, 1.0), (3, 0, 128, 1, 3, ALPHA), (3, 128, 2, 0, 1, 1.0),
             (4, 0, 33, 0, 3, 1.0), (4, 0, 33, 1, 3, 1.0),
             (5, 64, 64, 0, 3, 1.0), (5, 128, 64, 1, 1, 2.0), (5, 0, 192, 0, 1, 1.0),
             (6, 0, 200, 0, 3, 1.0), (6, 0, 200, 1, 3, 1.0), (6, 0, 128, 1, 3, ALPHA), (6, 128, 72, 0, 1, 1.0)]


def _matrix(case, arena, t):
    o, n = case["offsets"][t], case["sizes"][t]
    return arena[o:o + n].reshape(case["shapes"][t])


def _image_want(case, w, key):
    """oracle/x3_ref.py on the float32 weights `w` (arena): window rows, transposed for trans, times scale; one plane = plane 0."""
    t, row0, rows, trans, planes, scale = key
    x = _matrix(case, w, t)[row0:row0 + rows]
    img = X.image(x.T if trans else x, scale)
    return np.ascontiguousarray(img[:, :, :1] if planes == 1 else img)


def _images(g):
    torch.cuda.synchronize()
    return dict((k, buf.cpu().numpy().view(np.uint16).copy()) for k, buf in g.wimg.keys.items())


def _check_images(name, case, w, have, keys):
    for k in keys:
        want = _image_want(case, w, k)
        assert have[k].size == want.size, (name, k, have[k].size, want.size)
        bad = int((have[k] != want.ravel()).sum())
        print("%s: image %s: %d of %d halfwords differ from oracle/x3_ref.py" % (name, k, bad, want.size))
        assert bad == 0, (name, k)


def _tile_graph(dev, case):
    g = _graph(dev, case)
    assert g.wimg is not None and not g.wimg.active
    g.wimg.add(TILE_KEYS)
    assert g.wimg.active and sorted(g.wimg.keys) == sorted(TILE_KEYS) and g.wimg.job_tensor == [0, 1, 3, 4, 5, 6]
    assert g.wimg.tile_base == [0, 1, 3, 9, 13, 16, 28]
    return g


def test_tile_pass(dev):
    case = R.tile_case()
    h = R.hyper()
    g = _tile_graph(dev, case)
    try:
        s0 = _state(g)                                                         # first build (do_adam = 0): images only, no arena written
        for k in "wmvg":
            assert (_bits(s0[k]) == _bits(case[k])).all(), k
        _check_images("tile pass, first build", case, s0["w"], _images(g), TILE_KEYS)
        ops.sqnorm_and_adam(g, float(h["lr_t"]), **_hp(h))                     # six jobs from tile 0; the vector through the chunk pass
        s1 = _state(g)
        _check("tile pass", case, h, s1)
        assert float(np.abs(s1["w"][:4096] - case["w"][:4096]).max()) > 1e-4
        im1 = _images(g)
        _check_images("tile pass, adam", case, s1["w"], im1, TILE_KEYS)
        # jobs 2 .. 4 of the array (tensors 3, 4, 5): tile0 = 3 > 0; the images of the other jobs keep their bytes
        case2 = R.next_step_case(case, s1["w"], s1["m"], s1["v"], 22)
        _load(g, case2, only_grads=True)
        g.norms.copy_(torch.from_numpy(s1["norms"]))
        ops.sqnorm_and_adam(g, float(h["lr_t"]), tensors=(3, 6), **_hp(h))
        s2 = _state(g)
        _check("tile pass tensors (3, 6)", case2, h, s2, tensors=[(3, 6)], norms_before=s1["norms"])
        im2 = _images(g)
        inside = [k for k in TILE_KEYS if 3 <= k[0] < 6]
        _check_images("tile pass tensors (3, 6)", case2, s2["w"], im2, inside)
        for k in TILE_KEYS:
            if k not in inside:
                assert (im2[k] == im1[k]).all(), k
            else:
                assert (im2[k] != im1[k]).any(), k
    finally:
        g.wimg.close()


def test_optimizer_ranges_with_image_jobs(dev):
    """Ranges (0, 2) and (4, 6) of the tile arena: jobs 0, 1 and 3, 4 lie inside, jobs 2 (tensor 3) and 5 (tensor 6) and the vector
    outside.  Bitwise the ops.sqnorm_and_adam result over the same tensors, images included; outside nothing moves."""
    case = R.tile_case()
    h = R.hyper()
    ranges = [(0, 2), (4, 6)]
    twin, g = _tile_graph(dev, case), None
    try:
        g = _tile_graph(dev, case)
        im0 = _images(g)
        for lo, hi in ranges:
            ops.sqnorm_and_adam(twin, float(h["lr_t"]), tensors=(lo, hi), **_hp(h))
        _Ranges(g, ranges, h).run()
        got = _state(g)
        _same_bits(got, _state(twin), "ranges with jobs")
        _check("optimizer_ranges with image jobs", case, h, got, tensors=ranges)
        im, imt = _images(g), _images(twin)
        inside = [k for k in TILE_KEYS if k[0] in (0, 1, 4, 5)]
        _check_images("optimizer_ranges with image jobs", case, got["w"], im, inside)
        for k in TILE_KEYS:
            assert (im[k] == imt[k]).all(), k
            if k not in inside:
                assert (im[k] == im0[k]).all(), k
    finally:
        twin.wimg.close()
        if g is not None:
            g.wimg.close()


# ---- h2 images ------------------------------------------------------------------------------------------------------------------------------
H2_KEYS = [(t, 0, R.H2_SHAPES[t][0], trans, 2, 0.0) for t in range(3) for trans in (0, 1)]


def _h2_words(g):
    torch.cuda.synchronize()
    return dict((k, whole[:8].cpu().numpy().view(np.uint32).copy()) for k, whole in g.wimg.h2_whole.items())


def _h2_scale(word0):
    """2^(14 - e) with e from frexp of the float whose bits are word 0 (csrc/x3_image.h pow2_scale_for); 1 for a vanishing maximum."""
    m = np.array([word0], dtype=np.uint32).view(np.float32)[0]
    if not (m > 7.9e-31) or not (m < 3.0e38):
        return 1.0
    return float(np.ldexp(1.0, 14 - int(np.frexp(m)[1])))


def _check_h2(name, case, w, words, images, made_under):
    """Header word 1 = max |w| of the float32 weights as they are; word 0 = `made_under`; the image = x3_ref.image_h2 of the weights under
    the power of two that word 0 gives."""
    for k in H2_KEYS:
        t, row0, rows, trans, planes, scale = k
        x = _matrix(case, w, t)
        mx = np.array([np.abs(x).max()], dtype=np.float32).view(np.uint32)[0]
        assert words[k][1] == mx, (name, k, "word 1", words[k], mx)
        assert words[k][0] == made_under[t], (name, k, "word 0", words[k], made_under[t])
        sc = _h2_scale(words[k][0])
        want = X.image_h2(x.T if trans else x, sc)
        bad = int((images[k] != want.ravel()).sum()) if images[k].size == want.size else -1
        print("%s: h2 image %s under 2^%d: %d of %d halfwords differ from oracle/x3_ref.py" % (name, k, int(np.log2(sc)), bad, want.size))
        assert bad == 0, (name, k)


def test_h2_images(dev):
    case = R.h2_case()
    g = _graph(dev, case)
    try:
        g.wimg.add(H2_KEYS)
        assert sorted(g.wimg.h2_whole) == sorted(H2_KEYS)
        s = _state(g)
        mx0 = [np.array([np.abs(_matrix(case, s["w"], t)).max()], dtype=np.float32).view(np.uint32)[0] for t in range(3)]
        assert mx0[2] == 0
        _check_h2("h2 first build", case, s["w"], _h2_words(g), _images(g), mx0)
        exps = [[int(np.frexp(np.array([b], dtype=np.uint32).view(np.float32)[0])[1]) for b in mx0[:2]]]
        prev = mx0
        for i, lr in enumerate(R.H2_LR):
            if i > 0:                                                          # (the same gradients as R.host_cases)
                fresh = R.make_case(R.H2_SHAPES, 29 + i)["g"]
                o, n = case["offsets"][2], case["sizes"][2]
                fresh[o:o + n] = 0.0                                           # the all-zero matrix keeps zero gradients
                g.grads.copy_(torch.from_numpy(fresh))
            h = R.hyper(lr_t=lr)
            ops.sqnorm_and_adam(g, float(h["lr_t"]), **_hp(h))
            s = _state(g)
            for k in "wmv":
                assert R.padding_intact(case, s[k]), k
            words = _h2_words(g)
            _check_h2("h2 step %d" % (i + 1), case, s["w"], words, _images(g), prev)        # made under the PREVIOUS maximum
            prev = [words[(t, 0, R.H2_SHAPES[t][0], 0, 2, 0.0)][1] for t in range(3)]
            exps.append([int(np.frexp(np.array([b], dtype=np.uint32).view(np.float32)[0])[1]) for b in prev[:2]])
        # step 2 (lr_t = 0.2) carried max |w| across a power of two: its image was made under the old scale, step 3's under the new one
        print("h2: exponents of max |w| after build and steps: %s" % (exps,))
        assert exps[0] == exps[1] and exps[2] == [e + 1 for e in exps[1]] and exps[3] == exps[2], exps
        o, n = case["offsets"][2], case["sizes"][2]
        assert not s["w"][o:o + n].any() and not s["m"][o:o + n].any() and not s["v"][o:o + n].any()
        for trans in (0, 1):
            k = (2, 0, 70, trans, 2, 0.0)
            assert (words[k] == 0).all() and not _images(g)[k].any()
    finally:
        g.wimg.close()


# ---- yt8m_clip_by_norm_f32 ------------------------------------------------------------------------------------------------------------------
PAD = 64


@pytest.mark.parametrize("above", [False, True], ids=["below", "above"])
@pytest.mark.parametrize("n", R.CLIP_N)
def test_clip_by_norm(dev, n, above):
    lib = L.lib()
    g = R.clip_case(n, above)
    want, bound = R.clip_reference(g, 1.0), R.clip_bound(g, 1.0)
    sent = R.sentinel(n + 2 * PAD)
    for inplace in (False, True):
        src = sent.copy()
        src[PAD:PAD + n] = g
        a = torch.from_numpy(src).to(dev)
        b = a if inplace else torch.from_numpy(sent.copy()).to(dev)
        ws = torch.from_numpy(R.sentinel(256 + 2 * PAD).copy()).to(dev)
        L.check(lib.yt8m_clip_by_norm_f32(_p(a, 4 * PAD), _p(b, 4 * PAD), n, 1.0, _p(ws, 4 * PAD), _st()))
        torch.cuda.synchronize()
        out, inp, wsh = b.cpu().numpy(), a.cpu().numpy(), ws.cpu().numpy()
        ratio = R.worst_ratio(out[PAD:PAD + n], want, bound)
        print("clip_by_norm n %d %s %s: error / bound %.3f (K = %g times 2^-24 of |out|)"
              % (n, "above" if above else "below", "in place" if inplace else "out of place", ratio, (1 + (n + 65535) // 65536 + 18) / 2.0 + 3.0))
        assert ratio <= 1.0
        for arr in (out, inp, wsh):
            assert (_bits(arr)[:PAD] == R.SENTINEL_BITS).all() and (_bits(arr)[-PAD:] == R.SENTINEL_BITS).all()
        if not inplace:
            assert (_bits(inp)[PAD:PAD + n] == _bits(g)).all()
        if not above:
            assert (_bits(out)[PAD:PAD + n] == _bits(g)).all()                 # the factor is max_norm / max_norm: the input bit for bit
        else:
            assert float(np.abs(np.sqrt(np.sum(out[PAD:PAD + n].astype(np.float64) ** 2)) - 1.0)) < 1e-5


def test_clip_by_norm_empty(dev):
    a = torch.from_numpy(R.sentinel(PAD).copy()).to(dev)
    L.check(L.lib().yt8m_clip_by_norm_f32(_p(a), _p(a), 0, 1.0, _p(a), _st()))
    torch.cuda.synchronize()
    assert (_bits(a.cpu().numpy()) == R.SENTINEL_BITS).all()
