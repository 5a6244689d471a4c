"""-m gpu: every dispatch branch of the streaming / pointwise kernels (csrc/elementwise.hip, the pointwise part of csrc/sequence.hip,
csrc/dbof.hip, csrc/netvlad.hip) through the C ABI against fp64, at both sides of each shape threshold, at the models' own shapes, from
16-byte aligned and from 4-byte aligned base pointers, with sentinel margins around every operand and with the refusals of each entry
point.  tests/test_gpu_kernels.py and tests/test_gpu_round2.py keep the quick small-shape checks of the same entry points.

BRANCH_TABLE below is the reading of the dispatchers this module was written from: one row per `if` / `else` / `switch` arm of each
entry point (and per in-kernel path choice of dequant_l2norm_kernel), as (entry point, condition as written in the .hip file, kernel
launched, case of this module that takes it).  tests/test_streaming_branch_table.py checks every kernel named here against the sources
and every __global__ of those sources against the kernel list recorded from a profiled run of this module
(tests/golden/streaming_kernels_seen.txt, profiles/streaming_branches_kernel_stats.csv): a new dispatch condition comes with its row.

Bounds.  Pointwise results keep the project's constants (1e-6 activations and l2norm values, 2e-6 mixing, 2e-5 relative for the
cross-entropy loss and gradient, 1e-5 for the l2norm / softmax backward, 2e-5 for batch norm outputs); integer work, copies, casts and
maxima are compared bit for bit.  Every sum over rows or columns at a large shape (batch-norm moments and column sums, colsum,
colsum_weighted, the norms of 73728-column rows) is held to FOUR times the error of torch's own fp32 evaluation of the same expression
against fp64, measured on the same data -- never to anything the kernel under test produced.  Each case prints its error and bound.

Thresholds left out because one operand would exceed 1 GB: rows > 65536 at cols >= 8192 for l2norm (2.1 GB per operand)."""
import ctypes

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L

pytestmark = pytest.mark.gpu

BRANCH_TABLE = [
    # ---- elementwise.hip ------------------------------------------------------------------------------------------------------------
    ("yt8m_l2norm_fwd_f32", "cols >= 8192 && (cols & 3) == 0 && x, y 16-byte aligned && rows <= 65536", "l2norm_long_kernel<false>",
     "test_l2norm_branches[3-8192-0], [2-73728-0]"),
    ("yt8m_l2norm_fwd_f32", "else if cols >= 512 && rows <= 16384", "l2norm_fwd_row_kernel",
     "test_l2norm_branches[3-8188-0] (cols one step below 8192), [3-8194-0] (cols % 4 != 0), [3-8192-1] and [2-73728-1] (4-byte aligned), "
     "[3-512-0], [16384-512-0]"),
    ("yt8m_l2norm_fwd_f32", "else", "l2norm_fwd_kernel", "test_l2norm_branches[3-511-0], [16385-512-0], [38400-1152-0] (frame normalisation)"),
    ("yt8m_l2norm_fwd_f32", "rows > 65536 at cols >= 8192 (falls to the generic kernel)", "l2norm_fwd_kernel",
     "left out: 65537 x 8192 floats are 2.1 GB per operand"),
    ("yt8m_l2norm_bwd_f32", "cols >= 8192 && (cols & 3) == 0 && x, dy, dx 16-byte aligned && rows <= 65536", "l2norm_long_kernel<true>",
     "test_l2norm_branches[3-8192-0], [2-73728-0]"),
    ("yt8m_l2norm_bwd_f32", "else", "l2norm_bwd_kernel", "test_l2norm_branches: every other case"),
    ("yt8m_act_fwd_f32", "grid_for(n, 256, 8192): n <= 8192 * 256 one pass, above it the grid-stride loop", "act_fwd_kernel",
     "test_activation_grid_cap[*-2097152], [*-2097153], [*-4194381]"),
    ("yt8m_act_bwd_f32", "grid_for(n, 256, 8192)", "act_bwd_kernel", "test_activation_grid_cap (same n)"),
    ("yt8m_moe_mix_fwd", "switch (M) case 1", "moe_mix_fwd_kernel<1>", "test_moe_mix_head_shapes[*-4716-1]"),
    ("yt8m_moe_mix_fwd", "switch (M) case 2", "moe_mix_fwd_kernel<2>", "test_moe_mix_head_shapes[*-4716-2], [3-4717-2] (BV % 256 != 0)"),
    ("yt8m_moe_mix_fwd", "switch (M) case 4", "moe_mix_fwd_kernel<4>", "test_moe_mix_head_shapes[*-4716-4]"),
    ("yt8m_moe_mix_fwd", "switch (M) case 8", "moe_mix_fwd_kernel<8>", "test_moe_mix_head_shapes[*-4716-8]"),
    ("yt8m_moe_mix_fwd", "switch (M) default", "moe_mix_fwd_kernel<0>", "test_moe_mix_head_shapes[*-4716-3], [*-4716-16]"),
    ("yt8m_moe_mix_bwd", "switch (M) case 1", "moe_mix_bwd_kernel<1>", "test_moe_mix_head_shapes[*-4716-1]"),
    ("yt8m_moe_mix_bwd", "switch (M) case 2", "moe_mix_bwd_kernel<2>", "test_moe_mix_head_shapes[*-4716-2]"),
    ("yt8m_moe_mix_bwd", "switch (M) case 4", "moe_mix_bwd_kernel<4>", "test_moe_mix_head_shapes[*-4716-4]"),
    ("yt8m_moe_mix_bwd", "switch (M) case 8", "moe_mix_bwd_kernel<8>", "test_moe_mix_head_shapes[*-4716-8]"),
    ("yt8m_moe_mix_bwd", "switch (M) default", "moe_mix_bwd_kernel<0>", "test_moe_mix_head_shapes[*-4716-3], [*-4716-16]"),
    ("yt8m_moe_mix_xent_fwd", "label_dtype == YT8M_LABEL_U8, switch (M) 1 / 2 / 4 / 8 / default",
     "moe_mix_xent_fwd_kernel<1, unsigned char> moe_mix_xent_fwd_kernel<2, unsigned char> moe_mix_xent_fwd_kernel<4, unsigned char> "
     "moe_mix_xent_fwd_kernel<8, unsigned char> moe_mix_xent_fwd_kernel<0, unsigned char>", "test_moe_mix_xent_instantiations[u8-*]"),
    ("yt8m_moe_mix_xent_fwd", "else (float labels), switch (M) 1 / 2 / 4 / 8 / default",
     "moe_mix_xent_fwd_kernel<1, float> moe_mix_xent_fwd_kernel<2, float> moe_mix_xent_fwd_kernel<4, float> "
     "moe_mix_xent_fwd_kernel<8, float> moe_mix_xent_fwd_kernel<0, float>", "test_moe_mix_xent_instantiations[f32-*]"),
    ("yt8m_moe_mix_xent_fwd", "(always) the per-workgroup partials", "final_sum_kernel", "every test_moe_mix_xent_* case"),
    ("yt8m_moe_mix_xent_bwd", "zmax == NULL: per_wg = 256; labels u8 / float, switch (M)",
     "moe_mix_xent_bwd_kernel<1, unsigned char> moe_mix_xent_bwd_kernel<2, unsigned char> moe_mix_xent_bwd_kernel<4, unsigned char> "
     "moe_mix_xent_bwd_kernel<8, unsigned char> moe_mix_xent_bwd_kernel<0, unsigned char> moe_mix_xent_bwd_kernel<1, float> "
     "moe_mix_xent_bwd_kernel<2, float> moe_mix_xent_bwd_kernel<4, float> moe_mix_xent_bwd_kernel<8, float> "
     "moe_mix_xent_bwd_kernel<0, float>", "test_moe_mix_xent_instantiations"),
    ("yt8m_moe_mix_xent_bwd_absmax", "zmax != NULL: per_wg = 256 * ZMAX_IT = 2048 labels; same kernels", "moe_mix_xent_bwd_kernel",
     "test_moe_mix_xent_chunks[23-89] (BV = 2047: below one chunk), [32-64] (2048), [3-683] (2049), [7-1000] (partial last chunk), "
     "[128-4716] (the head)"),
    ("yt8m_xent_fwd_bwd", "B <= 65535 else YT8M_E_SHAPE", "(none)", "test_xent_rejects_large_batch"),
    ("yt8m_xent_fwd_bwd", "label_dtype == YT8M_LABEL_U8", "xent_kernel<unsigned char>",
     "test_xent_block_edges[u8-*]: V = 1023, 1024, 1025, 2048, 2049, 4716; B = 1 and 9"),
    ("yt8m_xent_fwd_bwd", "else (float labels)", "xent_kernel<float>", "test_xent_block_edges[f32-*]"),
    ("yt8m_xent_fwd_bwd", "(always) the per-workgroup partials", "final_sum_kernel", "test_xent_block_edges"),
    ("yt8m_xent_bwd", "B <= 65535 else YT8M_E_SHAPE; label_dtype u8 / float", "xent_kernel<unsigned char> xent_kernel<float>",
     "test_xent_block_edges, test_xent_rejects_large_batch"),
    ("yt8m_colsum_f32", "beta == 0 || beta == 1 else YT8M_E_BADARG; ldx >= cols else YT8M_E_SHAPE", "(none)", "test_colsum_rejections"),
    ("yt8m_colsum_f32", "workspace && colblocks < 512 && rows >= 4096, and nsplit * cols * 4 <= workspace_bytes: nsplit > 1",
     "colsum_kernel colsum_finish_kernel",
     "test_colsum_branches[4096-200-full], [4096-200-exact], [38400-64-full] (partial last row block), [4096-32704-full] (colblocks = 511)"),
    ("yt8m_colsum_f32", "workspace too small: nsplit = 1", "colsum_kernel", "test_colsum_branches[4096-200-short], [9000-72-short]"),
    ("yt8m_colsum_f32", "no workspace, rows < 4096 or colblocks >= 512: nsplit <= 1", "colsum_kernel",
     "test_colsum_branches[4096-200-none], [4095-200-full], [4096-32705-full] (colblocks = 512), [1-1-full]"),
    ("yt8m_colsum_weighted_f32", "the same three arms with 2 * nsplit * cols * 4 <= workspace_bytes", "colsum2_kernel colsum_finish_kernel",
     "test_colsum_branches (every case runs both entry points)"),
    ("yt8m_cast_f32_bf16", "transpose && cast_vec_ok(src, rows, cols, ld, true) && dal", "cast_bf16_tile_kernel<false, true>",
     "test_cast_bf16_branches[64-128-8-8-0-0], [4100-4100-0-0-0-0]"),
    ("yt8m_cast_f32_bf16", "transpose, else", "cast_bf16_transpose_kernel",
     "test_cast_bf16_branches[66-128-...] (rows % 4), [64-130-...] (cols % 4), [64-128-3-...] (ld % 4), [64-128-8-2-...] (dst_ld % 4), "
     "[...-1-0] (source 4-byte aligned), [...-0-1] / [...-0-2] (destination 2- / 4-byte aligned)"),
    ("yt8m_cast_f32_bf16", "else if cast_vec_ok(src, rows, cols, ld, false) && dal", "cast_bf16_vec_kernel",
     "test_cast_bf16_branches[64-128-8-8-0-0], [66-128-8-8-0-0] (rows % 4 does not matter here), [4100-4100-0-0-0-0] (grid cap 16384)"),
    ("yt8m_cast_f32_bf16", "else", "cast_bf16_kernel", "test_cast_bf16_branches: the misaligned / odd cases above, [4100-4100-0-0-1-0] (grid cap)"),
    ("yt8m_cast_f32_bf16", "dst_ld == 0: the tight leading dimension; ld < cols, dst_ld too small: YT8M_E_SHAPE", "(none)",
     "test_cast_bf16_default_ld_and_rejections"),
    ("yt8m_cast_f32_bf16_dual", "cast_vec_ok(..., true) && both destinations 8-byte aligned && plain_ld % 4 == 0 && trans_ld % 4 == 0",
     "cast_bf16_tile_kernel<true, true>", "test_cast_bf16_branches[64-128-8-8-0-0], [4100-4100-0-0-0-0]"),
    ("yt8m_cast_f32_bf16_dual", "else: two passes of yt8m_cast_f32_bf16", "cast_bf16_vec_kernel cast_bf16_kernel cast_bf16_transpose_kernel",
     "test_cast_bf16_branches: every other case ([66-128-8-8-0-0]: vector plain pass + scalar transpose)"),
    ("yt8m_dequant_l2norm_u8", "in kernel: !live (f >= num_frames[b])", "dequant_l2norm_kernel", "test_dequant_l2norm_paths: num_frames 0, 1, F"),
    ("yt8m_dequant_l2norm_u8", "in kernel: (D & 3) == 0 && D <= 2048 && q, x 16-byte aligned", "dequant_l2norm_kernel",
     "test_dequant_l2norm_paths[4-0-0], [260-0-0], [1152-0-0], [2048-0-0]"),
    ("yt8m_dequant_l2norm_u8", "in kernel: else (byte loop)", "dequant_l2norm_kernel",
     "test_dequant_l2norm_paths[2052-0-0] (D > 2048), [1150-0-0] (D % 4), [1152-1-0] (q off by a byte), [1152-0-1] (x off by a float)"),
    ("yt8m_moe_mix_fwd_bf16z", "M == 2 && B V % 4 == 0 && operands 16-byte aligned, else YT8M_E_BADARG / YT8M_E_SHAPE", "moe_mix_fwd_bf16z_kernel",
     "test_moe_mix_fwd_bf16z (no other test calls this entry point directly)"),
    ("yt8m_rank1_add_rows_f32", "cols % 4 == 0 && ldc % 4 == 0 && C, v 16-byte aligned, else YT8M_E_SHAPE", "rank1_rows_kernel",
     "test_rank1_add_rows (no other test calls this entry point)"),
    # ---- sequence.hip (pointwise part) ----------------------------------------------------------------------------------------------
    ("yt8m_attn_softmax_fwd", "(single kernel) one wave per (b, a), lanes stride F", "attn_softmax_fwd_kernel",
     "test_attn_softmax_shapes[128-300-8] (the model), [5-64-3], [5-65-3] (lane edge), [3-1-2]"),
    ("yt8m_attn_softmax_bwd", "(single kernel)", "attn_softmax_bwd_kernel", "test_attn_softmax_shapes"),
    ("yt8m_softmax_rows_fwd", "(single kernel) one wave per row, lanes stride K; masked rows", "softmax_rows_fwd_kernel",
     "test_softmax_rows_shapes: K = 1, 63, 64, 65, 100, 4096; [128-300-64] (NetVLAD)"),
    ("yt8m_softmax_rows_bwd", "(single kernel)", "softmax_rows_bwd_kernel", "test_softmax_rows_shapes"),
    ("yt8m_topk_rows", "k >= 1 && k <= 64 && k <= V else YT8M_E_BADARG; V * 4 <= 150 KB else YT8M_E_SHAPE", "(none)", "test_topk_perr_rejections"),
    ("yt8m_topk_rows", "shm <= 64 KB", "topk_rows_kernel", "test_topk_rows_lds[4716-64], [16384-20]"),
    ("yt8m_topk_rows", "shm > 64 KB: hipFuncSetAttribute(MaxDynamicSharedMemorySize) first", "topk_rows_kernel",
     "test_topk_rows_lds[16385-20], [38400-64]"),
    ("yt8m_perr_rows", "V * 8 <= 150 KB else YT8M_E_SHAPE", "(none)", "test_topk_perr_rejections"),
    ("yt8m_perr_rows", "shm <= 64 KB", "perr_rows_kernel", "test_perr_rows_lds[4716], [8192]"),
    ("yt8m_perr_rows", "shm > 64 KB: hipFuncSetAttribute first", "perr_rows_kernel", "test_perr_rows_lds[8193], [19200]"),
    # ---- dbof.hip -------------------------------------------------------------------------------------------------------------------
    ("yt8m_frame_pool_fwd", "B < 65536 else YT8M_E_SHAPE; mode 0 / 1 else YT8M_E_BADARG", "(none)", "test_frame_pool_rejections"),
    ("yt8m_frame_pool_fwd", "(C & 3) == 0 && x, out 16-byte aligned", "frame_pool_fwd_kernel<4>",
     "test_frame_pool_branches[*-128-30-8192] (DBoF), [*-3-16-72], [*-3-17-72], [*-2-30-1024], [*-2-30-1028], [*-4-1-12]"),
    ("yt8m_frame_pool_fwd", "else", "frame_pool_fwd_kernel<1>", "test_frame_pool_branches[*-3-16-70], [*-3-17-70]; every C % 4 == 0 case again "
     "from 4-byte aligned pointers"),
    ("yt8m_frame_pool_bwd", "(C & 3) == 0 && x, out, dy, dx 16-byte aligned", "frame_pool_bwd_kernel<4>",
     "as the forward; in kernel: mode != 0 (average), S <= 16 (register-resident: S = 1, 16), S > 16 (S = 17, 30)"),
    ("yt8m_frame_pool_bwd", "else", "frame_pool_bwd_kernel<1>", "as the forward"),
    ("yt8m_batchnorm_fwd", "training", "bn_stats_kernel bn_apply_kernel",
     "test_batchnorm_branches[1-1-64] .. [1-5-65] (N below / at / above the 4 row lanes, C at 64 / 65), [1-3840-8192] (DBoF: 128 x 30 rows), "
     "[1-30720-512] (1024 x 30 rows: the serial sums at full length; C shrunk to stay under 1 GB)"),
    ("yt8m_batchnorm_fwd", "else (frozen statistics)", "bn_frozen_stats_kernel bn_apply_kernel", "test_batchnorm_branches[0-5-65], [0-300-130]"),
    ("yt8m_batchnorm_bwd", "workspace_bytes >= 2 C floats else YT8M_E_SHAPE", "(none)", "test_batchnorm_branches (every case)"),
    ("yt8m_batchnorm_bwd", "(always)", "bn_bwd_reduce_kernel", "test_batchnorm_branches"),
    ("yt8m_batchnorm_bwd", "dgamma || dbeta", "bn_param_grads_kernel", "test_batchnorm_branches: both given (beta 0, then 1), both NULL"),
    ("yt8m_batchnorm_bwd", "dx", "bn_bwd_apply_kernel", "test_batchnorm_branches: given, NULL; training and frozen"),
    # ---- netvlad.hip ----------------------------------------------------------------------------------------------------------------
    ("yt8m_vlad_finish_fwd", "vlad_reg_ok: D >= 4 && D <= 2048 && (D & 3) == 0 && agg, centres, vlad 16-byte aligned", "vlad_finish_fwd_reg_kernel",
     "test_vlad_finish_branches[4-0], [8-0], [1152-0], [2048-0]; in kernel: a given / NULL (n_out precomputed)"),
    ("yt8m_vlad_finish_fwd", "else", "vlad_finish_fwd_kernel", "test_vlad_finish_branches[2052-0] (D > 2048), [1150-0], [6-0] (D % 4), [1152-1] (4-byte aligned)"),
    ("yt8m_vlad_finish_q_fwd", "register form as above; else q_out given: YT8M_E_SHAPE", "vlad_finish_fwd_reg_kernel", "test_vlad_finish_branches"),
    ("yt8m_vlad_finish_bwd", "vlad_reg_ok(D, agg, centres, dvlad, dagg)", "vlad_finish_bwd_reg_kernel", "test_vlad_finish_branches (register cases)"),
    ("yt8m_vlad_finish_bwd", "else", "vlad_finish_bwd_kernel", "test_vlad_finish_branches (generic cases)"),
    ("yt8m_vlad_finish_bwd", "dcentres (beta 0 / 1; other beta: YT8M_E_BADARG)", "vlad_dcentres_kernel", "test_vlad_finish_branches: given (0, 1), NULL"),
    ("yt8m_vlad_finish_q_bwd", "register form with dq (clamped row (b, k) = (0, 0)); else dq given: YT8M_E_SHAPE", "vlad_finish_bwd_reg_kernel",
     "test_vlad_finish_branches"),
]

EPS32 = float(np.finfo(np.float32).eps)
PAD = 64              # elements of sentinel on each side of a guarded operand (a multiple of 16 bytes for every dtype used)
SENT = -7.0


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class G:
    """A flat operand of n elements inside a larger sentinel-filled buffer; shift = 1 moves its base off 16-byte alignment by one
    element (which selects the scalar form of every entry point that has a vector path)."""

    def __init__(self, dev, n, shift=0, dtype=torch.float32, fill=SENT):
        self.fill, self.n, self.lo = fill, int(n), PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 4,), fill, dtype=dtype, device=dev)
        self.t = self.buf[self.lo:self.lo + self.n]

    def put(self, src):
        self.t.copy_(src.reshape(-1))
        return self

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def view(self, *shape):
        return self.t.view(*shape)

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    return g


def _randn(dev, seed, *shape):
    return torch.randn(*shape, generator=_gen(dev, seed), device=dev)


def _rand(dev, seed, *shape):
    return torch.rand(*shape, generator=_gen(dev, seed), device=dev)


def _maxerr(a, ref64):
    return float((a.double() - ref64).abs().max())


def _report(what, err, bound):
    print("%s: err %.3g (bound %.3g)" % (what, err, bound))
    assert err <= bound, "%s: err %.6g > bound %.6g" % (what, err, bound)


def _rowscaled(a, ref64):
    """max over rows of max|a - ref| / max(1, max|ref|) of that row (a clamped l2 row carries a 1e6 factor that must not set the scale
    of the others)."""
    e = (a.double() - ref64).abs().flatten(1).amax(1) if ref64.dim() > 1 else (a.double() - ref64).abs()
    s = ref64.abs().flatten(1).amax(1).clamp(min=1.0) if ref64.dim() > 1 else ref64.abs().clamp(min=1.0)
    return float((e / s).max())


# ================================================================================================================================
# l2norm
L2_CASES = [(3, 8192, 0), (3, 8188, 0), (3, 8194, 0), (3, 8192, 1), (2, 73728, 0), (2, 73728, 1), (3, 512, 0), (3, 511, 0), (16384, 512, 0),
            (16385, 512, 0), (38400, 1152, 0), (38400, 1152, 1)]


@pytest.mark.parametrize("rows,cols,shift", L2_CASES)
def test_l2norm_branches(dev, rows, cols, shift):
    lib, eps = L.lib(), 1e-12
    n = rows * cols

    def inputs():
        x = _randn(dev, 7 + cols, rows, cols)
        x[1] = 0.0                                                   # zero rows stay zero; their gradient is r dy with r = 1e6
        return x, _randn(dev, 8 + cols, rows, cols)

    gx, gdy, gy, gdx = G(dev, n, shift), G(dev, n, shift), G(dev, n, shift), G(dev, n, shift)
    xin, dyin = inputs()
    gx.put(xin), gdy.put(dyin)
    del xin, dyin
    L.check(lib.yt8m_l2norm_fwd_f32(gx.p, gy.p, rows, cols, eps, _st()))
    L.check(lib.yt8m_l2norm_bwd_f32(gx.p, gdy.p, gdx.p, rows, cols, eps, _st()))
    ef = eb = ef4 = eb4 = tf4 = tb4 = 0.0
    for r0 in range(0, rows, 4096):                                   # rows are independent: fp64 restatement 4096 at a time
        sl = slice(r0, min(r0 + 4096, rows))
        x, dy, y, dx = (g.view(rows, cols)[sl] for g in (gx, gdy, gy, gdx))
        x64, dy64 = x.double(), dy.double()
        ss = (x64 * x64).sum(1, keepdim=True)
        r = ss.clamp(min=eps).rsqrt()
        y64 = x64 * r
        k = torch.where(ss > eps, (x64 * dy64).sum(1, keepdim=True) * r * r, torch.zeros_like(ss))
        dx64 = r * (dy64 - x64 * k)
        ef, eb = max(ef, _maxerr(y, y64)), max(eb, _rowscaled(dx, dx64))
        if cols >= 65536:
            # the norm of a 73728-column row is a long sum: torch's own fp32 evaluation of the same expressions (the non-zero row)
            r32 = (x * x).sum(1, keepdim=True).clamp(min=eps).rsqrt()
            k32 = (x * dy).sum(1, keepdim=True) * r32 * r32
            ef4, tf4 = _maxerr(y[0], y64[0]), _maxerr((x * r32)[0], y64[0])
            eb4, tb4 = _maxerr(dx[0], dx64[0]), _maxerr((r32 * (dy - x * k32))[0], dx64[0])
    _report("l2norm fwd (%d,%d,+%d)" % (rows, cols, shift), ef, 1e-6)
    _report("l2norm bwd (%d,%d,+%d) rel" % (rows, cols, shift), eb, 1e-5)
    if cols >= 65536:
        _report("l2norm fwd long row vs 4 x torch fp32", ef4, 4 * tf4)
        _report("l2norm bwd long row vs 4 x torch fp32", eb4, 4 * tb4)
    assert bool((gy.view(rows, cols)[1] == 0).all())
    assert all(g.intact() for g in (gx, gdy, gy, gdx))
    xin, dyin = inputs()
    assert torch.equal(gx.view(rows, cols), xin) and torch.equal(gdy.view(rows, cols), dyin)


# ================================================================================================================================
# activations: the grid is capped at 8192 blocks of 256
ACT_CAP = 8192 * 256


def _act_ref(act, x64):
    return [torch.sigmoid(x64), x64.clamp(min=0), x64.clamp(0, 6), torch.tanh(x64), torch.where(x64 > 0, x64, torch.expm1(x64))][act]


def _act_grad_from_out(act, y64):
    one, zero = torch.ones_like(y64), torch.zeros_like(y64)
    return [y64 * (1 - y64), torch.where(y64 > 0, one, zero), torch.where((y64 > 0) & (y64 < 6), one, zero), 1 - y64 * y64,
            torch.where(y64 > 0, one, y64 + 1)][act]


@pytest.mark.parametrize("n", [ACT_CAP, ACT_CAP + 1, 2 * ACT_CAP + 77])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_activation_grid_cap(dev, act, n):
    lib = L.lib()
    x = _randn(dev, 20 + act, n) * 4
    x[:4] = torch.tensor([0.0, 6.0, -0.0, 9.0], device=dev)
    x[-1] = -9.0
    dy = _randn(dev, 30 + act, n)
    gx, gy, gdy, gdx = G(dev, n).put(x), G(dev, n), G(dev, n).put(dy), G(dev, n)
    L.check(lib.yt8m_act_fwd_f32(act, gx.p, gy.p, n, _st()))
    L.check(lib.yt8m_act_bwd_f32(act, gy.p, gdy.p, gdx.p, n, _st()))
    _report("act %d fwd n=%d" % (act, n), _maxerr(gy.t, _act_ref(act, x.double())), 1e-6)
    _report("act %d bwd n=%d" % (act, n), _maxerr(gdx.t, dy.double() * _act_grad_from_out(act, gy.t.double())), 1e-5)
    assert all(g.intact() for g in (gx, gy, gdy, gdx)) and torch.equal(gx.t, x)
    # the same data from a base pointer one element off: there is one kernel, so the result is the same bit for bit
    hx, hy, hdy, hdx = G(dev, n, 1).put(x), G(dev, n, 1), G(dev, n, 1).put(dy), G(dev, n, 1)
    L.check(lib.yt8m_act_fwd_f32(act, hx.p, hy.p, n, _st()))
    L.check(lib.yt8m_act_bwd_f32(act, hy.p, hdy.p, hdx.p, n, _st()))
    assert torch.equal(hy.t, gy.t) and torch.equal(hdx.t, gdx.t) and hy.intact() and hdx.intact()


def test_activation_rejections(dev):
    lib = L.lib()
    g = G(dev, 16)
    assert lib.yt8m_act_fwd_f32(5, g.p, g.p, 16, _st()) == -1 and lib.yt8m_act_fwd_f32(0, g.p, g.p, -1, _st()) == -2
    assert lib.yt8m_act_bwd_f32(-1, g.p, g.p, g.p, 16, _st()) == -1
    torch.cuda.synchronize()
    assert g.untouched()


# ================================================================================================================================
# MoE mixing at the head's shapes; inputs are made in blocks of 128 rows so that the fp64 restatement never holds more than one block
MIX_CH = 128


def _mix_block(dev, seed, b0, nb, V, M):
    g = _gen(dev, seed * 1000003 + b0)
    Zg = torch.randn(nb, V, M + 1, generator=g, device=dev) * 3
    Ze = torch.randn(nb, V, M, generator=g, device=dev) * 3
    dp = torch.randn(nb, V, generator=g, device=dev)
    if b0 == 0:                                                       # saturated softmax / sigmoid, as test_moe_mix_fwd_bwd
        Zg[0, 0, :] = -80.0
        Zg[0, 0, 0] = 80.0
        Ze[0, 0, :] = 90.0
        Ze[1, 0, :] = -90.0
        Zg[2, 1, :] = -80.0
        Zg[2, 1, M] = 80.0                                            # all the weight on the gate that has no expert
    return Zg, Ze, dp


def _mix_ref(Zg, Ze, M):
    g = torch.softmax(Zg.double(), -1)
    e = torch.sigmoid(Ze.double())
    p = (g[..., :M] * e).sum(-1)
    epad = torch.cat([e, torch.zeros_like(e[..., :1])], -1)
    return g, e, p, g * (epad - p[..., None]), g[..., :M] * e * (1 - e)      # dZg, dZe for dp = 1


@pytest.mark.parametrize("B,V,M", [(B, 4716, M) for B in (128, 1024) for M in (1, 2, 3, 4, 8, 16)] + [(3, 4717, 2)])      # last: B V % 256 != 0
def test_moe_mix_head_shapes(dev, B, V, M):
    lib = L.lib()
    BV = B * V
    gZg, gZe, gp, gdp = G(dev, BV * (M + 1)), G(dev, BV * M), G(dev, BV), G(dev, BV)
    Zg, Ze, p, dp = gZg.view(B, V, M + 1), gZe.view(B, V, M), gp.view(B, V), gdp.view(B, V)
    for b0 in range(0, B, MIX_CH):
        nb = min(MIX_CH, B - b0)
        Zg[b0:b0 + nb], Ze[b0:b0 + nb], dp[b0:b0 + nb] = _mix_block(dev, M, b0, nb, V, M)
    L.check(lib.yt8m_moe_mix_fwd(gZg.p, gZe.p, gp.p, B, V, M, _st()))
    L.check(lib.yt8m_moe_mix_bwd(gZg.p, gZe.p, gdp.p, B, V, M, _st()))      # in place: Zg, Ze now hold the gradients
    ep = eg = ee = 0.0
    for b0 in range(0, B, MIX_CH):
        nb = min(MIX_CH, B - b0)
        zg, ze, d = _mix_block(dev, M, b0, nb, V, M)
        assert torch.equal(d, dp[b0:b0 + nb])
        _, _, p64, dG, dE = _mix_ref(zg, ze, M)
        d64 = d.double()[..., None]
        ep = max(ep, _maxerr(p[b0:b0 + nb], p64))
        eg = max(eg, _maxerr(Zg[b0:b0 + nb], d64 * dG))
        ee = max(ee, _maxerr(Ze[b0:b0 + nb], d64 * dE))
    _report("moe_mix fwd [%d,%d] M=%d" % (B, V, M), ep, 2e-6)
    _report("moe_mix bwd dZg", eg, 2e-6)
    _report("moe_mix bwd dZe", ee, 2e-6)
    assert all(g.intact() for g in (gZg, gZe, gp, gdp))


def test_moe_mix_rejections(dev):
    lib = L.lib()
    g = G(dev, 64)
    assert lib.yt8m_moe_mix_fwd(g.p, g.p, g.p, 1, 1, 0, _st()) == -1 and lib.yt8m_moe_mix_fwd(g.p, g.p, g.p, 1, 1, 17, _st()) == -1
    assert lib.yt8m_moe_mix_bwd(g.p, g.p, g.p, 1, 1, 17, _st()) == -1 and lib.yt8m_moe_mix_fwd(g.p, g.p, g.p, -1, 1, 2, _st()) == -2
    torch.cuda.synchronize()
    assert g.untouched()


def test_moe_mix_fwd_bf16z(dev):
    """The M = 2 mixing on bf16 logits (four labels per thread): against fp64 on the rounded logits, 2e-6 as the fp32 form."""
    lib = L.lib()
    B, V, M = 9, 4716, 2                                              # B V / 4 = 10611: a partial last workgroup
    Zg, Ze, _ = _mix_block(dev, 40, 0, B, V, M)
    zg16, ze16 = Zg.to(torch.bfloat16), Ze.to(torch.bfloat16)
    gZg = G(dev, B * V * 3, 0, torch.int16, 0x5A5A).put(zg16.view(torch.int16))
    gZe = G(dev, B * V * 2, 0, torch.int16, 0x5A5A).put(ze16.view(torch.int16))
    gp = G(dev, B * V)
    L.check(lib.yt8m_moe_mix_fwd_bf16z(gZg.p, gZe.p, gp.p, B, V, M, _st()))
    _report("moe_mix_fwd_bf16z [%d,%d]" % (B, V), _maxerr(gp.view(B, V), _mix_ref(zg16.float(), ze16.float(), M)[2]), 2e-6)
    assert gp.intact() and gZg.intact() and gZe.intact()
    out = G(dev, 64)
    assert lib.yt8m_moe_mix_fwd_bf16z(gZg.p, gZe.p, out.p, 1, 8, 4, _st()) == -1          # M != 2
    assert lib.yt8m_moe_mix_fwd_bf16z(gZg.p, gZe.p, out.p, 1, 7, 2, _st()) == -2          # B V % 4
    off = G(dev, 64, 1)
    assert lib.yt8m_moe_mix_fwd_bf16z(gZg.p, gZe.p, off.p, 1, 8, 2, _st()) == -1          # 4-byte aligned output
    torch.cuda.synchronize()
    assert out.untouched() and off.untouched()


def test_rank1_add_rows(dev):
    """C[r, :] += scale v: one multiply-add per element (contracted or not: two roundings of the result's size at most)."""
    lib = L.lib()
    rows, cols, ldc, scale = 37, 1152, 1156, -0.37
    C0, v = _randn(dev, 45, rows, cols), _randn(dev, 46, cols)
    gC, gv = G(dev, rows * ldc), G(dev, cols).put(v)
    gC.view(rows, ldc)[:, :cols] = C0
    L.check(lib.yt8m_rank1_add_rows_f32(gC.p, rows, cols, ldc, gv.p, scale, _st()))
    s64 = float(np.float32(scale))
    want = C0.double() + s64 * v.double()
    bound = 2 * EPS32 * float((C0.double().abs() + abs(s64) * v.double().abs()).max())
    _report("rank1_add_rows (%d,%d) ldc=%d" % (rows, cols, ldc), _maxerr(gC.view(rows, ldc)[:, :cols], want), bound)
    assert gC.intact() and gv.intact() and bool((gC.view(rows, ldc)[:, cols:] == SENT).all())
    keep, off = G(dev, 64), G(dev, 64, 1)
    assert lib.yt8m_rank1_add_rows_f32(keep.p, 2, 6, 8, gv.p, 1.0, _st()) == -2            # cols % 4
    assert lib.yt8m_rank1_add_rows_f32(keep.p, 2, 8, 10, gv.p, 1.0, _st()) == -2           # ldc % 4
    assert lib.yt8m_rank1_add_rows_f32(keep.p, 2, 8, 7, gv.p, 1.0, _st()) == -2            # ldc < cols
    assert lib.yt8m_rank1_add_rows_f32(off.p, 2, 8, 8, gv.p, 1.0, _st()) == -2             # 4-byte aligned
    torch.cuda.synchronize()
    assert keep.untouched() and off.untouched()


# ---- mixing fused with the cross-entropy ---------------------------------------------------------------------------------------------
XENT_EPS = 1e-5


def _mix_xent_case(dev, B, V, M, lt, use_up):
    lib = L.lib()
    BV = B * V
    Zg0, Ze0, _ = _mix_block(dev, 50 + M, 0, B, V, M)
    yb = _rand(dev, 60 + M, B, V) < 0.05
    yb[0, 0] = True                                                  # p == 1 exactly with y = 1
    yb[1, 0] = True                                                  # p == 0 exactly with y = 1: -log(eps)
    yb[2, 1] = False                                                 # p == 0 with y = 0
    if lt == "u8":
        gy, code, y64 = G(dev, BV, dtype=torch.uint8, fill=7).put(yb.to(torch.uint8)), 0, yb.double()
    else:
        ys = yb.float() * 0.9 + 0.05                                  # label smoothing
        gy, code, y64 = G(dev, BV).put(ys), 1, ys.double()
    nws = lib.yt8m_moe_mix_xent_workspace_bytes(B, V)
    assert nws == 4 * ((BV + 255) // 256 + 1)
    gZg, gZe, gp, gloss, gws = G(dev, BV * (M + 1)).put(Zg0), G(dev, BV * M).put(Ze0), G(dev, BV), G(dev, 1), G(dev, nws // 4)
    L.check(lib.yt8m_moe_mix_xent_fwd(gZg.p, gZe.p, gy.p, code, gp.p, gloss.p, B, V, M, XENT_EPS, gws.p, _st()))
    g64, e64, p64, dG, dE = _mix_ref(Zg0, Ze0, M)
    ce = -(y64 * torch.log(p64 + XENT_EPS) + (1 - y64) * torch.log(1 - p64 + XENT_EPS))
    loss64 = float(ce.sum() / B)
    tag = "mix_xent [%d,%d] M=%d %s" % (B, V, M, lt)
    _report(tag + " p", _maxerr(gp.view(B, V), p64), 2e-6)
    _report(tag + " loss", abs(float(gloss.t[0]) - loss64), 2e-5 * abs(loss64))
    gloss2 = G(dev, 1)
    L.check(lib.yt8m_moe_mix_xent_fwd(gZg.p, gZe.p, gy.p, code, gp.p, gloss2.p, B, V, M, XENT_EPS, gws.p, _st()))
    assert torch.equal(gloss2.t, gloss.t)                             # fixed-order reduction: the same bits again
    assert torch.equal(gZg.view(B, V, M + 1), Zg0) and all(g.intact() for g in (gZg, gZe, gp, gloss, gws, gy))

    # backward, in place.  dL/dZ = d * (mixing backward for dp = 1), d = -(y / (p + eps) - (1 - y) / (1 - p + eps)) * upstream / B.
    # Bound, element by element: the mixing factor is held to the project's 2e-6; each of the two terms of d carries the relative error
    # of its denominator.  p is a quotient of sums of positive terms, so its own error is relative: 2e-6 p (the 2e-6 of the mixing bound
    # taken as a fraction of p; at most 2e-6), plus a few roundings of the denominators.  With smoothed labels the two terms have opposite
    # signs and can cancel, so the error of d is bounded by the terms, not by |d|:
    #   |err| <= 2e-6 |d| + |mixing factor| (t1 (2e-6 p / (p + eps) + 8 ulp) + t2 (2e-6 p / (1 - p + eps) + 8 ulp)),  t1, t2 = |the terms|.
    upstream = 0.7
    up = torch.tensor([0.35], device=dev) if use_up else None
    dscale = upstream / B * (0.35 if use_up else 1.0)
    a64, c64 = p64 + XENT_EPS, 1 - p64 + XENT_EPS
    d64 = -(y64 / a64 - (1 - y64) / c64) * dscale
    dd = (y64 / a64 * (2e-6 * p64 / a64 + 8 * EPS32) + (1 - y64) / c64 * (2e-6 * p64 / c64 + 8 * EPS32)) * dscale
    rZg, rZe = d64[..., None] * dG, d64[..., None] * dE
    tolg = 2e-6 * d64.abs()[..., None] + dG.abs() * dd[..., None] + 1e-30
    tole = 2e-6 * d64.abs()[..., None] + dE.abs() * dd[..., None] + 1e-30
    upp = ctypes.c_void_p(up.data_ptr()) if use_up else None
    hZg, hZe = G(dev, BV * (M + 1)).put(Zg0), G(dev, BV * M).put(Ze0)
    L.check(lib.yt8m_moe_mix_xent_bwd(hZg.p, hZe.p, gy.p, code, upp, B, V, M, XENT_EPS, upstream, _st()))
    _report(tag + " dZg err/tol", float(((hZg.view(B, V, M + 1).double() - rZg).abs() / tolg).max()), 1.0)
    _report(tag + " dZe err/tol", float(((hZe.view(B, V, M).double() - rZe).abs() / tole).max()), 1.0)
    assert hZg.intact() and hZe.intact() and gy.intact()
    # the absmax form: the same gradients bit for bit, and the two words are exactly their largest magnitudes
    words = []
    for _ in range(2):
        aZg, aZe = G(dev, BV * (M + 1)).put(Zg0), G(dev, BV * M).put(Ze0)
        w = G(dev, 2, dtype=torch.int32, fill=-1)
        L.check(lib.yt8m_moe_mix_xent_bwd_absmax(aZg.p, aZe.p, gy.p, code, upp, B, V, M, XENT_EPS, upstream, w.p, _st()))
        assert torch.equal(aZg.t, hZg.t) and torch.equal(aZe.t, hZe.t) and aZg.intact() and aZe.intact() and w.intact()
        want = torch.stack([aZg.t.abs().max(), aZe.t.abs().max()]).view(torch.int32)
        assert torch.equal(w.t, want), (w.t.tolist(), want.tolist())
        words.append(w.t.clone())
    assert torch.equal(words[0], words[1])
    print(tag + " absmax words %s == max|dZg|, max|dZe| bit for bit" % words[0].tolist())


@pytest.mark.parametrize("M", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("lt", ["u8", "f32"])
def test_moe_mix_xent_instantiations(dev, lt, M):
    _mix_xent_case(dev, 7, 1000, M, lt, use_up=(M % 2 == 0))


@pytest.mark.parametrize("B,V", [(23, 89), (32, 64), (3, 683), (7, 1000), (128, 4716)])
def test_moe_mix_xent_chunks(dev, B, V):
    """B V = 2047 / 2048 / 2049 around one ZMAX_IT * 256 chunk of the absmax walk, a partial last chunk, the head's shape."""
    _mix_xent_case(dev, B, V, 2, "u8", use_up=True)


def test_moe_mix_xent_rejections(dev):
    lib = L.lib()
    g = G(dev, 64)
    assert lib.yt8m_moe_mix_xent_fwd(g.p, g.p, g.p, 0, g.p, g.p, 1, 1, 17, XENT_EPS, g.p, _st()) == -1
    assert lib.yt8m_moe_mix_xent_fwd(g.p, g.p, g.p, 2, g.p, g.p, 1, 1, 2, XENT_EPS, g.p, _st()) == -1      # label dtype
    assert lib.yt8m_moe_mix_xent_fwd(g.p, g.p, g.p, 0, g.p, g.p, 0, 1, 2, XENT_EPS, g.p, _st()) == -2      # empty batch
    assert lib.yt8m_moe_mix_xent_bwd(g.p, g.p, g.p, 2, None, 1, 1, 2, XENT_EPS, 1.0, _st()) == -1
    assert lib.yt8m_moe_mix_xent_bwd_absmax(g.p, g.p, g.p, 0, None, 1, 1, 2, XENT_EPS, 1.0, None, _st()) == -1
    torch.cuda.synchronize()
    assert g.untouched()


# ================================================================================================================================
# cross-entropy: grid = (ceil(V / 1024), B)
@pytest.mark.parametrize("B,V", [(1, 1023), (1, 1024), (1, 1025), (9, 1025), (2, 2048), (2, 2049), (9, 4716)])
@pytest.mark.parametrize("lt", ["u8", "f32"])
def test_xent_block_edges(dev, lt, B, V):
    lib = L.lib()
    BV, upstream = B * V, 0.7
    p = _rand(dev, 70 + V, B, V) * 0.98 + 0.01
    p[0, :4] = torch.tensor([0.0, 1.0, 1.0, 0.0], device=dev)       # the eps guards
    p[-1, -1] = 0.0
    yb = _rand(dev, 71 + V, B, V) < 0.01
    yb[0, :4] = torch.tensor([True, True, False, False], device=dev)
    yb[-1, -1] = True
    if lt == "u8":
        gy, code, y64 = G(dev, BV, dtype=torch.uint8, fill=7).put(yb.to(torch.uint8)), 0, yb.double()
    else:
        ys = yb.float() * 0.9 + 0.05
        gy, code, y64 = G(dev, BV).put(ys), 1, ys.double()
    w = _rand(dev, 72, B) + 0.5
    nws = lib.yt8m_xent_workspace_bytes(B, V)
    assert nws == 4 * (B * ((V + 1023) // 1024) + 1)
    gp = G(dev, BV).put(p)
    p64 = p.double()
    a, c = p64 + XENT_EPS, 1 - p64 + XENT_EPS
    for weights in (None, w):
        w64 = torch.ones(B, 1, device=dev, dtype=torch.float64) if weights is None else weights.double()[:, None]
        loss64 = float((-(y64 * torch.log(a) + (1 - y64) * torch.log(c)) * w64).sum() / B)
        dp64 = -(y64 / a - (1 - y64) / c) * w64 * (upstream / B)
        terms = (y64 / a + (1 - y64) / c) * w64 * (upstream / B)      # 2e-5 of the two terms' size, element by element (they can cancel)
        gw = None if weights is None else G(dev, B).put(weights)
        gdp, gloss, gws = G(dev, BV), G(dev, 1), G(dev, nws // 4)
        L.check(lib.yt8m_xent_fwd_bwd(gp.p, gy.p, code, gw.p if gw else None, gloss.p, gdp.p, B, V, XENT_EPS, upstream, gws.p, _st()))
        tag = "xent [%d,%d] %s %s" % (B, V, lt, "weighted" if gw else "plain")
        _report(tag + " loss", abs(float(gloss.t[0]) - loss64), 2e-5 * abs(loss64))
        _report(tag + " dp", _maxerr(gdp.view(B, V), dp64), 2e-5 * float(dp64.abs().max()))
        _report(tag + " dp err / (2e-5 terms)", float(((gdp.view(B, V).double() - dp64).abs() / (2e-5 * terms)).max()), 1.0)
        # loss only (dp = NULL), and again: the same bits
        gloss2 = G(dev, 1)
        L.check(lib.yt8m_xent_fwd_bwd(gp.p, gy.p, code, gw.p if gw else None, gloss2.p, None, B, V, XENT_EPS, upstream, gws.p, _st()))
        assert torch.equal(gloss2.t, gloss.t)
        # gradient only, upstream partly on the device
        up = torch.tensor([0.35], device=dev)
        gdp2 = G(dev, BV)
        L.check(lib.yt8m_xent_bwd(gp.p, gy.p, code, gw.p if gw else None, ctypes.c_void_p(up.data_ptr()), gdp2.p, B, V, XENT_EPS, 2.0, _st()))
        _report(tag + " dp (xent_bwd)", _maxerr(gdp2.view(B, V), dp64), 2e-5 * float(dp64.abs().max()))
        assert all(g.intact() for g in (gdp, gdp2, gloss, gloss2, gws, gp, gy)) and (gw is None or gw.intact())
    assert torch.equal(gp.view(B, V), p)


def test_xent_rejects_large_batch(dev):
    lib = L.lib()
    g, out = G(dev, 64), G(dev, 64)
    assert lib.yt8m_xent_fwd_bwd(g.p, g.p, 1, None, out.p, out.p, 65536, 1, XENT_EPS, 1.0, out.p, _st()) == -2
    assert lib.yt8m_xent_bwd(g.p, g.p, 1, None, None, out.p, 65536, 1, XENT_EPS, 1.0, _st()) == -2
    assert lib.yt8m_xent_fwd_bwd(g.p, g.p, 1, None, out.p, out.p, 0, 4, XENT_EPS, 1.0, out.p, _st()) == -2
    assert lib.yt8m_xent_fwd_bwd(g.p, g.p, 3, None, out.p, out.p, 2, 4, XENT_EPS, 1.0, out.p, _st()) == -1
    torch.cuda.synchronize()
    assert out.untouched() and g.untouched()


# ================================================================================================================================
# column sums
def _colsum_nsplit0(rows, cols):
    """The dispatcher's first choice of row blocks (before it checks the workspace and re-derives the count from rows_per)."""
    cb = (cols + 63) // 64
    if not (cb < 512 and rows >= 4096):
        return 1
    return min(256, (1024 + cb - 1) // cb, rows // 1024)


def _colsum_refs(Xv, w):
    """fp64 and torch-fp32 column sums (plain and weighted) of the view Xv, 4096 columns at a time."""
    outs = [[], [], [], []]
    for c0 in range(0, Xv.shape[1], 4096):
        xs = Xv[:, c0:c0 + 4096]
        x64 = xs.double()
        outs[0].append(x64.sum(0))
        outs[1].append((x64 * w.double()[:, None]).sum(0))
        outs[2].append(xs.sum(0))
        outs[3].append((xs * w[:, None]).sum(0))
    return [torch.cat(o) for o in outs]


@pytest.mark.parametrize("rows,cols,wsmode", [(4095, 200, "full"), (4096, 200, "full"), (4096, 200, "exact"), (4096, 200, "short"),
                                              (4096, 200, "none"), (38400, 64, "full"), (9000, 72, "short"), (4096, 32704, "full"),
                                              (4096, 32705, "full"), (1, 1, "full")])
def test_colsum_branches(dev, rows, cols, wsmode):
    lib = L.lib()
    ldx = cols + 3
    gX = G(dev, rows * ldx)
    Xw = gX.view(rows, ldx)
    Xw[:, :cols] = _randn(dev, 80 + cols, rows, cols) + 0.25
    Xv = Xw[:, :cols]
    w = _rand(dev, 81, rows) + 0.5
    gw = G(dev, rows).put(w)
    s64, sw64, s32, sw32 = _colsum_refs(Xv, w)
    n0 = _colsum_nsplit0(rows, cols)
    split = n0 > 1 and wsmode in ("full", "exact")
    for weighted in (False, True):
        mult = 2 if weighted else 1
        need = mult * n0 * cols * 4
        nbytes = {"full": mult * lib.yt8m_colsum_workspace_bytes(rows, cols), "exact": need, "short": need - 4, "none": 0}[wsmode]
        gws = G(dev, max(nbytes // 4, 1))
        wsp = gws.p if wsmode != "none" else None

        def run(gx, ld, out, outw, beta):
            if weighted:
                return lib.yt8m_colsum_weighted_f32(gx.p, rows, cols, ld, gw.p, out.p, beta, outw.p, wsp, nbytes, _st())
            return lib.yt8m_colsum_f32(gx.p, rows, cols, ld, out.p, beta, wsp, nbytes, _st())

        out, outw = G(dev, cols), G(dev, cols)
        out.t.fill_(5.0)
        L.check(run(gX, ldx, out, outw, 0.0))
        tag = "colsum%s (%d,%d) ws=%s%s" % ("_weighted" if weighted else "", rows, cols, wsmode, " [row split]" if split else "")
        _report(tag, _maxerr(out.t, s64), 4 * _maxerr(s32, s64))
        if weighted:
            _report(tag + " weighted sum", _maxerr(outw.t, sw64), 4 * _maxerr(sw32, sw64))
        first, firstw = out.t.clone(), outw.t.clone()
        # the row split writes its partials to the workspace; every other arm leaves it alone
        assert gws.intact() and (wsmode == "none" or gws.untouched() != split)
        # beta = 1 adds the same sum to what was there (only the plain sum accumulates); a second run gives the same bits
        L.check(run(gX, ldx, out, outw, 1.0))
        assert torch.equal(out.t, first + first) and (not weighted or torch.equal(outw.t, firstw))
        out2, outw2 = G(dev, cols), G(dev, cols)
        L.check(run(gX, ldx, out2, outw2, 0.0))
        assert torch.equal(out2.t, first) and (not weighted or torch.equal(outw2.t, firstw))
        # the tight leading dimension: fixed summation order, so the same bits
        if rows * cols <= 1 << 24:                                    # (the two 536 MB inputs are not copied a second time)
            gT = G(dev, rows * cols).put(Xv)
            out3, outw3 = G(dev, cols), G(dev, cols)
            L.check(run(gT, cols, out3, outw3, 0.0))
            assert torch.equal(out3.t, first) and (not weighted or torch.equal(outw3.t, firstw))
            assert all(g.intact() for g in (out3, outw3, gT))
        assert all(g.intact() for g in (out, outw, out2, outw2, gX, gw))
    assert bool((Xw[:, cols:] == SENT).all())


def test_colsum_rejections(dev):
    lib = L.lib()
    g, out = G(dev, 64), G(dev, 8)
    assert lib.yt8m_colsum_f32(g.p, 8, 8, 8, out.p, 0.5, None, 0, _st()) == -1
    assert lib.yt8m_colsum_f32(g.p, 8, 8, 7, out.p, 0.0, None, 0, _st()) == -2
    assert lib.yt8m_colsum_weighted_f32(g.p, 8, 8, 8, g.p, out.p, 0.5, out.p, None, 0, _st()) == -1
    assert lib.yt8m_colsum_weighted_f32(g.p, 8, 8, 7, g.p, out.p, 0.0, out.p, None, 0, _st()) == -2
    torch.cuda.synchronize()
    assert out.untouched() and g.untouched()


# ================================================================================================================================
# fp32 -> bf16 casts: every form is round-to-nearest-even, so every path gives torch's bits
def _bf16_bits(x):
    return x.to(torch.bfloat16).view(torch.int16)


def _cast_input(dev, rows, cols, seed):
    x = _randn(dev, seed, rows, cols) * 3
    f = x.view(-1)
    special = [1.00390625, -1.00390625, 1.01171875, float("inf"), -float("inf"), -0.0, 3.3895314e38, 65280.0]  # ties, inf, overflow to inf
    n = min(len(special), f.numel())
    f[:n] = torch.tensor(special[:n], device=dev)
    return x


CAST_CASES = [(64, 128, 8, 8, 0, 0), (66, 128, 8, 8, 0, 0), (64, 130, 8, 8, 0, 0), (64, 128, 3, 8, 0, 0), (64, 128, 8, 2, 0, 0),
              (64, 128, 8, 8, 1, 0), (64, 128, 8, 8, 0, 1), (64, 128, 8, 8, 0, 2), (5, 7, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0),
              (132, 260, 4, 4, 0, 0), (4100, 4100, 0, 0, 0, 0), (4100, 4100, 0, 0, 1, 0)]


@pytest.mark.parametrize("rows,cols,ldpad,dldpad,sshift,dshift", CAST_CASES)
def test_cast_bf16_branches(dev, rows, cols, ldpad, dldpad, sshift, dshift):
    lib = L.lib()
    ld, pld, tld = cols + ldpad, cols + dldpad, rows + dldpad
    x = _cast_input(dev, rows, cols, 90 + cols)
    gs = G(dev, rows * ld, sshift)
    gs.view(rows, ld)[:, :cols] = x
    want = _bf16_bits(x)
    FILL = 0x5A5A

    def dsts():
        return G(dev, rows * pld, dshift, torch.int16, FILL), G(dev, cols * tld, dshift, torch.int16, FILL)

    def check(gp, gt, what):
        if gp is not None:
            assert torch.equal(gp.view(rows, pld)[:, :cols], want), what + " plain"
            assert bool((gp.view(rows, pld)[:, cols:] == FILL).all()) and gp.intact()
        if gt is not None:
            assert torch.equal(gt.view(cols, tld)[:, :rows], want.t()), what + " transposed"
            assert bool((gt.view(cols, tld)[:, rows:] == FILL).all()) and gt.intact()

    gp, gt = dsts()
    L.check(lib.yt8m_cast_f32_bf16(gs.p, rows, cols, ld, gp.p, pld, 0, _st()))
    L.check(lib.yt8m_cast_f32_bf16(gs.p, rows, cols, ld, gt.p, tld, 1, _st()))
    check(gp, gt, "single")
    gp2, gt2 = dsts()
    L.check(lib.yt8m_cast_f32_bf16_dual(gs.p, rows, cols, ld, gp2.p, pld, gt2.p, tld, _st()))
    check(gp2, gt2, "dual")
    assert gs.intact() and torch.equal(gs.view(rows, ld)[:, :cols], x) and bool((gs.view(rows, ld)[:, cols:] == SENT).all())
    print("cast (%d,%d) ld+%d dld+%d src+%d dst+%d: plain, transposed and dual equal torch's bf16 bits" % (rows, cols, ldpad, dldpad, sshift, dshift))


def test_cast_bf16_default_ld_and_rejections(dev):
    lib = L.lib()
    rows, cols = 8, 12
    x = _cast_input(dev, rows, cols, 99)
    x[3, 5] = float("nan")
    gs = G(dev, rows * cols).put(x)
    gp, gt = G(dev, rows * cols, 0, torch.int16, 0x5A5A), G(dev, rows * cols, 0, torch.int16, 0x5A5A)
    L.check(lib.yt8m_cast_f32_bf16(gs.p, rows, cols, cols, gp.p, 0, 0, _st()))        # dst_ld = 0: cols / rows
    L.check(lib.yt8m_cast_f32_bf16(gs.p, rows, cols, cols, gt.p, 0, 1, _st()))
    ok = ~torch.isnan(x)
    want = _bf16_bits(x)
    assert torch.equal(gp.view(rows, cols)[ok], want[ok]) and torch.equal(gt.view(cols, rows)[ok.t()], want.t()[ok.t()])
    assert bool(torch.isnan(gp.view(rows, cols).view(torch.bfloat16)[3, 5])) and bool(torch.isnan(gt.view(cols, rows).view(torch.bfloat16)[5, 3]))
    assert gp.intact() and gt.intact()
    out = G(dev, 256, 0, torch.int16, 0x5A5A)
    assert lib.yt8m_cast_f32_bf16(gs.p, rows, cols, cols - 1, out.p, 0, 0, _st()) == -2
    assert lib.yt8m_cast_f32_bf16(gs.p, rows, cols, cols, out.p, cols - 1, 0, _st()) == -2
    assert lib.yt8m_cast_f32_bf16(gs.p, rows, cols, cols, out.p, rows - 1, 1, _st()) == -2
    assert lib.yt8m_cast_f32_bf16_dual(gs.p, rows, cols, cols, out.p, cols - 1, out.p, 0, _st()) == -2
    torch.cuda.synchronize()
    assert out.untouched()


# ================================================================================================================================
# dequantise + l2-normalise of raw uint8 frames: the path is chosen inside the kernel
@pytest.mark.parametrize("D,qshift,xshift", [(4, 0, 0), (260, 0, 0), (1152, 0, 0), (2048, 0, 0), (2052, 0, 0), (1150, 0, 0), (1152, 1, 0),
                                             (1152, 0, 1)])
def test_dequant_l2norm_paths(dev, D, qshift, xshift):
    from oracle import np_ref
    lib = L.lib()
    B, F = 3, 7                                                      # 21 rows: the last workgroup is partial
    rs = np.random.RandomState(D)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    q[0, 0], q[0, 1] = 0, 255
    nf = np.array([F, 1, 0], dtype=np.int32)
    gq = G(dev, B * F * D, qshift, torch.uint8, 77).put(torch.from_numpy(q).to(dev))
    nfd = torch.from_numpy(nf).to(dev)
    for frames in (nfd, None):
        gx = G(dev, B * F * D, xshift)
        L.check(lib.yt8m_dequant_l2norm_u8(gq.p, ctypes.c_void_p(frames.data_ptr()) if frames is not None else None, gx.p, B, F, D, 1e-12, _st()))
        ref = torch.from_numpy(np_ref.dequant_l2norm_folded(q, nf if frames is not None else None)).to(dev)
        x = gx.view(B, F, D)
        _report("dequant_l2norm D=%d q+%d x+%d nf=%s" % (D, qshift, xshift, frames is not None), _maxerr(x, ref), 1e-6)
        if frames is not None:
            assert bool((x[1, 1:] == 0).all()) and bool((x[2] == 0).all())      # padding rows are exactly 0
        assert gx.intact() and gq.intact()
    assert torch.equal(gq.view(B, F, D).cpu(), torch.from_numpy(q))


# ================================================================================================================================
# attention softmax over frames / assignment softmax over clusters
def _frames(dev, B, F, seed):
    nf = torch.randint(0, F + 1, (B,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    nf[0] = F
    if B > 1:
        nf[1] = 1
    if B > 2:
        nf[2] = 0
    return nf.to(dev)


@pytest.mark.parametrize("B,F,A", [(128, 300, 8), (5, 64, 3), (5, 65, 3), (3, 1, 2)])
def test_attn_softmax_shapes(dev, B, F, A):
    lib = L.lib()
    n = B * F * A
    act = _randn(dev, 110 + F, B, F, A) * 2
    dw = _randn(dev, 111 + F, B, F, A)
    nf = _frames(dev, B, F, 112)
    ga, gw, gdw, gda = G(dev, n).put(act), G(dev, n), G(dev, n).put(dw), G(dev, n)
    nfp = ctypes.c_void_p(nf.data_ptr())
    L.check(lib.yt8m_attn_softmax_fwd(ga.p, nfp, gw.p, B, F, A, _st()))
    L.check(lib.yt8m_attn_softmax_bwd(gw.p, gdw.p, nfp, gda.p, B, F, A, _st()))
    mask = (torch.arange(F, device=dev)[None, :] < nf[:, None]).double()[:, :, None]
    e = torch.exp(act.double() - act.double().amax(1, keepdim=True)) * mask
    live = nf > 0
    w64 = e[live] / e[live].sum(1, keepdim=True)
    w = gw.view(B, F, A)
    _report("attn_softmax fwd (%d,%d,%d)" % (B, F, A), _maxerr(w[live], w64), 1e-6)
    assert bool(torch.isnan(w[~live]).all())                          # num_frames = 0: 0 / 0, as the reference computes it
    wk = w[live].double()                                             # the backward's own input
    da64 = wk * (dw[live].double() - (wk * dw[live].double()).sum(1, keepdim=True))
    _report("attn_softmax bwd", _maxerr(gda.view(B, F, A)[live], da64), 1e-5)
    assert bool((gda.view(B, F, A)[~live] == 0).all())
    assert bool((gda.view(B, F, A) * (1 - mask) == 0)[live].all()) and bool((w * (1 - mask) == 0)[live].all())      # masked frames: exactly 0
    # num_frames = NULL: every frame counts
    gw2 = G(dev, n)
    L.check(lib.yt8m_attn_softmax_fwd(ga.p, None, gw2.p, B, F, A, _st()))
    _report("attn_softmax fwd, no num_frames", _maxerr(gw2.view(B, F, A), torch.softmax(act.double(), 1)), 1e-6)
    assert all(g.intact() for g in (ga, gw, gdw, gda, gw2)) and torch.equal(ga.view(B, F, A), act)


@pytest.mark.parametrize("B,F,K", [(3, 7, 1), (3, 7, 63), (3, 7, 64), (3, 7, 65), (3, 7, 100), (2, 5, 4096), (128, 300, 64)])
def test_softmax_rows_shapes(dev, B, F, K):
    lib = L.lib()
    n = B * F * K
    s = _randn(dev, 120 + K, B, F, K) * 3
    da = _randn(dev, 121 + K, B, F, K)
    nf = _frames(dev, B, F, 122)
    gs, ga, gda, gds = G(dev, n).put(s), G(dev, n), G(dev, n).put(da), G(dev, n)
    nfp = ctypes.c_void_p(nf.data_ptr())
    L.check(lib.yt8m_softmax_rows_fwd(gs.p, nfp, ga.p, B, F, K, _st()))
    L.check(lib.yt8m_softmax_rows_bwd(ga.p, gda.p, nfp, gds.p, B, F, K, _st()))
    mask = (torch.arange(F, device=dev)[None, :] < nf[:, None])[:, :, None]
    a = ga.view(B, F, K)
    _report("softmax_rows fwd (%d,%d,%d)" % (B, F, K), _maxerr(a, torch.softmax(s.double(), 2) * mask), 1e-6)
    ak = a.double()
    _report("softmax_rows bwd", _maxerr(gds.view(B, F, K), ak * (da.double() - (ak * da.double()).sum(2, keepdim=True)) * mask), 1e-5)
    dead = ~mask.expand(B, F, K)
    assert bool((a[dead] == 0).all()) and bool((gds.view(B, F, K)[dead] == 0).all())
    ga2 = G(dev, n)
    L.check(lib.yt8m_softmax_rows_fwd(gs.p, None, ga2.p, B, F, K, _st()))
    _report("softmax_rows fwd, no num_frames", _maxerr(ga2.view(B, F, K), torch.softmax(s.double(), 2)), 1e-6)
    assert all(g.intact() for g in (gs, ga, gda, gds, ga2)) and torch.equal(gs.view(B, F, K), s)


# ================================================================================================================================
# top-k and precision at equal recall: above 64 KB of dynamic LDS the entry point raises the kernel's limit first
def _topk_ref(p, k):
    """Stable descending order of the scores above -inf (NaN never compares greater), then the lowest unused indices."""
    idx = np.zeros((p.shape[0], k), dtype=np.int32)
    for r in range(p.shape[0]):
        row = p[r]
        cand = np.nonzero(row > -np.inf)[0]
        order = cand[np.lexsort((cand, -row[cand]))][:k].tolist()
        used = set(order)
        c = 0
        while len(order) < k:
            if c not in used:
                order.append(c)
            c += 1
        idx[r] = order
    return idx


@pytest.mark.parametrize("V,k", [(4716, 64), (16384, 20), (16385, 20), (38400, 64)])
def test_topk_rows_lds(dev, V, k):
    lib = L.lib()
    rs = np.random.RandomState(V)
    B = 5
    p = rs.rand(B, V).astype(np.float32)
    p[0, 10] = p[0, 20] = p[0, 5] = p[0, V - 1] = 2.0                 # ties: the lower index first
    p[1, :] = np.nan
    p[2, :] = -np.inf
    p[3, :] = np.nan
    p[3, 7], p[3, V - 2], p[3, 300] = 0.5, 0.9, -np.inf
    p[4, 3], p[4, 4] = np.inf, -np.inf
    gp = G(dev, B * V).put(torch.from_numpy(p).to(dev))
    gv, gi = G(dev, B * k), G(dev, B * k, 0, torch.int32, -5)
    L.check(lib.yt8m_topk_rows(gp.p, B, V, k, gv.p, gi.p, _st()))
    want = _topk_ref(p, k)
    got = gi.view(B, k).cpu().numpy()
    assert np.array_equal(got, want), (V, k)
    wv = np.take_along_axis(p, want.astype(np.int64), 1)
    assert np.array_equal(gv.view(B, k).cpu().numpy().view(np.int32), wv.view(np.int32))      # the scores themselves, NaN payloads included
    assert got[0, :4].tolist() == [5, 10, 20, V - 1] and got[1].tolist() == list(range(k)) and got[3, :2].tolist() == [V - 2, 7]
    assert gp.intact() and gv.intact() and gi.intact() and torch.equal(gp.view(B, V).view(torch.int32).cpu(), torch.from_numpy(p.view(np.int32)))
    print("topk V=%d k=%d (%d bytes of LDS): indices and scores exact" % (V, k, 4 * V))


@pytest.mark.parametrize("V", [4716, 8192, 8193, 19200])
def test_perr_rows_lds(dev, V):
    import yt8m_amd.eval_util as eval_util
    lib = L.lib()
    rs = np.random.RandomState(V)
    B = 5
    p = rs.rand(B, V).astype(np.float32)
    p[1] -= 0.9                                                      # mostly non-positive scores: the (score > 0) filter matters
    y = rs.rand(B, V) < 20.0 / V
    y[0] = False                                                     # a video without labels
    y[2, :] = False
    y[2, V - 1] = True                                                # one label, in the last class
    gp = G(dev, B * V).put(torch.from_numpy(p).to(dev))
    gy = G(dev, B * V, 0, torch.uint8, 9).put(torch.from_numpy(y.astype(np.uint8)).to(dev))
    go = G(dev, B)
    L.check(lib.yt8m_perr_rows(gp.p, gy.p, B, V, go.p, _st()))
    got = go.t.cpu().numpy()
    for r in range(B):
        exp = eval_util.calculate_precision_at_equal_recall_rate(p[r:r + 1], y[r:r + 1])
        nl = int(y[r].sum())
        hits = int(round(exp * nl))
        assert got[r] == (np.float32(hits) / np.float32(nl) if nl else np.float32(0)), (V, r, got[r], exp)      # integer counting: exact
    assert gp.intact() and gy.intact() and go.intact()
    print("perr V=%d (%d bytes of LDS): %s exact" % (V, 8 * V, got.tolist()))


def test_topk_perr_rejections(dev):
    lib = L.lib()
    g, v, i = G(dev, 64), G(dev, 128), G(dev, 128, 0, torch.int32, -5)
    assert lib.yt8m_topk_rows(g.p, 1, 38401, 20, v.p, i.p, _st()) == -2       # over the LDS limit
    assert lib.yt8m_topk_rows(g.p, 1, 64, 65, v.p, i.p, _st()) == -1          # k > 64
    assert lib.yt8m_topk_rows(g.p, 1, 5, 6, v.p, i.p, _st()) == -1            # k > V
    assert lib.yt8m_topk_rows(g.p, 1, 5, 0, v.p, i.p, _st()) == -1
    assert lib.yt8m_perr_rows(g.p, g.p, 1, 19201, v.p, _st()) == -2
    assert lib.yt8m_perr_rows(g.p, g.p, 1, 0, v.p, _st()) == -2
    torch.cuda.synchronize()
    assert g.untouched() and v.untouched() and i.untouched()


# ================================================================================================================================
# frame pooling
@pytest.mark.parametrize("B,S,C", [(128, 30, 8192), (3, 16, 72), (3, 17, 72), (3, 16, 70), (3, 17, 70), (2, 30, 1024), (2, 30, 1028), (4, 1, 12)])
@pytest.mark.parametrize("mode", [0, 1])
def test_frame_pool_branches(dev, mode, B, S, C):
    lib = L.lib()
    x = (_randn(dev, 130 + C + S, B, S, C) * 4 + 3).clamp(0, 6)      # relu6 output: ties at both clamp values in most columns
    dy = _randn(dev, 131 + C, B, C)
    if mode == 0 and S > 1:
        assert float(((x == x.amax(1, keepdim=True)).sum(1) > 1).float().mean()) > 0.05
    # the maximum is exact; the average keeps the project's 1e-6, and at the DBoF model's shape (a serial fp32 sum over S for each of a
    # million columns) it is held to the rule for sums: four times the error of torch's own fp32 x.mean(1) against fp64 on the same data
    fwd_bound = 0.0 if mode == 0 else 1e-6
    big_sum = mode == 1 and B * C >= 1 << 20
    t_mean = 0.0
    res = []
    for shift in (0, 1):
        gx, gdy, go, gdx = G(dev, B * S * C, shift).put(x), G(dev, B * C, shift).put(dy), G(dev, B * C, shift), G(dev, B * S * C, shift)
        L.check(lib.yt8m_frame_pool_fwd(gx.p, B, S, C, mode, go.p, _st()))
        L.check(lib.yt8m_frame_pool_bwd(gx.p, go.p, gdy.p, B, S, C, mode, gdx.p, _st()))
        assert all(g.intact() for g in (gx, gdy, go, gdx)) and torch.equal(gx.view(B, S, C), x)
        if shift == 0:
            ef = eb = 0.0
            for b0 in range(0, B, 16):                                # videos are independent: fp64 autograd 16 at a time
                xr = x[b0:b0 + 16].double().requires_grad_(True)
                ref = xr.amax(1) if mode == 0 else xr.mean(1)        # amax shares the gradient between tied maxima, as tf.reduce_max does
                (ref * dy[b0:b0 + 16].double()).sum().backward()
                ef = max(ef, _maxerr(go.view(B, C)[b0:b0 + 16], ref.detach()))
                if big_sum:
                    t_mean = max(t_mean, _maxerr(x[b0:b0 + 16].mean(1), ref.detach()))
                eb = max(eb, _maxerr(gdx.view(B, S, C)[b0:b0 + 16], xr.grad))
            tag = "frame_pool %s (%d,%d,%d)" % ("max" if mode == 0 else "avg", B, S, C)
            _report(tag + (" fwd vs 4 x torch fp32" if big_sum else " fwd"), ef, 4 * t_mean if big_sum else fwd_bound)
            _report(tag + " bwd", eb, 1e-6)
        res.append((go.t.clone(), gdx.t.clone()))
        del gx, gdx
    # float4 (16-byte aligned, C % 4 == 0) and scalar forms do the same arithmetic in the same order
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_frame_pool_rejections(dev):
    lib = L.lib()
    g, out = G(dev, 64), G(dev, 64)
    assert lib.yt8m_frame_pool_fwd(g.p, 65536, 1, 4, 0, out.p, _st()) == -2
    assert lib.yt8m_frame_pool_bwd(g.p, g.p, g.p, 65536, 1, 4, 0, out.p, _st()) == -2
    assert lib.yt8m_frame_pool_fwd(g.p, 2, 0, 4, 0, out.p, _st()) == -2
    assert lib.yt8m_frame_pool_fwd(g.p, 2, 2, 4, 2, out.p, _st()) == -1
    assert lib.yt8m_frame_pool_bwd(g.p, g.p, g.p, 2, 2, 4, 2, out.p, _st()) == -1
    torch.cuda.synchronize()
    assert out.untouched() and g.untouched()


# ================================================================================================================================
# batch norm
BN_EPS, BN_DECAY = 1e-3, 0.999


def _close_fp32(got, want32, ulps=4):
    return bool(((got - want32).abs() <= ulps * EPS32 * want32.abs().clamp(min=1.0)).all())


@pytest.mark.parametrize("training,N,C", [(1, 1, 64), (1, 3, 64), (1, 4, 65), (1, 5, 65), (1, 203, 150), (1, 3840, 8192), (1, 30720, 512),
                                          (0, 5, 65), (0, 300, 130)])
def test_batchnorm_branches(dev, training, N, C):
    lib = L.lib()
    colscale = 0.5 + _rand(dev, 140, C) * 2
    colshift = _randn(dev, 141, C)
    gx, gdy = G(dev, N * C).put(_randn(dev, 142 + N, N, C) * colscale + colshift), G(dev, N * C).put(_randn(dev, 143 + N, N, C))
    x, dy = gx.view(N, C), gdy.view(N, C)
    xsum = x.double().sum()
    gamma, beta = 0.5 + _rand(dev, 144, C), _rand(dev, 145, C) - 0.5
    mm0, mv0 = _randn(dev, 146, C), _rand(dev, 147, C) + 0.5
    gg, gb = G(dev, C).put(gamma), G(dev, C).put(beta)
    nws = lib.yt8m_batchnorm_workspace_bytes(C)
    assert nws == 8 * C

    def fwd():
        o = dict(y=G(dev, N * C), mean=G(dev, C), rstd=G(dev, C), mm=G(dev, C).put(mm0), mv=G(dev, C).put(mv0))
        L.check(lib.yt8m_batchnorm_fwd(gx.p, N, C, gg.p, gb.p, o["mm"].p, o["mv"].p, training, BN_EPS, BN_DECAY, o["y"].p, o["mean"].p,
                                       o["rstd"].p, _st()))
        return o

    def bwd(f, want_dx=True, want_params=True, pbeta=0.0, into=None):
        o = into or dict(dx=G(dev, N * C) if want_dx else None, dgamma=G(dev, C) if want_params else None,
                         dbeta=G(dev, C) if want_params else None, ws=G(dev, nws // 4))
        pp = lambda g: g.p if g is not None else None
        L.check(lib.yt8m_batchnorm_bwd(gx.p, gdy.p, N, C, gg.p, f["mean"].p, f["rstd"].p, training, pp(o["dx"]), pp(o["dgamma"]), pbeta,
                                       pp(o["dbeta"]), pbeta, o["ws"].p, nws, _st()))
        return o

    f = fwd()
    b = bwd(f)
    mean, rstd = f["mean"].t, f["rstd"].t
    y, dx = f["y"].view(N, C), b["dx"].view(N, C)
    e = dict(mean=0.0, var=0.0, y=0.0, dbeta=0.0, dgamma=0.0, dx=0.0)
    t = dict(mean=0.0, var=0.0, dbeta=0.0, dgamma=0.0)
    dxscale = 1.0
    for c0 in range(0, C, 1024):                                      # columns are independent: fp64 restatement 1024 at a time
        sl = slice(c0, min(c0 + 1024, C))
        xs, ds = x[:, sl], dy[:, sl]
        x64, d64, g64, b64 = xs.double(), ds.double(), gamma[sl].double(), beta[sl].double()
        if training:
            mean64 = x64.mean(0)
            var64 = ((x64 - mean64) ** 2).mean(0)
            t_mean = xs.sum(0) / N                                    # torch's own fp32 evaluation of the same expressions
            t_var = ((xs - t_mean) ** 2).sum(0) / N
        else:
            mean64, var64 = mm0[sl].double(), mv0[sl].double()
            t_mean, t_var = mm0[sl], mv0[sl]
        rstd64 = (var64 + BN_EPS).rsqrt()
        xhat64 = (x64 - mean64) * rstd64
        y64 = xhat64 * g64 + b64
        sdy, sdyx = d64.sum(0), (d64 * xhat64).sum(0)
        dx64 = g64 * rstd64 * (d64 - sdy / N - xhat64 * (sdyx / N)) if training else g64 * rstd64 * d64
        t_xhat = (xs - t_mean) * (t_var + BN_EPS).rsqrt()
        t["mean"] = max(t["mean"], _maxerr(t_mean, mean64))
        t["var"] = max(t["var"], _maxerr(t_var, var64))
        t["dbeta"] = max(t["dbeta"], _maxerr(ds.sum(0), sdy))
        t["dgamma"] = max(t["dgamma"], _maxerr((ds * t_xhat).sum(0), sdyx))
        e["mean"] = max(e["mean"], _maxerr(mean[sl], mean64))
        # the variance the kernel's rstd stands for (rstd itself is one sqrt and one division away: 4 ulp of var + eps, relative)
        var_k = 1.0 / rstd[sl].double() ** 2 - BN_EPS
        e["var"] = max(e["var"], float(((var_k - var64).abs() - 4 * EPS32 * (var64 + BN_EPS)).clamp(min=0).max()))
        e["y"] = max(e["y"], _maxerr(y[:, sl], y64))
        e["dbeta"] = max(e["dbeta"], _maxerr(b["dbeta"].t[sl], sdy))
        e["dgamma"] = max(e["dgamma"], _maxerr(b["dgamma"].t[sl], sdyx))
        e["dx"] = max(e["dx"], _maxerr(dx[:, sl], dx64))
        dxscale = max(dxscale, float(dx64.abs().max()))
    tag = "batchnorm %s (%d,%d)" % ("train" if training else "frozen", N, C)
    if training:
        _report(tag + " mean", e["mean"], 4 * t["mean"])
        _report(tag + " var beyond rstd rounding", e["var"], 4 * t["var"])
        dec, om = float(np.float32(BN_DECAY)), float(np.float32(1.0) - np.float32(BN_DECAY))
        assert _close_fp32(f["mm"].t, dec * mm0 + om * mean)
        var_k = (1.0 / rstd.double() ** 2 - BN_EPS)
        want_mv = BN_DECAY * mv0.double() + (1.0 - BN_DECAY) * var_k
        assert float((f["mv"].t.double() - want_mv).abs().max()) <= 4 * EPS32 * float(want_mv.abs().max()) + (1.0 - BN_DECAY) * 8 * EPS32 * float((var_k + BN_EPS).max())
    else:
        assert torch.equal(mean, mm0) and _close_fp32(rstd, 1.0 / torch.sqrt(mv0 + BN_EPS))
        assert torch.equal(f["mm"].t, mm0) and torch.equal(f["mv"].t, mv0)
    _report(tag + " y", e["y"], 2e-5)
    _report(tag + " dbeta (column sum of dy)", e["dbeta"], 4 * t["dbeta"])
    _report(tag + " dgamma (column sum of dy xhat)", e["dgamma"], 4 * t["dgamma"])
    _report(tag + " dx", e["dx"], 2e-5 * dxscale)
    # fixed-order sums: a second run gives the same bits
    f2 = fwd()
    b2 = bwd(f2)
    for k in ("y", "mean", "rstd", "mm", "mv"):
        assert torch.equal(f2[k].t, f[k].t), k
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(b2[k].t, b[k].t), k
    # accumulate into dgamma / dbeta (beta 1); dx = NULL; no parameter gradients
    first_g, first_b = b["dgamma"].t.clone(), b["dbeta"].t.clone()
    bwd(f, pbeta=1.0, into=b2)
    assert torch.equal(b2["dgamma"].t, first_g + first_g) and torch.equal(b2["dbeta"].t, first_b + first_b)
    b3 = bwd(f, want_dx=False)
    assert torch.equal(b3["dgamma"].t, first_g) and torch.equal(b3["dbeta"].t, first_b)
    b4 = bwd(f, want_params=False)
    assert torch.equal(b4["dx"].t, b["dx"].t)
    # a workspace one float short is refused before any launch
    small, keep = G(dev, nws // 4), G(dev, C)
    assert lib.yt8m_batchnorm_bwd(gx.p, gdy.p, N, C, gg.p, f["mean"].p, f["rstd"].p, training, None, keep.p, 0.0, keep.p, 0.0, small.p, nws - 4,
                                  _st()) == -2
    torch.cuda.synchronize()
    assert small.untouched() and keep.untouched()
    for o in (f, f2, b, b2, b3, b4):
        assert all(g.intact() for g in o.values() if g is not None)
    assert all(g.intact() for g in (gx, gdy, gg, gb)) and torch.equal(x.double().sum(), xsum)


# ================================================================================================================================
# NetVLAD residual + intra-normalisation
def _vlad_ref(agg, n, cen, dy, dq, eps):
    """fp64 autograd of vlad = pre rsqrt(max(|pre|^2, eps)), q = |pre|^2 r^2 with pre = agg - n c; n is a leaf, as it is for the kernel."""
    agg64, n64, c64 = (t.double().clone().requires_grad_(True) for t in (agg, n, cen))
    pre = agg64 - n64[..., None] * c64[None]
    ss = (pre * pre).sum(-1)
    r = ss.clamp(min=eps).rsqrt()
    vlad = pre * r[..., None]
    q = ss * r * r
    loss = (vlad * dy.double()).sum()
    if dq is not None:
        loss = loss + (q * dq.double()).sum()
    loss.backward()
    return vlad.detach(), q.detach(), agg64.grad, n64.grad, c64.grad


@pytest.mark.parametrize("D,shift", [(4, 0), (8, 0), (1152, 0), (2048, 0), (2052, 0), (1150, 0), (6, 0), (1152, 1)])
def test_vlad_finish_branches(dev, D, shift):
    lib = L.lib()
    B, F, K, eps = 3, 70, 6, 1e-12                                    # B K = 18 rows: a partial last workgroup; F > 64 lanes
    reg = D % 4 == 0 and D <= 2048 and shift == 0
    assert lib.yt8m_vlad_finish_q_supported(D) == (1 if D % 4 == 0 and 4 <= D <= 2048 else 0)
    agg = _randn(dev, 150 + D, B, K, D)
    a = torch.softmax(_randn(dev, 151 + D, B, F, K), 2)
    cen = _randn(dev, 152 + D, K, D) * 0.1
    agg[0, 0] = 0.0
    a[0, :, 0] = 0.0                                                  # row (0, 0): pre = 0, the norm is clamped
    dy, dq = _randn(dev, 153 + D, B, K, D), _randn(dev, 154 + D, B, K)
    gagg, ga, gc = G(dev, B * K * D, shift).put(agg), G(dev, B * F * K).put(a), G(dev, K * D, shift).put(cen)
    gdy, gdq = G(dev, B * K * D, shift).put(dy), G(dev, B * K).put(dq)
    n64 = a.double().sum(1)
    tag = "vlad_finish D=%d +%d (%s)" % (D, shift, "register" if reg else "generic")
    # forward, from the assignments
    gv, gn = G(dev, B * K * D, shift), G(dev, B * K)
    L.check(lib.yt8m_vlad_finish_fwd(gagg.p, ga.p, gc.p, gv.p, gn.p, B, F, K, D, eps, _st()))
    n = gn.view(B, K).clone()
    _report(tag + " n", _maxerr(n, n64), 1e-6 * max(1.0, float(n64.abs().max())))       # a sum of F assignments: 1e-6 relative
    v64, q64 = _vlad_ref(agg, n64, cen, dy, None, eps)[:2]                   # forward: from the fp64 n
    _, _, dagg64, dn64, dc64 = _vlad_ref(agg, n, cen, dy, None, eps)          # backward: from the kernel's own n, which is its input
    _report(tag + " vlad", _maxerr(gv.view(B, K, D), v64), 1e-6)
    assert bool((gv.view(B, K, D)[0, 0] == 0).all())
    # forward with n precomputed (a = NULL): the same bits
    gv2, gn2 = G(dev, B * K * D, shift), G(dev, B * K).put(n)
    L.check(lib.yt8m_vlad_finish_fwd(gagg.p, None, gc.p, gv2.p, gn2.p, B, F, K, D, eps, _st()))
    assert torch.equal(gv2.t, gv.t) and torch.equal(gn2.view(B, K), n)
    # the q output: the register form only
    gv3, gn3, gq = G(dev, B * K * D, shift), G(dev, B * K), G(dev, B * K)
    rc = lib.yt8m_vlad_finish_q_fwd(gagg.p, ga.p, gc.p, gv3.p, gn3.p, gq.p, B, F, K, D, eps, _st())
    if reg:
        L.check(rc)
        assert torch.equal(gv3.t, gv.t) and torch.equal(gn3.t, gn.t)
        _report(tag + " q", _maxerr(gq.view(B, K), q64), 1e-6)
    else:
        torch.cuda.synchronize()
        assert rc == -2 and gv3.untouched() and gn3.untouched() and gq.untouched()
    # backward without / with the q gradient; dcentres overwritten, accumulated, absent
    for with_q in (False, True):
        gda, gdn, gdc = G(dev, B * K * D, shift), G(dev, B * K), G(dev, K * D)
        if with_q:
            rc = lib.yt8m_vlad_finish_q_bwd(gagg.p, gn.p, gc.p, gdy.p, gdq.p, gda.p, gdn.p, gdc.p, 0.0, B, K, D, eps, _st())
            if not reg:
                torch.cuda.synchronize()
                assert rc == -2 and gda.untouched() and gdn.untouched() and gdc.untouched()
                continue
            L.check(rc)
            _, _, dagg64, dn64, dc64 = _vlad_ref(agg, n, cen, dy, dq, eps)
        else:
            L.check(lib.yt8m_vlad_finish_bwd(gagg.p, gn.p, gc.p, gdy.p, gda.p, gdn.p, gdc.p, 0.0, B, K, D, eps, _st()))
        sfx = " (+dq)" if with_q else ""
        _report(tag + " dagg rel" + sfx, _rowscaled(gda.view(B * K, D), dagg64.view(B * K, D)), 1e-5)
        _report(tag + " dn rel" + sfx, _rowscaled(gdn.t, dn64.view(-1)), 1e-5)
        _report(tag + " dcentres rel" + sfx, _rowscaled(gdc.view(K, D), dc64), 1e-5)
        first = gdc.t.clone()
        gda2, gdn2 = G(dev, B * K * D, shift), G(dev, B * K)
        if with_q:
            L.check(lib.yt8m_vlad_finish_q_bwd(gagg.p, gn.p, gc.p, gdy.p, gdq.p, gda2.p, gdn2.p, gdc.p, 1.0, B, K, D, eps, _st()))
        else:
            L.check(lib.yt8m_vlad_finish_bwd(gagg.p, gn.p, gc.p, gdy.p, gda2.p, gdn2.p, gdc.p, 1.0, B, K, D, eps, _st()))
        assert torch.equal(gdc.t, first + first) and torch.equal(gda2.t, gda.t) and torch.equal(gdn2.t, gdn.t)
        gda3, gdn3 = G(dev, B * K * D, shift), G(dev, B * K)
        L.check(lib.yt8m_vlad_finish_bwd(gagg.p, gn.p, gc.p, gdy.p, gda3.p, gdn3.p, None, 0.0, B, K, D, eps, _st()))
        assert with_q or (torch.equal(gda3.t, gda.t) and torch.equal(gdn3.t, gdn.t))
        assert all(g.intact() for g in (gda, gdn, gdc, gda2, gdn2, gda3, gdn3))
    keep = G(dev, B * K * D, shift)
    assert lib.yt8m_vlad_finish_bwd(gagg.p, gn.p, gc.p, gdy.p, keep.p, keep.p, keep.p, 0.5, B, K, D, eps, _st()) == -1
    torch.cuda.synchronize()
    assert keep.untouched()
    assert all(g.intact() for g in (gagg, ga, gc, gdy, gdq, gv, gn, gv2, gn2, gv3, gn3, gq))
    assert torch.equal(gagg.view(B, K, D), agg) and torch.equal(gc.view(K, D), cen)
