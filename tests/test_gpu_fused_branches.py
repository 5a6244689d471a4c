"""-m gpu: every dispatch branch of the fused kernels of the byte path and of the bf16 head (csrc/netvlad_fused.hip, csrc/gemm_skinny.hip,
csrc/moe_bf16.hip, csrc/cnn_pool.hip, csrc/cnn_pool_f32.hip) through the C ABI against fp64 written here (numpy / torch on the CPU), at
both sides of each shape threshold, with sentinel margins around every output and with the refusals of each entry point.  The quick
small-shape tests of the same entry points stay where they are (tests/test_gpu_kernels.py, test_gpu_round3.py, test_gpu_round5.py,
test_gpu_round6.py, test_gpu_lstmcnn.py).

BRANCH_TABLE below is the reading of the dispatchers this module was written from: one row per `if` / `else` / `switch` arm of each
extern "C" entry point, as (entry point, condition as written in the .hip file, kernel instantiation launched -- as the profiler prints
it, default template arguments included -- and the case of this module that takes it).  Refusals are rows with kernel "(none)"; an arm
no case takes says "left out:" and why.  tests/test_fused_branch_table.py checks every kernel named here against the sources and every
__global__ of those sources against the list recorded from a profiled run of this module (tests/golden/fused_kernels_seen.txt,
profiles/fused_branches_kernel_stats.csv).

Bounds.
  NetVLAD: the constants of test_netvlad_fused_u8 -- assignment, sum and aggregate 2e-6 (nsplit 2) and 3e-3 (nsplit 1), dW_c / db_c 2e-5
    and 5e-3 of the reference's largest magnitude.  No case of this module needed a measured bound in their place.  Padding zeros of
    cT[:, :, F:], masked frames and a second call are compared bit for bit.
  Skinny GEMM / attention pooling: 2e-5 of max(1, largest |reference|) (test_skinny_gemm_kernels).  dW at M > 4096: FOUR times the
    error of torch's own fp32 evaluation of x^T dy against fp64 on the same data -- never anything the kernel produced.
  bf16 mixing backward: the fp64 gradient rounded to bf16 (round to nearest even, as _bf16_round of tests/test_gpu_kernels.py) with two
    bf16 ulps (2^-6 of the larger magnitude) plus 2e-6 of the largest reference magnitude.  The transposed outputs and the images are
    the plain outputs bit for bit (images decoded with oracle/x3_ref.py).  be_part is DEFINED as the column sums of the rounded values
    the kernel wrote: it is held to the fp64 column sum of those bf16 values under the four-times-torch-fp32 rule (the values
    themselves are held to fp64 by the element check), and to the fp64 column sum of the fp64 gradient within that plus the elements'
    own slack.
  CNN pooling: maxima and arg-max indices bit for bit on data whose sums are exact (small integers: equal maxima everywhere, the
    index must be the first); on real-valued data the values to (fs + 1) roundings of the terms' size and the index must point at a
    frame whose fp64 value is within that of the fp64 maximum.  The gathered dW element by element to (B + 8) roundings of the sum of
    the terms' magnitudes.
Each case prints its error and bound."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "yt8m_amd" not in sys.modules:              # the P128 child runs this file as a script, without the suite's conftest
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.load_package()

import yt8m_amd._lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

_ROWS = "vlad_rows_kernel<%d, %s, %d, false>"
BRANCH_TABLE = [
    # ---- netvlad_fused.hip -----------------------------------------------------------------------------------------------------------
    ("yt8m_netvlad_supported", "K == NK && D >= 64 && (D % 64) == 0 && B >= 1 && F >= 1 && B <= 65535 && F * D < 2^31", "(none)",
     "test_netvlad_refusals (K = 32, D = 100, B = 65536)"),
    ("yt8m_netvlad_workspace_bytes", "!supported: 0; else make_layout(B, F, D).total", "(none)",
     "every NetVLAD case (the workspace is allocated to the byte); test_netvlad_refusals: one byte short"),
    ("yt8m_netvlad_set_single", "mode < 0: -1 (environment / default), else 0 / 1", "(none)", "test_netvlad_single_pass (1, restored to -1)"),
    ("yt8m_netvlad_single_pass", "on && supported && (D % 128) == 0 && D <= 1152 && F <= VF", "(none)",
     "test_netvlad_single_pass[4-320-128-1], [3-300-1152-1] (1); [4-321-128-0] (F = 321), [3-20-1280-0] (D = 1280), [5-50-64-0] (D % 128): 0"),
    ("yt8m_netvlad_fwd_u8", "supported / nsplit 1 or 2 / null / 16-byte alignment / workspace_bytes >= total, else YT8M_E_*", "(none)",
     "test_netvlad_refusals"),
    ("yt8m_netvlad_fwd_u8", "(always) scale, pack and column sums of W_c",
     "vlad_absmax_part_kernel vlad_pack_kernel<false> vlad_cs_sum_kernel", "every NetVLAD case"),
    ("yt8m_netvlad_fwd_u8", "yt8m_netvlad_single_pass(B, F, D, K), nsplit == 2", "vlad_video_kernel<2>",
     "test_netvlad_single_pass[4-320-128-1], [3-300-1152-1]"),
    ("yt8m_netvlad_fwd_u8", "yt8m_netvlad_single_pass(B, F, D, K), else", "vlad_video_kernel<1>", "test_netvlad_single_pass[4-320-128-1], [3-300-1152-1]"),
    ("yt8m_netvlad_fwd_u8", "launch_rows<2, false>: switch (nt) case 1", _ROWS % (2, "false", 1),
     "test_netvlad_rows[5-50-64-1]; every B = 3 / grouping case"),
    ("yt8m_netvlad_fwd_u8", "launch_rows<2, false>: case 2", _ROWS % (2, "false", 2),
     "test_netvlad_rows[503-65-64-2] (partial tile), [128-640-64-2] (5 ranges), [512-128-64-2] (exact tile)"),
    ("yt8m_netvlad_fwd_u8", "launch_rows<2, false>: case 3", _ROWS % (2, "false", 3), "test_netvlad_rows[493-129-64-3], [256-330-64-3] (2 ranges)"),
    ("yt8m_netvlad_fwd_u8", "launch_rows<2, false>: case 4", _ROWS % (2, "false", 4), "test_netvlad_rows[494-193-64-4]"),
    ("yt8m_netvlad_fwd_u8", "launch_rows<2, false>: default (5)", _ROWS % (2, "false", 5), "test_netvlad_rows[475-257-64-5], [512-320-64-5] (exact tile)"),
    ("yt8m_netvlad_fwd_u8", "launch_rows<1, false>: switch (nt) 1 / 2 / 3 / 4 / default",
     " ".join(_ROWS % (1, "false", nt) for nt in (1, 2, 3, 4, 5)), "test_netvlad_rows: every case runs nsplit 2 and nsplit 1"),
    ("yt8m_netvlad_fwd_u8", "(pair) scale of c, n = sum over the ranges", "vlad_max_to_scale_kernel vlad_sum_parts_kernel",
     "test_netvlad_rows (ranges 1, 2, 5)"),
    ("yt8m_netvlad_fwd_u8", "launch_cols: nsplit == 2; grid ((D + 383) / 384, B), vids = 1", "vlad_cols_kernel<2>",
     "test_netvlad_cols_slices[64], [384] (one slice), [448] (64 of the second), [1024] (partial third), [1152] (three whole)"),
    ("yt8m_netvlad_fwd_u8", "launch_cols: else", "vlad_cols_kernel<1>", "test_netvlad_cols_slices (nsplit 1)"),
    ("yt8m_netvlad_bwd_u8", "supported / nsplit / null / beta 0 or 1 / alignment / workspace, else YT8M_E_*", "(none)",
     "test_netvlad_refusals (beta 0.5, nsplit 3, cT off by 4 bytes)"),
    ("yt8m_netvlad_bwd_u8", "(always) per-video scale, pack and column sums of dagg",
     "vlad_absmax_part_kernel vlad_pack_kernel<true> vlad_cs_sum_kernel", "every NetVLAD case (vanishing dagg: scale 1)"),
    ("yt8m_netvlad_bwd_u8", "launch_rows<2, true>: switch (nt) 1 / 2 / 3 / 4 / default",
     " ".join(_ROWS % (2, "true", nt) for nt in (1, 2, 3, 4, 5)), "test_netvlad_rows (the cases of the forward rows)"),
    ("yt8m_netvlad_bwd_u8", "launch_rows<1, true>: switch (nt) 1 / 2 / 3 / 4 / default",
     " ".join(_ROWS % (1, "true", nt) for nt in (1, 2, 3, 4, 5)), "test_netvlad_rows (nsplit 1)"),
    ("yt8m_netvlad_bwd_u8", "launch_cols over video groups: vids = 1", "vlad_cols_kernel<2> vlad_cols_kernel<1>",
     "test_netvlad_bwd_grouping[16-9-64-16-1] (groups = 16), [17-9-64-17-1]; test_netvlad_cols_slices"),
    ("yt8m_netvlad_bwd_u8", "launch_cols over video groups: vids > 1 (B > 384 / slices)", "vlad_cols_kernel<2> vlad_cols_kernel<1>",
     "test_netvlad_bwd_grouping[512-9-64-256-2] (groups = 256, vids = 2), [130-9-1152-65-2] (three slices: groups = 65, vids = 2); the NT cases"),
    ("yt8m_netvlad_bwd_u8", "L.groups > RED2: two-stage reduce", "vlad_part_reduce_kernel vlad_dw_reduce_kernel",
     "test_netvlad_bwd_grouping[17-9-64-17-1], [512-9-64-256-2], [130-9-1152-65-2]"),
    ("yt8m_netvlad_bwd_u8", "else: single-stage reduce", "vlad_dw_reduce_kernel", "test_netvlad_bwd_grouping[16-9-64-16-1]; test_netvlad_cols_slices (3 groups)"),
    ("yt8m_netvlad_bwd_u8", "dWc_beta != 0 (accumulate) / dbc_beta through yt8m_colsum_f32", "vlad_dw_reduce_kernel",
     "every NetVLAD case: beta 0, then beta 1 on top"),
    ("yt8m_netvlad_fwd_u8", "rows_p128(D): YT8M_NETVLAD_K128 != 0 && D % 128 == 0, nsplit 2, nt 1 and default (5)",
     "vlad_rows_kernel<2, false, 1, true> vlad_rows_kernel<2, false, 5, true>", "child: test_netvlad_p128_child_process (5, 50, 128), (475, 257, 128)"),
    ("yt8m_netvlad_bwd_u8", "rows_p128(D), nsplit 2, nt 1 and default (5)",
     "vlad_rows_kernel<2, true, 1, true> vlad_rows_kernel<2, true, 5, true>", "child: test_netvlad_p128_child_process"),
    ("yt8m_netvlad_fwd_u8", "rows_p128(D): the other instantiations",
     " ".join("vlad_rows_kernel<%d, %s, %d, true>" % (ns, bw, nt) for ns in (1, 2) for bw in ("false", "true") for nt in (1, 2, 3, 4, 5)
              if not (ns == 2 and nt in (1, 5))),
     "left out: the switch is a static read of the environment, so each needs a process of its own; the child covers both ends of NT at "
     "nsplit 2, the other sixteen share its code (template NT / NSPLIT loops, held by the P128 = false cases)"),
    # ---- gemm_skinny.hip -------------------------------------------------------------------------------------------------------------
    ("yt8m_skinny_supported", "N in 1..16, K >= 4, K % 4 == 0, M >= 1, ceil(K / 256) * 256 * NT * 4 <= 144 KiB", "(none)",
     "test_skinny_limits: K = 4608 / 4612 (NT 8), 2304 / 2308 (NT 16)"),
    ("yt8m_skinny_workspace_bytes", "max(chunks, 1) * K * NT * 4", "(none)", "test_skinny_f32 (allocated to the byte); test_skinny_limits: one byte short"),
    ("yt8m_skinny_fwd_f32", "skinny_check / supported / ld / alignment, else YT8M_E_*", "(none)", "test_skinny_limits"),
    ("yt8m_skinny_fwd_f32", "N <= 8", "skinny_fwd_kernel<8, float, 8>",
     "test_skinny_f32[1-1024-8], [65-1028-8], [37-4608-8] (largest K), [16384-64-8] (rows_per_wg 16), [32768-64-8], [32769-64-8]"),
    ("yt8m_skinny_fwd_f32", "else", "skinny_fwd_kernel<16, float, 8>", "test_skinny_f32[37-1028-9], [64-1024-9], [37-2304-16] (largest K), [16385-64-9] (rows_per_wg 32)"),
    ("yt8m_skinny_dw_f32", "skinny_check / null / ld / workspace, else YT8M_E_*", "(none)", "test_skinny_limits"),
    ("yt8m_skinny_dw_f32", "N <= 8, chunks > 0", "skinny_bwd_kernel<8, false, false, float> skinny_dw_reduce_kernel<8>",
     "test_skinny_f32: K = 1024 (nslices 1) / 1028 (2) / 4608 (5); M = 64 (1 chunk) / 65 (2); M = 32768 (rows 64) / 32769 (rows 128)"),
    ("yt8m_skinny_dw_f32", "else, chunks > 0", "skinny_bwd_kernel<16, false, false, float> skinny_dw_reduce_kernel<16>", "test_skinny_f32 (N = 9, 16)"),
    ("yt8m_skinny_dw_f32", "chunks == 0 (M = 0): the reduce alone writes beta * dW", "skinny_dw_reduce_kernel<8> skinny_dw_reduce_kernel<16>",
     "test_skinny_f32: every case ends with M = 0 at beta 0 and 1"),
    ("yt8m_skinny_dw_f32", "bwd_plan: want = 384 (nslices 4) / 308 (nslices 5) row chunks, where chunk_rows steps at M = 24576 / 19712", "skinny_bwd_kernel",
     "left out: M above those steps at K > 3072 is more than 300 MB of x; the same function is stepped at want = 512 (M = 32768 / 32769)"),
    ("yt8m_skinny_dx_f32", "skinny_check / null / ld / alignment, else YT8M_E_*", "(none)", "test_skinny_limits"),
    ("yt8m_skinny_dx_f32", "N <= 8", "skinny_bwd_kernel<8, true, false, float>", "test_skinny_f32 (N = 8)"),
    ("yt8m_skinny_dx_f32", "else", "skinny_bwd_kernel<16, true, false, float>", "test_skinny_f32 (N = 9, 16)"),
    ("yt8m_attn_pool_supported", "B in 1..65535, F >= 1, A in 1..16, H >= 4, H % 4 == 0, LDS image <= 144 KiB", "(none)", "test_attn_pool_refusals"),
    ("yt8m_attn_pool_fwd", "A <= 8", "skinny_bwd_kernel<8, false, true, float>", "test_attn_pool_f32[2-1-8-1024], [3-65-8-2048]"),
    ("yt8m_attn_pool_fwd", "else", "skinny_bwd_kernel<16, false, true, float>", "test_attn_pool_f32[2-64-9-1028], [2-65-9-1024]"),
    ("yt8m_attn_pool_bwd", "dw, A <= 8 / else", "skinny_fwd_kernel<8, float, 8> skinny_fwd_kernel<16, float, 8>", "test_attn_pool_f32: dw only, and with dx"),
    ("yt8m_attn_pool_bwd", "dx, A <= 8 / else", "skinny_bwd_kernel<8, true, true, float> skinny_bwd_kernel<16, true, true, float>",
     "test_attn_pool_f32: dx only, and with dw"),
    ("yt8m_attn_pool_bwd", "supported / null / alignment, else YT8M_E_*", "(none)", "test_attn_pool_refusals"),
    ("yt8m_u8_frame_scales", "(single kernel) D % 4 == 0, else YT8M_E_SHAPE", "u8_frame_scales_kernel", "test_skinny_u8, test_attn_pool_u8 (rs of every case); test_attn_pool_refusals"),
    ("yt8m_skinny_fwd_u8", "u8_check: K <= 2048, 4-byte alignment, else YT8M_E_SHAPE", "(none)", "test_skinny_limits (K = 2052, q off by a byte)"),
    ("yt8m_skinny_fwd_u8", "N <= 8 && K <= 1280", "skinny_fwd_kernel<8, unsigned char, 5>", "test_skinny_u8[1280-8]"),
    ("yt8m_skinny_fwd_u8", "N <= 8, else", "skinny_fwd_kernel<8, unsigned char, 8>", "test_skinny_u8[1288-8], [2048-8]"),
    ("yt8m_skinny_fwd_u8", "else (N > 8)", "skinny_fwd_kernel<16, unsigned char, 8>", "test_skinny_u8[1280-12], [1288-12], [2048-12]"),
    ("yt8m_skinny_dw_u8", "N <= 8", "skinny_bwd_kernel<8, false, false, unsigned char> skinny_dw_reduce_kernel<8>", "test_skinny_u8[*-8]"),
    ("yt8m_skinny_dw_u8", "else", "skinny_bwd_kernel<16, false, false, unsigned char> skinny_dw_reduce_kernel<16>", "test_skinny_u8[*-12]"),
    ("yt8m_attn_pool_fwd_u8", "A <= 8", "skinny_bwd_kernel<8, false, true, unsigned char>", "test_attn_pool_u8[2-1-8-1280], [2-64-8-1284], [2-65-8-2048]"),
    ("yt8m_attn_pool_fwd_u8", "else", "skinny_bwd_kernel<16, false, true, unsigned char>", "test_attn_pool_u8[3-65-9-1280], [2-64-12-1284]"),
    ("yt8m_attn_pool_dw_u8", "H <= 2048 && supported, else YT8M_E_SHAPE", "(none)", "test_attn_pool_refusals (H = 2052)"),
    ("yt8m_attn_pool_dw_u8", "A <= 8 && H <= 1280", "skinny_fwd_kernel<8, unsigned char, 5>", "test_attn_pool_u8[2-1-8-1280]"),
    ("yt8m_attn_pool_dw_u8", "A <= 8, else", "skinny_fwd_kernel<8, unsigned char, 8>", "test_attn_pool_u8[2-64-8-1284], [2-65-8-2048]"),
    ("yt8m_attn_pool_dw_u8", "else (A > 8)", "skinny_fwd_kernel<16, unsigned char, 8>", "test_attn_pool_u8[3-65-9-1280], [2-64-12-1284]"),
    # ---- moe_bf16.hip ----------------------------------------------------------------------------------------------------------------
    ("yt8m_moe_mix_bwd_bf16_partial_rows", "(B + 63) / 64", "(none)", "test_moe_mix_bwd_bf16 (the be_part buffer is allocated to the row)"),
    ("yt8m_moe_mix_bwd_bf16", "M == 2 / null / dp xor labels / pitches / label_dtype, else YT8M_E_*", "(none)", "test_moe_mix_bwd_bf16_refusals"),
    ("yt8m_moe_mix_bwd_bf16", "dp", "moe_mix_bwd_bf16_kernel<0, unsigned char, false, float>", "test_moe_mix_bwd_bf16[dp-*]"),
    ("yt8m_moe_mix_bwd_bf16", "label_dtype == 0", "moe_mix_bwd_bf16_kernel<1, unsigned char, false, float>", "test_moe_mix_bwd_bf16[u8-*]"),
    ("yt8m_moe_mix_bwd_bf16", "else (label_dtype == 1)", "moe_mix_bwd_bf16_kernel<1, float, false, float>", "test_moe_mix_bwd_bf16[f32-*]"),
    ("yt8m_moe_mix_bwd_bf16_images", "dp / label_dtype 0 / 1",
     "moe_mix_bwd_bf16_kernel<0, unsigned char, true, float> moe_mix_bwd_bf16_kernel<1, unsigned char, true, float> "
     "moe_mix_bwd_bf16_kernel<1, float, true, float>", "test_moe_mix_bwd_bf16 (every case decodes the images)"),
    ("yt8m_moe_mix_bwd_bf16_images", "image mode: K-block counts / 16-byte alignment, else YT8M_E_*", "(none)", "test_moe_mix_bwd_bf16_refusals"),
    ("yt8m_moe_mix_bwd_bf16_images_z16", "z16: dp / label_dtype 0 / 1",
     "moe_mix_bwd_bf16_kernel<0, unsigned char, true, unsigned short> moe_mix_bwd_bf16_kernel<1, unsigned char, true, unsigned short> "
     "moe_mix_bwd_bf16_kernel<1, float, true, unsigned short>", "test_moe_mix_bwd_bf16 (bf16 logits; V = 64 vector loads, V = 65 / 129 by element)"),
    ("yt8m_moe_mix_bwd_bf16", "z16 && !img (instantiated by the launch macro)",
     "moe_mix_bwd_bf16_kernel<0, unsigned char, false, unsigned short> moe_mix_bwd_bf16_kernel<1, unsigned char, false, unsigned short> "
     "moe_mix_bwd_bf16_kernel<1, float, false, unsigned short>",
     "left out: no extern \"C\" entry point passes bf16 logits with row-major outputs, so the C ABI cannot reach these three"),
    # ---- cnn_pool.hip ----------------------------------------------------------------------------------------------------------------
    ("yt8m_timepool_max_f32", "N % 4, ldy % 4, ldo % 4, null, alignment, else YT8M_E_*", "(none)", "test_timepool_refusals (N = 63, 65)"),
    ("yt8m_timepool_max_f32", "(single kernel) one filter of length 1; in kernel: 16 frame classes merged, the earlier frame on a tie",
     "timepool_shiftmax_kernel", "test_timepool_max: F = 1, 15, 16, 17, 40; N = 60, 64, 68; B = 1, 5"),
    ("yt8m_timepool_shiftmax_f32", "1..8 filters, columns % 4, ldz / ldo, else YT8M_E_*", "(none)", "test_timepool_refusals"),
    ("yt8m_timepool_shiftmax_f32", "(single kernel) in kernel: i < fs && i <= t", "timepool_shiftmax_kernel",
     "test_timepool_shiftmax: filters (1, 2, 4), F = 3, 4, 5, 37; B = 1, 5; a block that straddles two filters"),
    ("yt8m_u8_cnn_pool_dw", "dimensions / D % 4, D <= 2048 / beta / null / alignment, else YT8M_E_*", "(none)", "test_timepool_refusals"),
    ("yt8m_u8_cnn_pool_dw", "(single kernel) in kernel: t = idx - i >= 0; B > blockDim: several passes; t0 < D / 4", "u8_cnn_pool_dw_kernel",
     "test_u8_cnn_pool_dw: F = 3, 4, 5 (fs = 4); N = 63, 64, 65; B = 1, 5, 70 (two passes at D = 8); D = 260 (a partial wave)"),
    # ---- cnn_pool_f32.hip ------------------------------------------------------------------------------------------------------------
    ("yt8m_f32_cnn_pool_dw", "(single kernel)", "f32_cnn_pool_dw_kernel", "excluded: tests/test_gpu_lstmcnn.py::test_gather_kernels_against_float64_index_add"),
    ("yt8m_f32_cnn_pool_dx", "(single kernel) WS = slices per block, WT = 16 / WS frame classes", "f32_cnn_pool_dx_kernel",
     "excluded: tests/test_gpu_lstmcnn.py::test_gather_kernels_against_float64_index_add (D = 12, 132, 1152: WS = 1, 2, 3)"),
]

EPS32 = float(np.finfo(np.float32).eps)
PAD = 64              # elements of sentinel on each side of a guarded operand (a multiple of 16 bytes for every dtype used)
SENT = -7.0
A0, C0 = 4.0 / 255.0, 4.0 / 512.0 - 2.0
VEPS = 1e-12


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None


class G:
    """A flat operand of n elements inside a larger sentinel-filled buffer; the margins are checked after the call."""

    def __init__(self, dev, n, dtype=torch.float32, fill=SENT, body=None):
        self.fill, self.n, self.lo = fill, int(n), PAD
        self.buf = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.t = self.buf[self.lo:self.lo + self.n]
        if body is not None:
            self.t.fill_(body)

    def put(self, src):
        self.t.copy_(torch.as_tensor(src).reshape(-1))
        return self

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def view(self, *shape):
        return self.t.view(*shape)

    def cpu(self, *shape):
        return self.t.view(*shape).cpu()

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _report(what, err, bound):
    print("%s: err %.3g (bound %.3g)" % (what, err, bound))
    assert err <= bound, "%s: err %.6g > bound %.6g" % (what, err, bound)


def _maxerr(a, ref64):
    return float((a.double() - ref64).abs().max())


# ================================================================================================================================
# NetVLAD
def pick_nt(B, F):
    """Restatement of pick_nt of csrc/netvlad_fused.hip: a change of the heuristic fails the cases below instead of moving them."""
    best, best_score = 1, -1.0
    for nt in range(1, 6):
        ranges = (F + 64 * nt - 1) // (64 * nt)
        score = (F / (ranges * 64 * nt)) * min(1.0, (B * ranges) / 512.0) * (1.0 + 0.02 * nt)
        if score > best_score:
            best, best_score = nt, score
    return best


def vlad_layout(B, F, D):
    """(nt, ranges, groups, vids) of make_layout."""
    nt = pick_nt(B, F)
    groups = min(B, max(1, 384 // ((D + 383) // 384)))
    vids = (B + groups - 1) // groups
    return nt, (F + 64 * nt - 1) // (64 * nt), (B + vids - 1) // vids, vids


def _vlad_case(B, F, D):
    rs = np.random.RandomState(B * 1000 + F + D)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    q[0, 0] = 0
    q[0, F - 1] = 255
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0], nf[1], nf[2] = F, 1, 0
    Wc = (rs.randn(D, 64) * 3.0 / np.sqrt(D)).astype(np.float32)
    bc = (rs.randn(64) * 0.5).astype(np.float32)
    dagg = (rs.randn(B, 64, D) * 1e-3 * np.exp(rs.uniform(-1.0, 1.0, size=(B, 1, 1)))).astype(np.float32)   # per-video scales over e^+-1
    dn = (rs.randn(B, 64) * 1e-3).astype(np.float32)
    return dict(B=B, F=F, D=D, q=q, nf=nf, Wc=Wc, bc=bc, dagg=dagg, dn=dn)


def _vlad_ref(c):
    """fp64 on the CPU: x = l2_normalize(dequantise(q)) for EVERY frame, a = softmax(x W_c + b_c) [f < num_frames], agg = a^T x, and the
    backward into W_c / b_c for d(loss)/d(agg) = dagg, d(loss)/d(sum_f a) = dn."""
    B, F, D = c["B"], c["F"], c["D"]
    x0 = torch.from_numpy(c["q"]).double() * A0 + C0
    r = (x0 * x0).sum(-1).clamp(min=VEPS).rsqrt()                     # [B, F]
    xa = x0 * r[..., None]
    del x0
    mask = (torch.arange(F)[None, :] < torch.from_numpy(c["nf"])[:, None]).double()
    a = torch.softmax(xa @ torch.from_numpy(c["Wc"]).double() + torch.from_numpy(c["bc"]).double(), -1) * mask[..., None]
    agg = a.transpose(1, 2) @ xa
    da = xa @ torch.from_numpy(c["dagg"]).double().transpose(1, 2) + torch.from_numpy(c["dn"]).double()[:, None, :]
    ds = a * (da - (a * da).sum(-1, keepdim=True))
    dW = xa.reshape(B * F, D).t() @ ds.reshape(B * F, 64)
    return dict(a=a, r=r, agg=agg, n=a.sum(1), dW=dW, db=ds.sum((0, 1)))


class _VladDev:
    """The device operands of a case; q sits between sentinels and is compared with its source at the end."""

    def __init__(self, dev, c):
        self.c, self.dev = c, dev
        B, F, D = c["B"], c["F"], c["D"]
        self.Fp = (F + 31) // 32 * 32
        self.q = G(dev, B * F * D, torch.uint8, 0xA5).put(torch.from_numpy(c["q"]))
        self.nf = torch.from_numpy(c["nf"]).to(dev)
        self.Wc, self.bc = torch.from_numpy(c["Wc"]).to(dev), torch.from_numpy(c["bc"]).to(dev)
        self.dagg, self.dn = torch.from_numpy(c["dagg"]).to(dev), torch.from_numpy(c["dn"]).to(dev)
        self.nws = L.lib().yt8m_netvlad_workspace_bytes(B, F, D, 64)
        assert self.nws > 0

    def fwd(self, nsplit):
        c, dev = self.c, self.dev
        B, F, D = c["B"], c["F"], c["D"]
        ws = G(dev, self.nws, torch.uint8, 0xA5)
        cT, n, agg = G(dev, B * 64 * self.Fp), G(dev, B * 64), G(dev, B * 64 * D)
        L.check(L.lib().yt8m_netvlad_fwd_u8(self.q.p, _p(self.nf), _p(self.Wc), _p(self.bc), B, F, D, 64, nsplit, VEPS, cT.p, n.p, agg.p,
                                            ws.p, self.nws, _st()))
        torch.cuda.synchronize()
        assert all(g.intact() for g in (ws, cT, n, agg, self.q)), "a margin was written"
        return cT, n, agg

    def bwd(self, nsplit, cT, dW, db, beta, scale=1.0):
        c, dev = self.c, self.dev
        ws = G(dev, self.nws, torch.uint8, 0xA5)
        dagg, dn = (self.dagg, self.dn) if scale == 1.0 else (self.dagg * scale, self.dn * scale)
        L.check(L.lib().yt8m_netvlad_bwd_u8(self.q.p, _p(self.nf), cT.p, _p(dagg), _p(dn), c["B"], c["F"], c["D"], 64, nsplit, VEPS, dW.p, beta,
                                            db.p, beta, ws.p, self.nws, _st()))
        torch.cuda.synchronize()
        assert all(g.intact() for g in (ws, cT, dW, db, self.q)), "a margin was written"


def _vlad_check_fwd(tag, c, ref, cT, n, agg, nsplit):
    B, F, D = c["B"], c["F"], c["D"]
    Fp = (F + 31) // 32 * 32
    tol = 2e-6 if nsplit == 2 else 3e-3
    cTh = cT.cpu(B, 64, Fp)
    a = cTh[:, :, :F].transpose(1, 2).double() / ref["r"][..., None]                 # cT[b, k, f] = a[b, f, k] r[b, f]
    _report(tag + " assignment", _maxerr(a, ref["a"]), tol)
    _report(tag + " n = sum_f a", _maxerr(n.cpu(B, 64), ref["n"]), tol * F)
    aggh = agg.cpu(B, 64, D)
    _report(tag + " agg", _maxerr(aggh, ref["agg"]), tol * max(1.0, float(ref["agg"].abs().max())))
    # integer work, bit for bit: the padding of the frame axis, the masked frames, the empty video
    assert bool((cTh[:, :, F:] == 0).all()), "padding of cT is not zero"
    live = torch.arange(F)[None, :] < torch.from_numpy(c["nf"])[:, None]
    assert bool((cTh[:, :, :F].transpose(1, 2)[~live] == 0).all()), "a masked frame has a non-zero assignment"
    assert bool((aggh[2] == 0).all()) and bool((n.cpu(B, 64)[2] == 0).all())


def _vlad_run(dev, B, F, D, nsplits=(2, 1), expect_nt=None, backward=True):
    if expect_nt is not None:
        assert pick_nt(B, F) == expect_nt, "pick_nt(%d, %d) = %d: the heuristic changed, this case no longer takes NT = %d" % (
            B, F, pick_nt(B, F), expect_nt)
    c = _vlad_case(B, F, D)
    ref = _vlad_ref(c)
    v = _VladDev(dev, c)
    for nsplit in nsplits:
        tag = "netvlad (%d,%d,%d) nt=%d nsplit=%d" % (B, F, D, pick_nt(B, F), nsplit)
        cT, n, agg = v.fwd(nsplit)
        _vlad_check_fwd(tag, c, ref, cT, n, agg, nsplit)
        c2, n2, agg2 = v.fwd(nsplit)
        assert torch.equal(cT.t, c2.t) and torch.equal(n.t, n2.t) and torch.equal(agg.t, agg2.t), "the forward is not deterministic"
        del c2, n2, agg2
        if not backward:
            continue
        gt = 2e-5 if nsplit == 2 else 5e-3
        sW, sb = float(ref["dW"].abs().max()), max(float(ref["db"].abs().max()), 1e-6)
        dW, db = G(dev, D * 64), G(dev, 64)
        v.bwd(nsplit, cT, dW, db, 0.0)                                 # the kernel's own cT, as the training step
        _report(tag + " dW_c", _maxerr(dW.cpu(D, 64), ref["dW"]), gt * sW)
        _report(tag + " db_c", _maxerr(db.cpu(64), ref["db"]), gt * sb)
        first = dW.t.clone(), db.t.clone()
        v.bwd(nsplit, cT, dW, db, 1.0)                                 # beta = 1 accumulates
        _report(tag + " dW_c beta 1", _maxerr(dW.cpu(D, 64), 2 * ref["dW"]), 2 * gt * sW)
        _report(tag + " db_c beta 1", _maxerr(db.cpu(64), 2 * ref["db"]), 2 * gt * sb)
        dW2, db2 = G(dev, D * 64), G(dev, 64)
        v.bwd(nsplit, cT, dW2, db2, 0.0)
        assert torch.equal(dW2.t, first[0]) and torch.equal(db2.t, first[1]), "the backward is not deterministic"
        v.bwd(nsplit, cT, dW2, db2, 0.0, scale=1e-35)                  # vanishing upstream gradients: finite, no scale overflow
        assert bool(torch.isfinite(dW2.t).all()) and bool(torch.isfinite(db2.t).all()) and float(dW2.t.abs().max()) < 1e-30
    assert torch.equal(v.q.t.cpu(), torch.from_numpy(c["q"]).reshape(-1))
    return c, ref, v


# (B, F, D, nt): the smallest B F for which pick_nt returns 1 .. 5 (one range, partial last tile); several ranges; exact tiles
VLAD_ROWS = [(5, 50, 64, 1), (503, 65, 64, 2), (493, 129, 64, 3), (494, 193, 64, 4), (475, 257, 64, 5), (256, 330, 64, 3), (128, 640, 64, 2),
             (512, 128, 64, 2), (512, 320, 64, 5)]


@pytest.mark.parametrize("B,F,D,nt", VLAD_ROWS)
def test_netvlad_rows(dev, B, F, D, nt):
    want_ranges = {(256, 330): 2, (128, 640): 5}.get((B, F), 1)
    assert vlad_layout(B, F, D)[:2] == (nt, want_ranges)
    _vlad_run(dev, B, F, D, expect_nt=nt)


@pytest.mark.parametrize("D", [64, 384, 448, 1024, 1152])
def test_netvlad_cols_slices(dev, D):
    """vlad_cols_kernel: one 384-feature slice, exactly one, 64 features of a second, a partial third, three whole; F = 37 leaves the
    second 32-frame step partial."""
    _vlad_run(dev, 3, 37, D, expect_nt=1)


@pytest.mark.parametrize("B,F,D,groups,vids", [(16, 9, 64, 16, 1), (17, 9, 64, 17, 1), (512, 9, 64, 256, 2), (130, 9, 1152, 65, 2)])
def test_netvlad_bwd_grouping(dev, B, F, D, groups, vids):
    """groups = 16 is the last single-stage reduce (RED2 = 16), 17 the first two-stage one; B = 512 puts two videos on a workgroup of
    the cols kernel; D = 1152 caps the groups at 128, so B = 130 gives 65 groups of two."""
    assert vlad_layout(B, F, D)[2:] == (groups, vids)
    _vlad_run(dev, B, F, D, expect_nt=1)


@pytest.mark.parametrize("B,F,D,single", [(4, 320, 128, 1), (3, 300, 1152, 1), (4, 321, 128, 0), (3, 20, 1280, 0), (5, 50, 64, 0)])
def test_netvlad_single_pass(dev, B, F, D, single):
    """yt8m_netvlad_set_single(1): the one-workgroup-per-video forward where it applies (against fp64, not against the pair), the
    rows + cols pair where it does not (F > 320, D > 1152, D % 128 != 0)."""
    lib = L.lib()
    L.check(lib.yt8m_netvlad_set_single(1))
    try:
        assert lib.yt8m_netvlad_single_pass(B, F, D, 64) == single
        assert lib.yt8m_netvlad_single_pass(B, F, D, 32) == 0
        _vlad_run(dev, B, F, D, backward=bool(single))                 # (the backward reads the single pass's cT)
    finally:
        L.check(lib.yt8m_netvlad_set_single(-1))
    L.check(lib.yt8m_netvlad_set_single(0))
    try:
        assert lib.yt8m_netvlad_single_pass(B, F, D, 64) == 0
    finally:
        L.check(lib.yt8m_netvlad_set_single(-1))


def test_netvlad_refusals(dev):
    lib = L.lib()
    B, F, D = 3, 9, 64
    nws = lib.yt8m_netvlad_workspace_bytes(B, F, D, 64)
    assert lib.yt8m_netvlad_workspace_bytes(B, F, D, 32) == 0 and lib.yt8m_netvlad_workspace_bytes(B, F, 100, 64) == 0
    assert lib.yt8m_netvlad_supported(65535, 1, 64, 64) == 1 and lib.yt8m_netvlad_supported(65536, 1, 64, 64) == 0
    assert lib.yt8m_netvlad_supported(1, 1 << 20, 2048, 64) == 0      # F D = 2^31
    q = G(dev, B * F * D + 16, torch.uint8, 0xA5)
    ws = G(dev, nws, torch.uint8, 0xA5)
    out = [G(dev, B * 64 * 32), G(dev, B * 64), G(dev, B * 64 * D), G(dev, D * 64), G(dev, 64)]
    cT, n, agg, dW, db = out
    x = torch.zeros(B * 64 * D, device=dev)
    nf = torch.full((B,), F, dtype=torch.int32, device=dev)

    def fwd(K=64, D_=D, B_=B, nsplit=2, qp=q.p, nbytes=nws):
        return lib.yt8m_netvlad_fwd_u8(qp, _p(nf), _p(x), _p(x), B_, F, D_, K, nsplit, VEPS, cT.p, n.p, agg.p, ws.p, nbytes, _st())

    def bwd(K=64, D_=D, B_=B, nsplit=2, qp=q.p, nbytes=nws, beta=0.0, cp=cT.p):
        return lib.yt8m_netvlad_bwd_u8(qp, _p(nf), cp, _p(x), _p(x), B_, F, D_, K, nsplit, VEPS, dW.p, beta, db.p, beta, ws.p, nbytes, _st())

    off = ctypes.c_void_p(q.t.data_ptr() + 4)
    for f in (fwd, bwd):
        assert f(K=32) == -2 and f(D_=100) == -2 and f(B_=65536) == -2
        assert f(nsplit=3) == -1 and f(qp=off) == -1 and f(nbytes=nws - 1) == -1
    assert bwd(beta=0.5) == -1 and bwd(cp=ctypes.c_void_p(cT.t.data_ptr() + 4)) == -1
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out) and ws.untouched()


P128_SHAPES = [(5, 50, 128, 1), (475, 257, 128, 5)]


def _p128_child():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    assert os.environ.get("YT8M_NETVLAD_K128") == "1"
    for B, F, D, nt in P128_SHAPES:
        _vlad_run(dev, B, F, D, nsplits=(2,), expect_nt=nt)
    print("P128-CHILD-OK")


def test_netvlad_p128_child_process(dev):
    """The 128-byte walk of the rows kernels (YT8M_NETVLAD_K128=1) is a static read of the environment: a fresh process with the switch
    set for it alone runs nsplit 2 forward and backward at nt = 1 and nt = 5 against the same fp64 reference and prints the errors."""
    env = dict(os.environ, YT8M_NETVLAD_K128="1")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--p128-child"]
    res = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=240)
    print(res.stdout)
    assert res.returncode == 0, "the P128 child ended with status %d" % res.returncode
    assert "P128-CHILD-OK" in res.stdout
    lines = re.findall(r"^(netvlad .*): err (\S+) \(bound (\S+)\)$", res.stdout, re.M)
    assert len(lines) == 7 * len(P128_SHAPES), len(lines)             # 3 forward + 4 backward figures per shape
    for what, err, bound in lines:
        assert float(err) <= float(bound), what


# ================================================================================================================================
# skinny GEMM
def _rel_bound(ref64):
    return 2e-5 * max(1.0, float(ref64.abs().max()))


def _padded(dev, a, ld):
    """a [rows, cols] inside a guarded [rows, ld] buffer whose padding columns hold the sentinel."""
    rows, cols = a.shape
    g = G(dev, rows * ld, a.dtype, SENT if a.dtype.is_floating_point else 0x5A)
    if rows:
        g.view(rows, ld)[:, :cols] = a.to(dev)
    return g


def _pad_ok(g, rows, cols, ld):
    return g.intact() and (rows == 0 or ld == cols or bool((g.view(rows, ld)[:, cols:] == g.fill).all()))


SK_F32 = [(1, 1024, 8), (37, 1028, 9), (64, 1024, 9), (65, 1028, 8), (37, 4608, 8), (37, 2304, 16), (16384, 64, 8), (16385, 64, 9),
          (32768, 64, 8), (32769, 64, 8)]


def _bwd_plan(M, K):
    ns = (K + 1023) // 1024
    want = min(512, max(64, (1536 + ns - 1) // ns))
    rows = max(64, ((M + want - 1) // want + 63) // 64 * 64)
    return ns, rows, (M + rows - 1) // rows


@pytest.mark.parametrize("M,K,N", SK_F32)
def test_skinny_f32(dev, M, K, N):
    lib = L.lib()
    assert lib.yt8m_skinny_supported(M, K, N) == 1
    plan = _bwd_plan(M, K)
    want_plan = {(1, 1024): (1, 64, 1), (64, 1024): (1, 64, 1), (65, 1028): (2, 64, 2), (37, 4608): (5, 64, 1), (32768, 64): (1, 64, 512),
                 (32769, 64): (1, 128, 257)}.get((M, K))
    assert want_plan is None or plan == want_plan, plan
    NT = 8 if N <= 8 else 16
    assert lib.yt8m_skinny_workspace_bytes(M, K, N) == max(plan[2], 1) * K * NT * 4
    gen = torch.Generator().manual_seed(M + K + N)
    x, W, bias = torch.randn(M, K, generator=gen), torch.randn(K, N, generator=gen), torch.randn(N, generator=gen)
    dy, y0 = torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen)
    ldx, ldw, ldy, lddw = K + 4, N + 3, N + 1, N + 2
    gx, gW, gdy = _padded(dev, x, ldx), _padded(dev, W, ldw), _padded(dev, dy, ldy)
    gb = G(dev, N).put(bias)
    x64, W64, dy64 = x.double(), W.double(), dy.double()
    tag = "skinny (%d,%d,%d)" % (M, K, N)
    # forward: bias, then accumulate on top of y0 without it
    gy = _padded(dev, torch.zeros(M, N), ldy)
    L.check(lib.yt8m_skinny_fwd_f32(gx.p, ldx, gW.p, ldw, gb.p, gy.p, ldy, M, K, N, 0.0, _st()))
    ref = x64 @ W64 + bias.double()
    _report(tag + " fwd", _maxerr(gy.cpu(M, ldy)[:, :N], ref), _rel_bound(ref))
    gy2 = _padded(dev, y0, ldy)
    L.check(lib.yt8m_skinny_fwd_f32(gx.p, ldx, gW.p, ldw, None, gy2.p, ldy, M, K, N, 1.0, _st()))
    _report(tag + " fwd beta 1", _maxerr(gy2.cpu(M, ldy)[:, :N], x64 @ W64 + y0.double()), _rel_bound(ref))
    assert _pad_ok(gy, M, N, ldy) and _pad_ok(gy2, M, N, ldy)
    # dW through the chunked reduction
    nws = lib.yt8m_skinny_workspace_bytes(M, K, N)
    ws = G(dev, nws, torch.uint8, 0xA5)
    refdw = x64.t() @ dy64
    if M > 4096:
        bound = 4 * _maxerr((gx.view(M, ldx)[:, :K].t() @ gdy.view(M, ldy)[:, :N]).cpu(), refdw)     # torch's own fp32 product, same data
    else:
        bound = _rel_bound(refdw)
    gdW = _padded(dev, torch.zeros(K, N), lddw)
    L.check(lib.yt8m_skinny_dw_f32(gx.p, ldx, gdy.p, ldy, gdW.p, lddw, M, K, N, 0.0, ws.p, nws, _st()))
    _report(tag + " dW", _maxerr(gdW.cpu(K, lddw)[:, :N], refdw), bound)
    first = gdW.t.clone()
    L.check(lib.yt8m_skinny_dw_f32(gx.p, ldx, gdy.p, ldy, gdW.p, lddw, M, K, N, 1.0, ws.p, nws, _st()))
    _report(tag + " dW beta 1", _maxerr(gdW.cpu(K, lddw)[:, :N], 2 * refdw), 2 * bound)
    gdW2 = _padded(dev, torch.zeros(K, N), lddw)
    L.check(lib.yt8m_skinny_dw_f32(gx.p, ldx, gdy.p, ldy, gdW2.p, lddw, M, K, N, 0.0, ws.p, nws, _st()))
    assert torch.equal(gdW2.t, first), "dW is not deterministic"
    # M = 0: the reduce alone writes beta * dW
    L.check(lib.yt8m_skinny_dw_f32(None, ldx, None, ldy, gdW2.p, lddw, 0, K, N, 1.0, ws.p, nws, _st()))
    assert torch.equal(gdW2.t, first), "M = 0 at beta 1 changed dW"
    L.check(lib.yt8m_skinny_dw_f32(None, ldx, None, ldy, gdW2.p, lddw, 0, K, N, 0.0, ws.p, nws, _st()))
    assert bool((gdW2.view(K, lddw)[:, :N] == 0).all()), "M = 0 at beta 0 did not clear dW"
    assert _pad_ok(gdW, K, N, lddw) and _pad_ok(gdW2, K, N, lddw) and ws.intact()
    # dx
    refdx = dy64 @ W64.t()
    gdx = _padded(dev, torch.zeros(M, K), ldx)
    L.check(lib.yt8m_skinny_dx_f32(gdy.p, ldy, gW.p, ldw, gdx.p, ldx, M, K, N, 0.0, _st()))
    _report(tag + " dx", _maxerr(gdx.cpu(M, ldx)[:, :K], refdx), _rel_bound(refdx))
    L.check(lib.yt8m_skinny_dx_f32(gdy.p, ldy, gW.p, ldw, gdx.p, ldx, M, K, N, 1.0, _st()))
    _report(tag + " dx beta 1", _maxerr(gdx.cpu(M, ldx)[:, :K], 2 * refdx), 2 * _rel_bound(refdx))
    assert _pad_ok(gdx, M, K, ldx) and _pad_ok(gx, M, K, ldx) and _pad_ok(gW, K, N, ldw) and _pad_ok(gdy, M, N, ldy) and gb.intact()
    assert torch.equal(gx.cpu(M, ldx)[:, :K], x)


def test_skinny_limits(dev):
    lib = L.lib()
    sup = lib.yt8m_skinny_supported
    assert sup(1, 4608, 8) == 1 and sup(1, 4612, 8) == 0 and sup(1, 2304, 9) == 1 and sup(1, 2308, 9) == 0
    assert sup(1, 1026, 8) == 0 and sup(1, 8, 17) == 0 and sup(0, 8, 8) == 0
    g, out = G(dev, 64 * 4616), G(dev, 64 * 16)
    ws = G(dev, 4616 * 16 * 4, torch.uint8, 0xA5)
    s = _st()
    assert lib.yt8m_skinny_fwd_f32(g.p, 4612, g.p, 8, None, out.p, 8, 4, 4612, 8, 0.0, s) == -2      # K past the LDS image, NT = 8
    assert lib.yt8m_skinny_fwd_f32(g.p, 2308, g.p, 9, None, out.p, 9, 4, 2308, 9, 0.0, s) == -2      # NT = 16
    assert lib.yt8m_skinny_fwd_f32(g.p, 8, g.p, 17, None, out.p, 17, 4, 8, 17, 0.0, s) == -2         # N > 16
    assert lib.yt8m_skinny_fwd_f32(g.p, 8, g.p, 8, None, out.p, 8, 4, 6, 8, 0.0, s) == -2            # K % 4
    assert lib.yt8m_skinny_fwd_f32(g.p, 8, g.p, 8, None, out.p, 8, 4, 8, 8, 0.5, s) == -1            # beta
    assert lib.yt8m_skinny_fwd_f32(g.p, 6, g.p, 8, None, out.p, 8, 4, 8, 8, 0.0, s) == -2            # ldx < K
    assert lib.yt8m_skinny_fwd_f32(_p(g.t, 4), 8, g.p, 8, None, out.p, 8, 4, 8, 8, 0.0, s) == -2     # x 4-byte aligned
    nws = lib.yt8m_skinny_workspace_bytes(4, 8, 8)
    assert lib.yt8m_skinny_dw_f32(g.p, 8, g.p, 8, out.p, 8, 4, 8, 8, 0.0, ws.p, nws - 1, s) == -1    # workspace one byte short
    assert lib.yt8m_skinny_dw_f32(g.p, 8, g.p, 8, out.p, 7, 4, 8, 8, 0.0, ws.p, nws, s) == -2        # lddw < N
    assert lib.yt8m_skinny_dx_f32(g.p, 8, g.p, 8, out.p, 6, 4, 8, 8, 0.0, s) == -2                   # lddx < K
    assert lib.yt8m_skinny_dx_f32(g.p, 8, g.p, 8, out.p, 8, 4, 8, 8, 0.5, s) == -1
    q = G(dev, 4 * 2052 + 16, torch.uint8, 0xA5)
    assert lib.yt8m_skinny_fwd_u8(q.p, 2052, g.p, 8, None, None, g.p, out.p, 8, 4, 2052, 8, 0.0, s) == -2       # K > 2048
    assert lib.yt8m_skinny_fwd_u8(_p(q.t, 1), 8, g.p, 8, None, None, g.p, out.p, 8, 4, 8, 8, 0.0, s) == -2      # q off by a byte
    assert lib.yt8m_skinny_dw_u8(q.p, 2052, g.p, 8, None, out.p, 8, 4, 2052, 8, 0.0, ws.p, ws.n, s) == -2
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched()


def _u8_frames(dev, B, F, D, seed):
    """q, num_frames (F, 1, 0 among them), and the fp64 masked l2-normalised frames; rs from yt8m_u8_frame_scales, held to 2e-6."""
    lib = L.lib()
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    q[0, 0] = 0
    q[0, F - 1] = 255
    nf = rs.randint(1, F + 1, size=B).astype(np.int32)
    nf[0] = F
    if B > 1:
        nf[1] = 1
    if B > 2:
        nf[2] = 0
    xt = torch.from_numpy(q).double() * A0 + C0
    live = (torch.arange(F)[None, :] < torch.from_numpy(nf)[:, None]).double()
    r64 = live * (xt * xt).sum(-1).clamp(min=VEPS).rsqrt()
    gq = G(dev, B * F * D, torch.uint8, 0xA5).put(torch.from_numpy(q))
    grs = G(dev, B * F)
    nfd = torch.from_numpy(nf).to(dev)
    L.check(lib.yt8m_u8_frame_scales(gq.p, _p(nfd), B, F, D, VEPS, grs.p, _st()))
    _report("u8_frame_scales (%d,%d,%d)" % (B, F, D), _maxerr(grs.cpu(B, F), r64), 2e-6 * float(r64.max()))
    assert bool((grs.cpu(B, F)[live == 0] == 0).all()) and grs.intact()
    return gq, grs, xt * r64[..., None], rs


@pytest.mark.parametrize("K,N", [(1280, 8), (1288, 8), (2048, 8), (1280, 12), (1288, 12), (2048, 12)])
def test_skinny_u8(dev, K, N):
    lib = L.lib()
    B, F = 3, 23
    M = B * F
    gq, grs, x64, rs = _u8_frames(dev, B, F, K, K + N)
    x64 = x64.reshape(M, K)
    W = torch.from_numpy((rs.randn(K, N) * 0.3).astype(np.float32))
    bias = torch.from_numpy(rs.randn(N).astype(np.float32))
    dy = torch.from_numpy(rs.randn(M, N).astype(np.float32))
    ldw, ldy, lddw = N + 3, N + 1, N + 2
    gW, gdy, gb = _padded(dev, W, ldw), _padded(dev, dy, ldy), G(dev, N).put(bias)
    gcs = G(dev, N).put(W.double().sum(0).float())
    tag = "skinny u8 (%d,%d,%d)" % (M, K, N)
    gy = _padded(dev, torch.zeros(M, N), ldy)
    L.check(lib.yt8m_skinny_fwd_u8(gq.p, K, gW.p, ldw, gb.p, grs.p, gcs.p, gy.p, ldy, M, K, N, 0.0, _st()))
    ref = x64 @ W.double() + bias.double()
    _report(tag + " fwd", _maxerr(gy.cpu(M, ldy)[:, :N], ref), _rel_bound(ref))
    L.check(lib.yt8m_skinny_fwd_u8(gq.p, K, gW.p, ldw, None, grs.p, gcs.p, gy.p, ldy, M, K, N, 1.0, _st()))
    _report(tag + " fwd beta 1", _maxerr(gy.cpu(M, ldy)[:, :N], 2 * ref - bias.double()), 2 * _rel_bound(ref))
    nws = lib.yt8m_skinny_workspace_bytes(M, K, N)
    ws = G(dev, nws, torch.uint8, 0xA5)
    old = torch.from_numpy(rs.randn(K, N).astype(np.float32))
    refdw = x64.t() @ dy.double()
    gdW = _padded(dev, old, lddw)
    L.check(lib.yt8m_skinny_dw_u8(gq.p, K, gdy.p, ldy, grs.p, gdW.p, lddw, M, K, N, 0.0, ws.p, nws, _st()))
    _report(tag + " dW", _maxerr(gdW.cpu(K, lddw)[:, :N], refdw), _rel_bound(refdw))
    gdW1 = _padded(dev, old, lddw)
    L.check(lib.yt8m_skinny_dw_u8(gq.p, K, gdy.p, ldy, grs.p, gdW1.p, lddw, M, K, N, 1.0, ws.p, nws, _st()))
    _report(tag + " dW beta 1", _maxerr(gdW1.cpu(K, lddw)[:, :N], old.double() + refdw), _rel_bound(refdw))
    assert all(_pad_ok(g, r, c, ld) for g, r, c, ld in ((gy, M, N, ldy), (gdW, K, N, lddw), (gdW1, K, N, lddw), (gW, K, N, ldw), (gdy, M, N, ldy)))
    assert ws.intact() and gq.intact() and grs.intact() and gcs.intact() and gb.intact()


# ---- attention pooling -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,A,H", [(2, 1, 8, 1024), (2, 64, 9, 1028), (3, 65, 8, 2048), (2, 65, 9, 1024)])
def test_attn_pool_f32(dev, B, F, A, H):
    lib = L.lib()
    assert lib.yt8m_attn_pool_supported(B, F, A, H) == 1
    gen = torch.Generator().manual_seed(B + F + A + H)
    w, x, dC = torch.rand(B, F, A, generator=gen), torch.randn(B, F, H, generator=gen), torch.randn(B, A, H, generator=gen)
    gw, gx, gdC = G(dev, B * F * A).put(w), G(dev, B * F * H).put(x), G(dev, B * A * H).put(dC)
    tag = "attn_pool (%d,%d,%d,%d)" % (B, F, A, H)
    gC = G(dev, B * A * H)
    L.check(lib.yt8m_attn_pool_fwd(gw.p, gx.p, gC.p, B, F, A, H, _st()))
    refC = w.double().transpose(1, 2) @ x.double()
    _report(tag + " fwd", _maxerr(gC.cpu(B, A, H), refC), _rel_bound(refC))
    refdw = x.double() @ dC.double().transpose(1, 2)
    refdx = w.double() @ dC.double()
    outs = []
    for want_dw, want_dx in ((True, False), (False, True), (True, True)):
        gdw, gdx = G(dev, B * F * A), G(dev, B * F * H)
        L.check(lib.yt8m_attn_pool_bwd(gw.p, gx.p, gdC.p, gdw.p if want_dw else None, gdx.p if want_dx else None, B, F, A, H, _st()))
        what = " bwd (%s)" % ("both" if want_dw and want_dx else "dw only" if want_dw else "dx only")
        if want_dw:
            _report(tag + what + " dw", _maxerr(gdw.cpu(B, F, A), refdw), _rel_bound(refdw))
        else:
            assert gdw.untouched()
        if want_dx:
            _report(tag + what + " dx", _maxerr(gdx.cpu(B, F, H), refdx), _rel_bound(refdx))
        else:
            assert gdx.untouched()
        assert gdw.intact() and gdx.intact()
        outs.append((gdw.t.clone(), gdx.t.clone()))
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])
    assert all(g.intact() for g in (gw, gx, gdC, gC)) and torch.equal(gx.cpu(B, F, H), x)


@pytest.mark.parametrize("B,F,A,H", [(2, 1, 8, 1280), (2, 64, 8, 1284), (3, 65, 9, 1280), (2, 65, 8, 2048), (2, 64, 12, 1284)])
def test_attn_pool_u8(dev, B, F, A, H):
    lib = L.lib()
    gq, grs, x64, rs = _u8_frames(dev, B, F, H, B + F + A + H)
    w = torch.from_numpy(rs.rand(B, F, A).astype(np.float32))
    dC = torch.from_numpy(rs.randn(B, A, H).astype(np.float32))
    gw, gdC = G(dev, B * F * A).put(w), G(dev, B * A * H).put(dC)
    gsum = G(dev, B * A).put(dC.double().sum(-1).float())
    tag = "attn_pool u8 (%d,%d,%d,%d)" % (B, F, A, H)
    gC = G(dev, B * A * H)
    L.check(lib.yt8m_attn_pool_fwd_u8(gw.p, gq.p, grs.p, gC.p, B, F, A, H, _st()))
    refC = w.double().transpose(1, 2) @ x64
    _report(tag + " fwd", _maxerr(gC.cpu(B, A, H), refC), _rel_bound(refC))
    gdw = G(dev, B * F * A)
    L.check(lib.yt8m_attn_pool_dw_u8(gq.p, grs.p, gdC.p, gsum.p, gdw.p, B, F, A, H, _st()))
    refdw = x64 @ dC.double().transpose(1, 2)
    _report(tag + " dw", _maxerr(gdw.cpu(B, F, A), refdw), _rel_bound(refdw))
    assert all(g.intact() for g in (gq, grs, gw, gdC, gsum, gC, gdw))


def test_attn_pool_refusals(dev):
    lib = L.lib()
    sup = lib.yt8m_attn_pool_supported
    assert sup(1, 1, 8, 4608) == 1 and sup(1, 1, 8, 4612) == 0 and sup(1, 1, 9, 2304) == 1 and sup(1, 1, 9, 2308) == 0
    assert sup(1, 1, 17, 8) == 0 and sup(65536, 1, 8, 8) == 0 and sup(1, 1, 8, 6) == 0
    g, out = G(dev, 4 * 2052 * 8), G(dev, 4 * 2052 * 8)
    q = G(dev, 4 * 2052 + 16, torch.uint8, 0xA5)
    s = _st()
    assert lib.yt8m_attn_pool_fwd(g.p, g.p, out.p, 1, 4, 17, 8, s) == -2
    assert lib.yt8m_attn_pool_fwd(g.p, g.p, out.p, 1, 4, 8, 6, s) == -2
    assert lib.yt8m_attn_pool_fwd(g.p, _p(g.t, 4), out.p, 1, 4, 8, 8, s) == -1
    assert lib.yt8m_attn_pool_bwd(g.p, g.p, g.p, out.p, out.p, 1, 4, 17, 8, s) == -2
    assert lib.yt8m_attn_pool_bwd(g.p, g.p, g.p, out.p, _p(out.t, 4), 1, 4, 8, 8, s) == -1
    assert lib.yt8m_attn_pool_bwd(g.p, None, g.p, out.p, None, 1, 4, 8, 8, s) == -1                   # dw without x
    assert lib.yt8m_attn_pool_dw_u8(q.p, g.p, g.p, g.p, out.p, 1, 4, 8, 2052, s) == -2                 # H > 2048
    assert lib.yt8m_attn_pool_dw_u8(q.p, g.p, g.p, g.p, out.p, 1, 4, 8, 2048, s) == 0                  # (the last accepted width)
    out.t.fill_(SENT)
    assert lib.yt8m_attn_pool_dw_u8(_p(q.t, 1), g.p, g.p, g.p, out.p, 1, 4, 8, 8, s) == -1
    assert lib.yt8m_attn_pool_fwd_u8(g.p, _p(q.t, 2), g.p, out.p, 1, 4, 8, 8, s) == -1
    assert lib.yt8m_u8_frame_scales(q.p, None, 1, 4, 6, VEPS, out.p, s) == -2                          # D % 4
    torch.cuda.synchronize()
    assert out.untouched()


# ================================================================================================================================
# bf16 mixing backward
def _bf16_round(a):
    """round-to-nearest-even fp32 -> bf16, returned as float32 values (as _bf16_round of tests/test_gpu_kernels.py)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _bits_f32(t16):
    """int16 tensor of bf16 bit patterns -> float32 numpy values."""
    return (t16.contiguous().cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def _mixb_ref(Zg, Ze, dp, y, eps, dscale):
    """fp64 mixing backward (M = 2): g = softmax(Zg), e = sigmoid(Ze), p = g0 e0 + g1 e1; d = dp, or the cross-entropy's dL/dp."""
    g = torch.softmax(Zg.double(), -1)
    e = torch.sigmoid(Ze.double())
    p = (g[..., :2] * e).sum(-1)
    d = dp.double() if y is None else -(y.double() / (p + eps) - (1 - y.double()) / (1 - p + eps)) * dscale
    epad = torch.cat([e, torch.zeros_like(e[..., :1])], -1)
    return (d[..., None] * g * (epad - p[..., None])).numpy(), (d[..., None] * g[..., :2] * e * (1 - e)).numpy()


def _mixb_close(what, a, ref64):
    ref = _bf16_round(ref64.astype(np.float32)).astype(np.float64)
    tol = np.maximum(np.abs(ref), np.abs(a)) * 2.0 ** -6 + 2e-6 * np.abs(ref).max()
    _report(what + " err / (2 bf16 ulp + 2e-6 max)", float((np.abs(a - ref) / tol).max()), 1.0)
    return tol


MIXB_MODES = {"dp": (0, None), "u8": (1, 0), "f32": (1, 1)}


@pytest.mark.parametrize("B,V", [(64, 64), (65, 65), (37, 129)])
@pytest.mark.parametrize("mode", ["dp", "u8", "f32"])
def test_moe_mix_bwd_bf16(dev, mode, B, V):
    """All three entry points against fp64: row-major outputs from fp32 logits; images from fp32 logits; images from bf16 logits (the
    fp64 reference then starts from the rounded logits).  (64, 64) is one whole tile with aligned pitches (16-byte stores), (65, 65) is
    ragged in both directions with odd pitches (stores by element), (37, 129) is a partial row tile over three label tiles."""
    from oracle import x3_ref
    lib = L.lib()
    gen = torch.Generator().manual_seed(B * 7 + V)
    Zg, Ze = torch.randn(B, V, 3, generator=gen) * 2, torch.randn(B, V, 2, generator=gen) * 2
    eps, upstream, upv = 1e-5, 0.7, 0.35
    if mode == "dp":
        dp, lab, y, code, dscale, up = torch.randn(B, V, generator=gen), None, None, 0, 1.0, None
    else:
        yb = torch.rand(B, V, generator=gen) < 0.1
        dp, dscale, up = None, upstream / B, torch.tensor([upv], device=dev)
        if mode == "u8":
            lab, y, code = G(dev, B * V, torch.uint8, 7).put(yb.to(torch.uint8)), yb.double(), 0
        else:
            ys = yb.float() * 0.9 + 0.05                              # smoothed labels
            lab, y, code = G(dev, B * V).put(ys), ys.double(), 1
    gdp = G(dev, B * V).put(dp) if dp is not None else None
    nrow = lib.yt8m_moe_mix_bwd_bf16_partial_rows(B)
    assert nrow == (B + 63) // 64
    al = V % 8 == 0
    ldg, lde, ldt = (3 * V + 8, 2 * V + 8, B + 8) if al else (3 * V + 5, 2 * V + 3, B + 3)
    kb = lambda K: (K + 15) // 16
    img_n = lambda rows, K: (rows + 31) // 32 * kb(K) * 512
    tag = "mix_bwd_bf16 %s [%d,%d]" % (mode, B, V)
    plain = {}
    for zt in ("f32", "bf16"):
        zg_in = Zg if zt == "f32" else Zg.to(torch.bfloat16).float()
        ze_in = Ze if zt == "f32" else Ze.to(torch.bfloat16).float()
        rg, re = _mixb_ref(zg_in, ze_in, dp, y, eps, dscale * (upv if mode != "dp" else 1.0))
        rg, re = rg.reshape(B, 3 * V), re.reshape(B, 2 * V)
        gZg, gZe = G(dev, B * V * 3).put(zg_in), G(dev, B * V * 2).put(ze_in)
        # row-major outputs (fp32 logits: the only form the C ABI offers; for the bf16 case the rounded logits as floats)
        outs = [G(dev, n, torch.int16, 0x5A5A) for n in (B * ldg, 3 * V * ldt, B * lde, 2 * V * ldt)]
        part = G(dev, nrow * 2 * V)
        L.check(lib.yt8m_moe_mix_bwd_bf16(gZg.p, gZe.p, gdp.p if gdp else None, lab.p if lab else None, code, B, V, 2, eps, dscale,
                                          _p(up), outs[0].p, ldg, outs[1].p, ldt, outs[2].p, lde, outs[3].p, ldt, part.p, _st()))
        gb, gt, eb, et = outs[0].view(B, ldg), outs[1].view(3 * V, ldt), outs[2].view(B, lde), outs[3].view(2 * V, ldt)
        vg, ve = _bits_f32(gb[:, :3 * V]), _bits_f32(eb[:, :2 * V])
        tolg = _mixb_close(tag + " Z " + zt + " dZg", vg.astype(np.float64), rg)
        tole = _mixb_close(tag + " Z " + zt + " dZe", ve.astype(np.float64), re)
        assert torch.equal(gt[:, :B], gb[:, :3 * V].t()) and torch.equal(et[:, :B], eb[:, :2 * V].t()), "transposed outputs differ from the plain ones"
        assert bool((gb[:, 3 * V:] == 0x5A5A).all()) and bool((eb[:, 2 * V:] == 0x5A5A).all()) and bool((gt[:, B:] == 0x5A5A).all()) \
            and bool((et[:, B:] == 0x5A5A).all()), "the pitch padding was written"
        assert all(o.intact() for o in outs) and part.intact() and gZg.intact() and gZe.intact()
        # be_part: column sums of the rounded values over each 64-row block
        ebv = torch.from_numpy(ve)
        pad = torch.zeros(nrow * 64, 2 * V)
        pad[:B] = ebv
        blocks = pad.view(nrow, 64, 2 * V)
        s64 = blocks.double().sum(1)
        b4 = 4 * _maxerr(blocks.to(dev).sum(1).cpu(), s64)             # torch's own fp32 sum of the same values
        _report(tag + " Z " + zt + " be_part vs fp64 sum of the written bf16 values (4 x torch fp32)", _maxerr(part.cpu(nrow, 2 * V), s64), b4)
        refpad = np.zeros((nrow * 64, 2 * V))
        refpad[:B] = re
        tolpad = np.zeros((nrow * 64, 2 * V))
        tolpad[:B] = tole
        e2 = np.abs(part.cpu(nrow, 2 * V).numpy().astype(np.float64) - refpad.reshape(nrow, 64, -1).sum(1))
        _report(tag + " Z " + zt + " be_part vs fp64 sum of the fp64 gradient, err / (elements' slack + 4 x torch fp32)",
                float((e2 / (tolpad.reshape(nrow, 64, -1).sum(1) + b4 + 1e-30)).max()), 1.0)
        plain[zt] = (vg, ve, part.t.clone())
        # images: every entry point that writes them, decoded with the oracle, against the plain outputs bit for bit
        forms = [("images", lib.yt8m_moe_mix_bwd_bf16_images, gZg, gZe)]
        if zt == "bf16":
            z16g = G(dev, B * V * 3, torch.int16, 0x5A5A).put(Zg.to(torch.bfloat16).view(torch.int16))
            z16e = G(dev, B * V * 2, torch.int16, 0x5A5A).put(Ze.to(torch.bfloat16).view(torch.int16))
            forms.append(("images_z16", lib.yt8m_moe_mix_bwd_bf16_images_z16, z16g, z16e))
        for name, fn, zg_dev, ze_dev in forms:
            imgs = [G(dev, img_n(r, K), torch.int16, 0x5A5A, body=0) for r, K in ((B, 3 * V), (3 * V, B), (B, 2 * V), (2 * V, B))]
            ipart = G(dev, nrow * 2 * V)
            L.check(fn(zg_dev.p, ze_dev.p, gdp.p if gdp else None, lab.p if lab else None, code, B, V, 2, eps, dscale, _p(up), imgs[0].p,
                       kb(3 * V), imgs[1].p, kb(B), imgs[2].p, kb(2 * V), imgs[3].p, kb(B), ipart.p, _st()))
            for img, mat in zip(imgs, (vg, vg.T, ve, ve.T)):
                want = x3_ref.image(mat)[:, :, 0].reshape(-1).astype(np.uint16)
                got = img.t.cpu().numpy().view(np.uint16)
                assert np.array_equal(got, want), "%s %s: an image differs from the plain output" % (tag, name)
                assert img.intact()
            assert torch.equal(ipart.t, part.t) and ipart.intact() and zg_dev.intact() and ze_dev.intact()
        print("%s Z %s: the images of %s decode to the plain outputs bit for bit" % (tag, zt, " and ".join(f[0] for f in forms)))
    if lab is not None:
        assert lab.intact()


def test_moe_mix_bwd_bf16_instantiations_named():
    """The launch macro instantiates MODE 0 / 1 x labels uint8 / float (MODE 1) x plain / image x fp32 / bf16 logits = twelve; the table
    names exactly those, three of them as out of the C ABI's reach."""
    names = set()
    for row in BRANCH_TABLE:
        names.update(re.findall(r"moe_mix_bwd_bf16_kernel<[^>]*>", row[2]))
    assert len(names) == 12, sorted(names)
    want = {"moe_mix_bwd_bf16_kernel<%s, %s, %s>" % (ml, img, zt) for ml in ("0, unsigned char", "1, unsigned char", "1, float")
            for img in ("false", "true") for zt in ("float", "unsigned short")}
    assert names == want


def test_moe_mix_bwd_bf16_refusals(dev):
    lib = L.lib()
    g = G(dev, 4096)
    out = G(dev, 4096, torch.int16, 0x5A5A)
    o, s = out.p, _st()
    f, fi = lib.yt8m_moe_mix_bwd_bf16, lib.yt8m_moe_mix_bwd_bf16_images
    assert f(g.p, g.p, g.p, None, 0, 4, 8, 3, 1e-5, 1.0, None, o, 24, o, 8, o, 16, o, 8, None, s) == -1          # M != 2
    assert f(g.p, g.p, g.p, g.p, 0, 4, 8, 2, 1e-5, 1.0, None, o, 24, o, 8, o, 16, o, 8, None, s) == -1           # dp and labels
    assert f(g.p, g.p, None, None, 0, 4, 8, 2, 1e-5, 1.0, None, o, 24, o, 8, o, 16, o, 8, None, s) == -1         # neither
    assert f(g.p, g.p, g.p, None, 0, 4, 8, 2, 1e-5, 1.0, None, o, 20, o, 8, o, 16, o, 8, None, s) == -2          # pitch < 3 V
    assert f(g.p, g.p, g.p, None, 0, 4, 8, 2, 1e-5, 1.0, None, o, 24, o, 3, o, 16, o, 8, None, s) == -2          # pitch < B
    assert f(g.p, g.p, None, g.p, 2, 4, 8, 2, 1e-5, 1.0, None, o, 24, o, 8, o, 16, o, 8, None, s) == -1          # label_dtype
    assert fi(g.p, g.p, g.p, None, 0, 4, 8, 2, 1e-5, 1.0, None, o, 24, o, 1, o, 1, o, 1, None, s) == -2          # not the K-block count
    assert fi(g.p, g.p, g.p, None, 0, 4, 8, 2, 1e-5, 1.0, None, _p(out.t, 2), 2, o, 1, o, 1, o, 1, None, s) == -1   # image off by 2 bytes
    torch.cuda.synchronize()
    assert out.untouched()


# ================================================================================================================================
# CNN pooling
def _shiftmax_ref(z, F, B, filters):
    """z [F B rows (t B + b), sum fs_k N_k] fp64 -> cnn_output [F, B, sum N_k]: sum over the shifts i < fs, i <= t."""
    cols, zb = [], 0
    z3 = z.reshape(F, B, -1)
    for fs, nk in filters:
        o = np.zeros((F, B, nk))
        for i in range(fs):
            o[i:] += z3[:F - i, :, zb + i * nk:zb + (i + 1) * nk] if i < F else 0.0
        cols.append(o)
        zb += fs * nk
    return np.concatenate(cols, -1)


def _run_shiftmax(dev, F, B, filters, data, plain):
    lib = L.lib()
    ztot, ntot = sum(fs * nk for fs, nk in filters), sum(nk for _, nk in filters)
    ldz, ldo = ztot + 4, ntot + 4
    rs = np.random.RandomState(F * 100 + B + ntot)
    z = rs.randint(-3, 4, size=(F * B, ztot)).astype(np.float32) if data == "int" else rs.randn(F * B, ztot).astype(np.float32)
    gz = _padded(dev, torch.from_numpy(z), ldz)
    gout, gidx = G(dev, B * ldo), G(dev, B * ldo, torch.int32, -77)
    if plain:
        L.check(lib.yt8m_timepool_max_f32(gz.p, F, B, ntot, ldz, gout.p, gidx.p, ldo, _st()))
    else:
        fsa = (ctypes.c_int32 * len(filters))(*[fs for fs, _ in filters])
        nca = (ctypes.c_int32 * len(filters))(*[nk for _, nk in filters])
        L.check(lib.yt8m_timepool_shiftmax_f32(gz.p, F, B, ldz, len(filters), fsa, nca, gout.p, gidx.p, ldo, _st()))
    o64 = _shiftmax_ref(z.astype(np.float64), F, B, filters)           # [F, B, ntot]
    want_v, want_i = o64.max(0), o64.argmax(0)                         # argmax: the first of equal maxima
    got_v, got_i = gout.cpu(B, ldo)[:, :ntot].numpy(), gidx.cpu(B, ldo)[:, :ntot].numpy()
    tag = "timepool %s F=%d B=%d %s %s" % ("max" if plain else "shiftmax", F, B, filters, data)
    if data == "int":                                                  # every sum is exact: values and first indices bit for bit
        ties = int(((o64 == want_v[None]).sum(0) > 1).sum())
        assert F == 1 or ties > 0
        assert np.array_equal(got_v.astype(np.float64), want_v), tag
        assert np.array_equal(got_i, want_i), tag + ": an arg-max index is not the first maximum"
        print("%s: values and indices bit for bit (%d of %d columns have equal maxima)" % (tag, ties, B * ntot))
    else:
        S = max(fs for fs, _ in filters)
        bound = (S + 1) * EPS32 * _shiftmax_ref(np.abs(z).astype(np.float64), F, B, filters).max()
        _report(tag + " values", float(np.abs(got_v - want_v).max()), bound if S > 1 else 0.0)
        assert got_i.min() >= 0 and got_i.max() < F
        at = np.take_along_axis(o64, got_i[None].astype(np.int64), 0)[0]
        _report(tag + " fp64 value at the kept frame below the fp64 maximum", float((want_v - at).max()), 2 * bound if S > 1 else 0.0)
    assert _pad_ok(gout, B, ntot, ldo) and _pad_ok(gidx, B, ntot, ldo) and _pad_ok(gz, F * B, ztot, ldz)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [60, 64, 68])
@pytest.mark.parametrize("F", [1, 15, 16, 17, 40])
def test_timepool_max(dev, F, N, B):
    """The plain maximum over the frames: F below / at / above the kernel's 16 frame classes, N below / at / above one 64-column block."""
    _run_shiftmax(dev, F, B, [(1, N)], "int", True)
    _run_shiftmax(dev, F, B, [(1, N)], "real", True)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("F", [3, 4, 5, 37])
def test_timepool_shiftmax(dev, F, B):
    """Filters of length 1, 2 and 4: F below, at and above the longest; 60 + 8 + 64 columns put two filters into the first block."""
    for filters in ([(1, 60), (2, 8), (4, 64)], [(4, 64)]):
        _run_shiftmax(dev, F, B, filters, "int", False)
        _run_shiftmax(dev, F, B, filters, "real", False)


@pytest.mark.parametrize("B,F,D,N,fs", [(1, 3, 8, 63, 4), (5, 4, 8, 64, 4), (5, 5, 260, 65, 4), (70, 9, 8, 5, 3), (5, 5, 64, 64, 1)])
def test_u8_cnn_pool_dw(dev, B, F, D, N, fs):
    lib = L.lib()
    rs = np.random.RandomState(B + F + D + N)
    q = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8)
    ldg = N + 3
    idx = rs.randint(0, F, size=(B, N)).astype(np.int32)
    idx[:, 0], idx[:, 1], idx[:, 2] = 0, min(1, F - 1), F - 1
    g = rs.randn(B, N).astype(np.float32)
    xt = A0 * q.astype(np.float64) + C0
    r_tm = (1.0 / np.sqrt((xt ** 2).sum(-1))).T.astype(np.float32)   # [F, B], time-major
    r_tm[F - 1, B - 1] = 0.0                                           # a padding frame
    old = rs.randn(fs * D, N).astype(np.float32)
    ref = np.zeros((fs * D, N))
    mag = np.zeros((fs * D, N))
    bb = np.arange(B)[:, None]
    for i in range(fs):
        t = idx - i
        coef = np.where(t >= 0, g.astype(np.float64) * r_tm.astype(np.float64)[t.clip(0), bb], 0.0)    # [B, N]
        X = xt[bb, t.clip(0)]                                          # [B, N, D]
        ref[i * D:(i + 1) * D] = np.einsum("bn,bnd->dn", coef, X)
        mag[i * D:(i + 1) * D] = np.einsum("bn,bnd->dn", np.abs(coef), A0 * q[bb, t.clip(0)].astype(np.float64) + abs(C0))
    gq = G(dev, B * F * D, torch.uint8, 0xA5).put(torch.from_numpy(q))
    gr, gi, gg = G(dev, F * B).put(torch.from_numpy(r_tm)), _padded(dev, torch.from_numpy(idx), ldg), _padded(dev, torch.from_numpy(g), ldg)
    tag = "u8_cnn_pool_dw (%d,%d,%d,%d) fs=%d" % (B, F, D, N, fs)
    tol = (B + 8) * EPS32 * mag + 1e-30
    for beta in (0.0, 1.0):
        gd = G(dev, fs * D * N).put(torch.from_numpy(old))
        L.check(lib.yt8m_u8_cnn_pool_dw(gq.p, gr.p, gi.p, gg.p, ldg, B, F, D, N, fs, gd.p, beta, _st()))
        want = ref + beta * old.astype(np.float64)
        err = np.abs(gd.cpu(fs * D, N).numpy().astype(np.float64) - want)
        _report(tag + " beta %g err / ((B + 8) roundings of the terms)" % beta, float((err / (tol + beta * EPS32 * np.abs(want))).max()), 1.0)
        assert gd.intact()
    assert gq.intact() and gr.intact() and _pad_ok(gi, B, N, ldg) and _pad_ok(gg, B, N, ldg)


def test_timepool_refusals(dev):
    lib = L.lib()
    g, out, idx = G(dev, 4096), G(dev, 4096), G(dev, 4096, torch.int32, -77)
    s = _st()
    for N in (63, 65):
        assert lib.yt8m_timepool_max_f32(g.p, 4, 2, N, 68, out.p, idx.p, 68, s) == -2
    assert lib.yt8m_timepool_max_f32(g.p, 4, 2, 64, 66, out.p, idx.p, 68, s) == -2
    assert lib.yt8m_timepool_max_f32(g.p, 4, 2, 64, 64, out.p, idx.p, 60, s) == -2
    assert lib.yt8m_timepool_max_f32(g.p, 0, 2, 64, 64, out.p, idx.p, 64, s) == -2
    assert lib.yt8m_timepool_max_f32(_p(g.t, 4), 4, 2, 64, 64, out.p, idx.p, 64, s) == -1
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert lib.yt8m_timepool_shiftmax_f32(g.p, 4, 2, 64, 1, i32(2), i32(6), out.p, idx.p, 8, s) == -2          # columns % 4
    assert lib.yt8m_timepool_shiftmax_f32(g.p, 4, 2, 64, 9, i32(*[1] * 9), i32(*[4] * 9), out.p, idx.p, 64, s) == -2
    assert lib.yt8m_timepool_shiftmax_f32(g.p, 4, 2, 12, 1, i32(2), i32(8), out.p, idx.p, 8, s) == -2          # ldz < fs N
    q = G(dev, 4096, torch.uint8, 0xA5)
    assert lib.yt8m_u8_cnn_pool_dw(q.p, g.p, idx.p, g.p, 8, 2, 4, 6, 8, 2, out.p, 0.0, s) == -2               # D % 4
    assert lib.yt8m_u8_cnn_pool_dw(q.p, g.p, idx.p, g.p, 8, 2, 4, 8, 8, 17, out.p, 0.0, s) == -2              # fs > 16
    assert lib.yt8m_u8_cnn_pool_dw(q.p, g.p, idx.p, g.p, 7, 2, 4, 8, 8, 2, out.p, 0.0, s) == -2               # ldg < N
    assert lib.yt8m_u8_cnn_pool_dw(q.p, g.p, idx.p, g.p, 8, 2, 4, 8, 8, 2, out.p, 0.5, s) == -1               # beta
    assert lib.yt8m_u8_cnn_pool_dw(_p(q.t, 1), g.p, idx.p, g.p, 8, 2, 4, 8, 8, 2, out.p, 0.0, s) == -1
    torch.cuda.synchronize()
    assert out.untouched() and idx.untouched()


if __name__ == "__main__":
    if sys.argv[1:] == ["--p128-child"]:
        _p128_child()
    else:
        sys.exit("run this module with pytest -m gpu")
