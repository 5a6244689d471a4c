"""-m gpu: every dispatch branch of the GEMM family (csrc/gemm_f32.hip, csrc/gemm_bf16.hip, csrc/gemm_x3.hip's launch, csrc/gemm_auto.hip)
through the C ABI with raw pointers -- base alignment, leading dimensions and workspace sizes are chosen exactly -- against an exact
reference.  tests/test_gpu_kernels.py, tests/test_gpu_x3.py and tests/test_gpu_h2.py keep the quick checks of the same entry points.

BRANCH_TABLE below is the reading of the dispatchers this module was written from: (entry point, condition as written in the .hip file,
kernel launched, case of this module that takes it).  tests/test_gemm_branch_table.py checks every kernel named here against the sources
and every __global__ of those sources against the kernel list recorded from a profiled run of this module
(tests/golden/gemm_kernels_seen.txt, profiles/gemm_branches_kernel_stats.csv): a new dispatch condition comes with its row.

Two data sets per case, both made on the host from a seed (_data):

  integer data, compared bit for bit.  A and B hold integers drawn uniformly from [-8, 8], bias and the pre-existing C integers from
  [-64, 64], stored as fp32.  Every partial sum of K <= 131072 such products stays below 2^24 in magnitude, so an fp32 accumulation in ANY
  order and under any split is exact: the expected result is the fp64 product (+ bias) (+ C) and the assertion is np.array_equal.  The
  same holds for the image forms: these integers are exact in bf16 and in f16, their lower planes are zero and the h2 scales are powers of
  two; each image case first asserts that the oracle of its form (oracle/x3_ref.py six_products / three_products) returns exactly the
  fp64 product on the case's data.  A dropped, doubled or misplaced term changes an integer, whatever the K.

  real data, held to a derived bound.  randn times a per-row power of two spread over six binades.  fp32 kernels: element (i, j) of the
  result is a sum of K products a_ik b_kj, each exact inside the MFMA's fused multiply-add, accumulated in fp32 in an order the kernel is
  free to choose, in S split-K parts that the fix-up kernel adds.  Whatever the order, a term passes through at most K - 1 + S additions,
  each of relative error <= u = 2^-24, so |fl(c_ij) - c_ij| <= ((1 + u)^(K + S) - 1) sum_k |a_ik| |b_kj| <= (K + S + 2) u (|A| |B|)_ij
  (the + 2 covers the second-order terms for K + S <= 5792; the two K = 16384 split-K cases lack 6 u of their 16 481 u, with errors below a
  tenth of the bound).  The bias and the accumulate additions add one
  rounding of the result each: + u |result| apiece (first order: where the pre-existing C cancels most of product + bias, the rounding of
  that intermediate is counted at the size of the smaller result; the closest any case comes is 0.984 of its bound, a K = 1 element of
  the 130 x 258 matrix case with bias and beta = 1 -- everything else stays below 0.15).  S = 1 where the entry point cannot split (yt8m_gemm_f32, _batched) and 96, the
  dispatcher's cap, for every grouped call.  The image forms keep the constants the project already holds them to, against the fp32
  kernel's own error e32 on the same operands (relative to max |C|): six products max(4 e32, 3e-7) (tests/test_gpu_x3.py
  test_gemm_x3_error_is_fp32_grade), three f16 products max(2 e32, 6e-7) (tests/test_gpu_h2.py test_gemm_h2_error_is_fp32_grade), one-plane
  bf16 2e-6 max|A| max|B| K against the fp64 product of the rounded operands (tests/test_gpu_kernels.py test_bf16_large_tile_gemm).
  Each real case prints its largest error next to its bound.

Margins (Mat).  Every operand sits inside a larger allocation.  Around C -- in front of it, behind it and in the ldc - N padding of every
row -- lies a sentinel bit pattern that must come back unchanged, compared as int32; with beta = 0 the inside of C starts as the
sentinel too, so an element the kernel never stores fails the comparison.  Around A and B (fp32 kernels), and around the fp32 sources the
chooser hands to the split passes (image forms), the padding of every row and the rows in front and behind are NaN: rows and columns
beyond the matrix may be read (fill_dma redirects them) but only ever feed outputs that are never stored.

Left out, each with its row below: arms behind process-wide `static` environment knobs (YT8M_GEMM_X3, YT8M_GEMM_H2, YT8M_GEMM_H2_MINK,
YT8M_GEMM_H2_PRICE, YT8M_BF16_K64, YT8M_X3_SLOTS; YT8M_X3_PIPE, YT8M_B1_PIPE and YT8M_X3_FUSED_COMBINE only set defaults whose arms are
reached through yt8m_x3_set_schedule / yt8m_x3_set_combine), resident weight images
(yt8m_wimg_lookup hits: tests/test_gpu_round5.py, tests/test_gpu_round6.py), dimensions >= 2^31 and tile counts >= 2^30 (beyond 1 GB per operand)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import yt8m_amd._lib as L

pytestmark = pytest.mark.gpu

BRANCH_TABLE = [
    # ---- gemm_f32.hip: yt8m_gemm_f32 / yt8m_gemm_f32_batched (gemm_launch) -----------------------------------------------------------
    ("yt8m_gemm_f32", "launch_by_layout: !transA && !transB", "gemm_f32_kernel<true, false>", "test_f32_path_layout_matrix[single-0-0-*]"),
    ("yt8m_gemm_f32", "launch_by_layout: transA && !transB", "gemm_f32_kernel<false, false>", "test_f32_path_layout_matrix[single-1-0-*]"),
    ("yt8m_gemm_f32", "launch_by_layout: !transA && transB", "gemm_f32_kernel<true, true>", "test_f32_path_layout_matrix[single-0-1-*]"),
    ("yt8m_gemm_f32", "launch_by_layout: transA && transB", "gemm_f32_kernel<false, true>", "test_f32_path_layout_matrix[single-1-1-*]"),
    ("yt8m_gemm_f32", "process_tile: dma = g.vecA && g.vecB (lda % 4 == 0, ldb % 4 == 0, A and B 16-byte aligned)", "gemm_f32_kernel",
     "test_f32_path_layout_matrix[*-aligned]: A_KC and B_KC each way"),
    ("yt8m_gemm_f32", "process_tile: else (guarded path); load_guarded: vec && inside -> float4, else element by element", "gemm_f32_kernel",
     "test_f32_path_layout_matrix[*-A+4B] (vecA = 0, vecB = 1), [*-Bodd] (vecA = 1, vecB = 0), [*-both]"),
    ("yt8m_gemm_f32", "fill_dma: gx >= X redirected to row X - 1 (KC) / chunk (X - 1) & ~3 (XC, X % 4 != 0 included)", "gemm_f32_kernel",
     "test_f32_path_layout_matrix[*-aligned]: (M, N) = (1, 1), (127, 129), (129, 127), (130, 258), (3, 260) with NaN padding"),
    ("yt8m_gemm_f32", "fill_step: (kt + 1) * BK <= K, else the guarded K tail", "gemm_f32_kernel",
     "test_f32_path_layout_matrix: K = 16, 32, 48, 64 against 1, 15, 17, 31, 33, 47, 49, 65"),
    ("yt8m_gemm_f32", "mainloop prologue: kb + 2 < ke || (kb + 1 < ke && ke * BK <= K) -> vmcnt(4), else vmcnt(0)", "gemm_f32_kernel",
     "test_f32_path_layout_matrix: K = 48 / 33 / 32 (vmcnt(4): three steps / tail third / two whole steps); K = 1, 15, 16, 17, 31 (drain)"),
    ("yt8m_gemm_f32", "mainloop: kt + 2 < ke && (kt + 3) * BK <= K -> vmcnt(4), else vmcnt(0)", "gemm_f32_kernel",
     "test_f32_path_layout_matrix: K = 48, 64 (whole step kt + 2), 33, 47, 49, 65 (step kt + 2 is the tail), 32 and below (nothing to issue)"),
    ("yt8m_gemm_f32", "epilogue: col < N, row < M, bias NULL / given, accumulate", "gemm_f32_kernel",
     "test_f32_path_layout_matrix (bias on odd M + K, beta = 1 on K % 3 == 0)"),
    ("yt8m_gemm_f32", "tile_coords: tiles_m <= 16 (plain M-fastest order)", "gemm_f32_kernel", "test_f32_path_layout_matrix (1 .. 2 x 3 tiles)"),
    ("yt8m_gemm_f32", "M == 0 || N == 0 || batch == 0: YT8M_OK without a launch", "(none)", "test_batched[0-*], test_refusals_f32 (M = 0 with NULL operands)"),
    ("yt8m_gemm_f32", "fill_problem: negative dimension / beta not 0, 1 / ld too small / NULL operand", "(none)", "test_refusals_f32"),
    ("yt8m_gemm_f32", "fill_problem: dimension >= 2^31; gemm_launch: nwg >= 2^31", "(none)", "left out: no operand under 1 GB reaches them"),
    ("yt8m_gemm_f32_batched", "vecA = vecA && strideA % 4 == 0; vecB likewise", "gemm_f32_kernel<true, false> gemm_f32_kernel<false, false> "
     "gemm_f32_kernel<true, true> gemm_f32_kernel<false, true>", "test_batched[*-0] and [*-4] (vector loads) against [*-1] (strides % 4 != 0)"),
    ("yt8m_gemm_f32_batched", "blockIdx.y * strideA / strideB / strideC", "gemm_f32_kernel", "test_batched[3-*]: sentinel between the C matrices"),
    ("yt8m_gemm_f32_batched", "batch >= 0 && batch <= 65535 else YT8M_E_SHAPE", "(none)", "test_batched_refusals: -1, 65536"),
    # ---- gemm_f32.hip: yt8m_gemm_f32_grouped (grouped_launch) ------------------------------------------------------------------------
    ("yt8m_gemm_f32_grouped", "launch_by_layout, four layouts", "gemm_grouped_kernel<true, false, false, false> gemm_grouped_kernel<false, false, false, false> "
     "gemm_grouped_kernel<true, true, false, false> gemm_grouped_kernel<false, true, false, false>",
     "test_f32_path_layout_matrix[grouped-*], test_vepi_epilogue[2049] / [2064] (transA && !transB above the threshold)"),
    ("yt8m_gemm_f32_grouped", "transA && !transB && kmax <= 2048", "gemm_grouped_kernel<false, false, false, true>",
     "test_vepi_epilogue[2032], [2048]; test_f32_path_layout_matrix[grouped-1-0-*]; test_vepi_mixed_k_group (512 + 2048)"),
    ("yt8m_gemm_f32_grouped", "kmax over the group: one K above 2048 takes the plain kernel for all", "gemm_grouped_kernel<false, false, false, false>",
     "test_vepi_mixed_k_group (512 + 4096), test_vepi_epilogue[2049]"),
    ("yt8m_gemm_f32_grouped", "VEPI in kernel: (ldc & 3) == 0 && C, bias 16-byte aligned, else the dword epilogue", "gemm_grouped_kernel<false, false, false, true>",
     "test_vepi_epilogue: ldc = N4 / N4 + 1, C and bias at 0 / 4 bytes, bias NULL"),
    ("yt8m_gemm_f32_grouped", "VEPI in kernel: col + 3 < N float4, else the partial last column group", "gemm_grouped_kernel<false, false, false, true>",
     "test_vepi_epilogue: N = 256 against 258, 259"),
    ("yt8m_gemm_f32_grouped", "T < SLOTS: everything is remainder (P = 768, full_rounds = 0)", "gemm_grouped_kernel",
     "test_rounds[*-767], test_splitk, test_groups"),
    ("yt8m_gemm_f32_grouped", "T >= SLOTS: full_rounds = T / 768, rem = T % 768 (0 and > 0)", "gemm_grouped_kernel",
     "test_rounds[*-768] (rem = 0), [*-769] (rem = 1), [*-band] (782 tiles, rem = 14)"),
    ("yt8m_gemm_f32_grouped", "tile_coords: tiles_m > 16, tiles_m % 16 != 0 (short last band)", "gemm_grouped_kernel", "test_rounds[*-band]: 17 x 46 tiles"),
    ("yt8m_gemm_f32_grouped", "Smax = min_nk / 8, capped at 96", "gemm_grouped_kernel splitk_fixup_kernel",
     "test_splitk: K = 128 (1), 136 (1, odd nk), 256 and 272 (2), 1000 (7), 4101 (Smax = 32: S = 31), 16384 on 1 and 2 tiles (min_nk / 8 = 128, capped: "
     "S = 95 where the cost model alone takes 126); every S measured from the parts written to a sentinel-filled workspace"),
    ("yt8m_gemm_f32_grouped", "workspace NULL: ws_items = 0 -> Smax = 0 -> S = 1", "gemm_grouped_kernel", "test_splitk[*] ws = none; test_vepi_epilogue"),
    ("yt8m_gemm_f32_grouped", "rem * Smax > ws_items: Smax = ws_items / rem (1 for one part short of rem * 2, 0 for a tiny one)", "gemm_grouped_kernel",
     "test_splitk[*] ws = short, tiny (both bitwise equal to ws = none)"),
    ("yt8m_gemm_f32_grouped", "cost model picks S <= Smax; ws of exactly rem * S parts", "gemm_grouped_kernel splitk_fixup_kernel",
     "test_splitk[*] ws = exact (bitwise equal to ws = full, sentinel behind the declared bytes)"),
    ("yt8m_gemm_f32_grouped", "kb = nk * part / nparts, ke = nk * (part + 1) / nparts (uneven), the tail step in the last part only", "gemm_grouped_kernel",
     "test_splitk: K = 1000 (nk = 63 over 7 parts), 4101 (nk = 257, tail), 136 / 272 (S = 1 / 2 with a tail)"),
    ("yt8m_gemm_f32_grouped", "process_tile: ws != NULL parks raw accumulators; G.S > 1 launches the fix-up", "splitk_fixup_kernel",
     "test_splitk: bias, beta = 1, ragged M (130, 100), N % 4 != 0 (258, 90, 259); same call twice bitwise equal"),
    ("yt8m_gemm_f32_grouped", "q.M == 0 || q.N == 0: continue (tile_base compacted); find_problem at each tile_base", "gemm_grouped_kernel",
     "test_groups[*-full], [*-M0] (second problem empty), [*-N0] (last problem empty)"),
    ("yt8m_gemm_f32_grouped", "G.nprob == 0: YT8M_OK without a launch", "(none)", "test_groups_all_empty"),
    ("yt8m_gemm_f32_grouped", "nprob 1..4 && probs; fill_problem's refusals per problem", "(none)", "test_refusals_f32"),
    ("yt8m_gemm_f32_grouped", "T >= 2^30", "(none)", "left out: no operand under 1 GB reaches it"),
    # ---- gemm_bf16.hip / yt8m_gemm_bf16_nt_grouped -----------------------------------------------------------------------------------
    ("yt8m_gemm_bf16_nt_grouped", "simple && gemm_bf16_big_ok: T >= min_tiles (256 unless YT8M_BF16_BIG_MIN)", "gemm_bf16_k64_kernel",
     "test_bf16_tile_floor[256] (16 x 16 tiles of 256 x 256 at K = 32)"),
    ("yt8m_gemm_bf16_nt_grouped", "T < min_tiles: grouped_launch(0, 1, bf16 = 1)", "gemm_grouped_kernel<true, true, true, false>", "test_bf16_tile_floor[255] (15 x 17 tiles)"),
    ("yt8m_gemm_bf16_nt_grouped", "gemm_bf16_big_ok: K < 32 || K % 2 || lda % 8 || ldb % 8 -> small tiles", "gemm_grouped_kernel<true, true, true, false>",
     "test_bf16_small_floor: K = 30; lda = K + 2; ldb = K + 2; K = 510 with lda = K"),
    ("yt8m_gemm_bf16_nt_grouped", "gemm_bf16_big_ok: A | B not 16-byte aligned -> small tiles", "gemm_grouped_kernel<true, true, true, false>",
     "test_bf16_small_floor: A 8 bytes off"),
    ("yt8m_gemm_bf16_nt_grouped", "big kernel: whole steps, the guarded K tail (K % 64 != 0), ragged M and N, float4 / scalar epilogue", "gemm_bf16_k64_kernel",
     "test_bf16_small_floor: K = 32, 34, 512, 1024, 4608; (257, 255), (256, 257); ldc = N and N4 + 4; bias; beta 0 / 1"),
    ("yt8m_gemm_bf16_nt_grouped", "gemm_bf16_big_launch: S = 256 / rem capped by min_nk / 16, by 8, by a NULL and by a short workspace", "gemm_bf16_k64_kernel bf16_fixup_kernel",
     "test_bf16_small_floor: K = 512 (S = 1), 1024 (2), 4608 (8 = the cap; min_nk / 16 = 9); ws none / short (one part short of rem * 2) / full"),
    ("yt8m_gemm_bf16_nt_grouped", "gemm_bf16_big_ok / gemm_bf16_big_launch: q.M == 0 || q.N == 0: continue", "gemm_bf16_k64_kernel bf16_fixup_kernel",
     "test_empty_problem_in_a_large_tile_bf16_group"),
    ("yt8m_gemm_bf16_nt_grouped", "YT8M_BF16_K64 = 0 (static)", "gemm_bf16_big_kernel", "left out: process-wide static knob; tools/build_variant.sh A/B only"),
    ("yt8m_gemm_bf16_nt_grouped", "simple == false: grouped_launch states the refusal (odd K, NULL operand, nprob)", "(none)", "test_refusals_bf16"),
    # ---- gemm_x3.hip: x3_launch ------------------------------------------------------------------------------------------------------
    ("yt8m_gemm_x3_nt_grouped", "xpiped (yt8m_x3_set_schedule 0 / 1)", "gemm_x3q_kernel<3>", "test_x3_launch_parts, test_auto_chooser_both_sides, test_auto_roles (the default schedule)"),
    ("yt8m_gemm_x3_nt_grouped", "!xpiped (yt8m_x3_set_schedule(2))", "gemm_x3_kernel<3>", "test_x3_launch_parts: bitwise equal to the default schedule"),
    ("yt8m_gemm_x3_nt_grouped", "S: c <= 16 while KB / c >= 8 and the parts fit the workspace; workspace NULL: S = 1", "gemm_x3q_kernel<3> x3_fixup_kernel",
     "test_x3_launch_parts: K = 4096 on one tile (16 parts), 1024 (8), 100 (1); ws none / one part / full"),
    ("yt8m_gemm_x3_nt_grouped", "fix > 0 && !G.cnt (yt8m_x3_set_combine(2), and 0 unless YT8M_X3_FUSED_COMBINE = 1): the separate pass", "x3_fixup_kernel",
     "test_x3_launch_parts (combine 2)"),
    ("yt8m_gemm_x3_nt_grouped", "G.cnt = g_cnt.take(fix) (yt8m_x3_set_combine(1)): x_epilogue's arrival counter, the last part of a tile combines inside the launch",
     "gemm_x3q_kernel<3> gemm_x3_kernel<3>", "test_x3_launch_parts (combine 1, both schedules: bitwise equal to the separate pass, integer data exact)"),
    ("yt8m_gemm_x3_nt_grouped", "q.M == 0 || q.N == 0: continue (before the operand checks)", "gemm_x3q_kernel<3>", "test_empty_problem_in_an_image_group"),
    ("yt8m_gemm_x3_nt_grouped", "YT8M_X3_PIPE / YT8M_B1_PIPE / YT8M_X3_SLOTS / YT8M_X3_FUSED_COMBINE (static)", "gemm_x3_kernel", "left out: process-wide static defaults; the arms they choose between are "
     "reached per thread through yt8m_x3_set_schedule and yt8m_x3_set_combine (YT8M_X3_SLOTS, a tuning aid, has no setter)"),
    ("yt8m_gemm_x3_nt_grouped", "x3_launch's refusals: K < 1, beta, NULL, image alignment, K-block stride, nprob", "(none)", "test_refusals_images"),
    ("yt8m_gemm_h2_nt_grouped", "PA == 2", "gemm_h2q_kernel<2>", "test_auto_roles (declared h2 products), test_auto_absmax_words"),
    ("yt8m_gemm_h2_nt_grouped", "a scaled product needs N % 4 == 0", "(none)", "test_refusals_images"),
    ("yt8m_gemm_h1x2_nt_ex", "PA == 4", "gemm_h2q_kernel<1>", "left out: its A operand is a uint8 frame image; tests/test_gpu_h2.py::test_u8_projection_and_weight_gradient_on_two_f16_products"),
    ("yt8m_gemm_x1x3_nt", "PA == 1", "gemm_x3q_kernel<1> gemm_x3_kernel<1>", "left out: its A operand is a uint8 frame image; tests/test_gpu_x3.py::test_u8_projection_on_the_x3_kernel"),
    # ---- gemm_auto.hip ---------------------------------------------------------------------------------------------------------------
    ("yt8m_gemm_auto_grouped", "x3_allowed / image_form_pays true", "x3_split_kernel<3> gemm_x3q_kernel<3>", "test_auto_chooser_both_sides (256^3 pays: used_x3 = 1)"),
    ("yt8m_gemm_auto_grouped", "image_form_pays false", "gemm_grouped_kernel", "test_auto_chooser_both_sides (257 x 255 x 256, 130 x 258 x 65: used_x3 = 0)"),
    ("yt8m_gemm_auto_grouped", "h2_role: transA_flags & YT8M_GEMM_ROLE_H2", "h2_absmax_kernel x3_split_kernel<2> gemm_h2q_kernel<2>", "test_auto_roles[h2-notrans], [h2-trans]"),
    ("yt8m_gemm_auto_grouped", "h2_role: ROLE_DW && transA && !transB", "gemm_h2q_kernel<2>", "test_auto_roles[dw-tb0] (h2) against [dw-tb1] (six products)"),
    ("yt8m_gemm_auto_grouped", "h2_role: K < 512", "gemm_x3q_kernel<3>", "test_auto_roles[dw-k511] against [dw-k512]"),
    ("yt8m_gemm_auto_grouped", "h2 && N % 4 == 0, else the six-product form", "gemm_x3q_kernel<3>", "test_auto_roles[dw-n518] against [dw-n516]"),
    ("yt8m_gemm_auto_grouped", "image_of: the same operand of two problems is split once", "x3_split_kernel<3>", "test_auto_shared_operand[full]"),
    ("yt8m_gemm_auto_grouped", "image_of: off + bytes > image_scratch_bytes for the second problem: imgs.resize(nimg); off = mark", "gemm_x3q_kernel<3> gemm_grouped_kernel",
     "test_auto_shared_operand[short] (used_x3 = 1: the second problem on the fp32 kernel), "
     "test_auto_rollback_frees_the_scratch_of_a_problem_that_does_not_fit (used_x3 = 0b1101: the third problem needs the room given back, the fourth shares the rolled-back A)"),
    ("yt8m_gemm_auto_grouped", "image_of: image_scratch NULL", "gemm_grouped_kernel", "test_auto_shared_operand[none] (used_x3 = 0)"),
    ("yt8m_gemm_auto_grouped", "ph / px / p32 launched in fours", "gemm_h2q_kernel<2> gemm_x3q_kernel<3> gemm_grouped_kernel",
     "test_auto_chunks_of_four[h2-5], [h2-9], [x3-5], [x3-9], [f32-9]"),
    ("yt8m_gemm_auto_grouped_ex", "absmaxA[i] / absmaxB[i] given: no memset + yt8m_h2_absmax for that operand", "x3_split_kernel<2> gemm_h2q_kernel<2>",
     "test_auto_absmax_words: the true maximum, twice the true maximum; the scratch word slots stay untouched (test_auto_roles: filled when measured)"),
    ("yt8m_gemm_auto_grouped", "nprob 1..64, transA flags, transB 0 / 1, image scratch 256-byte aligned", "(none)", "test_refusals_auto"),
    ("yt8m_gemm_auto_grouped", "YT8M_GEMM_X3 / YT8M_GEMM_H2 / YT8M_GEMM_H2_MINK / YT8M_GEMM_H2_PRICE (static)", "(none)", "left out: process-wide static knobs"),
    ("yt8m_gemm_auto_grouped", "resident(): yt8m_wimg_lookup hit (a weight with a resident image)", "(none)", "left out: resident weight images are out of scope here (tests/test_gpu_round5.py and tests/test_gpu_round6.py register them)"),
    ("yt8m_gemm_auto_grouped", "x3_allowed: max(M, N, K) >= 64 * 65535", "(none)", "left out: over 1 GB per operand at any K the form pays for"),
]

U = 2.0 ** -24
SENT = 0x7FC5A5A5                                   # a quiet NaN with a payload: the sentinel around (and, at beta = 0, inside) C
NAN32 = 0x7FC00000
NAN16 = 0x7FC0                                      # bf16 NaN
E_BADARG, E_SHAPE = -1, -2
ROLE_DW, ROLE_H2 = 0x100, 0x200
F_GEMM, F_X3, F_H2 = 0, 7, 12                        # csrc/common.h enum Family


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r4(n):
    return (n + 3) // 4 * 4


class Mat:
    """batch matrices [rows, cols] with leading dimension ld and batch stride `stride` (elements), `shift` elements off a 256-byte
    aligned address, inside an allocation filled with a bit pattern: two rows (at least 64 elements) in front and behind, the ld - cols
    padding of every row, the gap between batch items."""

    def __init__(self, dev, rows, cols, ld, shift=0, fill=SENT, dtype=torch.float32, batch=1, stride=None):
        self.rows, self.cols, self.ld, self.batch = int(rows), int(cols), int(ld), int(batch)
        self.stride = int(stride) if stride is not None else self.rows * self.ld
        margin = (max(64, 2 * self.ld) + 63) // 64 * 64
        self.front = margin + shift
        self.n = max(self.batch, 1) * max(self.stride, self.rows * self.ld)
        self.fill = fill
        self.ibuf = torch.full((self.front + self.n + margin,), fill, dtype=torch.int32 if dtype == torch.float32 else torch.int16, device=dev)
        self.buf = self.ibuf.view(dtype)
        self.m = self.buf.as_strided((self.batch, self.rows, self.cols), (self.stride, self.ld, 1), self.front)

    def put(self, data):
        t = torch.from_numpy(np.array(data)) if isinstance(data, np.ndarray) else data      # (a copy: the shared inputs are read-only)
        self.m.copy_(t.reshape(self.batch, self.rows, self.cols).to(self.buf.dtype))
        return self

    @property
    def p(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.front * self.buf.element_size())

    @property
    def addr(self):
        return self.buf.data_ptr() + self.front * self.buf.element_size()

    def read(self):
        """-> (values [batch, rows, cols] as numpy fp32 (squeezed when batch == 1), margins intact as bool)."""
        if self.ibuf.numel() <= (1 << 22):
            h = self.ibuf.cpu().numpy()
            mask = np.ones(h.shape, dtype=bool)
            view = np.lib.stride_tricks.as_strided(mask[self.front:], (self.batch, self.rows, self.cols), (self.stride, self.ld, 1))
            view[...] = False
            vals = np.lib.stride_tricks.as_strided(h[self.front:], (self.batch, self.rows, self.cols), (self.stride * 4, self.ld * 4, 4)).copy()
            ok = bool((h[mask] == self.fill).all())
        else:                                                                      # large C (one matrix): compare on the device
            assert self.batch == 1
            body = self.ibuf[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)
            ok = bool((self.ibuf[:self.front] == self.fill).all() & (self.ibuf[self.front + self.rows * self.ld:] == self.fill).all()
                      & (body[:, self.cols:] == self.fill).all())
            vals = body[:, :self.cols].contiguous().cpu().numpy().reshape(1, self.rows, self.cols)
        vals = vals.view(np.float32)
        return (vals[0] if self.batch == 1 else vals), ok


class Vec(Mat):
    """A bias: n floats, `shift` floats off 16-byte alignment, NaN around it."""

    def __init__(self, dev, data, shift=0):
        super().__init__(dev, 1, len(data), len(data), shift, NAN32)
        self.put(np.asarray(data, dtype=np.float32))


def _seed(*k):
    s = 17
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _ref64(A, B):
    """fp64 product on the host; products above 2e9 multiply-adds on the device's fp64 BLAS (torch.matmul on doubles: independent of the
    kernels under test, and exact like any other summation on the integer data)."""
    if A.shape[0] * A.shape[1] * B.shape[1] <= 2e9 or not torch.cuda.is_available():
        return A.astype(np.float64) @ B.astype(np.float64)
    return (torch.from_numpy(A).cuda().double() @ torch.from_numpy(B).cuda().double()).cpu().numpy()


def _make(kind, M, N, K, seed=0):
    rs = np.random.RandomState(_seed(M, N, K, seed, kind == "int"))
    if kind == "int":
        A = rs.randint(-8, 9, size=(M, K)).astype(np.float32)
        B = rs.randint(-8, 9, size=(K, N)).astype(np.float32)
        bias = rs.randint(-64, 65, size=N).astype(np.float32)
        C0 = rs.randint(-64, 65, size=(M, N)).astype(np.float32)
    else:
        A = (rs.randn(M, K) * 2.0 ** ((np.arange(M) * 5) % 6 - 3)[:, None]).astype(np.float32)
        B = (rs.randn(K, N) * 2.0 ** ((np.arange(K) * 7) % 6 - 3)[:, None]).astype(np.float32)
        bias = rs.randn(N).astype(np.float32)
        C0 = rs.randn(M, N).astype(np.float32)
    d = dict(kind=kind, M=M, N=N, K=K, A=A, B=B, bias=bias, C0=C0, ref=_ref64(A, B))
    d["mag"] = None if kind == "int" else _ref64(np.abs(A), np.abs(B))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)                                                # shared among the tests: never changed
    return d


@functools.lru_cache(maxsize=None)
def _data(kind, M, N, K, seed=0):
    """The case's inputs and its fp64 product, computed once and shared (small cases only: the large ones use _make and let go)."""
    return _make(kind, M, N, K, seed)


def _expected(d, bias, beta):
    e = d["ref"]
    if bias:
        e = e + d["bias"].astype(np.float64)
    if beta:
        e = e + d["C0"].astype(np.float64)
    return e


def _judge(what, d, got, ok, bias, beta, S, worst=None):
    """Integer data: array_equal.  Real data: the derived bound of the module docstring, element by element."""
    assert ok, "%s: the sentinel around C changed" % what
    exp = _expected(d, bias, beta)
    if d["kind"] == "int":
        assert np.array_equal(got.astype(np.float64), exp), "%s: integer data differ from the fp64 product at %d elements (first %s)" % (
            what, int((got != exp).sum()), np.argwhere(got != exp)[:4].tolist())
        return
    bound = (d["K"] + S + 2) * U * d["mag"] + (int(bool(bias)) + int(bool(beta))) * U * np.abs(exp)
    err = np.abs(got.astype(np.float64) - exp)
    assert not np.isnan(got).any(), "%s: NaN in the result (padding reached a stored element)" % what
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    if worst is not None:
        worst.append((ratio, what, float(err.max()) if err.size else 0.0, float(bound.max()) if bound.size else 0.0))
    else:
        print("%s: max err %.3g, max bound %.3g, worst err / bound %.3g" % (what, float(err.max()) if err.size else 0.0,
                                                                         float(bound.max()) if bound.size else 0.0, ratio))
    assert ratio <= 1.0, "%s: error %.6g of its bound" % (what, ratio)


def _summary(title, worst):
    if worst:
        r = max(worst)
        print("%s: %d real-data cases, worst err / bound %.3g at %s (err %.3g, bound %.3g)" % (title, len(worst), r[0], r[1], r[2], r[3]))


def _operands(dev, d, tA, tB, shiftA=0, oddB=0, lda=None, ldb=None, fill=NAN32):
    """A and B of the case as stored for the layout: A [M, K] or [K, M], B [K, N] or [N, K], NaN around them."""
    sa = d["A"].T if tA else d["A"]
    sb = d["B"].T if tB else d["B"]
    lda = lda if lda is not None else _r4(sa.shape[1]) + 4
    ldb = ldb if ldb is not None else _r4(sb.shape[1]) + (5 if oddB else 4)
    a = Mat(dev, sa.shape[0], sa.shape[1], lda, shiftA, fill).put(sa)
    b = Mat(dev, sb.shape[0], sb.shape[1], ldb, 0, fill).put(sb)
    return a, b


def _cmat(dev, d, ldc, beta, shift=0):
    c = Mat(dev, d["M"], d["N"], ldc, shift, SENT)
    if beta:
        c.put(d["C0"])
    return c


def _problems(items):
    arr = (L.GemmProblem * max(len(items), 1))()
    for i, (M, N, K, a, lda, b, ldb, c, ldc, bias, beta) in enumerate(items):
        arr[i].M, arr[i].N, arr[i].K = M, N, K
        arr[i].A, arr[i].lda, arr[i].B, arr[i].ldb, arr[i].C, arr[i].ldc = a, lda, b, ldb, c, ldc
        arr[i].bias, arr[i].beta = bias, beta
    return arr


def _prob(d, a, b, c, bias, beta):
    return (d["M"], d["N"], d["K"], a.addr, a.ld, b.addr, b.ld, c.addr, c.ld, bias.addr if bias is not None else None, float(beta))


_WS = {}
WS_GUARD = 16384                                      # ints of sentinel behind the declared end of a workspace


def _workspace(dev, nbytes=None):
    """(pointer, bytes, check): the split-K workspace, `nbytes` of it declared (None: all of yt8m_gemm_workspace_bytes()); check() is
    false if anything was written behind the declared end."""
    full = int(L.lib().yt8m_gemm_workspace_bytes())
    if "buf" not in _WS:
        _WS["buf"] = torch.zeros((full // 4 + WS_GUARD,), dtype=torch.int32, device=dev)
    buf = _WS["buf"]
    nbytes = full if nbytes is None else int(nbytes)
    assert 0 <= nbytes <= full and nbytes % 4 == 0
    guard = buf[nbytes // 4:nbytes // 4 + WS_GUARD]
    guard.fill_(SENT)
    return ctypes.c_void_p(buf.data_ptr()), nbytes, lambda: bool((guard == SENT).all())


PART = 128 * 128 * 4                                  # bytes of one split-K part of the fp32 kernel


def _pick_s(T, nks, ws_items):
    """grouped_launch's split factor, restated: only used to size the `exact` workspace and to say which S a case pins; the bitwise
    comparisons between workspaces (exact == full, short == tiny == none) are what holds the library to it."""
    rem = T if T < 768 else T % 768
    if rem == 0:
        return 1
    smax = min(min(nks) // 8, 96)
    if rem * smax > ws_items:
        smax = ws_items // rem
    s, best = 1, 1e30
    for c in range(1, smax + 1):
        rounds = (rem * c + 767) // 768
        cost = rounds * (max(nks) / c + 8.0) + (2.0 if c > 1 else 0.0)
        if cost < best * 0.98:
            best, s = cost, c
    return s


def _tiles(M, N, t=128):
    return ((M + t - 1) // t) * ((N + t - 1) // t)


# ================================================================================================================================
# path x layout matrix of yt8m_gemm_f32 and of yt8m_gemm_f32_grouped with a workspace
LAYOUTS = [(0, 0), (1, 0), (0, 1), (1, 1)]
STATES = {"aligned": (0, 0), "A+4B": (1, 0), "Bodd": (0, 1), "both": (1, 1)}        # (A off by 4 bytes, B with an odd ld)
MATRIX_K = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65]
MATRIX_MN = [(1, 1), (127, 129), (128, 128), (129, 127), (130, 258), (3, 260)]


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("tA,tB", LAYOUTS)
@pytest.mark.parametrize("entry", ["single", "grouped"])
def test_f32_path_layout_matrix(dev, entry, tA, tB, state):
    lib = L.lib()
    shiftA, oddB = STATES[state]
    ws, wsb, ws_ok = _workspace(dev)
    worst = []
    for (M, N) in MATRIX_MN:
        for K in MATRIX_K:
            use_bias, beta = (M + K) % 2 == 1, 1.0 if K % 3 == 0 else 0.0
            for kind in ("int", "real"):
                d = _data(kind, M, N, K)
                a, b = _operands(dev, d, tA, tB, shiftA, oddB)
                c = _cmat(dev, d, _r4(N) + (4 if K % 2 else 1), beta)
                bias = Vec(dev, d["bias"]) if use_bias else None
                if entry == "single":
                    rc = lib.yt8m_gemm_f32(tA, tB, M, N, K, a.p, a.ld, b.p, b.ld, c.p, c.ld, bias.p if bias else None, beta, _st())
                else:
                    rc = lib.yt8m_gemm_f32_grouped(tA, tB, 1, _problems([_prob(d, a, b, c, bias, beta)]), ws, wsb, _st())
                L.check(rc)
                got, ok = c.read()
                _judge("%s tA=%d tB=%d %s M=%d N=%d K=%d %s" % (entry, tA, tB, state, M, N, K, kind), d, got, ok, use_bias, beta,
                       1 if entry == "single" else 96, worst)
    assert ws_ok()
    _summary("f32 matrix %s tA=%d tB=%d %s" % (entry, tA, tB, state), worst)


# ================================================================================================================================
# the float4 epilogue of the grouped transA && !transB kernel (kmax <= 2048), its in-kernel fallback and its partial last column group
@pytest.mark.parametrize("K", [2032, 2048, 2049, 2064])
def test_vepi_epilogue(dev, K):
    """Workspace NULL, so S = 1 and the kernel's own epilogue stores C (with a workspace these 6 tiles are split along K and the fix-up
    kernel stores: test_splitk).  K = 2049 and 2064 take the plain kernel: the same cases must hold on it."""
    lib = L.lib()
    M, worst = 130, []
    for N in (256, 258, 259):
        for kind in ("int", "real"):
            d = _data(kind, M, N, K)
            a, b = _operands(dev, d, 1, 0)
            for ldc in (_r4(N), _r4(N) + 1):
                for cshift in (0, 1):
                    for bmode in ("none", 0, 1):
                        for beta in (0.0, 1.0):
                            c = _cmat(dev, d, ldc, beta, cshift)
                            bias = None if bmode == "none" else Vec(dev, d["bias"], bmode)
                            L.check(lib.yt8m_gemm_f32_grouped(1, 0, 1, _problems([_prob(d, a, b, c, bias, beta)]), None, 0, _st()))
                            got, ok = c.read()
                            _judge("vepi K=%d N=%d ldc=%d C+%d bias=%s beta=%g %s" % (K, N, ldc, 4 * cshift, bmode, beta, kind), d, got, ok,
                                   bias is not None, beta, 1, worst)
    _summary("vepi K=%d" % K, worst)


@pytest.mark.parametrize("K2", [2048, 4096])
def test_vepi_mixed_k_group(dev, K2):
    """A group of two with K = 512 and K2: kmax decides for the whole group (2048: the float4 epilogue, 4096: the plain kernel)."""
    lib = L.lib()
    for kind in ("int", "real"):
        ds = [_data(kind, 130, 258, 512), _data(kind, 129, 256, K2)]
        ops_, cs, items = [], [], []
        for i, d in enumerate(ds):
            a, b = _operands(dev, d, 1, 0)
            c = _cmat(dev, d, _r4(d["N"]), float(i))
            bias = Vec(dev, d["bias"])
            ops_.append((a, b, bias))
            cs.append(c)
            items.append(_prob(d, a, b, c, bias, float(i)))
        L.check(lib.yt8m_gemm_f32_grouped(1, 0, 2, _problems(items), None, 0, _st()))
        for i, (d, c) in enumerate(zip(ds, cs)):
            got, ok = c.read()
            _judge("mixed K group 512 + %d problem %d %s" % (K2, i, kind), d, got, ok, True, float(i), 1)


# ================================================================================================================================
# split-K of the remainder tiles
SPLIT_MN = [(100, 90), (129, 127), (130, 258), (130, 259)]                     # 1, 2, 6, 6 tiles; ragged M; N % 4 = 2, 3, 2, 3
SPLIT_K = [128, 136, 256, 272, 1000, 4096 + 5]
SPLIT_LONG = [(100, 90, 16384), (129, 127, 16384)]     # min_nk / 8 = 128: the cap of 96 binds (without it the cost model takes 126 parts)


def _parts_written(probe):
    """How many 128 x 128 split-K parts of a sentinel-filled workspace a launch wrote (a part is stored whole): rem * S, measured."""
    return int((probe.view(-1, PART // 4)[:, 0] != SENT).sum())


@pytest.mark.parametrize("tA,tB", LAYOUTS)
def test_splitk(dev, tA, tB):
    """S is measured, not only restated: the full workspace starts as the sentinel and the number of parts the launch wrote must be
    rem * S for the S of _pick_s (0 parts at S = 1)."""
    lib = L.lib()
    full_items = int(lib.yt8m_gemm_workspace_bytes()) // PART
    worst, pinned = [], {}
    for (M, N, K) in [(M, N, K) for (M, N) in SPLIT_MN for K in SPLIT_K] + SPLIT_LONG:
        T = _tiles(M, N)
        nk = (K + 15) // 16
        s_full = _pick_s(T, [nk], full_items)
        use_bias, beta = (K // 8) % 2 == 1, 1.0 if K % 16 == 0 else 0.0
        for kind in ("int", "real"):
            d = _data(kind, M, N, K)
            a, b = _operands(dev, d, tA, tB)
            bias = Vec(dev, d["bias"]) if use_bias else None
            res = {}
            for name, nbytes in (("none", None), ("tiny", PART // 2), ("short", (2 * T - 1) * PART), ("exact", T * s_full * PART),
                                 ("full", full_items * PART), ("again", full_items * PART)):
                probe = None
                if name == "none":
                    ws, wsb, ws_ok = None, 0, lambda: True
                else:
                    ws, wsb, ws_ok = _workspace(dev, nbytes)
                if name == "full":
                    probe = _WS["buf"][:T * (s_full + 2) * (PART // 4)]
                    probe.fill_(SENT)
                c = _cmat(dev, d, N + 3, beta)
                L.check(lib.yt8m_gemm_f32_grouped(tA, tB, 1, _problems([_prob(d, a, b, c, bias, beta)]), ws, wsb, _st()))
                got, ok = c.read()
                assert ws_ok(), "split-K parts written behind the declared %d workspace bytes (%s)" % (wsb, name)
                if probe is not None:
                    wrote = _parts_written(probe)
                    assert wrote == (T * s_full if s_full > 1 else 0), "M=%d N=%d K=%d: the launch wrote %d parts, %d tiles x S = %d expected" % (
                        M, N, K, wrote, T, s_full)
                    pinned[(T, K)] = wrote // T if wrote else 1
                _judge("splitk tA=%d tB=%d M=%d N=%d K=%d ws=%s (S=%d with a full one) %s" % (tA, tB, M, N, K, name, s_full, kind), d, got, ok,
                       use_bias, beta, s_full if name in ("exact", "full", "again") else 1, worst)
                res[name] = got
            # S = 1 whichever way the workspace is too small; the same S, so the same bits, from exactly enough and from all of it
            assert np.array_equal(res["tiny"], res["none"]) and np.array_equal(res["short"], res["none"])
            assert np.array_equal(res["exact"], res["full"]) and np.array_equal(res["again"], res["full"])
    print("split factors measured from the workspace (tiles, K) -> S: %s" % sorted(pinned.items()))
    assert pinned[(1, 128)] == 1 and pinned[(1, 256)] == 2 and pinned[(6, 1000)] == 7 and pinned[(6, 4101)] == 31
    assert pinned[(1, 16384)] == 95 and pinned[(2, 16384)] == 95            # Smax = min(1024 / 8, 96): the cap, one below it by the 2 % rule
    _summary("splitk tA=%d tB=%d" % (tA, tB), worst)


# ================================================================================================================================
# whole-tile rounds of 768, the remainder behind them, the banded tile order
ROUNDS = {"767": (128, 128 * 767), "768": (128, 128 * 768), "769": (128, 128 * 769), "band": (128 * 17 - 5, 128 * 46)}


@pytest.mark.parametrize("which", list(ROUNDS))
@pytest.mark.parametrize("K", [16, 256])
def test_rounds(dev, K, which):
    lib = L.lib()
    M, N = ROUNDS[which]
    ws, wsb, ws_ok = _workspace(dev)
    for kind in ("int", "real"):
        d = _make(kind, M, N, K)
        a, b = _operands(dev, d, 0, 0)
        c = _cmat(dev, d, N + 4, 0.0)
        bias = Vec(dev, d["bias"])
        L.check(lib.yt8m_gemm_f32_grouped(0, 0, 1, _problems([_prob(d, a, b, c, bias, 0.0)]), ws, wsb, _st()))
        got, ok = c.read()
        _judge("rounds %s (%d tiles) K=%d %s" % (which, _tiles(M, N), K, kind), d, got, ok, True, 0.0, 96)
        del d, a, b, c, got
    assert ws_ok()


# ================================================================================================================================
# groups of four, with an empty problem in the middle and at the end
GROUP_SHAPES = [(130, 258, 272), (100, 90, 256), (257, 127, 300), (64, 300, 1000)]     # 13 tiles; min_nk = 16, so S = 2 with a workspace


@pytest.mark.parametrize("variant", ["full", "M0", "N0"])
@pytest.mark.parametrize("tA,tB", LAYOUTS)
def test_groups(dev, tA, tB, variant):
    lib = L.lib()
    shapes = list(GROUP_SHAPES)
    if variant == "M0":
        shapes[1] = (0, 90, 256)
    if variant == "N0":
        shapes[3] = (64, 0, 1000)
    for wsmode in ("full", "none"):
        ws, wsb, ws_ok = _workspace(dev) if wsmode == "full" else (None, 0, lambda: True)
        for kind in ("int", "real"):
            keep, items, outs = [], [], []
            for i, (M, N, K) in enumerate(shapes):
                d = _data(kind, M, N, K, seed=i)
                a, b = _operands(dev, d, tA, tB)
                use_bias, beta = i % 2 == 0, float(i >= 2)
                c = _cmat(dev, d, N + 1 + i, beta)
                bias = Vec(dev, d["bias"]) if (use_bias and N > 0) else None
                keep.append((a, b, bias))
                items.append(_prob(d, a, b, c, bias, beta))
                outs.append((d, c, bias is not None, beta))
            L.check(lib.yt8m_gemm_f32_grouped(tA, tB, 4, _problems(items), ws, wsb, _st()))
            for i, (d, c, ub, beta) in enumerate(outs):
                got, ok = c.read()
                _judge("group %s tA=%d tB=%d ws=%s problem %d %s" % (variant, tA, tB, wsmode, i, kind), d, got, ok, ub, beta, 96)
        assert ws_ok()


def test_groups_all_empty(dev):
    lib = L.lib()
    d = _data("int", 0, 90, 256)
    a, b = _operands(dev, d, 0, 0)
    c = _cmat(dev, d, 96, 0.0)
    assert lib.yt8m_gemm_f32_grouped(0, 0, 2, _problems([_prob(d, a, b, c, None, 0.0)] * 2), None, 0, _st()) == 0
    assert c.read()[1]


# ================================================================================================================================
# yt8m_gemm_f32_batched
@pytest.mark.parametrize("extra", [0, 1, 4])
@pytest.mark.parametrize("batch", [0, 1, 3])
def test_batched(dev, batch, extra):
    lib = L.lib()
    worst = []
    for (M, N, K) in ((8, 70, 30), (129, 130, 33)):
        for (tA, tB) in LAYOUTS:
            for beta in (0.0, 1.0):
                for kind in ("int", "real"):
                    ds = [_data(kind, M, N, K, seed=100 + i) for i in range(max(batch, 1))]
                    sa = [d["A"].T if tA else d["A"] for d in ds]
                    sb = [d["B"].T if tB else d["B"] for d in ds]
                    ra, ca, rb, cb = sa[0].shape[0], sa[0].shape[1], sb[0].shape[0], sb[0].shape[1]
                    lda, ldb, ldc = _r4(ca), _r4(cb), _r4(N) + 4
                    a = Mat(dev, ra, ca, lda, 0, NAN32, batch=len(ds), stride=ra * lda + extra).put(np.stack(sa))
                    b = Mat(dev, rb, cb, ldb, 0, NAN32, batch=len(ds), stride=rb * ldb + extra).put(np.stack(sb))
                    c = Mat(dev, M, N, ldc, 0, SENT, batch=len(ds), stride=M * ldc + extra + 8)
                    if beta:
                        c.put(np.stack([d["C0"] for d in ds]))
                    before = c.ibuf.clone()
                    L.check(lib.yt8m_gemm_f32_batched(tA, tB, M, N, K, a.p, lda, a.stride, b.p, ldb, b.stride, c.p, ldc, c.stride, beta, batch, _st()))
                    if batch == 0:
                        assert torch.equal(c.ibuf, before)
                        continue
                    got, ok = c.read()
                    got = got.reshape(batch, M, N)
                    for i, d in enumerate(ds):
                        _judge("batched %d/%d stride+%d tA=%d tB=%d M=%d N=%d K=%d beta=%g %s" % (i, batch, extra, tA, tB, M, N, K, beta, kind), d, got[i], ok,
                               False, beta, 1, worst)
    _summary("batched batch=%d stride+%d" % (batch, extra), worst)


def test_batched_refusals(dev):
    lib = L.lib()
    d = _data("int", 8, 70, 30)
    a, b = _operands(dev, d, 0, 0)
    c = _cmat(dev, d, 72, 0.0)
    for batch in (65536, -1):
        assert lib.yt8m_gemm_f32_batched(0, 0, 8, 70, 30, a.p, a.ld, 0, b.p, b.ld, 0, c.p, c.ld, 0, 0.0, batch, _st()) == E_SHAPE
    assert lib.yt8m_gemm_f32_batched(0, 0, 8, 70, 30, a.p, a.ld, 0, b.p, b.ld, 0, c.p, c.ld, 0, 0.5, 1, _st()) == E_BADARG
    torch.cuda.synchronize()
    assert bool((c.ibuf == SENT).all())


# ================================================================================================================================
# refusals of the fp32 entry points: the documented code, C untouched
def test_refusals_f32(dev):
    lib = L.lib()
    M, N, K = 8, 70, 30
    d = _data("int", M, N, K)
    for (tA, tB) in LAYOUTS:
        a, b = _operands(dev, d, tA, tB)
        c = _cmat(dev, d, 72, 0.0)
        good = dict(M=M, N=N, K=K, a=a.addr, lda=a.ld, b=b.addr, ldb=b.ld, c=c.addr, ldc=c.ld, beta=0.0)
        min_lda, min_ldb = (M if tA else K), (K if tB else N)
        bad = [(dict(beta=0.5), E_BADARG), (dict(M=-1), E_SHAPE), (dict(N=-1), E_SHAPE), (dict(K=-1), E_SHAPE), (dict(lda=min_lda - 1), E_SHAPE),
               (dict(ldb=min_ldb - 1), E_SHAPE), (dict(ldc=N - 1), E_SHAPE), (dict(a=None), E_BADARG), (dict(b=None), E_BADARG),
               (dict(c=None), E_BADARG)]
        for change, code in bad:
            g = dict(good, **change)
            assert lib.yt8m_gemm_f32(tA, tB, g["M"], g["N"], g["K"], g["a"], g["lda"], g["b"], g["ldb"], g["c"], g["ldc"], None, g["beta"], _st()) == code, change
            item = (g["M"], g["N"], g["K"], g["a"], g["lda"], g["b"], g["ldb"], g["c"], g["ldc"], None, g["beta"])
            ok_item = (M, N, K, a.addr, a.ld, b.addr, b.ld, c.addr, c.ld, None, 0.0)
            # a refused problem behind a good one refuses the whole group before anything is launched
            assert lib.yt8m_gemm_f32_grouped(tA, tB, 2, _problems([ok_item, item]), None, 0, _st()) == code, change
        ok_item = (M, N, K, a.addr, a.ld, b.addr, b.ld, c.addr, c.ld, None, 0.0)
        assert lib.yt8m_gemm_f32_grouped(tA, tB, 0, _problems([ok_item]), None, 0, _st()) == E_BADARG
        assert lib.yt8m_gemm_f32_grouped(tA, tB, 5, _problems([ok_item] * 5), None, 0, _st()) == E_BADARG
        assert lib.yt8m_gemm_f32_grouped(tA, tB, 1, None, None, 0, _st()) == E_BADARG
        # an empty product needs no operands
        assert lib.yt8m_gemm_f32(tA, tB, 0, N, K, None, a.ld, None, b.ld, None, c.ld, None, 0.0, _st()) == 0
        torch.cuda.synchronize()
        assert bool((c.ibuf == SENT).all())


# ================================================================================================================================
# bf16 "NT": the large-tile kernel against the small-tile one
def _bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def _make_bf16(kind, M, N, K, seed=0):
    """A [M, K], B [N, K] holding bf16 values (as fp32), the fp64 product of exactly those, and the project's scale for the bound."""
    rs = np.random.RandomState(_seed(M, N, K, seed, kind == "int", 16))
    if kind == "int":
        A = rs.randint(-8, 9, size=(M, K)).astype(np.float32)
        Bt = rs.randint(-8, 9, size=(N, K)).astype(np.float32)
        bias = rs.randint(-64, 65, size=N).astype(np.float32)
        C0 = rs.randint(-64, 65, size=(M, N)).astype(np.float32)
    else:
        A = _bf16_round(rs.randn(M, K) * 2.0 ** ((np.arange(M) * 5) % 6 - 3)[:, None])
        Bt = _bf16_round(rs.randn(N, K) * 2.0 ** ((np.arange(N) * 7) % 6 - 3)[:, None])
        bias = rs.randn(N).astype(np.float32)
        C0 = rs.randn(M, N).astype(np.float32)
    return dict(kind=kind, M=M, N=N, K=K, A=A, Bt=Bt, bias=bias, C0=C0, ref=_ref64(A, np.ascontiguousarray(Bt.T)),
                scale=float(np.abs(A).max() * np.abs(Bt).max() * K) if A.size and Bt.size else 0.0)


@functools.lru_cache(maxsize=None)
def _data_bf16(kind, M, N, K):
    return _make_bf16(kind, M, N, K)


def _judge_bf16(what, d, got, ok, bias, beta):
    assert ok, "%s: the sentinel around C changed" % what
    exp = _expected(d, bias, beta)
    if d["kind"] == "int":
        assert np.array_equal(got.astype(np.float64), exp), "%s: integer data differ from the fp64 product at %d elements" % (what, int((got != exp).sum()))
        return 0.0
    err = float(np.abs(got.astype(np.float64) - exp).max())
    # tests/test_gpu_kernels.py test_bf16_large_tile_gemm: 2e-6 max|A| max|B| K (bias included); the accumulate addition is one more rounding
    bound = 2e-6 * d["scale"] + (U * float(np.abs(exp).max()) if beta else 0.0)
    assert err <= bound, "%s: err %.6g > bound %.6g" % (what, err, bound)
    return err / bound


def _run_bf16(dev, d, lda, ldb, ashift, ldc, use_bias, beta, ws, wsb):
    a = Mat(dev, d["M"], d["K"], lda, ashift, NAN16, torch.bfloat16).put(d["A"])
    b = Mat(dev, d["N"], d["K"], ldb, 0, NAN16, torch.bfloat16).put(d["Bt"])
    c = _cmat(dev, d, ldc, beta)
    bias = Vec(dev, d["bias"]) if use_bias else None
    L.check(L.lib().yt8m_gemm_bf16_nt_grouped(1, _problems([_prob(d, a, b, c, bias, beta)]), ws, wsb, _st()))
    return c.read()


@pytest.mark.parametrize("tiles", [255, 256])
def test_bf16_tile_floor(dev, monkeypatch, tiles):
    """15 x 17 = 255 tiles of 256 x 256 stay on the small-tile kernel, 16 x 16 = 256 take the large one (one full round, no remainder)."""
    monkeypatch.delenv("YT8M_BF16_BIG_MIN", raising=False)
    M, N = (3840, 4352) if tiles == 255 else (4096, 4096)
    assert _tiles(M, N, 256) == tiles
    ws, wsb, ws_ok = _workspace(dev)
    for kind in ("int", "real"):
        d = _make_bf16(kind, M, N, 32)
        got, ok = _run_bf16(dev, d, 32, 40, 0, N, True, 0.0, ws, wsb)
        r = _judge_bf16("bf16 %d tiles %s" % (tiles, kind), d, got, ok, True, 0.0)
        print("bf16 %d tiles %s: err / bound %.3g (bound %.3g)" % (tiles, kind, r, 2e-6 * d["scale"]))
    assert ws_ok()


BF16_BIG_PART = 256 * 256 * 4


@pytest.mark.parametrize("K", [30, 32, 34, 510, 512, 1024, 4608])
def test_bf16_small_floor(dev, monkeypatch, K):
    """YT8M_BF16_BIG_MIN = 1 (read on every call): every problem the large-tile kernel accepts takes it; the others fall to the small tiles."""
    monkeypatch.setenv("YT8M_BF16_BIG_MIN", "1")
    worst = 0.0
    for (M, N) in ((257, 255), (256, 257)):
        T = _tiles(M, N, 256)
        for kind in ("int", "real"):
            d = _data_bf16(kind, M, N, K)
            for (lda, ldb, ashift) in ((K, K, 0), (K + 8, K, 0), (K + 2, K + 8, 0), (K + 8, K + 2, 0), (K + 8, K + 8, 4)):
                res = {}
                for wsmode in ("none", "short", "full"):
                    if wsmode == "none":
                        ws, wsb, ws_ok = None, 0, lambda: True
                    else:
                        ws, wsb, ws_ok = _workspace(dev, (2 * T - 1) * BF16_BIG_PART if wsmode == "short" else None)
                    use_bias, beta = wsmode != "short", 1.0 if wsmode == "full" else 0.0
                    ldc = N if lda == K else _r4(N) + 4
                    got, ok = _run_bf16(dev, d, lda, ldb, ashift, ldc, use_bias, beta, ws, wsb)
                    assert ws_ok()
                    worst = max(worst, _judge_bf16("bf16 K=%d M=%d N=%d lda=%d ldb=%d A+%dB ws=%s %s" % (K, M, N, lda, ldb, 2 * ashift, wsmode, kind),
                                                   d, got, ok, use_bias, beta))
    print("bf16 small floor K=%d: worst err / bound %.3g" % (K, worst))


def test_empty_problem_in_a_large_tile_bf16_group(dev, monkeypatch):
    """q.M == 0 || q.N == 0: continue, in gemm_bf16_big_ok and gemm_bf16_big_launch: the tile bases of the problems behind are compacted."""
    monkeypatch.setenv("YT8M_BF16_BIG_MIN", "1")
    ws, wsb, ws_ok = _workspace(dev)
    shapes = [(257, 255, 1024), (0, 255, 64), (256, 257, 1024), (64, 0, 64)]          # 2 + 2 tiles, min_nk / 16 = 2: S = 2 and the fix-up pass
    for kind in ("int", "real"):
        keep, items, outs = [], [], []
        for i, (M, N, K) in enumerate(shapes):
            d = _data_bf16(kind, M, N, K)
            a = Mat(dev, M, K, K + 8, 0, NAN16, torch.bfloat16).put(d["A"])
            b = Mat(dev, N, K, K, 0, NAN16, torch.bfloat16).put(d["Bt"])
            beta = float(i % 2)
            c = _cmat(dev, d, _r4(N) + 4, beta)
            bias = Vec(dev, d["bias"]) if N else None
            keep.append((a, b, bias))
            items.append(_prob(d, a, b, c, bias, beta))
            outs.append((d, c, bias is not None, beta))
        L.check(L.lib().yt8m_gemm_bf16_nt_grouped(4, _problems(items), ws, wsb, _st()))
        for i, (d, c, ub, beta) in enumerate(outs):
            got, ok = c.read()
            assert ok
            if d["M"] and d["N"]:
                _judge_bf16("bf16 group with empty problems, problem %d %s" % (i, kind), d, got, ok, ub, beta)
    assert ws_ok()


def test_refusals_bf16(dev):
    lib = L.lib()
    d = _data_bf16("int", 257, 255, 32)
    a = Mat(dev, 257, 32, 32, 0, NAN16, torch.bfloat16).put(d["A"])
    b = Mat(dev, 255, 32, 32, 0, NAN16, torch.bfloat16).put(d["Bt"])
    c = _cmat(dev, d, 256, 0.0)
    good = (257, 255, 32, a.addr, 32, b.addr, 32, c.addr, 256, None, 0.0)

    def change(**kw):
        names = ["M", "N", "K", "a", "lda", "b", "ldb", "c", "ldc", "bias", "beta"]
        return tuple(kw.get(n, v) for n, v in zip(names, good))
    for item, code in ((change(K=31), E_SHAPE), (change(lda=33), E_SHAPE), (change(ldb=33), E_SHAPE), (change(beta=0.5), E_BADARG), (change(M=-1), E_SHAPE),
                       (change(lda=30), E_SHAPE), (change(ldc=254), E_SHAPE), (change(a=None), E_BADARG), (change(b=None), E_BADARG), (change(c=None), E_BADARG)):
        assert lib.yt8m_gemm_bf16_nt_grouped(1, _problems([item]), None, 0, _st()) == code, item
    assert lib.yt8m_gemm_bf16_nt_grouped(0, _problems([good]), None, 0, _st()) == E_BADARG
    assert lib.yt8m_gemm_bf16_nt_grouped(5, _problems([good] * 5), None, 0, _st()) == E_BADARG
    torch.cuda.synchronize()
    assert bool((c.ibuf == SENT).all())


# ================================================================================================================================
# the image forms: x3_launch directly, then the chooser
def _x3_image(dev, src_mat, R, C):
    """The three-plane image of the fp32 matrix in `src_mat` ([R, C] with its ld and NaN padding), by the library's split pass."""
    lib = L.lib()
    img = torch.empty((int(lib.yt8m_x3_image_bytes(R, C)) + 256,), dtype=torch.uint8, device=dev)
    L.check(lib.yt8m_x3_split(src_mat.p, R, C, src_mat.ld, 1.0, ctypes.c_void_p(img.data_ptr()), None, _st()))
    return img


def _rel(got, exp):
    return float(np.abs(got.astype(np.float64) - exp).max() / np.abs(exp).max())


def _f32_error(dev, d, bias, beta):
    """e32 of the project's image-form bounds: the fp32 kernel's own error on the same operands, relative to max |C|."""
    a, b = _operands(dev, d, 0, 0)
    c = _cmat(dev, d, d["N"], beta)
    bv = Vec(dev, d["bias"]) if bias else None
    L.check(L.lib().yt8m_gemm_f32(0, 0, d["M"], d["N"], d["K"], a.p, a.ld, b.p, b.ld, c.p, c.ld, bv.p if bv else None, beta, _st()))
    return _rel(c.read()[0], _expected(d, bias, beta))


def _oracle_exact(d, form):
    """The oracle of the image form returns exactly the fp64 product on this integer data: what lets the case demand equality."""
    from oracle import x3_ref
    bt = np.ascontiguousarray(d["B"].T)
    got = x3_ref.six_products(d["A"], bt) if form == "six" else x3_ref.three_products(d["A"], bt, 2.0 ** 10, 2.0 ** 10)
    assert np.array_equal(got, d["ref"]), "the %s oracle is not exact on this data" % form


def _judge_image(what, dev, d, got, ok, bias, beta, form):
    assert ok, "%s: the sentinel around C changed" % what
    exp = _expected(d, bias, beta)
    if d["kind"] == "int":
        if form != "f32":
            _oracle_exact(d, form)
        assert np.array_equal(got.astype(np.float64), exp), "%s: integer data differ from the fp64 product at %d elements" % (what, int((got != exp).sum()))
        return
    if form == "f32":
        return _judge(what, d, got, ok, bias, beta, 96)
    e32 = _f32_error(dev, d, bias, beta)
    err = _rel(got, exp)
    bound = max(4 * e32, 3e-7) if form == "six" else max(2 * e32, 6e-7)
    print("%s: rel err %.3g (bound %.3g, the fp32 kernel's %.3g)" % (what, err, bound, e32))
    assert err < bound, "%s: rel err %.6g >= bound %.6g" % (what, err, bound)


X3_PART = 256 * 256 * 4


@pytest.mark.parametrize("M,N,K", [(256, 256, 4096), (257, 255, 1024), (100, 300, 100)])
def test_x3_launch_parts(dev, M, N, K):
    """yt8m_gemm_x3_nt_grouped on split images: no workspace (S = 1), room for one part per tile (S = 1), all of it (up to 16 parts and the
    fix-up pass); the round-3 schedule gives the same bits as the interleaved one, and so does the combine inside the launch
    (yt8m_x3_set_combine(1): the last part of a tile to arrive sums the slabs, ordered by an arrival counter) as the separate pass."""
    lib = L.lib()
    T = _tiles(M, N, 256)
    try:
        for kind in ("int", "real"):
            d = _data(kind, M, N, K)
            a, b = _operands(dev, d, 0, 1)
            ia, ib = _x3_image(dev, a, M, K), _x3_image(dev, b, N, K)
            res = {}
            for sched, combine in ((0, 2), (2, 2), (0, 1), (2, 1)):                # combine 2: the separate fix-up pass, 1: inside the launch
                L.check(lib.yt8m_x3_set_schedule(sched))
                L.check(lib.yt8m_x3_set_combine(combine))
                for wsmode in ("none", "one", "full"):
                    ws, wsb, ws_ok = (None, 0, lambda: True) if wsmode == "none" else _workspace(dev, T * X3_PART if wsmode == "one" else None)
                    use_bias, beta = wsmode != "one", 1.0 if wsmode == "full" else 0.0
                    c = _cmat(dev, d, N + 3, beta)
                    bias = Vec(dev, d["bias"]) if use_bias else None
                    item = (M, N, K, ia.data_ptr(), 0, ib.data_ptr(), 0, c.addr, c.ld, bias.addr if bias else None, beta)
                    L.check(lib.yt8m_gemm_x3_nt_grouped(1, _problems([item]), ws, wsb, _st()))
                    got, ok = c.read()
                    assert ws_ok()
                    _judge_image("x3 launch M=%d N=%d K=%d sched=%d combine=%d ws=%s %s" % (M, N, K, sched, combine, wsmode, kind), dev, d, got, ok,
                                 use_bias, beta, "six")
                    res[(sched, combine, wsmode)] = got
            for wsmode in ("none", "one", "full"):                                 # the parts are summed in the same fixed order either way
                for key in ((2, 2), (0, 1), (2, 1)):
                    assert np.array_equal(res[(0, 2, wsmode)], res[key + (wsmode,)]), (key, wsmode)
    finally:
        lib.yt8m_x3_set_schedule(0)
        lib.yt8m_x3_set_combine(0)


def test_empty_problem_in_an_image_group(dev):
    """q.M == 0 || q.N == 0: continue in x3_launch (before the operand checks: an empty problem needs no images): full_base / part_base /
    fix_base of the problems behind are compacted."""
    lib = L.lib()
    ws, wsb, ws_ok = _workspace(dev)
    shapes = [(257, 255, 1024), (0, 300, 100), (100, 300, 100), (64, 0, 100)]
    for kind in ("int", "real"):
        keep, items, outs = [], [], []
        for i, (M, N, K) in enumerate(shapes):
            d = _data(kind, M, N, K, seed=30 + i)
            beta = float(i % 2)
            c = _cmat(dev, d, N + 3, beta)
            if M and N:
                a, b = _operands(dev, d, 0, 1)
                ia, ib = _x3_image(dev, a, M, K), _x3_image(dev, b, N, K)
                keep.append((ia, ib))
                items.append((M, N, K, ia.data_ptr(), 0, ib.data_ptr(), 0, c.addr, c.ld, None, beta))
            else:
                items.append((M, N, K, None, 0, None, 0, c.addr, c.ld, None, beta))
            outs.append((d, c, beta))
        L.check(lib.yt8m_gemm_x3_nt_grouped(4, _problems(items), ws, wsb, _st()))
        for i, (d, c, beta) in enumerate(outs):
            got, ok = c.read()
            assert ok
            if d["M"] and d["N"]:
                _judge_image("x3 group with empty problems, problem %d %s" % (i, kind), dev, d, got, ok, False, beta, "six")
    assert ws_ok()


class _Prof:
    """Launch counts per kernel family (csrc/runtime.hip yt8m_prof_*): which form a product took, asserted next to the used_x3 mask."""

    def __enter__(self):
        lib = L.lib()
        torch.cuda.synchronize()
        L.check(lib.yt8m_prof_enable(1))
        L.check(lib.yt8m_prof_reset())
        return self

    def counts(self):
        lib, out = L.lib(), {}
        for fam in (F_GEMM, F_X3, F_H2):
            n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
            L.check(lib.yt8m_prof_get(fam, ctypes.byref(n), ctypes.byref(ms)))
            out[fam] = n.value
        return out

    def __exit__(self, *exc):
        L.lib().yt8m_prof_enable(0)
        return False


def _up256(n):
    return (int(n) + 255) // 256 * 256


def _scratch(dev, nbytes):
    """(tensor, pointer, check): 256-byte aligned image scratch of nbytes with a sentinel behind it."""
    t = torch.full(((int(nbytes) + 255) // 256 * 64 + WS_GUARD,), SENT, dtype=torch.int32, device=dev)
    assert t.data_ptr() % 256 == 0
    guard = t[(int(nbytes) + 3) // 4:]
    return t, ctypes.c_void_p(t.data_ptr()), lambda: bool((guard == SENT).all())


def _auto(dev, flags, tB, cases, scratch_bytes="need", absmax=None, ws=True, info=None):
    """Runs cases = [(d, bias, beta)] through yt8m_gemm_auto_grouped(_ex) from NaN-padded fp32 sources; -> (mask, family counts, results)."""
    lib = L.lib()
    tA = flags & 1
    keep, items, cs = [], [], []
    for (d, use_bias, beta) in cases:
        a, b = d.get("_ops", {}).get((tA, tB)) or _operands(dev, d, tA, tB)
        c = _cmat(dev, d, _r4(d["N"]) + 4, beta)
        bias = Vec(dev, d["bias"]) if use_bias else None
        keep.append((a, b, bias))
        cs.append(c)
        items.append(_prob(d, a, b, c, bias, beta))
    probs = _problems(items)
    need = int(lib.yt8m_gemm_auto_scratch_bytes(flags, tB, len(items), probs))
    nbytes = need if scratch_bytes == "need" else scratch_bytes
    if nbytes is None:
        st, sp, s_ok = None, None, lambda: True
        nbytes = 0
    else:
        st, sp, s_ok = _scratch(dev, nbytes)
    wsp, wsb, ws_ok = _workspace(dev) if ws else (None, 0, lambda: True)
    mask = ctypes.c_uint64(0xDEAD)
    with _Prof() as prof:
        if absmax is None:
            rc = lib.yt8m_gemm_auto_grouped(flags, tB, len(items), probs, wsp, wsb, sp, nbytes, ctypes.byref(mask), _st())
        else:
            wa = (ctypes.c_void_p * len(items))(*[w[0] for w in absmax])
            wb = (ctypes.c_void_p * len(items))(*[w[1] for w in absmax])
            rc = lib.yt8m_gemm_auto_grouped_ex(flags, tB, len(items), probs, wa, wb, wsp, wsb, sp, nbytes, ctypes.byref(mask), _st())
        L.check(rc)
        fam = prof.counts()
    assert s_ok() and ws_ok()
    if info is not None:
        info["scratch"] = st
    return mask.value, fam, [c.read() for c in cs], need


def _img_bytes(M, N, K):
    lib = L.lib()
    return _up256(lib.yt8m_x3_image_bytes(M, K)), _up256(lib.yt8m_x3_image_bytes(N, K))


def test_auto_chooser_both_sides(dev):
    """Shapes chosen by asking yt8m_gemm_x3_pays, the expected answer asserted on both sides: 256^3 pays (one 256 x 256 tile in two K
    parts against four half-filled fp32 tiles), 257 x 255 x 256 does not (four quarter-filled large tiles), nor does 130 x 258 x 65."""
    lib = L.lib()
    assert lib.yt8m_gemm_x3_pays(256, 256, 256) == 1 and lib.yt8m_gemm_x3_pays(2048, 2048, 2048) == 1
    assert lib.yt8m_gemm_x3_pays(257, 255, 256) == 0 and lib.yt8m_gemm_x3_pays(130, 258, 65) == 0 and lib.yt8m_gemm_x3_pays(0, 256, 256) == 0
    for (tA, tB) in LAYOUTS:
        for kind in ("int", "real"):
            for (M, N, K), pays in (((256, 256, 256), True), ((257, 255, 256), False), ((130, 258, 65), False)):
                d = _data(kind, M, N, K)
                mask, fam, res, need = _auto(dev, tA, tB, [(d, True, 1.0)])
                ia, ib = _img_bytes(M, N, K)
                assert need == (ia + ib if pays else 0)
                assert mask == (1 if pays else 0) and fam == ({F_GEMM: 0, F_X3: 1, F_H2: 0} if pays else {F_GEMM: 1, F_X3: 0, F_H2: 0}), (mask, fam)
                _judge_image("auto %dx%dx%d tA=%d tB=%d %s" % (M, N, K, tA, tB, kind), dev, d, res[0][0], res[0][1], True, 1.0, "six" if pays else "f32")


ROLE_CASES = {
    # name: (transA flags, transB, (M, N, K), form)
    "dw-tb0": (ROLE_DW | 1, 0, (512, 512, 512), "h2"),
    "dw-tb1": (ROLE_DW | 1, 1, (512, 512, 512), "six"),
    "dw-notrans": (ROLE_DW, 0, (512, 512, 512), "six"),
    "plain-trans": (1, 0, (512, 512, 512), "six"),
    "h2-notrans": (ROLE_H2, 0, (512, 512, 512), "h2"),
    "h2-trans": (ROLE_H2 | 1, 1, (512, 512, 512), "h2"),
    "dw-k512": (ROLE_DW | 1, 0, (512, 516, 512), "h2"),
    "dw-k511": (ROLE_DW | 1, 0, (512, 516, 511), "six"),
    "dw-n516": (ROLE_DW | 1, 0, (256, 516, 640), "h2"),
    "dw-n518": (ROLE_DW | 1, 0, (256, 518, 640), "six"),
    "dw-nopay": (ROLE_DW | 1, 0, (512, 518, 512), "f32"),
}


@pytest.mark.parametrize("name", list(ROLE_CASES))
def test_auto_roles(dev, name):
    flags, tB, (M, N, K), form = ROLE_CASES[name]
    ia, ib = _img_bytes(M, N, K)
    want_need = {"h2": ia + ib + 512, "six": ia + ib, "f32": 0}[form]
    want_fam = {"h2": {F_GEMM: 0, F_X3: 0, F_H2: 1}, "six": {F_GEMM: 0, F_X3: 1, F_H2: 0}, "f32": {F_GEMM: 1, F_X3: 0, F_H2: 0}}[form]
    for kind in ("int", "real"):
        d = _data(kind, M, N, K)
        keep = {}
        mask, fam, res, need = _auto(dev, flags, tB, [(d, True, 0.0)], info=keep)
        assert need == want_need, (need, want_need)
        if form == "h2":                                                           # [word A | image A | word B | image B]: measured by h2_absmax_kernel
            words = keep["scratch"][[0, (256 + ia) // 4]].view(torch.float32).cpu().tolist()
            assert words == [float(np.abs(d["A"]).max()), float(np.abs(d["B"]).max())], words
        assert mask == (0 if form == "f32" else 1) and fam == want_fam, (mask, fam)
        _judge_image("auto role %s %s" % (name, kind), dev, d, res[0][0], res[0][1], True, 0.0, form)


@pytest.mark.parametrize("scratch", ["full", "short", "none"])
def test_auto_shared_operand(dev, scratch):
    """Two paying problems with the same A: its image is made once, so the de-duplicated need is enough; 256 bytes less and the second
    problem's B image does not fit -- it is rolled back and that problem alone runs on the fp32 kernel; without scratch both do."""
    M, N, K = 256, 256, 256
    ia, ib = _img_bytes(M, N, K)
    dedup = ia + 2 * ib
    for kind in ("int", "real"):
        d0 = dict(_data(kind, M, N, K, seed=0))
        d1 = dict(_data(kind, M, N, K, seed=1))
        d1["A"], d1["ref"] = d0["A"], _ref64(d0["A"], d1["B"])
        if kind == "real":
            d1["mag"] = _ref64(np.abs(d0["A"]), np.abs(d1["B"]))
        a0, b0 = _operands(dev, d0, 0, 0)
        _, b1 = _operands(dev, d1, 0, 0)
        d0["_ops"], d1["_ops"] = {(0, 0): (a0, b0)}, {(0, 0): (a0, b1)}
        nbytes = {"full": dedup, "short": dedup - 256, "none": None}[scratch]
        mask, fam, res, need = _auto(dev, 0, 0, [(d0, True, 0.0), (d1, False, 1.0)], scratch_bytes=nbytes)
        assert need == 2 * (ia + ib)                                               # the size query does not de-duplicate
        want = {"full": (3, {F_GEMM: 0, F_X3: 1, F_H2: 0}), "short": (1, {F_GEMM: 1, F_X3: 1, F_H2: 0}), "none": (0, {F_GEMM: 1, F_X3: 0, F_H2: 0})}[scratch]
        assert (mask, fam) == want, (mask, fam)
        _judge_image("shared A %s problem 0 %s" % (scratch, kind), dev, d0, res[0][0], res[0][1], True, 0.0, "six" if mask & 1 else "f32")
        _judge_image("shared A %s problem 1 %s" % (scratch, kind), dev, d1, res[1][0], res[1][1], False, 1.0, "six" if mask & 2 else "f32")


def test_auto_rollback_frees_the_scratch_of_a_problem_that_does_not_fit(dev):
    """Four paying problems; the scratch holds three pairs of 256 x 256 images.  The second problem's A image fits behind the first
    problem's, its four times larger B image does not: the offset is given back (off = mark), so the third and fourth find their room,
    and the A image is forgotten (imgs.resize(nimg)), so the fourth problem, which shares the second one's A, splits it afresh instead of
    finding a stale entry that by now points at the third problem's image -- used_x3 = 0b1101."""
    lib = L.lib()
    shapes = [(256, 256, 256), (256, 1024, 256), (256, 256, 256), (256, 256, 256)]
    assert all(lib.yt8m_gemm_x3_pays(*s) == 1 for s in shapes)
    ia, ib = _img_bytes(256, 256, 256)
    assert _img_bytes(256, 1024, 256) == (ia, 4 * ib) and ia == ib
    for kind in ("int", "real"):
        ds = [dict(_data(kind, M, N, K, seed=20 + i)) for i, (M, N, K) in enumerate(shapes)]
        ds[3]["A"], ds[3]["ref"] = ds[1]["A"], _ref64(ds[1]["A"], ds[3]["B"])
        if kind == "real":
            ds[3]["mag"] = _ref64(np.abs(ds[1]["A"]), np.abs(ds[3]["B"]))
        a1, b1 = _operands(dev, ds[1], 0, 0)
        _, b3 = _operands(dev, ds[3], 0, 0)
        ds[1]["_ops"], ds[3]["_ops"] = {(0, 0): (a1, b1)}, {(0, 0): (a1, b3)}
        cases = [(d, i == 1, float(i == 2)) for i, d in enumerate(ds)]
        mask, fam, res, need = _auto(dev, 0, 0, cases, scratch_bytes=3 * (ia + ib))
        assert need == 4 * ia + 7 * ib
        assert mask == 0b1101 and fam == {F_GEMM: 1, F_X3: 1, F_H2: 0}, (mask, fam)
        for i, ((d, ub, beta), (got, ok)) in enumerate(zip(cases, res)):
            _judge_image("auto roll-back problem %d %s" % (i, kind), dev, d, got, ok, ub, beta, "six" if i != 1 else "f32")


@pytest.mark.parametrize("form,count", [("h2", 5), ("h2", 9), ("x3", 5), ("x3", 9), ("f32", 9)])
def test_auto_chunks_of_four(dev, form, count):
    flags, (M, N, K), jf = {"h2": (ROLE_DW | 1, (512, 512, 512), "h2"), "x3": (0, (256, 256, 256), "six"), "f32": (0, (129, 127, 64), "f32")}[form]
    for kind in ("int", "real"):
        cases = [(_data(kind, M, N, K, seed=10 + i), i % 2 == 0, float(i % 3 == 0)) for i in range(count)]
        mask, fam, res, need = _auto(dev, flags, 0, cases)
        launches = (count + 3) // 4
        assert mask == (0 if form == "f32" else (1 << count) - 1)
        assert fam == {F_GEMM: launches if form == "f32" else 0, F_X3: launches if form == "x3" else 0, F_H2: launches if form == "h2" else 0}, fam
        for i, ((d, ub, beta), (got, ok)) in enumerate(zip(cases, res)):
            _judge_image("auto %d x %s problem %d %s" % (count, form, i, kind), dev, d, got, ok, ub, beta, jf)


@pytest.mark.parametrize("factor", [1.0, 2.0])
def test_auto_absmax_words(dev, factor):
    """yt8m_gemm_auto_grouped_ex with the caller's absmax words: the true maximum of each stored operand, and twice it (one bit of the
    22 the h2 contract gives is lost, the bound is the same)."""
    M, N, K = 512, 512, 512
    for kind in ("int", "real"):
        d = _data(kind, M, N, K)
        words = torch.tensor([float(np.abs(d["A"]).max()) * factor, float(np.abs(d["B"]).max()) * factor], dtype=torch.float32, device=dev)
        keep = {}
        mask, fam, res, need = _auto(dev, ROLE_DW | 1, 0, [(d, True, 1.0)], absmax=[(words.data_ptr(), words.data_ptr() + 4)], info=keep)
        assert mask == 1 and fam == {F_GEMM: 0, F_X3: 0, F_H2: 1}
        # the caller's words were used: the slots in front of the images, which the library's own measurement fills (test_auto_roles), stay untouched
        ia = _img_bytes(M, N, K)[0]
        assert keep["scratch"][[0, (256 + ia) // 4]].cpu().tolist() == [SENT, SENT]
        _judge_image("auto absmax words x %g %s" % (factor, kind), dev, d, res[0][0], res[0][1], True, 1.0, "h2")
        assert words.cpu().tolist() == [float(np.abs(d["A"]).max()) * factor, float(np.abs(d["B"]).max()) * factor]   # read, never written


def test_refusals_auto(dev):
    lib = L.lib()
    d = _data("int", 256, 256, 256)
    a, b = _operands(dev, d, 0, 0)
    c = _cmat(dev, d, 256, 0.0)
    item = _prob(d, a, b, c, None, 0.0)
    st, sp, s_ok = _scratch(dev, 1 << 22)
    mask = ctypes.c_uint64(0)
    call = lambda flags, tB, n, probs, scratch: lib.yt8m_gemm_auto_grouped(flags, tB, n, probs, None, 0, scratch, 1 << 21, ctypes.byref(mask), _st())
    assert call(0, 0, 0, _problems([item]), sp) == E_BADARG
    assert call(0, 0, 65, _problems([item] * 65), sp) == E_BADARG
    assert call(0, 0, 1, None, sp) == E_BADARG
    assert call(2, 0, 1, _problems([item]), sp) == E_BADARG and call(0, 2, 1, _problems([item]), sp) == E_BADARG
    assert call(0, 0, 1, _problems([item]), ctypes.c_void_p(st.data_ptr() + 128)) == E_BADARG       # 256-byte alignment of the image scratch
    bad = list(item)
    bad[10] = 0.5
    assert call(0, 0, 1, _problems([tuple(bad)]), sp) == E_BADARG                                   # beta 0.5: no image form, the fp32 launch refuses
    for k in (3, 5, 7):                                                                             # A, B, C NULL: no image form, the fp32 launch refuses
        bad = list(item)
        bad[k] = None
        assert call(0, 0, 1, _problems([tuple(bad)]), sp) == E_BADARG
    assert lib.yt8m_gemm_auto_scratch_bytes(0, 0, 0, _problems([item])) == 0
    torch.cuda.synchronize()
    assert bool((c.ibuf == SENT).all())


def test_refusals_images(dev):
    lib = L.lib()
    M, N, K = 100, 300, 100
    d = _data("int", M, N, K)
    a, b = _operands(dev, d, 0, 1)
    ia, ib = _x3_image(dev, a, M, K), _x3_image(dev, b, N, K)
    c = _cmat(dev, d, N, 0.0)
    good = (M, N, K, ia.data_ptr(), 0, ib.data_ptr(), 0, c.addr, c.ld, None, 0.0)

    def change(**kw):
        names = ["M", "N", "K", "a", "lda", "b", "ldb", "c", "ldc", "bias", "beta"]
        return tuple(kw.get(n, v) for n, v in zip(names, good))
    word = torch.ones(1, device=dev)
    wp = (ctypes.c_void_p * 1)(word.data_ptr())
    for fn in (lambda n, p: lib.yt8m_gemm_x3_nt_grouped(n, p, None, 0, _st()), lambda n, p: lib.yt8m_gemm_h2_nt_grouped(n, p, None, None, None, None, 0, _st())):
        for item, code in ((change(K=0), E_BADARG), (change(M=-1), E_BADARG), (change(ldc=N - 1), E_BADARG), (change(beta=0.5), E_BADARG), (change(a=None), E_BADARG),
                           (change(b=None), E_BADARG), (change(c=None), E_BADARG), (change(a=ia.data_ptr() + 8), E_BADARG), (change(lda=3), E_BADARG),
                           (change(ldb=-1), E_BADARG), (change(lda=16), E_SHAPE)):
            assert fn(1, _problems([item])) == code, item
        assert fn(0, _problems([good])) == E_BADARG and fn(5, _problems([good] * 5)) == E_BADARG and fn(1, None) == E_BADARG
    # a product scaled by a device word stores float4: N % 4 != 0 is refused
    assert lib.yt8m_gemm_h2_nt_grouped(1, _problems([change(N=298)]), None, wp, None, None, 0, _st()) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((c.ibuf == SENT).all())
