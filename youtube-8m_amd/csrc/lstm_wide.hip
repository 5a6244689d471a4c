// lstm_wide.hip -- the BasicLSTM forward step at MANY rows: one launch per step, a tiled GEMM with the cell as its epilogue
// (Z/frame_level_models.py:3653-3668: LstmLayerModel's RNN-1 runs one cell over B * (F // lstm_length) clip rows -- 3840 at B = 128 --
// for lstm_length steps; Z = youtube-8m-zhangteng).  lstm_fused.hip is shaped for B = 128 (32 rows x 8 units per workgroup, fp32 MFMA,
// no operand reuse across rows) and lstm_persist.hip refuses more than 64 row tiles per workgroup; at thousands of rows the step is a
// full-size product [B, H] x [H, 4H] and wants GEMM tiles on the f16 pipe.
//
// Tiling.  A workgroup (256 threads, 4 waves) owns ROWS = 128 rows x 32 hidden units = the 128 gate columns i|j|f|o of those units: four
//   row offsets g H + 32 ug into the W_h^T image, no repacking.  A wave owns 32 rows x the 4 gate tiles, so the four accumulators of a lane
//   at one register index are the four gates of ONE (row, unit) and the epilogue needs no exchange.  Workgroup id % (H / 32) is the unit
//   group, as in lstm_fused.hip: a unit group is always served by the same XCD, whose L2 keeps that share of W_h^T across the steps.
// Product.  The project's h2 form, hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  W_h^T is a two-half-plane image
//   (x3_image.h) under its device-measured power of two (yt8m_h2_absmax / yt8m_h2_split(trans), once per op call); h goes under the STATIC
//   power of two 2^13 because |h| = |o tanh c| <= 1: no absmax pass, no clamp.  The epilogue writes h_t twice, as fp32 into the tape and as
//   the h2 image the next step reads (two images, ping-pong; the first one is built from hs[t0]).
// Instruction choice: 32x32x16, not 16x16x32.  An image block (32 rows x 16 k, 1 KiB per plane) IS one 32x32x16 operand: lane l reads the
//   16 bytes of row l & 31, half l >> 5 -- a fully coalesced 1 KiB load for the h fragments, which no other wave shares and which therefore
//   go straight to registers one step ahead.  The W_h^T strip is shared by the four waves: 16 KiB per 32-k step through LDS (two buffers,
//   one barrier per step), read back by ds_read_b128 -- 16 reads per 24 MFMAs and wave, 1.3 per MFMA gap at two waves per SIMD, under the
//   2 per gap that MI355X_MICROARCH.md gives as free.  16x16x32 would halve the accumulator tile and double the fragment reads per FLOP.
// Schedule.  The z tile (64 registers) and c_{t-1} (16) are fetched ahead of the K loop and consumed after it, so the epilogue's reads
//   are not serialised behind the matrix time; two workgroups per CU (__launch_bounds__(256, 2): at most 256 VGPRs per lane) let one
//   workgroup's epilogue stores run under the other's K loop.  Registers per lane: 64 accumulators + 64 z + 16 c + 2 x 16 h fragments +
//   16 staged W + the fragments in flight; the build must show no spill and no scratch (tests/test_lstm_layer_host.py reads the remarks).
// Measured (tools/lstm_layer_step.py, DESIGN_LOG.md 38): 126 us per step at 3840 rows x 1024 cells against 376-381 for both existing per-step
//   routes -- 0.76 PF of f16 products, 31 % of the matrix pipe, at 1.62 TB/s of tape traffic: nearer the matrix roof than the memory one.
// num_frames must be NULL: every row runs every step (dynamic_rnn with sequence_length=None, the only form LstmLayerModel's clip pass
//   uses); a caller with lengths takes yt8m_lstm_steps_fwd.  Gates and cell update are lstm_gates_fwd_kernel's (libm expf / tanhf).
#include "step_kernels.h"
#include "x3_image.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int ROWS = 128;                    // rows of a workgroup (4 waves x 32)
constexpr float SH = 8192.f;                 // the static scale of the h images: 2^13
constexpr int64_t WORD_BYTES = 256;          // the absmax word of W_h, alone in its 256 bytes

__host__ __device__ inline int64_t up256(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline int64_t h2_bytes(int64_t rows, int64_t K) { return ((rows + 31) / 32) * ((K + 15) / 16) * 2048; }
inline int64_t pad_rows(int64_t B) { return ((B + ROWS - 1) / ROWS) * ROWS; }

__device__ __forceinline__ f16x8 frag(const uint4& v) { return __builtin_bit_cast(f16x8, v); }

// h [B, H] fp32 -> its h2 image under SH, rows B .. rows_padded - 1 zero
__global__ __launch_bounds__(256) void lstm_wide_image_kernel(const float* __restrict__ h, float* __restrict__ img, int B, int H,
                                                              int rows_padded) {
  const int KB = H >> 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows_padded * KB) return;
  const int row = (int)(idx / KB), kb = (int)(idx - (int64_t)row * KB);
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = 0.f;
  if (row < B) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(h + (int64_t)row * H + kb * 16 + 4 * q);
      v[4 * q] = x.x * SH; v[4 * q + 1] = x.y * SH; v[4 * q + 2] = x.z * SH; v[4 * q + 3] = x.w * SH;
    }
  }
  yt8m_x3::store_block_h2(v, img + ((int64_t)(row >> 5) * KB + kb) * 2 * yt8m_x3::RG_F, row);
}

// one step: z [B, 4H] in = x_t . W_x + b, out = the activated gates; c_new, h_new [B, H]; hin / hout: the h2 images of h_{t-1} / h_t
__global__ __launch_bounds__(256, 2) void lstm_wide_step_kernel(float* __restrict__ z, const uint4* __restrict__ Wimg,
                                                                const unsigned* __restrict__ wword, const uint4* __restrict__ hin,
                                                                float* __restrict__ hout, const float* __restrict__ c_prev,
                                                                float* __restrict__ c_new, float* __restrict__ h_new, int B, int H,
                                                                float fb) {
  __shared__ uint4 sB[2 * 4 * 256];          // [buffer][gate][2 k blocks x 2 planes x 64]: 32 KiB; the epilogue's h tiles afterwards
  const int groups = H >> 5, KB = H >> 4, NS = H >> 5;
  const int ug = blockIdx.x % groups, rt = blockIdx.x / groups;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int slot = r * 2 + (hh ^ ((r >> 3) & 1));          // a lane's 16 bytes inside an image block (x3_image.h)
  const int m0 = rt * ROWS + w * 32;
  const int unit = ug * 32 + r;
  const uint4* ap = hin + (int64_t)(rt * 4 + w) * KB * 128 + slot;           // + s * 256 + (k block * 2 + plane) * 64
  const uint4* bp[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bp[g] = Wimg + (int64_t)(g * groups + ug) * KB * 128 + tid;   // + s * 256
  uint4 a[4], an[4], bst[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bst[g] = bp[g][0];
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = ap[q * 64];
  // the epilogue's operands do not depend on the product: fetched here, their latency hides under the K loop
  float zpre[4][16], cpre[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    int row = m0 + (reg & 3) + 8 * (reg >> 2) + 4 * hh;
    if (row >= B) row = B - 1;                             // clamped rows feed rows >= B only (never stored)
#pragma unroll
    for (int g = 0; g < 4; ++g) zpre[g][reg] = z[(int64_t)row * 4 * H + g * H + unit];
    cpre[reg] = c_prev[(int64_t)row * H + unit];
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) sB[g * 256 + tid] = bst[g];
  f32x16 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[g][reg] = 0.f;
  __syncthreads();
  for (int s = 0; s < NS; ++s) {
    const int sn = (s + 1 < NS) ? s + 1 : s;               // no branch around the loads: the last step re-fetches itself
#pragma unroll
    for (int g = 0; g < 4; ++g) bst[g] = bp[g][sn * 256];
#pragma unroll
    for (int q = 0; q < 4; ++q) an[q] = ap[sn * 256 + q * 64];
    __builtin_amdgcn_sched_barrier(0);                     // keep the prefetch ABOVE the MFMA block (the scheduler sinks loads)
    const uint4* sb = sB + (s & 1) * 1024 + slot;
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl) {
      const f16x8 ahi = frag(a[2 * kbl]), alo = frag(a[2 * kbl + 1]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f16x8 bhi = frag(sb[g * 256 + (2 * kbl) * 64]), blo = frag(sb[g * 256 + (2 * kbl + 1) * 64]);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc[g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) sB[((s + 1) & 1) * 1024 + g * 256 + tid] = bst[g];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = an[q];
  }
  // ---- the cell: lane (unit r, half hh) holds rows (reg & 3) + 8 (reg >> 2) + 4 hh of its wave's 32
  const float inv = 1.0f / (SH * yt8m_x3::pow2_scale_for(__uint_as_float(wword[0]), 14));   // exact: powers of two
  float* hT = reinterpret_cast<float*>(sB) + w * (32 * 33);                                 // this wave's h tile [32 rows][32 units + 1]
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int rl = (reg & 3) + 8 * (reg >> 2) + 4 * hh;
    const int row = m0 + rl;
    const float gi = sigmoidf_(zpre[0][reg] + acc[0][reg] * inv);
    const float gj = tanhf(zpre[1][reg] + acc[1][reg] * inv);
    const float gf = sigmoidf_(zpre[2][reg] + acc[2][reg] * inv + fb);
    const float go = sigmoidf_(zpre[3][reg] + acc[3][reg] * inv);
    const float c = cpre[reg] * gf + gi * gj;
    const float hn = tanhf(c) * go;
    const bool ok = row < B;
    if (ok) {
      float* zr = z + (int64_t)row * 4 * H + unit;
      zr[0] = gi; zr[H] = gj; zr[2 * H] = gf; zr[3 * H] = go;
      c_new[(int64_t)row * H + unit] = c;
      h_new[(int64_t)row * H + unit] = hn;
    }
    hT[rl * 33 + r] = ok ? hn * SH : 0.f;
  }
  __syncthreads();
  // the image of h_t: lane -> (row lane & 31, k block lane >> 5) of the wave's 32 rows x 32 units
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = hT[r * 33 + hh * 16 + j];
  yt8m_x3::store_block_h2(v, hout + ((int64_t)(rt * 4 + w) * KB + ug * 2 + hh) * 2 * yt8m_x3::RG_F, r);
}

struct WideWs {
  unsigned* word;
  uint4* Wimg;
  float* himg[2];
};
inline WideWs carve(void* ws, int64_t B, int64_t H) {
  char* p = static_cast<char*>(ws);
  WideWs v;
  v.word = reinterpret_cast<unsigned*>(p);
  p += WORD_BYTES;
  v.Wimg = reinterpret_cast<uint4*>(p);
  p += up256(h2_bytes(4 * H, H));
  v.himg[0] = reinterpret_cast<float*>(p);
  p += up256(h2_bytes(pad_rows(B), H));
  v.himg[1] = reinterpret_cast<float*>(p);
  return v;
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_lstm_wide_supported(int64_t B, int64_t H) {
  return (B >= 1 && B <= (1LL << 20) && H >= 32 && H <= 4096 && (H % 32) == 0) ? 1 : 0;
}

extern "C" int yt8m_lstm_wide_row_tile(void) { return ROWS; }

extern "C" int64_t yt8m_lstm_wide_workspace_bytes(int64_t B, int64_t H) {
  if (!yt8m_lstm_wide_supported(B, H)) return 0;
  return WORD_BYTES + up256(h2_bytes(4 * H, H)) + 2 * up256(h2_bytes(pad_rows(B), H));
}

extern "C" int yt8m_lstm_wide_prepare(const float* Wh, int64_t ldw, int64_t B, int64_t H, void* workspace, int64_t workspace_bytes,
                                      yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && H >= 0, YT8M_E_SHAPE, "negative dimension");
  if (B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(Wh && workspace, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(ldw >= 4 * H, YT8M_E_SHAPE, "ldw < 4H");
  YT8M_REQUIRE(yt8m_lstm_wide_supported(B, H), YT8M_E_SHAPE, "the wide step needs H % 32 == 0, 32 <= H <= 4096, B <= 2^20");
  YT8M_REQUIRE(workspace_bytes >= yt8m_lstm_wide_workspace_bytes(B, H), YT8M_E_BADARG, "workspace too small");
  YT8M_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, YT8M_E_BADARG, "workspace must be 256-byte aligned");
  const WideWs v = carve(workspace, B, H);
  YT8M_HIP_CHECK(hipMemsetAsync(v.word, 0, WORD_BYTES, as_stream(stream)));
  int rc = yt8m_h2_absmax(Wh, H, 4 * H, ldw, v.word, stream);
  if (rc == YT8M_OK)
    rc = yt8m_h2_split(Wh, H, 4 * H, ldw, 1.0f, reinterpret_cast<const float*>(v.word), nullptr, v.Wimg, nullptr, stream);
  return rc;
}

extern "C" int yt8m_lstm_wide_steps_fwd(float* z, void* workspace, int64_t workspace_bytes, float* cs, float* hs,
                                        const int32_t* num_frames, int64_t t0, int64_t T, int64_t B, int64_t H, float forget_bias,
                                        yt8m_stream_t stream) {
  YT8M_REQUIRE(t0 >= 0 && T >= 0 && B >= 0 && H >= 0, YT8M_E_SHAPE, "negative dimension");
  if (T * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(z && workspace && cs && hs, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(num_frames == nullptr, YT8M_E_BADARG, "the wide step takes no lengths (num_frames must be NULL)");
  YT8M_REQUIRE(yt8m_lstm_wide_supported(B, H), YT8M_E_SHAPE, "the wide step needs H % 32 == 0, 32 <= H <= 4096, B <= 2^20");
  YT8M_REQUIRE(workspace_bytes >= yt8m_lstm_wide_workspace_bytes(B, H), YT8M_E_BADARG, "workspace too small");
  YT8M_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, YT8M_E_BADARG, "workspace must be 256-byte aligned");
  hipStream_t s = as_stream(stream);
  const WideWs v = carve(workspace, B, H);
  const int64_t BH = B * H, Z = B * 4 * H, rows = pad_rows(B);
  ProfScope prof(F_LSTM, s, 6.0 * (double)T * (double)B * (double)H * 4.0 * (double)H);
  hipLaunchKernelGGL(lstm_wide_image_kernel, dim3((unsigned)cdiv(rows * (H / 16), 256)), dim3(256), 0, s, hs + t0 * BH, v.himg[0],
                     (int)B, (int)H, (int)rows);
  int rc = launch_status("lstm_wide_image_kernel");
  const unsigned grid = (unsigned)((rows / ROWS) * (H / 32));
  for (int64_t i = 0; i < T && rc == YT8M_OK; ++i) {
    const int64_t t = t0 + i;
    hipLaunchKernelGGL(lstm_wide_step_kernel, dim3(grid), dim3(256), 0, s, z + t * Z, v.Wimg, v.word,
                       reinterpret_cast<const uint4*>(v.himg[i & 1]), v.himg[(i + 1) & 1], cs + t * BH, cs + (t + 1) * BH,
                       hs + (t + 1) * BH, (int)B, (int)H, forget_bias);
    rc = launch_status("lstm_wide_step_kernel");
  }
  return rc;
}
