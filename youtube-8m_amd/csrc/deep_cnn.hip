// deep_cnn.hip -- what joins a level of the deep CNN of DeepCnnDeepCombineChainModel to the classifier and to the next, half-as-long level
// (W/all_frame_models/deep_cnn_deep_combine_chain_model.py:42-63,93,115): a level's output y [F,B,C] is used twice, by tf.reduce_max over
// all frames and by tf.nn.pool(MAX, window 2, stride 2, VALID), on TIME-major rows (row t B + b) as the CNN products write them.
//
//   yt8m_timepool_max_pool2_f32_fwd   ONE pass over y: out[b,c] = max_t y[t,b,c], idx[b,c] = the FIRST frame that attains it (the contract
//                                     of yt8m_timepool_max_f32) and pooled[j,b,c] = max(y[2j,b,c], y[2j+1,b,c]) [F/2,B,C]
//   yt8m_timepool_max_pool2_f32_bwd   ONE pass that writes every element of dy: the global maximum's gradient at frame idx plus the pooled
//                                     gradient at the frame of the pair that won (recomputed from y) -- no zero-fill, no atomics
//
// Streams, bound by HBM: forward reads y once and writes half of it, backward reads y and dp and writes dy.
//
// Forward: timepool_shiftmax_kernel's decomposition (csrc/cnn_pool.hip) with a frame class owning frame PAIRS: a workgroup owns one video
// and 64 columns, 16 column groups of four (16-byte accesses) x 16 pair classes (j mod 16); a class stores its pairs' maxima while it keeps
// its own running maximum and first frame, the classes are merged through LDS (larger value, the earlier frame on a tie).
// Backward: a pure map over "pair rows" r = j B + b, the row walk of ms_bn_relu_pool2_fwd_kernel (csrc/multiscale.hip).
//
// Tie rule: tf.reduce_max (and tf.nn.pool's gradient through it) splits a gradient between equal maxima; here the FIRST frame takes it
// all, in the global maximum and inside a pair (frame 2j wins iff y[2j] >= y[2j+1]).  Exact ties do occur: a CNN output row whose window
// lies wholly in the padding is exactly 0, so padding pairs tie at 0, and a column whose live outputs are all negative has its global
// maximum 0 on several padding rows.  Those rows have all-zero inputs, so whichever of them receives the gradient hands nothing on to any
// filter: the variables' gradients are those of the splitting rule (checked on the CPU in fp64: three levels, B = 6, F = 13, num_frames
// 13, 1, 2, 5, 12, 7; 10 of 192 pooled columns had a maximum of exactly 0; every filter gradient identical under both rules, difference
// 0.0 at a largest gradient of 8.4).  Ties between live rows are a set of measure zero.
#include "common.h"

namespace yt8m {
namespace {

constexpr int DC_CL = 64;            // column lanes (float4 each) per workgroup of the backward map
constexpr int DC_RL = 4;             // row lanes per workgroup of the backward map
constexpr int DC_MAP_BLOCKS = 512;   // row blocks of the backward map
constexpr int DC_NONE = 0x7fffffff;  // "no frame seen yet"

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

// the running maximum of a class: frames arrive in ascending order, so `>` keeps the first one (its first frame always enters)
__device__ __forceinline__ void take(float v, int t, float& m, int& at) {
  if (v > m || at == DC_NONE) { m = v; at = t; }
}
__device__ __forceinline__ void take4(const float4& v, int t, float4& m, int4& at) {
  take(v.x, t, m.x, at.x); take(v.y, t, m.y, at.y); take(v.z, t, m.z, at.z); take(v.w, t, m.w, at.w);
}
__device__ __forceinline__ void merge(float v, int w, float& m, int& at) {
  if (w != DC_NONE && (at == DC_NONE || v > m || (v == m && w < at))) { m = v; at = w; }
}

// block = (64 columns, video): 16 column groups of four x 16 pair classes
__global__ __launch_bounds__(256) void dc_max_pool2_fwd_kernel(const float* __restrict__ y, long long ldy, int F, int B, int C,
                                                               float* __restrict__ out, int32_t* __restrict__ idx, long long ldo,
                                                               float* __restrict__ pooled, long long ldp) {
  __shared__ float4 s_m[16][16];
  __shared__ int4 s_t[16][16];
  const int cg = threadIdx.x & 15, tg = threadIdx.x >> 4;
  const int b = blockIdx.y, c = blockIdx.x * 64 + 4 * cg;
  const bool live = c < C;
  const float NEG = -3.402823466e38f;
  float4 m = make_float4(NEG, NEG, NEG, NEG);
  int4 at = make_int4(DC_NONE, DC_NONE, DC_NONE, DC_NONE);
  if (live) {
    const float* p = y + (long long)b * ldy + c;
    const long long step = (long long)B * ldy;                      // one frame
    const int NPR = (F + 1) / 2;                                    // pairs, the unpaired last frame of an odd F included
#pragma unroll 2
    for (int j = tg; j < NPR; j += 16) {
      const bool has1 = 2 * j + 1 < F;
      const float4 v0 = ld4(p + (long long)(2 * j) * step);
      take4(v0, 2 * j, m, at);
      if (has1) {
        const float4 v1 = ld4(p + (long long)(2 * j + 1) * step);
        take4(v1, 2 * j + 1, m, at);
        if (pooled)
          st4(pooled + ((long long)j * B + b) * ldp + c,
              make_float4(fmaxf(v0.x, v1.x), fmaxf(v0.y, v1.y), fmaxf(v0.z, v1.z), fmaxf(v0.w, v1.w)));
      }
    }
  }
  s_m[tg][cg] = m;
  s_t[tg][cg] = at;
  __syncthreads();
  if (tg == 0 && live) {                                            // (class 0 holds frame 0: F >= 1)
#pragma unroll
    for (int j = 1; j < 16; ++j) {
      const float4 v = s_m[j][cg];
      const int4 w = s_t[j][cg];
      merge(v.x, w.x, m.x, at.x); merge(v.y, w.y, m.y, at.y); merge(v.z, w.z, m.z, at.z); merge(v.w, w.w, m.w, at.w);
    }
    st4(out + (long long)b * ldo + c, m);
    *reinterpret_cast<int4*>(idx + (long long)b * ldo + c) = at;
  }
}

// gradient of one column at the two frames of a pair: g at the frame of the global maximum, dp at the pair's winner (the first on a tie)
__device__ __forceinline__ void pair_dy(float y0, float y1, float g, int at, float dp, int t0, bool has1, float& d0, float& d1) {
  const bool first = y0 >= y1;
  d0 = (at == t0 ? g : 0.f) + (has1 && first ? dp : 0.f);
  d1 = (at == t0 + 1 ? g : 0.f) + (first ? 0.f : dp);
}

// "pair row" r = j B + b stands for the rows (2j) B + b and (2j + 1) B + b: both frames of a pair for 4 columns per thread.  The last
// frame of an odd F has no partner (has1 false): it takes the global maximum's gradient only.
__global__ __launch_bounds__(256) void dc_max_pool2_bwd_kernel(const float* __restrict__ y, long long ldy, int F, int B, int C,
                                                               const float* __restrict__ g, const int32_t* __restrict__ idx, long long ldg,
                                                               const float* __restrict__ dp, long long lddp, float* __restrict__ dy,
                                                               long long lddy, int rows_per_block) {
  const int cl = threadIdx.x & (DC_CL - 1), rl = threadIdx.x / DC_CL;
  const int c = (blockIdx.x * DC_CL + cl) * 4;
  if (c >= C) return;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const int NP = ((F + 1) / 2) * B;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(r0 + rows_per_block, NP);
#pragma unroll 2
  for (int r = r0 + rl; r < r1; r += DC_RL) {
    const int j = r / B, b = r - j * B;
    const long long row0 = (long long)r + (long long)j * B;         // (2j) B + b
    const bool has1 = 2 * j + 1 < F;
    const float4 y0 = ld4(y + row0 * ldy + c);
    const int4 at = *reinterpret_cast<const int4*>(idx + (long long)b * ldg + c);
    const float4 gg = g ? ld4(g + (long long)b * ldg + c) : z;
    float4 y1 = y0, p = z;
    if (has1) {
      y1 = ld4(y + (row0 + B) * ldy + c);
      if (dp) p = ld4(dp + (long long)r * lddp + c);
    }
    float4 d0, d1;
    pair_dy(y0.x, y1.x, gg.x, at.x, p.x, 2 * j, has1, d0.x, d1.x);
    pair_dy(y0.y, y1.y, gg.y, at.y, p.y, 2 * j, has1, d0.y, d1.y);
    pair_dy(y0.z, y1.z, gg.z, at.z, p.z, 2 * j, has1, d0.z, d1.z);
    pair_dy(y0.w, y1.w, gg.w, at.w, p.w, 2 * j, has1, d0.w, d1.w);
    st4(dy + row0 * lddy + c, d0);
    if (has1) st4(dy + (row0 + B) * lddy + c, d1);
  }
}


}  // namespace
}  // namespace yt8m

using namespace yt8m;

static int max_pool2_check(const float* y, int64_t ldy, int64_t F, int64_t B, int64_t C) {
  YT8M_REQUIRE(F >= 1 && B >= 1 && C >= 4 && C < (1LL << 31) && B < 65536, YT8M_E_SHAPE, "F, B >= 1, C >= 4, B < 65536");
  YT8M_REQUIRE(F < (1LL << 31) && F * B < (1LL << 31) - 64, YT8M_E_SHAPE, "too many frame rows (F B must stay below 2^31)");
  YT8M_REQUIRE(C % 4 == 0, YT8M_E_SHAPE, "C must be a multiple of 4 (16-byte accesses)");
  YT8M_REQUIRE(ldy >= C && ldy % 4 == 0, YT8M_E_SHAPE, "ldy must be >= C and a multiple of 4");
  YT8M_REQUIRE(y, YT8M_E_BADARG, "null operand (y)");
  return YT8M_OK;
}

extern "C" int yt8m_timepool_max_pool2_f32_fwd(const float* y, int64_t ldy, int64_t F, int64_t B, int64_t C, float* out, int32_t* idx,
                                               int64_t ldo, float* pooled, int64_t ldp, yt8m_stream_t stream) {
  int rc = max_pool2_check(y, ldy, F, B, C);
  if (rc != YT8M_OK) return rc;
  YT8M_REQUIRE(ldo >= C && ldo % 4 == 0 && (!pooled || (ldp >= C && ldp % 4 == 0)), YT8M_E_SHAPE,
               "ldo / ldp must be >= C and a multiple of 4");
  YT8M_REQUIRE(out && idx, YT8M_E_BADARG, "null operand (out, idx)");
  YT8M_REQUIRE(aligned16(y) && aligned16(out) && aligned16(idx) && aligned16(pooled), YT8M_E_BADARG, "operands must be 16-byte aligned");
  YT8M_REQUIRE(out != y && pooled != y && pooled != out && (const void*)idx != (const void*)y && (const void*)idx != (const void*)out &&
               (const void*)idx != (const void*)pooled, YT8M_E_BADARG, "outputs must not alias the input or each other");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  hipLaunchKernelGGL(dc_max_pool2_fwd_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(256), 0, s, y, (long long)ldy, (int)F, (int)B,
                     (int)C, out, idx, (long long)ldo, F >= 2 ? pooled : (float*)nullptr, (long long)ldp);
  return launch_status("dc_max_pool2_fwd_kernel");
}

extern "C" int yt8m_timepool_max_pool2_f32_bwd(const float* y, int64_t ldy, int64_t F, int64_t B, int64_t C, const float* g,
                                               const int32_t* idx, int64_t ldg, const float* dp, int64_t lddp, float* dy, int64_t lddy,
                                               yt8m_stream_t stream) {
  int rc = max_pool2_check(y, ldy, F, B, C);
  if (rc != YT8M_OK) return rc;
  YT8M_REQUIRE(ldg >= C && ldg % 4 == 0 && (!dp || (lddp >= C && lddp % 4 == 0)) && lddy >= C && lddy % 4 == 0, YT8M_E_SHAPE,
               "ldg / lddp / lddy must be >= C and a multiple of 4");
  YT8M_REQUIRE(idx && dy, YT8M_E_BADARG, "null operand (idx, dy)");
  YT8M_REQUIRE(aligned16(y) && aligned16(g) && aligned16(idx) && aligned16(dp) && aligned16(dy), YT8M_E_BADARG,
               "operands must be 16-byte aligned");
  YT8M_REQUIRE(dy != y && dy != dp && dy != g && (const void*)dy != (const void*)idx, YT8M_E_BADARG, "dy must not alias an input");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int64_t NP = (F + 1) / 2 * B;
  int64_t rpb = (NP + DC_MAP_BLOCKS - 1) / DC_MAP_BLOCKS;           // at most DC_MAP_BLOCKS row blocks; every row lane gets a few rows
  if (rpb < 4 * DC_RL) rpb = 4 * DC_RL;
  hipLaunchKernelGGL(dc_max_pool2_bwd_kernel, dim3((unsigned)((C / 4 + DC_CL - 1) / DC_CL), (unsigned)((NP + rpb - 1) / rpb)), dim3(256), 0, s,
                     y, (long long)ldy, (int)F, (int)B, (int)C, g, idx, (long long)ldg, F >= 2 ? dp : (const float*)nullptr, (long long)lddp, dy,
                     (long long)lddy, (int)rpb);
  return launch_status("dc_max_pool2_bwd_kernel");
}
