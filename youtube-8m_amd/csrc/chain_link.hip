// chain_link.hip -- one "link" of the chain / distillchain plugins in one pass each way (gfx950, wave64; launch-latency-bound:
// the tensors are [B, 128..256] and live in L2):
//   fwd:  a = act(z) (+ stddev * N(0,1));  y = a * rsqrt(max(sum a^2, eps));  rinv[row] = +-r  (sign: ss > eps)
//   bwd:  da = R (dy - y (y.dy)) if rinv > 0 else R dy, R = |rinv|;  dz = da * act'(z)        (from the output)
// i.e. yt8m_act_fwd_f32 -> yt8m_add_noise_f32 -> yt8m_l2norm_fwd_f32 and yt8m_l2norm_bwd_f32 -> yt8m_act_bwd_f32 without the
// intermediate tensors (call sites: W/all_video_models/distillchain_deep_combine_chain_model.py:27-56 and the distillrelu / relu-<l>
// projections of W/all_frame_models/distillchain_*.py).  The noise is the draw of random.hip's noise_kernel at (seed, offset + element).
// One wave per row, 4 rows per workgroup (as l2norm_fwd_kernel); a row of up to 1024 columns stays in registers between the reduction
// and the write: one global read per element, 16-byte accesses where cols % 4 == 0 and the rows are 16-byte aligned.  Wider rows are
// read twice.  Per-lane sums in pass order, then the wave butterfly: a fixed order, no atomics, no LDS.
#include <math.h>
#include "common.h"
#include "philox.h"

namespace {

using yt8m_rng::philox4x32_10;

constexpr int REG_COLS = 1024;           // widest register-resident row: 16 floats per lane
constexpr int PASSES = REG_COLS / 64;    // single-element passes of a wave over such a row
constexpr int PASSES4 = REG_COLS / 256;  // 16-byte passes

// N(0,1) of logical element e: word (e & 3) of block e >> 2, the layout of noise_kernel
__device__ __forceinline__ float normal_at(int64_t e, uint64_t seed) {
  float n[4];
  yt8m_rng::normal4(philox4x32_10((uint64_t)(e >> 2), seed), n);
  const int w = (int)(e & 3);
  return w == 0 ? n[0] : w == 1 ? n[1] : w == 2 ? n[2] : n[3];
}
// ... of the 4 consecutive elements from e0: one block when e0 starts one
__device__ __forceinline__ void normal4_at(int64_t e0, uint64_t seed, float n[4]) {
  if ((e0 & 3) == 0) {
    yt8m_rng::normal4(philox4x32_10((uint64_t)(e0 >> 2), seed), n);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) n[k] = normal_at(e0 + k, seed);
}

// VEC: cols % 4 == 0 and z, y 16-byte aligned (checked by the caller).  reps = 1 / sqrt(eps), rounded once on the host.
template <bool VEC>
__global__ __launch_bounds__(256) void chain_link_fwd_kernel(int elu_, const float* __restrict__ z, float* __restrict__ y,
                                                             float* __restrict__ rinv, int64_t rows, int64_t cols, float eps, float reps,
                                                             float stddev, uint64_t seed, int64_t offset) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                              // wave-uniform
  const bool elu = elu_ != 0, noisy = stddev > 0.f;
  const float* zr = z + row * cols;
  float* yr = y + row * cols;
  const int64_t e_row = offset + row * cols;                            // logical element of the row's first column
  float ss = 0.f;
  if (cols <= REG_COLS) {
    float a[PASSES];
    if (VEC) {
      const int n4 = (int)(cols >> 2);
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c4 < n4) {
          const float4 q = reinterpret_cast<const float4*>(zr)[c4];
          v[0] = link_act(elu, q.x); v[1] = link_act(elu, q.y); v[2] = link_act(elu, q.z); v[3] = link_act(elu, q.w);
          if (noisy) {
            float n[4];
            normal4_at(e_row + 4 * (int64_t)c4, seed, n);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = yt8m_rng::add_normal(v[k], stddev, n[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[4 * p + k] = v[k];
        ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        float v = 0.f;
        if (c < cols) {
          v = link_act(elu, zr[c]);
          if (noisy) v = yt8m_rng::add_normal(v, stddev, normal_at(e_row + c, seed));
        }
        a[p] = v;
        ss += v * v;
      }
    }
    ss = wave_sum(ss);
    const float r = link_r(ss, eps, reps);
    if (VEC) {
      const int n4 = (int)(cols >> 2);
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        if (c4 < n4)
          reinterpret_cast<float4*>(yr)[c4] = make_float4(a[4 * p] * r, a[4 * p + 1] * r, a[4 * p + 2] * r, a[4 * p + 3] * r);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < cols) yr[c] = a[p] * r;
      }
    }
    if (lane == 0) rinv[row] = ss > eps ? r : -r;
    return;
  }
  // wide rows: the activation (and its noise) is computed twice, z read twice
  for (int64_t c = lane; c < cols; c += 64) {
    float v = link_act(elu, zr[c]);
    if (noisy) v = yt8m_rng::add_normal(v, stddev, normal_at(e_row + c, seed));
    ss += v * v;
  }
  ss = wave_sum(ss);
  const float r = link_r(ss, eps, reps);
  for (int64_t c = lane; c < cols; c += 64) {
    float v = link_act(elu, zr[c]);
    if (noisy) v = yt8m_rng::add_normal(v, stddev, normal_at(e_row + c, seed));
    yr[c] = v * r;
  }
  if (lane == 0) rinv[row] = ss > eps ? r : -r;
}

// VEC: cols % 4 == 0 and z, y, dy, dz 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void chain_link_bwd_kernel(int elu_, const float* __restrict__ z, const float* __restrict__ y,
                                                             const float* __restrict__ rinv, const float* __restrict__ dy,
                                                             float* __restrict__ dz, int64_t rows, int64_t cols) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bool elu = elu_ != 0;
  const float* zr = z + row * cols;
  const float* yr = y + row * cols;
  const float* gr = dy + row * cols;
  float* dr = dz + row * cols;
  const float ri = rinv[row], R = fabsf(ri);
  const bool unit = ri > 0.f;                                           // the row was divided by its own norm (ss > eps)
  float yg = 0.f;
  if (cols <= REG_COLS) {
    float yv[PASSES], gv[PASSES], mv[PASSES];                           // y, dy, act'(z)
    if (VEC) {
      const int n4 = (int)(cols >> 2);
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a, q = a;
        if (c4 < n4) {
          a = reinterpret_cast<const float4*>(yr)[c4];
          g = reinterpret_cast<const float4*>(gr)[c4];
          q = reinterpret_cast<const float4*>(zr)[c4];
        }
        yv[4 * p] = a.x; yv[4 * p + 1] = a.y; yv[4 * p + 2] = a.z; yv[4 * p + 3] = a.w;
        gv[4 * p] = g.x; gv[4 * p + 1] = g.y; gv[4 * p + 2] = g.z; gv[4 * p + 3] = g.w;
        mv[4 * p] = link_act_grad(elu, q.x); mv[4 * p + 1] = link_act_grad(elu, q.y);
        mv[4 * p + 2] = link_act_grad(elu, q.z); mv[4 * p + 3] = link_act_grad(elu, q.w);
        yg += (a.x * g.x + a.y * g.y) + (a.z * g.z + a.w * g.w);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        const bool in = c < cols;
        yv[p] = in ? yr[c] : 0.f;
        gv[p] = in ? gr[c] : 0.f;
        mv[p] = in ? link_act_grad(elu, zr[c]) : 0.f;
        yg += yv[p] * gv[p];
      }
    }
    const float k = wave_sum(yg);
    float d[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) d[p] = (unit ? R * (gv[p] - yv[p] * k) : R * gv[p]) * mv[p];
    if (VEC) {
      const int n4 = (int)(cols >> 2);
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        if (c4 < n4) reinterpret_cast<float4*>(dr)[c4] = make_float4(d[4 * p], d[4 * p + 1], d[4 * p + 2], d[4 * p + 3]);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < cols) dr[c] = d[p];
      }
    }
    return;
  }
  for (int64_t c = lane; c < cols; c += 64) yg += yr[c] * gr[c];
  const float k = wave_sum(yg);
  for (int64_t c = lane; c < cols; c += 64) dr[c] = (unit ? R * (gr[c] - yr[c] * k) : R * gr[c]) * link_act_grad(elu, zr[c]);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_chain_link_fwd(int act, const float* z, float* y, float* rinv, int64_t rows, int64_t cols, float eps, float stddev,
                                   uint64_t seed, int64_t offset, yt8m_stream_t stream) {
  YT8M_REQUIRE(act == YT8M_ACT_RELU || act == YT8M_ACT_ELU, YT8M_E_BADARG, "a link's activation is relu or elu");
  YT8M_REQUIRE(z && y && rinv, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(rows > 0 && cols > 0, YT8M_E_BADARG, "rows and cols must be positive");
  YT8M_REQUIRE(eps > 0.f && stddev >= 0.f && offset >= 0, YT8M_E_BADARG, "eps must be > 0, stddev and offset >= 0");
  YT8M_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, YT8M_E_SHAPE, "too many rows");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const float reps = (float)(1.0 / sqrt((double)eps));
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const int elu = act == YT8M_ACT_ELU;
  if ((cols & 3) == 0 && aligned16(z) && aligned16(y))
    hipLaunchKernelGGL(chain_link_fwd_kernel<true>, grid, block, 0, s, elu, z, y, rinv, rows, cols, eps, reps, stddev, seed, offset);
  else
    hipLaunchKernelGGL(chain_link_fwd_kernel<false>, grid, block, 0, s, elu, z, y, rinv, rows, cols, eps, reps, stddev, seed, offset);
  return launch_status("chain_link_fwd_kernel");
}

extern "C" int yt8m_chain_link_bwd(int act, const float* z, const float* y, const float* rinv, const float* dy, float* dz, int64_t rows,
                                   int64_t cols, float eps, yt8m_stream_t stream) {
  YT8M_REQUIRE(act == YT8M_ACT_RELU || act == YT8M_ACT_ELU, YT8M_E_BADARG, "a link's activation is relu or elu");
  YT8M_REQUIRE(z && y && rinv && dy && dz, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(rows > 0 && cols > 0, YT8M_E_BADARG, "rows and cols must be positive");
  YT8M_REQUIRE(eps > 0.f, YT8M_E_BADARG, "eps must be > 0");
  YT8M_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, YT8M_E_SHAPE, "too many rows");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const int elu = act == YT8M_ACT_ELU;
  if ((cols & 3) == 0 && aligned16(z) && aligned16(y) && aligned16(dy) && aligned16(dz))
    hipLaunchKernelGGL(chain_link_bwd_kernel<true>, grid, block, 0, s, elu, z, y, rinv, dy, dz, rows, cols);
  else
    hipLaunchKernelGGL(chain_link_bwd_kernel<false>, grid, block, 0, s, elu, z, y, rinv, dy, dz, rows, cols);
  return launch_status("chain_link_bwd_kernel");
}
