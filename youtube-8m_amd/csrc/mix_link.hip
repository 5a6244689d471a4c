// mix_link.hip -- the step between two MoE stages of the MoeMix4 / MoeKnowledge heads (Z/video_level_models.py:1872-2044, :1331-1438) in
// one pass each way (gfx950, wave64; launch-latency-bound: the tensors are [B, 1152..2400] and [B, 200..512] and live in L2).  The host
// makes ONE product z = p . [W1 | W2] [rows, 2 C] (MoeKnowledge: z2 = (p . seq) . W2) and one vector u = [u1 | u2] [2 C]:
//   fwd, per row:  a1 = elu(z1 + u1);  a2 = elu(u2 - z2) (complement: (1 - p) . W2 + b2 with u2 = colsum(W2) + b2, no 1 - p tensor) or
//         elu(z2 + u2) (plain);  norm mode: y_k = (a_k * r_k) * scale, r_k = rsqrt(max(sum a_k^2, eps)), per segment;  none mode: y_k = a_k;
//         out[row] = [prev[row] | y1 | y2] written straight into the new, wider row;  stats[k * rows + row] = +-r_k (sign: ss > eps; 1 in
//         none mode)
//   bwd, per row:  dprev[:, dx_from:] = dy[:, dx_from:Wprev] (the leading dx_from data columns are neither read nor written; a null dprev
//         is skipped);  per segment, with a and act' recomputed from z and u:  yh = a R, R = |r|;  da = scale R (dy - yh (yh . dy)) if r > 0
//         else scale R dy (chain_link.hip's rule at the clamp);  none mode: da = dy;  dz1 = da1 elu'(z1 + u1),  dz2 = -+ da2 elu'(-+z2 + u2):
//         the complement's sign is in dz, so that dp is ONE product dz . [W1 | W2]^T and dW ONE p^T . dz.
// i.e. two products on [B, V], a materialised 1 - p, two yt8m_act_fwd_f32, two yt8m_l2norm_fwd_f32, two scalings and torch.cat (and their
// backward passes) without the tensors in between.  One wave per row, 4 rows per workgroup (as chain_link.hip and distill_head.hip); a
// segment (C <= 1024 columns: what yt8m_mix_link_supported accepts) stays in registers between its reduction and the write: one global
// read per element; 16-byte accesses where Wprev % 4 == 0, C % 4 == 0 (bwd: dx_from % 4 == 0 too) and every operand is 16-byte aligned,
// single elements otherwise.  Per-lane sums in pass order, then the wave butterfly: a fixed order, no atomics, no LDS; every output
// element is written exactly once.
#include <math.h>
#include "common.h"

namespace {

constexpr int REG_COLS = 1024;           // widest segment: 16 floats per lane
constexpr int PASSES = REG_COLS / 64;    // single-element passes of a wave over such a segment
constexpr int PASSES4 = REG_COLS / 256;  // 16-byte passes

constexpr int M_PLAIN = YT8M_MIX_LINK_PLAIN, M_NONE = YT8M_MIX_LINK_NONE;
constexpr int64_t MAX_PREV = (int64_t)1 << 24;

// a segment's pre-activation: z + u, or u - z for the complement
__device__ __forceinline__ float pre_act(bool neg, float z, float u) { return neg ? u - z : z + u; }

// dst[c] = src[c] for the columns [c0, cols) of a row; VEC: c0, cols % 4 == 0 and both rows 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void copy_cols(const float* __restrict__ src, float* __restrict__ dst, int c0, int cols, int lane) {
  if (VEC) {
    for (int c4 = (c0 >> 2) + lane; c4 < (cols >> 2); c4 += 64) reinterpret_cast<float4*>(dst)[c4] = reinterpret_cast<const float4*>(src)[c4];
  } else {
    for (int c = c0 + lane; c < cols; c += 64) dst[c] = src[c];
  }
}

// One segment of a row: dst[c] = (elu(+-z[c] + u[c]) * r) * scale, or the elu alone.  Returns the signed reciprocal norm (1 in none mode).
template <bool VEC>
__device__ __forceinline__ float seg_fwd(const float* __restrict__ zr, const float* __restrict__ u, float* __restrict__ dst, int C, bool neg,
                                         bool norm, float scale, float eps, float reps, int lane) {
  const int n4 = C >> 2;
  float a[PASSES];
  float ss = 0.f;
  if (VEC) {
#pragma unroll
    for (int p = 0; p < PASSES4; ++p) {
      const int c4 = lane + 64 * p;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (c4 < n4) {
        const float4 q = reinterpret_cast<const float4*>(zr)[c4];
        const float4 b = reinterpret_cast<const float4*>(u)[c4];
        v[0] = link_act(true, pre_act(neg, q.x, b.x)); v[1] = link_act(true, pre_act(neg, q.y, b.y));
        v[2] = link_act(true, pre_act(neg, q.z, b.z)); v[3] = link_act(true, pre_act(neg, q.w, b.w));
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) a[4 * p + k] = v[k];
      ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
  } else {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int c = lane + 64 * p;
      const float v = c < C ? link_act(true, pre_act(neg, zr[c], u[c])) : 0.f;
      a[p] = v;
      ss += v * v;
    }
  }
  float r = 1.f;
  if (norm) {                                                           // wave-uniform
    ss = wave_sum(ss);
    r = link_r(ss, eps, reps);
#pragma unroll
    for (int p = 0; p < PASSES; ++p) a[p] = (a[p] * r) * scale;         // the reference's order: l2_normalize, then the scale
  }
  if (VEC) {
#pragma unroll
    for (int p = 0; p < PASSES4; ++p) {
      const int c4 = lane + 64 * p;
      if (c4 < n4) reinterpret_cast<float4*>(dst)[c4] = make_float4(a[4 * p], a[4 * p + 1], a[4 * p + 2], a[4 * p + 3]);
    }
  } else {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int c = lane + 64 * p;
      if (c < C) dst[c] = a[p];
    }
  }
  return norm ? (ss > eps ? r : -r) : 1.f;
}

// VEC: Wprev % 4 == 0, C % 4 == 0 and prev, z, u, out 16-byte aligned (checked by the caller).  reps = 1 / sqrt(eps), rounded once on the
// host.  stats: [2, rows].
template <bool VEC>
__global__ __launch_bounds__(256) void mix_link_fwd_kernel(int mode, const float* __restrict__ prev, const float* __restrict__ z,
                                                           const float* __restrict__ u, float* __restrict__ out, float* __restrict__ stats,
                                                           int64_t rows, int Wprev, int C, float scale, float eps, float reps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                              // wave-uniform
  const bool norm = (mode & M_NONE) == 0;
  float* o = out + row * ((int64_t)Wprev + 2 * C);
  const float* zr = z + row * (2 * (int64_t)C);
  copy_cols<VEC>(prev + row * Wprev, o, 0, Wprev, lane);
  const float r1 = seg_fwd<VEC>(zr, u, o + Wprev, C, false, norm, scale, eps, reps, lane);
  const float r2 = seg_fwd<VEC>(zr + C, u + C, o + Wprev + C, C, (mode & M_PLAIN) == 0, norm, scale, eps, reps, lane);
  if (lane == 0) {
    stats[row] = r1;
    stats[rows + row] = r2;
  }
}

// One segment of a row backwards: dzr[c] = +-da[c] * elu'(pre[c]), da from the recomputed a and dy by the rule above.
template <bool VEC>
__device__ __forceinline__ void seg_bwd(const float* __restrict__ zr, const float* __restrict__ u, const float* __restrict__ gr,
                                        float* __restrict__ dzr, int C, bool neg, bool norm, float ri, float scale, int lane) {
  const int n4 = C >> 2;
  float yv[PASSES], gv[PASSES], mv[PASSES];                             // a R, dy, +-elu'(pre)
  const float R = fabsf(ri), sg = neg ? -1.f : 1.f;
  float yg = 0.f;
  if (VEC) {
#pragma unroll
    for (int p = 0; p < PASSES4; ++p) {
      const int c4 = lane + 64 * p;
      float pv[4] = {0.f, 0.f, 0.f, 0.f}, g4[4] = {0.f, 0.f, 0.f, 0.f};
      const bool in = c4 < n4;
      if (in) {
        const float4 q = reinterpret_cast<const float4*>(zr)[c4];
        const float4 b = reinterpret_cast<const float4*>(u)[c4];
        const float4 g = reinterpret_cast<const float4*>(gr)[c4];
        pv[0] = pre_act(neg, q.x, b.x); pv[1] = pre_act(neg, q.y, b.y); pv[2] = pre_act(neg, q.z, b.z); pv[3] = pre_act(neg, q.w, b.w);
        g4[0] = g.x; g4[1] = g.y; g4[2] = g.z; g4[3] = g.w;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        yv[4 * p + k] = in ? link_act(true, pv[k]) * R : 0.f;
        mv[4 * p + k] = in ? sg * link_act_grad(true, pv[k]) : 0.f;
        gv[4 * p + k] = g4[k];
      }
      yg += (yv[4 * p] * g4[0] + yv[4 * p + 1] * g4[1]) + (yv[4 * p + 2] * g4[2] + yv[4 * p + 3] * g4[3]);
    }
  } else {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int c = lane + 64 * p;
      const bool in = c < C;
      const float pre = in ? pre_act(neg, zr[c], u[c]) : 0.f;
      yv[p] = in ? link_act(true, pre) * R : 0.f;
      mv[p] = in ? sg * link_act_grad(true, pre) : 0.f;
      gv[p] = in ? gr[c] : 0.f;
      yg += yv[p] * gv[p];
    }
  }
  float d[PASSES];
  if (norm) {                                                           // wave-uniform
    const float k = wave_sum(yg), sR = scale * R;
    const bool unit = ri > 0.f;                                         // the segment was divided by its own norm (ss > eps)
#pragma unroll
    for (int p = 0; p < PASSES; ++p) d[p] = (unit ? sR * (gv[p] - yv[p] * k) : sR * gv[p]) * mv[p];
  } else {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) d[p] = gv[p] * mv[p];
  }
  if (VEC) {
#pragma unroll
    for (int p = 0; p < PASSES4; ++p) {
      const int c4 = lane + 64 * p;
      if (c4 < n4) reinterpret_cast<float4*>(dzr)[c4] = make_float4(d[4 * p], d[4 * p + 1], d[4 * p + 2], d[4 * p + 3]);
    }
  } else {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int c = lane + 64 * p;
      if (c < C) dzr[c] = d[p];
    }
  }
}

// VEC: Wprev % 4 == 0, C % 4 == 0, dx_from % 4 == 0 and z, u, dy, dz and a non-null dprev 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void mix_link_bwd_kernel(int mode, const float* __restrict__ z, const float* __restrict__ u,
                                                           const float* __restrict__ stats, const float* __restrict__ dy,
                                                           float* __restrict__ dprev, float* __restrict__ dz, int64_t rows, int Wprev, int C,
                                                           int dx_from, float scale) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bool norm = (mode & M_NONE) == 0;
  const float* g = dy + row * ((int64_t)Wprev + 2 * C);
  const float* zr = z + row * (2 * (int64_t)C);
  float* dzr = dz + row * (2 * (int64_t)C);
  if (dprev) copy_cols<VEC>(g, dprev + row * Wprev, dx_from, Wprev, lane);
  seg_bwd<VEC>(zr, u, g + Wprev, dzr, C, false, norm, stats[row], scale, lane);
  seg_bwd<VEC>(zr + C, u + C, g + Wprev + C, dzr + C, C, (mode & M_PLAIN) == 0, norm, stats[rows + row], scale, lane);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_mix_link_supported(int64_t Wprev, int64_t C) { return Wprev >= 1 && Wprev <= MAX_PREV && C >= 1 && C <= REG_COLS; }

extern "C" int yt8m_mix_link_fwd(int mode, const float* prev, const float* z, const float* u, float* out, float* stats, int64_t rows,
                                 int64_t Wprev, int64_t C, float scale, float eps, yt8m_stream_t stream) {
  YT8M_REQUIRE(mode >= 0 && mode <= 3, YT8M_E_BADARG, "mix_link: mode is a sum of YT8M_MIX_LINK_PLAIN and YT8M_MIX_LINK_NONE");
  YT8M_REQUIRE(rows > 0 && (rows + 3) / 4 <= 0x7fffffffLL, YT8M_E_SHAPE, "mix_link: rows must be positive (at most 2^33)");
  YT8M_REQUIRE(yt8m_mix_link_supported(Wprev, C), YT8M_E_SHAPE, "mix_link: 1 <= Wprev <= 2^24 and 1 <= C <= 1024");
  YT8M_REQUIRE(prev && z && u && out && stats, YT8M_E_BADARG, "mix_link: null operand");
  YT8M_REQUIRE(eps > 0.f && scale > 0.f, YT8M_E_BADARG, "mix_link: eps and scale must be > 0");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const float reps = (float)(1.0 / sqrt((double)eps));
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (((Wprev | C) & 3) == 0 && aligned16(prev) && aligned16(z) && aligned16(u) && aligned16(out))
    hipLaunchKernelGGL(mix_link_fwd_kernel<true>, grid, block, 0, s, mode, prev, z, u, out, stats, rows, (int)Wprev, (int)C, scale, eps, reps);
  else
    hipLaunchKernelGGL(mix_link_fwd_kernel<false>, grid, block, 0, s, mode, prev, z, u, out, stats, rows, (int)Wprev, (int)C, scale, eps, reps);
  return launch_status("mix_link_fwd_kernel");
}

extern "C" int yt8m_mix_link_bwd(int mode, const float* z, const float* u, const float* stats, const float* dy, float* dprev, float* dz,
                                 int64_t rows, int64_t Wprev, int64_t C, int64_t dx_from, float scale, yt8m_stream_t stream) {
  YT8M_REQUIRE(mode >= 0 && mode <= 3, YT8M_E_BADARG, "mix_link: mode is a sum of YT8M_MIX_LINK_PLAIN and YT8M_MIX_LINK_NONE");
  YT8M_REQUIRE(rows > 0 && (rows + 3) / 4 <= 0x7fffffffLL, YT8M_E_SHAPE, "mix_link: rows must be positive (at most 2^33)");
  YT8M_REQUIRE(yt8m_mix_link_supported(Wprev, C), YT8M_E_SHAPE, "mix_link: 1 <= Wprev <= 2^24 and 1 <= C <= 1024");
  YT8M_REQUIRE(z && u && stats && dy && dz, YT8M_E_BADARG, "mix_link: null operand (only dprev may be null)");
  YT8M_REQUIRE(dx_from >= 0 && dx_from <= Wprev, YT8M_E_BADARG, "mix_link: 0 <= dx_from <= Wprev");
  YT8M_REQUIRE(scale > 0.f, YT8M_E_BADARG, "mix_link: scale must be > 0");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (((Wprev | C | dx_from) & 3) == 0 && aligned16(z) && aligned16(u) && aligned16(dy) && aligned16(dprev) && aligned16(dz))
    hipLaunchKernelGGL(mix_link_bwd_kernel<true>, grid, block, 0, s, mode, z, u, stats, dy, dprev, dz, rows, (int)Wprev, (int)C, (int)dx_from,
                       scale);
  else
    hipLaunchKernelGGL(mix_link_bwd_kernel<false>, grid, block, 0, s, mode, z, u, stats, dy, dprev, dz, rows, (int)Wprev, (int)C,
                       (int)dx_from, scale);
  return launch_status("mix_link_bwd_kernel");
}
