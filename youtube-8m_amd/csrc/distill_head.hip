// distill_head.hip -- what the MoeDistillChain* / MoeDistillSplit heads (Z/video_level_models.py:286-582) do around their MoE block, in one
// pass each way (gfx950, wave64; launch-latency-bound: the tensors are [B, 1280..2304] and [B, 4716] and live in L2):
//   distill_input fwd, per row:  s = sum_{v >= v0} t[v] (dividing modes only);  a = act(z), or act(z) / s (a true division, 0 where s == 0);
//         y = [x' | a'] written straight into the concatenated row, p' = p * rsqrt(max(sum p^2, eps)) where that part is normalised, else p;
//         rx[row], rc[row] = +-r (sign: ss > eps; 1 where the part is not normalised), sinv[row] = 1 / s (0 where s == 0; 1 without division)
//   distill_input bwd, per row:  da = R (dy - y (y.dy)) if rinv > 0 else R dy, R = |rinv| (chain_link.hip's rule, from the output), or dy where
//         the part is not normalised;  dz = da * act'(z) * sinv with act' from the INPUT z (a relu tie at 0 gets 0);  dx the same rule on
//         the x part, written only when asked for: with a null dx the x part of dout is never read
//   distill_blend fwd:  out = (v < V1 ? p1 : t) * w + t * (1 - w), each product and the sum rounded on its own as the reference's
//         final_probabilities * ensemble_w + distill_labels * (1.0 - ensemble_w);  bwd: dp1 = w * dout[:, :V1]
// i.e. yt8m_act_fwd_f32, a row sum, a divide, two yt8m_l2norm_fwd_f32 and torch.cat (and their backward passes) without the tensors in
// between.  distill_input: one wave per row, 4 rows per workgroup (as chain_link.hip); a part of up to 1024 columns stays in registers
// between its reduction and the write -- one global read per element --, wider parts are read twice; 16-byte accesses where both widths
// % 4 == 0 and every operand is 16-byte aligned, single elements otherwise.  t is read with its own row pitch from column v0: the
// elements before the first 16-byte boundary singly, then 16 bytes at a time, then the tail.  Per-lane sums in pass order, then the
// wave butterfly: a fixed order, no atomics, no LDS; every output element is written exactly once.
#include <math.h>
#include "common.h"

namespace {

constexpr int REG_COLS = 1024;           // widest register-resident part: 16 floats per lane
constexpr int PASSES = REG_COLS / 64;    // single-element passes of a wave over such a part
constexpr int PASSES4 = REG_COLS / 256;  // 16-byte passes

constexpr int M_NORM_X = YT8M_DISTILL_NORM_X, M_RELU = YT8M_DISTILL_RELU, M_DIV = YT8M_DISTILL_DIV, M_NORM_C = YT8M_DISTILL_NORM_C;

// the class part's element from its pre-activation: relu or nothing, then the true division by the row sum of t (0 for a zero sum)
struct ClassFn {
  bool relu, div;
  float s;
  __device__ __forceinline__ float operator()(float z) const {
    const float a = relu ? fmaxf(z, 0.f) : z;
    return div ? (s != 0.f ? a / s : 0.f) : a;
  }
};
struct Identity {
  __device__ __forceinline__ float operator()(float v) const { return v; }
};

// sum of p[0 .. n): lane-strided partial sums in pass order, then the butterfly
__device__ __forceinline__ float row_sum(const float* __restrict__ p, int64_t n, int lane) {
  float s = 0.f;
  int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);       // 0..3 elements before a 16-byte boundary
  if (head > n) head = n;
  if (lane < head) s += p[lane];
  const float* q = p + head;
  const int64_t m = n - head, n4 = m >> 2;
  for (int64_t c4 = lane; c4 < n4; c4 += 64) {
    const float4 v = reinterpret_cast<const float4*>(q)[c4];
    s += (v.x + v.y) + (v.z + v.w);
  }
  const int64_t c = 4 * n4 + lane;                                        // fewer than 4 elements are left
  if (c < m) s += q[c];
  return wave_sum(s);
}

// One part of a row: dst[c] = f(src[c]) * r.  Returns the signed reciprocal norm (1 where the part is not normalised).
template <bool VEC, class F>
__device__ __forceinline__ float part_fwd(const float* __restrict__ src, float* __restrict__ dst, int cols, bool normalize, float eps,
                                          float reps, int lane, F f) {
  const int n4 = cols >> 2;
  if (!normalize) {
    if (VEC) {
      for (int c4 = lane; c4 < n4; c4 += 64) {
        const float4 q = reinterpret_cast<const float4*>(src)[c4];
        reinterpret_cast<float4*>(dst)[c4] = make_float4(f(q.x), f(q.y), f(q.z), f(q.w));
      }
    } else {
      for (int c = lane; c < cols; c += 64) dst[c] = f(src[c]);
    }
    return 1.f;
  }
  float ss = 0.f;
  if (cols <= REG_COLS) {
    float a[PASSES];
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c4 < n4) {
          const float4 q = reinterpret_cast<const float4*>(src)[c4];
          v[0] = f(q.x); v[1] = f(q.y); v[2] = f(q.z); v[3] = f(q.w);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[4 * p + k] = v[k];
        ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        const float v = c < cols ? f(src[c]) : 0.f;
        a[p] = v;
        ss += v * v;
      }
    }
    ss = wave_sum(ss);
    const float r = link_r(ss, eps, reps);
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        if (c4 < n4)
          reinterpret_cast<float4*>(dst)[c4] = make_float4(a[4 * p] * r, a[4 * p + 1] * r, a[4 * p + 2] * r, a[4 * p + 3] * r);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < cols) dst[c] = a[p] * r;
      }
    }
    return ss > eps ? r : -r;
  }
  // wide parts: the source is read twice
  if (VEC) {
    for (int c4 = lane; c4 < n4; c4 += 64) {
      const float4 q = reinterpret_cast<const float4*>(src)[c4];
      const float v0 = f(q.x), v1 = f(q.y), v2 = f(q.z), v3 = f(q.w);
      ss += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
    }
  } else {
    for (int c = lane; c < cols; c += 64) {
      const float v = f(src[c]);
      ss += v * v;
    }
  }
  ss = wave_sum(ss);
  const float r = link_r(ss, eps, reps);
  if (VEC) {
    for (int c4 = lane; c4 < n4; c4 += 64) {
      const float4 q = reinterpret_cast<const float4*>(src)[c4];
      reinterpret_cast<float4*>(dst)[c4] = make_float4(f(q.x) * r, f(q.y) * r, f(q.z) * r, f(q.w) * r);
    }
  } else {
    for (int c = lane; c < cols; c += 64) dst[c] = f(src[c]) * r;
  }
  return ss > eps ? r : -r;
}

// VEC: D % 4 == 0, C % 4 == 0 and x, z, y 16-byte aligned (checked by the caller).  reps = 1 / sqrt(eps), rounded once on the host.
template <bool VEC>
__global__ __launch_bounds__(256) void distill_input_fwd_kernel(int mode, const float* __restrict__ x, const float* __restrict__ z,
                                                                const float* __restrict__ t, int64_t ldt, int64_t v0, int64_t V,
                                                                float* __restrict__ y, float* __restrict__ rx, float* __restrict__ rc,
                                                                float* __restrict__ sinv, int64_t rows, int D, int C, float eps,
                                                                float reps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                              // wave-uniform
  const bool div = (mode & M_DIV) != 0;
  float* yr = y + row * ((int64_t)D + C);
  const float s = div ? row_sum(t + row * ldt + v0, V - v0, lane) : 1.f;
  const float r_x = part_fwd<VEC>(x + row * D, yr, D, (mode & M_NORM_X) != 0, eps, reps, lane, Identity());
  const float r_c = part_fwd<VEC>(z + row * C, yr + D, C, (mode & M_NORM_C) != 0, eps, reps, lane, ClassFn{(mode & M_RELU) != 0, div, s});
  if (lane == 0) {
    rx[row] = r_x;
    rc[row] = r_c;
    sinv[row] = div ? (s != 0.f ? 1.f / s : 0.f) : 1.f;
  }
}

// One part of a row backwards: dst[c] = da[c] * m[c], da from y and dy by the rule above, m = scale * (relu ? z > 0 : 1) (zsrc null: scale).
template <bool VEC>
__device__ __forceinline__ void part_bwd(const float* __restrict__ yr, const float* __restrict__ gr, const float* __restrict__ zsrc,
                                         float* __restrict__ dst, int cols, bool normalize, float ri, bool relu, float scale, int lane) {
  const int n4 = cols >> 2;
  const bool mask = relu && zsrc;
  if (!normalize) {
    if (VEC) {
      for (int c4 = lane; c4 < n4; c4 += 64) {
        const float4 g = reinterpret_cast<const float4*>(gr)[c4];
        float4 q = make_float4(1.f, 1.f, 1.f, 1.f);
        if (mask) q = reinterpret_cast<const float4*>(zsrc)[c4];
        reinterpret_cast<float4*>(dst)[c4] = make_float4(g.x * (q.x > 0.f ? scale : 0.f), g.y * (q.y > 0.f ? scale : 0.f),
                                                         g.z * (q.z > 0.f ? scale : 0.f), g.w * (q.w > 0.f ? scale : 0.f));
      }
    } else {
      for (int c = lane; c < cols; c += 64) dst[c] = gr[c] * ((mask ? zsrc[c] : 1.f) > 0.f ? scale : 0.f);
    }
    return;
  }
  const float R = fabsf(ri);
  const bool unit = ri > 0.f;                                           // the part was divided by its own norm (ss > eps)
  float yg = 0.f;
  if (cols <= REG_COLS) {
    float yv[PASSES], gv[PASSES], mv[PASSES];                           // y, dy, scale * act'(z)
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a, q = make_float4(1.f, 1.f, 1.f, 1.f);
        if (c4 < n4) {
          a = reinterpret_cast<const float4*>(yr)[c4];
          g = reinterpret_cast<const float4*>(gr)[c4];
          if (mask) q = reinterpret_cast<const float4*>(zsrc)[c4];
        }
        yv[4 * p] = a.x; yv[4 * p + 1] = a.y; yv[4 * p + 2] = a.z; yv[4 * p + 3] = a.w;
        gv[4 * p] = g.x; gv[4 * p + 1] = g.y; gv[4 * p + 2] = g.z; gv[4 * p + 3] = g.w;
        mv[4 * p] = q.x > 0.f ? scale : 0.f; mv[4 * p + 1] = q.y > 0.f ? scale : 0.f;
        mv[4 * p + 2] = q.z > 0.f ? scale : 0.f; mv[4 * p + 3] = q.w > 0.f ? scale : 0.f;
        yg += (a.x * g.x + a.y * g.y) + (a.z * g.z + a.w * g.w);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        const bool in = c < cols;
        yv[p] = in ? yr[c] : 0.f;
        gv[p] = in ? gr[c] : 0.f;
        mv[p] = ((in && mask) ? zsrc[c] : 1.f) > 0.f ? scale : 0.f;
        yg += yv[p] * gv[p];
      }
    }
    const float k = wave_sum(yg);
    float d[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) d[p] = (unit ? R * (gv[p] - yv[p] * k) : R * gv[p]) * mv[p];
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        if (c4 < n4) reinterpret_cast<float4*>(dst)[c4] = make_float4(d[4 * p], d[4 * p + 1], d[4 * p + 2], d[4 * p + 3]);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < cols) dst[c] = d[p];
      }
    }
    return;
  }
  // wide parts: y and dy are read twice
  for (int c = lane; c < cols; c += 64) yg += yr[c] * gr[c];
  const float k = wave_sum(yg);
  for (int c = lane; c < cols; c += 64)
    dst[c] = (unit ? R * (gr[c] - yr[c] * k) : R * gr[c]) * ((mask ? zsrc[c] : 1.f) > 0.f ? scale : 0.f);
}

// VEC: D % 4 == 0, C % 4 == 0 and z, y, dy, dz and a non-null dx 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void distill_input_bwd_kernel(int mode, const float* __restrict__ z, const float* __restrict__ y,
                                                                const float* __restrict__ rx, const float* __restrict__ rc,
                                                                const float* __restrict__ sinv, const float* __restrict__ dy,
                                                                float* __restrict__ dx, float* __restrict__ dz, int64_t rows, int D,
                                                                int C) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t w = (int64_t)D + C;
  const float* yr = y + row * w;
  const float* gr = dy + row * w;
  if (dx) part_bwd<VEC>(yr, gr, nullptr, dx + row * D, D, (mode & M_NORM_X) != 0, rx[row], false, 1.f, lane);
  part_bwd<VEC>(yr + D, gr + D, z + row * C, dz + row * C, C, (mode & M_NORM_C) != 0, rc[row], (mode & M_RELU) != 0, sinv[row], lane);
}

// VW consecutive columns per thread; VW = 4: V, V1 and ldt % 4 == 0 and every operand 16-byte aligned, so that no access straddles V1.
template <int VW>
__global__ __launch_bounds__(256) void distill_blend_fwd_kernel(const float* __restrict__ p1, const float* __restrict__ t, int64_t ldt,
                                                                float* __restrict__ out, int64_t rows, int64_t V, int64_t V1, float w,
                                                                float omw) {
  const int64_t per_row = (V + VW - 1) / VW;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * per_row) return;
  const int64_t row = i / per_row, v = (i - row * per_row) * VW;
  float tv[VW], av[VW], o[VW];
  ldv<VW>(t + row * ldt + v, tv);
#pragma unroll
  for (int k = 0; k < VW; ++k) av[k] = 0.f;
  if (v < V1) ldv<VW>(p1 + row * V1 + v, av);
#pragma unroll
  for (int k = 0; k < VW; ++k) o[k] = __fadd_rn(__fmul_rn(v < V1 ? av[k] : tv[k], w), __fmul_rn(tv[k], omw));
  stv<VW>(out + row * V + v, o);
}

template <int VW>
__global__ __launch_bounds__(256) void distill_blend_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dp1, int64_t rows,
                                                                int64_t V, int64_t V1, float w) {
  const int64_t per_row = (V1 + VW - 1) / VW;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * per_row) return;
  const int64_t row = i / per_row, v = (i - row * per_row) * VW;
  float g[VW];
  ldv<VW>(dout + row * V + v, g);
#pragma unroll
  for (int k = 0; k < VW; ++k) g[k] *= w;
  stv<VW>(dp1 + row * V1 + v, g);
}

constexpr int64_t MAX_COLS = (int64_t)1 << 24, MAX_V = 0x7fffffffLL, MAX_ELEMS = (int64_t)1 << 38;

inline bool blend_shape_ok(int64_t rows, int64_t V, int64_t V1) {
  return rows >= 1 && V >= 1 && V <= MAX_V && V1 >= 1 && V1 <= V && rows <= MAX_ELEMS / V;
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_distill_input_supported(int64_t D, int64_t C, int64_t V) {
  return D >= 1 && D <= MAX_COLS && C >= 1 && C <= MAX_COLS && V >= 1 && V <= MAX_V;
}

extern "C" int yt8m_distill_input_fwd(int mode, const float* x, const float* z, const float* t, int64_t ldt, int64_t v0, int64_t V,
                                      float* y, float* rx, float* rc, float* sinv, int64_t rows, int64_t D, int64_t C, float eps,
                                      yt8m_stream_t stream) {
  YT8M_REQUIRE(mode >= 0 && mode <= 15, YT8M_E_BADARG, "distill_input: mode is a sum of the four YT8M_DISTILL_* bits");
  YT8M_REQUIRE(yt8m_distill_input_supported(D, C, V), YT8M_E_SHAPE, "distill_input: 1 <= D, C <= 2^24 and 1 <= V < 2^31");
  YT8M_REQUIRE(rows > 0 && (rows + 3) / 4 <= 0x7fffffffLL, YT8M_E_SHAPE, "distill_input: rows must be positive (at most 2^33)");
  YT8M_REQUIRE(x && z && y && rx && rc && sinv, YT8M_E_BADARG, "distill_input: null operand");
  YT8M_REQUIRE(eps > 0.f, YT8M_E_BADARG, "distill_input: eps must be > 0");
  if (mode & M_DIV) {
    YT8M_REQUIRE(t, YT8M_E_BADARG, "distill_input: the dividing modes read t");
    YT8M_REQUIRE(v0 >= 0 && v0 < V && ldt >= V, YT8M_E_BADARG, "distill_input: 0 <= v0 < V <= ldt");
  }
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const float reps = (float)(1.0 / sqrt((double)eps));
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (((D | C) & 3) == 0 && aligned16(x) && aligned16(z) && aligned16(y))
    hipLaunchKernelGGL(distill_input_fwd_kernel<true>, grid, block, 0, s, mode, x, z, t, ldt, v0, V, y, rx, rc, sinv, rows, (int)D, (int)C,
                       eps, reps);
  else
    hipLaunchKernelGGL(distill_input_fwd_kernel<false>, grid, block, 0, s, mode, x, z, t, ldt, v0, V, y, rx, rc, sinv, rows, (int)D, (int)C,
                       eps, reps);
  return launch_status("distill_input_fwd_kernel");
}

extern "C" int yt8m_distill_input_bwd(int mode, const float* z, const float* y, const float* rx, const float* rc, const float* sinv,
                                      const float* dy, float* dx, float* dz, int64_t rows, int64_t D, int64_t C, yt8m_stream_t stream) {
  YT8M_REQUIRE(mode >= 0 && mode <= 15, YT8M_E_BADARG, "distill_input: mode is a sum of the four YT8M_DISTILL_* bits");
  YT8M_REQUIRE(yt8m_distill_input_supported(D, C, 1), YT8M_E_SHAPE, "distill_input: 1 <= D, C <= 2^24");
  YT8M_REQUIRE(rows > 0 && (rows + 3) / 4 <= 0x7fffffffLL, YT8M_E_SHAPE, "distill_input: rows must be positive (at most 2^33)");
  YT8M_REQUIRE(z && y && rx && rc && sinv && dy && dz, YT8M_E_BADARG, "distill_input: null operand (only dx may be null)");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (((D | C) & 3) == 0 && aligned16(z) && aligned16(y) && aligned16(dy) && aligned16(dx) && aligned16(dz))
    hipLaunchKernelGGL(distill_input_bwd_kernel<true>, grid, block, 0, s, mode, z, y, rx, rc, sinv, dy, dx, dz, rows, (int)D, (int)C);
  else
    hipLaunchKernelGGL(distill_input_bwd_kernel<false>, grid, block, 0, s, mode, z, y, rx, rc, sinv, dy, dx, dz, rows, (int)D, (int)C);
  return launch_status("distill_input_bwd_kernel");
}

extern "C" int yt8m_distill_blend_supported(int64_t rows, int64_t V, int64_t V1) { return blend_shape_ok(rows, V, V1); }

extern "C" int yt8m_distill_blend_fwd(const float* p1, const float* t, int64_t ldt, float* out, int64_t rows, int64_t V, int64_t V1,
                                      float w, yt8m_stream_t stream) {
  YT8M_REQUIRE(blend_shape_ok(rows, V, V1), YT8M_E_SHAPE, "distill_blend: rows >= 1, 1 <= V1 <= V < 2^31, rows * V <= 2^38");
  YT8M_REQUIRE(p1 && t && out, YT8M_E_BADARG, "distill_blend: null operand");
  YT8M_REQUIRE(ldt >= V, YT8M_E_BADARG, "distill_blend: t's row pitch must be at least V");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const float omw = 1.0f - w;                                            // formed in fp32
  const dim3 block(256);
  if (((V | V1 | ldt) & 3) == 0 && aligned16(p1) && aligned16(t) && aligned16(out))
    hipLaunchKernelGGL(distill_blend_fwd_kernel<4>, dim3((unsigned)cdiv(rows * (V / 4), 256)), block, 0, s, p1, t, ldt, out, rows, V, V1, w,
                       omw);
  else
    hipLaunchKernelGGL(distill_blend_fwd_kernel<1>, dim3((unsigned)cdiv(rows * V, 256)), block, 0, s, p1, t, ldt, out, rows, V, V1, w, omw);
  return launch_status("distill_blend_fwd_kernel");
}

extern "C" int yt8m_distill_blend_bwd(const float* dout, float* dp1, int64_t rows, int64_t V, int64_t V1, float w, yt8m_stream_t stream) {
  YT8M_REQUIRE(blend_shape_ok(rows, V, V1), YT8M_E_SHAPE, "distill_blend: rows >= 1, 1 <= V1 <= V < 2^31, rows * V <= 2^38");
  YT8M_REQUIRE(dout && dp1, YT8M_E_BADARG, "distill_blend: null operand");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 block(256);
  if (((V | V1) & 3) == 0 && aligned16(dout) && aligned16(dp1))
    hipLaunchKernelGGL(distill_blend_bwd_kernel<4>, dim3((unsigned)cdiv(rows * (V1 / 4), 256)), block, 0, s, dout, dp1, rows, V, V1, w);
  else
    hipLaunchKernelGGL(distill_blend_bwd_kernel<1>, dim3((unsigned)cdiv(rows * V1, 256)), block, 0, s, dout, dp1, rows, V, V1, w);
  return launch_status("distill_blend_bwd_kernel");
}
